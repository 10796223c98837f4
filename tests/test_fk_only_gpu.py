"""``WatchPhoneUarm`` on the device: ``process_row`` through a one-stream FK bank against the reference's trace,
``FkStreamBank`` lockstep and subset frames against independent estimators and the oracle, ``process_recording`` (``ape_fk_replay``)
against fresh ``process_row`` loops and a bank, big-endian rows and float32 messages."""
import ctypes as C
from array import array

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


@pytest.fixture(scope="module")
def trace():
    return np.load(GOLDEN / "fk_only_trace.npz")


def _recordings(t):
    ends = np.cumsum(t["lengths"])
    return [(int(e - n), int(e)) for n, e in zip(t["lengths"], ends)]


def _est(**kw):
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    return WatchPhoneUarm(**kw)


def _random_rows(rng, n):
    """float32 [n, 55] WATCH_PHONE_IMU messages: random sensors, unit rotation and calibration quaternions"""
    from wear_mocap_ape_amd.data_types import messaging
    slp = messaging.WATCH_PHONE_IMU_LOOKUP
    rows = rng.normal(size=(n, 55)).astype(np.float32)
    for pre in ("sw_rotvec", "sw_forward", "ph_rotvec", "ph_forward"):
        q = rng.normal(size=(n, 4))
        rows[:, [slp[f"{pre}_{c}"] for c in "wxyz"]] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    rows[:, slp["sw_pres"]] = 1000.0 + rng.normal(size=n).astype(np.float32)
    rows[:, slp["sw_init_pres"]] = 1000.5
    return rows


def _swap(rows):
    return np.ascontiguousarray(rows).byteswap()


def _oracle_msg(xx_stack, body):
    pred = np.array([np.r_[x[13:19], x[32:38]] for x in xx_stack])
    est = orc.arm_pose_from_targets(pred, body, orc.LAYOUT_ORI_CAL_LARM_UARM)
    return orc.msg_from_est(est, body, orc.LAYOUT_ORI_CAL_LARM_UARM)


# ---------------- process_row ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth", [1, 2, 5, 10])
def test_process_row_against_reference(trace, smooth):
    rows = trace["rows"]
    want = trace[f"msg_s{smooth}"]
    dev, staged = _est(smooth=smooth), _est(smooth=smooth)
    staged.use_device_frame = False
    for r, (lo, hi) in enumerate(_recordings(trace)):
        dev.reset(); staged.reset()
        for f in range(lo, hi):
            row = array("f", rows[f].tolist())
            m = dev.process_row(row)
            s = staged.process_row(row)
            assert isinstance(m, np.ndarray) and m.dtype == np.float64 and m.shape == (25,)
            np.testing.assert_array_equal(np.isnan(m), np.isnan(want[f]))
            assert np.nanmax(np.abs(m - want[f])) < 1e-5
            assert np.nanmax(np.abs(m - np.asarray(s))) < 1e-10
        last = dev.get_last_msg()
        assert np.abs(last - trace[f"last_msg_s{smooth}"][r]).max() < 1e-5
        np.testing.assert_array_equal(last, m)
    # the azimuth sweep, reference-finite rows only (the reference raises on the NaN calibration)
    dev.reset()
    for row, w in zip(trace["edge_rows"][trace["edge_ok"]], trace[f"edge_msg_s{smooth}"]):
        m = dev.process_row(array("f", row.tolist()))
        assert np.abs(m - w).max() < 1e-5
    # the NaN calibration: no exception on the device, NaN in the message
    dev.reset()
    m = dev.process_row(trace["edge_rows"][~trace["edge_ok"]][0])
    assert np.isnan(m).any()


def test_process_row_non_default_body(trace):
    class BM:
        left_lower_arm_length, left_upper_arm_length = (float(v) for v in trace["bm_lengths"])
        left_upper_arm_origin_rh = trace["bm_uarm_orig"]
    est = _est(smooth=5, bonemap=BM())
    lo, hi = _recordings(trace)[0]
    for f in range(lo, hi):
        assert np.abs(est.process_row(trace["rows"][f]) - trace["bm_msg"][f]).max() < 1e-5


# ---------------- bank: lockstep ---------------------------------------------------------------------------------------
def test_bank_lockstep_against_estimators_and_oracle():
    from wear_mocap_ape_amd.estimate.watch_phone_uarm_nn import features_from_row
    from wear_mocap_ape_amd.data_types import messaging
    from wear_mocap_ape_amd.streams import FkStreamBank
    S, T, smooth = 4096, 30, 5
    rng = np.random.default_rng(4)
    rows = _random_rows(rng, S * T).reshape(T, S, 55)
    bank = FkStreamBank(S, smooth=smooth, dtype=torch.float64)
    out = np.stack([bank.step_rows(torch.from_numpy(rows[t]).cuda()).cpu().numpy() for t in range(T)])
    assert out.shape == (T, S, 25)
    sample = rng.choice(S, size=6, replace=False)
    for s in sample:
        est = _est(smooth=smooth)
        got = np.stack([est.process_row(rows[t, s]) for t in range(T)])
        np.testing.assert_array_equal(got, out[:, s])
    slp = messaging.WATCH_PHONE_IMU_LOOKUP
    body = orc.DEFAULT_BODY
    for t in (0, 3, 12, T - 1):
        hist = range(max(0, t - smooth + 1), t + 1)
        xx = {h: [features_from_row(rows[h, s].astype(np.float64), slp) for s in range(S)] for h in hist}
        worst = 0.0
        for s in range(S):
            stack = [xx[max(0, t - smooth + 1 + i)][s] for i in range(smooth)]
            worst = max(worst, float(np.abs(_oracle_msg(stack, body) - out[t, s]).max()))
        assert worst < 1e-12, (t, worst)


# ---------------- bank: subset frames ----------------------------------------------------------------------------------
def test_bank_subset_frames_against_fresh_estimators():
    from wear_mocap_ape_amd.streams import FkStreamBank
    S, smooth = 48, 5
    rng = np.random.default_rng(11)
    bank = FkStreamBank(S, smooth=smooth, dtype=torch.float64)
    ests = [_est(smooth=smooth) for _ in range(S)]
    for step in range(60):
        if step % 7 == 3:                                   # per-stream cold starts
            rs = rng.choice(S, size=int(rng.integers(1, 6)), replace=False)
            bank.reset(streams=rs)
            for s in rs:
                ests[s].reset()
        if step % 10 == 9:                                  # a lockstep frame in between
            streams = np.arange(S)
        else:
            streams = rng.choice(S, size=int(rng.integers(0, S + 1)), replace=False)
        rows = _random_rows(rng, len(streams))
        if step % 10 == 9:
            got = bank.step_rows(rows).cpu().numpy()
        else:
            got = bank.frame(rows, streams).cpu().numpy()
        assert got.shape == (len(streams), 25)
        for j, s in enumerate(streams):
            np.testing.assert_array_equal(got[j], ests[s].process_row(rows[j]))
    # a full lockstep frame at the end: every stream's history, listed or not, is what its own estimator holds
    rows = _random_rows(rng, S)
    got = bank.step_rows(rows).cpu().numpy()
    for s in range(S):
        np.testing.assert_array_equal(got[s], ests[s].process_row(rows[s]))


def test_bank_subset_frames_back_to_back():
    """20 subset frames enqueued with no host synchronisation in between (rows already on the device): the pinned descriptor ring
    (csrc/bank_host.h) wraps more than twice, and a slot rewritten before its copy had run would hand a frame another frame's list.
    Bit-equal to the same frames with a device synchronisation after each, and to fresh estimators fed each stream's rows."""
    from wear_mocap_ape_amd.streams import FkStreamBank
    S, smooth, frames = 5, 2, 20
    rng = np.random.default_rng(21)
    lists = [rng.choice(S, size=int(rng.integers(1, S + 1)), replace=False) for _ in range(frames)]
    rows = [_random_rows(rng, len(l)) for l in lists]
    rows_dev = [torch.from_numpy(r).cuda() for r in rows]

    def run(sync):
        bank = FkStreamBank(S, smooth=smooth, dtype=torch.float64)
        torch.cuda.synchronize()
        outs = []
        for rd, l in zip(rows_dev, lists):
            outs.append(bank.frame(rd, l).clone())          # (the bank's buffer is overwritten by the next frame)
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]

    queued, synced = run(False), run(True)
    ests = [_est(smooth=smooth) for _ in range(S)]
    for f, l in enumerate(lists):
        np.testing.assert_array_equal(queued[f], synced[f], err_msg=f"frame {f}")
        for j, s in enumerate(l):
            np.testing.assert_array_equal(queued[f][j], ests[s].process_row(rows[f][j]), err_msg=f"frame {f} stream {s}")


def test_bank_unlisted_streams_untouched_and_refusals():
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import FkStreamBank
    S = 16
    rng = np.random.default_rng(5)
    a, b = FkStreamBank(S, smooth=3, dtype=torch.float64), FkStreamBank(S, smooth=3, dtype=torch.float64)
    r0 = _random_rows(rng, S)
    a.step_rows(r0); b.step_rows(r0)
    r1 = _random_rows(rng, 4)
    a.frame(r1, [3, 9, 0, 12])                              # b does not see this frame
    assert a.frame(np.zeros((0, 55), np.float32), []).shape == (0, 25)       # K = 0: no-op
    keep = [s for s in range(S) if s not in (3, 9, 0, 12)]
    r2 = _random_rows(rng, len(keep))
    np.testing.assert_array_equal(a.frame(r2, keep).cpu().numpy(), b.frame(r2, keep).cpu().numpy())
    for bad in ([1, 1], [S], [-1]):
        with pytest.raises(UserWarning):
            a.frame(_random_rows(rng, len(bad)), bad)
        with pytest.raises(UserWarning):
            a.reset(streams=bad)
    with pytest.raises(UserWarning):
        a.frame(np.zeros((2, 28), np.float32), [0, 1])       # watch-only width
    with pytest.raises(UserWarning):
        a.step_rows(np.zeros((S - 1, 55), np.float32))
    # the C ABI refuses what the binding would let through
    lib = _hip.lib()
    rows = torch.from_numpy(_random_rows(rng, 2)).cuda()
    out = torch.empty((S, 25), dtype=torch.float64, device="cuda")
    for kind, idx in ((_hip.PARSE_WATCH_PHONE_POCKET, [0, 1]), (_hip.PARSE_WATCH_ONLY, [0, 1]), (_hip.PARSE_WATCH_PHONE_UARM, [2, 2]),
                      (_hip.PARSE_WATCH_PHONE_UARM, [0, S])):
        i = np.array(idx, dtype=np.int32)
        rc = lib.ape_fk_bank_frame(a._handle, kind, C.c_void_p(rows.data_ptr()), C.c_void_p(i.ctypes.data), 2, C.c_void_p(out.data_ptr()),
                                   _hip.F64, None)
        assert rc != 0 and lib.ape_last_error()
    rc = lib.ape_fk_bank_frame(a._handle, _hip.PARSE_WATCH_PHONE_UARM, C.c_void_p(rows.data_ptr()), None, 2, C.c_void_p(out.data_ptr()),
                               _hip.F64, None)
    assert rc != 0                                          # no list: K must be S
    # and refused calls changed nothing
    r3 = _random_rows(rng, S)
    c = FkStreamBank(S, smooth=3, dtype=torch.float64)
    c.step_rows(r0); c.frame(r1, [3, 9, 0, 12]); c.frame(r2, keep)
    np.testing.assert_array_equal(a.step_rows(r3).cpu().numpy(), c.step_rows(r3).cpu().numpy())


# ---------------- replay ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth", [1, 2, 5, 10])
def test_replay_matches_process_row(trace, smooth):
    rows = trace["rows"]
    starts = [lo for lo, _ in _recordings(trace)]
    est = _est(smooth=smooth)
    want = []
    for lo, hi in _recordings(trace):
        est.reset()
        want += [est.process_row(rows[f]) for f in range(lo, hi)]
    want = np.array(want)
    got = est.process_recording(rows, starts=starts).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(est.process_recording(_swap(rows), starts=starts, big_endian=True).cpu().numpy(), want)
    f32 = est.process_recording(rows, starts=starts, out_dtype=torch.float32).cpu().numpy()
    np.testing.assert_array_equal(f32, want.astype(np.float32))
    with pytest.raises(UserWarning):
        est.process_recording(rows, starts=[0, 70])


def test_replay_million_rows_against_subset_bank():
    from wear_mocap_ape_amd.streams import FkStreamBank
    F, R, smooth = 10 ** 6, 50, 10
    rng = np.random.default_rng(8)
    cut = np.sort(rng.choice(np.arange(2, F), size=R - 2, replace=False))
    starts = np.r_[0, 1, cut].astype(np.int64)             # recording 0 is one frame long
    lengths = np.diff(np.r_[starts, F])
    rows = torch.from_numpy(_random_rows(rng, F)).cuda()
    got = _est(smooth=smooth).process_recording(rows, starts=starts)
    bank = FkStreamBank(R, smooth=smooth, dtype=torch.float64)
    want = torch.empty((F, 25), dtype=torch.float64, device="cuda")
    st = torch.from_numpy(starts).cuda()
    ln = torch.from_numpy(lengths).cuda()
    n_frames = int(lengths.max())
    for k in range(n_frames):
        live = np.nonzero(lengths > k)[0]
        li = torch.from_numpy(live).cuda()
        src = st[li] + k
        out = bank.frame(rows.index_select(0, src), live)
        want.index_copy_(0, src, out)
    assert n_frames > 15000 and int(ln.sum()) == F
    assert torch.equal(got, want)


def test_bank_big_endian_and_f32():
    from wear_mocap_ape_amd.streams import FkStreamBank
    S = 300
    rng = np.random.default_rng(9)
    b64, be, b32 = (FkStreamBank(S, smooth=4, dtype=d) for d in (torch.float64, torch.float64, torch.float32))
    for t in range(8):
        rows = _random_rows(rng, S)
        m = b64.step_rows(rows).cpu().numpy()
        np.testing.assert_array_equal(be.step_rows(_swap(rows), big_endian=True).cpu().numpy(), m)
        np.testing.assert_array_equal(b32.step_rows(rows).cpu().numpy(), m.astype(np.float32))
