"""The Kalman bank's spread record (``APE_FLAG_SPREAD`` on ``ape_kalman_bank_frame`` / ``_frame_host`` / ``ape_kalman_replay*``,
``KalmanStreamBank.frame(spread=)``, ``WatchPhonePocketKalman.spread``) on the GPU.

Reference of every record: ``estimate/_post.spread_rows(est, msg[:25], LAYOUT)`` (plain numpy, two-pass covariance) of the frame's own
stacked est rows.  The rows are the stream's smoothing stack right after the frame -- ``export_state``, the stack part cut to its row
counts, in time order -- through ``ape_fk`` (de-normalising, float64) on a pocket-layout handle made only for that, with the bank's
statistics and body: the device functions the tail kernel runs.  Their ``[:, 0:6]`` are asserted EQUAL to the packed tail of the same
float64 frame, bit for bit.

Tolerances are the derived ones of DESIGN.md 4.28 (``check_record`` / ``bound`` of tests/test_spread_gpu.py): means, covariances and
sin^2(angle / 2) at 16 N 2^-53 max(1, max |est[:, :6]|^2) absolute; the angle at 1e-6 relative where sin^2(angle / 2) > 1e-6."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from oracle import kalman_oracle as ko
from tests.test_kalman import make_model, pack_noise
from tests.test_kalman_bank_gpu import _estimator, make_bank, make_rows, pocket_stats
from tests.test_spread_gpu import bound, check_record

pytestmark = pytest.mark.gpu

SW = 21
LAYOUT = orc.LAYOUT_ORI_CAL_LARM_UARM_HIPS


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


class FkHandle:
    """a pocket-layout ape_model handle made only for ape_fk, carrying the bank's statistics"""

    def __init__(self, stats):
        from wear_mocap_ape_amd import _hip
        from wear_mocap_ape_amd.estimate import _post
        self.ctx = _post._PostContext(LAYOUT, 0)
        self.denorm = stats is not None
        if stats is not None:
            a = [np.zeros(1), np.ones(1), np.ascontiguousarray(stats["yy_m"], dtype=np.float64), np.ascontiguousarray(stats["yy_s"], dtype=np.float64)]
            _hip.check(_hip.lib().ape_model_set_norm_stats(self.ctx.handle, *[_hip.dptr(v, C.c_double) for v in a]), "ape_model_set_norm_stats")

    def est(self, targets, body):
        from wear_mocap_ape_amd.estimate import _post
        return _post.fk_rows(self.ctx.handle, LAYOUT, 0, targets, body, denormalize=self.denorm)


def stack_rows(bank, streams):
    """the stacked (normalised) target rows [K][N, 14] of the listed streams right after a frame: export -> the stack part cut to its
    row counts, in time order (oldest entry first)"""
    from wear_mocap_ape_amd import stream_state as ss
    desc = bank.state_desc()
    state, age = bank.export_state(streams)
    state = state.cpu().numpy()
    out = []
    for j in range(len(streams)):
        assert age[j] > 0
        _, _, stack, counts, _ = ss.kalman_unpack(state[j], desc)
        out.append(np.concatenate([stack[k, :counts[k]] for k in range(stack.shape[0])]))
    return out


def check_rows(fk, bank, streams, bodies, rows64, n_rows, what):
    """every listed entry's record (the last 21 columns of its flagged float64 packed row) against spread_rows of its own stacked rows;
    -> (largest deviation in units of the bound, the reference records)"""
    from wear_mocap_ape_amd.estimate import _post
    worst, refs = 0.0, []
    for j, targets in enumerate(stack_rows(bank, streams)):
        N = int(n_rows[j])
        assert targets.shape[0] == N, (what, j, targets.shape, N)
        est = fk.est(targets, bodies[j])
        row = rows64[j]
        tail = row[25:25 + 6 * N].reshape(N, 6)
        d = float(np.nanmax(np.abs(est[:, :6] - tail), initial=0.0))
        print(f"{what} entry {j}: N {N} est vs packed tail {d:.1e}", end="")
        assert np.array_equal(est[:, :6], tail, equal_nan=True), (what, j, d)       # the rows of this very frame, bit for bit
        assert not row[25 + 6 * N:-SW].any()                                           # the zeros stop in front of the record
        ref = _post.spread_rows(est, row[:25], LAYOUT)
        u = check_record(row[-SW:], ref, est, N, (what, j))
        print(f" record {u:.3f} of the bound {bound(est, N):.2e}")
        worst = max(worst, u)
        refs.append(ref)
    return worst, refs


def injected(rng, W, K, E):
    nz, init = ko.draw_noise(rng, W, K * E), rng.standard_normal((K, E, 14)).astype(np.float32)
    return torch.from_numpy(pack_noise(nz)), torch.from_numpy(init)


def host(*ts):
    return tuple(t.cpu().numpy().copy() for t in ts)


# ---------------- 1: the ragged stack, two trips of the row loop ---------------------------------------------------------------------------
def test_one_stream_ragged_stack_and_second_trip(norm_stats):
    """E = 48, W = 2, smooth = 6, 3 + 6 frames: N = 6 on the three init frames (one row per entry: the record is the smoothing lag of the
    sensor means), then 53, 100, 147, 194, 241 and 288 = 256 + 32 (a second, partial trip of the KB_BLOCK row loop).  Every frame's 21
    values; message, tail, zeros, n_rows and targets bit-equal to a twin bank fed the same injected frames unflagged"""
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    E, W, smooth = 48, 2, 6
    stats = pocket_stats(norm_stats)
    m, _ = make_model(E, W, 31)
    bank, twin = make_bank(m, 1, smooth, stats), make_bank(m, 1, smooth, stats)
    fk = FkHandle(stats)
    rng = np.random.default_rng(31)
    rows = make_rows(rng, 9)
    counts, worst = [], 0.0
    for f in range(9):
        nz, ini = injected(rng, W, 1, E)
        out, n, y = host(*bank.step_rows(rows[f:f + 1], datagrams=True, noise=nz, init_noise=ini, return_targets=True, spread=True))
        po, pn, py = host(*twin.step_rows(rows[f:f + 1], datagrams=True, noise=nz, init_noise=ini, return_targets=True))
        assert out.shape == (1, 25 + 6 * smooth * E + SW) and po.shape == (1, 25 + 6 * smooth * E)
        head, rec = KalmanStreamBank.split_spread(out)
        assert np.array_equal(head, po) and np.array_equal(n, pn)
        k = 1 if f <= W else E
        assert np.array_equal(y[:, :k], py[:, :k])
        u, _ = check_rows(fk, bank, [0], [orc.DEFAULT_BODY], out, n, f"frame {f}")
        worst = max(worst, u)
        counts.append(int(n[0]))
        assert np.isfinite(rec).all()
        if f > W:
            assert rec[0, 3] > 0 and (rec[0, 18:21] > 1e-6).all()              # the ensemble does spread, the hips included
        # the unpacked flagged row of a third bank would draw other samples; the same bank's unflagged buffers kept their shapes
    assert counts == [6, 6, 6, 53, 100, 147, 194, 241, 288]
    assert tuple(twin._bufs[("step", "out", True)].shape) == (1, 25 + 6 * smooth * E)
    print(f"worst {worst:.3f} of the bound")
    m.check()


# ---------------- 2: N = 1 -------------------------------------------------------------------------------------------------------------------
def test_single_row_record_is_origins_and_exact_zeros(norm_stats):
    """E = 2, W = 2, smooth = 1: N = 1 on the init frames -- the row's two origins and exact zeros, by rule -- then N = 2; message rows
    [S, 25 + 21] without PACKED_MSG"""
    E, W = 2, 2
    stats = pocket_stats(norm_stats)
    m, _ = make_model(E, W, 32)
    bank, packed = make_bank(m, 1, 1, stats, seed=5), make_bank(m, 1, 1, stats, seed=5)
    fk = FkHandle(stats)
    rows = make_rows(np.random.default_rng(32), 5)
    zeros = [3, 4, 5, 6, 7, 8, 12, 13, 14, 15, 16, 17, 18, 19, 20]
    for f in range(5):
        out = bank.step_rows(rows[f:f + 1], spread=True).cpu().numpy().copy()
        pk, n = host(*packed.step_rows(rows[f:f + 1], datagrams=True, spread=True))
        assert out.shape == (1, 25 + SW) and pk.shape == (1, 25 + 6 * E + SW)
        assert np.array_equal(out[:, :25], pk[:, :25]) and np.array_equal(out[:, -SW:], pk[:, -SW:])
        assert int(n[0]) == (1 if f <= W else 2)
        rec = out[0, -SW:]
        if f <= W:
            assert np.array_equal(rec[[0, 1, 2, 9, 10, 11]], pk[0, 25:31]) and not rec[zeros].any()
            assert np.array_equal(rec[[0, 1, 2]], out[0, 4:7]) and np.array_equal(rec[[9, 10, 11]], out[0, 11:14])     # N == 1: the message copies the row
        check_rows(fk, packed, [0], [orc.DEFAULT_BODY], pk, n, f"E 2 frame {f}")
    m.check()


# ---------------- 3: subset frames, resets, per-stream bodies ---------------------------------------------------------------------------------
def test_subset_frames_resets_and_body_table(norm_stats):
    """five streams, E = 16, W = 4, smooth = 3, per-stream bodies: lockstep and subset frames in scrambled list order around a
    reset(streams=[1, 3]); the record follows the list position like the message row, is computed with the STREAM's body (the body-table
    instantiations), and streams that are not listed keep their state (export before == export after)"""
    S, E, W, smooth = 5, 16, 4, 3
    stats = pocket_stats(norm_stats)
    m, _ = make_model(E, W, 33)
    bank, twin = make_bank(m, S, smooth, stats, seed=3), make_bank(m, S, smooth, stats, seed=3)
    rng = np.random.default_rng(33)
    bodies = np.tile(np.asarray(orc.DEFAULT_BODY, dtype=np.float64).reshape(1, 9), (S, 1)) * (1.0 + 0.1 * rng.random((S, 9)))
    bank.set_bodies(bodies)
    twin.set_bodies(bodies)
    fk = FkHandle(stats)
    everyone = list(range(S))
    plan = [None, None, [3, 0], [4, 1, 2], [2, 4, 0, 3], "reset", [3, 1], None, None, [0, 4, 2], None, [1, 0]]
    seen, worst = set(), 0.0
    for step, item in enumerate(plan):
        if item == "reset":
            bank.reset(streams=[1, 3])
            twin.reset(streams=[1, 3])
            continue
        order = everyone if item is None else item
        rows = make_rows(rng, len(order))
        # (records compared as 32-bit words: the halves of the window's float64 values are no float32 numbers)
        before = None if step < 2 else bank.export_state(everyone)[0].cpu().numpy().view(np.uint32).copy()
        if item is None:
            out, n = host(*bank.step_rows(rows, datagrams=True, spread=True))
            po, pn = host(*twin.step_rows(rows, datagrams=True))
        else:
            out, n = host(*bank.frame(rows, order, datagrams=True, spread=True))
            po, pn = host(*twin.frame(rows, order, datagrams=True))
        assert np.array_equal(out[:, :-SW], po) and np.array_equal(n, pn)
        if before is not None:
            after = bank.export_state(everyone)[0].cpu().numpy().view(np.uint32)
            idle = [s for s in everyone if s not in order]
            assert np.array_equal(before[idle], after[idle]), (step, idle)
        u, _ = check_rows(fk, bank, order, bodies[order], out, n, f"step {step} {order}")
        worst = max(worst, u)
        seen.update(int(v) for v in n)
    assert seen == {3, 2 + E, 1 + 2 * E, 3 * E}                       # init frames, the ragged transition, the full stack
    print(f"worst {worst:.3f} of the bound")
    m.check()


# ---------------- 4: float32 --------------------------------------------------------------------------------------------------------------------
def test_float32_record_is_the_float64_record_rounded_once(norm_stats):
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    S, E, W, smooth = 2, 16, 4, 3
    stats = pocket_stats(norm_stats)
    m, _ = make_model(E, W, 34)
    f64 = make_bank(m, S, smooth, stats, seed=9)
    f32 = KalmanStreamBank(m, S, smooth=smooth, normalize=False, seed=9, dtype=torch.float32)
    f32.set_norm_stats(stats)
    f32.set_body(orc.DEFAULT_BODY)
    rows = make_rows(np.random.default_rng(34), 8 * S).reshape(8, S, 55)
    for f in range(8):
        a, na = host(*f32.step_rows(rows[f], datagrams=True, spread=True))
        b, nb = host(*f64.step_rows(rows[f], datagrams=True, spread=True))
        assert a.dtype == np.float32 and b.dtype == np.float64 and np.array_equal(na, nb)
        assert np.array_equal(a, b.astype(np.float32))                  # message, tail, zeros and record
        assert b[:, -SW:].any(axis=1).all()
    assert nb.tolist() == [3 * E] * S
    m.check()


# ---------------- 5: the host entry -----------------------------------------------------------------------------------------------------------
def _frame_host(bank, rows, flags, width, big_endian=False):
    from wear_mocap_ape_amd import _hip
    S = bank.n_streams
    out, n = np.full((S, width), 7.0), np.zeros(S, dtype=np.int32)
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if big_endian:
        rows = rows.byteswap()
    kind = _hip.PARSE_WATCH_PHONE_POCKET | (_hip.PARSE_BIG_ENDIAN if big_endian else 0)
    _hip.check(_hip.lib().ape_kalman_bank_frame_host(bank._handle, kind, C.c_void_p(rows.ctypes.data), flags, C.c_void_p(out.ctypes.data),
                                                     _hip.F64, C.c_void_p(n.ctypes.data), None), "frame_host")
    return out, n


def test_host_entry_rows_equal_the_device_entry(norm_stats):
    """ape_kalman_bank_frame_host with the flag: packed and unpacked rows equal the device entry's, a big-endian row included; one bank
    alternates flagged and unflagged host frames (its pinned buffer serves every width)"""
    from wear_mocap_ape_amd import _hip
    S, E, W, smooth = 3, 16, 4, 2
    stats = pocket_stats(norm_stats)
    m, _ = make_model(E, W, 35)
    hp, hu, hb, dev, mix, ref = (make_bank(m, S, smooth, stats, seed=99) for _ in range(6))
    wp = 25 + 6 * smooth * E
    rng = np.random.default_rng(35)
    for f in range(W + 4):
        rows = make_rows(rng, S)
        want, wn = host(*dev.step_rows(torch.from_numpy(rows).cuda(), datagrams=True, spread=True))
        op, n1 = _frame_host(hp, rows, _hip.FLAG_PACKED_MSG | _hip.FLAG_SPREAD, wp + SW)
        ou, n2 = _frame_host(hu, rows, _hip.FLAG_SPREAD, 25 + SW)
        ob, n3 = _frame_host(hb, rows, _hip.FLAG_PACKED_MSG | _hip.FLAG_SPREAD, wp + SW, big_endian=True)
        assert np.array_equal(op, want) and np.array_equal(ob, want)
        assert np.array_equal(ou[:, :25], want[:, :25]) and np.array_equal(ou[:, 25:], want[:, -SW:])
        assert np.array_equal(n1, wn) and np.array_equal(n2, wn) and np.array_equal(n3, wn)
        flags, width = [(_hip.FLAG_PACKED_MSG | _hip.FLAG_SPREAD, wp + SW), (_hip.FLAG_PACKED_MSG, wp), (_hip.FLAG_SPREAD, 25 + SW), (0, 25)][f % 4]
        om, _ = _frame_host(mix, rows, flags, width)
        cols = list(range(width - (SW if flags & _hip.FLAG_SPREAD else 0)))
        assert np.array_equal(om[:, cols], want[:, cols])
        if flags & _hip.FLAG_SPREAD:
            assert np.array_equal(om[:, -SW:], want[:, -SW:])
        assert np.array_equal(ref.step_rows(rows, datagrams=True)[0].cpu().numpy(), want[:, :-SW])
    assert wn.tolist() == [smooth * E] * S
    m.check()


# ---------------- 6: replay -------------------------------------------------------------------------------------------------------------------
def test_replay_records_equal_the_banks_and_chain(norm_stats):
    """two recordings of 9 and 5 frames, E = 16, W = 4, smooth = 3: process_recording(spread=True) == a bank stepped frame by frame;
    the first recording in two chained pieces (cut inside the ragged transition) == the one call, out and spread"""
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    E, W, smooth, seed = 16, 4, 3, 4242
    sd = ko.make_state_dict(W, 36)
    est = _estimator(sd, E, W, smooth=smooth)
    rng = np.random.default_rng(36)
    lens = [9, 5]
    starts = np.cumsum([0] + lens[:-1])
    rows = make_rows(rng, sum(lens))
    plain, pn = host(*est.process_recording(rows, starts=starts, seed=seed))
    out, n, y, rec = est.process_recording(rows, starts=starts, seed=seed, return_targets=True, spread=True)
    assert tuple(out.shape) == (14, 25 + 6 * smooth * E) and tuple(rec.shape) == (14, SW) and rec.dtype == torch.float64
    out, n, rec = host(out, n, rec)
    assert np.array_equal(out, plain) and np.array_equal(n, pn)
    bank = KalmanStreamBank(est.model, 2, smooth=smooth, normalize=True, seed=seed)
    for t in range(max(lens)):
        order = [r for r in range(2) if lens[r] > t]
        idx = [starts[r] + t for r in order]
        o, nn = host(*bank.frame(rows[idx], order, datagrams=True, spread=True))
        assert np.array_equal(o[:, :-SW], out[idx]) and np.array_equal(o[:, -SW:], rec[idx]) and np.array_equal(nn, n[idx])
    assert n[:9].tolist() == [3] * 5 + [2 + E, 1 + 2 * E, 3 * E, 3 * E] and rec[5:9, 18:21].min() > 0
    # float32 rows: the float64 ones rounded once
    o32, _, r32 = est.process_recording(rows, starts=starts, seed=seed, out_dtype=torch.float32, spread=True)
    assert r32.dtype == torch.float32 and np.array_equal(r32.cpu().numpy(), rec.astype(np.float32))
    # without add_mc_samples: [F, 25] and the same records
    lean = _estimator(sd, E, W, smooth=smooth, add_mc_samples=False)
    lo, _, lr = host(*lean.process_recording(rows, starts=starts, seed=seed, spread=True))
    assert lo.shape == (14, 25) and np.array_equal(lo, out[:, :25]) and np.array_equal(lr, rec)
    # chained pieces of the first recording
    one, n1, r1 = host(*est.process_recording(rows[:9], seed=seed, spread=True))
    state = age = None
    for a, b in ((0, 6), (6, 9)):
        o, nn, rr, state, age = est.process_recording(rows[a:b], seed=seed, spread=True, state_in=state, age_in=age, return_state=True, call_base=a)
        o, nn, rr = host(o, nn, rr)
        assert np.array_equal(o, one[a:b]) and np.array_equal(rr, r1[a:b]) and np.array_equal(nn, n1[a:b])
    est.model.check()


# ---------------- 7: the estimator's switch -----------------------------------------------------------------------------------------------
def test_estimator_switch():
    """process_row with spread on returns what it returns with it off (same seed, same rows); get_last_spread() is the record of a
    one-stream bank with that seed; reset() and switching off clear it; the staged path fills it from spread_rows"""
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    E, W, smooth = 16, 4, 3
    sd = ko.make_state_dict(W, 37)
    rows = make_rows(np.random.default_rng(37), W + 4)
    off, on = _estimator(sd, E, W, smooth=smooth), _estimator(sd, E, W, smooth=smooth)
    off.manual_seed(77)
    on.manual_seed(77)
    assert on.spread is False and on.get_last_spread() is None
    on.spread = True
    bank = KalmanStreamBank(on.model, 1, smooth=smooth, normalize=True, seed=77)
    for r in rows:
        a, b = off.process_row(r), on.process_row(r)
        assert isinstance(b, list) and a == b
        want, _ = bank.step_rows(r[None, :], datagrams=True, spread=True)
        got = on.get_last_spread()
        assert got.dtype == np.float64 and got.shape == (SW,) and np.array_equal(got, want.cpu().numpy()[0, -SW:])
        assert off.get_last_spread() is None
    assert len(b) == 25 + 6 * smooth * E and got[18:21].min() > 0
    np.testing.assert_array_equal(on.get_last_msg(), np.asarray(b[:25]))
    on.reset()
    assert on.get_last_spread() is None and on.spread is True
    assert on.process_row(rows[0]) == off_first(sd, E, W, smooth, rows[0])
    assert on.get_last_spread() is not None
    on.spread = False
    assert on.get_last_spread() is None
    assert on.process_row(rows[1]) is not None and on.get_last_spread() is None
    # add_mc_samples = False: the 25-value message, the record all the same
    lean = _estimator(sd, E, W, smooth=smooth, add_mc_samples=False)
    lean.manual_seed(77)
    lean.spread = True
    msg = lean.process_row(rows[0])
    assert isinstance(msg, np.ndarray) and msg.shape == (25,) and lean.get_last_spread().shape == (SW,)
    # the staged path: spread_rows of its own est rows
    staged = _estimator(sd, E, W, smooth=smooth)
    staged.use_device_frame = False
    staged.spread = True
    staged.process_row(rows[0])
    rec = staged.get_last_spread()
    assert getattr(staged, "_device_frame", None) is None and rec.shape == (SW,) and np.isfinite(rec).all()
    on.model.check()


def off_first(sd, E, W, smooth, row):
    fresh = _estimator(sd, E, W, smooth=smooth)
    fresh.manual_seed(77)
    return fresh.process_row(row)


# ---------------- 8: a NaN target row ---------------------------------------------------------------------------------------------------------
def test_nan_target_row_touches_exactly_its_entries(norm_stats):
    """a NaN in one lower-arm target of one stacked row, brought in through import_state of a doctored stack: the next frame's record
    is NaN exactly where spread_rows of those rows is (the hand, which hangs on the lower arm, and the lower-arm angle), finite elsewhere"""
    from wear_mocap_ape_amd import stream_state as ss
    E, W, smooth = 16, 4, 3
    stats = pocket_stats(norm_stats)
    m, _ = make_model(E, W, 38)
    bank = make_bank(m, 2, smooth, stats, seed=11)
    fk = FkHandle(stats)
    rng = np.random.default_rng(38)
    for f in range(W + 4):
        bank.step_rows(make_rows(rng, 2))
    desc = bank.state_desc()
    state, age = bank.export_state([1])
    window, history, stack, counts, _ = ss.kalman_unpack(state.cpu().numpy()[0], desc)
    assert counts.tolist() == [E] * smooth
    stack[2, 5, 1] = np.nan                                   # the newest entry: still stacked after the next frame (as entry 1)
    bank.import_state([1], ss.kalman_pack(window, history, stack, counts)[np.newaxis, :], age)
    out, n = host(*bank.step_rows(make_rows(rng, 2), datagrams=True, spread=True))
    _, refs = check_rows(fk, bank, [0, 1], [orc.DEFAULT_BODY] * 2, out, n, "nan row")
    assert np.isfinite(out[0]).all() and np.isfinite(refs[0]).all()
    rec = out[1, -SW:]
    nan = np.isnan(rec)
    assert nan[0:9].all() and nan[18] and not nan[9:18].any() and not nan[19:21].any(), rec
    m.check()
