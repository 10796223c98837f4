"""The Kalman estimator's device stream bank, one-call frames and replay (``ape_kalman_bank_*``, ``ape_kalman_replay``)
on the GPU, against the oracle chain ``KalmanFrameLogic`` (oracle/kalman_oracle.py) inside ``WindowOracle`` + the float64 post-filter
(oracle/ape_oracle.py).  PARITY UNPINNED: these tests prove HIP == restatement, like tests/test_kalman.py.

Tolerances, both the project's own: normalised targets within 5e-4 of the oracle over W + 4 = 14 frames of feedback (the bound of
test_estimator_frame_logic_vs_oracle: the oracle inverts in float64, the kernel in float32); messages and packed tails within 1e-12 of
the oracle's float64 post-filter applied to the product's OWN returned targets (de-normalised and stacked by WindowOracle's rules), which
keeps the float32 feedback error out of the float64 comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from oracle import kalman_oracle as ko
from tests import mc_check
from tests.conftest import GOLDEN
from tests.test_kalman import make_model, pack_noise

pytestmark = pytest.mark.gpu

TOL_Y, TOL_MSG = 5e-4, 1e-12
LAYOUT = orc.LAYOUT_ORI_CAL_LARM_UARM_HIPS


def make_rows(rng, n):
    """raw WATCH_PHONE_IMU messages: the recorded trace's rows in turn, the sensor columns jittered (quaternions as recorded)"""
    base = np.load(GOLDEN / "stream_trace_pocket.npz")["rows"].astype(np.float32)
    rows = base[rng.integers(0, len(base), n)].copy()
    cols = list(range(10, 23)) + list(range(33, 46))
    rows[:, cols] += (0.05 * rng.normal(size=(n, len(cols)))).astype(np.float32)
    return rows


def features(row):
    from wear_mocap_ape_amd.data_types import messaging
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import features_from_row
    return np.asarray(features_from_row(row, messaging.WATCH_PHONE_IMU_LOOKUP), dtype=np.float64)


def pocket_stats(norm_stats):
    return {k: norm_stats["pocket"][k] for k in ("xx_m", "xx_s", "yy_m", "yy_s")}


def slice_noise(nz, j, E):
    return {name: dict(v, sign_in=v["sign_in"][j * E:(j + 1) * E], sign_out=v["sign_out"][j * E:(j + 1) * E]) for name, v in nz.items()}


class StreamOracle:
    """one stream: the oracle chain fed its rows (targets), and the float64 post-filter fed the PRODUCT's targets (messages)"""

    def __init__(self, sd, E, W, smooth, stats):
        self.sd, self.E, self.W, self.cur = sd, E, W, {}
        self.fl = ko.KalmanFrameLogic(sd, E, W)
        self.win = orc.WindowOracle(W, smooth, stats, self._predict)
        self.post = orc.WindowOracle(W, smooth, stats, lambda hist: self.cur["y"])

    def _predict(self, hist):
        self.last_y = self.fl.step(hist, self.cur["nz"], self.cur["init"])      # [1,14] or [E,14], normalised
        return self.last_y

    def reset(self):
        self.fl = ko.KalmanFrameLogic(self.sd, self.E, self.W)
        self.win.reset()
        self.post.reset()

    def check(self, row, nz, init, y_got, n_got, packed_got, what):
        from wear_mocap_ape_amd.streams import trim_packed
        xx = features(row)
        self.cur.update(nz=nz, init=np.asarray(init, dtype=np.float32))
        want_stack = self.win.push(xx)
        y = y_got[:self.last_y.shape[0]]
        dy = float(np.abs(y - self.last_y).max())
        print(f"{what}: rows {n_got} target err {dy:.3e}", end="")
        assert dy < TOL_Y, (what, dy)
        self.cur["y"] = y
        stack = self.post.push(xx)
        assert n_got == stack.shape[0] == want_stack.shape[0], (what, n_got, stack.shape, want_stack.shape)
        est = orc.arm_pose_from_targets(stack, orc.DEFAULT_BODY, LAYOUT, route="closed")
        full = np.asarray(orc.msg_with_mc_samples(orc.msg_from_est(est, orc.DEFAULT_BODY, LAYOUT), est, True), dtype=np.float64)
        got = trim_packed(packed_got, n_got)
        assert got.shape == full.shape, (what, got.shape, full.shape)
        dm = float(np.abs(got - full).max())
        print(f" message err {dm:.3e}")
        assert dm < TOL_MSG, (what, dm)
        # behind the stacked rows: zeros (one row: its hand and elbow still sit at 25:31, the reference sends 25 values)
        assert np.all(packed_got[25 + 6 * n_got:] == 0.0), what


def new_oracle(sd, E, W, smooth, stats):
    return StreamOracle(sd, E, W, smooth, stats)


def make_bank(model, S, smooth, stats, seed=0x5EED):
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    bank = KalmanStreamBank(model, S, smooth=smooth, normalize=False, seed=seed)
    if stats is not None:
        bank.set_norm_stats(stats)
    bank.set_body(orc.DEFAULT_BODY)
    return bank


def run_frame(bank, rows, streams, nz, init):
    """one injected frame -> host arrays (packed [K, w], n_rows [K], y [K, E, 14])"""
    blob = torch.from_numpy(pack_noise(nz))
    ini = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32))
    if streams is None:
        out, n, y = bank.step_rows(rows, datagrams=True, noise=blob, init_noise=ini, return_targets=True)
    else:
        out, n, y = bank.frame(rows, streams, datagrams=True, noise=blob, init_noise=ini, return_targets=True)
    return out.cpu().numpy().copy(), n.cpu().numpy().copy(), y.cpu().numpy().copy()


@pytest.mark.parametrize("smooth", [1, 3])
@pytest.mark.parametrize("normalize", [False, True])
def test_one_stream_bank_against_the_oracle_chain(norm_stats, smooth, normalize):
    """14 frames: both transitions -- init to ensemble, and the ragged stack smooth -> ... -> smooth * E"""
    E, W = 32, 10
    stats = pocket_stats(norm_stats) if normalize else None
    m, sd = make_model(E, W, 21)
    bank = make_bank(m, 1, smooth, stats)
    so = new_oracle(sd, E, W, smooth, stats)
    rng = np.random.default_rng(100 + smooth)
    rows = make_rows(rng, W + 4)
    counts = []
    for f in range(W + 4):
        nz, init = ko.draw_noise(rng, W, E), rng.standard_normal((1, E, 14)).astype(np.float32)
        out, n, y = run_frame(bank, rows[f:f + 1], None, nz, init)
        so.check(rows[f], nz, init[0], y[0], int(n[0]), out[0], f"smooth {smooth} norm {normalize} frame {f}")
        counts.append(int(n[0]))
    want = {1: [1] * (W + 1) + [E] * 3, 3: [3] * (W + 1) + [2 + E, 1 + 2 * E, 3 * E]}[smooth]
    assert counts == want
    bank.check()


@pytest.mark.parametrize("E,W", [(48, 10), (16, 4)])
def test_five_streams_with_staggered_cold_starts(norm_stats, E, W):
    """lockstep frames, subset frames in scrambled list order, reset(streams=[...]) mid-run, lockstep again: every stream equals its
    own oracle chain fed only its rows, the call's shared eps and its slice of signs and init noise by list position"""
    S, smooth = 5, 2
    stats = pocket_stats(norm_stats)
    m, sd = make_model(E, W, 22)
    bank = make_bank(m, S, smooth, stats)
    oracles = [new_oracle(sd, E, W, smooth, stats) for _ in range(S)]
    rng = np.random.default_rng(E)
    # at most 14 frames per stream since its cold start (the feedback length the target bound is stated for): streams 0, 2 and 4 end
    # with 14, 14 and 13 frames -- past the W + 1 init frames for both window sizes -- streams 1 and 3 with 10 since their reset
    plan = ([None] * 2 + [[3, 0], [4, 1, 2], [2, 4, 0, 3], [1], [0, 2]] + ["reset:1,3"] + [[3, 1], None, None] +
            [[4, 0, 1], [2, 3]] + [None] * 6)
    for step, item in enumerate(plan):
        if isinstance(item, str):
            idx = [int(v) for v in item.split(":")[1].split(",")]
            bank.reset(streams=idx)
            for s in idx:
                oracles[s].reset()
            continue
        order = list(range(S)) if item is None else item
        K = len(order)
        rows = make_rows(rng, K)
        nz, init = ko.draw_noise(rng, W, K * E), rng.standard_normal((K, E, 14)).astype(np.float32)
        out, n, y = run_frame(bank, rows, item, nz, init)
        for j, s in enumerate(order):
            oracles[s].check(rows[j], slice_noise(nz, j, E), init[j], y[j], int(n[j]), out[j], f"E {E} step {step} stream {s}")
    # every phase was visited: some stream is past its W + 1 init frames, some stream was cold-started mid-run
    assert [o.fl.init_step for o in oracles] == [min(v, W + 1) for v in (14, 10, 14, 10, 13)]
    bank.check()


def test_unlisted_streams_are_untouched(norm_stats):
    """bank A: frames that never list stream 3, then stream 3 alone; bank B: only that frame, same draws -> bit-equal outputs"""
    E, W, S = 32, 10, 5
    stats = pocket_stats(norm_stats)
    m, _ = make_model(E, W, 23)
    a, b = make_bank(m, S, 3, stats), make_bank(m, S, 3, stats)
    rng = np.random.default_rng(7)
    for order in ([0, 1, 2, 4], [4, 2], [1, 0, 4, 2], [2]):
        K = len(order)
        run_frame(a, make_rows(rng, K), order, ko.draw_noise(rng, W, K * E), rng.standard_normal((K, E, 14)))
    # (both frames are init frames of stream 3: its prediction is row 0 of y, the other rows are unspecified)
    for _ in range(2):            # the second frame reads what the first left in stream 3's rings
        row, nz, init = make_rows(rng, 1), ko.draw_noise(rng, W, E), rng.standard_normal((1, E, 14))
        (oa, na, ya), (ob, nb, yb) = run_frame(a, row, [3], nz, init), run_frame(b, row, [3], nz, init)
        np.testing.assert_array_equal(oa, ob)
        np.testing.assert_array_equal(na, nb)
        np.testing.assert_array_equal(ya[:, :1], yb[:, :1])
        assert na.tolist() == [3] and np.all(np.isfinite(oa))
    a.check()


def test_subset_frames_back_to_back(norm_stats):
    """20 subset frames enqueued with no host synchronisation in between (rows and draws already on the device): the pinned ring of
    stream lists (csrc/bank_host.h) wraps more than twice.  Bit-equal to the same frames with a device synchronisation after each,
    and every stream within the suite's bounds of its own oracle chain."""
    E, W, S, smooth, frames = 16, 4, 3, 2, 20
    stats = pocket_stats(norm_stats)
    m, sd = make_model(E, W, 24)
    rng = np.random.default_rng(24)
    # two of the three streams per frame, scrambled: 13, 13 and 14 frames per stream (the feedback length the target bound is stated for)
    lists = [[int(s) for s in rng.permutation([s for s in range(S) if s != f % S])] for f in range(frames)]
    rows = [make_rows(rng, 2) for _ in lists]
    draws = [(ko.draw_noise(rng, W, 2 * E), rng.standard_normal((2, E, 14)).astype(np.float32)) for _ in lists]
    dev = [(torch.from_numpy(r).cuda(), torch.from_numpy(pack_noise(nz)).cuda(), torch.from_numpy(init).cuda())
           for r, (nz, init) in zip(rows, draws)]

    def run(sync):
        bank = make_bank(m, S, smooth, stats)
        torch.cuda.synchronize()
        res = []
        for (rd, blob, ini), order in zip(dev, lists):
            res.append(tuple(t.clone() for t in bank.frame(rd, order, datagrams=True, noise=blob, init_noise=ini, return_targets=True)))
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        bank.check()
        return [tuple(t.cpu().numpy() for t in r) for r in res]

    queued, synced = run(False), run(True)
    oracles = [new_oracle(sd, E, W, smooth, stats) for _ in range(S)]
    seen = [0] * S
    for f, order in enumerate(lists):
        (out, n, y), (out_s, n_s, y_s) = queued[f], synced[f]
        np.testing.assert_array_equal(out, out_s, err_msg=f"frame {f}")
        np.testing.assert_array_equal(n, n_s, err_msg=f"frame {f}")
        nz, init = draws[f]
        for j, s in enumerate(order):
            k = 1 if seen[s] <= W else E                        # (an init frame's prediction is row 0 of y alone)
            np.testing.assert_array_equal(y[j, :k], y_s[j, :k], err_msg=f"frame {f} stream {s}")
            oracles[s].check(rows[f][j], slice_noise(nz, j, E), init[j], y[j], int(n[j]), out[j], f"back to back frame {f} stream {s}")
            seen[s] += 1
    assert seen == [13, 13, 14]


def _frame_host(bank, rows, big_endian=False, packed=True):
    from wear_mocap_ape_amd import _hip
    S, w = bank.n_streams, bank.packed_width if packed else 25
    out, n = np.zeros((S, w)), np.zeros(S, dtype=np.int32)
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if big_endian:
        rows = rows.byteswap()
    kind = _hip.PARSE_WATCH_PHONE_POCKET | (_hip.PARSE_BIG_ENDIAN if big_endian else 0)
    _hip.check(_hip.lib().ape_kalman_bank_frame_host(bank._handle, kind, C.c_void_p(rows.ctypes.data), _hip.FLAG_PACKED_MSG if packed else 0,
                                                     C.c_void_p(out.ctypes.data), _hip.F64, C.c_void_p(n.ctypes.data), None), "frame_host")
    return out, n


def test_host_entry_equals_the_device_entry_and_big_endian_rows(norm_stats):
    E, W, S = 32, 4, 4
    stats = pocket_stats(norm_stats)
    m, _ = make_model(E, W, 24)
    host, dev, be = (make_bank(m, S, 2, stats, seed=99) for _ in range(3))
    rng = np.random.default_rng(8)
    for f in range(W + 4):
        rows = make_rows(rng, S)
        oh, nh = _frame_host(host, rows)
        od, nd = dev.step_rows(torch.from_numpy(rows).cuda(), datagrams=True)
        ob, nb = be.step_rows(rows.byteswap(), big_endian=True, datagrams=True)
        np.testing.assert_array_equal(oh, od.cpu().numpy())
        np.testing.assert_array_equal(nh, nd.cpu().numpy())
        np.testing.assert_array_equal(oh, ob.cpu().numpy())
        np.testing.assert_array_equal(nh, nb.cpu().numpy())
    assert nh.tolist() == [2 * E] * S
    # float32 messages are the float64 ones rounded; the unpacked row is the packed row's head
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    f32 = KalmanStreamBank(m, S, smooth=2, normalize=False, seed=99, dtype=torch.float32)
    f32.set_norm_stats(stats)
    f32.set_body(orc.DEFAULT_BODY)
    f64 = make_bank(m, S, 2, stats, seed=99)
    rows = make_rows(rng, S)
    a = f32.step_rows(rows, datagrams=True)[0].cpu().numpy()
    b = f64.step_rows(rows).cpu().numpy()
    assert a.dtype == np.float32 and b.shape == (S, 25)
    np.testing.assert_array_equal(a[:, :25], b.astype(np.float32))
    dev.check()


def _estimator(sd, E, W, smooth=1, **kw):
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    return WatchPhonePocketKalman({k: torch.from_numpy(v) for k, v in sd.items()}, smooth=smooth, num_ensemble=E, window_size=W, **kw)


def test_process_row():
    E, W = 32, 10
    sd = ko.make_state_dict(W, 25)
    rng = np.random.default_rng(9)
    rows = make_rows(rng, W + 3)
    est = _estimator(sd, E, W)                       # normalize=True: the shipped statistics
    est.manual_seed(77)
    first = [est.process_row(r) for r in rows]
    assert all(isinstance(mm, list) for mm in first)
    assert [len(mm) for mm in first] == [25] * (W + 1) + [25 + 6 * E] * 2
    assert all(np.all(np.isfinite(np.asarray(mm))) for mm in first)
    np.testing.assert_array_equal(est.get_last_msg(), np.asarray(first[-1][:25]))
    est.reset()
    again = [est.process_row(r) for r in rows]
    assert again == first                            # reset() reproduces the run
    est.manual_seed(78)
    est.reset()
    other = [est.process_row(r) for r in rows]
    assert other[0] != first[0] and [len(mm) for mm in other] == [len(mm) for mm in first]
    # a one-stream bank with that seed: the same bits
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    bank = KalmanStreamBank(est.model, 1, smooth=1, normalize=True, seed=77)
    for r, mm in zip(rows, first):
        msg = bank.step_rows(r[None, :]).cpu().numpy()[0]
        np.testing.assert_array_equal(msg, np.asarray(mm[:25]))
    # msg_as_array, add_mc_samples=False
    arr = _estimator(sd, E, W)
    arr.msg_as_array = True
    arr.manual_seed(77)
    got = [arr.process_row(r) for r in rows]
    assert all(isinstance(g, np.ndarray) and g.dtype == np.float64 for g in got)
    assert [g.tolist() for g in got] == first
    plain = _estimator(sd, E, W, add_mc_samples=False)
    plain.manual_seed(77)
    got = [plain.process_row(r) for r in rows]
    assert all(isinstance(g, np.ndarray) and g.shape == (25,) for g in got)
    assert [g.tolist() for g in got] == [mm[:25] for mm in first]
    # the staged path still runs
    staged = _estimator(sd, E, W)
    staged.use_device_frame = False
    msgs = [staged.process_row(r) for r in rows]
    assert getattr(staged, "_device_frame", None) is None
    assert [len(mm) for mm in msgs] == [25] * (W + 1) + [25 + 6 * E] * 2 and all(isinstance(mm, list) for mm in msgs)
    # smooth 3: the ragged lengths
    s3 = _estimator(sd, E, W, smooth=3)
    assert [len(s3.process_row(r)) for r in rows] == [25 + 18] * (W + 1) + [25 + 6 * (2 + E), 25 + 6 * (1 + 2 * E)]
    est.model.check()


def test_replay(norm_stats):
    """three ragged recordings (one shorter than W + 1 frames): bit-equal to a fresh bank stepped as the definition says; one recording
    with starts=None equals frame-by-frame process_row with the same seed"""
    E, W, smooth, seed = 16, 4, 2, 4242
    sd = ko.make_state_dict(W, 26)
    est = _estimator(sd, E, W, smooth=smooth)
    rng = np.random.default_rng(10)
    lens = [9, 3, 7]
    starts = np.cumsum([0] + lens[:-1])
    rows = make_rows(rng, sum(lens))
    out, n, y = est.process_recording(rows, starts=starts, seed=seed, return_targets=True)
    assert tuple(out.shape) == (sum(lens), 25 + 6 * smooth * E) and out.dtype == torch.float64 and n.dtype == torch.int32
    out, n, y = out.cpu().numpy(), n.cpu().numpy(), y.cpu().numpy()
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    bank = KalmanStreamBank(est.model, 3, smooth=smooth, normalize=True, seed=seed)
    for t in range(max(lens)):
        order = [r for r in range(3) if lens[r] > t]
        idx = [starts[r] + t for r in order]
        o, nn, yy = bank.frame(rows[idx], order, datagrams=True, return_targets=True)
        np.testing.assert_array_equal(out[idx], o.cpu().numpy())
        np.testing.assert_array_equal(n[idx], nn.cpu().numpy())
        for j, i in enumerate(idx):
            k = 1 if t <= W else E
            np.testing.assert_array_equal(y[i, :k], yy.cpu().numpy()[j, :k])
    assert n[starts[1]:starts[1] + 3].tolist() == [smooth] * 3 and n[starts[0] + 8] == 2 * E
    # big-endian rows, float32 output
    o32, n32 = est.process_recording(rows.byteswap(), starts=starts, big_endian=True, out_dtype=torch.float32, seed=seed)
    np.testing.assert_array_equal(o32.cpu().numpy(), out.astype(np.float32))
    np.testing.assert_array_equal(n32.cpu().numpy(), n)
    # one recording == process_row frame by frame
    one, n1 = est.process_recording(rows[:9], seed=seed)
    one, n1 = one.cpu().numpy(), n1.cpu().numpy()
    est.manual_seed(seed)
    est.reset()
    from wear_mocap_ape_amd.streams import trim_packed
    for f in range(9):
        assert est.process_row(rows[f]) == trim_packed(one[f], n1[f]).tolist()
    # without add_mc_samples: [F, 25]
    plain = _estimator(sd, E, W, smooth=smooth, add_mc_samples=False)
    p, pn = plain.process_recording(rows, starts=starts, seed=seed)
    assert tuple(p.shape) == (sum(lens), 25)
    np.testing.assert_array_equal(p.cpu().numpy(), out[:, :25])
    np.testing.assert_array_equal(pn.cpu().numpy(), n)
    est.model.check()


def test_device_draws_match_the_oracles_distribution():
    """frame 0 of a fresh one-stream bank depends on the draws alone (the zero state through the process model; the sensor model gives
    z): 260 banks with different seeds against 260 oracle calls under numpy draws, tests/mc_check.py at 5.5 standard errors"""
    E, W = 32, 10
    m, sd = make_model(E, W, 27)
    rng = np.random.default_rng(11)
    row = make_rows(rng, 1)
    xx = features(row[0])
    hist = np.vstack([xx] * W)
    state = np.zeros((1, E, W, 14), np.float32)
    ref = np.stack([ko.kalman_forward(sd, hist.astype(np.float32)[None, :, None, :], state, ko.draw_noise(rng, W, E))[3][0, 0]
                    for _ in range(260)])
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    got = []
    for k in range(260):
        bank = KalmanStreamBank(m, 1, smooth=1, normalize=False, seed=1000 + k)
        _, y = bank.step_rows(row, return_targets=True)
        got.append(y.cpu().numpy()[0, 0].copy())
        if k == 0:
            _, y1 = bank.step_rows(row, return_targets=True)
            assert not np.array_equal(y1.cpu().numpy()[0, 0], got[0])      # the key advances: same row, other draws
    got = np.stack(got)
    levels = np.array([0.1, 0.5, 0.9])
    bad = mc_check.compare(got, ref.mean(axis=0), np.cov(ref, rowvar=False), np.quantile(ref, levels, axis=0), levels, 260, "frame 0 z")
    assert not bad, bad
    m.check()


def test_refusals_that_need_a_model(norm_stats):
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import kalman_models
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    lib = _hip.lib()
    m, _ = make_model(128, 4, 28)
    with pytest.raises(UserWarning, match="not loaded"):
        KalmanStreamBank(kalman_models.KalmanSmartwatchModel(32, 10), 2, normalize=False)
    with pytest.raises(UserWarning, match="smooth"):
        KalmanStreamBank(m, 2, smooth=65, normalize=False)
    with pytest.raises(UserWarning, match="stacked rows"):
        KalmanStreamBank(m, 2, smooth=33, normalize=False)            # 33 x 128 > 4096
    bank = make_bank(m, 4, 1, None)
    rows = torch.zeros((4, 55), dtype=torch.float32, device="cuda")
    out = torch.zeros((4, 25), dtype=torch.float64, device="cuda")
    n = torch.zeros((4,), dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                # noqa: E731
    pocket = _hip.PARSE_WATCH_PHONE_POCKET

    def frame(idx, K, kind=pocket, dtype=_hip.F64):
        a = np.asarray(idx, dtype=np.int32) if idx is not None else None
        return lib.ape_kalman_bank_frame(bank._handle, kind, p(rows), C.c_void_p(a.ctypes.data) if a is not None else None, K, None, None,
                                         0, p(out), dtype, p(n), None, None)
    for idx, K in (([0, 1], -1), ([0, 1, 2, 3, 0], 5), (None, 3), ([0, 4], 2), ([-1], 1), ([2, 2], 2)):
        assert frame(idx, K) != 0 and lib.ape_last_error(), (idx, K)
    assert frame([0], 1, kind=_hip.PARSE_WATCH_PHONE_UARM) != 0
    assert frame([0], 1, dtype=5) != 0
    idx = np.array([1, 1], dtype=np.int32)
    assert lib.ape_kalman_bank_reset_subset(bank._handle, C.c_void_p(idx.ctypes.data), 2) != 0
    assert frame([], 0) == 0                                   # K = 0: a no-op
    with pytest.raises(UserWarning):
        bank.frame(np.zeros((2, 55), np.float32), [1, 1])
    # ... and after all that the bank still works, and no frame of this module met a singular innovation
    row = make_rows(np.random.default_rng(0), 4)
    assert tuple(bank.step_rows(row).shape) == (4, 25)
    m.check()
