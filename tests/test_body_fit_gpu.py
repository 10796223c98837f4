"""Each recording's arm lengths and shoulder origin against the truth (`ape_body_sums`, `ape_rebody_rows`) on the GPU.

References: `score.body_sums_numpy` and `score.rebody_rows_numpy` (tests/test_body_fit_cpu.py holds them to hand-written numpy).
Tolerances: every sum within 16 n 2^-53 max(1, max |t|^2) of the statement, n the pairs summed (rotation entries are <= 1, so no term
exceeds the largest squared norm of a truth position) -- the rule tests/test_frame_fit_gpu.py uses -- and the two counts exact; a
rewritten float64 row within 1e-14 (about 60 float64 operations on values below 2), a float32 one within one float32 ulp of the statement
rounded to float32.  End to end: bodies and mean errors within 1e-9, as tests/test_frame_fit_gpu.py asks of the heading."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_body_fit_cpu import HIPS, POS, WATCH, check_sums, default_body, planted_body, planted_case, truth_bound
from tests.test_frame_fit_cpu import general_quat, msgs_from_est, turn_est, walk_est, yaw_quat
from tests.test_score_gpu import dev

pytestmark = pytest.mark.gpu

F = 1000
STARTS, LAGS, REC_LAGS, SKIP = [0, 37, 300, 301, 900], (-5, 7), [0, 2, -3, 0, 1], 2       # [300, 301): one frame, no support
WIDE = 70


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def sums(layout, msg, truth, lags, kind="est", **kw):
    from wear_mocap_ape_amd import score
    t = lambda a: a if a is None or isinstance(a, torch.Tensor) else dev(a)              # noqa: E731
    acc = score.body_sums(layout, t(msg), t(truth), lags, kind, **kw)
    torch.cuda.synchronize()
    return acc.cpu().numpy()


# ---- 1: against the statement --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case1(golden):
    """per layout: messages, NN targets, the est rows the reference's FK makes of them (fixtures), and the statement's sums for float64 and
    for float32 messages and for the truth's rotations -- computed once"""
    from wear_mocap_ape_amd.score import body_sums_numpy
    cache = {}

    def get(layout):
        if layout not in cache:
            g = golden(f"fk_layout{layout}.npz")
            pick = np.random.default_rng(11 + layout).integers(0, 300, size=F)
            msg = msgs_from_est(walk_est(F, WATCH if layout == WATCH else HIPS, seed=21 + layout), layout)
            d = {"msg": msg, "preds": g["preds_bd_N300"][pick], "est": g["est_bd_N300"][pick]}
            for name, m in (("f64", msg), ("f32", msg.astype(np.float32).astype(np.float64))):
                d[name] = body_sums_numpy(m, d["est"], layout, LAGS, STARTS, SKIP, REC_LAGS)
            d["truth"] = body_sums_numpy(None, d["est"], layout, (0, 0), STARTS, SKIP, rotations="truth")
            d["bound"] = truth_bound(d["est"])
            cache[layout] = d
        return cache[layout]
    return get


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("layout,kind", [(HIPS, "est"), (WATCH, "est"), (POS, "est"), (POS, "targets")])
def test_sums_against_the_statement(case1, layout, kind, dtype, strided):
    d = case1(layout)
    md = dev(d["msg"], dtype)
    if strided:                                             # messages inside NaN-filled 70-wide rows
        wide = torch.full((F, WIDE), float("nan"), dtype=dtype, device="cuda")
        wide[:, :25] = md
        md = wide[:, :25]
        assert not md.is_contiguous() and md.stride(0) == WIDE
    truth = d["est"] if kind == "est" else d["preds"]
    got = sums(layout, md, truth, LAGS, kind, starts=STARTS, skip=SKIP, rec_lags=REC_LAGS)
    ref = d["f64" if dtype == torch.float64 else "f32"]
    assert got.shape == (5, 13, 46)
    worst = check_sums(got, ref, d["bound"], (layout, kind, dtype, strided))
    print(f"layout {layout} {kind} {dtype} strided={strided}: worst deviation {worst:.3f} of the allowance")
    assert not got[2].any() and all(got[r].any() for r in (0, 1, 3, 4))                  # the one-frame recording is all zeros
    assert (got[:, :, 44] + got[:, :, 45] == (got[:, :1, 44] + got[:, :1, 45])).all()
    assert np.array_equal(got[:, :, :27], np.broadcast_to(got[:, :1, :27], got[:, :, :27].shape)) or got[:, :, 45].any()
    if layout == WATCH:                                     # R_h = I: [9:18] is the sum of R_l', [33:36] the sum of t_h
        from wear_mocap_ape_amd.score import _quat_matrix
        m = d["msg"] if dtype == torch.float64 else d["msg"].astype(np.float32).astype(np.float64)
        for r, j in ((0, 0), (4, 12)):
            s, e = STARTS[r], (STARTS + [F])[r + 1]
            a, b = max(s + SKIP, s + REC_LAGS[r] + LAGS[1]), min(e, e + REC_LAGS[r] + LAGS[0])
            want = np.transpose(_quat_matrix(m[a:b, 7:11]), (0, 2, 1)).reshape(-1, 9).sum(axis=0)
            assert np.abs(got[r, j, 9:18] - want).max() <= 16 * (b - a) * 2.0 ** -53


@pytest.mark.parametrize("layout,kind,tdtype", [(HIPS, "est", torch.float64), (WATCH, "est", torch.float64), (POS, "est", torch.float64),
                                                (POS, "targets", torch.float64), (HIPS, "est", torch.float32), (WATCH, "est", torch.float32)])
def test_sums_with_the_truths_rotations(case1, layout, kind, tdtype):
    """APE_BODY_ROT_TRUTH: the single lag 0, no message; a float32 truth is the statement of the rounded est rows (targets have no
    rounded est rows to state: float64 only)"""
    from wear_mocap_ape_amd.score import body_sums_numpy
    d = case1(layout)
    truth = d["est"] if kind == "est" else d["preds"]
    ref = d["truth"] if tdtype == torch.float64 else body_sums_numpy(None, d["est"].astype(np.float32).astype(np.float64), layout, (0, 0), STARTS,
                                                                     SKIP, rotations="truth")
    got = sums(layout, None, dev(truth, tdtype), (0, 0), kind, starts=STARTS, skip=SKIP, rotations="truth")
    assert got.shape == (5, 1, 46) and not got[2].any()
    worst = check_sums(got, ref, d["bound"], (layout, kind, "truth"))
    print(f"layout {layout} {kind} {tdtype} rotations=truth: worst deviation {worst:.3f} of the allowance")
    with pytest.raises(UserWarning, match="single lag 0"):
        sums(layout, None, dev(truth, tdtype), (0, 1), kind, starts=STARTS, rotations="truth")
    with pytest.raises(UserWarning, match="rec_lag_host"):
        sums(layout, None, dev(truth, tdtype), (0, 0), kind, starts=STARTS, rec_lags=REC_LAGS, rotations="truth")


def test_target_truth_of_the_body_made_layouts_is_refused(case1):
    for layout in (HIPS, WATCH):
        d = case1(layout)
        with pytest.raises(UserWarning, match="body being fitted"):
            sums(layout, d["msg"], d["preds"], (0, 0), "targets")


# ---- 2: edges ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_edges_of_waves_and_tiles(n):
    from wear_mocap_ape_amd.score import body_sums_numpy
    msg, truth, _ = planted_case(n, HIPS, seed=n, lag=1)
    bound = truth_bound(truth)
    md, td = dev(msg), dev(truth)
    cuts = [[0], [0, 64], [0, 63], [0, 65], [0, 256], [0, 255], [0, 257], [0, 63, 64, 65, 255, 256, 257], [0, 64, 128, 192, 256, 320]]
    for starts in cuts:
        starts = [s for s in starts if s < n]
        for lags, skip in (((0, 0), 0), ((-1, 2), 1)):
            got = sums(HIPS, md, td, lags, starts=starts, skip=skip)
            check_sums(got, body_sums_numpy(msg, truth, HIPS, lags, starts, skip), bound, (n, starts, lags))


# ---- 3: unusable input ---------------------------------------------------------------------------------------------------------------------------
def test_unusable_pairs_move_between_the_two_counts():
    from wear_mocap_ape_amd.score import body_sums_numpy
    msg, truth, _ = planted_case(12, HIPS, seed=5, lag=0)
    lags = (-2, 2)
    clean = sums(HIPS, msg, truth, lags)
    assert (clean[0, :, 44] == 8).all() and not clean[0, :, 45].any()
    truth[9, 6] = np.nan                                    # the est shoulder origin: not read
    assert np.array_equal(sums(HIPS, msg, truth, lags), clean)
    msg[3, 5] = np.nan                                      # a position of the message: not read either
    assert np.array_equal(sums(HIPS, msg, truth, lags), clean)
    msg[4, 9], truth[6, 1], msg[8, 14:18] = np.nan, np.inf, 0.0
    got = sums(HIPS, msg, truth, lags)
    ref = body_sums_numpy(msg, truth, HIPS, lags)
    check_sums(got, ref, truth_bound(truth), "unusable")
    # the support is frames 2 .. 9: frames 4 and 8 (its zero quaternion) are lost at every lag, truth row 6 meets frame 6 + l
    lost = [2 + (2 <= 6 + l <= 9 and 6 + l not in (4, 8)) for l in range(-2, 3)]
    assert got[0, :, 45].tolist() == lost and (got[0, :, 44] + got[0, :, 45] == 8).all()
    # with the truth's rotations a zero truth quaternion loses its row, the message's state is not read at all
    truth[7, 13:17] = 0.0
    got_t = sums(HIPS, None, truth, (0, 0), rotations="truth")
    check_sums(got_t, body_sums_numpy(None, truth, HIPS, (0, 0), rotations="truth"), truth_bound(truth), "unusable, truth")
    assert got_t[0, 0, 44:].tolist() == [10, 2]             # rows 6 and 7 of 12


# ---- 4: determinism -------------------------------------------------------------------------------------------------------------------------------
def test_same_inputs_same_bits(case1):
    from wear_mocap_ape_amd import score
    d = case1(HIPS)
    md, td = dev(d["msg"]), dev(d["est"])
    kw = dict(starts=STARTS, skip=SKIP, rec_lags=REC_LAGS)
    a = sums(HIPS, md, td, LAGS, **kw)
    b = sums(HIPS, md, td, LAGS, **kw)
    score.score_lags(HIPS, md, td, (-8, 8), "est", starts=STARTS)
    c = sums(HIPS, md, td, LAGS, **kw)
    assert np.array_equal(a, b) and np.array_equal(a, c)


# ---- 5: rebody_rows --------------------------------------------------------------------------------------------------------------------------------
def rebody(layout, msg, bodies, **kw):
    from wear_mocap_ape_amd import score
    res = score.rebody_rows(layout, msg, bodies, **kw)
    torch.cuda.synchronize()
    return res.cpu().numpy()


@pytest.mark.parametrize("layout", [HIPS, WATCH])
def test_rebody_rows_against_its_statement(layout):
    from wear_mocap_ape_amd.score import rebody_rows_numpy
    n, starts = 300, [0, 64, 65, 257]
    rng = np.random.default_rng(9)
    msg = msgs_from_est(walk_est(n, layout, seed=6), layout)
    msg[:, 0:4] = rng.uniform(-1.0, 1.0, size=(n, 4))
    msg[[10, 64, 299, 100, 200], [5, 22, 0, 8, 15]] = np.nan
    bodies = np.stack([planted_body(0), planted_body(1), default_body(), 2.0 * planted_body(0)])
    for bd, st in ((bodies, starts), (bodies[1], starts), (bodies[0], None)):
        want = rebody_rows_numpy(msg, bd, layout, st)
        got = rebody(layout, dev(msg), bd, starts=st)
        assert got.shape == (n, 25) and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.nanmax(np.abs(got - want)) <= 1e-14
        # NaN stays where the statement puts it: a NaN input position is made again, a NaN quaternion spoils what hangs on it
        assert np.isfinite(got[10]).all() and np.isnan(got[299, 0]) and np.isfinite(got[299, 1:]).all()
        assert np.isnan(got[100, 4:7]).all() and np.isfinite(got[100, 11:14]).all() and np.isfinite(got[100, 18:21]).all()
        assert np.isnan(got[200, 4:7]).all() and np.isnan(got[200, 11:14]).all() and np.isfinite(got[200, 18:21]).all()
        assert np.isnan(got[64, 22]) and np.isnan(got[64, [4, 11, 18]]).all() == (layout == HIPS)
        assert np.isfinite(got[[9, 11, 63, 65, 99, 101, 199, 201]]).all()
    # float32 storage: float64 arithmetic, rounded once; strided rows in, nothing past column 24 read
    m32 = msg.astype(np.float32)
    wide = torch.full((n, WIDE), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :25] = dev(m32)
    want = rebody_rows_numpy(m32.astype(np.float64), bodies, layout, starts)
    for out_dtype, npdt in ((None, np.float32), (torch.float32, np.float32), (torch.float64, np.float64)):
        got = rebody(layout, wide[:, :25], bodies, starts=starts, out_dtype=out_dtype)
        assert got.dtype == npdt and np.array_equal(np.isnan(got), np.isnan(want))
        if npdt == np.float32:
            w32 = want.astype(np.float32)
            ok = np.isfinite(w32)
            assert (np.abs(got[ok] - w32[ok]) <= np.spacing(np.abs(w32[ok]))).all()
        else:
            assert np.nanmax(np.abs(got - want)) <= 1e-14
    for bad in (np.zeros(8), np.ones((2, 9))):
        with pytest.raises(UserWarning):
            rebody(layout, dev(msg), bad, starts=starts)
    with pytest.raises(UserWarning, match="predicted"):
        rebody(POS, dev(msg), bodies[0])


# ---- 6: end to end on a replay ------------------------------------------------------------------------------------------------------------------------
def est_of(rows):
    """est rows [F, 14] of the FK-only estimator's messages"""
    return np.concatenate([rows[:, 4:7], rows[:, 11:14], rows[:, 7:11], rows[:, 14:18]], axis=1)


@pytest.fixture(scope="module")
def replay():
    """1000 random frames in two recordings through the FK-only estimator: under two planted bodies (the truth) and under the default one
    (the estimate) -- replayed once"""
    from tests.test_fk_only_gpu import _random_rows
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    est_obj = WatchPhoneUarm(smooth=1)
    starts, planted = [0, 400], np.stack([planted_body(0), planted_body(1)])
    rows = _random_rows(np.random.default_rng(17), 1000)
    truth_out = est_obj.process_recording(rows, starts=starts, bonemaps=planted)
    out = est_obj.process_recording(rows, starts=starts)
    torch.cuda.synchronize()
    assert torch.isfinite(truth_out).all() and torch.isfinite(out).all()
    return {"est_obj": est_obj, "rows": rows, "starts": starts, "ends": [400, 1000], "planted": planted, "truth_out": truth_out, "out": out}


def test_fit_bodies_recovers_planted_bodies(replay):
    from wear_mocap_ape_amd import score
    from wear_mocap_ape_amd.streams import FkStreamBank
    p = replay
    est_obj, starts, out = p["est_obj"], p["starts"], p["out"]
    td = dev(est_of(p["truth_out"].cpu().numpy()))
    _, acc0 = est_obj.score_recording(out, td, starts=starts, truth_kind="est")
    sc, acc, found = est_obj.fit_bodies(out, td, starts=starts)
    torch.cuda.synchronize()
    before, after = score.summarise(acc0), score.summarise(acc)
    for r in range(2):
        worst = np.abs(found[r]["body"] - p["planted"][r]).max()
        print(f"recording {r}: lag {found[r]['lag']}, cond {found[r]['cond']:.2f}, max |body - plant| {worst:.3e}, hand rms "
              f"{found[r]['hand_rms_before']:.4f} -> {found[r]['hand_rms_after']:.2e}, mean errors after {after[r]['mean']}")
        assert found[r]["ok"] and found[r]["lag"] == 0 and worst <= 1e-9 and found[r]["pairs"] == p["ends"][r] - starts[r]
        assert before[r]["mean"]["hand_pos"] > 0.005
        assert all(v <= 1e-9 for v in after[r]["mean"].values()), after[r]["mean"]
    assert tuple(sc.shape) == (1000, 7) and tuple(acc.shape) == (2, 25)
    bodies = score.bodies_of(found)
    again = score.rebody_rows(WATCH, out, bodies, starts)
    assert float((again - p["truth_out"]).abs().max()) <= 1e-12
    fitted = est_obj.process_recording(p["rows"], starts=starts, bonemaps=bodies)
    _, acc1 = est_obj.score_recording(fitted, td, starts=starts, truth_kind="est")
    for r, s in enumerate(score.summarise(acc1)):
        assert all(v <= 1e-9 for v in s["mean"].values()), (r, s["mean"])
    bank = FkStreamBank(2, smooth=1)
    bank.set_bodies(bodies)
    assert np.array_equal(bank.bodies, bodies)
    # the pieces: align_body is body_sums -> best_body -> rebody_rows -> score_lags; the lengths form does not reach a body whose
    # vectors are not the prior's scaled
    sums_ = score.body_sums(WATCH, out, td, (0, 0), "est", starts)
    pieces = score.best_body(sums_, (0, 0))
    assert all(np.array_equal(a["body"], b["body"]) for a, b in zip(pieces, found))
    _, _, rough = est_obj.fit_bodies(out, td, starts=starts, mode="lengths")
    assert all(f["ok"] and f["hand_rms_after"] < f["hand_rms_before"] and f["hand_rms_after"] > 1e-3 for f in rough)


# ---- 7: chained with the heading ------------------------------------------------------------------------------------------------------------------------
def test_heading_lag_and_body_are_removed_in_turn(replay):
    from wear_mocap_ape_amd import score
    p = replay
    est_obj, starts, ends, out = p["est_obj"], p["starts"], p["ends"], p["out"]
    yaws, adv = [0.3, -0.2], [3, 0]
    est = est_of(p["truth_out"].cpu().numpy())
    truth = np.empty_like(est)
    for s, e, psi, k in zip(starts, ends, yaws, adv):
        idx = np.clip(np.arange(s, e) + k, s, e - 1)        # truth row f states frame f + k: the estimate is late by k
        truth[s:e] = turn_est(est[idx], yaw_quat(psi), WATCH)
    td = dev(truth)
    _, acc_h, heading = est_obj.align_recording(out, td, starts=starts, truth_kind="est", lags=(-8, 8))
    quats, lags = np.stack([h["quat"] for h in heading]), [h["lag"] for h in heading]
    assert lags == adv and all(abs(h["yaw"] - psi) <= 1e-9 for h, psi in zip(heading, yaws))
    sc, acc, found = est_obj.fit_bodies(out, td, starts=starts, quats=quats, rec_lags=lags)
    torch.cuda.synchronize()
    half, after = score.summarise(acc_h), score.summarise(acc)
    for r in range(2):
        print(f"recording {r}: hand error with the heading removed {half[r]['mean']['hand_pos']:.4f}, with the body too {after[r]['mean']}")
        assert half[r]["mean"]["hand_pos"] > 0.005          # without the body step the hand error stays
        assert found[r]["ok"] and found[r]["lag"] == adv[r]
        assert all(v <= 1e-9 for v in after[r]["mean"].values()), after[r]["mean"]
        assert after[r]["scored"] == ends[r] - starts[r] - adv[r]
        # the arm vectors are the planted ones; without hips the shoulder origin found is the planted one in the truth's frame
        assert np.abs(found[r]["body"][:6] - p["planted"][r][:6]).max() <= 1e-9
    assert tuple(sc.shape) == (1000, 7)


# ---- 8: a capturing stream ----------------------------------------------------------------------------------------------------------------------------
def test_a_capturing_stream_is_refused_by_both_entries():
    """both entries stage host arrays per call: on a stream that is capturing a graph they return APE_ERR_INVALID_ARG and write nothing"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    n = 64
    msg_np, truth_np, _ = planted_case(n, HIPS, seed=1, lag=0)
    msg, truth = dev(msg_np), dev(truth_np)
    acc = torch.full((1, 1, 46), -7.0, dtype=torch.float64, device="cuda")
    out = torch.full((n, 25), -7.0, dtype=torch.float64, device="cuda")
    st, body = np.zeros(1, dtype=np.int32), default_body()
    ptr = lambda t: C.c_void_p(t.data_ptr())                # noqa: E731

    def body_sums(stream):
        return lib.ape_body_sums(HIPS, ptr(msg), 25, _hip.F64, ptr(truth), _hip.TRUTH_EST, _hip.F64, n, C.c_void_p(st.ctypes.data), 1, 0,
                                 _hip.BODY_ROT_MSG, 0, 0, None, ptr(acc), stream)

    def rebody_rows(stream):
        return lib.ape_rebody_rows(HIPS, ptr(msg), 25, _hip.F64, n, C.c_void_p(st.ctypes.data), 1, C.c_void_p(body.ctypes.data), 1, ptr(out),
                                   _hip.F64, stream)

    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros((4,), device="cuda")
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            handle = C.c_void_p(side.cuda_stream)
            rc_s, msg_s = body_sums(handle), lib.ape_last_error()
            rc_r, msg_r = rebody_rows(handle), lib.ape_last_error()
    torch.cuda.current_stream().wait_stream(side)
    assert rc_s == 1 and b"capturing" in msg_s and b"body_sums" in msg_s, (rc_s, msg_s)
    assert rc_r == 1 and b"capturing" in msg_r and b"rebody_rows" in msg_r, (rc_r, msg_r)
    torch.cuda.synchronize()
    assert (acc == -7.0).all() and (out == -7.0).all()      # nothing was written
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert body_sums(stream) == 0 and rebody_rows(stream) == 0     # ... and the same arguments on a stream that is not capturing are taken
    torch.cuda.synchronize()
    assert not (acc == -7.0).any() and not (out == -7.0).any()
