"""Each recording's heading and frame offset against the truth (`ape_frame_sums`, `ape_rotate_rows`) on the GPU.

References: `score.frame_sums_numpy` and `score.rotate_rows_numpy` (tests/test_frame_fit_cpu.py holds them to hand-written numpy).
Tolerances: every sum within 16 n 2^-53 max(1, max |term|) of the statement, n the pairs summed -- the rule tests/test_score_gpu.py
uses for sums -- and the two counts exact; a rotated float64 row within 1e-14 (about 30 float64 operations on values below 2), a
float32 one within one float32 ulp of the statement rounded to float32."""
import numpy as np
import pytest
import torch

from tests.test_frame_fit_cpu import (HIPS, POS, WATCH, general_quat, msgs_from_est, planted, spread_for, turn_est, walk_est,
                                      yaw_quat)
from tests.test_score_gpu import dev

pytestmark = pytest.mark.gpu

F = 1000
STARTS, LAGS, REC_LAGS, SKIP = [0, 37, 300, 301, 900], (-5, 7), [0, 2, -3, 0, 1], 2       # [300, 301): one frame, no support; [0, 37): 25
WIDE = 25 + 6 * 4 + 21                                                                    # frames of support.  A packed spread-flagged row


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def sums(layout, msg, truth, lags, kind="est", **kw):
    from wear_mocap_ape_amd import score
    t = lambda a: a if isinstance(a, torch.Tensor) else dev(a)                           # noqa: E731
    acc = score.frame_sums(layout, t(msg), t(truth), lags, kind, **kw)
    torch.cuda.synchronize()
    return acc.cpu().numpy()


def term_bound(msg, truth_est, layout):
    """max(1, the largest |term| any pair of these rows can contribute): rotation entries are <= 1, position terms <= the largest
    squared norm"""
    m, t = np.asarray(msg, dtype=np.float64), np.asarray(truth_est, dtype=np.float64)
    pos = np.concatenate([m[:, 4:7], m[:, 11:14], t[:, 0:3], t[:, 3:6]])
    pos = pos[np.isfinite(pos).all(axis=1)]
    return max(1.0, float((pos * pos).sum(axis=1).max(initial=0.0)))


def check_sums(got, ref, bound, what):
    """-> the largest deviation in units of the allowance"""
    assert got.shape == ref.shape, what
    assert np.array_equal(got[..., 49:], ref[..., 49:]), (what, got[..., 49:], ref[..., 49:])
    allow = 16.0 * np.maximum(ref[..., 49:50], 1.0) * 2.0 ** -53 * bound
    d = np.abs(got[..., :49] - ref[..., :49])
    assert (d <= allow).all(), (what, float((d / allow).max()))
    assert not got[ref[..., 49] == 0][..., :49].any(), what                              # nothing summed: exact zeros
    return float((d / allow).max())


# ---- 1: against the statement --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case1(golden):
    """per layout: messages, NN targets, the est rows the reference's FK makes of them (fixtures), and the statement's sums for float64 and
    for float32 messages -- computed once"""
    from wear_mocap_ape_amd.score import frame_sums_numpy
    cache = {}

    def get(layout):
        if layout not in cache:
            g = golden(f"fk_layout{layout}.npz")
            pick = np.random.default_rng(11 + layout).integers(0, 300, size=F)
            msg = msgs_from_est(walk_est(F, WATCH if layout == WATCH else HIPS, seed=21 + layout), layout)
            d = {"msg": msg, "preds": g["preds_bd_N300"][pick], "est": g["est_bd_N300"][pick], "body": g["body_bd"]}
            for name, m in (("f64", msg), ("f32", msg.astype(np.float32).astype(np.float64))):
                d[name] = frame_sums_numpy(m, d["est"], layout, LAGS, STARTS, SKIP, REC_LAGS)
            d["bound"] = term_bound(msg, d["est"], layout)
            cache[layout] = d
        return cache[layout]
    return get


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["est", "targets"])
@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_sums_against_the_statement(case1, layout, kind, dtype, strided):
    d = case1(layout)
    md = dev(d["msg"], dtype)
    if strided:                                             # packed spread-flagged rows: NaN between and behind the message
        wide = torch.full((F, WIDE), float("nan"), dtype=dtype, device="cuda")
        wide[:, :25] = md
        md = wide[:, :25]
        assert not md.is_contiguous() and md.stride(0) == WIDE
    truth = d["est"] if kind == "est" else d["preds"]
    got = sums(layout, md, truth, LAGS, kind, starts=STARTS, skip=SKIP, rec_lags=REC_LAGS, bodies=d["body"])
    ref = d["f64" if dtype == torch.float64 else "f32"]
    assert got.shape == (5, 13, 51)
    worst = check_sums(got, ref, d["bound"], (layout, kind, dtype, strided))
    print(f"layout {layout} {kind} {dtype} strided={strided}: worst deviation {worst:.3f} of the allowance")
    assert not got[2].any() and all(got[r].any() for r in (0, 1, 3, 4))                  # the one-frame recording has no support
    assert (got[:, :, 49] + got[:, :, 50] == (got[:, :1, 49] + got[:, :1, 50])).all()
    if layout == WATCH:
        assert not got[:, :, 18:27].any()
    else:
        assert got[:, :, 18:27].any()


# ---- 2: edges ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_edges_of_waves_and_tiles(n):
    from wear_mocap_ape_amd.score import frame_sums_numpy
    msg, truth = planted(yaw_quat(0.3), lag=1, n=n, seed=n)
    bound = term_bound(msg, truth, HIPS)
    cuts = [[0], [0, 64], [0, 63], [0, 65], [0, 256], [0, 255], [0, 257], [0, 63, 64, 65, 255, 256, 257], [0, 64, 128, 192, 256, 320]]
    for starts in cuts:
        starts = [s for s in starts if s < n]
        for lags, skip in (((0, 0), 0), ((-1, 2), 1)):
            got = sums(HIPS, msg, truth, lags, starts=starts, skip=skip)
            check_sums(got, frame_sums_numpy(msg, truth, HIPS, lags, starts, skip), bound, (n, starts, lags))


# ---- 3: unusable input ---------------------------------------------------------------------------------------------------------------------------
def test_unusable_pairs_move_between_the_two_counts():
    from wear_mocap_ape_amd.score import frame_sums_numpy
    msg, truth = planted(general_quat(), lag=0, n=12, seed=5)
    lags = (-2, 2)
    clean = sums(HIPS, msg, truth, lags)
    assert (clean[0, :, 49] == 8).all() and not clean[0, :, 50].any()
    truth[9, 6] = np.nan                                    # the est shoulder origin: not read
    assert np.array_equal(sums(HIPS, msg, truth, lags), clean)
    msg[4, 9], truth[6, 1], truth[8, 13:17] = np.nan, np.inf, 0.0
    got = sums(HIPS, msg, truth, lags)
    ref = frame_sums_numpy(msg, truth, HIPS, lags)
    check_sums(got, ref, term_bound(msg, truth, HIPS), "unusable")
    # the support is frames 2 .. 9: frame 4 is lost at every lag, truth rows 6 and 8 meet frames 6 + l and 8 + l
    lost = [1 + sum(2 <= r + l <= 9 and r + l != 4 for r in (6, 8)) for l in range(-2, 3)]
    assert got[0, :, 50].tolist() == lost and (got[0, :, 49] + got[0, :, 50] == 8).all()


# ---- 4: determinism -------------------------------------------------------------------------------------------------------------------------------
def test_same_inputs_same_bits(case1):
    from wear_mocap_ape_amd import score
    d = case1(HIPS)
    md, td = dev(d["msg"]), dev(d["preds"])
    kw = dict(starts=STARTS, skip=SKIP, rec_lags=REC_LAGS, bodies=d["body"])
    a = sums(HIPS, md, td, LAGS, "targets", **kw)
    b = sums(HIPS, md, td, LAGS, "targets", **kw)
    score.score_lags(HIPS, md, td, (-8, 8), "targets", starts=STARTS, bodies=d["body"])
    c = sums(HIPS, md, td, LAGS, "targets", **kw)
    assert np.array_equal(a, b) and np.array_equal(a, c)


# ---- 5: rotate_rows --------------------------------------------------------------------------------------------------------------------------------
def rotate(layout, msg, quats, spread=None, **kw):
    from wear_mocap_ape_amd import score
    res = score.rotate_rows(layout, msg, quats, spread, **kw)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in res) if isinstance(res, tuple) else res.cpu().numpy()


def test_rotate_rows_against_its_statement():
    from wear_mocap_ape_amd.score import rotate_rows_numpy
    n, starts = 300, [0, 64, 65, 257]
    rng = np.random.default_rng(9)
    msg = msgs_from_est(walk_est(n, WATCH, seed=6), WATCH)  # the no-hips message: identity hips, the constant shoulder origin
    msg[:, 0:4] = rng.uniform(-1.0, 1.0, size=(n, 4))
    rec = spread_for(msg)
    msg[[10, 64, 299], [5, 22, 0]] = np.nan
    rec[[20, 64], [4, 10]] = np.nan
    gs = np.stack([general_quat(), yaw_quat(-0.7), np.array([0.1, -0.8, 0.3, 0.5]), np.array([-2.0, 0.0, 0.0, 1.0])])
    assert np.nanmax(np.abs(msg)) < 2 and np.nanmax(np.abs(rec)) < 2
    for quats, st in ((gs, starts), (gs[2], starts), (gs[0], None)):
        want, want_rec = rotate_rows_numpy(msg, quats, rec, st)
        got, got_rec = rotate(WATCH, dev(msg), quats, dev(rec), starts=st)
        assert got.shape == (n, 25) and got_rec.shape == (n, 21)
        for g_, w_ in ((got, want), (got_rec, want_rec)):
            assert np.array_equal(np.isnan(g_), np.isnan(w_))
            assert np.nanmax(np.abs(g_ - w_)) <= 1e-14
        # NaN stays where the statement puts it: row 10 loses its hand origin only, its neighbours nothing
        assert np.isnan(got[10, 4:7]).all() and np.isfinite(got[10, 7:]).all() and np.isfinite(got[[9, 11]]).all()
        assert np.isnan(got[64, 21:25]).all() and np.isfinite(got[63]).all() and np.isfinite(got[65]).all()
        assert np.isnan(got_rec[20, 3:9]).all() and np.isfinite(got_rec[20, 9:]).all() and np.isfinite(got_rec[[19, 21]]).all()
        plain = rotate(WATCH, dev(msg), quats, starts=st)
        assert np.array_equal(plain, got, equal_nan=True)
    # the constant columns of the no-hips message are turned like the rest
    want = rotate_rows_numpy(msg, gs, None, starts)
    assert np.abs(want[0, 21:25] - gs[0]).max() <= 1e-15 and np.abs(want[1, 18:21] - msg[1, 18:21]).max() > 0.01
    # float32 storage: float64 arithmetic, rounded once; strided packed rows in, nothing past column 24 read
    m32, r32 = msg.astype(np.float32), rec.astype(np.float32)
    wide = torch.full((n, WIDE), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :25], wide[:, -21:] = dev(m32), dev(r32)
    want, want_rec = rotate_rows_numpy(m32.astype(np.float64), gs, r32.astype(np.float64), starts)
    for out_dtype, npdt in ((None, np.float32), (torch.float32, np.float32), (torch.float64, np.float64)):
        got, got_rec = rotate(WATCH, wide[:, :25], gs, wide[:, -21:], starts=starts, out_dtype=out_dtype)
        assert got.dtype == npdt
        for g_, w_ in ((got, want), (got_rec, want_rec)):
            assert np.array_equal(np.isnan(g_), np.isnan(w_))
            if npdt == np.float32:
                w32 = w_.astype(np.float32)
                ok = np.isfinite(w32)
                assert (np.abs(g_[ok] - w32[ok]) <= np.spacing(np.abs(w32[ok]))).all()
            else:
                assert np.nanmax(np.abs(g_ - w_)) <= 1e-14
    for bad in (np.zeros(4), np.ones((2, 4))):
        with pytest.raises(UserWarning):
            rotate(WATCH, dev(msg), bad, starts=starts)


# ---- 6: end to end on a replay ------------------------------------------------------------------------------------------------------------------------
def test_align_recording_removes_planted_lag_and_yaw():
    from tests.test_fk_only_gpu import _random_rows
    from wear_mocap_ape_amd import score
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    est_obj = WatchPhoneUarm(smooth=1)
    starts, ends, yaws, adv = [0, 400], [400, 1000], [0.3, -0.2], [3, 0]
    out = est_obj.process_recording(_random_rows(np.random.default_rng(17), 1000), starts=starts)
    rows = out.cpu().numpy()
    assert np.isfinite(rows).all()
    est = np.concatenate([rows[:, 4:7], rows[:, 11:14], rows[:, 7:11], rows[:, 14:18]], axis=1)
    truth = np.empty_like(est)
    for s, e, psi, k in zip(starts, ends, yaws, adv):
        idx = np.clip(np.arange(s, e) + k, s, e - 1)        # truth row f states frame f + k: the estimate is late by k
        truth[s:e] = turn_est(est[idx], yaw_quat(psi), WATCH)
    td = dev(truth)
    _, acc0 = est_obj.score_recording(out, td, starts=starts, truth_kind="est")
    sc, acc, found = est_obj.align_recording(out, td, starts=starts, truth_kind="est", lags=(-8, 8))
    torch.cuda.synchronize()
    before, after = score.summarise(acc0), score.summarise(acc)
    for r in range(2):
        print(f"recording {r}: lag {found[r]['lag']}, yaw {found[r]['yaw']:.12f}, mean errors before {before[r]['mean']}, after {after[r]['mean']}")
        assert found[r]["lag"] == adv[r] and abs(found[r]["yaw"] - yaws[r]) <= 1e-9
        assert before[r]["mean"]["uarm_rot"] > 0.1
        assert all(v <= 1e-9 for v in after[r]["mean"].values()), after[r]["mean"]
        assert after[r]["scored"] == ends[r] - starts[r] - adv[r]
        assert abs(found[r]["mean_cos_after"]["uarm"] - 1.0) <= 1e-9 and found[r]["mean_cos_before"]["uarm"] < 0.999
    assert tuple(sc.shape) == (1000, 7) and tuple(acc.shape) == (2, 25)
    # the pieces: align_frame is frame_sums -> best_frame -> rotate_rows -> score_lags
    sums_ = score.frame_sums(WATCH, out, td, (-8, 8), "est", starts)
    again = score.best_frame(sums_, (-8, 8))
    assert [b["lag"] for b in again] == adv and all(np.array_equal(a["quat"], b["quat"]) for a, b in zip(again, found))


# ---- 7: a Monte-Carlo replay: the coverage counts do not see the turn -------------------------------------------------------------------------------
def test_coverage_counts_survive_the_turn(golden, tmp_path, monkeypatch):
    from tests.test_replay import _estimator
    from wear_mocap_ape_amd import score
    est_obj = _estimator(tmp_path, monkeypatch, "pocket", 1, 0.2, smooth=2, add_mc_samples=True, monte_carlo_samples=4)
    rows = np.tile(golden("stream_trace_pocket.npz")["rows"].astype(np.float32), (10, 1))[:200]
    assert rows.shape[0] == 200
    out, rec = est_obj.process_recording(rows, seed=5, spread=True)
    m = out.cpu().numpy()
    est = np.concatenate([m[:, 4:7], m[:, 11:14], m[:, 18:21], m[:, 7:11], m[:, 14:18], m[:, 21:25]], axis=1)
    s0, acc0 = est_obj.score_recording(out, dev(est), spread=rec, truth_kind="est")
    torch.cuda.synchronize()
    s0, acc0 = s0.cpu().numpy(), acc0.cpu().numpy()
    d2 = s0[est_obj.sequence_len - 1:, 5:7]
    d2 = d2[np.isfinite(d2)]
    assert d2.size > 100, "the replay has usable covariances"
    for q in (score.CHI2_3_Q50, score.CHI2_3_Q90):
        assert np.abs(d2 - q).min() > 1e-6, "a frame sits on a coverage threshold: choose another seed"
    _, acc, found = est_obj.align_recording(out, dev(turn_est(est, yaw_quat(0.3), HIPS)), spread=rec, truth_kind="est")
    acc = acc.cpu().numpy()
    counts = [17, 19, 20, 21, 23, 24]
    print("coverage counts", acc0[0, counts], "yaw", found[0]["yaw"])
    assert found[0]["lag"] == 0 and abs(found[0]["yaw"] - 0.3) <= 1e-9
    assert np.array_equal(acc[:, counts], acc0[:, counts]) and acc0[0, 17] > 0 and acc0[0, 21] > 0
    assert np.array_equal(acc[:, 15:17], acc0[:, 15:17])
    assert np.abs(acc[0, [18, 22]] - acc0[0, [18, 22]]).max() <= 1e-9 * acc0[0, [18, 22]].max()
