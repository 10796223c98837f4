"""Scoring over a sweep of time lags (`ape_score_lags`) on the GPU.

References: for the per-frame rows `ape_score_rows` itself on gathered pair rows (message f, truth f - l) -- device against device, so
equality is of bits -- and `score.score_lags_numpy`; for the accumulators `score.accumulate_numpy` of the call's own per-frame rows over
the support.  Tolerances are those of tests/test_score_gpu.py, nothing new: columns 0-4 at 1e-13 absolute, the Mahalanobis columns at
1e-9 relative, sums within 16 n 2^-53 max(1, max term), counts and maxima exact.

The base case (tests/test_score_lags_cpu.py): F = 700 in six recordings, one of 3 frames (empty support), one boundary on a tile edge,
three inside a wave; skip 5, lags -5 .. 9, est-kind truth, the estimate of recording r late by PLANTED[r] frames exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_score_gpu import COUNTS, MAXIMA, TOL, check_acc, check_rows, dev, same
from tests.test_score_lags_cpu import F, HIPS, LAGS, PLANTED, POS, SKIP, STARTS, SUPPORTS, WATCH, msgs_from_est, planted_case, trajectory

pytestmark = pytest.mark.gpu

ENDS = STARTS[1:] + [F]
NL = LAGS[1] - LAGS[0] + 1


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def run_lags(layout, msg, truth, lags, kind="est", spread=None, per_frame=True, **kw):
    from wear_mocap_ape_amd import score
    t = lambda a: a if a is None or isinstance(a, torch.Tensor) else dev(a)               # noqa: E731
    s, a = score.score_lags(layout, t(msg), t(truth), lags, kind, t(spread), per_frame=per_frame, **kw)
    torch.cuda.synchronize()
    return (None if s is None else s.cpu().numpy()), a.cpu().numpy()


def run_rows(layout, msg, truth, kind="est", spread=None, **kw):
    from wear_mocap_ape_amd import score
    s, a = score.score_rows(layout, msg, truth, kind, spread, **kw)
    torch.cuda.synchronize()
    return (None if s is None else s.cpu().numpy()), a.cpu().numpy()


def support(s, e, skip, lo, hi):
    """[a, b): the frames of recording [s, e) with a pair at every lag of lo .. hi, past the skipped ones"""
    a, b = max(s + skip, s + hi), min(e, e + lo)
    return (a, b) if a < b else (s, s)


def check_sweep_acc(acc, rows, starts, skip, lags, what, rec_lags=None):
    """every acc[r, j] against numpy's accumulators of the call's own per-frame rows [F, L, 7] over the support"""
    ends = list(starts[1:]) + [rows.shape[0]]
    for r, (s, e) in enumerate(zip(starts, ends)):
        o = 0 if rec_lags is None else rec_lags[r]
        a, b = support(s, e, skip, o + lags[0], o + lags[1])
        for j in range(rows.shape[1]):
            if a == b:
                assert not acc[r, j].any(), (what, r, j)
            else:
                check_acc(acc[r, j][None], rows[a:b, j], [0], 0, (what, r, j))


@pytest.fixture(scope="module")
def base():
    """the base case on the device, its sweep (per-frame rows and accumulators, with the spread records) and numpy's"""
    from wear_mocap_ape_amd.score import score_lags_numpy
    msg, truth, rec = planted_case()
    d = {"msg": msg, "truth": truth, "rec": rec, "md": dev(msg), "td": dev(truth), "sd": dev(rec)}
    d["rows"], d["acc"] = run_lags(HIPS, d["md"], d["td"], LAGS, "est", d["sd"], starts=STARTS, skip=SKIP)
    d["np_rows"], d["np_acc"] = score_lags_numpy(msg, truth, HIPS, LAGS, STARTS, SKIP, rec)
    return d


# ---- 1, 2: the base case ----------------------------------------------------------------------------------------------------------------------
def test_base_per_frame_rows_are_score_rows_on_gathered_pairs(base):
    rows = base["rows"]
    assert rows.shape == (F, NL, 7)
    exists = np.zeros((F, NL), dtype=bool)
    for s, e in zip(STARTS, ENDS):
        for j in range(NL):
            l = LAGS[0] + j
            fs = np.arange(max(s, s + l), min(e, e + l))
            if fs.size == 0:
                continue
            exists[fs, j] = True
            ft = torch.as_tensor(fs, device="cuda")
            one, _ = run_rows(HIPS, base["md"][ft], base["td"][ft - l], "est", base["sd"][ft])
            assert same(rows[fs, j], one), (s, l)
    assert np.isnan(rows[~exists]).all() and np.isfinite(rows[exists]).all()
    assert exists[0:3].sum() == 3 + 2 * 2 + 2 * 1                       # the 3-frame recording: lags 0, +-1, +-2
    worst = check_rows(rows.reshape(-1, 7), base["np_rows"].reshape(-1, 7), "base rows")
    print(f"base case: max |device - numpy| columns 0-4 = {worst:.3e}")


def test_base_accumulators(base):
    from wear_mocap_ape_amd.score import best_lag
    acc = base["acc"]
    assert acc.shape == (6, NL, 25)
    check_sweep_acc(acc, base["rows"], STARTS, SKIP, LAGS, "base acc")
    assert np.array_equal(acc[:, :, COUNTS], base["np_acc"][:, :, COUNTS])
    assert np.array_equal(acc[:, :, 15], np.repeat(np.array(SUPPORTS, dtype=np.float64)[:, None], NL, axis=1)) and not acc[:, :, 16].any()
    # two calls give the same bits; the accumulators do not depend on the per-frame rows being written
    rows2, acc2 = run_lags(HIPS, base["md"], base["td"], LAGS, "est", base["sd"], starts=STARTS, skip=SKIP)
    assert same(base["rows"], rows2) and np.array_equal(acc, acc2)
    none, acc3 = run_lags(HIPS, base["md"], base["td"], LAGS, "est", base["sd"], starts=STARTS, skip=SKIP, per_frame=False)
    assert none is None and np.array_equal(acc, acc3)
    best = best_lag(acc, LAGS)
    assert best[0]["lag"] is None
    for r in range(1, 6):
        print(f"recording {r}: lag {best[r]['lag']}, hand rms {best[r]['rms']:.3e}, at lag 0 {best[r]['rms_lag0']:.3e}")
        assert best[r]["lag"] == PLANTED[r] and best[r]["rms"] <= 1e-13 and best[r]["scored"] == SUPPORTS[r], (r, best[r])


def test_half_frame_plant_refined_as_numpy_refines_it():
    from wear_mocap_ape_amd.score import best_lag, score_lags_numpy
    idx = np.arange(F)
    truth, msg = trajectory(idx), msgs_from_est(trajectory(idx - 3.4), HIPS)
    _, acc = run_lags(HIPS, msg, truth, LAGS, starts=STARTS, skip=SKIP, per_frame=False)
    _, ref = score_lags_numpy(msg, truth, HIPS, LAGS, STARTS, SKIP)
    got, want = best_lag(acc, LAGS), best_lag(ref, LAGS)
    for g, w in zip(got[1:], want[1:]):
        print(f"refined: device {g['refined']:.9f} numpy {w['refined']:.9f}")
        assert g["lag"] == w["lag"] == 3 and abs(g["refined"] - w["refined"]) <= 1e-6


# ---- 3: the sweep {0} is ape_score_rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [0, 5])
@pytest.mark.parametrize("spread", [False, True])
def test_sweep_zero_gives_the_bits_of_score_rows(base, golden, spread, skip):
    sd = base["sd"] if spread else None
    rows, acc = run_lags(HIPS, base["md"], base["td"], (0, 0), "est", sd, starts=STARTS, skip=skip)
    want_rows, want_acc = run_rows(HIPS, base["md"], base["td"], "est", sd, starts=STARTS, skip=skip)
    assert rows.shape == (F, 1, 7) and acc.shape == (6, 1, 25)
    assert same(rows[:, 0], want_rows) and np.array_equal(acc[:, 0], want_acc)
    # ... for NN targets through the truth FK too, ill-conditioned rows included, and over more than one workgroup per recording
    g = golden("fk_layout0.npz")
    msg = dev(np.tile(msgs_from_est(g["est_bo_N300"][::-1], HIPS), (3, 1)))
    preds = dev(np.tile(g["preds_bd_N300"], (3, 1)))
    kw = dict(starts=[0, 1, 257], skip=skip, bodies=g["body_bd"])
    rows, acc = run_lags(HIPS, msg, preds, (0, 0), "targets", **kw)
    want_rows, want_acc = run_rows(HIPS, msg, preds, "targets", **kw)
    assert same(rows[:, 0], want_rows) and np.array_equal(acc[:, 0], want_acc)
    assert np.array_equal(run_lags(HIPS, msg, preds, (0, 0), "targets", per_frame=False, **kw)[1][:, 0], want_acc)


# ---- 4: offsets ---------------------------------------------------------------------------------------------------------------------------------
def test_offsets_shift_the_sweep_per_recording(base):
    from wear_mocap_ape_amd import score
    off = [0, 2, -3, 7, 0, 1]
    rows, acc = run_lags(HIPS, base["md"], base["td"], (-2, 2), "est", base["sd"], starts=STARTS, skip=SKIP, rec_lags=off)
    assert rows.shape == (F, 5, 7)
    for r, (s, e) in enumerate(zip(STARTS, ENDS)):
        assert same(rows[s:e], base["rows"][s:e, off[r] + 3:off[r] + 8]), r            # lag off - 2 + j is index off + 3 + j of -5 .. 9
    check_sweep_acc(acc, rows, STARTS, SKIP, (-2, 2), "offsets", off)
    best, arows, aacc = score.align(HIPS, base["md"], base["td"], LAGS, truth_kind="est", spread=base["sd"], starts=STARTS, skip=SKIP)
    torch.cuda.synchronize()
    arows, aacc = arows.cpu().numpy(), aacc.cpu().numpy()
    assert [b["lag"] for b in best] == [None] + PLANTED[1:]
    assert arows.shape == (F, 7) and aacc.shape == (6, 25)
    for r, (s, e) in enumerate(zip(STARTS, ENDS)):
        lag = 0 if r == 0 else PLANTED[r]
        assert same(arows[s:e], base["rows"][s:e, lag - LAGS[0]]), r
        a, b = support(s, e, SKIP, lag, lag)
        check_acc(aacc[r][None], arows[a:b], [0], 0, ("align", r))
    assert aacc[1:, 0].max() <= 1e-13 * F                               # the hand error summed over a recording at its own lag


# ---- 5: gaps -------------------------------------------------------------------------------------------------------------------------------------
def test_gaps_move_with_the_lag_and_the_support_stays(base):
    from wear_mocap_ape_amd.score import score_lags_numpy
    msg, truth = base["msg"].copy(), base["truth"].copy()
    truth[[20, 90, 91, 280, 500], [0, 4, 10, 14, 18]] = np.nan
    msg[[40, 130, 600], [5, 0, 24]] = np.nan
    rows, acc = run_lags(HIPS, msg, truth, LAGS, "est", base["rec"], starts=STARTS, skip=SKIP)
    ref_rows, ref_acc = score_lags_numpy(msg, truth, HIPS, LAGS, STARTS, SKIP, base["rec"])
    check_rows(rows.reshape(-1, 7), ref_rows.reshape(-1, 7), "gaps")
    assert np.array_equal(acc[:, :, [15, 16]], ref_acc[:, :, [15, 16]])
    assert np.array_equal(acc[:, :, 15] + acc[:, :, 16], np.repeat(np.array(SUPPORTS, dtype=np.float64)[:, None], NL, axis=1))
    assert (acc[1, :, 16] == 2).all() and (acc[2, :, 16] == 3).all() and (acc[3, :, 16] == 1).all() and (acc[4, :, 16] == 2).all()
    for j in range(NL):                                                 # truth row 90 meets frame 90 + l
        l = LAGS[0] + j
        assert np.isnan(rows[90 + l, j]).all() and np.isfinite(rows[89 + l, j]).all() and np.isnan(rows[130, j]).all()
    check_sweep_acc(acc, rows, STARTS, SKIP, LAGS, "gaps acc")


# ---- 6: spans and edges --------------------------------------------------------------------------------------------------------------------------
def test_wide_sweep_single_frame_and_the_largest_lags():
    from wear_mocap_ape_amd.score import score_lags_numpy
    msg, truth, rec = planted_case(planted=[7], starts=[0], n=300)
    md, td, sd = dev(msg), dev(truth), dev(rec)
    rows, acc = run_lags(HIPS, md, td, (-32, 32), "est", sd, skip=3)
    ref_rows, ref_acc = score_lags_numpy(msg, truth, HIPS, (-32, 32), None, 3, rec)
    check_rows(rows.reshape(-1, 7), ref_rows.reshape(-1, 7), "65 lags")
    check_sweep_acc(acc, rows, [0], 3, (-32, 32), "65 lags")
    assert (acc[0, :, 15] == 300 - 64).all() and np.array_equal(acc[0, :, COUNTS], ref_acc[0, :, COUNTS])
    assert int(np.argmin(acc[0, :, 1])) == 7 + 32 and acc[0, 39, 1] <= 1e-26 * 300
    # one frame: only lag 0 has a pair
    r1, a1 = run_lags(HIPS, md[:1], td[:1], (-1, 1), "est", sd[:1])
    assert np.isnan(r1[0, [0, 2]]).all() and same(r1[0, 1][None], run_rows(HIPS, md[:1], td[:1], "est", sd[:1])[0]) and not a1.any()
    r1, a1 = run_lags(HIPS, md[:1], td[:1], (0, 0), "est", sd[:1])
    assert a1[0, 0, 15] == 1 and np.isfinite(r1).all()
    # L = 1 at the two largest lags: 172 pairs, the halo of the second workgroup reaches back into the first and the other way round
    for lag in (128, -128):
        rows, acc = run_lags(HIPS, md, td, (lag, lag), "est", sd)
        fs = np.arange(max(0, lag), min(300, 300 + lag))
        ft = torch.as_tensor(fs, device="cuda")
        one, one_acc = run_rows(HIPS, md[ft], td[ft - lag], "est", sd[ft])
        assert fs.size == 172 and same(rows[fs, 0], one) and np.isnan(np.delete(rows[:, 0], fs, axis=0)).all()
        assert np.array_equal(acc[0, 0, COUNTS + MAXIMA], one_acc[0, COUNTS + MAXIMA]) and acc[0, 0, 15] == 172
        check_sweep_acc(acc, rows, [0], 0, (lag, lag), lag)


def test_many_recordings_over_many_workgroups():
    """F = 20 000 in 40 recordings of seeded random lengths at lags -8 .. 8, gaps included: a sample of 2 000 frames against numpy, every
    accumulator against numpy's of the call's own rows, the counts against numpy's own"""
    from wear_mocap_ape_amd.score import score_lags_numpy
    rng = np.random.default_rng(61)
    n, lags, skip = 20000, (-8, 8), 4
    starts = [0] + sorted(int(v) for v in rng.choice(np.arange(1, n), 39, replace=False))
    starts[1], starts[2] = 5, 5 + 16                                    # recordings of 5 and of 16 frames: both supports are empty
    assert starts[3] > starts[2]
    planted = [int(v) for v in rng.integers(-6, 7, size=40)]
    msg, truth, rec = planted_case(planted=planted, starts=starts, n=n, seed=7)
    truth[rng.choice(n, 60, replace=False), 2] = np.nan
    msg[rng.choice(n, 30, replace=False), 12] = np.nan
    md, td, sd = dev(msg), dev(truth), dev(rec)
    rows, acc = run_lags(HIPS, md, td, lags, "est", sd, starts=starts, skip=skip)
    ref_rows, ref_acc = score_lags_numpy(msg, truth, HIPS, lags, starts, skip, rec)
    pick = np.sort(rng.choice(n, 2000, replace=False))
    check_rows(rows[pick].reshape(-1, 7), ref_rows[pick].reshape(-1, 7), "sample")
    assert np.array_equal(np.isnan(rows[:, :, 0]), np.isnan(ref_rows[:, :, 0]))
    check_sweep_acc(acc, rows, starts, skip, lags, "many")
    assert np.array_equal(acc[:, :, COUNTS], ref_acc[:, :, COUNTS])
    assert not acc[0].any() and not acc[1].any() and (acc[:, :, 15] + acc[:, :, 16] == (acc[:, :1, 15] + acc[:, :1, 16])).all()
    rows2, acc2 = run_lags(HIPS, md, td, lags, "est", sd, starts=starts, skip=skip)
    assert same(rows, rows2) and np.array_equal(acc, acc2)
    assert np.array_equal(run_lags(HIPS, md, td, lags, "est", sd, starts=starts, skip=skip, per_frame=False)[1], acc)


# ---- 7: dtypes and views -------------------------------------------------------------------------------------------------------------------------
def test_dtypes_and_strided_views(base):
    from wear_mocap_ape_amd.score import score_lags_numpy
    lags = (-3, 4)
    m32, s32, t32 = dev(base["msg"], torch.float32), dev(base["rec"], torch.float32), dev(base["truth"], torch.float32)
    up = lambda t: t.cpu().numpy().astype(np.float64)                   # noqa: E731
    for md, sd, td in ((m32, s32, t32), (m32, s32, base["td"]), (base["md"], base["sd"], t32)):
        rows, acc = run_lags(HIPS, md, td, lags, "est", sd, starts=STARTS, skip=SKIP)
        ref_rows, _ = score_lags_numpy(up(md), up(td), HIPS, lags, STARTS, SKIP, up(sd))
        check_rows(rows.reshape(-1, 7), ref_rows.reshape(-1, 7), (md.dtype, td.dtype))
        check_sweep_acc(acc, rows, STARTS, SKIP, lags, (md.dtype, td.dtype))
    # packed float32 rows [F, 25 + 6 * 25 + 21] with NaN between message and record go in as two views
    rows, acc = run_lags(HIPS, m32, t32, lags, "est", s32, starts=STARTS, skip=SKIP)
    wide = torch.full((F, 196), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :25], wide[:, -21:] = m32, s32
    assert not wide[:, :-21].is_contiguous()
    rows_w, acc_w = run_lags(HIPS, wide[:, :-21], t32, lags, "est", wide[:, -21:], starts=STARTS, skip=SKIP)
    assert same(rows, rows_w) and np.array_equal(acc, acc_w)
    # float32 output: the float64 row rounded once
    rows32, acc32 = run_lags(HIPS, m32, t32, lags, "est", s32, starts=STARTS, skip=SKIP, out_dtype=torch.float32)
    assert rows32.dtype == np.float32 and same(rows32, rows.astype(np.float32)) and np.array_equal(acc32, acc)


# ---- 8: NN targets as truth, one body per recording -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_targets_truth_equals_est_truth_at_every_lag(golden, layout):
    g = golden(f"fk_layout{layout}.npz")
    starts, lags = [0, 1, 257], (-3, 3)
    cut = lambda a, b: np.concatenate([a[0:1], b[1:257], a[257:]])      # noqa: E731
    preds, est = cut(g["preds_bd_N300"], g["preds_bo_N300"]), cut(g["est_bd_N300"], g["est_bo_N300"])
    bodies = np.concatenate([g["body_bd"].reshape(1, 9), g["body_bo"].reshape(1, 9), g["body_bd"].reshape(1, 9)])
    msg = msgs_from_est(g["est_bo_N300"][np.random.default_rng(0).permutation(300)], layout)
    a, acc_a = run_lags(layout, msg, preds, lags, "targets", starts=starts, bodies=bodies)
    b, acc_b = run_lags(layout, msg, est, lags, "est", starts=starts)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.isnan(a[0, [0, 1, 2, 4, 5, 6]]).all() and np.isfinite(a[0, 3, :5]).all()
    ok = np.isfinite(b[:, :, 0])
    d = np.abs(a[ok][:, :5] - b[ok][:, :5])
    print(f"targets vs est truth over lags -3 .. 3, layout {layout}: max {d.max():.3e}")
    assert d.max() <= TOL and np.array_equal(acc_a[:, :, COUNTS], acc_b[:, :, COUNTS])
    # the body is the truth row's recording's: one body for all gives other rows in the recording with the other body
    c, _ = run_lags(layout, msg, preds, lags, "targets", starts=starts, bodies=g["body_bd"])
    if layout != POS:                                                   # (positions are targets there: the body is not used)
        assert same(a[257:], c[257:]) and not same(a[1:257], c[1:257])


# ---- 9: plumbing -----------------------------------------------------------------------------------------------------------------------------------
def _plumbing(est_obj, out, rec, starts, truth, skip):
    from wear_mocap_ape_amd import score
    host = lambda pair: tuple(x.cpu().numpy() for x in pair)            # noqa: E731
    td = dev(truth)
    got = host(est_obj.score_recording(out, td, spread=rec, starts=starts, lags=(-2, 3), rec_lags=[1, 0, -1]))
    want = host(score.score_lags(est_obj._layout, out, td, (-2, 3), "targets", rec, starts, skip, est_obj.body_measurements, [1, 0, -1],
                                 per_frame=True))
    assert got[0].shape == (out.shape[0], 6, 7) and same(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.isfinite(got[0][:, :, 0]).sum() > out.shape[0] * 3 and got[1][:, :, 15].max() > 0
    today = host(est_obj.score_recording(out, td, spread=rec, starts=starts))
    rows = host(score.score_rows(est_obj._layout, out, td, "targets", rec, starts, skip, est_obj.body_measurements))
    assert same(today[0], rows[0]) and np.array_equal(today[1], rows[1])
    zero = host(est_obj.score_recording(out, td, spread=rec, starts=starts, lags=(0, 0)))
    assert same(zero[0][:, 0], today[0]) and np.array_equal(zero[1][:, 0], today[1])
    with pytest.raises(UserWarning):
        est_obj.score_recording(out, td, spread=rec, starts=starts, rec_lags=[1, 0, -1])


def test_score_recording_takes_lags_pocket_nn(golden, tmp_path, monkeypatch):
    from tests.test_replay import _estimator
    from tests.test_score_gpu import _truth_for
    est_obj = _estimator(tmp_path, monkeypatch, "pocket", 1, 0.2, smooth=1, add_mc_samples=True, monte_carlo_samples=25)
    rows = np.tile(golden("stream_trace_pocket.npz")["rows"].astype(np.float32), (3, 1))
    starts = [0, 20, 40]
    out, rec = est_obj.process_recording(rows, starts=starts, seed=5, spread=True)
    truth_t, _ = _truth_for(golden, HIPS, 60, np.random.default_rng(51))
    _plumbing(est_obj, out, rec, starts, truth_t, est_obj.sequence_len - 1)


def test_score_recording_takes_lags_fk_only(golden):
    from tests.test_score_gpu import _truth_for
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    est_obj = WatchPhoneUarm(smooth=5)
    rows = np.tile(golden("stream_trace_uarm.npz")["rows"].astype(np.float32), (3, 1))[:60]
    starts = [0, 20, 40]
    out = est_obj.process_recording(rows, starts=starts)
    truth_t, _ = _truth_for(golden, WATCH, 60, np.random.default_rng(52))
    _plumbing(est_obj, out, None, starts, truth_t, 0)


def test_score_recording_takes_lags_kalman(golden):
    from oracle import kalman_oracle as ko
    from tests.test_kalman_bank_gpu import _estimator, make_rows
    from tests.test_score_gpu import _truth_for
    E, W, smooth = 16, 4, 2
    est_obj = _estimator(ko.make_state_dict(W, 36), E, W, smooth=smooth)
    rows = make_rows(np.random.default_rng(36), 60)
    starts = [0, 20, 40]
    out, _, rec = est_obj.process_recording(rows, starts=starts, seed=4242, spread=True)
    truth_t, _ = _truth_for(golden, HIPS, 60, np.random.default_rng(53))
    _plumbing(est_obj, out, rec, starts, truth_t, W + 1)


# ---- 10: refusals: made on the host, nothing written ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    n = 10
    msg = torch.zeros((n, 25), dtype=torch.float64, device="cuda")
    rec = torch.zeros((n, 21), dtype=torch.float64, device="cuda")
    truth = torch.zeros((n, 21), dtype=torch.float64, device="cuda")
    score = torch.full((n, 5, 7), -7.0, dtype=torch.float64, device="cuda")
    acc = torch.full((3, 5, 25), -7.0, dtype=torch.float64, device="cuda")
    body = np.zeros((3, 9))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(layout=0, m=msg, ms=25, s=rec, ss=21, md=_hip.F64, t=truth, kind=1, td=_hip.F64, F=n, starts=(0, 3, 7), skip=0, bodies=body,
             nb=1, lo=-2, hi=2, offs=None, sc=score, sd=_hip.F64, ac=acc, R=None):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        of = None if offs is None else np.ascontiguousarray(offs, dtype=np.int32)
        return lib.ape_score_lags(layout, p(m), ms, p(s), ss, md, p(t), kind, td, F, C.c_void_p(st.ctypes.data) if len(st) else None,
                                  len(st) if R is None else R, skip, C.c_void_p(bodies.ctypes.data) if bodies is not None else None, nb,
                                  lo, hi, None if of is None else C.c_void_p(of.ctypes.data), p(sc), sd, p(ac), stream)

    bad = [dict(m=None), dict(t=None), dict(sc=None, ac=None), dict(F=0), dict(starts=()), dict(starts=(1, 3)), dict(starts=(0, 5, 5)),
           dict(starts=(0, 10)), dict(starts=(0, 7, 3)), dict(ms=24), dict(ss=20), dict(skip=-1), dict(nb=2), dict(nb=0), dict(bodies=None),
           dict(layout=_hip.LAYOUT_NONE), dict(layout=3), dict(kind=2), dict(kind=-1), dict(md=2), dict(td=2), dict(sd=2),
           dict(R=0), dict(R=-1), dict(R=11),
           dict(lo=1, hi=0), dict(lo=0, hi=65), dict(lo=-2 ** 31, hi=2 ** 31 - 1), dict(lo=129, hi=129), dict(lo=-129, hi=-128),
           dict(offs=(0, 127, 0)), dict(offs=(0, 0, -127)), dict(offs=(2 ** 31 - 1, 0, 0)), dict(lo=0, hi=0, offs=(-129, 0, 0))]
    for kw in bad:
        assert call(**kw) == 1, kw                          # APE_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (score == -7.0).all() and (acc == -7.0).all()
    assert call() == 0 and call(offs=(0, 126, -126)) == 0   # ... and the same arguments without the fault are taken
    torch.cuda.synchronize()
    assert not (score == -7.0).any() and not (acc == -7.0).any()
