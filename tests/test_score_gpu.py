"""Scoring against ground truth (`ape_score_rows`) on the GPU.

Reference of every per-frame value: `score.score_rows_numpy` (plain numpy) on the same inputs; of the accumulators:
`score.accumulate_numpy` of the call's own per-frame rows.

Tolerances, as the feature's issue states them: columns 0-4 at 1e-13 absolute (100 x the float64 post-filter parity of 1e-15: the norm
and the asin amplify by <= 6); the Mahalanobis columns at 1e-9 relative for covariances of condition number <= 1e3 (kappa 2^-53 times
~100 operations is 1e-11); sums within 16 n 2^-53 max(1, max term); counts and maxima exact.

Truth given as NN targets is compared with the REFERENCE's forward kinematics (the oracle's "eigh" route, which wrote the fixtures'
`est_*_N300`): the fixtures' rows 7-26 carry 6D rotations whose two columns are nearly parallel, Gram-Schmidt leaves their matrices 1e-11
off orthonormal, and there the closed form of fk_device.h alone is up to 3.7e-12 from the reference's eigenvector -- the two truth kinds
then differed by up to 1.0e-11 in columns 0-4 on 25-31 of the 300 rows (measured on an MI355X and in numpy alike).  The truth FK
therefore refines the closed form to that eigenvector (csrc/score.hip, truth_six_drr_to_quat)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc

pytestmark = pytest.mark.gpu

HIPS, WATCH, POS = 0, 1, 2
TOL = 1e-13


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def msgs_from_est(est, layout):
    """one message per est row stating that row's pose (compose_msg.py:72-78 columns)"""
    qc = (6, 10) if layout == WATCH else (9, 13, 17)
    m = np.zeros((est.shape[0], 25))
    m[:, 21] = 1.0
    m[:, 4:7], m[:, 11:14] = est[:, 0:3], est[:, 3:6]
    if layout != WATCH:
        m[:, 18:21] = est[:, 6:9]
    for k, c in enumerate(qc):
        m[:, 7 + 7 * k:11 + 7 * k] = est[:, c:c + 4]
    m[:, 0:4] = m[:, 7:11]
    return m


def spread_records(rng, msg, F, n=8, scale=0.05):
    """records whose means sit near the message's origins and whose covariances are A A' / n with condition number <= 1e3"""
    rec = np.zeros((F, 21))
    for o, c in ((0, 4), (9, 11)):
        rec[:, o:o + 3] = msg[:, c:c + 3] + scale * rng.normal(size=(F, 3))
        for f in range(F):
            while True:
                A = scale * 4 * rng.normal(size=(3, n))
                S = A @ A.T / n
                if np.linalg.cond(S) <= 1e3:
                    break
            rec[f, o + 3:o + 9] = S[np.triu_indices(3)]
    rec[:, 18:21] = 0.01
    return rec


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def run(layout, msg, truth, kind, spread=None, host=True, **kw):
    from wear_mocap_ape_amd import score
    s, a = score.score_rows(layout, msg if isinstance(msg, torch.Tensor) else dev(msg), truth if isinstance(truth, torch.Tensor) else dev(truth),
                            kind, spread if spread is None or isinstance(spread, torch.Tensor) else dev(spread), **kw)
    torch.cuda.synchronize()
    if not host:
        return s, a
    return (None if s is None else s.cpu().numpy()), a.cpu().numpy()


def same(a, b):
    """bit-equal up to the NaN payload"""
    return np.array_equal(a, b, equal_nan=True)


def check_rows(got, ref, what, mahal=True):
    """-> largest deviation of columns 0-4"""
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = np.isfinite(ref[:, 0])
    worst = float(np.abs(got[ok, :5] - ref[ok, :5]).max(initial=0.0))
    assert worst <= TOL, (what, worst)
    if mahal:
        for c in (5, 6):
            u = np.isfinite(ref[:, c])
            rel = np.abs(got[u, c] - ref[u, c]) / ref[u, c]
            assert rel.max(initial=0.0) <= 1e-9, (what, c, rel.max())
    return worst


COUNTS, MAXIMA = [15, 16, 17, 19, 20, 21, 23, 24], [2, 5, 8, 11, 14]


def check_acc(acc, rows, starts, skip, what):
    """the accumulators against numpy's of the call's own per-frame rows"""
    from wear_mocap_ape_amd import score
    ref = score.accumulate_numpy(rows, starts, skip)
    assert acc.shape == ref.shape, what
    assert np.array_equal(acc[:, COUNTS], ref[:, COUNTS]), (what, acc[:, COUNTS], ref[:, COUNTS])
    assert np.array_equal(acc[:, MAXIMA], ref[:, MAXIMA]), what          # bit-equal to the max of the call's own column
    st = list(starts) + [rows.shape[0]]
    for r in range(len(starts)):
        seg = rows[min(st[r] + skip, st[r + 1]):st[r + 1]]
        seg = seg[np.isfinite(seg[:, 0])]
        n = max(1, seg.shape[0])
        for c in range(5):
            top = float(seg[:, c].max(initial=0.0))
            assert abs(acc[r, 3 * c] - ref[r, 3 * c]) <= 16 * n * 2.0 ** -53 * max(1.0, top), (what, r, c)
            assert abs(acc[r, 3 * c + 1] - ref[r, 3 * c + 1]) <= 16 * n * 2.0 ** -53 * max(1.0, top * top), (what, r, c)
        for k in (0, 1):
            d2 = seg[:, 5 + k]
            top = float(d2[np.isfinite(d2)].max(initial=0.0))
            assert abs(acc[r, 18 + 4 * k] - ref[r, 18 + 4 * k]) <= 16 * n * 2.0 ** -53 * max(1.0, top), (what, r, k)
    return ref


def clear_of_thresholds(d2):
    from wear_mocap_ape_amd import score
    d2 = d2[np.isfinite(d2)]
    for q in (score.CHI2_3_Q50, score.CHI2_3_Q90):
        assert (np.abs(d2 - q) > 1e-6 * q).all()
    return d2


def case(golden, layout, tag, seed=0):
    """F = 300 messages from est_bo_N300, permuted (non-trivial errors), and the two truths of body `tag`"""
    g = golden(f"fk_layout{layout}.npz")
    perm = np.random.default_rng(seed).permutation(300)
    return msgs_from_est(g["est_bo_N300"][perm], layout), g[f"preds_{tag}_N300"], g[f"est_{tag}_N300"], g[f"body_{tag}"]


def reference_fk(preds, body, layout):
    """est rows of NN targets by the reference's route; a row with a gap is a NaN row (LAPACK is not handed NaN)"""
    ok = np.isfinite(preds).all(axis=1)
    est = np.full((preds.shape[0], 14 if layout == WATCH else 21), np.nan)
    est[ok] = orc.arm_pose_from_targets(preds[ok], body, layout, route="eigh")
    return est


STARTS = [0, 1, 257]                                       # a one-frame recording, and one that crosses a 256-frame boundary


@pytest.mark.parametrize("tag", ["bd", "bo"])
@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_est_truth_equals_numpy(golden, layout, tag):
    from wear_mocap_ape_amd.score import score_rows_numpy
    msg, _, est, _ = case(golden, layout, tag)
    ref = score_rows_numpy(msg, est, layout)
    assert np.isfinite(ref[:, :5]).all() and np.median(ref[:, :4], axis=0).min() > 1e-3       # the errors are non-trivial
    got, acc = run(layout, msg, est, "est", starts=STARTS)
    worst = check_rows(got, ref, (layout, tag))
    print(f"est truth, layout {layout} {tag}: max |device - numpy| columns 0-4 = {worst:.3e}")
    assert np.isnan(got[:, 5:]).all()
    if layout == WATCH:
        assert (got[:, 4] == 0.0).all()
    check_acc(acc, got, STARTS, 0, (layout, tag))
    assert acc[0, 15] == 1 and acc[1, 15] == 256 and acc[2, 15] == 43 and not acc[:, 16:].any()
    # two calls give the same bits; the accumulators do not depend on the per-frame rows being written
    got2, acc2 = run(layout, msg, est, "est", starts=STARTS)
    assert same(got, got2) and np.array_equal(acc, acc2)
    none, acc3 = run(layout, msg, est, "est", starts=STARTS, per_frame=False)
    assert none is None and np.array_equal(acc, acc3)


@pytest.mark.parametrize("tag", ["bd", "bo"])
@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_targets_truth_equals_est_truth(golden, layout, tag):
    """preds as TARGETS == the reference's est rows as EST, 1e-13 on columns 0-4, ill-conditioned rows included"""
    msg, preds, est, body = case(golden, layout, tag)
    a, _ = run(layout, msg, preds, "targets", bodies=body, starts=STARTS)
    b, _ = run(layout, msg, est, "est", starts=STARTS)
    d = np.abs(a[:, :5] - b[:, :5])
    print(f"targets vs est truth, layout {layout} {tag}: max {d.max():.3e}, rows above 1e-13: {int((d.max(axis=1) > TOL).sum())} of 300")
    assert d.max() <= TOL, (layout, tag, float(d.max()), int((d.max(axis=1) > TOL).sum()))


@pytest.mark.parametrize("tag", ["bd", "bo"])
@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_targets_truth_equals_reference_route(golden, layout, tag):
    """the device's truth FK against the reference's route restated in numpy (eigenvector of the 4x4 matrix)"""
    from wear_mocap_ape_amd.score import score_rows_numpy
    msg, preds, _, body = case(golden, layout, tag)
    ref = score_rows_numpy(msg, reference_fk(preds, body, layout), layout)
    got, acc = run(layout, msg, preds, "targets", bodies=body, starts=STARTS)
    worst = check_rows(got, ref, (layout, tag))
    print(f"targets truth, layout {layout} {tag}: max |device - numpy(reference route)| columns 0-4 = {worst:.3e}")
    check_acc(acc, got, STARTS, 0, (layout, tag))


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
@pytest.mark.parametrize("mdt", [torch.float32, torch.float64])
def test_dtypes_and_strided_views(golden, mdt, tdt):
    """float32 inputs are scored as the float64 values they round to; packed rows [F, 25 + 6 * 12 + 21] with NaN between message and
    record go in as two views and give the bits of contiguous rows"""
    from wear_mocap_ape_amd.score import score_rows_numpy
    rng = np.random.default_rng(11)
    msg, _, est, _ = case(golden, HIPS, "bd")
    rec = spread_records(rng, msg, 300)
    md, sd, td = dev(msg, mdt), dev(rec, mdt), dev(est, tdt)
    ref = score_rows_numpy(md.cpu().numpy().astype(np.float64), td.cpu().numpy().astype(np.float64), HIPS, sd.cpu().numpy().astype(np.float64))
    got, acc = run(HIPS, md, td, "est", sd, starts=STARTS)
    check_rows(got, ref, (mdt, tdt))
    assert np.isfinite(got).all()
    wide = torch.full((300, 25 + 72 + 21), float("nan"), dtype=mdt, device="cuda")
    wide[:, :25], wide[:, -21:] = md, sd
    got_w, acc_w = run(HIPS, wide[:, :-21], td, "est", wide[:, -21:], starts=STARTS)
    assert same(got, got_w) and np.array_equal(acc, acc_w)
    # float32 output: the float64 row rounded once
    got32, acc32 = run(HIPS, md, td, "est", sd, starts=STARTS, out_dtype=torch.float32)
    assert got32.dtype == np.float32 and same(got32, got.astype(np.float32)) and np.array_equal(acc32, acc)


def test_mahalanobis_columns_and_counts(golden):
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(21)
    msg, _, est, _ = case(golden, HIPS, "bd")
    F = 300
    est = est.copy()
    est[:, 0:6] = msg[:, [4, 5, 6, 11, 12, 13]] + 0.2 * rng.normal(size=(F, 6))        # truth a few sigma from the records' means
    rec = spread_records(rng, msg, F)
    u = rng.normal(size=3)
    B = rng.normal(size=(3, 2))
    rec[10, 3:9] = 0.0                                                                # an N = 1 record
    rec[11, 3:9] = np.outer(u, u)[np.triu_indices(3)]                                 # rank 1
    rec[12, 12:18] = (B @ B.T / 2)[np.triu_indices(3)]                                # rank 2, the elbow's
    rec[13, 5] = np.nan
    rec[258, 3:9] = 0.0
    ref = score.score_rows_numpy(msg, est, HIPS, rec)
    assert np.isnan(ref[[10, 11, 13, 258], 5]).all() and np.isnan(ref[12, 6]) and np.isfinite(ref[12, 5])
    d2 = clear_of_thresholds(np.r_[ref[:, 5], ref[:, 6]])
    inside = (d2 <= score.CHI2_3_Q90).mean()
    assert 0.05 < inside < 0.95                                                        # both sides of the thresholds are populated
    got, acc = run(HIPS, msg, est, "est", rec, starts=STARTS)
    check_rows(got, ref, "mahalanobis")
    refacc = check_acc(acc, got, STARTS, 0, "mahalanobis")
    want = score.accumulate_numpy(ref, STARTS, 0)                                      # ... and the counts numpy's own rows give
    assert np.array_equal(acc[:, COUNTS], want[:, COUNTS]) and np.array_equal(refacc[:, COUNTS], want[:, COUNTS])
    assert acc[:, 17].sum() == F - 4 and acc[:, 21].sum() == F - 1
    # no record given: NaN columns, nothing counted
    got0, acc0 = run(HIPS, msg, est, "est", starts=STARTS)
    assert np.isnan(got0[:, 5:]).all() and np.array_equal(got0[:, :5], got[:, :5]) and not acc0[:, 17:].any()


def test_skip_and_gaps(golden):
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(31)
    msg, preds, est, body = case(golden, POS, "bo")
    rec = spread_records(rng, msg, 300)
    starts, skip = [0, 40, 100, 257], 5
    for kind, truth in (("est", est.copy()), ("targets", preds.copy())):
        gaps = np.r_[rng.choice(300, 25, replace=False), 40:100]                      # scattered, and every row of recording 1
        truth[gaps, rng.integers(0, 6, size=gaps.shape[0])] = np.nan
        truth[3, 2] = np.nan                                                          # a gap inside the skipped frames
        gaps = np.unique(np.r_[gaps, 3])
        ref_truth = truth if kind == "est" else reference_fk(truth, body, POS)
        ref = score.score_rows_numpy(msg, ref_truth, POS, rec)
        got, acc = run(POS, msg, truth, kind, rec, starts=starts, skip=skip, bodies=body)
        assert np.array_equal(np.where(np.isnan(got).all(axis=1))[0], gaps) and np.isfinite(np.delete(got, gaps, axis=0)).all()
        check_rows(got, ref, kind)
        check_acc(acc, got, starts, skip, kind)
        assert not np.delete(acc[1], 16).any()                                        # the all-gap recording: zeros beside its 55 unscored frames
        st = starts + [300]
        for r in range(4):
            past = np.arange(st[r] + skip, st[r + 1])
            bad = np.isin(past, gaps).sum()
            assert acc[r, 15] == past.shape[0] - bad and acc[r, 16] == bad, (kind, r)
        assert acc[1, 16] == 55 and acc[0, 16] == np.isin(np.arange(5, 40), gaps).sum()


def test_long_and_many_recordings():
    """F = 70 001: one recording over 274 workgroups, and 64 recordings of 1 to > 8192 frames"""
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(41)
    F = 70001
    est = rng.normal(size=(F, 21))
    for c in (9, 13, 17):
        est[:, c:c + 4] /= np.linalg.norm(est[:, c:c + 4], axis=1, keepdims=True)
    msg = msgs_from_est(est[rng.permutation(F)], HIPS)
    msg[:, [4, 5, 6, 11, 12, 13]] = est[:, 0:6] + 0.1 * rng.normal(size=(F, 6))
    rec = np.zeros((F, 21))
    rec[:, 0:3], rec[:, 9:12] = msg[:, 4:7], msg[:, 11:14]
    rec[:, [3, 6, 8, 12, 15, 17]] = 0.01 * rng.uniform(0.5, 2.0, size=(F, 6))
    est[rng.choice(F, 500, replace=False), 1] = np.nan
    ref = score.score_rows_numpy(msg, est, HIPS, rec)
    clear_of_thresholds(np.r_[ref[:, 5], ref[:, 6]])
    lens = np.r_[1, 1, 2, 63, 64, 65, 255, 256, 257, 8193, 1, 511, 513, rng.integers(1, 900, size=50)]
    lens = np.r_[lens, F - lens.sum()]
    assert lens.shape[0] == 64 and lens[-1] > 8192
    md, td, sd = dev(msg), dev(est), dev(rec)
    for starts in ([0], list(np.cumsum(np.r_[0, lens[:-1]]))):
        got, acc = run(HIPS, md, td, "est", sd, starts=starts, skip=5)
        check_rows(got, ref, len(starts))
        check_acc(acc, got, starts, 5, len(starts))
        got2, acc2 = run(HIPS, md, td, "est", sd, starts=starts, skip=5)
        assert same(got, got2) and np.array_equal(acc, acc2)
        _, acc3 = run(HIPS, md, td, "est", sd, starts=starts, skip=5, per_frame=False)
        assert np.array_equal(acc, acc3)


def test_one_body_per_recording(golden):
    msg, preds, _, _ = case(golden, HIPS, "bd")
    g = golden("fk_layout0.npz")
    bodies = np.concatenate([g["body_bd"], g["body_bo"], 1.1 * g["body_bd"]])
    got, acc = run(HIPS, msg, preds, "targets", starts=STARTS, bodies=bodies)
    st = STARTS + [300]
    for r in range(3):
        one, acc1 = run(HIPS, msg[st[r]:st[r + 1]], preds[st[r]:st[r + 1]], "targets", bodies=bodies[r])
        assert same(one, got[st[r]:st[r + 1]]), r
        assert np.array_equal(acc1[0, COUNTS + MAXIMA], acc[r, COUNTS + MAXIMA])
    assert not np.array_equal(got[1:257], run(HIPS, msg, preds, "targets", starts=STARTS, bodies=bodies[0])[0][1:257])


def test_score_recording_takes_bonemaps(golden):
    """`score_recording(bonemaps=)`: one bonemap-like object for all recordings, or one entry per recording"""
    from types import SimpleNamespace
    from wear_mocap_ape_amd.data_types.bone_map import body9_from_bonemap
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    msg, preds, _, _ = case(golden, WATCH, "bd")
    a = SimpleNamespace(left_lower_arm_length=0.25, left_upper_arm_length=0.31, left_upper_arm_origin_rh=np.array([-0.2, 0.4, 0.01]))
    b = SimpleNamespace(left_lower_arm_length=0.21, left_upper_arm_length=0.27, left_upper_arm_origin_rh=np.array([-0.15, 0.45, 0.0]))
    est_obj, md, td = WatchPhoneUarm(smooth=1), dev(msg), dev(preds)
    host = lambda pair: tuple(x.cpu().numpy() for x in pair)                      # noqa: E731
    one = host(est_obj.score_recording(md, td, starts=STARTS, bonemaps=a))
    want = run(WATCH, md, td, "targets", starts=STARTS, bodies=body9_from_bonemap(a))
    assert same(one[0], want[0]) and np.array_equal(one[1], want[1])
    per = host(est_obj.score_recording(md, td, starts=STARTS, bonemaps=[a, None, b]))
    want = run(WATCH, md, td, "targets", starts=STARTS, bodies=np.stack([body9_from_bonemap(a), body9_from_bonemap(None), body9_from_bonemap(b)]))
    assert same(per[0], want[0]) and np.array_equal(per[1], want[1])
    assert same(per[0][:1], one[0][:1]) and not same(per[0][257:], one[0][257:])
    own = host(est_obj.score_recording(md, td, starts=STARTS))
    assert same(own[0], run(WATCH, md, td, "targets", starts=STARTS, bodies=est_obj.body_measurements)[0])
    with pytest.raises(UserWarning):
        est_obj.score_recording(md, td, starts=STARTS, bonemaps=[a, b])               # two entries for three recordings


# ---------------- end to end: replays scored through the estimators' one-line methods -----------------------------------------------------
def _truth_for(golden, layout, F, rng):
    g = golden(f"fk_layout{layout}.npz")
    pick = 60 + rng.permutation(240)[:F]                   # (the fixtures' ordinary rows)
    return g["preds_bd_N300"][pick], g["est_bd_N300"][pick]


def _end_to_end(est_obj, out, rec, starts, truth_t, truth_e, what):
    from wear_mocap_ape_amd import score
    layout = est_obj._layout
    s_e, a_e = est_obj.score_recording(out, dev(truth_e), spread=rec, starts=starts, truth_kind="est")
    s_t, a_t = est_obj.score_recording(out, dev(truth_t), spread=rec, starts=starts)
    torch.cuda.synchronize()
    s_e, a_e, s_t, a_t = (x.cpu().numpy() for x in (s_e, a_e, s_t, a_t))
    ref = score.score_rows_numpy(out.cpu().numpy(), truth_e, layout, None if rec is None else rec.cpu().numpy())
    check_rows(s_e, ref, what)
    fk = reference_fk(truth_t, est_obj.body_measurements, layout)
    check_rows(s_t, score.score_rows_numpy(out.cpu().numpy(), fk, layout, None if rec is None else rec.cpu().numpy()), what)
    return s_e, a_e


def test_end_to_end_pocket_nn(golden, tmp_path, monkeypatch):
    from tests.test_replay import _estimator
    from wear_mocap_ape_amd import score
    est_obj = _estimator(tmp_path, monkeypatch, "pocket", 1, 0.2, smooth=1, add_mc_samples=True, monte_carlo_samples=25)
    rows = np.tile(golden("stream_trace_pocket.npz")["rows"].astype(np.float32), (3, 1))
    starts = [0, 20, 40]
    out, rec = est_obj.process_recording(rows, starts=starts, seed=5, spread=True)
    assert tuple(out.shape) == (60, 25 + 6 * 25) and not out.is_contiguous() and tuple(rec.shape) == (60, 21)
    truth_t, truth_e = _truth_for(golden, HIPS, 60, np.random.default_rng(51))
    s, acc = _end_to_end(est_obj, out, rec, starts, truth_t, truth_e, "pocket")
    assert np.isfinite(s).all()                            # 25 samples: every covariance is usable
    skip = est_obj.sequence_len - 1
    check_acc(acc, s, starts, skip, "pocket")
    d = score.summarise(acc)
    assert [r["scored"] for r in d] == [20 - skip] * 3 and all(r["hand"]["frames"] == 20 - skip for r in d)


def test_end_to_end_fk_only(golden):
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    est_obj = WatchPhoneUarm(smooth=5)
    rows = np.tile(golden("stream_trace_uarm.npz")["rows"].astype(np.float32), (3, 1))[:60]
    starts = [0, 20, 40]
    out = est_obj.process_recording(rows, starts=starts)
    truth_t, truth_e = _truth_for(golden, WATCH, 60, np.random.default_rng(52))
    s, acc = _end_to_end(est_obj, out, None, starts, truth_t, truth_e, "uarm")
    assert np.isfinite(s[:, :5]).all() and np.isnan(s[:, 5:]).all() and (s[:, 4] == 0.0).all()
    check_acc(acc, s, starts, 0, "uarm")
    assert (acc[:, 15] == 20).all() and not acc[:, 17:].any()


def test_end_to_end_kalman(golden):
    from oracle import kalman_oracle as ko
    from tests.test_kalman_bank_gpu import _estimator, make_rows
    E, W, smooth = 16, 4, 2
    est_obj = _estimator(ko.make_state_dict(W, 36), E, W, smooth=smooth)
    rows = make_rows(np.random.default_rng(36), 60)
    starts = [0, 20, 40]
    out, n, rec = est_obj.process_recording(rows, starts=starts, seed=4242, spread=True)
    assert tuple(out.shape) == (60, 25 + 6 * smooth * E) and tuple(rec.shape) == (60, 21)
    truth_t, truth_e = _truth_for(golden, HIPS, 60, np.random.default_rng(53))
    s, acc = _end_to_end(est_obj, out, rec, starts, truth_t, truth_e, "kalman")
    n = n.cpu().numpy()
    assert np.isfinite(s[:, :5]).all()
    assert np.isnan(s[n <= smooth, 5:]).all() and (n <= smooth).sum() >= 15   # warm-up frames: one row per stacked frame, rank <= 1
    assert np.isfinite(s[n >= 8, 5:]).all() and (n >= 8).sum() >= 30
    check_acc(acc, s, starts, W + 1, "kalman")


# ---------------- refusals: made on the host, nothing written ---------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    F = 10
    msg = torch.zeros((F, 25), dtype=torch.float64, device="cuda")
    rec = torch.zeros((F, 21), dtype=torch.float64, device="cuda")
    truth = torch.zeros((F, 21), dtype=torch.float64, device="cuda")
    score = torch.full((F, 7), -7.0, dtype=torch.float64, device="cuda")
    acc = torch.full((3, 25), -7.0, dtype=torch.float64, device="cuda")
    body = np.zeros((3, 9))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(layout=0, m=msg, ms=25, s=rec, ss=21, md=_hip.F64, t=truth, kind=1, td=_hip.F64, F=F, starts=(0, 3, 7), skip=0, bodies=body,
             nb=1, sc=score, sd=_hip.F64, ac=acc, R=None):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        return lib.ape_score_rows(layout, p(m), ms, p(s), ss, md, p(t), kind, td, F, C.c_void_p(st.ctypes.data) if len(st) else None,
                                  len(st) if R is None else R, skip, C.c_void_p(bodies.ctypes.data) if bodies is not None else None, nb, p(sc), sd, p(ac), stream)

    bad = [dict(m=None), dict(t=None), dict(sc=None, ac=None), dict(F=0), dict(starts=()), dict(starts=(1, 3)), dict(starts=(0, 5, 5)),
           dict(starts=(0, 10)), dict(starts=(0, 7, 3)), dict(ms=24), dict(ss=20), dict(skip=-1), dict(nb=2), dict(nb=0), dict(bodies=None),
           dict(layout=_hip.LAYOUT_NONE), dict(layout=3), dict(kind=2), dict(kind=-1), dict(md=2), dict(td=2), dict(sd=2),
           dict(R=0), dict(R=-1), dict(R=11)]                  # R < 1 and R > F beside a valid starts pointer
    for kw in bad:
        assert call(**kw) == 1, kw                          # APE_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (score == -7.0).all() and (acc == -7.0).all()
    assert call() == 0                                      # ... and the same arguments without the fault are taken
    torch.cuda.synchronize()
    assert not (score == -7.0).any() and not (acc == -7.0).any()
