"""Joint angles of a pose (`ape_joint_angles`): the numpy statement `score.joint_angles_numpy` against poses built from
planted angles, without a GPU.

The builders below make quaternions from the angles by their geometric meaning (a shortest arc onto the planted bone direction, a
rotation about a planted axis in the parent's y-z plane, twists about the bone axis x) -- not by inverting the statement's formulas.
The statement must give the planted angles back within 1e-12 rad: on 200 000 such draws (swings in [0.3, pi - 0.3], twists in
(-pi + 0.01, pi - 0.01)) the worst deviation of these formulas in float64 is 2.4e-14, a margin of about 40.

Sums: within 16 n u max(1, max term) (the rule of tests/test_frame_fit_gpu.py); counts, minima and maxima exact."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests.test_frame_fit_cpu import qconj, qmat, qmul

REPO = Path(__file__).resolve().parent.parent
HIPS, WATCH, POS = 0, 1, 2
U = 2.0 ** -53
TOL = 1e-12
PERIODIC = (1, 2, 4, 5, 6)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


# ---------------- builders ---------------------------------------------------------------------------------------------------------------------
def twist_x(a):
    a = np.asarray(a, dtype=np.float64)
    z = np.zeros_like(a)
    return np.stack([np.cos(a / 2), np.sin(a / 2), z, z], axis=-1)


def shortest_arc(a, b):
    """the rotation of least angle that takes the unit vector a onto the unit vectors b [n, 3]"""
    a = np.broadcast_to(np.asarray(a, dtype=np.float64), b.shape)
    q = np.concatenate([1.0 + (a * b).sum(axis=1, keepdims=True), np.cross(a, b)], axis=1)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def upper_in_thorax(elevation, plane, htwist):
    d = np.stack([-np.sin(elevation) * np.cos(plane), -np.cos(elevation), np.sin(elevation) * np.sin(plane)], axis=1)
    return qmul(shortest_arc([-1.0, 0.0, 0.0], d), twist_x(htwist))


def fore_in_upper(flexion, azimuth, ftwist):
    z = np.zeros_like(flexion)
    swing = np.stack([np.cos(flexion / 2), z, np.sin(flexion / 2) * np.cos(azimuth), np.sin(flexion / 2) * np.sin(azimuth)], axis=1)
    return qmul(swing, twist_x(ftwist))


def quats_of(angles, layout, rng=None, s=None, e=None):
    """(q_l, q_u, q_h) stating angles [n, 7] in the statement's column order; random signs with rng; s / e: given joint rotations"""
    n = angles.shape[0]
    yaw = angles[:, 6] if layout != WATCH else np.zeros(n)
    z = np.zeros(n)
    qh = np.stack([np.cos(yaw / 2), z, np.sin(yaw / 2), z], axis=1)
    s = upper_in_thorax(angles[:, 3], angles[:, 4], angles[:, 5]) if s is None else s
    e = fore_in_upper(angles[:, 0], angles[:, 1], angles[:, 2]) if e is None else e
    qu = qmul(qh, s)
    ql = qmul(qu, e)
    if rng is not None:
        ql, qu, qh = (q * rng.choice([-1.0, 1.0], size=(n, 1)) for q in (ql, qu, qh))
    if layout == WATCH:
        qh = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    return ql, qu, qh


def est_of(ql, qu, qh, layout):
    """est rows [n, 21 | 14] with these quaternions (positions: the default body's forward kinematics)"""
    from wear_mocap_ape_amd.data_types.bone_map import body9_from_bonemap
    body = body9_from_bonemap(None)
    uo = np.einsum("nab,b->na", qmat(qh), body[6:9])
    elbow = np.einsum("nab,b->na", qmat(qu), body[3:6]) + uo
    hand = np.einsum("nab,b->na", qmat(ql), body[0:3]) + elbow
    if layout == WATCH:
        return np.concatenate([hand, elbow, ql, qu], axis=1)
    return np.concatenate([hand, elbow, uo, ql, qu, qh], axis=1)


def msgs_of(est, layout):
    from tests.test_frame_fit_cpu import msgs_from_est
    return msgs_from_est(est, layout)


def targets_of(est, layout):
    """NN targets that state the est rows' pose: 6D rotations (the first two columns of the matrices, row by row), the hips yaw as
    (sin, cos), and for the layout that predicts them the positions"""
    ql, qu = (6, 10) if layout == WATCH else (9, 13)
    six = lambda q: qmat(q)[:, :, :2].reshape(-1, 6)        # noqa: E731
    cols = [six(est[:, ql:ql + 4]), six(est[:, qu:qu + 4])]
    if layout != WATCH:
        w, y = est[:, 17], est[:, 19]
        cols.append(np.stack([2.0 * w * y, w * w - y * y], axis=1))
    if layout == POS:
        cols = [est[:, 0:3], cols[0], est[:, 3:6], cols[1], cols[2]]
    return np.concatenate(cols, axis=1)


def rows_of_kind(est, layout, kind):
    return {"est": est, "msg": msgs_of(est, layout), "targets": targets_of(est, layout)}[kind]


def draw_angles(rng, n):
    """[n, 7] in the statement's order: swings in [0.3, pi - 0.3], periodic angles in (-pi + 0.01, pi - 0.01)"""
    a = rng.uniform(-np.pi + 0.01, np.pi - 0.01, size=(n, 7))
    a[:, [0, 3]] = rng.uniform(0.3, np.pi - 0.3, size=(n, 2))
    return a


def circle(d):
    """|d| on the circle"""
    return np.abs(np.angle(np.exp(1j * d)))


def default_body():
    from wear_mocap_ape_amd.data_types.bone_map import body9_from_bonemap
    return body9_from_bonemap(None)


def check_sums(acc, angles, errors, starts, skip, what=""):
    """accumulators [R, 71] against numpy's sums of per-frame rows: sums within 16 n u max(1, max term); minima, maxima, counts exact"""
    F = angles.shape[0]
    ends = list(starts[1:]) + [F]
    assert acc.shape == (len(starts), 71), what
    for r, (s, e) in enumerate(zip(starts, ends)):
        lo = min(s + skip, e)
        assert acc[r, 70] == e - lo, (what, r)
        for k in range(7):
            v = angles[lo:e, k].astype(np.float64)
            v = v[np.isfinite(v)]
            n, top = max(1, v.shape[0]), float(np.abs(v).max(initial=0.0))
            assert acc[r, 5 * k + 4] == v.shape[0] and acc[r, 5 * k + 2] == v.min(initial=np.inf) and acc[r, 5 * k + 3] == v.max(initial=-np.inf), (what, r, k)
            assert abs(acc[r, 5 * k] - v.sum()) <= 16 * n * U * max(1.0, top), (what, r, k)
            assert abs(acc[r, 5 * k + 1] - (v * v).sum()) <= 16 * n * U * max(1.0, top * top), (what, r, k)
            assert acc[r, 5 * k + 4] + np.isnan(angles[lo:e, k]).sum() == acc[r, 70], (what, r, k)        # count + left out = support
            if errors is None:
                assert not acc[r, 35 + 5 * k:40 + 5 * k].any(), (what, r, k)
                continue
            d = errors[lo:e, k].astype(np.float64)
            d = d[np.isfinite(d)]
            n, top = max(1, d.shape[0]), float(np.abs(d).max(initial=0.0))
            assert acc[r, 35 + 5 * k + 4] == d.shape[0] and acc[r, 35 + 5 * k + 3] == top, (what, r, k)
            assert abs(acc[r, 35 + 5 * k] - d.sum()) <= 16 * n * U * max(1.0, top), (what, r, k)
            assert abs(acc[r, 35 + 5 * k + 1] - np.abs(d).sum()) <= 16 * n * U * max(1.0, top), (what, r, k)
            assert abs(acc[r, 35 + 5 * k + 2] - (d * d).sum()) <= 16 * n * U * max(1.0, top * top), (what, r, k)
            assert acc[r, 35 + 5 * k + 4] + np.isnan(errors[lo:e, k]).sum() == acc[r, 70], (what, r, k)


# ---------------- 1: planted poses -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_planted_angles_come_back(layout):
    from wear_mocap_ape_amd.score import joint_angles_numpy
    rng = np.random.default_rng(41 + layout)
    n = 4000
    want = draw_angles(rng, n)
    if layout == WATCH:
        want[:, 6] = 0.0
    ql, qu, qh = quats_of(want, layout, rng)
    est = est_of(ql, qu, qh, layout)
    # column 0 is the angle between the two bone axes in the world
    bu, bl = -qmat(qu)[:, :, 0], -qmat(ql)[:, :, 0]
    between = np.arctan2(np.linalg.norm(np.cross(bu, bl), axis=1), (bu * bl).sum(axis=1))
    worst = 0.0
    for kind in ("msg", "est", "targets"):
        rows = rows_of_kind(est, layout, kind)
        got, errors, acc = joint_angles_numpy(rows, layout, kind, bodies=default_body(), min_swing=0.0)
        assert errors is None and got.shape == (n, 7) and np.isfinite(got).all(), kind
        # at the default threshold the one angle these draws can leave ill-conditioned is the humeral twist, where the upper arm points
        # across the body within min_swing of +x (the swing of s within min_swing of pi); nothing else changes
        cond, _, _ = joint_angles_numpy(rows, layout, kind, bodies=default_body())
        to_pole = np.arccos(np.clip(-np.sin(want[:, 3]) * np.cos(want[:, 4]), -1.0, 1.0))
        assert not np.isnan(np.delete(cond, 5, axis=1)).any() and np.array_equal(cond[~np.isnan(cond)], got[~np.isnan(cond)]), kind
        clear = np.abs(to_pole - 0.05) > 1e-9
        assert np.array_equal(np.isnan(cond[clear, 5]), to_pole[clear] < 0.05), kind
        dev = np.abs(got - want)
        dev[:, PERIODIC] = circle(got[:, PERIODIC] - want[:, PERIODIC])
        worst = max(worst, float(dev.max()))
        assert dev.max() <= TOL, (layout, kind, dev.max(axis=0))
        assert np.abs(got[:, 0] - between).max() <= TOL, (layout, kind)
        assert (got[:, [0, 3]] >= 0.0).all() and (got[:, [0, 3]] <= np.pi).all() and (np.abs(got) <= np.pi).all()
        if layout == WATCH:
            assert (got[:, 6] == 0.0).all()
        check_sums(acc, got, None, [0], 0, (layout, kind))
    print(f"layout {layout}: worst deviation from the planted angles {worst:.2e} rad (allowed {TOL:.0e})")


# ---------------- 2: the singular cases ----------------------------------------------------------------------------------------------------------
def singular_rows(layout, rng, n=40):
    """(est rows, {row: column that must be NaN}): a walk of well-conditioned poses with one row of each singular case planted"""
    a = draw_angles(rng, n)
    a[5, 0] = 0.0                                           # a straight arm: no hinge axis
    a[9, 3] = 0.0                                           # the arm hanging: no plane of elevation
    a[13, 3] = np.pi                                        # ... and straight up
    a[17, 0] = 0.02                                         # inside the band, not on the pole
    a[21, 3] = np.pi - 0.03
    s = upper_in_thorax(a[:, 3], a[:, 4], a[:, 5])
    e = fore_in_upper(a[:, 0], a[:, 1], a[:, 2])
    e[25] = qmul(np.array([0.0, 0.0, np.cos(0.7), np.sin(0.7)]), twist_x(np.array(0.4)))      # a swing of pi: the forearm's twist is lost
    s[29] = qmul(np.array([0.0, 0.0, np.cos(-1.1), np.sin(-1.1)]), twist_x(np.array(-2.0)))   # ... and the upper arm's
    ql, qu, qh = quats_of(a, layout, rng, s, e)
    return est_of(ql, qu, qh, layout), {5: 1, 9: 4, 13: 4, 17: 1, 21: 4, 25: 2, 29: 5}


@pytest.mark.parametrize("layout", [HIPS, WATCH])
def test_singular_cases_blank_exactly_their_column(layout):
    from wear_mocap_ape_amd.score import joint_angles_numpy
    est, gone = singular_rows(layout, np.random.default_rng(7))
    n = est.shape[0]
    for kind in ("msg", "est", "targets"):
        rows = rows_of_kind(est, layout, kind)
        got, _, acc = joint_angles_numpy(rows, layout, kind, bodies=default_body(), min_swing=0.05)
        want_nan = np.zeros((n, 7), dtype=bool)
        for row, col in gone.items():
            want_nan[row, col] = True
        assert np.array_equal(np.isnan(got), want_nan), (layout, kind, np.argwhere(np.isnan(got) != want_nan))
        assert np.array_equal(acc[0, 4:35:5], n - want_nan.sum(axis=0)) and acc[0, 70] == n            # counted so
        assert abs(got[5, 0]) <= 1e-7 and abs(got[25, 0] - np.pi) <= 1e-7 and got[9, 3] <= 1e-7 and abs(got[13, 3] - np.pi) <= 1e-7
        free, _, acc0 = joint_angles_numpy(rows, layout, kind, bodies=default_body(), min_swing=0.0)
        assert np.isfinite(free).all() and (acc0[0, 4:35:5] == n).all(), (layout, kind)                # min_swing = 0 states everything
        keep = ~want_nan
        assert np.array_equal(free[keep], got[keep])                                                    # the threshold changes nothing else


def test_rows_that_state_no_pose_are_all_nan():
    from wear_mocap_ape_amd.score import joint_angles_numpy
    rng = np.random.default_rng(3)
    est = est_of(*quats_of(draw_angles(rng, 12), HIPS, rng), HIPS)
    msg = msgs_of(est, HIPS)
    msg[2, 15] = np.nan                                     # a quaternion component
    msg[4, 7:11] = 0.0                                      # a zero norm
    msg[6, 5] = np.nan                                      # a position: not read
    msg[8, 21:25] = np.inf
    got, _, acc = joint_angles_numpy(msg, HIPS, "msg", min_swing=0.0)
    assert np.array_equal(np.isnan(got).all(axis=1), np.isin(np.arange(12), [2, 4, 8])) and np.isfinite(got[[0, 1, 3, 5, 6, 7]]).all()
    assert (acc[0, 4:35:5] == 9).all() and acc[0, 70] == 12
    tg = targets_of(est, HIPS)
    tg[3, 13] = np.nan                                      # any target blanks a target row
    got, _, _ = joint_angles_numpy(tg, HIPS, "targets", bodies=default_body(), min_swing=0.0)
    assert np.isnan(got[3]).all() and np.isfinite(np.delete(got, 3, axis=0)).all()
    with pytest.raises(UserWarning):
        joint_angles_numpy(msg, HIPS, "msg", min_swing=np.pi / 2)
    with pytest.raises(UserWarning):
        joint_angles_numpy(msg, HIPS, "msg", min_swing=-0.1)


# ---------------- 3: errors: the wrap and the lags -----------------------------------------------------------------------------------------------
def test_errors_wrap_once_on_the_circle():
    from wear_mocap_ape_amd.score import joint_angles_numpy
    t = np.tile([1.0, 0.5, np.pi - 0.01, 1.2, -3.0, 3.0, 0.3], (4, 1))
    m = np.tile([1.5, 0.7, -np.pi + 0.01, 1.0, 3.0, -3.0, 0.1], (4, 1))
    truth = est_of(*quats_of(t, HIPS), HIPS)
    rows = msgs_of(est_of(*quats_of(m, HIPS), HIPS), HIPS)
    _, err, acc = joint_angles_numpy(rows, HIPS, "msg", truth, "est", min_swing=0.05)
    want = np.array([0.5, 0.2, 0.02, -0.2, 6.0 - 2 * np.pi, 2 * np.pi - 6.0, -0.2])
    assert np.abs(err - want[None, :]).max() <= TOL, err[0]
    assert np.abs(acc[0, 35::5][:7] - 4 * want).max() <= 1e-11 and np.abs(acc[0, 36::5][:7] - 4 * np.abs(want)).max() <= 1e-11
    assert np.abs(acc[0, 38::5][:7] - np.abs(want)).max() <= TOL and (acc[0, 39::5][:7] == 4).all()
    # the non-periodic columns are not folded, a NaN on either side is a NaN
    t2 = t.copy()
    t2[1, 0] = 0.0                                          # truth's arm straight: its hinge azimuth is NaN
    truth2 = est_of(*quats_of(t2, HIPS), HIPS)
    _, err2, acc2 = joint_angles_numpy(rows, HIPS, "msg", truth2, "est", min_swing=0.05)
    assert np.isnan(err2[1, 1]) and np.isfinite(np.delete(err2.reshape(-1), 8)).all() and acc2[0, 35 + 5 + 4] == 3
    assert abs(err2[1, 0] - 1.5) <= 1e-7


def test_a_lag_pairs_frames_inside_their_recording_only():
    from wear_mocap_ape_amd.score import joint_angles_numpy
    F, starts, lags = 30, [0, 10, 11, 20], [2, 0, -3, 1]
    rng = np.random.default_rng(5)
    t = draw_angles(rng, F)
    t[:, 0] = 0.5 + 0.01 * np.arange(F)
    m = t.copy()
    m[:, 0] = 1.0
    truth = targets_of(est_of(*quats_of(t, HIPS, rng), HIPS), HIPS)
    rows = est_of(*quats_of(m, HIPS, rng), HIPS)
    ang, err, acc = joint_angles_numpy(rows, HIPS, "est", truth, "targets", starts, 1, lags, default_body(), 0.05)
    check_sums(acc, ang, err, starts, 1, "lags")
    ends = starts[1:] + [F]
    for s, e, l in zip(starts, ends, lags):
        for f in range(s, e):
            if s <= f - l < e:
                assert abs(err[f, 0] - (1.0 - (0.5 + 0.01 * (f - l)))) <= TOL, f
                assert np.isfinite(err[f]).all()
            else:
                assert np.isnan(err[f]).all(), f
    # support f - s >= 1; paired: f >= 2 of 0 .. 9; nothing of the one-frame recording; 12 .. 16 of 11 .. 19; 21 .. 29
    assert acc[:, 39].tolist() == [8.0, 0.0, 5.0, 9.0] and acc[:, 70].tolist() == [9.0, 0.0, 8.0, 9.0]
    assert acc[1, 2] == np.inf and acc[1, 3] == -np.inf and not acc[1, [0, 1, 4]].any() and not acc[1, 35:70].any()    # the stated empties
    none = joint_angles_numpy(rows, HIPS, "est", truth, "targets", starts, 1, None, default_body(), 0.05)[1]
    assert np.isfinite(none).all() and np.abs(none[:, 0] - (1.0 - t[:, 0])).max() <= TOL


# ---------------- 4: accumulators, merging, summaries, edges ---------------------------------------------------------------------------------------
def walk_rows(layout=HIPS, n=100, seed=0):
    rng = np.random.default_rng(seed)
    a, b = draw_angles(rng, n), draw_angles(rng, n)
    return msgs_of(est_of(*quats_of(a, layout, rng), layout), layout), est_of(*quats_of(b, layout, rng), layout)


def test_accumulators_merge_and_summaries():
    from wear_mocap_ape_amd import score
    rows, truth = walk_rows()
    starts, skip = [0, 40], 0
    ang, err, acc = score.joint_angles_numpy(rows, HIPS, "msg", truth, "est", starts, skip)
    check_sums(acc, ang, err, starts, skip, "whole")
    _, _, skipped = score.joint_angles_numpy(rows, HIPS, "msg", truth, "est", starts, 7)
    check_sums(skipped, ang, err, starts, 7, "skip")
    # two pieces of both recordings: [0, 20) + [40, 70) and [20, 40) + [70, 100)
    ia, ib = np.r_[0:20, 40:70], np.r_[20:40, 70:100]
    pa = score.joint_angles_numpy(rows[ia], HIPS, "msg", truth[ia], "est", [0, 20], 0)[2]
    pb = score.joint_angles_numpy(rows[ib], HIPS, "msg", truth[ib], "est", [0, 20], 0)[2]
    merged = score.merge_angles(pa, pb)
    exact = sorted(list(score._ANGLE_MIN_COLS) + list(score._ANGLE_MAX_COLS) + list(range(4, 70, 5)) + [70])
    assert np.array_equal(merged[:, exact], acc[:, exact])
    check_sums(merged, ang, err, starts, skip, "merged")
    assert score.merge_angles(np.stack([pa, pa]), np.stack([pb, pb])).shape == (2, 2, 71)
    with pytest.raises(UserWarning):
        score.merge_angles(pa, pb[:1])
    res = score.summarise_angles(acc)
    assert len(res) == 2 and res[0]["frames"] == 40 and res[1]["frames"] == 60
    for r, (s, e) in enumerate(((0, 40), (40, 100))):
        for k, name in enumerate(score.ANGLE_NAMES):
            d, g = res[r]["rad"][name], res[r]["deg"][name]
            v, x = ang[s:e, k], err[s:e, k]
            assert d["count"] == e - s == d["error_count"]
            assert abs(d["mean"] - v.mean()) <= 1e-12 and abs(d["std"] - v.std()) <= 1e-10 and d["rom"] == v.max() - v.min()
            assert abs(d["bias"] - x.mean()) <= 1e-12 and abs(d["mae"] - np.abs(x).mean()) <= 1e-12
            assert abs(d["rmse"] - np.sqrt((x * x).mean())) <= 1e-12 and d["worst"] == np.abs(x).max()
            assert abs(g["rmse"] - np.degrees(d["rmse"])) <= 1e-9 and g["count"] == d["count"]
    empty = score.summarise_angles(score.joint_angles_numpy(rows[:3], HIPS, "msg", skip=5)[2])[0]
    assert empty["frames"] == 0 and np.isnan(empty["rad"]["elbow_flexion"]["mean"]) and np.isnan(empty["deg"]["hips_yaw"]["rmse"])


def test_angle_edges_and_the_histogram_statement():
    from wear_mocap_ape_amd import score
    e = score.angle_edges()
    assert e.shape == (14, 73) and (np.diff(e, axis=1) > 0).all()
    for k in range(14):
        lo = 0.0 if k in (0, 3) else -np.pi
        assert e[k, 0] == lo and e[k, -1] == np.pi
    assert abs(e[7, 37] - np.radians(5.0)) <= 1e-15 and abs(e[0, 2] - np.radians(5.0)) <= 1e-15         # an edge at 5 degrees
    assert score.angle_edges(8).shape == (14, 9)
    for bad in (0, 257):
        with pytest.raises(UserWarning):
            score.angle_edges(bad)
    before = score.default_edges("score"), score.default_edges("motion")
    assert before[0].shape == (7, 65) and before[1].shape == (12, 65)                                   # default_edges stays as it is
    rows, truth = walk_rows(seed=2)
    ang, err, _ = score.joint_angles_numpy(rows, HIPS, "msg", truth, "est", [0, 40])
    h = score.hist_numpy(np.concatenate([ang, err], axis=1), e, [0, 40], 0)
    assert h.shape == (2, 14, 75) and (h.sum(axis=2) == np.array([40, 60])[:, None]).all()
    assert not h[:, :, 72:74].any()                                                                     # nothing below or above the ranges


# ---------------- 5: header, binding, refusals -------------------------------------------------------------------------------------------------------
PARAMS = ["int32_t layout", "const void* rows_dev", "int32_t rows_kind", "int32_t rows_stride", "int32_t rows_dtype", "int32_t n_sets",
          "int64_t set_stride", "const void* truth_dev", "int32_t truth_kind", "int32_t truth_stride", "int32_t truth_dtype",
          "const int32_t* rec_lag_host", "int32_t F", "const int32_t* seg_starts_host", "int32_t R", "int32_t skip", "const double* bodies_host",
          "int32_t n_bodies", "double min_swing", "void* angles_dev", "void* errors_dev", "int32_t out_dtype", "double* acc_dev", "void* stream"]


def test_header_declares_and_hip_binds_the_entry():
    import inspect
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    for name, value in (("APE_ANGLE_WIDTH", 7), ("APE_ANGLE_ACC_WIDTH", 71)):
        assert re.search(rf"^#define {name}\s+{value}\b", text, flags=re.M), name
    assert (_hip.ANGLE_WIDTH, _hip.ANGLE_ACC_WIDTH) == (7, 71) == (score.ANGLE_WIDTH, score.ANGLE_ACC_WIDTH) and len(score.ANGLE_NAMES) == 7
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    decl = text[text.index("\nint ape_joint_angles(") + 1:]
    decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
    got = [" ".join(p.split()) for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
    assert got == PARAMS, got
    assert text.index("int ape_joint_angles(") > text.index("int ape_score_hist(")                      # after the 4.40 block
    res, args = _hip.SIGNATURES["ape_joint_angles"]
    assert hasattr(_hip.lib(), "ape_joint_angles") and res is C.c_int and len(args) == len(PARAMS)        # the library exports the symbol
    for p, a in zip(PARAMS, args):
        want = C.c_void_p if "*" in p else (C.c_int64 if p.startswith("int64_t") else (C.c_double if p.startswith("double") else C.c_int32))
        assert a is want, (p, a)
    assert _hip.lib().ape_joint_angles.argtypes == args
    make = (REPO / "arm-pose-estimation_amd" / "csrc" / "Makefile").read_text()
    assert "joint_angles.hip" in re.search(r"^SRCS\s*:=(.*)$", make, flags=re.M).group(1).split()
    for name in ("joint_angles", "joint_angles_numpy", "summarise_angles", "merge_angles", "angle_edges"):
        assert callable(getattr(score, name))
    sig = inspect.signature(score.joint_angles_numpy)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[2:]] == [
        ("kind", "msg"), ("truth", None), ("truth_kind", "est"), ("starts", None), ("skip", 0), ("rec_lags", None), ("bodies", None),
        ("min_swing", 0.05)]
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    for cls in (Estimator, WatchPhoneUarm, WatchPhonePocketKalman):
        assert "angles_recording" in vars(cls) and "truth_angles" in vars(cls)
    sig = inspect.signature(Estimator.angles_recording)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[2:]] == [
        ("truth", None), ("starts", None), ("skip", None), ("bonemaps", None), ("truth_kind", "targets"), ("rec_lags", None),
        ("per_frame", False), ("min_swing", 0.05)]


def refusals():
    """(keyword overrides of `call_entry`, a word of the message) of every refusal include/ape_hip.h states but the capturing stream"""
    from wear_mocap_ape_amd import _hip
    one = np.zeros((1, 9))
    T, E = _hip.ROWS_TARGETS, _hip.ROWS_EST
    return [(dict(rows=None), b"NULL"), (dict(starts=()), b"NULL"), (dict(angles=None, errors=None, acc=None), b"no output"),
            (dict(truth=None), b"without truth"),
            (dict(F=0), b"F=0"), (dict(R=0), b"recording starts"), (dict(R=11), b"recording starts"),
            (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 10)), b"seg_starts[1]"),
            (dict(skip=-1), b"skip"),
            (dict(kind=3), b"kind"), (dict(kind=-1), b"kind"), (dict(tk=3), b"kind"), (dict(rd=2), b"dtype"), (dict(od=-1), b"dtype"), (dict(td=7), b"dtype"),
            (dict(layout=_hip.LAYOUT_NONE), b"layout"), (dict(layout=3), b"layout"),
            (dict(rs=24), b"rows_stride"), (dict(kind=E, rs=20), b"rows_stride"), (dict(kind=E, layout=WATCH, rs=13, ts=14), b"rows_stride"),
            (dict(kind=T, layout=POS, rs=19, bodies=one, nb=1), b"rows_stride"),
            (dict(ts=20), b"truth_stride"), (dict(tk=_hip.ROWS_MSG, ts=24), b"truth_stride"), (dict(tk=T, ts=13, bodies=one, nb=1), b"truth_stride"),
            (dict(n_sets=0), b"n_sets"), (dict(n_sets=65, ss=250), b"n_sets"), (dict(n_sets=2, ss=249), b"set_stride"), (dict(n_sets=2, ss=0), b"set_stride"),
            (dict(kind=T, rs=14), b"bodies_host"), (dict(tk=T, ts=14), b"bodies_host"),
            (dict(kind=T, rs=14, bodies=np.zeros((2, 9)), nb=2), b"n_bodies"), (dict(tk=T, ts=14, bodies=one, nb=0), b"n_bodies"),
            (dict(min_swing=-1e-9), b"min_swing"), (dict(min_swing=np.pi / 2), b"min_swing"), (dict(min_swing=float("nan")), b"min_swing"),
            (dict(min_swing=float("inf")), b"min_swing"),
            (dict(angles="rows"), b"alias"), (dict(errors="truth"), b"alias"), (dict(acc="rows"), b"alias"), (dict(acc="truth"), b"alias"),
            (dict(errors="angles"), b"alias"), (dict(acc="angles"), b"alias"), (dict(acc="errors"), b"alias")]


def call_entry(ptrs, layout=0, rows="rows", kind=0, rs=25, rd=None, n_sets=1, ss=0, truth="truth", tk=1, ts=21, td=None, lags=None, F=10,
               starts=(0, 3, 7), skip=0, bodies=None, nb=0, min_swing=0.05, angles="angles", errors="errors", od=None, acc="acc", R=None,
               stream=None):
    """ape_joint_angles with the named pointers of `ptrs` (an output named after another buffer aliases it)"""
    from wear_mocap_ape_amd import _hip
    f64 = _hip.F64
    st = np.ascontiguousarray(starts, dtype=np.int32)
    b = None if bodies is None else np.ascontiguousarray(bodies, dtype=np.float64)
    lg = None if lags is None else np.ascontiguousarray(lags, dtype=np.int32)
    p = lambda name: None if name is None else ptrs[name]    # noqa: E731
    return _hip.lib().ape_joint_angles(layout, p(rows), kind, rs, f64 if rd is None else rd, n_sets, ss, p(truth), tk, ts, f64 if td is None else td,
                                       None if lg is None else C.c_void_p(lg.ctypes.data), F, C.c_void_p(st.ctypes.data) if len(st) else None,
                                       len(st) if R is None else R, skip, None if b is None else C.c_void_p(b.ctypes.data), nb, min_swing,
                                       p(angles), p(errors), f64 if od is None else od, p(acc), stream)


def test_refusals_are_made_on_the_host():
    """APE_ERR_INVALID_ARG before any device call (the pointers are never read)"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    ptrs = {name: C.c_void_p(4096 * (k + 1)) for k, name in enumerate(("rows", "truth", "angles", "errors", "acc"))}
    for kw, what in refusals():
        rc = call_entry(ptrs, **kw)
        assert rc == 1, (kw, rc)                            # APE_ERR_INVALID_ARG
        assert what in lib.ape_last_error() and b"joint_angles" in lib.ape_last_error(), (kw, lib.ape_last_error())
