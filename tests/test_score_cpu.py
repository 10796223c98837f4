"""Scoring against ground truth without a GPU: the constants of the C ABI and the binding, the numpy statement
`score.score_rows_numpy` on constructed cases with known answers, `summarise` / `merge` on split recordings, the refusals of
`ape_score_rows` (all made on the host), and the truth FK of the fixtures the device test scores against."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import ape_oracle as orc

REPO = Path(__file__).resolve().parents[1]
HIPS, WATCH, POS = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def _quat_about(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def _pose(layout, n, rng):
    """n finite est rows of the layout with unit quaternions and the messages that state exactly these poses"""
    W = 14 if layout == WATCH else 21
    est = rng.normal(size=(n, W))
    qc = (6, 10) if layout == WATCH else (9, 13, 17)
    for c in qc:
        est[:, c:c + 4] /= np.linalg.norm(est[:, c:c + 4], axis=1, keepdims=True)
    msg = np.zeros((n, 25))
    msg[:, 21] = 1.0
    msg[:, 4:7], msg[:, 11:14], msg[:, 18:21] = est[:, 0:3], est[:, 3:6], rng.normal(size=(n, 3))
    for k, c in enumerate(qc):
        msg[:, 7 + 7 * k:11 + 7 * k] = est[:, c:c + 4]
    msg[:, 0:4] = msg[:, 7:11]
    return est, msg


def test_header_constants_and_binding():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    assert re.search(r"^#define APE_SCORE_WIDTH 7\s*$", text, flags=re.M)
    assert re.search(r"^#define APE_SCORE_ACC_WIDTH 25\s*$", text, flags=re.M)
    assert re.search(r"^enum \{ APE_TRUTH_TARGETS = 0, APE_TRUTH_EST = 1 \};", text, flags=re.M)
    assert re.search(r"^int ape_score_rows\(int32_t layout, const void\* msg_dev, int32_t msg_stride,", text, flags=re.M)
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M)
    assert _hip.lib().ape_abi_version() == 7
    assert (_hip.SCORE_WIDTH, _hip.SCORE_ACC_WIDTH, _hip.TRUTH_TARGETS, _hip.TRUTH_EST) == (7, 25, 0, 1)
    assert "ape_score_rows" in _hip.SIGNATURES and hasattr(_hip.lib(), "ape_score_rows")
    assert len(_hip.SIGNATURES["ape_score_rows"][1]) == 19
    assert (score.CHI2_3_Q50, score.CHI2_3_Q90) == (2.3659738843753377, 6.251388631170325)
    assert "2.3659738843753377" in text and "6.251388631170325" in text and "NO counterpart" in text


@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_identical_poses_are_exact_zeros(layout):
    from wear_mocap_ape_amd.score import score_rows_numpy
    est, msg = _pose(layout, 9, np.random.default_rng(1))
    s = score_rows_numpy(msg, est, layout)
    assert s.shape == (9, 7) and not s[:, :5].any() and np.isnan(s[:, 5:]).all()
    # ... whatever the sign the truth's quaternions come in
    for c in ((6, 10) if layout == WATCH else (9, 13, 17)):
        est[::2, c:c + 4] *= -1.0
    assert not score_rows_numpy(msg, est, layout)[:, :5].any()


@pytest.mark.parametrize("angle", [1e-9, 1e-3, 1.0, 3.1])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_rotation_of_known_angle(angle, sign):
    """q = q_t rotated by `angle` about a random axis: the error is the angle, to 1e-15 + 1e-7 relative (normalising the float64
    quaternion of a 1e-9 rad rotation costs ~3e-8 relative)"""
    from wear_mocap_ape_amd.score import score_rows_numpy
    rng = np.random.default_rng(int(angle * 1000) + 7)
    for layout in (HIPS, WATCH, POS):
        est, msg = _pose(layout, 6, rng)
        qc = (6, 10) if layout == WATCH else (9, 13, 17)
        for i in range(6):
            for k, c in enumerate(qc):
                msg[i, 7 + 7 * k:11 + 7 * k] = _qmul(_quat_about(rng.normal(size=3), angle), est[i, c:c + 4])
                est[i, c:c + 4] *= sign
        s = score_rows_numpy(msg, est, layout)
        cols = s[:, 2:2 + len(qc)]
        assert np.abs(cols - angle).max() <= 1e-15 + 1e-7 * angle, (layout, angle, sign, cols)
        assert not s[:, 0:2].any()
        if layout == WATCH:
            assert not s[:, 4].any()


def test_position_errors_and_watch_only_column():
    from wear_mocap_ape_amd.score import score_rows_numpy
    est, msg = _pose(WATCH, 4, np.random.default_rng(2))
    msg[:, 4:7] += [3.0, 4.0, 0.0]
    msg[:, 11:14] -= [0.0, 0.0, 0.5]
    msg[:, 21:25] = [0.5, 0.5, 0.5, 0.5]                   # no hips in this layout: never compared
    s = score_rows_numpy(msg, est, WATCH)
    assert np.abs(s[:, 0] - 5.0).max() < 1e-14 and np.abs(s[:, 1] - 0.5).max() < 1e-15
    assert (s[:, 4] == 0.0).all() and not np.signbit(s[:, 4]).any()


def test_mahalanobis_columns():
    from wear_mocap_ape_amd.score import score_rows_numpy
    rng = np.random.default_rng(4)
    est, msg = _pose(HIPS, 8, rng)
    rec = np.zeros((8, 21))
    off_h, off_e = np.array([0.1, -0.2, 0.3]), np.array([-0.05, 0.0, 0.02])
    rec[:, 0:3], rec[:, 9:12] = est[:, 0:3] - off_h, est[:, 3:6] - off_e
    var_h, var_e = np.array([0.04, 0.01, 0.09]), np.array([0.0025, 1.0, 0.0004])
    rec[:, [3, 6, 8]], rec[:, [12, 15, 17]] = var_h, var_e
    s = score_rows_numpy(msg, est, HIPS, spread=rec)
    d2_h, d2_e = float((off_h ** 2 / var_h).sum()), float((off_e ** 2 / var_e).sum())     # 0.25 + 4 + 1, 1 + 0 + 1
    assert np.abs(s[:, 5] - d2_h).max() <= 1e-13 * d2_h and np.abs(s[:, 6] - d2_e).max() <= 1e-13 * d2_e
    # a full covariance A A' / N against numpy's inverse
    A = rng.normal(size=(3, 5))
    S = A @ A.T / 5
    rec[:, 3:9] = S[np.triu_indices(3)]
    s = score_rows_numpy(msg, est, HIPS, spread=rec)
    ref = off_h @ np.linalg.inv(S) @ off_h
    assert np.abs(s[:, 5] - ref).max() <= 1e-9 * ref
    # N = 1 records (exact zeros), rank 1, rank 2, a NaN entry, a negative-definite matrix: not usable
    rec[0, 3:9] = 0.0
    u = rng.normal(size=3)
    rec[1, 3:9] = np.outer(u, u)[np.triu_indices(3)]
    B = rng.normal(size=(3, 2))
    rec[2, 3:9] = (B @ B.T / 2)[np.triu_indices(3)]
    rec[3, 5] = np.nan
    rec[4, 3:9] = -S[np.triu_indices(3)]
    s = score_rows_numpy(msg, est, HIPS, spread=rec)
    assert np.isnan(s[:5, 5]).all() and np.isfinite(s[5:, 5]).all() and np.isfinite(s[:, 6]).all() and np.isfinite(s[:, :5]).all()


def test_gaps_give_nan_rows():
    from wear_mocap_ape_amd.score import score_rows_numpy
    est, msg = _pose(POS, 6, np.random.default_rng(5))
    rec = np.zeros((6, 21))
    rec[:, [3, 6, 8, 12, 15, 17]] = 1.0
    est[1, 10] = np.nan                                    # a truth quaternion
    est[2, 4] = np.inf                                     # the truth elbow
    msg[3, 0] = np.nan                                     # a message value the errors never read: still all 25 must be finite
    est[4, 7] = np.nan                                     # the truth's shoulder origin: not used
    s = score_rows_numpy(msg, est, POS, spread=rec)
    assert np.isnan(s[[1, 2, 3]]).all() and np.isfinite(s[[0, 4, 5]]).all()


def test_summarise_and_merge_on_split_recordings():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(6)
    F, starts = 500, [0, 137]
    est, msg = _pose(HIPS, F, rng)
    msg[:, 4:7] += 0.05 * rng.normal(size=(F, 3))
    msg[:, 11:14] += 0.03 * rng.normal(size=(F, 3))
    for k, c in enumerate((9, 13, 17)):
        for i in range(F):
            msg[i, 7 + 7 * k:11 + 7 * k] = _qmul(_quat_about(rng.normal(size=3), abs(rng.normal()) * 0.1), est[i, c:c + 4])
    rec = np.zeros((F, 21))
    rec[:, 0:3], rec[:, 9:12] = msg[:, 4:7], msg[:, 11:14]
    rec[:, [3, 6, 8]], rec[:, [12, 15, 17]] = 0.05 ** 2, 0.03 ** 2
    rec[40:60, 3:9] = 0.0
    est[rng.choice(F, 30, replace=False), 0] = np.nan
    s = score.score_rows_numpy(msg, est, HIPS, spread=rec)
    whole = score.accumulate_numpy(s, starts, skip=5)
    assert whole[0, 15] + whole[0, 16] == 137 - 5 and whole[1, 15] + whole[1, 16] == F - 137 - 5
    # each recording cut in two: the second piece continues it, so nothing is skipped there
    a = score.accumulate_numpy(np.r_[s[0:70], s[137:300]], [0, 70], skip=5)
    b = score.accumulate_numpy(np.r_[s[70:137], s[300:]], [0, 67], skip=0)
    m = score.merge(a, b)
    counts = [15, 16, 17, 19, 20, 21, 23, 24]
    maxima = [2, 5, 8, 11, 14]
    assert np.array_equal(m[:, counts], whole[:, counts]) and np.array_equal(m[:, maxima], whole[:, maxima])
    sums = [c for c in range(25) if c not in counts + maxima]
    assert (np.abs(m[:, sums] - whole[:, sums]) <= 4 * 2.0 ** -53 * np.abs(whole[:, sums])).all()
    out = score.summarise(whole)
    assert len(out) == 2
    for r, d in enumerate(out):
        lo, hi = starts[r] + 5, (starts + [F])[r + 1]
        good = s[lo:hi][np.isfinite(s[lo:hi, 0])]
        assert d["scored"] == good.shape[0] and d["unscored"] == hi - lo - good.shape[0]
        for c, name in enumerate(score.ERROR_NAMES):
            assert np.isclose(d["mean"][name], good[:, c].mean(), rtol=1e-12) and d["max"][name] == good[:, c].max()
            assert np.isclose(d["rms"][name], np.sqrt((good[:, c] ** 2).mean()), rtol=1e-12)
        d2 = good[:, 5][np.isfinite(good[:, 5])]
        assert d["hand"]["frames"] == d2.shape[0] and np.isclose(d["hand"]["mean_d2"], d2.mean(), rtol=1e-12)
        assert d["hand"]["coverage90"] == (d2 <= score.CHI2_3_Q90).mean() and d["hand"]["coverage50"] == (d2 <= score.CHI2_3_Q50).mean()
    # honest 3-D Gaussians: the 90 % region holds about 90 % of the frames
    assert abs(out[1]["hand"]["coverage90"] - 0.9) < 0.06 and abs(out[1]["elbow"]["coverage50"] - 0.5) < 0.1
    empty = score.summarise(np.zeros((1, 25)))[0]
    assert empty["scored"] == 0 and np.isnan(empty["mean"]["hand_pos"]) and np.isnan(empty["hand"]["coverage90"])
    with pytest.raises(UserWarning):
        score.merge(np.zeros((2, 25)), np.zeros((1, 25)))


def test_refusals_are_made_on_the_host():
    """every refusal of include/ape_hip.h: non-zero, APE_ERR_INVALID_ARG, before any device call (the pointers are never read)"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)
    body = np.zeros((3, 9))

    def call(layout=0, msg=dummy, ms=25, spread=dummy, ss=21, md=_hip.F64, truth=dummy, kind=0, td=_hip.F64, F=10, starts=(0, 3, 7),
             skip=0, bodies=body, nb=1, score=dummy, sd=_hip.F64, acc=dummy, R=None):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        return lib.ape_score_rows(layout, msg, ms, spread, ss, md, truth, kind, td, F, C.c_void_p(st.ctypes.data) if len(st) else None,
                                  len(st) if R is None else R, skip, C.c_void_p(bodies.ctypes.data) if bodies is not None else None, nb, score,
                                  sd, acc, None)

    bad = [(dict(msg=None), b"NULL"), (dict(truth=None), b"NULL"), (dict(score=None, acc=None), b"both NULL"), (dict(F=0), b"F=0"),
           (dict(starts=()), b"NULL"), (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"),
           (dict(starts=(0, 10)), b"seg_starts[1]"), (dict(ms=24), b"msg_stride"), (dict(ss=20), b"spread_stride"),
           (dict(skip=-1), b"skip"), (dict(nb=2), b"n_bodies"), (dict(nb=0), b"n_bodies"), (dict(bodies=None), b"NULL"),
           (dict(layout=_hip.LAYOUT_NONE), b"layout"), (dict(layout=3), b"layout"), (dict(kind=2), b"truth kind"),
           (dict(md=2), b"dtype"), (dict(td=-1), b"dtype"), (dict(sd=7), b"dtype"),
           # R < 1 beside a valid starts pointer (the NULL check does not catch these), and more recordings than frames
           (dict(R=0), b"recording starts"), (dict(R=-1), b"recording starts"), (dict(R=11), b"recording starts")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)                            # APE_ERR_INVALID_ARG
        assert what in lib.ape_last_error(), (kw, lib.ape_last_error())


def _msgs_from_est(est, layout):
    qc = (6, 10) if layout == WATCH else (9, 13, 17)
    m = np.zeros((est.shape[0], 25))
    m[:, 21] = 1.0
    m[:, 4:7], m[:, 11:14] = est[:, 0:3], est[:, 3:6]
    for k, c in enumerate(qc):
        m[:, 7 + 7 * k:11 + 7 * k] = est[:, c:c + 4]
    return m


@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_fixture_truths_scored_by_the_numpy_statement(golden, layout):
    """the device test scores against `preds_*_N300` as targets and `est_*_N300` as est rows; the reference wrote the second from the
    first (arm_pose_from_nn_targets).  In the terms of this feature: messages that state the reference's est rows score, by
    `score_rows_numpy`, <= 1e-13 against the truth the oracle's reference route makes of the targets on every row, while the closed form
    alone -- what the truth FK starts from and then refines -- leaves the rows with nearly parallel 6D columns (0-59) up to 1e-11 off and
    is the same to rounding on rows 60-299: the gap `truth_six_drr_to_quat` closes on the device"""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.score import score_rows_numpy
    g = golden(f"fk_layout{layout}.npz")
    for tag in ("bd", "bo"):
        preds, est, body = g[f"preds_{tag}_N300"], g[f"est_{tag}_N300"], g[f"body_{tag}"]
        assert np.isfinite(preds).all() and np.isfinite(est).all()
        assert preds.shape == (300, _hip.NUM_TARGETS[layout]) and est.shape == (300, _hip.EST_WIDTH[layout])
        msg = _msgs_from_est(est, layout)
        assert not score_rows_numpy(msg, est, layout)[:, :5].any()
        by_ref = score_rows_numpy(msg, orc.arm_pose_from_targets(preds, body, layout, route="eigh"), layout)[:, :5]
        assert by_ref.max() <= 1e-13, (tag, by_ref.max())
        by_closed = score_rows_numpy(msg, orc.arm_pose_from_targets(preds, body, layout, route="closed"), layout)[:, :5]
        assert by_closed[60:].max() <= 1e-13 and 1e-13 < by_closed[:60].max() < 1e-9, (tag, by_closed[60:].max(), by_closed[:60].max())
    assert not np.array_equal(g["body_bd"], g["body_bo"])
