"""Each recording's heading and frame offset against the truth without a GPU: the numpy statements
`score.frame_sums_numpy` and `score.rotate_rows_numpy`, `score.best_frame` on planted cases, the refusals of `ape_frame_sums` and
`ape_rotate_rows` (all made on the host), the header and the binding.

The planted case: est-kind truth of 1000 frames (random-walk quaternions, the hips a random-walk yaw, positions through the default
body); the messages state the truth turned by g^-1 and delayed by 3 frames, so truth = G . estimate at lag 3.  Tolerances are 100 x what
a float64 prototype of the formulas measured (yaw 7e-15, rotation entries 6e-15): 1e-12.  The builders are shared with
tests/test_frame_fit_gpu.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
HIPS, WATCH, POS = 0, 1, 2
F, LAG, YAW, LAGS = 1000, 3, 0.3, (-8, 8)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


# ---------------- builders (plain numpy, independent of the statements under test) ---------------------------------------------------------
def qmul(a, b):
    w1, x1, y1, z1 = (a[..., k] for k in range(4))
    w2, x2, y2, z2 = (b[..., k] for k in range(4))
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=-1)


def qconj(q):
    return np.asarray(q, dtype=np.float64) * np.array([1.0, -1.0, -1.0, -1.0])


def qmat(q):
    """rotation matrices [..., 3, 3] of unit quaternions, by rotating the basis vectors: q (0, e_k) q*"""
    q = np.asarray(q, dtype=np.float64)
    cols = []
    for k in range(3):
        e = np.zeros(q.shape[:-1] + (4,))
        e[..., 1 + k] = 1.0
        cols.append(qmul(qmul(q, e), qconj(q))[..., 1:])
    return np.stack(cols, axis=-1)


def yaw_quat(psi):
    psi = np.asarray(psi, dtype=np.float64)
    z = np.zeros_like(psi)
    return np.stack([np.cos(psi / 2), z, np.sin(psi / 2), z], axis=-1)


def random_walk_quats(rng, n, step=0.05):
    q = np.empty((n, 4))
    cur = rng.normal(size=4)
    cur /= np.linalg.norm(cur)
    for i in range(n):
        d = np.r_[1.0, step * rng.normal(size=3)]
        cur = qmul(cur, d / np.linalg.norm(d))
        cur /= np.linalg.norm(cur)
        q[i] = cur
    return q


def walk_est(n, layout=HIPS, seed=0):
    """est rows [n, 21 | 14] of a random walk: hand, elbow, (shoulder origin,) lower-arm, upper-arm (and hips) quaternions"""
    from wear_mocap_ape_amd.data_types.bone_map import body9_from_bonemap
    rng = np.random.default_rng(seed)
    body = body9_from_bonemap(None)
    lq, uq = random_walk_quats(rng, n), random_walk_quats(rng, n)
    hq = yaw_quat(np.cumsum(0.03 * rng.normal(size=n))) if layout != WATCH else np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    uo = np.einsum("nab,b->na", qmat(hq), body[6:9])
    elbow = np.einsum("nab,b->na", qmat(uq), body[3:6]) + uo
    hand = np.einsum("nab,b->na", qmat(lq), body[0:3]) + elbow
    if layout == WATCH:
        return np.concatenate([hand, elbow, lq, uq], axis=1)
    return np.concatenate([hand, elbow, uo, lq, uq, hq], axis=1)


def msgs_from_est(est, layout):
    """one message per est row stating that row's pose (compose_msg.py:72-78 columns); without hips: the identity and the default origin"""
    from wear_mocap_ape_amd.data_types.bone_map import body9_from_bonemap
    qc = (6, 10) if layout == WATCH else (9, 13, 17)
    m = np.zeros((est.shape[0], 25))
    m[:, 21] = 1.0
    m[:, 4:7], m[:, 11:14] = est[:, 0:3], est[:, 3:6]
    m[:, 18:21] = body9_from_bonemap(None)[6:9] if layout == WATCH else est[:, 6:9]
    for k, c in enumerate(qc):
        m[:, 7 + 7 * k:11 + 7 * k] = est[:, c:c + 4]
    m[:, 0:4] = m[:, 7:11]
    return m


def turn_est(est, g, layout):
    """est rows turned by the world-side rotation of the unit quaternion g: positions G p, quaternions g (x) q"""
    g = np.asarray(g, dtype=np.float64)
    G = qmat(g)
    out = est.copy()
    for c in ((0, 3) if layout == WATCH else (0, 3, 6)):
        out[:, c:c + 3] = est[:, c:c + 3] @ G.T
    for c in ((6, 10) if layout == WATCH else (9, 13, 17)):
        out[:, c:c + 4] = qmul(g, est[:, c:c + 4])
    return out


def planted(g, lag=LAG, layout=HIPS, n=F, seed=0):
    """(msg [n, 25], truth est rows): msg[f] states g^-1 . truth[f - lag] (the first row again where f - lag leaves the recording)"""
    truth = walk_est(n, layout, seed)
    idx = np.clip(np.arange(n) - lag, 0, n - 1)
    est = turn_est(truth[idx], qconj(g), layout)
    msg = msgs_from_est(est, layout)
    if layout == WATCH:                                    # the no-hips message's identity hips quaternion, turned like the rest of the
        msg[:, 21:25] = qconj(g)                           # estimate (the sums do not read it: the hips block is 0 for this layout)
    return msg, truth


def general_quat():
    g = np.array([0.9, 0.2, -0.3, 0.15])
    return g / np.linalg.norm(g)


# ---------------- 1: declarations ----------------------------------------------------------------------------------------------------------
def test_header_declares_and_hip_binds_both_entries():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    assert re.search(r"^#define APE_FRAME_ACC_WIDTH\s+51\b", text, flags=re.M) and _hip.FRAME_ACC_WIDTH == 51 == score.FRAME_ACC_WIDTH
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    want = {"ape_frame_sums": ["int32_t layout", "const void* msg_dev", "int32_t msg_stride", "int32_t msg_dtype", "const void* truth_dev",
                               "int32_t truth_kind", "int32_t truth_dtype", "int32_t F", "const int32_t* seg_starts_host", "int32_t R",
                               "int32_t skip", "const double* bodies_host", "int32_t n_bodies", "int32_t lag_min", "int32_t lag_max",
                               "const int32_t* rec_lag_host", "double* acc_dev", "void* stream"],
            "ape_rotate_rows": ["int32_t layout", "const void* msg_dev", "int32_t msg_stride", "const void* spread_dev", "int32_t spread_stride",
                                "int32_t msg_dtype", "int32_t F", "const int32_t* seg_starts_host", "int32_t R", "const double* quats_host",
                                "int32_t n_quats", "void* out_dev", "int32_t out_dtype", "void* stream"]}
    for name, params in want.items():
        decl = text[text.index(f"\nint {name}(") + 1:]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        got = [" ".join(p.split()) for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
        assert got == params, (name, got)
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name) and len(_hip.SIGNATURES[name][1]) == len(params)
    for name in ("frame_sums", "frame_sums_numpy", "best_frame", "rotate_rows", "rotate_rows_numpy", "align_frame"):
        assert callable(getattr(score, name))
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    assert "align_recording" in vars(Estimator) and "align_recording" in vars(WatchPhoneUarm) and "align_recording" in vars(WatchPhonePocketKalman)


# ---------------- 2: planted lag and rotation ------------------------------------------------------------------------------------------------
def test_planted_lag_and_yaw_are_found():
    from wear_mocap_ape_amd.score import best_frame, frame_sums_numpy
    msg, truth = planted(yaw_quat(YAW))
    acc = frame_sums_numpy(msg, truth, HIPS, LAGS)
    assert acc.shape == (1, 17, 51) and (acc[0, :, 49] == F - 16).all() and not acc[0, :, 50].any()
    for weights in ((1, 1, 1, 0, 0), (0, 0, 0, 1, 1)):
        b = best_frame(acc, LAGS, "yaw", weights)[0]
        print(f"weights {weights}: lag {b['lag']}, yaw error {abs(b['yaw'] - YAW):.3e}")
        assert b["lag"] == LAG and abs(b["yaw"] - YAW) <= 1e-12 and b["pairs"] == F - 16
        assert np.abs(b["quat"] - yaw_quat(YAW)).max() <= 1e-12 and b["objective"].shape == (17,)
        assert int(np.argmax(b["objective"])) == LAG - LAGS[0]
        for name in ("larm", "uarm", "hips"):
            assert abs(b["mean_cos_after"][name] - 1.0) <= 1e-12 and b["mean_cos_before"][name] < b["mean_cos_after"][name]


def test_planted_general_rotation_is_found_in_full_mode():
    from wear_mocap_ape_amd.score import best_frame, frame_sums_numpy
    g = general_quat()
    msg, truth = planted(g)
    acc = frame_sums_numpy(msg, truth, HIPS, LAGS)
    for weights in ((1, 1, 1, 0, 0), (1, 1, 1, 1, 1), (0, 0, 0, 1, 1)):
        b = best_frame(acc, LAGS, "full", weights)[0]
        worst = np.abs(b["matrix"] - qmat(g)).max()
        print(f"weights {weights}: lag {b['lag']}, max |G - G0| {worst:.3e}")
        assert b["lag"] == LAG and worst <= 1e-12 and b["yaw"] is None
        assert np.abs(b["quat"] - g).max() <= 1e-12 and b["quat"][0] >= 0.0
    # the yaw fit of a general rotation is its best turn about the vertical: a worse objective than the full fit's, never a better one
    assert best_frame(acc, LAGS, "yaw")[0]["objective"].max() < best_frame(acc, LAGS, "full")[0]["objective"].max()


def test_messages_equal_to_the_truth_give_the_identity():
    from wear_mocap_ape_amd.score import best_frame, frame_sums_numpy
    truth = walk_est(F)
    acc = frame_sums_numpy(msgs_from_est(truth, HIPS), truth, HIPS, LAGS)
    for mode in ("yaw", "full"):
        b = best_frame(acc, LAGS, mode)[0]
        assert b["lag"] == 0 and np.abs(b["matrix"] - np.eye(3)).max() <= 1e-14 and np.abs(b["quat"] - [1, 0, 0, 0]).max() <= 1e-14
        for name in ("larm", "uarm", "hips"):
            assert abs(b["mean_cos_before"][name] - 1.0) <= 1e-14 and abs(b["mean_cos_after"][name] - 1.0) <= 1e-14, (mode, name, b)
    assert abs(best_frame(acc, LAGS, "yaw")[0]["yaw"]) <= 1e-14


def test_supports_offsets_and_unusable_pairs():
    """the support is score_lags_numpy's; a pair the scoring would refuse, or with a zero quaternion, moves from [49] to [50]"""
    from wear_mocap_ape_amd.score import best_frame, frame_sums_numpy, score_lags_numpy
    msg, truth = planted(yaw_quat(YAW), n=300)
    starts, lags, skip, offs = [0, 1, 40, 250], (-3, 4), 2, [0, 2, 1, 1]
    msg[60, 5], truth[100, 9], truth[120, 6] = np.nan, np.inf, np.nan                # (truth[120, 6]: the shoulder origin, unused)
    truth[140, 13:17] = 0.0                                                          # a zero quaternion: scored, but its terms are not finite
    acc = frame_sums_numpy(msg, truth, HIPS, lags, starts, skip, offs)
    _, ref = score_lags_numpy(msg, truth, HIPS, lags, starts, skip, None, offs)
    total = ref[:, :, 15] + ref[:, :, 16]
    assert np.array_equal(acc[:, :, 49] + acc[:, :, 50], total) and not acc[0].any() and total[1:].all()
    assert (acc[2, :, 50] == 3).all() and (ref[2, :, 16] == 2).all()                 # frame 60 and truth row 100; row 140 for the sums alone
    assert not acc[1, :, 50].any() and not acc[3, :, 50].any()
    b = best_frame(acc, lags, "yaw", rec_lags=offs)
    assert b[0]["lag"] is None and b[0]["pairs"] == 0 and np.array_equal(b[0]["quat"], [1, 0, 0, 0]) and np.isnan(b[0]["objective"]).all()
    for r in (1, 2, 3):
        assert b[r]["lag"] == LAG and abs(b[r]["yaw"] - YAW) <= 1e-12, (r, b[r])
    for bad in (lambda: best_frame(acc, (-3, 5)), lambda: best_frame(acc, lags, "roll"), lambda: best_frame(acc[:, :, :25], lags),
                lambda: best_frame(acc, lags, weights=(0, 0, 0, 0, 0)), lambda: best_frame(acc, lags, weights=(1, 1, 1)),
                lambda: best_frame(acc, lags, rec_lags=[0, 1])):
        with pytest.raises(UserWarning):
            bad()


def test_ties_go_to_the_smaller_lag_magnitude():
    from wear_mocap_ape_amd.score import best_frame
    acc = np.zeros((1, 5, 51))
    acc[0, :, 49] = 10.0
    for j, s in enumerate([10.0, 9.0, 4.0, 9.0, 10.0]):
        acc[0, j, [0, 4, 8]] = s                            # the lower-arm block s I: objective 3 s at every lag
    assert best_frame(acc, (-2, 2))[0]["lag"] == -2         # |-2| == |2|: the smaller lag
    assert best_frame(acc, (-1, 3))[0]["lag"] == -1
    assert best_frame(acc, (0, 4), rec_lags=[-3])[0]["lag"] == 1     # lags -3 .. 1 tie at -3 and 1


# ---------------- 3: the layout without hips ---------------------------------------------------------------------------------------------------
def test_watch_layout_has_a_zero_hips_block_and_still_finds_the_yaw():
    from wear_mocap_ape_amd.score import best_frame, frame_sums_numpy
    msg, truth = planted(yaw_quat(YAW), layout=WATCH)
    acc = frame_sums_numpy(msg, truth, WATCH, LAGS)
    assert not acc[:, :, 18:27].any() and acc[0, :, 0:18].any()
    b = best_frame(acc, LAGS, "yaw")[0]
    assert b["lag"] == LAG and abs(b["yaw"] - YAW) <= 1e-12 and np.isnan(b["mean_cos_after"]["hips"])
    assert abs(b["mean_cos_after"]["larm"] - 1.0) <= 1e-12 and abs(b["mean_cos_after"]["uarm"] - 1.0) <= 1e-12


# ---------------- 4: the sign of d ---------------------------------------------------------------------------------------------------------------
def test_full_mode_returns_a_rotation_when_u_vt_is_a_reflection():
    from wear_mocap_ape_amd.score import best_frame, frame_sums_numpy
    acc = np.zeros((1, 1, 51))
    acc[0, 0, 49] = 2.0
    acc[0, 0, 0:9] = np.diag([2.0, 1.0, -0.5]).reshape(9)   # U V' = diag(1, 1, -1)
    b = best_frame(acc, (0, 0), "full", (1, 0, 0, 0, 0))[0]
    assert abs(np.linalg.det(b["matrix"]) - 1.0) <= 1e-14 and np.abs(b["matrix"] - np.eye(3)).max() <= 1e-14
    assert abs(b["objective"][0] - 2.5) <= 1e-14            # S0 + S1 - S2
    # from data: truth positions are the mirror image of the message's (no rotation maps one onto the other)
    truth = walk_est(3, seed=4)
    msg = msgs_from_est(truth, HIPS)
    truth[:, [2, 5]] *= -1.0
    acc = frame_sums_numpy(msg, truth, HIPS, (0, 0))
    P = (acc[0, 0, 27:36] + acc[0, 0, 36:45]).reshape(3, 3)
    U, _, Vt = np.linalg.svd(P)
    assert np.linalg.det(U @ Vt) < 0.0
    G = best_frame(acc, (0, 0), "full", (0, 0, 0, 1, 1))[0]["matrix"]
    assert abs(np.linalg.det(G) - 1.0) <= 1e-14 and np.abs(G @ G.T - np.eye(3)).max() <= 1e-14


# ---------------- 5: the rotation statement -----------------------------------------------------------------------------------------------------
def spread_for(msg, seed=3):
    """spread records near the message's origins with well-conditioned covariances D + u u' (condition number < 10)"""
    rng = np.random.default_rng(seed)
    n = msg.shape[0]
    rec = np.zeros((n, 21))
    for o, c in ((0, 4), (9, 11)):
        rec[:, o:o + 3] = msg[:, c:c + 3] + 0.02 * rng.normal(size=(n, 3))
        d, u = 0.01 * rng.uniform(0.5, 2.0, size=(n, 3)), 0.05 * rng.normal(size=(n, 3))
        S = u[:, :, None] * u[:, None, :]
        S[:, [0, 1, 2], [0, 1, 2]] += d
        rec[:, o + 3:o + 9] = S[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    rec[:, 18:21] = rng.uniform(0.01, 0.1, size=(n, 3))
    return rec


def full_cov(six):
    return six[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def test_rotate_rows_statement():
    from wear_mocap_ape_amd.score import rotate_rows_numpy, score_rows_numpy
    n, starts = 200, [0, 50, 51]
    truth = walk_est(n, seed=2)
    rng = np.random.default_rng(8)
    msg = msgs_from_est(walk_est(n, seed=3), HIPS) + 0.0
    msg[:, 0:4] = random_walk_quats(rng, n)
    rec = spread_for(msg)
    gs = np.stack([general_quat(), yaw_quat(-0.7), np.array([0.1, -0.8, 0.3, 0.5])])
    # by hand: positions G p, quaternions g (x) q, covariances G S G'
    out, rot = rotate_rows_numpy(msg, 3.0 * gs, rec, starts)                          # (normalised by the statement)
    unit = gs / np.linalg.norm(gs, axis=1, keepdims=True)
    which = np.searchsorted(starts, np.arange(n), side="right") - 1
    G = qmat(unit[which])
    for c in (0, 7, 14, 21):
        assert np.abs(out[:, c:c + 4] - qmul(unit[which], msg[:, c:c + 4])).max() <= 1e-15
    for c in (4, 11, 18):
        assert np.abs(out[:, c:c + 3] - np.einsum("nab,nb->na", G, msg[:, c:c + 3])).max() <= 1e-15
    for o in (0, 9):
        assert np.abs(rot[:, o:o + 3] - np.einsum("nab,nb->na", G, rec[:, o:o + 3])).max() <= 1e-15
        S = G @ full_cov(rec[:, o + 3:o + 9]) @ np.transpose(G, (0, 2, 1))
        assert np.abs(full_cov(rot[:, o + 3:o + 9]) - S).max() <= 1e-16               # symmetric: the six stored entries state all nine
        assert (np.linalg.eigvalsh(full_cov(rot[:, o + 3:o + 9])) > 0).all()
    assert np.array_equal(rot[:, 18:], rec[:, 18:])
    assert np.array_equal(rotate_rows_numpy(msg, gs, None, starts), rotate_rows_numpy(msg, gs, rec, starts)[0])
    # there and back
    back, rback = rotate_rows_numpy(out, qconj(unit), rot, starts)
    assert np.abs(back - msg).max() <= 1e-14 and np.abs(rback - rec).max() <= 1e-14
    # one quaternion for all recordings; NaN stays in its row
    one = rotate_rows_numpy(msg, gs[1], None, starts)
    assert np.array_equal(one, rotate_rows_numpy(msg, gs[1]))
    msg2 = msg.copy()
    msg2[7, 12] = np.nan
    two = rotate_rows_numpy(msg2, gs[1])
    assert np.isnan(two[7, 11:14]).all() and np.array_equal(np.delete(two, 7, axis=0), np.delete(one, 7, axis=0))
    for bad in (np.zeros(4), np.array([1.0, np.nan, 0, 0]), np.ones((2, 4)), np.ones(3)):
        with pytest.raises(UserWarning):
            rotate_rows_numpy(msg, bad, None, starts)
    # scoring does not see a rotation applied to both sides
    g = general_quat()
    base = score_rows_numpy(msg, truth, HIPS, rec)
    m2, r2 = rotate_rows_numpy(msg, g, rec)
    turned = score_rows_numpy(m2, turn_est(truth, g, HIPS), HIPS, r2)
    assert np.abs(turned[:, :5] - base[:, :5]).max() <= 1e-13
    assert np.isfinite(base[:, 5:]).all() and (np.abs(turned[:, 5:] - base[:, 5:]) / base[:, 5:]).max() <= 1e-9


# ---------------- 6: the C ABI -------------------------------------------------------------------------------------------------------------------
def test_frame_sums_refusals_are_made_on_the_host():
    """every refusal include/ape_hip.h states: APE_ERR_INVALID_ARG before any device call (the pointers are never read)"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)
    body = np.zeros((3, 9))

    def call(layout=0, msg=dummy, ms=25, md=_hip.F64, truth=dummy, kind=0, td=_hip.F64, F=10, starts=(0, 3, 7), skip=0, bodies=body, nb=1,
             lo=-2, hi=2, offs=None, acc=dummy, R=None):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        of = None if offs is None else np.ascontiguousarray(offs, dtype=np.int32)
        return lib.ape_frame_sums(layout, msg, ms, md, truth, kind, td, F, C.c_void_p(st.ctypes.data) if len(st) else None,
                                  len(st) if R is None else R, skip, C.c_void_p(bodies.ctypes.data) if bodies is not None else None, nb,
                                  lo, hi, None if of is None else C.c_void_p(of.ctypes.data), acc, None)

    big = 2 ** 31 - 1
    bad = [(dict(msg=None), b"NULL"), (dict(truth=None), b"NULL"), (dict(acc=None), b"NULL"), (dict(F=0), b"F=0"),
           (dict(starts=()), b"NULL"), (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"),
           (dict(starts=(0, 10)), b"seg_starts[1]"), (dict(ms=24), b"msg_stride"),
           (dict(skip=-1), b"skip"), (dict(nb=2), b"n_bodies"), (dict(nb=0), b"n_bodies"), (dict(bodies=None), b"NULL"),
           (dict(layout=_hip.LAYOUT_NONE), b"layout"), (dict(layout=3), b"layout"), (dict(kind=2), b"truth kind"),
           (dict(md=2), b"dtype"), (dict(td=-1), b"dtype"),
           (dict(R=0), b"recording starts"), (dict(R=-1), b"recording starts"), (dict(R=11), b"recording starts"),
           (dict(lo=1, hi=0), b"lag_min"), (dict(lo=big, hi=-big), b"lag_min"), (dict(lo=0, hi=65), b"66 lags"), (dict(lo=-big, hi=big), b"lags in the sweep"),
           (dict(lo=129, hi=129), b"|lag|"), (dict(lo=-129, hi=-128), b"|lag|"), (dict(lo=100, hi=129), b"|lag|"),
           (dict(offs=(0, 127, 0)), b"recording 1"), (dict(offs=(0, 0, -127)), b"recording 2"), (dict(offs=(big, 0, 0)), b"recording 0"),
           (dict(offs=(0, -big - 1, 0)), b"recording 1"), (dict(lo=0, hi=0, offs=(0, 0, 129)), b"recording 2")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)                            # APE_ERR_INVALID_ARG
        assert what in lib.ape_last_error() and b"frame_sums" in lib.ape_last_error(), (kw, lib.ape_last_error())


def test_rotate_rows_refusals_are_made_on_the_host():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy, other = C.c_void_p(256), C.c_void_p(4096)

    def call(layout=0, msg=dummy, ms=25, spread=None, ss=0, md=_hip.F64, F=10, starts=(0, 3, 7), quats=((1.0, 0, 0, 0),), nq=None,
             out=other, od=_hip.F64, R=None):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        q = None if quats is None else np.ascontiguousarray(quats, dtype=np.float64)
        return lib.ape_rotate_rows(layout, msg, ms, spread, ss, md, F, C.c_void_p(st.ctypes.data) if len(st) else None,
                                   len(st) if R is None else R, None if q is None else C.c_void_p(q.ctypes.data),
                                   (0 if q is None else len(q)) if nq is None else nq, out, od, None)

    unit = (1.0, 0.0, 0.0, 0.0)
    bad = [(dict(msg=None), b"NULL"), (dict(out=None), b"NULL"), (dict(quats=None, nq=1), b"NULL"), (dict(starts=()), b"NULL"),
           (dict(F=0), b"F=0"), (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 10)), b"seg_starts[1]"),
           (dict(R=0), b"recording starts"), (dict(R=11), b"recording starts"),
           (dict(ms=24), b"msg_stride"), (dict(spread=C.c_void_p(512), ss=20), b"spread_stride"),
           (dict(layout=_hip.LAYOUT_NONE), b"layout"), (dict(layout=3), b"layout"), (dict(md=2), b"dtype"), (dict(od=-1), b"dtype"),
           (dict(quats=(unit, unit)), b"n_quats"), (dict(nq=0), b"n_quats"), (dict(quats=(unit,) * 4), b"n_quats"),
           (dict(quats=((0.0, 0, 0, 0),)), b"quaternion 0"), (dict(quats=(unit, (float("nan"), 0, 0, 1), unit)), b"quaternion 1"),
           (dict(quats=(unit, unit, (float("inf"), 0, 0, 0))), b"quaternion 2"),
           (dict(out=dummy), b"aliases"), (dict(spread=other, ss=21), b"aliases")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)                            # APE_ERR_INVALID_ARG
        assert what in lib.ape_last_error() and b"rotate_rows" in lib.ape_last_error(), (kw, lib.ape_last_error())
