"""Windowed post-filter without a GPU: the header and the binding of `ape_post_window`, its refusals (all made on the
host), `score.window_weights`, the numpy statement `score.post_window_numpy` against a plain per-frame loop and against the sweep's
statement (tests/test_post_sweep_cpu.py), the workspace rule, and what the feature is for: on a planted trajectory (shared with
tests/test_post_window_gpu.py) a centred window has no lag and a tapered one keeps the curvature a boxcar flattens."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import ape_oracle as orc
from tests.test_post_sweep_cpu import post_sweep_numpy

REPO = Path(__file__).resolve().parents[1]
HIPS, WATCH, POS = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


# ---------------- 1. the C ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_hip_binds_the_entry():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    assert re.search(r"^#define APE_POST_MAX_WINDOW\s+64\b", text, flags=re.M) and _hip.POST_MAX_WINDOW == 64 == score.POST_MAX_WINDOW
    assert re.search(r"^int ape_post_window\(ape_model_t\* model, const float\* y_dev, int32_t F, int32_t n_mc,", text, flags=re.M)
    assert re.search(r"^int ape_post_window_last\(int32_t out4\[4\]\);", text, flags=re.M)
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    for name in ("ape_post_window", "ape_post_window_last"):
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name)
    decl = text[text.index("int ape_post_window("):]
    decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
    assert len(decl.split(",")) == len(_hip.SIGNATURES["ape_post_window"][1]) == 16
    for name in ("window_weights", "window", "post_window", "post_window_last", "post_window_plan", "post_window_numpy", "score_windows"):
        assert callable(getattr(score, name))
    mk = (REPO / "arm-pose-estimation_amd" / "csrc" / "Makefile").read_text()
    assert "post_window.hip" in mk.split("SRCS", 1)[1].split("\n", 1)[0]
    assert "post_window.hip" not in mk.split("HAZARD_SRCS :=", 1)[1].split("\n", 1)[0]
    for name in ("post_window.hip", "post_common.h"):
        src = (REPO / "arm-pose-estimation_amd" / "csrc" / name).read_text()
        assert "#pragma clang fp contract(off)" in src and "asm" not in src                   # contraction off, no inline assembly
        assert "atomic" not in src and "hipLaunchCooperativeKernel" not in src


# ---------------- 2. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_are_made_on_the_host():
    """every refusal include/ape_hip.h states that needs no model: before any device call (the pointers are never read)"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)
    body = np.zeros((3, 9))

    def call(y=dummy, F=10, n_mc=6, starts=(0, 3, 7), R=None, windows=((0, 0, 1), (1, 1, 6)), weights=None, Cn=None, flags=_hip.FLAG_SPREAD,
             bodies=body, nb=3, out=dummy, dtype=_hip.F64, ws=0, no_windows=False):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        wn = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1, 3)
        wt = None
        if weights is not None:
            wt = np.zeros((len(wn), 64))
            for c, row in enumerate(weights):
                wt[c, :len(row)] = row
        return lib.ape_post_window(None, y, F, n_mc, C.c_void_p(st.ctypes.data) if len(st) else None, len(st) if R is None else R,
                                   None if no_windows else C.c_void_p(wn.ctypes.data), C.c_void_p(wt.ctypes.data) if wt is not None else None,
                                   len(wn) if Cn is None else Cn, flags, C.c_void_p(bodies.ctypes.data) if bodies is not None else None, nb,
                                   out, dtype, ws, None)

    many = [(0, 0, 1)] * 65
    third = [1.0 / 3.0] * 3
    bad = [(dict(y=None), b"NULL"), (dict(out=None), b"NULL"), (dict(starts=()), b"NULL"), (dict(no_windows=True), b"NULL"),
           (dict(F=0), b"F=0"), (dict(R=0), b"recording starts"), (dict(R=11), b"recording starts"),
           (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 10)), b"seg_starts[1]"),
           (dict(n_mc=0), b"n_mc"), (dict(F=2 ** 30, n_mc=2, windows=((0, 0, 1),)), b"2^31"),
           (dict(Cn=0), b"C=0"), (dict(windows=many), b"C=65"),
           (dict(windows=((-1, 0, 1),)), b"back -1"), (dict(windows=((0, 0, 1), (0, -1, 1))), b"window 1: ahead -1"),
           (dict(windows=((32, 32, 1),)), b"back + ahead + 1 = 65"), (dict(windows=((64, 0, 1),)), b"back + ahead + 1 = 65"),
           (dict(windows=((1, 1, 0),)), b"0 samples"), (dict(windows=((1, 1, 7),)), b"7 samples"),
           (dict(n_mc=70, windows=((63, 0, 64), (32, 31, 65))), b"window 1: frames*samples = 4160"),
           (dict(weights=([1.0], [0.5, float("nan"), 0.5])), b"window 1: weight 1"), (dict(weights=([1.0], [0.5, float("inf"), 0.5])), b"weight 1"),
           (dict(weights=([1.0], [0.75, -0.25, 0.5])), b"weight 1"), (dict(weights=([1.0], [0.25, 0.125, 0.125])), b"sum to 0.5"),
           (dict(weights=([1.0], [0.5, 0.25, 0.25 + 1e-8])), b"sum to"), (dict(weights=([0.0], third)), b"window 0: weights sum to 0"),
           (dict(nb=2), b"n_bodies"), (dict(nb=0), b"n_bodies"), (dict(bodies=None, nb=1), b"n_bodies"), (dict(nb=-1), b"n_bodies"),
           (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(flags=_hip.FLAG_PACKED_MSG), b"SPREAD"),
           (dict(flags=_hip.FLAG_SPREAD | _hip.FLAG_NORMALIZE_INPUT), b"SPREAD"), (dict(ws=-1), b"workspace_bytes")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc in (1, 2), (kw, rc)                       # APE_ERR_INVALID_ARG (2^31 rows: APE_ERR_UNSUPPORTED, as ape_replay)
        assert what in lib.ape_last_error() and b"post_window" in lib.ape_last_error(), (kw, lib.ape_last_error())
    # valid arguments, no model: a loud failure (no CPU fallback); with no gfx950 device at all it says so
    ok = [dict(), dict(bodies=None, nb=0), dict(nb=1), dict(weights=([1.0], third)), dict(weights=([1.0], [0.5, 0.0, 0.5])),
          dict(weights=([1.0], [0.5, 0.25, 0.25 + 1e-10])), dict(flags=0, dtype=_hip.F32, ws=1 << 20, windows=((63, 0, 6), (0, 63, 1), (32, 31, 6)))]
    for kw in ok:
        rc = call(**kw)
        assert rc != 0 and b"model" in lib.ape_last_error(), (kw, lib.ape_last_error())
        if lib.ape_device_count() == 0:
            assert rc == 5                                  # APE_ERR_NO_DEVICE
    assert lib.ape_post_window_last(None) == 1


def test_python_refusals_without_a_device():
    from wear_mocap_ape_amd import score
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.utility.names import NNS_INPUTS, NNS_TARGETS

    class _NoRegressor(Estimator):
        def parse_row_to_xx(self, row):
            return np.zeros(22, np.float32)

        def make_prediction_from_row_hist(self, xx_hist):
            return np.zeros((1, 14))

    est = _NoRegressor(list(NNS_INPUTS)[0], list(NNS_TARGETS)[0], normalize=False, smooth=2, seq_len=6)
    with pytest.raises(UserWarning):
        est.repost_windows(np.zeros((4, 1, 14), np.float32), [(1, 1, 1)])
    with pytest.raises(UserWarning):
        est.sweep_windows(np.zeros((4, 55), np.float32), None, [(1, 1, 1)])
    with pytest.raises(UserWarning):
        score.post_window(None, np.zeros((4, 1, 14), np.float32), [(1, 1, 1)])              # y is no device tensor
    for bad in ([], [(0, 0, 1)] * 65, [(1, 2)], [(-1, 0, 1)], [(40, 30, 1)], [(1, 1, 1, [0.5, 0.5])], [(1, 1, 1, "boxcar")], 7):
        with pytest.raises(UserWarning):
            score._windows(bad)
    ws, wn, table = score._windows([(2, 0, 4), score.window(1, 1, 2, "hann"), (0, 1, 3, [0.25, 0.75])])
    assert wn.dtype == np.int32 and wn.tolist() == [[2, 0, 4], [1, 1, 2], [0, 1, 3]] and table.shape == (3, 64)
    assert ws[0] == (2, 0, 4, None) and np.array_equal(table[0, :4], [1 / 3, 1 / 3, 1 / 3, 0.0])        # a uniform row: bit-equal entries
    assert np.array_equal(table[1, :4], [0.25, 0.5, 0.25, 0.0]) and np.array_equal(table[2, :3], [0.25, 0.75, 0.0])
    assert score._windows([(2, 0, 4), (0, 0, 1, "uniform")])[2] is None


# ---------------- 3. window_weights ---------------------------------------------------------------------------------------------------------
def test_window_weights():
    from wear_mocap_ape_amd.score import window_weights
    for shape in ("triangle", "hann"):
        for back, ahead in ((0, 0), (1, 0), (2, 2), (4, 4), (8, 8), (5, 1), (1, 5), (8, 0), (0, 8), (31, 32), (63, 0)):
            w = window_weights(shape, back, ahead)
            assert w.dtype == np.float64 and w.shape == (back + ahead + 1,)
            assert abs(float(w.sum()) - 1.0) <= 1e-15, (shape, back, ahead)
            assert (w > 0.0).all() and int(np.argmax(w)) == back, (shape, back, ahead)
            if back == ahead:
                assert np.array_equal(w, w[::-1]), (shape, back)
            assert (np.diff(w[:back + 1]) > 0).all() and (np.diff(w[back:]) < 0).all()          # rising to the frame, falling behind it
        assert window_weights("uniform", 3, 2) is None
    assert np.array_equal(window_weights("triangle", 1, 1), [0.25, 0.5, 0.25]) and np.array_equal(window_weights("hann", 1, 1), [0.25, 0.5, 0.25])
    assert np.allclose(window_weights("triangle", 2, 0), np.array([1.0, 2.0, 3.0]) / 6.0, rtol=0, atol=1e-16)
    for bad in (lambda: window_weights("boxcar", 1, 1), lambda: window_weights("hann", -1, 1), lambda: window_weights("hann", 32, 32)):
        with pytest.raises(UserWarning):
            bad()


# ---------------- 4. the statement against a plain loop -------------------------------------------------------------------------------------
def _plain_tapered(stack, u, body, layout):
    """message and record of a tapered stack, every sum written out row by row"""
    hips = layout != WATCH
    qcols = (9, 13, 17) if hips else (6, 10)
    qs = []
    for c in qcols:
        q = stack[:, c:c + 4]
        a = q[0] * u[0]
        for i in range(1, len(q)):
            a = a + q[i] * (-u[i] if q[i] @ q[0] < 0.0 else u[i])
        qs.append(a / np.sqrt((a * a).sum()))
    lq, uq = qs[0], qs[1]
    hq = qs[2] if hips else np.array([1.0, 0.0, 0.0, 0.0])
    b = body.reshape(9)
    if layout == POS:
        ho, lo, uo = (sum(u[i] * stack[i, k:k + 3] for i in range(len(u))) for k in (0, 3, 6))
    else:
        uo = orc.quat_rotate(hq, b[6:9]) if hips else b[6:9]
        lo = orc.quat_rotate(uq, b[3:6]) + uo
        ho = orc.quat_rotate(lq, b[0:3]) + lo
    msg = np.concatenate([lq, ho, lq, lo, uq, uo, hq])
    rec = np.zeros(21)
    for c0, o0 in ((0, 0), (3, 9)):
        p = stack[:, c0:c0 + 3]
        mean = sum(u[i] * p[i] for i in range(len(u)))
        second = sum(u[i] * np.outer(p[i], p[i]) for i in range(len(u)))
        rec[o0:o0 + 3], rec[o0 + 3:o0 + 9] = mean, (second - np.outer(mean, mean))[np.triu_indices(3)]
    for k, c in enumerate(qcols):
        second = sum(u[i] * np.outer(stack[i, c:c + 4], stack[i, c:c + 4]) for i in range(len(u)))
        rec[18 + k] = 2.0 * np.arcsin(np.sqrt(np.clip(1.0 - qs[k] @ second @ qs[k], 0.0, 1.0)))
    return msg, rec


def test_numpy_statement_equals_the_plain_loop():
    """12 frames in recordings of 1, 3 and 8 frames, M = 3: every frame of every window stacked row by row by the stated rule; the uniform
    windows bit for bit, the tapered one (whose sums the loop takes in another association) within a few ulps"""
    from wear_mocap_ape_amd import score
    from wear_mocap_ape_amd.estimate import _post
    rng = np.random.default_rng(11)
    F, M, starts = 12, 3, [0, 1, 4]
    windows = [(0, 0, 1), (1, 0, 3), (2, 1, 2), (0, 3, 3), score.window(2, 2, 3, "triangle")]
    for layout, O in ((HIPS, 14), (WATCH, 12), (POS, 20)):
        y = rng.normal(size=(F, M, O)).astype(np.float32)
        yy_m, yy_s = np.linspace(-0.1, 0.2, O), np.linspace(0.5, 1.5, O)
        bodies = orc.DEFAULT_BODY.reshape(1, 9) * np.array([[1.0], [1.1], [0.9]])
        for bd in (orc.DEFAULT_BODY.reshape(1, 9), bodies):
            out, spread = score.post_window_numpy(y, yy_m, yy_s, bd, layout, starts, windows)
            assert out.shape == (5, F, 25) and spread.shape == (5, F, 21)
            for c, (back, ahead, m, w) in enumerate(score._windows(windows)[0]):
                n = back + ahead + 1
                for f in range(F):
                    rec = max(r for r, a in enumerate(starts) if a <= f)
                    s, e = starts[rec], starts[rec + 1] if rec + 1 < len(starts) else F
                    body = bd[rec if len(bd) > 1 else 0][np.newaxis, :]
                    rows = []
                    for i in range(n * m):                  # stack row i: sample i % m of frame min(e - 1, max(s, f - back + i // m))
                        h, k = min(e - 1, max(s, f - back + i // m)), i % m
                        pred = y[h, k].astype(np.float64) * yy_s + yy_m
                        rows.append(orc.arm_pose_from_targets(pred[np.newaxis, :], body, layout, route="closed")[0])
                    stack = np.array(rows)
                    if w is None:
                        msg = orc.msg_from_est(stack, body, layout)
                        assert np.array_equal(out[c, f], msg), (layout, c, f)
                        assert np.array_equal(spread[c, f], _post.spread_rows(stack, msg, layout)), (layout, c, f)
                    else:
                        u = np.array([w[i // m] / m for i in range(n * m)])
                        msg, record = _plain_tapered(stack, u, body, layout)
                        assert np.abs(out[c, f] - msg).max() <= 8 * 2.0 ** -52 * max(1.0, np.abs(msg).max()), (layout, c, f)
                        # covariances: differences of sums of magnitude |p|^2; the angle through sqrt of a small difference
                        big = max(1.0, float(np.abs(stack[:, :6]).max()) ** 2)
                        assert np.abs(spread[c, f, :18] - record[:18]).max() <= 16 * n * m * 2.0 ** -53 * big, (layout, c, f)
                        assert np.abs(np.sin(spread[c, f, 18:] / 2) ** 2 - np.sin(record[18:] / 2) ** 2).max() <= 16 * n * m * 2.0 ** -53
            # a one-frame recording: both clamps act on every row, whatever the window
            alone = score.post_window_numpy(y[:1], yy_m, yy_s, bd[:1], layout, [0], windows)[0][:, 0]
            assert np.array_equal(out[1:4, 0], alone[1:4]) and np.array_equal(out[0, 0], alone[0])


# ---------------- 5. identities of the statement --------------------------------------------------------------------------------------------
def test_uniform_windows_are_the_sweep():
    """uniform (s - 1, 0, m) is the sweep's (s, m); uniform (b, a, m) at frame f is the sweep's (b + a + 1, m) at frame f + a wherever
    f + a is a frame of the same recording"""
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(3)
    F, M, starts = 14, 3, [0, 1, 4]
    ends = starts[1:] + [F]
    for layout, O in ((HIPS, 14), (WATCH, 12), (POS, 20)):
        y = rng.normal(size=(F, M, O)).astype(np.float32)
        yy_m, yy_s = np.linspace(-0.1, 0.2, O), np.linspace(0.5, 1.5, O)
        bodies = orc.DEFAULT_BODY.reshape(1, 9) * np.array([[1.0], [1.1], [0.9]])
        configs = [(1, 1), (1, 3), (2, 3), (4, 2), (5, 3)]
        ref_out, ref_spread = post_sweep_numpy(y, yy_m, yy_s, bodies, layout, starts, configs)
        out, spread = score.post_window_numpy(y, yy_m, yy_s, bodies, layout, starts, [(s - 1, 0, m) for s, m in configs])
        assert np.array_equal(out, ref_out) and np.array_equal(spread, ref_spread), layout
        # bit-equal weights are uniform weights
        same = score.post_window_numpy(y, yy_m, yy_s, bodies, layout, starts, [(3, 0, 2, [0.25] * 4), (4, 0, 3, [0.2] * 5)])
        assert np.array_equal(same[0], ref_out[3:5]) and np.array_equal(same[1], ref_spread[3:5])
        shifted = [(1, 2, 2), (0, 3, 2), (2, 2, 3), (0, 4, 3), (0, 1, 3)]
        out, spread = score.post_window_numpy(y, yy_m, yy_s, bodies, layout, starts, shifted)
        for c, (b, a, m) in enumerate(shifted):
            k = configs.index((b + a + 1, m))
            checked = 0
            for s, e in zip(starts, ends):
                for f in range(s, e - a):                   # every f <= e - 1 - a
                    assert np.array_equal(out[c, f], ref_out[k, f + a]) and np.array_equal(spread[c, f], ref_spread[k, f + a]), (layout, c, f)
                    checked += 1
            assert checked == sum(max(0, e - s - a) for s, e in zip(starts, ends)) > 0


# ---------------- 6. the workspace rule -----------------------------------------------------------------------------------------------------
def test_workspace_rule():
    from wear_mocap_ape_amd.score import post_window_plan, window
    win = [(0, 0, 1), (0, 0, 6), (2, 0, 6), (6, 0, 6), (6, 0, 4), (3, 3, 6), (0, 6, 4), (4, 2, 2), window(3, 3, 6, "triangle"), window(5, 1, 6, "hann")]
    assert post_window_plan(HIPS, 150, win) == {"passes": 1, "chunk_frames": 150, "frame_bytes": 1008, "back_frames": 6, "ahead_frames": 6}
    p = post_window_plan(HIPS, 150, win, 2 * (6 + 30 + 6) * 1008)
    assert (p["passes"], p["chunk_frames"]) == (5, 30)
    p = post_window_plan(HIPS, 150, win, 2 * (6 + 30 + 6) * 1008 + 2015)                       # not yet a frame more
    assert (p["passes"], p["chunk_frames"]) == (5, 30)
    assert post_window_plan(HIPS, 150, win, 2 * (6 + 31 + 6) * 1008)["chunk_frames"] == 31
    assert post_window_plan(HIPS, 150, win, 2 * 15 * 1008)["passes"] == 50                     # three frames per pass
    assert post_window_plan(HIPS, 150, win, 2 * 13 * 1008) == {"passes": 150, "chunk_frames": 1, "frame_bytes": 1008, "back_frames": 6,
                                                               "ahead_frames": 6}            # one frame per pass: the smallest bound
    with pytest.raises(UserWarning, match=f"at least {2 * 13 * 1008}"):
        post_window_plan(HIPS, 150, win, 2 * 13 * 1008 - 1)
    assert post_window_plan(WATCH, 10 ** 5, [(5, 4, 25)])["frame_bytes"] == 8 * 14 * 25
    assert post_window_plan(HIPS, 10 ** 5, [(19, 0, 25), (0, 10, 1)]) == {"passes": 7, "chunk_frames": (128 << 20) // (2 * 4200) - 29,
                                                                          "frame_bytes": 4200, "back_frames": 19, "ahead_frames": 10}
    assert post_window_plan(HIPS, 40, [(63, 0, 64), (0, 63, 64)], 2 * 127 * 8 * 21 * 64)["passes"] == 40


# ---------------- 7. the point of the feature -----------------------------------------------------------------------------------------------
def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == 1:
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def planted(F=400, M=4):
    """a smooth arm motion and noisy samples of it, in the 14-target layout with yy_m = 0, yy_s = 1:
    -> (y float32 [F, M, 14], truth est rows [F, 21] of the clean targets under the default body)"""
    t = np.arange(F, dtype=np.float64)
    clean = np.zeros((F, 14))
    for i, x in enumerate(t):
        lower = _rot(2, 0.9 * np.sin(2 * np.pi * x / 97)) @ _rot(1, 0.6 * np.sin(2 * np.pi * x / 61 + 1))
        upper = _rot(0, 0.7 * np.sin(2 * np.pi * x / 83 + 2)) @ _rot(2, 0.5 * np.sin(2 * np.pi * x / 71))
        clean[i, 0:6], clean[i, 6:12] = lower[:, :2].reshape(-1), upper[:, :2].reshape(-1)     # the first two columns, row-major
        h = 0.4 * np.sin(2 * np.pi * x / 131)
        clean[i, 12], clean[i, 13] = np.sin(h), np.cos(h)
    noisy = clean[:, None, :] + 0.05 * np.random.default_rng(5).normal(size=(F, M, 14))
    truth = orc.arm_pose_from_targets(clean, orc.DEFAULT_BODY.reshape(1, 9), HIPS, route="closed")
    return noisy.astype(np.float32), truth


LAGS, SKIP = (-12, 12), 20


def test_a_centred_window_has_no_lag_and_a_taper_keeps_the_curvature():
    from wear_mocap_ape_amd import score
    y, truth = planted()
    M = y.shape[1]
    windows = [(4, 4, M), (8, 0, M), (0, 8, M), (8, 8, M), score.window(8, 8, M, "triangle"), score.window(8, 8, M, "hann")]
    out, _ = score.post_window_numpy(y, np.zeros(14), np.ones(14), orc.DEFAULT_BODY, HIPS, [0], windows)
    best = [score.best_lag(score.score_lags_numpy(out[c], truth, HIPS, LAGS, None, SKIP)[1], LAGS)[0] for c in range(len(windows))]
    centred, causal, ahead, box, tri, hann = best
    print("planted trajectory, hand RMS at lag 0 [mm]:", [round(1e3 * b["rms_lag0"], 2) for b in best], "lags:", [b["lag"] for b in best])
    assert centred["lag"] == 0 and abs(centred["refined"]) < 0.5            # a symmetric filter has no group delay ...
    assert causal["lag"] == 4 and ahead["lag"] == -4                        # ... a boxcar of n frames (n - 1) / 2
    assert centred["rms_lag0"] < causal["rms_lag0"]
    assert hann["rms_lag0"] < tri["rms_lag0"] < box["rms_lag0"]
    assert box["lag"] == tri["lag"] == hann["lag"] == 0
