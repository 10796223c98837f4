"""Speed-adaptive offline smoothing without a GPU: the header and the binding of `ape_post_select` and
`ape_select_rungs`, their refusals (all made on the host), the numpy statement `score.select_rungs_numpy` against a brute-force double
loop, `score.post_select_numpy` against `score.post_window_numpy`, and what the feature is for: on a planted trajectory of holds joined by
reaches (shared with tests/test_post_select_gpu.py) a window per frame, chosen from the hand speed under the envelope, beats every fixed
rung of its ladder, overall and inside the holds, and the same choice without the envelope is worse than the best fixed rung.

tests/golden/post_select_planted.npz holds the planted trajectory's selectors and figures as the numpy statements give them
(`record()`); the test below computes them again and compares, and the GPU file holds the device to the same fixture."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import ape_oracle as orc
from tests.test_post_window_cpu import _rot

REPO = Path(__file__).resolve().parents[1]
FIXTURE = REPO / "tests" / "golden" / "post_select_planted.npz"
HIPS, WATCH, POS = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


# ---------------- 1. the C ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_hip_binds_the_entries():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    assert re.search(r"^#define APE_SELECT_MAX_EDGES\s+256\b", text, flags=re.M) and _hip.SELECT_MAX_EDGES == 256 == score.SELECT_MAX_EDGES
    assert re.search(r"^#define APE_SELECT_MAX_SLOPE\s+8\b", text, flags=re.M) and _hip.SELECT_MAX_SLOPE == 8 == score.SELECT_MAX_SLOPE
    assert re.search(r"^int ape_post_select\(ape_model_t\* model, const float\* y_dev, int32_t F, int32_t n_mc,", text, flags=re.M)
    assert re.search(r"^int ape_post_select_last\(int32_t out4\[4\]\);", text, flags=re.M)
    assert re.search(r"^int ape_select_rungs\(const void\* keys_dev, int32_t keys_dtype,", text, flags=re.M)
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    for name, n_args in (("ape_post_select", 18), ("ape_post_select_last", 1), ("ape_select_rungs", 17)):
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name)
        decl = text[text.index(f"int {name}("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert len(decl.split(",")) == len(_hip.SIGNATURES[name][1]) == n_args, name
    for name in ("ladder", "speed_edges", "select_rungs", "select_rungs_numpy", "post_select", "post_select_last", "post_select_plan",
                 "post_select_numpy", "score_selected"):
        assert callable(getattr(score, name))
    mk = (REPO / "arm-pose-estimation_amd" / "csrc" / "Makefile").read_text()
    for name in ("post_select.hip", "select_rungs.hip", "post_window.hip"):
        assert name in mk.split("SRCS", 1)[1].split("\n", 1)[0]
        assert name not in mk.split("HAZARD_SRCS :=", 1)[1].split("\n", 1)[0]
    for name in ("post_window.hip", "post_select.hip", "post_common.h", "select_rungs.hip"):
        src = (REPO / "arm-pose-estimation_amd" / "csrc" / name).read_text()
        assert "asm" not in src and "atomic" not in src and "hipLaunchCooperativeKernel" not in src
        if name != "select_rungs.hip":                      # (integer work alone there)
            assert "#pragma clang fp contract(off)" in src
    # one copy of the pair function, of the conversion kernel and of the driver's loop
    pw = (REPO / "arm-pose-estimation_amd" / "csrc" / "post_window.hip").read_text()
    assert len(re.findall(r"^__device__ __forceinline__ void window_pair\(", pw, flags=re.M)) == 1
    assert pw.count("void ape_post_window_fk_kernel(") == 1 and pw.count("for (int f_lo = 0, c = 0; f_lo < F") == 1
    ps = (REPO / "arm-pose-estimation_amd" / "csrc" / "post_select.hip").read_text()
    assert "__global__" not in ps and "post_filter(" in ps and "post_window_args(" in ps


# ---------------- 2. refusals ---------------------------------------------------------------------------------------------------------------
def test_post_select_refusals_are_made_on_the_host():
    """`ape_post_window`'s refusals under the new name, and the selector's own: before any device call (the pointers are never read)"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)
    body = np.zeros((3, 9))

    def call(y=dummy, F=10, n_mc=6, starts=(0, 3, 7), R=None, windows=((0, 0, 1), (1, 1, 6)), weights=None, Ln=None, sel=dummy, S=2,
             flags=_hip.FLAG_SPREAD, bodies=body, nb=3, out=dummy, dtype=_hip.F64, ws=0, no_windows=False):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        wn = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1, 3)
        wt = None
        if weights is not None:
            wt = np.zeros((len(wn), 64))
            for c, row in enumerate(weights):
                wt[c, :len(row)] = row
        return lib.ape_post_select(None, y, F, n_mc, C.c_void_p(st.ctypes.data) if len(st) else None, len(st) if R is None else R,
                                   None if no_windows else C.c_void_p(wn.ctypes.data), C.c_void_p(wt.ctypes.data) if wt is not None else None,
                                   len(wn) if Ln is None else Ln, sel, S, flags, C.c_void_p(bodies.ctypes.data) if bodies is not None else None,
                                   nb, out, dtype, ws, None)

    many = [(0, 0, 1)] * 65
    third = [1.0 / 3.0] * 3
    bad = [(dict(y=None), b"NULL"), (dict(out=None), b"NULL"), (dict(starts=()), b"NULL"), (dict(no_windows=True), b"NULL"),
           (dict(sel=None), b"NULL selector"), (dict(S=0), b"S=0"), (dict(S=65), b"S=65"), (dict(S=-1), b"S=-1"),
           (dict(F=0), b"F=0"), (dict(R=0), b"recording starts"), (dict(R=11), b"recording starts"),
           (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 10)), b"seg_starts[1]"),
           (dict(n_mc=0), b"n_mc"), (dict(F=2 ** 30, n_mc=2, windows=((0, 0, 1),)), b"2^31"),
           (dict(Ln=0), b"C=0"), (dict(windows=many), b"C=65"),
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
        assert what in lib.ape_last_error() and b"post_select" in lib.ape_last_error(), (kw, lib.ape_last_error())
    # valid arguments, no model: a loud failure (no CPU fallback); with no gfx950 device at all it says so
    ok = [dict(), dict(S=1), dict(S=64), dict(bodies=None, nb=0), dict(nb=1), dict(weights=([1.0], third)),
          dict(flags=0, dtype=_hip.F32, ws=1 << 20, windows=((63, 0, 6), (0, 63, 1), (32, 31, 6)))]
    for kw in ok:
        rc = call(**kw)
        assert rc != 0 and b"model" in lib.ape_last_error() and b"post_select" in lib.ape_last_error(), (kw, lib.ape_last_error())
        if lib.ape_device_count() == 0:
            assert rc == 5                                  # APE_ERR_NO_DEVICE
    assert lib.ape_post_select_last(None) == 1


def test_select_rungs_refusals_are_made_on_the_host():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(4096)
    far = C.c_void_p(1 << 30)

    def call(keys=dummy, dtype=_hip.F64, S=2, ss=100, F=10, fs=1, starts=(0, 3, 7), R=None, edges=(0.1, 0.2, 0.4), B=None,
             ros=(2, 1, 0, 0), nan_rung=2, reach=(0, 2, 5), L=None, slope=2, sel=far):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        e = np.ascontiguousarray(edges, dtype=np.float64)
        rs = np.ascontiguousarray(ros, dtype=np.int32)
        rc = np.ascontiguousarray(reach, dtype=np.int32)
        return lib.ape_select_rungs(keys, dtype, S, ss, F, fs, C.c_void_p(st.ctypes.data) if len(st) else None, len(st) if R is None else R,
                                    C.c_void_p(e.ctypes.data) if len(e) else None, len(e) if B is None else B,
                                    C.c_void_p(rs.ctypes.data) if len(rs) else None, nan_rung, C.c_void_p(rc.ctypes.data) if len(rc) else None,
                                    len(rc) if L is None else L, slope, sel, None)

    bad = [(dict(keys=None), b"NULL"), (dict(sel=None), b"NULL"), (dict(starts=()), b"NULL"), (dict(edges=()), b"NULL"),
           (dict(ros=()), b"NULL"), (dict(reach=()), b"NULL"), (dict(dtype=2), b"dtype"),
           (dict(F=0), b"F=0"), (dict(R=0), b"recording starts"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"),
           (dict(S=0), b"S=0"), (dict(S=65), b"S=65"), (dict(L=0), b"L=0"), (dict(L=65), b"L=65"),
           (dict(B=0), b"B=0"), (dict(B=257), b"B=257"),
           (dict(edges=(0.1, 0.1, 0.4)), b"edges[1]"), (dict(edges=(0.2, 0.1, 0.4)), b"edges[1]"), (dict(edges=(0.1, 0.2, float("nan"))), b"edges[2]"),
           (dict(edges=(0.1, 0.2, float("inf"))), b"edges[2]"),
           (dict(slope=-1), b"slope -1"), (dict(slope=9), b"slope 9"),
           (dict(reach=(0, 3, 2)), b"reach[2] = 2 below reach[1] = 3"), (dict(reach=(0, 2, 64)), b"reach[2] = 64"), (dict(reach=(-1, 2, 5)), b"reach[0] = -1"),
           (dict(ros=(2, 1, 0, 3)), b"rung_of_slot[3] = 3"), (dict(ros=(2, -1, 0, 0)), b"rung_of_slot[1] = -1"),
           (dict(nan_rung=3), b"nan_rung 3"), (dict(nan_rung=-1), b"nan_rung -1"),
           (dict(fs=0), b"frame_stride"), (dict(ss=9), b"set_stride"), (dict(fs=12, ss=108), b"set_stride"),
           (dict(keys=C.c_void_p(4100)), b"aligned"), (dict(keys=C.c_void_p(4098), dtype=_hip.F32), b"aligned"),
           (dict(sel=C.c_void_p(4096 + 500)), b"overlaps")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)
        assert what in lib.ape_last_error() and b"select_rungs" in lib.ape_last_error(), (kw, lib.ape_last_error())
    if lib.ape_device_count() == 0:
        # valid arguments, no device: a loud failure (there is no CPU fallback)
        for kw in (dict(), dict(S=1, ss=0), dict(slope=0), dict(slope=8), dict(reach=(2, 2, 63)), dict(fs=12, ss=109, dtype=_hip.F32),
                   dict(edges=(0.5,), ros=(1, 0), B=1)):
            assert call(**kw) != 0, kw


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
    for call in (lambda: est.repost_selected(np.zeros((4, 1, 14), np.float32), [(1, 1, 1)], np.zeros(4, np.uint8)),
                 lambda: est.smooth_adaptive(np.zeros((4, 55), np.float32)),
                 lambda: est.sweep_adaptive(np.zeros((4, 55), np.float32), None, None, [(3, None, 2)]),
                 lambda: score.post_select(None, np.zeros((4, 1, 14), np.float32), [(1, 1, 1)], np.zeros(4, np.uint8)),
                 lambda: score.select_rungs(np.zeros(4), [0.1], [0, 1]),
                 lambda: score.ladder((0, 2, 1), 4), lambda: score.ladder((), 4), lambda: score.ladder((0, 32), 4),
                 lambda: score._reach([0, 3, 2]), lambda: score._reach([0, 64]), lambda: score._reach([]), lambda: score._reach(list(range(65))),
                 lambda: score.speed_edges(0.0), lambda: score.speed_edges(0.003, 1.0), lambda: score.speed_edges(count=257),
                 lambda: score.select_rungs_numpy(np.zeros(4), [0.2, 0.1], None, [0, 1], 2),
                 lambda: score.select_rungs_numpy(np.zeros(4), [0.1], [0, 2], [0, 1], 2),
                 lambda: score.select_rungs_numpy(np.zeros(4), [0.1], [0], [0, 1], 2),
                 lambda: score.select_rungs_numpy(np.zeros(4), [0.1], None, [0, 1], 9),
                 lambda: score.select_rungs_numpy(np.zeros(4), [0.1], None, [0, 1], 2, nan_rung=2)):
        with pytest.raises(UserWarning):
            call()
    windows, reach = score.ladder((0, 1, 3), 4)
    assert windows[0] == (0, 0, 4, None) and windows[1][:3] == (1, 1, 4) and np.array_equal(windows[1][3], [0.25, 0.5, 0.25])
    assert reach.dtype == np.int32 and reach.tolist() == [0, 1, 3] == score._reach((windows, reach)).tolist() == score._reach(windows).tolist()
    assert score._reach([(2, 0, 1), (1, 5, 1)]).tolist() == [2, 5]
    assert len(score.ladder(samples=25)[0]) == 11 and score.ladder()[1].tolist() == [0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 31]
    assert np.allclose(score.speed_edges(0.003, 1.3, 3), [0.003, 0.0039, 0.00507], rtol=1e-15, atol=0)
    # the default table: slot 0 the widest rung, each further slot one rung narrower, clamped at rung 0
    e, ros, nan_rung, k = score._select_tables([1.0, 2.0, 3.0, 4.0], np.array([0, 1, 2], np.int32), 2, None, None)
    assert ros.tolist() == [2, 1, 0, 0, 0] and nan_rung == 2 and k == 2


# ---------------- 3. the selector's statement against a double loop -------------------------------------------------------------------------
def _brute_select(keys, edges, ros, reach, k, starts, nan_rung):
    F = len(keys)
    ends = list(starts[1:]) + [F]
    r0 = []
    for f in range(F):
        v = keys[f]
        r0.append(nan_rung if not np.isfinite(v) else ros[sum(1 for e in edges if e < v)])
    if k == 0:
        return r0
    sel = []
    for f in range(F):
        rec = max(r for r, a in enumerate(starts) if a <= f)
        cap = min(reach[r0[g]] + abs(f - g) // k for g in range(starts[rec], ends[rec]))
        sel.append(min(r0[f], max(r for r in range(len(reach)) if reach[r] <= cap)))
    return sel


def test_select_rungs_numpy_equals_the_double_loop():
    """recordings of 1, 40, 7 and 72 frames; NaN and infinite keys; keys equal to an edge (right-closed: the lower slot); two rungs of
    equal reach; a table that is not monotone; every slope from none to the largest"""
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(44)
    F, starts = 120, [0, 1, 41, 48]
    edges = np.array([0.5, 1.0, 2.0, 4.0, 8.0])
    for reach, ros, nan_rung in (([0, 1, 2, 4, 8, 16], None, None), ([0, 2, 2, 5, 5, 30], None, 0), ([1, 1, 3, 9], [3, 0, 2, 1, 1, 3], 1),
                                 ([0, 63], [1, 0, 1, 0, 1, 0], None), ([4], None, None)):
        keys = np.exp(rng.normal(0.5, 1.2, size=(2, F)))
        keys[0, [0, 5, 41, 47, 119]] = np.nan
        keys[1, [3, 60]] = [np.inf, -np.inf]
        keys[0, [10, 11, 12]] = [1.0, 2.0, 0.5]             # on an edge: the edge is not strictly below the key
        keys[1, 70:75] = 100.0                              # a burst inside a slow stretch
        keys[1, 80:119] = 0.01
        L = len(reach)
        ros_ = list(np.maximum(L - 1 - np.arange(6), 0)) if ros is None else ros
        nan_ = L - 1 if nan_rung is None else nan_rung
        for k in (0, 1, 2, 3, 8):
            got = score.select_rungs_numpy(keys, edges, ros, reach, k, starts, nan_rung)
            assert got.dtype == np.uint8 and got.shape == (2, F)
            for s in range(2):
                assert got[s].tolist() == _brute_select(keys[s], edges, ros_, reach, k, starts, nan_), (reach, k, s)
            assert np.array_equal(score.select_rungs_numpy(keys[1], edges, ros, reach, k, starts, nan_rung), got[1])      # [F] alone
            assert np.array_equal(score.select_rungs_numpy(keys.astype(np.float32), edges, ros, reach, k, starts, nan_rung),
                                  np.array([_brute_select(keys[s].astype(np.float32), edges, ros_, reach, k, starts, nan_) for s in range(2)]))
    # right-closed bins, stated once more in plain numbers: 1.0 is in (0.5, 1.0], one edge below it
    assert score.select_rungs_numpy(np.array([0.5, 0.75, 1.0, 1.5]), edges, [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], 0).tolist() == [0, 1, 1, 2]
    # the envelope in plain numbers: one fast frame in a hold, reaches 0 .. 5, k = 2 -> the reach grows by one every two frames
    keys = np.full(15, 0.1)
    keys[7] = 100.0
    assert score.select_rungs_numpy(keys, edges, None, [0, 1, 2, 3, 4, 5], 2).tolist() == [3, 3, 2, 2, 1, 1, 0, 0, 0, 1, 1, 2, 2, 3, 3]
    assert score.select_rungs_numpy(keys, edges, None, [0, 1, 2, 3, 4, 5], 2, [0, 8]).tolist() == [3, 3, 2, 2, 1, 1, 0, 0] + [5] * 7


# ---------------- 4. the post-filter's statement --------------------------------------------------------------------------------------------
def test_post_select_numpy_is_the_gather_of_post_window_numpy():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(12)
    F, M, starts = 12, 3, [0, 1, 4]
    windows = [(0, 0, 1), (1, 0, 3), (2, 1, 2), score.window(2, 2, 3, "triangle")]
    y = rng.normal(size=(F, M, 14)).astype(np.float32)
    yy_m, yy_s = np.linspace(-0.1, 0.2, 14), np.linspace(0.5, 1.5, 14)
    bodies = orc.DEFAULT_BODY.reshape(1, 9) * np.array([[1.0], [1.1], [0.9]])
    ref_out, ref_spread = score.post_window_numpy(y, yy_m, yy_s, bodies, HIPS, starts, windows)
    for c in range(len(windows)):
        out, spread = score.post_select_numpy(y, yy_m, yy_s, bodies, HIPS, starts, windows, np.full(F, c))
        assert out.shape == (F, 25) and spread.shape == (F, 21)
        assert np.array_equal(out, ref_out[c]) and np.array_equal(spread, ref_spread[c]), c
    sel = rng.integers(0, len(windows), size=(3, F))
    sel[1, [0, 3, 11]] = [4, 255, 9]                        # no such rung: the row is NaN, every other row is what it was
    out, spread = score.post_select_numpy(y, yy_m, yy_s, bodies, HIPS, starts, (windows, None), sel.astype(np.uint8))
    assert out.shape == (3, F, 25) and spread.shape == (3, F, 21)
    for s in range(3):
        for f in range(F):
            if sel[s, f] >= len(windows):
                assert np.isnan(out[s, f]).all() and np.isnan(spread[s, f]).all()
            else:
                assert np.array_equal(out[s, f], ref_out[sel[s, f], f]) and np.array_equal(spread[s, f], ref_spread[sel[s, f], f])
    with pytest.raises(UserWarning):
        score.post_select_numpy(y, yy_m, yy_s, bodies, HIPS, starts, windows, np.zeros(F + 1, np.uint8))
    assert score.post_select_plan(HIPS, 150, score.ladder((0, 3, 6), 6)) == score.post_window_plan(HIPS, 150, [(0, 0, 6), (3, 3, 6), (6, 6, 6)])


# ---------------- 5. the point of the feature -----------------------------------------------------------------------------------------------
HOLD, REACH = 60, 12
PILOT = 3                                                   # the rung whose hand speed is the key: half-width 3
RULES = ((PILOT, (0.003, 1.3), 1), (PILOT, (0.003, 1.3), 2), (PILOT, (0.003, 1.3), 0))     # (pilot, (first edge [m/frame], ratio), slope)
MARGIN = 2                                                  # interior hold frames: at least this far from a reach


def reach_and_hold(F=432, M=4):
    """holds of 60 frames at random key poses joined by 12-frame smoothstep reaches, and noisy samples of it (noise 0.05 on the targets),
    in the 14-target layout with yy_m = 0, yy_s = 1:
    -> (y float32 [F, M, 14], truth est rows [F, 21] of the clean targets under the default body, interior hold frames bool [F])"""
    rng = np.random.default_rng(7)
    poses = rng.uniform(-1.0, 1.0, size=(F // (HOLD + REACH) + 2, 5)) * np.array([0.9, 0.6, 0.7, 0.5, 0.4])
    ang, hold = np.zeros((F, 5)), np.zeros(F, dtype=bool)
    for f in range(F):
        k, r = divmod(f, HOLD + REACH)
        if r < HOLD:
            ang[f], hold[f] = poses[k], True
        else:
            t = (r - HOLD + 1) / (REACH + 1)
            s = t * t * (3.0 - 2.0 * t)
            ang[f] = (1.0 - s) * poses[k] + s * poses[k + 1]
    clean = np.zeros((F, 14))
    for i in range(F):
        lower, upper = _rot(2, ang[i, 0]) @ _rot(1, ang[i, 1]), _rot(0, ang[i, 2]) @ _rot(2, ang[i, 3])
        clean[i, 0:6], clean[i, 6:12] = lower[:, :2].reshape(-1), upper[:, :2].reshape(-1)     # the first two columns, row-major
        clean[i, 12], clean[i, 13] = np.sin(ang[i, 4]), np.cos(ang[i, 4])
    noisy = clean[:, None, :] + 0.05 * rng.normal(size=(F, M, 14))
    truth = orc.arm_pose_from_targets(clean, orc.DEFAULT_BODY.reshape(1, 9), HIPS, route="closed")
    interior = hold.copy()
    for d in range(1, MARGIN + 1):
        interior[d:] &= hold[:-d]
        interior[:-d] &= hold[d:]
    return noisy.astype(np.float32), truth, interior


def hand_rms_mm(msg, truth, mask=None) -> float:
    """RMS distance [mm] of the message's hand origin (columns 4:7) from the truth's (est columns 0:3), at lag 0, over `mask`'s frames"""
    d = np.asarray(msg, dtype=np.float64)[:, 4:7] - truth[:, 0:3]
    e = (d * d).sum(axis=1)
    return float(1e3 * np.sqrt((e if mask is None else e[mask]).mean()))


def figures_of(fixed_out, adaptive_out, truth, interior) -> np.ndarray:
    """[L + S, 2]: hand RMS [mm] overall and on the interior hold frames, the fixed rungs and then the rules"""
    return np.array([[hand_rms_mm(o, truth), hand_rms_mm(o, truth, interior)] for o in list(fixed_out) + list(adaptive_out)])


@functools.lru_cache(maxsize=1)
def planted_numpy():
    """the planted trajectory through the numpy statements -> (sel uint8 [S, F], figures [L + S, 2])"""
    from wear_mocap_ape_amd import score
    y, truth, interior = reach_and_hold()
    windows, reach = score.ladder(samples=y.shape[1])
    out, _ = score.post_window_numpy(y, np.zeros(14), np.ones(14), orc.DEFAULT_BODY, HIPS, [0], windows)
    sel = np.stack([score.select_rungs_numpy(score.motion_sums_numpy(out[p], HIPS, "msg", [0])[0][:, 0],
                                             score.speed_edges(*e, count=len(reach) - 1), None, reach, k, [0]) for p, e, k in RULES])
    ada = out[sel, np.arange(y.shape[0])]
    return sel, figures_of(out, ada, truth, interior)


def record(path=FIXTURE):
    sel, fig = planted_numpy()
    np.savez_compressed(path, sel=sel, figures=fig)


def test_a_window_per_frame_beats_every_fixed_rung_and_needs_the_envelope():
    from wear_mocap_ape_amd import score
    sel, fig = planted_numpy()
    L = len(score.LADDER_HALVES)
    fixed, (slope1, slope2, bare) = fig[:L], fig[L:]
    print("planted reach-and-hold trajectory, hand RMS at lag 0 [mm] (overall, interior hold frames):")
    for h, row in zip(score.LADDER_HALVES, fixed):
        print(f"  fixed half-width {h:2d}: {row[0]:6.2f} {row[1]:6.2f}")
    for (p, e, k), row, s in zip(RULES, fig[L:], sel):
        print(f"  adaptive, pilot rung {p}, edges {e[0] * 1e3:g} mm/frame x {e[1]:g}, slope {k}: {row[0]:6.2f} {row[1]:6.2f}   rungs used "
              f"{np.bincount(s, minlength=L).tolist()}")
    for rule in (slope1, slope2):
        assert (rule[0] < fixed[:, 0]).all() and (rule[1] < fixed[:, 1]).all(), (rule, fixed)     # strictly below EVERY fixed rung
    assert bare[0] > fixed[:, 0].min() and bare[1] > fixed[:, 1].min()                            # the speed alone is worse than the best fixed
    # ... by a lot: a hold frame next to a reach gets a wide window that covers the reach
    assert bare[0] > 3 * fixed[:, 0].min()
    # the fixture the GPU file holds the device to is what the statements give
    with np.load(FIXTURE) as z:
        assert np.array_equal(z["sel"], sel)
        assert np.allclose(z["figures"], fig, rtol=1e-9, atol=0)
