"""Post-filter sweep without a GPU: the header and the binding of `ape_post_sweep`, its refusals (all made on the
host), `score.grid`, the numpy statement `post_sweep_numpy` (shared with tests/test_post_sweep_gpu.py) against a plain per-frame loop,
the workspace rule, and the scoring half of `Estimator.sweep_recording` on fabricated accumulators."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import ape_oracle as orc
from tests.test_replay import _seg_of, _stack_msgs

REPO = Path(__file__).resolve().parents[1]
HIPS, WATCH, POS = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def post_sweep_numpy(y, yy_m, yy_s, bodies, layout, starts, configs):
    """The statement of the sweep: y `[F, M, O]` normalised targets -> `(out [C, F, 25], spread [C, F, 21])` float64.  Every sample row
    is de-normalised in float64 and taken through the oracle's closed-form FK with its recording's body (`bodies [1 | R, 9]`) once;
    configuration (smooth, m) is `_stack_msgs` on the first m samples of every frame, its record `_post.spread_rows` of the same stack."""
    from wear_mocap_ape_amd.estimate import _post
    y = np.asarray(y)
    F, M, O = y.shape
    starts = [int(s) for s in starts]
    bodies = np.asarray(bodies, dtype=np.float64).reshape(-1, 9)
    seg = _seg_of(F, starts)
    pred = y.reshape(-1, O).astype(np.float64) * yy_s + yy_m
    E = None
    for r, a in enumerate(starts):
        b = starts[r + 1] if r + 1 < len(starts) else F
        body = bodies[r if bodies.shape[0] > 1 else 0][np.newaxis, :]
        e = orc.arm_pose_from_targets(pred[a * M:b * M], body, layout, route="closed")
        E = np.zeros((F, M, e.shape[1])) if E is None else E
        E[a:b] = e.reshape(b - a, M, -1)
    out, spread = np.zeros((len(configs), F, 25)), np.zeros((len(configs), F, 21))
    for c, (s, m) in enumerate(configs):
        for r, a in enumerate(starts):
            b = starts[r + 1] if r + 1 < len(starts) else F
            body = bodies[r if bodies.shape[0] > 1 else 0][np.newaxis, :]
            out[c, a:b] = _stack_msgs(E[:, :m], seg, s, body, layout, False, range(a, b))
        for f in range(F):
            stack = np.concatenate([E[max(seg[f], f - s + 1 + j), :m] for j in range(s)])
            spread[c, f] = _post.spread_rows(stack, out[c, f], layout)
    return out, spread


# ---------------- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_hip_binds_the_entry():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    assert re.search(r"^#define APE_POST_MAX_CONFIGS\s+64\b", text, flags=re.M) and _hip.POST_MAX_CONFIGS == 64
    assert re.search(r"^int ape_post_sweep\(ape_model_t\* model, const float\* y_dev, int32_t F, int32_t n_mc,", text, flags=re.M)
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    assert "ape_post_sweep" in _hip.SIGNATURES and hasattr(_hip.lib(), "ape_post_sweep")
    decl = text[text.index("int ape_post_sweep("):]
    decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
    assert len(decl.split(",")) == len(_hip.SIGNATURES["ape_post_sweep"][1]) == 15
    for ref in ("estimator.py:108-118,122-137", "compose_msg.py:13-108", "transformations.py:32-51"):
        assert ref in text[text.index("post-filter sweep"):text.index("#define APE_POST_MAX_CONFIGS")], ref
    assert "ape_post_sweep_last" in _hip.SIGNATURES and hasattr(_hip.lib(), "ape_post_sweep_last")
    for name in ("post_sweep", "grid", "post_sweep_plan", "post_sweep_last", "score_configs"):
        assert callable(getattr(score, name))
    mk = (REPO / "arm-pose-estimation_amd" / "csrc" / "Makefile").read_text()
    assert "post_sweep.hip" in mk.split("SRCS", 1)[1].split("\n", 1)[0]
    assert "post_sweep.hip" not in mk.split("HAZARD_SRCS :=", 1)[1].split("\n", 1)[0]
    for name in ("post_sweep.hip", "post_window.hip", "post_common.h"):                         # the front; the kernels it runs
        src = (REPO / "arm-pose-estimation_amd" / "csrc" / name).read_text()
        assert "#pragma clang fp contract(off)" in src and "asm" not in src, name              # contraction off, no inline assembly
        assert "atomic" not in src.replace("No atomics", "") and "hipLaunchCooperativeKernel" not in src, name


def test_refusals_are_made_on_the_host():
    """every refusal include/ape_hip.h states that needs no model: before any device call (the pointers are never read)"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)
    body = np.zeros((3, 9))

    def call(y=dummy, F=10, n_mc=6, starts=(0, 3, 7), R=None, configs=((1, 1), (3, 6)), Cn=None, flags=_hip.FLAG_SPREAD, bodies=body, nb=3,
             out=dummy, dtype=_hip.F64, ws=0, no_configs=False):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        cf = np.ascontiguousarray(configs, dtype=np.int32).reshape(-1, 2)
        return lib.ape_post_sweep(None, y, F, n_mc, C.c_void_p(st.ctypes.data) if len(st) else None, len(st) if R is None else R,
                                  None if no_configs else C.c_void_p(cf.ctypes.data), len(cf) if Cn is None else Cn, flags,
                                  C.c_void_p(bodies.ctypes.data) if bodies is not None else None, nb, out, dtype, ws, None)

    many = [(1, 1)] * 65
    bad = [(dict(y=None), b"NULL"), (dict(out=None), b"NULL"), (dict(starts=()), b"NULL"), (dict(no_configs=True), b"NULL"),
           (dict(F=0), b"F=0"), (dict(R=0), b"recording starts"), (dict(R=-1), b"recording starts"), (dict(R=11), b"recording starts"),
           (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 10)), b"seg_starts[1]"),
           (dict(n_mc=0), b"n_mc"), (dict(F=2 ** 30, n_mc=2, configs=((1, 1),)), b"2^31"),
           (dict(Cn=0), b"C=0"), (dict(Cn=-3), b"C=-3"), (dict(configs=many), b"C=65"),
           (dict(configs=((0, 1),)), b"smooth 0"), (dict(configs=((1, 1), (65, 1))), b"configuration 1: smooth 65"),
           (dict(configs=((1, 0),)), b"0 samples"), (dict(configs=((2, 7),)), b"7 samples"), (dict(configs=((-1, -1),)), b"smooth -1"),
           (dict(n_mc=70, configs=((64, 64), (64, 65))), b"configuration 1: smooth*samples = 4160"),
           (dict(nb=2), b"n_bodies"), (dict(nb=0), b"n_bodies"), (dict(bodies=None, nb=1), b"n_bodies"), (dict(nb=-1), b"n_bodies"),
           (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(flags=_hip.FLAG_PACKED_MSG), b"SPREAD"),
           (dict(flags=_hip.FLAG_SPREAD | _hip.FLAG_NORMALIZE_INPUT), b"SPREAD"), (dict(ws=-1), b"workspace_bytes")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc in (1, 2), (kw, rc)                       # APE_ERR_INVALID_ARG (2^31 rows: APE_ERR_UNSUPPORTED, as ape_replay)
        assert what in lib.ape_last_error() and b"post_sweep" in lib.ape_last_error(), (kw, lib.ape_last_error())
    # valid arguments, no model: a loud failure (no CPU fallback); with no gfx950 device at all it says so
    for kw in (dict(), dict(bodies=None, nb=0), dict(nb=1), dict(flags=0, dtype=_hip.F32, ws=1 << 20, configs=((64, 6), (1, 1)))):
        rc = call(**kw)
        assert rc != 0 and b"model" in lib.ape_last_error(), (kw, lib.ape_last_error())
        if lib.ape_device_count() == 0:
            assert rc == 5                                  # APE_ERR_NO_DEVICE
    assert lib.ape_post_sweep_last(None) == 1


# ---------------- Python: grid, the numpy statement, the workspace rule, the assembly ----------------------------------------------------------
def test_grid_order_and_duplicates():
    from wear_mocap_ape_amd.score import grid
    assert grid([1, 3], [1, 4, 8]) == [(1, 1), (1, 4), (1, 8), (3, 1), (3, 4), (3, 8)]          # smooth-major, the orders given
    assert grid([5, 1, 5], [2, 2, 1]) == [(5, 2), (5, 1), (1, 2), (1, 1)]                         # first occurrence keeps its place
    assert grid([], [1]) == [] and grid([2], []) == []
    assert grid(np.array([1, 3]), (np.int64(2),)) == [(1, 2), (3, 2)] and all(type(v) is int for p in grid(np.array([1]), [np.int32(2)]) for v in p)
    assert len(grid([1, 3, 5, 10, 20], [1, 4, 8, 16, 25])) == 25


def test_numpy_statement_equals_the_plain_loop():
    """12 frames in recordings of 1, 3 and 8 frames, M = 3: every frame of every configuration stacked row by row by the stated rule"""
    from wear_mocap_ape_amd.estimate import _post
    rng = np.random.default_rng(11)
    F, M, starts, configs = 12, 3, [0, 1, 4], [(1, 1), (2, 3), (4, 2)]
    for layout, O in ((HIPS, 14), (WATCH, 12), (POS, 20)):
        y = rng.normal(size=(F, M, O)).astype(np.float32)
        yy_m, yy_s = np.linspace(-0.1, 0.2, O), np.linspace(0.5, 1.5, O)
        bodies = orc.DEFAULT_BODY.reshape(1, 9) * np.array([[1.0], [1.1], [0.9]])
        for bd in (orc.DEFAULT_BODY.reshape(1, 9), bodies):
            out, spread = post_sweep_numpy(y, yy_m, yy_s, bd, layout, starts, configs)
            assert out.shape == (3, F, 25) and spread.shape == (3, F, 21)
            for c, (s, m) in enumerate(configs):
                for f in range(F):
                    rec = max(r for r, a in enumerate(starts) if a <= f)
                    body = bd[rec if len(bd) > 1 else 0][np.newaxis, :]
                    rows = []
                    for i in range(s * m):                  # stack row i: sample i % m of frame max(seg, f - s + 1 + i // m)
                        h, k = max(starts[rec], f - s + 1 + i // m), i % m
                        pred = y[h, k].astype(np.float64) * yy_s + yy_m
                        rows.append(orc.arm_pose_from_targets(pred[np.newaxis, :], body, layout, route="closed")[0])
                    stack = np.array(rows)
                    msg = orc.msg_from_est(stack, body, layout)
                    assert np.array_equal(out[c, f], msg), (layout, c, f)
                    assert np.array_equal(spread[c, f], _post.spread_rows(stack, msg, layout)), (layout, c, f)
            # a one-frame recording and the first frame of any recording: smooth copies of that frame's own samples
            assert np.array_equal(out[1, 0], post_sweep_numpy(y[:1], yy_m, yy_s, bd[:1], layout, [0], [(2, 3)])[0][0, 0])


def test_workspace_rule():
    from wear_mocap_ape_amd.score import post_sweep_plan
    cfg = [(1, 1), (1, 6), (2, 1), (3, 6), (7, 6), (7, 4), (5, 2)]
    assert post_sweep_plan(HIPS, 150, cfg) == {"passes": 1, "chunk_frames": 150, "frame_bytes": 1008, "halo_frames": 6}
    p = post_sweep_plan(HIPS, 150, cfg, 2 * (6 + 30) * 1008)
    assert (p["passes"], p["chunk_frames"]) == (5, 30)
    assert post_sweep_plan(HIPS, 150, cfg, 2 * 7 * 1008)["passes"] == 150                      # one frame per pass: the smallest bound
    with pytest.raises(UserWarning):
        post_sweep_plan(HIPS, 150, cfg, 2 * 7 * 1008 - 1)
    assert post_sweep_plan(WATCH, 10 ** 5, [(10, 25)])["frame_bytes"] == 8 * 14 * 25
    assert post_sweep_plan(HIPS, 10 ** 5, [(20, 25), (1, 1)]) == {"passes": 7, "chunk_frames": (128 << 20) // (2 * 4200) - 19,
                                                                   "frame_bytes": 4200, "halo_frames": 19}


def test_sweep_assembly_on_fabricated_accumulators(monkeypatch):
    """configs -> acc [C, R, L, 25] -> best, with score_lags replaced: configuration c's hand mean squares have their minimum at lag
    c - 1 in recording 0 and at lag 1 - c in recording 1"""
    from wear_mocap_ape_amd import score
    configs, lags, R = [(1, 1), (5, 4), (10, 25)], (-2, 2), 2
    seen = []

    def fake(layout, msg, truth, lags_, truth_kind, spread, starts, skip, bodies, *a, **kw):
        c = int(msg[0])
        seen.append((layout, c, int(spread[0]), truth, lags_, truth_kind, tuple(starts), skip, bodies))
        acc = np.zeros((R, 5, 25))
        acc[:, :, 15] = 10.0
        for r, best in enumerate((c - 1, 1 - c)):
            acc[r, :, 1] = 10.0 * (1.0 + (np.arange(-2, 3) - best) ** 2) * (c + 1)
        return None, acc

    monkeypatch.setattr(score, "score_lags", fake)
    out, spread = np.arange(3)[:, None] * np.ones((3, 4)), 10 + np.arange(3)[:, None] * np.ones((3, 4))
    res = score.score_configs(HIPS, out, spread, "truth", configs, lags, "est", [0, 7], 5, "bodies")
    assert res["configs"] == configs and res["acc"].shape == (3, R, 5, 25) and len(res["best"]) == 3
    assert [s[1] for s in seen] == [0, 1, 2] and [s[2] for s in seen] == [10, 11, 12]          # out[c] with spread[c], in order
    assert all(s[0] == HIPS and s[3:] == ("truth", lags, "est", (0, 7), 5, "bodies") for s in seen)
    for c in range(3):
        assert [b["lag"] for b in res["best"][c]] == [c - 1, 1 - c]
        assert res["best"][c] == score.best_lag(res["acc"][c], lags)
        assert res["best"][c][0]["rms"] == np.sqrt(c + 1.0) and res["best"][c][0]["scored"] == 10
    assert res["acc"][2, 1, 3, 1] == 10.0 * (1.0 + (1 - -1) ** 2) * 3
    for bad in (lambda: score.score_configs(HIPS, out[:2], spread, "t", configs, lags), lambda: score.score_configs(HIPS, out, spread, "t", [], lags),
                lambda: score.score_configs(HIPS, out, spread[:1], "t", configs, lags)):
        with pytest.raises(UserWarning):
            bad()


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
        est.repost(np.zeros((4, 1, 14), np.float32), [(1, 1)])
    with pytest.raises(UserWarning):
        est.sweep_recording(np.zeros((4, 55), np.float32), None, [1], [1])
    with pytest.raises(UserWarning):
        score.post_sweep(None, np.zeros((4, 1, 14), np.float32), [(1, 1)])                 # y is no device tensor
    for cfg in ([], [(1, 1)] * 65, [(1, 2, 3)], "ab"):
        with pytest.raises(UserWarning):
            score._configs(cfg)
