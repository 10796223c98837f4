"""`ape_post_window` gives the bits it gave before the sweep and the window were put behind one kernel and one driver.

The sweep's bits are held by tests/test_score_headers_gpu.py (`post_sweep-*`); this file does the same for the window entry, whose
kernels, plan and host loop every `post_sweep` now runs too.  tests/golden/post_window_parent.npz was recorded from a build of the
commit before the merge by running `cases()` below as it stands (`record()`, with APE_HIP_LIB naming that build's library); each test
runs one case again and compares the raw bytes of every output, NaN payloads included, as tests/test_score_headers_gpu.py does: the
SHA-256 of the whole output and every k-th raw word of it, which says where a difference lies.

Shapes: the smallest at which each path is taken.  F = 150 frames of M = 6 samples in recordings of 1, 39, 57 and 53 frames, so both
clamps act on every row of one recording and the boundaries fall inside windows of both directions.  The mixed call of ten windows
(uniform causal, uniform centred, ahead-only, single frames, Hann, triangle, one-sided Hann, hand-made weights with a zero, a row of
bit-equal weights) runs LDS tiles of 103 frames with the weight table beside them: two tiles, halos across the tile edge.  The same
call under a bound of 53 frames per buffer runs four passes with a carry of H + A = 13 frames.  C = 1 runs the device-rows form;
three uniform windows without a table run on the other two layouts."""
import json
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.test_score_headers_gpu import _noise, kept, words

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
FIXTURE = REPO / "tests" / "golden" / "post_window_parent.npz"

F, M, STARTS = 150, 6, [0, 1, 40, 97]
R = len(STARTS)
HIPS, WATCH, POS = 0, 1, 2
TARGETS = {HIPS: 14, WATCH: 12, POS: 20}
F32, F64 = "float32", "float64"
H, A = 7, 6                                             # the mixed call's longest reach back and ahead
FOUR_PASSES = 2 * 1008 * (H + A + 40)                   # a frame is 6 rows of 21 float64: 40 frames per pass behind a carry of 13


def mixed_windows():
    from wear_mocap_ape_amd import score
    return [(4, 0, 6), (3, 3, 4), (0, 5, 2), (0, 0, 1), (0, 0, 6), score.window(4, 4, 6, "hann"), score.window(2, 6, 3, "triangle"),
            score.window(7, 0, 5, "hann"), score.window(1, 1, 6, [0.5, 0.0, 0.5]), score.window(3, 0, 2, [0.25] * 4)]


# ---- the cases: (id, parameters) -----------------------------------------------------------------------------------------------------------
def cases():
    mixed = {"layout": HIPS, "windows": "mixed", "bodies": True, "spread": True, "out": F64, "bound": 0, "lds": True, "passes": 1}
    single = {"layout": HIPS, "bodies": False, "spread": False, "out": F32, "bound": 0, "lds": False, "passes": 1}
    uniform = {"windows": [(2, 0, 6), (1, 2, 4), (0, 3, 1)], "spread": True, "out": F64, "bound": 0, "lds": True, "passes": 1}
    return [("mixed-lds", dict(mixed, tile_frames=103)),
            ("mixed-four-passes", dict(mixed, bound=FOUR_PASSES, passes=4)),
            ("single-hann", dict(single, windows=[(4, 4, 6, "hann")])),
            ("single-uniform", dict(single, windows=[(9, 0, 6)])),
            ("uniform-watch", dict(uniform, layout=WATCH, bodies=True)),
            ("uniform-position", dict(uniform, layout=POS, bodies=False))]


CASES = cases()


# ---- models and inputs ---------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def model_of(layout):
    """the HIP regressor of a layout: tests/test_post_sweep_gpu.py::pocket, its watch-only counterpart, and the 20-target model of
    tests/test_post_window_gpu.py::test_position_layout_through_the_c_abi (the entry takes layout, output statistics and body)"""
    if not _MODELS:
        from oracle import ape_oracle as orc
        from tests.test_post_sweep_gpu import pocket
        from wear_mocap_ape_amd import _hip
        from wear_mocap_ape_amd.estimate import nn_models
        tmp = tempfile.TemporaryDirectory()
        ests = [pocket(Path(tmp.name), 3, M), pocket(Path(tmp.name), 10, M, name="watch", seed=4)]
        pos = nn_models.DropoutLSTM(22, 256, 2, 20, dropout=0.2, device=0, target_layout=_hip.LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS)
        pos.load_state_dict(orc.make_state_dict(22, 256, 2, 20, seed=4))
        st = json.loads((REPO / "tests" / "golden" / "norm_stats.json").read_text())["pocket"]
        pos.set_norm_stats(np.array(st["xx_m"]), np.array(st["xx_s"]), np.linspace(-0.2, 0.2, 20), np.full(20, 0.3))
        pos.set_body(orc.DEFAULT_BODY)
        _MODELS.update({HIPS: ests[0]._hip_model(), WATCH: ests[1]._hip_model(), POS: pos, "keep": (tmp, ests)})
    return _MODELS[layout]


def inputs(layout):
    """-> (y float32 [F, M, O] with one NaN sample, bodies [R, 9]), from a seed by correctly rounded operations alone"""
    rng = np.random.default_rng(4300 + layout)
    y = (1.7 * _noise(rng, F, M, TARGETS[layout])).astype(np.float32)
    y[60, 2, 3] = np.nan
    bodies = np.array([-0.25, 0.0, 0.0, -0.28, 0.0, 0.0, -0.17, 0.43, -0.03]) + 0.03 * _noise(rng, R, 9)
    return y, bodies


def run_case(p):
    """-> the call's outputs as host arrays (messages, then records)"""
    from wear_mocap_ape_amd import score
    y, bodies = inputs(p["layout"])
    windows = mixed_windows() if p["windows"] == "mixed" else p["windows"]
    got = score.post_window(model_of(p["layout"]), torch.as_tensor(y).cuda(), windows, STARTS, bodies if p["bodies"] else None, p["spread"],
                            getattr(torch, p["out"]), p["bound"])
    last = score.post_window_last()
    assert last["lds"] == p["lds"] and last["passes"] == p["passes"] and last["tile_frames"] == p.get("tile_frames", last["tile_frames"]), last
    torch.cuda.synchronize()
    return [np.ascontiguousarray(g.cpu().numpy()) for g in (got if p["spread"] else [got])]


def record(path=FIXTURE):
    """runs every case on the library in use (APE_HIP_LIB: a build of the parent commit) and writes the fixture"""
    store = {}
    for cid, p in CASES:
        for k, a in enumerate(run_case(p)):
            store[f"{cid}/{k}/sha256"], store[f"{cid}/{k}/words"] = kept(a)
            store[f"{cid}/{k}/shape"] = np.array(a.shape, dtype=np.int64)
    np.savez_compressed(path, **store)
    return len(CASES)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


@pytest.fixture(scope="module")
def parent():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_these_cases(parent):
    assert {k.split("/")[0] for k in parent} == {cid for cid, _ in CASES}
    # the two mixed calls differ in the bound alone, which must not show: already the parent gave one result for both
    for k in (0, 1):
        assert np.array_equal(parent[f"mixed-lds/{k}/sha256"], parent[f"mixed-four-passes/{k}/sha256"])


@pytest.mark.parametrize("cid,p", CASES, ids=[c[0] for c in CASES])
def test_bits_of_the_parent(parent, cid, p):
    got = run_case(p)
    assert len(got) == sum(1 for k in parent if k.startswith(f"{cid}/") and k.endswith("/sha256"))
    for k, a in enumerate(got):
        sha, w = kept(a)
        assert tuple(parent[f"{cid}/{k}/shape"]) == a.shape
        ref = parent[f"{cid}/{k}/words"]
        same = np.array_equal(w, ref)
        where = "" if same else f"first at kept word {int(np.flatnonzero(w != ref)[0])} of {w.shape[0]} (of {words(a).shape[0]} in the output)"
        assert same, f"{cid} output {k}: kept words differ from the parent's, {where}"
        assert np.array_equal(sha, parent[f"{cid}/{k}/sha256"]), f"{cid} output {k}: the kept words agree, the SHA-256 of the whole output does not"
