"""lstm_cluster32.hip, long-window steady-state sections with their gather pieces issued without a branch and the flag raised by one
buffer store (profiles/r10_cluster32_hot_gaps.md): the change is bit-identical by construction, so

1. the outputs equal, bit for bit, those the library of the commit in front of the change gave on an MI355X
   (tests/golden/c32_hot_gaps_parent.npz: the float32 rows and the seeds they came from), and
2. a library whose judges read "not yet" in every third steady-state phase (lib/diag/libape_hip_c32late.so, -DAPE_C32_LATE_EVERY=3:
   the early copy is then stale and the blocking path refills the block) gives the product library's outputs, with a clean status word.
   In a normal run that path is taken 0.05-2 times per 1024 x 64 launch, never in a test of this size."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests.test_hip_parity import _synthetic_windows

# (model, B, T, weight seed, input seed).  T = 9 is the shortest window of the long-window instantiation with steady-state phases (ph in 2 .. T - 3).
# The planner gives lstm_cluster32.hip calls of 513 rows and more (ape_plan.h, rest_kernel), so the shapes the change was specified with --
# (40, 9), (40, 13), (64, 24), watch (40, 13): a last cluster with 8 live rows -- run it 512 rows further up: 552 = 17 clusters + 8 live rows
# of the 18th, 576 = 18 whole clusters.  The small shapes themselves stay in the list: they take the first-generation kernel, as they did on the
# parent commit (whose kernel names the golden file holds), and must not move either.
BIG = [("pocket", 552, 9, 3, 31), ("pocket", 552, 13, 3, 32), ("pocket", 576, 24, 3, 33), ("watch", 552, 13, 4, 34)]
SMALL = [("pocket", 40, 9, 3, 31), ("pocket", 40, 13, 3, 32), ("pocket", 64, 24, 3, 33), ("watch", 40, 13, 4, 34)]
CASES = BIG + SMALL
LATE_CASES = [c for c in BIG if c[0] == "pocket" and c[2] in (13, 24)]
KERNEL = "ape_lstm_cluster32<256, 2, 32, false>"


def case_id(case):
    return f"{case[0]}_{case[1]}x{case[2]}"


def norm_stats_of(name):
    import json
    from tests.conftest import GOLDEN
    raw = json.loads((GOLDEN / "norm_stats.json").read_text())[name]
    return {k: np.array(raw[k]) for k in ("xx_m", "xx_s", "yy_m", "yy_s")}


def run_case(case, with_model=False):
    """last-step targets of the case on whatever library the process has loaded: (y, kernel name[, model]); model.check() has passed"""
    from wear_mocap_ape_amd.estimate import nn_models
    name, B, T, wseed, xseed = case
    cfg, st = orc.MODEL_CONFIGS[name], norm_stats_of(name)
    m = nn_models.DropoutLSTM(cfg["I"], cfg["H"], cfg["L"], cfg["O"], dropout=0.2, device=0)
    m.load_state_dict(orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], wseed))
    m.set_norm_stats(st["xx_m"], st["xx_s"], st["yy_m"], st["yy_s"])
    x = _synthetic_windows(st, B, T, cfg["I"], xseed)
    m.set_kernel("cluster")
    kernel = m.kernel_name(B, T)
    y = m(torch.from_numpy(x).cuda(), last_step_only=True, normalize_input=True).cpu().numpy()[:, 0]
    m.check()                                             # raises on a non-zero status word
    y = np.ascontiguousarray(y, dtype=np.float32)
    return (y, kernel, m) if with_model else (y, kernel)


def late_phases(T, every=3):
    """steady-state phases (2 .. T - 3) in which the judges of the late-judge library read 'not yet'"""
    return sum(1 for ph in range(2, T - 2) if ph % every == 0)


@pytest.fixture(scope="module")
def product_outputs():
    return {case_id(c): run_case(c) for c in CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bit_equal_to_the_parent_commit(golden, product_outputs, case):
    g = golden("c32_hot_gaps_parent.npz")
    y, kernel = product_outputs[case_id(case)]
    assert kernel == str(g["kernel_" + case_id(case)])
    assert kernel == KERNEL or case in SMALL
    assert list(g["seeds_" + case_id(case)]) == [case[3], case[4]]
    want = g["y_" + case_id(case)]
    assert y.shape == want.shape and y.dtype == want.dtype
    assert np.isfinite(y).all()
    assert np.array_equal(y, want), f"max |diff| {np.abs(y - want).max():.3e}"


@pytest.mark.gpu
def test_failed_judges_refill_by_the_blocking_path(product_outputs, tmp_path):
    from tests.conftest import REPO
    lib = REPO / "arm-pose-estimation_amd" / "lib" / "diag" / "libape_hip_c32late.so"
    assert lib.exists(), "make -C arm-pose-estimation_amd/csrc c32late"
    torch.cuda.synchronize()
    out = tmp_path / "late.npz"
    env = dict(os.environ, APE_HIP_LIB=str(lib))
    r = subprocess.run([sys.executable, str(REPO / "tests" / "hooks" / "c32_late_cases.py"), str(out)], env=env, cwd=str(REPO),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    late = np.load(out, allow_pickle=False)
    for c in LATE_CASES:
        y, _ = product_outputs[case_id(c)]
        assert str(late["kernel_" + case_id(c)]) == KERNEL
        assert np.array_equal(late["y_" + case_id(c)], y), case_id(c)
        # the path was really taken: every workgroup's wave 0 counted a blocking gather per late phase, for both layers (layer 0: + the pipeline fill)
        blocked = late["blocked_" + case_id(c)]
        assert blocked.shape[0] >= 8 and (blocked >= late_phases(c[2])).all(), blocked.min(axis=0)
        # ... and only then: layer 1's own gather is otherwise prefetched (a judge that reads "not yet" in EVERY phase gives the same outputs, slowly)
        assert np.median(blocked[:, 1]) == late_phases(c[2]), np.median(blocked[:, 1])
