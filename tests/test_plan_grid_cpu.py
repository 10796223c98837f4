"""CPU tests of the dispatch planner (`csrc/ape_plan.h`, no GPU).

`tests/golden/plan_grid.npz` holds what `ape_debug_plan2`, `ape_debug_bank_route` and `ape_debug_bank_chunks` answered at the last commit
before the planner existed (`tests/golden/gen_plan_grid.py`): every later build reproduces it.  Two groups of rows are NOT reproduced, because the
old debug function ignored `model_kind` and so disagreed with the launches of its own library -- the planner answers what is launched:
  * DropoutFF dims, B <= 4: recorded as the latency cluster kernel; such a model has no LSTM route at all (the MLP kernels serve it);
  * ImuPoseLSTM dims: recorded as a 22-wide 2 x 256 LSTM (latency kernel up to 4 rows, lstm_cluster32.hip above 512); its LSTM reads the
    256-wide input layer, which leaves the first-generation kernel with at most two row tiles and, above 512 windows, the layer-split route.
`tests/tools/plan_sweep.cpp` walks the planner alone, compiled with the host compiler under the address and undefined-behaviour sanitizers."""
import ctypes as C
import importlib.util
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
NONE, GEN1, C32, SMALL, C16, LV16, SPLIT32 = range(7)


@pytest.fixture(scope="module")
def grids():
    """(recorded, what this build answers) over the same axes"""
    import __graft_entry__ as entry
    entry.build()
    from wear_mocap_ape_amd import _hip
    spec = importlib.util.spec_from_file_location("gen_plan_grid", GOLDEN / "gen_plan_grid.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = np.load(GOLDEN / "plan_grid.npz")
    got = gen.record(gen.bind(C.CDLL(str(_hip.LIB_PATH))))
    for axis in ("dims", "n_cus", "rows", "steps", "bank_sizes"):
        assert np.array_equal(want[axis], got[axis]), f"the grid's {axis} axis differs from the recording's"
    return want, got


def test_lstm_plans_reproduce_the_recorded_grid(grids):
    want, got = grids
    names = list(want["dims_names"])
    for name in ("pocket", "watch", "uarm"):
        d = names.index(name)
        bad = np.argwhere((want["plan"][d] != got["plan"][d]).any(axis=-1))
        assert len(bad) == 0, (name, len(bad), [(tuple(i), want["plan"][d][tuple(i)], got["plan"][d][tuple(i)]) for i in bad[:5]])


def test_bank_routes_and_chunks_reproduce_the_recorded_grid(grids):
    want, got = grids
    for key in ("route", "chunks"):
        bad = np.argwhere((want[key] != got[key]).any(axis=-1))
        assert len(bad) == 0, (key, len(bad), [(tuple(i), want[key][tuple(i)], got[key][tuple(i)]) for i in bad[:5]])


def test_other_regressors_are_planned_as_they_are_launched(grids):
    """the two groups of rows of the module docstring: equal to the recording wherever it agreed with the launches, the launches' truth elsewhere"""
    want, got = grids
    names = list(want["dims_names"])
    n_cus, rows = want["n_cus"], want["rows"]
    ff, w_ff = got["plan"][names.index("ff")], want["plan"][names.index("ff")]
    assert (ff[..., 0] == rows[None, :, None, None, None]).all() and (ff[..., 1:4] == 0).all() and (ff[..., 5] == NONE).all()
    assert (ff[..., 4] == (n_cus // 16)[:, None, None, None, None]).all()
    big = rows > 4
    assert np.array_equal(ff[:, big], w_ff[:, big])                      # (the cost model already sent every larger batch to the tile kernel)
    imu, w_imu = got["plan"][names.index("imupose")], want["plan"][names.index("imupose")]
    assert not np.isin(imu[..., 5], (SMALL, C32, C16, LV16)).any()
    assert (imu[..., 1] <= 2).all()                                       # (wide input: at most two row tiles per cluster)
    for c, cus in enumerate(n_cus):
        for b, B in enumerate(rows):
            split = cus >= 64 and B > 512                                 # eight 32-row clusters of lstm_upper32.hip, eval mode, AUTO
            assert (imu[c, b, :, 0, 1, 5] == SPLIT32).all() == split, (cus, B)
            if split:
                assert (imu[c, b, :, 0, 1, 0] == 0).all() and (imu[c, b, :, 0, 1, 3] == -(-B // 4096)).all()
            assert (imu[c, b, :, :, 0, 5] != SPLIT32).all()               # (second generation switched off: never)
    agree = (w_imu[..., 5] == GEN1) & (w_imu[..., 1] <= 2) & (imu[..., 5] == GEN1) & (w_imu[..., 0] == imu[..., 0])
    assert agree.any() and np.array_equal(imu[agree], w_imu[agree])


def test_planner_alone_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "plan_sweep"
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(REPO / "tests" / "tools" / "plan_sweep.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failures" in r.stdout, r.stdout
