"""The pinned plan and the code that launches are ONE thing (`csrc/ape_plan.h`): for the deployed models in eval mode the route
`ape_debug_plan2` reports for this device's CU count is the kernel `ape_lstm_forward` launches, and where no row goes to the batch-tile
kernel the result holds the parity budget against the oracle.  `ape_lstm_kernel_name` keeps returning the strings recorded before the
planner existed (tests/golden/kernel_names.json; bench.py looks up its traffic profiles by them)."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc

pytestmark = pytest.mark.gpu

ROUTE_KERNEL = {0: "ape_lstm_tile16", 1: "ape_lstm_cluster", 2: "ape_lstm_cluster32", 3: "ape_lstm_cluster_small", 4: "ape_lstm_cluster16",
                5: "ape_lstm_level16", 6: "ape_lstm_upper32"}
BATCHES = (1, 4, 5, 512, 513, 1024, 1025)
STEPS = (6, 12, 48, 49)
TOL_Y = 1e-6          # the NN-target budget of tests/test_hip_parity.py


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def _plan2(dims, n_cus, B, T):
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    lib.ape_debug_plan2.restype = C.c_int
    lib.ape_debug_plan2.argtypes = [C.POINTER(_hip.ApeDims), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 6)]
    out = (C.c_int * 6)()
    assert lib.ape_debug_plan2(C.byref(dims), n_cus, B, T, 0, 1, C.byref(out)) == 0
    return dict(n16=out[0], kernel=out[5])


@pytest.mark.parametrize("name", ["pocket", "watch", "uarm"])
def test_the_planned_route_is_the_launched_kernel(name):
    from tests.test_hip_parity import make_model
    from wear_mocap_ape_amd import _hip
    m, sd, cfg = make_model(name, 21)
    dims = _hip.ApeDims(cfg["I"], cfg["H"], cfg["L"], cfg["O"], cfg["layout"], 0, _hip.MODEL_LSTM)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    for T in STEPS:
        x = np.random.default_rng(100 * T + cfg["I"]).normal(size=(max(BATCHES), T, cfg["I"])).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        ref = orc.lstm_forward(sd, x)[:, -1]             # once per window length: the smaller batches are its leading rows
        for B in BATCHES:
            plan = _plan2(dims, n_cus, B, T)
            y = m(xd[:B], last_step_only=True).cpu().numpy()[:, 0]
            want = ROUTE_KERNEL[plan["kernel"]] if plan["n16"] < B else "ape_lstm_tile16"
            assert m.last_kernel() == want, (name, B, T, plan, m.last_kernel())
            m.check()
            if plan["n16"] == 0:
                err = float(np.abs(y - ref[:B]).max())
                assert err < TOL_Y, (name, B, T, plan, err)


def test_kernel_names_are_the_recorded_ones():
    from tests.test_hip_parity import make_model
    recorded = json.loads((Path(__file__).parent / "golden" / "kernel_names.json").read_text())
    for name in ("pocket", "watch", "uarm"):
        m, _, _ = make_model(name, 3)
        for prec in ("f32", "f16"):
            m.set_precision(prec)
            for key, want in recorded[f"{name}/{prec}"].items():
                B, T = (int(v) for v in key.split("x"))
                assert m.kernel_name(B, T) == want, (name, prec, B, T, m.kernel_name(B, T), want)


def test_imupose_is_planned_as_its_forward_was_launched_before_the_planner():
    """tests/golden/imupose_last_kernel.json: `ape_model_last_kernel` after ImuPoseLSTM eval forwards, recorded on a whole MI355X at the last
    commit before the planner (whose `ape_debug_plan2` ignored the model kind, so the CPU grid has nothing true to compare these dims with):
    the forward launches the same kernels, and the plan names them -- PLAN_SPLIT32 above 512 windows, the wide first generation below."""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import nn_models
    recorded = json.loads((Path(__file__).parent / "golden" / "imupose_last_kernel.json").read_text())
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = nn_models.ImuPoseLSTM(22, 256, 2, 14, device=0)
    rng = np.random.default_rng(16)
    m.load_state_dict({k: torch.from_numpy(rng.normal(scale=0.05, size=s).astype(np.float32)) for k, s in m._wanted_shapes().items()})
    dims = _hip.ApeDims(22, 256, 2, 14, 0, 0, _hip.MODEL_IMUPOSE)
    for key, was in recorded.items():
        B, T = (int(v) for v in key.split("x"))
        x = torch.from_numpy(np.random.default_rng(B + T).normal(size=(B, T, 22)).astype(np.float32)).cuda()
        m(x, last_step_only=True)
        m.check()
        plan = _plan2(dims, n_cus, B, T)
        planned = ROUTE_KERNEL[plan["kernel"]] if plan["n16"] < B else "ape_lstm_tile16"
        assert m.last_kernel() == planned, (B, T, plan, m.last_kernel())
        if n_cus == 256:
            assert m.last_kernel() == was, (B, T, m.last_kernel(), was)
