"""Writes tests/golden/plan_grid.npz: what `ape_debug_plan2`, `ape_debug_bank_route` and `ape_debug_bank_chunks` of ONE build of the
library answer over a grid of model shapes, CU counts and batch sizes (pure host arithmetic: no GPU).  The committed file was recorded at
the last commit before the dispatch moved into csrc/ape_plan.h; tests/test_plan_grid_cpu.py holds every later build to it.

    python tests/golden/gen_plan_grid.py path/to/libape_hip.so [out.npz]

Run it with APE_C16_MIN_T, APE_LV16_MAX_T and APE_LV16_MIN_ROWS unset (the diagnostic overrides of the route thresholds)."""
import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np

# input_size, hidden_size, num_layers, output_size, target_layout, model_kind (0 LSTM, 1 FF, 2 ImuPoseLSTM)
DIMS = {
    "pocket": (22, 256, 2, 14, 0, 0),
    "watch": (20, 256, 2, 12, 1, 0),
    "uarm": (38, 128, 3, 12, 1, 0),
    "imupose": (22, 256, 2, 14, 0, 2),
    "ff": (22, 256, 2, 14, 0, 1),
}
N_CUS = (1, 7, 8, 15, 16, 32, 40, 63, 64, 128, 256, 304)
ROWS = (1, 4, 5, 16, 17, 256, 257, 512, 513, 1024, 1025, 2048, 2460, 4096, 4097, 4396, 8292, 12345)
STEPS = (1, 6, 11, 12, 48, 49, 64, 200)
N_MC = (1, 2, 19, 25, 50)


class ApeDims(C.Structure):
    _fields_ = [("input_size", C.c_int32), ("hidden_size", C.c_int32), ("num_layers", C.c_int32), ("output_size", C.c_int32),
                ("target_layout", C.c_int32), ("device", C.c_int32), ("model_kind", C.c_int32)]


def dims_of(name):
    i, h, l, o, layout, kind = DIMS[name]
    return ApeDims(i, h, l, o, layout, 0, kind)


def bank_sizes():
    """(S, n_mc) with S * n_mc on both sides of every value of ROWS"""
    out = []
    for n_mc in N_MC:
        for r in ROWS:
            for s in (r // n_mc, -(-r // n_mc)):
                if s >= 1 and (s, n_mc) not in out:
                    out.append((s, n_mc))
    return out


def bind(lib):
    lib.ape_debug_plan2.restype = C.c_int
    lib.ape_debug_plan2.argtypes = [C.POINTER(ApeDims), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 6)]
    lib.ape_debug_bank_route.restype = C.c_int
    lib.ape_debug_bank_route.argtypes = [C.POINTER(ApeDims), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong * 4)]
    lib.ape_debug_bank_chunks.restype = C.c_int
    lib.ape_debug_bank_chunks.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong * 3)]
    return lib


def record(lib):
    """the outputs as dense arrays over the axes above: plan[dims, n_cus, B, T, cdrop, c32, 6], route[dims, n_cus, bank size, T, 4],
    chunks[up128, bank size, T, 3]; the axes travel with them"""
    pairs = bank_sizes()
    plan = np.zeros((len(DIMS), len(N_CUS), len(ROWS), len(STEPS), 2, 2, 6), dtype=np.int32)
    route = np.zeros((len(DIMS), len(N_CUS), len(pairs), len(STEPS), 4), dtype=np.int32)
    chunks = np.zeros((2, len(pairs), len(STEPS), 3), dtype=np.int64)
    o6, o4, o3 = (C.c_int * 6)(), (C.c_longlong * 4)(), (C.c_longlong * 3)()
    for d, name in enumerate(DIMS):
        dims = dims_of(name)
        for c, n_cus in enumerate(N_CUS):
            for t, T in enumerate(STEPS):
                for b, B in enumerate(ROWS):
                    for cdrop in (0, 1):
                        for c32 in (0, 1):
                            assert lib.ape_debug_plan2(C.byref(dims), n_cus, B, T, cdrop, c32, C.byref(o6)) == 0
                            plan[d, c, b, t, cdrop, c32] = tuple(o6)
                for k, (S, n_mc) in enumerate(pairs):
                    assert lib.ape_debug_bank_route(C.byref(dims), n_cus, S, T, n_mc, C.byref(o4)) == 0
                    route[d, c, k, t] = tuple(o4)
    for up128 in (0, 1):
        for k, (S, n_mc) in enumerate(pairs):
            for t, T in enumerate(STEPS):
                assert lib.ape_debug_bank_chunks(up128, S, T, n_mc, C.byref(o3)) == 0
                chunks[up128, k, t] = tuple(o3)
    return dict(plan=plan, route=route, chunks=chunks, dims_names=np.array(list(DIMS)), dims=np.array(list(DIMS.values()), dtype=np.int32),
                n_cus=np.array(N_CUS, dtype=np.int32), rows=np.array(ROWS, dtype=np.int32), steps=np.array(STEPS, dtype=np.int32),
                bank_sizes=np.array(pairs, dtype=np.int32))


def main():
    for v in ("APE_C16_MIN_T", "APE_LV16_MAX_T", "APE_LV16_MIN_ROWS"):
        if v in os.environ:
            raise SystemExit(f"{v} is set: the grid records the built-in thresholds")
    lib = bind(C.CDLL(sys.argv[1]))
    out = Path(sys.argv[2]) if len(sys.argv) > 2 else Path(__file__).with_name("plan_grid.npz")
    rec = record(lib)
    np.savez_compressed(out, **rec)
    print(out, {k: v.shape for k, v in rec.items()}, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
