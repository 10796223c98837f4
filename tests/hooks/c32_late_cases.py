"""Child process of tests/test_c32_hot_gaps_gpu.py: its APE_HIP_LIB names lib/diag/libape_hip_c32late.so (lstm_cluster32.hip built with
-DAPE_C32_LATE_EVERY=3 -DAPE_C32_COUNTS).  Runs the late cases, each with a clean status word, and writes to the .npz named on the command
line the outputs and, per workgroup of the first 24 clusters, how many gathers of layer 0 / layer 1 took the blocking form."""
import ctypes as C
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[2]
for p in (str(REPO), str(REPO / "arm-pose-estimation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np

from tests.test_c32_hot_gaps_gpu import LATE_CASES, case_id, run_case
from wear_mocap_ape_amd import _hip

assert os.environ.get("APE_HIP_LIB", "").endswith("libape_hip_c32late.so"), "this file runs on the late-judge library (APE_HIP_LIB)"
lib = _hip.lib()
lib.ape_debug_read_wg.restype, lib.ape_debug_read_wg.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
res = {}
for c in LATE_CASES:
    y, kernel, m = run_case(c, with_model=True)
    buf = (C.c_ulonglong * (256 * 8))()
    assert lib.ape_debug_read_wg(m.handle, buf) == 0
    d = np.frombuffer(buf, dtype=np.uint64)[512:512 + 24 * 8 * 8].reshape(24 * 8, 8)
    res["y_" + case_id(c)] = y
    res["kernel_" + case_id(c)] = np.array(kernel)
    res["blocked_" + case_id(c)] = d[d[:, 7] > 0][:, :2].astype(np.int64)
np.savez(sys.argv[1], **res)
