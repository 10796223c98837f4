"""Where a steady-state phase of lstm_cluster32.hip waits, in a product-like build (-DAPE_C32_WAITS: s_memtime around each wait, nothing else in
the MFMA stream): shader clocks of wave 0 per steady-state section in layer 1's two `look_landed()` waits (own look, next section's look), in
its wait + barrier between the spans, and between a layer-0 section's entry and the exit of its top barrier; beside the launch time by HIP
events.  python tests/tools/waits_c32.py [B] [T] [extra flags]      (APE_HIP_LIB = a -DAPE_C32_WAITS variant, without -DAPE_C32_COUNTS)"""
import ctypes as C, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "arm-pose-estimation_amd"))
import numpy as np
import torch
from oracle import ape_oracle as orc
from wear_mocap_ape_amd import _hip
from wear_mocap_ape_amd.estimate import nn_models
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
T = int(sys.argv[2]) if len(sys.argv) > 2 else 64
EXTRA = int(sys.argv[3], 0) if len(sys.argv) > 3 else 0
cfg = orc.MODEL_CONFIGS["pocket"]
m = nn_models.DropoutLSTM(cfg["I"], cfg["H"], cfg["L"], cfg["O"], device=0)
m.load_state_dict(orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], 0))
m.set_kernel("cluster")
x = torch.randn(B, T, cfg["I"], device="cuda"); y = torch.empty(B, cfg["O"], device="cuda")
lib = _hip.lib()
lib.ape_debug_read_wg.restype, lib.ape_debug_read_wg.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
def fwd():
    _hip.check(lib.ape_lstm_forward(m.handle, C.c_void_p(x.data_ptr()), B, T, EXTRA, None, 0.0, 0, C.c_void_p(y.data_ptr()), None), "fwd")
for _ in range(20): fwd()
meds = []
for blk in range(5):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(40): fwd()
    b.record(); b.synchronize()
    meds.append(a.elapsed_time(b) / 40 * 1e3)
torch.cuda.synchronize(); m.check()
buf = (C.c_ulonglong * (256 * 8))()
assert lib.ape_debug_read_wg(m.handle, buf) == 0
d = np.frombuffer(buf, dtype=np.uint64)[512:512 + 24 * 8 * 8].reshape(24 * 8, 8).astype(np.float64)
d = d[d[:, 7] > 0]
assert len(d) > 0 and d[:, 4].max() > 0, "no record: APE_HIP_LIB is not a -DAPE_C32_WAITS build, or the window has no steady-state phase"
n1, n0 = np.maximum(d[:, 4], 1), np.maximum(d[:, 5], 1)
own, nxt, mid, top0 = d[:, 0] / n1, d[:, 1] / n1, d[:, 2] / n1, d[:, 3] / n0
print(f"{m.last_kernel()} B={B} T={T} flags {EXTRA:#x}: {statistics.median(meds):.1f} us per launch; last launch, {len(d)} workgroups (wave 0 of each), "
      f"{d[:, 4].mean():.0f} steady-state layer-1 sections each:")
for name, v in (("layer 1, own look's wait", own), ("layer 1, next section's look's wait", nxt), ("layer 1, wait + barrier between the spans", mid),
                ("layer 0, entry -> behind the top barrier", top0)):
    print(f"  {name:44s} cycles per section: mean {v.mean():6.0f}  median {np.median(v):6.0f}  min {v.min():6.0f}  max {v.max():6.0f}")
print(f"  sum of layer 1's three waits: mean {(own + nxt + mid).mean():6.0f} cycles per section;  blocking own gathers in steady-state sections: mean {d[:, 6].mean():5.2f}")
print(f"  kernel body (shader clocks, first section .. head): mean {d[:, 7].mean():9.0f}  min {d[:, 7].min():9.0f} max {d[:, 7].max():9.0f}")
