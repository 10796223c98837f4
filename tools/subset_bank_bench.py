"""Subset frames of the stream bank (StreamBank.frame / ape_streams_frame_subset) against the lockstep frame
(push_rows + step), pocket model (2 x 256, T = 6), S = 1024 streams, deterministic and at 25 Monte-Carlo samples.  Frames are
enqueued back to back on one stream and timed with events around the whole run; prints ONE JSON line (microseconds per frame).

    python tools/subset_bank_bench.py [--frames 200] [--warmup 20]

Seeded synthetic weights; the rows are the recorded trace of tests/golden/stream_trace_pocket.npz tiled with a little noise."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for _p in (str(ROOT), str(ROOT / "arm-pose-estimation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

S, T, KS = 1024, 6, (1, 64, 512, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    from oracle import ape_oracle as orc
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import nn_models
    from wear_mocap_ape_amd.streams import StreamBank
    torch.cuda.set_device(0)
    cfg = orc.MODEL_CONFIGS["pocket"]
    sd = orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], seed=0)
    raw = json.loads((ROOT / "tests" / "golden" / "norm_stats.json").read_text())["pocket"]
    model = nn_models.DropoutLSTM(cfg["I"], cfg["H"], cfg["L"], cfg["O"], dropout=0.2, device=0)
    model.load_state_dict(sd)
    model.set_norm_stats(*(np.array(raw[k]) for k in ("xx_m", "xx_s", "yy_m", "yy_s")))
    model.set_body(orc.DEFAULT_BODY)
    base = np.load(ROOT / "tests" / "golden" / "stream_trace_pocket.npz")["rows"].astype(np.float32)
    n_rows = 4 * S
    rows = np.tile(base, ((n_rows + len(base) - 1) // len(base), 1))[:n_rows]
    rows += np.float32(1e-3) * np.random.default_rng(0).standard_normal(rows.shape, dtype=np.float32)
    rows_d = torch.from_numpy(rows).cuda()
    kind = _hip.PARSE_WATCH_PHONE_POCKET
    rng = np.random.default_rng(1)
    result = {"S": S, "T": T, "model": "pocket 2x256", "frames": args.frames, "us_per_frame": {}}

    def timed(run, n):
        for i in range(args.warmup):
            run(i)
        torch.cuda.synchronize()
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(n):
            run(i)
        z.record()
        z.synchronize()
        return a.elapsed_time(z) * 1e3 / n

    for tag, mc in (("det", None), ("mc25", 25)):
        kw = dict(monte_carlo_samples=mc, dropout=0.2, seed=7) if mc else {}
        bank = StreamBank(model, S, T, smooth=1, normalize=True, dtype=torch.float32, **kw)
        n = mc or 1                                   # stacked rows per stream (smooth = 1)
        out = torch.empty((S, 25 + 6 * n if n > 1 else 25), dtype=torch.float32, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        flags = _hip.FLAG_NORMALIZE_INPUT | (_hip.FLAG_PACKED_MSG if n > 1 else 0)
        # lockstep: push_rows + step of all S streams
        lock_rows = [rows_d[(i % 4) * S:(i % 4 + 1) * S].contiguous() for i in range(4)]

        def lockstep(i):
            _hip.check(_hip.lib().ape_streams_push_rows(bank._handle, kind, C.c_void_p(lock_rows[i % 4].data_ptr()), stream), "push_rows")
            _hip.check(_hip.lib().ape_streams_step(bank._handle, flags, C.c_void_p(out.data_ptr()), None, _hip.F32, stream), "step")
        result["us_per_frame"][f"lockstep_{tag}_K{S}"] = round(timed(lockstep, args.frames), 2)
        bank.check()
        for K in KS:
            lists = [np.ascontiguousarray(rng.permutation(S)[:K], dtype=np.int32) for _ in range(16)]
            sub_rows = [rows_d[j * K % (3 * S):j * K % (3 * S) + K].contiguous() for j in range(16)]

            def subset(i):
                idx = lists[i % 16]
                _hip.check(_hip.lib().ape_streams_frame_subset(bank._handle, kind, C.c_void_p(sub_rows[i % 16].data_ptr()),
                                                               C.c_void_p(idx.ctypes.data), K, flags, C.c_void_p(out.data_ptr()),
                                                               _hip.F32, stream), "frame_subset")
            result["us_per_frame"][f"subset_{tag}_K{K}"] = round(timed(subset, args.frames), 2)
            result.setdefault("regressor_kernel", {})[f"{tag}_K{K}"] = model.last_kernel()
            bank.check()
        bank.reset()
        del bank
    print(json.dumps(result))


if __name__ == "__main__":
    main()
