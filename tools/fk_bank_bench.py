"""The estimator without a regressor (WatchPhoneUarm): the FK bank's lockstep and subset frames, offline replay and
process_row latency.  Frames are enqueued back to back on one stream and timed with HIP events around >= 200 of them, after a
warm-up; every figure is the median of three runs.

    python tools/fk_bank_bench.py [--frames 200] [--warmup 20] [--out profiles/fk_only_bench.json]
    python tools/fk_bank_bench.py --prof        # a short pass of every case, for rocprofv3 --kernel-trace --stats

Rows are seeded random WATCH_PHONE_IMU messages (unit quaternions).  Writes one JSON file and prints it as one line."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for _p in (str(ROOT), str(ROOT / "arm-pose-estimation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SMOOTH = 5
LOCKSTEP_S = (1024, 8192, 65536)
SUBSET_S, SUBSET_K = 8192, (1, 64, 1024)
REPLAY_F = 10 ** 6


def random_rows(rng, n):
    from wear_mocap_ape_amd.data_types import messaging
    slp = messaging.WATCH_PHONE_IMU_LOOKUP
    rows = rng.normal(size=(n, 55)).astype(np.float32)
    for pre in ("sw_rotvec", "sw_forward", "ph_rotvec", "ph_forward"):
        q = rng.normal(size=(n, 4))
        rows[:, [slp[f"{pre}_{c}"] for c in "wxyz"]] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    rows[:, slp["sw_pres"]] = 1000.0 + rng.normal(size=n).astype(np.float32)
    rows[:, slp["sw_init_pres"]] = 1000.5
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fk_only_bench.json"))
    ap.add_argument("--prof", action="store_true", help="one short pass of every case, nothing written")
    args = ap.parse_args()
    if args.prof:
        args.frames, args.warmup, args.runs = 50, 5, 1
    import __graft_entry__ as entry
    entry.build()
    import torch
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    from wear_mocap_ape_amd.streams import FkStreamBank
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    result = {"smooth": SMOOTH, "frames": args.frames, "runs": args.runs, "device": torch.cuda.get_device_name(0)}

    def timed(run):
        """median over runs of microseconds per call, calls enqueued back to back"""
        per = []
        for _ in range(args.runs):
            for i in range(args.warmup):
                run(i)
            torch.cuda.synchronize()
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.frames):
                run(i)
            z.record()
            z.synchronize()
            per.append(a.elapsed_time(z) * 1e3 / args.frames)
        return round(statistics.median(per), 2)

    # lockstep frames: all S streams in order
    lock = {}
    for S in LOCKSTEP_S:
        bank = FkStreamBank(S, smooth=SMOOTH, dtype=torch.float32)
        rows = [torch.from_numpy(random_rows(rng, S)).cuda() for _ in range(4)]
        us = timed(lambda i: bank.step_rows(rows[i % 4]))
        lock[str(S)] = {"us_per_frame": us, "stream_frames_per_s": round(S / us * 1e6)}
        del bank
    result["lockstep"] = lock

    # subset frames of an 8192-stream bank: K random distinct streams per frame (the lists drawn up front)
    sub = {}
    bank = FkStreamBank(SUBSET_S, smooth=SMOOTH, dtype=torch.float32)
    bank.step_rows(torch.from_numpy(random_rows(rng, SUBSET_S)).cuda())
    for K in SUBSET_K:
        lists = [rng.choice(SUBSET_S, size=K, replace=False) for _ in range(8)]
        rows = [torch.from_numpy(random_rows(rng, K)).cuda() for _ in range(8)]
        us = timed(lambda i: bank.frame(rows[i % 8], lists[i % 8]))
        sub[str(K)] = {"us_per_frame": us, "stream_frames_per_s": round(K / us * 1e6)}
    result["subset_S8192"] = sub
    del bank

    # offline replay: F frames in 50 recordings, one blocking call
    est = WatchPhoneUarm(smooth=SMOOTH)
    F = REPLAY_F
    rows = torch.from_numpy(random_rows(rng, F)).cuda()
    starts = np.r_[0, np.sort(rng.choice(np.arange(1, F), size=49, replace=False))]
    est.process_recording(rows[:1000], starts=[0])
    per = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        est.process_recording(rows, starts=starts, out_dtype=torch.float32)
        per.append(time.perf_counter() - t0)
    sec = statistics.median(per)
    result["replay"] = {"F": F, "recordings": 50, "ms_per_call": round(sec * 1e3, 3), "frames_per_s": round(F / sec)}
    del rows

    # process_row: host row in, host message out, against the staged reference-style methods
    host_rows = random_rows(rng, 64)
    lat = {}
    for name, device_frame in (("device_frame", True), ("staged", False)):
        e = WatchPhoneUarm(smooth=SMOOTH)
        e.use_device_frame = device_frame
        n = 200 if args.prof else 2000
        for i in range(50):
            e.process_row(host_rows[i % 64])
        ts = []
        for i in range(n):
            t0 = time.perf_counter()
            e.process_row(host_rows[i % 64])
            ts.append((time.perf_counter() - t0) * 1e6)
        lat[name] = {"p50_us": round(float(np.percentile(ts, 50)), 1), "p99_us": round(float(np.percentile(ts, 99)), 1), "calls": n}
    result["process_row"] = lat

    line = json.dumps(result)
    if not args.prof:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
