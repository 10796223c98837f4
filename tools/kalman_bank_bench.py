#!/usr/bin/env python3
"""Timing of the Kalman estimator's device stream bank against the paths it replaces, both legs in one process and
alternating, p50 of three runs each, after un-timed launches that settle the clocks:

  device frame   KalmanStreamBank.step_rows on device rows (HIP events), S = 1 and 256, E = 48, W = 10, smooth 1, against the loop of
                 tests/tools/time_kalman.py: KalmanSmartwatchModel.forward + the torch.cat state shift and nothing else
  process_row    host to host, 2000 frames after 200, E = 32 and 48: the device frame against use_device_frame = False (the staged path)
  replay         process_recording: one recording of 10 000 frames, 64 recordings of 1 000 frames; frames/s beside the process_row loop

python tools/kalman_bank_bench.py [--out-dir profiles] [--quick]   ->   <out-dir>/kalman_bank.json, <out-dir>/kalman_bank.md
PARITY UNPINNED for this estimator: synthetic weights (oracle/kalman_oracle.py), the numbers are about time only."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "arm-pose-estimation_amd")]

import torch  # noqa: E402

from oracle import kalman_oracle as ko  # noqa: E402
from wear_mocap_ape_amd.estimate import kalman_models  # noqa: E402
from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman  # noqa: E402
from wear_mocap_ape_amd.streams import KalmanStreamBank  # noqa: E402

RUNS = 3


def make_rows(rng, n):
    base = np.load(REPO / "tests" / "golden" / "stream_trace_pocket.npz")["rows"].astype(np.float32)
    rows = base[rng.integers(0, len(base), n)].copy()
    cols = list(range(10, 23)) + list(range(33, 46))
    rows[:, cols] += (0.05 * rng.normal(size=(n, len(cols)))).astype(np.float32)
    return rows


def p50(v):
    return float(np.percentile(v, 50))


def event_us(fn, n):
    us = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return us


def device_frame(S, E, W, frames, warm):
    m = kalman_models.KalmanSmartwatchModel(E, W)
    m.load_state_dict(ko.make_state_dict(W, 0))
    rng = np.random.default_rng(0)
    raw = torch.from_numpy(rng.normal(size=(S, W, 1, 22)).astype(np.float32)).cuda()
    st = {"state": torch.from_numpy((0.1 * rng.normal(size=(S, E, W, 14))).astype(np.float32)).cuda()}

    def parent():                     # tests/tools/time_kalman.py's loop body
        out = m.forward(raw, st["state"])
        st["state"] = torch.cat((st["state"][:, :, 1:, :], out[0][:, :, None, :]), axis=2)

    bank = KalmanStreamBank(m, S, smooth=1, normalize=True)
    rows = torch.from_numpy(make_rows(rng, S)).cuda()

    def new():
        bank.step_rows(rows)

    event_us(parent, warm)
    event_us(new, warm + W + 2)        # past the init frames: the ensemble phase is the steady state
    a, b = [], []
    for _ in range(RUNS):
        a.append(p50(event_us(parent, frames)))
        b.append(p50(event_us(new, frames)))
    m.check()
    return {"parent_forward_cat_us": a, "bank_frame_us": b, "parent_p50_us": p50(a), "bank_p50_us": p50(b), "ratio": p50(b) / p50(a)}


def estimator(E, W, device_frame_on, smooth=1):
    sd = ko.make_state_dict(W, 0)
    est = WatchPhonePocketKalman({k: torch.from_numpy(v) for k, v in sd.items()}, smooth=smooth, num_ensemble=E, window_size=W)
    est.use_device_frame = device_frame_on
    return est


def host_us(est, rows, warm):
    for r in rows[:warm]:
        est.process_row(r)
    us = []
    for r in rows[warm:]:
        t = time.perf_counter()
        est.process_row(r)
        us.append((time.perf_counter() - t) * 1e6)
    return us


def process_row(E, W, frames, warm):
    rows = make_rows(np.random.default_rng(1), warm + frames)
    new, staged = estimator(E, W, True), estimator(E, W, False)
    a, b, b99 = [], [], []
    for _ in range(RUNS):
        a.append(p50(host_us(staged, rows, warm)))
        u = host_us(new, rows, warm)
        b.append(p50(u))
        b99.append(float(np.percentile(u, 99)))
    new.model.check()
    return {"staged_us": a, "device_frame_us": b, "device_frame_p99_us": b99, "staged_p50_us": p50(a), "device_frame_p50_us": p50(b),
            "below_every_staged_run": bool(max(b) < min(a))}


def replay(E, W, F, R, row_loop_frames):
    rows = make_rows(np.random.default_rng(2), F * R)
    est = estimator(E, W, True)
    starts = np.arange(R, dtype=np.int32) * F
    rd = torch.from_numpy(rows).cuda()
    est.process_recording(rd[:min(F, 64) * 1], seed=1)           # un-timed: allocations, clocks
    secs = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        est.process_recording(rd, starts=starts, seed=1)
        secs.append(time.perf_counter() - t)
    est.reset()
    n = min(row_loop_frames, F * R)
    t = time.perf_counter()
    for r in rows[:n]:
        est.process_row(r)
    loop = n / (time.perf_counter() - t)
    est.model.check()
    return {"frames": F * R, "recordings": R, "seconds": secs, "frames_per_s": F * R / p50(secs), "process_row_loop_frames_per_s": loop}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=str(REPO / "profiles"))
    ap.add_argument("--quick", action="store_true", help="a tenth of the frames (a rehearsal)")
    args = ap.parse_args()
    q = 10 if args.quick else 1
    E, W = 48, 10
    res = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "E": E, "W": W, "smooth": 1}
    try:
        info = json.loads((REPO / "arm-pose-estimation_amd" / "lib" / "build_info.json").read_text())
        res["commit"] = info.get("commit", "unknown")
        res["object_sha256"] = {k: info["objects"][k] for k in ("kalman_bank.o", "kalman.o") if k in info.get("objects", {})}
    except Exception:
        res["commit"], res["object_sha256"] = "unknown", {}
    res["device_frame"] = {str(S): device_frame(S, E, W, 200 // q, 30) for S in (1, 256)}
    res["process_row"] = {str(e): process_row(e, W, 2000 // q, 200 // q) for e in (32, 48)}
    res["replay"] = {"1x10000": replay(E, W, 10000 // q, 1, 2000 // q), "64x1000": replay(E, W, 1000 // q, 64, 2000 // q)}
    out = Path(args.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    (out / "kalman_bank.json").write_text(json.dumps(res, indent=1) + "\n")
    d, pr, rp = res["device_frame"], res["process_row"], res["replay"]
    md = [f"# Kalman stream bank: frame times ({res['device']})", "",
          f"commit `{res['commit']}`, objects " + ", ".join(f"`{k}` {v[:12]}" for k, v in res["object_sha256"].items()), "",
          "Written by `tools/kalman_bank_bench.py`: both legs in one process, alternating, p50 of the three runs' p50s; synthetic weights "
          "(PARITY UNPINNED: the numbers are about time only).", "",
          "| device frame, E = 48, W = 10, smooth 1 (HIP events) | forward + torch.cat | bank frame | ratio |", "|---|---|---|---|"]
    md += [f"| S = {S} | {v['parent_p50_us']:.1f} us | {v['bank_p50_us']:.1f} us | {v['ratio']:.2f} |" for S, v in d.items()]
    md += ["", "| process_row, host to host, 2000 frames | staged | device frame (p99) | below every staged run |", "|---|---|---|---|"]
    md += [f"| E = {e} | {v['staged_p50_us']:.1f} us | {v['device_frame_p50_us']:.1f} us ({p50(v['device_frame_p99_us']):.1f}) | "
           f"{v['below_every_staged_run']} |" for e, v in pr.items()]
    md += ["", "| replay, E = 48 | frames/s | process_row loop, frames/s |", "|---|---|---|"]
    md += [f"| {k} | {v['frames_per_s']:.0f} | {v['process_row_loop_frames_per_s']:.0f} |" for k, v in rp.items()]
    (out / "kalman_bank.md").write_text("\n".join(md) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
