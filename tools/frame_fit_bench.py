"""Heading and frame offset against the truth (score.frame_sums / rotate_rows / align_frame) on the workload of
profiles/score_lags.md: 100 000 pocket frames, `[F, 196]` float64 rows from process_recording(spread=True) at 25 Monte-Carlo samples,
truth as NN targets, here in 64 recordings of equal length.  Legs, alternating within one session behind warmed shapes, timed by HIP
events:

    sums L     one ape_frame_sums call over L = 17 and 65 lags
    lags L     ape_score_lags at the same F and L, with the spread records (accumulators only): the call next to it in the chain
    rotate     ape_rotate_rows of the rows and their spread records, and the bytes it moves over the time against the HBM peak
    align      score.align_frame end to end over 17 lags (frame_sums, best_frame on the host behind a wait, rotate_rows, score_lags)

and, by the host clock, the route a user has without the device entry: a copy of the message columns to the host plus
score.frame_sums_numpy (on synthetic est-kind truth of the same shape: the statement takes est rows, and times do not depend on the
values).  Writes profiles/frame_fit.md's measured section and prints ONE JSON line.

    python tools/frame_fit_bench.py [--frames 100000] [--repeats 20] [--host-repeats 3] [--out profiles/frame_fit.md]

Models carry seeded synthetic weights, rows and truth are synthetic."""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for _p in (str(ROOT), str(ROOT / "arm-pose-estimation_amd"), str(ROOT / "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SWEEPS = ((-8, 8), (-32, 32))
RECORDINGS = 64
HBM_PEAK = 8.0e12                                           # bytes / s
MARKER, NOTES = "## Measured", "### Reading the figures"   # the section this tool writes; what follows it is written by hand and kept


def spread_of(v):
    return [round(min(v), 4), round(max(v), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "frame_fit.md"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return
    from replay_bench import deploy_tree, rows_for
    from score_lags_bench import alternate
    from wear_mocap_ape_amd import config, score
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import WatchPhonePocketNN
    torch.cuda.set_device(0)
    F, n_mc = args.frames, 25
    rng = np.random.default_rng(7)
    result = {"frames": F, "n_mc": n_mc, "recordings": RECORDINGS, "repeats": args.repeats, "sweeps": {}}
    with tempfile.TemporaryDirectory() as tmp:
        shipped, deploy = Path(config.PATHS["deploy"]), Path(tmp) / "deploy"
        config.PATHS["deploy"] = deploy
        est = WatchPhonePocketNN(model_hash=deploy_tree(shipped, deploy, "pocket", 0.2), smooth=1, add_mc_samples=True, monte_carlo_samples=n_mc)
        starts = [r * F // RECORDINGS for r in range(RECORDINGS)]
        out, rec = est.process_recording(torch.from_numpy(rows_for("pocket", F)).cuda(), starts=starts, spread=True)
        truth = torch.from_numpy(rng.normal(size=(F, 14))).cuda()
        layout, skip, body = est._layout, est.sequence_len - 1, est.body_measurements
        quats = rng.normal(size=(RECORDINGS, 4))
        torch.cuda.synchronize()

        legs = {}
        for lo, hi in SWEEPS:
            L = hi - lo + 1
            legs[f"sums_{L}"] = lambda lo=lo, hi=hi: score.frame_sums(layout, out, truth, (lo, hi), "targets", starts, skip, body)
            legs[f"lags_{L}"] = lambda lo=lo, hi=hi: score.score_lags(layout, out, truth, (lo, hi), "targets", rec, starts, skip, body)[1]
        legs["rotate"] = lambda: score.rotate_rows(layout, out, quats, rec, starts)
        legs["align"] = lambda: score.align_frame(layout, out, truth, SWEEPS[0], "yaw", (1, 1, 1, 0, 0), "targets", rec, starts, skip, body)[:2]
        times = alternate(legs, args.repeats)
        blocks = (F + 255) // 256
        for lo, hi in SWEEPS:
            L = hi - lo + 1
            a, b = times[f"sums_{L}"], times[f"lags_{L}"]
            result["sweeps"][str(L)] = {"lags": [lo, hi], "frame_sums_ms": round(a[0], 4), "frame_sums_range": spread_of(a[1]),
                                        "score_lags_ms": round(b[0], 4), "score_lags_range": spread_of(b[1]),
                                        "ratio_sums_over_lags": round(a[0] / b[0], 2),
                                        "partial_records_bytes": (blocks + RECORDINGS) * L * 51 * 8}
        moved = 2 * F * (25 + 21) * 8                       # every message and spread value read once and written once
        rot = times["rotate"]
        result["rotate_rows"] = {"ms": round(rot[0], 4), "range": spread_of(rot[1]), "bytes_moved": moved,
                                 "share_of_hbm_peak": round(moved / (rot[0] * 1e-3) / HBM_PEAK, 4)}
        result["align_frame_ms"] = round(times["align"][0], 4)
        result["align_frame_range"] = spread_of(times["align"][1])

        # the host route: the message columns to the host, then the numpy statement
        est_truth = rng.normal(size=(F, 21))
        host = {}
        for lo, hi in SWEEPS:
            t = []
            for _ in range(args.host_repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = out[:, :25].contiguous().cpu().numpy()
                t1 = time.perf_counter()
                score.frame_sums_numpy(m, est_truth, layout, (lo, hi), starts, skip)
                t.append((t1 - t0, time.perf_counter() - t1))
            host[str(hi - lo + 1)] = {"copy_ms": round(1e3 * float(np.median([x[0] for x in t])), 3),
                                      "numpy_ms": round(1e3 * float(np.median([x[1] for x in t])), 1),
                                      "numpy_range_ms": [round(1e3 * min(x[1] for x in t), 1), round(1e3 * max(x[1] for x in t), 1)]}
        result["host_route"] = host
        del est
    lines = [MARKER + f" (`python tools/frame_fit_bench.py --frames {F} --repeats {args.repeats}`, one MI355X)", "",
             f"{F} pocket frames in {RECORDINGS} recordings of equal length, `[F, 196]` float64 rows from `process_recording(spread=True)` at {n_mc} "
             "samples, truth as NN targets.  Medians (and the smallest and largest of the repeats) of HIP events around the Python calls, the "
             "legs alternating within one session behind three warm-up rounds; the host route by the host clock.  Nothing was fixed in advance.", "",
             "| L | lags | `frame_sums` | `score_lags` (with spread, accumulators only) | ratio | host: copy + `frame_sums_numpy` |", "|---|---|---|---|---|---|"]
    for L, d in result["sweeps"].items():
        h = result["host_route"][L]
        lines.append(f"| {L} | {d['lags'][0]} .. {d['lags'][1]} | {d['frame_sums_ms']:.3f} ms ({d['frame_sums_range'][0]:.3f} .. {d['frame_sums_range'][1]:.3f}) | "
                     f"{d['score_lags_ms']:.3f} ms ({d['score_lags_range'][0]:.3f} .. {d['score_lags_range'][1]:.3f}) | {d['ratio_sums_over_lags']:.2f} x | "
                     f"{h['copy_ms']:.2f} ms + {h['numpy_ms']:.0f} ms ({h['numpy_range_ms'][0]:.0f} .. {h['numpy_range_ms'][1]:.0f}) |")
    r = result["rotate_rows"]
    lines += ["", f"`rotate_rows` (rows and spread records): {r['ms']:.3f} ms ({r['range'][0]:.3f} .. {r['range'][1]:.3f}); it moves {r['bytes_moved'] / 1e6:.1f} MB, "
              f"{100 * r['share_of_hbm_peak']:.1f} % of the 8 TB/s HBM peak over that time.", "",
              f"`align_frame` end to end over lags {SWEEPS[0][0]} .. {SWEEPS[0][1]} (with the wait for `best_frame` on the host): {result['align_frame_ms']:.3f} ms "
              f"({result['align_frame_range'][0]:.3f} .. {result['align_frame_range'][1]:.3f}).", ""]
    old = Path(args.out).read_text() if Path(args.out).exists() else ""
    notes = "\n" + old[old.index(NOTES):] if NOTES in old else ""
    Path(args.out).write_text((old[:old.index(MARKER)] if MARKER in old else old.rstrip() + "\n\n") + "\n".join(lines) + notes)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
