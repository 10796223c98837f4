"""Scoring over a sweep of time lags (score.score_lags / ape_score_lags) on the workload of profiles/score.md: 100 000
pocket frames in 10 recordings, `[F, 196]` float64 rows from process_recording(spread=True) at 25 Monte-Carlo samples, truth as NN
targets, accumulators only.  Legs, alternating within one session behind warmed shapes, timed by HIP events:

    lags L     one ape_score_lags call over L = 1, 17 and 65 lags
    rows x L   the route a user has without it: L calls of ape_score_rows on row-shifted views (wrong at every recording boundary, on a
               different frame set per lag -- timed for its cost only)
    rows       at L = 1, ape_score_rows itself

and the bytes each route must read.  With --parent-tree DIR (a checkout of the parent commit with its library built) ape_score_rows is
also timed in child processes that alternate between that tree and this one, three runs each: this build's median against the
parent's own run-to-run range.  Writes profiles/score_lags.md's measured section and prints ONE JSON line.

    python tools/score_lags_bench.py [--frames 100000] [--repeats 20] [--parent-tree DIR] [--out profiles/score_lags.md]

Models carry seeded synthetic weights, rows and truth are synthetic: the times do not depend on the values."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
TREE = Path(os.environ.get("APE_BENCH_TREE", ROOT))          # (the child legs on the parent commit run against THAT tree's package and library)
for _p in (str(TREE), str(TREE / "arm-pose-estimation_amd"), str(ROOT / "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SWEEPS = ((0, 0), (-8, 8), (-32, 32))
RUNS = 3
MARKER, NOTES = "## Measured", "### Reading the figures"       # the section this tool writes; what follows it is written by hand and kept


def alternate(legs, repeats, warmup=3):
    """legs: name -> callable; every repeat runs each leg once, in turn, between two events; -> name -> (median ms, all)"""
    import torch
    for _ in range(warmup):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, f in legs.items():
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            keep = f()
            z.record()
            z.synchronize()
            ms[k].append(a.elapsed_time(z))
            del keep
    return {k: (float(np.median(v)), [round(x, 4) for x in v]) for k, v in ms.items()}


def synthetic(F, rng):
    """[F, 196] rows with a finite message and usable spread records, [F, 14] finite targets"""
    import torch
    rows = rng.normal(size=(F, 196))
    rows[:, 175 + 3:175 + 9] = rows[:, 175 + 12:175 + 18] = [0.01, 0.0, 0.0, 0.01, 0.0, 0.01]
    return torch.from_numpy(rows).cuda(), torch.from_numpy(rng.normal(size=(F, 14))).cuda()


def child_unchanged(args):
    """ape_score_rows of whichever tree APE_BENCH_TREE names, accumulators only and with per-frame rows: medians in ms"""
    import torch
    from wear_mocap_ape_amd import score
    torch.cuda.set_device(0)
    rows, truth = synthetic(args.frames, np.random.default_rng(7))
    msg, rec, starts = rows[:, :-21], rows[:, -21:], list(range(0, args.frames, 10_000))
    res = alternate({"acc_only": lambda: score.score_rows(0, msg, truth, "targets", rec, starts, 5, per_frame=False),
                     "per_frame": lambda: score.score_rows(0, msg, truth, "targets", rec, starts, 5)}, args.repeats)
    print(json.dumps({k: round(v[0], 4) for k, v in res.items()}))


def leg_unchanged(args):
    res = {"parent": [], "new": []}
    for _ in range(RUNS):
        for tag, tree in (("parent", args.parent_tree), ("new", None)):
            env = dict(os.environ)
            env.pop("APE_HIP_LIB", None)
            env.pop("APE_BENCH_TREE", None)
            if tree:
                env["APE_BENCH_TREE"] = str(Path(tree).resolve())
            r = subprocess.run([sys.executable, __file__, "--child-unchanged", "--frames", str(args.frames), "--repeats", str(args.repeats)],
                               env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            res[tag].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {}
    for k in ("acc_only", "per_frame"):
        p, n = [d[k] for d in res["parent"]], [d[k] for d in res["new"]]
        out[k] = {"parent_ms": p, "new_ms": n, "new_median_within_parent_range": bool(min(p) <= float(np.median(n)) <= max(p))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-unchanged", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "score_lags.md"))
    args = ap.parse_args()
    if args.child_unchanged:         # (the tree's library as it stands: nothing is built on the way)
        child_unchanged(args)
        return
    import __graft_entry__ as entry
    entry.build()
    import torch
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return
    from replay_bench import deploy_tree, rows_for
    from wear_mocap_ape_amd import config, score
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import WatchPhonePocketNN
    torch.cuda.set_device(0)
    F, n_mc = args.frames, 25
    rng = np.random.default_rng(7)
    result = {"frames": F, "n_mc": n_mc, "repeats": args.repeats, "sweeps": {}}
    with tempfile.TemporaryDirectory() as tmp:
        shipped, deploy = Path(config.PATHS["deploy"]), Path(tmp) / "deploy"
        config.PATHS["deploy"] = deploy
        est = WatchPhonePocketNN(model_hash=deploy_tree(shipped, deploy, "pocket", 0.2), smooth=1, add_mc_samples=True, monte_carlo_samples=n_mc)
        starts = list(range(0, F, 10_000))
        out, rec = est.process_recording(torch.from_numpy(rows_for("pocket", F)).cuda(), starts=starts, spread=True)
        truth = torch.from_numpy(rng.normal(size=(F, 14))).cuda()
        layout, skip, body = est._layout, est.sequence_len - 1, est.body_measurements
        torch.cuda.synchronize()

        def shifted(lo, hi):
            """L calls of score_rows on row-shifted views: message f against truth f - l on the frames both views have"""
            res = []
            for l in range(lo, hi + 1):
                a, b = max(0, l), F + min(0, l)
                res.append(score.score_rows(layout, out[a:b], truth[a - l:b - l], "targets", rec[a:b], [0] + [s - a for s in starts if a < s < b],
                                            skip, body, per_frame=False)[1])
            return res

        legs = {}
        for lo, hi in SWEEPS:
            L = hi - lo + 1
            legs[f"lags_{L}"] = lambda lo=lo, hi=hi: score.score_lags(layout, out, truth, (lo, hi), "targets", rec, starts, skip, body)[1]
            legs[f"rows_x{L}"] = lambda lo=lo, hi=hi: shifted(lo, hi)
        legs["rows"] = lambda: score.score_rows(layout, out, truth, "targets", rec, starts, skip, body, per_frame=False)[1]
        times = alternate(legs, args.repeats)
        row_bytes = (25 + 21 + 14) * 8
        for lo, hi in SWEEPS:
            L = hi - lo + 1
            one, many = times[f"lags_{L}"], times[f"rows_x{L}"]
            blocks = (F + 255) // 256
            result["sweeps"][str(L)] = {
                "lags": [lo, hi], "score_lags_ms": round(one[0], 4), "score_lags_all": one[1], "rows_x_L_ms": round(many[0], 4),
                "rows_x_L_all": many[1], "ratio_rows_x_L_over_lags": round(many[0] / one[0], 2),
                # one pass: every message and spread row once, every truth row once per workgroup whose window holds it (256 own + halo)
                "lags_must_read_bytes": F * (25 + 21) * 8 + (F + blocks * (max(0, hi) + max(0, -lo))) * 14 * 8,
                "rows_x_L_must_read_bytes": L * F * row_bytes,
                "partial_records_bytes": (blocks + len(starts)) * L * 25 * 8}
        result["score_rows_ms"] = round(times["rows"][0], 4)
        result["score_rows_all"] = times["rows"][1]
        del est
    result["unchanged"] = leg_unchanged(args) if args.parent_tree else "unmeasured: no --parent-tree given"
    lines = [MARKER + f" (`python tools/score_lags_bench.py --frames {F} --repeats {args.repeats}`, one MI355X)", "",
             f"{F} pocket frames in {len(starts)} recordings, `[F, 196]` float64 rows from `process_recording(spread=True)` at {n_mc} samples, truth as "
             "NN targets, accumulators only.  Medians of HIP events around the Python calls, the legs alternating within one session behind "
             "three warm-up rounds.  Nothing was fixed in advance.", "",
             "| L | lags | `score_lags` | L x `score_rows` on shifted views | ratio | one pass must read | L passes must read |", "|---|---|---|---|---|---|---|"]
    for L, d in result["sweeps"].items():
        lines.append(f"| {L} | {d['lags'][0]} .. {d['lags'][1]} | {d['score_lags_ms']:.3f} ms | {d['rows_x_L_ms']:.3f} ms | {d['ratio_rows_x_L_over_lags']:.2f} x | "
                     f"{d['lags_must_read_bytes'] / 1e6:.1f} MB | {d['rows_x_L_must_read_bytes'] / 1e6:.1f} MB |")
    lines += ["", f"`score_rows` itself (the L = 1 comparison): {result['score_rows_ms']:.3f} ms.", ""]
    if isinstance(result["unchanged"], dict):
        lines += ["`ape_score_rows` on this build beside a build of the parent commit (child processes alternating between the two trees, "
                  f"{RUNS} runs each, synthetic rows of the same shape; medians in ms):", "",
                  "| call | parent runs | this build's runs | this build's median within the parent's range |", "|---|---|---|---|"]
        for k, d in result["unchanged"].items():
            lines.append(f"| {k} | {d['parent_ms']} | {d['new_ms']} | {'yes' if d['new_median_within_parent_range'] else 'no'} |")
        lines.append("")
    old = Path(args.out).read_text() if Path(args.out).exists() else ""
    notes = "\n" + old[old.index(NOTES):] if NOTES in old else ""
    Path(args.out).write_text((old[:old.index(MARKER)] if MARKER in old else old.rstrip() + "\n\n") + "\n".join(lines) + notes)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
