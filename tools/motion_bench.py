"""Speed, acceleration and jerk of a replay (score.motion_sums / ape_motion_sums): 100 000 pocket frames in 64 recordings
of equal length, the `[25, F, 25]` rows of one `repost` over 25 smoothing lengths at 25 Monte-Carlo samples, as float64 and as float32,
on a jittered clock.  Legs, alternating within one session behind warmed shapes, timed by HIP events:

    motion C acc     one ape_motion_sums call over C = 1 and 25 sets, accumulators only
    motion C rows    the same with the per-frame rows written
    score acc/rows   ape_score_rows on the first set against est truth: the yardstick for a one-pass scoring kernel

with the bytes each motion call must read (and write) over its time against the 8 TB/s HBM peak; by the host clock the route it replaces,
a copy of the rows to the host plus score.motion_sums_numpy (one set; 25 sets are 25 of them).  With --parent-tree DIR (a checkout of the
parent commit with its library built) ape_score_rows, ape_score_lags (17 lags) and ape_post_sweep (7 configurations, 20 000 frames) are
timed in child processes that alternate between that tree and this one, three runs each: this build's median against the parent's own
run-to-run range.  Writes profiles/motion.md's measured section and prints ONE JSON line.

    python tools/motion_bench.py [--frames 100000] [--repeats 20] [--host-repeats 3] [--parent-tree DIR] [--out profiles/motion.md]

Models carry seeded synthetic weights, rows are synthetic: the times do not depend on the values."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
TREE = Path(os.environ.get("APE_BENCH_TREE", ROOT))          # (the child legs on the parent commit run against THAT tree's package and library)
for _p in (str(TREE), str(TREE / "arm-pose-estimation_amd"), str(ROOT / "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

RECORDINGS, SETS, RUNS = 64, 25, 3
HBM_PEAK = 8.0e12                                           # bytes / s
POST_CONFIGS = [(1, 1), (1, 6), (2, 1), (3, 6), (7, 6), (7, 4), (5, 2)]
MARKER, NOTES = "## Measured", "### Reading the figures"   # the section this tool writes; what follows it is written by hand and kept


def spread_of(v):
    return [round(min(v), 4), round(max(v), 4)]


def pocket_estimator(tmp, n_mc):
    from replay_bench import deploy_tree
    from wear_mocap_ape_amd import config
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import WatchPhonePocketNN
    shipped, deploy = Path(config.PATHS["deploy"]), Path(tmp) / "deploy"
    config.PATHS["deploy"] = deploy
    return WatchPhonePocketNN(model_hash=deploy_tree(shipped, deploy, "pocket", 0.2), smooth=1, add_mc_samples=True, monte_carlo_samples=n_mc)


def child_unchanged(args):
    """score_rows, score_lags and post_sweep of whichever tree APE_BENCH_TREE names: medians in ms"""
    import torch
    from replay_bench import rows_for
    from score_lags_bench import alternate, synthetic
    from wear_mocap_ape_amd import score
    torch.cuda.set_device(0)
    rows, truth = synthetic(args.frames, np.random.default_rng(7))
    msg, rec, starts = rows[:, :-21], rows[:, -21:], [r * args.frames // RECORDINGS for r in range(RECORDINGS)]
    with tempfile.TemporaryDirectory() as tmp:
        est = pocket_estimator(tmp, 6)
        n = min(args.frames, 20_000)
        st = [r * n // RECORDINGS for r in range(RECORDINGS)]
        _, y = est.process_recording(torch.from_numpy(rows_for("pocket", n)).cuda(), starts=st, return_targets=True)
        res = alternate({"score_rows": lambda: score.score_rows(0, msg, truth, "targets", rec, starts, 5, per_frame=False),
                         "score_lags": lambda: score.score_lags(0, msg, truth, (-8, 8), "targets", rec, starts, 5),
                         "post_sweep": lambda: est.repost(y, POST_CONFIGS, starts=st, spread=True)}, args.repeats)
        del est
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
    for k in ("score_rows", "score_lags", "post_sweep"):
        p, n = [d[k] for d in res["parent"]], [d[k] for d in res["new"]]
        out[k] = {"parent_ms": p, "new_ms": n, "new_median_within_parent_range": bool(min(p) <= float(np.median(n)) <= max(p))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-unchanged", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "motion.md"))
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
    from replay_bench import rows_for
    from score_lags_bench import alternate
    from wear_mocap_ape_amd import _hip, score
    torch.cuda.set_device(0)
    F, n_mc = args.frames, 25
    rng = np.random.default_rng(7)
    result = {"frames": F, "n_mc": n_mc, "recordings": RECORDINGS, "sets": SETS, "repeats": args.repeats, "motion": {}}
    with tempfile.TemporaryDirectory() as tmp:
        est = pocket_estimator(tmp, n_mc)
        starts = [r * F // RECORDINGS for r in range(RECORDINGS)]
        _, y = est.process_recording(torch.from_numpy(rows_for("pocket", F)).cuda(), starts=starts, return_targets=True)
        sets64 = est.repost(y, score.grid(range(1, SETS + 1), (n_mc,)), starts=starts)
        del y
        layout, skip, body = est._layout, est.sequence_len - 1, est.body_measurements
        dt = 0.02 * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=F))
        clock = score.frame_times(torch.from_numpy(dt).cuda(), starts)
        truth = torch.from_numpy(rng.normal(size=(F, _hip.EST_WIDTH[layout]))).cuda()
        torch.cuda.synchronize()
        rows = {"float64": sets64, "float32": sets64.float()}
        legs = {}
        for name, r in rows.items():
            for C_ in (1, SETS):
                view = r[0] if C_ == 1 else r
                legs[f"motion_{C_}_acc_{name}"] = lambda v=view: score.motion_sums(layout, v, "msg", starts, skip, clock)
                legs[f"motion_{C_}_rows_{name}"] = lambda v=view: score.motion_sums(layout, v, "msg", starts, skip, clock, per_frame=True)
            t = truth if name == "float64" else truth.float()
            legs[f"score_acc_{name}"] = lambda v=r[0], t=t: score.score_rows(layout, v, t, "est", None, starts, skip, body, per_frame=False)
            legs[f"score_rows_{name}"] = lambda v=r[0], t=t, o=r.dtype: score.score_rows(layout, v, t, "est", None, starts, skip, body, o)
        times = alternate(legs, args.repeats)
        for name, r in rows.items():
            size = r.element_size()
            for C_ in (1, SETS):
                for what in ("acc", "rows"):
                    ms, allv = times[f"motion_{C_}_{what}_{name}"]
                    moved = C_ * F * (25 * size + 8) + (C_ * F * 12 * size if what == "rows" else 0)
                    result["motion"][f"{name}_{C_}_{what}"] = {"ms": round(ms, 4), "range": spread_of(allv), "bytes_moved": moved,
                                                               "share_of_hbm_peak": round(moved / (ms * 1e-3) / HBM_PEAK, 4)}
            for what in ("acc", "rows"):
                ms, allv = times[f"score_{what}_{name}"]
                result["motion"][f"{name}_score_{what}"] = {"ms": round(ms, 4), "range": spread_of(allv)}

        # the route it replaces: the rows to the host, then the numpy statement (one set)
        host, clock_h = [], clock.cpu().numpy()
        for _ in range(args.host_repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = sets64[0].cpu().numpy()
            t1 = time.perf_counter()
            score.motion_sums_numpy(m, layout, "msg", starts, skip, clock_h)
            host.append((t1 - t0, time.perf_counter() - t1))
        result["host_route_one_set"] = {"copy_ms": round(1e3 * float(np.median([x[0] for x in host])), 3),
                                        "numpy_ms": round(1e3 * float(np.median([x[1] for x in host])), 1),
                                        "numpy_range_ms": [round(1e3 * min(x[1] for x in host), 1), round(1e3 * max(x[1] for x in host), 1)]}
        del est
    result["unchanged"] = leg_unchanged(args) if args.parent_tree else "unmeasured: no --parent-tree given"
    lines = [MARKER + f" (`python tools/motion_bench.py --frames {F} --repeats {args.repeats}`, one MI355X)", "",
             f"{F} pocket frames in {RECORDINGS} recordings of equal length, the `[{SETS}, F, 25]` rows of one `repost` over smoothing lengths 1 .. {SETS} at "
             f"{n_mc} samples, message rows on a jittered clock.  Medians (and the smallest and largest of the repeats) of HIP events around the Python "
             "calls, the legs alternating within one session behind three warm-up rounds; the host route by the host clock.  Bytes: every row value "
             "and stamp read once, every per-frame value written once.  Nothing was fixed in advance.", "",
             "| rows | sets | output | `motion_sums` | bytes moved | share of the 8 TB/s HBM peak | `score_rows` on one set (same session) |", "|---|---|---|---|---|---|---|"]
    for name in ("float64", "float32"):
        for C_ in (1, SETS):
            for what, label in (("acc", "accumulators"), ("rows", "accumulators + per-frame rows")):
                d, s = result["motion"][f"{name}_{C_}_{what}"], result["motion"][f"{name}_score_{what}"]
                lines.append(f"| {name} | {C_} | {label} | {d['ms']:.3f} ms ({d['range'][0]:.3f} .. {d['range'][1]:.3f}) | {d['bytes_moved'] / 1e6:.1f} MB | "
                             f"{100 * d['share_of_hbm_peak']:.1f} % | {s['ms']:.3f} ms ({s['range'][0]:.3f} .. {s['range'][1]:.3f}) |")
    h = result["host_route_one_set"]
    lines += ["", f"The route it replaces, one set: D2H copy {h['copy_ms']:.2f} ms + `motion_sums_numpy` {h['numpy_ms']:.0f} ms "
              f"({h['numpy_range_ms'][0]:.0f} .. {h['numpy_range_ms'][1]:.0f}); {SETS} sets are {SETS} of them.", ""]
    if isinstance(result["unchanged"], dict):
        lines += ["Untouched entries on this build beside a build of the parent commit (child processes alternating between the two trees, "
                  f"{RUNS} runs each, synthetic rows; medians in ms; `score_lags` over 17 lags, `post_sweep` of 7 configurations on 20 000 frames):", "",
                  "| call | parent runs | this build's runs | this build's median within the parent's range |", "|---|---|---|---|"]
        for k, d in result["unchanged"].items():
            lines.append(f"| {k} | {d['parent_ms']} | {d['new_ms']} | {'yes' if d['new_median_within_parent_range'] else 'no'} |")
        lines.append("")
    else:
        lines += ["Untouched entries against a build of the parent commit: not measured in this run (`--parent-tree`).", ""]
    old = Path(args.out).read_text() if Path(args.out).exists() else ""
    notes = "\n" + old[old.index(NOTES):] if NOTES in old else ""
    Path(args.out).write_text((old[:old.index(MARKER)] if MARKER in old else old.rstrip() + "\n\n") + "\n".join(lines) + notes)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
