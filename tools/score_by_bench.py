"""Errors by condition (score.stats_by / ape_score_by): 100 000 pocket frames, as 64 recordings of equal length and as one
recording; keys: the 7 joint angles of every frame, values: the 7 score columns, 36 bins per key column (`angle_edges(36)`); one set and
25 sets (keys and values per set).  Legs, alternating within one session behind warmed shapes, timed by HIP events, three runs each:

    stats_by         one ape_score_by call
    stats_by f32     the same on float32 keys and values
    torch            the same cells on the device by torch.bucketize per key column, one index_add_ of [x, x^2, 1] and one index_reduce_
                     (amax) per key column: float atomics; the tool also reports whether two runs of it agree in bits

and by the host clock the route it replaces: a copy of keys and values to the host plus the cells by np.bincount with weights (the
vectorised equivalent of score.stats_by_numpy: the same cells, not its order of summation).  With --parent-tree DIR (a checkout of the
parent commit with its library built) score_rows, hist_rows and joint_angles are timed in child processes that alternate between that
tree and this one, three runs each: this build's median against the parent's own run-to-run range, and by how much it lies outside; and
the object hashes of the two builds (lib/build_info.json) are compared.  Writes profiles/score_by.md's measured section and prints ONE
JSON line.

    python tools/score_by_bench.py [--frames 100000] [--repeats 20] [--parent-tree DIR] [--out profiles/score_by.md]

Rows are synthetic: the time of the call depends on the values only through which lane of a wave a frame's slot belongs to."""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
TREE = Path(os.environ.get("APE_BENCH_TREE", ROOT))          # (the child legs on the parent commit run against THAT tree's package and library)
for _p in (str(TREE), str(TREE / "arm-pose-estimation_amd"), str(ROOT / "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

RECORDINGS, SETS, RUNS, BINS = 64, 25, 3, 36
MARKER, NOTES = "## Measured", "### Reading the figures"   # the section this tool writes; what follows it is written by hand and kept


def spread_of(v):
    return [round(min(v), 4), round(max(v), 4)]


def child_unchanged(args):
    """score_rows, hist_rows and joint_angles of whichever tree APE_BENCH_TREE names: medians in ms"""
    import torch
    from score_lags_bench import alternate, synthetic
    from wear_mocap_ape_amd import score
    torch.cuda.set_device(0)
    F = args.frames
    rows, truth = synthetic(F, np.random.default_rng(7))
    msg, rec, starts = rows[:, :-21], rows[:, -21:], [r * F // RECORDINGS for r in range(RECORDINGS)]
    real, _ = score.score_rows(0, msg, truth, "targets", rec, starts, 5)
    edges = score.default_edges("score", 64)
    sets = torch.from_numpy(np.random.default_rng(8).normal(size=(SETS, F, 25))).cuda()
    res = alternate({"score_rows": lambda: score.score_rows(0, msg, truth, "targets", rec, starts, 5, per_frame=False),
                     "hist_rows": lambda: score.hist_rows(real, edges, starts, 5),
                     "joint_angles": lambda: score.joint_angles(0, sets, "msg", None, "est", starts, 5, per_frame=False)}, args.repeats)
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
    for k in ("score_rows", "hist_rows", "joint_angles"):
        p, n = [d[k] for d in res["parent"]], [d[k] for d in res["new"]]
        med = float(np.median(n))
        out[k] = {"parent_ms": p, "new_ms": n, "new_median_within_parent_range": bool(min(p) <= med <= max(p)),
                  "outside_by_ms": round(max(min(p) - med, med - max(p), 0.0), 4)}
    return out


def object_hashes(parent_tree):
    """which of the parent's objects keep their SHA-256 in this build (lib/build_info.json of both trees)"""
    def load(tree):
        return json.loads((Path(tree) / "arm-pose-estimation_amd" / "lib" / "build_info.json").read_text())["objects"]
    try:
        old, new = load(parent_tree), load(ROOT)
    except Exception as e:                                  # noqa: BLE001
        return f"not measured: {e}"
    return {"parent_objects": len(old), "kept": sorted(k for k in old if new.get(k) == old[k]), "changed": sorted(k for k in old if new.get(k) != old[k]),
            "added": sorted(k for k in new if k not in old)}


def torch_route(keys, values, edges_dev, rec_of, R):
    """keys [C, F, K], values [C, F, V] on the device -> (sums [C R K (B + 3), 3 V], maxima [.., V]) by bucketize per key column,
    index_add_ and index_reduce_ (slot order: torch's own, NaN keys in a slot of their own)"""
    import torch
    Cn, F, K = keys.shape
    V = values.shape[2]
    S = edges_dev.shape[1] + 2
    ok = ~torch.isnan(values)
    x = torch.where(ok, values, torch.zeros_like(values))
    payload = torch.cat([x, x * x, ok.double()], dim=2).reshape(Cn * F, 3 * V)
    tops = torch.where(ok, values, torch.full_like(values, -float("inf"))).reshape(Cn * F, V)
    sums = torch.zeros((Cn * R * K * S, 3 * V), dtype=torch.float64, device=keys.device)
    maxima = torch.full((Cn * R * K * S, V), -float("inf"), dtype=torch.float64, device=keys.device)
    base = (torch.arange(Cn, device=keys.device)[:, None] * R + rec_of[None, :]) * K
    for k in range(K):
        col = keys[:, :, k].contiguous()
        idx = torch.bucketize(col, edges_dev[k]) + torch.isnan(col) * 1
        flat = ((base + k) * S + idx).reshape(-1)
        sums.index_add_(0, flat, payload)
        maxima.index_reduce_(0, flat, tops, "amax", include_self=True)
    return sums, maxima


def host_route(keys, values, edges, rec_of, R):
    """the same cells on the host: searchsorted per key column, np.bincount with weights per value column"""
    Cn, F, K = keys.shape
    V = values.shape[2]
    S = edges.shape[1] + 2
    out = np.zeros((Cn, R, K, S, V, 4))
    for c in range(Cn):
        ok = ~np.isnan(values[c])
        x = np.where(ok, values[c], 0.0)
        for k in range(K):
            i = np.searchsorted(edges[k], keys[c, :, k], side="left")
            slot = np.where(np.isnan(keys[c, :, k]), S - 1, np.where(i == 0, S - 3, np.where(i > S - 3, S - 2, i - 1)))
            cell = rec_of * S + slot
            for v in range(V):
                out[c, :, k, :, v, 0] = np.bincount(cell, weights=ok[:, v].astype(np.float64), minlength=R * S).reshape(R, S)
                out[c, :, k, :, v, 1] = np.bincount(cell, weights=x[:, v], minlength=R * S).reshape(R, S)
                out[c, :, k, :, v, 2] = np.bincount(cell, weights=x[:, v] * x[:, v], minlength=R * S).reshape(R, S)
            order = np.argsort(cell, kind="stable")                         # the maxima: one reduceat over the frames sorted by cell
            at = np.flatnonzero(np.r_[True, np.diff(cell[order]) > 0])
            top = np.full((R * S, V), -np.inf)
            top[cell[order][at]] = np.maximum.reduceat(np.where(ok, values[c], -np.inf)[order], at, axis=0)
            out[c, :, k, :, :, 3] = top.reshape(R, S, V)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-unchanged", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "score_by.md"))
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
    from score_lags_bench import alternate, synthetic
    from wear_mocap_ape_amd import score
    torch.cuda.set_device(0)
    F = args.frames
    rng = np.random.default_rng(7)
    edges = score.angle_edges(BINS)[:7]
    edges_dev = torch.from_numpy(edges).cuda()
    result = {"frames": F, "sets": SETS, "bins": BINS, "repeats": args.repeats, "runs": RUNS, "by": {}, "host_route": {}}

    # the planted replay: synthetic messages against synthetic targets; per set the angles of its messages and its score rows
    rows, truth = synthetic(F, rng)
    rec = rows[:, -21:]
    sets_msg = torch.from_numpy(rng.normal(size=(SETS, F, 25))).cuda()
    keys, _, _ = score.joint_angles(0, sets_msg, "msg", None, "est", [0], 0, per_frame=True)                     # [25, F, 7]
    values = torch.stack([score.score_rows(0, sets_msg[c], truth, "targets", rec, [0], 0)[0] for c in range(SETS)])   # [25, F, 7]
    torch.cuda.synchronize()

    for tag, starts in (("64 recordings", [r * F // RECORDINGS for r in range(RECORDINGS)]), ("1 recording", [0])):
        R = len(starts)
        rec_np = np.searchsorted(np.asarray(starts), np.arange(F), side="right") - 1
        rec_of = torch.from_numpy(rec_np).cuda()
        for Cn in (1, SETS):
            k, v = keys[:Cn], values[:Cn]
            k32, v32 = k.float(), v.float()
            got = score.stats_by(k, v, edges, starts, 5)
            # the routes agree before anything is timed: the device's bits are the host statement's on the first recording of the first set
            ref = score.stats_by_numpy(k[0].cpu().numpy(), v[0].cpu().numpy(), edges, starts, 5)
            g0 = got[0].cpu().numpy()
            assert np.array_equal(np.isnan(g0), np.isnan(ref)) and np.array_equal(g0[~np.isnan(g0)].view(np.int64), ref[~np.isnan(ref)].view(np.int64)), tag
            a, b = torch_route(k, v, edges_dev, rec_of, R), torch_route(k, v, edges_dev, rec_of, R)
            torch.cuda.synchronize()
            agree = bool(torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)))
            legs = {"stats_by": lambda k=k, v=v: score.stats_by(k, v, edges, starts, 5),
                    "stats_by_float32": lambda k=k32, v=v32: score.stats_by(k, v, edges, starts, 5),
                    "torch": lambda k=k, v=v: torch_route(k, v, edges_dev, rec_of, R)}
            runs = [alternate(legs, args.repeats) for _ in range(RUNS)]
            entry_ = {name: {"ms": [round(r[name][0], 4) for r in runs], "range": spread_of([x for r in runs for x in r[name][1]])} for name in legs}
            entry_["torch_two_runs_agree_in_bits"] = agree
            result["by"][f"{tag}, {Cn} set" + ("s" if Cn > 1 else "")] = entry_
            host = []
            for _ in range(RUNS if Cn == 1 else 1):            # (25 sets are 25 of one set's: once)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                kh, vh = k.cpu().numpy(), v.cpu().numpy()
                t1 = time.perf_counter()
                host_route(kh, vh, edges, rec_np, R)
                host.append((t1 - t0, time.perf_counter() - t1))
            result["host_route"][f"{tag}, {Cn} set" + ("s" if Cn > 1 else "")] = {
                "copy_ms": [round(1e3 * x[0], 3) for x in host], "numpy_ms": [round(1e3 * x[1], 1) for x in host]}
    result["unchanged"] = leg_unchanged(args) if args.parent_tree else "not measured: no --parent-tree given"
    result["objects"] = object_hashes(args.parent_tree) if args.parent_tree else "not measured: no --parent-tree given"

    lines = [MARKER + f" (`python tools/score_by_bench.py --frames {F} --repeats {args.repeats}`, one MI355X)", "",
             f"{F} frames; keys the 7 joint angles `[C, F, 7]`, values the 7 score columns `[C, F, 7]`, float64, {BINS} bins per key column "
             f"(`angle_edges({BINS})`), skip 5.  Medians of {RUNS} runs of {args.repeats} repeats each (and the smallest and largest of all repeats) of HIP "
             "events around the Python calls, the legs alternating within one session behind three warm-up rounds; the host route by the host "
             "clock.  Nothing was fixed in advance.", "",
             "| workload | `stats_by` | `stats_by`, float32 | torch `bucketize` + `index_add_` | two torch runs agree in bits | host: D2H copy + numpy |",
             "|---|---|---|---|---|---|"]
    for key, d in result["by"].items():
        h = result["host_route"][key]
        cell = lambda e: f"{e['ms']} ms ({e['range'][0]:.3f} .. {e['range'][1]:.3f})"      # noqa: E731
        lines.append(f"| {key} | {cell(d['stats_by'])} | {cell(d['stats_by_float32'])} | {cell(d['torch'])} | "
                     f"{'yes' if d['torch_two_runs_agree_in_bits'] else 'no'} | {h['copy_ms']} + {h['numpy_ms']} ms |")
    lines.append("")
    if isinstance(result["unchanged"], dict):
        lines += ["Untouched entries on this build beside a build of the parent commit (child processes alternating between the two trees, "
                  f"{RUNS} runs each, synthetic rows; medians in ms; `joint_angles` of {SETS} sets, accumulators only):", "",
                  "| call | parent runs | this build's runs | this build's median within the parent's range | outside by |", "|---|---|---|---|---|"]
        for k, d in result["unchanged"].items():
            lines.append(f"| {k} | {d['parent_ms']} | {d['new_ms']} | {'yes' if d['new_median_within_parent_range'] else 'no'} | {d['outside_by_ms']} ms |")
        lines.append("")
    else:
        lines += ["Untouched entries against a build of the parent commit: not measured in this run (`--parent-tree`).", ""]
    o = result["objects"]
    if isinstance(o, dict):
        lines += [f"Objects: {len(o['kept'])} of the parent's {o['parent_objects']} keep their SHA-256 in this build"
                  + (f"; changed: {', '.join(o['changed'])}" if o["changed"] else "") + f"; added: {', '.join(o['added']) or 'none'}.", ""]
    else:
        lines += [f"Object hashes against the parent's build: {o}.", ""]
    old = Path(args.out).read_text() if Path(args.out).exists() else ""
    notes = "\n" + old[old.index(NOTES):] if NOTES in old else ""
    Path(args.out).write_text((old[:old.index(MARKER)] if MARKER in old else old.rstrip() + "\n\n") + "\n".join(lines) + notes)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
