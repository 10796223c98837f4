"""Error distributions per recording (score.hist_rows / ape_score_hist): 100 000 frames in 64 recordings of equal length
(the workload of 4.31), two inputs: score rows `[F, 7]` over 64 bins per column, and the motion rows `[25, F, 12]` of 25 sets.  Legs,
alternating within one session behind warmed shapes, timed by HIP events:

    hist uniform     one ape_score_hist call on values spread uniformly over the bins of every column
    hist one bin     the same with every value in one bin: the most same-address adds a wave can make
    hist real        the call on the rows the scorers wrote for a planted replay (score_rows; motion_sums for the motion input)
    hist many        the score input cut into recordings of 5 frames: every tile adds to the output directly
    torch            the same counts on the device by torch.bucketize per column and one flat torch.bincount
    scorer           score_rows (accumulators only) / motion_sums (accumulators only) on the same rows, as a yardstick

with the bytes a call must read over its time against the 8 TB/s HBM peak; by the host clock the route it replaces, a copy of the rows to
the host plus score.hist_numpy.  With --parent-tree DIR (a checkout of the parent commit with its library built) score_rows, score_lags
(17 lags) and motion_sums (25 sets) are timed in child processes that alternate between that tree and this one, three runs each: this
build's median against the parent's own run-to-run range; and the object hashes of the two builds (lib/build_info.json) are compared.
Writes profiles/score_hist.md's measured section and prints ONE JSON line.

    python tools/score_hist_bench.py [--frames 100000] [--repeats 20] [--host-repeats 3] [--parent-tree DIR] [--out profiles/score_hist.md]

Rows are synthetic: the times of the scorers do not depend on the values, those of the histogram do only through the bins hit."""
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

RECORDINGS, SETS, RUNS, BINS = 64, 25, 3, 64
HBM_PEAK = 8.0e12                                           # bytes / s
MARKER, NOTES = "## Measured", "### Reading the figures"   # the section this tool writes; what follows it is written by hand and kept


def spread_of(v):
    return [round(min(v), 4), round(max(v), 4)]


def child_unchanged(args):
    """score_rows, score_lags and motion_sums of whichever tree APE_BENCH_TREE names: medians in ms"""
    import torch
    from score_lags_bench import alternate, synthetic
    from wear_mocap_ape_amd import score
    torch.cuda.set_device(0)
    F = args.frames
    rows, truth = synthetic(F, np.random.default_rng(7))
    msg, rec, starts = rows[:, :-21], rows[:, -21:], [r * F // RECORDINGS for r in range(RECORDINGS)]
    sets = torch.from_numpy(np.random.default_rng(8).normal(size=(SETS, F, 25))).cuda()
    res = alternate({"score_rows": lambda: score.score_rows(0, msg, truth, "targets", rec, starts, 5, per_frame=False),
                     "score_lags": lambda: score.score_lags(0, msg, truth, (-8, 8), "targets", rec, starts, 5),
                     "motion_sums": lambda: score.motion_sums(0, sets, "msg", starts, 5)}, args.repeats)
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
    for k in ("score_rows", "score_lags", "motion_sums"):
        p, n = [d[k] for d in res["parent"]], [d[k] for d in res["new"]]
        out[k] = {"parent_ms": p, "new_ms": n, "new_median_within_parent_range": bool(min(p) <= float(np.median(n)) <= max(p))}
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


def uniform_over_bins(rng, shape, edges):
    """values [..., W]: a bin drawn uniformly per value, then a point inside it"""
    W, B = edges.shape[0], edges.shape[1] - 1
    b = rng.integers(0, B, size=shape + (W,))
    lo, hi = edges[np.arange(W), b], edges[np.arange(W), b + 1]
    return lo + (hi - lo) * rng.uniform(0.25, 0.75, size=b.shape)


def torch_route(v, edges_dev, rec_of, R):
    """v [N, F, W] on the device -> counts [N, R, W, B + 3] by bucketize per column and one flat bincount (slot order: torch's own)"""
    import torch
    N, F, W = v.shape
    S = edges_dev.shape[1] + 2
    idx = torch.stack([torch.bucketize(v[:, :, w], edges_dev[w]) for w in range(W)], dim=2)       # [N, F, W] in 0 .. B + 1
    idx = idx + torch.isnan(v) * 1
    flat = ((torch.arange(N, device=v.device)[:, None, None] * R + rec_of[None, :, None]) * W + torch.arange(W, device=v.device)[None, None, :]) * S + idx
    return torch.bincount(flat.reshape(-1), minlength=N * R * W * S).reshape(N, R, W, S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-unchanged", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "score_hist.md"))
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
    starts = [r * F // RECORDINGS for r in range(RECORDINGS)]
    many = list(range(0, F, 5))
    rec_of = torch.from_numpy(np.searchsorted(np.asarray(starts), np.arange(F), side="right") - 1).cuda()
    result = {"frames": F, "recordings": RECORDINGS, "sets": SETS, "bins": BINS, "repeats": args.repeats, "hist": {}}

    # the planted replay: synthetic messages and spread records against synthetic targets, scored on the device
    rows, truth = synthetic(F, rng)
    msg, rec = rows[:, :-21], rows[:, -21:]
    real_score, _ = score.score_rows(0, msg, truth, "targets", rec, starts, 5)
    sets_msg = torch.from_numpy(rng.normal(size=(SETS, F, 25))).cuda()
    real_motion, _ = score.motion_sums(0, sets_msg, "msg", starts, 5, per_frame=True)
    e_score, e_motion = score.default_edges("score", BINS), score.default_edges("motion", BINS)
    inputs = {"score": {"edges": e_score, "real": real_score[None], "scorer": lambda: score.score_rows(0, msg, truth, "targets", rec, starts, 5, per_frame=False)},
              "motion": {"edges": e_motion, "real": real_motion, "scorer": lambda: score.motion_sums(0, sets_msg, "msg", starts, 5)}}
    legs = {}
    for name, d in inputs.items():
        N, W, e = int(d["real"].shape[0]), int(d["real"].shape[2]), d["edges"]
        d["uniform"] = torch.from_numpy(uniform_over_bins(rng, (N, F), e)).cuda()
        d["one_bin"] = torch.from_numpy(np.broadcast_to(0.5 * (e[:, BINS // 2] + e[:, BINS // 2 + 1]), (N, F, W)).copy()).cuda()
        d["edges_dev"] = torch.from_numpy(e).cuda()
        for kind in ("uniform", "one_bin", "real"):
            legs[f"{name}_hist_{kind}"] = lambda v=d[kind], e=e: score.hist_rows(v[:, :, None], e, starts, 5)
            legs[f"{name}_hist_{kind}_float32"] = lambda v=d[kind].float(), e=e: score.hist_rows(v[:, :, None], e, starts, 5)
        legs[f"{name}_torch_real"] = lambda v=d["real"], ed=d["edges_dev"]: torch_route(v, ed, rec_of, RECORDINGS)
        legs[f"{name}_scorer"] = d["scorer"]
    legs["score_hist_many"] = lambda v=inputs["score"]["real"], e=e_score: score.hist_rows(v[:, :, None], e, many)
    legs["score_hist_many_one_bin"] = lambda v=inputs["score"]["one_bin"], e=e_score: score.hist_rows(v[:, :, None], e, many)
    # the routes agree before anything is timed: the device's counts are the host statement's, and torch's hold the same totals
    for name, d in inputs.items():
        got = score.hist_rows(d["real"][:1, :, None], d["edges"], starts, 5)
        assert np.array_equal(got.cpu().numpy()[:, :, 0], score.hist_numpy(d["real"][:1].cpu().numpy()[:, :, None], d["edges"], starts, 5)[:, :, 0]), name
    times = alternate(legs, args.repeats)
    for name, d in inputs.items():
        N, W = int(d["real"].shape[0]), int(d["real"].shape[2])
        for key in [k for k in times if k.startswith(name + "_")]:
            ms, allv = times[key]
            entry_ = {"ms": round(ms, 4), "range": spread_of(allv)}
            if "_hist_" in key:
                size = 4 if key.endswith("float32") else 8
                moved = N * F * W * size + N * (len(many) if "many" in key else RECORDINGS) * W * (BINS + 3) * 8
                entry_.update(bytes_moved=moved, share_of_hbm_peak=round(moved / (ms * 1e-3) / HBM_PEAK, 4))
            result["hist"][key] = entry_

    # the route it replaces: the rows to the host, then the numpy statement
    result["host_route"] = {}
    for name, d in inputs.items():
        host = []
        for _ in range(args.host_repeats if name == "score" else 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = d["real"].cpu().numpy()
            t1 = time.perf_counter()
            score.hist_numpy(m[:, :, None], d["edges"], starts, 5)
            host.append((t1 - t0, time.perf_counter() - t1))
        result["host_route"][name] = {"copy_ms": round(1e3 * float(np.median([x[0] for x in host])), 3),
                                      "numpy_ms": round(1e3 * float(np.median([x[1] for x in host])), 1), "runs": len(host)}
    result["unchanged"] = leg_unchanged(args) if args.parent_tree else "not measured: no --parent-tree given"
    result["objects"] = object_hashes(args.parent_tree) if args.parent_tree else "not measured: no --parent-tree given"

    lines = [MARKER + f" (`python tools/score_hist_bench.py --frames {F} --repeats {args.repeats}`, one MI355X)", "",
             f"{F} frames in {RECORDINGS} recordings of equal length; score rows `[F, 7]` and motion rows `[{SETS}, F, 12]`, {BINS} bins per column "
             "(`default_edges`), skip 5.  Medians (and the smallest and largest of the repeats) of HIP events around the Python calls, the legs "
             "alternating within one session behind three warm-up rounds; the host route by the host clock.  Bytes: every value read once, the "
             "output zeroed once.  Nothing was fixed in advance.", "",
             "| input | leg | time | bytes moved | share of the 8 TB/s HBM peak |", "|---|---|---|---|---|"]
    for key, d in result["hist"].items():
        name, leg = key.split("_", 1)
        extra = f"{d['bytes_moved'] / 1e6:.1f} MB | {100 * d['share_of_hbm_peak']:.2f} %" if "bytes_moved" in d else "- | -"
        lines.append(f"| {name} | {leg} | {d['ms']:.3f} ms ({d['range'][0]:.3f} .. {d['range'][1]:.3f}) | {extra} |")
    lines.append("")
    for name, h in result["host_route"].items():
        lines.append(f"The route it replaces, {name} rows: D2H copy {h['copy_ms']:.2f} ms + `hist_numpy` {h['numpy_ms']:.0f} ms (median of {h['runs']}).")
    lines.append("")
    if isinstance(result["unchanged"], dict):
        lines += ["Untouched entries on this build beside a build of the parent commit (child processes alternating between the two trees, "
                  f"{RUNS} runs each, synthetic rows; medians in ms; `score_lags` over 17 lags, `motion_sums` of {SETS} sets):", "",
                  "| call | parent runs | this build's runs | this build's median within the parent's range |", "|---|---|---|---|"]
        for k, d in result["unchanged"].items():
            lines.append(f"| {k} | {d['parent_ms']} | {d['new_ms']} | {'yes' if d['new_median_within_parent_range'] else 'no'} |")
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
