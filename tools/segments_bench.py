"""Reaches and holds (score.segment_frames / segment_runs / segment_stats, Estimator.segment_recording): 100 000 frames in
64 recordings of equal length, a planted hand that holds for 40 - 120 frames and reaches for 8 - 20, with noise; the key is the hand-speed
column of the frames' motion rows, the values are four per-frame columns.  Legs, alternating within one session behind warmed shapes,
timed by HIP events, three runs each:

    segment_frames      one ape_segment_frames call, (lo, hi) = (0.004, 0.008), minimum lengths (4, 4); and with (1, 1), and (256, 256)
    segment_runs        one ape_segment_runs call with room for F segments (cap given: no wait)
    segment_stats       one ape_segment_stats call over the four columns
    segment_recording   WatchPhoneUarm.segment_recording end to end (motion rows, labels, table, records; it reads the table's size back)
    torch               the table and the records from the same labels by torch.unique_consecutive, index_add_ of [x, x^2, 1] and
                        index_reduce_ (amax): float atomics; the tool also reports whether two runs of it agree in bits

and by the host clock the route they replace: a copy of the speed and the columns to the host plus the numpy statements.  With
--parent-tree DIR (a checkout of the parent commit with its library built) select_rungs, motion_sums and score_rows are timed in child
processes that alternate between that tree and this one, three runs each: this build's median against the parent's own run-to-run range;
and the object hashes of the two builds (lib/build_info.json) are compared.  Writes profiles/segments.md's measured section and prints ONE
JSON line.

    python tools/segments_bench.py [--frames 100000] [--repeats 20] [--parent-tree DIR] [--out profiles/segments.md]"""
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

RECORDINGS, RUNS = 64, 3
RULE = ((0.004, 0.008), (4, 4))
MARKER, NOTES = "## Measured", "### Reading the figures"   # the section this tool writes; what follows it is written by hand and kept
UNCHANGED = ("select_rungs", "motion_sums", "score_rows")


def spread_of(v):
    return [round(min(v), 4), round(max(v), 4)]


def planted(F, rng):
    """message rows [F, 25] whose hand (columns 4:7) holds and reaches, everything else finite noise"""
    msg = rng.normal(size=(F, 25))
    pos, f, at = np.zeros((F, 3)), 0, rng.uniform(-0.4, 0.4, size=3)
    while f < F:
        n = int(rng.integers(40, 121))
        pos[f:f + n] = at
        f += n
        m, to = int(rng.integers(8, 21)), rng.uniform(-0.4, 0.4, size=3)
        t = (np.arange(1, m + 1) / (m + 1))[:F - f if f < F else 0]
        s = t * t * (3.0 - 2.0 * t)
        pos[f:f + len(s)] = (1.0 - s)[:, None] * at + s[:, None] * to
        f, at = f + m, to
    msg[:, 4:7] = pos + 0.0005 * rng.normal(size=(F, 3))
    return msg


def child_unchanged(args):
    """select_rungs, motion_sums and score_rows of whichever tree APE_BENCH_TREE names: medians in ms"""
    import torch
    from score_lags_bench import alternate, synthetic
    from wear_mocap_ape_amd import score
    torch.cuda.set_device(0)
    F = args.frames
    rows, truth = synthetic(F, np.random.default_rng(7))
    msg, rec, starts = rows[:, :-21], rows[:, -21:], [r * F // RECORDINGS for r in range(RECORDINGS)]
    motion = score.motion_sums(0, msg, "msg", starts, 0, None, None, True)[0]
    ladder, edges = score.ladder(samples=1), score.speed_edges()
    res = alternate({"select_rungs": lambda: score.select_rungs(motion[:, 0], edges, ladder, 2, starts=starts),
                     "motion_sums": lambda: score.motion_sums(0, msg, "msg", starts, 0, None, None, True),
                     "score_rows": lambda: score.score_rows(0, msg, truth, "targets", rec, starts, 5)}, args.repeats)
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
    for k in UNCHANGED:
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


def torch_route(labels, rec_of, values):
    """labels uint8 [F], rec_of int64 [F], values [F, V] on the device -> (table columns, sums [n, 3 V], maxima [n, V])"""
    import torch
    key = rec_of * 256 + labels.long()
    _, sof, counts = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
    n = int(counts.shape[0])                                # (a wait: the shapes below hang on it)
    first = torch.cumsum(counts, 0) - counts
    ok = ~torch.isnan(values)
    x = torch.where(ok, values, torch.zeros_like(values))
    sums = torch.zeros((n, 3 * values.shape[1]), dtype=torch.float64, device=values.device)
    sums.index_add_(0, sof, torch.cat([x, x * x, ok.double()], dim=1))
    maxima = torch.full((n, values.shape[1]), -float("inf"), dtype=torch.float64, device=values.device)
    maxima.index_reduce_(0, sof, torch.where(ok, values, torch.full_like(values, -float("inf"))), "amax", include_self=True)
    return (first, counts), sums, maxima


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-unchanged", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "segments.md"))
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
    from score_lags_bench import alternate
    from wear_mocap_ape_amd import score
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    torch.cuda.set_device(0)
    F = args.frames
    rng = np.random.default_rng(7)
    starts = [r * F // RECORDINGS for r in range(RECORDINGS)]
    msg = torch.from_numpy(planted(F, rng)).cuda()
    est = WatchPhoneUarm(smooth=5)
    motion = score.motion_sums(est._layout, msg, "msg", starts, 0, None, None, True)[0]
    speed = motion[:, 0]
    values = motion[:, [0, 1, 3, 6]].contiguous()
    labels = score.segment_frames(speed, *RULE, starts)
    sof, n, table = score.segment_runs(labels, starts, cap=F)
    rec_of = torch.from_numpy(np.searchsorted(np.asarray(starts), np.arange(F), side="right") - 1).cuda()
    n_segs = int(n)
    result = {"frames": F, "recordings": RECORDINGS, "repeats": args.repeats, "runs": RUNS, "segments": n_segs,
              "longest_segment": int(table[:n_segs, 2].max())}

    # the routes agree before anything is timed: labels and table are the statements', the records the statement's bit for bit
    sp, vh = speed.cpu().numpy(), values.cpu().numpy()
    lab_ref = score.segment_frames_numpy(sp, *RULE, starts)
    tab_ref = score.segment_runs_numpy(lab_ref, starts)[2]
    assert np.array_equal(labels.cpu().numpy(), lab_ref) and np.array_equal(table[:n_segs].cpu().numpy(), tab_ref)
    got, ref = score.segment_stats(values, sof, n, table)[:n_segs].cpu().numpy(), score.segment_stats_numpy(vh, tab_ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~np.isnan(got)].view(np.int64), ref[~np.isnan(ref)].view(np.int64))
    a, b = torch_route(labels, rec_of, values), torch_route(labels, rec_of, values)
    torch.cuda.synchronize()
    result["torch_two_runs_agree_in_bits"] = bool(torch.equal(a[1].view(torch.int64), b[1].view(torch.int64)))
    result["torch_segments"] = int(a[0][0].shape[0])

    legs = {"segment_frames": lambda: score.segment_frames(speed, *RULE, starts),
            "segment_frames_1_1": lambda: score.segment_frames(speed, RULE[0], (1, 1), starts),
            "segment_frames_256_256": lambda: score.segment_frames(speed, RULE[0], (256, 256), starts),
            "segment_runs": lambda: score.segment_runs(labels, starts, cap=F),
            "segment_stats": lambda: score.segment_stats(values, sof, n, table),
            "segment_recording": lambda: est.segment_recording(msg, starts=starts),
            "torch": lambda: torch_route(labels, rec_of, values)}
    runs = [alternate(legs, args.repeats) for _ in range(RUNS)]
    result["legs"] = {name: {"ms": [round(r[name][0], 4) for r in runs], "range": spread_of([x for r in runs for x in r[name][1]])} for name in legs}
    host = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sp, vh = speed.cpu().numpy(), values.cpu().numpy()
        t1 = time.perf_counter()
        lab = score.segment_frames_numpy(sp, *RULE, starts)
        tab = score.segment_runs_numpy(lab, starts)[2]
        score.segment_stats_numpy(vh, tab)
        host.append((t1 - t0, time.perf_counter() - t1))
    result["host_route"] = {"copy_ms": [round(1e3 * x[0], 3) for x in host], "numpy_ms": [round(1e3 * x[1], 1) for x in host]}
    result["unchanged"] = leg_unchanged(args) if args.parent_tree else "not measured: no --parent-tree given"
    result["objects"] = object_hashes(args.parent_tree) if args.parent_tree else "not measured: no --parent-tree given"

    cell = lambda e: f"{e['ms']} ms ({e['range'][0]:.3f} .. {e['range'][1]:.3f})"      # noqa: E731
    lines = [MARKER + f" (`python tools/segments_bench.py --frames {F} --repeats {args.repeats}`, one MI355X)", "",
             f"{F} frames in {RECORDINGS} recordings, a planted hand (holds of 40 - 120 frames, reaches of 8 - 20), float64; the key is the "
             f"hand speed of the motion rows, thresholds {RULE[0]}, minimum lengths {RULE[1]}: {n_segs} segments, the longest of "
             f"{result['longest_segment']} frames; four value columns.  Medians of {RUNS} runs of {args.repeats} repeats each (and the smallest and "
             "largest of all repeats) of HIP events around the Python calls, the legs alternating within one session behind three warm-up "
             "rounds; the host route by the host clock.  Nothing was fixed in advance.", "",
             "| leg | time |", "|---|---|"]
    names = {"segment_frames": "`segment_frames`, minimum lengths (4, 4)", "segment_frames_1_1": "`segment_frames`, (1, 1)",
             "segment_frames_256_256": "`segment_frames`, (256, 256)", "segment_runs": "`segment_runs`, `cap = F`",
             "segment_stats": "`segment_stats`, 4 columns", "segment_recording": "`WatchPhoneUarm.segment_recording`, end to end",
             "torch": "torch `unique_consecutive` + `index_add_` + `index_reduce_` (table and records from given labels)"}
    for k, d in result["legs"].items():
        lines.append(f"| {names[k]} | {cell(d)} |")
    h = result["host_route"]
    lines += [f"| host: D2H copy + the numpy statements | {h['copy_ms']} + {h['numpy_ms']} ms |", "",
              f"Two runs of the torch route agree in bits: {'yes' if result['torch_two_runs_agree_in_bits'] else 'no'} "
              f"(it finds {result['torch_segments']} segments).", ""]
    if isinstance(result["unchanged"], dict):
        lines += ["Untouched entries on this build beside a build of the parent commit (child processes alternating between the two trees, "
                  f"{RUNS} runs each, synthetic rows; medians in ms):", "",
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
