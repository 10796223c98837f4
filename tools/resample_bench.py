"""Mocap truth on each frame's clock (score.frame_times / resample_truth / align(refine=True)): 100 000 frames in 64
recordings of equal length against 240 000 truth rows on a clock of their own.  Legs, alternating within one session behind warmed
shapes, timed by HIP events:

    times          ape_frame_times of column 0 of raw [F, 55] float32 rows (a strided view), and of the same values contiguous
    resample       ape_resample_truth at a shift per recording, float64 in and out: est-kind truth [Ft, 21], NN targets [Ft, 14]
    align          score.align(refine=True) end to end over lags -8 .. 8 on F truth rows (the sweep, best_lag on the host behind a wait,
                   resample_truth on the index clock, score_rows), and score.align as it was next to it

and, by the host clock, the route the feature replaces: truth, stamps and frame times copied to the host, score.resample_truth_numpy,
the result copied back.  With --parent-tree DIR (a checkout of the parent commit with its library built) ape_score_rows and
ape_score_lags are timed in fresh child processes on that tree and on this one in turn, to show that they did not move.  The bytes every
kernel must move are computed from the shapes, the cycles its vector instructions occupy from a count in its ISA; the larger bound binds.  Writes profiles/resample.md's measured section and prints ONE JSON line.

    python tools/resample_bench.py [--frames 100000] [--truth-rows 240000] [--repeats 20] [--parent-tree DIR] [--out profiles/resample.md]

Rows, truth and clocks are synthetic (times do not depend on the values)."""
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

RECORDINGS, LAGS, RUNS = 64, (-8, 8), 3
HBM_PEAK = 8.0e12                                           # bytes / s
# vector instructions a lane of ape_resample_kernel<double, kind> executes for layout 0, counted in the gfx950 ISA of the kernel compiled
# with the layout fixed (both sides of the chord / arc choice; the binary searches add a compare per step): (float64, others).  A wave's
# float64 instruction occupies its SIMD for 4 cycles (16 lanes a cycle), any other vector instruction for 2
VALU = {"resample_est": (2193, 1449), "resample_targets": (5261, 1879)}
SIMDS, CLOCK = 256 * 4, 2.4e9
MARKER, NOTES = "## Measured", "### Reading the figures"   # the section this tool writes; what follows it is written by hand and kept


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


def session(F, Ft, rng):
    """host arrays of the workload: raw rows [F, 55] float32 whose column 0 is a jittered sw_dt, the recordings' starts on both sides,
    truth stamps covering every recording's frames, est rows and NN targets, a shift per recording"""
    rows = rng.normal(size=(F, 55)).astype(np.float32)
    rows[:, 0] = rng.uniform(0.012, 0.03, size=F).astype(np.float32)
    starts = [r * F // RECORDINGS for r in range(RECORDINGS)]
    tstarts = [r * Ft // RECORDINGS for r in range(RECORDINGS)]
    tt = np.empty(Ft)
    for r in range(RECORDINGS):
        a, b = starts[r], starts[r + 1] if r + 1 < RECORDINGS else F
        ta, tb = tstarts[r], tstarts[r + 1] if r + 1 < RECORDINGS else Ft
        tt[ta:tb] = np.linspace(0.0, 1.001 * float(rows[a + 1:b, 0].astype(np.float64).sum()), tb - ta)
    return {"rows": rows, "starts": starts, "tstarts": tstarts, "tt": tt, "est": rng.normal(size=(Ft, 21)), "targets": rng.normal(size=(Ft, 14)),
            "shifts": rng.uniform(-0.1, 0.1, size=RECORDINGS)}


def bytes_moved(F, Ft):
    """what each kernel must move, from the shapes: every value it needs read once, every result written once"""
    rows = min(Ft, 2 * F)                                   # a frame needs two neighbouring truth rows; neighbouring frames share them
    return {"times": F * 4 + F * 8,
            "resample_est": rows * 21 * 8 + rows * 8 + F * 8 + F * 21 * 8,
            "resample_targets": rows * 14 * 8 + rows * 8 + F * 8 + F * 21 * 8}


def compute_seconds(leg, F):
    """the least time the vector units need for the leg's kernel: its waves' instruction cycles spread over every SIMD of the chip"""
    f64, other = VALU[leg]
    return -(-F // 64) * (4 * f64 + 2 * other) / (SIMDS * CLOCK)


def child_unchanged(args):
    """ape_score_rows and ape_score_lags of whichever tree APE_BENCH_TREE names (accumulators only): medians in ms"""
    import torch
    from wear_mocap_ape_amd import score
    torch.cuda.set_device(0)
    rng = np.random.default_rng(7)
    F = args.frames
    rows = rng.normal(size=(F, 196))
    rows[:, 175 + 3:175 + 9] = rows[:, 175 + 12:175 + 18] = [0.01, 0.0, 0.0, 0.01, 0.0, 0.01]
    rows, truth = torch.from_numpy(rows).cuda(), torch.from_numpy(rng.normal(size=(F, 14))).cuda()
    msg, rec, starts = rows[:, :-21], rows[:, -21:], [r * F // RECORDINGS for r in range(RECORDINGS)]
    res = alternate({"score_rows": lambda: score.score_rows(0, msg, truth, "targets", rec, starts, 5, per_frame=False),
                     "score_lags": lambda: score.score_lags(0, msg, truth, LAGS, "targets", rec, starts, 5)}, args.repeats)
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
    for k in ("score_rows", "score_lags"):
        p, n = [d[k] for d in res["parent"]], [d[k] for d in res["new"]]
        out[k] = {"parent_ms": p, "new_ms": n, "new_median_within_parent_range": bool(min(p) <= float(np.median(n)) <= max(p))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--truth-rows", type=int, default=240_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-unchanged", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resample.md"))
    args = ap.parse_args()
    if args.child_unchanged:         # (the tree's library as it stands: nothing is built on the way)
        child_unchanged(args)
        return
    import __graft_entry__ as entry
    entry.build()
    import torch
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU", "bytes": bytes_moved(args.frames, args.truth_rows)}))
        return
    from wear_mocap_ape_amd import score
    torch.cuda.set_device(0)
    F, Ft = args.frames, args.truth_rows
    s = session(F, Ft, np.random.default_rng(7))
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    rows, dt, tt, est, targets = cuda(s["rows"]), cuda(s["rows"][:, 0]), cuda(s["tt"]), cuda(s["est"]), cuda(s["targets"])
    starts, tstarts, shifts = s["starts"], s["tstarts"], s["shifts"]
    tq = score.frame_times(rows[:, 0], starts)
    msg, truth_f = cuda(np.random.default_rng(8).normal(size=(F, 25))), est[:F].contiguous()
    score.resample_truth(0, est, "est", tstarts, tt, tq, None, starts, shifts)           # (checks the stamps once: they are in order)
    torch.cuda.synchronize()

    legs = {"times_view": lambda: score.frame_times(rows[:, 0], starts),
            "times_contiguous": lambda: score.frame_times(dt, starts),
            "resample_est": lambda: score.resample_truth(0, est, "est", tstarts, tt, tq, None, starts, shifts, check_times=False),
            "resample_targets": lambda: score.resample_truth(0, targets, "targets", tstarts, tt, tq, None, starts, shifts, check_times=False),
            "align_refine": lambda: score.align(0, msg, truth_f, LAGS, truth_kind="est", starts=starts, skip=5, refine=True)[1:],
            "align": lambda: score.align(0, msg, truth_f, LAGS, truth_kind="est", starts=starts, skip=5)[1:]}
    times = alternate(legs, args.repeats)
    moved = bytes_moved(F, Ft)
    result = {"frames": F, "truth_rows": Ft, "recordings": RECORDINGS, "repeats": args.repeats, "legs": {}}
    for k, (med, every) in times.items():
        d = {"ms": round(med, 4), "range": [round(min(every), 4), round(max(every), 4)]}
        b = moved.get("times" if k.startswith("times") else k)
        if b:
            mem, cmp_ = b / HBM_PEAK, compute_seconds(k, F) if k in VALU else 0.0
            d["bytes_moved"] = b
            d["memory_bound_us"], d["compute_bound_us"] = round(1e6 * mem, 2), round(1e6 * cmp_, 2)
            d["bound"] = "compute" if cmp_ > mem else "memory"
            d["share_of_bound"] = round(max(mem, cmp_) / (med * 1e-3), 4)
        result["legs"][k] = d

    host = []
    for _ in range(args.host_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_est, h_tt, h_tq = est.cpu().numpy(), tt.cpu().numpy(), tq.cpu().numpy()
        t1 = time.perf_counter()
        out = score.resample_truth_numpy(0, h_est, tstarts, h_tt, h_tq, None, starts, shifts)
        t2 = time.perf_counter()
        back = torch.from_numpy(out).cuda()
        torch.cuda.synchronize()
        host.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
        del back
    result["host_route"] = {k: round(1e3 * float(np.median([x[i] for x in host])), 3) for i, k in enumerate(("d2h_ms", "numpy_ms", "h2d_ms"))}
    result["unchanged"] = leg_unchanged(args) if args.parent_tree else "unmeasured: no --parent-tree given"

    L = result["legs"]
    cell = lambda k: f"{L[k]['ms']:.3f} ms ({L[k]['range'][0]:.3f} .. {L[k]['range'][1]:.3f})"       # noqa: E731
    share = lambda k: (f"{L[k]['bytes_moved'] / 1e6:.1f} MB = {L[k]['memory_bound_us']:.2f} us, "                                          # noqa: E731
                       + (f"{L[k]['compute_bound_us']:.2f} us" if k in VALU else "far below it (a few dozen instructions a frame)")
                       + f": {L[k]['bound']}, {100 * L[k]['share_of_bound']:.1f} %")
    h = result["host_route"]
    lines = [MARKER + f" (`python tools/resample_bench.py --frames {F} --truth-rows {Ft} --repeats {args.repeats}`, one MI355X)", "",
             f"{F} frames in {RECORDINGS} recordings of equal length against {Ft} truth rows, float64 truth and output, a shift per recording.  "
             "Medians (and the smallest and largest of the repeats) of HIP events around the Python calls, the legs alternating within one "
             "session behind three warm-up rounds; the host route by the host clock.  Bounds: the bytes the kernel must move (from the shapes) "
             "at the 8 TB/s HBM peak, and the cycles its vector instructions occupy (counted in the ISA; float64 at 16 lanes a cycle and SIMD, "
             "1024 SIMDs at 2.4 GHz); the larger of the two is the bound, and the share is that bound over the measured time of the whole call.", "",
             "| leg | time | memory bound, compute bound: which binds, share of it |", "|---|---|---|",
             f"| `frame_times`, column 0 of `[F, 55]` float32 rows | {cell('times_view')} | {share('times_view')} |",
             f"| `frame_times`, the same values contiguous | {cell('times_contiguous')} | {share('times_contiguous')} |",
             f"| `resample_truth`, est-kind truth | {cell('resample_est')} | {share('resample_est')} |",
             f"| `resample_truth`, NN targets | {cell('resample_targets')} | {share('resample_targets')} |",
             f"| `align(refine=True)`, lags {LAGS[0]} .. {LAGS[1]}, with the wait for `best_lag` | {cell('align_refine')} | |",
             f"| `align` as it was | {cell('align')} | |", "",
             f"The host route the feature replaces (est-kind truth): {h['d2h_ms']:.2f} ms to the host, {h['numpy_ms']:.1f} ms in "
             f"`resample_truth_numpy`, {h['h2d_ms']:.2f} ms back: {(h['d2h_ms'] + h['numpy_ms'] + h['h2d_ms']) / L['resample_est']['ms']:.0f} x "
             "the device call.", ""]
    if isinstance(result["unchanged"], dict):
        lines += [f"Unchanged paths, parent commit and this tree in fresh processes in turn ({RUNS} runs each, medians of {args.repeats} in ms):", "",
                  "| call | parent | this tree |", "|---|---|---|"]
        for k, d in result["unchanged"].items():
            lines.append(f"| `{k}` (accumulators only) | {', '.join(f'{v:.3f}' for v in d['parent_ms'])} | {', '.join(f'{v:.3f}' for v in d['new_ms'])} |")
        lines.append("")
    else:
        lines += ["Unchanged paths against the parent commit: not measured (no `--parent-tree`).", ""]
    old = Path(args.out).read_text() if Path(args.out).exists() else ""
    notes = "\n" + old[old.index(NOTES):] if NOTES in old else ""
    Path(args.out).write_text((old[:old.index(MARKER)] if MARKER in old else old.rstrip() + "\n\n") + "\n".join(lines) + notes)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
