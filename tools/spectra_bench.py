"""Spectra of a replay (score.spectra / ape_spectra): 100 000 frames (rounded down to 64 x 1562) in 64 recordings of equal
length, `[25, F, 25]` message rows and `[F, 21]` est-row truth, N = 256, hop 128, Hann, the six position columns, float64.  Legs, alternating within one session behind
warmed shapes, timed by HIP events:

    spectra C            one ape_spectra call over C = 1 and 25 sets, without truth (W = 1) and with (W = 4)
    torch C              the same sums by torch.Tensor.unfold + torch.fft.rfft + sums on the device (one set per recording loop-free: the
                         recordings are of equal length here, which this route needs and ape_spectra does not)
    motion / score       ape_motion_sums and ape_score_rows on the first set: the yardsticks of a one-pass scoring kernel

with the float64 MFMA work of each spectra call (tiles x bin blocks x N / 4 steps x 2 or 4 instructions of 2048 flop, the idle rows of a
tile that is not full included) over its time; by the host clock the route it replaces, a copy of one set to the host plus score.spectra_numpy.  With
--parent-tree DIR (a checkout of the parent commit with its library built) ape_motion_sums and ape_score_rows are timed in child processes
that alternate between that tree and this one, three runs each, and the object hashes of both trees' build_info.json are compared.
With --ablate the 25-set legs are timed on the libraries of `make spectra_ablate`, each with one phase of the kernel taken out.
Writes profiles/spectra.md's measured section and prints ONE JSON line.

    python tools/spectra_bench.py [--frames 100000] [--repeats 20] [--host-repeats 3] [--parent-tree DIR] [--ablate] [--out profiles/spectra.md]

Rows are synthetic (a random walk plus noise): the times do not depend on the values."""
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

RECORDINGS, SETS, RUNS = 64, 25, 3
N, HOP = 256, 128
COLS, TCOLS = (4, 5, 6, 11, 12, 13), (0, 1, 2, 3, 4, 5)
MARKER, NOTES = "## Measured", "### Reading the figures"   # the section this tool writes; what follows it is written by hand and kept


def spread_of(v):
    return [round(min(v), 4), round(max(v), 4)]


def synthetic(F, sets, rng):
    import torch
    msg = np.cumsum(rng.normal(size=(sets, F, 25)) * 0.01, axis=1) + rng.normal(size=(sets, F, 25)) * 0.02
    msg[:, :, 7:11] = msg[:, :, 14:18] = msg[:, :, 21:25] = [1.0, 0.0, 0.0, 0.0]
    est = np.cumsum(rng.normal(size=(F, 21)) * 0.01, axis=0)
    est[:, 9:13] = est[:, 13:17] = est[:, 17:21] = [1.0, 0.0, 0.0, 0.0]
    return torch.from_numpy(msg).cuda(), torch.from_numpy(est).cuda()


def child_unchanged(args):
    """motion_sums and score_rows of whichever tree APE_BENCH_TREE names: medians in ms"""
    import torch
    from score_lags_bench import alternate
    from wear_mocap_ape_amd import score
    torch.cuda.set_device(0)
    msg, est = synthetic(args.frames, 1, np.random.default_rng(7))
    starts = [r * args.frames // RECORDINGS for r in range(RECORDINGS)]
    res = alternate({"motion_sums": lambda: score.motion_sums(0, msg[0], "msg", starts, 5),
                     "score_rows": lambda: score.score_rows(0, msg[0], est, "est", None, starts, 5, per_frame=False)}, args.repeats)
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
    for k in ("motion_sums", "score_rows"):
        p, n = [d[k] for d in res["parent"]], [d[k] for d in res["new"]]
        out[k] = {"parent_ms": p, "new_ms": n, "new_median_within_parent_range": bool(min(p) <= float(np.median(n)) <= max(p))}
    return out


ABLATIONS = (("product", None), ("no step loop (no operand reads, no MFMA)", 1), ("no gather (span filled with ones)", 2),
             ("no pass over means, finiteness and bin N/2", 4))


def child_spectra(args):
    """the 25-set spectra legs on whichever library APE_HIP_LIB names: medians in ms"""
    import torch
    from score_lags_bench import alternate
    from wear_mocap_ape_amd import score
    torch.cuda.set_device(0)
    F = args.frames // RECORDINGS * RECORDINGS
    msg, est = synthetic(F, SETS, np.random.default_rng(7))
    starts = [r * F // RECORDINGS for r in range(RECORDINGS)]
    res = alternate({"plain": lambda: score.spectra(msg, None, COLS, None, N, HOP, "hann", True, starts, 0),
                     "truth": lambda: score.spectra(msg, est, COLS, TCOLS, N, HOP, "hann", True, starts, 0)}, args.repeats)
    print(json.dumps({k: round(v[0], 4) for k, v in res.items()}))


def leg_ablate(args):
    """the 25-set legs on the product library and on `make spectra_ablate`'s three, a child process each: what each phase's absence saves"""
    diag = ROOT / "arm-pose-estimation_amd" / "lib" / "diag"
    out = {}
    for name, k in ABLATIONS:
        env = dict(os.environ)
        env.pop("APE_BENCH_TREE", None)
        env.pop("APE_HIP_LIB", None)
        if k is not None:
            lib = diag / f"libape_hip_spectra_ablate{k}.so"
            if not lib.exists():
                return f"not measured: {lib.name} is not built (make -C arm-pose-estimation_amd/csrc spectra_ablate)"
            env["APE_HIP_LIB"] = str(lib)
        r = subprocess.run([sys.executable, __file__, "--child-spectra", "--frames", str(args.frames), "--repeats", str(args.repeats)],
                           env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    return out


def object_hashes(args):
    """the objects of the parent's build_info.json beside this tree's: names whose hashes differ, names only here"""
    def objects(tree):
        info = json.loads((Path(tree) / "arm-pose-estimation_amd" / "lib" / "build_info.json").read_text())
        found = {}

        def walk(d):
            for k, v in d.items():
                if isinstance(v, dict):
                    walk(v)
                elif isinstance(v, str) and k.endswith(".o"):
                    found[k] = v
        walk(info)
        return found
    try:
        old, new = objects(args.parent_tree), objects(ROOT)
    except (OSError, ValueError) as e:
        return f"not measured: {e}"
    if not old or not new:
        return "not measured: build_info.json lists no object hashes"
    return {"compared": len(old), "differ": sorted(k for k in old if new.get(k) != old[k]), "only_here": sorted(k for k in new if k not in old)}


def torch_route(rows, truth, starts, F, w):
    """the sums of ape_spectra by unfold + rfft: rows [C, F, 6] (a strided view), truth [F, 6] or None; recordings of equal length"""
    import torch
    L = F // RECORDINGS
    x = rows[:, :RECORDINGS * L].reshape(rows.shape[0], RECORDINGS, L, 6).unfold(2, N, HOP)          # [C, R, J, 6, N]
    x = torch.fft.rfft((x - x.mean(dim=-1, keepdim=True)) * w, dim=-1)
    if truth is None:
        return (x.real * x.real + x.imag * x.imag).sum(dim=2)
    y = truth[:RECORDINGS * L].reshape(1, RECORDINGS, L, 6).unfold(2, N, HOP)
    y = torch.fft.rfft((y - y.mean(dim=-1, keepdim=True)) * w, dim=-1)
    c = torch.conj(y) * x
    return torch.stack([(x.real * x.real + x.imag * x.imag).sum(dim=2), (y.real * y.real + y.imag * y.imag).sum(dim=2).expand(x.shape[0], -1, -1, -1),
                        c.real.sum(dim=2), c.imag.sum(dim=2)], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-unchanged", action="store_true")
    ap.add_argument("--child-spectra", action="store_true")
    ap.add_argument("--ablate", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spectra.md"))
    args = ap.parse_args()
    if args.child_unchanged:         # (the tree's library as it stands: nothing is built on the way)
        child_unchanged(args)
        return
    if args.child_spectra:
        child_spectra(args)
        return
    import __graft_entry__ as entry
    entry.build()
    import torch
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return
    from score_lags_bench import alternate
    from wear_mocap_ape_amd import score
    torch.cuda.set_device(0)
    F, skip = args.frames // RECORDINGS * RECORDINGS, 0        # (recordings of equal length: the torch route needs them)
    msg, est = synthetic(F, SETS, np.random.default_rng(7))
    starts = [r * F // RECORDINGS for r in range(RECORDINGS)]
    w = torch.from_numpy(score.spectra_taper("hann", N)).cuda()
    pos, tpos = msg[:, :, list(COLS)], est[:, list(TCOLS)]                               # (the torch route's own gathered copies, made once, not timed)
    legs = {}
    for C_ in (1, SETS):
        rows, view = (msg[0] if C_ == 1 else msg), pos[:C_]
        legs[f"spectra_{C_}_plain"] = lambda r=rows: score.spectra(r, None, COLS, None, N, HOP, "hann", True, starts, skip)
        legs[f"spectra_{C_}_truth"] = lambda r=rows: score.spectra(r, est, COLS, TCOLS, N, HOP, "hann", True, starts, skip)
        legs[f"torch_{C_}_plain"] = lambda v=view: torch_route(v, None, starts, F, w)
        legs[f"torch_{C_}_truth"] = lambda v=view: torch_route(v, tpos, starts, F, w)
    legs["motion_sums"] = lambda: score.motion_sums(0, msg[0], "msg", starts, skip)
    legs["score_rows"] = lambda: score.score_rows(0, msg[0], est, "est", None, starts, skip, per_frame=False)
    times = alternate(legs, args.repeats)

    # agreement of the two device routes, so that the comparison is of the same sums
    a = score.spectra(msg[0], est, COLS, TCOLS, N, HOP, "hann", True, starts, skip)[0]
    b = torch_route(pos[:1], tpos, starts, F, w)[0]
    agree = float(((a - b).abs().amax() / a.abs().amax()).item())

    L = F // RECORDINGS
    J = (L - skip - N) // HOP + 1
    tiles, blocks = (J + 15) // 16, N // 32 + (1 if N % 32 else 0)         # (bin N/2 of a multiple of 32 is not MFMA work)
    result = {"frames": F, "recordings": RECORDINGS, "n": N, "hop": HOP, "segments_per_recording": J, "repeats": args.repeats,
              "torch_route_relative_difference": agree, "legs": {}}
    for C_ in (1, SETS):
        for what, per_step in (("plain", 2), ("truth", 4)):
            ms, allv = times[f"spectra_{C_}_{what}"]
            flop = C_ * RECORDINGS * 6 * tiles * blocks * (N // 4) * per_step * 2048.0
            tms, tall = times[f"torch_{C_}_{what}"]
            result["legs"][f"{C_}_{what}"] = {"ms": round(ms, 4), "range": spread_of(allv), "mfma_flop": flop,
                                              "mfma_tflops": round(flop / (ms * 1e-3) / 1e12, 3), "torch_ms": round(tms, 4), "torch_range": spread_of(tall)}
    for k in ("motion_sums", "score_rows"):
        result["legs"][k] = {"ms": round(times[k][0], 4), "range": spread_of(times[k][1])}

    host = []
    for _ in range(args.host_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m, t = msg[0].cpu().numpy(), est.cpu().numpy()
        t1 = time.perf_counter()
        score.spectra_numpy(m, t, COLS, TCOLS, N, HOP, "hann", True, starts, skip)
        host.append((t1 - t0, time.perf_counter() - t1))
    result["host_route_one_set"] = {"copy_ms": round(1e3 * float(np.median([x[0] for x in host])), 3),
                                    "numpy_ms": round(1e3 * float(np.median([x[1] for x in host])), 1)}
    result["unchanged"] = leg_unchanged(args) if args.parent_tree else "not measured: no --parent-tree given"
    result["object_hashes"] = object_hashes(args) if args.parent_tree else "not measured: no --parent-tree given"
    result["ablations"] = leg_ablate(args) if args.ablate else "not measured: no --ablate given"

    lines = [MARKER + f" (`python tools/spectra_bench.py --frames {F} --repeats {args.repeats}`, one MI355X)", "",
             f"{F} frames in {RECORDINGS} recordings of equal length ({J} segments each, {tiles} tiles), N = {N}, hop {HOP}, Hann, detrend, six position "
             f"columns of `[C, F, 25]` float64 message rows, truth `[F, 21]` shared by the sets.  Medians (and the smallest and largest of the repeats) of "
             "HIP events around the Python calls, the legs alternating within one session behind three warm-up rounds; the host route by the host "
             f"clock.  MFMA work: tiles x {blocks} bin blocks x {N // 4} steps x 2 (4 with truth) `v_mfma_f64_16x16x4_f64` of 2048 flop, "
             "the idle rows of a tile that is not full counted as work.", "",
             "| sets | truth | `spectra` | f64 MFMA work | rate | `unfold` + `rfft` + sums on the device |", "|---|---|---|---|---|---|"]
    for C_ in (1, SETS):
        for what in ("plain", "truth"):
            d = result["legs"][f"{C_}_{what}"]
            lines.append(f"| {C_} | {'yes' if what == 'truth' else 'no'} | {d['ms']:.3f} ms ({d['range'][0]:.3f} .. {d['range'][1]:.3f}) | "
                         f"{d['mfma_flop'] / 1e9:.2f} GFLOP | {d['mfma_tflops']:.2f} TFLOP/s | {d['torch_ms']:.3f} ms ({d['torch_range'][0]:.3f} .. "
                         f"{d['torch_range'][1]:.3f}) |")
    m, s, h = result["legs"]["motion_sums"], result["legs"]["score_rows"], result["host_route_one_set"]
    lines += ["", f"In the same session, on the first set: `motion_sums` {m['ms']:.3f} ms, `score_rows` {s['ms']:.3f} ms.  The two device routes agree to "
              f"{agree:.1e} of the largest sum.", "",
              f"The route it replaces, one set with truth: D2H copy {h['copy_ms']:.2f} ms + `spectra_numpy` {h['numpy_ms']:.0f} ms; {SETS} sets are {SETS} of them.", ""]
    if isinstance(result["unchanged"], dict):
        lines += ["Untouched entries on this build beside a build of the parent commit (child processes alternating between the two trees, "
                  f"{RUNS} runs each; medians in ms):", "",
                  "| call | parent runs | this build's runs | this build's median within the parent's range |", "|---|---|---|---|"]
        for k, d in result["unchanged"].items():
            lines.append(f"| {k} | {d['parent_ms']} | {d['new_ms']} | {'yes' if d['new_median_within_parent_range'] else 'no'} |")
        oh = result["object_hashes"]
        lines += ["", f"Object hashes (`build_info.json` of both trees): {oh['compared']} objects compared, differing: {oh['differ'] or 'none'}; only in this "
                  f"build: {oh['only_here']}." if isinstance(oh, dict) else f"Object hashes: {oh}.", ""]
    else:
        lines += ["Untouched entries against a build of the parent commit, and the object hashes: not measured in this run (`--parent-tree`).", ""]
    if isinstance(result["ablations"], dict):
        base = result["ablations"]["product"]
        lines += [f"The {SETS}-set legs with one phase of the kernel taken out (`make spectra_ablate`: timing-only libraries, a child process each; "
                  "medians in ms; the results of these libraries mean nothing):", "",
                  "| library | without truth | saved | with truth | saved |", "|---|---|---|---|---|"]
        for name, d in result["ablations"].items():
            lines.append(f"| {name} | {d['plain']:.3f} | {base['plain'] - d['plain']:.3f} | {d['truth']:.3f} | {base['truth'] - d['truth']:.3f} |")
        lines.append("")
    else:
        lines += [f"The kernel with one phase taken out: {result['ablations']}.", ""]
    old = Path(args.out).read_text() if Path(args.out).exists() else ""
    notes = "\n" + old[old.index(NOTES):] if NOTES in old else ""
    Path(args.out).write_text((old[:old.index(MARKER)] if MARKER in old else old.rstrip() + "\n\n") + "\n".join(lines) + notes)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
