"""Arm lengths and shoulder origin against the truth (score.body_sums / rebody_rows / align_body) on the workload of
profiles/frame_fit.md: 100 000 pocket frames, `[F, 196]` float64 rows from process_recording(spread=True) at 25 Monte-Carlo samples,
in 64 recordings of equal length; truth as est rows (the body-made layouts take no target truth).  Legs, alternating within one
session behind warmed shapes, timed by HIP events:

    body L     one ape_body_sums call over L = 1, 17 and 65 lags (the message's rotations)
    frame L    ape_frame_sums at the same F, L and truth: the yardstick -- the same structure, 51 columns against 46
    truth      ape_body_sums with the truth's rotations (the single lag 0, no message)
    rebody     ape_rebody_rows of the rows, and the bytes it moves over the time against the HBM peak
    align      score.align_body end to end over 17 lags (body_sums, best_body on the host behind a wait, rebody_rows, score_lags)

by the host clock the route a user has without the device entry: a copy of the message columns to the host plus score.body_sums_numpy;
and, with --parent-lib, ape_score_rows and ape_frame_sums of a build of the parent commit beside this build's on the same buffers, the
two libraries alternating: the paths this change does not touch.  Writes profiles/body_fit.md's measured section and prints ONE JSON line.

    python tools/body_fit_bench.py [--frames 100000] [--repeats 20] [--host-repeats 3] [--parent-lib PATH/libape_hip.so] [--out profiles/body_fit.md]

Models carry seeded synthetic weights, rows and truth are synthetic."""
import argparse
import ctypes as C
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

SWEEPS = ((0, 0), (-8, 8), (-32, 32))
RECORDINGS = 64
HBM_PEAK = 8.0e12                                           # bytes / s
MARKER, NOTES = "## Measured", "### Reading the figures"   # the section this tool writes; what follows it is written by hand and kept


def spread_of(v):
    return [round(min(v), 4), round(max(v), 4)]


def raw_calls(lib, layout, out, truth, rec, starts, skip, body, sweep):
    """(score_rows, frame_sums) as closures on `lib`'s C entries with this session's buffers (est-kind truth)"""
    import torch
    from wear_mocap_ape_amd import _hip
    F, R = int(out.shape[0]), len(starts)
    st = np.ascontiguousarray(starts, dtype=np.int32)
    bd = np.ascontiguousarray(np.asarray(body, dtype=np.float64).reshape(1, 9))
    lo, hi = sweep
    score = torch.empty((F, 7), dtype=torch.float64, device=out.device)
    acc = torch.empty((R, 25), dtype=torch.float64, device=out.device)
    sums = torch.empty((R, hi - lo + 1, 51), dtype=torch.float64, device=out.device)
    p = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
    for name in ("ape_score_rows", "ape_frame_sums", "ape_last_error"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _hip.SIGNATURES[name]

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {lib.ape_last_error().decode()}")
        return sums

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    return (lambda: check(lib.ape_score_rows(layout, p(out), int(out.stride(0)), p(rec), int(rec.stride(0)), _hip.F64, p(truth), _hip.TRUTH_EST,
                                             _hip.F64, F, C.c_void_p(st.ctypes.data), R, skip, C.c_void_p(bd.ctypes.data), 1, p(score), _hip.F64,
                                             p(acc), stream()), "ape_score_rows"),
            lambda: check(lib.ape_frame_sums(layout, p(out), int(out.stride(0)), _hip.F64, p(truth), _hip.TRUTH_EST, _hip.F64, F,
                                             C.c_void_p(st.ctypes.data), R, skip, C.c_void_p(bd.ctypes.data), 1, lo, hi, None, p(sums), stream()),
                          "ape_frame_sums"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libape_hip.so built from the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "body_fit.md"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU"}))
        return
    from replay_bench import deploy_tree, rows_for
    from score_lags_bench import alternate
    from wear_mocap_ape_amd import _hip, config, score
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
        layout, skip, body = est._layout, est.sequence_len - 1, est.body_measurements
        truth = torch.from_numpy(rng.normal(size=(F, _hip.EST_WIDTH[layout]))).cuda()
        bodies = np.asarray(body, dtype=np.float64).reshape(1, 9) * rng.uniform(0.8, 1.2, size=(RECORDINGS, 9))
        torch.cuda.synchronize()

        legs = {}
        for lo, hi in SWEEPS:
            L = hi - lo + 1
            legs[f"body_{L}"] = lambda lo=lo, hi=hi: score.body_sums(layout, out, truth, (lo, hi), "est", starts, skip)
            legs[f"frame_{L}"] = lambda lo=lo, hi=hi: score.frame_sums(layout, out, truth, (lo, hi), "est", starts, skip, body)
        legs["truth"] = lambda: score.body_sums(layout, None, truth, (0, 0), "est", starts, skip, rotations="truth")
        legs["rebody"] = lambda: score.rebody_rows(layout, out, bodies, starts)
        legs["align"] = lambda: score.align_body(layout, out, truth, SWEEPS[1], "vectors", (1, 1), "est", rec, starts, skip)[:2]
        times = alternate(legs, args.repeats)
        blocks = (F + 255) // 256
        for lo, hi in SWEEPS:
            L = hi - lo + 1
            a, b = times[f"body_{L}"], times[f"frame_{L}"]
            result["sweeps"][str(L)] = {"lags": [lo, hi], "body_sums_ms": round(a[0], 4), "body_sums_range": spread_of(a[1]),
                                        "frame_sums_ms": round(b[0], 4), "frame_sums_range": spread_of(b[1]),
                                        "ratio_body_over_frame": round(a[0] / b[0], 2),
                                        "partial_records_bytes": (blocks + RECORDINGS) * L * _hip.BODY_ACC_WIDTH * 8}
        result["body_sums_truth_rotations_ms"] = round(times["truth"][0], 4)
        result["body_sums_truth_rotations_range"] = spread_of(times["truth"][1])
        moved = 2 * F * 25 * 8                              # every message value read once and written once
        reb = times["rebody"]
        result["rebody_rows"] = {"ms": round(reb[0], 4), "range": spread_of(reb[1]), "bytes_moved": moved,
                                 "share_of_hbm_peak": round(moved / (reb[0] * 1e-3) / HBM_PEAK, 4)}
        result["align_body_ms"] = round(times["align"][0], 4)
        result["align_body_range"] = spread_of(times["align"][1])

        # the host route: the message columns to the host, then the numpy statement
        est_truth = truth.cpu().numpy()
        host = {}
        for lo, hi in SWEEPS:
            t = []
            for _ in range(args.host_repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = out[:, :25].contiguous().cpu().numpy()
                t1 = time.perf_counter()
                score.body_sums_numpy(m, est_truth, layout, (lo, hi), starts, skip)
                t.append((t1 - t0, time.perf_counter() - t1))
            host[str(hi - lo + 1)] = {"copy_ms": round(1e3 * float(np.median([x[0] for x in t])), 3),
                                      "numpy_ms": round(1e3 * float(np.median([x[1] for x in t])), 1),
                                      "numpy_range_ms": [round(1e3 * min(x[1] for x in t), 1), round(1e3 * max(x[1] for x in t), 1)]}
        result["host_route"] = host

        # the untouched paths: the parent's library beside this one on the same buffers
        if args.parent_lib:
            mine, parent = _hip.lib(), C.CDLL(str(Path(args.parent_lib).resolve()))
            ab = {}
            for tag, lib in (("this", mine), ("parent", parent)):
                ab[f"score_rows_{tag}"], ab[f"frame_sums_{tag}"] = raw_calls(lib, layout, out, truth, rec, starts, skip, body, SWEEPS[1])
            t = alternate(ab, args.repeats)
            result["unchanged"] = {k: {"ms": round(v[0], 4), "range": spread_of(v[1])} for k, v in t.items()}
        del est
    lines = [MARKER + f" (`python tools/body_fit_bench.py --frames {F} --repeats {args.repeats}`, one MI355X)", "",
             f"{F} pocket frames in {RECORDINGS} recordings of equal length, `[F, 196]` float64 rows from `process_recording(spread=True)` at {n_mc} "
             "samples, truth as est rows.  Medians (and the smallest and largest of the repeats) of HIP events around the Python calls, the "
             "legs alternating within one session behind three warm-up rounds; the host route by the host clock.  Nothing was fixed in advance.", "",
             "| L | lags | `body_sums` | `frame_sums` (same session) | ratio | host: copy + `body_sums_numpy` |", "|---|---|---|---|---|---|"]
    for L, d in result["sweeps"].items():
        h = result["host_route"][L]
        lines.append(f"| {L} | {d['lags'][0]} .. {d['lags'][1]} | {d['body_sums_ms']:.3f} ms ({d['body_sums_range'][0]:.3f} .. {d['body_sums_range'][1]:.3f}) | "
                     f"{d['frame_sums_ms']:.3f} ms ({d['frame_sums_range'][0]:.3f} .. {d['frame_sums_range'][1]:.3f}) | {d['ratio_body_over_frame']:.2f} x | "
                     f"{h['copy_ms']:.2f} ms + {h['numpy_ms']:.0f} ms ({h['numpy_range_ms'][0]:.0f} .. {h['numpy_range_ms'][1]:.0f}) |")
    r, tr = result["rebody_rows"], result["body_sums_truth_rotations_range"]
    lines += ["", f"`body_sums` with the truth's rotations (lag 0, no message): {result['body_sums_truth_rotations_ms']:.3f} ms ({tr[0]:.3f} .. {tr[1]:.3f}).", "",
              f"`rebody_rows`: {r['ms']:.3f} ms ({r['range'][0]:.3f} .. {r['range'][1]:.3f}); it moves {r['bytes_moved'] / 1e6:.1f} MB, "
              f"{100 * r['share_of_hbm_peak']:.1f} % of the 8 TB/s HBM peak over that time.", "",
              f"`align_body` end to end over lags {SWEEPS[1][0]} .. {SWEEPS[1][1]} (with the wait for `best_body` on the host): {result['align_body_ms']:.3f} ms "
              f"({result['align_body_range'][0]:.3f} .. {result['align_body_range'][1]:.3f}).", ""]
    if "unchanged" in result:
        u = result["unchanged"]
        lines += ["Untouched paths, this build and a build of the parent commit alternating on the same buffers (est truth, 17 lags for the sums):", "",
                  "| entry | this build | parent build |", "|---|---|---|"]
        for name in ("score_rows", "frame_sums"):
            a, b = u[f"{name}_this"], u[f"{name}_parent"]
            lines.append(f"| `ape_{name}` | {a['ms']:.3f} ms ({a['range'][0]:.3f} .. {a['range'][1]:.3f}) | {b['ms']:.3f} ms ({b['range'][0]:.3f} .. {b['range'][1]:.3f}) |")
        lines.append("")
    else:
        lines += ["Untouched paths against a build of the parent commit: not measured in this run (`--parent-lib`).", ""]
    old = Path(args.out).read_text() if Path(args.out).exists() else ""
    notes = "\n" + old[old.index(NOTES):] if NOTES in old else ""
    Path(args.out).write_text((old[:old.index(MARKER)] if MARKER in old else old.rstrip() + "\n\n") + "\n".join(lines) + notes)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
