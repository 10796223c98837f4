"""Scoring a replay against ground truth (score.score_rows / ape_score_rows): the time to score 100 000 pocket frames
whose rows are process_recording(spread=True) output at 25 Monte-Carlo samples, in float64 and float32, beside the replay call that
made the rows and beside the route without it (copy the rows to the host, score_rows_numpy there).  Writes profiles/score.md and
prints ONE JSON line.

    python tools/score_bench.py [--frames 100000] [--repeats 5] [--out profiles/score.md]

Without a GPU the file says that the run could not be made and holds no number.  Models carry seeded synthetic weights (the deployed
checkpoints are not shipped); rows and truth are synthetic: the times do not depend on the values."""
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

HBM_PEAK = 8.0e12          # bytes / s, the MI355X's nominal HBM3E rate


def timed(fn, repeats):
    import torch
    ms = []
    for _ in range(repeats):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        keep = fn()
        z.record()
        z.synchronize()
        ms.append(a.elapsed_time(z))
        del keep
    return float(np.median(ms)), [round(v, 4) for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "score.md"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    head = ["# Scoring replayed poses against ground truth (`tools/score_bench.py`)", ""]
    if not torch.cuda.is_available():
        Path(args.out).write_text("\n".join(head + ["The run could not be made: no GPU was visible to `tools/score_bench.py`.  No figure has been measured.", ""]))
        print(json.dumps({"error": "no GPU"}))
        return
    from replay_bench import deploy_tree, rows_for
    from wear_mocap_ape_amd import config, score
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import WatchPhonePocketNN
    torch.cuda.set_device(0)
    F, n_mc = args.frames, 25
    result = {"frames": F, "n_mc": n_mc, "repeats": args.repeats, "dtypes": {}}
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as tmp:
        shipped, deploy = Path(config.PATHS["deploy"]), Path(tmp) / "deploy"
        config.PATHS["deploy"] = deploy
        est = WatchPhonePocketNN(model_hash=deploy_tree(shipped, deploy, "pocket", 0.2), smooth=1, add_mc_samples=True, monte_carlo_samples=n_mc)
        rd = torch.from_numpy(rows_for("pocket", F)).cuda()
        O = 14
        truth = torch.from_numpy(rng.normal(size=(F, O))).cuda()                   # finite targets: every frame is scored
        starts = list(range(0, F, 10_000))
        for name, dt in (("float64", torch.float64), ("float32", torch.float32)):
            replay = lambda: est.process_recording(rd, starts=starts, out_dtype=dt, spread=True)          # noqa: E731
            out, rec = replay()
            tt = truth.to(dt)
            torch.cuda.synchronize()
            replay_ms, _ = timed(replay, max(2, args.repeats // 2))
            call = lambda: est.score_recording(out, tt, spread=rec, starts=starts)  # noqa: E731
            call()
            torch.cuda.synchronize()
            score_ms, score_all = timed(call, args.repeats)
            acc_only = lambda: score.score_rows(est._layout, out, tt, "targets", rec, starts, est.sequence_len - 1,   # noqa: E731
                                                est.body_measurements, per_frame=False)
            acc_only()
            torch.cuda.synchronize()
            acc_ms, _ = timed(acc_only, args.repeats)
            # the route without it: the same rows to the host, numpy there (est-kind truth: the FK is not even counted)
            truth_e = rng.normal(size=(F, 21))
            parent = out._base if out._base is not None else out                    # (the views' parent is what a user copies)
            torch.cuda.synchronize()
            d2h, host_np = [], []
            for _ in range(args.repeats):                                           # the same number of repeats, medians like the device route
                t0 = time.perf_counter()
                host = parent.cpu().numpy()                                         # (pageable memory, allocated by the call: what a user does)
                t1 = time.perf_counter()
                s = score.score_rows_numpy(host[:, :25], truth_e, est._layout, host[:, -21:])
                score.accumulate_numpy(s, starts, est.sequence_len - 1)
                t2 = time.perf_counter()
                d2h.append(t1 - t0)
                host_np.append(t2 - t1)
            d2h_s, np_s = float(np.median(d2h)), float(np.median(host_np))
            esz = 8 if dt == torch.float64 else 4
            must_read = F * ((25 + 21) * esz + O * esz)
            written = F * 7 * 8
            result["dtypes"][name] = {
                "row_width": int(parent.shape[1]), "rows_bytes": int(parent.numel() * esz),
                "replay_ms": round(replay_ms, 3), "score_ms": round(score_ms, 4), "score_ms_all": score_all, "acc_only_ms": round(acc_ms, 4),
                "d2h_ms": round(d2h_s * 1e3, 2), "numpy_ms": round(np_s * 1e3, 2),
                "must_read_bytes": must_read, "written_bytes": written,
                "read_bytes_per_s": round(must_read / (score_ms * 1e-3)), "fraction_of_hbm_peak": round(must_read / (score_ms * 1e-3) / HBM_PEAK, 4)}
            del out, rec
        del est
    marker = "## Parity figures of the GPU tests"                                   # written by hand from the tests' output: kept
    old = Path(args.out).read_text() if Path(args.out).exists() else ""
    lines = head + [
        f"One run of `python tools/score_bench.py --frames {F} --repeats {args.repeats}` on one MI355X: {F} pocket frames in {len(starts)} recordings, "
        f"rows from `process_recording(spread=True)` at {n_mc} Monte-Carlo samples (`[F, 25 + 6 * {n_mc} + 21]`), truth as NN targets "
        "(so the truth FK is inside the time), per-frame rows and accumulators both written.  Times are medians of device events around "
        "the Python call; the host route (a copy into fresh pageable memory, then numpy on one core, est-kind truth so no FK) is the median "
        "of the same number of repeats by the host clock.  Nothing was fixed in advance.", "",
        "| rows | row bytes | replay that made them | `score_recording` | accumulators only | D2H copy of the rows | numpy on the host | copy + numpy / score |",
        "|---|---|---|---|---|---|---|---|"]
    for name, d in result["dtypes"].items():
        lines.append(f"| {name} | {d['rows_bytes'] / 1e6:.1f} MB | {d['replay_ms']:.1f} ms | {d['score_ms']:.3f} ms | {d['acc_only_ms']:.3f} ms | "
                     f"{d['d2h_ms']:.1f} ms | {d['numpy_ms']:.1f} ms | {(d['d2h_ms'] + d['numpy_ms']) / d['score_ms']:.0f} x |")
    lines += ["", "Bytes the kernel must read (25 message + 21 record columns of every row, and the truth row; the `6N` columns between them "
              "are never touched) over the time of the call:", "",
              "| rows | must read | bytes / s | of the 8 TB/s HBM peak |", "|---|---|---|---|"]
    for name, d in result["dtypes"].items():
        lines.append(f"| {name} | {d['must_read_bytes'] / 1e6:.1f} MB | {d['read_bytes_per_s'] / 1e12:.3f} TB/s | {100 * d['fraction_of_hbm_peak']:.1f} % |")
    lines += ["", "How to read the fraction: the time is that of the whole call as a user makes it (one 25 + 21-column gather kernel with the "
              "truth FK, the per-recording combine, a small staged copy of starts and bodies, and the Python around them), not of the "
              "gather kernel alone; and the rows, written by the replay just before, are smaller than the 256 MiB Infinity Cache, so part "
              "of the read may never have reached HBM.  The figure is a lower bound of what the kernel sustains, not a roofline "
              "measurement.  At this size the call is far from the memory bound -- 391 workgroups of one-lane-per-frame float64 chains (the truth FK, three asin) over 256 CUs, plus the launches and the staged copy -- so the time is the figure to read; where the rest of the time goes has not been profiled.", ""]
    if marker in old:
        lines += [old[old.index(marker):].rstrip(), ""]
    Path(args.out).write_text("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
