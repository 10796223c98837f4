"""Windowed post-filter (score.post_window / ape_post_window): 100 000 pocket frames in 10 recordings at 25 Monte-Carlo
samples.  Legs, alternating within one session behind warmed shapes, timed by HIP events; the yardstick of every window leg is
post_sweep at the same stack heights in the same session:

    sweep 5         one post_sweep of the causal widths (1, 3, 5, 10, 20) x 25 samples with the spread records
    causal 5        the same five stacks as uniform windows (w - 1, 0, 25): what the two-sided clamp and the table lookups cost
    centred 5       the same widths centred, uniform: (w // 2, w - 1 - w // 2, 25)
    centred hann 5  the same windows with Hann weights: what the weighted statements cost
    sweep 1         post_sweep at C = 1, (smooth 10, 25 samples)
    window 1        post_window at C = 1: (9, 0, 25) uniform, (5, 4, 25) uniform, (5, 4, 25) Hann

With --parent-tree DIR (a checkout of the parent commit with its library built) the unchanged paths -- post_sweep of the five causal
configurations, score_lags at 17 lags and process_recording at smooth 10 x 25 samples -- are also timed in child processes that
alternate between that tree and this one, three runs each: this build's median against the parent's own run-to-run range.  Writes
profiles/post_window.md's measured section and prints ONE JSON line.

    python tools/post_window_bench.py [--frames 100000] [--repeats 5] [--parent-tree DIR] [--out profiles/post_window.md]

The model carries seeded synthetic weights and the rows are synthetic: the times do not depend on the values."""
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

from post_sweep_bench import OWN, estimator, rows_for, timed  # noqa: E402

WIDTHS, SAMPLES = [1, 3, 5, 10, 20], 25
RUNS = 3
MARKER, NOTES = "## Measured", "### Reading the figures"       # the section this tool writes; what follows it is written by hand and kept


def unchanged_leg(F, repeats):
    """the paths this feature does not touch, on whichever tree APE_BENCH_TREE names: -> {"sweep5": ms, "lags17": ms, "replay": ms}"""
    import torch
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(0)
    starts = [r * (F // 10) for r in range(10)]
    with tempfile.TemporaryDirectory() as tmp:
        est = estimator(tmp, *OWN)
        rows = torch.as_tensor(rows_for(F, rng)).cuda()
        out, y, spread = est.process_recording(rows, starts=starts, return_targets=True, spread=True)
        truth = (y.double().mean(dim=1) * torch.as_tensor(est._yy_s, device=y.device) + torch.as_tensor(est._yy_m, device=y.device)).contiguous()
        swp = timed(lambda: est.repost(y, [(w, SAMPLES) for w in WIDTHS], starts=starts, spread=True), repeats)[0]
        lag = timed(lambda: score.score_lags(est._layout, out, truth, (-8, 8), "targets", spread, starts, 5, est.body_measurements), 4 * repeats, 3)[0]
        rep = timed(lambda: est.process_recording(rows, starts=starts, spread=True), repeats)[0]
    return {"sweep5": swp, "lags17": lag, "replay": rep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "post_window.md"))
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == "unchanged":
        print(json.dumps(unchanged_leg(a.frames, a.repeats)))
        return
    import torch
    from wear_mocap_ape_amd import score
    F, rng = a.frames, np.random.default_rng(0)
    starts = [r * (F // 10) for r in range(10)]
    configs = [(w, SAMPLES) for w in WIDTHS]
    causal = [(w - 1, 0, SAMPLES) for w in WIDTHS]
    centred = [(w // 2, w - 1 - w // 2, SAMPLES) for w in WIDTHS]
    hann = [score.window(b, f, m, "hann") for b, f, m in centred]
    res = {"frames": F, "recordings": 10, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        est = estimator(tmp, *OWN)
        rows = torch.as_tensor(rows_for(F, rng)).cuda()
        _, y = est.process_recording(rows, starts=starts, return_targets=True, _config=(1, SAMPLES))
        legs = [("sweep5", lambda: est.repost(y, configs, starts=starts, spread=True), score.post_sweep_last),
                ("causal5", lambda: est.repost_windows(y, causal, starts=starts, spread=True), score.post_window_last),
                ("centred5", lambda: est.repost_windows(y, centred, starts=starts, spread=True), score.post_window_last),
                ("hann5", lambda: est.repost_windows(y, hann, starts=starts, spread=True), score.post_window_last),
                ("sweep1", lambda: est.repost(y, [OWN], starts=starts, spread=True), score.post_sweep_last),
                ("causal1", lambda: est.repost_windows(y, [(9, 0, SAMPLES)], starts=starts, spread=True), score.post_window_last),
                ("centred1", lambda: est.repost_windows(y, [(5, 4, SAMPLES)], starts=starts, spread=True), score.post_window_last),
                ("hann1", lambda: est.repost_windows(y, [score.window(5, 4, SAMPLES, "hann")], starts=starts, spread=True), score.post_window_last)]
        for name, f, last in legs:
            res[name + "_ms"], res[name + "_all"] = timed(f, a.repeats)
            res[name + "_plan"] = last()
        # the bits: the causal windows against the sweep at the same stacks
        so, ss = est.repost(y, configs, starts=starts, spread=True)
        wo, ws = est.repost_windows(y, causal, starts=starts, spread=True)
        res["bits_equal"] = bool(torch.equal(so, wo) and torch.equal(ss, ws))
    if a.parent_tree:
        runs = {"parent": [], "this": []}
        for _ in range(RUNS):
            for name, tree in (("parent", a.parent_tree), ("this", str(ROOT))):
                env = dict(os.environ, APE_BENCH_TREE=str(tree), APE_HIP_LIB=str(Path(tree) / "arm-pose-estimation_amd" / "lib" / "libape_hip.so"))
                p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--leg", "unchanged", "--frames", str(F), "--repeats", str(a.repeats)],
                                   env=env, capture_output=True, text=True, check=True)
                runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
        res["unchanged"] = runs
    what = {"sweep5": "one `post_sweep` of the causal widths 1, 3, 5, 10, 20 at 25 samples, spread records included",
            "causal5": "the same five stacks as uniform windows `(w - 1, 0, 25)`", "centred5": "the same widths centred, uniform",
            "hann5": "the same widths centred, Hann weights", "sweep1": "`post_sweep` at C = 1, (10, 25)",
            "causal1": "`post_window` at C = 1, (9, 0, 25) uniform", "centred1": "`post_window` at C = 1, (5, 4, 25) uniform",
            "hann1": "`post_window` at C = 1, (5, 4, 25) Hann"}
    lines = [MARKER, "", f"`tools/post_window_bench.py --frames {F} --repeats {a.repeats}` on one {res['device']}, one session; medians, HIP events.", "",
             "| leg | ms | all runs |", "|---|---|---|"]
    lines += [f"| {what[k]} ({res[k + '_plan']}) | {res[k + '_ms']:.2f} | {res[k + '_all']} |" for k in what]
    lines += ["", f"The causal windows against the sweep at the same stacks: bits equal = {res['bits_equal']}.", ""]
    if a.parent_tree:
        for key, name in (("sweep5", "`post_sweep` of the five causal configurations"), ("lags17", "`score_lags` at 17 lags"),
                          ("replay", "`process_recording(spread=True)` at (10, 25)")):
            par, this = [r[key] for r in res["unchanged"]["parent"]], [r[key] for r in res["unchanged"]["this"]]
            lines.append(f"Unchanged path {name}: parent {min(par):.3f} - {max(par):.3f} ms over {RUNS} runs (median {np.median(par):.3f}), "
                         f"this build {min(this):.3f} - {max(this):.3f} ms (median {np.median(this):.3f}).")
        lines.append("")
    out = Path(a.out)
    old = out.read_text() if out.exists() else "# Windowed post-filter (DESIGN.md 4.43)\n\n"
    head = old[:old.index(MARKER)] if MARKER in old else old
    tail = old[old.index(NOTES):] if NOTES in old else ""
    out.write_text(head + "\n".join(lines) + "\n" + tail)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
