"""Windowed post-filter (score.post_window / ape_post_window): 100 000 pocket frames in 10 recordings at 25 Monte-Carlo
samples.  Legs, alternating within one session behind warmed shapes, timed by HIP events; the yardstick of every window leg is
post_sweep at the same stack heights in the same session:

    sweep 5         one post_sweep of the causal widths (1, 3, 5, 10, 20) x 25 samples with the spread records
    causal 5        the same five stacks as uniform windows (w - 1, 0, 25): what the two-sided clamp and the table lookups cost
    centred 5       the same widths centred, uniform: (w // 2, w - 1 - w // 2, 25)
    centred hann 5  the same windows with Hann weights: what the weighted statements cost
    sweep 1         post_sweep at C = 1, (smooth 10, 25 samples)
    window 1        post_window at C = 1: (9, 0, 25) uniform, (5, 4, 25) uniform, (5, 4, 25) Hann

With --parent-tree DIR (a checkout of the parent commit with its library built; both trees have both entries) the same calls are
timed in child processes that alternate between that tree and this one, three runs each: post_sweep of the five causal configurations
and at C = 1, the five causal stacks as windows, the five centred Hann windows, one pair that takes the LDS form (smooths 1 .. 10 at 4
samples as a sweep, the same stacks as centred uniform windows) and, as a control, score_lags at 17 lags and process_recording at smooth
10 x 25 samples.  A leg is accepted when this build's median lies within the parent's own range of runs, or above its maximum by no
more than the width of that range.  Writes profiles/post_window.md's measured section and prints ONE JSON line.

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


PARENT_LEGS = {"sweep5": "`post_sweep` of the five causal configurations", "sweep1": "`post_sweep` at C = 1, (10, 25)",
               "causal5": "the five causal stacks as uniform windows", "hann5": "the five centred Hann windows",
               "lds_sweep": "`post_sweep` of smooths 1 .. 10 at 4 samples (LDS form)",
               "lds_centred": "the same ten stacks as centred uniform windows (LDS form)",
               "lags17": "control: `score_lags` at 17 lags", "replay": "control: `process_recording(spread=True)` at (10, 25)"}


def parent_legs(F, repeats):
    """the legs both trees can run, on whichever tree APE_BENCH_TREE names: -> {leg of PARENT_LEGS: ms}"""
    import torch
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(0)
    starts = [r * (F // 10) for r in range(10)]
    centred = [(w // 2, w - 1 - w // 2, SAMPLES) for w in WIDTHS]
    with tempfile.TemporaryDirectory() as tmp:
        est = estimator(tmp, *OWN)
        rows = torch.as_tensor(rows_for(F, rng)).cuda()
        out, y, spread = est.process_recording(rows, starts=starts, return_targets=True, spread=True)
        truth = (y.double().mean(dim=1) * torch.as_tensor(est._yy_s, device=y.device) + torch.as_tensor(est._yy_m, device=y.device)).contiguous()
        legs = {"sweep5": lambda: est.repost(y, [(w, SAMPLES) for w in WIDTHS], starts=starts, spread=True),
                "sweep1": lambda: est.repost(y, [OWN], starts=starts, spread=True),
                "causal5": lambda: est.repost_windows(y, [(w - 1, 0, SAMPLES) for w in WIDTHS], starts=starts, spread=True),
                "hann5": lambda: est.repost_windows(y, [score.window(b, f, m, "hann") for b, f, m in centred], starts=starts, spread=True),
                "lds_sweep": lambda: est.repost(y, [(w, 4) for w in range(1, 11)], starts=starts, spread=True),
                "lds_centred": lambda: est.repost_windows(y, [(w // 2, w - 1 - w // 2, 4) for w in range(1, 11)], starts=starts, spread=True)}
        res = {name: timed(f, repeats)[0] for name, f in legs.items()}
        assert score.post_sweep_last()["lds"] and score.post_window_last()["lds"]      # each entry's last call: the LDS pair
        res["lags17"] = timed(lambda: score.score_lags(est._layout, out, truth, (-8, 8), "targets", spread, starts, 5, est.body_measurements), 4 * repeats, 3)[0]
        res["replay"] = timed(lambda: est.process_recording(rows, starts=starts, spread=True), repeats)[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "post_window.md"))
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == "parent":
        print(json.dumps(parent_legs(a.frames, a.repeats)))
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
                p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--leg", "parent", "--frames", str(F), "--repeats", str(a.repeats)],
                                   env=env, capture_output=True, text=True, check=True)
                runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
        res["parent_legs"] = runs
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
        lines += [f"Against a build of the parent commit, child processes alternating between the two trees, {RUNS} runs each (ms):", "",
                  "| leg | parent min - max (median) | this build min - max (median) | this median |", "|---|---|---|---|"]
        for key, name in PARENT_LEGS.items():
            par, this = [r[key] for r in res["parent_legs"]["parent"]], [r[key] for r in res["parent_legs"]["this"]]
            med, lo, hi = float(np.median(this)), min(par), max(par)
            verdict = "inside the parent's range" if lo <= med <= hi else "below the parent's range" if med < lo else \
                f"{med - hi:.3f} above the parent's maximum, the range is {hi - lo:.3f} wide: " + ("accepted" if med - hi <= hi - lo else "NOT accepted")
            res["parent_legs"][key] = verdict
            lines.append(f"| {name} | {lo:.3f} - {hi:.3f} ({np.median(par):.3f}) | {min(this):.3f} - {max(this):.3f} ({med:.3f}) | {verdict} |")
        lines.append("")
    out = Path(a.out)
    old = out.read_text() if out.exists() else "# Windowed post-filter (DESIGN.md 4.43)\n\n"
    head = old[:old.index(MARKER)] if MARKER in old else old
    tail = old[old.index(NOTES):] if NOTES in old else ""
    out.write_text(head + "\n".join(lines) + "\n" + tail)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
