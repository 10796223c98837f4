"""Post-filter sweep (score.post_sweep / ape_post_sweep): 100 000 pocket frames in 10 recordings at 25 Monte-Carlo
samples.  Legs, alternating within one session behind warmed shapes, timed by HIP events:

    replay        the one process_recording(return_targets=True) at 25 samples that produces y
    sweep 25      one post_sweep of grid([1, 3, 5, 10, 20], [1, 4, 8, 16, 25]) with the spread records
    replays x 25  the route a user has without it: the same 25 configurations as 25 process_recording(spread=True) calls of this build
    sweep 1       post_sweep at C = 1, (smooth 10, 25 samples): what the replay's own post-filter does for its one configuration
    replay 10x25  the replay at that configuration; its post-filter share is not separated here (a kernel trace does that, in a run of
                  its own:  rocprofv3 --kernel-trace --stats -- python tools/post_sweep_bench.py --frames 100000 --repeats 3 --only replay)

With --parent-tree DIR (a checkout of the parent commit with its library built) the unchanged paths -- process_recording at smooth 10 x
25 samples and score_lags at 17 lags -- are also timed in child processes that alternate between that tree and this one, three runs
each: this build's median against the parent's own run-to-run range.  Writes profiles/post_sweep.md's measured section and prints ONE
JSON line.

    python tools/post_sweep_bench.py [--frames 100000] [--repeats 5] [--parent-tree DIR] [--out profiles/post_sweep.md]

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

SMOOTHS, SAMPLES, OWN = [1, 3, 5, 10, 20], [1, 4, 8, 16, 25], (10, 25)
RUNS = 3
MARKER, NOTES = "## Measured", "### Reading the figures"       # the section this tool writes; what follows it is written by hand and kept


def timed(f, repeats, warmup=1):
    import torch
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        keep = f()
        z.record()
        z.synchronize()
        ms.append(a.elapsed_time(z))
        del keep
    return float(np.median(ms)), [round(x, 3) for x in ms]


def estimator(tmp, smooth, mc):
    """a pocket estimator on seeded weights with dropout 0.2 (tests/test_hip_parity._deploy_dir writes the deploy tree)"""
    from wear_mocap_ape_amd import config
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import WatchPhonePocketNN
    from tests.test_hip_parity import _deploy_dir
    deploy, h = _deploy_dir(Path(tmp) / f"s{smooth}m{mc}", "pocket", 2, dropout=0.2)
    config.PATHS["deploy"] = deploy
    return WatchPhonePocketNN(model_hash=h, smooth=smooth, add_mc_samples=False, monte_carlo_samples=mc)


def rows_for(F, rng):
    base = np.load(TREE / "tests" / "golden" / "stream_trace_pocket.npz")["rows"].astype(np.float32)
    rows = np.tile(base, ((F + len(base) - 1) // len(base), 1))[:F]
    return rows + np.float32(1e-3) * rng.standard_normal(rows.shape, dtype=np.float32)


def unchanged_leg(F, repeats):
    """the paths this feature does not touch, on whichever tree APE_BENCH_TREE names: -> {"replay": ms, "lags17": ms}"""
    import torch
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(0)
    starts = [r * (F // 10) for r in range(10)]
    with tempfile.TemporaryDirectory() as tmp:
        est = estimator(tmp, *OWN)
        rows = torch.as_tensor(rows_for(F, rng)).cuda()
        out, y, spread = est.process_recording(rows, starts=starts, return_targets=True, spread=True)
        truth = (y.double().mean(dim=1) * torch.as_tensor(est._yy_s, device=y.device) + torch.as_tensor(est._yy_m, device=y.device)).contiguous()
        rep = timed(lambda: est.process_recording(rows, starts=starts, spread=True), repeats)[0]
        lag = timed(lambda: score.score_lags(est._layout, out, truth, (-8, 8), "targets", spread, starts, 5, est.body_measurements), 4 * repeats, 3)[0]
    return {"replay": rep, "lags17": lag}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "post_sweep.md"))
    ap.add_argument("--only", default=None, help="replay: the replay leg alone (for a kernel trace)")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == "unchanged":
        print(json.dumps(unchanged_leg(a.frames, a.repeats)))
        return
    import torch
    from wear_mocap_ape_amd import score
    F, rng = a.frames, np.random.default_rng(0)
    starts = [r * (F // 10) for r in range(10)]
    configs = score.grid(SMOOTHS, SAMPLES)
    res = {"frames": F, "recordings": 10, "configs": len(configs), "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        est = estimator(tmp, *OWN)
        rows = torch.as_tensor(rows_for(F, rng)).cuda()
        if a.only == "replay":
            print(json.dumps({"replay_ms": timed(lambda: est.process_recording(rows, starts=starts, spread=True), a.repeats)[0]}))
            return
        _, y = est.process_recording(rows, starts=starts, return_targets=True, _config=(1, max(SAMPLES)))
        res["replay_ms"] = timed(lambda: est.process_recording(rows, starts=starts, return_targets=True, _config=(1, max(SAMPLES))), a.repeats)[0]
        res["sweep25_ms"], res["sweep25_all"] = timed(lambda: est.repost(y, configs, starts=starts, spread=True), a.repeats)
        res["sweep25_plan"] = score.post_sweep_last()
        res["replays_x25_ms"] = timed(lambda: [est.process_recording(rows, starts=starts, spread=True, _config=c)[0][:1].clone() for c in configs],
                                      max(1, a.repeats // 2), 1)[0]
        res["sweep1_ms"], res["sweep1_all"] = timed(lambda: est.repost(y, [OWN], starts=starts, spread=True), a.repeats)
        res["sweep1_plan"] = score.post_sweep_last()
        res["replay_own_ms"] = timed(lambda: est.process_recording(rows, starts=starts, spread=True), a.repeats)[0]
        # the bits: the sweep's (10, 25) against the replay at that configuration
        ro, rr = est.process_recording(rows, starts=starts, spread=True)
        out, spread = est.repost(y, configs, starts=starts, spread=True)
        c = configs.index(OWN)
        res["bits_equal"] = bool(torch.equal(out[c], ro[:, :25]) and torch.equal(spread[c], rr))
    if a.parent_tree:
        runs = {"parent": [], "this": []}
        for _ in range(RUNS):
            for name, tree in (("parent", a.parent_tree), ("this", str(ROOT))):
                env = dict(os.environ, APE_BENCH_TREE=str(tree), APE_HIP_LIB=str(Path(tree) / "arm-pose-estimation_amd" / "lib" / "libape_hip.so"))
                p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--leg", "unchanged", "--frames", str(F), "--repeats", str(a.repeats)],
                                   env=env, capture_output=True, text=True, check=True)
                runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
        res["unchanged"] = runs
    lines = [MARKER, "", f"`tools/post_sweep_bench.py --frames {F} --repeats {a.repeats}` on one {res['device']}, one session; medians, HIP events.", "",
             "| leg | ms |", "|---|---|",
             f"| replay that produces y (smooth 1 x 25 samples, targets returned) | {res['replay_ms']:.1f} |",
             f"| one `post_sweep` of the 25 configurations, spread records included ({res['sweep25_plan']}) | {res['sweep25_ms']:.2f} |",
             f"| the same 25 configurations as 25 `process_recording(spread=True)` calls | {res['replays_x25_ms']:.1f} |",
             f"| `post_sweep` at C = 1, (10, 25) ({res['sweep1_plan']}) | {res['sweep1_ms']:.2f} |",
             f"| `process_recording(spread=True)` at (10, 25), regressor included | {res['replay_own_ms']:.1f} |", "",
             f"The sweep's (10, 25) against that replay: bits equal = {res['bits_equal']}.", ""]
    if a.parent_tree:
        for key, what in (("replay", "`process_recording(spread=True)` at (10, 25)"), ("lags17", "`score_lags` at 17 lags")):
            par, this = [r[key] for r in res["unchanged"]["parent"]], [r[key] for r in res["unchanged"]["this"]]
            lines.append(f"Unchanged path {what}: parent {min(par):.3f} - {max(par):.3f} ms over {RUNS} runs (median {np.median(par):.3f}), "
                         f"this build {min(this):.3f} - {max(this):.3f} ms (median {np.median(this):.3f}).")
        lines.append("")
    out = Path(a.out)
    old = out.read_text() if out.exists() else "# Post-filter sweep (DESIGN.md 4.33)\n\n"
    head = old[:old.index(MARKER)] if MARKER in old else old
    tail = old[old.index(NOTES):] if NOTES in old else ""
    out.write_text(head + "\n".join(lines) + "\n" + tail)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
