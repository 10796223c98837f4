"""Offline replay throughput (Estimator.process_recording / ape_replay): frames per second of whole recordings
resident on the device, against the per-frame process_row loop over the first 2 000 of the same rows.  Prints ONE JSON line.

    python tools/replay_bench.py [--frames 100000] [--repeats 3]

Models carry seeded synthetic weights (the deployed checkpoints are not shipped); the rows are the recorded trace of
tests/golden/stream_trace_<name>.npz tiled to length with a little noise."""
import argparse
import json
import shutil
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for _p in (str(ROOT), str(ROOT / "arm-pose-estimation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HASHES = {"pocket": "670b66fa7664252d1cfb3b5a8a362002ffeeba5c", "watch": "04f4ad63bfccb3668f7598c9375403e10b1fae2a",
          "uarm": "7cb5cdf94ef4c66388c7f15f642005d5e008146a"}
# name, model, Monte-Carlo samples, smooth
CONFIGS = [("pocket_T6_mc1_s1", "pocket", 1, 1), ("pocket_T6_mc25_s1", "pocket", 25, 1),
           ("watch_T8_mc25_s10", "watch", 25, 10), ("uarm_T6_mc50_s1", "uarm", 50, 1)]


def deploy_tree(src: Path, dst: Path, name: str, dropout: float) -> str:
    """a copy of the shipped deploy tree `src` with a seeded synthetic checkpoint in the reference's (model_state, optimizer_state) format"""
    import torch
    from oracle import ape_oracle as orc
    shutil.copytree(src / "data_stats", dst / "data_stats", dirs_exist_ok=True)
    d = dst / "nn" / HASHES[name]
    d.mkdir(parents=True, exist_ok=True)
    p = json.loads((src / "nn" / HASHES[name] / "results.json").read_text())
    p["dropout"] = dropout
    (d / "results.json").write_text(json.dumps(p))
    cfg = orc.MODEL_CONFIGS[name]
    sd = orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], 0)
    torch.save(({k: torch.from_numpy(v) for k, v in sd.items()}, {"state": {}, "param_groups": []}), d / "checkpoint.pt")
    return HASHES[name]


def rows_for(name: str, F: int) -> np.ndarray:
    base = np.load(ROOT / "tests" / "golden" / f"stream_trace_{name}.npz")["rows"].astype(np.float32)
    rows = np.tile(base, ((F + len(base) - 1) // len(base), 1))[:F]
    rows += np.float32(1e-3) * np.random.default_rng(F).standard_normal(rows.shape, dtype=np.float32)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-frames", type=int, default=2000)
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    from wear_mocap_ape_amd import config
    from wear_mocap_ape_amd.estimate.watch_only import WatchOnlyNN
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import WatchPhonePocketNN
    from wear_mocap_ape_amd.estimate.watch_phone_uarm_nn import WatchPhoneUarmNN
    torch.cuda.set_device(0)
    classes = {"pocket": WatchPhonePocketNN, "watch": WatchOnlyNN, "uarm": WatchPhoneUarmNN}
    result = {"frames": args.frames, "repeats": args.repeats, "configs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        shipped, deploy = Path(config.PATHS["deploy"]), Path(tmp) / "deploy"
        config.PATHS["deploy"] = deploy
        for tag, name, mc, smooth in CONFIGS:
            h = deploy_tree(shipped, deploy, name, 0.0 if mc == 1 else 0.2)      # (1, 1): the deterministic regressor
            est = classes[name](model_hash=h, smooth=smooth, add_mc_samples=True, monte_carlo_samples=mc)
            rows = rows_for(name, args.frames)
            rd = torch.from_numpy(rows).cuda()
            est.process_recording(rd)                         # warm-up (workspaces, code objects)
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.repeats):
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = est.process_recording(rd)
                z.record()
                z.synchronize()
                ms.append(a.elapsed_time(z))
                del out
            med = float(np.median(ms))
            kernel = est._hip_model().last_kernel()
            # baseline: a fresh estimator's process_row loop over the first rows of the same recording
            est.reset()
            n_loop = min(args.loop_frames, args.frames)
            for r in rows[:50]:
                est.process_row(r)
            est.reset()
            t0 = time.perf_counter()
            for r in rows[:n_loop]:
                est.process_row(r)
            loop_s = time.perf_counter() - t0
            result["configs"][tag] = {"T": est.sequence_len, "n_mc": mc, "smooth": smooth, "ms_median": round(med, 3),
                                      "ms_all": [round(v, 3) for v in ms], "frames_per_s": round(args.frames / (med * 1e-3)),
                                      "loop_frames_per_s": round(n_loop / loop_s), "speedup": round(args.frames / (med * 1e-3) / (n_loop / loop_s), 1),
                                      "regressor_kernel": kernel}
            del est, rd
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
