#!/usr/bin/env python3
"""Timing of the stream banks with and without per-stream body measurements: the lockstep frame of

  pocket_1024_mc1   StreamBank, pocket model, S = 1024, T = 6, smooth 5, one sample per stream
  pocket_1024_mc25  the same bank with 25 Monte-Carlo samples
  fk_8192, fk_65536 FkStreamBank (the estimator without a regressor), smooth 5

in `uniform` mode (the bank was never given bodies: the body travels in the kernel arguments) and in `table` mode (S distinct bodies),
HIP events around each frame after un-timed frames that settle the clocks, the two modes alternating, REPEATS times each; per repeat
the p50 over the timed frames.  Run it on the parent commit (it then reports `uniform` only: no set_bodies there) and on this one in the
same session; the allowance for `uniform` is the parent's own spread over its repeats.

python tools/bodies_bench.py [--out profiles/bodies_bench.json] [--label NAME] [--quick]"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "arm-pose-estimation_amd")]

import torch  # noqa: E402

REPEATS = 5


def frame_us(fn, warm, frames):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(frames):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return float(np.percentile(us, 50))


def random_bodies(rng, n):
    b = np.zeros((n, 9))
    b[:, 0], b[:, 3] = -rng.uniform(0.18, 0.33, n), -rng.uniform(0.22, 0.40, n)
    b[:, 6:9] = rng.uniform([-0.25, 0.35, -0.1], [-0.12, 0.55, 0.1], (n, 3))
    return b


def legs(quick):
    from oracle import ape_oracle as orc
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import nn_models
    from wear_mocap_ape_amd.streams import FkStreamBank, StreamBank
    rng = np.random.default_rng(0)
    base = np.load(REPO / "tests" / "golden" / "stream_trace_pocket.npz")["rows"].astype(np.float32)
    cfg = orc.MODEL_CONFIGS["pocket"]
    model = nn_models.DropoutLSTM(cfg["I"], cfg["H"], cfg["L"], cfg["O"], dropout=0.2, target_layout=cfg["layout"])
    model.load_state_dict(orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], 3))
    out = {}
    has_table = hasattr(StreamBank, "set_bodies")
    for mc in (None, 25):
        S = 1024
        rows = torch.from_numpy(base[rng.integers(0, len(base), S)]).cuda()
        banks = {"uniform": StreamBank(model, S, 6, smooth=5, normalize=False, monte_carlo_samples=mc)}
        if has_table:
            banks["table"] = StreamBank(model, S, 6, smooth=5, normalize=False, monte_carlo_samples=mc)
            banks["table"].set_bodies(random_bodies(rng, S))

        def frame(bank):
            bank.push_rows(rows, _hip.PARSE_WATCH_PHONE_POCKET)
            bank.step_datagrams()

        res = {k: [] for k in banks}
        for _ in range(REPEATS):
            for k, bank in banks.items():
                res[k].append(frame_us(lambda: frame(bank), 20 if quick else 100, 50 if quick else (300 if mc is None else 100)))
        model.check()
        out[f"pocket_1024_mc{mc or 1}"] = res
    for S in (8192, 65536):
        rows = torch.from_numpy(np.tile(base, (S // len(base) + 1, 1))[:S].copy()).cuda()
        banks = {"uniform": FkStreamBank(S, smooth=5)}
        if has_table:
            banks["table"] = FkStreamBank(S, smooth=5)
            banks["table"].set_bodies(random_bodies(rng, S))
        res = {k: [] for k in banks}
        for _ in range(REPEATS):
            for k, bank in banks.items():
                res[k].append(frame_us(lambda: bank.step_rows(rows), 20 if quick else 200, 50 if quick else 500))
        out[f"fk_{S}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "bodies_bench.json"))
    ap.add_argument("--label", default="")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    try:
        commit = subprocess.run(["git", "-C", str(REPO), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"label": a.label, "commit": commit, "device": torch.cuda.get_device_name(0), "repeats": REPEATS, "unit": "us per frame, p50 per repeat",
           "legs": legs(a.quick)}
    for leg, modes in res["legs"].items():
        for mode, v in modes.items():
            print(f"{leg:18s} {mode:8s} median {np.median(v):9.2f} us   min {min(v):9.2f}   max {max(v):9.2f}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
