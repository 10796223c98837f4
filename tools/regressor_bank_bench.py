#!/usr/bin/env python3
"""Timing of the DropoutFF / ImuPoseLSTM frames, banks and replays against what the commit before them could do with
these models, both legs in one session and alternating, p50 of three runs each, after un-timed launches that settle the clocks:

  process_row   pocket estimator over DropoutFF and over ImuPoseLSTM, (mc, smooth) = (1, 1), (25, 1), (60, 5): the one-call device frame
                against the staged methods (use_device_frame = False), the only path these models had; host to host, p50 / p99
  ff_bank       lockstep frame (push_rows + step_datagrams), S = 1024 and 8192, 25 samples, against the composition the parent offered:
                ape_parse_rows + DropoutFF forward over the S * 25 repeated rows with Philox dropout + ape_fk (no smoothing, no
                message, the trunk 25 times)
  imupose_bank  lockstep frame, S = 1024, T = 6, against ape_parse_rows + ImuPoseLSTM forward on pre-gathered windows + ape_fk; the
                LSTM launches' share of the frame from ape_streams_profile (the rest = builder + window copy + input layer + post)
  lstm_bank     the unchanged path: pocket DropoutLSTM bank, S = 1024, mc 1 and 25, lockstep frame -- in child processes, alternating
                between this tree and `--parent-tree` (a checkout of the parent commit with its library built)
  replay        process_recording at F = 100 000 for both models: frames / s


The first three legs time "what the parent offered" -- the staged methods, parse_rows + forward + fk -- on THIS tree's library, alternating
with the new path inside one process: those calls and their kernels are the parent's, unchanged by this feature (the lstm_bank leg is the
check of that claim on a library built from the parent commit).  The report says so.

python tools/regressor_bank_bench.py [--out-dir profiles] [--quick] [--parent-tree DIR]  ->  <out-dir>/regressor_banks.{json,md}
rocprofv3 --kernel-trace --stats -d DIR -- python tools/regressor_bank_bench.py --trace-child DropoutFF|ImuPoseLSTM [--streams S]
    200 lockstep frames of that bank and nothing else, for the frame split by kernel"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from array import array
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
# (child legs on the parent commit run this file against THAT tree's package and library: APE_BENCH_TREE)
TREE = Path(os.environ.get("APE_BENCH_TREE", REPO))
sys.path[:0] = [str(TREE), str(TREE / "arm-pose-estimation_amd")]

import torch  # noqa: E402

from oracle import ape_oracle as orc  # noqa: E402

RUNS = 3
HASH = "670b66fa7664252d1cfb3b5a8a362002ffeeba5c"


def p50(v):
    return float(np.percentile(v, 50))


def event_us(fn, n):
    us = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return us


def base_rows(n, seed=0):
    base = np.load(REPO / "tests" / "golden" / "stream_trace_pocket.npz")["rows"].astype(np.float32)
    rng = np.random.default_rng(seed)
    rows = base[rng.integers(0, len(base), n)].copy()
    rows += np.float32(1e-3) * rng.standard_normal(rows.shape, dtype=np.float32)
    return rows


def deploy(tmp, model, dropout=0.2):
    """a deploy tree whose pocket results.json names `model` (DropoutLSTM | DropoutFF | ImuPoseLSTM), seeded weights"""
    import shutil
    from wear_mocap_ape_amd import config
    src = Path(deploy.shipped.setdefault("d", config.PATHS["deploy"]))
    dst = Path(tmp) / f"deploy_{model}_{len(os.listdir(tmp))}"
    shutil.copytree(src / "data_stats", dst / "data_stats")
    d = dst / "nn" / HASH
    d.mkdir(parents=True)
    p = json.loads((src / "nn" / HASH / "results.json").read_text())
    p["dropout"], p["model"] = dropout, model
    cfg = orc.MODEL_CONFIGS["pocket"]
    if model == "DropoutFF":
        p["hidden_layer_size"], p["hidden_layer_count"] = 256, 2
        sd = orc.make_ff_state_dict(cfg["I"], 256, 2, cfg["O"], 3)
    elif model == "ImuPoseLSTM":
        sd = orc.make_imupose_state_dict(cfg["I"], cfg["O"], 3)
    else:
        sd = orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], 3)
    (d / "results.json").write_text(json.dumps(p))
    torch.save(({k: torch.from_numpy(v) for k, v in sd.items()}, {"state": {}, "param_groups": []}), d / "checkpoint.pt")
    config.PATHS["deploy"] = dst
    return HASH


deploy.shipped = {}


def estimator(tmp, model, **kw):
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import WatchPhonePocketNN
    return WatchPhonePocketNN(model_hash=deploy(tmp, model), **kw)


def leg_process_row(tmp, frames, warm):
    out = {}
    wire = [array("f", r.tolist()) for r in base_rows(256)]
    for model in ("DropoutFF", "ImuPoseLSTM"):
        for mc, smooth in ((1, 1), (25, 1), (60, 5)):
            new = estimator(tmp, model, smooth=smooth, monte_carlo_samples=mc)
            old = estimator(tmp, model, smooth=smooth, monte_carlo_samples=mc)
            old.use_device_frame = False

            def run(est, n):
                us = []
                for i in range(n):
                    t0 = time.perf_counter()
                    est.process_row(wire[i % len(wire)])
                    us.append((time.perf_counter() - t0) * 1e6)
                return us
            run(old, warm), run(new, warm)
            a, b = [], []
            for _ in range(RUNS):
                a += run(old, frames)
                b += run(new, frames)
            out[f"{model}_mc{mc}_s{smooth}"] = {
                "staged_p50_us": p50(a), "staged_p99_us": float(np.percentile(a, 99)),
                "frame_p50_us": p50(b), "frame_p99_us": float(np.percentile(b, 99)), "ratio_p50": p50(a) / p50(b)}
    return out


def leg_bank(tmp, model, S, mc, frames, warm):
    """lockstep frame of the bank against parse_rows + forward + fk, alternating"""
    import ctypes as C
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    est = estimator(tmp, model, smooth=1, monte_carlo_samples=mc)
    m, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    rows = torch.from_numpy(base_rows(S, 1)).cuda()
    bank = StreamBank(m, S, T, smooth=1, normalize=True, dtype=torch.float32, monte_carlo_samples=mc)
    n_eff = bank._n_mc

    def new():
        bank.push_rows(rows, kind)
        bank.step_datagrams()

    win = torch.from_numpy(np.random.default_rng(2).normal(size=(S, T, m.input_size)).astype(np.float32)).cuda()
    est_out = torch.empty((S * n_eff, 21), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def parent():                      # what the parent commit offered for these models: three calls, no smoothing, no message
        est.parse_rows(rows)
        if model == "DropoutFF":
            m._do.train()
            y = m.forward(win[:, -1:, :].repeat((n_eff, 1, 1)), last_step_only=True, normalize_input=True)
        else:
            y = m.forward(win, last_step_only=True, normalize_input=True)
        y2 = y.reshape(-1, m.output_size)
        _hip.check(_hip.lib().ape_fk(m.handle, C.c_void_p(y2.data_ptr()), _hip.F32, int(y2.shape[0]), 1, C.c_void_p(est_out.data_ptr()),
                                     _hip.F32, st), "ape_fk")

    event_us(parent, warm), event_us(new, warm)
    a, b = [], []
    for _ in range(RUNS):
        a.append(p50(event_us(parent, frames)))
        b.append(p50(event_us(new, frames)))
    m.recover()
    bank.profile(True)
    t = p50(event_us(new, frames))
    ms, n = bank.profile_read()
    bank.profile(False)
    return {"S": S, "mc": n_eff, "parent_composition_us": a, "bank_frame_us": b, "ratio_p50": p50(a) / p50(b),
            "regressor_share": (ms * 1e3 / max(1, min(n, frames))) / t if n else None, "kernel": m.last_kernel()}


def leg_lstm_child(S, mc, frames, warm):
    """(child process) the unchanged pocket DropoutLSTM bank's lockstep frame on whatever library APE_HIP_LIB names"""
    from wear_mocap_ape_amd.streams import StreamBank
    with tempfile.TemporaryDirectory() as tmp:
        est = estimator(tmp, "DropoutLSTM", smooth=1, monte_carlo_samples=mc)
        m, kind = est._hip_model(), est._parse_kind
        rows = torch.from_numpy(base_rows(S, 1)).cuda()
        bank = StreamBank(m, S, est.sequence_len, smooth=1, normalize=True, dtype=torch.float32, monte_carlo_samples=mc, dropout=0.2)

        def new():
            bank.push_rows(rows, kind)
            bank.step_datagrams()
        event_us(new, warm)
        v = p50(event_us(new, frames))
        m.recover()
    print(json.dumps({"us": v}))


def trace_child(model, S):
    """(under rocprofv3) 220 lockstep frames of one bank and nothing else on the device: the kernel statistics are the frame split"""
    from wear_mocap_ape_amd.streams import StreamBank
    with tempfile.TemporaryDirectory() as tmp:
        est = estimator(tmp, model, smooth=1, monte_carlo_samples=25)
        m, kind = est._hip_model(), est._parse_kind
        rows = torch.from_numpy(base_rows(S, 1)).cuda()
        bank = StreamBank(m, S, est.sequence_len, smooth=1, normalize=True, dtype=torch.float32, monte_carlo_samples=25)
        for _ in range(220):
            bank.push_rows(rows, kind)
            bank.step_datagrams()
        torch.cuda.synchronize()
        m.recover()
    print(json.dumps({"model": model, "S": S, "frames": 220}))


def leg_lstm(parent_tree, frames, warm):
    out = {}
    for mc in (1, 25):
        res = {"new": [], "parent": []}
        for _ in range(RUNS):
            for tag, tree in (("parent", parent_tree), ("new", None)):
                env = dict(os.environ)
                env.pop("APE_HIP_LIB", None)
                env.pop("APE_BENCH_TREE", None)
                if tree:
                    env["APE_BENCH_TREE"] = str(Path(tree).resolve())
                r = subprocess.run([sys.executable, __file__, "--child-lstm", str(mc), "--frames", str(frames), "--warm", str(warm)],
                                   env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(r.stderr[-2000:])
                res[tag].append(json.loads(r.stdout.strip().splitlines()[-1])["us"])
        out[f"mc{mc}"] = res
    return out


def leg_replay(tmp, F):
    out = {}
    rows = torch.from_numpy(base_rows(F, 4)).cuda()
    for model in ("DropoutFF", "ImuPoseLSTM"):
        est = estimator(tmp, model, smooth=5, monte_carlo_samples=25)
        est.process_recording(rows[:4096])
        ts = []
        for _ in range(RUNS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            est.process_recording(rows, out_dtype=torch.float32)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[model] = {"F": F, "seconds": ts, "frames_per_s": F / p50(ts)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=str(REPO / "profiles"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-lstm", type=int, default=0)
    ap.add_argument("--trace-child", default=None)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--warm", type=int, default=0)
    a = ap.parse_args()
    if a.child_lstm:                 # (the tree's library as it stands: nothing is built on the way)
        return leg_lstm_child(1024, a.child_lstm, a.frames, a.warm)
    if a.trace_child:
        return trace_child(a.trace_child, a.streams)
    import __graft_entry__ as entry
    entry.build()
    frames, warm = (100, 30) if a.quick else (300, 100)
    res = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "frames": frames, "warm": warm}
    with tempfile.TemporaryDirectory() as tmp:
        res["process_row"] = leg_process_row(tmp, 300 if a.quick else 1500, 100)
        res["ff_bank"] = [leg_bank(tmp, "DropoutFF", S, 25, frames, warm) for S in (1024, 8192)]
        res["imupose_bank"] = leg_bank(tmp, "ImuPoseLSTM", 1024, 25, frames, warm)
        res["replay"] = leg_replay(tmp, 20000 if a.quick else 100000)
    res["lstm_bank"] = leg_lstm(a.parent_tree, frames, warm) if a.parent_tree else "unmeasured: no --parent-tree given"
    out = Path(a.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    (out / "regressor_banks.json").write_text(json.dumps(res, indent=1))
    md = ["# DropoutFF / ImuPoseLSTM frames, banks and replays (tools/regressor_bank_bench.py)", "",
          f"{res['device']}; p50 of {RUNS} alternated runs of {frames} frames after {warm} un-timed ones.", "",
          "The \"staged\" and \"composition\" sides are the parent commit's calls (staged estimator methods; ape_parse_rows + forward + ape_fk) "
          "run on this tree's library inside the same process: their code is unchanged from the parent. Only the last table runs a library "
          "built from the parent commit.", "",
          "## process_row, host to host (us): staged methods (the only path before) / one-call frame", "",
          "| model, mc, smooth | staged p50 | staged p99 | frame p50 | frame p99 | ratio p50 |", "|---|---|---|---|---|---|"]
    for k, v in res["process_row"].items():
        md.append(f"| {k} | {v['staged_p50_us']:.1f} | {v['staged_p99_us']:.1f} | {v['frame_p50_us']:.1f} | {v['frame_p99_us']:.1f} | {v['ratio_p50']:.2f} |")
    md += ["", "## lockstep bank frame (us) against parse_rows + forward + fk", "",
           "| bank | composition runs | frame runs | ratio p50 | regressor share of the frame |", "|---|---|---|---|---|"]
    for tag, v in [(f"DropoutFF S={x['S']} x {x['mc']}", x) for x in res["ff_bank"]] + [("ImuPoseLSTM S=1024 T=6", res["imupose_bank"])]:
        fmt = lambda r: " ".join(f"{u:.1f}" for u in r)      # noqa: E731
        share = "-" if v["regressor_share"] is None else f"{v['regressor_share']:.2f}"
        md.append(f"| {tag} | {fmt(v['parent_composition_us'])} | {fmt(v['bank_frame_us'])} | {v['ratio_p50']:.2f} | {share} |")
    md += ["", "## unchanged path: pocket DropoutLSTM bank, S = 1024 (us), parent library / this tree", ""]
    if isinstance(res["lstm_bank"], dict):
        for k, v in res["lstm_bank"].items():
            md.append(f"* {k}: parent {' '.join(f'{u:.1f}' for u in v['parent'])} -- new {' '.join(f'{u:.1f}' for u in v['new'])}")
    else:
        md.append(res["lstm_bank"])
    md += ["", "## replay", ""]
    for k, v in res["replay"].items():
        md.append(f"* {k}: F = {v['F']}, smooth 5, 25 samples: {v['frames_per_s']:.0f} frames/s")
    (out / "regressor_banks.md").write_text("\n".join(md) + "\n")
    print("\n".join(md))


if __name__ == "__main__":
    main()
