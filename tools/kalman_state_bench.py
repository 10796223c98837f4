#!/usr/bin/env python3
"""The Kalman bank's state hand-over on the clock, E = 48, W = 10, smooth 1:

  a  export / import of K = 1 / 16 / 256 of 256 streams (HIP events, p50 of the three runs' p50s)
  b  the bank frame at S = 1 and S = 256 (HIP events) and process_row (host to host), this library beside the PARENT commit's library
     (--parent-lib, built from a `git worktree` of the parent): a fresh child process per run, the two libraries alternating
  c  one 10 000-frame recording replayed in 10 chained pieces (this library) against the one call (the parent's library, and this one)

python tools/kalman_state_bench.py --parent-lib PATH [--out-dir profiles] [--quick]  ->  <out-dir>/kalman_state.json, kalman_state.md
Without --parent-lib the parent legs are left out and the note says so.  PARITY UNPINNED for this estimator: synthetic weights
(oracle/kalman_oracle.py), the numbers are about time only."""
import argparse
import ctypes
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "arm-pose-estimation_amd")]

RUNS = 3
E, W, SMOOTH, S_BANK = 48, 10, 1, 256
HBM_PEAK_TBS = 8.0                   # MI355X HBM3E peak


def p50(v):
    return float(np.percentile(v, 50))


def make_rows(rng, n):
    base = np.load(REPO / "tests" / "golden" / "stream_trace_pocket.npz")["rows"].astype(np.float32)
    rows = base[rng.integers(0, len(base), n)].copy()
    cols = list(range(10, 23)) + list(range(33, 46))
    rows[:, cols] += (0.05 * rng.normal(size=(n, len(cols)))).astype(np.float32)
    return rows


def load(lib_path):
    """the package on the given library; entries the library lacks (the parent's) are not bound"""
    from wear_mocap_ape_amd import _hip
    if lib_path:
        _hip.LIB_PATH = Path(lib_path)
        probe = ctypes.CDLL(str(lib_path))
        for name in [n for n in _hip.SIGNATURES if not hasattr(probe, n)]:
            del _hip.SIGNATURES[name]
    return _hip.lib()


def event_us(fn, n):
    import torch
    us = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return us


def model_and_sd():
    import torch
    from oracle import kalman_oracle as ko
    from wear_mocap_ape_amd.estimate import kalman_models
    sd = ko.make_state_dict(W, 0)
    m = kalman_models.KalmanSmartwatchModel(E, W)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m, sd


def leg_frames(q):
    """one run: bank frame S = 1 and 256 past the init frames, process_row"""
    import torch
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    m, sd = model_and_sd()
    rng = np.random.default_rng(0)
    res = {}
    for S in (1, S_BANK):
        bank = KalmanStreamBank(m, S, smooth=SMOOTH, normalize=True)
        rows = torch.from_numpy(make_rows(rng, S)).cuda()
        event_us(lambda: bank.step_rows(rows), 30 + W + 2)
        res[f"frame_S{S}_us"] = p50(event_us(lambda: bank.step_rows(rows), 200 // q))
    est = WatchPhonePocketKalman({k: torch.from_numpy(v) for k, v in sd.items()}, smooth=SMOOTH, num_ensemble=E, window_size=W)
    rows = make_rows(rng, (200 + 2000) // q)
    for r in rows[:200 // q]:
        est.process_row(r)
    us = []
    for r in rows[200 // q:]:
        t = time.perf_counter()
        est.process_row(r)
        us.append((time.perf_counter() - t) * 1e6)
    res["process_row_us"] = p50(us)
    m.check()
    return res


def leg_replay(q, pieces):
    """one run: a 10 000-frame recording in one call, or (pieces > 1, this library only) in chained pieces"""
    import torch
    from oracle import kalman_oracle as ko
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    sd = ko.make_state_dict(W, 0)
    est = WatchPhonePocketKalman({k: torch.from_numpy(v) for k, v in sd.items()}, smooth=SMOOTH, num_ensemble=E, window_size=W)
    F = 10000 // q
    rd = torch.from_numpy(make_rows(np.random.default_rng(2), F)).cuda()
    est.process_recording(rd[:64], seed=1)                       # un-timed: allocations, clocks
    torch.cuda.synchronize()
    t = time.perf_counter()
    if pieces == 1:
        est.process_recording(rd, seed=1)
    else:
        state = age = None
        step = F // pieces
        for a in range(0, F, step):
            _, _, state, age = est.process_recording(rd[a:a + step], seed=1, state_in=state, age_in=age, return_state=True, call_base=a)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t
    est.model.check()
    return {"seconds": sec, "frames": F, "pieces": pieces}


def leg_state(q):
    """export / import of K of 256 mature streams"""
    import torch
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    m, _ = model_and_sd()
    rng = np.random.default_rng(3)
    bank = KalmanStreamBank(m, S_BANK, smooth=SMOOTH, normalize=True)
    rows = torch.from_numpy(make_rows(rng, S_BANK)).cuda()
    for _ in range(W + 3):
        bank.step_rows(rows)
    words = bank.state_desc()["words_per_stream"]
    res = {"words_per_stream": words}
    for K in (1, 16, S_BANK):
        idx = np.arange(K, dtype=np.int32)
        state, age = bank.export_state(idx)
        ex, im = [], []
        event_us(lambda: bank.export_state(idx), 20)
        event_us(lambda: bank.import_state(idx, state, age), 20)
        for _ in range(RUNS):
            ex.append(p50(event_us(lambda: bank.export_state(idx), 200 // q)))
            im.append(p50(event_us(lambda: bank.import_state(idx, state, age), 200 // q)))
        moved = 2 * K * words * 4                                   # read + written
        res[str(K)] = {"export_us": ex, "import_us": im, "export_p50_us": p50(ex), "import_p50_us": p50(im), "bytes_moved": moved,
                       "hbm_floor_us": moved / (HBM_PEAK_TBS * 1e12) * 1e6}
    m.check()
    return res


def child(leg, lib, q, pieces=1):
    cmd = [sys.executable, str(Path(__file__).resolve()), "--leg", leg, "--pieces", str(pieces)] + (["--lib", str(lib)] if lib else []) + \
          (["--quick"] if q > 1 else [])
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=str(REPO / "profiles"))
    ap.add_argument("--parent-lib", default=None, help="libape_hip.so built from the parent commit")
    ap.add_argument("--quick", action="store_true", help="a tenth of the frames (a rehearsal)")
    ap.add_argument("--frame-runs", type=int, default=RUNS, help="runs per library of leg b (fresh processes, alternating)")
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process and print its JSON")
    ap.add_argument("--lib", default=None, help="(internal) the library the leg loads")
    ap.add_argument("--pieces", type=int, default=1)
    args = ap.parse_args()
    q = 10 if args.quick else 1
    if args.leg:
        load(args.lib)
        res = {"frames": leg_frames, "state": leg_state}[args.leg](q) if args.leg != "replay" else leg_replay(q, args.pieces)
        print(json.dumps(res))
        return
    import torch
    res = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "E": E, "W": W, "smooth": SMOOTH, "parent_lib": bool(args.parent_lib)}
    try:
        res["commit"] = json.loads((REPO / "arm-pose-estimation_amd" / "lib" / "build_info.json").read_text()).get("commit", "unknown")
    except Exception:
        res["commit"] = "unknown"
    res["state"] = child("state", None, q)
    libs = [("new", None)] + ([("parent", args.parent_lib)] if args.parent_lib else [])
    res["frames"] = {name: [] for name, _ in libs}
    res["replay_one_call"] = {name: [] for name, _ in libs}
    res["replay_10_pieces"] = []
    for _ in range(args.frame_runs):                                # alternating: new, parent, new, parent, ...
        for name, lib in libs:
            res["frames"][name].append(child("frames", lib, q))
    for _ in range(RUNS):
        for name, lib in libs:
            res["replay_one_call"][name].append(child("replay", lib, q)["seconds"])
        res["replay_10_pieces"].append(child("replay", None, q, pieces=10)["seconds"])
    out = Path(args.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    (out / "kalman_state.json").write_text(json.dumps(res, indent=1) + "\n")
    st = res["state"]
    md = [f"# Kalman bank state hand-over: times ({res['device']})", "",
          f"commit `{res['commit']}`.  Written by `tools/kalman_state_bench.py`; E = {E}, W = {W}, smooth {SMOOTH}; synthetic weights "
          "(PARITY UNPINNED: the numbers are about time only).", "",
          f"## a. export / import of K of {S_BANK} mature streams ({st['words_per_stream']} words = {4 * st['words_per_stream']} bytes a record)", "",
          "HIP events around the Python call (one descriptor copy and one launch), p50 of three runs' p50s of 200 calls.  The launch floor "
          "the NN banks' export shows is 10 - 14 us (`profiles/stream_state.md`).", "",
          f"| K | export | import | bytes moved (read + written) | bytes / HBM peak ({HBM_PEAK_TBS:.0f} TB/s) |", "|---|---|---|---|---|"]
    for K in ("1", "16", str(S_BANK)):
        v = st[K]
        md.append(f"| {K} | {v['export_p50_us']:.1f} us | {v['import_p50_us']:.1f} us | {v['bytes_moved']} | {v['hbm_floor_us']:.2f} us |")
    md += ["", "## b. bank frame and process_row beside the parent commit's library", "",
           "A fresh process per run, the libraries alternating (new, parent, new, ...); every figure is one run's p50 (200 frames by HIP "
           "events, 2000 process_row calls host to host).", "", "| leg | this library: runs (range) | parent: runs (range) | p50 inside the parent's range | ranges overlap |",
           "|---|---|---|---|---|"]
    for key, label in (("frame_S1_us", "frame S = 1"), (f"frame_S{S_BANK}_us", f"frame S = {S_BANK}"), ("process_row_us", "process_row")):
        new = [r[key] for r in res["frames"]["new"]]
        cell = lambda v: ", ".join(f"{x:.1f}" for x in v) + f" us ({min(v):.1f} - {max(v):.1f})"      # noqa: E731
        if args.parent_lib:
            par = [r[key] for r in res["frames"]["parent"]]
            inside = min(par) <= p50(new) <= max(par)
            overlap = min(new) <= max(par) and min(par) <= max(new)
            md.append(f"| {label} | {cell(new)} | {cell(par)} | p50 {p50(new):.1f} (parent p50 {p50(par):.1f}): {'yes' if inside else 'NO'} | "
                      f"{'yes' if overlap else 'NO'} |")
        else:
            md.append(f"| {label} | {cell(new)} | not measured | - | - |")
    one_new, ten = res["replay_one_call"]["new"], res["replay_10_pieces"]
    md += ["", f"## c. one recording of {10000 // q} frames: 10 chained pieces against the one call", "",
           "| leg | seconds (three runs) | frames/s (p50) |", "|---|---|---|"]
    rows = [("one call, this library", one_new), ("10 pieces, this library", ten)]
    if args.parent_lib:
        rows.insert(0, ("one call, parent library", res["replay_one_call"]["parent"]))
    for label, v in rows:
        md.append(f"| {label} | {', '.join(f'{x:.3f}' for x in v)} | {10000 // q / p50(v):.0f} |")
    base = res["replay_one_call"]["parent"] if args.parent_lib else one_new
    md += ["", f"10 pieces / one call ({'parent' if args.parent_lib else 'this library'}): **{p50(ten) / p50(base):.3f}** "
           "(ten bank builds, imports and exports more)."]
    md += ["", "## Not measured", "",
           "- export / import between two GPUs or two processes (the record is a plain device buffer: the copy is the caller's)",
           "- the estimator's `get_state` / `set_state` (a blocking copy of one record to and from the host)",
           "- chunked replay of R > 1 recordings; pieces other than 10",
           "- the frame of a bank whose streams were imported (the frame kernels are the parent's, only the counters differ)"]
    if not args.parent_lib:
        md.append("- everything beside the parent commit's library (no --parent-lib was given)")
    (out / "kalman_state.md").write_text("\n".join(md) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
