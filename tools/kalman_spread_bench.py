#!/usr/bin/env python3
"""What the spread record (APE_FLAG_SPREAD) costs on the Kalman bank and what it saves, measured in one session.

    python tools/kalman_spread_bench.py [--parent-lib PATH/libape_hip.so] [--rounds 3] [--quick]

E = 48, W = 10, smooth 5 (the issue's example: 25 + 6 * 5 * 48 = 1465 packed values), synthetic weights (PARITY UNPINNED: the numbers
are about time only).  Per child process, on ONE library:

  frame        the device frame (KalmanStreamBank.step_rows, float32 rows, past the init frames) of S = 1 and S = 256 streams: HIP events
               around 200 single frames, p50 -- unflagged messages [S, 25], unflagged datagrams [S, 1465], and with this commit's
               library messages + record [S, 46] and datagrams + record [S, 1486]
  process_row  WatchPhonePocketKalman.process_row host to host, 2000 calls, p50 -- spread off, and (this library) on
  replay       one 10 000-frame recording, process_recording, seconds on the host clock behind an un-timed short call -- unflagged, and
               (this library) with spread=True
  d2h          the device-to-host copy (pinned) of one frame of 256 streams: packed cloud [S, 1465] against message + record [S, 46]

With --parent-lib (a build of the parent commit) children of the two libraries alternate, `rounds` times each, swapping who goes first,
so that both see the same machine.  Prints ONE JSON line: per library and figure the per-round values and their median."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for _p in (str(ROOT), str(ROOT / "arm-pose-estimation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

E, W, SMOOTH, S_BANK = 48, 10, 5, 256


def p50(v):
    return float(np.percentile(v, 50))


def make_rows(rng, n):
    base = np.load(ROOT / "tests" / "golden" / "stream_trace_pocket.npz")["rows"].astype(np.float32)
    rows = base[rng.integers(0, len(base), n)].copy()
    cols = list(range(10, 23)) + list(range(33, 46))
    rows[:, cols] += (0.05 * rng.normal(size=(n, len(cols)))).astype(np.float32)
    return rows


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


def child(args):
    """every figure on the library APE_HIP_LIB names (default: this tree's); flagged figures only where the library takes the flag"""
    import torch
    from oracle import kalman_oracle as ko
    from wear_mocap_ape_amd import _hip
    probe = ctypes.CDLL(str(_hip.LIB_PATH))
    for name in [n for n in _hip.SIGNATURES if not hasattr(probe, n)]:
        del _hip.SIGNATURES[name]                               # a parent build: bind what it has
    from wear_mocap_ape_amd.estimate import kalman_models
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    q = 10 if args.quick else 1
    torch.cuda.set_device(0)
    sd = ko.make_state_dict(W, 0)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    m = kalman_models.KalmanSmartwatchModel(E, W)
    m.load_state_dict(tsd)
    # does this library take the flag?  (refused before anything is read: NULL-free dummy arguments are not needed, a real bank is)
    probe_bank = KalmanStreamBank(m, 1, smooth=SMOOTH, normalize=True, dtype=torch.float32)
    try:
        probe_bank.step_rows(make_rows(np.random.default_rng(9), 1), spread=True)
        has_spread = True
    except UserWarning:
        has_spread = False
    del probe_bank
    rng = np.random.default_rng(0)
    res = {"has_spread": has_spread}
    for S in (1, S_BANK):
        rows = torch.from_numpy(make_rows(rng, S)).cuda()
        variants = [("msg", dict()), ("packed", dict(datagrams=True))]
        if has_spread:
            variants += [("msg_spread", dict(spread=True)), ("packed_spread", dict(datagrams=True, spread=True))]
        for tag, kw in variants:
            bank = KalmanStreamBank(m, S, smooth=SMOOTH, normalize=True, dtype=torch.float32)
            event_us(lambda: bank.step_rows(rows, **kw), 30 + W + 2 + SMOOTH)       # warm-up, past the init frames and the ragged stack
            res[f"frame_S{S}_us.{tag}"] = round(p50(event_us(lambda: bank.step_rows(rows, **kw), 200 // q)), 2)
            if S == S_BANK and tag in ("packed", "msg_spread"):
                out = bank.step_rows(rows, **kw)
                out = out[0] if isinstance(out, tuple) else out
                pinned = torch.empty(tuple(out.shape), dtype=out.dtype).pin_memory()
                event_us(lambda: pinned.copy_(out, non_blocking=True), 20)
                res[f"d2h_S{S}_us.{tag}"] = round(p50(event_us(lambda: pinned.copy_(out, non_blocking=True), 200 // q)), 2)
                res[f"d2h_S{S}_bytes.{tag}"] = int(out.numel() * out.element_size())
            del bank
    for tag in ["off"] + (["on"] if has_spread else []):
        est = WatchPhonePocketKalman(tsd, smooth=SMOOTH, num_ensemble=E, window_size=W)
        if tag == "on":
            est.spread = True
        rows = make_rows(rng, (200 + 2000) // q)
        for r in rows[:200 // q]:
            est.process_row(r)
        us = []
        for r in rows[200 // q:]:
            t = time.perf_counter()
            est.process_row(r)
            us.append((time.perf_counter() - t) * 1e6)
        res[f"process_row_us.{tag}"] = round(p50(us), 2)
    est = WatchPhonePocketKalman(tsd, smooth=SMOOTH, num_ensemble=E, window_size=W)
    F = 10000 // q
    rd = torch.from_numpy(make_rows(np.random.default_rng(2), F)).cuda()
    for tag, kw in [("unflagged", dict())] + ([("spread", dict(spread=True))] if has_spread else []):
        est.process_recording(rd[:64], seed=1, out_dtype=torch.float32, **kw)          # un-timed: allocations, clocks
        torch.cuda.synchronize()
        t = time.perf_counter()
        est.process_recording(rd, seed=1, out_dtype=torch.float32, **kw)
        torch.cuda.synchronize()
        res[f"replay_F{F}_s.{tag}"] = round(time.perf_counter() - t, 4)
    m.check()
    print("KALMAN_SPREAD_BENCH " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libape_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a tenth of the frames (a rehearsal)")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    import __graft_entry__ as entry
    entry.build()
    libs = [("this", None)] + ([("parent", str(Path(args.parent_lib).resolve()))] if args.parent_lib else [])
    runs = {tag: [] for tag, _ in libs}
    for rnd in range(args.rounds):
        for tag, path in (libs if rnd % 2 == 0 else libs[::-1]):          # alternate, and swap who goes first
            env = dict(os.environ)
            if path:
                env["APE_HIP_LIB"] = path
            cmd = [sys.executable, str(Path(__file__).resolve()), "--child"] + (["--quick"] if args.quick else [])
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"kalman_spread_bench: the {tag} child failed (exit {p.returncode})")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("KALMAN_SPREAD_BENCH ")][-1]
            runs[tag].append(json.loads(line[len("KALMAN_SPREAD_BENCH "):]))
    out = {"E": E, "W": W, "smooth": SMOOTH, "S": S_BANK, "rounds": args.rounds, "quick": bool(args.quick)}
    for tag, rs in runs.items():
        out[tag] = {k: {"rounds": [r[k] for r in rs], "median": statistics.median(r[k] for r in rs)} for k in rs[0] if k != "has_spread"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
