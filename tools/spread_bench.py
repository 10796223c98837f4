"""What the spread record (APE_FLAG_SPREAD) costs and what it saves, measured in one session.

    python tools/spread_bench.py [--parent-lib PATH/libape_hip.so] [--rounds 3] [--frames 200] [--warmup 20] [--replay-frames 100000]

Cases: lockstep frames (push_rows + step, float32 datagram rows) of S = 1024 streams, pocket model at 25 samples x smooth 1 and
watch-only model at 25 samples x smooth 10; the offline replay of F frames x 25 samples (pocket, smooth 1).  Per case: the
unflagged call, and with this commit's library the flagged ones (PACKED_MSG | SPREAD, and SPREAD alone = [S, 25 + 21] rows).  For
the lockstep cases also the device-to-host copy (pinned) of the packed rows against the [S, 25 + 21] rows: bytes and time.

Every measurement runs in a fresh child process on ONE library; with --parent-lib (a build of the parent commit) children of the two
libraries alternate, `rounds` times each, so that both see the same machine.  Times are device events around `frames` back-to-back
frames (microseconds per frame).  The replay is a blocking call: milliseconds per call on the host clock, per child the median of five
calls behind one warm-up call.  Prints ONE JSON line: per
library and case the per-round figures and their median.  Seeded synthetic weights, rows from the recorded traces tiled with noise."""
import argparse
import ctypes as C
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

S = 1024
CASES = (("pocket_mc25_s1", "pocket", 25, 1), ("watch_mc25_s10", "watch", 25, 10))


def child(args):
    """all cases on the library APE_HIP_LIB names (default: this tree's); flagged cases only where the library has the entry"""
    import torch
    from oracle import ape_oracle as orc
    from wear_mocap_ape_amd import _hip
    import ctypes
    raw = ctypes.CDLL(str(_hip.LIB_PATH))
    has_spread = hasattr(raw, "ape_spread_reduce")
    for name in [n for n in _hip.SIGNATURES if not hasattr(raw, n)]:
        del _hip.SIGNATURES[name]                           # a parent build: bind what it has
    from wear_mocap_ape_amd.estimate import nn_models
    from wear_mocap_ape_amd.streams import StreamBank
    torch.cuda.set_device(0)
    lib, res = _hip.lib(), {}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    stats_all = json.loads((ROOT / "tests" / "golden" / "norm_stats.json").read_text())

    def model_of(name):
        cfg = orc.MODEL_CONFIGS[name]
        m = nn_models.DropoutLSTM(cfg["I"], cfg["H"], cfg["L"], cfg["O"], dropout=0.2, device=0)
        m.load_state_dict(orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], seed=0))
        m.set_norm_stats(*(np.array(stats_all[name][k]) for k in ("xx_m", "xx_s", "yy_m", "yy_s")))
        m.set_body(orc.DEFAULT_BODY)
        return m, cfg

    def rows_of(name, n):
        base = np.load(ROOT / "tests" / "golden" / f"stream_trace_{name}.npz")["rows"].astype(np.float32)
        rows = np.tile(base, ((n + len(base) - 1) // len(base), 1))[:n]
        return rows + np.float32(1e-3) * np.random.default_rng(0).standard_normal(rows.shape, dtype=np.float32)

    def timed(run, n):
        for i in range(args.warmup):
            run(i)
        torch.cuda.synchronize()
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(n):
            run(i)
        z.record()
        z.synchronize()
        return a.elapsed_time(z) * 1e3 / n

    for tag, name, mc, smooth in CASES:
        m, cfg = model_of(name)
        kind = _hip.PARSE_WATCH_PHONE_POCKET if name == "pocket" else _hip.PARSE_WATCH_ONLY
        N = mc * smooth
        rows_d = torch.from_numpy(rows_of(name, 4 * S)).cuda()
        lock_rows = [rows_d[i * S:(i + 1) * S].contiguous() for i in range(4)]
        bank = StreamBank(m, S, cfg["T"], smooth=smooth, normalize=True, dtype=torch.float32, monte_carlo_samples=mc, dropout=0.2, seed=7)
        variants = [("unflagged_packed", _hip.FLAG_PACKED_MSG, 25 + 6 * N)]
        if has_spread:
            variants += [("spread_packed", _hip.FLAG_PACKED_MSG | _hip.FLAG_SPREAD, 25 + 6 * N + 21), ("spread_rows", _hip.FLAG_SPREAD, 46)]
        for vtag, vflags, width in variants:
            out = torch.empty((S, width), dtype=torch.float32, device="cuda")
            flags = _hip.FLAG_NORMALIZE_INPUT | vflags

            def frame(i):
                _hip.check(lib.ape_streams_push_rows(bank._handle, kind, C.c_void_p(lock_rows[i % 4].data_ptr()), stream), "push_rows")
                _hip.check(lib.ape_streams_step(bank._handle, flags, C.c_void_p(out.data_ptr()), None, _hip.F32, stream), "step")
            res[f"{tag}.frame_us.{vtag}"] = round(timed(frame, args.frames), 2)
            bank.check()
            host = torch.empty((S, width), dtype=torch.float32).pin_memory()
            res[f"{tag}.d2h_us.{vtag}"] = round(timed(lambda i: host.copy_(out, non_blocking=True), args.frames), 2)
            res[f"{tag}.d2h_bytes.{vtag}"] = S * width * 4
        del bank
    # the offline replay: F frames x 25 samples, pocket, smooth 1, float32 rows
    m, cfg = model_of("pocket")
    F, mc = args.replay_frames, 25
    rd = torch.from_numpy(rows_of("pocket", F)).cuda()
    st = np.zeros(1, dtype=np.int32)
    variants = [("unflagged_packed", _hip.FLAG_PACKED_MSG, 25 + 6 * mc)]
    if has_spread:
        variants += [("spread_packed", _hip.FLAG_PACKED_MSG | _hip.FLAG_SPREAD, 25 + 6 * mc + 21), ("spread_rows", _hip.FLAG_SPREAD, 46)]
    for vtag, vflags, width in variants:
        out = torch.empty((F, width), dtype=torch.float32, device="cuda")
        ts = []
        for rep in range(6):                                # the first call warms up; the median of the other five counts
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _hip.check(lib.ape_replay(m.handle, _hip.PARSE_WATCH_PHONE_POCKET, C.c_void_p(rd.data_ptr()), F, C.c_void_p(st.ctypes.data), 1,
                                      cfg["T"], 1, mc, 0.2, 5, _hip.FLAG_NORMALIZE_INPUT | vflags, C.c_void_p(out.data_ptr()), _hip.F32, None, 0,
                                      stream), "ape_replay")
            ts.append((time.perf_counter() - t0) * 1e3)
        res[f"replay_F{F}_mc25.call_ms.{vtag}"] = round(statistics.median(ts[1:]), 3)
    print("SPREAD_BENCH " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--replay-frames", type=int, default=100000)
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
            cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--frames", str(args.frames), "--warmup", str(args.warmup),
                   "--replay-frames", str(args.replay_frames)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"spread_bench: the {tag} child failed (exit {p.returncode})")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("SPREAD_BENCH ")][-1]
            runs[tag].append(json.loads(line[len("SPREAD_BENCH "):]))
    out = {"S": S, "rounds": args.rounds, "frames": args.frames}
    for tag, rs in runs.items():
        out[tag] = {k: {"rounds": [r[k] for r in rs], "median": statistics.median(r[k] for r in rs)} for k in rs[0]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
