"""Host subset frames (``frame_host`` / ``ape_*_frame_subset_host``) against the composed route the same build offers --
``frame(host rows)`` + ``.cpu()`` + ``recover()`` -- and the capacity of one GPU host to host.  Wall-clock per call (the calls are
blocking), the two legs alternating within one process behind warm-up frames; p50 and p99 in microseconds; prints ONE JSON line.

    python tools/subset_host_bench.py [--frames 300] [--warmup 30] [--legs nn,fk,kalman,capacity] [--parent-tree DIR]

nn        pocket 2 x 256, T = 6, S = 1024, K = 1 / 64 / 512 / 1024, deterministic and 25 samples
fk        FkStreamBank S = 8192, K = 1 / 64 / 1024
kalman    KalmanStreamBank E = 48, W = 10, S = 256, K = 1 / 16 / 256
capacity  a full tick (K = S, big-endian rows in, float32 datagrams out) at S = 1024 and 8192 for pocket (mc 25), watch-only (mc 25,
          smooth 10) and upper-arm (mc 50), with the frame_stats split; which of the two sizes stays under the 20 ms of a 50 Hz stream
unchanged (with --parent-tree DIR, a checkout of the parent commit with its library built) the paths this feature must not slow down --
          device subset frame at K = 64 / 1024 of S = 1024, lockstep ape_streams_frame_host at S = 1, lockstep bank frame at S = 1024
          (pocket, deterministic) -- in child processes that alternate between that tree and this one, three runs each: the p50 of every
          run, and whether this tree's median lies within the parent's own run-to-run range

Seeded synthetic weights; rows are the recorded traces of tests/golden tiled with a little noise."""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
# (the child legs on the parent commit run this file against THAT tree's package and library: APE_BENCH_TREE)
TREE = Path(os.environ.get("APE_BENCH_TREE", ROOT))
RUNS = 3
for _p in (str(TREE), str(TREE / "arm-pose-estimation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _pcts(us):
    return {"p50": round(float(np.percentile(us, 50)), 1), "p99": round(float(np.percentile(us, 99)), 1)}


def _alternate(legs, frames, warmup):
    """legs: name -> callable(i); every frame runs each leg once, in turn; -> name -> {p50, p99} of the call's wall-clock"""
    for i in range(warmup):
        for f in legs.values():
            f(i)
    t = {k: [] for k in legs}
    for i in range(frames):
        for k, f in legs.items():
            a = time.perf_counter()
            f(i)
            t[k].append((time.perf_counter() - a) * 1e6)
    return {k: _pcts(v) for k, v in t.items()}


def _ratio(r):
    r["host_over_composed_p50"] = round(r["frame_host"]["p50"] / r["composed"]["p50"], 3)
    return r


def _lstm(name, dropout=0.2):
    from oracle import ape_oracle as orc
    from wear_mocap_ape_amd.estimate import nn_models
    cfg = orc.MODEL_CONFIGS[name]
    raw = json.loads((ROOT / "tests" / "golden" / "norm_stats.json").read_text())[name]
    model = nn_models.DropoutLSTM(cfg["I"], cfg["H"], cfg["L"], cfg["O"], dropout=dropout, device=0)
    model.load_state_dict(orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], seed=0))
    model.set_norm_stats(*(np.array(raw[k]) for k in ("xx_m", "xx_s", "yy_m", "yy_s")))
    model.set_body(orc.DEFAULT_BODY)
    return model, cfg


def _rows(name, n, seed=0):
    base = np.load(ROOT / "tests" / "golden" / f"stream_trace_{name}.npz")["rows"].astype(np.float32)
    rows = np.tile(base, ((n + len(base) - 1) // len(base), 1))[:n]
    return rows + np.float32(1e-3) * np.random.default_rng(seed).standard_normal(rows.shape, dtype=np.float32)


def leg_nn(args):
    import torch
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    S, T, kind = 1024, 6, _hip.PARSE_WATCH_PHONE_POCKET
    model, _ = _lstm("pocket")
    rows = _rows("pocket", 4 * S)
    rng = np.random.default_rng(1)
    out = {}
    for tag, mc in (("det", None), ("mc25", 25)):
        kw = dict(monte_carlo_samples=mc, dropout=0.2, seed=7) if mc else {}
        composed, host = (StreamBank(model, S, T, smooth=1, normalize=True, dtype=torch.float32, **kw) for _ in range(2))
        for K in (1, 64, 512, 1024):
            lists = [rng.permutation(S)[:K] for _ in range(4)]
            batches = [np.ascontiguousarray(rows[i * S:i * S + K]) for i in range(4)]

            def run_composed(i):
                d = composed.frame(batches[i % 4], lists[i % 4], kind, datagrams=True).cpu()
                composed.recover()
                return d

            def run_host(i):
                return host.frame_host(batches[i % 4], lists[i % 4], kind, datagrams=True)
            out[f"{tag}_K{K}"] = _ratio(_alternate({"composed": run_composed, "frame_host": run_host}, args.frames, args.warmup))
        del composed, host
    return {"S": S, "T": T, "model": "pocket 2x256", "us_per_frame": out}


def leg_fk(args):
    import torch
    from wear_mocap_ape_amd.streams import FkStreamBank
    S = 8192
    rows = _rows("pocket", 2 * S)          # (WATCH_PHONE_IMU messages: the layout the FK estimator reads too)
    composed, host = FkStreamBank(S, smooth=5, dtype=torch.float32), FkStreamBank(S, smooth=5, dtype=torch.float32)
    rng = np.random.default_rng(2)
    out = {}
    for K in (1, 64, 1024):
        lists = [rng.permutation(S)[:K] for _ in range(4)]
        batches = [np.ascontiguousarray(rows[i * K:(i + 1) * K]) for i in range(4)]
        out[f"K{K}"] = _ratio(_alternate({"composed": lambda i: composed.frame(batches[i % 4], lists[i % 4]).cpu(),
                                          "frame_host": lambda i: host.frame_host(batches[i % 4], lists[i % 4])}, args.frames, args.warmup))
    return {"S": S, "smooth": 5, "us_per_frame": out}


def leg_kalman(args):
    import torch
    from oracle import kalman_oracle as ko
    from wear_mocap_ape_amd.estimate import kalman_models
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    S, E, W = 256, 48, 10
    model = kalman_models.KalmanSmartwatchModel(E, W)
    model.load_state_dict(ko.make_state_dict(W, 0))
    rows = _rows("pocket", 4 * S)
    composed, host = (KalmanStreamBank(model, S, smooth=5, normalize=True, seed=3, dtype=torch.float32) for _ in range(2))
    rng = np.random.default_rng(3)
    out = {}
    for K in (1, 16, 256):
        lists = [rng.permutation(S)[:K] for _ in range(4)]
        batches = [np.ascontiguousarray(rows[i * S:i * S + K]) for i in range(4)]

        def run_composed(i):
            d, n = composed.frame(batches[i % 4], lists[i % 4], datagrams=True)
            return d.cpu(), n.cpu()
        out[f"K{K}"] = _ratio(_alternate({"composed": run_composed,
                                          "frame_host": lambda i: host.frame_host(batches[i % 4], lists[i % 4], datagrams=True)},
                                         max(20, args.frames // 4), max(5, args.warmup // 4)))
    composed.check()
    return {"S": S, "E": E, "W": W, "smooth": 5, "us_per_frame": out}


def leg_capacity(args):
    import torch
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    res = {}
    for name, trace, mc, smooth, kind in (("pocket", "pocket", 25, 1, _hip.PARSE_WATCH_PHONE_POCKET), ("watch", "watch", 25, 10, _hip.PARSE_WATCH_ONLY),
                                          ("uarm", "uarm", 50, 1, _hip.PARSE_WATCH_PHONE_UARM)):
        model, cfg = _lstm(name)
        for S in (1024, 8192):
            bank = StreamBank(model, S, cfg["T"], smooth=smooth, normalize=True, dtype=torch.float32, monte_carlo_samples=mc, dropout=0.2, seed=9)
            rows = np.ascontiguousarray(_rows(trace, S).byteswap())
            ids = np.arange(S)
            n = max(10, args.frames // 10)
            for _ in range(3):
                bank.frame_host(rows, ids, kind, big_endian=True, datagrams=True)
            bank.frame_stats(reset=True)
            t = []
            for _ in range(n):
                a = time.perf_counter()
                bank.frame_host(rows, ids, kind, big_endian=True, datagrams=True)
                t.append((time.perf_counter() - a) * 1e6)
            fs = bank.frame_stats()
            res[f"{name}_S{S}"] = dict(_pcts(t), launch_us=round(float(np.median(fs["launch_us"])), 1), wait_us=round(float(np.median(fs["wait_us"])), 1),
                                       copy_us=round(float(np.median(fs["copy_us"])), 1), fallback_syncs=fs["fallback_syncs"],
                                       under_20ms=bool(np.percentile(t, 99) < 20000.0))
            del bank
        del model
    return {"tick_us": res}


def child_unchanged(args):
    """(child process) the paths this feature leaves alone, on the tree APE_BENCH_TREE names: p50 wall-clock per frame, the device legs
    closed by a stream synchronisation"""
    import ctypes as C
    import torch
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    torch.cuda.set_device(0)
    lib, S, T, kind = _hip.lib(), 1024, 6, _hip.PARSE_WATCH_PHONE_POCKET
    model, _ = _lstm("pocket")
    rows = _rows("pocket", 2 * S)
    rows_d = torch.from_numpy(rows).cuda()
    rng = np.random.default_rng(5)
    sub, lock, one = (StreamBank(model, n, T, smooth=1, normalize=True, dtype=torch.float32) for n in (S, S, 1))
    legs = {}
    for K in (64, 1024):
        lists = [rng.permutation(S)[:K] for _ in range(4)]

        def run_subset(i, K=K, lists=lists):
            sub.frame(rows_d[(i % 2) * S:(i % 2) * S + K], lists[i % 4], kind, datagrams=True)
            torch.cuda.synchronize()
        legs[f"subset_frame_K{K}"] = run_subset

    def run_lockstep(i):
        lock.push_rows(rows_d[(i % 2) * S:(i % 2 + 1) * S], kind)
        lock.step_datagrams()
        torch.cuda.synchronize()
    legs["lockstep_bank_S1024"] = run_lockstep
    out1 = np.zeros((1, 25), dtype=np.float32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run_host_s1(i):
        _hip.check(lib.ape_streams_frame_host(one._handle, kind, C.c_void_p(rows[i % S:i % S + 1].ctypes.data), _hip.FLAG_NORMALIZE_INPUT,
                                              C.c_void_p(out1.ctypes.data), _hip.F32, st), "ape_streams_frame_host")
    legs["frame_host_S1"] = run_host_s1
    res = _alternate(legs, args.frames, args.warmup)
    model.recover()
    print(json.dumps({k: v["p50"] for k, v in res.items()}))


def leg_unchanged(args):
    res = {}
    for _ in range(RUNS):
        for tag, tree in (("parent", args.parent_tree), ("new", None)):
            env = dict(os.environ)
            env.pop("APE_HIP_LIB", None)
            env.pop("APE_BENCH_TREE", None)
            if tree:
                env["APE_BENCH_TREE"] = str(Path(tree).resolve())
            r = subprocess.run([sys.executable, __file__, "--child-unchanged", "--frames", str(args.frames), "--warmup", str(args.warmup)],
                               env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                res.setdefault(k, {"parent": [], "new": []})[tag].append(v)
    for v in res.values():
        v["new_median_within_parent_range"] = bool(min(v["parent"]) <= float(np.median(v["new"])) <= max(v["parent"]))
        v["new_over_parent_median"] = round(float(np.median(v["new"]) / np.median(v["parent"])), 3)
    return {"p50_us_per_run": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--legs", default="nn,fk,kalman,capacity")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-unchanged", action="store_true")
    args = ap.parse_args()
    if args.child_unchanged:         # (the tree's library as it stands: nothing is built on the way)
        return child_unchanged(args)
    import __graft_entry__ as entry
    entry.build()
    import torch
    torch.cuda.set_device(0)
    legs = {"nn": leg_nn, "fk": leg_fk, "kalman": leg_kalman, "capacity": leg_capacity}
    result = {"frames": args.frames, "warmup": args.warmup}
    for name in filter(None, args.legs.split(",")):
        result[name] = legs[name](args)
    result["unchanged"] = leg_unchanged(args) if args.parent_tree else "unmeasured: no --parent-tree given"
    print(json.dumps(result))


if __name__ == "__main__":
    main()
