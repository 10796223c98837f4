"""What per-stream smoothing lengths (ape_*_set_smooths) cost, measured in one session.

    python tools/smooths_bench.py [--parent-tree DIR] [--rounds 3] [--frames 200] [--warmup 20] [--out profiles/smooths_bank.md]

Cases, lockstep frames (push_rows + step, float32 datagram rows):
  pocket_mc25   1024 pocket streams, 25 samples, smooth (capacity) 5
  pocket_mc1    the same at one sample
  fk            the forward-kinematics bank at 8192 streams, smooth 5 (one launch per frame)
Per case: `uniform` (no table: what the parent runs too), and with this commit's library `table_all5` (a table of all 5) and
`table_mixed` (stream s has smooth 1 + s % 5).  The regressor does not depend on smooth, so a difference is the post-filter's alone.

Every measurement runs in a fresh child process on ONE library; with --parent-tree (a checkout of the parent commit with its library
built: DIR/arm-pose-estimation_amd/lib/libape_hip.so) children of the two libraries alternate, `rounds` times each, so that both see the
same machine; the parent's own run-to-run range is the bound for `uniform` on this build.  Times are device events around `frames`
back-to-back frames (microseconds per frame).  Prints ONE JSON line and writes the profile (--out, default profiles/smooths_bank.md).  Seeded synthetic
weights, rows from the recorded traces tiled with noise."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for _p in (str(ROOT), str(ROOT / "arm-pose-estimation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

S_NN, S_FK, CAP = 1024, 8192, 5


def child(args):
    """all cases on the library APE_HIP_LIB names (default: this tree's); the table cases only where the library has the entry"""
    import torch
    from oracle import ape_oracle as orc
    from wear_mocap_ape_amd import _hip
    import ctypes
    raw = ctypes.CDLL(str(_hip.LIB_PATH))
    has_table = hasattr(raw, "ape_streams_set_smooths")
    for name in [n for n in _hip.SIGNATURES if not hasattr(raw, n)]:
        del _hip.SIGNATURES[name]                           # a parent build: bind what it has
    from wear_mocap_ape_amd.estimate import nn_models
    from wear_mocap_ape_amd.streams import FkStreamBank, StreamBank
    torch.cuda.set_device(0)
    lib, res = _hip.lib(), {}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    stats_all = json.loads((ROOT / "tests" / "golden" / "norm_stats.json").read_text())

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

    def tables(S):
        t = [("uniform", None)]
        if has_table:
            t += [("table_all5", np.full((S,), CAP, dtype=np.int32)), ("table_mixed", (1 + np.arange(S) % CAP).astype(np.int32))]
        return t

    cfg = orc.MODEL_CONFIGS["pocket"]
    m = nn_models.DropoutLSTM(cfg["I"], cfg["H"], cfg["L"], cfg["O"], dropout=0.2, device=0)
    m.load_state_dict(orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], seed=0))
    m.set_norm_stats(*(np.array(stats_all["pocket"][k]) for k in ("xx_m", "xx_s", "yy_m", "yy_s")))
    m.set_body(orc.DEFAULT_BODY)
    base = np.load(ROOT / "tests" / "golden" / "stream_trace_pocket.npz")["rows"].astype(np.float32)
    rows = np.tile(base, ((4 * S_NN + len(base) - 1) // len(base), 1))[:4 * S_NN]
    rows = rows + np.float32(1e-3) * np.random.default_rng(0).standard_normal(rows.shape, dtype=np.float32)
    rows_d = torch.from_numpy(rows).cuda()
    lock_rows = [rows_d[i * S_NN:(i + 1) * S_NN].contiguous() for i in range(4)]
    kind = _hip.PARSE_WATCH_PHONE_POCKET
    for tag, mc in (("pocket_mc25", 25), ("pocket_mc1", None)):
        width = 25 + 6 * CAP * (mc or 1)
        for vtag, table in tables(S_NN):
            bank = StreamBank(m, S_NN, cfg["T"], smooth=CAP, normalize=True, dtype=torch.float32, monte_carlo_samples=mc, dropout=0.2, seed=7)
            if table is not None:
                bank.set_smooths(table)
            out = torch.empty((S_NN, width), dtype=torch.float32, device="cuda")
            flags = _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG

            def frame(i):
                _hip.check(lib.ape_streams_push_rows(bank._handle, kind, C.c_void_p(lock_rows[i % 4].data_ptr()), stream), "push_rows")
                _hip.check(lib.ape_streams_step(bank._handle, flags, C.c_void_p(out.data_ptr()), None, _hip.F32, stream), "step")
            res[f"{tag}.frame_us.{vtag}"] = round(timed(frame, args.frames), 2)
            bank.check()
            del bank
    # the forward-kinematics bank: random unit quaternions in the rotation and calibration columns
    from wear_mocap_ape_amd.data_types import messaging
    slp = messaging.WATCH_PHONE_IMU_LOOKUP
    rng = np.random.default_rng(1)
    fk_rows = rng.normal(size=(4 * S_FK, 55)).astype(np.float32)
    for pre in ("sw_rotvec", "sw_forward", "ph_rotvec", "ph_forward"):
        q = rng.normal(size=(4 * S_FK, 4))
        fk_rows[:, [slp[f"{pre}_{c}"] for c in "wxyz"]] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    fk_d = torch.from_numpy(fk_rows).cuda()
    fk_lock = [fk_d[i * S_FK:(i + 1) * S_FK].contiguous() for i in range(4)]
    for vtag, table in tables(S_FK):
        bank = FkStreamBank(S_FK, smooth=CAP, dtype=torch.float32)
        if table is not None:
            bank.set_smooths(table)
        out = torch.empty((S_FK, 25), dtype=torch.float32, device="cuda")

        def fk_frame(i):
            _hip.check(lib.ape_fk_bank_frame(bank._handle, _hip.PARSE_WATCH_PHONE_UARM, C.c_void_p(fk_lock[i % 4].data_ptr()), None, S_FK,
                                             C.c_void_p(out.data_ptr()), _hip.F32, stream), "fk_bank_frame")
        res[f"fk.frame_us.{vtag}"] = round(timed(fk_frame, args.frames), 2)
        del bank
    print("SMOOTHS_BENCH " + json.dumps(res))


def markdown(out):
    """the profile: how it was taken, every round, and the two questions it answers"""
    lines = ["# Per-stream smoothing lengths: what the table costs (DESIGN.md 4.35)", "",
             f"`tools/smooths_bench.py`, {out['rounds']} rounds per library, {out['frames']} back-to-back lockstep frames per figure (device events, "
             "microseconds per frame), a fresh child process per library and round, the two libraries alternating in one session.",
             f"`pocket_*`: {out['S_nn']} pocket streams, capacity {out['cap']}; `fk`: {out['S_fk']} forward-kinematics streams, capacity {out['cap']}.",
             "`uniform`: no table (what the parent runs); `table_all5`: a table of all 5; `table_mixed`: stream s at 1 + s % 5.", "",
             "| case | library | rounds (us per frame) | median |", "|---|---|---|---|"]
    for lib in ("parent", "this"):
        for k, v in sorted(out.get(lib, {}).items()):
            lines.append(f"| `{k}` | {lib} | {', '.join(str(x) for x in v['rounds'])} | {v['median']} |")
    lines += ["", "## A bank without a table against the parent's own run-to-run range", ""]
    if "parent" not in out:
        lines.append("not measured (no --parent-tree)")
    else:
        for k, v in sorted(out["parent"].items()):
            lo, hi, mine = min(v["rounds"]), max(v["rounds"]), out["this"][k]
            inside = "inside" if lo <= mine["median"] <= hi else ("below" if mine["median"] < lo else "ABOVE")
            lines.append(f"- `{k}`: parent {lo} .. {hi}, this build median {mine['median']} (rounds {', '.join(str(x) for x in mine['rounds'])}): {inside}")
    lines += ["", "## The table forms against the same bank without a table (this build, medians)", ""]
    for case in ("pocket_mc25", "pocket_mc1", "fk"):
        base = out["this"].get(f"{case}.frame_us.uniform")
        for v in ("table_all5", "table_mixed"):
            t = out["this"].get(f"{case}.frame_us.{v}")
            if base and t:
                lines.append(f"- `{case}` `{v}`: {t['median']} against {base['median']} us ({t['median'] - base['median']:+.2f} us, "
                             f"{100.0 * (t['median'] / base['median'] - 1.0):+.1f} %)")
    lines += ["", "The regressor does not depend on `smooth`: the differences are the post-filter's alone.  Split form: the shipped table form "
              "lets chunks past a stream's rows arrive with zero partial sums; the alternative (the one-workgroup loop only) was priced in "
              "DESIGN.md 4.35 and not measured -- these banks are too large to hold the split form's workspaces, so neither is on their path."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "smooths_bank.md"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    import __graft_entry__ as entry
    entry.build()
    libs = [("this", None)]
    if args.parent_tree:
        plib = Path(args.parent_tree).resolve() / "arm-pose-estimation_amd" / "lib" / "libape_hip.so"
        if not plib.exists():
            raise SystemExit(f"smooths_bench: {plib} does not exist (build the parent tree first)")
        libs.append(("parent", str(plib)))
    runs = {tag: [] for tag, _ in libs}
    for rnd in range(args.rounds):
        for tag, path in (libs if rnd % 2 == 0 else libs[::-1]):          # alternate, and swap who goes first
            env = dict(os.environ)
            if path:
                env["APE_HIP_LIB"] = path
            cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--frames", str(args.frames), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"smooths_bench: the {tag} child failed (exit {p.returncode})")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("SMOOTHS_BENCH ")][-1]
            runs[tag].append(json.loads(line[len("SMOOTHS_BENCH "):]))
    out = {"S_nn": S_NN, "S_fk": S_FK, "cap": CAP, "rounds": args.rounds, "frames": args.frames}
    for tag, rs in runs.items():
        out[tag] = {k: {"rounds": [r[k] for r in rs], "median": statistics.median(r[k] for r in rs)} for k in rs[0]}
    if args.out:
        Path(args.out).write_text(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
