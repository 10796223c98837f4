"""The output layer fitted to a wearer: 100 000 pocket frames (rounded down to 64 x 1562) in 64 recordings of equal length.
Legs, alternating within one session behind warmed shapes, timed by HIP events (the blocking replays by the host clock around them):

    features             ape_replay_features against the deterministic ape_replay of the same rows (smooth 1, one sample), and
                         ape_lstm_features against ape_lstm_forward pinned to the batch-tile kernel on the same [F, T, I] windows: the same
                         launches with and without the store of h
    fit sums             ape_fit_sums at P = 256, Q = 14 (float32 features, float64 truth, shift and scale given, skip 5) against torch
                         float64 Z'Z per recording (torch.bmm) and over all frames (one matmul) on rows that were already masked,
                         shifted and concatenated for it, that preparation timed on its own; against the float64 MFMA rate that
                         tools/ubench/mfma_f64_rate measures in the same session (--mfma-rate PATH: the built program; its last
                         "TFLOP/s" figure is taken); against the bytes it must read and the piece records it writes and reads again
    unchanged paths      with --parent-tree DIR (a checkout of the parent commit with its library built): ape_lstm_forward on the
                         batch-tile kernel and ape_replay in child processes that alternate between that tree and this one, three runs each

Writes profiles/head_fit.md's measured section and prints ONE JSON line.

    python tools/head_fit_bench.py [--frames 100000] [--repeats 10] [--mfma-rate tools/ubench/mfma_f64_rate] [--parent-tree DIR] [--out profiles/head_fit.md]

Rows are the recorded pocket trace tiled with a little noise; features and truth of the fit-sums leg are synthetic: the times do not
depend on the values."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
TREE = Path(os.environ.get("APE_BENCH_TREE", ROOT))          # (the child legs on the parent commit run against THAT tree's package and library)
for _p in (str(TREE), str(TREE / "arm-pose-estimation_amd"), str(ROOT / "tools"), str(ROOT)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

RECORDINGS, RUNS, T = 64, 3, 6
P, Q, SKIP = 256, 14, 5
MARKER, NOTES = "## Measured", "### Reading the figures"   # the section this tool writes; what follows it is written by hand and kept


def pocket_model():
    """(model, stats) of the pocket configuration with seeded weights, norm stats and body set"""
    from oracle import ape_oracle as orc
    from wear_mocap_ape_amd.estimate import nn_models
    cfg = orc.MODEL_CONFIGS["pocket"]
    raw = json.loads((ROOT / "tests" / "golden" / "norm_stats.json").read_text())["pocket"]
    st = {k: np.array(raw[k]) for k in ("xx_m", "xx_s", "yy_m", "yy_s")}
    m = nn_models.DropoutLSTM(cfg["I"], cfg["H"], cfg["L"], cfg["O"], device=0)
    m.load_state_dict(orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], seed=0))
    m.set_norm_stats(st["xx_m"], st["xx_s"], st["yy_m"], st["yy_s"])
    m.set_body(orc.DEFAULT_BODY)
    return m, st


def pocket_rows(F, seed=7):
    base = np.load(ROOT / "tests" / "golden" / "stream_trace_pocket.npz")["rows"].astype(np.float32)
    rows = np.tile(base, ((F + len(base) - 1) // len(base), 1))[:F]
    return rows + np.float32(1e-3) * np.random.default_rng(seed).standard_normal(rows.shape, dtype=np.float32)


def host_ms(f, repeats):
    """median and all of a blocking call by the host clock, the device idle in front of it"""
    import torch
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), [round(v, 3) for v in ms]


def replay_legs(model, rows, starts, with_features=True):
    """name -> blocking callable over the C ABI"""
    import torch
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    F = int(rows.shape[0])
    rd = torch.from_numpy(rows).cuda()
    st = np.ascontiguousarray(starts, dtype=np.int32)
    out = torch.empty((F, 25), dtype=torch.float64, device="cuda")
    y = torch.empty((F, model.output_size), dtype=torch.float32, device="cuda")
    h = torch.empty((F, model.hidden_layer_size), dtype=torch.float32, device="cuda")
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    keep = (rd, st, out, y, h)

    def replay():
        _hip.check(lib.ape_replay(model.handle, _hip.PARSE_WATCH_PHONE_POCKET, C.c_void_p(rd.data_ptr()), F, C.c_void_p(st.ctypes.data), len(st), T, 1, 1,
                                  0.0, 7, _hip.FLAG_NORMALIZE_INPUT, C.c_void_p(out.data_ptr()), _hip.F64, C.c_void_p(y.data_ptr()), 0, stream()),
                   "ape_replay")
        return keep

    legs = {"replay": replay}
    if with_features:
        def features():
            _hip.check(lib.ape_replay_features(model.handle, _hip.PARSE_WATCH_PHONE_POCKET, C.c_void_p(rd.data_ptr()), F, C.c_void_p(st.ctypes.data),
                                               len(st), T, _hip.FLAG_NORMALIZE_INPUT, C.c_void_p(h.data_ptr()), C.c_void_p(y.data_ptr()), 0, stream()),
                       "ape_replay_features")
            return keep
        legs["replay_features"] = features
    return legs


def child_unchanged(args):
    """ape_lstm_forward on the batch-tile kernel and ape_replay of whichever tree APE_BENCH_TREE names: medians in ms"""
    import torch
    from score_lags_bench import alternate
    torch.cuda.set_device(0)
    model, st = pocket_model()
    F = args.frames // RECORDINGS * RECORDINGS
    rng = np.random.default_rng(3)
    x = torch.from_numpy((st["xx_m"] + st["xx_s"] * rng.standard_normal((F, T, model.input_size))).astype(np.float32)).cuda()
    model.set_kernel("tile16")
    fwd = alternate({"forward_tile16": lambda: model(x, last_step_only=True, normalize_input=True)}, args.repeats)
    model.recover()
    model.set_kernel("auto")
    rows = pocket_rows(F)
    starts = [r * F // RECORDINGS for r in range(RECORDINGS)]
    legs = replay_legs(model, rows, starts, with_features=False)
    legs["replay"]()
    rep = host_ms(legs["replay"], max(3, args.repeats // 2))
    print(json.dumps({"forward_tile16": round(fwd["forward_tile16"][0], 4), "replay": round(rep[0], 4)}))


def leg_unchanged(args):
    res = {"parent": [], "new": []}
    for _ in range(RUNS):
        for tag, tree in (("parent", args.parent_tree), ("new", None)):
            env = dict(os.environ)
            env.pop("APE_HIP_LIB", None)
            env.pop("APE_BENCH_TREE", None)
            if tree:
                env["APE_BENCH_TREE"] = str(Path(tree).resolve())
            r = subprocess.run([sys.executable, __file__, "--child-unchanged", "--frames", str(args.frames), "--repeats", str(args.repeats)],
                               env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            res[tag].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {}
    for k in ("forward_tile16", "replay"):
        p, n = [d[k] for d in res["parent"]], [d[k] for d in res["new"]]
        out[k] = {"parent_ms": p, "new_ms": n, "new_median_over_parent_median": round(float(np.median(n) / np.median(p)), 4)}
    return out


def mfma_rate(path):
    """the last TFLOP/s figure the microbenchmark prints, and its output"""
    if not path:
        return None, "not measured: no --mfma-rate program given"
    r = subprocess.run([str(path)], capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        return None, f"not measured: {path} ended with {r.returncode}"
    found = re.findall(r"([0-9.]+)\s*TFLOP/s", r.stdout)
    return (max(float(v) for v in found) if found else None), r.stdout.strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--mfma-rate", default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "head_fit.md"))
    ap.add_argument("--child-unchanged", action="store_true")
    args = ap.parse_args()
    if args.child_unchanged:
        return child_unchanged(args)

    import torch
    from score_lags_bench import alternate
    from wear_mocap_ape_amd import _hip, score
    if not torch.cuda.is_available():
        raise SystemExit("head_fit_bench needs a GPU: there is no CPU fallback and no time to report without one")
    torch.cuda.set_device(0)
    F = args.frames // RECORDINGS * RECORDINGS
    starts = [r * F // RECORDINGS for r in range(RECORDINGS)]
    res = {"frames": F, "recordings": RECORDINGS, "device": torch.cuda.get_device_name(0)}

    # ---- features -------------------------------------------------------------------------------------------------------------------
    model, st = pocket_model()
    legs = replay_legs(model, pocket_rows(F), starts)
    for f in legs.values():
        f()
    res["replay_ms"], res["replay_features_ms"] = host_ms(legs["replay"], args.repeats), host_ms(legs["replay_features"], args.repeats)
    rng = np.random.default_rng(3)
    x = torch.from_numpy((st["xx_m"] + st["xx_s"] * rng.standard_normal((F, T, model.input_size))).astype(np.float32)).cuda()
    model.set_kernel("tile16")
    both = alternate({"forward_tile16": lambda: model(x, last_step_only=True, normalize_input=True),
                      "features": lambda: model.features(x, normalize_input=True)}, args.repeats)
    model.recover()
    model.set_kernel("auto")
    res["forward_tile16_ms"], res["lstm_features_ms"] = both["forward_tile16"], both["features"]
    res["h_store_bytes"] = F * model.hidden_layer_size * 4

    # ---- fit sums ---------------------------------------------------------------------------------------------------------------------
    hx = torch.from_numpy(np.tanh(rng.standard_normal((F, P))).astype(np.float32)).cuda()
    tt = torch.from_numpy(rng.standard_normal((F, Q)) * st["yy_s"] + st["yy_m"]).cuda()
    M = P + 1 + Q
    n_rec = F // RECORDINGS

    def prepare():
        z = torch.cat([hx.double(), torch.ones((F, 1), dtype=torch.float64, device="cuda"),
                       (tt - torch.from_numpy(st["yy_m"]).cuda()) / torch.from_numpy(st["yy_s"]).cuda()], dim=1)
        ok = torch.isfinite(z).all(dim=1)
        ok.view(RECORDINGS, n_rec)[:, :SKIP] = False
        return z * ok[:, None]

    Z = prepare()
    Z3 = Z.view(RECORDINGS, n_rec, M)
    fit = alternate({"fit_sums": lambda: score.fit_sums(hx, tt, starts, SKIP, None, st["yy_m"], st["yy_s"]),
                     "torch_bmm": lambda: torch.bmm(Z3.transpose(1, 2), Z3),
                     "torch_one_matmul": lambda: Z.T @ Z,
                     "torch_prepare": prepare}, args.repeats)
    res["fit"] = {k: {"median_ms": round(v[0], 4), "all_ms": v[1]} for k, v in fit.items()}
    got = score.fit_sums(hx, tt, starts, SKIP, None, st["yy_m"], st["yy_s"])[:, :M * M].view(RECORDINGS, M, M)
    ref = torch.bmm(Z3.transpose(1, 2), Z3)
    res["fit"]["max_abs_diff_to_torch"] = float((got - ref).abs().max())
    # what the kernel does and must move
    NT = (M + 15) // 16
    tiles, pieces = NT * (NT + 1) // 2, RECORDINGS * ((n_rec - SKIP + score.FIT_PIECE - 1) // score.FIT_PIECE)
    subtiles = RECORDINGS * sum((min(score.FIT_PIECE, n_rec - SKIP - p0) + 15) // 16 for p0 in range(0, n_rec - SKIP, score.FIT_PIECE))
    row_blocks = ((NT + 1) // 2 + 3) // 4
    res["fit"]["work"] = {
        "useful_flop": 2.0 * (F - RECORDINGS * SKIP) * M * M,
        "mfma_flop": float(subtiles) * 4 * tiles * 2048,            # every computed tile, padding columns and frames of a last sub-tile included
        "input_bytes": F * (P * 4 + Q * 8), "input_bytes_as_staged": F * (P * 4 + Q * 8) * row_blocks,
        "piece_record_bytes_written_and_read": 2 * pieces * tiles * 2048, "output_bytes": RECORDINGS * (M * M + 2) * 8,
        "pieces": pieces, "row_blocks": row_blocks, "tiles": tiles}
    rate, rate_out = mfma_rate(args.mfma_rate)
    res["mfma_f64_tflops"], res["mfma_f64_output"] = rate, rate_out

    # ---- unchanged paths ------------------------------------------------------------------------------------------------------------
    res["unchanged"] = leg_unchanged(args) if args.parent_tree else "not measured: no --parent-tree given"

    # ---- the record -------------------------------------------------------------------------------------------------------------------
    w, ms = res["fit"]["work"], res["fit"]["fit_sums"]["median_ms"]
    lines = [MARKER, "", f"`tools/head_fit_bench.py --frames {args.frames} --repeats {args.repeats}` on {res['device']}; {F} frames in {RECORDINGS} recordings of {n_rec}.", "",
             "| leg | median ms | all |", "|---|---|---|",
             f"| `ape_replay` (deterministic, smooth 1; host clock) | {res['replay_ms'][0]:.3f} | {res['replay_ms'][1]} |",
             f"| `ape_replay_features` (host clock) | {res['replay_features_ms'][0]:.3f} | {res['replay_features_ms'][1]} |",
             f"| `ape_lstm_forward` on `ape_lstm_tile16`, B = {F}, T = {T} | {res['forward_tile16_ms'][0]:.4f} | {res['forward_tile16_ms'][1]} |",
             f"| `ape_lstm_features`, the same launch with the store of h ({res['h_store_bytes'] / 1e6:.1f} MB) | {res['lstm_features_ms'][0]:.4f} | {res['lstm_features_ms'][1]} |"]
    for k in ("fit_sums", "torch_bmm", "torch_one_matmul", "torch_prepare"):
        lines.append(f"| {k} (P = {P}, Q = {Q}) | {res['fit'][k]['median_ms']:.4f} | {res['fit'][k]['all_ms']} |")
    lines += ["", f"`ape_fit_sums`: {w['useful_flop'] / 1e9:.2f} GFLOP asked for (2 n M^2), {w['mfma_flop'] / 1e9:.2f} GFLOP issued on the matrix cores "
              f"({w['tiles']} tiles of {NT} x {NT}, {w['pieces']} pieces, {w['row_blocks']} row blocks): {w['mfma_flop'] / ms / 1e9:.2f} TFLOP/s issued, "
              f"{w['useful_flop'] / ms / 1e9:.2f} TFLOP/s useful over the call's {ms:.4f} ms (two launches and the staging copy).",
              f"Float64 MFMA rate of the device in this session: {rate if rate is not None else rate_out} TFLOP/s"
              + (f"; the issued work alone needs {w['mfma_flop'] / rate / 1e9:.4f} ms at that rate." if rate else "."),
              f"Bytes: {w['input_bytes'] / 1e6:.1f} MB of input ({w['input_bytes_as_staged'] / 1e6:.1f} MB as staged by {w['row_blocks']} row blocks), "
              f"{w['piece_record_bytes_written_and_read'] / 1e6:.1f} MB of piece records written and read, {w['output_bytes'] / 1e6:.2f} MB out: "
              f"{(w['input_bytes'] + w['piece_record_bytes_written_and_read'] + w['output_bytes']) / ms / 1e6:.1f} GB/s over the call.",
              f"Largest |difference| to torch's per-recording Z'Z: {res['fit']['max_abs_diff_to_torch']:.3e}.", ""]
    if isinstance(res["unchanged"], dict):
        lines += ["| unchanged path | parent ms (3 runs) | this tree ms (3 runs) | medians, new / parent |", "|---|---|---|---|"]
        for k, v in res["unchanged"].items():
            lines.append(f"| {k} | {v['parent_ms']} | {v['new_ms']} | {v['new_median_over_parent_median']} |")
    else:
        lines.append(f"Unchanged paths: {res['unchanged']}")
    lines.append("")
    out = Path(args.out)
    old = out.read_text() if out.exists() else ""
    head = old[:old.index(MARKER)] if MARKER in old else old
    tail = old[old.index(NOTES):] if NOTES in old else ""
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(head + "\n".join(lines) + "\n" + tail)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
