"""Speed-adaptive smoothing (score.select_rungs / score.post_select): 100 000 pocket frames in 10 recordings at 25
Monte-Carlo samples, the ladder of 11 centred Hann windows (half-widths 0 .. 31).  Legs, alternating within one session behind warmed
shapes, timed by HIP events; the yardstick of every leg is the composed route it replaces, in the same session:

    ladder + gather 1   post_window of all 11 rungs, then the gather of one selector row from its [11, F, 25] result
    select 1            post_select with that selector row (S = 1)
    ladder + gather 4   post_window of all 11 rungs, then the gather of four selector rows
    select 4            post_select with the four rows (S = 4)
    pilot 1             post_window of the pilot rung alone (what the adaptive chain pays in front of the selector)
    bucketize           torch.bucketize of the hand-speed column over the edges: the binning alone
    select_rungs        ape_select_rungs at slope 0 (the binning alone), 2 (the default envelope) and 8 (the widest halo)
    smooth_adaptive     the whole Estimator.smooth_adaptive, against its own replay (process_recording(return_targets=True))

Messages only (no spread records) on both routes.  The selector comes from the pilot rung's hand speed at the default rule, so the
rungs' shares are those of the replayed rows; the file records them.  Writes profiles/post_select.md's measured section and prints ONE
JSON line.

    python tools/post_select_bench.py [--frames 100000] [--repeats 5] [--out profiles/post_select.md]

The unchanged paths (post_sweep, post_window) are measured against a build of the parent commit by tools/post_window_bench.py
--parent-tree.  The model carries seeded synthetic weights and the rows are synthetic: the times do not depend on the values."""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for _p in (str(ROOT), str(ROOT / "arm-pose-estimation_amd"), str(ROOT / "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from post_sweep_bench import estimator, rows_for, timed  # noqa: E402

SAMPLES, PILOT = 25, 3
MARKER, NOTES = "## Measured", "### Reading the figures"       # the section this tool writes; what follows it is written by hand and kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "post_select.md"))
    a = ap.parse_args()
    import torch
    from wear_mocap_ape_amd import score
    F, rng = a.frames, np.random.default_rng(0)
    starts = [r * (F // 10) for r in range(10)]
    ladder = score.ladder(samples=SAMPLES)
    L = len(ladder[1])
    edges = score.speed_edges(count=L - 1)
    res = {"frames": F, "recordings": 10, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        est = estimator(tmp, 10, SAMPLES)
        rows = torch.as_tensor(rows_for(F, rng)).cuda()
        _, y = est.process_recording(rows, starts=starts, return_targets=True, _config=(1, SAMPLES))
        pilot = est.repost_windows(y, [ladder[0][PILOT]], starts=starts)[0]
        speed = score.motion_sums(est._layout, pilot, "msg", starts, per_frame=True)[0][:, 0]
        sel1 = score.select_rungs(speed, edges, ladder, 2, starts=starts)
        sel4 = torch.stack([score.select_rungs(speed, edges, ladder, k, starts=starts) for k in (1, 2, 3, 4)])
        res["rung_shares_slope2"] = [round(float(x), 4) for x in torch.bincount(sel1.long(), minlength=L).double().div(F).tolist()]
        frames = torch.arange(F, device=y.device)
        idx1, idx4 = sel1.long(), sel4.long()
        edges_d = torch.as_tensor(edges, device=y.device)

        def composed(idx):
            out = est.repost_windows(y, ladder[0], starts=starts)
            return out[idx, frames]

        legs = [("ladder_gather1", lambda: composed(idx1), score.post_window_last),
                ("select1", lambda: est.repost_selected(y, ladder, sel1, starts=starts), score.post_select_last),
                ("ladder_gather4", lambda: composed(idx4), score.post_window_last),
                ("select4", lambda: est.repost_selected(y, ladder, sel4, starts=starts), score.post_select_last),
                ("pilot1", lambda: est.repost_windows(y, [ladder[0][PILOT]], starts=starts), score.post_window_last),
                ("bucketize", lambda: torch.bucketize(speed, edges_d), None),
                ("rungs_slope0", lambda: score.select_rungs(speed, edges, ladder, 0, starts=starts), None),
                ("rungs_slope2", lambda: score.select_rungs(speed, edges, ladder, 2, starts=starts), None),
                ("rungs_slope8", lambda: score.select_rungs(speed, edges, ladder, 8, starts=starts), None),
                ("replay", lambda: est.process_recording(rows, starts=starts, return_targets=True, _config=(1, SAMPLES)), None),
                ("smooth_adaptive", lambda: est.smooth_adaptive(rows, ladder, PILOT, edges, 2, starts=starts), None)]
        for name, f, last in legs:
            res[name + "_ms"], res[name + "_all"] = timed(f, a.repeats)
            res[name + "_plan"] = last() if last is not None else None
        # the bits: the selected rows against the gather of the ladder's
        res["bits_equal"] = bool(torch.equal(est.repost_selected(y, ladder, sel4, starts=starts).view(torch.int64), composed(idx4).contiguous().view(torch.int64)))
    what = {"ladder_gather1": "`post_window` of the 11 rungs + the gather of one selector row", "select1": "`post_select`, S = 1",
            "ladder_gather4": "`post_window` of the 11 rungs + the gather of four selector rows", "select4": "`post_select`, S = 4",
            "pilot1": "`post_window` of the pilot rung alone", "bucketize": "`torch.bucketize` of the speed column: the binning alone",
            "rungs_slope0": "`select_rungs`, slope 0: the binning alone", "rungs_slope2": "`select_rungs`, slope 2 (halo 62 frames)",
            "rungs_slope8": "`select_rungs`, slope 8 (halo 248 frames)", "replay": "`process_recording(return_targets=True)` at 25 samples",
            "smooth_adaptive": "`Estimator.smooth_adaptive`, replay included"}
    lines = [MARKER, "", f"`tools/post_select_bench.py --frames {F} --repeats {a.repeats}` on one {res['device']}, one session; medians, HIP events.", "",
             "| leg | ms | all runs |", "|---|---|---|"]
    lines += [f"| {what[k]}{'' if res[k + '_plan'] is None else ' (' + str(res[k + '_plan']) + ')'} | {res[k + '_ms']:.3f} | {res[k + '_all']} |" for k in what]
    lines += ["", f"`post_select` over the composed route: S = 1 {res['select1_ms'] / res['ladder_gather1_ms']:.3f}, "
                  f"S = 4 {res['select4_ms'] / res['ladder_gather4_ms']:.3f} of its time.  `smooth_adaptive` less its replay: "
                  f"{res['smooth_adaptive_ms'] - res['replay_ms']:.3f} ms.",
              f"The selected rows against the gather of the ladder's: bits equal = {res['bits_equal']}.  "
              f"Shares of the rungs under the default rule (slope 2): {res['rung_shares_slope2']}.", ""]
    out = Path(a.out)
    old = out.read_text() if out.exists() else "# Speed-adaptive smoothing (DESIGN.md 4.44)\n\n"
    head = old[:old.index(MARKER)] if MARKER in old else old
    tail = old[old.index(NOTES):] if NOTES in old else ""
    out.write_text(head + "\n".join(lines) + "\n" + tail)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
