#!/usr/bin/env python3
"""Generate tests/golden/fk_only_trace.npz by running the REFERENCE ``WatchPhoneUarm`` (estimate/watch_phone_uarm.py:10-108),
the estimator without a regressor: features -> the two calibrated 6D columns -> smoothing stack -> FK -> message.

Run in the build container only (the reference does not exist on the GPU box):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python /path/to/repo/tests/golden/gen_fk_only.py

Importing gen_golden registers its ``aenum`` stand-in and puts the reference on sys.path; its ``synth_rows`` and
``edge_forward_quats`` build the rows.  The frames are driven the way gen_stream_traces drives the NN estimators: ``array('f')``
rows through ``parse_row_to_xx -> add_xx_to_row_hist_and_make_prediction -> msg_from_pred``.  Writes data only."""
import sys
import warnings
from array import array
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_golden as gg  # noqa: E402

SMOOTHS = (1, 2, 5, 10)
LENGTHS = (40, 1, 25)


class _BoneMapStandIn:
    """the three attributes Estimator.__init__ reads from a BoneMap (estimator.py:55-63)"""
    left_lower_arm_length = 0.2473
    left_upper_arm_length = 0.3115
    left_upper_arm_origin_rh = np.array([-0.1822, 0.4417, 0.0108])


def run(est, rows, with_msgs=True):
    """one estimator over one recording: per frame xx, the stacked pred, the message (or the exception's name)"""
    xs, preds, msgs, errs = [], [], [], []
    for row32 in rows:
        row = array("f", row32.tolist())
        with np.errstate(all="ignore"):
            xx = est.parse_row_to_xx(row)
            xs.append(np.asarray(xx, dtype=np.float64))
            if not with_msgs:
                continue
            pred = est.add_xx_to_row_hist_and_make_prediction(xx)
            preds.append(np.asarray(pred, dtype=np.float64))
            try:
                msgs.append(np.asarray(est.msg_from_pred(pred, False), dtype=np.float64))
                errs.append("")
            except Exception as e:        # recorded, not hidden
                msgs.append(np.full(25, np.nan))
                errs.append(type(e).__name__)
    return xs, preds, msgs, errs


def main():
    from wear_mocap_ape.data_types import messaging
    from wear_mocap_ape.estimate.watch_phone_uarm import WatchPhoneUarm
    lookup = messaging.WATCH_PHONE_IMU_LOOKUP
    width = len(lookup)
    rng = np.random.default_rng(57)
    recs = [gg.synth_rows(rng, n, width, lookup) for n in LENGTHS]

    # the azimuth sweep of gen_feature_edges (uarm rows), the all-zero calibration included
    rng_e = np.random.default_rng(33)
    fwd = gg.edge_forward_quats(rng_e)
    edge = gg.synth_rows(rng_e, len(fwd), width, lookup)
    edge[:, [lookup[f"sw_forward_{c}"] for c in "wxyz"]] = fwd.astype(np.float32)
    ph = fwd[rng_e.permutation(len(fwd))].astype(np.float32)
    edge[:, [lookup[f"ph_forward_{c}"] for c in "wxyz"]] = ph
    edge[:3, [lookup[f"ph_rotvec_{c}"] for c in "wxyz"]] = ph[:3]

    # features of every edge row, and what the reference's message does with each row on its own (smooth 1, fresh estimator)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one = WatchPhoneUarm(smooth=1)
    edge_xx, edge_err = [], []
    for row32 in edge:
        one.reset()
        x, _, _, e = run(one, row32[None])
        edge_xx += x; edge_err += e
    edge_ok = np.array([not e for e in edge_err])

    blob = {"lengths": np.array(LENGTHS, dtype=np.int32), "rows": np.concatenate(recs), "smooths": np.array(SMOOTHS, dtype=np.int32),
            "edge_rows": edge, "edge_xx": np.array(edge_xx), "edge_err": np.array(edge_err), "edge_ok": edge_ok}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        probe = WatchPhoneUarm()
    blob["body"] = probe.body_measurements
    blob["sequence_len"] = np.array(probe.sequence_len)
    blob["x_inputs"] = np.array(str(probe.x_inputs.name))
    blob["y_targets"] = np.array(str(probe.y_targets.name))

    for smooth in SMOOTHS:
        est = WatchPhoneUarm(smooth=smooth)
        xs, preds, msgs, last = [], [], [], []
        for r in recs:                       # every recording from a cold start (reset between them)
            est.reset()
            x, p, m, e = run(est, r)
            assert not any(e), e
            xs += x; preds += p; msgs += m
            last.append(np.asarray(est.get_last_msg(), dtype=np.float64))
        blob[f"xx_s{smooth}"] = np.array(xs)
        # the stack is [smooth, 12] for smooth > 1, [1, 12] for smooth == 1
        blob[f"pred_s{smooth}"] = np.array(preds)
        blob[f"msg_s{smooth}"] = np.array(msgs)
        blob[f"last_msg_s{smooth}"] = np.array(last)
        blob[f"msg_type_s{smooth}"] = np.array(type(est.msg_from_pred(preds[-1], False)).__name__)

        # the edge sweep: the reference's eigh raises LinAlgError on the NaN stack of an all-zero calibration instead of returning NaN
        # (recorded once, below); such rows stay in the feature fixture and out of the message trace
        est.reset()
        x, _, m, _ = run(est, edge[edge_ok])
        blob[f"edge_msg_s{smooth}"] = np.array(m)

    # calibrate_orientation_quats on a few rows (the public method subclasses call)
    sl = lookup
    cal_rows = np.concatenate([recs[0][:4], edge[[0, 3, 20, len(edge) - 1]]])
    cal_sw, cal_ph = [], []
    for row in cal_rows:
        q = lambda pre: np.array([row[sl[f"{pre}_{c}"]] for c in "wxyz"])
        with np.errstate(all="ignore"):
            a, b = probe.calibrate_orientation_quats(sw_quat=q("sw_rotvec"), sw_fwd=q("sw_forward"),
                                                     ph_quat=q("ph_rotvec"), ph_fwd=q("ph_forward"))
        cal_sw.append(np.asarray(a, dtype=np.float64)); cal_ph.append(np.asarray(b, dtype=np.float64))
    blob["cal_rows"] = cal_rows
    blob["cal_sw"] = np.array(cal_sw)
    blob["cal_ph"] = np.array(cal_ph)

    # a non-default body: a bonemap stand-in, smooth 5, the first recording
    bm = _BoneMapStandIn()
    est = WatchPhoneUarm(smooth=5, bonemap=bm)
    x, p, m, e = run(est, recs[0])
    blob["bm_lengths"] = np.array([bm.left_lower_arm_length, bm.left_upper_arm_length])
    blob["bm_uarm_orig"] = np.asarray(bm.left_upper_arm_origin_rh, dtype=np.float64)
    blob["bm_body"] = est.body_measurements
    blob["bm_pred"] = np.array(p)
    blob["bm_msg"] = np.array(m)

    out = gg.OUT / "fk_only_trace.npz"
    np.savez_compressed(out, **blob)
    print("wrote", out, f"({out.stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
