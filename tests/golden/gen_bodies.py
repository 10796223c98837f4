#!/usr/bin/env python3
"""Generate tests/golden/body_traces.npz: the REFERENCE estimators built once per body (``Estimator(bonemap=...)``,
estimate/estimator.py:57-68) over rows that are already stored -- ``WatchPhonePocketNN``, ``WatchOnlyNN`` and ``WatchPhoneUarmNN`` over
the rows of ``stream_trace_<name>.npz`` (seeded weights, dropout 0, the loader patch of gen_stream_traces) and ``WatchPhoneUarm`` over
the first recording of ``fk_only_trace.npz``, at smooth 1 and 5, one Monte-Carlo sample.

Run in the build container only (the reference does not exist on the GPU box):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python /path/to/repo/tests/golden/gen_bodies.py

Importing gen_golden registers its ``aenum`` stand-in and puts the reference on sys.path.  Writes data only:
  bodies [B,9]                       the reference's own ``est.body_measurements`` of every stand-in
  bm_lengths [B,2], bm_origins [B,3] what the stand-ins carry (NaN row 0: no bonemap at all, the defaults)
  msg_<name>_s<smooth> [B,frames,25] the message of every frame; tail_<name>_s5 [B,frames,30] what msg_from_pred appends to it
  (name = pocket | watch | uarm | fk)"""
import sys
import warnings
from array import array
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_golden as gg  # noqa: E402

SMOOTHS = (1, 5)
# lower-arm length, upper-arm length, shoulder origin relative to the hips.  Row 0 is built with bonemap=None (the defaults); the others
# differ from the defaults in all nine values, the last one with a clearly non-zero third origin component and lengths far from 0.22 / 0.26
STAND_INS = (
    None,
    (0.2473, 0.3115, (-0.1822, 0.4417, 0.0108)),
    (0.1985, 0.2352, (-0.1511, 0.3893, -0.0214)),
    (0.3120, 0.3840, (-0.2290, 0.5160, 0.0870)),
)


class BoneMapStandIn:
    """the three attributes Estimator.__init__ reads from a BoneMap (estimator.py:55-63)"""

    def __init__(self, larm, uarm, orig):
        self.left_lower_arm_length = larm
        self.left_upper_arm_length = uarm
        self.left_upper_arm_origin_rh = np.array(orig, dtype=np.float64)


def stand_ins():
    return [None if s is None else BoneMapStandIn(*s) for s in STAND_INS]


def run(est, rows):
    msgs = []
    for row32 in rows:
        row = array("f", row32.tolist())          # wire type of ImuListener (stream/listener/imu.py:66-69)
        with np.errstate(all="ignore"):
            xx = est.parse_row_to_xx(row)
            pred = est.add_xx_to_row_hist_and_make_prediction(xx)
            msgs.append(np.asarray(est.msg_from_pred(pred, True), dtype=np.float64))
    return np.array(msgs)


def main():
    from wear_mocap_ape.estimate.watch_only import WatchOnlyNN
    from wear_mocap_ape.estimate.watch_phone_pocket_nn import WatchPhonePocketNN
    from wear_mocap_ape.estimate.watch_phone_uarm import WatchPhoneUarm
    from wear_mocap_ape.estimate.watch_phone_uarm_nn import WatchPhoneUarmNN

    bms = stand_ins()
    blob = {"bm_lengths": np.array([[np.nan, np.nan] if b is None else [b.left_lower_arm_length, b.left_upper_arm_length] for b in bms]),
            "bm_origins": np.array([[np.nan] * 3 if b is None else b.left_upper_arm_origin_rh for b in bms])}
    bodies = None

    def build(make):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return make()

    def record(name, make, rows):
        nonlocal bodies
        for smooth in SMOOTHS:
            msgs, got = [], []
            for bm in bms:
                est = build(lambda: make(smooth, bm))
                got.append(np.asarray(est.body_measurements, dtype=np.float64).reshape(9))
                msgs.append(run(est, rows))
            got = np.array(got)
            assert bodies is None or np.array_equal(bodies, got)      # every estimator class derives the same nine values
            bodies = got
            m = np.array(msgs)
            blob[f"msg_{name}_s{smooth}"] = m[:, :, :25]
            if smooth > 1:
                assert m.shape[2] == 25 + 6 * smooth
                blob[f"tail_{name}_s{smooth}"] = m[:, :, 25:]

    real_loader = gg.ref_nn.load_deployed_model_from_hash
    classes = {"pocket": WatchPhonePocketNN, "watch": WatchOnlyNN, "uarm": WatchPhoneUarmNN}
    for name, cls in classes.items():
        tr = np.load(gg.OUT / f"stream_trace_{name}.npz")
        seed = int(tr["weights_seed"])

        def fake_load(hash_str, _name=name, _seed=seed):
            # checkpoints are absent: same class + params as nn_models.py:390-408, seeded weights, dropout 0 (gen_stream_traces)
            model, p, _ = gg.ref_model(_name, _seed, dropout=0.0)
            return model, p

        gg.ref_nn.load_deployed_model_from_hash = fake_load
        record(name, lambda smooth, bm, _cls=cls, _name=name: _cls(model_hash=gg.HASHES[_name], smooth=smooth, add_mc_samples=True,
                                                                    monte_carlo_samples=1, bonemap=bm), tr["rows"])
    gg.ref_nn.load_deployed_model_from_hash = real_loader

    fk = np.load(gg.OUT / "fk_only_trace.npz")
    record("fk", lambda smooth, bm: WatchPhoneUarm(smooth=smooth, bonemap=bm), fk["rows"][:int(fk["lengths"][0])])

    blob["bodies"] = bodies
    blob["smooths"] = np.array(SMOOTHS, dtype=np.int32)
    out = gg.OUT / "body_traces.npz"
    np.savez_compressed(out, **blob)
    print("wrote", out, f"({out.stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
