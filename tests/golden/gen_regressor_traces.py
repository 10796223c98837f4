#!/usr/bin/env python3
"""Generate tests/golden/regressor_traces.npz: the REFERENCE estimators over the two regressors its loader dispatches besides
``DropoutLSTM`` (nn_models.py:393-400) -- ``WatchPhonePocketNN`` over the rows already stored in ``stream_trace_pocket.npz`` and
``WatchOnlyNN`` over those in ``stream_trace_watch.npz``, with the loader patched to return in turn

  * the reference ``DropoutFF(14|12, 256, 2, 22|20, dropout=0.0)`` with ``orc.make_ff_state_dict`` weights,
  * the reference ``ImuPoseLSTM`` with ``orc.make_imupose_state_dict`` weights,

at smooth 1 and 5, ``monte_carlo_samples = 3``, ``add_mc_samples = True``.  What the estimator does with these models is pinned by
the reference itself: a ``DropoutFF`` frame stacks 3 rows per frame (25 + 6*3*smooth values), an ``ImuPoseLSTM`` frame ONE, whatever
the sample count says (nn_models.py:246-251: 25 values at smooth 1, 55 at smooth 5) -- asserted below.

Run in the build container only (the reference does not exist on the GPU box):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python /path/to/repo/tests/golden/gen_regressor_traces.py

Importing gen_golden registers its ``aenum`` stand-in and puts the reference on sys.path.  Writes data only:
  msg_<model>_<name>_s<smooth> [frames, width]  the full ``msg_from_pred`` output of every frame (model = ff | imupose, name = pocket | watch)
  weights_seed, mc_samples, smooths, ff_hidden [H, n_hidden], seq_len_<name>"""
import sys
import warnings
from array import array
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_golden as gg  # noqa: E402

SMOOTHS = (1, 5)
MC_SAMPLES = 3
WEIGHTS_SEED = 3
FF_HIDDEN, FF_LAYERS = 256, 2


def main():
    import torch
    from oracle import ape_oracle as orc
    from wear_mocap_ape.estimate.watch_only import WatchOnlyNN
    from wear_mocap_ape.estimate.watch_phone_pocket_nn import WatchPhonePocketNN

    def make_ff(I, O):
        m = gg.ref_nn.DropoutFF(O, FF_HIDDEN, FF_LAYERS, I, dropout=0.0)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in orc.make_ff_state_dict(I, FF_HIDDEN, FF_LAYERS, O, WEIGHTS_SEED).items()})
        return m.eval()

    def make_imupose(I, O):
        m = gg.ref_nn.ImuPoseLSTM(input_size=I, hidden_layer_size=256, hidden_layer_count=2, output_size=O, dropout=0.0)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in orc.make_imupose_state_dict(I, O, WEIGHTS_SEED).items()})
        return m.eval()

    blob = {"weights_seed": np.array(WEIGHTS_SEED), "mc_samples": np.array(MC_SAMPLES), "smooths": np.array(SMOOTHS, dtype=np.int32),
            "ff_hidden": np.array([FF_HIDDEN, FF_LAYERS])}
    real_loader = gg.ref_nn.load_deployed_model_from_hash
    try:
        for name, cls in (("pocket", WatchPhonePocketNN), ("watch", WatchOnlyNN)):
            rows = np.load(gg.OUT / f"stream_trace_{name}.npz")["rows"]
            p = gg.ref_params(name)
            I, O = len(p["x_inputs_v"]), len(p["y_targets_v"])
            blob[f"seq_len_{name}"] = np.array(p["sequence_len"])
            for model_name, make in (("ff", make_ff), ("imupose", make_imupose)):
                # checkpoints are absent: the deployed params of nn_models.py:390-408 with another regressor class behind them
                gg.ref_nn.load_deployed_model_from_hash = lambda hash_str, _m=make, _p=p, _I=I, _O=O: (_m(_I, _O), dict(_p))
                for smooth in SMOOTHS:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        est = cls(model_hash=gg.HASHES[name], smooth=smooth, add_mc_samples=True, monte_carlo_samples=MC_SAMPLES)
                    msgs = []
                    for row32 in rows:
                        row = array("f", row32.tolist())          # wire type of ImuListener (stream/listener/imu.py:66-69)
                        with np.errstate(all="ignore"):
                            pred = est.add_xx_to_row_hist_and_make_prediction(est.parse_row_to_xx(row))
                            msgs.append(np.asarray(est.msg_from_pred(pred, True), dtype=np.float64))
                    m = np.array(msgs)
                    # the reference's own widths: n_mc rows per frame for DropoutFF, ONE for ImuPoseLSTM (the count is ignored)
                    want = 25 + 6 * MC_SAMPLES * smooth if model_name == "ff" else (25 if smooth == 1 else 25 + 6 * smooth)
                    assert m.shape == (len(rows), want), (model_name, name, smooth, m.shape, want)
                    blob[f"msg_{model_name}_{name}_s{smooth}"] = m
    finally:
        gg.ref_nn.load_deployed_model_from_hash = real_loader
    out = gg.OUT / "regressor_traces.npz"
    np.savez_compressed(out, **blob)
    print("wrote", out, f"({out.stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
