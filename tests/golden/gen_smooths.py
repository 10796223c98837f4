#!/usr/bin/env python3
"""Generate tests/golden/smooth_traces.npz: the REFERENCE estimators built once per smoothing length (``Estimator(smooth=...)``,
estimate/estimator.py:45,112-118) over rows that are already stored -- ``WatchPhonePocketNN``, ``WatchOnlyNN`` and ``WatchPhoneUarmNN``
over the rows of ``stream_trace_<name>.npz`` (seeded weights, dropout 0, one Monte-Carlo sample, ``add_mc_samples=True``; the loader
patch of gen_bodies) and ``WatchPhoneUarm`` over the first recording of ``fk_only_trace.npz``, at smooth 1, 2, 3, 5 and 8.  The traces are
20 frames long, so every ring up to 8 wraps.

Run in the build container only (the reference does not exist on the GPU box):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python /path/to/repo/tests/golden/gen_smooths.py

Importing gen_golden registers its ``aenum`` stand-in and puts the reference on sys.path.  Writes data only:
  smooths [5]                         the smoothing lengths
  msg_<name>_s<k> [frames,25]         the message of every frame of the estimator built with smooth = k
  tail_<name>_s<k> [frames,6k]        what msg_from_pred appends to it (k = 1: the reference appends nothing; stored as est[0, :6],
                                      which the single-row message carries in columns 4:7 and 11:14)
  (name = pocket | watch | uarm | fk)"""
import sys
import warnings
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, str(Path(__file__).resolve().parent))
import gen_golden as gg  # noqa: E402
from gen_bodies import run  # noqa: E402

SMOOTHS = (1, 2, 3, 5, 8)
FRAMES = 20


def main():
    from wear_mocap_ape.estimate.watch_only import WatchOnlyNN
    from wear_mocap_ape.estimate.watch_phone_pocket_nn import WatchPhonePocketNN
    from wear_mocap_ape.estimate.watch_phone_uarm import WatchPhoneUarm
    from wear_mocap_ape.estimate.watch_phone_uarm_nn import WatchPhoneUarmNN

    blob = {"smooths": np.array(SMOOTHS, dtype=np.int32)}

    def record(name, make, rows):
        rows = rows[:FRAMES]
        for k in SMOOTHS:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                est = make(k)
            m = run(est, rows)
            blob[f"msg_{name}_s{k}"] = m[:, :25]
            if k > 1:
                assert m.shape[1] == 25 + 6 * k
                blob[f"tail_{name}_s{k}"] = m[:, 25:]
            else:
                assert m.shape[1] == 25
                blob[f"tail_{name}_s1"] = np.concatenate([m[:, 4:7], m[:, 11:14]], axis=1)

    real_loader = gg.ref_nn.load_deployed_model_from_hash
    classes = {"pocket": WatchPhonePocketNN, "watch": WatchOnlyNN, "uarm": WatchPhoneUarmNN}
    for name, cls in classes.items():
        tr = np.load(gg.OUT / f"stream_trace_{name}.npz")
        seed = int(tr["weights_seed"])

        def fake_load(hash_str, _name=name, _seed=seed):
            model, p, _ = gg.ref_model(_name, _seed, dropout=0.0)
            return model, p

        gg.ref_nn.load_deployed_model_from_hash = fake_load
        record(name, lambda k, _cls=cls, _name=name: _cls(model_hash=gg.HASHES[_name], smooth=k, add_mc_samples=True, monte_carlo_samples=1),
               tr["rows"])
    gg.ref_nn.load_deployed_model_from_hash = real_loader

    fk = np.load(gg.OUT / "fk_only_trace.npz")
    record("fk", lambda k: WatchPhoneUarm(smooth=k), fk["rows"][:int(fk["lengths"][0])])

    out = gg.OUT / "smooth_traces.npz"
    np.savez_compressed(out, **blob)
    print("wrote", out, f"({out.stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
