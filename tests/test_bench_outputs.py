"""bench.py's plain run on the GPU: the result line carries the contract keys and nothing of the --full legs, `--steps` is the
number of timed steps, and `--dump-outputs` writes what the last timed step computed -- checked here against the CPU oracle on
bench.py's own seeded inputs (the first 64 of the 1024 windows; tolerances as tests/test_hip_parity.py)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import ape_oracle as orc

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "roofline"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert abs(d["value"] - 1024 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    for k in ("batch1", "cpu_baseline", "bank_frame_ms", "other_paths_us", "fp16_config4", "detail"):
        assert k not in d, k
    assert not (tmp_path / "bench_detail.json").exists()

    y = np.load(out / "targets.npy")
    est = np.load(out / "est.npy")
    assert y.dtype == np.float32 and y.shape == (1024, 14)
    assert est.dtype == np.float32 and est.shape == (1024, 21)

    sys.path.insert(0, str(REPO))
    import bench
    from wear_mocap_ape_amd.utility import data_stats
    from wear_mocap_ape_amd.utility.names import NNS_INPUTS, NNS_TARGETS
    P = bench.POCKET
    sd = bench.synthetic_state_dict(P["I"], P["H"], P["L"], P["O"], seed=0)
    stats = data_stats.get_norm_stats(NNS_INPUTS.WATCH_PHONE_CAL_HIP, NNS_TARGETS.ORI_CAL_LARM_UARM_HIPS)
    n = 64
    x = bench.synthetic_windows(stats, 0, n, bench.T_FRAMES, P["I"])
    y_ref, est_ref = orc.infer_windows(sd, stats, bench.DEFAULT_BODY, P["layout"], x)
    assert np.abs(y[:n] - y_ref).max() < 1e-6
    e = est[:n].astype(np.float64)
    assert np.abs(e[:, :9] - est_ref[:, :9]).max() < 2e-6
    for c in (9, 13, 17):               # quaternions: sign-aware only where the reference w ~ 0 (as bench.py's parity)
        a, b = e[:, c:c + 4], est_ref[:, c:c + 4]
        dp, dm = np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1)
        assert np.where(np.abs(b[:, 0]) < 1e-4, np.minimum(dp, dm), dp).max() < 2e-6, c
