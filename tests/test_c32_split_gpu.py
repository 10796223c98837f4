"""lstm_cluster32.hip with its recurrent products on f16 MFMAs (hi / lo split of power-of-two scaled operands) against the f32
oracle where the split is most exposed: trained-like weight magnitudes, saturated hidden states, z-scored inputs up to +-1e3, and a
NaN row that must stay in its own window.  Both instantiations (T <= 8 with the end forms, and the long form)."""
import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests.test_hip_parity import _synthetic_windows


def _model(name, st, wscale=1.0, seed=3):
    from wear_mocap_ape_amd.estimate import nn_models
    cfg = orc.MODEL_CONFIGS[name]
    sd = orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], seed)
    sd = {k: (v * np.float32(wscale)).astype(np.float32) if k.startswith("lstm.") else v for k, v in sd.items()}
    m = nn_models.DropoutLSTM(cfg["I"], cfg["H"], cfg["L"], cfg["O"], dropout=0.2, device=0)
    m.load_state_dict(sd)
    m.set_norm_stats(st["xx_m"], st["xx_s"], st["yy_m"], st["yy_s"])
    return m, sd, cfg


def _run(model, x, kernel):
    model.set_kernel(kernel)
    y = model(torch.from_numpy(x).cuda(), last_step_only=True, normalize_input=True).cpu().numpy()[:, 0]
    model.check()
    model.set_kernel("auto")
    return y


def _check(model, sd, st, x, label):
    B, T, _ = x.shape
    model.set_kernel("cluster")
    assert model.kernel_name(B, T) == f"ape_lstm_cluster32<256, 2, 32, {'true' if T <= 8 else 'false'}>"
    y = _run(model, x, "cluster")
    y1 = _run(model, x, "cluster_gen1")                   # the f32 first-generation kernel: the same sums in another order
    xn = ((x.astype(np.float64) - st["xx_m"]) / st["xx_s"]).astype(np.float32)
    y_ref = orc.lstm_forward(sd, xn)[:, -1]
    e, e1 = float(np.abs(y - y_ref).max()), float(np.abs(y1 - y_ref).max())
    print(f"\n[{label} {B}x{T}] split vs oracle {e:.2e}, f32 gen-1 vs oracle {e1:.2e}")
    assert np.isfinite(y).all()
    assert e <= max(1e-6, 3.0 * e1)
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("T", [64, 6])
def test_split_trained_magnitudes(norm_stats, T):
    """weights x 8: pre-activations of several units, most gates saturated (what trained models look like)"""
    st = norm_stats["pocket"]
    model, sd, cfg = _model("pocket", st, wscale=8.0)
    _check(model, sd, st, _synthetic_windows(st, 1024, T, cfg["I"], 21), "pocket W x 8")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [13, 5])
def test_split_saturated_hidden_states(norm_stats, T):
    """inputs at 30 standard deviations and weights x 4: |h| runs up to 1, the top of the f16 range of h * 2^15"""
    st = norm_stats["watch"]
    model, sd, cfg = _model("watch", st, wscale=4.0)
    rng = np.random.default_rng(5)
    x = (st["xx_m"] + st["xx_s"] * 30.0 * np.sign(rng.normal(size=(1024, T, cfg["I"])))).astype(np.float32)
    _check(model, sd, st, x, "watch saturated")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [64, 8])
def test_split_large_z_scores(norm_stats, T):
    """z-scored inputs up to +-1e3: the input columns stay on the f32 chain, nothing of them passes through f16"""
    st = norm_stats["pocket"]
    model, sd, cfg = _model("pocket", st)
    rng = np.random.default_rng(7)
    z = rng.uniform(-1e3, 1e3, size=(1024, T, cfg["I"]))
    x = (st["xx_m"] + st["xx_s"] * z).astype(np.float32)
    _check(model, sd, st, x, "pocket |z| <= 1e3")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [64, 6])
def test_split_nan_row_stays_in_its_window(norm_stats, T):
    st = norm_stats["pocket"]
    model, sd, cfg = _model("pocket", st)
    x = _synthetic_windows(st, 1024, T, cfg["I"], 9)
    y_clean = _run(model, x, "cluster")
    bad = 37                                              # a window in the middle of a 32-window cluster
    x[bad, T // 2, 3] = np.nan
    y = _run(model, x, "cluster")
    assert np.isnan(y[bad]).all()
    rest = np.arange(1024) != bad
    assert np.isfinite(y[rest]).all()
    assert np.array_equal(y[rest], y_clean[rest])
