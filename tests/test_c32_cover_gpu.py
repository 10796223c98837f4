"""lstm_cluster32.hip, long-window instantiation, with the input span of layer 0 cut to the k-blocks that carry data: three where the
fourth is padding (I <= 24), four otherwise.  Against the f32 oracle at the module tolerance 1e-6 and against the first-generation cluster
kernel (the same sums in another order; the bound the suite has always held the pair to, test_hip_round2.py), at the window lengths where
the pipeline fills and drains just above the short-window boundary, on ragged and multi-launch batches, on both input-span forms, and
launch after launch on one model."""
import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests.test_hip_parity import make_model, _synthetic_windows

pytestmark = pytest.mark.gpu
TOL = 1e-6


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def _forward(model, x, kernel, normalize):
    model.set_kernel(kernel)
    y = model(torch.from_numpy(x).cuda(), last_step_only=True, normalize_input=normalize).cpu().numpy()[:, 0]
    model.check()                                          # (raises if a bounded spin gave up)
    model.set_kernel("auto")
    return y


def _check(model, sd, x, xn, label, normalize):
    B, T, _ = x.shape
    model.set_kernel("cluster")
    assert model.kernel_name(B, T) == "ape_lstm_cluster32<256, 2, 32, false>"
    model.set_kernel("cluster_gen1")
    assert "ape_lstm_cluster<" in model.kernel_name(B, T)
    y = _forward(model, x, "cluster", normalize)
    y1 = _forward(model, x, "cluster_gen1", normalize)
    y_ref = orc.lstm_forward(sd, xn)[:, -1]
    e_ref, e_gen = float(np.abs(y - y_ref).max()), float(np.abs(y - y1).max())
    print(f"\n[{label} B={B} T={T}] vs oracle {e_ref:.2e}, vs gen-1 kernel {e_gen:.2e}")
    assert np.isfinite(y).all()
    assert e_ref < TOL and e_gen < TOL
    return y


def _synthetic_model(I, seed=5, O=14):
    from wear_mocap_ape_amd.estimate import nn_models
    sd = orc.make_state_dict(I, 256, 2, O, seed)
    m = nn_models.DropoutLSTM(I, 256, 2, O, dropout=0.2, device=0)
    m.load_state_dict(sd)
    return m, sd


@pytest.mark.parametrize("name", ["pocket", "watch"])
@pytest.mark.parametrize("B,T", [(1024, 9), (1024, 12), (1024, 64), (700, 9), (513, 12), (2081, 12), (700, 64)])
def test_cover_deployed_models(norm_stats, name, B, T):
    """T = 9 | 12 | 64: fill and drain just above the short-window boundary (T = 9 has four steady-state phases), and the steady state; ragged
    last clusters (700, 513) and a batch of more than one launch (2081)"""
    st = norm_stats[name]
    model, sd, cfg = make_model(name, 3, st)
    assert cfg["I"] in (20, 22)                            # both on the three-block input span
    x = _synthetic_windows(st, B, T, cfg["I"], 31)
    xn = ((x.astype(np.float64) - st["xx_m"]) / st["xx_s"]).astype(np.float32)
    _check(model, sd, x, xn, name, True)


@pytest.mark.parametrize("I", [30, 25, 24, 22, 20])
@pytest.mark.parametrize("T", [9, 64])
def test_cover_input_span_forms(I, T):
    """a synthetic 2 x 256 model per input width: I = 30 | 25 keep the four-block input span (k-block 3 carries data), I = 24 | 22 | 20
    run three blocks.  Columns 16 .. I - 1 are made large so that a block dropped by mistake cannot hide below the tolerance."""
    model, sd = _synthetic_model(I)
    rng = np.random.default_rng(100 + I)
    x = rng.normal(size=(1024, T, I)).astype(np.float32)
    x[..., 16:] *= 3.0
    _check(model, sd, x, x, f"synthetic I={I}", False)


@pytest.mark.parametrize("name,T", [("pocket", 9), ("pocket", 12), ("watch", 64)])
def test_cover_consecutive_launches_see_their_own_x(norm_stats, name, T):
    """two launches with different x on ONE model, back to back: each must equal a fresh single launch of its x bit for bit -- x staged
    in the wrong buffer, or left over from the launch in front, shows here"""
    st = norm_stats[name]
    model, sd, cfg = make_model(name, 3, st)
    xa = _synthetic_windows(st, 1024, T, cfg["I"], 41)
    xb = _synthetic_windows(st, 1024, T, cfg["I"], 42)
    model.set_kernel("cluster")
    da, db = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
    ya = model(da, last_step_only=True, normalize_input=True)
    yb = model(db, last_step_only=True, normalize_input=True)
    ya2 = model(da, last_step_only=True, normalize_input=True)
    torch.cuda.synchronize()
    model.check()
    ya, yb, ya2 = (v.cpu().numpy()[:, 0] for v in (ya, yb, ya2))
    fresh, sd_f, _ = make_model(name, 3, st)
    yb_fresh = _forward(fresh, xb, "cluster", True)
    fresh2, _, _ = make_model(name, 3, st)
    ya_fresh = _forward(fresh2, xa, "cluster", True)
    assert not np.array_equal(ya, yb)
    assert np.array_equal(ya, ya_fresh) and np.array_equal(yb, yb_fresh) and np.array_equal(ya2, ya_fresh)
