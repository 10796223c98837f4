"""lstm_cluster32.hip, long-window instantiations: a steady-state layer-1 section runs layer 0's input span of the NEXT step under its own
hand-over and parks the sums in LDS, the layer-0 section behind it starts from the park; x is staged one step further ahead, in two buffers
by step parity.  The sums are formed in the order they always were, so every bound is the suite's own: below 1e-6 against the f32 oracle
and against the first-generation cluster kernel.  What can go wrong is WHICH section reads the park and WHICH x buffer a span reads: every
window length from the shortest (T = 9: phases 2 .. 6 park, phase 7's layer-0 section is the last reader) to T = 13 gives four to eight
parking phases and both parities of the first and the last parked step; 513 rows leave a one-row last cluster."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests.test_hip_parity import make_model, _synthetic_windows
from tests.test_c32_cover_gpu import _check, _forward, _synthetic_model

pytestmark = pytest.mark.gpu
TOL = 1e-6
LONG = "ape_lstm_cluster32<256, 2, 32, false>"


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def _deployed(norm_stats, name, B, T, seed):
    st = norm_stats[name]
    model, sd, cfg = make_model(name, 3, st)
    assert cfg["I"] in (20, 22)                            # the three-block input span
    x = _synthetic_windows(st, B, T, cfg["I"], seed)
    xn = ((x.astype(np.float64) - st["xx_m"]) / st["xx_s"]).astype(np.float32)
    return model, sd, x, xn


def _synthetic30(B, T):
    model, sd = _synthetic_model(30)
    x = np.random.default_rng(1000 + T).normal(size=(B, T, 30)).astype(np.float32)
    x[..., 16:] *= 3.0                                     # (a block dropped or taken from the wrong step cannot hide below the tolerance)
    return model, sd, x


@pytest.mark.parametrize("name", ["pocket", "watch"])
@pytest.mark.parametrize("B", [513, 1024])
@pytest.mark.parametrize("T", [9, 10, 11, 12, 13])
def test_xspan_fill_drain_and_transitions(norm_stats, name, B, T):
    model, sd, x, xn = _deployed(norm_stats, name, B, T, 51)
    _check(model, sd, x, xn, name, True)                   # (asserts kernel_name == the long-window kernel)


@pytest.mark.parametrize("B", [513, 1024])
@pytest.mark.parametrize("T", [9, 13])
def test_xspan_four_block_input_span(B, T):
    model, sd, x = _synthetic30(B, T)
    _check(model, sd, x, x, "synthetic I=30", False)


@pytest.mark.parametrize("name", ["pocket", "watch", "synthetic30"])
def test_xspan_steady_state(norm_stats, name):
    if name == "synthetic30":
        model, sd, x = _synthetic30(1024, 64)
        _check(model, sd, x, x, name, False)
    else:
        model, sd, x, xn = _deployed(norm_stats, name, 1024, 64, 52)
        _check(model, sd, x, xn, name, True)


def test_xspan_no_leftovers_between_launches(norm_stats):
    """x_a at T = 64, x_b at T = 9, x_a at T = 64 on ONE model: each output bit-equal to a fresh model's single launch -- a park slot or an
    x buffer half left over from the launch in front shows here"""
    name = "pocket"
    st = norm_stats[name]
    model, sd, cfg = make_model(name, 3, st)
    xa = _synthetic_windows(st, 1024, 64, cfg["I"], 61)
    xb = _synthetic_windows(st, 1024, 9, cfg["I"], 62)
    model.set_kernel("cluster")
    assert model.kernel_name(1024, 64) == LONG and model.kernel_name(1024, 9) == LONG
    da, db = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
    ya = model(da, last_step_only=True, normalize_input=True)
    yb = model(db, last_step_only=True, normalize_input=True)
    ya2 = model(da, last_step_only=True, normalize_input=True)
    torch.cuda.synchronize()
    model.check()
    ya, yb, ya2 = (v.cpu().numpy()[:, 0] for v in (ya, yb, ya2))
    fresh_a, _, _ = make_model(name, 3, st)
    ya_fresh = _forward(fresh_a, xa, "cluster", True)
    fresh_b, _, _ = make_model(name, 3, st)
    yb_fresh = _forward(fresh_b, xb, "cluster", True)
    assert np.array_equal(ya, ya_fresh) and np.array_equal(yb, yb_fresh) and np.array_equal(ya2, ya_fresh)


def test_xspan_deterministic_on_both_hand_over_forms(norm_stats):
    """1024 x 13 twice, and once more with the opt-in plain in-XCD hand-over: all three bit-equal"""
    from wear_mocap_ape_amd import _hip
    model, sd, x, xn = _deployed(norm_stats, "pocket", 1024, 13, 71)
    B, T, _ = x.shape
    xd = torch.from_numpy(x).cuda()
    model.set_kernel("cluster")
    assert model.kernel_name(B, T) == LONG
    y1 = model(xd, last_step_only=True, normalize_input=True).cpu().numpy()[:, 0]
    model.check()
    y2 = model(xd, last_step_only=True, normalize_input=True).cpu().numpy()[:, 0]
    model.check()
    y3 = torch.empty((B, y1.shape[1]), dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().ape_lstm_forward(model.handle, C.c_void_p(xd.data_ptr()), B, T, _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_IN_XCD_PLAIN,
                                           None, 0.0, 0, C.c_void_p(y3.data_ptr()), None), "ape_lstm_forward")
    torch.cuda.synchronize()
    model.check()
    model.set_kernel("auto")
    assert np.array_equal(y1, y2) and np.array_equal(y1, y3.cpu().numpy())
    assert float(np.abs(y1 - orc.lstm_forward(sd, xn)[:, -1]).max()) < TOL


class Streamer:
    """a queue of 256 MiB device copies on a second stream (the pattern of tests/hooks/uneven_load_cases.py): the copies take whatever CUs
    are free, stream through every XCD's L2 and load the memory side while the cluster kernel hands its slices over"""

    def __init__(self):
        self.stream = torch.cuda.Stream()
        self.a = torch.full((64 << 20,), 1.0, dtype=torch.float32, device="cuda")
        self.b = torch.empty_like(self.a)
        self.bursts = 0

    def burst(self, n=24):
        with torch.cuda.stream(self.stream):
            for _ in range(n):
                self.b.copy_(self.a, non_blocking=True)
        self.bursts += 1

    def drain(self):
        self.stream.synchronize()


@pytest.fixture(scope="module")
def streamer():
    s = Streamer()
    yield s
    s.drain()
    assert s.bursts > 0 and float(s.b[12345]) == 1.0


@pytest.mark.parametrize("B", [640, 1024])
def test_xspan_under_uneven_load(norm_stats, streamer, B):
    """the shortest windows that park at both parities, beside a burst of device copies: 640 rows leave a quarter of the chip to the copies,
    1024 fill it (staggered start); four launches, every row against the oracle, nothing aborted"""
    model, sd, x, xn = _deployed(norm_stats, "pocket", B, 13, 81)
    xd = torch.from_numpy(x).cuda()
    ref = orc.lstm_forward(sd, xn)[:, -1]
    model.set_kernel("cluster")
    worst = 0.0
    for rep in range(4):
        streamer.burst()
        y = model(xd, last_step_only=True, normalize_input=True)          # launched while the copies run
        assert "ape_lstm_cluster32" in model.last_kernel(), model.last_kernel()
        worst = max(worst, float(np.abs(y.cpu().numpy()[:, 0] - ref).max()))
    streamer.drain()
    model.check()
    assert model.stats()["aborted_checks"] == 0, model.stats()
    model.set_kernel("auto")
    assert worst < TOL, (B, worst)
