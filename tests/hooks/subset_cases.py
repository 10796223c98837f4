"""Subset frames of the stream bank on the test-hooks library (lib/diag/libape_hip_testhooks.so): the Monte-Carlo contract, read through
`ape_debug_subset_targets`, and the re-issue of an aborted subset frame, staged with `ape_debug_poke`.  Not collected with the suite:
tests/test_streams_subset.py runs this file in a child process whose APE_HIP_LIB names that library."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_replay import _estimator, _synthetic_rows
from tests.test_streams_subset import _frame_c, _History

pytestmark = pytest.mark.gpu


def _hook(lib, name, argtypes):
    assert hasattr(lib, name), "this file runs on the test-hooks library (APE_HIP_LIB)"
    f = getattr(lib, name)
    f.restype, f.argtypes = C.c_int, argtypes
    return f


def _windows(feats, T):
    """the window of a stream's newest row: its last T feature rows since the cold start, the first one repeated in front"""
    n = len(feats)
    return np.stack([feats[max(0, n - T + t)] for t in range(T)])


@pytest.mark.parametrize("n_mc", [4, 25, 70])
def test_subset_monte_carlo_contract(golden, tmp_path, monkeypatch, n_mc):
    """a frame's samples are those of ONE ape_lstm_forward(DROPOUT_PHILOX, p, seed + c) over the repeated compact windows in list order"""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    lib = _hip.lib()
    targets = _hook(lib, "ape_debug_subset_targets", [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
    S, smooth, p, seed, ticks = 20, 2, 0.2, 987654321, 6
    est = _estimator(tmp_path, monkeypatch, "pocket", 1, p, smooth=smooth, add_mc_samples=True, monte_carlo_samples=n_mc)
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    pool = _synthetic_rows(golden, "pocket", S * ticks, n_mc)
    feats = est.parse_rows(pool, out_dtype=torch.float32).cpu().numpy()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kernel in ("tile16", "auto"):
        model.set_kernel(kernel)
        bank = StreamBank(model, S, T, smooth=smooth, normalize=True, dtype=torch.float64, monte_carlo_samples=n_mc, dropout=p, seed=seed)
        rng = np.random.default_rng(3)
        hist = [[] for _ in range(S)]
        for t in range(ticks):
            streams = rng.permutation(S)[:int(rng.integers(1, S + 1))]
            if t == 2:
                bank.reset(streams=streams[:3])
                for s in streams[:3]:
                    hist[s] = []
            K = len(streams)
            _frame_c(bank, kind, torch.from_numpy(pool[t * S + streams]).cuda(), streams,
                     _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG, torch.float64)
            for j, s in enumerate(streams):
                hist[s].append(feats[t * S + s])
            y = torch.empty((K * n_mc, model.output_size), dtype=torch.float32, device="cuda")
            assert targets(bank._handle, K, C.c_void_p(y.data_ptr()), st) == 0
            x = np.repeat(np.stack([_windows(hist[s], T) for s in streams]), n_mc, axis=0)
            xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
            yr = torch.empty_like(y)
            _hip.check(lib.ape_lstm_forward(model.handle, C.c_void_p(xd.data_ptr()), K * n_mc, T,
                                            _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_DROPOUT_PHILOX, None, p, seed + t,
                                            C.c_void_p(yr.data_ptr()), st), "ape_lstm_forward")
            model.recover()
            y, yr = y.cpu().numpy().reshape(K, n_mc, -1), yr.cpu().numpy().reshape(K, n_mc, -1)
            assert np.std(y[:, 0] - y[:, 1]) > 1e-3                     # the samples differ: dropout is on
            if kernel == "tile16":
                assert np.array_equal(y, yr), t
            else:
                assert np.abs(y - yr).max() < 1e-6, t
        del bank
    model.set_kernel("auto")


def test_aborted_subset_frame_is_reissued(golden, tmp_path, monkeypatch):
    """a subset frame on a cooperative route, then the sticky status word set (nothing is made to give up): recover() re-issues the
    frame's regressor and post-filter on the kernels that need no co-residency, into the same output, and counts it"""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    poke = _hook(_hip.lib(), "ape_debug_poke", [C.c_void_p, C.c_int, C.c_uint])
    S, smooth = 64, 3
    est = _estimator(tmp_path, monkeypatch, "pocket", 2, 0.0, smooth=smooth, add_mc_samples=True, monte_carlo_samples=1)
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    pool = _synthetic_rows(golden, "pocket", 3 * S, 17)
    flags = _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG
    streams = [np.arange(S), np.random.default_rng(1).permutation(S)]
    rows = [torch.from_numpy(pool[:S]).cuda(), torch.from_numpy(pool[S:2 * S]).cuda()]

    def run(abort):
        bank = StreamBank(model, S, T, smooth=smooth, normalize=True, dtype=torch.float64)
        outs = [_frame_c(bank, kind, rows[0], streams[0], flags, torch.float64)]
        bank.recover()                                  # (recover behind a frame, before the next one is enqueued)
        outs.append(_frame_c(bank, kind, rows[1], streams[1], flags, torch.float64))
        kernel = model.last_kernel()
        torch.cuda.synchronize()
        if abort:
            outs[1].fill_(float("nan"))
            assert poke(model.handle, 0, 1) == 0
        bank.recover()
        return [o.cpu().numpy() for o in outs], kernel

    clean, kernel = run(False)
    assert "cluster" in kernel, kernel
    before = model.stats()
    got, _ = run(True)
    after = model.stats()
    assert after["aborted_checks"] == before["aborted_checks"] + 1
    assert after["reissued_calls"] == before["reissued_calls"] + 1
    assert after["lost_calls"] == before["lost_calls"]
    assert np.array_equal(got[0], clean[0])
    assert np.isfinite(got[1]).all() and np.abs(got[1] - clean[1]).max() < 1e-6
    hist = _History(S)
    for t in range(2):
        hist.add(streams[t], pool[t * S:(t + 1) * S], got[t])
    hist.check_against_replay(est, 5e-6)
