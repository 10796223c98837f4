"""Host subset frames on the test-hooks library (lib/diag/libape_hip_testhooks.so): the recovery branch of
`ape_streams_frame_subset_host`, staged with `ape_debug_poke` the way tests/hooks/poke_cases.py stages it for `ape_streams_frame_host` --
the model's sticky status word is set in front of the frame, nothing is made to give up.  Not collected with the suite:
tests/test_subset_host_gpu.py runs this file in a child process whose APE_HIP_LIB names that library."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.hooks.subset_cases import _hook
from tests.test_replay import _estimator, _synthetic_rows

pytestmark = pytest.mark.gpu


def test_aborted_host_subset_frame_recovers_inside_the_call(golden, tmp_path, monkeypatch):
    """a host frame on a cooperative route behind the staged status word: the call re-issues regressor and post-filter on the batch-tile
    kernel before it returns -- the bits of a twin bank with the same history whose frame ran on that kernel -- and
    ape_streams_frame_stats counts it"""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    poke = _hook(_hip.lib(), "ape_debug_poke", [C.c_void_p, C.c_int, C.c_uint])
    S, smooth = 64, 3
    est = _estimator(tmp_path, monkeypatch, "pocket", 2, 0.0, smooth=smooth, add_mc_samples=True, monte_carlo_samples=1)
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    pool = _synthetic_rows(golden, "pocket", 2 * S, 17)
    lists = [np.arange(S), np.random.default_rng(1).permutation(S)]
    # the twin shares the bank's history: frame 0 on the same cooperative route (same list, same S), and only the frame under test on
    # the batch-tile kernel, where the re-issue runs
    twin = StreamBank(model, S, T, smooth=smooth, normalize=True, dtype=torch.float64)
    bank = StreamBank(model, S, T, smooth=smooth, normalize=True, dtype=torch.float64)
    want = [twin.frame_host(pool[:S], lists[0], kind, datagrams=True)]
    got = [bank.frame_host(pool[:S], lists[0], kind, datagrams=True)]
    assert "cluster" in model.last_kernel(), model.last_kernel()
    assert np.isfinite(got[0]).all() and np.array_equal(got[0], want[0])
    model.set_kernel("tile16")
    want.append(twin.frame_host(pool[S:], lists[1], kind, datagrams=True))
    model.set_kernel("auto")
    before = model.stats()
    assert poke(model.handle, 0, 1) == 0
    got.append(bank.frame_host(pool[S:], lists[1], kind, datagrams=True))
    after, fs = model.stats(), bank.frame_stats()
    print("stats", before, after, {k: fs[k] for k in ("frames", "fallback_syncs", "recovered")},
          "max |recovered - twin| =", float(np.abs(got[1] - want[1]).max()))
    assert fs["frames"] == 2 and fs["recovered"] == 1
    assert after["aborted_checks"] == before["aborted_checks"] + 1 and after["reissued_calls"] == before["reissued_calls"] + 1
    assert after["lost_calls"] == before["lost_calls"]
    assert np.isfinite(got[1]).all() and np.array_equal(got[1], want[1])             # the whole row: message, stack and all
    # the bank goes on: the next frame is clean
    nxt = bank.frame_host(pool[:S], lists[0], kind, datagrams=True)
    assert np.isfinite(nxt).all() and bank.frame_stats()["recovered"] == 1
