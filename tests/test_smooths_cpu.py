"""Per-stream smoothing lengths without a GPU: the fixture ``smooth_traces.npz`` (tests/golden/gen_smooths.py: the
reference estimators built with smooth 1, 2, 3, 5, 8) is consistent with the stacking rule the banks implement, the library exports the
four entries, and the Python side refuses bad input and trims datagram rows."""
import ctypes as C

import numpy as np
import pytest

from oracle import ape_oracle as orc

SMOOTHS = (1, 2, 3, 5, 8)
# float64 throughout, values of order 1, a few dozen operations per message: 1e-12 is four orders above the rounding of either side and
# seven below the banks' budget against the same arrays
TOL_FIXTURE = 1e-12


@pytest.fixture(scope="module")
def traces(golden):
    return golden("smooth_traces.npz")


def _est_from_single_msg(m, layout):
    """the est row a single-row (smooth 1, one sample) message is a copy of (compose_msg.py:63-68 / :98-104)"""
    if layout == orc.LAYOUT_ORI_CAL_LARM_UARM:
        return np.concatenate([m[4:7], m[11:14], m[7:11], m[14:18]])
    return np.concatenate([m[4:7], m[11:14], m[18:21], m[7:11], m[14:18], m[21:25]])


def stack_by_rule(msg1, k, body, layout):
    """frames [F,25] of the k = 1 estimator -> (msg [F,25], tail [F,6k]) of an estimator built with smooth = k: row i of frame f's stack is
    the prediction k - 1 - i frames back, the first prediction after the cold start standing in for what is not there yet"""
    est1 = np.array([_est_from_single_msg(m, layout) for m in msg1])
    msgs, tails = [], []
    for f in range(len(est1)):
        rows = est1[[max(0, f - k + 1 + i) for i in range(k)]]
        msgs.append(orc.msg_from_est(rows, body, layout))
        tails.append(rows[:, :6].reshape(-1))
    return np.array(msgs), np.array(tails)


@pytest.mark.parametrize("name", ["pocket", "watch", "uarm", "fk"])
def test_fixture_follows_the_stacking_rule(golden, traces, name):
    assert tuple(traces["smooths"]) == SMOOTHS
    layout = orc.MODEL_CONFIGS[name]["layout"] if name != "fk" else orc.LAYOUT_ORI_CAL_LARM_UARM
    msg1 = traces[f"msg_{name}_s1"]
    assert msg1.shape == (20, 25)
    worst = 0.0
    for k in SMOOTHS:
        ref_m, ref_t = traces[f"msg_{name}_s{k}"], traces[f"tail_{name}_s{k}"]
        assert ref_m.shape == (20, 25) and ref_t.shape == (20, 6 * k)
        m, t = stack_by_rule(msg1, k, orc.DEFAULT_BODY, layout)
        worst = max(worst, float(np.abs(m - ref_m).max()), float(np.abs(t - ref_t).max()))
    print(f"{name}: worst |rule - reference| = {worst:.3e}")
    assert worst < TOL_FIXTURE, (name, worst)
    # the stored traces agree with the older fixtures of the same rows where they overlap
    if name != "fk":
        g = golden(f"stream_trace_{name}.npz")
        assert np.array_equal(g["msg_s5_mc1"][:, :25], traces[f"msg_{name}_s5"]) and np.array_equal(g["msg_s5_mc1"][:, 25:], traces[f"tail_{name}_s5"])


def test_library_exports_the_four_entries():
    import __graft_entry__ as entry
    entry.build()
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    for sym in ("ape_streams_set_smooths", "ape_streams_get_smooths", "ape_fk_bank_set_smooths", "ape_fk_bank_get_smooths"):
        assert sym in _hip.SIGNATURES and hasattr(lib, sym), sym
    # refused before any device is touched: a NULL bank
    vals = np.ones((1,), dtype=np.int32)
    assert lib.ape_streams_set_smooths(None, None, 1, C.c_void_p(vals.ctypes.data), None) != 0
    assert b"streams_set_smooths: NULL" in lib.ape_last_error()
    assert lib.ape_fk_bank_set_smooths(None, None, 1, C.c_void_p(vals.ctypes.data), None) != 0
    assert lib.ape_streams_get_smooths(None, C.c_void_p(vals.ctypes.data)) != 0
    assert lib.ape_fk_bank_get_smooths(None, C.c_void_p(vals.ctypes.data)) != 0


def _stub(cls, S, cap, n_mc, smooths):
    """a bank object without a device: the arguments are checked before the library is called"""
    sub = type("Stub" + cls.__name__, (cls,), {"smooths": property(lambda self: np.asarray(smooths, dtype=np.int32)), "__del__": lambda self: None})
    b = object.__new__(sub)
    b._n, b._smooth, b._n_mc, b._C, b._handle = S, cap, n_mc, C, None
    return b


@pytest.mark.parametrize("which", ["StreamBank", "FkStreamBank"])
def test_python_side_refuses_bad_input(which):
    from wear_mocap_ape_amd import streams
    bank = _stub(getattr(streams, which), 4, 5, 1, [1, 2, 3, 5])
    for values, idx in (([1, 2, 3], None), ([1, 2, 3, 4, 5], None), ([0, 1, 1, 1], None), ([1, 1, 1, 6], None), ([1.5, 1, 1, 1], None),
                        ([[1, 2, 3, 4]], None), ([1, 2], [0]), ([1, 2], [0, 0]), ([1, 2], [0, 4]), ([1, 2], [-1, 0]), ([1], [[0]]),
                        ([1], [0.5])):
        with pytest.raises(UserWarning):
            bank.set_smooths(values, streams=idx)
    rows = np.zeros((4, 25 + 6 * 5), dtype=np.float32)
    for r, idx in ((rows[:3], None), (rows[0], None), (rows[:, :30], None), (rows[:2], [0]), (rows[:2], [0, 0]), (rows[:2], [0, 9])):
        with pytest.raises(UserWarning):
            bank.split_datagrams(r, streams=idx)
    for sm, mc in (([0, 1], 1), ([1, 2], 0), ([[1]], 1), ([1.0], 1)):
        with pytest.raises(UserWarning):
            streams.datagram_lengths_of(sm, mc)


def test_split_datagrams_trims_rows_to_the_stated_lengths():
    from wear_mocap_ape_amd import streams
    smooths, cap, M = [1, 2, 3, 5, 5, 1], 5, 4
    bank = _stub(streams.StreamBank, 6, cap, M, smooths)
    ln = bank.datagram_lengths()
    assert ln.tolist() == [25 + 24, 25 + 48, 25 + 72, 25 + 120, 25 + 120, 25 + 24]
    one = _stub(streams.StreamBank, 6, cap, 1, smooths)
    assert one.datagram_lengths().tolist() == [25, 37, 43, 55, 55, 25]            # a single stacked row: the message alone
    assert _stub(streams.FkStreamBank, 6, cap, 1, smooths).datagram_lengths().tolist() == [25, 37, 43, 55, 55, 25]
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((6, 25 + 6 * cap * M + 21)).astype(np.float32)    # (with a spread record behind the fixed stride)
    parts = bank.split_datagrams(rows)
    assert [p.shape for p in parts] == [(int(n),) for n in ln]
    for s, p in enumerate(parts):
        assert np.shares_memory(p, rows) and np.array_equal(p, rows[s, :ln[s]]) and p.tobytes() == rows[s, :ln[s]].tobytes()
    sub = bank.split_datagrams(rows[[4, 0, 2]], streams=[4, 0, 2])
    assert [p.shape[0] for p in sub] == [int(ln[4]), int(ln[0]), int(ln[2])]
    assert np.array_equal(sub[1], rows[0, :ln[0]])
    assert bank.split_datagrams(rows[:0], streams=[]) == []
