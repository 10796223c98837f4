"""Host subset frames (``ape_*_frame_subset_host``, ``*.frame_host``, ``streams.tick``) without a GPU: the three entries are
declared and bound, they refuse NULL arguments before touching a device, and ``tick``'s round splitter is the pure function it is
documented to be."""
import ctypes as C
import re

import numpy as np
import pytest

from tests.conftest import REPO

ENTRIES = ("ape_streams_frame_subset_host", "ape_fk_bank_frame_subset_host", "ape_kalman_bank_frame_subset_host")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def test_header_declares_and_hip_binds_the_three_entries():
    from wear_mocap_ape_amd import _hip
    header = (REPO / "include" / "ape_hip.h").read_text()
    assert "#define APE_ABI_VERSION 7" in header                       # additive: the ABI number stays
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name), name
        assert len(_hip.SIGNATURES[name][1]) == n_args, (name, n_args)
    assert "replaces:" in header[header.index("host subset frames"):header.index("int ape_streams_frame_subset_host")]


def test_entries_refuse_null_arguments_without_a_device():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    d = C.c_void_p(256)                                                 # never dereferenced: every call below is refused first
    idx = np.arange(2, dtype=np.int32)
    ip = C.c_void_p(idx.ctypes.data)
    pocket, uarm = _hip.PARSE_WATCH_PHONE_POCKET, _hip.PARSE_WATCH_PHONE_UARM
    calls = [lambda: lib.ape_streams_frame_subset_host(None, pocket, d, ip, 2, 0, d, _hip.F32, None),
             lambda: lib.ape_streams_frame_subset_host(d, pocket, None, ip, 2, 0, d, _hip.F32, None),
             lambda: lib.ape_streams_frame_subset_host(d, pocket, d, None, 2, 0, d, _hip.F32, None),
             lambda: lib.ape_streams_frame_subset_host(d, pocket, d, ip, 2, 0, None, _hip.F32, None),
             lambda: lib.ape_fk_bank_frame_subset_host(None, uarm, d, ip, 2, d, _hip.F64, None),
             lambda: lib.ape_fk_bank_frame_subset_host(d, uarm, None, ip, 2, d, _hip.F64, None),
             lambda: lib.ape_fk_bank_frame_subset_host(d, uarm, d, ip, 2, None, _hip.F64, None),
             lambda: lib.ape_kalman_bank_frame_subset_host(None, pocket, d, ip, 2, 0, d, _hip.F64, d, None),
             lambda: lib.ape_kalman_bank_frame_subset_host(d, pocket, None, ip, 2, 0, d, _hip.F64, d, None),
             lambda: lib.ape_kalman_bank_frame_subset_host(d, pocket, d, ip, 2, 0, None, _hip.F64, d, None),
             lambda: lib.ape_kalman_bank_frame_subset_host(d, pocket, d, ip, 2, 0, d, _hip.F64, None, None)]
    for i, call in enumerate(calls):
        assert call() != 0 and b"NULL" in lib.ape_last_error(), i
    # kind, dtype and flags are checked before the bank is looked at
    assert lib.ape_fk_bank_frame_subset_host(d, pocket, d, ip, 2, d, _hip.F64, None) != 0 and b"kind" in lib.ape_last_error()
    assert lib.ape_fk_bank_frame_subset_host(d, uarm, d, ip, 2, d, 7, None) != 0 and b"dtype" in lib.ape_last_error()
    assert lib.ape_kalman_bank_frame_subset_host(d, uarm, d, ip, 2, 0, d, _hip.F64, d, None) != 0 and b"kind" in lib.ape_last_error()
    assert lib.ape_kalman_bank_frame_subset_host(d, pocket, d, ip, 2, _hip.FLAG_NORMALIZE_INPUT, d, _hip.F64, d, None) != 0
    assert b"flags" in lib.ape_last_error()


def test_banks_have_frame_host():
    from wear_mocap_ape_amd import streams
    for cls in (streams.StreamBank, streams.FkStreamBank, streams.KalmanStreamBank):
        doc = cls.frame_host.__doc__
        assert "BLOCKING" in doc and "mix freely" in doc, cls.__name__          # the mode rules are stated
    assert "per-stream mode" in streams.StreamBank.frame_host.__doc__ and "list position" in streams.StreamBank.frame_host.__doc__
    assert "list position" in streams.KalmanStreamBank.frame_host.__doc__ and "skip-ahead" in streams.tick.__doc__


def _ids_of(rounds, ids):
    return [np.asarray(ids)[r].tolist() for r in rounds]


def test_tick_rounds_example_of_the_issue():
    from wear_mocap_ape_amd.streams import tick_rounds
    ids = [3, 1, 3, 3, 1, 0]
    rounds, order = tick_rounds(ids)
    assert _ids_of(rounds, ids) == [[3, 1, 0], [3, 1], [3]]
    assert [r.tolist() for r in rounds] == [[0, 1, 5], [2, 4], [3]]
    assert np.array_equal(np.concatenate(rounds)[order], np.arange(6))


@pytest.mark.parametrize("ids", [[], [4], [2, 0, 1, 7], [5] * 6, [0, 1, 0, 1, 0, 1], [9, 9, 1, 9, 3, 1, 1, 9]])
def test_tick_rounds_properties(ids):
    from wear_mocap_ape_amd.streams import tick_rounds
    rounds, order = tick_rounds(ids)
    n = len(ids)
    a = np.asarray(ids, dtype=np.int64)
    if n == 0:
        assert rounds == [] and order.shape == (0,)
        return
    assert len(rounds) == max(ids.count(s) for s in set(ids))          # one round per repeat of the most frequent stream
    flat = np.concatenate(rounds)
    assert sorted(flat.tolist()) == list(range(n)) and np.array_equal(flat[order], np.arange(n))
    for r in rounds:
        assert len(set(a[r].tolist())) == len(r)                        # distinct streams within a round
        assert np.all(np.diff(r) > 0)                                   # arrival order within a round
    for s in set(ids):                                                  # a stream's k-th row sits in round k
        pos = [i for i, v in enumerate(ids) if v == s]
        assert [next(k for k, r in enumerate(rounds) if p in r) for p in pos] == list(range(len(pos)))
    if len(set(ids)) == n:
        assert len(rounds) == 1 and rounds[0].tolist() == list(range(n))
    if len(set(ids)) == 1:
        assert [r.tolist() for r in rounds] == [[i] for i in range(n)]


def test_tick_rounds_refuses_non_indices():
    from wear_mocap_ape_amd.streams import tick_rounds
    for bad in ([[0, 1]], [0.5, 1.0]):
        with pytest.raises(UserWarning):
            tick_rounds(bad)


class _StandInBank:
    """frame_host of a bank whose output row names (stream, how many rows that stream has had, a checksum of the row)"""

    def __init__(self, pair=False):
        self.count, self.calls, self.pair = {}, [], pair

    def frame_host(self, rows, streams, scale=1.0):
        streams = np.asarray(streams)
        assert len(set(streams.tolist())) == len(streams), "a round lists distinct streams"
        self.calls.append(streams.tolist())
        out = np.zeros((len(streams), 3))
        for j, s in enumerate(streams.tolist()):
            self.count[s] = self.count.get(s, 0) + 1
            out[j] = (s, self.count[s], scale * float(rows[j].sum()))
        return (out, np.arange(len(streams), dtype=np.int32) + 100 * len(self.calls)) if self.pair else out


def test_tick_reorders_outputs_through_a_stand_in_bank():
    from wear_mocap_ape_amd.streams import tick
    ids = [3, 1, 3, 3, 1, 0]
    rows = np.arange(12, dtype=np.float32).reshape(6, 2)
    bank = _StandInBank()
    out = tick(bank, rows, ids, scale=2.0)
    assert bank.calls == [[3, 1, 0], [3, 1], [3]]
    assert out[:, 0].tolist() == ids                                    # input order
    assert out[:, 1].tolist() == [1, 1, 2, 3, 2, 1]                     # per-stream arrival order
    assert out[:, 2].tolist() == (2.0 * rows.sum(axis=1)).tolist()      # every output belongs to its own row
    pair = _StandInBank(pair=True)
    o2, n2 = tick(pair, rows, ids)
    assert o2[:, 0].tolist() == ids and n2.tolist() == [100, 101, 200, 300, 201, 102]
    empty = tick(_StandInBank(), np.zeros((0, 2), np.float32), np.zeros((0,), np.int64))
    assert empty.shape == (0, 3)
    with pytest.raises(UserWarning):
        tick(_StandInBank(), rows[:5], ids)
