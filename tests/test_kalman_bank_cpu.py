"""The Kalman estimator's device stream bank, one-call frames and replay (``ape_kalman_bank_*``, ``ape_kalman_replay``)
on the CPU: the header and the library's exports, the refusals that need no live model, the host helpers, and the oracle chain that is
the yardstick of tests/test_kalman_bank_gpu.py.  PARITY UNPINNED: the oracle restates the reference (oracle/kalman_oracle.py's header)."""
import ctypes as C
import re

import numpy as np
import pytest

from oracle import ape_oracle as orc
from oracle import kalman_oracle as ko
from tests.conftest import REPO

ENTRIES = ("ape_kalman_bank_create", "ape_kalman_bank_destroy", "ape_kalman_bank_reset", "ape_kalman_bank_reset_subset",
           "ape_kalman_bank_set_norm_stats", "ape_kalman_bank_set_body", "ape_kalman_bank_set_seed", "ape_kalman_bank_frame",
           "ape_kalman_bank_frame_host", "ape_kalman_replay")


def _lib():
    import __graft_entry__ as entry
    entry.build()
    from wear_mocap_ape_amd import _hip
    return _hip, _hip.lib()


def test_header_declares_the_kalman_bank_entries_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "ape_hip.h").read_text(), flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", text), name
    assert "#define APE_ABI_VERSION 7" in text
    _hip, lib = _lib()
    for name in ENTRIES:
        assert name in _hip.SIGNATURES and hasattr(lib, name), name
    assert lib.ape_abi_version() == 7


def test_entries_refuse_bad_arguments_without_a_device():
    _hip, lib = _lib()
    dummy = C.c_void_p(256)                          # never dereferenced: every call below is refused first
    starts = np.array([0, 3], dtype=np.int32)
    sp = C.c_void_p(starts.ctypes.data)
    body = np.zeros(9)
    bp = _hip.dptr(body, C.c_double)
    nul = [None] * 4
    pocket = _hip.PARSE_WATCH_PHONE_POCKET

    def replay(model=dummy, kind=pocket, rows=dummy, F=8, st=sp, R=2, smooth=3, b=bp, out=dummy, dtype=_hip.F64, n=dummy, flags=0):
        return lib.ape_kalman_replay(model, kind, rows, F, st, R, smooth, *nul, b, 1, flags, out, dtype, n, None, None)

    cases = {
        "replay NULL model": lambda: replay(model=None),
        "replay NULL rows": lambda: replay(rows=None),
        "replay NULL out": lambda: replay(out=None),
        "replay NULL n_rows": lambda: replay(n=None),
        "replay NULL body": lambda: replay(b=None),
        "replay NULL starts": lambda: replay(st=None),
        "replay kind": lambda: replay(kind=_hip.PARSE_WATCH_PHONE_UARM),
        "replay kind watch": lambda: replay(kind=_hip.PARSE_WATCH_ONLY | _hip.PARSE_BIG_ENDIAN),
        "replay F=0": lambda: replay(F=0),
        "replay start 3 >= F": lambda: replay(F=2),
        "replay R=0": lambda: replay(R=0),
        "replay R>F": lambda: replay(F=1, R=2),
        "replay smooth 65": lambda: replay(smooth=65),
        "replay dtype": lambda: replay(dtype=7),
        "replay flags": lambda: replay(flags=_hip.FLAG_NORMALIZE_INPUT),
        "create NULL model": lambda: lib.ape_kalman_bank_create(None, 4, 1, C.byref(C.c_void_p())),
        "create NULL out": lambda: lib.ape_kalman_bank_create(dummy, 4, 1, None),
        "frame NULL bank": lambda: lib.ape_kalman_bank_frame(None, pocket, dummy, None, 1, None, None, 0, dummy, _hip.F64, dummy, None, None),
        "frame_host NULL bank": lambda: lib.ape_kalman_bank_frame_host(None, pocket, dummy, 0, dummy, _hip.F64, dummy, None),
        "reset NULL bank": lambda: lib.ape_kalman_bank_reset(None),
        "reset_subset NULL bank": lambda: lib.ape_kalman_bank_reset_subset(None, sp, 2),
        "set_norm_stats NULL bank": lambda: lib.ape_kalman_bank_set_norm_stats(None, bp, bp, bp, bp),
        "set_body NULL bank": lambda: lib.ape_kalman_bank_set_body(None, bp),
        "set_seed NULL bank": lambda: lib.ape_kalman_bank_set_seed(None, 1),
    }
    for name, call in cases.items():
        assert call() != 0, f"{name} was accepted"
        assert lib.ape_last_error(), name
    bad = np.array([1], dtype=np.int32)
    assert replay(st=C.c_void_p(bad.ctypes.data), R=1) != 0
    assert b"seg_starts[0]" in lib.ape_last_error()
    falling = np.array([0, 5, 4], dtype=np.int32)
    assert replay(st=C.c_void_p(falling.ctypes.data), R=3) != 0
    assert b"seg_starts[2]" in lib.ape_last_error()
    assert lib.ape_kalman_bank_destroy(None) == 0      # like the other destroy entries


def test_bank_index_validation():
    from wear_mocap_ape_amd.streams import KalmanStreamBank

    class _Sized:
        _n = 5
    ok = KalmanStreamBank._indices(_Sized(), [4, 0, 2])
    assert ok.dtype == np.int32 and ok.tolist() == [4, 0, 2]
    assert KalmanStreamBank._indices(_Sized(), np.zeros(0, dtype=np.int64)).shape == (0,)
    for bad in ([0, 5], [-1], [1, 1], [[0, 1]], [0.5], 3):
        with pytest.raises(UserWarning):
            KalmanStreamBank._indices(_Sized(), bad)


@pytest.mark.parametrize("n", ["one", "smooth", "full"])
def test_trimming_a_packed_row_gives_the_reference_length(n):
    """msg_with_mc_samples (estimator.py:131-137): 25 values for one est row, 25 + 6 n for n > 1"""
    from wear_mocap_ape_amd.streams import trim_packed
    smooth, E = 3, 32
    n = {"one": 1, "smooth": smooth, "full": smooth * E}[n]
    rng = np.random.default_rng(n)
    est = rng.normal(size=(n, 21))
    msg = rng.normal(size=25)
    want = orc.msg_with_mc_samples(msg, est, True)
    packed = np.zeros(25 + 6 * smooth * E)
    packed[:25] = msg
    packed[25:25 + 6 * n] = est[:, :6].reshape(-1)
    got = trim_packed(packed, n)
    assert len(got) == len(want) == (25 if n == 1 else 25 + 6 * n)
    np.testing.assert_array_equal(np.asarray(got), np.asarray(want))


def test_oracle_chain_ragged_stack_sequence():
    """the yardstick of the GPU tests, pinned: KalmanFrameLogic inside WindowOracle at E = 32, W = 10, smooth = 3 stacks 3 rows for
    W + 1 frames, then 34, 65, 96, 96 ...; the message lengths follow (25 + 6 n)"""
    E, W, smooth = 32, 10, 3
    rng = np.random.default_rng(5)
    fl = ko.KalmanFrameLogic(ko.make_state_dict(W, 9), E, W)
    cur = {}
    win = orc.WindowOracle(W, smooth, None, lambda hist: fl.step(hist, cur["nz"], cur["init"]))
    counts, lengths = [], []
    for f in range(16):
        cur["nz"], cur["init"] = ko.draw_noise(rng, W, E), rng.standard_normal((E, 14)).astype(np.float32)
        pred = win.push(rng.normal(size=22))
        est = orc.arm_pose_from_targets(pred, orc.DEFAULT_BODY, orc.LAYOUT_ORI_CAL_LARM_UARM_HIPS, route="closed")
        msg = orc.msg_with_mc_samples(orc.msg_from_est(est, orc.DEFAULT_BODY, orc.LAYOUT_ORI_CAL_LARM_UARM_HIPS), est, True)
        assert np.all(np.isfinite(np.asarray(msg, dtype=np.float64)))
        counts.append(pred.shape[0])
        lengths.append(len(msg))
    assert counts == [3] * (W + 1) + [34, 65, 96, 96, 96]
    assert lengths == [43] * (W + 1) + [229, 415, 601, 601, 601]


def test_the_new_source_has_no_inline_asm_and_the_hazard_scan_list_is_unchanged():
    """tests/test_asm_hazards.py scans a fixed list of files; kalman_bank.hip stays out of it by holding no asm at all"""
    src = (REPO / "arm-pose-estimation_amd" / "csrc" / "kalman_bank.hip").read_text()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\basm\b|__asm__|__builtin_amdgcn_mfma", code)
    dev = (REPO / "arm-pose-estimation_amd" / "csrc" / "kalman_device.h").read_text()
    assert not re.search(r"\basm\b|__asm__", re.sub(r"//[^\n]*", "", dev))
    mk = (REPO / "arm-pose-estimation_amd" / "csrc" / "Makefile").read_text()
    assert "kalman_bank.hip" in mk.split("SRCS", 1)[1].split("\n", 1)[0]
    assert "kalman_bank.hip" not in mk.split("HAZARD_SRCS :=", 1)[1].split("\n", 1)[0]
