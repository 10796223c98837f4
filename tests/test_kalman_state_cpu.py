"""The Kalman bank's state hand-over without a device: the numpy restatement of the canonical record, the header and
the built library declare the six entries and the descriptor, and NULL arguments are refused before anything touches a device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
ENTRIES = ["ape_kalman_bank_state_desc", "ape_kalman_bank_export", "ape_kalman_bank_import", "ape_kalman_bank_get_draw_position",
           "ape_kalman_bank_set_draw_position", "ape_kalman_replay_resume"]
INVALID_ARG = 1            # APE_ERR_INVALID_ARG


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


@pytest.mark.parametrize("E,W,smooth", [(48, 10, 1), (16, 4, 3), (32, 10, 5)])
def test_kalman_words_is_the_formula(E, W, smooth):
    from wear_mocap_ape_amd import stream_state as ss
    want = (2 * W * 22 + E * W * 14 + smooth * E * 14 + smooth + 3) & ~3
    assert ss.kalman_words(E, W, smooth) == want and want % 4 == 0
    d = ss.kalman_desc(E, W, smooth)
    assert d == {"version": ss.KALMAN_VERSION, "E": E, "W": W, "smooth": smooth, "words_per_stream": want}
    if (E, W, smooth) == (48, 10, 1):
        assert want == 7836 and want * 4 == 31344


@pytest.mark.parametrize("E,W,smooth", [(48, 10, 1), (16, 4, 3), (32, 10, 5), (3, 1, 2)])
def test_kalman_pack_unpack_round_trip(E, W, smooth):
    from wear_mocap_ape_amd import stream_state as ss
    rng = np.random.default_rng(E + W + smooth)
    window = rng.standard_normal((W, 22))
    history = rng.standard_normal((E, W, 14)).astype(np.float32)
    stack = rng.standard_normal((smooth, E, 14)).astype(np.float32)
    counts = np.asarray([1 if k % 2 else E for k in range(smooth)], dtype=np.int32)
    rec = ss.kalman_pack(window, history, stack, counts)
    assert rec.dtype == np.float32 and rec.shape == (ss.kalman_words(E, W, smooth),)
    w2, h2, s2, c2, pad = ss.kalman_unpack(rec, ss.kalman_desc(E, W, smooth))
    assert w2.dtype == np.float64 and np.array_equal(w2, window)            # float64 and int32 parts keep their bits
    assert np.array_equal(h2, history) and np.array_equal(s2, stack)
    assert c2.dtype == np.int32 and np.array_equal(c2, counts)
    assert pad.size == rec.size - (2 * W * 22 + E * W * 14 + smooth * E * 14 + smooth) and not pad.view(np.int32).any()
    # the layout, word for word: window, history with the time step minor, stack, counts
    nw, nh = 2 * W * 22, E * W * 14
    assert np.array_equal(rec[:nw].view(np.float64), window.reshape(-1))
    assert np.array_equal(rec[nw + 14 * (W - 1):nw + 14 * W], history[0, W - 1])        # member 0's newest entry
    assert np.array_equal(rec[nw + nh + (smooth - 1) * E * 14:nw + nh + smooth * E * 14], stack[-1].reshape(-1))
    assert np.array_equal(rec[nw + nh + smooth * E * 14:][:smooth].view(np.int32), counts)
    with pytest.raises(UserWarning):
        ss.kalman_unpack(rec[:-4], ss.kalman_desc(E, W, smooth))
    with pytest.raises(UserWarning):
        ss.kalman_pack(window, history[:, :-1] if W > 1 else history[:, :0], stack, counts)


def test_header_declares_the_six_entries_and_the_struct():
    text = (REPO / "include" / "ape_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", text), name
    m = re.search(r"typedef struct ape_kalman_state_desc \{(.*?)\} ape_kalman_state_desc_t;", text, re.S)
    assert m, "ape_kalman_state_desc_t"
    fields = re.findall(r"\b(version|E|W|smooth|words_per_stream)\b", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == ["version", "E", "W", "smooth", "words_per_stream"]
    assert re.search(r"#define APE_KALMAN_STATE_VERSION 1\b", text)
    assert re.search(r"#define APE_ABI_VERSION 7\b", text)
    # the resumable replay: the arguments of ape_kalman_replay_bodies, then the four state arguments and the call base
    sig = lambda name: re.sub(r"\s+", " ", re.search(rf"\bint {name}\((.*?)\);", text, re.S).group(1))      # noqa: E731
    assert sig("ape_kalman_replay_resume") == sig("ape_kalman_replay_bodies") + (
        ", const void* state_in_dev, const int32_t* age_in_host, void* state_out_dev, int32_t* age_out_host, uint64_t call_base")


def test_the_built_library_exports_the_six_entries():
    from wear_mocap_ape_amd import _hip, stream_state as ss
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    from wear_mocap_ape_amd.streams import KalmanStreamBank
    lib = _hip.lib()
    assert lib.ape_abi_version() == 7 == _hip.ABI_VERSION
    for name in ENTRIES:
        assert name in _hip.SIGNATURES and hasattr(lib, name), name
    assert [f for f, _ in _hip.ApeKalmanStateDesc._fields_] == list(ss.KALMAN_DESC_KEYS)
    assert C.sizeof(_hip.ApeKalmanStateDesc) == 20 and _hip.KALMAN_STATE_VERSION == ss.KALMAN_VERSION == 1
    assert _hip.SIGNATURES["ape_kalman_replay_resume"][1][:-5] == _hip.SIGNATURES["ape_kalman_replay_bodies"][1]
    for meth in ("state_desc", "export_state", "import_state", "get_draw_position", "set_draw_position"):
        assert callable(getattr(KalmanStreamBank, meth)), meth
    for meth in ("get_state", "set_state"):
        assert callable(getattr(WatchPhonePocketKalman, meth)), meth


def test_null_arguments_are_refused_without_a_device():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)                          # never dereferenced: every call below is refused first
    d = _hip.ApeKalmanStateDesc()
    seed, calls = C.c_uint64(), C.c_uint64()

    def refused(status):
        return status == INVALID_ARG and b"NULL" in lib.ape_last_error()
    assert refused(lib.ape_kalman_bank_state_desc(None, C.byref(d)))
    assert refused(lib.ape_kalman_bank_state_desc(dummy, None))
    assert refused(lib.ape_kalman_bank_export(None, dummy, 1, dummy, dummy, None))
    for hole in (1, 3, 4):                           # streams, records, ages
        args = [dummy, dummy, 1, dummy, dummy, None]
        args[hole] = None
        assert refused(lib.ape_kalman_bank_export(*args)), hole
    assert refused(lib.ape_kalman_bank_import(None, C.byref(d), dummy, 1, dummy, dummy, None))
    assert refused(lib.ape_kalman_bank_import(dummy, None, dummy, 1, dummy, dummy, None))
    assert refused(lib.ape_kalman_bank_import(dummy, C.byref(d), None, 1, dummy, dummy, None))
    assert refused(lib.ape_kalman_bank_import(dummy, C.byref(d), dummy, 1, None, dummy, None))
    assert refused(lib.ape_kalman_bank_import(dummy, C.byref(d), dummy, 1, dummy, None, None))
    assert refused(lib.ape_kalman_bank_get_draw_position(None, C.byref(seed), C.byref(calls)))
    assert refused(lib.ape_kalman_bank_get_draw_position(dummy, None, C.byref(calls)))
    assert refused(lib.ape_kalman_bank_get_draw_position(dummy, C.byref(seed), None))
    assert refused(lib.ape_kalman_bank_set_draw_position(None, 1, 2))
    body = (C.c_double * 9)()
    tail = [None, None, None, None, 0]
    head = [_hip.PARSE_WATCH_PHONE_POCKET, dummy, 4, dummy, 1, 1, None, None, None, None, body, 7, 0, dummy, _hip.F64, dummy, None, None, None]
    assert refused(lib.ape_kalman_replay_resume(None, *head, *tail))
    for hole in (1, 13, 15):                         # rows, messages, row counts
        args = list(head)
        args[hole] = None
        assert refused(lib.ape_kalman_replay_resume(dummy, *args, *tail)), hole
