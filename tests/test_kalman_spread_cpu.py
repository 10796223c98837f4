"""The Kalman bank's spread record (``APE_FLAG_SPREAD`` on ``ape_kalman_bank_frame`` / ``_frame_host`` / ``ape_kalman_replay*``; DESIGN.md
4.29) on the CPU: the refusals that happen before any model is read, the host helper, and the header's statement of the flag."""
import ctypes as C
import re

import numpy as np

from tests.conftest import REPO

FIVE = ("ape_kalman_bank_frame", "ape_kalman_bank_frame_host", "ape_kalman_replay", "ape_kalman_replay_bodies", "ape_kalman_replay_resume")


def _lib():
    import __graft_entry__ as entry
    entry.build()
    from wear_mocap_ape_amd import _hip
    return _hip, _hip.lib()


def _calls(_hip, lib):
    """the five entries as functions of `flags`, on pointers that are never dereferenced: every call below is refused first"""
    dummy = C.c_void_p(256)
    starts = np.array([0, 3], dtype=np.int32)
    sp = C.c_void_p(starts.ctypes.data)
    body = np.zeros(9)
    bp = _hip.dptr(body, C.c_double)
    nul = [None] * 4
    pocket = _hip.PARSE_WATCH_PHONE_POCKET
    head = lambda flags: (dummy, pocket, dummy, 8, sp, 2, 3, *nul, bp, 1, flags, dummy, _hip.F64, dummy, None, None)      # noqa: E731
    return {
        "ape_kalman_bank_frame": lambda flags: lib.ape_kalman_bank_frame(dummy, pocket, dummy, None, 1, None, None, flags, dummy, _hip.F64,
                                                                         dummy, None, None),
        "ape_kalman_bank_frame_host": lambda flags: lib.ape_kalman_bank_frame_host(dummy, pocket, dummy, flags, dummy, _hip.F64, dummy, None),
        "ape_kalman_replay": lambda flags: lib.ape_kalman_replay(*head(flags)),
        "ape_kalman_replay_bodies": lambda flags: lib.ape_kalman_replay_bodies(*head(flags), None),
        "ape_kalman_replay_resume": lambda flags, state_in=None: lib.ape_kalman_replay_resume(*head(flags), None, state_in, None, None, None, 0),
    }, starts, body


def test_flagged_resume_gets_as_far_as_the_state_age_pairing():
    """a state_in without age_in is what this call is refused for: the flag itself passed (the parent refused the flags first)"""
    _hip, lib = _lib()
    calls, *_keep = _calls(_hip, lib)
    for flags in (_hip.FLAG_SPREAD, _hip.FLAG_SPREAD | _hip.FLAG_PACKED_MSG):
        assert calls["ape_kalman_replay_resume"](flags, C.c_void_p(256)) != 0
        err = lib.ape_last_error()
        assert b"state_in and age_in" in err and b"flags" not in err, err


def test_every_other_flag_is_still_refused_and_the_message_names_both():
    _hip, lib = _lib()
    calls, *_keep = _calls(_hip, lib)
    for name in FIVE:
        for flags in (_hip.FLAG_NORMALIZE_INPUT, _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_SPREAD, _hip.FLAG_SPREAD | 0x80):
            assert calls[name](flags) != 0, (name, flags)
            err = lib.ape_last_error()
            assert b"flags" in err and b"APE_FLAG_PACKED_MSG" in err and b"APE_FLAG_SPREAD" in err, (name, err)


def test_split_spread_on_a_plain_array():
    from wear_mocap_ape_amd.streams import KalmanStreamBank, StreamBank
    rows = np.arange(3 * (25 + 12 + 21), dtype=np.float64).reshape(3, -1)
    head, rec = KalmanStreamBank.split_spread(rows)
    assert head.shape == (3, 37) and rec.shape == (3, 21)
    assert np.array_equal(head, rows[:, :37]) and np.array_equal(rec, rows[:, 37:])
    a, b = StreamBank.split_spread(rows)
    assert np.array_equal(a, head) and np.array_equal(b, rec)


def test_header_documents_the_flag_at_the_five_entries():
    text = (REPO / "include" / "ape_hip.h").read_text()
    for name in FIVE:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", text, flags=re.S)
        assert m, name
        doc = m.group(1)
        assert "APE_FLAG_SPREAD" in doc and "21" in doc, name
    assert "#define APE_ABI_VERSION 7" in text and "#define APE_SPREAD_WIDTH 21" in text
