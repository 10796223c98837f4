"""Stream state hand-over without a device: the header and the binding declare the new entries, the canonical record's
numpy restatement round-trips, and an ``Estimator`` on the staged host path continues bit for bit from ``get_state`` / ``set_state``."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
ENTRIES = ["ape_streams_state_desc", "ape_streams_export", "ape_streams_import",
           "ape_fk_bank_state_desc", "ape_fk_bank_export", "ape_fk_bank_import", "ape_replay_resume"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def test_header_declares_the_state_entries_and_the_descriptor():
    text = (REPO / "include" / "ape_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", text), name
    m = re.search(r"typedef struct ape_stream_state_desc \{(.*?)\} ape_stream_state_desc_t;", text, re.S)
    assert m, "ape_stream_state_desc_t"
    fields = re.findall(r"\b(version|T|I|smooth|n_mc|O|words_per_stream)\b", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == ["version", "T", "I", "smooth", "n_mc", "O", "words_per_stream"]
    assert re.search(r"#define APE_ABI_VERSION 7\b", text)


def test_abi_version_stays_7_and_every_entry_is_bound():
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import FkStreamBank, StreamBank
    lib = _hip.lib()
    assert lib.ape_abi_version() == 7 == _hip.ABI_VERSION
    for name in ENTRIES:
        assert name in _hip.SIGNATURES and hasattr(lib, name), name
    assert [f for f, _ in _hip.ApeStreamStateDesc._fields_] == ["version", "T", "I", "smooth", "n_mc", "O", "words_per_stream"]
    assert C.sizeof(_hip.ApeStreamStateDesc) == 28
    for cls in (StreamBank, FkStreamBank):
        for meth in ("state_desc", "export_state", "import_state"):
            assert callable(getattr(cls, meth))
            assert "bodies" in getattr(cls, "export_state").__doc__.lower()


def test_state_entries_refuse_null_arguments_without_a_device():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)                          # never dereferenced: every call below is refused first
    d = _hip.ApeStreamStateDesc()
    for prefix in ("ape_streams", "ape_fk_bank"):
        assert getattr(lib, prefix + "_state_desc")(None, C.byref(d)) != 0 and b"NULL" in lib.ape_last_error()
        assert getattr(lib, prefix + "_export")(None, dummy, 1, dummy, dummy, None) != 0 and b"NULL" in lib.ape_last_error()
        assert getattr(lib, prefix + "_import")(None, C.byref(d), dummy, 1, dummy, dummy, None) != 0 and b"NULL" in lib.ape_last_error()
        assert getattr(lib, prefix + "_import")(dummy, None, dummy, 1, dummy, dummy, None) != 0 and b"NULL" in lib.ape_last_error()


@pytest.mark.parametrize("T,I,smooth,n_mc,O", [(6, 22, 5, 1, 14), (8, 20, 10, 1, 12), (1, 22, 3, 4, 14), (3, 5, 1, 1, 3), (6, 22, 3, 3, 14)])
def test_canonical_packing_round_trips(T, I, smooth, n_mc, O):
    from wear_mocap_ape_amd import stream_state as ss
    rng = np.random.default_rng(T * 100 + smooth)
    window = rng.standard_normal((T, I)).astype(np.float32)
    stack = rng.standard_normal((smooth, n_mc, O)).astype(np.float32)
    rec = ss.pack(window, stack)
    words = T * I + smooth * n_mc * O
    # the documented alignment: records are whole 16-byte units, the padding is zero
    assert rec.dtype == np.float32 and rec.shape == ((words + 3) // 4 * 4,) == (ss.words_per_stream(T, I, smooth, n_mc, O),)
    assert not rec[words:].any()
    desc = ss.make_desc(T, I, smooth, n_mc, O)
    assert desc["words_per_stream"] == rec.shape[0] and desc["version"] == ss.VERSION
    w2, s2 = ss.unpack(rec, desc)
    assert np.array_equal(w2, window) and np.array_equal(s2, stack)
    # time order: the newest row is the window's last, the newest prediction the stack's last
    assert np.array_equal(rec[(T - 1) * I:T * I], window[-1]) and np.array_equal(rec[words - n_mc * O:words], stack[-1].reshape(-1))
    with pytest.raises(UserWarning):
        ss.unpack(rec[:-4], desc)


def _stub(smooth, T=3):
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.utility.names import NNS_INPUTS, NNS_TARGETS

    class _Stub(Estimator):
        """staged host path, deterministic fake regressor: two 'samples' that depend on every row of the window and its order"""

        def parse_row_to_xx(self, row):
            return np.asarray(row, dtype=np.float32)

        def make_prediction_from_row_hist(self, xx_hist):
            w = np.arange(1, xx_hist.shape[0] + 1, dtype=np.float64)[:, None]
            base = (xx_hist.astype(np.float64) * w).sum(axis=0)[:4]
            return np.stack([base, np.cos(base)])

    return _Stub(list(NNS_INPUTS)[0], list(NNS_TARGETS)[0], normalize=False, smooth=smooth, seq_len=T)


def _feed(est, rows):
    return [est.add_xx_to_row_hist_and_make_prediction(est.parse_row_to_xx(r)).copy() for r in rows]


@pytest.mark.parametrize("smooth", [1, 4])
@pytest.mark.parametrize("n", [0, 1, 2, 5])
def test_host_estimator_continues_from_its_state(smooth, n):
    from wear_mocap_ape_amd import stream_state as ss
    m = 6
    rows = np.random.default_rng(10 * smooth + n).standard_normal((n + m, 5)).astype(np.float32)
    whole = _feed(_stub(smooth), rows)
    first = _stub(smooth)
    assert first._frame_runner() is None, "the stub must be on the staged host path"
    _feed(first, rows[:n])
    state = first.get_state()
    assert state["form"] == "host"
    assert bool(state["warm"] & ss.WINDOW_WARM) == (n > 0)
    assert bool(state["warm"] & ss.STACK_WARM) == (n > 0 and smooth > 1)
    if n == 1:                                           # the first row pads the whole window
        assert state["window"].shape == (3, 5) and all(np.array_equal(state["window"][t], rows[0]) for t in range(3))
    if n == 5:                                           # wrapped: the last T rows, oldest first
        assert np.array_equal(state["window"], rows[2:5])
    second = _stub(smooth)
    second.set_state(state)
    rest = _feed(second, rows[n:])
    assert len(rest) == m
    for a, b in zip(rest, whole[n:]):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_host_state_converts_to_the_device_form_with_the_models_stats():
    from wear_mocap_ape_amd import stream_state as ss
    est = _stub(4)
    est._normalize = True
    est._xx_m, est._xx_s = np.zeros(5), np.ones(5)
    est._yy_m, est._yy_s = np.linspace(-1, 1, 4), np.linspace(0.5, 2, 4)
    rows = np.random.default_rng(3).standard_normal((7, 5)).astype(np.float32)
    _feed(est, rows)
    state = est.get_state()
    desc, rec, warm = est.state_record(state)
    assert rec.shape == (1, desc["words_per_stream"]) and warm.tolist() == [ss.WINDOW_WARM | ss.STACK_WARM]
    window, stack = ss.unpack(rec[0], desc)
    assert np.array_equal(window, rows[4:7])
    # the device form is what the ring holds: the model's outputs, still normalised, float32
    want = ((state["stack"] - est._yy_m) / est._yy_s).astype(np.float32)
    assert np.array_equal(stack, want)
    back = est._stack_to_form(stack, "device", "host")
    assert np.abs(back - state["stack"]).max() <= 4 * np.finfo(np.float32).eps * np.abs(state["stack"]).max()
