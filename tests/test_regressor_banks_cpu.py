"""DropoutFF and ImuPoseLSTM behind the device frames, stream banks and replays: what holds without a GPU -- the new
C entry is declared and bound and the ABI version is unchanged, the stacked-row count the three Python layers share, the fixture the
reference wrote (tests/golden/gen_regressor_traces.py), the bank route of an ImuPoseLSTM model."""
import ctypes as C
import re

import numpy as np
import pytest

from tests.conftest import REPO


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def test_new_replay_entry_is_declared_and_the_abi_version_stays():
    from wear_mocap_ape_amd import _hip
    header = (REPO / "include" / "ape_hip.h").read_text()
    assert re.search(r"#define\s+APE_ABI_VERSION\s+7\b", header)
    assert _hip.ABI_VERSION == 7 and _hip.lib().ape_abi_version() == 7
    assert re.search(r"\bint\s+ape_replay_regressor\s*\(", header)
    assert "ape_replay_regressor" in _hip.SIGNATURES and hasattr(_hip.lib(), "ape_replay_regressor")
    # the argument list of ape_replay_bodies
    assert _hip.SIGNATURES["ape_replay_regressor"][1] == _hip.SIGNATURES["ape_replay_bodies"][1]
    decl = lambda name: re.sub(r"\s+", " ", re.search(name + r"\s*\(([^;]*)\)\s*;", header).group(1))      # noqa: E731
    assert decl(r"\bape_replay_regressor") == decl(r"\bape_replay_bodies")


def test_new_replay_entry_refuses_bad_arguments_without_a_device():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)                          # never dereferenced: every call below is refused first
    st = np.zeros(1, dtype=np.int32)

    def call(F=10, smooth=1, n_mc=1, rows=dummy):
        return lib.ape_replay_regressor(None, 0, rows, F, C.c_void_p(st.ctypes.data), 1, 6, smooth, n_mc, 0.0, 7, 0, dummy, _hip.F64, None,
                                        0, None, None)

    for kw, what in ((dict(F=0), b"F=0"), (dict(smooth=65), b"smooth"), (dict(n_mc=0), b"n_mc"), (dict(rows=None), b"NULL")):
        assert call(**kw) != 0 and what in lib.ape_last_error(), kw
    assert call() != 0 and b"model" in lib.ape_last_error()          # valid arguments, no model: no CPU fallback


def test_effective_mc_for_the_three_model_kinds():
    from wear_mocap_ape_amd.estimate.nn_models import DropoutFF, DropoutLSTM, ImuPoseLSTM, effective_mc
    for n in (1, 3, 25, 60):
        assert effective_mc(DropoutLSTM, n) == n
        assert effective_mc(DropoutFF, n) == n
        assert effective_mc(ImuPoseLSTM, n) == 1                     # the reference ignores the count (nn_models.py:246-251)

    class _Sub(ImuPoseLSTM):
        pass
    assert effective_mc(_Sub, 25) == 1
    # instances count like their classes (no device needed to make one: __new__ only)
    assert effective_mc(object.__new__(ImuPoseLSTM), 25) == 1 and effective_mc(object.__new__(DropoutFF), 25) == 25


def test_fixture_widths_are_the_references(golden):
    g = golden("regressor_traces.npz")
    mc = int(g["mc_samples"])
    assert mc == 3 and list(g["smooths"]) == [1, 5]
    for name in ("pocket", "watch"):
        frames = golden(f"stream_trace_{name}.npz")["rows"].shape[0]
        for smooth in (1, 5):
            assert g[f"msg_ff_{name}_s{smooth}"].shape == (frames, 25 + 6 * mc * smooth)
            assert g[f"msg_imupose_{name}_s{smooth}"].shape == (frames, 25 if smooth == 1 else 25 + 6 * smooth)
            # dropout 0: the three samples of a DropoutFF frame are the same row, so are their hand / elbow columns
            t = g[f"msg_ff_{name}_s{smooth}"][:, 25:].reshape(frames, smooth, mc, 6)
            assert np.array_equal(t[:, :, 0], t[:, :, 1]) and np.array_equal(t[:, :, 0], t[:, :, 2])


def test_bank_route_of_an_imupose_model_is_unchanged():
    """ape_debug_bank_route (pure arithmetic): an ImuPoseLSTM bank never shares layer 0 -- it has one row per stream and no dropout"""
    from wear_mocap_ape_amd import _hip

    class Dims(C.Structure):
        _fields_ = [(n, C.c_int32) for n in ("input_size", "hidden_size", "num_layers", "output_size", "target_layout", "device", "model_kind")]
    lib = _hip.lib()
    lib.ape_debug_bank_route.restype = C.c_int
    lib.ape_debug_bank_route.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    out = (C.c_longlong * 4)()
    for S, n_mc in ((1, 25), (1024, 1), (1024, 25), (8192, 25)):
        d = Dims(22, 256, 2, 14, 0, 0, _hip.MODEL_IMUPOSE)
        assert lib.ape_debug_bank_route(C.byref(d), 256, S, 6, n_mc, out) == 0
        assert out[0] == 0, (S, n_mc, list(out))
