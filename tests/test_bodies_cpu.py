"""Per-stream body measurements, the parts that need no GPU: the reference fixture ``body_traces.npz``
(tests/golden/gen_bodies.py: the reference estimators built once per bonemap), ``body9_from_bonemap``, the C entries' refusals and
the Python wrappers' argument checks."""
import ctypes as C

import numpy as np
import pytest

from oracle import ape_oracle as orc
from tests.conftest import GOLDEN


class BoneMapStandIn:
    """what the generator's stand-ins carried: the three attributes Estimator.__init__ reads from a BoneMap"""

    def __init__(self, lengths, origin):
        self.left_lower_arm_length, self.left_upper_arm_length = float(lengths[0]), float(lengths[1])
        self.left_upper_arm_origin_rh = np.array(origin, dtype=np.float64)


def stand_ins():
    """the bonemaps the reference estimators of body_traces.npz were built with (a NaN row: ``bonemap=None``, the defaults)"""
    g = np.load(GOLDEN / "body_traces.npz")
    return [None if np.isnan(ln).any() else BoneMapStandIn(ln, og) for ln, og in zip(g["bm_lengths"], g["bm_origins"])]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


@pytest.fixture(scope="module")
def traces(golden):
    return golden("body_traces.npz")


def test_body9_from_bonemap_equals_the_references_body_measurements(traces):
    from wear_mocap_ape_amd.data_types.bone_map import BoneMap, bodies_from, body9_from_bonemap
    bms = stand_ins()
    assert len(bms) == traces["bodies"].shape[0] >= 4 and bms[0] is None
    for b, bm in enumerate(bms):
        got = body9_from_bonemap(bm)
        assert got.dtype == np.float64 and got.shape == (9,)
        assert got.tobytes() == traces["bodies"][b].tobytes()                # bit for bit
        if bm is not None:                                                   # the product's own BoneMap gives the same nine values
            assert np.array_equal(body9_from_bonemap(BoneMap(bm.left_lower_arm_length, bm.left_upper_arm_length, bm.left_upper_arm_origin_rh)), got)
    assert np.array_equal(bodies_from(bms, len(bms)), traces["bodies"])
    assert np.array_equal(bodies_from(traces["bodies"], len(bms)), traces["bodies"])
    # one default body, three that differ from it in all nine values that a bonemap can change, one with a clear third origin component
    d = traces["bodies"]
    for b in range(1, len(d)):
        assert np.all(d[b, [0, 3, 6, 7, 8]] != d[0, [0, 3, 6, 7, 8]])
    assert np.abs(d[:, 8]).max() > 0.05


@pytest.mark.parametrize("name", ["pocket", "watch", "uarm"])
def test_fixture_messages_follow_from_the_stored_predictions(golden, traces, name):
    """the reference's messages per body = the oracle's post-filter over the reference's own (body-independent) stacked predictions
    of stream_trace_<name>.npz with that body, at the tolerance test_oracle_golden.test_stream_trace uses for these traces"""
    g = golden(f"stream_trace_{name}.npz")
    layout = orc.MODEL_CONFIGS[name]["layout"]
    for smooth in (1, 5):
        preds = g[f"pred_s{smooth}_mc1"]
        for b, body in enumerate(traces["bodies"]):
            for f, pred in enumerate(preds):
                est = orc.arm_pose_from_targets(pred, body[None], layout, "eigh")
                msg = np.asarray(orc.msg_with_mc_samples(orc.msg_from_est(est, body[None], layout), est, True))
                ref = traces[f"msg_{name}_s{smooth}"][b, f]
                if smooth > 1:
                    ref = np.r_[ref, traces[f"tail_{name}_s{smooth}"][b, f]]
                assert msg.shape == ref.shape
                assert np.allclose(msg, ref, rtol=0, atol=1e-11), (smooth, b, f, float(np.abs(msg - ref).max()))
    # the bodies matter: no two stand-ins share a hand origin
    m = traces[f"msg_{name}_s5"]
    for b in range(1, m.shape[0]):
        assert np.abs(m[b, :, 4:7] - m[0, :, 4:7]).min() > 1e-3


def test_fixture_fk_only_messages_against_the_host_path(golden, traces):
    """WatchPhoneUarm has a host path up to the stacked predictions (feature builder and smoothing stack of the product estimator built
    with each stand-in); the oracle's post-filter with that estimator's body turns them into the reference's messages"""
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    fk = golden("fk_only_trace.npz")
    rows = fk["rows"][:int(fk["lengths"][0])]
    for smooth in (1, 5):
        for b, bm in enumerate(stand_ins()):
            est = WatchPhoneUarm(smooth=smooth, bonemap=bm)
            assert np.array_equal(est.body_measurements.reshape(9), traces["bodies"][b])
            for f, row in enumerate(rows):
                pred = np.asarray(est.add_xx_to_row_hist_and_make_prediction(est.parse_row_to_xx(row)), dtype=np.float64)
                e = orc.arm_pose_from_targets(pred, est.body_measurements, orc.LAYOUT_ORI_CAL_LARM_UARM, "eigh")
                msg = np.asarray(orc.msg_with_mc_samples(orc.msg_from_est(e, est.body_measurements, orc.LAYOUT_ORI_CAL_LARM_UARM), e, True))
                assert np.allclose(msg[:25], traces[f"msg_fk_s{smooth}"][b, f], rtol=0, atol=1e-11)
                if smooth > 1:
                    assert np.allclose(msg[25:], traces[f"tail_fk_s{smooth}"][b, f], rtol=0, atol=1e-11)


# ---------------- the C ABI ---------------------------------------------------------------------------------------------
NEW = ("ape_streams_set_bodies", "ape_streams_get_bodies", "ape_fk_bank_set_bodies", "ape_fk_bank_get_bodies",
       "ape_kalman_bank_set_bodies", "ape_kalman_bank_get_bodies", "ape_replay_bodies", "ape_fk_replay_bodies", "ape_kalman_replay_bodies")


def test_new_entries_are_bound():
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import FkStreamBank, KalmanStreamBank, StreamBank
    for name in NEW:
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name), name
    for cls in (StreamBank, FkStreamBank, KalmanStreamBank):
        assert callable(cls.set_bodies) and isinstance(cls.bodies, property)
    assert _hip.lib().ape_abi_version() == 7
    for name in ("ape_replay", "ape_fk_replay", "ape_kalman_replay"):       # every argument of the plain entry, then the bodies
        assert _hip.SIGNATURES[name + "_bodies"][1][:-1] == _hip.SIGNATURES[name][1]


def test_body_entries_refuse_null_arguments():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)                          # never dereferenced: every call below is refused first
    idx = np.arange(4, dtype=np.int32)
    ip = C.c_void_p(idx.ctypes.data)
    vals = np.zeros((4, 9))
    vp = C.c_void_p(vals.ctypes.data)
    for kind in ("streams", "fk_bank", "kalman_bank"):
        set_fn, get_fn = getattr(lib, f"ape_{kind}_set_bodies"), getattr(lib, f"ape_{kind}_get_bodies")
        for bank, v in ((None, vp), (dummy, None)):
            assert set_fn(bank, ip, 4, v, None) != 0 and b"NULL" in lib.ape_last_error() and kind.encode() in lib.ape_last_error()
        for bank, out in ((None, vp), (dummy, None)):
            assert get_fn(bank, out) != 0 and b"NULL" in lib.ape_last_error()
    # the replays: the plain entries' refusals come first and unchanged, with or without bodies
    st = np.zeros(1, dtype=np.int32)
    sp = C.c_void_p(st.ctypes.data)
    body = np.zeros(9)
    bp = body.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ape_replay_bodies(None, 0, dummy, 0, sp, 1, 6, 1, 1, 0.0, 7, 0, dummy, _hip.F64, None, 0, None, vp) != 0
    assert b"F=0" in lib.ape_last_error()
    assert lib.ape_fk_replay_bodies(_hip.PARSE_WATCH_PHONE_UARM, dummy, 0, sp, 1, 1, bp, 0, dummy, _hip.F64, None, vp) != 0
    assert b"F=0" in lib.ape_last_error()
    assert lib.ape_fk_replay_bodies(_hip.PARSE_WATCH_PHONE_UARM, dummy, 4, sp, 1, 1, None, 0, dummy, _hip.F64, None, None) != 0
    assert b"NULL" in lib.ape_last_error()           # neither one body nor one per recording
    none4 = [None] * 4
    assert lib.ape_kalman_replay_bodies(dummy, 0, dummy, 4, sp, 1, 1, *none4, None, 7, 0, dummy, _hip.F64, dummy, None, None, None) != 0
    assert b"NULL" in lib.ape_last_error()
    assert lib.ape_kalman_replay_bodies(dummy, 0, dummy, 0, sp, 1, 1, *none4, None, 7, 0, dummy, _hip.F64, dummy, None, None, vp) != 0
    assert b"F=0" in lib.ape_last_error()


class _FakeBank:
    """the Python wrappers check their arguments before any library call: a stand-in with S = 4 and no handle"""
    _n = 4

    def __init__(self):
        from wear_mocap_ape_amd import _hip
        from wear_mocap_ape_amd.streams import StreamBank
        self._hip, self._C, self._handle = _hip, C, None
        self._indices = lambda streams: StreamBank._indices(self, streams)


@pytest.mark.parametrize("bodies,streams", [
    (np.zeros((3, 9)), None),                        # three rows for four streams
    (np.zeros((4, 8)), None),                        # eight values a row
    (np.zeros((2, 9)), [0, 1, 2]),                   # rows != listed streams
    (np.zeros((2, 9)), [1, 1]),                      # a duplicate index
    (np.zeros((1, 9)), [4]),                         # an index outside [0, S)
    ([None, None], None),                            # two bonemaps for four streams
    ([object()] * 4, None),                          # not bonemap-like
    (np.zeros((4, 9, 1)), None),
])
def test_set_bodies_wrappers_raise_for_bad_arguments(bodies, streams):
    from wear_mocap_ape_amd.streams import _set_bodies
    with pytest.raises(UserWarning):
        _set_bodies(_FakeBank(), "ape_streams_set_bodies", bodies, streams)


def test_bodies_from_accepts_values_and_bonemaps():
    from wear_mocap_ape_amd.data_types.bone_map import bodies_from, body9_from_bonemap
    bms = stand_ins()
    assert bodies_from(bms[:2], 2).shape == (2, 9)
    assert np.array_equal(bodies_from([None], 1)[0], body9_from_bonemap(None))
    assert bodies_from([[0.0] * 9] * 3, 3).shape == (3, 9)
    assert bodies_from([], 0).shape == (0, 9)
    with pytest.raises(UserWarning):
        bodies_from(bms, 3)
