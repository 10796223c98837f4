"""The Monte-Carlo spread record without a GPU: the constants of the C ABI, the binding, the numpy statement
`estimate/_post.spread_rows` on constructed stacks, the estimator's switch and the refusals that need no device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
HIPS, WATCH, POS = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def _quat_about(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def _stack(layout, n, rng):
    """n finite est rows of the layout with unit quaternions, and a message whose quaternions are row 0's"""
    W = 14 if layout == WATCH else 21
    est = rng.normal(size=(n, W))
    for c in ((6, 10) if layout == WATCH else (9, 13, 17)):
        est[:, c:c + 4] /= np.linalg.norm(est[:, c:c + 4], axis=1, keepdims=True)
    msg = np.zeros(25)
    msg[21:25] = [1.0, 0.0, 0.0, 0.0]
    for k, c in enumerate((6, 10) if layout == WATCH else (9, 13, 17)):
        msg[7 + 7 * k:11 + 7 * k] = est[0, c:c + 4]
    return est, msg


def test_header_constants_and_binding():
    from wear_mocap_ape_amd import _hip
    text = (REPO / "include" / "ape_hip.h").read_text()
    assert re.search(r"^#define APE_SPREAD_WIDTH 21\s*$", text, flags=re.M)
    flag = re.search(r"^#define APE_FLAG_SPREAD\s+(0x[0-9a-fA-F]+)u", text, flags=re.M)
    assert flag and int(flag.group(1), 16) == _hip.FLAG_SPREAD == 0x40
    # the bit is free: no other public flag or selector uses it
    others = {n: int(v, 16) for n, v in re.findall(r"^#define (APE_FLAG_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+)u", text, flags=re.M) if n != "APE_FLAG_SPREAD"}
    assert others and all(v & 0x40 == 0 for v in others.values()), others
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M)
    assert _hip.lib().ape_abi_version() == 7 and _hip.SPREAD_WIDTH == 21
    assert "ape_spread_reduce" in _hip.SIGNATURES and hasattr(_hip.lib(), "ape_spread_reduce")
    # the header says where the rows come from and that the record itself has no counterpart
    assert "estimator.py:112-118" in text and "estimator.py:122-137" in text and "compose_msg.py:48-108" in text
    assert "NO counterpart of this record" in text and "compose_msg.py:54-61" in text


@pytest.mark.parametrize("theta", [1e-3, 1e-2, 0.1, 0.5, 1.0, 2.0])
def test_rotations_by_plus_minus_theta_give_theta(theta):
    """rows that are qm rotated by +-theta about one axis: every row is at angle theta from qm, so the spread is theta"""
    from wear_mocap_ape_amd.estimate._post import spread_rows
    rng = np.random.default_rng(3)
    est, msg = _stack(HIPS, 8, rng)
    qm = [_quat_about(rng.normal(size=3), rng.uniform(0.2, 2.5)) for _ in range(3)]
    for k, c in enumerate((9, 13, 17)):
        msg[7 + 7 * k:11 + 7 * k] = qm[k]
        for i in range(8):
            q = _qmul(qm[k], _quat_about([0.3, -1.0, 0.5], theta if i % 2 else -theta))
            est[i, c:c + 4] = q if i % 3 else -q          # the sign of a row does not matter
    out = spread_rows(est, msg, HIPS)
    # sin^2(theta/2) is reproduced to a few ulp of 1 (the 1 - x cancellation): the angle to ~1e-16 / sin(theta)
    assert np.abs(np.sin(out[18:21] / 2) ** 2 - np.sin(theta / 2) ** 2).max() < 8 * 2.0 ** -53 * 8
    assert np.abs(out[18:21] - theta).max() < 1e-12 / theta


def test_known_point_set_gives_its_covariance():
    from wear_mocap_ape_amd.estimate._post import spread_rows
    rng = np.random.default_rng(5)
    est, msg = _stack(HIPS, 4, rng)
    est[:, 0:3] = [[0, 0, 0], [2, 0, 0], [0, 4, 0], [2, 4, 8]]              # mean (1, 2, 2)
    est[:, 3:6] = [[1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1]]
    out = spread_rows(est, msg, HIPS)
    assert np.array_equal(out[0:3], [1.0, 2.0, 2.0]) and np.array_equal(out[9:12], [1.0, 1.0, 1.0])
    assert np.array_equal(out[3:9], [1.0, 0.0, 2.0, 4.0, 4.0, 12.0])        # xx xy xz yy yz zz, divisor 1/N
    assert np.array_equal(out[12:18], np.zeros(6))
    # against numpy's own population covariance on a random set, every layout
    for layout in (HIPS, WATCH, POS):
        est, msg = _stack(layout, 37, rng)
        out = spread_rows(est, msg, layout)
        iu = np.triu_indices(3)
        assert np.allclose(out[3:9], np.cov(est[:, 0:3].T, bias=True)[iu], rtol=0, atol=1e-14)
        assert np.allclose(out[12:18], np.cov(est[:, 3:6].T, bias=True)[iu], rtol=0, atol=1e-14)
        assert np.array_equal(out[0:3], est[:, 0:3].mean(axis=0)) and out.shape == (21,) and out.dtype == np.float64


def test_single_row_and_watch_layout_rules():
    from wear_mocap_ape_amd.estimate._post import spread_rows
    rng = np.random.default_rng(7)
    for layout in (HIPS, WATCH, POS):
        est, msg = _stack(layout, 1, rng)
        msg[7:11] = [0.0, 1.0, 0.0, 0.0]                  # whatever the message says: zeros by rule, not by arithmetic
        out = spread_rows(est, msg, layout)
        assert np.array_equal(out[0:3], est[0, 0:3]) and np.array_equal(out[9:12], est[0, 3:6])
        assert np.array_equal(out[3:9], np.zeros(6)) and np.array_equal(out[12:21], np.zeros(9))
    est, msg = _stack(WATCH, 9, rng)
    out = spread_rows(est, msg, WATCH)
    assert out[20] == 0.0 and out[18] > 0.0 and out[19] > 0.0
    est, msg = _stack(HIPS, 9, rng)
    assert spread_rows(est, msg, HIPS)[20] > 0.0


def test_nan_row_propagates_like_numpy():
    from wear_mocap_ape_amd.estimate._post import spread_rows
    rng = np.random.default_rng(9)
    est, msg = _stack(HIPS, 6, rng)
    ref = spread_rows(est, msg, HIPS)
    est[2, 0] = np.nan                                    # hand x of one row
    out = spread_rows(est, msg, HIPS)
    touched = np.zeros(21, dtype=bool)
    touched[[0, 3, 4, 5]] = True                          # mean x; xx, xy, xz
    assert np.isnan(out[touched]).all() and np.array_equal(out[~touched], ref[~touched])
    est, msg = _stack(HIPS, 6, rng)
    est[4, 13:17] = np.nan                                # one upper-arm quaternion
    out = spread_rows(est, msg, HIPS)
    assert np.isnan(out[19]) and np.isfinite(np.delete(out, 19)).all()


def test_spread_rows_refuses_bad_shapes():
    from wear_mocap_ape_amd.estimate._post import spread_rows
    with pytest.raises(UserWarning):
        spread_rows(np.zeros((3, 14)), np.zeros(25), HIPS)          # watch rows, hips layout
    with pytest.raises(UserWarning):
        spread_rows(np.zeros((0, 21)), np.zeros(25), HIPS)
    with pytest.raises(UserWarning):
        spread_rows(np.zeros((3, 21)), np.zeros(24), HIPS)
    with pytest.raises(UserWarning):
        spread_rows(np.zeros((3, 21)), np.zeros(25), 5)


def test_estimator_switch_defaults_off():
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.estimate.watch_only import WatchOnlyNN
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import WatchPhonePocketNN
    from wear_mocap_ape_amd.estimate.watch_phone_uarm_nn import WatchPhoneUarmNN
    from wear_mocap_ape_amd.utility.names import NNS_INPUTS, NNS_TARGETS
    for cls in (Estimator, WatchPhonePocketNN, WatchOnlyNN, WatchPhoneUarmNN):
        assert isinstance(cls.spread, property) and callable(cls.get_last_spread)

    class Plain(Estimator):                               # no HIP regressor: the record is not served
        def make_prediction_from_row_hist(self, xx_hist):
            return xx_hist

        def parse_row_to_xx(self, row):
            return row
    est = Plain(NNS_INPUTS.WATCH_PHONE_CAL_HIP, NNS_TARGETS.ORI_CAL_LARM_UARM_HIPS, normalize=False)
    assert est.spread is False and est.get_last_spread() is None
    est.spread = False                                    # switching it off is always fine
    with pytest.raises(UserWarning, match="spread"):
        est.spread = True
    assert est.spread is False


def test_c_abi_refusals_without_a_device():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)                               # never dereferenced: every call below is refused first
    assert lib.ape_spread_reduce(None, dummy, 3, dummy, dummy, None) != 0 and b"spread_reduce" in lib.ape_last_error()
    # the regressor entries keep refusing the bit
    assert lib.ape_lstm_forward(None, dummy, 1, 6, _hip.FLAG_SPREAD, None, 0.0, 0, dummy, None) != 0
    assert lib.ape_infer(dummy, dummy, 1, 6, _hip.FLAG_SPREAD, None, dummy, _hip.F64, None) != 0
    assert b"infer" in lib.ape_last_error()
    # the replay accepts it (the refusal names another argument) and still refuses undeclared bits
    st = np.zeros(1, dtype=np.int32)

    def replay(flags, F):
        return lib.ape_replay(None, 0, dummy, F, C.c_void_p(st.ctypes.data), 1, 6, 1, 1, 0.0, 7, flags, dummy, _hip.F64, None, 0, None)
    assert replay(_hip.FLAG_SPREAD | _hip.FLAG_PACKED_MSG, 0) != 0 and b"F=0" in lib.ape_last_error()
    assert replay(_hip.FLAG_SPREAD | 0x80, 10) != 0 and b"SPREAD" in lib.ape_last_error()
