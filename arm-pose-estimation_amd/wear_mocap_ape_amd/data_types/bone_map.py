"""Arm measurements used by the forward-kinematics post-filter.

Only the nine floats of ``Estimator.body_measurements`` are on the hot path (reference
``estimate/estimator.py:57-68``).  The defaults below are the reference's
``data_types/bone_map.py:42-45``; a ``BoneMap`` can also be built from explicit measurements.
Parsing a mocap skeleton XML (bone_map.py:47-99) is host-side configuration and out of scope."""
import numpy as np


class BoneMap:
    DEFAULT_LARM_LEN = 0.22
    DEFAULT_UARM_LEN = 0.26
    # default left shoulder origin relative to hip
    DEFAULT_UARM_ORIG_RH = np.array([-0.1704612, 0.4309841, -0.00670862])

    def __init__(self, left_lower_arm_length: float = DEFAULT_LARM_LEN,
                 left_upper_arm_length: float = DEFAULT_UARM_LEN,
                 left_upper_arm_origin_rh=None):
        self._larm_len = float(left_lower_arm_length)
        self._uarm_len = float(left_upper_arm_length)
        self._uarm_orig = np.array(self.DEFAULT_UARM_ORIG_RH if left_upper_arm_origin_rh is None
                                   else left_upper_arm_origin_rh, dtype=np.float64)

    @property
    def left_lower_arm_length(self):
        return self._larm_len

    @property
    def left_upper_arm_length(self):
        return self._uarm_len

    @property
    def left_upper_arm_origin_rh(self):
        return self._uarm_orig


def body9_from_bonemap(bonemap=None) -> np.ndarray:
    """float64 ``[9]`` = ``[larm_vec, uarm_vec, uarm_orig_rh]`` of ``Estimator.body_measurements`` (reference
    ``estimate/estimator.py:57-68``: both arm bones point along -x) from an object with ``left_lower_arm_length``,
    ``left_upper_arm_length`` and ``left_upper_arm_origin_rh``; ``None``: the defaults.  The one place that does this: estimators,
    banks and the per-stream body tables all take their nine values from here."""
    larm = BoneMap.DEFAULT_LARM_LEN if bonemap is None else bonemap.left_lower_arm_length
    uarm = BoneMap.DEFAULT_UARM_LEN if bonemap is None else bonemap.left_upper_arm_length
    orig = BoneMap.DEFAULT_UARM_ORIG_RH if bonemap is None else bonemap.left_upper_arm_origin_rh
    return np.ascontiguousarray(np.r_[[-larm, 0, 0], [-uarm, 0, 0], orig], dtype=np.float64)


def bodies_from(bodies, n: int, what: str = "bodies") -> np.ndarray:
    """float64 ``[n, 9]`` from a float array ``[n, 9]`` or a sequence of ``n`` bonemap-like objects / ``None`` (``body9_from_bonemap``);
    ``UserWarning`` for any other length or shape"""
    is_array = isinstance(bodies, np.ndarray) or (hasattr(bodies, "__len__") and len(bodies) > 0 and
                                                   all(isinstance(b, (list, tuple, np.ndarray)) for b in bodies))
    if is_array:
        try:
            a = np.ascontiguousarray(np.asarray(bodies, dtype=np.float64))
        except (TypeError, ValueError):
            raise UserWarning(f"{what}: expected float values [{n},9] or {n} bonemaps")
    else:
        try:
            a = np.stack([body9_from_bonemap(b) for b in bodies]) if len(bodies) else np.zeros((0, 9))
        except (TypeError, AttributeError):
            raise UserWarning(f"{what}: expected float values [{n},9] or {n} bonemaps")
    if a.ndim != 2 or a.shape[1] != 9 or a.shape[0] != n:
        raise UserWarning(f"{what}: expected [{n},9] values or {n} bonemaps, got shape {tuple(a.shape)}")
    return a
