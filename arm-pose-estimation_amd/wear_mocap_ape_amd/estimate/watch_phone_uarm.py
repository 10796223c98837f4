"""``WatchPhoneUarm`` -- watch on the wrist + phone strapped to the upper arm, no regressor (reference
``estimate/watch_phone_uarm.py:10-108``): the calibrated orientations of both devices ARE the arm's orientations, so a frame
is the feature builder, the two 6D columns as the 12 targets, the smoothing stack and forward kinematics.

``process_row`` / ``processing_loop`` run one call per frame into a one-stream FK bank (``ape_fk_bank_frame_host``,
DESIGN.md 4.22); ``process_recording`` replays whole recordings (``ape_fk_replay``).  The staged methods keep the
reference's semantics for callers and subclasses that use them one by one."""
import ctypes as C

import numpy as np
import torch

from wear_mocap_ape_amd import _hip
from wear_mocap_ape_amd.data_types import messaging
from wear_mocap_ape_amd.data_types.bone_map import BoneMap, bodies_from
from wear_mocap_ape_amd.estimate.estimator import Estimator
from wear_mocap_ape_amd.estimate.watch_phone_uarm_nn import _LARM_DST_G, _LEFT_HAND_CAL, _UARM_DST_G, features_from_row
from wear_mocap_ape_amd.utility import transformations as ts
from wear_mocap_ape_amd.utility.names import NNS_INPUTS, NNS_TARGETS


def _body9(body) -> np.ndarray:
    b = np.ascontiguousarray(np.asarray(body, dtype=np.float64).reshape(-1))
    if b.size != 9:
        raise UserWarning("body_measurements must be [1,9]: larm_vec, uarm_vec, uarm_orig_rh")
    return b


class _FkFrame:
    """One iteration of the consumer loop (estimator.py:174-177) as ONE call into libape_hip.so: a one-stream FK bank keeps the
    smoothing stack on the device, ``ape_fk_bank_frame_host`` takes the raw 55-float message and returns the float64 message."""

    def __init__(self, smooth: int, body, device: int):
        self._lib = _hip.lib()
        self._body = _body9(body)
        self._bank = C.c_void_p()
        _hip.check(self._lib.ape_fk_bank_create(1, int(smooth), _hip.dptr(self._body, C.c_double), int(device), C.byref(self._bank)),
                   "ape_fk_bank_create")
        self._row = np.empty((55,), dtype=np.float32)
        self._out = np.empty((25,), dtype=np.float64)
        self._row_p = C.c_void_p(self._row.ctypes.data)
        self._out_p = C.c_void_p(self._out.ctypes.data)

    def __del__(self):
        bank, self._bank = getattr(self, "_bank", None), None
        try:
            if bank:
                self._lib.ape_fk_bank_destroy(bank)
        except Exception:          # interpreter shutdown
            pass

    def reset(self):
        _hip.check(self._lib.ape_fk_bank_reset(self._bank), "ape_fk_bank_reset")

    def frame(self, row) -> np.ndarray:
        """raw message -> float64 [25] (a view of this object's buffer, overwritten by the next frame)"""
        self._row[:] = row                       # array('f') (stream/listener/imu.py:68-70), list or ndarray
        _hip.check(self._lib.ape_fk_bank_frame_host(self._bank, _hip.PARSE_WATCH_PHONE_UARM, self._row_p, self._out_p, _hip.F64, None),
                   "ape_fk_bank_frame_host")
        return self._out


class WatchPhoneUarm(Estimator):
    def __init__(self,
                 smooth: int = 5,
                 tag: str = "Forward Kinematics",
                 bonemap: BoneMap = None):
        super().__init__(
            x_inputs=NNS_INPUTS.WATCH_PHONE_CAL_ALL,
            y_targets=NNS_TARGETS.ORI_CAL_LARM_UARM,
            smooth=smooth,
            normalize=False,
            seq_len=1,
            add_mc_samples=False,
            tag=tag,
            bonemap=bonemap
        )
        self.__tag = tag
        self.__slp = messaging.WATCH_PHONE_IMU_LOOKUP

    _parse_kind = _hip.PARSE_WATCH_PHONE_UARM

    def calibrate_orientation_quats(self, sw_quat: np.array, sw_fwd: np.array, ph_quat: np.array,
                                    ph_fwd: np.array) -> (np.array, np.array):
        """both devices' orientations in the global frame, offset to the calibration pose (left arm forward):
        (watch = lower arm, phone = upper arm), watch_phone_uarm.py:32-57"""
        north = ts.quat_mul(_LEFT_HAND_CAL, ts.north_quat_from_forward(np.asarray(sw_fwd, dtype=np.float64)))

        def calibrated(rot, fwd, dst_g):
            rot_g = ts.android_to_global(np.asarray(rot, dtype=np.float64), north)
            fwd_g = ts.android_to_global(np.asarray(fwd, dtype=np.float64), north)
            return ts.quat_mul(rot_g, ts.quat_mul(ts.quat_invert(fwd_g), dst_g))

        return calibrated(sw_quat, sw_fwd, _LARM_DST_G), calibrated(ph_quat, ph_fwd, _UARM_DST_G)

    def parse_row_to_xx(self, row: np.array):
        return features_from_row(row, self.__slp)

    def make_prediction_from_row_hist(self, row_hist):
        # the watch's and the phone's calibrated 6D columns are the targets (watch_phone_uarm.py:107-108)
        return np.c_[row_hist[:, 13:19], row_hist[:, -6:]]

    def _frame_runner(self):
        """the one-stream FK bank of process_row (no regressor: the base class's NN frame does not apply)"""
        if not self.use_device_frame:
            return None
        if getattr(self, "_device_frame", None) is None:
            self._device_frame = _FkFrame(self._smooth, self._body_measurements, torch.cuda.current_device())
        return self._device_frame

    def process_recording(self, rows, starts=None, big_endian: bool = False, out_dtype=torch.float64, bonemaps=None):
        """rows: float32 ``[F, 55]`` raw messages of one or more recordings back to back (host array or CUDA tensor);
        ``starts``: the recordings' first rows (default ``[0]``).  Returns, on the device, ``[F, 25]``: what ``process_row``
        of a fresh estimator fed each recording in order returns for every row (``ape_fk_replay``, blocking).  ``bonemaps``: one
        entry per recording (bonemap-like objects, ``None``, or float64 ``[R, 9]`` values): every recording as by an estimator built
        with its bonemap (``ape_fk_replay_bodies``); default: this estimator's body for all."""
        if out_dtype not in (torch.float32, torch.float64):
            raise UserWarning(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
        if isinstance(rows, torch.Tensor) and rows.is_cuda:
            dev = rows.device
        else:
            dev = torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(dev):
            rd = torch.as_tensor(rows, dtype=torch.float32).to(dev).contiguous()
            if rd.dim() != 2 or rd.shape[1] != 55 or rd.shape[0] < 1:
                raise UserWarning(f"expected rows [F>=1,55], got {tuple(rd.shape)}")
            F = int(rd.shape[0])
            st = np.ascontiguousarray(np.asarray([0] if starts is None else starts, dtype=np.int32).reshape(-1))
            out = torch.empty((F, 25), dtype=out_dtype, device=dev)
            body = _body9(self._body_measurements)
            kind = self._parse_kind | (_hip.PARSE_BIG_ENDIAN if big_endian else 0)
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            bodies = None if bonemaps is None else bodies_from(bonemaps, int(st.shape[0]), "process_recording bonemaps")
            _hip.check(_hip.lib().ape_fk_replay_bodies(kind, C.c_void_p(rd.data_ptr()), F, C.c_void_p(st.ctypes.data), int(st.shape[0]),
                                                       self._smooth, _hip.dptr(body, C.c_double), dev.index, C.c_void_p(out.data_ptr()),
                                                       _hip.F64 if out_dtype == torch.float64 else _hip.F32, stream,
                                                       C.c_void_p(bodies.ctypes.data) if bodies is not None else None), "ape_fk_replay_bodies")
        return out

    def score_recording(self, out, truth, spread=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", lags=None, rec_lags=None):
        """``Estimator.score_recording`` for ``[F, 25]`` FK replays (no cold-start frames: ``skip`` defaults to 0; no spread record)"""
        return super().score_recording(out, truth, spread, starts, 0 if skip is None else skip, bonemaps, truth_kind, lags, rec_lags)

    def error_distribution(self, out, truth, spread=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", rec_lags=None,
                           edges=None, bins=64):
        """``Estimator.error_distribution`` for ``[F, 25]`` FK replays (``skip`` defaults to 0, as in ``score_recording``)"""
        return super().error_distribution(out, truth, spread, starts, 0 if skip is None else skip, bonemaps, truth_kind, rec_lags, edges, bins)

    def motion_recording(self, out, starts=None, skip=None, times=None, per_frame=False):
        """``Estimator.motion_recording`` for ``[F, 25]`` FK replays (``skip`` defaults to 0, as in ``score_recording``)"""
        return super().motion_recording(out, starts, 0 if skip is None else skip, times, per_frame)

    def truth_motion(self, truth, truth_kind="targets", starts=None, skip=None, times=None, bonemaps=None):
        """``Estimator.truth_motion`` for FK replays (``skip`` defaults to 0, as in ``score_recording``)"""
        return super().truth_motion(truth, truth_kind, starts, 0 if skip is None else skip, times, bonemaps)

    def spectrum_recording(self, out, truth=None, starts=None, skip=None, truth_kind="est", bonemaps=None, n=256, hop=None, taper="hann",
                           rate=1.0):
        """``Estimator.spectrum_recording`` for ``[F, 25]`` FK replays (``skip`` defaults to 0, as in ``motion_recording``)"""
        return super().spectrum_recording(out, truth, starts, 0 if skip is None else skip, truth_kind, bonemaps, n, hop, taper, rate)

    def angles_recording(self, out, truth=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", rec_lags=None,
                         per_frame=False, min_swing=0.05):
        """``Estimator.angles_recording`` for ``[F, 25]`` FK replays (``skip`` defaults to 0, as in ``score_recording``)"""
        return super().angles_recording(out, truth, starts, 0 if skip is None else skip, bonemaps, truth_kind, rec_lags, per_frame, min_swing)

    def truth_angles(self, truth, truth_kind="targets", starts=None, skip=None, bonemaps=None, per_frame=False, min_swing=0.05):
        """``Estimator.truth_angles`` for FK replays (``skip`` defaults to 0, as in ``score_recording``)"""
        return super().truth_angles(truth, truth_kind, starts, 0 if skip is None else skip, bonemaps, per_frame, min_swing)

    def errors_by(self, out, truth, by, spread=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", rec_lags=None,
                  edges=None, bins=36, times=None):
        """``Estimator.errors_by`` for ``[F, 25]`` FK replays (``skip`` defaults to 0, as in ``score_recording``)"""
        return super().errors_by(out, truth, by, spread, starts, 0 if skip is None else skip, bonemaps, truth_kind, rec_lags, edges, bins, times)

    def align_recording(self, out, truth, spread=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", lags=(0, 0), mode="yaw",
                        weights=(1, 1, 1, 0, 0)):
        """``Estimator.align_recording`` for ``[F, 25]`` FK replays (``skip`` defaults to 0, as in ``score_recording``)"""
        return super().align_recording(out, truth, spread, starts, 0 if skip is None else skip, bonemaps, truth_kind, lags, mode, weights)

    def fit_bodies(self, out, truth, starts=None, skip=None, truth_kind="est", lags=(0, 0), rec_lags=None, quats=None, mode="vectors",
                   weights=(1, 1), bonemaps=None):
        """``Estimator.fit_bodies`` for ``[F, 25]`` FK replays (``skip`` defaults to 0, as in ``score_recording``)"""
        return super().fit_bodies(out, truth, starts, 0 if skip is None else skip, truth_kind, lags, rec_lags, quats, mode, weights, bonemaps)

    def truth_on_frames(self, rows, truth, truth_times, truth_starts=None, starts=None, shifts=None, max_gap: float = 0.0,
                        truth_kind="targets", bonemaps=None, big_endian: bool = False):
        """``Estimator.truth_on_frames`` for raw ``[F, 55]`` watch-and-phone rows"""
        return super().truth_on_frames(rows, truth, truth_times, truth_starts, starts, shifts, max_gap, truth_kind, bonemaps, big_endian)
