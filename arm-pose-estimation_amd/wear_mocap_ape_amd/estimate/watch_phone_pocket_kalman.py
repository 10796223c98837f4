"""``WatchPhonePocketKalman`` -- the ensemble-Kalman phone-in-pocket estimator of the reference's main example script
(``estimate/watch_phone_pocket_kalman.py:12-169``, ``example_scripts/stream/watch_phone_pocket.py``): same features and
targets as ``WatchPhonePocketNN``, the regressor replaced by ``KalmanSmartwatchModel``; the corrected ensemble takes the
place of the Monte-Carlo samples.  PARITY UNPINNED (see ``estimate/kalman_models.py``)."""
import ctypes as C
from pathlib import Path

import numpy as np
import torch

from wear_mocap_ape_amd import _hip
from wear_mocap_ape_amd.data_types import messaging
from wear_mocap_ape_amd.data_types.bone_map import bodies_from
from wear_mocap_ape_amd.estimate import kalman_models
from wear_mocap_ape_amd.estimate.estimator import Estimator
from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import features_from_row
from wear_mocap_ape_amd.utility.names import NNS_INPUTS, NNS_TARGETS


class _KalmanDeviceFrame:
    """One iteration of the consumer loop as ONE call into libape_hip.so: a one-stream bank (``ape_kalman_bank_*``)
    keeps the window, the state history and the smoothing stack on the device; ``ape_kalman_bank_frame_host`` takes the raw 55-float
    message and returns the packed message row and its stacked-row count.  PARITY UNPINNED like the model it runs."""

    def __init__(self, model, smooth: int, stats, body, add_mc_samples: bool, seed: int):
        self._lib, self._model, self._seed = _hip.lib(), model, int(seed) & (2 ** 64 - 1)
        self._bank = C.c_void_p()
        _hip.check(self._lib.ape_kalman_bank_create(model.handle, 1, smooth, C.byref(self._bank)), "ape_kalman_bank_create")
        b = np.ascontiguousarray(np.asarray(body, dtype=np.float64).reshape(9))
        _hip.check(self._lib.ape_kalman_bank_set_body(self._bank, _hip.dptr(b, C.c_double)), "ape_kalman_bank_set_body")
        if stats is not None:
            self.set_norm_stats(stats)
        self.manual_seed(self._seed)
        self._flags = _hip.FLAG_PACKED_MSG if add_mc_samples else 0
        self._row = np.empty((55,), dtype=np.float32)
        self._out = np.zeros((25 + 6 * max(1, smooth) * model._num_ensemble,), dtype=np.float64)
        self._n = np.zeros((1,), dtype=np.int32)
        self._row_p, self._out_p, self._n_p = (C.c_void_p(a.ctypes.data) for a in (self._row, self._out, self._n))
        # frames with the spread record behind the row (APE_FLAG_SPREAD): a buffer of their own
        self._out_spread = np.zeros((self._out.shape[0] + _hip.SPREAD_WIDTH,), dtype=np.float64)
        self._out_spread_p = C.c_void_p(self._out_spread.ctypes.data)

    def __del__(self):
        bank, self._bank = getattr(self, "_bank", None), None
        try:
            if bank:
                self._lib.ape_kalman_bank_destroy(bank)
        except Exception:          # interpreter shutdown
            pass

    def set_norm_stats(self, stats):
        a = [np.ascontiguousarray(np.asarray(stats[k], dtype=np.float64).reshape(-1)) for k in ("xx_m", "xx_s", "yy_m", "yy_s")]
        _hip.check(self._lib.ape_kalman_bank_set_norm_stats(self._bank, *[_hip.dptr(v, C.c_double) for v in a]),
                   "ape_kalman_bank_set_norm_stats")

    def manual_seed(self, seed: int):
        self._seed = int(seed) & (2 ** 64 - 1)
        _hip.check(self._lib.ape_kalman_bank_set_seed(self._bank, self._seed), "ape_kalman_bank_set_seed")

    def reset(self):
        """cold start, and the draws start again: a reset estimator repeats its run"""
        _hip.check(self._lib.ape_kalman_bank_reset(self._bank), "ape_kalman_bank_reset")
        self.manual_seed(self._seed)

    # ---- state hand-over: the one stream of this bank as a canonical record, and the bank's draw position ----
    def get_state(self):
        from wear_mocap_ape_amd import stream_state as ss
        d = _hip.ApeKalmanStateDesc()
        _hip.check(self._lib.ape_kalman_bank_state_desc(self._bank, C.byref(d)), "ape_kalman_bank_state_desc")
        desc = {k: int(getattr(d, k)) for k in ss.KALMAN_DESC_KEYS}
        dev = self._model.torch_device
        with torch.cuda.device(dev):
            rec = torch.zeros((1, desc["words_per_stream"]), dtype=torch.float32, device=dev)
            age, idx = np.zeros((1,), dtype=np.int32), np.zeros((1,), dtype=np.int32)
            _hip.check(self._lib.ape_kalman_bank_export(self._bank, C.c_void_p(idx.ctypes.data), 1, C.c_void_p(rec.data_ptr()),
                                                        C.c_void_p(age.ctypes.data), None), "ape_kalman_bank_export")
            record = rec.cpu().numpy()[0].copy()              # (synchronises the null stream the export ran on)
        seed, calls = C.c_uint64(), C.c_uint64()
        _hip.check(self._lib.ape_kalman_bank_get_draw_position(self._bank, C.byref(seed), C.byref(calls)), "ape_kalman_bank_get_draw_position")
        return {"form": "kalman-device", "desc": desc, "record": record, "age": int(age[0]), "seed": int(seed.value),
                "calls": int(calls.value)}

    def set_state(self, state):
        from wear_mocap_ape_amd import stream_state as ss
        desc = state["desc"]
        d = _hip.ApeKalmanStateDesc(*[int(desc[k]) for k in ss.KALMAN_DESC_KEYS])
        dev = self._model.torch_device
        with torch.cuda.device(dev):
            rec = ss.kalman_records_tensor(np.asarray(state["record"], dtype=np.float32).reshape(1, -1), 1, int(d.words_per_stream), dev)
            age, idx = np.asarray([int(state["age"])], dtype=np.int32), np.zeros((1,), dtype=np.int32)
            _hip.check(self._lib.ape_kalman_bank_import(self._bank, C.byref(d), C.c_void_p(idx.ctypes.data), 1, C.c_void_p(rec.data_ptr()),
                                                        C.c_void_p(age.ctypes.data), None), "ape_kalman_bank_import")
            torch.cuda.synchronize(dev)                       # the launch has read the record before it is released
        if "seed" in state and "calls" in state:
            self._seed = int(state["seed"]) & (2 ** 64 - 1)
            _hip.check(self._lib.ape_kalman_bank_set_draw_position(self._bank, self._seed, int(state["calls"]) & (2 ** 64 - 1)),
                       "ape_kalman_bank_set_draw_position")

    def frame(self, row, spread: bool = False):
        """raw message -> (float64 packed row, stacked-row count); a view of this object's buffer, overwritten by the next frame.
        ``spread``: the row is 21 columns longer and ends in the spread record of the frame's stacked rows (a buffer of its own)"""
        self._row[:] = row
        if spread:
            _hip.check(self._lib.ape_kalman_bank_frame_host(self._bank, _hip.PARSE_WATCH_PHONE_POCKET, self._row_p,
                                                            self._flags | _hip.FLAG_SPREAD, self._out_spread_p, _hip.F64, self._n_p, None),
                       "ape_kalman_bank_frame_host")
            return (self._out_spread if self._flags else self._out_spread[:25 + _hip.SPREAD_WIDTH]), int(self._n[0])
        _hip.check(self._lib.ape_kalman_bank_frame_host(self._bank, _hip.PARSE_WATCH_PHONE_POCKET, self._row_p, self._flags, self._out_p,
                                                        _hip.F64, self._n_p, None), "ape_kalman_bank_frame_host")
        return self._out, int(self._n[0])


class WatchPhonePocketKalman(Estimator):
    def __init__(self,
                 model_path: Path,
                 smooth: int = 1,
                 num_ensemble: int = 32,
                 window_size: int = 10,
                 add_mc_samples: bool = True,
                 normalize: bool = True,
                 tag: str = "KALMAN POCKET PHONE"):
        super().__init__(
            x_inputs=NNS_INPUTS.WATCH_PHONE_CAL_HIP,
            y_targets=NNS_TARGETS.ORI_CAL_LARM_UARM_HIPS,
            smooth=smooth,
            seq_len=window_size,
            add_mc_samples=add_mc_samples,
            normalize=normalize,
            tag=tag
        )
        self.__tag = tag
        self.__slp = messaging.WATCH_PHONE_IMU_LOOKUP
        self.__num_ensemble = num_ensemble
        self.__win_size = window_size
        self.__dim_x = 14
        self.__model = kalman_models.KalmanSmartwatchModel(self.__num_ensemble, self.__win_size)
        self.__model.eval()
        # the pretrained model: the reference's checkpoint file ({"model": state_dict}, :50-54) or a ready state_dict
        if isinstance(model_path, dict):
            checkpoint = model_path if "model" in model_path else {"model": model_path}
        else:
            checkpoint = torch.load(model_path, map_location=torch.device("cpu"))
        self.__model.load_state_dict(checkpoint["model"])
        self._device = self.__model.torch_device
        self.__init_state()

    def __init_state(self):
        # the filter starts from a history of zero tensors (:57-63)
        self.__init_step = 0
        self.__input_state = torch.zeros((1, self.__num_ensemble, self.__win_size, self.__dim_x), dtype=torch.float32,
                                         device=self._device)

    def reset(self):
        super().reset()
        self.__init_state()

    model = property(lambda self: self.__model)

    # the spread record: the device frame serves it (the one-stream bank's tail kernel), the staged methods fill it from
    # ``_post.spread_rows`` like the NN classes -- so this estimator accepts the switch on either path
    @property
    def spread(self) -> bool:
        """off by default.  On: every frame also reduces its stacked rows to the 21-value spread record (``_post.spread_rows`` states
        the layout), kept for ``get_last_spread()`` -- the corrected ensemble's spread once the filter is initialised, the smoothing
        lag of the sensor means during the first W + 1 frames (origins and zeros at ``smooth`` 1); what ``process_row`` /
        ``processing_loop`` return is unchanged."""
        return self._spread

    @spread.setter
    def spread(self, on):
        self._spread = bool(on)
        if not self._spread:
            self._last_spread = None                      # no record outlives the switch

    _parse_kind = _hip.PARSE_WATCH_PHONE_POCKET

    def parse_row_to_xx(self, row):
        return features_from_row(row, self.__slp)            # the same 22 features as the LSTM estimator (:73-131)

    def make_prediction_from_row_hist(self, xx_hist):
        # -> batch size, window_size, ensembles, raw_obs (:135)
        xx_seq = torch.tensor(xx_hist, dtype=torch.float32).to(self._device)[None, :, None, :]
        output = self.__model(xx_seq, self.__input_state)
        # not enough history yet: sensor-model predictions until a time window worth of states exists (:141-156)
        if self.__init_step <= self.__win_size:
            self.__init_step += 1
            pred = self.__model.format_state(output[3][0])[None, :, None, :]       # -> bs en k dim
            self.__input_state = torch.cat((self.__input_state[:, :, 1:, :], pred), axis=2)
            return output[3].cpu().numpy()[0][:, :14]
        # initialised: the corrected ensemble is the next input state and the output (:159-169)
        ensemble = output[0]
        self.__input_state = torch.cat((self.__input_state[:, :, 1:, :], ensemble[:, :, None, :]), axis=2)
        return ensemble.cpu().numpy()[0][:, :14]

    # ---- the device-resident frame and the offline replay; PARITY UNPINNED like everything above ----------------
    frame_seed = 0x5EED        # seed of the device frame's draws (manual_seed)

    def manual_seed(self, seed: int):
        """seed of the device-resident frame's draws (flipout perturbations, signs, format_state); the call counter starts again"""
        self.frame_seed = int(seed)
        if getattr(self, "_device_frame", None) is not None:
            self._device_frame.manual_seed(seed)
        return self

    def _stats(self):
        return {"xx_m": self._xx_m, "xx_s": self._xx_s, "yy_m": self._yy_m, "yy_s": self._yy_s} if self._normalize else None

    def set_norm_stats(self, stats: dict):
        super().set_norm_stats(stats)
        if getattr(self, "_device_frame", None) is not None:
            self._device_frame.set_norm_stats(stats)

    def _frame_runner(self):
        if not self.use_device_frame:
            return None
        if getattr(self, "_device_frame", None) is None:
            self._device_frame = _KalmanDeviceFrame(self.__model, self._smooth, self._stats(), self._body_measurements,
                                                    self._add_mc_samples, self.frame_seed)
        return self._device_frame

    # ---- state hand-over ----
    def get_state(self) -> dict:
        """The estimator's history on the device-frame path: ``{"form": "kalman-device", "desc", "record", "age", "seed", "calls"}``
        -- the canonical record of its one-stream bank as float32 words on the host (``stream_state.kalman_unpack`` gives window, state
        history, stack and row counts), ``age = min(frames since the cold start, W + 1)`` and the bank's draw position.  Bodies are not
        part of it.  The staged host path (``use_device_frame = False``) keeps its history in the torch model's own tensors and has no
        such record: there this raises ``UserWarning``."""
        frame = self._frame_runner()
        if frame is None:
            raise UserWarning("WatchPhonePocketKalman.get_state needs the device frame: with use_device_frame = False the staged host "
                              "path keeps no canonical record")
        return frame.get_state()

    def set_state(self, state: dict):
        """continue from a ``get_state`` dict (of this estimator or another one, or built from a bank's ``export_state`` or a
        replay's ``return_state``): the one-stream bank imports the record and takes over the draw position when the dict carries
        ``"seed"`` and ``"calls"``, so ``process_row`` continues bit for bit.  Raises ``UserWarning`` with
        ``use_device_frame = False``."""
        frame = self._frame_runner()
        if frame is None:
            raise UserWarning("WatchPhonePocketKalman.set_state needs the device frame: with use_device_frame = False the staged host "
                              "path keeps no canonical record")
        if state.get("form") != "kalman-device":
            raise UserWarning(f"WatchPhonePocketKalman.set_state wants a 'kalman-device' state, got form {state.get('form')!r}")
        frame.set_state(state)
        if "seed" in state:
            self.frame_seed = int(state["seed"])

    def process_row(self, row):
        """one iteration of the consumer loop (estimator.py:174-177) as one ``ape_kalman_bank_frame_host`` call: the same types and
        lengths as the staged path (``use_device_frame = False``) -- 25 values while the stack holds one row, 25 + 6 n for n > 1
        stacked rows (n grows from ``smooth`` to ``smooth * num_ensemble`` once the filter is initialised)"""
        frame = self._frame_runner()
        if frame is None:
            return super().process_row(row)
        if self._spread:                          # the frame's record rides behind the row and is stripped here
            out, n = frame.frame(row, spread=True)
            self._last_spread = out[-_hip.SPREAD_WIDTH:].copy()
            out = out[:-_hip.SPREAD_WIDTH]
        else:
            out, n = frame.frame(row)
        self._last_msg = out[:25].copy()
        if not self._add_mc_samples:
            return self._last_msg.copy()
        cut = out[:25 + 6 * n] if n > 1 else out[:25]
        return cut.copy() if self.msg_as_array else cut.tolist()

    def process_recording(self, rows, starts=None, big_endian: bool = False, out_dtype=torch.float64, return_targets: bool = False,
                          seed: int = 0x5EED, bonemaps=None, state_in=None, age_in=None, return_state: bool = False, call_base: int = 0,
                          spread: bool = False):
        """rows: float32 ``[F, 55]`` raw messages of one or more recordings back to back (host array or CUDA tensor); ``starts``: the
        recordings' first rows (default ``[0]``).  Returns ``(out, n_rows)`` on the device -- for every row what ``process_row`` of a
        fresh estimator with ``manual_seed(seed)`` fed that recording returns (no row skipped; several recordings share the flipout
        draw of a frame, ``ape_kalman_replay``): ``out`` is ``[F, 25 + 6 * smooth * num_ensemble]`` with ``add_mc_samples`` (message,
        hand and elbow xyz of the ``n_rows[f]`` stacked rows, zeros; ``streams.trim_packed`` cuts a row), else ``[F, 25]``.  With
        ``return_targets`` also the normalised predictions float32 ``[F, num_ensemble, 14]`` (row 0 alone on a recording's first
        W + 1 frames).  ``bonemaps``: one entry per recording (bonemap-like objects, ``None``, or float64 ``[R, 9]`` values): every
        recording as by an estimator built with its bonemap (``ape_kalman_replay_bodies``); default: this
        estimator's body for all.

        Resumable (``ape_kalman_replay_resume``): ``state_in`` float32 words ``[R, words]`` and ``age_in`` int32
        ``[R]`` (from an earlier call's ``return_state``, a bank's ``export_state`` or ``get_state``) continue every recording with
        age > 0 instead of starting it cold; ``return_state`` appends ``(state, age)`` -- the records after each recording's last
        frame on the device and their ages -- to the result; ``call_base`` is the number of frames the recordings have already been
        through: pieces ``[0, a), [a, b), ...`` of one recording that chain state and age with ``call_base = a, b, ...`` return the
        rows of the one call, device draws included (several recordings: when every piece lists the same recordings cut at the same
        offsets).

        ``spread`` (``APE_FLAG_SPREAD``): the result becomes ``(out, n_rows, spread)`` (``(out, n_rows, y, spread)``
        with ``return_targets``; the state / age pair stays last) with ``spread`` ``[F, 21]`` of ``out_dtype``, every frame's spread
        record over its ``n_rows[f]`` stacked rows (``_post.spread_rows``); ``out`` and ``spread`` are views of one wider device
        tensor.  Chained pieces give the records of the one call."""
        if out_dtype not in (torch.float32, torch.float64):
            raise UserWarning(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
        model = self.__model
        dev = model.torch_device
        with torch.cuda.device(dev):
            rd = torch.as_tensor(rows, dtype=torch.float32).to(dev).contiguous()
            if rd.dim() != 2 or rd.shape[1] != 55 or rd.shape[0] < 1:
                raise UserWarning(f"expected rows [F>=1,55], got {tuple(rd.shape)}")
            F = int(rd.shape[0])
            st = np.ascontiguousarray(np.asarray([0] if starts is None else starts, dtype=np.int32).reshape(-1))
            packed = bool(self._add_mc_samples)
            out = torch.empty((F, (25 + 6 * self._smooth * self.__num_ensemble if packed else 25) + (_hip.SPREAD_WIDTH if spread else 0)),
                              dtype=out_dtype, device=dev)
            n_rows = torch.empty((F,), dtype=torch.int32, device=dev)
            y = torch.empty((F, self.__num_ensemble, 14), dtype=torch.float32, device=dev) if return_targets else None
            stats = self._stats()
            sp = [None] * 4 if stats is None else [_hip.dptr(np.ascontiguousarray(stats[k], dtype=np.float64), C.c_double)
                                                   for k in ("xx_m", "xx_s", "yy_m", "yy_s")]
            body = np.ascontiguousarray(self._body_measurements.reshape(9), dtype=np.float64)
            kind = _hip.PARSE_WATCH_PHONE_POCKET | (_hip.PARSE_BIG_ENDIAN if big_endian else 0)
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            bodies = None if bonemaps is None else bodies_from(bonemaps, int(st.shape[0]), "process_recording bonemaps")
            R = int(st.shape[0])
            from wear_mocap_ape_amd import stream_state as ss
            words = ss.kalman_words(self.__num_ensemble, self.__win_size, max(1, self._smooth))
            if (state_in is None) != (age_in is None):
                raise UserWarning("process_recording wants state_in and age_in together")
            s_in = a_in = s_out = a_out = None
            if state_in is not None:
                s_in = ss.kalman_records_tensor(state_in, R, words, dev)
                a_in = np.ascontiguousarray(np.asarray(age_in, dtype=np.int32).reshape(-1))
                if a_in.shape[0] != R:
                    raise UserWarning(f"process_recording wants {R} ages, got {a_in.shape[0]}")
            if return_state:
                s_out = torch.zeros((R, words), dtype=torch.float32, device=dev)
                a_out = np.zeros((R,), dtype=np.int32)
            vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
            ap = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None         # noqa: E731
            args = (model.handle, kind, C.c_void_p(rd.data_ptr()), F, C.c_void_p(st.ctypes.data), R, self._smooth, *sp,
                    _hip.dptr(body, C.c_double), int(seed) & (2 ** 64 - 1),
                    (_hip.FLAG_PACKED_MSG if packed else 0) | (_hip.FLAG_SPREAD if spread else 0),
                    C.c_void_p(out.data_ptr()), _hip.F64 if out_dtype == torch.float64 else _hip.F32, C.c_void_p(n_rows.data_ptr()),
                    C.c_void_p(y.data_ptr()) if y is not None else None, stream,
                    C.c_void_p(bodies.ctypes.data) if bodies is not None else None)
            if s_in is None and s_out is None and not call_base:
                _hip.check(_hip.lib().ape_kalman_replay_bodies(*args), "ape_kalman_replay_bodies")
            else:
                _hip.check(_hip.lib().ape_kalman_replay_resume(*args, vp(s_in), ap(a_in), vp(s_out), ap(a_out), int(call_base) & (2 ** 64 - 1)),
                           "ape_kalman_replay_resume")
        rec = None
        if spread:
            out, rec = out[:, :-_hip.SPREAD_WIDTH], out[:, -_hip.SPREAD_WIDTH:]
        res = (out, n_rows, y) if return_targets else (out, n_rows)
        if spread:
            res = res + (rec,)
        return res + (s_out, a_out) if return_state else res

    def score_recording(self, out, truth, spread=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", lags=None, rec_lags=None):
        """``Estimator.score_recording`` for Kalman replays: ``skip`` defaults to the ``window_size + 1`` frames every recording runs on
        its first row alone, whose spread records have no usable covariance"""
        return super().score_recording(out, truth, spread, starts, self.__win_size + 1 if skip is None else skip, bonemaps, truth_kind, lags,
                                       rec_lags)

    def error_distribution(self, out, truth, spread=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", rec_lags=None,
                           edges=None, bins=64):
        """``Estimator.error_distribution`` for Kalman replays (``skip`` defaults to ``window_size + 1``, as in ``score_recording``)"""
        return super().error_distribution(out, truth, spread, starts, self.__win_size + 1 if skip is None else skip, bonemaps, truth_kind,
                                          rec_lags, edges, bins)

    def motion_recording(self, out, starts=None, skip=None, times=None, per_frame=False):
        """``Estimator.motion_recording`` for Kalman replays (``skip`` defaults to ``window_size + 1``, as in ``score_recording``)"""
        return super().motion_recording(out, starts, self.__win_size + 1 if skip is None else skip, times, per_frame)

    def truth_motion(self, truth, truth_kind="targets", starts=None, skip=None, times=None, bonemaps=None):
        """``Estimator.truth_motion`` for Kalman replays (``skip`` defaults to ``window_size + 1``, as in ``score_recording``)"""
        return super().truth_motion(truth, truth_kind, starts, self.__win_size + 1 if skip is None else skip, times, bonemaps)

    def spectrum_recording(self, out, truth=None, starts=None, skip=None, truth_kind="est", bonemaps=None, n=256, hop=None, taper="hann",
                           rate=1.0):
        """``Estimator.spectrum_recording`` for Kalman replays (``skip`` defaults to ``window_size + 1``, as in ``motion_recording``)"""
        return super().spectrum_recording(out, truth, starts, self.__win_size + 1 if skip is None else skip, truth_kind, bonemaps, n, hop,
                                          taper, rate)

    def angles_recording(self, out, truth=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", rec_lags=None,
                         per_frame=False, min_swing=0.05):
        """``Estimator.angles_recording`` for Kalman replays (``skip`` defaults to ``window_size + 1``, as in ``score_recording``)"""
        return super().angles_recording(out, truth, starts, self.__win_size + 1 if skip is None else skip, bonemaps, truth_kind, rec_lags,
                                        per_frame, min_swing)

    def truth_angles(self, truth, truth_kind="targets", starts=None, skip=None, bonemaps=None, per_frame=False, min_swing=0.05):
        """``Estimator.truth_angles`` for Kalman replays (``skip`` defaults to ``window_size + 1``, as in ``score_recording``)"""
        return super().truth_angles(truth, truth_kind, starts, self.__win_size + 1 if skip is None else skip, bonemaps, per_frame, min_swing)

    def errors_by(self, out, truth, by, spread=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", rec_lags=None,
                  edges=None, bins=36, times=None):
        """``Estimator.errors_by`` for Kalman replays (``skip`` defaults to ``window_size + 1``, as in ``score_recording``)"""
        return super().errors_by(out, truth, by, spread, starts, self.__win_size + 1 if skip is None else skip, bonemaps, truth_kind, rec_lags,
                                 edges, bins, times)

    def align_recording(self, out, truth, spread=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", lags=(0, 0), mode="yaw",
                        weights=(1, 1, 1, 0, 0)):
        """``Estimator.align_recording`` for Kalman replays (``skip`` defaults to ``window_size + 1``, as in ``score_recording``)"""
        return super().align_recording(out, truth, spread, starts, self.__win_size + 1 if skip is None else skip, bonemaps, truth_kind, lags,
                                       mode, weights)

    def fit_bodies(self, out, truth, starts=None, skip=None, truth_kind="est", lags=(0, 0), rec_lags=None, quats=None, mode="vectors",
                   weights=(1, 1), bonemaps=None):
        """``Estimator.fit_bodies`` for Kalman replays (``skip`` defaults to ``window_size + 1``, as in ``score_recording``)"""
        return super().fit_bodies(out, truth, starts, self.__win_size + 1 if skip is None else skip, truth_kind, lags, rec_lags, quats, mode,
                                  weights, bonemaps)

    def truth_on_frames(self, rows, truth, truth_times, truth_starts=None, starts=None, shifts=None, max_gap: float = 0.0,
                        truth_kind="targets", bonemaps=None, big_endian: bool = False):
        """``Estimator.truth_on_frames`` for raw ``[F, 28]`` pocket rows"""
        return super().truth_on_frames(rows, truth, truth_times, truth_starts, starts, shifts, max_gap, truth_kind, bonemaps, big_endian)
