"""``Estimator`` base class with the reference's template-method contract
(``estimate/estimator.py:16-218``): window history with pad-by-newest cold start, z-score /
de-normalise bookkeeping in float64, smoothing stack, FK + message, consumer-thread loop.

Host side keeps only bookkeeping (list membership and order -- compared bit-exactly against the
reference in the tests); ``msg_from_pred`` runs the FK and message kernels of libape_hip.so."""
import logging
import queue
import threading
from abc import abstractmethod
from datetime import datetime

import numpy as np
import torch

from wear_mocap_ape_amd.data_types.bone_map import BoneMap, bodies_from, body9_from_bonemap
from wear_mocap_ape_amd.estimate import _post
from wear_mocap_ape_amd.utility import data_stats
from wear_mocap_ape_amd.utility.names import NNS_INPUTS, NNS_TARGETS, TARGET_LAYOUT


class _DeviceFrame:
    """One iteration of the consumer loop (estimator.py:174-177) as ONE call into libape_hip.so: a one-stream bank
    (``ape_streams_*``) keeps the window and smoothing histories on the device, ``ape_streams_frame_host`` takes the raw
    55 / 28-float message (220 / 112 bytes in) and returns the message list ``msg_from_pred`` would (25 + 6N values out) --
    feature builder, z-score, regressor with its Monte-Carlo samples, de-normalisation, smoothing stack, FK and message all run
    on the GPU.  The staged methods of the estimator keep their reference semantics (host histories) for callers that use
    them one by one; this object serves ``processing_loop`` / ``process_row`` only."""

    def __init__(self, model, kind: int, seq_len: int, smooth: int, n_mc: int, normalize: bool, seed: int = 0x5EED):
        import ctypes as C
        from wear_mocap_ape_amd import _hip
        from wear_mocap_ape_amd.estimate.nn_models import effective_mc
        self._C, self._hip, self._lib = C, _hip, _hip.lib()
        self._model, self._kind = model, kind
        self._width = _hip.PARSE_SHAPES[kind][0]
        n_mc = effective_mc(model, n_mc)         # (ImuPoseLSTM ignores the sample count: one row per frame)
        self._rows = smooth * n_mc
        self._flags = _hip.FLAG_NORMALIZE_INPUT if normalize else 0
        self._bank = C.c_void_p()
        _hip.check(self._lib.ape_streams_create(model.handle, 1, seq_len, smooth, C.byref(self._bank)), "ape_streams_create")
        # monte_carlo_predictions switches the dropout on whatever n is (nn_models.py:204, :367), also for one sample
        _hip.check(self._lib.ape_streams_set_mc(self._bank, n_mc, float(model.dropout), int(seed) & (2 ** 64 - 1)),
                   "ape_streams_set_mc")
        self._row = np.empty((self._width,), dtype=np.float32)
        self._out = np.empty((25 + 6 * self._rows,), dtype=np.float64)
        self._row_p = C.c_void_p(self._row.ctypes.data)
        self._out_p = C.c_void_p(self._out.ctypes.data)
        # frames with the spread record behind the message list (APE_FLAG_SPREAD): a buffer of their own
        self._out_spread = np.empty((25 + 6 * self._rows + _hip.SPREAD_WIDTH,), dtype=np.float64)
        self._out_spread_p = C.c_void_p(self._out_spread.ctypes.data)

    def __del__(self):
        bank, self._bank = getattr(self, "_bank", None), None
        try:
            if bank:
                self._lib.ape_streams_destroy(bank)
        except Exception:          # interpreter shutdown
            pass

    def reset(self):
        self._hip.check(self._lib.ape_streams_reset(self._bank), "ape_streams_reset")
        self._per_stream = False

    # ---- state hand-over: the one stream of this bank as a canonical record ----
    _per_stream = False        # set_state puts the bank into per-stream mode: frames then run as subset frames until the next reset

    def _device(self):
        return torch.device("cuda", self._model.device_index)

    def state_desc(self) -> dict:
        from wear_mocap_ape_amd import stream_state
        d = self._hip.ApeStreamStateDesc()
        self._hip.check(self._lib.ape_streams_state_desc(self._bank, self._C.byref(d)), "ape_streams_state_desc")
        return {k: int(getattr(d, k)) for k in stream_state.DESC_KEYS}

    def get_state(self):
        """-> (desc, float32 record [1, words] on the device, warm np.uint8 [1]) of the one stream"""
        C, desc = self._C, self.state_desc()
        dev = self._device()
        state = torch.zeros((1, desc["words_per_stream"]), dtype=torch.float32, device=dev)
        warm, idx = np.zeros((1,), dtype=np.uint8), np.zeros((1,), dtype=np.int32)
        self._hip.check(self._lib.ape_streams_export(self._bank, C.c_void_p(idx.ctypes.data), 1, C.c_void_p(state.data_ptr()),
                                                     C.c_void_p(warm.ctypes.data), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                        "ape_streams_export")
        return desc, state, warm

    def set_state(self, desc: dict, state, warm):
        from wear_mocap_ape_amd import stream_state
        C, dev = self._C, self._device()
        d = self._hip.ApeStreamStateDesc(*[int(desc[k]) for k in stream_state.DESC_KEYS])
        st = torch.as_tensor(state, dtype=torch.float32).reshape(1, -1).to(dev).contiguous()
        if st.shape[1] != int(d.words_per_stream):
            raise UserWarning(f"set_state wants one record of {int(d.words_per_stream)} words, got {st.shape[1]}")
        w, idx = np.asarray(warm, dtype=np.uint8).reshape(1).copy(), np.zeros((1,), dtype=np.int32)
        self._hip.check(self._lib.ape_streams_import(self._bank, C.byref(d), C.c_void_p(idx.ctypes.data), 1, C.c_void_p(st.data_ptr()),
                                                     C.c_void_p(w.ctypes.data), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                        "ape_streams_import")
        torch.cuda.current_stream(dev).synchronize()     # (the record is this call's own copy)
        self._per_stream = True

    def _frame_subset(self, spread: bool = False) -> np.ndarray:
        """a frame of a bank in per-stream mode: ``ape_streams_frame_subset`` over the one stream (the host frame is lockstep-only)"""
        C, hip, dev = self._C, self._hip, self._device()
        packed = self._rows > 1
        if spread:
            return self._frame_subset_spread(packed)
        if getattr(self, "_sub_bufs", None) is None:         # once: the device row, the device message, pinned mirrors, the list [0]
            w = 25 + 6 * self._rows if packed else 25
            self._sub_bufs = (torch.empty((1, self._width), dtype=torch.float32, device=dev),
                              torch.empty((1, w), dtype=torch.float64, device=dev),
                              torch.empty((1, self._width), dtype=torch.float32).pin_memory(),
                              torch.empty((1, w), dtype=torch.float64).pin_memory(), np.zeros((1,), dtype=np.int32))
        rd, out, row_pin, out_pin, idx = self._sub_bufs
        row_pin.numpy()[0, :] = self._row
        rd.copy_(row_pin, non_blocking=True)
        hip.check(self._lib.ape_streams_frame_subset(self._bank, self._kind, C.c_void_p(rd.data_ptr()), C.c_void_p(idx.ctypes.data), 1,
                                                     self._flags | (hip.FLAG_PACKED_MSG if packed else 0), C.c_void_p(out.data_ptr()),
                                                     hip.F64, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "ape_streams_frame_subset")
        self._model.recover()                            # blocking, like the host frame: the message is valid on return
        out_pin.copy_(out)                                # (behind the blocking recover: the stream is idle)
        self._out[:] = 0.0                                # N = 1: no tail behind the 25 values
        self._out[:out.shape[1]] = out_pin.numpy()[0]
        return self._out

    def _frame_subset_spread(self, packed: bool) -> np.ndarray:
        """``_frame_subset`` with APE_FLAG_SPREAD: the row is 21 columns longer; returned in the host frame's layout [25 + 6N + 21]"""
        C, hip, dev = self._C, self._hip, self._device()
        w = (25 + 6 * self._rows if packed else 25) + hip.SPREAD_WIDTH
        if getattr(self, "_sub_bufs_spread", None) is None:
            self._sub_bufs_spread = (torch.empty((1, self._width), dtype=torch.float32, device=dev),
                                     torch.empty((1, w), dtype=torch.float64, device=dev), np.zeros((1,), dtype=np.int32))
        rd, out, idx = self._sub_bufs_spread
        rd.copy_(torch.from_numpy(self._row).reshape(1, -1))
        hip.check(self._lib.ape_streams_frame_subset(self._bank, self._kind, C.c_void_p(rd.data_ptr()), C.c_void_p(idx.ctypes.data), 1,
                                                     self._flags | (hip.FLAG_PACKED_MSG if packed else 0) | hip.FLAG_SPREAD,
                                                     C.c_void_p(out.data_ptr()), hip.F64, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "ape_streams_frame_subset")
        self._model.recover()                            # blocking, like the host frame
        host = out.cpu().numpy()[0]
        self._out_spread[:] = 0.0                        # N = 1: no tail between the 25 values and the record
        self._out_spread[:w - hip.SPREAD_WIDTH] = host[:-hip.SPREAD_WIDTH]
        self._out_spread[-hip.SPREAD_WIDTH:] = host[-hip.SPREAD_WIDTH:]
        return self._out_spread

    def frame_stats(self, reset: bool = False) -> dict:
        """where the frames' host time went (ape_streams_frame_stats, ABI 7): per-frame microseconds of the last <= 4096 frames in
        `launch` (rows into pinned staging + the launch calls), `wait` (last launch call returned -> completion words seen) and `copy`
        (pinned output -> the caller's buffer), and the number of frames that fell through to a stream synchronisation"""
        C = self._C

        class _FS(C.Structure):
            _fields_ = [("frames", C.c_uint64), ("fallback_syncs", C.c_uint64), ("recovered", C.c_uint64)]
        fs, n = _FS(), C.c_int32(0)
        trace = np.zeros((4096, 3), dtype=np.float32)
        self._hip.check(self._lib.ape_streams_frame_stats(self._bank, C.byref(fs), C.c_void_p(trace.ctypes.data), 4096, C.byref(n),
                                                          1 if reset else 0), "ape_streams_frame_stats")
        t = trace[:n.value]
        return {"frames": int(fs.frames), "fallback_syncs": int(fs.fallback_syncs), "recovered": int(fs.recovered),
                "launch_us": t[:, 0].copy(), "wait_us": t[:, 1].copy(), "copy_us": t[:, 2].copy()}

    def frame(self, row, spread: bool = False) -> np.ndarray:
        """raw message -> float64 [25 + 6N]: the message followed by hand / elbow xyz of the N stacked rows (a view of
        this object's buffer, overwritten by the next frame); ``spread``: [25 + 6N + 21], the spread record behind them"""
        self._row[:] = row                       # array('f') (stream/listener/imu.py:68-70), list or ndarray
        if self._per_stream:
            return self._frame_subset(spread)
        if spread:
            self._hip.check(self._lib.ape_streams_frame_host(self._bank, self._kind, self._row_p, self._flags | self._hip.FLAG_SPREAD,
                                                             self._out_spread_p, self._hip.F64, None), "ape_streams_frame_host")
            return self._out_spread
        self._hip.check(self._lib.ape_streams_frame_host(self._bank, self._kind, self._row_p, self._flags, self._out_p,
                                                         self._hip.F64, None), "ape_streams_frame_host")
        return self._out


class Estimator:
    """Template-method base of the estimators.  Subclasses provide ``parse_row_to_xx`` (raw message ->
    features) and ``make_prediction_from_row_hist`` (normalised window -> NN targets); everything else --
    window and smoothing histories, float64 (de-)normalisation, FK + message, the consumer thread -- lives
    here.  Constructor arguments, methods and properties are the reference's (estimator.py:16-218)."""

    def __init__(self, x_inputs: NNS_INPUTS, y_targets: NNS_TARGETS, normalize: bool = True, smooth: int = 1,
                 seq_len: int = 1, add_mc_samples: bool = True, bonemap: BoneMap = None, tag: str = "Estimator"):
        self.__tag, self._active = tag, False
        self._x_inputs, self._y_targets = x_inputs, y_targets
        self._layout = TARGET_LAYOUT[y_targets]
        self._device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')

        # pre-computed column statistics: float64 arrays xx_m, xx_s [I] and yy_m, yy_s [O]
        self._normalize = normalize
        if normalize:
            self._take_stats(data_stats.get_norm_stats(x_inputs=x_inputs, y_targets=y_targets))

        # histories: feature rows of the current window, predictions of the last `smooth` frames
        self._sequence_len, self._smooth = max(1, seq_len), max(1, smooth)
        self._row_hist, self._smooth_hist = [], []
        self._add_mc_samples, self._last_msg = add_mc_samples, None

        # arm geometry: both arm bones point along -x; [[larm_vec, uarm_vec, uarm_orig_rh]] as one [1,9] row
        self._uarm_orig = BoneMap.DEFAULT_UARM_ORIG_RH if bonemap is None else bonemap.left_upper_arm_origin_rh
        body9 = body9_from_bonemap(bonemap)
        self._larm_vec, self._uarm_vec = body9[0:3].copy(), body9[3:6].copy()
        self._body_measurements = body9[np.newaxis, :]
        self._sync_model_config()

    def _take_stats(self, stats: dict):
        self._xx_m, self._xx_s, self._yy_m, self._yy_s = (stats[k] for k in ("xx_m", "xx_s", "yy_m", "yy_s"))

    # subclasses that own a HIP model expose it here so stats/body reach the device handle
    def _hip_model(self):
        return None

    def _sync_model_config(self):
        model = self._hip_model()
        if model is None:
            return
        model.set_body(self._body_measurements)
        if self._normalize:
            model.set_norm_stats(self._xx_m, self._xx_s, self._yy_m, self._yy_s)

    def set_norm_stats(self, stats: dict):
        """replace the statistics loaded at construction (also on the device handle)"""
        self._take_stats(stats)
        self._sync_model_config()
        logging.info("Replaced norm stats xx m+/-s and yy m+/-s")

    def get_last_msg(self):
        return self._last_msg

    # ---- Monte-Carlo spread record (the reference has no counterpart) ----
    _spread, _last_spread = False, None

    @property
    def spread(self) -> bool:
        """off by default.  On: every frame also reduces its stacked rows to the 21-value spread record (``_post.spread_rows``
        states the layout), kept for ``get_last_spread()``; what ``process_row`` / ``processing_loop`` return is unchanged."""
        return self._spread

    @spread.setter
    def spread(self, on):
        if on and (self._frame_samples() is None or self._hip_model() is None):
            raise UserWarning(f"{type(self).__name__} does not serve the spread record (estimators with a HIP regressor do)")
        self._spread = bool(on)
        if not self._spread:
            self._last_spread = None                      # no record outlives the switch

    def get_last_spread(self):
        """float64 [21] record of the newest frame made with ``spread`` on since the last ``reset()``, or None"""
        return self._last_spread

    def is_active(self):
        return self._active

    def terminate(self):
        self._active = False

    def reset(self):
        self._active, self._row_hist, self._smooth_hist = False, [], []
        self._last_spread = None
        frame = getattr(self, "_device_frame", None)
        if frame is not None:
            frame.reset()

    # ---- state hand-over: this estimator's window and stack as one canonical record ----------
    def get_state(self) -> dict:
        """The estimator's history as a canonical stream record (``stream_state``): ``{"desc", "window" [T, I], "stack" [smooth,
        n, O], "warm", "form"}``, window and stack in time order (oldest first), ``warm`` the two bits ``WINDOW_WARM | STACK_WARM``.
        Bodies are not part of the record.  Two forms, named in ``"form"``:

        ``"device"`` (estimators whose frames run on the device, ``process_row``): read from the one-stream bank with
        ``ape_streams_export``; the stack holds what the bank's ring holds -- the model's float32 outputs, still normalised.
        ``"host"`` (the staged path: ``add_xx_to_row_hist_and_make_prediction``): read from ``_row_hist`` / ``_smooth_hist``; the
        stack holds the DE-NORMALISED float64 predictions, as in the reference (estimator.py:108-118).  With ``smooth == 1`` that
        path keeps no stack: the stack is zeros and its warm bit clear (a stack of one is rebuilt by the next frame).

        ``state_record(state)`` converts either form to the device record a bank or a replay takes; ``set_state`` accepts both."""
        from wear_mocap_ape_amd import stream_state as ss
        frame = self._frame_runner()
        if frame is not None:
            desc, rec, warm = frame.get_state()
            window, stack = ss.unpack(rec.cpu().numpy()[0], desc)
            return {"desc": desc, "window": window, "stack": stack, "warm": int(warm[0]), "form": "device"}
        T, smooth = self._sequence_len, self._smooth
        warm = (ss.WINDOW_WARM if self._row_hist else 0) | (ss.STACK_WARM if self._row_hist and self._smooth_hist else 0)
        window = np.vstack(self._row_hist) if self._row_hist else np.zeros((T, 0), dtype=np.float32)
        stack = (np.stack([np.atleast_2d(p) for p in self._smooth_hist]) if warm & ss.STACK_WARM
                 else np.zeros((smooth, 1, 0), dtype=np.float64))
        desc = ss.make_desc(T, window.shape[1], smooth, stack.shape[1], stack.shape[2])
        return {"desc": desc, "window": window, "stack": stack, "warm": warm, "form": "host"}

    def _stack_to_form(self, stack, src: str, dst: str):
        """the stack between the host form (de-normalised float64) and the device form (normalised float32), with this estimator's
        own statistics (estimator.py:108-109 and its inverse)"""
        if src == dst:
            return stack
        if dst == "host":
            s = np.asarray(stack, dtype=np.float32)
            return s * self._yy_s + self._yy_m if self._normalize else s.astype(np.float64)
        s = np.asarray(stack, dtype=np.float64)
        return ((s - self._yy_m) / self._yy_s if self._normalize else s).astype(np.float32)

    def state_record(self, state: dict):
        """a ``get_state`` dict -> ``(desc, float32 [1, words] host array, np.uint8 [1])`` in the device form: what
        ``StreamBank.import_state`` takes"""
        from wear_mocap_ape_amd import stream_state as ss
        stack = self._stack_to_form(state["stack"], state["form"], "device")
        window = np.asarray(state["window"], dtype=np.float32)
        if not (state["warm"] & ss.STACK_WARM) and stack.shape[2] == 0:      # a host stack that was never filled has no width yet
            raise UserWarning("state_record: this host-form state has no stack shape; use it with set_state on an estimator")
        desc = ss.make_desc(window.shape[0], window.shape[1], *stack.shape)
        return desc, ss.pack(window, stack)[np.newaxis, :], np.array([state["warm"]], dtype=np.uint8)

    def set_state(self, state: dict):
        """continue from a ``get_state`` dict of either form (from this estimator, another one, or built from a bank's or a
        replay's record with ``stream_state.unpack``, ``"form": "device"``).  The stack is converted to this path's own form with
        this estimator's statistics where the forms differ (float64 -> float32 rounds).  On the device path the one-stream bank is
        then in per-stream mode: its frames run as subset frames until the next ``reset``."""
        from wear_mocap_ape_amd import stream_state as ss
        warm = int(state["warm"])
        frame = self._frame_runner()
        if frame is not None:
            own = frame.state_desc()
            if warm & ss.WINDOW_WARM:
                shape = tuple(np.shape(state["window"])) + (tuple(np.shape(state["stack"])) if warm & ss.STACK_WARM else ())
                want = (own["T"], own["I"]) + ((own["smooth"], own["n_mc"], own["O"]) if warm & ss.STACK_WARM else ())
                if shape != want:
                    raise UserWarning(f"set_state: window / stack of shape {shape}, this estimator keeps {want}")
            if not warm & ss.WINDOW_WARM:
                rec = np.zeros((1, own["words_per_stream"]), dtype=np.float32)
            else:
                stack = self._stack_to_form(state["stack"], state["form"], "device")
                if not warm & ss.STACK_WARM:
                    stack = np.zeros((own["smooth"], own["n_mc"], own["O"]), dtype=np.float32)
                rec = ss.pack(state["window"], stack)[np.newaxis, :]
            frame.set_state(own, rec, np.array([warm], dtype=np.uint8))
            return
        if not warm & ss.WINDOW_WARM:
            self._row_hist, self._smooth_hist = [], []
            return
        window = np.asarray(state["window"])
        if window.shape[0] != self._sequence_len:
            raise UserWarning(f"set_state: a window of {window.shape[0]} rows, this estimator keeps {self._sequence_len}")
        self._row_hist = [window[t].copy() for t in range(window.shape[0])]
        self._smooth_hist = []
        if warm & ss.STACK_WARM and self._smooth > 1:
            stack = self._stack_to_form(state["stack"], state["form"], "host")
            if stack.shape[0] != self._smooth:
                raise UserWarning(f"set_state: a stack of {stack.shape[0]} predictions, this estimator keeps {self._smooth}")
            self._smooth_hist = [stack[j].copy() for j in range(stack.shape[0])]

    # ---- the device-resident frame (processing_loop's fast path) ----------------------------------------------
    def _frame_samples(self):
        """subclasses with a HIP regressor and a batched feature builder return their Monte-Carlo sample count"""
        return None

    def _frame_runner(self):
        """the one-stream device-side frame of this estimator, or None (no GPU regressor: the staged methods run)"""
        if getattr(self, "_device_frame", None) is None:
            n_mc, model = self._frame_samples(), self._hip_model()
            if n_mc is None or model is None or self._parse_kind is None or not self.use_device_frame:
                return None
            self._device_frame = _DeviceFrame(model, self._parse_kind, self._sequence_len, self._smooth, int(n_mc),
                                              self._normalize)
        return self._device_frame

    use_device_frame = True    # False: processing_loop runs the staged methods (parse -> predict -> message) like the reference
    # True: with add_mc_samples the message is ONE float array of 25 + 6 N values instead of the reference's Python list of them
    # (estimator.py:131-137).  Everything the reference does with the message takes either (`struct.pack('f' * len(msg), *msg)`,
    # stream/publisher/pose_est_udp.py:47; np.array(msg)); building the list is the largest host cost of a Monte-Carlo frame -- 1825 floats
    # at 60 samples x smooth 5: ~20 us of a 58 us frame, and most of its p99 (bench.py batch1.estimator_loop).  Opt-in: the default keeps
    # the reference's type.
    msg_as_array = False

    def process_row(self, row):
        """one iteration of the consumer loop (estimator.py:174-177): raw message -> the message put on the queue"""
        frame = self._frame_runner()
        if frame is None:
            pred = self.add_xx_to_row_hist_and_make_prediction(self.parse_row_to_xx(row))
            return self.msg_from_pred(pred, self._add_mc_samples)
        if self._spread:                          # the frame's record rides behind the row and is stripped here
            out = frame.frame(row, spread=True)
            self._last_spread = out[-_post.SPREAD_WIDTH:].copy()
            out = out[:-_post.SPREAD_WIDTH]
        else:
            out = frame.frame(row)
        self._last_msg = out[:25].copy()
        if not self._add_mc_samples:
            return self._last_msg.copy()
        # list of 25 floats followed, for N > 1 stacked rows, by every row's hand and elbow xyz (estimator.py:131-137)
        if self.msg_as_array:
            return out.copy() if out.shape[0] > 31 else self._last_msg.copy()
        return out.tolist() if out.shape[0] > 31 else out[:25].tolist()

    @staticmethod
    def _push_padded(hist: list, item, size: int):
        """append ``item``; a history shorter than ``size`` is filled with copies of the NEWEST item
        (cold start, estimator.py:96-97 / :114-115); the oldest entries beyond ``size`` are dropped"""
        hist.append(item)
        hist.extend([item] * (size - len(hist)))
        del hist[:len(hist) - size]

    def add_xx_to_row_hist_and_make_prediction(self, xx) -> np.array:
        self._push_padded(self._row_hist, xx, self._sequence_len)
        xx_hist = np.vstack(self._row_hist)                       # [T, I]
        if self._normalize:                                       # float64 z-score (estimator.py:103-104)
            xx_hist = (xx_hist - self._xx_m) / self._xx_s
        pred = self.make_prediction_from_row_hist(xx_hist)        # [n, O]
        if self._normalize:                                       # float64 de-normalise (:108-109)
            pred = pred * self._yy_s + self._yy_m
        if self._smooth > 1:                                      # stack of the last `smooth` predictions
            self._push_padded(self._smooth_hist, pred, self._smooth)
            pred = np.vstack(self._smooth_hist)
        return pred

    def msg_from_pred(self, pred: np.array, add_mc_samples: bool) -> np.array:
        # arm_pose_from_nn_targets + msg_from_nn_targets_est in one device round trip
        ctx = _post.context(self._layout)
        with ctx.lock:
            est, msg = _post.fk_and_msg(ctx.handle, self._layout, ctx.device, pred, self._body_measurements)
        self._last_msg = msg.copy()
        if self._spread:
            self._last_spread = _post.spread_rows(est, msg, self._layout)
        if add_mc_samples:
            # list of 25 floats followed, for N > 1 rows, by every row's hand and elbow xyz (estimator.py:131-137)
            msg = list(msg)
            if est.shape[0] > 1:
                msg += list(est[:, :6].reshape(-1))
        return msg

    def process_in_thread(self, sensor_q: queue):
        """start the consumer thread; returns the queue the messages are put on"""
        msg_q = queue.Queue()
        threading.Thread(target=self.processing_loop, args=(sensor_q, msg_q)).start()
        return msg_q

    def _newest_row(self, sensor_q: queue):
        """latency policy of estimator.py:159-161: block up to 2 s for a row; when more than 5 rows are
        queued behind it, skip ahead (newest wins).  Raises ``queue.Empty`` when nothing arrives."""
        row = sensor_q.get(timeout=2)
        while sensor_q.qsize() > 5:
            row = sensor_q.get(timeout=2)
        return row

    def processing_loop(self, sensor_q: queue, msg_q: queue):
        logging.info(f"[{self.__tag}] wearable streaming loop")
        self.reset()
        self._active = True
        tick, frames = datetime.now(), 0          # processing rate is logged every >= 5 s as frames / 5
        while self._active:
            try:
                row = self._newest_row(sensor_q)
            except queue.Empty:
                logging.info(f"[{self.__tag}] no data")
                continue
            now = datetime.now()
            if (now - tick).seconds >= 5:
                logging.info(f"[{self.__tag}] {frames / 5} Hz")
                tick, frames = now, 0
            msg_q.put(self.process_row(row))
            frames += 1

    @abstractmethod
    def make_prediction_from_row_hist(self, xx_hist: np.array) -> np.array:
        return

    @abstractmethod
    def parse_row_to_xx(self, row) -> np.array:
        return

    # ---- batched feature builder: raw messages of many streams -> features on the GPU ----
    _parse_kind = None        # subclasses: the APE_PARSE_* selector of their message/feature layout

    def parse_rows(self, rows, out_dtype=None):
        """rows: float32 ``[N, 55|28]`` raw messages (host array or CUDA tensor) -> features ``[N, I]`` on the
        device, the batched equivalent of ``parse_row_to_xx`` (``ape_parse_rows`` kernel, float64 arithmetic).
        Default dtype is what the reference's ``parse_row_to_xx`` returns (float32; float64 for the
        upper-arm estimator)."""
        import ctypes as C
        from wear_mocap_ape_amd import _hip
        if self._parse_kind is None:
            raise UserWarning("this estimator has no batched feature builder")
        width, n_feat = _hip.PARSE_SHAPES[self._parse_kind]
        if out_dtype is None:
            out_dtype = torch.float64 if self._parse_kind == _hip.PARSE_WATCH_PHONE_UARM else torch.float32
        model = self._hip_model()
        dev = model.torch_device if model is not None else torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(dev):
            rd = torch.as_tensor(rows, dtype=torch.float32).to(dev).contiguous()
            if rd.dim() != 2 or rd.shape[1] != width or rd.shape[0] < 1:
                raise UserWarning(f"expected rows [N>=1,{width}], got {tuple(rd.shape)}")
            xx = torch.empty((rd.shape[0], n_feat), dtype=out_dtype, device=dev)
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _hip.check(_hip.lib().ape_parse_rows(self._parse_kind, C.c_void_p(rd.data_ptr()), int(rd.shape[0]),
                                                 C.c_void_p(xx.data_ptr()),
                                                 _hip.F64 if out_dtype == torch.float64 else _hip.F32, stream),
                       "ape_parse_rows")
        return xx

    # ---- batched entry the reference lacks: many independent windows at once ----
    def infer_windows(self, x, est_dtype=torch.float64, return_targets: bool = False):
        """x: raw (un-normalised) features float32 ``[B,T,I]``, host array or CUDA tensor ->
        est ``[B,21|14]`` (same rows ``arm_pose_from_nn_targets`` yields), on the device.
        One ``ape_infer`` call: z-score -> LSTM -> last step -> de-normalise -> FK."""
        import ctypes as C
        from wear_mocap_ape_amd import _hip
        model = self._hip_model()
        if model is None:
            raise UserWarning("this estimator has no HIP regressor")
        dev = model.torch_device
        with torch.cuda.device(dev):
            xd = torch.as_tensor(x, dtype=torch.float32).to(dev).contiguous()
            if xd.dim() != 3 or xd.shape[2] != model.input_size or xd.shape[0] < 1 or xd.shape[1] < 1:
                raise UserWarning(f"expected x [B>=1,T>=1,{model.input_size}], got {tuple(xd.shape)}")
            B, T = int(xd.shape[0]), int(xd.shape[1])
            est = torch.empty((B, _hip.EST_WIDTH[self._layout]), dtype=est_dtype, device=dev)
            y = torch.empty((B, model.output_size), dtype=torch.float32, device=dev) if return_targets else None
            flags = _hip.FLAG_NORMALIZE_INPUT if self._normalize else 0
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _hip.check(_hip.lib().ape_infer(model.handle, C.c_void_p(xd.data_ptr()), B, T, flags,
                                            C.c_void_p(y.data_ptr()) if y is not None else None,
                                            C.c_void_p(est.data_ptr()),
                                            _hip.F64 if est_dtype == torch.float64 else _hip.F32, stream), "ape_infer")
            model._pending.append((xd, y, est))      # journaled by the handle: alive until its next check / recover (nn_models._run)
            if len(model._pending) > 64:
                del model._pending[0]
        return (est, y) if return_targets else est

    # ---- offline replay: every frame of recorded sessions in one call ----
    def process_recording(self, rows, starts=None, big_endian: bool = False, out_dtype=torch.float64,
                          return_targets: bool = False, seed: int = 0x5EED, max_rows_per_launch: int = 0, bonemaps=None,
                          state_in=None, warm_in=None, return_state: bool = False, sample_row_base: int = 0, spread: bool = False,
                          _config=None):
        """rows: float32 ``[F, 55|28]`` raw messages of one or more recordings back to back (host array or CUDA
        tensor); ``starts``: the recordings' first rows (default ``[0]``: one recording).  Returns, on the device,
        what ``process_row`` returns for every row of a fresh estimator fed each recording in order (no row skipped):
        ``[F, 25 + 6N]`` with ``add_mc_samples`` and N = smooth x Monte-Carlo samples > 1, else ``[F, 25]``.  With
        ``return_targets`` also the normalised NN targets float32 ``[F, n_mc, O]``.  Over an ``ImuPoseLSTM`` the sample count is
        ignored as in the reference (n_mc = 1 in every shape above); ``DropoutFF`` and ``ImuPoseLSTM`` models go through
        ``ape_replay_regressor``.  The Monte-Carlo samples are those
        of one dropout forward keyed by ``seed`` over the repeated windows (``ape_replay``); ``max_rows_per_launch``
        bounds the sample rows of one regressor launch (0: the library's default) and with it the device workspace.
        ``bonemaps``: one entry per recording (bonemap-like objects, ``None`` for the defaults, or float64 ``[R, 9]`` values) --
        every recording is then replayed as by an estimator built with ITS bonemap (``ape_replay_bodies``);
        default: this estimator's body for all.

        Resumable replay (``ape_replay_resume``): ``state_in`` float32 ``[R, words]`` (device tensor or host array) with
        ``warm_in`` uint8 ``[R]`` -- one canonical stream record per listed recording, from an earlier call's ``return_state``, a bank's
        ``export_state`` or ``state_record(get_state())`` -- lets every recording continue instead of starting cold; ``return_state``
        appends ``(state, warm)``, the recordings' final records in the same form, to the result (``StreamBank.import_state`` takes
        them).  ``sample_row_base`` is added to the Philox row counter: one recording replayed over rows ``[0, a), [a, b), ...`` with
        the states chained and ``sample_row_base = a * n_mc, ...`` returns the rows of the one call (a multiple of 4; Monte-Carlo
        samples included where the regressor kernel's row granule divides it, see ``ape_hip.h``).  With several recordings the
        deterministic results are equal and the samples are valid draws, not the one call's.  A recording that ended in an earlier call
        is not listed.  Bodies are not part of a record.  With none of the four given the call is the old path, entry and all.

        ``spread``: the result becomes ``(out, spread)`` (``(out, y, spread)`` with ``return_targets``; the state pair stays last) with
        ``spread`` ``[F, 21]`` of ``out_dtype``, every frame's spread record (``_post.spread_rows``); both are views
        of one wider device tensor.  Chained pieces give the records of the one call.

        ``_config`` (``sweep_recording``): ``(smooth, samples)`` for this call in place of the estimator's own, which stay as they
        are; the rows are then never packed."""
        import ctypes as C
        from wear_mocap_ape_amd import _hip
        model, n_mc = self._hip_model(), self._frame_samples()
        if model is None or n_mc is None or self._parse_kind is None:
            raise UserWarning("this estimator has no HIP regressor or no batched feature builder")
        width = _hip.PARSE_SHAPES[self._parse_kind][0]
        if out_dtype not in (torch.float32, torch.float64):
            raise UserWarning(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
        from wear_mocap_ape_amd.estimate.nn_models import DropoutFF, ImuPoseLSTM, effective_mc
        smooth = self._smooth
        if _config is not None:
            smooth, n_mc = int(_config[0]), int(_config[1])
        n_mc = effective_mc(model, n_mc)
        n_rows = smooth * n_mc
        # (DropoutLSTM models keep the entry they always took)
        entry = "ape_replay_regressor" if isinstance(model, (DropoutFF, ImuPoseLSTM)) else "ape_replay_bodies"
        dev = model.torch_device
        with torch.cuda.device(dev):
            rd = torch.as_tensor(rows, dtype=torch.float32).to(dev).contiguous()
            if rd.dim() != 2 or rd.shape[1] != width or rd.shape[0] < 1:
                raise UserWarning(f"expected rows [F>=1,{width}], got {tuple(rd.shape)}")
            F = int(rd.shape[0])
            st = np.ascontiguousarray(np.asarray([0] if starts is None else starts, dtype=np.int32).reshape(-1))
            packed = self._add_mc_samples and n_rows > 1 and _config is None
            out = torch.empty((F, (25 + 6 * n_rows if packed else 25) + (_hip.SPREAD_WIDTH if spread else 0)), dtype=out_dtype, device=dev)
            y = torch.empty((F, n_mc, model.output_size), dtype=torch.float32, device=dev) if return_targets else None
            flags = (_hip.FLAG_NORMALIZE_INPUT if self._normalize else 0) | (_hip.FLAG_PACKED_MSG if packed else 0) | \
                    (_hip.FLAG_SPREAD if spread else 0)
            kind = self._parse_kind | (_hip.PARSE_BIG_ENDIAN if big_endian else 0)
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            bodies = None if bonemaps is None else bodies_from(bonemaps, int(st.shape[0]), "process_recording bonemaps")
            extra, state_out, warm_out = (), None, None
            if state_in is not None or return_state or sample_row_base:
                from wear_mocap_ape_amd import stream_state as ss
                entry, n_rec = "ape_replay_resume", int(st.shape[0])
                words = ss.words_per_stream(1 if isinstance(model, DropoutFF) else self._sequence_len, model.input_size, smooth,
                                            n_mc, model.output_size)
                sin = win = None
                if state_in is not None:
                    if warm_in is None:
                        raise UserWarning("process_recording: state_in needs warm_in")
                    sin = torch.as_tensor(state_in, dtype=torch.float32).to(dev).contiguous()
                    win = np.ascontiguousarray(np.asarray(warm_in, dtype=np.uint8).reshape(-1))
                    if tuple(sin.shape) != (n_rec, words) or win.shape[0] != n_rec:
                        raise UserWarning(f"process_recording: state_in must be [{n_rec},{words}] with {n_rec} warm bytes, got "
                                          f"{tuple(sin.shape)} and {win.shape[0]}")
                if return_state:
                    state_out = torch.zeros((n_rec, words), dtype=torch.float32, device=dev)
                    warm_out = np.zeros((n_rec,), dtype=np.uint8)
                extra = (C.c_void_p(sin.data_ptr()) if sin is not None else None, C.c_void_p(win.ctypes.data) if win is not None else None,
                         C.c_void_p(state_out.data_ptr()) if return_state else None,
                         C.c_void_p(warm_out.ctypes.data) if return_state else None, int(sample_row_base))
            _hip.check(getattr(_hip.lib(), entry)(model.handle, kind, C.c_void_p(rd.data_ptr()), F, C.c_void_p(st.ctypes.data),
                                                    int(st.shape[0]), self._sequence_len, smooth, n_mc, float(model.dropout),
                                                    int(seed) & (2 ** 64 - 1), flags, C.c_void_p(out.data_ptr()),
                                                    _hip.F64 if out_dtype == torch.float64 else _hip.F32,
                                                    C.c_void_p(y.data_ptr()) if y is not None else None,
                                                    int(max_rows_per_launch), stream,
                                                    C.c_void_p(bodies.ctypes.data) if bodies is not None else None, *extra), entry)
            model._pending.clear()         # the call is blocking and checked the handle (its journal is empty)
        rec = None
        if spread:
            out, rec = out[:, :-_hip.SPREAD_WIDTH], out[:, -_hip.SPREAD_WIDTH:]
        res = (out, y) if return_targets else out
        if spread:
            res = (res if isinstance(res, tuple) else (res,)) + (rec,)
        if return_state:
            res = (res if isinstance(res, tuple) else (res,)) + ((state_out, warm_out),)
        return res

    # ---- the output layer fitted to a wearer (the reference has no counterpart) ----
    def features_recording(self, rows, starts=None, big_endian: bool = False, max_rows_per_launch: int = 0, return_targets: bool = False):
        """rows, ``starts``, ``big_endian``, ``max_rows_per_launch``: as in ``process_recording``.  Returns, on the device, float32
        ``[F, H]``: for every frame the top LSTM layer's output of the last step of its window, the vector ``output_layer`` multiplies
        (``ape_replay_features``: one row per frame, no dropout, every recording starts cold as a replay starts it); with
        ``return_targets`` also the normalised NN targets ``[F, O]`` the present head makes of them.  ``DropoutLSTM`` models only."""
        import ctypes as C
        from wear_mocap_ape_amd import _hip
        model = self._hip_model()
        if model is None or self._parse_kind is None:
            raise UserWarning("this estimator has no HIP regressor or no batched feature builder")
        width = _hip.PARSE_SHAPES[self._parse_kind][0]
        dev = model.torch_device
        with torch.cuda.device(dev):
            rd = torch.as_tensor(rows, dtype=torch.float32).to(dev).contiguous()
            if rd.dim() != 2 or rd.shape[1] != width or rd.shape[0] < 1:
                raise UserWarning(f"expected rows [F>=1,{width}], got {tuple(rd.shape)}")
            F = int(rd.shape[0])
            st = np.ascontiguousarray(np.asarray([0] if starts is None else starts, dtype=np.int32).reshape(-1))
            h = torch.empty((F, model.hidden_layer_size), dtype=torch.float32, device=dev)
            y = torch.empty((F, model.output_size), dtype=torch.float32, device=dev) if return_targets else None
            kind = self._parse_kind | (_hip.PARSE_BIG_ENDIAN if big_endian else 0)
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _hip.check(_hip.lib().ape_replay_features(model.handle, kind, C.c_void_p(rd.data_ptr()), F, C.c_void_p(st.ctypes.data),
                                                      int(st.shape[0]), self._sequence_len, _hip.FLAG_NORMALIZE_INPUT if self._normalize else 0,
                                                      C.c_void_p(h.data_ptr()), C.c_void_p(y.data_ptr()) if y is not None else None,
                                                      int(max_rows_per_launch), stream), "ape_replay_features")
            model._pending.clear()         # the call is blocking and checked the handle (its journal is empty)
        return (h, y) if return_targets else h

    def fit_head(self, rows, truth, starts=None, skip=None, rec_lags=None, ridge: float = 1e-3, install: bool = False,
                 big_endian: bool = False, max_rows_per_launch: int = 0, min_pairs=None):
        """A linear probe: the LSTM stays, ``output_layer`` is fitted again to these recordings.  ``rows``, ``starts``: as in
        ``features_recording``; ``truth``: device ``[F, O]`` de-normalised NN targets, as ``score_recording(truth_kind="targets")`` takes
        them (this estimator's ``yy_m`` / ``yy_s`` go in as shift and scale when it normalises: the fit is in the head's own units);
        ``skip`` defaults to the ``sequence_len - 1`` cold-start frames; ``rec_lags``: each recording's lag, as ``score.best_lag`` finds
        it; ``ridge``: the pull towards the present head, ``min_pairs``: the fewest pairs a fit is made from, ``2 (H + 1)`` by default
        (``score.best_head``; ``score.sweep_ridge`` prices candidates on the sums this returns).  Returns ``(w [O, H], b [O], report, sums)``; ``install`` also makes it this estimator's head (``set_head``)
        unless the fit was refused."""
        from wear_mocap_ape_amd import score
        h = self.features_recording(rows, starts, big_endian, max_rows_per_launch)
        td = torch.as_tensor(truth).to(h.device)
        if td.dtype not in (torch.float32, torch.float64):
            td = td.to(torch.float64)
        skip = self._sequence_len - 1 if skip is None else skip
        shift, scale = (self._yy_m, self._yy_s) if self._normalize else (None, None)
        sums = score.fit_sums(h, td, starts, skip, rec_lags, shift, scale)
        w0, b0 = self.head
        w, b, report = score.best_head(sums, w0, b0, ridge, min_pairs=min_pairs)
        if install and not report["refused"]:
            self.set_head(w, b)
        return w, b, report, sums

    def set_head(self, w, b):
        """installs ``output_layer.weight`` ``[O, H]`` and ``.bias`` ``[O]`` on the regressor (``DropoutLSTM.set_head``: the device handle and
        the kept ``state_dict``), so ``process_row``, the banks, replays and the reference-style methods all run on it"""
        model = self._hip_model()
        if model is None:
            raise UserWarning("this estimator has no HIP regressor")
        model.set_head(w, b)

    @property
    def head(self):
        """``(w [O, H], b [O])`` float32: the output layer the regressor runs"""
        model = self._hip_model()
        if model is None:
            raise UserWarning("this estimator has no HIP regressor")
        return model.get_head()

    # ---- scoring a replay against ground truth (the reference has no counterpart) ----
    def score_recording(self, out, truth, spread=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", lags=None,
                        rec_lags=None):
        """``score.score_rows`` with this estimator's layout and body: ``out`` (and ``spread``) as ``process_recording`` returned them,
        ``truth`` device ``[F, O]`` de-normalised targets (or est rows with ``truth_kind="est"``); ``skip`` defaults to the
        ``sequence_len - 1`` cold-start frames of every recording; ``bonemaps``: one bonemap-like object for all recordings or one entry
        per recording (default: this estimator's body).  Returns ``(score [F, 7], acc [R, 25])`` on the device.
        ``lags=(lo, hi)``: ``score.score_lags`` over that sweep of time lags instead (``rec_lags``: per-recording offsets; DESIGN.md
        4.32), returning ``(score [F, L, 7], acc [R, L, 25])``."""
        from wear_mocap_ape_amd import score
        skip = self._sequence_len - 1 if skip is None else skip
        bodies = self._body_measurements if bonemaps is None else bonemaps
        if lags is None:
            if rec_lags is not None:
                raise UserWarning("rec_lags are offsets of a sweep: give lags=(lo, hi) with them")
            return score.score_rows(self._layout, out, truth, truth_kind, spread, starts, skip, bodies)
        return score.score_lags(self._layout, out, truth, lags, truth_kind, spread, starts, skip, bodies, rec_lags, per_frame=True)

    def error_distribution(self, out, truth, spread=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", rec_lags=None,
                           edges=None, bins=64):
        """The shape of a replay's errors: ``score_recording``'s per-frame rows -- with ``rec_lags`` at each recording's
        own lag, the sweep ``(0, 0)`` with offsets -- counted over ``edges`` per recording on the device (``score.hist_rows`` over
        ``score.lag_trim``'s windows: the frames the accumulators cover).  ``edges``: ``[B + 1]`` or ``[7, B + 1]``, default
        ``score.default_edges("score", bins)``; the other arguments are ``score_recording``'s.  Returns ``(hist, edges, acc)``: int64
        ``[R, 7, B + 3]`` and float64 ``[R, 25]`` on the device, the edges float64 ``[7, B + 1]`` on the host (``score.quantiles``,
        ``fraction_within``, ``pit``, ``summarise_hist``, ``merge_hist``)."""
        from wear_mocap_ape_amd import score
        skip = self._sequence_len - 1 if skip is None else skip
        if rec_lags is None:
            rows, acc = self.score_recording(out, truth, spread, starts, skip, bonemaps, truth_kind)
        else:
            rows, acc = self.score_recording(out, truth, spread, starts, skip, bonemaps, truth_kind, (0, 0), rec_lags)
            rows, acc = rows[:, 0], acc[:, 0]
        edges = score.default_edges("score", bins) if edges is None else score._edges(edges, score.SCORE_WIDTH)
        trim = score.lag_trim(starts, int(rows.shape[0]), (0, 0), skip, rec_lags)
        return score.hist_rows(rows, edges, starts, 0, trim), edges, acc

    def align_recording(self, out, truth, spread=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", lags=(0, 0),
                        mode="yaw", weights=(1, 1, 1, 0, 0)):
        """``score.align_frame`` with this estimator's layout and body and ``score_recording``'s defaults: each recording's lag (over the
        sweep ``lags=(lo, hi)``) and constant world-side rotation against the truth (``mode`` ``"yaw"`` or ``"full"``, ``weights`` of the
        lower-arm, upper-arm and hips rotations and the hand and elbow positions) are found together, the rows (and
        ``spread``) are turned by it and scored at the lags found.  Returns ``(score [F, 7], acc [R, 25], found)``, ``found`` being
        ``score.best_frame``'s list (``lag``, ``quat``, ``yaw``, ...)."""
        from wear_mocap_ape_amd import score
        skip = self._sequence_len - 1 if skip is None else skip
        bodies = self._body_measurements if bonemaps is None else bonemaps
        return score.align_frame(self._layout, out, truth, lags, mode, weights, truth_kind, spread, starts, skip, bodies)

    def fit_bodies(self, out, truth, starts=None, skip=None, truth_kind="est", lags=(0, 0), rec_lags=None, quats=None, mode="vectors",
                   weights=(1, 1), bonemaps=None):
        """``score.align_body`` with this estimator's layout and ``score_recording``'s defaults: each recording's arm vectors and shoulder
        origin (``mode="vectors"``) or the three lengths of the prior body (``"lengths"``) that make ``out``'s positions fit ``truth``
        (est rows) best, with the rotations ``out`` states.  ``lags`` / ``rec_lags``: the sweep, as in
        ``score_recording``; ``quats``: ``align_recording``'s headings, taken out first; ``weights``: of the hand and the elbow;
        ``bonemaps``: the prior -- one bonemap-like object, one per recording or float64 ``[R, 9]`` (default: this estimator's body).
        Returns ``(score [F, 7], acc [R, 25], found)``: the rows made again under the bodies found and scored at the lags found, and
        ``score.best_body``'s list; ``score.bodies_of(found)`` goes into ``set_bodies``, ``process_recording(bonemaps=)`` and
        ``repost(bonemaps=)``."""
        from wear_mocap_ape_amd import score
        skip = self._sequence_len - 1 if skip is None else skip
        prior = self._body_measurements if bonemaps is None else bonemaps
        return score.align_body(self._layout, out, truth, lags, mode, weights, truth_kind, None, starts, skip, rec_lags, quats, prior)

    def truth_on_frames(self, rows, truth, truth_times, truth_starts=None, starts=None, shifts=None, max_gap: float = 0.0,
                        truth_kind="targets", bonemaps=None, big_endian: bool = False):
        """``score.truth_on_frames`` with this estimator's layout and body: the mocap ``truth`` (device ``[Ft, O]`` de-normalised targets,
        or est rows with ``truth_kind="est"``) with its stamps ``truth_times`` resampled onto the clock that the raw ``rows``' ``sw_dt``
        column states, less ``shifts``.  Returns float64 est rows ``[F, 21 | 14]`` on the device, for
        ``score_recording(..., truth_kind="est")``.  ``bonemaps``: as in ``score_recording``."""
        from wear_mocap_ape_amd import score
        bodies = self._body_measurements if bonemaps is None else bonemaps
        return score.truth_on_frames(self._layout, rows, truth, truth_times, truth_starts, starts, shifts, max_gap, truth_kind, bodies, big_endian)

    # ---- how smooth a replay is (the reference has no counterpart) ----
    def motion_recording(self, out, starts=None, skip=None, times=None, per_frame=False):
        """``score.motion_sums`` with this estimator's layout: ``out`` as ``process_recording`` returned it (or ``repost``'s
        ``[C, F, 25]``), ``times`` device float64 ``[F]`` (``score.frame_times``; None: per-frame units); ``skip`` defaults to
        ``score_recording``'s.  Returns ``(motion [F, 12] | None, acc [R, 38])`` on the device (``score.summarise_motion``)."""
        from wear_mocap_ape_amd import score
        skip = self._sequence_len - 1 if skip is None else skip
        return score.motion_sums(self._layout, out, "msg", starts, skip, times, None, per_frame)

    def truth_motion(self, truth, truth_kind="targets", starts=None, skip=None, times=None, bonemaps=None):
        """The floor the truth itself sets: ``score.motion_sums`` of ``truth`` (device ``[F, O]`` de-normalised targets, or est rows
        with ``truth_kind="est"``) with this estimator's layout and body and ``motion_recording``'s defaults.  Returns
        ``(None, acc [R, 38])``."""
        from wear_mocap_ape_amd import score
        skip = self._sequence_len - 1 if skip is None else skip
        bodies = self._body_measurements if bonemaps is None else bonemaps
        return score.motion_sums(self._layout, truth, truth_kind, starts, skip, times, bodies)

    # ---- spectra of a replay (the reference has no counterpart) ----
    def spectrum_recording(self, out, truth=None, starts=None, skip=None, truth_kind="est", bonemaps=None, n=256, hop=None, taper="hann",
                           rate=1.0):
        """At which frequencies a replay follows the arm: ``score.spectra`` of the six hand and elbow position columns
        (``score.pose_cols``, ``score.POSE_COL_NAMES``) of ``out`` as ``process_recording`` returned it (or ``repost``'s
        ``[C, F, 25]``), against ``truth`` if given: device est rows ``[F, 21 | 14]`` (``truth_kind="est"``), or de-normalised targets
        ``[F, O]`` (``"targets"``), which ``score.resample_truth`` turns into est rows on the device, on the frames' own index clock,
        with this estimator's body or ``bonemaps``.  Welch segments of ``n`` frames every ``hop`` (``n // 2``), ``taper`` and the mean
        taken off each segment; ``skip`` defaults to ``score_recording``'s; ``rate``: frames per second (the clock is the frame index:
        jitter of the stamps is ignored).  Returns ``(acc, counts, summary)``: the raw sums on the device and
        ``score.summarise_spectra`` of them (``score.bandwidth``, ``score.band_power``); waits for the device."""
        from wear_mocap_ape_amd import score
        skip = self._sequence_len - 1 if skip is None else skip
        bodies = self._body_measurements if bonemaps is None else bonemaps
        acc, counts = score.pose_spectra(self._layout, out, truth, truth_kind, starts, skip, bodies, n, hop, taper)
        return acc, counts, score.summarise_spectra(acc, counts, score.spectra_taper(taper, n), rate)

    # ---- reaches and holds (the reference has no counterpart) ----
    def _segments_of(self, score, speed, thresholds, mins, times, starts, extra=None):
        """labels, table and per-segment records of one hand-speed column: the value columns are the speed (its maximum is the peak speed)
        and ``speed * dt`` (its sum is the path length; ``dt`` is 1 on the index clock), then ``extra``'s"""
        labels = score.segment_frames(speed, thresholds, mins, starts)
        sof, n, table = score.segment_runs(labels, starts)
        path = speed
        if times is not None:
            dt = torch.zeros_like(times)
            dt[1:] = times[1:] - times[:-1]                  # (a recording's first frames have no speed: what dt holds there is not read)
            path = speed * dt.to(speed.dtype)
        cols = [speed.to(torch.float64), path.to(torch.float64)] + ([] if extra is None else [c.to(torch.float64) for c in extra])
        stats = score.segment_stats(torch.stack(cols, dim=1), sof, n, table)
        return {"labels": labels, "seg_of_frame": sof, "n_segs": n, "table": table, "stats": stats}

    def segment_recording(self, out, pilot_rows=None, thresholds=(0.004, 0.008), mins=(4, 4), times=None, starts=None, truth=None,
                          truth_kind="targets", truth_thresholds=None, bonemaps=None, truth_mins=(1, 1)):
        """Where a replay holds and where it reaches, and every segment's figures (``score.segment_frames``, ``segment_runs``,
        ``segment_stats``).  ``out`` as ``process_recording`` returned it; ``pilot_rows``: the rows whose hand speed is
        the key (a smoothed rendering of the same replay, e.g. a rung of ``repost_windows``; default ``out`` itself); ``thresholds``
        ``(lo, hi)`` of the hand speed in metres per frame, or per unit of ``times`` (device float64 ``[F]``, ``score.frame_times``);
        ``mins`` ``(min_hold, min_move)`` in frames.  A recording's first three frames have no speed and take the label hold.
        Returns a dict on the device: ``labels`` uint8 ``[F]`` (0 hold, 1 move), ``seg_of_frame`` int32 ``[F]``, ``n_segs``, ``table``
        int32 ``[n, 4]`` of ``(recording, first frame, length, label)``, ``stats`` float64 ``[n, V, 5]`` (``score.SEG_STAT_NAMES``) over
        the columns ``names``: ``hand_speed`` (its maximum is the peak speed) and ``path`` (speed times the frame's step: its sum is the
        path length).  With ``truth`` (device ``[F, O]`` de-normalised targets, or est rows with ``truth_kind="est"``; ``bonemaps`` as in
        ``score_recording``) the columns ``hand_pos`` and ``elbow_pos`` follow, ``score_recording``'s per-frame errors at lag 0, and
        the dict holds ``truth``: ``truth_segments``' dict at ``truth_thresholds`` (default: half of ``thresholds``) and ``truth_mins``;
        ``match``: ``score.match_segments`` of the two tables, moves against moves; ``hold_error`` float64 ``[n_truth]``: for every
        hold of the truth the distance between the mean estimated and the mean true hand position over its frames (NaN for a move).
        The table's size is read back: the call waits for the device."""
        from wear_mocap_ape_amd import score
        rows = out if pilot_rows is None else pilot_rows
        speed = score.motion_sums(self._layout, rows, "msg", starts, 0, times, None, True)[0]
        if speed.dim() != 2:
            raise UserWarning("segment_recording: one set of rows [F, >= 25] (pick a rung of a [C, F, 25] rendering)")
        speed = speed[:, 0]
        names, extra = ["hand_speed", "path"], None
        if truth is not None:
            bodies = self._body_measurements if bonemaps is None else bonemaps
            errors = score.score_rows(self._layout, out, truth, truth_kind, None, starts, 0, bodies)[0]
            names, extra = names + ["hand_pos", "elbow_pos"], [errors[:, 0], errors[:, 1]]
        res = self._segments_of(score, speed, thresholds, mins, times, starts, extra)
        res["names"] = names
        if truth is None:
            return res
        th = np.asarray(thresholds, dtype=np.float64) / 2.0 if truth_thresholds is None else truth_thresholds
        tr = self.truth_segments(truth, truth_kind, th, truth_mins, times, starts, bonemaps)
        res["truth"] = tr
        res["match"] = score.match_segments(res["table"], tr["table"], score.MOVE, 0, times)
        # the endpoint error of the truth's holds: six more columns over the truth's segments, the hand as estimated and as it was
        est_rows = truth if truth_kind == "est" else score.resample_truth(self._layout, truth, truth_kind, starts, None, None, int(truth.shape[0]),
                                                                           starts, None, 0.0, bodies)
        hands = torch.cat([out[:, 4:7].to(torch.float64), est_rows[:, 0:3].to(torch.float64)], dim=1)
        hs = score.segment_stats(hands, tr["seg_of_frame"], tr["n_segs"], tr["table"])
        mean = hs[:, :, 1] / hs[:, :, 0]
        d = mean[:, 0:3] - mean[:, 3:6]
        err = torch.sqrt((d * d).sum(dim=1))
        res["hold_error"] = torch.where(tr["table"][:, 3] == score.HOLD, err, torch.full_like(err, float("nan")))
        return res

    def truth_segments(self, truth, truth_kind="targets", thresholds=(0.002, 0.004), mins=(1, 1), times=None, starts=None, bonemaps=None):
        """The truth's own holds and reaches: ``segment_recording``'s dict (``labels``, ``seg_of_frame``, ``n_segs``, ``table``, ``stats``
        over ``hand_speed`` and ``path``, ``names``) from the hand speed of ``truth`` (device ``[F, O]`` de-normalised targets, or est
        rows with ``truth_kind="est"``) with this estimator's layout and body."""
        from wear_mocap_ape_amd import score
        bodies = self._body_measurements if bonemaps is None else bonemaps
        speed = score.motion_sums(self._layout, truth, truth_kind, starts, 0, times, bodies, True)[0][:, 0]
        res = self._segments_of(score, speed, thresholds, mins, times, starts)
        res["names"] = ["hand_speed", "path"]
        return res

    # ---- joint angles (the reference has no counterpart) ----
    def angles_recording(self, out, truth=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", rec_lags=None,
                         per_frame=False, min_swing=0.05):
        """``score.joint_angles`` with this estimator's layout and body: the joint angles of ``out`` as ``process_recording`` returned it
        (or ``repost``'s ``[C, F, 25]``) and, with ``truth`` (device ``[F, O]`` de-normalised targets, or est rows with
        ``truth_kind="est"``), their errors, each recording at its own lag ``rec_lags``; ``skip`` defaults to ``score_recording``'s.
        Returns ``(angles [F, 7] | None, errors [F, 7] | None, acc [R, 71])`` on the device (``score.summarise_angles``)."""
        from wear_mocap_ape_amd import score
        skip = self._sequence_len - 1 if skip is None else skip
        bodies = self._body_measurements if bonemaps is None else bonemaps
        return score.joint_angles(self._layout, out, "msg", truth, truth_kind, starts, skip, rec_lags, bodies, min_swing, per_frame)

    def truth_angles(self, truth, truth_kind="targets", starts=None, skip=None, bonemaps=None, per_frame=False, min_swing=0.05):
        """The truth's own joint angles -- its range of motion: ``score.joint_angles`` of ``truth`` (device ``[F, O]`` de-normalised
        targets, or est rows with ``truth_kind="est"``) with this estimator's layout and body and ``angles_recording``'s defaults.
        Returns ``(angles [F, 7] | None, None, acc [R, 71])``."""
        from wear_mocap_ape_amd import score
        skip = self._sequence_len - 1 if skip is None else skip
        bodies = self._body_measurements if bonemaps is None else bonemaps
        return score.joint_angles(self._layout, truth, truth_kind, None, "est", starts, skip, None, bodies, min_swing, per_frame)

    # ---- errors by condition (the reference has no counterpart) ----
    def errors_by(self, out, truth, by, spread=None, starts=None, skip=None, bonemaps=None, truth_kind="targets", rec_lags=None,
                  edges=None, bins=36, times=None):
        """Where a replay is wrong: ``score_recording``'s per-frame ``[F, 7]`` rows (with ``rec_lags`` at each recording's own lag, as in
        ``error_distribution``) as the values of ``score.stats_by``, keyed per frame by ``by``:
        ``"angles"``: ``angles_recording(per_frame=True)`` of ``out``, the seven joint angles, over ``score.angle_edges(bins)``;
        ``"truth_angles"``: ``truth_angles(per_frame=True)``, the truth's own angles (refused with ``rec_lags``: the truth frame of a pair
        is then another frame than the keyed one);
        ``"motion"``: ``motion_recording(per_frame=True)`` on the clock ``times``, twelve columns over
        ``score.default_edges("motion", bins)``;
        ``"spread"``: ``score.spread_sigma(spread)`` over the position and angle columns of ``score.default_edges("score", bins)`` -- the
        reliability curve of the spread record;
        a device tensor ``[F, K]``: any keys, with ``edges`` (``[B + 1]`` or ``[K, B + 1]``) required.
        The window is ``score.lag_trim``'s, the frames the accumulators cover.  Returns ``(by, edges, key_names)``: float64
        ``[R, K, B + 3, 7, 4]`` on the device, the edges float64 ``[K, B + 1]`` on the host, the key columns' names
        (``score.summarise_by``, ``pool_by``, ``merge_by``; the value columns are ``score.SCORE_HIST_NAMES``)."""
        from wear_mocap_ape_amd import score
        skip = self._sequence_len - 1 if skip is None else skip
        if rec_lags is None:
            rows, _ = self.score_recording(out, truth, spread, starts, skip, bonemaps, truth_kind)
        else:
            rows, _ = self.score_recording(out, truth, spread, starts, skip, bonemaps, truth_kind, (0, 0), rec_lags)
            rows = rows[:, 0]
        default = None
        if isinstance(by, torch.Tensor):
            if edges is None:
                raise UserWarning("errors_by: keys given as a tensor need edges")
            keys, names = by, tuple(f"key{k}" for k in range(int(by.shape[-1])))
        elif by == "angles":
            keys, names = self.angles_recording(out, None, starts, skip, bonemaps, truth_kind, None, True)[0], score.ANGLE_NAMES
            default = lambda: score.angle_edges(bins)[:score.ANGLE_WIDTH]      # noqa: E731
        elif by == "truth_angles":
            if rec_lags is not None:
                raise UserWarning("errors_by: by='truth_angles' with rec_lags: the truth frame of a pair is another frame than the keyed one")
            keys, names = self.truth_angles(truth, truth_kind, starts, skip, bonemaps, True)[0], score.ANGLE_NAMES
            default = lambda: score.angle_edges(bins)[:score.ANGLE_WIDTH]      # noqa: E731
        elif by == "motion":
            keys, names = self.motion_recording(out, starts, skip, times, True)[0], score.MOTION_NAMES
            default = lambda: score.default_edges("motion", bins)              # noqa: E731
        elif by == "spread":
            if spread is None:
                raise UserWarning("errors_by: by='spread' needs the spread records")
            keys, names = score.spread_sigma(spread), score.SIGMA_NAMES
            default = lambda: score.default_edges("score", bins)[:5]           # noqa: E731
        else:
            raise UserWarning(f"errors_by: by must be 'angles', 'truth_angles', 'motion', 'spread' or a device tensor, got {by!r}")
        edges = default() if edges is None else score._edges(edges, int(keys.shape[-1]))
        trim = score.lag_trim(starts, int(rows.shape[0]), (0, 0), skip, rec_lags)
        return score.stats_by(keys, rows, edges, starts, 0, trim), edges, names

    # ---- post-filter sweep (the reference has no counterpart) ----
    def repost(self, y, configs, starts=None, bonemaps=None, spread: bool = False, out_dtype=torch.float64, workspace_bytes: int = 0):
        """``score.post_sweep`` with this estimator's model and body: ``y`` device float32 ``[F, M, O]`` as
        ``process_recording(return_targets=True)`` returned it, ``configs`` a list of ``(smooth, samples)`` pairs (``score.grid``) ->
        ``out [C, F, 25]`` (``(out, spread [C, F, 21])`` with ``spread``), ``out[c]`` the first 25 columns an estimator with configuration
        ``c`` would have returned for the same recordings.  ``bonemaps``: one entry per recording (default: this estimator's body)."""
        from wear_mocap_ape_amd import score
        return self._repost("repost", score.post_sweep, y, configs, starts, bonemaps, spread, out_dtype, workspace_bytes)

    def _repost(self, who: str, post, y, sets, starts, bonemaps, spread, out_dtype, workspace_bytes):
        """``repost`` and ``repost_windows``: their guard and the bodies of ``bonemaps``, then ``post`` (``score.post_sweep`` /
        ``score.post_window``) with this estimator's model"""
        model = self._hip_model()
        if model is None or self._frame_samples() is None:
            raise UserWarning("this estimator has no HIP regressor")
        if not self._normalize:
            raise UserWarning(f"{who} de-normalises its targets: this estimator does not normalise")
        if bonemaps is not None:
            R = len(np.asarray([0] if starts is None else starts).reshape(-1))
            bonemaps = bodies_from(bonemaps, R, f"{who} bonemaps")
        return post(model, y, sets, starts, bonemaps, spread, out_dtype, workspace_bytes)

    def sweep_recording(self, rows, truth, smooths, samples, starts=None, lags=(0, 0), truth_kind="targets", bonemaps=None,
                        seed: int = 0x5EED, skip=None, big_endian: bool = False, spectra: bool = False, motion: bool = False, times=None):
        """Which ``smooth`` and how many Monte-Carlo samples: ONE ``process_recording(return_targets=True)`` at ``max(samples)`` samples
        (this estimator's own ``smooth`` and sample count stay what they are), one ``score.post_sweep`` of
        ``score.grid(smooths, samples)`` with the spread records, then one ``score.score_lags`` over ``lags`` per configuration against
        ``truth`` (device ``[F, O]`` de-normalised targets, or est rows with ``truth_kind="est"``).  Over an ``ImuPoseLSTM`` every sample
        count is 1 (``nn_models.effective_mc``).  ``skip`` defaults to the ``sequence_len - 1`` cold-start frames of every recording.
        Returns ``{"configs": [(smooth, samples), ...], "acc": ndarray [C, R, L, 25], "best": [score.best_lag(acc[c], lags) per
        configuration]}`` (waits for the device).  ``motion=True``: the dict also holds ``"motion": ndarray [C, R, 38]``, what every
        configuration's smoothing buys -- one ``score.motion_sums`` call on the sweep's ``out`` (``times``: the frames' clock, device
        float64 ``[F]``; None: per-frame units).  ``spectra=True``: the dict also holds ``"bandwidth"``, ndarray
        ``[C, R, 6]``: the -3 dB bandwidth in cycles per frame of every configuration's hand and elbow positions against the truth
        (``spectrum_recording``'s defaults; NaN where a recording is shorter than a segment).  Pass everything after
        ``big_endian`` by keyword: ``spectra`` stands ahead of ``motion`` and ``times``, which stay the last two."""
        from wear_mocap_ape_amd import score
        from wear_mocap_ape_amd.estimate.nn_models import effective_mc
        model = self._hip_model()
        if model is None or self._frame_samples() is None:
            raise UserWarning("this estimator has no HIP regressor or no batched feature builder")
        configs = score.grid(smooths, [effective_mc(model, int(m)) for m in samples])
        if not configs:
            raise UserWarning("sweep_recording: no configuration")
        return self._sweep(self.repost, score.score_configs, configs, max(m for _, m in configs), rows, truth, starts, lags, truth_kind,
                           bonemaps, seed, skip, big_endian, motion, times, spectra)

    def _sweep(self, repost, score_sets, configs, top: int, rows, truth, starts, lags, truth_kind, bonemaps, seed, skip, big_endian, motion,
               times, spectra=False):
        """``sweep_recording`` and ``sweep_windows`` once their list is made: the replay at ``top`` samples, ``repost`` (``self.repost``
        / ``self.repost_windows``) of ``configs`` with the spread records, the defaults of ``skip`` and the bodies, ``score_sets``
        (``score.score_configs`` / ``score.score_windows``), ``motion`` and ``spectra``"""
        from wear_mocap_ape_amd import score
        _, y = self.process_recording(rows, starts=starts, big_endian=big_endian, return_targets=True, seed=seed, bonemaps=bonemaps,
                                      _config=(1, top))
        out, rec = repost(y, configs, starts=starts, bonemaps=bonemaps, spread=True)
        skip = self._sequence_len - 1 if skip is None else skip
        bodies = self._body_measurements if bonemaps is None else bonemaps
        res = score_sets(self._layout, out, rec, truth, configs, lags, truth_kind, starts, skip, bodies)
        if motion:
            res["motion"] = score.motion_sums(self._layout, out, "msg", starts, skip, times)[1].cpu().numpy()
        if spectra:
            acc, counts = score.pose_spectra(self._layout, out, truth, truth_kind, starts, skip, bodies)
            res["bandwidth"] = score.bandwidth(score.summarise_spectra(acc, counts, "hann"))
        return res

    # ---- windowed post-filter: windows that look ahead, tapered weights (the reference has no counterpart) ----
    def repost_windows(self, y, windows, starts=None, bonemaps=None, spread: bool = False, out_dtype=torch.float64, workspace_bytes: int = 0):
        """``score.post_window`` with this estimator's model and body: ``y`` as for ``repost``, ``windows`` a list of
        ``score.window(back, ahead, samples, shape_or_weights)`` entries -> ``out [C, F, 25]`` (``(out, spread [C, F, 21])`` with
        ``spread``): frame ``f`` of ``out[c]`` is smoothed over the frames ``f - back .. f + ahead`` of its recording.  A uniform
        ``(smooth - 1, 0, samples)`` is ``repost``'s ``(smooth, samples)``, bit for bit.  ``bonemaps``: one entry per recording."""
        from wear_mocap_ape_amd import score
        return self._repost("repost_windows", score.post_window, y, windows, starts, bonemaps, spread, out_dtype, workspace_bytes)

    def sweep_windows(self, rows, truth, windows, starts=None, lags=(0, 0), truth_kind="targets", bonemaps=None, seed: int = 0x5EED,
                      skip=None, big_endian: bool = False, spectra: bool = False, motion: bool = False, times=None):
        """What looking ahead and tapering buy, for a recording processed offline: ONE ``process_recording(return_targets=True)`` at the
        largest sample count of ``windows`` (``score.window`` entries; this estimator's own ``smooth`` and sample count stay what they
        are), one ``score.post_window`` with the spread records, then one ``score.score_lags`` over ``lags`` per window against
        ``truth``.  Over an ``ImuPoseLSTM`` every sample count is 1.  ``skip``, ``truth_kind``, ``bonemaps``, ``motion``, ``times``,
        ``spectra``: ``sweep_recording``'s (everything after ``big_endian`` by keyword).  Returns ``sweep_recording``'s dict with ``"configs"`` holding the windows as ``score.window`` returns
        them (waits for the device)."""
        from wear_mocap_ape_amd import score
        from wear_mocap_ape_amd.estimate.nn_models import effective_mc
        model = self._hip_model()
        if model is None or self._frame_samples() is None:
            raise UserWarning("this estimator has no HIP regressor or no batched feature builder")
        windows = [(b, a, effective_mc(model, int(m)), w) for b, a, m, w in score._windows(windows)[0]]
        return self._sweep(self.repost_windows, score.score_windows, windows, max(m for _, _, m, _ in windows), rows, truth, starts, lags,
                           truth_kind, bonemaps, seed, skip, big_endian, motion, times, spectra)

    # ---- speed-adaptive smoothing: a window per frame from a ladder (the reference has no counterpart) ----
    def repost_selected(self, y, ladder, sel, starts=None, bonemaps=None, spread: bool = False, out_dtype=torch.float64,
                        workspace_bytes: int = 0):
        """``score.post_select`` with this estimator's model and body: ``y`` as for ``repost``, ``ladder`` as ``score.ladder`` returns it (or
        a list of ``score.window`` entries), ``sel`` uint8 device ``[F]`` or ``[S, F]`` (``score.select_rungs``) -> ``out [(S,) F, 25]``
        (``(out, spread [(S,) F, 21])`` with ``spread``): frame ``f`` of set ``s`` is ``repost_windows``' frame ``f`` of window
        ``sel[s, f]``, bit for bit.  ``bonemaps``: one entry per recording."""
        from wear_mocap_ape_amd import score
        return self._repost("repost_selected", lambda model, y_, lad, *rest: score.post_select(model, y_, lad, sel, *rest), y, ladder, starts,
                            bonemaps, spread, out_dtype, workspace_bytes)

    def _adaptive_ladder(self, ladder):
        """(windows at this model's effective sample counts, reach) of ``score.ladder``'s pair, a list of windows or None (the default
        ladder at this estimator's sample count)"""
        from wear_mocap_ape_amd import score
        from wear_mocap_ape_amd.estimate.nn_models import effective_mc
        model = self._hip_model()
        if model is None or self._frame_samples() is None:
            raise UserWarning("this estimator has no HIP regressor or no batched feature builder")
        wins = score.ladder(samples=self._frame_samples())[0] if ladder is None else score._ladder_windows(ladder)
        wins = [(b, a, effective_mc(model, int(m)), w) for b, a, m, w in score._windows(wins)[0]]
        return wins, score._reach(wins)

    def _rule_selector(self, pilot_rows, edges, slope, reach, starts, times):
        """the selector of one rule: the hand speed of the pilot's rows (``score.motion_sums``, column 0; per frame, or per unit of
        ``times``) binned over ``edges`` (None: ``score.speed_edges``, one edge per step of the ladder) with the envelope ``slope``"""
        from wear_mocap_ape_amd import score
        motion = score.motion_sums(self._layout, pilot_rows, "msg", starts, 0, times, per_frame=True)[0]
        edges = score.speed_edges(count=max(1, len(reach) - 1)) if edges is None else edges
        return score.select_rungs(motion[:, 0], edges, reach, slope, starts=starts)

    def smooth_adaptive(self, rows, ladder=None, pilot: int = 3, edges=None, slope: int = 2, times=None, starts=None, bonemaps=None,
                        seed: int = 0x5EED, big_endian: bool = False, spread: bool = False, out_dtype=torch.float64, workspace_bytes: int = 0):
        """Offline smoothing whose window follows the hand speed: ONE ``process_recording(return_targets=True)`` at the ladder's largest
        sample count, one ``score.post_window`` of rung ``pilot`` of the ladder, ``score.motion_sums(per_frame=True)`` of it for the
        hand-speed column, ``score.select_rungs`` (``edges``, ``slope``: its arguments; the default edges are metres per frame, so give
        edges with ``times``), then ``score.post_select``.  ``ladder``: ``score.ladder``'s pair (default: centred Hann windows of
        half-widths ``score.LADDER_HALVES`` at this estimator's sample count).  Returns ``(out [F, 25], sel uint8 [F])`` on the device,
        ``(out, sel, spread [F, 21])`` with ``spread``.  Does not wait."""
        wins, reach = self._adaptive_ladder(ladder)
        if not 0 <= int(pilot) < len(wins):
            raise UserWarning(f"smooth_adaptive: pilot {pilot} is no rung of a ladder of {len(wins)}")
        _, y = self.process_recording(rows, starts=starts, big_endian=big_endian, return_targets=True, seed=seed, bonemaps=bonemaps,
                                      _config=(1, max(m for _, _, m, _ in wins)))
        first = self.repost_windows(y, [wins[int(pilot)]], starts=starts, bonemaps=bonemaps, workspace_bytes=workspace_bytes)[0]
        sel = self._rule_selector(first, edges, slope, reach, starts, times)
        got = self.repost_selected(y, wins, sel, starts=starts, bonemaps=bonemaps, spread=spread, out_dtype=out_dtype,
                                   workspace_bytes=workspace_bytes)
        return (got[0], sel, got[1]) if spread else (got, sel)

    def sweep_adaptive(self, rows, truth, ladder, rules, starts=None, lags=(0, 0), truth_kind="targets", bonemaps=None, seed: int = 0x5EED,
                       skip=None, big_endian: bool = False, motion: bool = False, times=None):
        """Does adapting beat the best fixed window on this recording: ONE replay, ``sweep_windows`` of the ladder's rungs, and one more
        set per rule ``(pilot, edges, slope)`` of ``rules`` -- the selector ``smooth_adaptive`` makes from rung ``pilot`` (its rows are
        the fixed sweep's), all rules in one ``score.post_select``.  Returns ``sweep_windows``' dict with ``"configs"`` holding the
        ladder's windows and then the rules, ``"acc" [L + S, R, lags, 25]`` and ``"best"`` in that order (``"motion" [L + S, R, 38]``
        with ``motion=True``), and ``"sel"``: the selectors, uint8 ``[S, F]`` on the host (waits for the device)."""
        from wear_mocap_ape_amd import score
        wins, reach = self._adaptive_ladder(ladder)
        rules = [(int(p), None if e is None else np.asarray(e, dtype=np.float64), int(k)) for p, e, k in rules]
        if not rules or len(rules) > 64 or any(not 0 <= p < len(wins) for p, _, _ in rules):
            raise UserWarning(f"sweep_adaptive: between 1 and 64 rules (pilot, edges, slope) with pilot a rung of the ladder of {len(wins)}")
        _, y = self.process_recording(rows, starts=starts, big_endian=big_endian, return_targets=True, seed=seed, bonemaps=bonemaps,
                                      _config=(1, max(m for _, _, m, _ in wins)))
        out, rec = self.repost_windows(y, wins, starts=starts, bonemaps=bonemaps, spread=True)
        skip = self._sequence_len - 1 if skip is None else skip
        bodies = self._body_measurements if bonemaps is None else bonemaps
        res = score.score_windows(self._layout, out, rec, truth, wins, lags, truth_kind, starts, skip, bodies)
        sel = torch.stack([self._rule_selector(out[p], e, k, reach, starts, times) for p, e, k in rules])
        aout, arec = self.repost_selected(y, wins, sel, starts=starts, bonemaps=bonemaps, spread=True)
        ada = score.score_selected(self._layout, aout, arec, truth, rules, lags, truth_kind, starts, skip, bodies)
        res = {"configs": res["configs"] + ada["configs"], "acc": np.concatenate([res["acc"], ada["acc"]]), "best": res["best"] + ada["best"],
               "sel": sel.cpu().numpy()}
        if motion:
            res["motion"] = np.concatenate([score.motion_sums(self._layout, o, "msg", starts, skip, times)[1].cpu().numpy() for o in (out, aout)])
        return res

    # read-only views, same names as the reference's properties (estimator.py:188-218)
    sequence_len = property(lambda self: self._sequence_len)
    body_measurements = property(lambda self: self._body_measurements)
    uarm_orig = property(lambda self: self._uarm_orig)
    uarm_vec = property(lambda self: self._uarm_vec)
    larm_vec = property(lambda self: self._larm_vec)
    device = property(lambda self: self._device)
    x_inputs = property(lambda self: self._x_inputs)
    y_targets = property(lambda self: self._y_targets)
