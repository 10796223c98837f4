"""Data-parallel sharding of independent sensor streams / windows over the GPUs of one node.

The reference has no parallelism of any kind (last row); windows are fully
independent (zero initial state per window, nn_models.py:180-189), so the path shards with NO
per-step exchange: one process per GPU, a contiguous range of streams per rank, and a single
broadcast of the weight blob from rank 0 at start-up (RCCL over xGMI when the process group's
backend is "nccl"; the same code runs on "gloo" for CPU tests)."""
from typing import Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import stream_state as _state


def shard_range(n_streams: int, rank: int, world_size: int) -> Tuple[int, int]:
    """contiguous [lo, hi) of stream indices owned by ``rank``; sizes differ by at most one and
    the ranges tile [0, n_streams) in rank order (8192 streams on 8 GPUs -> 1024 each)."""
    if n_streams < 0 or world_size < 1 or not (0 <= rank < world_size):
        raise UserWarning(f"bad shard request: n={n_streams} rank={rank} world={world_size}")
    base, rem = divmod(n_streams, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def flatten_state_dict(state_dict, keys) -> np.ndarray:
    """state_dict -> flat float32 blob in ``keys`` order (the layout ``ape_model_load_weights`` takes)"""
    parts = []
    for k in keys:
        v = state_dict[k]
        a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        parts.append(np.ascontiguousarray(a, dtype=np.float32).reshape(-1))
    return np.concatenate(parts)


def broadcast_blob(blob, n_floats: int, device: torch.device, src: int = 0, always: bool = False) -> torch.Tensor:
    """rank ``src`` passes the float32 blob, the others pass None; every rank returns a tensor on
    ``device`` holding identical bytes.  One collective, init-time only."""
    if not dist.is_initialized() or (dist.get_world_size() == 1 and not always):     # `always`: 1-rank rehearsals
        return torch.as_tensor(blob, dtype=torch.float32).to(device)
    # the collective runs where the backend lives: device memory for nccl (RCCL over xGMI), host for gloo
    comm_dev = device if dist.get_backend() == "nccl" else torch.device("cpu")
    if dist.get_rank() == src:
        t = torch.as_tensor(blob, dtype=torch.float32).to(comm_dev).contiguous()
        if t.numel() != n_floats:
            raise UserWarning(f"blob has {t.numel()} floats, expected {n_floats}")
    else:
        t = torch.empty((n_floats,), dtype=torch.float32, device=comm_dev)
    dist.broadcast(t, src=src)
    return t.to(device)


def broadcast_stats(stats: dict, I: int, O: int, device: torch.device, src: int = 0, always: bool = False) -> dict:
    """float64 normalisation statistics travel the same way (exact bits)."""
    if not dist.is_initialized() or (dist.get_world_size() == 1 and not always):
        return stats
    comm_dev = device if dist.get_backend() == "nccl" else torch.device("cpu")
    t = torch.empty((2 * I + 2 * O,), dtype=torch.float64, device=comm_dev)
    if dist.get_rank() == src:
        t.copy_(torch.from_numpy(np.concatenate([np.asarray(stats[k], dtype=np.float64).reshape(-1)
                                                 for k in ("xx_m", "xx_s", "yy_m", "yy_s")])))
    dist.broadcast(t, src=src)
    h = t.cpu().numpy()
    return {"xx_m": h[:I], "xx_s": h[I:2 * I], "yy_m": h[2 * I:2 * I + O], "yy_s": h[2 * I + O:]}


def _set_bodies(bank, entry: str, bodies, streams):
    """the ``set_bodies`` of the three banks (C ABI ``ape_*_set_bodies``)"""
    from .data_types.bone_map import bodies_from
    C = bank._C
    idx = None if streams is None else bank._indices(streams)
    K = bank._n if idx is None else int(idx.shape[0])
    vals = bodies_from(bodies, K, "set_bodies")
    bank._hip.check(getattr(bank._hip.lib(), entry)(bank._handle, C.c_void_p(idx.ctypes.data) if idx is not None else None, K,
                                                    C.c_void_p(vals.ctypes.data), bank._stream()), entry)


def _get_bodies(bank, entry: str) -> np.ndarray:
    out = np.empty((bank._n, 9), dtype=np.float64)
    bank._hip.check(getattr(bank._hip.lib(), entry)(bank._handle, bank._C.c_void_p(out.ctypes.data)), entry)
    return out


def _set_smooths(bank, entry: str, values, streams):
    """the ``set_smooths`` of the NN and FK banks (C ABI ``ape_*_set_smooths``)"""
    C = bank._C
    idx = None if streams is None else bank._indices(streams)
    K = bank._n if idx is None else int(idx.shape[0])
    a = np.asarray(values)
    if a.ndim != 1 or a.shape[0] != K or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise UserWarning(f"set_smooths wants {K} integer smoothing lengths, got {values!r}")
    if a.size and (a.min() < 1 or a.max() > bank._smooth):
        raise UserWarning(f"smoothing lengths must lie in [1, {bank._smooth}], the smooth the bank was built with")
    vals = np.ascontiguousarray(a, dtype=np.int32)
    bank._hip.check(getattr(bank._hip.lib(), entry)(bank._handle, C.c_void_p(idx.ctypes.data) if idx is not None else None, K,
                                                    C.c_void_p(vals.ctypes.data), bank._stream()), entry)


def _get_smooths(bank, entry: str) -> np.ndarray:
    out = np.empty((bank._n,), dtype=np.int32)
    bank._hip.check(getattr(bank._hip.lib(), entry)(bank._handle, bank._C.c_void_p(out.ctypes.data)), entry)
    return out


def datagram_lengths_of(smooths, n_mc: int) -> np.ndarray:
    """int ``[S]``: floats of each stream's datagram -- ``25 + 6 N_s`` with ``N_s = smooths[s] * n_mc`` stacked rows, or 25 where
    ``N_s == 1`` (the reference appends est[i, :6] only when there is more than one stacked row, estimator.py:131-137).  Pure."""
    k = np.asarray(smooths)
    if k.ndim != 1 or (k.size and not np.issubdtype(k.dtype, np.integer)) or int(n_mc) < 1 or (k.size and k.min() < 1):
        raise UserWarning(f"datagram_lengths wants integer smoothing lengths >= 1 and n_mc >= 1, got {smooths!r}, {n_mc!r}")
    n = k.astype(np.int64) * int(n_mc)
    return np.where(n > 1, 25 + 6 * n, 25)


def split_datagrams_of(rows, lengths):
    """rows ``[K, >= max(lengths)]`` (fixed stride: a table bank's datagram rows) -> a list of K views, row j cut to ``lengths[j]``.
    Pure: numpy arrays and tensors alike."""
    ln = np.asarray(lengths)
    if ln.ndim != 1 or (ln.size and not np.issubdtype(ln.dtype, np.integer)):
        raise UserWarning(f"split_datagrams wants one integer length per row, got {lengths!r}")
    if getattr(rows, "ndim", None) != 2 or rows.shape[0] != ln.shape[0]:
        raise UserWarning(f"split_datagrams wants one row per length: {ln.shape[0]} lengths, rows {getattr(rows, 'shape', None)}")
    if ln.size and (ln.min() < 0 or ln.max() > rows.shape[1]):
        raise UserWarning(f"datagram lengths must lie in [0, {rows.shape[1]}]")
    return [rows[j, :int(ln[j])] for j in range(ln.shape[0])]


_SET_SMOOTHS_DOC = """Per-stream smoothing lengths (DESIGN.md 4.35): ``values`` K integers in ``[1, smooth]`` -- the constructor's ``smooth``
        is the bank's CAPACITY --, ``streams`` K distinct indices, or ``None`` for all S streams in order.  From the next frame enqueued on
        the current stream on, stream s behaves like a reference estimator BUILT with ``smooth = values[s]`` (frames already enqueued keep
        the old values).  A COLD START of the listed streams, window and stack (the reference fixes ``smooth`` at construction): with a
        list what ``reset(streams=...)`` does for them, with ``None`` a ``reset()``.  Buffers keep the capacity's shapes: stream s's tail
        and datagram rows hold ``N_s = values[s] * samples`` live rows followed by exact zeros (``datagram_lengths``, ``split_datagrams``).
        ``export_state`` / ``import_state`` records keep the capacity's size and do NOT carry the length: to move a stream, first
        ``set_smooths`` the target slot to the source's value (that cold-starts the slot), then ``import_state`` (that warms it)."""


def _host_rows(rows, K: int, width: int) -> np.ndarray:
    """the rows of a ``frame_host`` call: a contiguous float32 host array ``[K, width]``"""
    if isinstance(rows, torch.Tensor):
        raise UserWarning("frame_host takes host rows (a numpy array); device tensors go to frame()")
    a = np.asarray(rows)
    if a.dtype != np.float32 or a.shape != (K, width):
        raise UserWarning(f"frame_host wants float32 rows [{K},{width}] for {K} streams, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def tick_rounds(stream_ids):
    """The round splitter of ``tick`` (pure: no bank, no GPU).  ``stream_ids``: the streams of a bag of rows in arrival order, repeats
    allowed.  -> ``(rounds, order)``: ``rounds[r]`` int64 positions into the bag of the r-th row of every stream that has one, in
    arrival order (so the streams of one round are distinct and every stream's rows keep their order over the rounds); ``order``
    the inverse permutation: ``np.concatenate(rounds)[order]`` is ``arange(n)``, i.e. outputs concatenated round by round and
    indexed with ``order`` are back in input order."""
    ids = np.asarray(stream_ids)
    if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
        raise UserWarning(f"stream_ids must be a sequence of stream indices, got {stream_ids!r}")
    n = int(ids.shape[0])
    if n == 0:
        return [], np.zeros((0,), dtype=np.int64)
    # occurrence number of every entry among the entries of its stream (stable sort: arrival order within a stream)
    by_stream = np.argsort(ids, kind="stable")
    sorted_ids = ids[by_stream]
    first = np.flatnonzero(np.r_[True, sorted_ids[1:] != sorted_ids[:-1]])
    occ = np.empty((n,), dtype=np.int64)
    occ[by_stream] = np.arange(n) - np.repeat(first, np.diff(np.r_[first, n]))
    rounds = [np.flatnonzero(occ == r) for r in range(int(occ.max()) + 1)]
    order = np.empty((n,), dtype=np.int64)
    order[np.concatenate(rounds)] = np.arange(n)
    return rounds, order


def tick(bank, rows, stream_ids, **kw):
    """The bag of one receive-loop iteration through a bank's ``frame_host``: ``rows`` float32 host ``[n, width]``, ``stream_ids`` the
    stream of every row in ARRIVAL order -- a stream may appear more than once.  The bag is split into rounds (``tick_rounds``), one
    ``frame_host(rows[round], stream_ids[round], **kw)`` runs per round, and the outputs come back in input order (a tuple of arrays
    where ``frame_host`` returns one, e.g. ``(rows, n_rows)`` of a Kalman bank with ``datagrams``).  Every row is processed as
    ``process_row`` would, in per-stream arrival order; the live loop's queue skip-ahead (estimator.py:166-173 drops all but the
    newest queued row) is NOT applied, as in the replay.  Mode rules are ``frame_host``'s; Monte-Carlo samples depend on a row's
    position within its round."""
    ids = np.asarray(stream_ids)
    rounds, order = tick_rounds(ids)
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[0] != ids.shape[0]:
        raise UserWarning(f"tick wants one row per stream id: {ids.shape[0]} ids, rows {rows.shape}")
    if not rounds:
        return bank.frame_host(rows, ids, **kw)
    outs = [bank.frame_host(np.ascontiguousarray(rows[r]), ids[r], **kw) for r in rounds]
    if isinstance(outs[0], tuple):
        return tuple(np.concatenate([o[i] for o in outs])[order] for i in range(len(outs[0])))
    return np.concatenate(outs)[order]


_SET_BODIES_DOC = """Per-stream body measurements (DESIGN.md 4.24): ``bodies`` float64 ``[K, 9]`` (``[larm_vec, uarm_vec,
        uarm_orig_rh]`` per row) or a sequence of K bonemap-like objects / ``None`` (the defaults); ``streams`` K distinct indices, or
        ``None`` for all S streams in order.  From the next frame enqueued on the current stream on, stream s takes its body from row s
        (frames already enqueued keep the old values).  NOT a cold start: the stream's next message is computed from its existing
        window and stack with the new body -- handing a slot to a new wearer is ``set_bodies`` + ``reset(streams=[s])``."""


class StreamBank:
    """The per-frame step of many independent wearable streams with all state on the device: window rings,
    smoothing stacks, regressor, FK and messages (C ABI ``ape_streams_*``).  For every stream it does what one
    ``Estimator`` does per frame (estimator.py:93-137), so S estimator threads of the reference become three kernel
    launches per frame.  Rank-local: give each rank its ``shard_range`` of streams.

    ``model`` is a HIP-backed ``DropoutLSTM``, ``DropoutFF`` or ``ImuPoseLSTM`` (nn_models.py) with weights, norm stats and body set.
    ``monte_carlo_samples=None`` runs the regressor once per stream with deterministic weights; an integer n runs
    it n times per stream and frame with dropout ``dropout`` (default: the model's) like ``monte_carlo_predictions``
    (nn_models.py:191-207; ``DropoutFF``: the dropout in front of the output layer, :351, the trunk once per stream), and the
    stack / tail hold ``smooth * n`` rows per stream.  An ``ImuPoseLSTM`` ignores n like the reference (nn_models.py:246-251): one
    row per stream and frame, ``smooth`` stacked rows (``nn_models.effective_mc``).  For a ``DropoutFF`` the window has no influence
    (``[:, -1, :]`` of a row-wise MLP): ``seq_len`` is accepted and only the newest row of a stream counts."""

    def __init__(self, model, n_streams: int, seq_len: int, smooth: int = 1, normalize: bool = True,
                 dtype: torch.dtype = torch.float32, monte_carlo_samples=None, dropout=None, seed: int = 0x5EED):
        from . import _hip
        import ctypes as C
        self._hip, self._C = _hip, C
        if dtype not in (torch.float32, torch.float64):
            raise UserWarning(f"StreamBank messages are float32 or float64, not {dtype}")
        self._model, self._n, self._smooth = model, n_streams, smooth
        self._flags = _hip.FLAG_NORMALIZE_INPUT if normalize else 0
        self._dtype, self._sel = dtype, (_hip.F32 if dtype == torch.float32 else _hip.F64)
        self._device = torch.device("cuda", model.device_index)
        handle = C.c_void_p()
        _hip.check(_hip.lib().ape_streams_create(model.handle, n_streams, seq_len, smooth, C.byref(handle)),
                   "ape_streams_create")
        self._handle = handle
        self._n_mc = 1
        if monte_carlo_samples is not None:
            from .estimate.nn_models import effective_mc
            self._n_mc = effective_mc(model, monte_carlo_samples)
            p = float(model.dropout if dropout is None else dropout)
            _hip.check(_hip.lib().ape_streams_set_mc(handle, int(monte_carlo_samples), p, int(seed) & (2 ** 64 - 1)), "ape_streams_set_mc")
        self._msg = torch.empty((n_streams, 25), dtype=dtype, device=self._device)
        self._tail = torch.empty((n_streams, smooth * self._n_mc, 6), dtype=dtype, device=self._device)

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        try:
            if h:
                self._hip.lib().ape_streams_destroy(h)
        except Exception:          # interpreter shutdown: the binding module may already be torn down
            pass

    def _stream(self):
        return self._C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)

    def reset(self, streams=None):
        """cold start.  ``streams=None``: every stream, and the bank is back in lockstep mode; a sequence of distinct stream
        indices: only those (``ape_streams_reset_subset``) -- the bank is then in per-stream mode, see ``frame``"""
        if streams is None:
            self._hip.check(self._hip.lib().ape_streams_reset(self._handle), "ape_streams_reset")
            return
        idx = self._indices(streams)
        self._hip.check(self._hip.lib().ape_streams_reset_subset(self._handle, self._C.c_void_p(idx.ctypes.data), int(idx.shape[0])),
                        "ape_streams_reset_subset")

    def set_bodies(self, bodies, streams=None):
        _set_bodies(self, "ape_streams_set_bodies", bodies, streams)
    set_bodies.__doc__ = _SET_BODIES_DOC

    bodies = property(lambda self: _get_bodies(self, "ape_streams_get_bodies"),
                      doc="float64 [S, 9] mirror of the per-stream bodies; S copies of the model's body before the first set_bodies")

    def set_smooths(self, values, streams=None):
        _set_smooths(self, "ape_streams_set_smooths", values, streams)
    set_smooths.__doc__ = _SET_SMOOTHS_DOC

    smooths = property(lambda self: _get_smooths(self, "ape_streams_get_smooths"),
                       doc="int32 [S] mirror of the per-stream smoothing lengths; S copies of the bank's ``smooth`` before the first set_smooths")

    def datagram_lengths(self) -> np.ndarray:
        """int ``[S]``: the floats of each stream's datagram, ``25 + 6 N_s`` (``N_s = smooths[s] * samples``), or 25 where ``N_s == 1``:
        what the reference sends for an estimator built with that ``smooth``"""
        return datagram_lengths_of(self.smooths, self._n_mc)

    def split_datagrams(self, rows, streams=None):
        """datagram rows of ``step_datagrams`` (``streams=None``: row s is stream s) or of ``frame`` / ``frame_host`` with ``datagrams``
        (row j is stream ``streams[j]``), with or without the spread record behind them -> a list of per-stream float32 views, each cut
        to its stream's ``datagram_lengths()`` entry: byte for byte the reference's payload for that stream"""
        ln = self.datagram_lengths()
        return split_datagrams_of(rows, ln if streams is None else ln[self._indices(streams)])

    def _indices(self, streams) -> np.ndarray:
        a = np.asarray(streams)
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise UserWarning(f"streams must be a sequence of stream indices, got {streams!r}")
        if a.size and (a.min() < 0 or a.max() >= self._n):
            raise UserWarning(f"stream indices must lie in [0, {self._n})")
        if np.unique(a).size != a.size:
            raise UserWarning("stream indices must be distinct")
        return np.ascontiguousarray(a, dtype=np.int32)

    def frame(self, rows, streams, kind: int, big_endian: bool = False, datagrams: bool = False, spread: bool = False):
        """One ``process_row`` for each listed stream (``ape_streams_frame_subset``): ``rows`` float32
        ``[K, 55|28]`` (host array or device tensor), row j for stream ``streams[j]``; ``streams`` K distinct indices.
        Streams not listed are untouched; each stream keeps its own window, stack and cold start (``reset(streams=...)``).
        -> ``[K, 25]`` of the bank's dtype in list order, or with ``datagrams`` float32 ``[K, 25 + 6N]`` (N = smooth x
        samples > 1): per listed stream the ``PoseEstPublisherUDP`` payload, as ``step_datagrams``.  The returned tensor is
        the bank's own buffer, overwritten by the next call.  The first call puts the bank into per-stream mode: ``push_rows``,
        ``push_features`` and ``step`` are refused until ``reset()``.  Monte-Carlo samples depend on a stream's list position.
        ``spread``: every row is ``SPREAD_WIDTH`` columns longer and ends in the stream's spread record (``split_spread``)."""
        hip, C = self._hip, self._C
        if kind not in hip.PARSE_SHAPES:
            raise UserWarning(f"unknown row kind {kind}")
        width = hip.PARSE_SHAPES[kind][0]
        idx = self._indices(streams)
        K = int(idx.shape[0])
        if isinstance(rows, torch.Tensor):
            rd = rows
            if rd.is_cuda and rd.device != self._device:
                raise UserWarning(f"rows live on {rd.device}, the bank on {self._device}")
        else:
            rd = torch.from_numpy(np.asarray(rows))
        if rd.dtype != torch.float32 or tuple(rd.shape) != (K, width):
            raise UserWarning(f"frame wants float32 rows [{K},{width}] for {K} streams, got {rd.dtype} {tuple(rd.shape)}")
        rd = rd.to(self._device).contiguous()
        n = self._smooth * self._n_mc
        packed = datagrams and n > 1
        if datagrams:
            key, dtype, sel, w = "_sub_dgram", torch.float32, hip.F32, (25 + 6 * n if packed else 25)
        else:
            key, dtype, sel, w = "_sub_msg", self._dtype, self._sel, 25
        if spread:
            key, w = key + "_spread", w + hip.SPREAD_WIDTH
        if getattr(self, key, None) is None:
            setattr(self, key, torch.empty((self._n, w), dtype=dtype, device=self._device))
        out = getattr(self, key)[:K]
        if K == 0:
            return out
        flags = self._flags | (hip.FLAG_PACKED_MSG if packed else 0) | (hip.FLAG_SPREAD if spread else 0)
        k = kind | (hip.PARSE_BIG_ENDIAN if big_endian else 0)
        hip.check(hip.lib().ape_streams_frame_subset(self._handle, k, C.c_void_p(rd.data_ptr()), C.c_void_p(idx.ctypes.data), K, flags,
                                                     C.c_void_p(out.data_ptr()), sel, self._stream()), "ape_streams_frame_subset")
        return out

    def frame_host(self, rows, streams, kind: int, big_endian: bool = False, datagrams: bool = False, spread: bool = False) -> np.ndarray:
        """``frame`` host to host (``ape_streams_frame_subset_host``): ``rows`` a float32 HOST array ``[K, 55|28]``,
        row j for stream ``streams[j]`` (K distinct indices) -> a fresh host array with the widths, dtypes and bits of ``frame``.
        BLOCKING: the datagrams are there when the call returns, an aborted cooperative launch has been re-issued (no ``recover()``
        needed) and the frame is counted by ``frame_stats``.  No copy command and no event go onto the stream.  Mode rules are those
        of ``frame``: the first call puts the bank into per-stream mode (``push_rows`` / ``push_features`` / ``step`` refused until
        ``reset()``); ``frame`` and ``frame_host`` mix freely.  Monte-Carlo samples still depend on a stream's list position."""
        hip, C = self._hip, self._C
        if kind not in hip.PARSE_SHAPES:
            raise UserWarning(f"unknown row kind {kind}")
        idx = self._indices(streams)
        K = int(idx.shape[0])
        rh = _host_rows(rows, K, hip.PARSE_SHAPES[kind][0])
        n = self._smooth * self._n_mc
        packed = datagrams and n > 1
        w = (25 + 6 * n if packed else 25) + (hip.SPREAD_WIDTH if spread else 0)
        dtype, sel = (np.float32, hip.F32) if datagrams else ((np.float32 if self._dtype == torch.float32 else np.float64), self._sel)
        out = np.empty((K, w), dtype=dtype)
        if K == 0:
            return out
        flags = self._flags | (hip.FLAG_PACKED_MSG if packed else 0) | (hip.FLAG_SPREAD if spread else 0)
        k = kind | (hip.PARSE_BIG_ENDIAN if big_endian else 0)
        hip.check(hip.lib().ape_streams_frame_subset_host(self._handle, k, C.c_void_p(rh.ctypes.data), C.c_void_p(idx.ctypes.data), K, flags,
                                                          C.c_void_p(out.ctypes.data), sel, self._stream()), "ape_streams_frame_subset_host")
        return out

    def frame_stats(self, reset: bool = False) -> dict:
        """where the host frames' time went (``ape_streams_frame_stats``): frames counted, how many fell through to a stream
        synchronisation, how many were recovered, and per frame (the last <= 4096) the microseconds of ``launch`` (rows and
        descriptors into pinned staging + the launch calls), ``wait`` (until the completion words / the stream) and ``copy``"""
        C = self._C

        class _FS(C.Structure):
            _fields_ = [("frames", C.c_uint64), ("fallback_syncs", C.c_uint64), ("recovered", C.c_uint64)]
        fs, n = _FS(), C.c_int32(0)
        trace = np.zeros((4096, 3), dtype=np.float32)
        self._hip.check(self._hip.lib().ape_streams_frame_stats(self._handle, C.byref(fs), C.c_void_p(trace.ctypes.data), 4096, C.byref(n),
                                                                1 if reset else 0), "ape_streams_frame_stats")
        t = trace[:n.value]
        return {"frames": int(fs.frames), "fallback_syncs": int(fs.fallback_syncs), "recovered": int(fs.recovered),
                "launch_us": t[:, 0].copy(), "wait_us": t[:, 1].copy(), "copy_us": t[:, 2].copy()}

    # ---- state hand-over: a stream's window and stack leave the bank and enter another ----
    def state_desc(self) -> dict:
        return _state.bank_state_desc(self, "ape_streams")
    state_desc.__doc__ = _state.STATE_DESC_DOC

    def export_state(self, streams):
        return _state.bank_export_state(self, "ape_streams", streams)
    export_state.__doc__ = _state.EXPORT_DOC

    def import_state(self, streams, state, warm, desc=None):
        _state.bank_import_state(self, "ape_streams", streams, state, warm, desc)
    import_state.__doc__ = _state.IMPORT_DOC

    def check(self):
        """blocking health check of the model's launches (``ape_model_check``): the bank's outputs stay on the device,
        so the caller decides where to pay for the synchronisation -- e.g. once per batch of frames, before the
        datagrams leave the host"""
        self._model.check()

    def recover(self):
        """like ``check``, but an aborted step is run again on the kernels that need no co-residency (``ape_model_recover``):
        call it behind a step, before the next row is pushed, wherever the datagrams are about to leave the device"""
        self._model.recover()

    def profile(self, enable: bool = True):
        """measurement aid: HIP events around every launch of the step's dominant kernel (``ape_streams_profile``)"""
        self._hip.check(self._hip.lib().ape_streams_profile(self._handle, 1 if enable else 0), "ape_streams_profile")

    def profile_read(self):
        """-> (summed kernel ms, launches) since the last read"""
        ms, n = self._C.c_double(0.0), self._C.c_int32(0)
        self._hip.check(self._hip.lib().ape_streams_profile_read(self._handle, self._C.byref(ms), self._C.byref(n)),
                        "ape_streams_profile_read")
        return float(ms.value), int(n.value)

    def push_rows(self, rows: torch.Tensor, kind: int, big_endian: bool = False):
        """rows: float32 [S, 55|28] on the device -- one raw message per stream (data_types/messaging.py layouts)"""
        width = self._hip.PARSE_SHAPES[kind][0]
        if rows.dtype != torch.float32 or tuple(rows.shape) != (self._n, width) or not rows.is_cuda or not rows.is_contiguous():
            raise UserWarning(f"push_rows wants a contiguous float32 [{self._n},{width}] device tensor")
        k = kind | (self._hip.PARSE_BIG_ENDIAN if big_endian else 0)
        self._hip.check(self._hip.lib().ape_streams_push_rows(self._handle, k, self._C.c_void_p(rows.data_ptr()),
                                                              self._stream()), "ape_streams_push_rows")

    def push_features(self, xx: torch.Tensor):
        """xx: float32 [S, I] on the device -- what ``parse_row_to_xx`` returns, one row per stream"""
        if xx.dtype != torch.float32 or xx.shape[0] != self._n or not xx.is_cuda or not xx.is_contiguous():
            raise UserWarning(f"push_features wants a contiguous float32 [{self._n},I] device tensor")
        self._hip.check(self._hip.lib().ape_streams_push_features(self._handle, self._C.c_void_p(xx.data_ptr()),
                                                                  self._stream()), "ape_streams_push_features")

    def last_post_form(self) -> str:
        """the post-filter form the newest frame of this bank ran (``ape_streams_last_post_form``): ``"none"``, ``"wide"``,
        ``"one workgroup"`` or ``"split xC"``"""
        f = self._C.c_int32(-1)
        self._hip.check(self._hip.lib().ape_streams_last_post_form(self._handle, self._C.byref(f)), "ape_streams_last_post_form")
        return {-1: "none", 0: "wide", 1: "one workgroup"}.get(f.value, f"split x{f.value}")

    @staticmethod
    def split_spread(rows):
        """rows of a ``spread=True`` call -> ``(rows[:, :-21], rows[:, -21:])``: what the call returns without the flag, and the
        spread records (layout: ``estimate._post.spread_rows``)"""
        from . import _hip
        return rows[:, :-_hip.SPREAD_WIDTH], rows[:, -_hip.SPREAD_WIDTH:]

    def step(self, with_tail: bool = False, with_spread: bool = False):
        """-> msg [S,25] (and, with_tail, the hand/elbow xyz of every stacked row [S,smooth*n_mc,6]; and, with_spread, the spread
        record of every stream [S,21] of the bank's dtype: the Monte-Carlo / smoothing spread of the same stacked rows, layout in
        ``estimate._post.spread_rows``); the returned tensors are the bank's own buffers, overwritten by the next step"""
        tail = self._C.c_void_p(self._tail.data_ptr()) if with_tail else None
        if with_spread:
            if getattr(self, "_msg_spread", None) is None:
                self._msg_spread = torch.empty((self._n, 25 + self._hip.SPREAD_WIDTH), dtype=self._dtype, device=self._device)
            self._hip.check(self._hip.lib().ape_streams_step(self._handle, self._flags | self._hip.FLAG_SPREAD,
                                                             self._C.c_void_p(self._msg_spread.data_ptr()), tail, self._sel, self._stream()),
                            "ape_streams_step")
            msg, rec = self.split_spread(self._msg_spread)
            return (msg, self._tail, rec) if with_tail else (msg, rec)
        self._hip.check(self._hip.lib().ape_streams_step(self._handle, self._flags, self._C.c_void_p(self._msg.data_ptr()),
                                                         tail, self._sel, self._stream()), "ape_streams_step")
        return (self._msg, self._tail) if with_tail else self._msg

    def step_datagrams(self, spread: bool = False):
        """-> float32 [S, 25 + 6*smooth*n_mc]: per stream the message followed by the hand/elbow xyz of every stacked
        row -- byte for byte what ``PoseEstPublisherUDP`` sends for one estimator frame (pose_est_udp.py:47 packs
        the list of estimator.py:131-137 as native float32), so ``row.cpu().numpy().tobytes()`` is the datagram.
        Like the reference, rows only carry the tail when there is more than one stacked row.
        ``spread``: every row is ``SPREAD_WIDTH`` columns longer and ends in the stream's spread record as float32
        (``split_spread`` separates the two; the reference has no such record)."""
        n = self._smooth * self._n_mc
        if n == 1:
            if self._dtype != torch.float32:
                raise UserWarning("step_datagrams wants a float32 bank")
            if spread:
                self.step(with_spread=True)
                return self._msg_spread
            return self.step()
        if spread:
            if getattr(self, "_packed_spread", None) is None:
                self._packed_spread = torch.empty((self._n, 25 + 6 * n + self._hip.SPREAD_WIDTH), dtype=torch.float32, device=self._device)
            self._hip.check(self._hip.lib().ape_streams_step(self._handle, self._flags | self._hip.FLAG_PACKED_MSG | self._hip.FLAG_SPREAD,
                                                             self._C.c_void_p(self._packed_spread.data_ptr()), None, self._hip.F32,
                                                             self._stream()), "ape_streams_step")
            return self._packed_spread
        if getattr(self, "_packed", None) is None:
            self._packed = torch.empty((self._n, 25 + 6 * n), dtype=torch.float32, device=self._device)
        self._hip.check(self._hip.lib().ape_streams_step(self._handle, self._flags | self._hip.FLAG_PACKED_MSG,
                                                         self._C.c_void_p(self._packed.data_ptr()), None, self._hip.F32,
                                                         self._stream()), "ape_streams_step")
        return self._packed


class FkStreamBank:
    """The per-frame step of many independent ``WatchPhoneUarm`` streams (the estimator without a regressor) with the smoothing
    stacks on the device (C ABI ``ape_fk_bank_*``): for every stream what one ``WatchPhoneUarm.process_row`` does,
    one launch per frame.  Each stream keeps its own count of rows since its cold start, so lockstep frames (``step_rows``) and
    subset frames (``frame``) mix freely.  Rank-local: give each rank its ``shard_range`` of streams.

    ``bonemap``: an object with ``left_lower_arm_length``, ``left_upper_arm_length`` and ``left_upper_arm_origin_rh`` (None: the
    defaults), as ``Estimator``.  ``dtype``: of the messages, float32 (the ``PoseEstPublisherUDP`` payload) or float64."""

    def __init__(self, n_streams: int, smooth: int = 5, bonemap=None, dtype: torch.dtype = torch.float32, device=None):
        from . import _hip
        from .data_types.bone_map import body9_from_bonemap
        import ctypes as C
        self._hip, self._C = _hip, C
        if dtype not in (torch.float32, torch.float64):
            raise UserWarning(f"FkStreamBank messages are float32 or float64, not {dtype}")
        if int(n_streams) < 1:
            raise UserWarning(f"FkStreamBank needs n_streams >= 1, got {n_streams}")
        self._n, self._smooth = int(n_streams), max(1, int(smooth))
        self._dtype, self._sel = dtype, (_hip.F32 if dtype == torch.float32 else _hip.F64)
        if device is None:
            device = torch.cuda.current_device()
        self._device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self._device.index is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        self._body = body9_from_bonemap(bonemap)
        handle = C.c_void_p()
        _hip.check(_hip.lib().ape_fk_bank_create(self._n, self._smooth, _hip.dptr(self._body, C.c_double), self._device.index,
                                                 C.byref(handle)), "ape_fk_bank_create")
        self._handle = handle
        self._msg = torch.empty((self._n, 25), dtype=dtype, device=self._device)
        self._sub_msg = torch.empty((self._n, 25), dtype=dtype, device=self._device)

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        try:
            if h:
                self._hip.lib().ape_fk_bank_destroy(h)
        except Exception:          # interpreter shutdown
            pass

    body_measurements = property(lambda self: self._body[np.newaxis, :].copy())

    def set_bodies(self, bodies, streams=None):
        _set_bodies(self, "ape_fk_bank_set_bodies", bodies, streams)
    set_bodies.__doc__ = _SET_BODIES_DOC

    bodies = property(lambda self: _get_bodies(self, "ape_fk_bank_get_bodies"),
                      doc="float64 [S, 9] mirror of the per-stream bodies; S copies of ``body_measurements`` before the first set_bodies")

    def set_smooths(self, values, streams=None):
        _set_smooths(self, "ape_fk_bank_set_smooths", values, streams)
    set_smooths.__doc__ = _SET_SMOOTHS_DOC

    smooths = property(lambda self: _get_smooths(self, "ape_fk_bank_get_smooths"),
                       doc="int32 [S] mirror of the per-stream smoothing lengths; S copies of the bank's ``smooth`` before the first set_smooths")

    def datagram_lengths(self) -> np.ndarray:
        """int ``[S]``: ``25 + 6 smooths[s]``, or 25 where ``smooths[s] == 1`` -- the floats the reference sends for an estimator built
        with that ``smooth``.  The bank's own frames return the 25-value messages only."""
        return datagram_lengths_of(self.smooths, 1)

    def split_datagrams(self, rows, streams=None):
        """rows ``[K, w]``, row j for stream ``streams[j]`` (``None``: row s for stream s) -> a list of views cut to each stream's
        ``datagram_lengths()`` entry"""
        ln = self.datagram_lengths()
        return split_datagrams_of(rows, ln if streams is None else ln[self._indices(streams)])

    def _stream(self):
        return self._C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)

    _indices = StreamBank._indices          # in range, distinct, int32

    def _rows(self, rows, K: int):
        if isinstance(rows, torch.Tensor):
            rd = rows
            if rd.is_cuda and rd.device != self._device:
                raise UserWarning(f"rows live on {rd.device}, the bank on {self._device}")
        else:
            rd = torch.from_numpy(np.asarray(rows))
        if rd.dtype != torch.float32 or tuple(rd.shape) != (K, 55):
            raise UserWarning(f"the bank wants float32 rows [{K},55] (WATCH_PHONE_IMU messages), got {rd.dtype} {tuple(rd.shape)}")
        return rd.to(self._device).contiguous()

    def reset(self, streams=None):
        """cold start: ``streams=None`` every stream, else only the listed (distinct) ones"""
        if streams is None:
            self._hip.check(self._hip.lib().ape_fk_bank_reset(self._handle), "ape_fk_bank_reset")
            return
        idx = self._indices(streams)
        self._hip.check(self._hip.lib().ape_fk_bank_reset_subset(self._handle, self._C.c_void_p(idx.ctypes.data), int(idx.shape[0])),
                        "ape_fk_bank_reset_subset")

    # ---- state hand-over: the record is the stack alone, [smooth][8] float64 quaternion pairs (T = I = 0) ----
    def state_desc(self) -> dict:
        return _state.bank_state_desc(self, "ape_fk_bank")
    state_desc.__doc__ = _state.STATE_DESC_DOC

    def export_state(self, streams):
        return _state.bank_export_state(self, "ape_fk_bank", streams)
    export_state.__doc__ = _state.EXPORT_DOC

    def import_state(self, streams, state, warm, desc=None):
        _state.bank_import_state(self, "ape_fk_bank", streams, state, warm, desc)
    import_state.__doc__ = _state.IMPORT_DOC

    def step_rows(self, rows, big_endian: bool = False):
        """lockstep frame: float32 ``[S, 55]`` rows (host array or device tensor), row s for stream s -> ``[S, 25]`` messages (the
        bank's own buffer, overwritten by the next lockstep frame)"""
        hip, C = self._hip, self._C
        rd = self._rows(rows, self._n)
        kind = hip.PARSE_WATCH_PHONE_UARM | (hip.PARSE_BIG_ENDIAN if big_endian else 0)
        hip.check(hip.lib().ape_fk_bank_frame(self._handle, kind, C.c_void_p(rd.data_ptr()), None, self._n,
                                              C.c_void_p(self._msg.data_ptr()), self._sel, self._stream()), "ape_fk_bank_frame")
        return self._msg

    def frame(self, rows, streams, big_endian: bool = False):
        """subset frame: float32 ``[K, 55]`` rows, row j for stream ``streams[j]`` (K distinct indices) -> ``[K, 25]`` in list order
        (the bank's own buffer, overwritten by the next subset frame).  Streams not listed are untouched."""
        hip, C = self._hip, self._C
        idx = self._indices(streams)
        K = int(idx.shape[0])
        rd = self._rows(rows, K)
        out = self._sub_msg[:K]
        if K == 0:
            return out
        kind = hip.PARSE_WATCH_PHONE_UARM | (hip.PARSE_BIG_ENDIAN if big_endian else 0)
        hip.check(hip.lib().ape_fk_bank_frame(self._handle, kind, C.c_void_p(rd.data_ptr()), C.c_void_p(idx.ctypes.data), K,
                                              C.c_void_p(out.data_ptr()), self._sel, self._stream()), "ape_fk_bank_frame")
        return out

    def frame_host(self, rows, streams, big_endian: bool = False) -> np.ndarray:
        """``frame`` host to host (``ape_fk_bank_frame_subset_host``): float32 HOST rows ``[K, 55]`` -> a fresh host
        array ``[K, 25]`` of the bank's dtype with the bits of ``frame``.  BLOCKING; no copy command and no event on the stream.
        Lockstep frames, ``frame`` and ``frame_host`` mix freely: every stream keeps its own count."""
        hip, C = self._hip, self._C
        idx = self._indices(streams)
        K = int(idx.shape[0])
        rh = _host_rows(rows, K, 55)
        out = np.empty((K, 25), dtype=np.float32 if self._dtype == torch.float32 else np.float64)
        if K == 0:
            return out
        kind = hip.PARSE_WATCH_PHONE_UARM | (hip.PARSE_BIG_ENDIAN if big_endian else 0)
        hip.check(hip.lib().ape_fk_bank_frame_subset_host(self._handle, kind, C.c_void_p(rh.ctypes.data), C.c_void_p(idx.ctypes.data), K,
                                                          C.c_void_p(out.ctypes.data), self._sel, self._stream()),
                  "ape_fk_bank_frame_subset_host")
        return out


def trim_packed(row, n_rows: int):
    """a packed row ``[25 + 6 * smooth * E]`` of a Kalman bank cut to what the reference sends (estimator.py:131-137): the 25-value
    message, followed by hand and elbow xyz of the ``n_rows`` stacked rows when there is more than one"""
    n = int(n_rows)
    return row[:25 + 6 * n] if n > 1 else row[:25]


class KalmanStreamBank:
    """The per-frame step of many independent ``WatchPhonePocketKalman`` streams with every history on the device (C ABI
    ``ape_kalman_bank_*``): for every listed stream what one ``WatchPhonePocketKalman.process_row`` does -- feature
    builder, window, float64 z-score, the ensemble Kalman model on the stream's own state history, the sensor mean on the stream's
    first W + 1 frames and the corrected ensemble afterwards, de-normalisation, the smoothing stack with its ragged entries, FK and
    message.  PARITY UNPINNED (see ``estimate/kalman_models.py``): the checker is the oracle's restatement.

    ``model``: a loaded ``kalman_models.KalmanSmartwatchModel`` (the bank keeps it alive).  Each stream keeps its own count of frames
    since its cold start, so lockstep frames (``step_rows``) and subset frames (``frame``) mix freely.  One flipout draw per call is
    shared by the call's streams; the signs and ``format_state`` draws of a stream depend on its list position.  ``seed`` keys the
    device-side draws together with the number of the call: two banks with one seed fed the same calls return the same bits."""

    def __init__(self, model, n_streams: int, smooth: int = 1, normalize: bool = True, bonemap=None, seed: int = 0x5EED,
                 dtype: torch.dtype = torch.float64):
        from . import _hip
        from .data_types.bone_map import body9_from_bonemap
        import ctypes as C
        self._hip, self._C = _hip, C
        if dtype not in (torch.float32, torch.float64):
            raise UserWarning(f"KalmanStreamBank messages are float32 or float64, not {dtype}")
        if int(n_streams) < 1:
            raise UserWarning(f"KalmanStreamBank needs n_streams >= 1, got {n_streams}")
        self._model = model
        self._n, self._smooth = int(n_streams), max(1, int(smooth))
        self._E, self._W = int(model._num_ensemble), int(model.win_size)
        self._dtype, self._sel = dtype, (_hip.F32 if dtype == torch.float32 else _hip.F64)
        self._device = model.torch_device
        handle = C.c_void_p()
        _hip.check(_hip.lib().ape_kalman_bank_create(model.handle, self._n, self._smooth, C.byref(handle)), "ape_kalman_bank_create")
        self._handle = handle
        self.set_body(body9_from_bonemap(bonemap))
        if normalize:
            from .utility import data_stats
            from .utility.names import NNS_INPUTS, NNS_TARGETS
            self.set_norm_stats(data_stats.get_norm_stats(x_inputs=NNS_INPUTS.WATCH_PHONE_CAL_HIP, y_targets=NNS_TARGETS.ORI_CAL_LARM_UARM_HIPS))
        self.manual_seed(seed)
        self._width = 25 + 6 * self._smooth * self._E
        self._bufs = {}

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        try:
            if h:
                self._hip.lib().ape_kalman_bank_destroy(h)
        except Exception:          # interpreter shutdown
            pass

    n_streams = property(lambda self: self._n)
    packed_width = property(lambda self: self._width)
    body_measurements = property(lambda self: self._body[np.newaxis, :].copy())

    def set_bodies(self, bodies, streams=None):
        _set_bodies(self, "ape_kalman_bank_set_bodies", bodies, streams)
    set_bodies.__doc__ = _SET_BODIES_DOC

    bodies = property(lambda self: _get_bodies(self, "ape_kalman_bank_get_bodies"),
                      doc="float64 [S, 9] mirror of the per-stream bodies; S copies of ``body_measurements`` before the first set_bodies")

    def set_body(self, body9):
        """one body for every stream; on a bank that was given per-stream bodies it overwrites every row"""
        self._body = np.ascontiguousarray(np.asarray(body9, dtype=np.float64).reshape(9))
        self._hip.check(self._hip.lib().ape_kalman_bank_set_body(self._handle, self._hip.dptr(self._body, self._C.c_double)),
                        "ape_kalman_bank_set_body")

    def set_norm_stats(self, stats: dict):
        """float64 statistics ``xx_m, xx_s`` [22] and ``yy_m, yy_s`` [14]; from the next frame on"""
        a = [np.ascontiguousarray(np.asarray(stats[k], dtype=np.float64).reshape(-1)) for k in ("xx_m", "xx_s", "yy_m", "yy_s")]
        if [v.size for v in a] != [22, 22, 14, 14]:
            raise UserWarning(f"the Kalman bank wants 22 input and 14 target statistics, got {[v.size for v in a]}")
        self._hip.check(self._hip.lib().ape_kalman_bank_set_norm_stats(self._handle, *[self._hip.dptr(v, self._C.c_double) for v in a]),
                        "ape_kalman_bank_set_norm_stats")

    def manual_seed(self, seed: int):
        """seed of the device-side draws; the call counter starts again"""
        self._hip.check(self._hip.lib().ape_kalman_bank_set_seed(self._handle, int(seed) & (2 ** 64 - 1)), "ape_kalman_bank_set_seed")
        return self

    def _stream(self):
        return self._C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)

    def reset(self, streams=None):
        """cold start: ``streams=None`` every stream, else only the listed (distinct) ones"""
        if streams is None:
            self._hip.check(self._hip.lib().ape_kalman_bank_reset(self._handle), "ape_kalman_bank_reset")
            return
        idx = self._indices(streams)
        self._hip.check(self._hip.lib().ape_kalman_bank_reset_subset(self._handle, self._C.c_void_p(idx.ctypes.data), int(idx.shape[0])),
                        "ape_kalman_bank_reset_subset")

    def _buf(self, key, shape, dtype):
        if key not in self._bufs:
            self._bufs[key] = torch.empty(shape, dtype=dtype, device=self._device)
        return self._bufs[key]

    _indices = StreamBank._indices          # in range, distinct, int32
    _rows = FkStreamBank._rows
    split_spread = staticmethod(StreamBank.split_spread)      # rows of a ``spread=True`` call -> (unflagged part, records [., 21])

    def _frame(self, rows, idx, big_endian, datagrams, noise, init_noise, return_targets, tag, spread=False):
        hip, C = self._hip, self._C
        K = self._n if idx is None else int(idx.shape[0])
        rd = self._rows(rows, K)
        w = (self._width if datagrams else 25) + (hip.SPREAD_WIDTH if spread else 0)
        # (flagged frames have buffers of their own: an unflagged call's buffer keeps its shape)
        out = self._buf((tag, "out", datagrams) + (("spread",) if spread else ()), (self._n, w), self._dtype)[:K]
        n_rows = self._buf((tag, "n"), (self._n,), torch.int32)[:K]
        y = self._buf((tag, "y"), (self._n, self._E, 14), torch.float32)[:K] if return_targets else None
        res = (out, n_rows) if datagrams else out
        if return_targets:
            res = (res + (y,)) if datagrams else (out, y)
        if K == 0:
            return res
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
        nz = ini = None
        if noise is not None:
            nz = torch.as_tensor(noise, dtype=torch.float32).to(self._device).contiguous()
            if nz.numel() != self._model.noise_floats(K):
                raise UserWarning(f"frame noise must hold {self._model.noise_floats(K)} values for {K} streams")
        if init_noise is not None:
            ini = torch.as_tensor(init_noise, dtype=torch.float32).to(self._device).contiguous()
            if ini.numel() != K * self._E * 14:
                raise UserWarning(f"frame init_noise must hold [{K},{self._E},14] values")
        kind = hip.PARSE_WATCH_PHONE_POCKET | (hip.PARSE_BIG_ENDIAN if big_endian else 0)
        hip.check(hip.lib().ape_kalman_bank_frame(self._handle, kind, p(rd), C.c_void_p(idx.ctypes.data) if idx is not None else None, K,
                                                  p(nz), p(ini), (hip.FLAG_PACKED_MSG if datagrams else 0) | (hip.FLAG_SPREAD if spread else 0),
                                                  p(out), self._sel, p(n_rows),
                                                  p(y), self._stream()), "ape_kalman_bank_frame")
        self._keep = (rd, nz, ini)           # the launches read them behind this call
        return res

    def step_rows(self, rows, big_endian: bool = False, datagrams: bool = False, noise=None, init_noise=None, return_targets: bool = False,
                  spread: bool = False):
        """lockstep frame: float32 ``[S, 55]`` rows (host array or device tensor), row s for stream s -> ``[S, 25]`` messages of the
        bank's dtype; see ``frame`` for the other arguments.  The bank's own buffers, overwritten by the next lockstep frame."""
        return self._frame(rows, None, big_endian, datagrams, noise, init_noise, return_targets, "step", spread)

    def frame(self, rows, streams, big_endian: bool = False, datagrams: bool = False, noise=None, init_noise=None,
              return_targets: bool = False, spread: bool = False):
        """subset frame: float32 ``[K, 55]`` rows, row j for stream ``streams[j]`` (K distinct indices) -> ``[K, 25]`` in list order.
        Streams not listed are untouched.  ``datagrams``: ``([K, 25 + 6 * smooth * E], n_rows int32 [K])`` instead -- the message,
        hand and elbow xyz of the ``n_rows[j]`` stacked rows, zeros; ``trim_packed(row, n)`` cuts a row to the reference's length.
        ``return_targets`` appends the frame's normalised predictions float32 ``[K, E, 14]`` (row 0 alone while a stream is in its
        first W + 1 frames).  ``noise`` / ``init_noise`` inject the draws of this call (``ape_kalman_noise_floats(K)`` values and
        ``[K, E, 14]``): tests.  ``spread``: every row, message or datagram, is ``SPREAD_WIDTH`` = 21 columns longer
        and ends in the spread record of the entry's ``n_rows[j]`` stacked rows (layout: ``estimate._post.spread_rows``;
        ``split_spread(rows)`` separates the two, ``trim_packed`` takes the unflagged part) -- the corrected ensemble's spread once the
        stream is past its first W + 1 frames, the smoothing lag of the sensor means before (one row: origins and zeros); flagged
        frames use buffers of their own.  The bank's own buffers, overwritten by the next subset frame of the same kind."""
        return self._frame(rows, self._indices(streams), big_endian, datagrams, noise, init_noise, return_targets, "sub", spread)

    def frame_host(self, rows, streams, big_endian: bool = False, datagrams: bool = False, spread: bool = False):
        """``frame`` host to host (``ape_kalman_bank_frame_subset_host``): float32 HOST rows ``[K, 55]`` -> a fresh
        host array ``[K, 25]`` of the bank's dtype, or with ``datagrams`` ``([K, 25 + 6 * smooth * E], n_rows int32 [K])``, as
        ``frame`` returns them (``spread``: 21 columns more) -- the same bits, the same call counter behind the draw keys.
        BLOCKING; no copy command and no event on the stream; a singular innovation is still reported by ``check()``.  ``noise`` /
        ``init_noise`` injection and ``return_targets`` stay on ``frame``.  Lockstep frames, ``frame`` and ``frame_host`` mix freely;
        the signs and ``format_state`` draws of a stream depend on its list position."""
        hip, C = self._hip, self._C
        idx = self._indices(streams)
        K = int(idx.shape[0])
        rh = _host_rows(rows, K, 55)
        w = (self._width if datagrams else 25) + (hip.SPREAD_WIDTH if spread else 0)
        out = np.empty((K, w), dtype=np.float32 if self._dtype == torch.float32 else np.float64)
        n_rows = np.zeros((K,), dtype=np.int32)
        if K:
            kind = hip.PARSE_WATCH_PHONE_POCKET | (hip.PARSE_BIG_ENDIAN if big_endian else 0)
            hip.check(hip.lib().ape_kalman_bank_frame_subset_host(
                self._handle, kind, C.c_void_p(rh.ctypes.data), C.c_void_p(idx.ctypes.data), K,
                (hip.FLAG_PACKED_MSG if datagrams else 0) | (hip.FLAG_SPREAD if spread else 0), C.c_void_p(out.ctypes.data), self._sel,
                C.c_void_p(n_rows.ctypes.data), self._stream()), "ape_kalman_bank_frame_subset_host")
        return (out, n_rows) if datagrams else out

    # ---- state hand-over ----
    def state_desc(self) -> dict:
        """the bank's ``ape_kalman_state_desc_t`` as a dict: ``version, E, W, smooth, words_per_stream``"""
        from . import stream_state as ss
        d = self._hip.ApeKalmanStateDesc()
        self._hip.check(self._hip.lib().ape_kalman_bank_state_desc(self._handle, self._C.byref(d)), "ape_kalman_bank_state_desc")
        return {k: int(getattr(d, k)) for k in ss.KALMAN_DESC_KEYS}

    def export_state(self, streams):
        """-> ``(state, age)``: float32 words ``[K, words_per_stream]`` on the device, record j the canonical state of stream
        ``streams[j]`` (``stream_state.kalman_unpack`` gives its time-ordered window, state history, stack and row counts), and
        ``np.int32 [K]`` ages, ``min(frames since the cold start, W + 1)``: 0 cold (a zero record), 1..W the init phase, W + 1
        mature.  Read-only, one launch on the current stream, no synchronisation.  Bodies are NOT part of the record (``bodies`` /
        ``set_bodies`` move them), nor is the draw position (``get_draw_position``)."""
        C = self._C
        idx = self._indices(streams)
        K = int(idx.shape[0])
        # (the launch writes every word of every record: no fill in front of it)
        state = torch.empty((K, self.state_desc()["words_per_stream"]), dtype=torch.float32, device=self._device)
        age = np.zeros((K,), dtype=np.int32)
        if K:
            self._hip.check(self._hip.lib().ape_kalman_bank_export(self._handle, C.c_void_p(idx.ctypes.data), K, C.c_void_p(state.data_ptr()),
                                                                   C.c_void_p(age.ctypes.data), self._stream()), "ape_kalman_bank_export")
        return state, age

    def import_state(self, streams, state, age, desc=None):
        """the reverse of ``export_state``: the listed streams continue from the given records (from this bank, another bank or GPU,
        a replay's ``return_state``, or ``WatchPhonePocketKalman.get_state``); ``desc`` (default: this bank's own) must equal this
        bank's ``state_desc()``.  A stream with age 0 is cold-started as by ``reset(streams=)``.  Streams not listed stay untouched.
        Bodies are NOT part of the record: move them with ``set_bodies``.  The imported stream draws the samples of THIS bank and its
        list position; ``set_draw_position(*source.get_draw_position())`` continues the source bank's sequence."""
        from . import stream_state as ss
        C = self._C
        idx = self._indices(streams)
        K = int(idx.shape[0])
        own = self.state_desc()
        src = own if desc is None else desc
        missing = [k for k in ss.KALMAN_DESC_KEYS if k not in src]
        if missing:
            raise UserWarning(f"state descriptor lacks {missing}")
        d = self._hip.ApeKalmanStateDesc(*[int(src[k]) for k in ss.KALMAN_DESC_KEYS])
        state = ss.kalman_records_tensor(state, K, int(d.words_per_stream), self._device)
        a = np.ascontiguousarray(np.asarray(age, dtype=np.int32).reshape(-1))
        if a.shape[0] != K:
            raise UserWarning(f"import_state wants {K} ages, got {a.shape[0]}")
        self._hip.check(self._hip.lib().ape_kalman_bank_import(self._handle, C.byref(d), C.c_void_p(idx.ctypes.data), K,
                                                               C.c_void_p(state.data_ptr()), C.c_void_p(a.ctypes.data), self._stream()),
                        "ape_kalman_bank_import")
        self._state_keep = state           # the launch reads it behind this call

    def get_draw_position(self):
        """-> ``(seed, calls)``: the seed of the device-side draws and the number of frames this bank has issued since it was set"""
        C = self._C
        seed, calls = C.c_uint64(), C.c_uint64()
        self._hip.check(self._hip.lib().ape_kalman_bank_get_draw_position(self._handle, C.byref(seed), C.byref(calls)),
                        "ape_kalman_bank_get_draw_position")
        return int(seed.value), int(calls.value)

    def set_draw_position(self, seed: int, calls: int):
        """continue another bank's draw sequence: the next frame draws with the key of call ``calls + 1`` under ``seed``"""
        self._hip.check(self._hip.lib().ape_kalman_bank_set_draw_position(self._handle, int(seed) & (2 ** 64 - 1), int(calls) & (2 ** 64 - 1)),
                        "ape_kalman_bank_set_draw_position")
        return self

    def check(self):
        """blocking: raises if a frame met an exactly singular innovation matrix (``ape_kalman_check``)"""
        self._model.check()
