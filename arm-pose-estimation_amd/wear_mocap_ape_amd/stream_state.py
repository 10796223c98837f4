"""The canonical per-stream state record (C ABI ``ape_stream_state_desc_t``) restated in numpy, and the
``state_desc`` / ``export_state`` / ``import_state`` of the banks.

A record is ``words_per_stream`` 4-byte words: ``window[T][I]`` float32 (the stream's feature rows, oldest first), ``stack[smooth]
[n_mc][O]`` float32 (the model outputs of its last ``smooth`` frames, oldest first), zero words up to the next multiple of 4 (records
are 16-byte units).  It does not depend on ring phase, slot or bank.  Two warm bits per stream travel beside it on the host:
``WINDOW_WARM`` (at least one row since the cold start) and ``STACK_WARM`` (at least one prediction).  Bodies and the Philox position
are not part of it.

The Kalman bank's record (``ape_kalman_state_desc_t``) is restated at the end: ``kalman_words``, ``kalman_pack``,
``kalman_unpack``."""
import numpy as np

VERSION = 1
WINDOW_WARM, STACK_WARM = 1, 2
DESC_KEYS = ("version", "T", "I", "smooth", "n_mc", "O", "words_per_stream")


def words_per_stream(T: int, I: int, smooth: int, n_mc: int, O: int) -> int:
    """``T*I + smooth*n_mc*O`` rounded up to a multiple of 4 words (16 bytes)"""
    return (T * I + smooth * n_mc * O + 3) & ~3


def make_desc(T: int, I: int, smooth: int, n_mc: int, O: int) -> dict:
    return {"version": VERSION, "T": int(T), "I": int(I), "smooth": int(smooth), "n_mc": int(n_mc), "O": int(O),
            "words_per_stream": words_per_stream(T, I, smooth, n_mc, O)}


def pack(window, stack) -> np.ndarray:
    """``window`` [T, I] and ``stack`` [smooth, n_mc, O] (time order, oldest first) -> one float32 record [words]"""
    w = np.asarray(window, dtype=np.float32)
    s = np.asarray(stack, dtype=np.float32)
    if w.ndim != 2 or s.ndim != 3:
        raise UserWarning(f"pack wants window [T,I] and stack [smooth,n_mc,O], got {w.shape} and {s.shape}")
    out = np.zeros((words_per_stream(w.shape[0], w.shape[1], *s.shape),), dtype=np.float32)
    out[:w.size] = w.reshape(-1)
    out[w.size:w.size + s.size] = s.reshape(-1)
    return out


def unpack(record, desc: dict):
    """one record -> (window [T, I], stack [smooth, n_mc, O]) float32 copies"""
    r = np.asarray(record, dtype=np.float32).reshape(-1)
    T, I, smooth, n_mc, O = (int(desc[k]) for k in ("T", "I", "smooth", "n_mc", "O"))
    if r.size != words_per_stream(T, I, smooth, n_mc, O):
        raise UserWarning(f"a record of {r.size} words does not match {desc}")
    nx, ny = T * I, smooth * n_mc * O
    return r[:nx].reshape(T, I).copy(), r[nx:nx + ny].reshape(smooth, n_mc, O).copy()


# ---- the banks' three methods (StreamBank: ape_streams_*, FkStreamBank: ape_fk_bank_*) ------------------------------------------------

def _desc_struct(hip, desc: dict):
    missing = [k for k in DESC_KEYS if k not in desc]
    if missing:
        raise UserWarning(f"state descriptor lacks {missing}")
    return hip.ApeStreamStateDesc(*[int(desc[k]) for k in DESC_KEYS])


def bank_state_desc(bank, prefix: str) -> dict:
    d = bank._hip.ApeStreamStateDesc()
    bank._hip.check(getattr(bank._hip.lib(), prefix + "_state_desc")(bank._handle, bank._C.byref(d)), prefix + "_state_desc")
    return {k: int(getattr(d, k)) for k in DESC_KEYS}


def bank_export_state(bank, prefix: str, streams):
    import torch
    C = bank._C
    idx = bank._indices(streams)
    K = int(idx.shape[0])
    words = bank_state_desc(bank, prefix)["words_per_stream"]
    state = torch.zeros((K, words), dtype=torch.float32, device=bank._device)
    warm = np.zeros((K,), dtype=np.uint8)
    if K:
        bank._hip.check(getattr(bank._hip.lib(), prefix + "_export")(bank._handle, C.c_void_p(idx.ctypes.data), K, C.c_void_p(state.data_ptr()),
                                                                     C.c_void_p(warm.ctypes.data), bank._stream()), prefix + "_export")
    return state, warm


def bank_import_state(bank, prefix: str, streams, state, warm, desc=None):
    import torch
    C = bank._C
    idx = bank._indices(streams)
    K = int(idx.shape[0])
    own = bank_state_desc(bank, prefix)
    d = _desc_struct(bank._hip, own if desc is None else desc)
    words = int(d.words_per_stream)
    if not isinstance(state, torch.Tensor):
        state = torch.from_numpy(np.ascontiguousarray(state))
    if state.dtype == torch.uint8:
        state = state.contiguous().view(torch.float32)
    if state.dtype != torch.float32 or state.dim() != 2 or state.shape[0] != K or state.shape[1] != words:
        raise UserWarning(f"import_state wants {K} records of {words} words, got {state.dtype} {tuple(state.shape)}")
    if state.is_cuda and state.device != bank._device:
        raise UserWarning(f"the records live on {state.device}, the bank on {bank._device}")
    state = state.to(bank._device).contiguous()
    w = np.ascontiguousarray(np.asarray(warm, dtype=np.uint8).reshape(-1))
    if w.shape[0] != K:
        raise UserWarning(f"import_state wants {K} warm bytes, got {w.shape[0]}")
    bank._hip.check(getattr(bank._hip.lib(), prefix + "_import")(bank._handle, C.byref(d), C.c_void_p(idx.ctypes.data), K,
                                                                 C.c_void_p(state.data_ptr()), C.c_void_p(w.ctypes.data), bank._stream()),
                    prefix + "_import")
    bank._state_keep = state           # the launch reads it behind this call


STATE_DESC_DOC = """the bank's ``ape_stream_state_desc_t`` as a dict: ``version, T, I, smooth, n_mc, O, words_per_stream``"""
EXPORT_DOC = """-> ``(state, warm)``: float32 ``[K, words_per_stream]`` on the device, record j the canonical state of stream
        ``streams[j]`` (``stream_state.unpack`` gives its time-ordered window and stack), and ``np.uint8 [K]`` warm bits
        (``stream_state.WINDOW_WARM``, ``STACK_WARM``).  Read-only, one launch on the current stream, no synchronisation; a lockstep
        bank stays in lockstep mode.  Bodies are NOT part of the record (``bodies`` / ``set_bodies`` move them), nor is the
        Monte-Carlo seed or call counter.  A bank with per-stream smoothing lengths (``set_smooths``, DESIGN.md 4.35) keeps the record
        size of its capacity: the stack part holds stream s's ``smooths[s]`` predictions oldest first, followed by zeros; the length
        itself is NOT part of the record."""
IMPORT_DOC = """the reverse of ``export_state``: the listed streams continue from the given records (from this bank, another
        bank or GPU, a replay, or ``Estimator.get_state``); ``desc`` (default: this bank's own) must equal this bank's
        ``state_desc()``.  A stream whose ``WINDOW_WARM`` bit is clear is cold-started, one with only ``STACK_WARM`` clear keeps the
        window and gets a cold stack.  Puts the bank into per-stream mode like ``frame``; streams not listed stay untouched.  Bodies
        are NOT part of the record: move them with ``set_bodies``.  A pending frame that ``recover`` could still re-issue is dropped
        from the journal: recover first if its outputs are still wanted.  In a bank with per-stream smoothing lengths the record is
        read with the TARGET slot's length: to move a stream, first ``set_smooths`` the slot to the source's value (a cold start of the
        slot), then ``import_state`` (which warms it)."""


# ---- the Kalman bank's record (C ABI ``ape_kalman_state_desc_t``) -------------------------------------------------------
# 4-byte words, every part oldest first: window float64 [W, 22], state history float32 [E, W, 14] (time step minor; entries that do not
# exist yet are zeros), stack float32 [smooth, E, 14] (normalised predictions; rows at or beyond an entry's count are zeros), counts
# int32 [smooth] (1 or E), zero words up to a multiple of 4.  Beside it on the host: ``age = min(frames since the cold start, W + 1)``.

KALMAN_VERSION = 1
KALMAN_DESC_KEYS = ("version", "E", "W", "smooth", "words_per_stream")


def kalman_words(E: int, W: int, smooth: int) -> int:
    """``2*W*22 + E*W*14 + smooth*E*14 + smooth`` rounded up to a multiple of 4 words (16 bytes)"""
    return (2 * W * 22 + E * W * 14 + smooth * E * 14 + smooth + 3) & ~3


def kalman_desc(E: int, W: int, smooth: int) -> dict:
    return {"version": KALMAN_VERSION, "E": int(E), "W": int(W), "smooth": int(smooth), "words_per_stream": kalman_words(E, W, smooth)}


def kalman_pack(window, history, stack, counts) -> np.ndarray:
    """``window`` [W, 22] float64, ``history`` [E, W, 14], ``stack`` [smooth, E, 14] float32 and ``counts`` [smooth] int32 (time order,
    oldest first) -> one record as float32 words [words] (the float64 and int32 parts keep their bits)"""
    w = np.ascontiguousarray(window, dtype=np.float64)
    h = np.ascontiguousarray(history, dtype=np.float32)
    s = np.ascontiguousarray(stack, dtype=np.float32)
    c = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if w.ndim != 2 or w.shape[1] != 22 or h.ndim != 3 or h.shape[1:] != (w.shape[0], 14) or s.shape != (c.shape[0], h.shape[0], 14):
        raise UserWarning(f"kalman_pack wants window [W,22], history [E,W,14], stack [smooth,E,14], counts [smooth], got {w.shape}, "
                          f"{h.shape}, {s.shape}, {c.shape}")
    out = np.zeros((kalman_words(h.shape[0], w.shape[0], c.shape[0]),), dtype=np.float32)
    parts = (w.reshape(-1).view(np.float32), h.reshape(-1), s.reshape(-1), c.view(np.float32))
    at = 0
    for part in parts:
        out[at:at + part.size] = part
        at += part.size
    return out


def kalman_unpack(record, desc: dict):
    """one record -> (window float64 [W, 22], history float32 [E, W, 14], stack float32 [smooth, E, 14], counts int32 [smooth], padding
    float32 words) as copies"""
    r = np.ascontiguousarray(np.asarray(record).reshape(-1))
    if r.dtype != np.float32:
        raise UserWarning(f"a Kalman record is float32 words, got {r.dtype}")
    E, W, smooth = (int(desc[k]) for k in ("E", "W", "smooth"))
    if r.size != kalman_words(E, W, smooth):
        raise UserWarning(f"a record of {r.size} words does not match {desc}")
    nw, nh, ns = 2 * W * 22, E * W * 14, smooth * E * 14
    window = r[:nw].view(np.float64).reshape(W, 22).copy()
    history = r[nw:nw + nh].reshape(E, W, 14).copy()
    stack = r[nw + nh:nw + nh + ns].reshape(smooth, E, 14).copy()
    counts = r[nw + nh + ns:nw + nh + ns + smooth].view(np.int32).copy()
    return window, history, stack, counts, r[nw + nh + ns + smooth:].copy()


def kalman_records_tensor(state, K: int, words: int, device):
    """records given as a device / host tensor or array -> contiguous float32 [K, words] on ``device``"""
    import torch
    if not isinstance(state, torch.Tensor):
        state = torch.from_numpy(np.ascontiguousarray(state))
    if state.dtype != torch.float32 or state.dim() != 2 or state.shape[0] != K or state.shape[1] != words:
        raise UserWarning(f"wanted {K} records of {words} float32 words, got {state.dtype} {tuple(state.shape)}")
    if state.is_cuda and state.device != device:
        raise UserWarning(f"the records live on {state.device}, the bank on {device}")
    return state.to(device).contiguous()
