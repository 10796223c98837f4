"""Device plumbing for the quaternion / forward-kinematics post-filter: moves the (small) row
sets to the GPU, calls ``ape_fk`` / ``ape_msg_reduce`` of libape_hip.so, brings results back.
``spread_rows`` is the plain numpy statement of the spread record."""
import ctypes as C
import threading

import numpy as np
import torch

from wear_mocap_ape_amd import _hip

_ctx_lock = threading.Lock()
_ctx = {}


class _PostContext:
    """a weight-less handle that carries only layout + body measurements"""

    def __init__(self, layout: int, device: int):
        self.layout, self.device = layout, device
        dims = _hip.ApeDims(1, 128, 1, _hip.NUM_TARGETS[layout], layout, device)
        self.handle = C.c_void_p()
        _hip.check(_hip.lib().ape_model_create(C.byref(dims), C.byref(self.handle)), "ape_model_create")
        self.lock = threading.Lock()

    def __del__(self):
        try:
            if self.handle.value:
                _hip.lib().ape_model_destroy(self.handle)
        except Exception:
            pass


def context(layout: int, device: int = None) -> _PostContext:
    if not torch.cuda.is_available():
        raise UserWarning("no GPU visible: the arm-pose post-filter has no CPU fallback")
    if device is None:
        device = torch.cuda.current_device()
    key = (layout, device)
    with _ctx_lock:
        if key not in _ctx:
            _ctx[key] = _PostContext(layout, device)
        return _ctx[key]


def _set_body(handle, body):
    b = np.ascontiguousarray(np.asarray(body, dtype=np.float64).reshape(-1))
    if b.size != 9:
        raise UserWarning("body_measurements must be [1,9]: larm_vec, uarm_vec, uarm_orig_rh")
    _hip.check(_hip.lib().ape_model_set_body(handle, _hip.dptr(b, C.c_double)), "ape_model_set_body")


def fk_rows(handle, layout, device, preds: np.ndarray, body, denormalize=False) -> np.ndarray:
    """preds [N,O] (host) -> est float64 [N,W] (host) through ``ape_fk``."""
    preds = np.asarray(preds)
    if preds.ndim != 2 or preds.shape[1] != _hip.NUM_TARGETS[layout]:
        raise UserWarning(f"preds must be [N,{_hip.NUM_TARGETS[layout]}], got {preds.shape}")
    if preds.shape[0] < 1:
        raise UserWarning("preds holds no rows")
    dev = torch.device("cuda", device)
    _set_body(handle, body)
    with torch.cuda.device(dev):
        pd = torch.from_numpy(np.ascontiguousarray(preds, dtype=np.float64)).to(dev)
        est = torch.empty((preds.shape[0], _hip.EST_WIDTH[layout]), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_fk(handle, C.c_void_p(pd.data_ptr()), _hip.F64, preds.shape[0],
                                     1 if denormalize else 0, C.c_void_p(est.data_ptr()), _hip.F64, stream), "ape_fk")
        return est.cpu().numpy()


def msg_rows(handle, layout, device, est: np.ndarray, body) -> np.ndarray:
    """est float64 [N,W] (host) -> msg float64 [25] through ``ape_msg_reduce``."""
    est = np.asarray(est)
    if est.ndim != 2 or est.shape[1] != _hip.EST_WIDTH[layout] or est.shape[0] < 1:
        raise UserWarning(f"est must be [N>=1,{_hip.EST_WIDTH[layout]}], got {est.shape}")
    dev = torch.device("cuda", device)
    _set_body(handle, body)
    with torch.cuda.device(dev):
        ed = torch.from_numpy(np.ascontiguousarray(est, dtype=np.float64)).to(dev)
        msg = torch.empty((25,), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_msg_reduce(handle, C.c_void_p(ed.data_ptr()), est.shape[0],
                                             C.c_void_p(msg.data_ptr()), stream), "ape_msg_reduce")
        return msg.cpu().numpy()


def fk_and_msg(handle, layout, device, preds: np.ndarray, body):
    """one upload: preds [N,O] -> (est [N,W], msg [25]) -- FK and message kernels back to back"""
    preds = np.asarray(preds)
    if preds.ndim != 2 or preds.shape[1] != _hip.NUM_TARGETS[layout] or preds.shape[0] < 1:
        raise UserWarning(f"preds must be [N>=1,{_hip.NUM_TARGETS[layout]}], got {preds.shape}")
    dev = torch.device("cuda", device)
    _set_body(handle, body)
    N, W = preds.shape[0], _hip.EST_WIDTH[layout]
    with torch.cuda.device(dev):
        pd = torch.from_numpy(np.ascontiguousarray(preds, dtype=np.float64)).to(dev)
        out = torch.empty((N * W + 25,), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        lib = _hip.lib()
        _hip.check(lib.ape_fk(handle, C.c_void_p(pd.data_ptr()), _hip.F64, N, 0, C.c_void_p(out.data_ptr()),
                              _hip.F64, stream), "ape_fk")
        _hip.check(lib.ape_msg_reduce(handle, C.c_void_p(out.data_ptr()), N,
                                      C.c_void_p(out.data_ptr() + N * W * 8), stream), "ape_msg_reduce")
        host = out.cpu().numpy()
    return host[:N * W].reshape(N, W), host[N * W:]


SPREAD_WIDTH = _hip.SPREAD_WIDTH


def spread_rows(est, msg, layout: int) -> np.ndarray:
    """The spread record of N stacked est rows (``APE_SPREAD_WIDTH`` = 21 float64 values; include/ape_hip.h) in
    plain numpy: the statement the device kernels are tested against, and what the staged reference-style ``Estimator`` methods
    fill ``get_last_spread()`` with.  The reference has no counterpart: it appends ``est[i, :6]`` of every row to the message
    (estimator.py:131-137).

    ``est`` float64 ``[N, W]`` rows of ``arm_pose_from_nn_targets`` in the reference's stack order, ``msg`` the 25-value message of
    the same rows (only its quaternions ``msg[7:11]``, ``msg[14:18]``, ``msg[21:25]`` are read), ``layout`` an ``APE_LAYOUT_*``.

    ``[0:3]`` mean hand origin (NOT ``msg[4:7]``, which is recomputed from mean quaternions, compose_msg.py:54-61), ``[3:9]`` its
    population covariance xx, xy, xz, yy, yz, zz, ``[9:12]`` / ``[12:18]`` the same for the elbow, ``[18:21]`` the angular spread in
    radians of the lower-arm, upper-arm and hips quaternions about the message's: ``2 asin(sqrt(1 - mean((q_i . qm)^2)))``.
    N == 1: covariances and angles are exactly 0 by rule.  No hips in the layout: ``[20]`` is exactly 0."""
    est = np.asarray(est, dtype=np.float64)
    msg = np.asarray(msg, dtype=np.float64).reshape(-1)
    if layout not in _hip.EST_WIDTH:
        raise UserWarning(f"unknown target layout {layout}")
    if est.ndim != 2 or est.shape[1] != _hip.EST_WIDTH[layout] or est.shape[0] < 1:
        raise UserWarning(f"est must be [N>=1,{_hip.EST_WIDTH[layout]}], got {est.shape}")
    if msg.shape[0] < 25:
        raise UserWarning(f"msg must hold the 25-value message, got {msg.shape}")
    n = est.shape[0]
    out = np.zeros((SPREAD_WIDTH,), dtype=np.float64)
    out[0:3], out[9:12] = est[:, 0:3].mean(axis=0), est[:, 3:6].mean(axis=0)
    if n == 1:
        out[0:3], out[9:12] = est[0, 0:3], est[0, 3:6]
        return out
    iu = np.triu_indices(3)
    for c0, o0 in ((0, 3), (3, 12)):
        d = est[:, c0:c0 + 3] - est[:, c0:c0 + 3].mean(axis=0)
        out[o0:o0 + 6] = (d.T @ d / n)[iu]
    hips = layout != _hip.LAYOUT_ORI_CAL_LARM_UARM
    q_cols = (9, 13, 17) if hips else (6, 10)
    for k, c in enumerate(q_cols):
        qm = msg[7 + 7 * k:11 + 7 * k]
        dots = est[:, c:c + 4] @ qm
        out[18 + k] = 2.0 * np.arcsin(np.sqrt(np.clip(1.0 - np.mean(dots * dots), 0.0, 1.0)))
    return out


def spread_reduce(handle, layout, device, est: np.ndarray, msg: np.ndarray) -> np.ndarray:
    """est float64 [N,W] + msg float64 [25] (host) -> spread record float64 [21] through ``ape_spread_reduce``."""
    est = np.asarray(est)
    if est.ndim != 2 or est.shape[1] != _hip.EST_WIDTH[layout] or est.shape[0] < 1:
        raise UserWarning(f"est must be [N>=1,{_hip.EST_WIDTH[layout]}], got {est.shape}")
    msg = np.asarray(msg).reshape(-1)
    if msg.shape[0] != 25:
        raise UserWarning(f"msg must be [25], got {msg.shape}")
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        ed = torch.from_numpy(np.ascontiguousarray(est, dtype=np.float64)).to(dev)
        md = torch.from_numpy(np.ascontiguousarray(msg, dtype=np.float64)).to(dev)
        out = torch.empty((SPREAD_WIDTH,), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_spread_reduce(handle, C.c_void_p(ed.data_ptr()), est.shape[0], C.c_void_p(md.data_ptr()),
                                                C.c_void_p(out.data_ptr()), stream), "ape_spread_reduce")
        return out.cpu().numpy()
