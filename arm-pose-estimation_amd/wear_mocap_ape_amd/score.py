"""Scoring replayed poses against ground truth (``ape_score_rows``, include/ape_hip.h).

The reference has no counterpart: it never compares a message with the mocap truth its recordings carry.  ``score_rows`` does it on
the device for every frame of a replay -- five errors and, with the frames' spread records, two squared Mahalanobis distances -- and
accumulates them per recording; ``score_rows_numpy`` is the plain numpy statement of the per-frame values, ``summarise`` and
``merge`` work on the raw accumulators on the host."""
import ctypes as C

import numpy as np
import torch

from wear_mocap_ape_amd import _hip

SCORE_WIDTH = _hip.SCORE_WIDTH
ACC_WIDTH = _hip.SCORE_ACC_WIDTH
TRUTH_KINDS = {"targets": _hip.TRUTH_TARGETS, "est": _hip.TRUTH_EST}
CHI2_3_Q50, CHI2_3_Q90 = 2.3659738843753377, 6.251388631170325      # the 50 % and 90 % quantiles of chi^2 with 3 degrees of freedom
ERROR_NAMES = ("hand_pos", "elbow_pos", "larm_rot", "uarm_rot", "hips_rot")
_MAX_COLS = (2, 5, 8, 11, 14)


def _angle(q, qt):
    """4 asin(min(1, |q - s qt| / 2)) with s = -1 where q . qt < 0.0 (the flip rule of average_quaternions)"""
    d = q[:, 0] * qt[:, 0] + q[:, 1] * qt[:, 1] + q[:, 2] * qt[:, 2] + q[:, 3] * qt[:, 3]
    s = np.where(d < 0.0, -1.0, 1.0)[:, None]
    v = q - s * qt
    h = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2] + v[:, 3] * v[:, 3]) / 2.0
    return 4.0 * np.arcsin(np.minimum(h, 1.0))


def _dist(a, t):
    v = a - t
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def _mahalanobis(rec, t):
    """rec ``[F, 9]`` = mean, covariance xx xy xz yy yz zz; NaN where the covariance is not usable"""
    a, b, c, d, e, f = (rec[:, 3 + k] for k in range(6))
    tr = a + d + f
    a00, a01, a02 = d * f - e * e, c * e - b * f, b * e - c * d
    a11, a12, a22 = a * f - c * c, b * c - a * e, a * d - b * b
    det = a * a00 + b * a01 + c * a02
    third = tr / 3.0
    usable = np.isfinite(rec[:, 3:9]).all(axis=1) & (tr > 0.0) & (det > 1e-12 * (third * third * third))
    x, y, z = t[:, 0] - rec[:, 0], t[:, 1] - rec[:, 1], t[:, 2] - rec[:, 2]
    quad = a00 * x * x + a11 * y * y + a22 * z * z + 2.0 * (a01 * x * y + a02 * x * z + a12 * y * z)
    return np.where(usable, quad / np.where(usable, det, 1.0), np.nan)


def score_rows_numpy(msg, truth_est, layout: int, spread=None) -> np.ndarray:
    """The per-frame score record, float64 ``[F, 7]`` (include/ape_hip.h states the columns), of messages ``msg [F, >= 25]`` against
    est-kind truth ``truth_est [F, 21 | 14]`` in the layout's est columns; ``spread [F, >= 21]``: the frames' spread records for
    columns 5 and 6 (NaN without).  A frame whose message or truth has a non-finite value it uses is an all-NaN row."""
    hips = layout != _hip.LAYOUT_ORI_CAL_LARM_UARM
    with np.errstate(all="ignore"):
        m = np.asarray(msg, dtype=np.float64)[:, :25]
        t = np.asarray(truth_est, dtype=np.float64)
        ql, qu = (9, 13) if hips else (6, 10)
        out = np.full((m.shape[0], SCORE_WIDTH), np.nan)
        out[:, 0] = _dist(m[:, 4:7], t[:, 0:3])
        out[:, 1] = _dist(m[:, 11:14], t[:, 3:6])
        out[:, 2] = _angle(m[:, 7:11], t[:, ql:ql + 4])
        out[:, 3] = _angle(m[:, 14:18], t[:, qu:qu + 4])
        out[:, 4] = _angle(m[:, 21:25], t[:, 17:21]) if hips else 0.0
        used = np.r_[0:6, ql:ql + 4, qu:qu + 4, 17:21] if hips else np.r_[0:6, ql:ql + 4, qu:qu + 4]
        if spread is not None:
            s = np.asarray(spread, dtype=np.float64)
            out[:, 5] = _mahalanobis(s[:, 0:9], t[:, 0:3])
            out[:, 6] = _mahalanobis(s[:, 9:18], t[:, 3:6])
        out[~(np.isfinite(m).all(axis=1) & np.isfinite(t[:, used]).all(axis=1))] = np.nan
    return out


def accumulate_numpy(score, starts=None, skip: int = 0) -> np.ndarray:
    """The raw accumulators float64 ``[R, 25]`` of per-frame rows ``score [F, 7]`` (host statement of what ``score_rows`` returns as
    ``acc``; numpy's summation order, so sums agree to rounding)."""
    score = np.asarray(score, dtype=np.float64)
    st = np.asarray([0] if starts is None else starts, dtype=np.int64).reshape(-1)
    ends = np.r_[st[1:], score.shape[0]]
    acc = np.zeros((st.shape[0], ACC_WIDTH))
    for r, (a, b) in enumerate(zip(st, ends)):
        rows = score[min(a + skip, b):b]
        ok = np.isfinite(rows[:, 0])
        good = rows[ok]
        for c in range(5):
            if good.shape[0]:
                acc[r, 3 * c:3 * c + 3] = good[:, c].sum(), (good[:, c] * good[:, c]).sum(), good[:, c].max()
        acc[r, 15], acc[r, 16] = good.shape[0], rows.shape[0] - good.shape[0]
        for k in range(2):
            d2 = good[:, 5 + k]
            d2 = d2[np.isfinite(d2)]
            acc[r, 17 + 4 * k:21 + 4 * k] = d2.shape[0], d2.sum(), (d2 <= CHI2_3_Q50).sum(), (d2 <= CHI2_3_Q90).sum()
    return acc


def _as_host(acc) -> np.ndarray:
    a = acc.detach().cpu().numpy() if isinstance(acc, torch.Tensor) else np.asarray(acc)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != ACC_WIDTH:
        raise UserWarning(f"expected accumulators [R,{ACC_WIDTH}], got {tuple(a.shape)}")
    return a


def merge(acc_a, acc_b) -> np.ndarray:
    """the accumulators of two pieces of the same recordings as one: sums and counts added, the larger of the maxima"""
    a, b = _as_host(acc_a), _as_host(acc_b)
    if a.shape != b.shape:
        raise UserWarning(f"merge: {tuple(a.shape)} and {tuple(b.shape)} accumulators")
    out = a + b
    out[:, _MAX_COLS] = np.maximum(a[:, _MAX_COLS], b[:, _MAX_COLS])
    return out


def summarise(acc) -> list:
    """per recording a dict: ``scored`` / ``unscored`` frame counts, ``mean``, ``rms`` and ``max`` of the five errors (dicts keyed by
    ``ERROR_NAMES``; NaN where nothing was scored), and for ``hand`` and ``elbow`` the number of frames with a usable ``d2``, its
    mean, and the fraction of those frames inside the 50 % and 90 % regions of their covariance (``coverage50`` / ``coverage90``)."""
    res = []
    with np.errstate(all="ignore"):
        for row in _as_host(acc):
            n = row[15]
            d = {"scored": int(n), "unscored": int(row[16]), "mean": {}, "rms": {}, "max": {}}
            for c, name in enumerate(ERROR_NAMES):
                d["mean"][name] = float(row[3 * c] / n) if n else float("nan")
                d["rms"][name] = float(np.sqrt(row[3 * c + 1] / n)) if n else float("nan")
                d["max"][name] = float(row[3 * c + 2]) if n else float("nan")
            for k, name in enumerate(("hand", "elbow")):
                u, s, c50, c90 = row[17 + 4 * k:21 + 4 * k]
                d[name] = {"frames": int(u), "mean_d2": float(s / u) if u else float("nan"),
                           "coverage50": float(c50 / u) if u else float("nan"), "coverage90": float(c90 / u) if u else float("nan")}
            res.append(d)
    return res


def _rows_view(t, width: int, what: str):
    """(tensor, stride in elements) of a device view [F, >= width] whose rows are contiguous"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2 or t.shape[1] < width:
        raise UserWarning(f"{what}: expected a device tensor [F, >= {width}]")
    if t.dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"{what}: float32 or float64, got {t.dtype}")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < width):
        t = t[:, :width].contiguous()
    return t, max(int(t.stride(0)), width)


def score_rows(layout: int, msg, truth, truth_kind: str = "targets", spread=None, starts=None, skip: int = 0, bodies=None,
               out_dtype=torch.float64, per_frame: bool = True):
    """``msg`` device ``[F, >= 25]`` (the message at the front of every row: plain, packed or spread-flagged replay and bank rows, or
    a strided view of them) scored against ``truth`` device ``[F, O]`` NN targets (``truth_kind="targets"``, de-normalised, through
    the float64 FK with ``bodies``) or ``[F, 21 | 14]`` est rows (``"est"``).  ``spread``: device ``[F, >= 21]`` spread records
    of ``msg``'s dtype (the second view ``process_recording(spread=True)`` returns goes in as it is).  ``starts``: the recordings'
    first frames (default one recording); ``skip``: leading frames of every recording left out of the accumulators; ``bodies``:
    float64 ``[9]`` / ``[1, 9]`` / ``[R, 9]`` values, one bonemap-like object (for all recordings) or a sequence of R (default: the default bonemap).
    Returns ``(score, acc)``: ``[F, 7]`` of ``out_dtype`` (None with ``per_frame=False``) and float64 ``[R, 25]`` raw accumulators
    (``summarise``, ``merge``), both on the device.  The call does not wait for the device."""
    from wear_mocap_ape_amd.data_types.bone_map import bodies_from, body9_from_bonemap
    if truth_kind not in TRUTH_KINDS:
        raise UserWarning(f"truth_kind must be one of {sorted(TRUTH_KINDS)}, got {truth_kind!r}")
    if layout not in _hip.EST_WIDTH:
        raise UserWarning(f"layout {layout} has no pose to score")
    if out_dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
    md, ms = _rows_view(msg, 25, "msg")
    F, dev = int(md.shape[0]), md.device
    sd, ss = (None, 0)
    if spread is not None:
        sd, ss = _rows_view(spread, _hip.SPREAD_WIDTH, "spread")
        if sd.dtype != md.dtype or sd.shape[0] != F or sd.device != dev:
            raise UserWarning("spread: the dtype, device and frame count of msg")
    tw = (_hip.NUM_TARGETS if truth_kind == "targets" else _hip.EST_WIDTH)[layout]
    if not isinstance(truth, torch.Tensor) or truth.dtype not in (torch.float32, torch.float64):
        raise UserWarning("truth: a float32 or float64 device tensor")
    if tuple(truth.shape) != (F, tw) or truth.device != dev:
        raise UserWarning(f"truth: expected [{F},{tw}] on {dev}, got {tuple(truth.shape)} on {truth.device}")
    td = truth.contiguous()
    st = np.ascontiguousarray(np.asarray([0] if starts is None else starts, dtype=np.int32).reshape(-1))
    R = int(st.shape[0])
    if bodies is None:
        body = body9_from_bonemap(None)[np.newaxis, :]
    elif isinstance(bodies, np.ndarray) and bodies.size == 9:
        body = np.ascontiguousarray(bodies.reshape(1, 9), dtype=np.float64)
    elif not isinstance(bodies, np.ndarray) and not hasattr(bodies, "__len__"):
        body = body9_from_bonemap(bodies)[np.newaxis, :]              # one bonemap-like object: that body for every recording
    else:
        body = bodies_from(bodies, R, "score_rows bodies")
    f64 = lambda t: _hip.F64 if t == torch.float64 else _hip.F32          # noqa: E731
    with torch.cuda.device(dev):
        score = torch.empty((F, SCORE_WIDTH), dtype=out_dtype, device=dev) if per_frame else None
        acc = torch.empty((max(R, 1), ACC_WIDTH), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_score_rows(int(layout), C.c_void_p(md.data_ptr()), ms, C.c_void_p(sd.data_ptr()) if sd is not None else None,
                                             ss, f64(md.dtype), C.c_void_p(td.data_ptr()), TRUTH_KINDS[truth_kind], f64(td.dtype), F,
                                             C.c_void_p(st.ctypes.data), R, int(skip), C.c_void_p(body.ctypes.data), int(body.shape[0]),
                                             C.c_void_p(score.data_ptr()) if score is not None else None, f64(out_dtype),
                                             C.c_void_p(acc.data_ptr()), stream), "ape_score_rows")
    return score, acc
