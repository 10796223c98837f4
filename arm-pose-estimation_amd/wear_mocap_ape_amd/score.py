"""Scoring replayed poses against ground truth (``ape_score_rows``, ``ape_score_lags``, include/ape_hip.h).

The reference has no counterpart: it never compares a message with the mocap truth its recordings carry.  ``score_rows`` does it on
the device for every frame of a replay -- five errors and, with the frames' spread records, two squared Mahalanobis distances -- and
accumulates them per recording; ``score_rows_numpy`` is the plain numpy statement of the per-frame values, ``summarise`` and
``merge`` work on the raw accumulators on the host.

A smoothed estimate trails the motion and the mocap and IMU clocks are not aligned to the frame, so frame ``f`` of a replay need not
belong to frame ``f`` of the truth: ``score_lags`` scores every frame against the truth of a whole sweep of lags in one pass (never across
a recording boundary, and on the same frames for every lag), ``best_lag`` reads each recording's lag off the accumulators, ``align`` does
both and scores once more at the lags found; ``score_lags_numpy`` is the host statement.

Which ``smooth`` and how many Monte-Carlo samples to run is answered from ONE replay: ``post_sweep`` runs the float64 post-filter from
the replay's stored targets for many ``(smooth, samples)`` configurations in one pass (``ape_post_sweep``), ``grid``
builds the list, ``score_configs`` scores every configuration over a sweep of lags.

A recording whose wearer stood a few degrees off during the calibration pose is turned as a whole against the truth: ``frame_sums``
takes, for every lag of a sweep, the sums the least-squares rotation is read off (``ape_frame_sums``), ``best_frame``
finds lag and rotation together on the host, ``rotate_rows`` applies it (``ape_rotate_rows``), ``align_frame`` does all of it and scores
what remains; ``frame_sums_numpy`` and ``rotate_rows_numpy`` are the host statements.

Watch frames sit on a jittered clock and a mocap system runs at its own rate: ``frame_times`` builds a recording's clock from its
``sw_dt`` column, ``resample_truth`` gives est-kind truth rows at each frame's time less a shift (``ape_frame_times``,
``ape_resample_truth``), ``truth_on_frames`` does both from raw rows, ``align(refine=True)`` scores at ``best_lag``'s
fractional lag; ``frame_times_numpy`` and ``resample_truth_numpy`` are the host statements.

The positions of a message are made from its quaternions and the nine values of a body, and the wearer's are rarely the default's:
``body_sums`` takes, for every lag of a sweep, the sums a recording's least-squares body is read off (``ape_body_sums``, DESIGN.md
4.37), ``best_body`` solves for nine values or three lengths on the host, ``bodies_of`` gives them to ``set_bodies`` and
``process_recording(bonemaps=)``, ``rebody_rows`` makes the rows' positions again (``ape_rebody_rows``), ``align_body`` does all of it
and scores what remains; ``body_sums_numpy`` and ``rebody_rows_numpy`` are the host statements.

What a longer ``smooth`` buys is a steadier arm: ``motion_sums`` takes the linear and angular speed, acceleration and jerk of every
frame of any rows that state a pose -- messages, est rows or targets, many sets at once -- on the frames' own clock and sums them per
recording (``ape_motion_sums``); it needs no truth.  ``summarise_motion`` and ``merge_motion`` work on the raw
accumulators, ``motion_sums_numpy`` is the host statement.

A mean, an RMS and one worst frame say nothing of the shape between them: ``hist_rows`` counts any per-frame rows that lie on the
device -- score rows, a lag sweep's, motion rows -- over fixed edges per recording and column (``ape_score_hist``).  The
counts are integers and add across the pieces of a chained replay (``merge_hist``); ``quantiles``, ``fraction_within``, ``pit`` and
``summarise_hist`` read medians, percentiles, the share of frames within 5 cm and the spread record's reliability curve off them on the
host; ``default_edges`` and ``pit_edges`` make edges, ``lag_trim`` the windows of a lag sweep's common support; ``hist_numpy`` is the host
statement.

``joint_angles`` states every frame as the angles its users ask in (elbow flexion, forearm twist, shoulder elevation and its plane,
humeral twist, hips yaw) with their errors against truth and their sums per recording; ``summarise_angles``,
``merge_angles`` and ``angle_edges`` go with it, ``joint_angles_numpy`` is the host statement.

All of these state their numbers per recording.  ``stats_by`` states one per-frame column as a function of another: the count, sum, sum
of squares and maximum of any value columns over the bins of any key columns -- the hand error over the elbow flexion, over the hand
speed, over the predicted sigma (``spread_sigma``; ``ape_score_by``) -- in a stated order of summation, so the same
inputs give the same bits; ``merge_by``, ``pool_by`` and ``summarise_by`` work on the records, ``stats_by_numpy`` is the host statement.

Every smoothing route looks backwards and pays for it in lag.  A recording processed offline need not: ``post_window`` runs the
post-filter from one replay's stored targets at windows that look ahead as far as they look back, with per-frame weights that taper
(``ape_post_window``); ``window`` and ``window_weights`` make the configurations, ``score_windows`` scores every window
over a sweep of lags, ``post_window_numpy`` is the host statement.

A window that is the same on every frame is a compromise for arm motion, which is holds joined by reaches.  ``select_rungs`` picks a rung
of a ``ladder`` of windows for every frame from a per-frame key (the hand speed) under an envelope, and ``post_select`` runs the
post-filter at the rung chosen (``ape_select_rungs``, ``ape_post_select``); ``select_rungs_numpy`` and
``post_select_numpy`` are the host statements, ``score_selected`` scores the sets.

Where those holds and reaches are, and what each of them was like: ``segment_frames`` labels every frame hold or move from a per-frame
key with two thresholds and minimum lengths, ``segment_runs`` turns any labels into a table of segments, ``segment_stats`` reduces
per-frame columns over every segment in a stated order of summation (``ape_segment_frames``, ``ape_segment_runs``,
``ape_segment_stats``); ``match_segments`` pairs an estimate's moves with the truth's and ``summarise_segments`` reads
the records per recording and label on the host; ``segment_frames_numpy``, ``segment_runs_numpy`` and ``segment_stats_numpy`` are the
host statements.

At which frequencies: ``spectra`` takes Welch sums of any per-frame columns against an optional truth per recording, column and
frequency bin on the float64 matrix cores (``ape_spectra``); ``summarise_spectra`` reads densities, the gain, phase and
delay of the estimate against the truth, the coherence and the error's spectrum off them, ``bandwidth`` and ``band_power`` reduce those,
``merge_spectra`` adds records, ``pose_cols`` and ``pose_spectra`` pick the hand and elbow positions; ``spectra_numpy`` is the host
statement.

Acting on the regressor's own error: ``fit_sums`` takes, per recording, the normal-equation sums of ``[h, 1, t]`` -- the hidden features
``Estimator.features_recording`` returns, a one, the truth targets -- on the float64 matrix cores (``ape_fit_sums``);
``best_head`` solves them for an output layer fitted to the wearer under a ridge towards the present one, ``sweep_ridge`` prices ridges
leave-one-recording-out from the sums alone, ``price_head`` prices any head, ``merge_fit`` adds records; ``fit_sums_numpy`` is the host
statement."""
import ctypes as C
import math

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


def _as_host(acc, ndims=(2,)) -> np.ndarray:
    a = acc.detach().cpu().numpy() if isinstance(acc, torch.Tensor) else np.asarray(acc)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim not in ndims or a.shape[-1] != ACC_WIDTH:
        raise UserWarning(f"expected accumulators {' or '.join('[R,L,25]' if n == 3 else '[R,25]' for n in ndims)}, got {tuple(a.shape)}")
    return a


def merge(acc_a, acc_b) -> np.ndarray:
    """the accumulators ``[R, 25]``, or ``[R, L, 25]`` of the same sweep, of two pieces of the same recordings as one: sums and counts
    added, the larger of the maxima.  Of a lag sweep this is the union of the two pieces' supports: a pair whose message lies in one
    piece and whose truth row in the other is in neither, so the frames within the sweep's reach of the cut are not scored."""
    a, b = _as_host(acc_a, (2, 3)), _as_host(acc_b, (2, 3))
    if a.shape != b.shape:
        raise UserWarning(f"merge: {tuple(a.shape)} and {tuple(b.shape)} accumulators")
    out = a + b
    out[..., _MAX_COLS] = np.maximum(a[..., _MAX_COLS], b[..., _MAX_COLS])
    return out


def summarise(acc) -> list:
    """``acc [R, 25]`` (of a lag sweep: one lag's slice ``acc[:, j]``) -> per recording a dict: ``scored`` / ``unscored`` frame
    counts, ``mean``, ``rms`` and ``max`` of the five errors (dicts keyed by
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


def _f64(t):
    return _hip.F64 if t == torch.float64 else _hip.F32


def _prepared(layout, msg, truth, truth_kind, spread, starts, bodies, out_dtype):
    """the checked views and host arrays of one scoring call: (msg view, its stride, spread view | None, its stride, truth, starts int32
    ``[R]``, bodies float64 ``[1 | R, 9]``)"""
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
    return md, ms, sd, ss, td, st, _body_rows(bodies, R, "score_rows bodies")


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
    md, ms, sd, ss, td, st, body = _prepared(layout, msg, truth, truth_kind, spread, starts, bodies, out_dtype)
    F, R, dev = int(md.shape[0]), int(st.shape[0]), md.device
    with torch.cuda.device(dev):
        score = torch.empty((F, SCORE_WIDTH), dtype=out_dtype, device=dev) if per_frame else None
        acc = torch.empty((max(R, 1), ACC_WIDTH), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_score_rows(int(layout), C.c_void_p(md.data_ptr()), ms, C.c_void_p(sd.data_ptr()) if sd is not None else None,
                                             ss, _f64(md.dtype), C.c_void_p(td.data_ptr()), TRUTH_KINDS[truth_kind], _f64(td.dtype), F,
                                             C.c_void_p(st.ctypes.data), R, int(skip), C.c_void_p(body.ctypes.data), int(body.shape[0]),
                                             C.c_void_p(score.data_ptr()) if score is not None else None, _f64(out_dtype),
                                             C.c_void_p(acc.data_ptr()), stream), "ape_score_rows")
    return score, acc


# ---- the same over a sweep of time lags (ape_score_lags) ---------------------------------------------------------------------
def _sweep(lags, R: int, rec_lags):
    """(lag_min, lag_max, offsets int32 [R]) of ``lags=(lo, hi)`` and per-recording offsets"""
    lo, hi = (int(v) for v in lags)
    off = np.zeros(R, dtype=np.int32) if rec_lags is None else np.ascontiguousarray(np.asarray(rec_lags, dtype=np.int32).reshape(-1))
    if off.shape[0] != R:
        raise UserWarning(f"rec_lags: {off.shape[0]} offsets for {R} recordings")
    return lo, hi, off


def score_lags(layout: int, msg, truth, lags=(0, 0), truth_kind: str = "targets", spread=None, starts=None, skip: int = 0, bodies=None,
               rec_lags=None, out_dtype=torch.float64, per_frame: bool = False):
    """``score_rows`` over the sweep of lags ``lags=(lo, hi)`` (both inclusive, ``L = hi - lo + 1 <= 65``) in one pass.  In recording
    ``r`` sweep index ``j`` stands for the lag ``l = rec_lags[r] + lo + j`` (``rec_lags``: integer offsets ``[R]``, default zeros;
    every ``|l| <= 128``); a positive lag means the estimate is late: message and spread row ``f`` are scored against truth row
    ``f - l`` of the same recording, and a pair that would leave the recording does not exist.  The other arguments, the views and the
    dtypes are ``score_rows``'s.  Returns ``(score, acc)`` on the device: ``[F, L, 7]`` of ``out_dtype`` (NaN rows where the pair
    does not exist or cannot be scored; None unless ``per_frame``) and float64 ``[R, L, 25]`` raw accumulators over the frames that
    have a pair at every lag of the sweep and lie past the recording's first ``skip`` frames -- the same frames for every lag, so
    ``acc[r, j]`` compare across ``j`` (``best_lag``; ``summarise(acc[:, j])``).  The call does not wait for the device."""
    md, ms, sd, ss, td, st, body = _prepared(layout, msg, truth, truth_kind, spread, starts, bodies, out_dtype)
    F, R, dev = int(md.shape[0]), int(st.shape[0]), md.device
    lo, hi, off = _sweep(lags, R, rec_lags)
    L = hi - lo + 1
    if not 1 <= L <= _hip.SCORE_MAX_LAGS:
        raise UserWarning(f"lags=({lo}, {hi}): between 1 and {_hip.SCORE_MAX_LAGS} lags")
    with torch.cuda.device(dev):
        score = torch.empty((F, L, SCORE_WIDTH), dtype=out_dtype, device=dev) if per_frame else None
        acc = torch.empty((max(R, 1), L, ACC_WIDTH), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_score_lags(int(layout), C.c_void_p(md.data_ptr()), ms, C.c_void_p(sd.data_ptr()) if sd is not None else None,
                                             ss, _f64(md.dtype), C.c_void_p(td.data_ptr()), TRUTH_KINDS[truth_kind], _f64(td.dtype), F,
                                             C.c_void_p(st.ctypes.data), R, int(skip), C.c_void_p(body.ctypes.data), int(body.shape[0]),
                                             lo, hi, C.c_void_p(off.ctypes.data) if rec_lags is not None else None,
                                             C.c_void_p(score.data_ptr()) if score is not None else None, _f64(out_dtype),
                                             C.c_void_p(acc.data_ptr()), stream), "ape_score_lags")
    return score, acc


def score_lags_numpy(msg, truth_est, layout: int, lags, starts=None, skip: int = 0, spread=None, rec_lags=None):
    """The host statement of ``score_lags`` for est-kind truth: ``(score [F, L, 7], acc [R, L, 25])`` float64, made of
    ``score_rows_numpy`` on every recording's and lag's pair rows (message ``f``, truth ``f - l``) and ``accumulate_numpy`` over the
    support."""
    msg, truth_est = np.asarray(msg), np.asarray(truth_est)
    st = np.asarray([0] if starts is None else starts, dtype=np.int64).reshape(-1)
    F, R = msg.shape[0], st.shape[0]
    lo, hi, off = _sweep(lags, R, rec_lags)
    L = hi - lo + 1
    ends = np.r_[st[1:], F]
    score = np.full((F, L, SCORE_WIDTH), np.nan)
    acc = np.zeros((R, L, ACC_WIDTH))
    for r in range(R):
        s, e, o = int(st[r]), int(ends[r]), int(off[r])
        a, b = max(s + skip, s + o + hi), min(e, e + o + lo)                # the support: a pair at every lag, past the skipped frames
        for j in range(L):
            l = o + lo + j
            f0, f1 = max(s, s + l), min(e, e + l)                            # the frames with s <= f - l < e
            if f0 < f1:
                score[f0:f1, j] = score_rows_numpy(msg[f0:f1], truth_est[f0 - l:f1 - l], layout, None if spread is None else spread[f0:f1])
            if a < b:
                acc[r, j] = accumulate_numpy(score[a:b, j])[0]
    return score, acc


def best_lag(acc, lags, error: str = "hand_pos", rec_lags=None) -> list:
    """Each recording's lag, read off the accumulators ``acc [R, L, 25]`` of a sweep ``lags=(lo, hi)`` (with the ``rec_lags`` the sweep
    was made with).  Per recording a dict:
    ``lag``       the lag ``l`` with the smallest mean square of ``error`` (one of ``ERROR_NAMES``) over the support; ties go to the
                  smaller ``|l|``, then to the smaller ``l``
    ``refined``   the vertex of the parabola through the mean squares at ``l - 1, l, l + 1``, clamped to ``l +- 0.5``, where both
                  neighbours are in the sweep (and scored) and the second difference is > 0; ``float(lag)`` otherwise
    ``at_edge``   ``lag`` is the first or the last of the sweep: the minimum may lie outside it
    ``scored``    frames scored at ``lag``;  ``rms`` of ``error`` there;  ``rms_lag0``: at lag 0 (NaN where 0 is not in the sweep)
    A recording with nothing scored at any lag (an empty support): ``lag`` and ``at_edge`` None, ``scored`` 0, the others NaN."""
    if error not in ERROR_NAMES:
        raise UserWarning(f"error must be one of {ERROR_NAMES}, got {error!r}")
    a = _as_host(acc, (3,))
    R, L = a.shape[0], a.shape[1]
    lo, hi, off = _sweep(lags, R, rec_lags)
    if hi - lo + 1 != L:
        raise UserWarning(f"best_lag: lags=({lo}, {hi}) for accumulators of {L} lags")
    c = 3 * ERROR_NAMES.index(error) + 1
    res = []
    for r in range(R):
        n = a[r, :, 15]
        with np.errstate(all="ignore"):
            ms = np.where(n > 0, a[r, :, c] / n, np.nan)
        ls = int(off[r]) + lo + np.arange(L)
        cand = [j for j in range(L) if np.isfinite(ms[j])]
        if not cand:
            res.append({"lag": None, "refined": float("nan"), "at_edge": None, "scored": 0, "rms": float("nan"), "rms_lag0": float("nan")})
            continue
        j = min(cand, key=lambda k: (ms[k], abs(int(ls[k])), int(ls[k])))
        l = int(ls[j])
        refined = float(l)
        if 0 < j < L - 1 and np.isfinite(ms[j - 1]) and np.isfinite(ms[j + 1]):
            curve = ms[j - 1] - 2.0 * ms[j] + ms[j + 1]
            if curve > 0.0:
                refined = l + float(np.clip(0.5 * (ms[j - 1] - ms[j + 1]) / curve, -0.5, 0.5))
        j0 = -int(ls[0])
        res.append({"lag": l, "refined": refined, "at_edge": j in (0, L - 1), "scored": int(n[j]), "rms": float(np.sqrt(ms[j])),
                    "rms_lag0": float(np.sqrt(ms[j0])) if 0 <= j0 < L else float("nan")})
    return res


def align(layout: int, msg, truth, lags, error: str = "hand_pos", truth_kind: str = "targets", spread=None, starts=None, skip: int = 0,
          bodies=None, rec_lags=None, out_dtype=torch.float64, refine: bool = False):
    """Find each recording's lag and score at it: a ``score_lags`` sweep (accumulators only), ``best_lag`` on it (this waits for the
    device), then one more pass with ``lags=(0, 0)`` and the lags found as offsets (0 for a recording with an empty support).
    Returns ``(best, score [F, 7], acc [R, 25])``: ``best_lag``'s list, and the per-frame rows and accumulators at every recording's own
    lag, as ``score_rows`` would return them for aligned rows.
    ``refine=True``: the second pass is at ``best_lag``'s fractional ``refined`` lag instead: ``resample_truth`` on the index clock with
    each recording's ``refined`` as its shift (0 for an empty support), then ``score_rows`` against the resampled est rows -- a frame whose
    shifted time leaves its recording's truth is not scored (``acc[:, 16]``)."""
    _, sweep = score_lags(layout, msg, truth, lags, truth_kind, spread, starts, skip, bodies, rec_lags, out_dtype, per_frame=False)
    best = best_lag(sweep, lags, error, rec_lags)
    if refine:
        shifts = [0.0 if b["lag"] is None else b["refined"] for b in best]
        frames = int(truth.shape[0])
        moved = resample_truth(layout, truth, truth_kind, starts, None, None, frames, starts, shifts, 0.0, bodies, check_times=False)
        score, acc = score_rows(layout, msg, moved, "est", spread, starts, skip, bodies, out_dtype)
        return best, score, acc
    found = [0 if b["lag"] is None else b["lag"] for b in best]
    score, acc = score_lags(layout, msg, truth, (0, 0), truth_kind, spread, starts, skip, bodies, found, out_dtype, per_frame=True)
    return best, score[:, 0], acc[:, 0]


# ---- post-filter sweep: one replay's targets at many (smooth, samples) (ape_post_sweep) ----------------------------------
def grid(smooths, samples) -> list:
    """the configurations ``(smooth, samples)`` of the product ``smooths x samples``: smooth-major (every sample count of the first
    smooth in the order given, then the second smooth, ...), a pair that occurs again is dropped (the first occurrence keeps its place)"""
    out, seen = [], set()
    for s in smooths:
        for m in samples:
            pair = (int(s), int(m))
            if pair not in seen:
                seen.add(pair)
                out.append(pair)
    return out


def _configs(configs) -> np.ndarray:
    """int32 ``[C, 2]`` of a list of ``(smooth, samples)`` pairs"""
    try:
        cf = np.ascontiguousarray(np.asarray(list(configs), dtype=np.int32))
    except (TypeError, ValueError):
        raise UserWarning("configs: a list of (smooth, samples) pairs")
    if cf.ndim != 2 or cf.shape[1] != 2 or not 1 <= cf.shape[0] <= _hip.POST_MAX_CONFIGS:
        raise UserWarning(f"configs: between 1 and {_hip.POST_MAX_CONFIGS} (smooth, samples) pairs, got shape {tuple(cf.shape)}")
    return cf


def post_sweep(model, y, configs, starts=None, bodies=None, spread: bool = False, out_dtype=torch.float64, workspace_bytes: int = 0):
    """The float64 post-filter of a replay -- de-normalise, forward kinematics, the clamped sliding stack, the sign-aligned quaternion
    mean, the spread record -- from stored targets, for many configurations in one pass (``ape_post_sweep``).  ``model``: the HIP
    regressor whose replay made ``y`` (its layout, ``yy_m`` / ``yy_s`` and body are used, its weights are not); ``y``: device float32
    ``[F, M, O]``, the normalised targets ``process_recording(return_targets=True)`` returns; ``configs``: a list of
    ``(smooth, samples)`` pairs with ``samples <= M`` (``grid``): configuration ``c`` stacks the first ``samples`` samples of the last
    ``smooth`` frames.  ``starts``: the recordings' first frames (default one recording); ``bodies``: float64 ``[9]`` / ``[1, 9]`` /
    ``[R, 9]`` values or a sequence of R bonemap-like objects (default: the model's body); ``workspace_bytes``: bound on the device
    workspace (0: 128 MiB; include/ape_hip.h states the rule), which does not change the result.
    Returns ``out [C, F, 25]`` of ``out_dtype`` on the device -- ``out[c]`` is what ``process_recording`` of an estimator with
    configuration ``c`` returns in its first 25 columns, bit for bit where ``samples == M`` -- or, with ``spread``, ``(out, spread)``
    with ``spread [C, F, 21]``: two views of one tensor, as ``process_recording(spread=True)`` returns them.  Does not wait."""
    return _post_call("post_sweep", lambda: (_configs(configs),), model, y, starts, bodies, spread, out_dtype, workspace_bytes)


def _post_call(entry: str, lists_of, model, y, starts, bodies, spread, out_dtype, workspace_bytes, sel_of=None):
    """what ``post_sweep``, ``post_window`` and ``post_select`` share: the checks of ``out_dtype`` and ``y``, ``starts``, the bodies rule,
    the allocation, the call of ``ape_<entry>`` and the ``(out, spread)`` split.  ``lists_of()``: the arrays (or None) the entry takes
    between ``R`` and ``C``, the first with one row per configuration; ``sel_of()``: the device selector ``[S, F]`` the entry takes
    behind ``C`` (with ``S``), which then counts the sets of the result"""
    from wear_mocap_ape_amd.data_types.bone_map import bodies_from
    if out_dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
    if not isinstance(y, torch.Tensor) or not y.is_cuda or y.dtype != torch.float32 or y.dim() != 3 or y.shape[0] < 1:
        raise UserWarning("y: a float32 device tensor [F >= 1, M, O] (process_recording(return_targets=True))")
    if y.shape[2] != model.output_size:
        raise UserWarning(f"y: {y.shape[2]} targets per row, the model has {model.output_size}")
    lists = lists_of()
    sel = None if sel_of is None else sel_of()
    st = np.ascontiguousarray(np.asarray([0] if starts is None else starts, dtype=np.int32).reshape(-1))
    F, M, R, C_ = int(y.shape[0]), int(y.shape[1]), int(st.shape[0]), int(lists[0].shape[0])
    body = None
    if bodies is not None:
        body = np.ascontiguousarray(bodies.reshape(1, 9), dtype=np.float64) if isinstance(bodies, np.ndarray) and bodies.size == 9 \
            else bodies_from(bodies, R, f"{entry} bodies")
    yd = y.contiguous()
    dev = yd.device
    with torch.cuda.device(dev):
        width = 25 + (_hip.SPREAD_WIDTH if spread else 0)
        out = torch.empty((C_ if sel is None else int(sel.shape[0]), F, width), dtype=out_dtype, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(getattr(_hip.lib(), "ape_" + entry)(model.handle, C.c_void_p(yd.data_ptr()), F, M, C.c_void_p(st.ctypes.data), R,
                                                       *(C.c_void_p(a.ctypes.data) if a is not None else None for a in lists), C_,
                                                       *(() if sel is None else (C.c_void_p(sel.data_ptr()), int(sel.shape[0]))),
                                                       _hip.FLAG_SPREAD if spread else 0, C.c_void_p(body.ctypes.data) if body is not None else None,
                                                       int(body.shape[0]) if body is not None else 0, C.c_void_p(out.data_ptr()), _f64(out_dtype),
                                                       int(workspace_bytes), stream), "ape_" + entry)
    if spread:
        return out[:, :, :25], out[:, :, 25:]
    return out


def _post_last(entry: str) -> dict:
    """the four plan numbers ``ape_<entry>_last`` returns, named"""
    v = (C.c_int32 * 4)()
    _hip.check(getattr(_hip.lib(), f"ape_{entry}_last")(v), f"ape_{entry}_last")
    return {"passes": int(v[0]), "chunk_frames": int(v[1]), "tile_frames": int(v[2]), "lds": bool(v[3])}


def _post_plan(layout: int, F: int, back: int, ahead: int, samples: int, workspace_bytes: int) -> dict:
    """the workspace rule of include/ape_hip.h: the buffers hold ``back + chunk + ahead`` frames of ``samples`` rows twice"""
    frame_bytes = 8 * _hip.EST_WIDTH[layout] * samples
    bound = int(workspace_bytes) if workspace_bytes else 128 << 20
    chunk = min(int(F), bound // (2 * frame_bytes) - back - ahead)
    if chunk < 1:
        raise UserWarning(f"workspace_bytes {bound} holds no frame (at least {2 * frame_bytes * (back + ahead + 1)})")
    return {"passes": -(-int(F) // chunk), "chunk_frames": chunk, "frame_bytes": frame_bytes}


def post_sweep_last() -> dict:
    """the plan of this thread's last ``post_sweep`` (debug counter): passes over the workspace, frames per pass, frames per workgroup
    tile, and whether the tiles were staged in LDS"""
    return _post_last("post_sweep")


def post_sweep_plan(layout: int, F: int, configs, workspace_bytes: int = 0) -> dict:
    """the workspace rule of include/ape_hip.h on the host: frames per pass and passes of a ``post_sweep`` over ``F`` frames"""
    cf = _configs(configs)
    H = int(cf[:, 0].max()) - 1
    return dict(_post_plan(layout, F, H, 0, int(cf[:, 1].max()), workspace_bytes), halo_frames=H)


def score_configs(layout: int, out, spread, truth, configs, lags=(0, 0), truth_kind: str = "targets", starts=None, skip: int = 0,
                  bodies=None, error: str = "hand_pos") -> dict:
    """The scoring half of ``Estimator.sweep_recording``: one ``score_lags`` sweep per configuration on the strided views ``out[c]``
    (and ``spread[c]``; ``spread`` may be None) of a ``post_sweep`` result, assembled into ``{"configs": [(smooth, samples), ...],
    "acc": ndarray [C, R, L, 25], "best": [best_lag(acc[c], lags, error) per configuration]}`` (waits for the device)."""
    return _score_sets("score_configs", [(int(s), int(m)) for s, m in configs], layout, out, spread, truth, lags, truth_kind, starts, skip,
                       bodies, error)


def _score_sets(who: str, configs: list, layout: int, out, spread, truth, lags, truth_kind, starts, skip, bodies, error) -> dict:
    """one ``score_lags`` sweep per set ``out[c]`` (with ``spread[c]``), assembled: what ``score_configs`` and ``score_windows`` share"""
    if not configs or len(out) != len(configs) or (spread is not None and len(spread) != len(configs)):
        raise UserWarning(f"{who}: {len(configs)} configurations for {len(out)} results")
    accs = [_as_host(score_lags(layout, out[c], truth, lags, truth_kind, None if spread is None else spread[c], starts, skip, bodies)[1], (3,))
            for c in range(len(configs))]
    if any(a.shape != accs[0].shape for a in accs):
        raise UserWarning(f"{who}: accumulators of different sweeps")
    acc = np.stack(accs)
    return {"configs": configs, "acc": acc, "best": [best_lag(acc[c], lags, error) for c in range(len(configs))]}


# ---- windowed post-filter: centred and tapered windows over one replay's targets (ape_post_window) -------------------------
# ``smooth = n`` stacks the last n frames, so the estimate trails the motion by (n - 1) / 2 frames.  A recording processed offline can
# look ahead as far as it looks back: a window ``(back, ahead)`` with ``back == ahead`` has no group delay, and per-frame weights that
# fall off towards its ends keep the motion's curvature where a boxcar of the same width flattens it.  The same window is what a live
# estimator delayed by ``ahead`` frames could emit, so one call also answers what k frames of look-ahead would buy.
POST_MAX_WINDOW = _hip.POST_MAX_WINDOW
WINDOW_SHAPES = ("uniform", "triangle", "hann")


def window_weights(shape: str, back: int, ahead: int):
    """The frame weights of a window of ``back`` frames behind and ``ahead`` frames ahead of its frame, oldest frame first: float64
    ``[back + ahead + 1]`` summing to 1, or None for ``"uniform"``.  With ``d = j - back`` and ``D = max(back, ahead)``: ``"triangle"``
    is ``1 - |d| / (D + 1)``, ``"hann"`` is ``0.5 (1 + cos(pi d / (D + 1)))``, each divided by its sum.  Every weight is > 0 and the
    largest sits on the frame itself (index ``back``): a one-sided window peaks at its newest (``ahead == 0``) or oldest frame."""
    back, ahead = int(back), int(ahead)
    if back < 0 or ahead < 0 or back + ahead + 1 > POST_MAX_WINDOW:
        raise UserWarning(f"window ({back}, {ahead}): back, ahead >= 0 and back + ahead + 1 <= {POST_MAX_WINDOW}")
    if shape not in WINDOW_SHAPES:
        raise UserWarning(f"shape must be one of {WINDOW_SHAPES}, got {shape!r}")
    if shape == "uniform":
        return None
    d, D = np.arange(back + ahead + 1, dtype=np.float64) - back, max(back, ahead)
    w = 1.0 - np.abs(d) / (D + 1) if shape == "triangle" else 0.5 * (1.0 + np.cos(np.pi * d / (D + 1)))
    return w / w.sum()


def window(back: int, ahead: int, samples: int, shape_or_weights="uniform") -> tuple:
    """one configuration of ``post_window``: ``(back, ahead, samples, weights)`` with ``weights`` None (uniform) or float64
    ``[back + ahead + 1]``; ``shape_or_weights``: one of ``WINDOW_SHAPES`` or the frame weights themselves, oldest frame first, which
    must sum to 1 (they are passed on as they are)"""
    back, ahead, samples = int(back), int(ahead), int(samples)
    if isinstance(shape_or_weights, str):
        return (back, ahead, samples, window_weights(shape_or_weights, back, ahead))
    if shape_or_weights is None:
        return (back, ahead, samples, None)
    w = np.array(shape_or_weights, dtype=np.float64).reshape(-1)
    if back < 0 or ahead < 0 or w.shape[0] != back + ahead + 1:
        raise UserWarning(f"window ({back}, {ahead}): {w.shape[0]} weights for {back + ahead + 1} frames")
    return (back, ahead, samples, w)


def _windows(windows):
    """``(windows, int32 [C, 3], float64 [C, 64] | None)`` of a list of ``(back, ahead, samples[, shape or weights])`` entries: the list
    with every entry as ``window`` returns it, and the two arrays of the C ABI (no weight table where every window is uniform; the row
    of a uniform window in a table holds ``1 / n``, bit-equal entries)"""
    try:
        ws = [window(*w) for w in windows]
    except TypeError:
        raise UserWarning("windows: a list of (back, ahead, samples[, shape or weights]) entries (score.window)")
    if not 1 <= len(ws) <= _hip.POST_MAX_CONFIGS:
        raise UserWarning(f"windows: between 1 and {_hip.POST_MAX_CONFIGS} windows, got {len(ws)}")
    wn = np.ascontiguousarray(np.asarray([w[:3] for w in ws], dtype=np.int32).reshape(-1, 3))
    if (wn[:, :2] < 0).any() or (wn[:, 0] + wn[:, 1] + 1 > POST_MAX_WINDOW).any():
        raise UserWarning(f"windows: back, ahead >= 0 and back + ahead + 1 <= {POST_MAX_WINDOW}")
    if all(w[3] is None for w in ws):
        return ws, wn, None
    table = np.zeros((len(ws), POST_MAX_WINDOW), dtype=np.float64)
    for c, (b, a, _, w) in enumerate(ws):
        table[c, :b + a + 1] = 1.0 / (b + a + 1) if w is None else w
    return ws, wn, table


def post_window(model, y, windows, starts=None, bodies=None, spread: bool = False, out_dtype=torch.float64, workspace_bytes: int = 0):
    """The float64 post-filter of a replay from stored targets, as ``post_sweep``, at windows that may look ahead and may be tapered
    (``ape_post_window``).  ``model``, ``y``, ``starts``, ``bodies``, ``workspace_bytes``: ``post_sweep``'s; ``windows``: a list of
    ``window(back, ahead, samples, shape_or_weights)`` entries (plain ``(back, ahead, samples)`` tuples are uniform): window ``c`` stacks the
    first ``samples`` samples of the frames ``f - back .. f + ahead``, both ends clamped to the frame's recording, frame ``j`` weighted by
    ``weights[j]``.  A uniform ``(smooth - 1, 0, samples)`` gives the bits of ``post_sweep``'s ``(smooth, samples)``.
    Returns ``out [C, F, 25]`` of ``out_dtype`` on the device or, with ``spread``, ``(out, spread)`` with ``spread [C, F, 21]``: two
    views of one tensor.  Does not wait."""
    return _post_call("post_window", lambda: _windows(windows)[1:], model, y, starts, bodies, spread, out_dtype, workspace_bytes)


def post_window_last() -> dict:
    """the plan of this thread's last ``post_window`` (debug counter): passes over the workspace, frames per pass, frames per workgroup
    tile, and whether the tiles were staged in LDS"""
    return _post_last("post_window")


def post_window_plan(layout: int, F: int, windows, workspace_bytes: int = 0) -> dict:
    """the workspace rule of include/ape_hip.h on the host: frames per pass and passes of a ``post_window`` over ``F`` frames"""
    _, wn, _ = _windows(windows)
    H, A = int(wn[:, 0].max()), int(wn[:, 1].max())
    return dict(_post_plan(layout, F, H, A, int(wn[:, 2].max()), workspace_bytes), back_frames=H, ahead_frames=A)


def _targets_est(pred, body, layout: int) -> np.ndarray:
    """de-normalised targets ``[n, O]`` -> est rows ``[n, 21 | 14]`` under one body ``[9]``: the forward kinematics of
    estimate_joints.py:16-92 in numpy, with the closed-form quaternion of csrc/fk_device.h (the largest of trace, m00, m11, m22 as the
    pivot, then ``w >= 0``) where the reference takes an eigenvector"""
    def quat(s):
        a1, a2 = s[:, [0, 2, 4]], s[:, [1, 3, 5]]
        b1 = a1 / np.linalg.norm(a1, axis=1, keepdims=True)
        u2 = a2 - np.sum(b1 * a2, axis=1, keepdims=True) * b1
        b2 = u2 / np.linalg.norm(u2, axis=1, keepdims=True)
        b3 = np.cross(b1, b2, axis=1)
        m00, m01, m02, m10, m11, m12, m20, m21, m22 = b1[:, 0], b2[:, 0], b3[:, 0], b1[:, 1], b2[:, 1], b3[:, 1], b1[:, 2], b2[:, 2], b3[:, 2]
        tr = m00 + m11 + m22
        cand = np.stack([tr, m00, m11, m22], axis=1)
        piv = np.where(np.isnan(cand).any(axis=1), 0, np.argmax(np.nan_to_num(cand, nan=-np.inf), axis=1))
        s0, s1 = np.sqrt(tr + 1.0) * 2.0, np.sqrt(1.0 + m00 - m11 - m22) * 2.0
        s2, s3 = np.sqrt(1.0 + m11 - m00 - m22) * 2.0, np.sqrt(1.0 + m22 - m00 - m11) * 2.0
        forms = [np.stack([0.25 * s0, (m21 - m12) / s0, (m02 - m20) / s0, (m10 - m01) / s0], axis=1),
                 np.stack([(m21 - m12) / s1, 0.25 * s1, (m01 + m10) / s1, (m02 + m20) / s1], axis=1),
                 np.stack([(m02 - m20) / s2, (m01 + m10) / s2, 0.25 * s2, (m12 + m21) / s2], axis=1),
                 np.stack([(m10 - m01) / s3, (m02 + m20) / s3, (m12 + m21) / s3, 0.25 * s3], axis=1)]
        q = np.choose(piv[:, None], forms)
        return np.where(q[:, :1] < 0, -q, q)

    def hips_quat(sn, cs):
        half = 0.5 * np.arctan2(sn, cs)
        zero = np.zeros_like(half)
        return np.stack([np.cos(half), zero, np.sin(half), zero], axis=-1)

    n = pred.shape[0]
    larm_vec, uarm_vec, uarm_orig = (np.tile(body[i:i + 3], (n, 1)) for i in (0, 3, 6))
    with np.errstate(all="ignore"):
        if layout == _hip.LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS:
            uq, lq, hq = quat(pred[:, 12:18]), quat(pred[:, 3:9]), hips_quat(pred[:, 18], pred[:, 19])
            return np.concatenate([pred[:, 0:3], pred[:, 9:12], _qrot(hq, uarm_orig), lq, uq, hq], axis=1)
        uq, lq = quat(pred[:, 6:12]), quat(pred[:, 0:6])
        if layout == _hip.LAYOUT_ORI_CAL_LARM_UARM:
            lo = _qrot(uq, uarm_vec) + uarm_orig
            return np.concatenate([_qrot(lq, larm_vec) + lo, lo, lq, uq], axis=1)
        hq = hips_quat(pred[:, 12], pred[:, 13])
        uo = _qrot(hq, uarm_orig)
        lo = _qrot(uq, uarm_vec) + uo
        return np.concatenate([_qrot(lq, larm_vec) + lo, lo, uo, lq, uq, hq], axis=1)


def _stack_quat(qs, u=None) -> np.ndarray:
    """the sign-aligned mean of utility/transformations.py:32-51 over stacked quaternions ``[N, 4]``: row 0 is the reference direction,
    a row whose dot product with it is < 0.0 is subtracted, rows added in order, the sum normalised; ``u [N]``: the rows' weights
    (None: ``1 / N`` each)"""
    w = 1 / len(qs)
    acc = qs[0] * (w if u is None else u[0])
    for i in range(1, len(qs)):
        wi = w if u is None else u[i]
        acc = acc + qs[i] * (-wi if float(np.dot(qs[i], qs[0])) < 0.0 else wi)
    return acc / np.linalg.norm(acc)


def _stack_msg(stack, body, layout: int, u=None) -> np.ndarray:
    """the 25-value message of stacked est rows ``[N, W]`` (compose_msg.py:13-108; one row is copied): mean quaternions by ``_stack_quat``,
    the origins made again from them and the body ``[9]`` -- for the 20-target layout the means of the rows' origins, weighted:
    ``sum u_i e_i`` from +0.0 in stack order"""
    hips = layout != _hip.LAYOUT_ORI_CAL_LARM_UARM
    ql, qu = (9, 13) if hips else (6, 10)
    larm_vec, uarm_vec, uarm_orig = body[np.newaxis, 0:3], body[np.newaxis, 3:6], body[np.newaxis, 6:9]
    if stack.shape[0] == 1:
        ho, lo, lq, uq = stack[0, 0:3], stack[0, 3:6], stack[0, ql:ql + 4], stack[0, qu:qu + 4]
        uo, hq = (stack[0, 6:9], stack[0, 17:21]) if hips else (body[6:9], np.array([1.0, 0.0, 0.0, 0.0]))
        return np.concatenate([lq, ho, lq, lo, uq, uo, hq])
    hq = _stack_quat(stack[:, 17:21], u) if hips else np.array([1.0, 0.0, 0.0, 0.0])
    lq, uq = _stack_quat(stack[:, ql:ql + 4], u), _stack_quat(stack[:, qu:qu + 4], u)
    if layout == _hip.LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS:
        if u is None:
            uo, lo, ho = stack[:, 6:9].mean(axis=0), stack[:, 3:6].mean(axis=0), stack[:, 0:3].mean(axis=0)
        else:
            o = np.zeros(9)
            for i in range(stack.shape[0]):
                o = o + u[i] * stack[i, 0:9]
            ho, lo, uo = o[0:3], o[3:6], o[6:9]
    else:
        uo = _qrot(hq[np.newaxis], uarm_orig)[0] if hips else body[6:9]
        lo = _qrot(uq[np.newaxis], uarm_vec)[0] + uo
        ho = _qrot(lq[np.newaxis], larm_vec)[0] + lo
    return np.concatenate([lq, ho, lq, lo, uq, uo, hq])


def _taper_record(stack, msg, layout: int, u) -> np.ndarray:
    """the spread record of a tapered stack (``u [N]`` row weights summing to 1) from the weighted sums ``sum u p``, ``sum u (p_a p_b)``
    and ``sum u (q_a q_b)``, the rows in order: the mean is the first sum, the covariance ``sum u p p' - mean mean'``, the angle
    ``2 asin(sqrt(clip(1 - qm' (sum u q q') qm, 0, 1)))``"""
    out = np.zeros(_hip.SPREAD_WIDTH)
    ia, ib = np.triu_indices(3)
    for c0, o0 in ((0, 0), (3, 9)):
        s1, s2 = np.zeros(3), np.zeros(6)
        for i in range(stack.shape[0]):
            p = stack[i, c0:c0 + 3]
            s1, s2 = s1 + u[i] * p, s2 + u[i] * (p[ia] * p[ib])
        out[o0:o0 + 3], out[o0 + 3:o0 + 9] = s1, s2 - s1[ia] * s1[ib]
    ja, jb = np.triu_indices(4)
    diag = ja == jb
    for k, c in enumerate((9, 13, 17) if layout != _hip.LAYOUT_ORI_CAL_LARM_UARM else (6, 10)):
        s = np.zeros(10)
        for i in range(stack.shape[0]):
            q = stack[i, c:c + 4]
            s = s + u[i] * (q[ja] * q[jb])
        qm = msg[7 + 7 * k:11 + 7 * k]
        t = s * (qm[ja] * qm[jb])
        a = 1.0 - (t[diag].sum() + 2.0 * t[~diag].sum())
        out[18 + k] = 2.0 * np.arcsin(np.sqrt(np.clip(a, 0.0, 1.0)))
    return out


def post_window_numpy(y, yy_m, yy_s, bodies, layout: int, starts, windows):
    """The host statement of ``post_window``: ``y [F, M, O]`` normalised targets -> ``(out [C, F, 25], spread [C, F, 21])`` float64.
    Every sample row is de-normalised in float64 and taken through ``_targets_est`` with its recording's body (``bodies [1 | R, 9]``)
    once.  Stack row ``i`` of frame ``f`` of the recording ``[s, e)`` at window ``(back, ahead, m, weights)`` is sample ``i % m`` of
    frame ``min(e - 1, max(s, f - back + i // m))``.  A uniform window (no weights, or bit-equal ones) is the message ``_stack_msg`` of
    the stack at ``1 / N`` per row and the record ``_post.spread_rows`` of it; a tapered one weighs row ``i`` by
    ``u_i = weights[i // m] / m`` in ``_stack_msg`` and takes its record from ``_taper_record``."""
    from wear_mocap_ape_amd.estimate import _post
    y = np.asarray(y)
    F, M, O = y.shape
    st = [int(s) for s in ([0] if starts is None else starts)]
    ends = st[1:] + [F]
    bodies = np.asarray(bodies, dtype=np.float64).reshape(-1, 9)
    ws = _windows(windows)[0]
    pred = y.reshape(-1, O).astype(np.float64) * yy_s + yy_m
    E = np.zeros((F, M, _hip.EST_WIDTH[layout]))
    for r, (a, b) in enumerate(zip(st, ends)):
        E[a:b] = _targets_est(pred[a * M:b * M], bodies[r if bodies.shape[0] > 1 else 0], layout).reshape(b - a, M, -1)
    out, spread = np.zeros((len(ws), F, 25)), np.zeros((len(ws), F, _hip.SPREAD_WIDTH))
    with np.errstate(all="ignore"):
        for c, (back, ahead, m, w) in enumerate(ws):
            n = back + ahead + 1
            u = None if w is None or bool((w.view(np.int64) == w.view(np.int64)[0]).all()) else np.repeat(w / float(m), m)
            for r, (a, b) in enumerate(zip(st, ends)):
                body = bodies[r if bodies.shape[0] > 1 else 0]
                for f in range(a, b):
                    stack = np.concatenate([E[min(b - 1, max(a, f - back + j)), :m] for j in range(n)])
                    out[c, f] = _stack_msg(stack, body, layout, u)
                    spread[c, f] = _post.spread_rows(stack, out[c, f], layout) if u is None else _taper_record(stack, out[c, f], layout, u)
    return out, spread


def score_windows(layout: int, out, spread, truth, windows, lags=(0, 0), truth_kind: str = "targets", starts=None, skip: int = 0,
                  bodies=None, error: str = "hand_pos") -> dict:
    """The scoring half of ``Estimator.sweep_windows``: ``score_configs`` for the views ``out[c]`` (and ``spread[c]``; ``spread`` may be
    None) of a ``post_window`` result -> ``{"configs": [window(...) per window], "acc": ndarray [C, R, L, 25], "best":
    [best_lag(acc[c], lags, error) per window]}`` (waits for the device)."""
    return _score_sets("score_windows", _windows(windows)[0], layout, out, spread, truth, lags, truth_kind, starts, skip, bodies, error)


# ---- speed-adaptive smoothing: a window per frame from a ladder (ape_select_rungs, ape_post_select) ------------------------
# Arm motion is holds joined by reaches.  A hold wants a wide window, a reach a narrow one, and any fixed width is a compromise.  A ladder
# is a list of windows from narrow to wide; ``select_rungs`` picks a rung for every frame from a per-frame key (the hand speed of a pilot
# smoothing) with an envelope that keeps a wide window from covering a neighbouring reach, and ``post_select`` runs the post-filter at
# the rung chosen.  ``select_rungs_numpy`` and ``post_select_numpy`` are the host statements.
SELECT_MAX_EDGES, SELECT_MAX_SLOPE = _hip.SELECT_MAX_EDGES, _hip.SELECT_MAX_SLOPE
LADDER_HALVES = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 31)


def ladder(halves=LADDER_HALVES, samples: int = 1, shape: str = "hann") -> tuple:
    """``(windows, reach)`` of a ladder of centred windows: ``window(h, h, samples, shape)`` per half-width ``h`` of ``halves`` (the single
    frame ``(0, 0, samples)`` for ``h = 0``) and int32 ``reach [L]``, each rung's ``max(back, ahead)``.  ``halves`` must not decrease:
    a ladder runs narrow to wide."""
    hs = [int(h) for h in halves]
    if not hs or any(b < a for a, b in zip(hs, hs[1:])):
        raise UserWarning(f"ladder: half-widths that do not decrease, got {hs}")
    return [window(h, h, samples, shape if h > 0 else "uniform") for h in hs], np.asarray(hs, dtype=np.int32)


def _reach(ladder_or_reach) -> np.ndarray:
    """int32 ``[L]`` reaches of ``ladder``'s pair, of a list of windows, or of the reaches themselves; checked as the C ABI checks them"""
    lr = ladder_or_reach
    if isinstance(lr, tuple) and len(lr) == 2 and isinstance(lr[0], list):
        lr = lr[1]
    try:
        if len(lr) and isinstance(lr[0], (tuple, list)):
            lr = [max(int(w[0]), int(w[1])) for w in lr]
        reach = np.ascontiguousarray(np.asarray(lr, dtype=np.int32).reshape(-1))
    except (TypeError, ValueError):
        raise UserWarning("ladder_or_reach: score.ladder's pair, a list of windows, or the reaches [L]")
    if not 1 <= reach.shape[0] <= _hip.POST_MAX_CONFIGS:
        raise UserWarning(f"ladder: between 1 and {_hip.POST_MAX_CONFIGS} rungs, got {reach.shape[0]}")
    if (reach < 0).any() or (reach >= POST_MAX_WINDOW).any() or (np.diff(reach) < 0).any():
        raise UserWarning(f"ladder: reaches 0 .. {POST_MAX_WINDOW - 1} that do not decrease (narrow to wide), got {reach.tolist()}")
    return reach


def speed_edges(first: float = 0.003, ratio: float = 1.3, count: int = 10) -> np.ndarray:
    """a geometric ladder of ``count`` speed edges, ``first * ratio ** i``: with ``select_rungs``' default table a key up to ``first``
    takes the widest rung and every further edge below it one rung narrower"""
    if not (first > 0 and ratio > 1 and 1 <= int(count) <= SELECT_MAX_EDGES):
        raise UserWarning(f"speed_edges: first > 0, ratio > 1 and 1 .. {SELECT_MAX_EDGES} edges")
    return float(first) * float(ratio) ** np.arange(int(count), dtype=np.float64)


def _select_tables(edges, reach, slope, rung_of_slot, nan_rung):
    """the host arrays of ``ape_select_rungs`` with the defaults filled in: slot 0 -> the widest rung, each further slot one rung
    narrower, clamped at rung 0; a key that is not finite -> the widest rung (the frame then takes its cap from its neighbours)"""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
    L, B = int(reach.shape[0]), int(e.shape[0])
    if not 1 <= B <= SELECT_MAX_EDGES or not np.isfinite(e).all() or (np.diff(e) <= 0).any():
        raise UserWarning(f"edges: between 1 and {SELECT_MAX_EDGES} finite, strictly increasing values")
    ros = np.maximum(L - 1 - np.arange(B + 1), 0) if rung_of_slot is None else np.asarray(rung_of_slot).reshape(-1)
    ros = np.ascontiguousarray(ros, dtype=np.int32)
    nan_rung = L - 1 if nan_rung is None else int(nan_rung)
    if ros.shape[0] != B + 1 or (ros < 0).any() or (ros >= L).any() or not 0 <= nan_rung < L:
        raise UserWarning(f"rung_of_slot: {B + 1} rungs 0 .. {L - 1} (and nan_rung one of them)")
    if not 0 <= int(slope) <= SELECT_MAX_SLOPE:
        raise UserWarning(f"slope: 0 .. {SELECT_MAX_SLOPE}, got {slope}")
    return e, ros, nan_rung, int(slope)


def select_rungs_numpy(keys, edges, rung_of_slot, reach, slope: int, starts=None, nan_rung=None) -> np.ndarray:
    """The host statement of ``select_rungs``: ``keys [(S,) F]`` -> uint8 ``[(S,) F]``.  ``slot`` = the number of edges strictly below the
    key (right-closed bins), ``r0 = rung_of_slot[slot]``, ``nan_rung`` for a key that is not finite.  ``slope == 0``: ``r0``.  Otherwise,
    per recording, ``cap[f] = min_g reach[r0[g]] + |f - g| // slope`` and ``sel[f] = min(r0[f], the largest r with reach[r] <= cap[f])``."""
    k = np.asarray(keys)
    reach = _reach(reach)
    e, ros, nan_rung, slope = _select_tables(edges, reach, slope, rung_of_slot, nan_rung)
    k2 = k.reshape(-1, k.shape[-1]).astype(np.float64)
    F = k2.shape[1]
    st = [int(s) for s in ([0] if starts is None else starts)]
    r0 = np.where(np.isfinite(k2), ros[np.searchsorted(e, np.where(np.isfinite(k2), k2, 0.0), side="left")], nan_rung).astype(np.int64)
    sel = r0.copy()
    if slope > 0:
        for a, b in zip(st, st[1:] + [F]):
            idx = np.arange(a, b)
            dist = np.abs(idx[:, None] - idx[None, :]) // slope                               # [f, g]
            for s in range(k2.shape[0]):
                cap = (reach[r0[s, a:b]].astype(np.int64)[None, :] + dist).min(axis=1)
                widest = np.searchsorted(reach, cap, side="right") - 1                        # the largest r with reach[r] <= cap
                sel[s, a:b] = np.minimum(r0[s, a:b], widest)
    return sel.astype(np.uint8).reshape(k.shape)


def select_rungs(keys, edges, ladder_or_reach, slope: int = 2, rung_of_slot=None, starts=None, nan_rung=None):
    """A rung of a ladder for every frame, on the device (``ape_select_rungs``).  ``keys``: a device ``[F]`` or ``[S, F]`` view, float32 or
    float64, ``S <= 64`` -- a column of ``motion_sums``' per-frame rows (``motion[..., 0]``, the hand speed) goes in without a copy;
    ``edges``: float64 ``[B]``, strictly increasing (``speed_edges``); ``ladder_or_reach``: ``ladder``'s pair, a list of windows or the
    reaches themselves, narrow to wide; ``slope``: the envelope -- a frame's reach may exceed the reach chosen at frame ``g`` by at most
    ``|f - g| // slope`` (0: no envelope, the binning alone); ``rung_of_slot``: int ``[B + 1]``, the rung of every bin ``(e[i - 1], e[i]]``
    (default: slot 0 the widest rung, each further slot one rung narrower, clamped at rung 0); ``nan_rung``: the rung of a key that is
    not finite (default: the widest, so that such a frame takes its cap from its neighbours); ``starts``: the recordings' first frames
    -- nothing is read across a boundary.  Returns uint8 ``[(S,) F]`` on the device for ``post_select``.  Integer work: the same inputs
    give the same bits.  Does not wait."""
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda or keys.dim() not in (1, 2) or min(keys.shape) < 1:
        raise UserWarning("keys: a device tensor [F] or [S, F]")
    if keys.dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"keys: float32 or float64, got {keys.dtype}")
    reach = _reach(ladder_or_reach)
    e, ros, nan_rung, slope = _select_tables(edges, reach, slope, rung_of_slot, nan_rung)
    k = keys[None] if keys.dim() == 1 else keys
    S, F = int(k.shape[0]), int(k.shape[1])
    if S > _hip.POST_MAX_CONFIGS:
        raise UserWarning(f"keys: at most {_hip.POST_MAX_CONFIGS} sets, got {S}")
    ss, fs = int(k.stride(0)), int(k.stride(1))
    fs = fs if F > 1 else max(fs, 1)
    if fs < 1 or (S > 1 and ss <= (F - 1) * fs):
        k = k.contiguous()
        ss, fs = int(k.stride(0)), max(int(k.stride(1)), 1)
    st = _recording_starts(starts)
    dev = k.device
    with torch.cuda.device(dev):
        sel = torch.empty((S, F), dtype=torch.uint8, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_select_rungs(C.c_void_p(k.data_ptr()), _f64(k.dtype), S, ss if S > 1 else 0, F, fs, C.c_void_p(st.ctypes.data),
                                               int(st.shape[0]), C.c_void_p(e.ctypes.data), int(e.shape[0]), C.c_void_p(ros.ctypes.data), nan_rung,
                                               C.c_void_p(reach.ctypes.data), int(reach.shape[0]), slope, C.c_void_p(sel.data_ptr()), stream),
                   "ape_select_rungs")
    return sel[0] if keys.dim() == 1 else sel


def _ladder_windows(ladder_):
    """the windows of ``ladder``'s pair or of a plain list of windows"""
    return ladder_[0] if isinstance(ladder_, tuple) and len(ladder_) == 2 and isinstance(ladder_[0], list) else ladder_


def _selector(sel, F: int):
    """(uint8 device tensor [S, F] contiguous, whether ``sel`` came as ``[F]``)"""
    if not isinstance(sel, torch.Tensor) or not sel.is_cuda or sel.dtype != torch.uint8 or sel.dim() not in (1, 2) or sel.shape[-1] != F:
        raise UserWarning(f"sel: a uint8 device tensor [F] or [S, F] with F = {F} (select_rungs)")
    s2 = (sel[None] if sel.dim() == 1 else sel).contiguous()
    if not 1 <= s2.shape[0] <= _hip.POST_MAX_CONFIGS:
        raise UserWarning(f"sel: between 1 and {_hip.POST_MAX_CONFIGS} selector rows, got {s2.shape[0]}")
    return s2, sel.dim() == 1


def post_select(model, y, ladder, sel, starts=None, bodies=None, spread: bool = False, out_dtype=torch.float64, workspace_bytes: int = 0):
    """``post_window`` with a window per frame (``ape_post_select``).  ``model``, ``y``, ``starts``, ``bodies``, ``workspace_bytes``:
    ``post_window``'s; ``ladder``: ``ladder()``'s pair or a list of ``window`` entries (``post_window``'s list and limits); ``sel``: uint8
    device ``[F]`` or ``[S, F]``, the rung of every frame (``select_rungs``), ``S <= 64`` sets.  Row ``(s, f)`` of the result holds the
    bits ``post_window(ladder)[sel[s, f], f]`` holds; a selector value ``>= len(ladder)`` gives a row of NaN and touches nothing else.
    Returns ``out [(S,) F, 25]`` of ``out_dtype`` on the device or, with ``spread``, ``(out, spread [(S,) F, 21])``: two views of one
    tensor.  Does not wait."""
    F = int(y.shape[0]) if isinstance(y, torch.Tensor) and y.dim() == 3 else -1
    got = _post_call("post_select", lambda: _windows(_ladder_windows(ladder))[1:], model, y, starts, bodies, spread, out_dtype, workspace_bytes,
                     sel_of=lambda: _selector(sel, F)[0])
    if isinstance(sel, torch.Tensor) and sel.dim() == 1:
        return (got[0][0], got[1][0]) if spread else got[0]
    return got


def post_select_last() -> dict:
    """the plan of this thread's last ``post_select`` (debug counter), as ``post_window_last``"""
    return _post_last("post_select")


def post_select_plan(layout: int, F: int, ladder, workspace_bytes: int = 0) -> dict:
    """the workspace rule of include/ape_hip.h on the host: ``post_window_plan`` of the ladder (the halos are its longest reaches)"""
    return post_window_plan(layout, F, _ladder_windows(ladder), workspace_bytes)


def post_select_numpy(y, yy_m, yy_s, bodies, layout: int, starts, ladder, sel):
    """The host statement of ``post_select``: ``post_window_numpy`` of the ladder, then row ``(s, f)`` is that of window ``sel[s, f]`` at
    frame ``f`` and all NaN where ``sel[s, f] >= len(ladder)``.  ``sel``: integer ``[(S,) F]``; returns ``(out [(S,) F, 25], spread
    [(S,) F, 21])`` float64."""
    out, spread = post_window_numpy(y, yy_m, yy_s, bodies, layout, starts, _ladder_windows(ladder))
    s = np.asarray(sel).astype(np.int64)
    L, F = out.shape[0], out.shape[1]
    if s.ndim not in (1, 2) or s.shape[-1] != F:
        raise UserWarning(f"sel: [F] or [S, F] with F = {F}")
    ok = (s >= 0) & (s < L)
    pick = np.where(ok, s, 0)
    frames = np.broadcast_to(np.arange(F), s.shape)
    return (np.where(ok[..., None], out[pick, frames], np.nan), np.where(ok[..., None], spread[pick, frames], np.nan))


def score_selected(layout: int, out, spread, truth, names, lags=(0, 0), truth_kind: str = "targets", starts=None, skip: int = 0,
                   bodies=None, error: str = "hand_pos") -> dict:
    """``score_windows`` for the ``S`` sets ``out[s]`` (and ``spread[s]``; ``spread`` may be None) of a ``post_select`` result; ``names``:
    what to list under ``"configs"``, one entry per set (the rules that made the selectors)."""
    return _score_sets("score_selected", list(names), layout, out, spread, truth, lags, truth_kind, starts, skip, bodies, error)


# ---- each recording's heading and frame offset against the truth (ape_frame_sums, ape_rotate_rows) -------------------------
# A wearer who stood a few degrees off during the calibration pose, or a mocap frame that is not levelled, leaves a recording's whole
# estimate turned against the truth by a constant world-side rotation G, truth ~ G . estimate.  ``frame_sums`` takes the sums the
# least-squares G is read off, for every lag of a sweep in one pass; ``best_frame`` reads lag and rotation off them on the host;
# ``rotate_rows`` applies the rotation; ``align_frame`` does all three and scores the turned rows at the lags found.
FRAME_ACC_WIDTH = _hip.FRAME_ACC_WIDTH
JOINT_NAMES = ("larm", "uarm", "hips")


def _quat_matrix(q) -> np.ndarray:
    """``[..., 4]`` quaternions ``[w, x, y, z]`` -> ``[..., 3, 3]``, with the factor ``2 / |q|^2`` (an unnormalised quaternion is the
    rotation it stands for; the zero quaternion gives non-finite entries) -- the operations of csrc/frame_fit.hip in their order"""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    with np.errstate(all="ignore"):
        s = 2.0 / (w * w + x * x + y * y + z * z)
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        m = np.stack([1.0 - s * (yy + zz), s * (xy - wz), s * (xz + wy),
                      s * (xy + wz), 1.0 - s * (xx + zz), s * (yz - wx),
                      s * (xz - wy), s * (yz + wx), 1.0 - s * (xx + yy)], axis=-1)
    return m.reshape(q.shape[:-1] + (3, 3))


def _abt(t, e):
    """``T E'`` for stacks of 3x3 matrices, each entry ``t0 e0 + t1 e1 + t2 e2`` added left to right"""
    return (t[:, :, None, 0] * e[:, None, :, 0] + t[:, :, None, 1] * e[:, None, :, 1]) + t[:, :, None, 2] * e[:, None, :, 2]


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _pair_terms(m, t, layout: int):
    """the 49 terms ``[n, 49]`` of message rows ``m [n, 25]`` paired with est rows ``t``, and which pairs are summed ``[n]``"""
    hips = layout != _hip.LAYOUT_ORI_CAL_LARM_UARM
    ql, qu = (9, 13) if hips else (6, 10)
    used = np.r_[0:6, ql:ql + 4, qu:qu + 4, 17:21] if hips else np.r_[0:6, ql:ql + 4, qu:qu + 4]
    n = m.shape[0]
    v = np.zeros((n, 49))
    with np.errstate(all="ignore"):
        v[:, 0:9] = _abt(_quat_matrix(t[:, ql:ql + 4]), _quat_matrix(m[:, 7:11])).reshape(n, 9)
        v[:, 9:18] = _abt(_quat_matrix(t[:, qu:qu + 4]), _quat_matrix(m[:, 14:18])).reshape(n, 9)
        if hips:
            v[:, 18:27] = _abt(_quat_matrix(t[:, 17:21]), _quat_matrix(m[:, 21:25])).reshape(n, 9)
        v[:, 27:36] = (t[:, 0:3, None] * m[:, None, 4:7]).reshape(n, 9)
        v[:, 36:45] = (t[:, 3:6, None] * m[:, None, 11:14]).reshape(n, 9)
        v[:, 45], v[:, 46] = _dot3(t[:, 0:3], t[:, 0:3]), _dot3(m[:, 4:7], m[:, 4:7])
        v[:, 47], v[:, 48] = _dot3(t[:, 3:6], t[:, 3:6]), _dot3(m[:, 11:14], m[:, 11:14])
    ok = np.isfinite(m).all(axis=1) & np.isfinite(t[:, used]).all(axis=1) & np.isfinite(v).all(axis=1)
    return v, ok


def frame_sums_numpy(msg, truth_est, layout: int, lags, starts=None, skip: int = 0, rec_lags=None) -> np.ndarray:
    """The host statement of ``frame_sums`` for est-kind truth: float64 ``[R, L, 51]`` (include/ape_hip.h states the columns), over
    ``score_lags_numpy``'s pairs and support; every column is summed pairwise (an error of a few ulps of the sum, where adding row by
    row would leave ~sqrt(n) of them)."""
    m = np.asarray(msg, dtype=np.float64)[:, :25]
    t = np.asarray(truth_est, dtype=np.float64)
    st = np.asarray([0] if starts is None else starts, dtype=np.int64).reshape(-1)
    F, R = m.shape[0], st.shape[0]
    lo, hi, off = _sweep(lags, R, rec_lags)
    L = hi - lo + 1
    ends = np.r_[st[1:], F]
    acc = np.zeros((R, L, FRAME_ACC_WIDTH))
    for r in range(R):
        s, e, o = int(st[r]), int(ends[r]), int(off[r])
        a, b = max(s + skip, s + o + hi), min(e, e + o + lo)                # the support: a pair at every lag, past the skipped frames
        if a >= b:
            continue
        for j in range(L):
            l = o + lo + j
            v, ok = _pair_terms(m[a:b], t[a - l:b - l], layout)
            acc[r, j, :49] = np.ascontiguousarray(v[ok].T).sum(axis=1)       # along the contiguous axis: numpy's pairwise summation
            acc[r, j, 49], acc[r, j, 50] = ok.sum(), (~ok).sum()
    return acc


def frame_sums(layout: int, msg, truth, lags=(0, 0), truth_kind: str = "targets", starts=None, skip: int = 0, bodies=None, rec_lags=None):
    """The sums each recording's heading is read off, for the sweep of lags ``lags=(lo, hi)`` in one pass (``ape_frame_sums``).
    ``msg``, ``truth``, ``truth_kind``, ``starts``, ``skip``, ``bodies``, ``rec_lags``, the pairing and the support: ``score_lags``'s.
    Returns float64 ``[R, L, 51]`` on the device: ``[0:27]`` the sums of ``T_j E_j'`` over the matrices of the truth's and the
    message's lower-arm, upper-arm and hips quaternions (the hips block exactly 0 for the layout without hips), ``[27:45]`` the sums of
    ``t e'`` for hand and elbow, ``[45:49]`` the sums of their squared norms, ``[49]`` / ``[50]`` the pairs summed / not summed
    (``best_frame``).  The call does not wait for the device."""
    md, ms, _, _, td, st, body = _prepared(layout, msg, truth, truth_kind, None, starts, bodies, torch.float64)
    F, R, dev = int(md.shape[0]), int(st.shape[0]), md.device
    lo, hi, off = _sweep(lags, R, rec_lags)
    L = hi - lo + 1
    if not 1 <= L <= _hip.SCORE_MAX_LAGS:
        raise UserWarning(f"lags=({lo}, {hi}): between 1 and {_hip.SCORE_MAX_LAGS} lags")
    with torch.cuda.device(dev):
        acc = torch.empty((max(R, 1), L, FRAME_ACC_WIDTH), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_frame_sums(int(layout), C.c_void_p(md.data_ptr()), ms, _f64(md.dtype), C.c_void_p(td.data_ptr()),
                                             TRUTH_KINDS[truth_kind], _f64(td.dtype), F, C.c_void_p(st.ctypes.data), R, int(skip),
                                             C.c_void_p(body.ctypes.data), int(body.shape[0]), lo, hi,
                                             C.c_void_p(off.ctypes.data) if rec_lags is not None else None, C.c_void_p(acc.data_ptr()),
                                             stream), "ape_frame_sums")
    return acc


def _matrix_quat(G) -> np.ndarray:
    """unit quaternion ``[w, x, y, z]``, ``w >= 0``, of a rotation matrix (the largest of the four pivots)"""
    G = np.asarray(G, dtype=np.float64)
    tr = G[0, 0] + G[1, 1] + G[2, 2]
    piv = [tr, G[0, 0], G[1, 1], G[2, 2]]
    k = int(np.argmax(piv))
    if k == 0:
        q = np.array([1.0 + tr, G[2, 1] - G[1, 2], G[0, 2] - G[2, 0], G[1, 0] - G[0, 1]])
    elif k == 1:
        q = np.array([G[2, 1] - G[1, 2], 1.0 + G[0, 0] - G[1, 1] - G[2, 2], G[0, 1] + G[1, 0], G[0, 2] + G[2, 0]])
    elif k == 2:
        q = np.array([G[0, 2] - G[2, 0], G[0, 1] + G[1, 0], 1.0 + G[1, 1] - G[0, 0] - G[2, 2], G[1, 2] + G[2, 1]])
    else:
        q = np.array([G[1, 0] - G[0, 1], G[0, 2] + G[2, 0], G[1, 2] + G[2, 1], 1.0 + G[2, 2] - G[0, 0] - G[1, 1]])
    q = q / np.sqrt((q * q).sum())
    return -q if q[0] < 0.0 else q


def _fit(M, mode: str):
    """(objective, G [3, 3], yaw | None) of the rotation that maximises ``tr(G' M)``"""
    if mode == "yaw":
        sn, cs = M[0, 2] - M[2, 0], M[0, 0] + M[2, 2]
        psi = float(np.arctan2(sn, cs))
        c, s = np.cos(psi), np.sin(psi)
        return float(M[1, 1] + np.hypot(sn, cs)), np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]), psi
    U, S, Vt = np.linalg.svd(M)
    d = 1.0 if np.linalg.det(U @ Vt) >= 0.0 else -1.0
    return float(S[0] + S[1] + d * S[2]), U @ np.diag([1.0, 1.0, d]) @ Vt, None


def best_frame(acc, lags, mode: str = "yaw", weights=(1, 1, 1, 0, 0), rec_lags=None) -> list:
    """Each recording's lag and world-side rotation ``G`` (truth ~ G . estimate), read off the accumulators ``acc [R, L, 51]`` of a
    ``frame_sums`` sweep ``lags=(lo, hi)`` (with the ``rec_lags`` the sweep was made with).  ``weights``: of the lower-arm, upper-arm
    and hips rotation sums and of the hand and elbow position sums in ``M = sum_j w_j M_j + w_hand P_hand + w_elbow P_elbow``;
    the rotation maximises ``tr(G' M)``.
    ``mode="yaw"``   a turn about the vertical (y): ``psi = atan2(M[0,2] - M[2,0], M[0,0] + M[2,2])``, ``g = [cos psi/2, 0, sin psi/2, 0]``
                     (the hips quaternion's convention), objective ``M[1,1] + hypot(M[0,2] - M[2,0], M[0,0] + M[2,2])``
    ``mode="full"``  ``M = U S V'``, ``d = sign det(U V')``, ``G = U diag(1, 1, d) V'``, objective ``S0 + S1 + d S2``
    Per recording a dict: ``lag`` the lag with the largest objective (ties: the smaller ``|l|``, then the smaller ``l``), ``quat``
    ``[w, x, y, z]`` with ``w >= 0``, ``matrix`` ``G``, ``yaw`` (``"yaw"`` mode; None otherwise), ``objective`` ``[L]`` (NaN where a lag has no pair),
    ``pairs`` summed at ``lag``, and ``mean_cos_before`` / ``mean_cos_after``: per joint of ``JOINT_NAMES`` the mean cosine of the residual angle
    between truth and estimate before and after the rotation, ``(tr(G' M_j) / pairs - 1) / 2`` (NaN for a joint whose block is zero).
    A recording with no pairs: ``lag`` None, the identity, ``pairs`` 0."""
    if mode not in ("yaw", "full"):
        raise UserWarning(f"mode must be 'yaw' or 'full', got {mode!r}")
    a = acc.detach().cpu().numpy() if isinstance(acc, torch.Tensor) else np.asarray(acc)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 3 or a.shape[-1] != FRAME_ACC_WIDTH:
        raise UserWarning(f"expected accumulators [R,L,{FRAME_ACC_WIDTH}], got {tuple(a.shape)}")
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != 5 or not np.isfinite(w).all() or (w < 0.0).any() or not (w > 0.0).any():
        raise UserWarning("weights: five finite values >= 0 (lower arm, upper arm, hips, hand, elbow), not all zero")
    R, L = a.shape[0], a.shape[1]
    lo, hi, off = _sweep(lags, R, rec_lags)
    if hi - lo + 1 != L:
        raise UserWarning(f"best_frame: lags=({lo}, {hi}) for accumulators of {L} lags")
    res = []
    for r in range(R):
        ls = int(off[r]) + lo + np.arange(L)
        blocks = a[r, :, :45].reshape(L, 5, 3, 3)
        M = (blocks * w[None, :, None, None]).sum(axis=1)
        fits = [_fit(M[j], mode) if a[r, j, 49] > 0 else None for j in range(L)]
        obj = np.array([np.nan if f is None else f[0] for f in fits])
        cand = [j for j in range(L) if fits[j] is not None and np.isfinite(obj[j])]
        if not cand:
            nan3 = {k: float("nan") for k in JOINT_NAMES}
            res.append({"lag": None, "quat": np.array([1.0, 0.0, 0.0, 0.0]), "matrix": np.eye(3), "yaw": 0.0 if mode == "yaw" else None,
                        "objective": obj, "pairs": 0, "mean_cos_before": dict(nan3), "mean_cos_after": dict(nan3)})
            continue
        j = min(cand, key=lambda k: (-obj[k], abs(int(ls[k])), int(ls[k])))
        _, G, psi = fits[j]
        n = float(a[r, j, 49])
        before, after = {}, {}
        for k, name in enumerate(JOINT_NAMES):
            Mj = blocks[j, k]
            zero = not Mj.any()
            before[name] = float("nan") if zero else float((np.trace(Mj) / n - 1.0) / 2.0)
            after[name] = float("nan") if zero else float(((G * Mj).sum() / n - 1.0) / 2.0)
        quat = np.array([np.cos(psi / 2.0), 0.0, np.sin(psi / 2.0), 0.0]) if mode == "yaw" else _matrix_quat(G)
        res.append({"lag": int(ls[j]), "quat": quat, "matrix": G, "yaw": psi, "objective": obj, "pairs": int(n),
                    "mean_cos_before": before, "mean_cos_after": after})
    return res


def _qmul(a, b):
    """the quaternion product of utility/transformations.py, term order as in csrc/fk_device.h"""
    return np.stack([a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2],
                     a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1],
                     a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]], axis=-1)


def _mat_vec(G, p):
    """``G p`` per row, each entry added left to right"""
    return (G[:, :, 0] * p[:, None, 0] + G[:, :, 1] * p[:, None, 1]) + G[:, :, 2] * p[:, None, 2]


def _unit_quats(quats, R: int) -> np.ndarray:
    """float64 ``[1 | R, 4]`` of one quaternion or one per recording, normalised; zero and non-finite quaternions are refused"""
    q = np.asarray(quats, dtype=np.float64)
    q = q.reshape(1, 4) if q.size == 4 else q
    if q.ndim != 2 or q.shape[1] != 4 or q.shape[0] not in (1, R):
        raise UserWarning(f"quats: one quaternion [4] or one per recording [{R}, 4], got {tuple(q.shape)}")
    with np.errstate(all="ignore"):
        n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    if not (np.isfinite(n).all() and (n > 0.0).all()):
        raise UserWarning("quats: a zero or non-finite quaternion")
    return np.ascontiguousarray(q / n[:, None])


def rotate_rows_numpy(msg, quats, spread=None, starts=None):
    """The host statement of ``rotate_rows``: float64 ``out [F, 25]`` or ``(out, spread [F, 21])``.  With ``g`` the recording's
    quaternion (normalised) and ``G`` its matrix: message quaternions ``g (x) q``, origins ``G p``, spread means ``G m``, covariances
    ``G S G'``, angular spreads as they are."""
    m = np.asarray(msg, dtype=np.float64)[:, :25]
    st = np.asarray([0] if starts is None else starts, dtype=np.int64).reshape(-1)
    F, R = m.shape[0], st.shape[0]
    unit = _unit_quats(quats, R)
    rec = np.searchsorted(st, np.arange(F), side="right") - 1 if unit.shape[0] > 1 else np.zeros(F, dtype=np.int64)
    g = unit[rec]
    G = _quat_matrix(g)
    out = np.empty((F, 25))
    with np.errstate(all="ignore"):
        for c in (0, 7, 14, 21):
            out[:, c:c + 4] = _qmul(g, m[:, c:c + 4])
        for c in (4, 11, 18):
            out[:, c:c + 3] = _mat_vec(G, m[:, c:c + 3])
        if spread is None:
            return out
        s = np.asarray(spread, dtype=np.float64)[:, :_hip.SPREAD_WIDTH]
        rot = np.empty((F, _hip.SPREAD_WIDTH))
        for o in (0, 9):
            rot[:, o:o + 3] = _mat_vec(G, s[:, o:o + 3])
            S = s[:, o + 3:o + 9][:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(F, 3, 3)
            A = (G[:, :, None, 0] * S[:, None, 0, :] + G[:, :, None, 1] * S[:, None, 1, :]) + G[:, :, None, 2] * S[:, None, 2, :]     # G S
            full = _abt(A, G)                                                                                                       # (G S) G'
            rot[:, o + 3:o + 9] = full.reshape(F, 9)[:, [0, 1, 2, 4, 5, 8]]
        rot[:, 18:] = s[:, 18:]
    return out, rot


def rotate_rows(layout: int, msg, quats, spread=None, starts=None, out_dtype=None):
    """Replay rows turned by a world-side rotation per recording (``ape_rotate_rows``): ``msg`` device ``[F, >= 25]`` (nothing past
    column 24 is read), ``quats`` ``[4]`` or ``[R, 4]`` ``[w, x, y, z]`` (normalised here; ``best_frame``'s ``quat``), ``spread``
    device ``[F, >= 21]`` of ``msg``'s dtype or None, ``starts`` the recordings' first frames.  Returns ``out [F, 25]`` of ``out_dtype``
    (default: ``msg``'s), or with ``spread`` ``(out, spread [F, 21])``, two views of one ``[F, 46]`` tensor as
    ``process_recording(spread=True)`` returns them.  The call does not wait for the device."""
    if layout not in _hip.EST_WIDTH:
        raise UserWarning(f"layout {layout} has no pose to rotate")
    md, ms = _rows_view(msg, 25, "msg")
    out_dtype = md.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
    F, dev = int(md.shape[0]), md.device
    sd, ss = (None, 0)
    if spread is not None:
        sd, ss = _rows_view(spread, _hip.SPREAD_WIDTH, "spread")
        if sd.dtype != md.dtype or sd.shape[0] != F or sd.device != dev:
            raise UserWarning("spread: the dtype, device and frame count of msg")
    st = np.ascontiguousarray(np.asarray([0] if starts is None else starts, dtype=np.int32).reshape(-1))
    R = int(st.shape[0])
    unit = _unit_quats(quats, R)
    with torch.cuda.device(dev):
        width = 25 + (_hip.SPREAD_WIDTH if sd is not None else 0)
        out = torch.empty((F, width), dtype=out_dtype, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_rotate_rows(int(layout), C.c_void_p(md.data_ptr()), ms, C.c_void_p(sd.data_ptr()) if sd is not None else None,
                                              ss, _f64(md.dtype), F, C.c_void_p(st.ctypes.data), R, C.c_void_p(unit.ctypes.data),
                                              int(unit.shape[0]), C.c_void_p(out.data_ptr()), _f64(out_dtype), stream), "ape_rotate_rows")
    if sd is not None:
        return out[:, :25], out[:, 25:]
    return out


def align_frame(layout: int, msg, truth, lags, mode: str = "yaw", weights=(1, 1, 1, 0, 0), truth_kind: str = "targets", spread=None,
                starts=None, skip: int = 0, bodies=None):
    """Find each recording's lag and heading together and score with both removed: a ``frame_sums`` sweep, ``best_frame`` on it (this
    waits for the device), ``rotate_rows`` by the rotations found, then ``score_lags`` of the turned rows with ``lags=(0, 0)`` and the
    lags found as offsets (lag 0 and no turn for a recording with an empty support).  Returns ``(score, acc, found)``: the per-frame
    rows ``[F, 7]`` and accumulators ``[R, 25]`` at every recording's own lag and heading, and ``best_frame``'s list."""
    sums = frame_sums(layout, msg, truth, lags, truth_kind, starts, skip, bodies)
    found = best_frame(sums, lags, mode, weights)
    quats = np.stack([b["quat"] for b in found])
    rec_lags = [0 if b["lag"] is None else b["lag"] for b in found]
    turned = rotate_rows(layout, msg, quats, spread, starts)
    out, rec = turned if spread is not None else (turned, None)
    score, acc = score_lags(layout, out, truth, (0, 0), truth_kind, rec, starts, skip, bodies, rec_lags, per_frame=True)
    return score[:, 0], acc[:, 0], found


# ---- mocap truth on each frame's clock (ape_frame_times, ape_resample_truth) -------------------------------------------------
# Every scorer above pairs message row f with truth row f - l for an integer l and expects one truth row per frame.  ``frame_times``
# builds a recording's clock from its sw_dt column, ``resample_truth`` produces est-kind truth rows at each frame's time (less a shift
# per recording) from truth on a clock of its own; a row it cannot produce is all NaN, which the scorers count as not scorable.
def _recording_starts(starts) -> np.ndarray:
    return np.ascontiguousarray(np.asarray([0] if starts is None else starts, dtype=np.int32).reshape(-1))


def frame_times_numpy(dt, starts=None) -> np.ndarray:
    """The host statement of ``frame_times``: float64 ``[F]``, per recording ``t[s] = 0`` and ``t[f] = t[f - 1] + float64(dt[f])`` (a
    ``np.cumsum`` whose first term is 0: the first row's ``dt`` points before the recording)."""
    d = np.asarray(dt).reshape(-1).astype(np.float64)
    st = _recording_starts(starts).astype(np.int64)
    out = np.empty(d.shape[0])
    with np.errstate(all="ignore"):
        for a, b in zip(st, np.r_[st[1:], d.shape[0]]):
            seg = d[a:b].copy()
            seg[0] = 0.0
            out[a:b] = np.cumsum(seg)
    return out


def frame_times(dt, starts=None, big_endian: bool = False):
    """Each recording's clock from its ``sw_dt`` column (``ape_frame_times``): ``dt`` a 1-D float32 or float64 device tensor or a
    strided column view (``rows[:, 0]`` of raw ``[F, 55 | 28]`` rows goes in without a copy), ``starts`` the recordings' first frames,
    ``big_endian``: the float32 values are UDP payload bytes as received.  Returns float64 ``[F]`` on the device: 0 at a recording's
    first frame, then the running sum of the following ``dt`` (a non-finite ``dt`` spoils the rest of its own recording only).  The
    same inputs give the same bits.  The call does not wait for the device."""
    if not isinstance(dt, torch.Tensor) or not dt.is_cuda or dt.dim() != 1 or dt.shape[0] < 1 or dt.dtype not in (torch.float32, torch.float64):
        raise UserWarning("dt: a 1-D float32 or float64 device tensor [F >= 1] (a column view of raw rows is fine)")
    if big_endian and dt.dtype != torch.float32:
        raise UserWarning("big_endian: the rows are float32 payloads")
    if dt.shape[0] > 1 and dt.stride(0) < 1:
        dt = dt.contiguous()
    F, stride, dev = int(dt.shape[0]), max(int(dt.stride(0)), 1), dt.device
    st = _recording_starts(starts)
    with torch.cuda.device(dev):
        times = torch.empty((F,), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_frame_times(C.c_void_p(dt.data_ptr()), stride, _f64(dt.dtype), _hip.PARSE_BIG_ENDIAN if big_endian else 0, F,
                                              C.c_void_p(st.ctypes.data), int(st.shape[0]), C.c_void_p(times.data_ptr()), stream),
                   "ape_frame_times")
    return times


def _slerp(a, b, w):
    """the quaternion between ``a`` and ``b [n, 4]`` at weights ``w [n]``, the operations of csrc/resample.hip in their order: both
    normalised, ``b`` flipped where ``a . b < 0.0``, ``theta = 2 asin(min(1, |a - s b| / 2))``, the chord below 1e-6 rad and the arc
    ``(sin((1 - w) theta) a + sin(w theta) s b) / sin(theta)`` otherwise, normalised again"""
    def norm(v):
        return np.sqrt(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) + v[:, 3] * v[:, 3])

    a, b, w = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(w, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        a, b = a / norm(a)[:, None], b / norm(b)[:, None]
        dot = ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]) + a[:, 3] * b[:, 3]
        b = np.where(dot < 0.0, -1.0, 1.0)[:, None] * b
        theta = (2.0 * np.arcsin(np.minimum(norm(a - b) / 2.0, 1.0)))[:, None]
        chord = a + w * (b - a)
        arc = (np.sin((1.0 - w) * theta) * a + np.sin(w * theta) * b) / np.sin(theta)
        q = np.where(theta < 1e-6, chord, arc)
        return q / norm(q)[:, None]


def resample_truth_numpy(layout: int, truth_est, truth_starts=None, truth_times=None, times=None, frames=None, starts=None, shifts=None,
                         max_gap: float = 0.0) -> np.ndarray:
    """The host statement of ``resample_truth`` for est-kind truth ``[Ft, 21 | 14]``: float64 ``[F, 21 | 14]`` by the seven rules of
    include/ape_hip.h in their order -- a non-finite query, no truth row at or before it, an exact hit (the row itself), past the last
    sample, a gap above ``max_gap``, a non-finite value in either neighbour, else positions ``a + w (b - a)`` and quaternions by
    ``_slerp``.  Clocks, recordings and shifts as ``resample_truth`` takes them (host arrays)."""
    if layout not in _hip.EST_WIDTH:
        raise UserWarning(f"layout {layout} has no pose to resample")
    t = np.asarray(truth_est, dtype=np.float64)
    W = _hip.EST_WIDTH[layout]
    if t.ndim != 2 or t.shape[1] != W:
        raise UserWarning(f"truth_est: expected [Ft,{W}], got {tuple(t.shape)}")
    hips = layout != _hip.LAYOUT_ORI_CAL_LARM_UARM
    Ft = t.shape[0]
    tts = None if truth_times is None else np.asarray(truth_times, dtype=np.float64).reshape(-1)
    tqs = None if times is None else np.asarray(times, dtype=np.float64).reshape(-1)
    if tqs is None and frames is None:
        raise UserWarning("frames: the number of output frames, where times is None")
    F = int(frames) if tqs is None else tqs.shape[0]
    st, tst = _recording_starts(starts).astype(np.int64), _recording_starts(truth_starts).astype(np.int64)
    R = st.shape[0]
    if tst.shape[0] != R:
        raise UserWarning(f"truth_starts: {tst.shape[0]} recordings of truth for {R} of frames")
    sh = np.zeros(R) if shifts is None else np.broadcast_to(np.asarray(shifts, dtype=np.float64).reshape(-1), (R,))
    npos = 9 if hips else 6
    out = np.full((F, W), np.nan)
    with np.errstate(all="ignore"):
        for r in range(R):
            s, e = int(st[r]), int(st[r + 1]) if r + 1 < R else F
            ts, te = int(tst[r]), int(tst[r + 1]) if r + 1 < R else Ft
            n = te - ts
            tt = np.arange(n, dtype=np.float64) if tts is None else tts[ts:te]
            u = (np.arange(e - s, dtype=np.float64) if tqs is None else tqs[s:e]) - sh[r]
            rows = t[ts:te]
            fin = np.isfinite(u)
            i = np.searchsorted(tt, np.where(fin, u, 0.0), side="right") - 1          # the last row with tt <= u: of equal stamps the last
            has = fin & (i >= 0)
            ic = np.clip(i, 0, n - 1)
            hit = has & (u == tt[ic])
            seg = out[s:e]
            seg[hit] = rows[ic[hit]]
            i1 = np.clip(ic + 1, 0, n - 1)
            gap = tt[i1] - tt[ic]
            mid = has & ~hit & (i < n - 1)
            if max_gap > 0.0:
                mid &= ~(gap > max_gap)
            mid &= np.isfinite(rows[ic]).all(axis=1) & np.isfinite(rows[i1]).all(axis=1)
            a, b = rows[ic[mid]], rows[i1[mid]]
            w = (u[mid] - tt[ic[mid]]) / gap[mid]
            res = np.empty((a.shape[0], W))
            res[:, :npos] = a[:, :npos] + w[:, None] * (b[:, :npos] - a[:, :npos])
            for c in range(npos, W, 4):
                res[:, c:c + 4] = _slerp(a[:, c:c + 4], b[:, c:c + 4], w)
            seg[mid] = res
    return out


def _body_rows(bodies, R: int, what: str) -> np.ndarray:
    """float64 ``[1 | R, 9]`` of ``score_rows``'s ``bodies`` argument"""
    from wear_mocap_ape_amd.data_types.bone_map import bodies_from, body9_from_bonemap
    if bodies is None:
        return body9_from_bonemap(None)[np.newaxis, :]
    if isinstance(bodies, np.ndarray) and bodies.size == 9:
        return np.ascontiguousarray(bodies.reshape(1, 9), dtype=np.float64)
    if not isinstance(bodies, np.ndarray) and not hasattr(bodies, "__len__"):
        return body9_from_bonemap(bodies)[np.newaxis, :]              # one bonemap-like object: that body for every recording
    return bodies_from(bodies, R, what)


def _clock(t, n: int, dev, what: str):
    if not isinstance(t, torch.Tensor) or t.device != dev or t.dim() != 1 or t.shape[0] != n or not t.dtype.is_floating_point:
        raise UserWarning(f"{what}: a floating-point device tensor [{n}] on {dev}")
    return t.to(torch.float64).contiguous()


def resample_truth(layout: int, truth, truth_kind: str = "est", truth_starts=None, truth_times=None, times=None, frames=None, starts=None,
                   shifts=None, max_gap: float = 0.0, bodies=None, out_dtype=torch.float64, check_times: bool = True):
    """Truth rows at each frame's time (``ape_resample_truth``).  ``truth``: device ``[Ft, 21 | 14]`` est rows (``truth_kind="est"``) or
    ``[Ft, O]`` de-normalised NN targets (``"targets"``, converted as ``score_rows`` converts them, with ``bodies``), float32 or
    float64, on a clock of its own: ``truth_times`` device float64 ``[Ft]`` (None: the index clock, row ``i`` of a recording at time
    ``i``), ``truth_starts`` the recordings' first truth rows.  ``times``: device float64 ``[F]``, the frames' clock (``frame_times``;
    None: the index clock, with ``frames`` giving ``F``); ``starts`` the recordings' first frames, as many as ``truth_starts``.
    ``shifts``: one value or ``[R]``, frame ``f`` is asked at ``times[f] - shifts[r]`` -- positive: the estimate is late, ``score_lags``'s
    sign; in frames on two index clocks (``best_lag``'s ``refined``), else in the clocks' unit.  ``max_gap > 0``: two truth samples
    further apart are not bridged.  Returns device ``[F, 21 | 14]`` est rows of ``out_dtype`` for ``score_rows(..., truth_kind="est")``
    and the other scorers: the truth row itself on an exact hit, positions interpolated linearly and quaternions along the arc between
    two samples, all NaN where there is none (before the first or past the last sample, a dropout, a non-finite neighbour or time).
    ``check_times=True`` verifies on the device that the truth times are finite and non-decreasing inside every recording and raises
    ``UserWarning`` if not: THIS WAITS FOR THE DEVICE.  With ``check_times=False`` (or without ``truth_times``) the call does not wait;
    unsorted times then give rows from somewhere inside the recording, never a read outside it."""
    if truth_kind not in TRUTH_KINDS:
        raise UserWarning(f"truth_kind must be one of {sorted(TRUTH_KINDS)}, got {truth_kind!r}")
    if layout not in _hip.EST_WIDTH:
        raise UserWarning(f"layout {layout} has no pose to resample")
    if out_dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
    tw = (_hip.NUM_TARGETS if truth_kind == "targets" else _hip.EST_WIDTH)[layout]
    if not isinstance(truth, torch.Tensor) or not truth.is_cuda or truth.dtype not in (torch.float32, torch.float64) or truth.dim() != 2 \
            or truth.shape[0] < 1 or truth.shape[1] != tw:
        raise UserWarning(f"truth: a float32 or float64 device tensor [Ft >= 1, {tw}]")
    td, dev = truth.contiguous(), truth.device
    Ft = int(td.shape[0])
    tst, st = _recording_starts(truth_starts), _recording_starts(starts)
    R = int(st.shape[0])
    if tst.shape[0] != R:
        raise UserWarning(f"truth_starts: {tst.shape[0]} recordings of truth for {R} of frames")
    if times is None:
        if frames is None:
            raise UserWarning("frames: the number of output frames, where times is None")
        F, tq = int(frames), None
    else:
        if frames is not None and int(frames) != int(times.shape[0]):
            raise UserWarning(f"frames={frames} for {int(times.shape[0])} times")
        F = int(times.shape[0])
        tq = _clock(times, F, dev, "times")
    tt = None if truth_times is None else _clock(truth_times, Ft, dev, "truth_times")
    sh = None
    if shifts is not None:
        sh = np.asarray(shifts, dtype=np.float64).reshape(-1)
        if sh.shape[0] not in (1, R):
            raise UserWarning(f"shifts: one value or one per recording [{R}], got {sh.shape[0]}")
        sh = np.ascontiguousarray(np.broadcast_to(sh, (R,)))
    body = _body_rows(bodies, R, "resample_truth bodies")
    with torch.cuda.device(dev):
        if check_times and tt is not None:
            ok = torch.isfinite(tt).all()
            if Ft > 1:
                rising = tt[1:] >= tt[:-1]
                if R > 1 and int(tst.max()) < Ft and int(tst[1:].min()) >= 1:
                    rising[torch.as_tensor(tst[1:].astype(np.int64) - 1, device=dev)] = True      # across a boundary anything goes
                ok = ok & rising.all()
            if not bool(ok):
                raise UserWarning("truth_times: not finite, or decreasing inside a recording")
        out = torch.empty((F, _hip.EST_WIDTH[layout]), dtype=out_dtype, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_resample_truth(int(layout), C.c_void_p(td.data_ptr()), TRUTH_KINDS[truth_kind], _f64(td.dtype), Ft,
                                                 C.c_void_p(tst.ctypes.data), C.c_void_p(tt.data_ptr()) if tt is not None else None,
                                                 C.c_void_p(tq.data_ptr()) if tq is not None else None, F, C.c_void_p(st.ctypes.data), R,
                                                 C.c_void_p(sh.ctypes.data) if sh is not None else None, float(max_gap),
                                                 C.c_void_p(body.ctypes.data), int(body.shape[0]), C.c_void_p(out.data_ptr()),
                                                 _f64(out_dtype), stream), "ape_resample_truth")
    return out


def truth_on_frames(layout: int, rows, truth, truth_times, truth_starts=None, starts=None, shifts=None, max_gap: float = 0.0,
                    truth_kind: str = "targets", bodies=None, big_endian: bool = False):
    """The truth of a recording session on its IMU frames.  ``rows``: raw messages ``[F, 55 | 28]``, float32, whose column 0 is
    ``sw_dt`` -- a device tensor, or a host array that is copied to ``truth``'s device; ``big_endian``: UDP payloads as received.
    ``truth`` and ``truth_times``: the mocap rows and their stamps on the device, in the unit of ``sw_dt`` (seconds); both clocks start
    at 0 with each recording (``frame_times``); ``shifts``: what the estimate is late by.  ``frame_times(rows[:, 0])`` and then
    ``resample_truth``; returns float64 est rows ``[F, 21 | 14]`` on the device.  Checks the truth times, so it waits for the device."""
    if not isinstance(truth, torch.Tensor) or not truth.is_cuda:
        raise UserWarning("truth: a device tensor")
    if isinstance(rows, np.ndarray):
        rows = torch.from_numpy(np.ascontiguousarray(rows)).to(truth.device)
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[1] not in (55, 28) or rows.dtype != torch.float32 \
            or rows.device != truth.device:
        raise UserWarning("rows: float32 raw messages [F, 55 | 28] on truth's device (or a host array)")
    times = frame_times(rows[:, 0], starts, big_endian)
    return resample_truth(layout, truth, truth_kind, truth_starts, truth_times, times, None, starts, shifts, max_gap, bodies)


# ---- each recording's arm lengths and shoulder origin against the truth (ape_body_sums, ape_rebody_rows) -------------------
# Every position of a message is forward kinematics of its own quaternions through the nine numbers of a body (larm_vec, uarm_vec,
# uarm_orig): elbow = R_h o + R_u v_u, hand = elbow + R_l v_l.  The body enters linearly, so a recording's least-squares body solves a
# 9 x 9 system of sums over its frames: ``body_sums`` takes the sums for every lag of a sweep in one pass, ``best_body`` solves on the
# host, ``rebody_rows`` makes the rows' positions again under the body found, ``align_body`` does all three and scores what remains.
BODY_ACC_WIDTH = _hip.BODY_ACC_WIDTH
ROTATIONS = {"estimate": _hip.BODY_ROT_MSG, "truth": _hip.BODY_ROT_TRUTH}


def _atb(x, y):
    """``X' Y`` for stacks of 3x3 matrices, each entry ``x0 y0 + x1 y1 + x2 y2`` added left to right"""
    return (x[:, 0, :, None] * y[:, 0, None, :] + x[:, 1, :, None] * y[:, 1, None, :]) + x[:, 2, :, None] * y[:, 2, None, :]


def _atv(x, t):
    """``X' t`` per row, each entry added left to right"""
    return (x[:, 0, :] * t[:, None, 0] + x[:, 1, :] * t[:, None, 1]) + x[:, 2, :] * t[:, None, 2]


def _body_terms(m, t, layout: int, from_truth: bool):
    """the 44 terms ``[n, 44]`` of message rows ``m [n, 25]`` (None with ``from_truth``) paired with est rows ``t``, and which pairs
    are summed ``[n]``"""
    hips = layout != _hip.LAYOUT_ORI_CAL_LARM_UARM
    ql, qu = (9, 13) if hips else (6, 10)
    used = np.r_[0:6, ql:ql + 4, qu:qu + 4, 17:21] if hips else np.r_[0:6, ql:ql + 4, qu:qu + 4]
    n = t.shape[0]
    if from_truth:
        quats = [t[:, ql:ql + 4], t[:, qu:qu + 4]] + ([t[:, 17:21]] if hips else [])
    else:
        quats = [m[:, 7:11], m[:, 14:18]] + ([m[:, 21:25]] if hips else [])
    v = np.zeros((n, 44))
    with np.errstate(all="ignore"):
        Rl, Ru = _quat_matrix(quats[0]), _quat_matrix(quats[1])
        Rh = _quat_matrix(quats[2]) if hips else np.broadcast_to(np.eye(3), (n, 3, 3))
        th, te = t[:, 0:3], t[:, 3:6]
        v[:, 0:9], v[:, 9:18], v[:, 18:27] = _atb(Rl, Ru).reshape(n, 9), _atb(Rl, Rh).reshape(n, 9), _atb(Ru, Rh).reshape(n, 9)
        v[:, 27:30], v[:, 30:33], v[:, 33:36] = _atv(Rl, th), _atv(Ru, th), _atv(Rh, th)
        v[:, 36:39], v[:, 39:42] = _atv(Ru, te), _atv(Rh, te)
        v[:, 42], v[:, 43] = _dot3(th, th), _dot3(te, te)
    ok = np.isfinite(t[:, used]).all(axis=1) & np.isfinite(v).all(axis=1)
    for q in quats:
        ok &= np.isfinite(q).all(axis=1)
    return v, ok


def _rotations(rotations) -> int:
    if rotations not in ROTATIONS:
        raise UserWarning(f"rotations must be one of {sorted(ROTATIONS)}, got {rotations!r}")
    return ROTATIONS[rotations]


def body_sums_numpy(msg, truth_est, layout: int, lags, starts=None, skip: int = 0, rec_lags=None, rotations: str = "estimate") -> np.ndarray:
    """The host statement of ``body_sums`` for est-kind truth: float64 ``[R, L, 46]`` (include/ape_hip.h states the columns), over
    ``score_lags_numpy``'s pairs and support; every column is summed pairwise, as in ``frame_sums_numpy``.  ``rotations="truth"``: the
    matrices are the paired truth row's, ``msg`` is not read (None is fine) and the sweep must be ``(0, 0)`` without ``rec_lags``."""
    from_truth = _rotations(rotations) == _hip.BODY_ROT_TRUTH
    t = np.asarray(truth_est, dtype=np.float64)
    m = None if from_truth else np.asarray(msg, dtype=np.float64)[:, :25]
    st = np.asarray([0] if starts is None else starts, dtype=np.int64).reshape(-1)
    F, R = t.shape[0], st.shape[0]
    lo, hi, off = _sweep(lags, R, rec_lags)
    if from_truth and ((lo, hi) != (0, 0) or rec_lags is not None):
        raise UserWarning("rotations='truth': the sweep must be the single lag 0, without rec_lags")
    L = hi - lo + 1
    ends = np.r_[st[1:], F]
    acc = np.zeros((R, L, BODY_ACC_WIDTH))
    for r in range(R):
        s, e, o = int(st[r]), int(ends[r]), int(off[r])
        a, b = max(s + skip, s + o + hi), min(e, e + o + lo)                # the support: a pair at every lag, past the skipped frames
        if a >= b:
            continue
        for j in range(L):
            l = o + lo + j
            v, ok = _body_terms(None if from_truth else m[a:b], t[a - l:b - l], layout, from_truth)
            acc[r, j, :44] = np.ascontiguousarray(v[ok].T).sum(axis=1)       # along the contiguous axis: numpy's pairwise summation
            acc[r, j, 44], acc[r, j, 45] = ok.sum(), (~ok).sum()
    return acc


def body_sums(layout: int, msg, truth, lags=(0, 0), truth_kind: str = "est", starts=None, skip: int = 0, rec_lags=None,
              rotations: str = "estimate"):
    """The sums each recording's body is read off, for the sweep of lags ``lags=(lo, hi)`` in one pass (``ape_body_sums``).  ``msg``,
    ``truth``, ``starts``, ``skip``, ``rec_lags``, the pairing and the support: ``score_lags``'s.  ``truth_kind``: ``"est"`` rows for
    every layout; ``"targets"`` only for the layout whose targets carry positions (the two others' positions would be made with the
    body being fitted).  ``rotations="estimate"``: the matrices are those of the message's quaternions -- the body that makes THIS
    estimator's positions fit; ``"truth"``: those of the paired truth row -- the wearer's skeleton from mocap alone; ``msg`` may then be
    None and the sweep must be ``(0, 0)`` without ``rec_lags``.  Returns float64 ``[R, L, 46]`` on the device (``best_body``;
    include/ape_hip.h states the columns).  The call does not wait for the device."""
    rot = _rotations(rotations)
    if truth_kind not in TRUTH_KINDS:
        raise UserWarning(f"truth_kind must be one of {sorted(TRUTH_KINDS)}, got {truth_kind!r}")
    if layout not in _hip.EST_WIDTH:
        raise UserWarning(f"layout {layout} has no pose to fit")
    tw = (_hip.NUM_TARGETS if truth_kind == "targets" else _hip.EST_WIDTH)[layout]
    if not isinstance(truth, torch.Tensor) or not truth.is_cuda or truth.dtype not in (torch.float32, torch.float64) or truth.dim() != 2 \
            or truth.shape[1] != tw:
        raise UserWarning(f"truth: a float32 or float64 device tensor [F, {tw}]")
    td, dev = truth.contiguous(), truth.device
    F = int(td.shape[0])
    md, ms = (None, 25)
    if msg is not None:
        md, ms = _rows_view(msg, 25, "msg")
        if md.shape[0] != F or md.device != dev:
            raise UserWarning(f"msg: expected {F} rows on {dev}, got {int(md.shape[0])} on {md.device}")
    elif rot == _hip.BODY_ROT_MSG:
        raise UserWarning("msg: a device tensor [F, >= 25] (None only with rotations='truth')")
    st = np.ascontiguousarray(np.asarray([0] if starts is None else starts, dtype=np.int32).reshape(-1))
    R = int(st.shape[0])
    lo, hi, off = _sweep(lags, R, rec_lags)
    L = hi - lo + 1
    if not 1 <= L <= _hip.SCORE_MAX_LAGS:
        raise UserWarning(f"lags=({lo}, {hi}): between 1 and {_hip.SCORE_MAX_LAGS} lags")
    with torch.cuda.device(dev):
        acc = torch.empty((max(R, 1), L, BODY_ACC_WIDTH), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_body_sums(int(layout), C.c_void_p(md.data_ptr()) if md is not None else None, ms,
                                            _f64(md.dtype) if md is not None else _hip.F64, C.c_void_p(td.data_ptr()),
                                            TRUTH_KINDS[truth_kind], _f64(td.dtype), F, C.c_void_p(st.ctypes.data), R, int(skip), rot, lo, hi,
                                            C.c_void_p(off.ctypes.data) if rec_lags is not None else None, C.c_void_p(acc.data_ptr()),
                                            stream), "ape_body_sums")
    return acc


def _prior_rows(prior, R: int) -> np.ndarray:
    """float64 ``[R, 9]`` of ``best_body``'s ``prior``"""
    p = _body_rows(prior, R, "best_body prior")
    if not np.isfinite(p).all():
        raise UserWarning("prior: a non-finite value")
    return np.ascontiguousarray(np.broadcast_to(p, (R, 9)))


def _body_systems(rows):
    """of the 46-value records ``[L, 46]`` of one recording: the unweighted normal matrices ``[L, 9, 9]`` and right sides ``[L, 9]`` of
    the hand and of the elbow ``(N_h, b_h, N_e, b_e)`` in the unknowns ``x = [larm_vec, uarm_vec, uarm_orig]``"""
    L = rows.shape[0]
    A, B, Cm = (rows[:, 9 * k:9 * k + 9].reshape(L, 3, 3) for k in range(3))
    I = rows[:, 44, None, None] * np.eye(3)
    Nh, Ne = np.zeros((L, 9, 9)), np.zeros((L, 9, 9))
    Nh[:, 0:3, 0:3] = Nh[:, 3:6, 3:6] = Nh[:, 6:9, 6:9] = Ne[:, 3:6, 3:6] = Ne[:, 6:9, 6:9] = I
    Nh[:, 0:3, 3:6], Nh[:, 0:3, 6:9], Nh[:, 3:6, 6:9], Ne[:, 3:6, 6:9] = A, B, Cm, Cm
    At, Bt, Ct = (np.transpose(m, (0, 2, 1)) for m in (A, B, Cm))
    Nh[:, 3:6, 0:3], Nh[:, 6:9, 0:3], Nh[:, 6:9, 3:6], Ne[:, 6:9, 3:6] = At, Bt, Ct, Ct
    bh = rows[:, 27:36].copy()
    be = np.concatenate([np.zeros((L, 3)), rows[:, 36:42]], axis=1)
    return Nh, bh, Ne, be


def _joint_squares(tt, N, b, x):
    """``sum |t - prediction|^2 = sum |t|^2 - 2 x'b + x'N x`` per lag, clamped at 0; ``x [L, 9]``"""
    return np.maximum(tt - 2.0 * np.einsum("lk,lk->l", x, b) + np.einsum("lj,ljk,lk->l", x, N, x), 0.0)


def best_body(acc, lags, mode: str = "vectors", weights=(1, 1), prior=None, ridge: float = 0.0, max_cond: float = 1e8, rec_lags=None) -> list:
    """Each recording's lag and least-squares body, read off the accumulators ``acc [R, L, 46]`` of a ``body_sums`` sweep
    ``lags=(lo, hi)`` (with the ``rec_lags`` the sweep was made with).  ``weights = (w_hand, w_elbow)``: of the hand's and the elbow's
    squared residuals.  In the unknowns ``x = [larm_vec, uarm_vec, uarm_orig]`` and with ``n`` pairs, ``A, B, C`` the three product
    blocks per pair, the normal matrix is ``n [[w_h I, w_h A, w_h B], [., (w_h + w_e) I, (w_h + w_e) C], [., ., (w_h + w_e) I]]``, the
    right side ``[w_h R_l't_h, w_h R_u't_h + w_e R_u't_e, w_h R_h't_h + w_e R_h't_e]`` summed.  With ``w_hand = 0`` the forearm is not
    observable: ``larm_vec`` stays the prior's and the other six values are fitted.
    ``mode="vectors"``  all nine values (six with ``w_hand = 0``)
    ``mode="lengths"``  three scales ``s`` of the prior body's three vectors, ``x = D s`` with ``D [9, 3]`` holding the prior's vectors:
                        normal ``D'N D``, right side ``D'b`` (two scales with ``w_hand = 0``) -- for a recording whose motion does not
                        separate the nine values (an upper arm that is rigid against the hips)
    ``prior``: float64 ``[9]`` / ``[R, 9]`` values or bonemap-like objects as ``score_rows`` takes ``bodies`` (default: the default
    bonemap).  ``ridge >= 0`` adds ``ridge n I`` to the system solved, towards the prior (its values, or scales of 1).
    Per recording a dict: ``lag`` the lag with the smallest weighted mean squared residual after the fit (ties: the smaller ``|l|``,
    then the smaller ``l``), ``body [9]``, ``larm_length`` / ``uarm_length`` (the norms of its two vectors), ``hand_rms_before`` /
    ``hand_rms_after`` / ``elbow_rms_before`` / ``elbow_rms_after`` from the sums as ``sqrt(max(0, sum |t|^2 - 2 x'b + x'N x) / n)`` per
    joint ("before": under the prior), ``pairs`` summed at ``lag``, ``cond`` the condition number of the system solved at ``lag``,
    ``residual [L]`` the weighted mean squared residual after the fit per lag (NaN where a lag has no usable fit), ``ok``.
    A lag is usable where it has at least as many pairs as unknowns, a condition number of at most ``max_cond`` and a finite solution.
    A recording without a usable lag: ``ok`` False, ``body`` the prior, and ``lag`` the lag with the smallest residual under the prior
    -- None, with ``pairs`` 0 and NaN values, where no lag has a pair."""
    if mode not in ("vectors", "lengths"):
        raise UserWarning(f"mode must be 'vectors' or 'lengths', got {mode!r}")
    a = acc.detach().cpu().numpy() if isinstance(acc, torch.Tensor) else np.asarray(acc)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 3 or a.shape[-1] != BODY_ACC_WIDTH:
        raise UserWarning(f"expected accumulators [R,L,{BODY_ACC_WIDTH}], got {tuple(a.shape)}")
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != 2 or not np.isfinite(w).all() or (w < 0.0).any() or not (w > 0.0).any():
        raise UserWarning("weights: two finite values >= 0 (hand, elbow), not both zero")
    if not (np.isfinite(ridge) and ridge >= 0.0) or not max_cond > 0.0:
        raise UserWarning("ridge: a finite value >= 0; max_cond: above 0")
    R, L = a.shape[0], a.shape[1]
    lo, hi, off = _sweep(lags, R, rec_lags)
    if hi - lo + 1 != L:
        raise UserWarning(f"best_body: lags=({lo}, {hi}) for accumulators of {L} lags")
    priors = _prior_rows(prior, R)
    wh, we = float(w[0]), float(w[1])
    res = []
    for r in range(R):
        x0 = priors[r]
        ls = int(off[r]) + lo + np.arange(L)
        if mode == "vectors":
            D, u0 = np.eye(9), x0                                            # x = D u, the unknowns u start at the prior's values
        else:
            D, u0 = np.zeros((9, 3)), np.ones(3)
            for k in range(3):
                D[3 * k:3 * k + 3, k] = x0[3 * k:3 * k + 3]
        free = np.arange(D.shape[1]) if wh > 0.0 else np.arange(D.shape[1])[3 if mode == "vectors" else 1:]
        Df, k = D[:, free], free.shape[0]
        fixed = x0 - Df @ u0[free]                                           # what is not fitted stays the prior's
        n = a[r, :, 44]
        Nh, bh, Ne, be = _body_systems(a[r])
        N, b = wh * Nh + we * Ne, wh * bh + we * be
        with np.errstate(all="ignore"):
            safe = np.where(n > 0, n, 1.0)
            prior_rows = np.broadcast_to(x0, (L, 9))
            h0, e0 = _joint_squares(a[r, :, 42], Nh, bh, prior_rows), _joint_squares(a[r, :, 43], Ne, be, prior_rows)
            resid0 = np.where(n > 0, (wh * h0 + we * e0) / safe, np.nan)
            M = np.einsum("ia,lij,jb->lab", Df, N, Df) + ridge * n[:, None, None] * np.eye(k)
            rhs = np.einsum("ia,li->la", Df, b - np.einsum("lij,j->li", N, fixed)) + ridge * n[:, None] * u0[free]
            enough = (n > 0) & (n >= k)
            finite = np.isfinite(M).all(axis=(1, 2))
            cond = np.full(L, np.nan)
            cond[enough & ~finite] = np.inf
            if (enough & finite).any():
                cond[enough & finite] = np.linalg.cond(M[enough & finite])
            good = enough & (cond <= max_cond)
            X = np.full((L, 9), np.nan)
            if good.any():
                try:
                    X[good] = fixed + np.linalg.solve(M[good], rhs[good][:, :, None])[:, :, 0] @ Df.T
                except np.linalg.LinAlgError:
                    pass
            usable = good & np.isfinite(X).all(axis=1)
            Xs = np.where(usable[:, None], X, prior_rows)
            h1, e1 = _joint_squares(a[r, :, 42], Nh, bh, Xs), _joint_squares(a[r, :, 43], Ne, be, Xs)
            resid = np.where(usable, (wh * h1 + we * e1) / safe, np.nan)
        ok = bool(usable.any())
        pick = resid if ok else resid0
        cand = [j for j in range(L) if np.isfinite(pick[j])]
        if not cand:
            nan = float("nan")
            res.append({"lag": None, "body": x0.copy(), "larm_length": float(np.linalg.norm(x0[0:3])), "uarm_length": float(np.linalg.norm(x0[3:6])),
                        "hand_rms_before": nan, "hand_rms_after": nan, "elbow_rms_before": nan, "elbow_rms_after": nan, "pairs": 0,
                        "cond": nan, "residual": resid, "ok": False})
            continue
        j = min(cand, key=lambda i: (pick[i], abs(int(ls[i])), int(ls[i])))
        x = Xs[j].copy()
        rms = lambda sq: float(np.sqrt(sq[j] / n[j]))                                                         # noqa: E731
        res.append({"lag": int(ls[j]), "body": x, "larm_length": float(np.linalg.norm(x[0:3])), "uarm_length": float(np.linalg.norm(x[3:6])),
                    "hand_rms_before": rms(h0), "hand_rms_after": rms(h1), "elbow_rms_before": rms(e0), "elbow_rms_after": rms(e1),
                    "pairs": int(n[j]), "cond": float(cond[j]), "residual": resid, "ok": ok})
    return res


def bodies_of(found) -> np.ndarray:
    """float64 ``[R, 9]`` of ``best_body``'s list, ready for ``set_bodies``, ``process_recording(bonemaps=)`` and ``repost(bonemaps=)``"""
    return np.ascontiguousarray(np.stack([np.asarray(b["body"], dtype=np.float64).reshape(9) for b in found]))


def _qrot(q, v):
    """``q (0, v) q*``, the two products of csrc/fk_device.h's qrot in their order; ``q [n, 4]``, ``v [n, 3]`` -> ``[n, 3]``"""
    t = _qmul(q, np.concatenate([np.zeros((v.shape[0], 1)), v], axis=1))
    return _qmul(t, q * np.array([1.0, -1.0, -1.0, -1.0]))[:, 1:]


def _bodies(bodies, R: int, what: str) -> np.ndarray:
    """float64 ``[1 | R, 9]`` of one body or one per recording"""
    b = np.asarray(bodies, dtype=np.float64)
    b = b.reshape(1, 9) if b.size == 9 else b
    if b.ndim != 2 or b.shape[1] != 9 or b.shape[0] not in (1, R):
        raise UserWarning(f"{what}: one body [9] or one per recording [{R}, 9], got {tuple(b.shape)}")
    return np.ascontiguousarray(b)


def rebody_rows_numpy(msg, bodies, layout: int, starts=None) -> np.ndarray:
    """The host statement of ``rebody_rows``: float64 ``[F, 25]``.  With the recording's body ``larm_vec, uarm_vec, uarm_orig``: the four
    quaternions as they are, ``[18:21] = q_hips (x) uarm_orig`` (without hips: ``uarm_orig`` itself), ``[11:14] = q_uarm (x) uarm_vec +
    [18:21]``, ``[4:7] = q_larm (x) larm_vec + [11:14]``."""
    if layout not in (_hip.LAYOUT_ORI_CAL_LARM_UARM_HIPS, _hip.LAYOUT_ORI_CAL_LARM_UARM):
        raise UserWarning(f"layout {layout}: its positions are not made from a body")
    m = np.asarray(msg, dtype=np.float64)[:, :25]
    st = np.asarray([0] if starts is None else starts, dtype=np.int64).reshape(-1)
    F, R = m.shape[0], st.shape[0]
    b = _bodies(bodies, R, "bodies")
    rec = np.searchsorted(st, np.arange(F), side="right") - 1 if b.shape[0] > 1 else np.zeros(F, dtype=np.int64)
    b = b[rec]
    out = m.copy()
    with np.errstate(all="ignore"):
        out[:, 18:21] = _qrot(m[:, 21:25], b[:, 6:9]) if layout == _hip.LAYOUT_ORI_CAL_LARM_UARM_HIPS else b[:, 6:9]
        out[:, 11:14] = _qrot(m[:, 14:18], b[:, 3:6]) + out[:, 18:21]
        out[:, 4:7] = _qrot(m[:, 7:11], b[:, 0:3]) + out[:, 11:14]
    return out


def rebody_rows(layout: int, msg, bodies, starts=None, out_dtype=None):
    """Replay rows with their positions made again under a body per recording (``ape_rebody_rows``): ``msg`` device ``[F, >= 25]``
    (nothing past column 24 is read), ``bodies`` float64 ``[9]`` or ``[R, 9]`` (``bodies_of(best_body(...))``), ``starts`` the
    recordings' first frames.  Returns ``out [F, 25]`` of ``out_dtype`` (default: ``msg``'s): the quaternions copied, the shoulder, elbow
    and hand origins from them and the body.  The layout whose positions are predicted is refused.  A spread record is not rewritten:
    its covariances cannot be made again from 21 values.  The call does not wait for the device."""
    if layout not in _hip.EST_WIDTH:
        raise UserWarning(f"layout {layout} has no pose to rebuild")
    md, ms = _rows_view(msg, 25, "msg")
    out_dtype = md.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
    F, dev = int(md.shape[0]), md.device
    st = np.ascontiguousarray(np.asarray([0] if starts is None else starts, dtype=np.int32).reshape(-1))
    R = int(st.shape[0])
    body = _bodies(bodies, R, "bodies")
    with torch.cuda.device(dev):
        out = torch.empty((F, 25), dtype=out_dtype, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_rebody_rows(int(layout), C.c_void_p(md.data_ptr()), ms, _f64(md.dtype), F, C.c_void_p(st.ctypes.data), R,
                                              C.c_void_p(body.ctypes.data), int(body.shape[0]), C.c_void_p(out.data_ptr()), _f64(out_dtype),
                                              stream), "ape_rebody_rows")
    return out


def align_body(layout: int, msg, truth, lags=(0, 0), mode: str = "vectors", weights=(1, 1), truth_kind: str = "est", spread=None, starts=None,
               skip: int = 0, rec_lags=None, quats=None, prior=None):
    """Find each recording's lag and body together and score with both removed: ``rotate_rows`` by ``quats`` where given
    (``best_frame``'s, ``[4]`` or ``[R, 4]``: the heading is taken out first), a ``body_sums`` sweep with the message's rotations,
    ``best_body`` on it (this waits for the device), ``rebody_rows`` under the bodies found (the prior where a recording has no usable
    fit), then ``score_lags`` of the rewritten rows with ``lags=(0, 0)`` and the lags found as offsets (a recording's own ``rec_lags``
    entry, or 0, where it has no pair).  Returns ``(score [F, 7], acc [R, 25], found)``, ``found`` being ``best_body``'s list
    (``bodies_of(found)`` for ``set_bodies`` and ``process_recording(bonemaps=)``).  The spread record (``spread``) passes through
    unchanged but for the turn by ``quats``: the Mahalanobis columns then describe the OLD body's cloud around positions made with the
    new one.  ``truth``: est rows; the layout whose positions are predicted cannot be rewritten and is refused."""
    rec = spread
    if quats is not None:
        turned = rotate_rows(layout, msg, quats, spread, starts)
        msg, rec = turned if spread is not None else (turned, None)
    sums = body_sums(layout, msg, truth, lags, truth_kind, starts, skip, rec_lags, "estimate")
    found = best_body(sums, lags, mode, weights, prior, rec_lags=rec_lags)
    bodies = bodies_of(found)
    base = np.zeros(len(found), dtype=np.int64) if rec_lags is None else np.asarray(rec_lags, dtype=np.int64).reshape(-1)
    at = [int(base[r]) if b["lag"] is None else b["lag"] for r, b in enumerate(found)]
    out = rebody_rows(layout, msg, bodies, starts)
    if rec is not None and rec.dtype != out.dtype:
        rec = rec.to(out.dtype)
    score, acc = score_lags(layout, out, truth, (0, 0), truth_kind, rec, starts, skip, bodies, at, per_frame=True)
    return score[:, 0], acc[:, 0], found


# ---- how smooth a replay is: speed, acceleration and jerk of every frame (ape_motion_sums) ----------------------------------
# A longer ``smooth`` makes the arm stop shaking and costs lag: ``score_lags`` measures the lag, ``motion_sums`` what it buys -- the jerk
# of the joint positions, the literature's jitter -- from the rows alone, on the frames' own clock and never across a recording boundary.
# It needs no truth: ``truth_motion`` of an estimator is the floor the truth itself sets.
MOTION_WIDTH = _hip.MOTION_WIDTH
MOTION_ACC_WIDTH = _hip.MOTION_ACC_WIDTH
ROWS_KINDS = {"msg": _hip.ROWS_MSG, "est": _hip.ROWS_EST, "targets": _hip.ROWS_TARGETS}
MOTION_NAMES = ("hand_speed", "hand_acc", "hand_jerk", "elbow_speed", "elbow_acc", "elbow_jerk",
                "larm_ang_speed", "uarm_ang_speed", "hips_ang_speed", "larm_ang_acc", "uarm_ang_acc", "hips_ang_acc")
_MOTION_MAX_COLS = tuple(range(2, 3 * MOTION_WIDTH, 3))


def _rows_width(layout: int, kind: str) -> int:
    if kind not in ROWS_KINDS:
        raise UserWarning(f"kind must be one of {sorted(ROWS_KINDS)}, got {kind!r}")
    if layout not in _hip.EST_WIDTH:
        raise UserWarning(f"layout {layout} has no pose to difference")
    return 25 if kind == "msg" else (_hip.NUM_TARGETS if kind == "targets" else _hip.EST_WIDTH)[layout]


def _norm3(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def _six_drr_quat(s):
    """truth_six_drr_to_quat of csrc/score_device.h operation for operation: ``s [n, 6]`` -> unit quaternions ``[n, 4]`` with
    ``w >= 0`` -- Gram-Schmidt, the closed form of fk_device.h's six_drr_to_quat with its four pivots, two power steps on ``K + I``"""
    a1x, a1y, a1z, a2x, a2y, a2z = s[:, 0], s[:, 2], s[:, 4], s[:, 1], s[:, 3], s[:, 5]
    n1 = np.sqrt((a1x * a1x + a1y * a1y) + a1z * a1z)
    m00, m10, m20 = a1x / n1, a1y / n1, a1z / n1
    d = (m00 * a2x + m10 * a2y) + m20 * a2z
    ux, uy, uz = a2x - d * m00, a2y - d * m10, a2z - d * m20
    n2 = np.sqrt((ux * ux + uy * uy) + uz * uz)
    m01, m11, m21 = ux / n2, uy / n2, uz / n2
    m02, m12, m22 = m10 * m21 - m20 * m11, m20 * m01 - m00 * m21, m00 * m11 - m10 * m01
    tr = (m00 + m11) + m22
    s0, s1 = 2.0 * np.sqrt(tr + 1.0), 2.0 * np.sqrt(((1.0 + m00) - m11) - m22)
    s2, s3 = 2.0 * np.sqrt(((1.0 + m11) - m00) - m22), 2.0 * np.sqrt(((1.0 + m22) - m00) - m11)
    forms = [np.stack([0.25 * s0, (m21 - m12) / s0, (m02 - m20) / s0, (m10 - m01) / s0], axis=1),
             np.stack([(m21 - m12) / s1, 0.25 * s1, (m01 + m10) / s1, (m02 + m20) / s1], axis=1),
             np.stack([(m02 - m20) / s2, (m01 + m10) / s2, 0.25 * s2, (m12 + m21) / s2], axis=1),
             np.stack([(m10 - m01) / s3, (m02 + m20) / s3, (m12 + m21) / s3, 0.25 * s3], axis=1)]
    c0 = ~(tr < m00) & ~(tr < m11) & ~(tr < m22)           # the trace is the pivot (also the NaN path)
    c1 = ~c0 & (m00 >= m11) & (m00 >= m22)
    c2 = ~c0 & ~c1 & (m11 >= m22)
    q = np.where(c0[:, None], forms[0], np.where(c1[:, None], forms[1], np.where(c2[:, None], forms[2], forms[3])))
    q = np.where((q[:, 0] < 0.0)[:, None], -q, q)
    k00, k11, k22, k33 = ((m00 - m11) - m22) + 1.0, ((m11 - m00) - m22) + 1.0, ((m22 - m00) - m11) + 1.0, ((m00 + m11) + m22) + 1.0
    k01, k02, k12, k03, k13, k23 = m01 + m10, m02 + m20, m12 + m21, m21 - m12, m02 - m20, m10 - m01
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    for _ in range(2):
        nx, ny = ((k00 * x + k01 * y) + k02 * z) + k03 * w, ((k01 * x + k11 * y) + k12 * z) + k13 * w
        nz, nw = ((k02 * x + k12 * y) + k22 * z) + k23 * w, ((k03 * x + k13 * y) + k23 * z) + k33 * w
        nn = np.sqrt(((nx * nx + ny * ny) + nz * nz) + nw * nw)
        x, y, z, w = nx / nn, ny / nn, nz / nn, nw / nn
    q = np.stack([w, x, y, z], axis=1)
    return np.where((w < 0.0)[:, None], -q, q)


def _hips_quat(sn, cs):
    """hips_quat of csrc/fk_device.h: ``(cos(a / 2), 0, sin(a / 2), 0)`` of ``a = atan2(sn, cs)`` by angle_device.h's half-angle identities
    (the routine's own route outside the band 1e-140 <= r <= 1e140)"""
    r = np.sqrt(cs * cs + sn * sn)
    plain = (r >= 1e-140) & (r <= 1e140)
    rr = np.where(plain, r, 1.0)
    c, sa = cs / rr, np.abs(sn) / rr
    big = np.sqrt(0.5 * (1.0 + np.abs(c)))
    small = sa / (2.0 * big)
    hc, hs = np.where(c >= 0.0, big, small), np.copysign(np.where(c >= 0.0, small, big), sn)
    h = 0.5 * np.arctan2(sn, cs)
    hc, hs = np.where(plain, hc, np.cos(h)), np.where(plain, hs, np.sin(h))
    zero = np.zeros_like(hc)
    return np.stack([hc, zero, hs, zero], axis=1)


def _pose_rows(rows, layout: int, kind: str, body):
    """``(pose [F, 18], usable [F])`` of rows of a kind: hand, elbow, lower-arm, upper-arm and hips quaternion (the identity without
    hips), by the operations of csrc/score_device.h's truth_pose (targets: targets_to_pose with the frames' bodies ``body [F, 9]``);
    usable: every value the pose is made of is finite"""
    n = rows.shape[0]
    hips = layout != _hip.LAYOUT_ORI_CAL_LARM_UARM
    ident = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    ok = np.ones(n, dtype=bool)
    if kind == "msg":
        hand, elbow, lq, uq, hq = rows[:, 4:7], rows[:, 11:14], rows[:, 7:11], rows[:, 14:18], rows[:, 21:25] if hips else ident
    elif kind == "est":
        ql, qu = (9, 13) if hips else (6, 10)
        hand, elbow, lq, uq, hq = rows[:, 0:3], rows[:, 3:6], rows[:, ql:ql + 4], rows[:, qu:qu + 4], rows[:, 17:21] if hips else ident
    else:
        ok = np.isfinite(rows).all(axis=1)
        larm_vec, uarm_vec, uarm_orig = body[:, 0:3], body[:, 3:6], body[:, 6:9]
        if layout == _hip.LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS:
            lq, uq, hq = _six_drr_quat(rows[:, 3:9]), _six_drr_quat(rows[:, 12:18]), _hips_quat(rows[:, 18], rows[:, 19])
            hand, elbow = rows[:, 0:3], rows[:, 9:12]
        else:
            lq, uq = _six_drr_quat(rows[:, 0:6]), _six_drr_quat(rows[:, 6:12])
            hq = _hips_quat(rows[:, 12], rows[:, 13]) if hips else ident
            uo = _qrot(hq, uarm_orig) if hips else uarm_orig
            elbow = _qrot(uq, uarm_vec) + uo
            hand = _qrot(lq, larm_vec) + elbow
    pose = np.concatenate([hand, elbow, lq, uq, hq], axis=1)
    return pose, ok & np.isfinite(pose).all(axis=1)


def _unit4(q):
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    return q / n[:, None]


def _ang_vel(a, b, h):
    """the world-frame angular velocity over the step ``h`` from unit quaternions ``b`` to ``a``: ``d = a (x) conj(b)``, negated where
    ``d.w < 0.0``, ``v`` its vector part, ``n = |v|``: ``(s v) / h`` with ``s = (2 atan2(n, d.w)) / n`` for ``n >= 1e-8``, else 2"""
    d = _qmul(a, b * np.array([1.0, -1.0, -1.0, -1.0]))
    d = np.where((d[:, 0] < 0.0)[:, None], -d, d)
    n = _norm3(d[:, 1:])
    big = n >= 1e-8
    s = np.where(big, (2.0 * np.arctan2(n, d[:, 0])) / np.where(big, n, 1.0), 2.0)
    return (s[:, None] * d[:, 1:]) / h[:, None]


def motion_sums_numpy(rows, layout: int, kind: str = "msg", starts=None, skip: int = 0, times=None, bodies=None):
    """The host statement of ``motion_sums`` for one set of rows: ``(motion [F, 12], acc [R, 38])`` float64, plain numpy with the
    operations of include/ape_hip.h in their order.  ``rows [F, >= w]`` of ``kind`` ``"msg"`` (w = 25), ``"est"`` (21 | 14) or
    ``"targets"`` (O; through the numpy statement of the device's truth FK with ``bodies``); float32 rows are widened exactly.
    ``times`` float64 ``[F]`` or None (the index clock).  A frame holds its 12 values iff it lies at least three frames into its
    recording, the poses of ``f-3 .. f`` are finite, the three steps are finite and positive and all 12 results are finite; else NaN.
    ``acc``: sum, sum of squares and maximum of every value over the frames with ``f - s_r >= skip + 3``, then the frames summed and
    the frames left out (numpy's summation order, so sums agree with the device to rounding)."""
    w = _rows_width(layout, kind)
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] < w:
        raise UserWarning(f"rows: expected [F, >= {w}], got {tuple(rows.shape)}")
    rows = rows[:, :w].astype(np.float64)
    F = rows.shape[0]
    st = _recording_starts(starts).astype(np.int64)
    R = st.shape[0]
    hips = layout != _hip.LAYOUT_ORI_CAL_LARM_UARM
    rec = np.searchsorted(st, np.arange(F), side="right") - 1
    idx = np.arange(F) - st[rec]
    t = idx.astype(np.float64) if times is None else np.asarray(times, dtype=np.float64).reshape(-1)
    if t.shape[0] != F:
        raise UserWarning(f"times: {t.shape[0]} stamps for {F} frames")
    body = None
    if kind == "targets":
        b = _body_rows(bodies, R, "motion_sums bodies")
        body = b[rec] if b.shape[0] > 1 else np.broadcast_to(b, (F, 9))
    motion = np.full((F, MOTION_WIDTH), np.nan)
    with np.errstate(all="ignore"):
        pose, ok = _pose_rows(rows, layout, kind, body)
        pose = np.concatenate([pose[:, 0:6], _unit4(pose[:, 6:10]), _unit4(pose[:, 10:14]), _unit4(pose[:, 14:18])], axis=1)
        if F > 3:
            t0, t1, t2, t3 = t[3:], t[2:-1], t[1:-2], t[:-3]
            h1, h2, h3 = t0 - t1, t1 - t2, t2 - t3
            s2a, s2b, s3 = t0 - t2, t1 - t3, t0 - t3
            val = np.zeros((F - 3, MOTION_WIDTH))
            for k, c in enumerate((0, 3)):
                p = pose[:, c:c + 3]
                a, b, e = (p[3:] - p[2:-1]) / h1[:, None], (p[2:-1] - p[1:-2]) / h2[:, None], (p[1:-2] - p[:-3]) / h3[:, None]
                a2, b2 = (a - b) / s2a[:, None], (b - e) / s2b[:, None]
                d3 = (a2 - b2) / s3[:, None]
                val[:, 3 * k], val[:, 3 * k + 1], val[:, 3 * k + 2] = _norm3(a), 2.0 * _norm3(a2), 6.0 * _norm3(d3)
            half = s2a / 2.0
            for j in range(3 if hips else 2):
                q = pose[:, 6 + 4 * j:10 + 4 * j]
                wa, wb = _ang_vel(q[3:], q[2:-1], h1), _ang_vel(q[2:-1], q[1:-2], h2)
                val[:, 6 + j], val[:, 9 + j] = _norm3(wa), _norm3(wa - wb) / half
            good = (idx[3:] >= 3) & ok[3:] & ok[2:-1] & ok[1:-2] & ok[:-3]
            for h in (h1, h2, h3):
                good &= np.isfinite(h) & (h > 0.0)
            good &= np.isfinite(val).all(axis=1)
            motion[3:][good] = val[good]
    acc = np.zeros((R, MOTION_ACC_WIDTH))
    ends = np.r_[st[1:], F]
    for r, (a, b) in enumerate(zip(st, ends)):
        seg = motion[min(a + int(skip) + 3, b):b]
        use = seg[np.isfinite(seg[:, 0])]
        if use.shape[0]:
            acc[r, 0:36:3], acc[r, 1:36:3], acc[r, 2:36:3] = use.sum(axis=0), (use * use).sum(axis=0), use.max(axis=0)
        acc[r, 36], acc[r, 37] = use.shape[0], seg.shape[0] - use.shape[0]
    return motion, acc


def _sets_view(t, width: int, what: str):
    """(tensor, row stride, set stride, C | None) of a device view ``[F, >= width]`` or ``[C, F, >= width]`` whose rows are contiguous
    and whose sets do not overlap; anything else is copied"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() not in (2, 3) or t.shape[-1] < width or t.shape[-2] < 1:
        raise UserWarning(f"{what}: expected a device tensor [F, >= {width}] or [C, F, >= {width}]")
    if t.dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"{what}: float32 or float64, got {t.dtype}")
    F = int(t.shape[-2])
    if t.dim() == 2:
        t, rs = _rows_view(t, width, what)
        return t, rs, 0, None
    n = int(t.shape[0])
    if not 1 <= n <= _hip.POST_MAX_CONFIGS:
        raise UserWarning(f"{what}: between 1 and {_hip.POST_MAX_CONFIGS} sets, got {n}")
    rs = max(int(t.stride(1)), width) if F > 1 else width
    if t.stride(2) != 1 or (F > 1 and t.stride(1) < width) or (n > 1 and t.stride(0) < F * rs):
        t = t[:, :, :width].contiguous()
        rs = width
    return t, rs, (int(t.stride(0)) if n > 1 else 0), n


def motion_sums(layout: int, rows, kind: str = "msg", starts=None, skip: int = 0, times=None, bodies=None, per_frame: bool = False,
                out_dtype=None):
    """Speed, acceleration and jerk of every frame and their sums per recording (``ape_motion_sums``).  ``rows``: device ``[F, >= w]``
    or ``[C, F, >= w]`` (C sets of the same recordings, at most 64: ``repost``'s ``out`` goes in as it is), float32 or float64, a
    strided view is taken without a copy; ``kind``: ``"msg"`` messages (w = 25), ``"est"`` est rows (21 | 14), ``"targets"``
    de-normalised NN targets (O), converted with ``bodies`` as ``score_rows`` converts truth.  ``starts``: the recordings' first
    frames; ``skip``: leading frames of every recording left out of the accumulators, on top of the three a third difference needs;
    ``times``: device float64 ``[F]`` (``frame_times``; None: the index clock, results per frame).  Returns ``(motion, acc)`` on the
    device: ``[F, 12]`` of ``out_dtype`` (default: the rows'; None unless ``per_frame``) in ``MOTION_NAMES``' order, NaN rows where a
    frame is not differenced, and float64 ``[R, 38]`` raw accumulators (``summarise_motion``, ``merge_motion``); both with a leading
    ``C`` for ``[C, F, w]`` rows.  The same inputs give the same bits.  The call does not wait for the device."""
    w = _rows_width(layout, kind)
    rd, rs, ss, n = _sets_view(rows, w, "rows")
    if rs > 2 ** 31 - 1:
        raise UserWarning(f"rows: a row stride of {rs} elements does not fit the entry's int32 (copy the view)")
    out_dtype = rd.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
    F, dev, sets = int(rd.shape[-2]), rd.device, 1 if n is None else n
    st = _recording_starts(starts)
    R = int(st.shape[0])
    body = _body_rows(bodies, R, "motion_sums bodies") if kind == "targets" else None
    tq = None if times is None else _clock(times, F, dev, "times")
    with torch.cuda.device(dev):
        motion = torch.empty((sets, F, MOTION_WIDTH), dtype=out_dtype, device=dev) if per_frame else None
        acc = torch.empty((sets, max(R, 1), MOTION_ACC_WIDTH), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_motion_sums(int(layout), C.c_void_p(rd.data_ptr()), ROWS_KINDS[kind], rs, _f64(rd.dtype), sets, ss, F,
                                              C.c_void_p(st.ctypes.data), R, int(skip), C.c_void_p(tq.data_ptr()) if tq is not None else None,
                                              C.c_void_p(body.ctypes.data) if body is not None else None,
                                              int(body.shape[0]) if body is not None else 0,
                                              C.c_void_p(motion.data_ptr()) if motion is not None else None, _f64(out_dtype),
                                              C.c_void_p(acc.data_ptr()), stream), "ape_motion_sums")
    if n is None:
        return (None if motion is None else motion[0]), acc[0]
    return motion, acc


def _motion_host(acc, ndims=(2,)) -> np.ndarray:
    a = acc.detach().cpu().numpy() if isinstance(acc, torch.Tensor) else np.asarray(acc)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim not in ndims or a.shape[-1] != MOTION_ACC_WIDTH:
        raise UserWarning(f"expected motion accumulators [..., R, {MOTION_ACC_WIDTH}] of {' or '.join(str(n) for n in ndims)} dimensions, "
                          f"got {tuple(a.shape)}")
    return a


def summarise_motion(acc) -> list:
    """``acc [R, 38]`` (of several sets: one set's slice ``acc[c]``) -> per recording a dict: ``scored`` and ``left_out`` frame counts
    and ``mean``, ``rms`` and ``max`` of the 12 values, dicts keyed by ``MOTION_NAMES`` (NaN where nothing was summed)."""
    res = []
    with np.errstate(all="ignore"):
        for row in _motion_host(acc):
            n = row[36]
            d = {"scored": int(n), "left_out": int(row[37]), "mean": {}, "rms": {}, "max": {}}
            for k, name in enumerate(MOTION_NAMES):
                d["mean"][name] = float(row[3 * k] / n) if n else float("nan")
                d["rms"][name] = float(np.sqrt(row[3 * k + 1] / n)) if n else float("nan")
                d["max"][name] = float(row[3 * k + 2]) if n else float("nan")
            res.append(d)
    return res


def merge_motion(acc_a, acc_b) -> np.ndarray:
    """the accumulators ``[R, 38]`` (or ``[C, R, 38]``) of two pieces of the same recordings as one: sums and counts added, the larger
    of the maxima.  Where the pieces are chained -- the second continues the first's recording -- the second piece's first three
    frames have no three frames below them in their own piece: the three frames at a joint are in neither piece's support, so the
    merged counts are three short of the whole recording's per joint."""
    a, b = _motion_host(acc_a, (2, 3)), _motion_host(acc_b, (2, 3))
    if a.shape != b.shape:
        raise UserWarning(f"merge_motion: {tuple(a.shape)} and {tuple(b.shape)} accumulators")
    out = a + b
    cols = list(_MOTION_MAX_COLS)
    out[..., cols] = np.maximum(a[..., cols], b[..., cols])
    return out


# ---- the shape of the errors: counts over fixed edges (ape_score_hist) --------------------------------------------------------
# A histogram [..., W, B + 3] holds, per column, the B bins (e[b], e[b + 1]], then the slots below (v <= e[0]), above (v > e[B]) and NaN.
HIST_MAX_BINS, HIST_MAX_WIDTH = _hip.HIST_MAX_BINS, _hip.HIST_MAX_WIDTH
SCORE_HIST_NAMES = ERROR_NAMES + ("hand_d2", "elbow_d2")
# default_edges' ranges, first and last edge per column.  "score": positions in metres, angles in radians (4 asin reaches 2 pi).  "motion":
# speed, acceleration and jerk of a position in m / s^k, angular speed and acceleration in rad / s^k; on the index clock the same
# numbers are per frame, and the edges want scaling by the frame rate's powers.
_SCORE_RANGES = ((1e-4, 10.0), (1e-4, 10.0), (1e-5, 6.4), (1e-5, 6.4), (1e-5, 6.4))
_MOTION_RANGES = ((1e-4, 1e2), (1e-3, 1e4), (1e-2, 1e6)) * 2 + ((1e-4, 1e3),) * 3 + ((1e-3, 1e5),) * 3
_POSITION_MARKS = (0.05, 0.10)                          # the thresholds pose papers print: edges of the position columns, bit for bit


def chi2_3_cdf(x: float) -> float:
    """the CDF of chi^2 with 3 degrees of freedom in closed form: erf(sqrt(x / 2)) - sqrt(2 x / pi) exp(-x / 2)"""
    import math
    return math.erf(math.sqrt(x / 2.0)) - math.sqrt(2.0 * x / math.pi) * math.exp(-x / 2.0) if x > 0.0 else 0.0


def pit_edges(cells: int) -> np.ndarray:
    """``cells`` edges (``cells - 1`` bins): the chi^2(3) quantiles at the levels ``k / cells``, ``k = 0 .. cells - 1`` (the first is
    0), by bisection on ``chi2_3_cdf``; a level of 0.5 or 0.9 gives ``CHI2_3_Q50`` / ``CHI2_3_Q90`` themselves.  A ``d^2`` column counted
    over them is the probability integral transform of the spread record in ``cells`` cells of equal probability (``pit``)."""
    cells = int(cells)
    if not 2 <= cells <= HIST_MAX_BINS + 1:
        raise UserWarning(f"pit_edges: between 2 and {HIST_MAX_BINS + 1} cells, got {cells}")
    e = np.zeros(cells)
    for k in range(1, cells):
        level = k / cells
        if level == 0.5 or level == 0.9:
            e[k] = CHI2_3_Q50 if level == 0.5 else CHI2_3_Q90
            continue
        lo, hi = 0.0, 128.0
        while True:
            mid = 0.5 * (lo + hi)
            if mid <= lo or mid >= hi:
                break
            if chi2_3_cdf(mid) < level:
                lo = mid
            else:
                hi = mid
        e[k] = hi
    return e


def default_edges(kind: str, bins: int = 64) -> np.ndarray:
    """float64 ``[W, bins + 1]`` edges for ``kind`` ``"score"`` (``score_rows``' 7 columns) or ``"motion"`` (``motion_sums``' 12):
    geometric spacing per column in that column's unit -- positions 1e-4 .. 10 m, angles 1e-5 .. 6.4 rad, speeds 1e-4 .. 1e2 m/s,
    accelerations 1e-3 .. 1e4 m/s^2, jerks 1e-2 .. 1e6 m/s^3, angular speeds 1e-4 .. 1e3 rad/s, angular accelerations 1e-3 .. 1e5
    rad/s^2 (what lies outside is counted below and above).  The inner edge nearest to 0.05 and to 0.10 of the position columns is moved
    onto them, so that ``fraction_within`` answers 5 cm and 10 cm.  The two ``d^2`` columns of ``"score"`` get ``pit_edges(bins + 1)``."""
    bins = int(bins)
    if kind not in ("score", "motion"):
        raise UserWarning(f"default_edges: kind must be 'score' or 'motion', got {kind!r}")
    if not 8 <= bins <= HIST_MAX_BINS:
        raise UserWarning(f"default_edges: between 8 and {HIST_MAX_BINS} bins, got {bins}")
    ranges = _SCORE_RANGES if kind == "score" else _MOTION_RANGES
    rows = []
    for c, (a, b) in enumerate(ranges):
        e = np.exp(np.linspace(np.log(a), np.log(b), bins + 1))
        e[0], e[-1] = a, b
        if kind == "score" and c < 2:
            at = [1 + int(np.argmin(np.abs(np.log(e[1:-1]) - np.log(mark)))) for mark in _POSITION_MARKS]
            if len(set(at)) != len(at):
                raise UserWarning(f"default_edges: {bins} bins do not keep the marks {_POSITION_MARKS} apart")
            e[at] = _POSITION_MARKS
        rows.append(e)
    if kind == "score":
        rows += [pit_edges(bins + 1)] * 2
    out = np.ascontiguousarray(np.stack(rows))
    if not (np.diff(out, axis=1) > 0.0).all():
        raise UserWarning(f"default_edges: {bins} bins do not keep the marks apart")
    return out


def _edges(edges, W: int) -> np.ndarray:
    """float64 ``[W, B + 1]`` of ``[B + 1]`` (for all columns) or ``[W, B + 1]``"""
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim == 1:
        e = np.broadcast_to(e, (W, e.shape[0]))
    if e.ndim != 2 or e.shape[0] != W or e.shape[1] < 2:
        raise UserWarning(f"edges: expected [B+1] or [{W}, B+1] with B >= 1, got {tuple(np.shape(edges))}")
    return np.ascontiguousarray(e)


def _trims(R: int, skip: int, trim) -> np.ndarray:
    """int32 ``[R, 2]``: ``trim`` (None: zeros) with ``skip`` added at the head"""
    if int(skip) < 0:
        raise UserWarning(f"skip {skip} is negative")
    t = np.zeros((R, 2), dtype=np.int64) if trim is None else np.asarray(trim, dtype=np.int64).reshape(-1, 2).copy()
    if t.shape[0] != R:
        raise UserWarning(f"trim: {t.shape[0]} rows for {R} recordings")
    t[:, 0] += int(skip)
    if (t < 0).any() or (t > 2 ** 31 - 1).any():
        raise UserWarning("trim: between 0 and 2^31 - 1")
    return np.ascontiguousarray(t.astype(np.int32))


def lag_trim(starts, F: int, lags, skip: int = 0, rec_lags=None) -> np.ndarray:
    """int32 ``[R, 2]``: what to trim off the head and the tail of every recording so that its window is the common support of the
    sweep ``lags=(lo, hi)`` with offsets ``rec_lags`` (``score_lags``): ``max(skip, o_r + hi, 0)`` and ``max(0, -(o_r + lo))``.  With
    it the slots of ``hist_rows(score, ..., trim=)`` add up to ``acc[r, j, 15] + acc[r, j, 16]`` for every ``j``."""
    st = _recording_starts(starts)
    if st.shape[0] < 1 or int(F) < 1:
        raise UserWarning("lag_trim: at least one recording and one frame")
    lo, hi, off = _sweep(lags, int(st.shape[0]), rec_lags)
    o = off.astype(np.int64)
    out = np.stack([np.maximum(np.maximum(int(skip), o + hi), 0), np.maximum(0, -(o + lo))], axis=1)
    return np.ascontiguousarray(out.astype(np.int32))


def _slots(v, e) -> np.ndarray:
    """the slot of every value of ``v`` over the edges ``e [B + 1]``: searchsorted from the left counts the edges below ``v``"""
    B = e.shape[0] - 1
    i = np.searchsorted(e, v, side="left")
    return np.where(np.isnan(v), B + 2, np.where(i == 0, B, np.where(i > B, B + 1, i - 1)))


def hist_numpy(values, edges, starts=None, skip: int = 0, trim=None) -> np.ndarray:
    """The host statement of ``hist_rows``: ``np.searchsorted(e, v, side="left")`` and ``np.bincount`` per recording, group and column.
    ``values``: ``[F, W]``, ``[F, G, W]`` or ``[C, F, G, W]`` (float32 is widened); returns int64 ``[(C,) R, (G,) W, B + 3]``."""
    v = np.asarray(values)
    if v.ndim not in (2, 3, 4):
        raise UserWarning(f"values: expected [F, W], [F, G, W] or [C, F, G, W], got {tuple(v.shape)}")
    nd = v.ndim
    v = v.astype(np.float64)
    v = v[:, None, :] if nd == 2 else v
    v = v[None] if nd < 4 else v
    Cn, F, G, W = v.shape
    e = _edges(edges, W)
    B = e.shape[1] - 1
    st = _recording_starts(starts).astype(np.int64)
    R = st.shape[0]
    tr = _trims(R, skip, trim).astype(np.int64)
    ends = np.r_[st[1:], F]
    out = np.zeros((Cn, R, G, W, B + 3), dtype=np.int64)
    for r in range(R):
        a, b = int(st[r] + tr[r, 0]), int(ends[r] - tr[r, 1])
        if a >= b:
            continue
        for c in range(Cn):
            for g in range(G):
                for w in range(W):
                    out[c, r, g, w] = np.bincount(_slots(v[c, a:b, g, w], e[w]), minlength=B + 3)
    out = out[0] if nd < 4 else out
    return out[:, 0] if nd == 2 else out


def _hist_view(t):
    """(tensor, C, F, G, W, set / frame / group stride in elements) of a device view ``[F, W]``, ``[F, G, W]`` or ``[C, F, G, W]`` whose
    last dimension is contiguous and whose frames, groups and sets lie apart (``_rows_view``'s rules); anything else is copied"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() not in (2, 3, 4) or min(t.shape) < 1:
        raise UserWarning("values: expected a device tensor [F, W], [F, G, W] or [C, F, G, W]")
    if t.dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"values: float32 or float64, got {t.dtype}")
    v = t[:, None, :] if t.dim() == 2 else t
    v = v[None] if v.dim() == 3 else v
    Cn, F, G, W = (int(n) for n in v.shape)
    if not 1 <= W <= HIST_MAX_WIDTH:
        raise UserWarning(f"values: between 1 and {HIST_MAX_WIDTH} columns, got {W}")
    if not 1 <= G <= _hip.SCORE_MAX_LAGS or not 1 <= Cn <= _hip.POST_MAX_CONFIGS:
        raise UserWarning(f"values: at most {_hip.SCORE_MAX_LAGS} groups and {_hip.POST_MAX_CONFIGS} sets, got {G} and {Cn}")
    ss, fs, gs, ws = (int(s) for s in v.stride())
    fs = fs if F > 1 else max(fs, W)
    if (W > 1 and ws != 1) or fs < W or (G > 1 and gs < W) or (Cn > 1 and ss < F * fs):
        v = v.contiguous()
        ss, fs, gs, ws = (int(s) for s in v.stride())
        fs = max(fs, W)
    return v, Cn, F, G, W, (ss if Cn > 1 else 0), fs, (gs if G > 1 else 0)


def hist_rows(values, edges, starts=None, skip: int = 0, trim=None):
    """Counts of per-frame values over fixed edges, per recording and column, on the device (``ape_score_hist``).  ``values``: a device
    ``[F, W]``, ``[F, G, W]`` or ``[C, F, G, W]`` view, float32 or float64, ``W <= 16``, ``G <= 65``, ``C <= 64``: ``score_rows``'
    ``[F, 7]``, ``score_lags``' ``[F, L, 7]``, ``motion_sums``' ``[C, F, 12]`` (as ``values[:, :, None]``), column slices and strided
    views go in without a copy.  ``edges``: float64 ``[B + 1]`` for all columns or ``[W, B + 1]``, strictly increasing, ``B <= 256``
    (``default_edges``, ``pit_edges``).  ``starts``: the recordings' first frames; recording ``r``'s window is its frames less
    ``skip + trim[r, 0]`` at the head and ``trim[r, 1]`` at the tail (``trim``: ``[R, 2]``, ``lag_trim``).  Returns int64
    ``[(C,) R, (G,) W, B + 3]`` on the device: per column the ``B`` bins ``(e[b], e[b + 1]]``, then the counts below (``v <= e[0]``),
    above (``v > e[B]``) and NaN; every row sums to the window's length.  Integer counts: the same inputs give the same bits, and pieces
    add (``merge_hist``).  The call does not wait for the device."""
    nd = values.dim() if isinstance(values, torch.Tensor) else 0
    v, Cn, F, G, W, ss, fs, gs = _hist_view(values)
    e = _edges(edges, W)
    B = int(e.shape[1]) - 1
    if B > HIST_MAX_BINS:
        raise UserWarning(f"edges: at most {HIST_MAX_BINS} bins, got {B}")
    st = _recording_starts(starts)
    R = int(st.shape[0])
    tr = _trims(R, skip, trim)
    dev = v.device
    with torch.cuda.device(dev):
        hist = torch.empty((Cn, max(R, 1), G, W, B + 3), dtype=torch.int64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_score_hist(C.c_void_p(v.data_ptr()), _f64(v.dtype), W, Cn, ss, F, fs, G, gs, C.c_void_p(st.ctypes.data), R,
                                             C.c_void_p(tr.ctypes.data), C.c_void_p(e.ctypes.data), B, C.c_void_p(hist.data_ptr()), stream),
                   "ape_score_hist")
    hist = hist[0] if nd < 4 else hist
    return hist[:, 0] if nd == 2 else hist


def _hist_host(hist) -> np.ndarray:
    h = hist.detach().cpu().numpy() if isinstance(hist, torch.Tensor) else np.asarray(hist)
    if h.ndim < 1 or h.shape[-1] < 4 or not np.issubdtype(h.dtype, np.integer):
        raise UserWarning(f"expected an integer histogram [..., B + 3], got {h.dtype} {tuple(h.shape)}")
    return h.astype(np.int64)


def merge_hist(hist_a, hist_b) -> np.ndarray:
    """the histograms of two pieces of the same recordings over the same edges as one: the sum (int64, on the host)"""
    a, b = _hist_host(hist_a), _hist_host(hist_b)
    if a.shape != b.shape:
        raise UserWarning(f"merge_hist: {tuple(a.shape)} and {tuple(b.shape)} histograms")
    return a + b


def _hist_and_edges(hist, edges):
    """(h int64 [..., W, B + 3], e float64 [W, B + 1], the ordered counts below | bins | above [..., W, B + 2])"""
    h = _hist_host(hist)
    if h.ndim < 2:
        raise UserWarning(f"expected a histogram [..., W, B + 3], got {tuple(h.shape)}")
    e = _edges(edges, h.shape[-2])
    B = e.shape[1] - 1
    if h.shape[-1] != B + 3:
        raise UserWarning(f"a histogram of {h.shape[-1] - 3} bins against {B + 1} edges")
    return h, e, np.concatenate([h[..., B:B + 1], h[..., :B], h[..., B + 1:B + 2]], axis=-1)


def quantiles(hist, edges, q) -> dict:
    """Quantiles read off a histogram ``[..., W, B + 3]`` over ``edges`` (``[B + 1]`` or ``[W, B + 1]``).  ``q``: a level in [0, 1] or a
    sequence of them (the results then end in a dimension over them).  Over the ``n`` counted values that are not NaN, the value of
    rank ``max(1, ceil(q n))`` in ascending order -- ``np.quantile(..., method="inverted_cdf")`` -- lies in a known bin ``(lo, hi]``.
    Returns a dict of arrays ``[..., W(, Q)]``: ``lo`` and ``hi``, that bin's edges (the quantile of the values themselves lies between
    them, always); ``value``, the rank placed linearly within the bin (the ``j``-th of the bin's ``c`` values at ``(j - 0.5) / c`` of
    its width); ``clipped``: None, or ``"below"`` / ``"above"`` where the rank falls outside the edges, with ``e[0]`` / ``e[B]`` for all
    three; and ``n [..., W]``.  NaN where ``n == 0``."""
    h, e, ordered = _hist_and_edges(hist, edges)
    B = e.shape[1] - 1
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if qs.ndim != 1 or not ((qs >= 0.0) & (qs <= 1.0)).all():
        raise UserWarning("quantiles: levels in [0, 1]")
    n = ordered.sum(axis=-1)
    cum = np.cumsum(ordered, axis=-1)
    shape = n.shape + (qs.shape[0],)
    value, lo, hi = (np.full(shape, np.nan) for _ in range(3))
    clipped = np.full(shape, None, dtype=object)
    for idx in np.ndindex(*n.shape):
        if n[idx] == 0:
            continue
        ew = e[idx[-1]]
        for k, level in enumerate(qs):
            rank = max(1, int(np.ceil(level * n[idx])))
            pos = int(np.searchsorted(cum[idx], rank, side="left"))      # the first slot whose cumulative count reaches the rank
            if pos == 0 or pos == B + 1:
                value[idx + (k,)] = lo[idx + (k,)] = hi[idx + (k,)] = ew[0] if pos == 0 else ew[B]
                clipped[idx + (k,)] = "below" if pos == 0 else "above"
                continue
            a, b = ew[pos - 1], ew[pos]
            j, c = rank - (cum[idx][pos - 1]), ordered[idx][pos]
            lo[idx + (k,)], hi[idx + (k,)] = a, b
            value[idx + (k,)] = min(max(a + (b - a) * ((j - 0.5) / c), a), b)
    res = {"value": value, "lo": lo, "hi": hi, "clipped": clipped}
    if np.ndim(q) == 0:
        res = {k: v[..., 0] for k, v in res.items()}
    res["n"] = n
    return res


def fraction_within(hist, edges, thresholds) -> np.ndarray:
    """The share of the counted values that are not NaN with ``v <=`` each threshold: float64 ``[..., W, T]`` of a histogram
    ``[..., W, B + 3]``.  ``thresholds``: ``[T]`` for all columns or ``[W, T]``; each must be one of its column's edges bit for bit --
    a threshold between edges is refused, not interpolated (choose the edges to hold it).  NaN where nothing was counted."""
    h, e, ordered = _hist_and_edges(hist, edges)
    W, B = e.shape[0], e.shape[1] - 1
    t = np.asarray(thresholds, dtype=np.float64)
    t = np.broadcast_to(np.atleast_1d(t), (W, np.atleast_1d(t).shape[0])) if t.ndim < 2 else t
    if t.ndim != 2 or t.shape[0] != W:
        raise UserWarning(f"thresholds: expected [T] or [{W}, T], got {tuple(np.shape(thresholds))}")
    n = ordered.sum(axis=-1).astype(np.float64)
    cum = np.cumsum(ordered, axis=-1)                                    # cum[..., i]: values <= e[i], i = 0 .. B
    out = np.full(n.shape + (t.shape[1],), np.nan)
    ebits = np.ascontiguousarray(e).view(np.int64)
    for w in range(W):
        for k in range(t.shape[1]):
            hit = np.flatnonzero(ebits[w] == np.float64(t[w, k]).view(np.int64))
            if hit.shape[0] != 1:
                raise UserWarning(f"fraction_within: {t[w, k]!r} is not an edge of column {w} (no interpolation between edges)")
            with np.errstate(all="ignore"):
                out[..., w, k] = np.where(n[..., w] > 0, cum[..., w, int(hit[0])] / n[..., w], np.nan)
    return out


def pit(hist_column) -> dict:
    """The probability integral transform of a ``d^2`` column counted over ``pit_edges(cells)``: ``hist_column [..., cells + 2]`` (one
    column of a histogram) -> a dict: ``cells`` int64 ``[..., cells]``, the counts per cell of equal probability (below and the first
    bin, the inner bins, above); ``levels [cells - 1]`` = ``k / cells``; ``cumulative`` int64 ``[..., cells - 1]``, the values with
    ``d^2 <=`` the quantile of each level, and ``coverage``, their share of ``n`` (NaN where ``n == 0``): the reliability curve of which
    ``summarise``'s ``coverage50`` / ``coverage90`` are two points; ``n [...]`` values that are not NaN.  An honest spread record gives
    flat cells and ``coverage == levels``."""
    h = _hist_host(hist_column)
    B = h.shape[-1] - 3
    cells = np.concatenate([h[..., B:B + 1] + h[..., 0:1], h[..., 1:B], h[..., B + 1:B + 2]], axis=-1)
    n = cells.sum(axis=-1)
    cumulative = np.cumsum(cells, axis=-1)[..., :-1]
    with np.errstate(all="ignore"):
        coverage = np.where(n[..., None] > 0, cumulative / n[..., None].astype(np.float64), np.nan)
    return {"cells": cells, "levels": np.arange(1, B + 1) / (B + 1), "cumulative": cumulative, "coverage": coverage, "n": n}


def summarise_hist(hist, edges, names=None) -> list:
    """``hist [R, W, B + 3]`` (one set's, one group's slice) over ``edges`` -> per recording a dict: ``window``, the frames of the
    recording's window, and per column name ``nan`` (frames counted as NaN), ``median``, ``p90`` and ``p95`` (``quantiles``' ``value``;
    NaN where nothing was counted) with ``median_bin`` / ``p90_bin`` / ``p95_bin``, the ``(lo, hi)`` they lie between.  ``names``
    defaults to ``SCORE_HIST_NAMES`` for 7 columns and ``MOTION_NAMES`` for 12."""
    h, e, _ = _hist_and_edges(hist, edges)
    if h.ndim != 3:
        raise UserWarning(f"summarise_hist: expected [R, W, B + 3], got {tuple(h.shape)}")
    W = h.shape[1]
    if names is None:
        names = {len(SCORE_HIST_NAMES): SCORE_HIST_NAMES, len(MOTION_NAMES): MOTION_NAMES}.get(W)
    if names is None or len(names) != W:
        raise UserWarning(f"summarise_hist: {W} names for {W} columns")
    qt = quantiles(h, e, (0.5, 0.9, 0.95))
    res = []
    for r in range(h.shape[0]):
        d = {"window": int(h[r, 0].sum()), "nan": {}}
        for k, key in enumerate(("median", "p90", "p95")):
            d[key] = {name: float(qt["value"][r, w, k]) for w, name in enumerate(names)}
            d[key + "_bin"] = {name: (float(qt["lo"][r, w, k]), float(qt["hi"][r, w, k])) for w, name in enumerate(names)}
        for w, name in enumerate(names):
            d["nan"][name] = int(h[r, w, -1])
        res.append(d)
    return res


# ---- joint angles of every frame, and their errors against truth (ape_joint_angles) ----------------------------------------
# ``score_rows`` speaks in metres and whole-rotation angles; these state a pose as elbow flexion, forearm twist, shoulder elevation and its
# plane, humeral twist and hips yaw -- a swing-twist split of each joint about the bone's long axis (local -x), NaN where an angle is not
# conditioned (``min_swing``).
ANGLE_WIDTH = _hip.ANGLE_WIDTH
ANGLE_ACC_WIDTH = _hip.ANGLE_ACC_WIDTH
ANGLE_NAMES = ("elbow_flexion", "hinge_azimuth", "forearm_twist", "shoulder_elevation", "elevation_plane", "humeral_twist", "hips_yaw")
ANGLE_PERIODIC = (False, True, True, False, True, True, True)
_ANGLE_MIN_COLS = tuple(range(2, 5 * ANGLE_WIDTH, 5))
_ANGLE_MAX_COLS = tuple(range(3, 5 * ANGLE_WIDTH, 5)) + tuple(range(5 * ANGLE_WIDTH + 3, 10 * ANGLE_WIDTH, 5))


def _min_swing(min_swing) -> float:
    m = float(min_swing)
    if not 0.0 <= m < np.pi / 2.0:
        raise UserWarning(f"min_swing must lie in [0, pi / 2), got {min_swing!r}")
    return m


def _swing_twist(r):
    """``(rho, n, swing, twist, azimuth)`` of quaternions ``r [n, 4]``, negated first where ``w < 0.0``: ``r = swing (x) twist`` about x"""
    r = np.where((r[:, 0] < 0.0)[:, None], -r, r)
    w, x, y, z = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    rho, n = np.sqrt(w * w + x * x), np.sqrt(y * y + z * z)
    return rho, n, 2.0 * np.arctan2(n, rho), 2.0 * np.arctan2(x, w), np.arctan2(y * x + z * w, y * w - z * x)


def _row_angles(rows, layout: int, kind: str, body, min_swing: float) -> np.ndarray:
    """the seven angles ``[F, 7]`` of rows of a kind, by the operations of include/ape_hip.h in their order (csrc/joint_angles.hip:
    row_angles)"""
    sh, sf = math.sin(min_swing / 2.0), math.sin(min_swing)    # (the C library's, as the entry computes them)
    conj = np.array([1.0, -1.0, -1.0, -1.0])
    with np.errstate(all="ignore"):
        pose, ok = _pose_rows(rows, layout, kind, body)
        q = [pose[:, 6:10], pose[:, 10:14], pose[:, 14:18]]
        if kind != "targets":                               # only the quaternions of a message or an est row are read
            ok = np.isfinite(pose[:, 6:18]).all(axis=1)
        for j in range(3):
            n = np.sqrt(((q[j][:, 0] * q[j][:, 0] + q[j][:, 1] * q[j][:, 1]) + q[j][:, 2] * q[j][:, 2]) + q[j][:, 3] * q[j][:, 3])
            ok = ok & np.isfinite(n) & (n > 0.0)
            q[j] = _unit4(q[j])
        ql, qu, qh = q
        e_rho, e_n, e_swing, e_twist, e_az = _swing_twist(_qmul(qu * conj, ql))
        s = _qmul(qh * conj, qu)
        s_rho, _, _, s_twist, _ = _swing_twist(s)
        w, x, y, z = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
        dx = -((w * w + x * x) - (y * y + z * z))
        dy = -(2.0 * (x * y + w * z))
        dz = -(2.0 * (x * z - w * y))
        h = np.sqrt(dx * dx + dz * dz)
        qh = np.where((qh[:, 0] < 0.0)[:, None], -qh, qh)
        nan = np.nan
        a = np.stack([e_swing, np.where(e_n < sh, nan, e_az), np.where(e_rho < sh, nan, e_twist), np.arctan2(h, -dy),
                      np.where(h < sf, nan, np.arctan2(dz, -dx)), np.where(s_rho < sh, nan, s_twist), 2.0 * np.arctan2(qh[:, 2], qh[:, 0])],
                     axis=1)
    a[~ok] = np.nan
    return a


def _kind_rows(rows, layout: int, kind: str, what: str):
    w = _rows_width(layout, kind)
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] < w:
        raise UserWarning(f"{what}: expected [F, >= {w}], got {tuple(rows.shape)}")
    return rows[:, :w].astype(np.float64)


def joint_angles_numpy(rows, layout: int, kind: str = "msg", truth=None, truth_kind: str = "est", starts=None, skip: int = 0, rec_lags=None,
                       bodies=None, min_swing: float = 0.05):
    """The host statement of ``joint_angles`` for one set of rows: ``(angles [F, 7], errors [F, 7] | None, acc [R, 71])`` float64, plain
    numpy with the operations of include/ape_hip.h in their order.  ``rows [F, >= w]`` of ``kind`` ``"msg"``, ``"est"`` or ``"targets"``
    (through the numpy statement of the device's truth FK with ``bodies``), ``truth [F, >= w']`` of ``truth_kind`` likewise; float32 is
    widened exactly.  Frame ``f`` of recording ``r`` is paired with truth row ``f - rec_lags[r]`` where that lies in the recording.
    ``acc``: per angle the sum, sum of squares, minimum, maximum and count of its finite values over the frames with ``f - s_r >=
    skip``, per error the sum, sum of magnitudes, sum of squares, largest magnitude and count, then the frames of the support (numpy's
    summation order, so sums agree with the device to rounding)."""
    m = _min_swing(min_swing)
    rows = _kind_rows(rows, layout, kind, "rows")
    F = rows.shape[0]
    st = _recording_starts(starts).astype(np.int64)
    R = st.shape[0]
    rec = np.searchsorted(st, np.arange(F), side="right") - 1
    ends = np.r_[st[1:], F]
    b = None
    if kind == "targets" or (truth is not None and truth_kind == "targets"):
        b = _body_rows(bodies, R, "joint_angles bodies")
        b = b[rec] if b.shape[0] > 1 else np.broadcast_to(b, (F, 9))
    angles = _row_angles(rows, layout, kind, b, m)
    errors = None
    if truth is not None:
        truth = _kind_rows(truth, layout, truth_kind, "truth")
        if truth.shape[0] != F:
            raise UserWarning(f"truth: {truth.shape[0]} rows for {F} frames")
        tang = _row_angles(truth, layout, truth_kind, b, m)
        _, _, off = _sweep((0, 0), R, rec_lags)
        tf = np.arange(F) - off.astype(np.int64)[rec]
        paired = (tf >= st[rec]) & (tf < ends[rec])
        ta = np.where(paired[:, None], tang[np.clip(tf, 0, F - 1)], np.nan)
        with np.errstate(all="ignore"):
            errors = angles - ta
            for k in range(ANGLE_WIDTH):
                if ANGLE_PERIODIC[k]:
                    d = errors[:, k]
                    errors[:, k] = np.where(d > np.pi, d - 2.0 * np.pi, np.where(d <= -np.pi, d + 2.0 * np.pi, d))
    acc = np.zeros((R, ANGLE_ACC_WIDTH))
    for r, (s0, e0) in enumerate(zip(st, ends)):
        lo = min(s0 + int(skip), e0)
        acc[r, 70] = e0 - lo
        for k in range(ANGLE_WIDTH):
            v = angles[lo:e0, k]
            v = v[np.isfinite(v)]
            acc[r, 5 * k:5 * k + 5] = [v.sum(), (v * v).sum(), v.min(initial=np.inf), v.max(initial=-np.inf), v.shape[0]]
            if errors is not None:
                d = errors[lo:e0, k]
                d = d[np.isfinite(d)]
                acc[r, 35 + 5 * k:40 + 5 * k] = [d.sum(), np.abs(d).sum(), (d * d).sum(), np.abs(d).max(initial=0.0), d.shape[0]]
    return angles, errors, acc


def joint_angles(layout: int, rows, kind: str = "msg", truth=None, truth_kind: str = "est", starts=None, skip: int = 0, rec_lags=None,
                 bodies=None, min_swing: float = 0.05, per_frame: bool = True, out_dtype=None):
    """The joint angles of every frame, their errors against truth and their sums per recording (``ape_joint_angles``).  ``rows``: device
    ``[F, >= w]`` or ``[C, F, >= w]`` (C sets of the same recordings, at most 64), float32 or float64, a strided view is taken without a
    copy; ``kind``: ``"msg"``, ``"est"`` or ``"targets"`` (converted with ``bodies``), as ``motion_sums`` takes them.  ``truth``: device
    ``[F, >= w']`` rows of ``truth_kind`` (any of the three; shared by all sets), or None; ``rec_lags``: int ``[R]``, frame ``f`` of
    recording ``r`` is paired with truth row ``f - rec_lags[r]``.  ``starts``: the recordings' first frames; ``skip``: leading frames of
    every recording left out of the accumulators.  ``min_swing`` (radians, in ``[0, pi / 2)``): below it the azimuth and twist angles of
    a joint are NaN.  Returns ``(angles, errors, acc)`` on the device: ``[F, 7]`` of ``out_dtype`` (default: the rows'; None unless
    ``per_frame``; errors None without truth) in ``ANGLE_NAMES``' order, radians, and float64 ``[R, 71]`` raw accumulators
    (``summarise_angles``, ``merge_angles``); all with a leading ``C`` for ``[C, F, w]`` rows.  The same inputs give the same bits.  The
    call does not wait for the device."""
    m = _min_swing(min_swing)
    w = _rows_width(layout, kind)
    rd, rs, ss, n = _sets_view(rows, w, "rows")
    if rs > 2 ** 31 - 1:
        raise UserWarning(f"rows: a row stride of {rs} elements does not fit the entry's int32 (copy the view)")
    out_dtype = rd.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
    F, dev, sets = int(rd.shape[-2]), rd.device, 1 if n is None else n
    st = _recording_starts(starts)
    R = int(st.shape[0])
    td, ts, off = None, 0, None
    if truth is not None:
        td, ts = _rows_view(truth, _rows_width(layout, truth_kind), "truth")
        if td.shape[0] != F or td.device != dev or ts > 2 ** 31 - 1:
            raise UserWarning(f"truth: {F} rows on {dev} with a stride that fits int32, got {tuple(td.shape)} on {td.device}")
        off = _sweep((0, 0), R, rec_lags)[2]
    elif rec_lags is not None:
        raise UserWarning("rec_lags pair rows with truth: give truth with them")
    body = _body_rows(bodies, R, "joint_angles bodies") if kind == "targets" or (td is not None and truth_kind == "targets") else None
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())                       # noqa: E731
    with torch.cuda.device(dev):
        angles = torch.empty((sets, F, ANGLE_WIDTH), dtype=out_dtype, device=dev) if per_frame else None
        errors = torch.empty((sets, F, ANGLE_WIDTH), dtype=out_dtype, device=dev) if per_frame and td is not None else None
        acc = torch.empty((sets, max(R, 1), ANGLE_ACC_WIDTH), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_joint_angles(int(layout), ptr(rd), ROWS_KINDS[kind], rs, _f64(rd.dtype), sets, ss,
                                               ptr(td), ROWS_KINDS[truth_kind] if td is not None else 0, ts,
                                               _f64(td.dtype) if td is not None else _hip.F64,
                                               C.c_void_p(off.ctypes.data) if off is not None else None, F, C.c_void_p(st.ctypes.data), R, int(skip),
                                               C.c_void_p(body.ctypes.data) if body is not None else None,
                                               int(body.shape[0]) if body is not None else 0, m, ptr(angles), ptr(errors), _f64(out_dtype),
                                               ptr(acc), stream), "ape_joint_angles")
    if n is None:
        return (None if angles is None else angles[0]), (None if errors is None else errors[0]), acc[0]
    return angles, errors, acc


def _angles_host(acc, ndims=(2,)) -> np.ndarray:
    a = acc.detach().cpu().numpy() if isinstance(acc, torch.Tensor) else np.asarray(acc)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim not in ndims or a.shape[-1] != ANGLE_ACC_WIDTH:
        raise UserWarning(f"expected angle accumulators [..., R, {ANGLE_ACC_WIDTH}] of {' or '.join(str(n) for n in ndims)} dimensions, "
                          f"got {tuple(a.shape)}")
    return a


def summarise_angles(acc) -> list:
    """``acc [R, 71]`` (of several sets: one set's slice ``acc[c]``) -> per recording a dict: ``frames`` of the support and, under
    ``"rad"`` and ``"deg"``, per name of ``ANGLE_NAMES`` a dict with ``mean``, ``std``, ``min``, ``max`` and ``rom`` (range of motion,
    max - min) of the angle and ``bias`` (mean signed error), ``mae``, ``rmse`` and ``worst`` (largest magnitude) of its error against
    truth, NaN where nothing was counted; ``count`` and ``error_count`` are the frames behind them.  The mean and the standard deviation
    of a periodic angle are those of its values in ``(-pi, pi]``, not circular statistics."""
    res = []
    nan = float("nan")
    with np.errstate(all="ignore"):
        for row in _angles_host(acc):
            d = {"frames": int(row[70]), "rad": {}, "deg": {}}
            for k, name in enumerate(ANGLE_NAMES):
                s1, s2, lo, hi, n = row[5 * k:5 * k + 5]
                e1, ea, e2, ew, m = row[35 + 5 * k:40 + 5 * k]
                mean = s1 / n if n else nan
                v = {"count": int(n), "mean": mean, "std": float(np.sqrt(max(s2 / n - mean * mean, 0.0))) if n else nan,
                     "min": lo if n else nan, "max": hi if n else nan, "rom": hi - lo if n else nan,
                     "error_count": int(m), "bias": e1 / m if m else nan, "mae": ea / m if m else nan,
                     "rmse": float(np.sqrt(e2 / m)) if m else nan, "worst": ew if m else nan}
                d["rad"][name] = {key: (val if key.endswith("count") else float(val)) for key, val in v.items()}
                d["deg"][name] = {key: (val if key.endswith("count") else float(np.degrees(val))) for key, val in v.items()}
            res.append(d)
    return res


def merge_angles(acc_a, acc_b) -> np.ndarray:
    """the accumulators ``[R, 71]`` (or ``[C, R, 71]``) of two pieces of the same recordings as one: sums, counts and frames added, the
    smaller of the minima, the larger of the maxima and of the largest error magnitudes.  An angle needs no frames below it, so chained
    pieces merge to the whole recording's counts."""
    a, b = _angles_host(acc_a, (2, 3)), _angles_host(acc_b, (2, 3))
    if a.shape != b.shape:
        raise UserWarning(f"merge_angles: {tuple(a.shape)} and {tuple(b.shape)} accumulators")
    out = a + b
    lo, hi = list(_ANGLE_MIN_COLS), list(_ANGLE_MAX_COLS)
    out[..., lo] = np.minimum(a[..., lo], b[..., lo])
    out[..., hi] = np.maximum(a[..., hi], b[..., hi])
    return out


def angle_edges(bins: int = 72) -> np.ndarray:
    """float64 ``[14, bins + 1]`` linear edges for ``hist_rows`` over ``[angles | errors]`` (the two ``[F, 7]`` outputs of
    ``joint_angles`` side by side): ``[0, pi]`` for elbow flexion and shoulder elevation, ``[-pi, pi]`` for the other angles and for the
    seven errors.  With the default 72 bins an edge lies every 2.5 and every 5 degrees: ``fraction_within`` at the edges ``e[k, 35]`` and
    ``e[k, 37]`` of an error column (-5 and +5 degrees; thresholds must be edges bit for bit) gives the shares whose difference is the
    share of frames within 5 degrees."""
    bins = int(bins)
    if not 1 <= bins <= HIST_MAX_BINS:
        raise UserWarning(f"angle_edges: between 1 and {HIST_MAX_BINS} bins, got {bins}")
    half, full = np.linspace(0.0, np.pi, bins + 1), np.linspace(-np.pi, np.pi, bins + 1)
    rows = [full if ANGLE_PERIODIC[k] else half for k in range(ANGLE_WIDTH)] + [full] * ANGLE_WIDTH
    return np.ascontiguousarray(np.stack(rows))


# ---- errors by condition: per-slot sums of any per-frame column keyed by any other (ape_score_by) ---------------------------
# A record [..., K, B + 3, V, 4] holds, per key column, slot of its edges (``hist_rows``' slots) and value column: n, the sum, the sum of
# squares and the maximum of the values of the window's frames whose key lies in the slot (NaN values left out of their own cell).
BY_MAX_KEYS, BY_MAX_VALUES, BY_MAX_BINS, BY_PIECE = _hip.BY_MAX_KEYS, _hip.BY_MAX_VALUES, _hip.BY_MAX_BINS, _hip.BY_PIECE
SIGMA_NAMES = ("hand_sigma", "elbow_sigma", "larm_spread", "uarm_spread", "hips_spread")


def _by_sides(keys, values):
    """(keys [Ck, F, K], values [Cv, F, V] float64, C, whether the result has a set dimension) of host arrays [F, .] or [C, F, .]"""
    k, v = np.asarray(keys), np.asarray(values)
    if k.ndim not in (2, 3) or v.ndim not in (2, 3) or min(k.shape) < 1 or min(v.shape) < 1:
        raise UserWarning(f"keys and values: expected [F, K] or [C, F, K] and [F, V] or [C, F, V], got {tuple(k.shape)} and {tuple(v.shape)}")
    sets = k.ndim == 3 or v.ndim == 3
    k3, v3 = (k if k.ndim == 3 else k[None]).astype(np.float64), (v if v.ndim == 3 else v[None]).astype(np.float64)
    if k3.shape[1] != v3.shape[1] or (k.ndim == 3 and v.ndim == 3 and k3.shape[0] != v3.shape[0]):
        raise UserWarning(f"keys {tuple(k.shape)} and values {tuple(v.shape)}: the same frames, and the same sets where both have sets")
    return k3, v3, max(k3.shape[0], v3.shape[0]), sets


def stats_by_numpy(keys, values, edges, starts=None, skip: int = 0, trim=None) -> np.ndarray:
    """The host statement of ``stats_by``, order included: ``_slots`` per key column; the window cut into pieces of ``BY_PIECE`` frames
    from its first frame; per piece and cell ``np.cumsum`` (which adds one by one in frame order; ``np.sum`` adds pairwise) over ``+0.0``
    and then the cell's terms; the piece sums added in a loop from ``+0.0``.  A NaN value is a term of ``+0.0``, which a sum that started
    at ``+0.0`` cannot see.  ``keys``: ``[F, K]`` or ``[C, F, K]``, ``values``: ``[F, V]`` or ``[C, F, V]`` (float32 is widened; a side
    without sets is shared); returns float64 ``[(C,) R, K, B + 3, V, 4]``."""
    k3, v3, Cn, sets = _by_sides(keys, values)
    F, K, V = k3.shape[1], k3.shape[2], v3.shape[2]
    e = _edges(edges, K)
    B = e.shape[1] - 1
    st = _recording_starts(starts).astype(np.int64)
    R = st.shape[0]
    tr = _trims(R, skip, trim).astype(np.int64)
    ends = np.r_[st[1:], F]
    out = np.zeros((Cn, R, K, B + 3, V, 4))
    out[..., 3] = -np.inf
    zero = np.zeros((1, V))
    with np.errstate(all="ignore"):
        for r in range(R):
            a, b = int(st[r] + tr[r, 0]), int(ends[r] - tr[r, 1])
            for c in range(Cn if a < b else 0):
                kc, vc = k3[c if k3.shape[0] > 1 else 0], v3[c if v3.shape[0] > 1 else 0]
                for kk in range(K):
                    slots = _slots(kc[a:b, kk], e[kk])
                    for p0 in range(a, b, BY_PIECE):
                        p1 = min(b, p0 + BY_PIECE)
                        sl, x = slots[p0 - a:p1 - a], vc[p0:p1]
                        for s in np.unique(sl):
                            rows = x[sl == s]                       # the cell's frames of the piece, in frame order
                            ok = ~np.isnan(rows)
                            t = np.where(ok, rows, 0.0)
                            cell = out[c, r, kk, s]
                            cell[:, 0] = cell[:, 0] + ok.sum(axis=0)
                            cell[:, 1] = cell[:, 1] + np.cumsum(np.concatenate([zero, t]), axis=0)[-1]
                            cell[:, 2] = cell[:, 2] + np.cumsum(np.concatenate([zero, t * t]), axis=0)[-1]
                            cell[:, 3] = np.maximum(cell[:, 3], np.where(ok, rows, -np.inf).max(axis=0))
    return out if sets else out[0]


def _by_view(t, what: str):
    """(tensor [C, F, W], C, F, W, set / frame stride in elements, whether it has sets) of a device view ``[F, W]`` or ``[C, F, W]`` under
    ``_hist_view``'s rules: the last dimension contiguous, frames and sets apart; anything else is copied"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() not in (2, 3) or min(t.shape) < 1:
        raise UserWarning(f"{what}: expected a device tensor [F, W] or [C, F, W]")
    if t.dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"{what}: float32 or float64, got {t.dtype}")
    v = t[None] if t.dim() == 2 else t
    Cn, F, W = (int(n) for n in v.shape)
    ss, fs, ws = (int(s) for s in v.stride())
    fs = fs if F > 1 else max(fs, W)
    if (W > 1 and ws != 1) or fs < W or (Cn > 1 and ss < F * fs):
        v = v.contiguous()
        ss, fs, ws = (int(s) for s in v.stride())
        fs = max(fs, W)
    return v, Cn, F, W, (ss if Cn > 1 else 0), fs, t.dim() == 3


def stats_by(keys, values, edges, starts=None, skip: int = 0, trim=None):
    """Per-slot count, sum, sum of squares and maximum of value columns keyed by other columns, per recording, on the device
    (``ape_score_by``).  ``keys``: a device ``[F, K]`` or ``[C, F, K]`` view, ``values``: ``[F, V]`` or ``[C, F, V]``, ``V <= 16``,
    ``C <= 64``, float32 or float64 per side; a side without sets is shared by all sets of the other.  ``joint_angles``' ``[C, F, 7]``,
    ``score_rows``' ``[F, 7]``, ``motion_sums``' ``[C, F, 12]``, ``spread_sigma``'s ``[F, 5]``, column slices and strided views go in
    without a copy (``_hist_view``'s rules).  ``edges``: float64 ``[B + 1]`` for all key columns or ``[K, B + 1]``, ``B <= 125``;
    ``starts``, ``skip``, ``trim``: the windows, as in ``hist_rows``.  More than 8 key columns are taken 8 to a call (a key column's
    record does not depend on the others).  Returns float64 ``[(C,) R, K, B + 3, V, 4]`` on the device: ``n``, the sum, the sum of
    squares, the maximum (``-inf`` for an empty cell).  The order of every sum is stated (``stats_by_numpy``): the same inputs give the
    same bits, a recording's record does not depend on the batch around it.  The call does not wait for the device."""
    kv, Ck, F, K, kss, kfs, ksets = _by_view(keys, "keys")
    vv, Cv, Fv, V, vss, vfs, vsets = _by_view(values, "values")
    if F != Fv or (ksets and vsets and Ck != Cv) or kv.device != vv.device:
        raise UserWarning(f"keys {tuple(keys.shape)} and values {tuple(values.shape)}: the same frames on one device, and the same sets "
                          "where both have sets")
    Cn = max(Ck, Cv)
    if not 1 <= V <= BY_MAX_VALUES or not 1 <= Cn <= _hip.POST_MAX_CONFIGS:
        raise UserWarning(f"values: between 1 and {BY_MAX_VALUES} columns and at most {_hip.POST_MAX_CONFIGS} sets, got {V} and {Cn}")
    e = _edges(edges, K)
    B = int(e.shape[1]) - 1
    if B > BY_MAX_BINS:
        raise UserWarning(f"edges: at most {BY_MAX_BINS} bins, got {B}")
    st = _recording_starts(starts)
    R = int(st.shape[0])
    tr = _trims(R, skip, trim)
    dev = kv.device
    outs = []
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for k0 in range(0, K, BY_MAX_KEYS):
            nk = min(BY_MAX_KEYS, K - k0)
            by = torch.empty((Cn, max(R, 1), nk, B + 3, V, 4), dtype=torch.float64, device=dev)
            ek = np.ascontiguousarray(e[k0:k0 + nk])
            _hip.check(_hip.lib().ape_score_by(C.c_void_p(kv.data_ptr() + k0 * kv.element_size()), _f64(kv.dtype), nk, kss, kfs,
                                               C.c_void_p(vv.data_ptr()), _f64(vv.dtype), V, vss, vfs, Cn, F, C.c_void_p(st.ctypes.data), R,
                                               C.c_void_p(tr.ctypes.data), C.c_void_p(ek.ctypes.data), B, C.c_void_p(by.data_ptr()), stream),
                       "ape_score_by")
            outs.append(by)
    by = outs[0] if len(outs) == 1 else torch.cat(outs, dim=2)
    return by if (ksets or vsets) else by[0]


def _by_host(by) -> np.ndarray:
    b = by.detach().cpu().numpy() if isinstance(by, torch.Tensor) else np.asarray(by)
    if b.ndim < 4 or b.shape[-1] != 4 or b.shape[-3] < 4:
        raise UserWarning(f"expected a record [..., K, B + 3, V, 4], got {tuple(b.shape)}")
    return b.astype(np.float64)


def merge_by(by_a, by_b) -> np.ndarray:
    """the records of two pieces of the same recordings over the same edges as one (float64, on the host): ``n``, sums and sums of squares
    added, the larger of the maxima.  For chained pieces: ``n`` and the maxima are the one call's exactly, a sum of ``n`` terms lies within
    ``n 2^-53 sum|x|`` of it (another order of the same terms)."""
    a, b = _by_host(by_a), _by_host(by_b)
    if a.shape != b.shape:
        raise UserWarning(f"merge_by: {tuple(a.shape)} and {tuple(b.shape)} records")
    with np.errstate(all="ignore"):
        out = a + b
    out[..., 3] = np.maximum(a[..., 3], b[..., 3])
    return out


def pool_by(by) -> np.ndarray:
    """``by [(C,) R, K, B + 3, V, 4]`` -> ``[(C,) K, B + 3, V, 4]``: the recordings folded in order, from ``+0.0`` (the maxima from
    ``-inf``)"""
    b = _by_host(by)
    if b.ndim not in (5, 6):
        raise UserWarning(f"pool_by: expected [(C,) R, K, B + 3, V, 4], got {tuple(b.shape)}")
    out = np.zeros(b.shape[:-5] + b.shape[-4:])
    out[..., 3] = -np.inf
    with np.errstate(all="ignore"):
        for r in range(b.shape[-5]):
            piece = b[..., r, :, :, :, :]
            top = np.maximum(out[..., 3], piece[..., 3])
            out = out + piece
            out[..., 3] = top
    return out


def summarise_by(by, edges, key_names=None, value_names=None) -> dict:
    """A record ``[..., K, B + 3, V, 4]`` over ``edges`` -> a dict of float64 arrays ``[..., K, B + 3, V]``: ``n``, ``mean``, ``rms`` and
    ``max`` per cell (``mean`` and ``rms`` NaN where ``n == 0``, ``max`` ``-inf`` there), with ``edges [K, B + 1]``, ``key_names`` and
    ``value_names`` (default ``key0 ..`` / ``value0 ..``) and ``slots``, the names of the ``B + 3`` slots (``"(lo, hi]"`` per bin, then
    ``"below"``, ``"above"``, ``"nan"``) per key column.  For a reliability curve: keys ``spread_sigma``, the same sigma among the
    values; each bin's ``rms`` of an error beside its ``mean`` of the sigma."""
    b = _by_host(by)
    K, S, V = b.shape[-4], b.shape[-3], b.shape[-2]
    e = _edges(edges, K)
    if e.shape[1] + 2 != S:
        raise UserWarning(f"a record of {S - 3} bins against {e.shape[1]} edges")
    key_names = tuple(f"key{k}" for k in range(K)) if key_names is None else tuple(key_names)
    value_names = tuple(f"value{v}" for v in range(V)) if value_names is None else tuple(value_names)
    if len(key_names) != K or len(value_names) != V:
        raise UserWarning(f"summarise_by: {len(key_names)} and {len(value_names)} names for {K} key and {V} value columns")
    n = b[..., 0]
    with np.errstate(all="ignore"):
        some = n > 0
        div = np.where(some, n, 1.0)
        mean = np.where(some, b[..., 1] / div, np.nan)
        rms = np.where(some, np.sqrt(b[..., 2] / div), np.nan)
    slots = [[f"({e[k, i]:g}, {e[k, i + 1]:g}]" for i in range(S - 3)] + ["below", "above", "nan"] for k in range(K)]
    return {"n": n, "mean": mean, "rms": rms, "max": b[..., 3].copy(), "edges": e, "key_names": key_names, "value_names": value_names,
            "slots": slots}


def spread_sigma(spread):
    """``spread [..., >= 21]`` (the spread records of a replay in its first 21 columns, a device tensor) -> ``[..., 5]`` of the same dtype by torch operations on
    the device: ``sqrt(xx + yy + zz)`` of the hand covariance (columns 3, 6, 8; added left to right), the same of the elbow covariance
    (12, 15, 17), and the three angular spreads (18:21).  The keys of a reliability curve (``SIGMA_NAMES``); a covariance with a
    negative or NaN trace gives NaN."""
    if not isinstance(spread, torch.Tensor) or spread.dim() < 1 or spread.shape[-1] < _hip.SPREAD_WIDTH:
        raise UserWarning(f"spread: expected a tensor [..., >= {_hip.SPREAD_WIDTH}]")
    s = spread
    hand = torch.sqrt((s[..., 3] + s[..., 6]) + s[..., 8])
    elbow = torch.sqrt((s[..., 12] + s[..., 15]) + s[..., 17])
    return torch.cat([hand[..., None], elbow[..., None], s[..., 18:21]], dim=-1)


# ---- reaches and holds: segment a replay and score each segment ----
# Arm motion is holds joined by reaches, and its users count in movements.  ``segment_frames`` labels every frame hold or move from a
# per-frame key (the hand speed) with hysteresis and minimum lengths, ``segment_runs`` turns any labels into a table of segments,
# ``segment_stats`` reduces per-frame columns over every segment in a stated order; ``match_segments`` and ``summarise_segments`` read the
# tables on the host.  ``segment_frames_numpy``, ``segment_runs_numpy`` and ``segment_stats_numpy`` are the host statements.
SEGMENT_MAX_MIN, SEG_TABLE_WIDTH, SEG_MAX_VALUES = _hip.SEGMENT_MAX_MIN, _hip.SEG_TABLE_WIDTH, _hip.SEG_MAX_VALUES
SEG_STAT_WIDTH, SEG_PIECE = _hip.SEG_STAT_WIDTH, _hip.SEG_PIECE
SEG_STAT_NAMES = ("n", "sum", "sum_sq", "max", "argmax")
HOLD, MOVE = 0, 1


def _segment_rules(thresholds, mins, S: int, first_label):
    """the host arrays of ``ape_segment_frames``, checked as the C ABI checks them: float64 ``[P, 2]`` of ``(lo, hi)``, int32 ``[P, 2]`` of
    ``(min_hold, min_move)``, ``P`` 1 or ``S`` (one pair for every set, or a row per set), ``first_label``"""
    try:
        th = np.asarray(thresholds, dtype=np.float64).reshape(-1, 2)
        mn = np.asarray(mins, dtype=np.int32).reshape(-1, 2)
    except (TypeError, ValueError):
        raise UserWarning("thresholds: (lo, hi) or [P, 2]; mins: (min_hold, min_move) or [P, 2]")
    P = max(th.shape[0], mn.shape[0])
    if P not in (1, S) or th.shape[0] not in (1, P) or mn.shape[0] not in (1, P):
        raise UserWarning(f"thresholds / mins: one row or one per set ({S}), got {th.shape[0]} and {mn.shape[0]}")
    th = np.ascontiguousarray(np.broadcast_to(th, (P, 2)))
    mn = np.ascontiguousarray(np.broadcast_to(mn, (P, 2)))
    if not np.isfinite(th).all() or (th[:, 1] < th[:, 0]).any():
        raise UserWarning(f"thresholds: finite (lo, hi) with lo <= hi, got {th.tolist()}")
    if (mn < 1).any() or (mn > SEGMENT_MAX_MIN).any():
        raise UserWarning(f"mins: minimum lengths 1 .. {SEGMENT_MAX_MIN}, got {mn.tolist()}")
    if first_label not in (0, 1):
        raise UserWarning(f"first_label: 0 (hold) or 1 (move), got {first_label!r}")
    return th, mn, P, int(first_label)


def _runs(lab, a: int, b: int):
    """the maximal runs of equal values of ``lab[a:b]`` as ``(first, end)`` pairs"""
    f = a
    while f < b:
        g = f + 1
        while g < b and lab[g] == lab[f]:
            g += 1
        yield f, g
        f = g


def segment_frames_numpy(keys, thresholds=(0.004, 0.008), mins=(1, 1), starts=None, first_label: int = 0) -> np.ndarray:
    """The host statement of ``segment_frames`` as a plain loop: ``keys [(S,) F]`` -> uint8 ``[(S,) F]``, 0 hold and 1 move.  Per set and
    recording ``[a, b)``, on the key widened to float64: (1) a frame decides 1 if ``v > hi``, 0 if ``v <= lo``, and is undecided otherwise
    (NaN fails both); (2) ``s[f]`` is the decision of the last decisive frame in ``[a, f]``, ``first_label`` without one; (3) a run of 0
    shorter than ``min_hold`` with a 1 on both sides inside the recording becomes 1; (4) then a run of 1 shorter than ``min_move`` becomes
    0, at the recording's ends too."""
    k = np.asarray(keys)
    k2 = k.reshape(-1, k.shape[-1]).astype(np.float64)
    S, F = k2.shape
    th, mn, P, first_label = _segment_rules(thresholds, mins, S, first_label)
    st = [int(s) for s in _recording_starts(starts)]
    out = np.zeros((S, F), dtype=np.uint8)
    for s in range(S):
        (lo, hi), (min_hold, min_move) = th[s if P > 1 else 0], mn[s if P > 1 else 0]
        lab = out[s]
        for a, b in zip(st, st[1:] + [F]):
            cur = first_label
            for f in range(a, b):
                v = k2[s, f]
                if v > hi:
                    cur = 1
                elif v <= lo:
                    cur = 0
                lab[f] = cur
            for f, g in list(_runs(lab, a, b)):
                if lab[f] == 0 and g - f < min_hold and f > a and g < b:
                    lab[f:g] = 1
            for f, g in list(_runs(lab, a, b)):
                if lab[f] == 1 and g - f < min_move:
                    lab[f:g] = 0
    return out.reshape(k.shape)


def _key_sets(keys, what: str):
    """(tensor [S, F], set stride, frame stride) of a device view ``[F]`` or ``[S, F]`` as the strided entries take it; copied if need be"""
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda or keys.dim() not in (1, 2) or min(keys.shape) < 1:
        raise UserWarning(f"{what}: a device tensor [F] or [S, F]")
    if keys.dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"{what}: float32 or float64, got {keys.dtype}")
    k = keys[None] if keys.dim() == 1 else keys
    S, F = int(k.shape[0]), int(k.shape[1])
    if S > _hip.POST_MAX_CONFIGS:
        raise UserWarning(f"{what}: at most {_hip.POST_MAX_CONFIGS} sets, got {S}")
    ss, fs = int(k.stride(0)), int(k.stride(1))
    fs = fs if F > 1 else max(fs, 1)
    if fs < 1 or (S > 1 and ss <= (F - 1) * fs):
        k = k.contiguous()
        ss, fs = int(k.stride(0)), max(int(k.stride(1)), 1)
    return k, (ss if S > 1 else 0), fs


def segment_frames(keys, thresholds=(0.004, 0.008), mins=(1, 1), starts=None, first_label: int = 0):
    """Hold or move for every frame, on the device (``ape_segment_frames``).  ``keys``: a device ``[F]`` or ``[S, F]`` view, float32 or
    float64, ``S <= 64`` -- column 0 of ``motion_sums``' per-frame rows, the hand speed, goes in without a copy; ``thresholds``:
    ``(lo, hi)`` or ``[S, 2]``: a frame above ``hi`` moves, one at or below ``lo`` holds, one between keeps the label of the frame before
    it (``lo == hi``: a plain threshold); ``mins``: ``(min_hold, min_move)`` or ``[S, 2]``, 1 .. 256: a hold shorter than ``min_hold``
    between two moves is filled, then a move shorter than ``min_move`` is dropped; ``starts``: the recordings' first frames -- a
    recording never inherits from the one before; ``first_label``: the label of a recording's frames before its first decisive one (NaN
    keys, such as the first three motion rows of a recording, are undecided).  Returns uint8 ``[(S,) F]`` on the device, 0 hold and 1
    move.  Integer work: the same inputs give the same bits.  Does not wait."""
    k, ss, fs = _key_sets(keys, "keys")
    S, F = int(k.shape[0]), int(k.shape[1])
    th, mn, P, first_label = _segment_rules(thresholds, mins, S, first_label)
    st = _recording_starts(starts)
    dev = k.device
    with torch.cuda.device(dev):
        labels = torch.empty((S, F), dtype=torch.uint8, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_segment_frames(C.c_void_p(k.data_ptr()), _f64(k.dtype), S, ss, F, fs, C.c_void_p(st.ctypes.data), int(st.shape[0]),
                                                 C.c_void_p(th.ctypes.data), C.c_void_p(mn.ctypes.data), P, first_label,
                                                 C.c_void_p(labels.data_ptr()), stream), "ape_segment_frames")
    return labels[0] if keys.dim() == 1 else labels


def segment_runs_numpy(labels, starts=None):
    """The host statement of ``segment_runs``: ``labels [(S,) F]`` of any integers -> ``(seg_of_frame int32 [(S,) F], n_segs, table)``.  A
    segment is a maximal run of equal labels inside one recording; ids count from 0 per set in frame order; a table row is ``(recording,
    first frame, length, label)``.  One set: ``n_segs`` an int and ``table`` int32 ``[n_segs, 4]``; ``S`` sets: int32 ``[S]`` and a list."""
    lab = np.asarray(labels)
    l2 = lab.reshape(-1, lab.shape[-1])
    S, F = l2.shape
    st = [int(s) for s in _recording_starts(starts)]
    sof, tables = np.zeros((S, F), dtype=np.int32), []
    for s in range(S):
        rows = []
        for r, (a, b) in enumerate(zip(st, st[1:] + [F])):
            for f, g in _runs(l2[s], a, b):
                sof[s, f:g] = len(rows)
                rows.append((r, f, g - f, int(l2[s, f])))
        tables.append(np.asarray(rows, dtype=np.int32).reshape(-1, SEG_TABLE_WIDTH))
    if lab.ndim == 1:
        return sof[0], len(tables[0]), tables[0]
    return sof, np.asarray([len(t) for t in tables], dtype=np.int32), tables


def segment_runs(labels, starts=None, cap=None, seg_of_frame: bool = True):
    """The table of segments of any labels, on the device (``ape_segment_runs``).  ``labels``: device uint8 ``[F]`` or ``[S, F]``, any
    values (``segment_frames``' labels, ``select_rungs``' selector); ``starts``: the recordings' first frames -- a segment ends with its
    recording.  Returns ``(seg_of_frame, n_segs, table)`` on the device: int32 ``[(S,) F]`` (None with ``seg_of_frame=False``), the id of
    every frame's segment counted from 0 per set; int32 ``[(S)]`` the number of segments; int32 ``[(S,) cap, 4]`` rows of ``(recording,
    first frame, length, label)``.  ``cap=None``: room for ``F`` segments is made and the table comes back sliced to ``n_segs`` (to the
    largest of the sets'), which READS ``n_segs`` BACK AND WAITS FOR THE DEVICE; with a ``cap`` the call does not wait, rows at or
    beyond ``cap`` are dropped (``n_segs`` still counts them: call again with more room) and rows from ``n_segs`` on are not written.
    Integer work: the same inputs give the same bits."""
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda or labels.dim() not in (1, 2) or min(labels.shape) < 1 or labels.dtype != torch.uint8:
        raise UserWarning("labels: a device uint8 tensor [F] or [S, F]")
    lab = (labels[None] if labels.dim() == 1 else labels).contiguous()
    S, F = int(lab.shape[0]), int(lab.shape[1])
    if S > _hip.POST_MAX_CONFIGS:
        raise UserWarning(f"labels: at most {_hip.POST_MAX_CONFIGS} sets, got {S}")
    room = F if cap is None else int(cap)
    if room < 1:
        raise UserWarning(f"cap: at least 1, got {cap}")
    st = _recording_starts(starts)
    dev = lab.device
    with torch.cuda.device(dev):
        sof = torch.empty((S, F), dtype=torch.int32, device=dev) if seg_of_frame else None
        n = torch.empty((S,), dtype=torch.int32, device=dev)
        table = torch.empty((S, room, SEG_TABLE_WIDTH), dtype=torch.int32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_segment_runs(C.c_void_p(lab.data_ptr()), S, F, C.c_void_p(st.ctypes.data), int(st.shape[0]),
                                               C.c_void_p(sof.data_ptr()) if sof is not None else None, C.c_void_p(n.data_ptr()),
                                               C.c_void_p(table.data_ptr()), room, stream), "ape_segment_runs")
        if cap is None:
            table = table[:, :int(n.max().item())]          # the one wait
    if labels.dim() == 1:
        return (None if sof is None else sof[0]), n[0], table[0]
    return sof, n, table


def _piece_sum(x) -> float:
    """``x`` float64 ``[n]`` added left to right from ``+0.0``, one rounding per element (``np.add.accumulate`` is that loop)"""
    return float(np.add.accumulate(np.concatenate([[0.0], x]))[-1])


def segment_stats_numpy(values, table) -> np.ndarray:
    """The host statement of ``segment_stats`` for one set: ``values [F]`` or ``[F, V]`` and ``table [n, 4]`` -> float64 ``[n, V, 5]`` of
    ``SEG_STAT_NAMES``: the count of values that are not NaN, their sum, the sum of their squares, their maximum (``-inf`` without any)
    and the batch frame of its first occurrence (``-1``).  The order, bit for bit: a value is widened to float64 and its square rounded
    before it is added; the segment is cut into pieces of 1024 frames counted from its first frame; a piece is added in frame order from
    ``+0.0`` and the pieces in order from ``+0.0``."""
    x = np.asarray(values)
    x = (x[:, None] if x.ndim == 1 else x).astype(np.float64)
    tab = np.asarray(table).reshape(-1, SEG_TABLE_WIDTH)
    out = np.zeros((tab.shape[0], x.shape[1], SEG_STAT_WIDTH))
    with np.errstate(all="ignore"):
        for i, (_, first, length, _) in enumerate(tab.tolist()):
            for v in range(x.shape[1]):
                n, total, total_sq = 0, 0.0, 0.0
                for p in range(first, first + length, SEG_PIECE):
                    piece = x[p:min(p + SEG_PIECE, first + length), v]
                    piece = piece[piece == piece]
                    n += piece.shape[0]
                    total = total + _piece_sum(piece)
                    total_sq = total_sq + _piece_sum(piece * piece)
                seg = x[first:first + length, v]
                live = np.flatnonzero(seg == seg)
                mx, arg = -np.inf, -1.0
                if n:
                    k = live[np.flatnonzero(seg[live] == seg[live].max())[0]]
                    mx, arg = seg[k], float(first + k)      # the value AT that frame: of +0.0 and -0.0, which compare equal, the earlier
                out[i, v] = n, total, total_sq, mx, arg
    return out


def segment_stats(values, seg_of_frame, n_segs, table):
    """Per-segment reductions of per-frame columns, on the device (``ape_segment_stats``).  ``values``: a device view ``[F]``, ``[F, V]``
    (shared by every set) or ``[S, F, V]``, float32 or float64, ``V <= 16``, any positive strides (columns of motion or score rows go in
    without a copy); ``seg_of_frame``, ``n_segs``, ``table``: what ``segment_runs`` returned for ``[F]`` or ``[S, F]`` labels (a table
    sliced to ``n_segs`` or one with a ``cap``).  Returns float64 ``[(S,) cap, V, 5]`` on the device, per segment and column
    ``SEG_STAT_NAMES``: the count of values that are not NaN, their sum, the sum of their squares, their maximum and the batch frame of its
    first occurrence; rows from ``n_segs`` on are not written.  The order of summation is ``segment_stats_numpy``'s: a segment's record
    has the same bits wherever it lies in a batch.  Does not wait."""
    if not isinstance(values, torch.Tensor) or not values.is_cuda or values.dim() not in (1, 2, 3) or min(values.shape) < 1:
        raise UserWarning("values: a device tensor [F], [F, V] or [S, F, V]")
    if values.dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"values: float32 or float64, got {values.dtype}")
    for t, what in ((seg_of_frame, "seg_of_frame"), (n_segs, "n_segs"), (table, "table")):
        if not isinstance(t, torch.Tensor) or t.device != values.device or t.dtype != torch.int32:
            raise UserWarning(f"{what}: segment_runs' int32 device tensor")
    one = seg_of_frame.dim() == 1
    sof = (seg_of_frame[None] if one else seg_of_frame).contiguous()
    tab = (table[None] if table.dim() == 2 else table).contiguous()
    n = n_segs.reshape(-1).contiguous()
    x = values[:, None] if values.dim() == 1 else values
    if sof.dim() != 2 or tab.dim() != 3 or tab.shape[2] != SEG_TABLE_WIDTH or tab.shape[0] != sof.shape[0] or n.shape[0] != sof.shape[0]:
        raise UserWarning("seg_of_frame [(S,) F], n_segs [(S)] and table [(S,) cap, 4] of one segment_runs call")
    S, F, cap = int(sof.shape[0]), int(sof.shape[1]), int(tab.shape[1])
    V = int(x.shape[-1])
    if x.shape[-2] != F or (x.dim() == 3 and x.shape[0] != S) or not 1 <= V <= SEG_MAX_VALUES:
        raise UserWarning(f"values: [{F}, V] or [{S}, {F}, V] with V <= {SEG_MAX_VALUES}, got {tuple(values.shape)}")
    dev = x.device
    with torch.cuda.device(dev):
        if cap < 1:
            return torch.empty((S, 0, V, SEG_STAT_WIDTH), dtype=torch.float64, device=dev)[0 if one else slice(None)]
        fs, cs = int(x.stride(-2)), int(x.stride(-1))
        ss = int(x.stride(0)) if x.dim() == 3 else 0
        fs, cs = (fs if F > 1 else max(fs, 1)), (cs if V > 1 else max(cs, 1))
        if fs < 1 or cs < 1 or (x.dim() == 3 and S > 1 and ss <= (F - 1) * fs + (V - 1) * cs):
            x = x.contiguous()
            fs, cs, ss = V, 1, (F * V if x.dim() == 3 else 0)
        sets = S if x.dim() == 3 else 1
        out = torch.empty((S, cap, V, SEG_STAT_WIDTH), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_segment_stats(C.c_void_p(x.data_ptr()), _f64(x.dtype), sets, ss if sets > 1 else 0, fs, cs, V, S, F,
                                                C.c_void_p(sof.data_ptr()), C.c_void_p(tab.data_ptr()), C.c_void_p(n.data_ptr()), cap,
                                                C.c_void_p(out.data_ptr()), stream), "ape_segment_stats")
    return out[0] if one else out


def _table_host(table) -> np.ndarray:
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    if t.ndim != 2 or t.shape[1] != SEG_TABLE_WIDTH:
        raise UserWarning(f"table: one set's [n, {SEG_TABLE_WIDTH}] rows of (recording, first frame, length, label)")
    return t.astype(np.int64)


def match_segments(table_est, table_truth, label: int = MOVE, lag: int = 0, times=None) -> dict:
    """The moves of an estimate paired with the truth's, on the host.  ``table_est``, ``table_truth``: one set's ``[n, 4]`` tables
    (``segment_runs``); ``label``: the segments compared; ``lag``: frame ``f`` of the estimate is held against frame ``f - lag`` of the
    truth (``score_lags``' sign).  The truth's segments are taken in order; each takes the still unmatched segment of the estimate in its
    recording that overlaps it in the most frames (at least one), ties to the earlier one.  Returns ``pairs`` (rows of the truth's and the
    estimate's table), ``onset`` and ``offset`` (the estimate's first frame and end less the truth's, in frames: positive is late),
    ``onset_s`` and ``offset_s`` with ``times`` (the frames' clock ``[F]``: the same differences on it, the end taken at the last
    frame), ``matched``, ``missed`` (the truth's without a partner) and ``spurious`` (the estimate's) with the rows of both."""
    est, tru = _table_host(table_est), _table_host(table_truth)
    e_rows = [i for i in range(est.shape[0]) if est[i, 3] == label]
    t_rows = [i for i in range(tru.shape[0]) if tru[i, 3] == label]
    taken, pairs, missed = set(), [], []
    for i in t_rows:
        r, a, n = int(tru[i, 0]), int(tru[i, 1]), int(tru[i, 2])
        best, most = None, 0
        for j in e_rows:
            if j in taken or int(est[j, 0]) != r:
                continue
            b = int(est[j, 1]) - int(lag)
            over = min(a + n, b + int(est[j, 2])) - max(a, b)
            if over > most:
                best, most = j, over
        if best is None:
            missed.append(i)
        else:
            taken.add(best)
            pairs.append((i, best))
    on = np.asarray([int(est[j, 1]) - int(lag) - int(tru[i, 1]) for i, j in pairs], dtype=np.int64)
    off = np.asarray([int(est[j, 1] + est[j, 2]) - int(lag) - int(tru[i, 1] + tru[i, 2]) for i, j in pairs], dtype=np.int64)
    res = {"pairs": pairs, "onset": on, "offset": off, "matched": len(pairs), "missed": len(missed), "spurious": len(e_rows) - len(taken),
           "missed_rows": missed, "spurious_rows": [j for j in e_rows if j not in taken]}
    if times is not None:
        t = times.detach().cpu().numpy() if isinstance(times, torch.Tensor) else np.asarray(times)
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        at = lambda f: t[np.clip(f, 0, t.shape[0] - 1)]
        res["onset_s"] = np.asarray([at(int(est[j, 1]) - int(lag)) - at(int(tru[i, 1])) for i, j in pairs], dtype=np.float64)
        res["offset_s"] = np.asarray([at(int(est[j, 1] + est[j, 2]) - 1 - int(lag)) - at(int(tru[i, 1] + tru[i, 2]) - 1) for i, j in pairs],
                                     dtype=np.float64)
    return res


def summarise_segments(table, stats, names, times=None) -> list:
    """One set's segments per recording and label, on the host.  ``table [n, 4]``, ``stats [n, V, 5]`` (``segment_stats``; rows past ``n``
    are ignored), ``names``: the ``V`` columns' names; ``times``: the frames' clock ``[F]`` -- durations are then the time from a
    segment's first to its last frame, else its frames.  Returns a list of dicts ordered by ``(recording, label)``: ``recording``,
    ``label``, ``count``, ``mean_duration``, ``longest_duration``, ``mean`` and ``max`` (by column name: the mean over the segments of
    each segment's mean of its values that are not NaN, and the largest of their maxima; NaN where no segment has a value)."""
    tab = _table_host(table)
    st = stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    st = np.asarray(st, dtype=np.float64)[:tab.shape[0]]
    names = list(names)
    if st.ndim != 3 or st.shape != (tab.shape[0], len(names), SEG_STAT_WIDTH):
        raise UserWarning(f"stats: [{tab.shape[0]}, {len(names)}, {SEG_STAT_WIDTH}] for this table and these names, got {st.shape}")
    dur = tab[:, 2].astype(np.float64)
    if times is not None:
        t = times.detach().cpu().numpy() if isinstance(times, torch.Tensor) else np.asarray(times)
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        dur = t[tab[:, 1] + tab[:, 2] - 1] - t[tab[:, 1]]
    res = []
    for r, lab in sorted({(int(a), int(b)) for a, b in zip(tab[:, 0], tab[:, 3])}):
        rows = np.flatnonzero((tab[:, 0] == r) & (tab[:, 3] == lab))
        s = st[rows]
        with np.errstate(all="ignore"):
            means = np.where(s[:, :, 0] > 0, s[:, :, 1] / np.where(s[:, :, 0] > 0, s[:, :, 0], 1.0), np.nan)
            some = (s[:, :, 0] > 0).any(axis=0)
            mean = np.where(some, np.nansum(means, axis=0) / np.maximum((s[:, :, 0] > 0).sum(axis=0), 1), np.nan)
            top = np.where(some, s[:, :, 3].max(axis=0), np.nan)
        res.append({"recording": r, "label": lab, "count": int(rows.shape[0]), "mean_duration": float(dur[rows].mean()),
                    "longest_duration": float(dur[rows].max()), "mean": dict(zip(names, mean.tolist())), "max": dict(zip(names, top.tolist()))})
    return res


# ---- spectra of a replay: Welch sums per frequency (ape_spectra) ----------------------------------------------------------------
# The scorers say how wrong a replay is, at which lag and how much it shakes; the spectra say at which frequencies.  The device takes raw
# sums over a recording's segments -- |X|^2, |Y|^2, conj(Y) X per bin -- and the host reads densities, gain, phase, delay and coherence
# off them.  The clock is the frame index: a bin is k / n cycles per frame, times ``rate`` in Hz.
SPECTRA_MAX_N, SPECTRA_MAX_COLS = _hip.SPECTRA_MAX_N, _hip.SPECTRA_MAX_COLS
TAPERS = ("hann", "boxcar")


def spectra_taper(taper, n: int) -> np.ndarray:
    """float64 ``[n]`` weights: ``"hann"`` (periodic: ``0.5 - 0.5 cos(2 pi i / n)``), ``"boxcar"`` (ones) or the caller's ``n`` finite
    values"""
    n = int(n)
    if isinstance(taper, str):
        if taper == "hann":
            return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)
        if taper == "boxcar":
            return np.ones(n, dtype=np.float64)
        raise UserWarning(f"taper: one of {TAPERS} or {n} weights, got {taper!r}")
    w = np.ascontiguousarray(np.asarray(taper, dtype=np.float64).reshape(-1))
    if w.shape[0] != n or not np.isfinite(w).all():
        raise UserWarning(f"taper: {n} finite weights, got {w.shape[0]}")
    return w


def _spectra_plan(n, hop):
    n = int(n)
    hop = n // 2 if hop is None else int(hop)
    if n < 16 or n > SPECTRA_MAX_N or n % 16 or not 1 <= hop <= n:
        raise UserWarning(f"spectra: n a multiple of 16 in 16 .. {SPECTRA_MAX_N} and hop in 1 .. n, got n = {n}, hop = {hop}")
    return n, hop


def _spectra_cols(cols, width: int, what: str) -> np.ndarray:
    c = np.arange(width, dtype=np.int32) if cols is None else np.ascontiguousarray(np.asarray(cols, dtype=np.int32).reshape(-1))
    if not 1 <= c.shape[0] <= SPECTRA_MAX_COLS or (c < 0).any() or (c >= width).any():
        raise UserWarning(f"{what}: between 1 and {SPECTRA_MAX_COLS} columns of the rows' {width}, got {c.tolist()}")
    return c


def pose_cols(layout: int, kind: str = "msg") -> tuple:
    """the six columns that hold the hand and the elbow position (x, y, z each) in rows of ``kind``: ``"msg"`` messages ``[4:7]`` and
    ``[11:14]``, ``"est"`` est rows ``[0:3]`` and ``[3:6]``.  Target rows state no positions in every layout: convert them first."""
    if layout not in _hip.EST_WIDTH:
        raise UserWarning(f"layout {layout} has no pose")
    if kind == "msg":
        return (4, 5, 6, 11, 12, 13)
    if kind == "est":
        return (0, 1, 2, 3, 4, 5)
    raise UserWarning(f"pose_cols: kind 'msg' or 'est', got {kind!r}")


POSE_COL_NAMES = ("hand_x", "hand_y", "hand_z", "elbow_x", "elbow_y", "elbow_z")


def spectra_numpy(rows, truth=None, cols=None, truth_cols=None, n: int = 256, hop=None, taper="hann", detrend: bool = True, starts=None,
                  skip: int = 0):
    """The host statement of ``spectra`` for one set: ``rows [F, w]`` (and ``truth [F, wt]``) -> ``(acc [R, V, n/2 + 1, W], counts
    [R, V, 2])``, float64 and int32, plain numpy with ``np.fft.rfft`` per segment: segment ``j`` of recording ``r`` is the frames
    ``s_r + skip + j hop + [0, n)``; ``a = w * (x - mean(x))`` (no mean without ``detrend``), ``X = rfft(a)``; ``acc[..., 0]`` sums
    ``re(X)^2 + im(X)^2``, with truth ``[1]`` the same of ``Y``, ``[2]`` and ``[3]`` the real and imaginary part of ``conj(Y) X``.  A
    segment with a value that is not finite on either side is left out for that column."""
    n, hop = _spectra_plan(n, hop)
    w = spectra_taper(taper, n)
    x = np.asarray(rows, dtype=np.float64)
    y = None if truth is None else np.asarray(truth, dtype=np.float64)
    F = x.shape[0]
    xc = _spectra_cols(cols, x.shape[1], "cols")
    yc = None if y is None else _spectra_cols(xc if truth_cols is None else truth_cols, y.shape[1], "truth_cols")
    if y is not None and (y.shape[0] != F or yc.shape[0] != xc.shape[0]):
        raise UserWarning("spectra: rows and truth of the same frames and as many columns")
    st = _recording_starts(starts)
    R, V, W = int(st.shape[0]), int(xc.shape[0]), 1 if y is None else 4
    acc = np.zeros((R, V, n // 2 + 1, W))
    counts = np.zeros((R, V, 2), dtype=np.int32)
    for r in range(R):
        s, e = int(st[r]), int(st[r + 1]) if r + 1 < R else F
        length = e - s - int(skip)
        J = (length - n) // hop + 1 if length >= n else 0
        for j in range(J):
            f0 = s + int(skip) + j * hop
            for v in range(V):
                sx = x[f0:f0 + n, xc[v]]
                sy = None if y is None else y[f0:f0 + n, yc[v]]
                if not np.isfinite(sx).all() or (sy is not None and not np.isfinite(sy).all()):
                    counts[r, v, 1] += 1
                    continue
                counts[r, v, 0] += 1
                X = np.fft.rfft(w * (sx - (sx.mean() if detrend else 0.0)))
                acc[r, v, :, 0] += X.real * X.real + X.imag * X.imag
                if sy is not None:
                    Y = np.fft.rfft(w * (sy - (sy.mean() if detrend else 0.0)))
                    acc[r, v, :, 1] += Y.real * Y.real + Y.imag * Y.imag
                    acc[r, v, :, 2] += Y.real * X.real + Y.imag * X.imag
                    acc[r, v, :, 3] += Y.real * X.imag - Y.imag * X.real
    return acc, counts


def spectra(rows, truth=None, cols=None, truth_cols=None, n: int = 256, hop=None, taper="hann", detrend: bool = True, starts=None,
            skip: int = 0):
    """Welch sums per recording, column and frequency bin on the device (``ape_spectra``).  ``rows``: a device ``[F, w]`` or
    ``[C, F, w]`` view (``C <= 64`` sets), float32 or float64 -- messages, est rows, ``motion_sums``' ``[C, F, 12]``, ``joint_angles``'
    ``[C, F, 7]`` go in as they lie (``_hist_view``'s rules); ``cols``: up to 16 of its columns (default: all of them).  ``truth``: the
    same frames, with or without sets (one truth for all sets), its own dtype and ``truth_cols`` (default: ``cols``).  Segments of ``n``
    frames (a multiple of 16 in 16 .. 512) every ``hop`` (default ``n // 2``) from ``skip`` frames into each recording of ``starts``,
    never across a boundary; ``taper``: ``"hann"``, ``"boxcar"`` or ``n`` weights; ``detrend`` takes each segment's mean off.  Returns
    ``(acc, counts)`` on the device: float64 ``[(C,) R, V, n/2 + 1, W]`` -- ``[0]`` the sum of ``|X|^2``, with truth also ``[1]`` of
    ``|Y|^2`` and ``[2]``, ``[3]`` real and imaginary part of the sum of ``conj(Y) X`` -- and int32 ``[(C,) R, V, 2]``, segments summed
    and left out (a value that is not finite).  The order of every sum is stated (include/ape_hip.h): the same inputs give the same
    bits.  ``summarise_spectra`` reads them.  The call does not wait for the device."""
    n, hop = _spectra_plan(n, hop)
    w = spectra_taper(taper, n)
    xv, Cx, F, Wx, xss, xfs, xsets = _by_view(rows, "rows")
    xc = _spectra_cols(cols, Wx, "cols")
    V = int(xc.shape[0])
    yv = None
    if truth is not None:
        yv, Cy, Fy, Wy, yss, yfs, ysets = _by_view(truth, "truth")
        yc = _spectra_cols(xc if truth_cols is None else truth_cols, Wy, "truth_cols")
        if Fy != F or yv.device != xv.device or yc.shape[0] != V or (ysets and Cy != Cx):
            raise UserWarning(f"rows {tuple(rows.shape)} and truth {tuple(truth.shape)}: the same frames on one device, as many columns, "
                              "and the rows' sets or none")
    if Cx > _hip.POST_MAX_CONFIGS:
        raise UserWarning(f"rows: at most {_hip.POST_MAX_CONFIGS} sets, got {Cx}")
    st = _recording_starts(starts)
    R, dev = int(st.shape[0]), xv.device
    with torch.cuda.device(dev):
        acc = torch.empty((Cx, max(R, 1), V, n // 2 + 1, 1 if yv is None else 4), dtype=torch.float64, device=dev)
        counts = torch.empty((Cx, max(R, 1), V, 2), dtype=torch.int32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if yv is None:
            ya = (None, 0, 0, 0, None)
        else:
            ya = (C.c_void_p(yv.data_ptr()), _f64(yv.dtype), yss, yfs, C.c_void_p(yc.ctypes.data))
        _hip.check(_hip.lib().ape_spectra(C.c_void_p(xv.data_ptr()), _f64(xv.dtype), xss, xfs, C.c_void_p(xc.ctypes.data), *ya, V, Cx, F,
                                          C.c_void_p(st.ctypes.data), R, int(skip), n, hop, C.c_void_p(w.ctypes.data),
                                          _hip.SPECTRA_DETREND if detrend else 0, C.c_void_p(acc.data_ptr()),
                                          C.c_void_p(counts.data_ptr()), stream), "ape_spectra")
    return (acc, counts) if xsets else (acc[0], counts[0])


def _spectra_host(acc, counts):
    a = acc.detach().cpu().numpy() if isinstance(acc, torch.Tensor) else np.asarray(acc)
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.int64)
    if a.ndim < 3 or a.shape[-1] not in (1, 4) or c.shape != a.shape[:-2] + (2,):
        raise UserWarning(f"expected spectra [..., V, bins, 1 | 4] and counts [..., V, 2], got {tuple(a.shape)} and {tuple(c.shape)}")
    return a, c


def merge_spectra(a, b) -> tuple:
    """the records ``(acc, counts)`` of two pieces of the same recordings, columns and plan as one: sums and counts added (raw sums, so
    the pieces of a chained replay merge; the segments that would straddle the joint are in neither piece)"""
    aa, ac = _spectra_host(*a)
    ba, bc = _spectra_host(*b)
    if aa.shape != ba.shape:
        raise UserWarning(f"merge_spectra: {tuple(aa.shape)} and {tuple(ba.shape)} records")
    return aa + ba, (ac + bc).astype(np.int32)


def summarise_spectra(acc, counts, taper, rate: float = 1.0) -> dict:
    """``(acc [..., V, n/2 + 1, W], counts [..., V, 2])`` of ``spectra`` (any leading dimensions: sets, recordings) -> a dict of float64
    arrays on the host.  ``taper``: the call's (a name or the weights; its length states ``n``).  ``rate``: frames per second; the
    clock is the frame index scaled by it -- jitter of the frames' stamps is ignored, a recording with uneven stamps is read as if
    they were even.  ``freqs [n/2 + 1]`` in Hz (cycles per frame at ``rate`` 1); ``segments [..., V]``; ``psd [..., V, n/2 + 1]``
    one-sided density, the mean over the segments of ``|X|^2 / (rate sum(w^2))``, doubled except at 0 and at ``rate / 2``
    (``scipy.signal.welch``'s density scaling).  With truth also ``truth_psd``; ``error_psd``, the density of ``x - y`` from the identity
    ``Pxx + Pyy - 2 Re Pxy``; ``coherence`` ``|Pxy|^2 / (Pxx Pyy)``; ``gain`` and ``phase`` of ``H = Pyx / Pyy``, the transfer function
    from the truth to the estimate (phase in radians, negative where the estimate trails); ``delay = -phase / (2 pi f)`` in seconds
    (frames at ``rate`` 1; NaN at 0).  NaN where no segment was summed."""
    a, c = _spectra_host(acc, counts)
    bins = a.shape[-2]
    n = 2 * (bins - 1)
    w = spectra_taper(taper, n)
    rate = float(rate)
    freqs = np.arange(bins, dtype=np.float64) * (rate / n)
    side = np.full(bins, 2.0)
    side[0] = side[-1] = 1.0
    seg = c[..., 0].astype(np.float64)
    with np.errstate(all="ignore"):
        scale = side / (rate * float((w * w).sum())) / np.where(seg > 0, seg, np.nan)[..., None]
        res = {"freqs": freqs, "segments": c[..., 0].copy(), "psd": a[..., 0] * scale}
        if a.shape[-1] == 4:
            pxx, pyy, re, im = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
            res["truth_psd"] = pyy * scale
            res["error_psd"] = (pxx + pyy - 2.0 * re) * scale
            res["coherence"] = np.where(seg[..., None] > 0, (re * re + im * im) / (pxx * pyy), np.nan)
            h = (re + 1j * im) / np.where(seg[..., None] > 0, pyy, np.nan)
            res["gain"] = np.abs(h)
            res["phase"] = np.where(np.isnan(h.real), np.nan, np.angle(h))
            res["delay"] = -res["phase"] / (2.0 * np.pi * np.where(freqs > 0, freqs, np.nan))
    return res


def bandwidth(summary: dict, level: float = 2.0 ** -0.5) -> np.ndarray:
    """``[..., V]``: the lowest frequency at which ``summary["gain"]`` falls below ``level`` (default: -3 dB), interpolated linearly
    between the last bin at or above it and the first below.  Bin 0 is not looked at (a detrended segment has no power there); NaN
    where the gain is below ``level`` from bin 1 on, never falls below it, or is NaN on the way."""
    if "gain" not in summary:
        raise UserWarning("bandwidth: a summary of spectra with truth")
    g, f = np.asarray(summary["gain"], dtype=np.float64), np.asarray(summary["freqs"], dtype=np.float64)
    out = np.full(g.shape[:-1], np.nan)
    for at in np.ndindex(*g.shape[:-1]):
        row = g[at]
        for k in range(2, row.shape[0]):
            if not (row[k - 1] >= level):
                break
            if row[k] < level:
                out[at] = f[k - 1] + (row[k - 1] - level) / (row[k - 1] - row[k]) * (f[k] - f[k - 1])
                break
            if np.isnan(row[k]):
                break
    return out


def band_power(summary: dict, lo: float, hi: float, key: str = "psd") -> np.ndarray:
    """``[..., V]``: the power of ``summary[key]`` in the band ``lo <= f < hi``, the density times the bin width summed over the band's
    bins (voluntary motion: below about 2 Hz; tremor and sensor shake: 4 - 12 Hz)"""
    f = np.asarray(summary["freqs"], dtype=np.float64)
    d = np.asarray(summary[key], dtype=np.float64)
    pick = (f >= float(lo)) & (f < float(hi))
    return d[..., pick].sum(axis=-1) * (f[1] - f[0])


def pose_spectra(layout: int, out, truth=None, truth_kind: str = "est", starts=None, skip: int = 0, bodies=None, n: int = 256, hop=None,
                 taper="hann", detrend: bool = True):
    """``spectra`` of the six hand and elbow position columns (``pose_cols``, ``POSE_COL_NAMES``) of messages ``out [(C,) F, >= 25]``
    against those of ``truth``: device est rows ``[F, 21 | 14]``, or with ``truth_kind="targets"`` de-normalised NN targets ``[F, O]``,
    which ``resample_truth`` turns into est rows on the device (the frames' own index clock, no shift: every row is an exact hit; the
    recordings' ``bodies``).  Returns ``spectra``'s ``(acc, counts)``."""
    if truth_kind not in TRUTH_KINDS:
        raise UserWarning(f"truth_kind must be one of {sorted(TRUTH_KINDS)}, got {truth_kind!r}")
    if truth is not None and truth_kind == "targets":
        truth = resample_truth(layout, truth, "targets", starts, None, None, int(out.shape[-2]), starts, None, 0.0, bodies)
    return spectra(out, truth, pose_cols(layout, "msg"), None if truth is None else pose_cols(layout, "est"), n, hop, taper, detrend, starts,
                   skip)


# ---- the output layer fitted to a wearer (the reference has no counterpart) ---------------------------------------------
FIT_PIECE, FIT_MAX_P, FIT_MAX_Q = _hip.FIT_PIECE, _hip.FIT_MAX_P, _hip.FIT_MAX_Q


def _fit_affine(shift, scale, Q: int):
    """(shift, scale) float64 ``[Q]`` or None each: finite, the scale not zero"""
    out = []
    for name, v in (("shift", shift), ("scale", scale)):
        if v is None:
            out.append(None)
            continue
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
        if a.shape[0] != Q or not np.isfinite(a).all() or (name == "scale" and (a == 0.0).any()):
            raise UserWarning(f"{name}: {Q} finite values" + (", none of them zero" if name == "scale" else ""))
        out.append(a)
    return out


def _fit_lags(rec_lags, R: int):
    if rec_lags is None:
        return None
    l = np.ascontiguousarray(np.asarray(rec_lags, dtype=np.int32).reshape(-1))
    if l.shape[0] != R:
        raise UserWarning(f"rec_lags: one lag per recording ({R}), got {l.shape[0]}")
    return l


def fit_sums_numpy(x, t, starts=None, skip: int = 0, rec_lags=None, shift=None, scale=None) -> np.ndarray:
    """The host statement of ``fit_sums``, the order of the pieces included: float64 ``[R, M * M + 2]``, ``M = P + 1 + Q``.  Per
    recording ``[s, e)`` with lag ``l`` the support is the frames ``f >= s + skip`` with ``s <= f - l < e``; ``z_f = [x_f, 1,
    (t_{f-l} - shift) / scale]`` in float64, a row of zeros where any of the pair's ``P + Q`` values is not finite (or a truth value
    overflows under shift and scale); the support is cut into pieces of ``FIT_PIECE`` frames from its first, a piece's sums are
    ``Z'Z`` (the device chains fused multiply-adds in frame order: another order of the same terms), the pieces are added in order
    from ``+0.0``, and ``(j, i)`` is a copy of ``(i, j)``.  ``[M * M]``, ``[M * M + 1]``: pairs summed and left out."""
    xa, ta = np.asarray(x), np.asarray(t)
    if xa.ndim != 2 or ta.ndim != 2 or xa.shape[0] != ta.shape[0] or min(xa.shape) < 1 or min(ta.shape) < 1:
        raise UserWarning(f"x and t: expected [F, P] and [F, Q], got {tuple(xa.shape)} and {tuple(ta.shape)}")
    xa, ta = xa.astype(np.float64), ta.astype(np.float64)
    F, P, Q = xa.shape[0], xa.shape[1], ta.shape[1]
    M = P + 1 + Q
    sh, sc = _fit_affine(shift, scale, Q)
    st = _recording_starts(starts).astype(np.int64)
    R = st.shape[0]
    lags = _fit_lags(rec_lags, R)
    ends = np.r_[st[1:], F]
    out = np.zeros((R, M * M + 2))
    iu = np.triu_indices(M, 1)
    with np.errstate(all="ignore"):
        for r in range(R):
            s, e, l = int(st[r]), int(ends[r]), int(lags[r]) if lags is not None else 0
            lo, up = s + max(int(skip), l), e + min(0, l)
            if up <= lo:
                continue
            f = np.arange(lo, up)
            tt = ta[f - l]
            tz = (tt - (0.0 if sh is None else sh)) / (1.0 if sc is None else sc)
            ok = np.isfinite(xa[f]).all(axis=1) & np.isfinite(tt).all(axis=1) & np.isfinite(tz).all(axis=1)
            Z = np.concatenate([xa[f], np.ones((f.shape[0], 1)), tz], axis=1)
            Z[~ok] = 0.0
            G = np.zeros((M, M))
            for p0 in range(0, Z.shape[0], FIT_PIECE):
                Zp = Z[p0:p0 + FIT_PIECE]
                G = G + Zp.T @ Zp
            G[iu[1], iu[0]] = G[iu]
            out[r, :M * M] = G.reshape(-1)
            out[r, M * M], out[r, M * M + 1] = ok.sum(), (~ok).sum()
    return out


def _fit_view(t, what: str):
    """(tensor, F, W, frame stride in elements) of a device view ``[F, W]`` whose last dimension is contiguous; anything else is copied"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2 or min(t.shape) < 1:
        raise UserWarning(f"{what}: expected a device tensor [F, W]")
    if t.dtype not in (torch.float32, torch.float64):
        raise UserWarning(f"{what}: float32 or float64, got {t.dtype}")
    F, W = (int(n) for n in t.shape)
    fs, ws = (int(v) for v in t.stride())
    if (W > 1 and ws != 1) or (F > 1 and fs < W):
        t = t.contiguous()
        fs = W
    return t, F, W, max(fs, W)


def fit_sums(x, t, starts=None, skip: int = 0, rec_lags=None, shift=None, scale=None):
    """The normal-equation sums of ``[x, 1, (t - shift) / scale]`` per recording on the float64 matrix cores (``ape_fit_sums``).  ``x``: a
    device ``[F, P]`` view, ``P`` a multiple of 16 up to 256 (the hidden features); ``t``: ``[F, Q]``, ``Q <= 32`` (the truth targets);
    float32 or float64 per side, column slices of wider rows go in without a copy.  ``starts``, ``skip``: the recordings and their
    cold-start frames, as in ``score_rows``; ``rec_lags``: one lag per recording, ``x`` row ``f`` goes with ``t`` row ``f - l`` (as
    ``best_lag`` finds it); ``shift``, ``scale``: float64 ``[Q]``, an estimator's ``yy_m`` / ``yy_s``.  Returns float64
    ``[R, M * M + 2]`` on the device (``fit_sums_numpy`` states the layout and the order): the same inputs give the same bits, a
    recording's record does not depend on the batch around it.  The call does not wait for the device."""
    xv, F, P, xs = _fit_view(x, "x")
    tv, Ft, Q, ts = _fit_view(t, "t")
    if F != Ft or xv.device != tv.device:
        raise UserWarning(f"x {tuple(x.shape)} and t {tuple(t.shape)}: the same frames on one device")
    sh, sc = _fit_affine(shift, scale, Q)
    st = _recording_starts(starts)
    R = int(st.shape[0])
    lags = _fit_lags(rec_lags, R)
    M = P + 1 + Q
    dev = xv.device
    with torch.cuda.device(dev):
        acc = torch.empty((max(R, 1), M * M + 2), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(_hip.lib().ape_fit_sums(C.c_void_p(xv.data_ptr()), xs, _f64(xv.dtype), P, C.c_void_p(tv.data_ptr()), ts, _f64(tv.dtype), Q,
                                           C.c_void_p(sh.ctypes.data) if sh is not None else None,
                                           C.c_void_p(sc.ctypes.data) if sc is not None else None, F, C.c_void_p(st.ctypes.data), R,
                                           int(skip), C.c_void_p(lags.ctypes.data) if lags is not None else None,
                                           C.c_void_p(acc.data_ptr()), stream), "ape_fit_sums")
    return acc


def _fit_host(sums) -> tuple:
    """(records float64 ``[R, M * M + 2]``, M) of ``fit_sums``' result or one record of it"""
    a = sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    a = np.asarray(a, dtype=np.float64)
    a = a[None] if a.ndim == 1 else a
    M = math.isqrt(max(a.shape[-1] - 2, 0)) if a.ndim == 2 else 0
    if a.ndim != 2 or M < 3 or M * M + 2 != a.shape[-1]:
        raise UserWarning(f"expected fit records [R, M * M + 2], got {tuple(a.shape)}")
    return a, M


def merge_fit(a, b) -> np.ndarray:
    """the records of two pieces of the same recordings as one (float64, on the host): every sum and both counts added.  For a
    recording cut at a multiple of ``FIT_PIECE`` frames of its support whose second piece is at most ``FIT_PIECE`` frames long these are
    the bits of the one call (its pieces, folded in the same order); otherwise another order of the same terms."""
    x, Ma = _fit_host(a)
    y, Mb = _fit_host(b)
    if x.shape != y.shape:
        raise UserWarning(f"merge_fit: {tuple(x.shape)} and {tuple(y.shape)} records")
    with np.errstate(all="ignore"):
        return x + y


def _fit_blocks(rec, M: int, P: int):
    """(A [P + 1, P + 1], C [P + 1, Q], T [Q, Q], n) of one record: the blocks of ``[x, 1]`` against itself, against ``t``, ``t't``"""
    G = rec[:M * M].reshape(M, M)
    return G[:P + 1, :P + 1], G[:P + 1, P + 1:], G[P + 1:, P + 1:], float(rec[M * M])


def _fit_prior(prior_w, prior_b, M: int):
    w = np.asarray(prior_w.detach().cpu().numpy() if isinstance(prior_w, torch.Tensor) else prior_w, dtype=np.float64)
    b = np.asarray(prior_b.detach().cpu().numpy() if isinstance(prior_b, torch.Tensor) else prior_b, dtype=np.float64).reshape(-1)
    if w.ndim != 2 or w.shape[0] != b.shape[0] or w.shape[0] + w.shape[1] + 1 != M:
        raise UserWarning(f"prior head: w [Q, P] and b [Q] with P + 1 + Q = {M}, got {tuple(w.shape)} and {tuple(b.shape)}")
    return w, b


def _fit_sse(A, Cx, T, theta) -> np.ndarray:
    """per-column sum of squared residuals of ``theta [P + 1, Q]`` from the sums alone: ``t't - 2 theta'C + theta'A theta`` (diagonals)"""
    return np.diag(T) - 2.0 * np.einsum("iq,iq->q", theta, Cx) + np.einsum("iq,ij,jq->q", theta, A, theta)


def _fit_pool(a, M: int, keep) -> np.ndarray:
    rec = np.zeros(M * M + 2)
    for r in keep:                                      # in recording order, from +0.0
        rec = rec + a[r]
    return rec


def price_head(sums, w, b, recordings=None) -> tuple:
    """``(rmse [Q], n)`` of the head ``(w [Q, P], b [Q])`` over the listed recordings' records (default: all), from the sums alone:
    ``sqrt(max(0, SSE) / n)`` per column, in the units of the fitted targets (``fit_sums``' shift and scale); NaN without a pair."""
    a, M = _fit_host(sums)
    wv, bv = _fit_prior(w, b, M)
    P = wv.shape[1]
    keep = range(a.shape[0]) if recordings is None else [int(r) for r in recordings]
    A, Cx, T, n = _fit_blocks(_fit_pool(a, M, keep), M, P)
    theta = np.concatenate([wv.T, bv[None]], axis=0)
    with np.errstate(all="ignore"):
        return (np.sqrt(np.maximum(_fit_sse(A, Cx, T, theta), 0.0) / n) if n > 0 else np.full(wv.shape[0], np.nan)), int(n)


def best_head(sums, prior_w, prior_b, ridge: float = 0.0, leave_out=None, min_pairs=None) -> tuple:
    """The output layer that fits the recordings best, read off ``fit_sums``' records ``[R, M * M + 2]``: ``(w [Q, P], b [Q], report)``
    in float64.  Over the sum of the records of all recordings but those listed in ``leave_out``, with ``A`` the sums of ``[x, 1]``
    against itself, ``C`` against ``t`` and ``n`` the pairs summed, it solves ``(A + ridge n D) Theta = C + ridge n D Theta0`` for
    ``Theta = [W'; b']``: ``Theta0`` is the prior head ``(prior_w [Q, P], prior_b [Q])``, ``D = diag(1, .., 1, 0)`` -- the bias is not
    penalised, the penalty pulls the weights towards the present head.  ``ridge = inf``: the prior's weights with the bias that fits.
    ``report``: ``pairs``; ``rmse_prior`` and ``rmse_fit`` ``[Q]`` from the sums alone (``price_head``); ``cond`` of the matrix solved;
    ``ridge``; ``refused`` with ``reason``.  Refused -- the prior is returned -- with fewer than ``2 (P + 1)`` pairs (``min_pairs``
    states another floor: under a ridge the system is definite with fewer pairs than unknowns, at the caller's risk), a sum that is not
    finite, or a matrix that is not positive definite (no Cholesky factor, a pivot within ``(P + 1) eps`` of its diagonal entry, or a
    solution that is not finite)."""
    a, M = _fit_host(sums)
    w0, b0 = _fit_prior(prior_w, prior_b, M)
    Q, P = w0.shape
    if not (ridge >= 0.0):
        raise UserWarning("ridge: a value >= 0 (inf: the prior's weights)")
    out = set(int(r) for r in ([] if leave_out is None else leave_out))
    if any(r < 0 or r >= a.shape[0] for r in out):
        raise UserWarning(f"leave_out: recordings of 0 .. {a.shape[0] - 1}")
    rec = _fit_pool(a, M, [r for r in range(a.shape[0]) if r not in out])
    A, Cx, T, n = _fit_blocks(rec, M, P)
    theta0 = np.concatenate([w0.T, b0[None]], axis=0)
    nan = np.full(Q, np.nan)
    report = {"pairs": int(n) if np.isfinite(n) else 0, "rmse_prior": nan, "rmse_fit": nan, "cond": float("nan"), "ridge": float(ridge),
              "refused": True, "reason": None}

    def refuse(reason):
        report["reason"] = reason
        report["rmse_fit"] = report["rmse_prior"]
        return w0.copy(), b0.copy(), report

    if not np.isfinite(rec).all():
        return refuse("a sum is not finite")
    with np.errstate(all="ignore"):
        if n > 0:
            report["rmse_prior"] = np.sqrt(np.maximum(_fit_sse(A, Cx, T, theta0), 0.0) / n)
        floor = 2 * (P + 1) if min_pairs is None else max(1, int(min_pairs))
        if n < floor:
            return refuse(f"{int(n)} pairs, fewer than " + (f"2 (P + 1) = {floor}" if min_pairs is None else f"min_pairs = {floor}"))
        if np.isinf(ridge):                             # the weights stay; the bias that fits them: sum t - W sum x over n
            theta = theta0.copy()
            theta[P] = (Cx[P] - w0 @ A[:P, P]) / n
            report["cond"] = 1.0
        else:
            D = np.ones(P + 1)
            D[P] = 0.0
            Ms = A + np.diag(ridge * n * D)
            rhs = Cx + (ridge * n * D)[:, None] * theta0
            try:
                Lc = np.linalg.cholesky(Ms)
            except np.linalg.LinAlgError:
                return refuse("the matrix is not positive definite")
            if (np.diag(Lc) ** 2 <= (P + 1) * np.finfo(np.float64).eps * np.diag(Ms)).any():
                return refuse("the matrix is not positive definite to working precision (a pivot at the rounding of its diagonal)")
            theta = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))
            if not np.isfinite(theta).all():
                return refuse("the matrix is not positive definite (no finite solution)")
            report["cond"] = float(np.linalg.cond(Ms))
        report["rmse_fit"] = np.sqrt(np.maximum(_fit_sse(A, Cx, T, theta), 0.0) / n)
    report["refused"] = False
    return np.ascontiguousarray(theta[:P].T), theta[P].copy(), report


def sweep_ridge(sums, prior_w, prior_b, ridges, min_pairs=None) -> tuple:
    """Leave-one-recording-out prices of ridges, from the sums alone: for every ridge and recording ``r`` the head fitted on all records
    but ``r`` (``best_head(leave_out=[r], min_pairs=min_pairs)``; a refused fit is the prior) is priced on record ``r``, the squared residuals are pooled over
    the recordings that have pairs.  Returns ``(rmse [len(ridges), Q], prior_rmse [Q])``: the held-out RMSE per ridge and column and
    that of the prior head over the same pairs, which no ridge enters."""
    a, M = _fit_host(sums)
    w0, b0 = _fit_prior(prior_w, prior_b, M)
    Q, P = w0.shape
    rs = [float(v) for v in np.asarray(ridges, dtype=np.float64).reshape(-1)]
    R = a.shape[0]
    if R < 2:
        raise UserWarning("sweep_ridge: at least two recordings")
    theta0 = np.concatenate([w0.T, b0[None]], axis=0)
    blocks = [_fit_blocks(a[r], M, P) for r in range(R)]
    held = [r for r in range(R) if np.isfinite(a[r]).all() and blocks[r][3] > 0]
    total = sum(blocks[r][3] for r in held)
    if not held:
        raise UserWarning("sweep_ridge: no recording has a pair")
    with np.errstate(all="ignore"):
        prior_sse = np.zeros(Q)
        for r in held:
            prior_sse = prior_sse + _fit_sse(*blocks[r][:3], theta0)
        out = np.zeros((len(rs), Q))
        for k, ridge in enumerate(rs):
            sse = np.zeros(Q)
            for r in held:
                w, b, _ = best_head(a, w0, b0, ridge, leave_out=[r], min_pairs=min_pairs)
                sse = sse + _fit_sse(*blocks[r][:3], np.concatenate([w.T, b[None]], axis=0))
            out[k] = np.sqrt(np.maximum(sse, 0.0) / total)
        return out, np.sqrt(np.maximum(prior_sse, 0.0) / total)
