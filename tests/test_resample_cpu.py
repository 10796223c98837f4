"""Mocap truth on each frame's clock without a GPU: the numpy statements `score.frame_times_numpy`, `score._slerp` and
`score.resample_truth_numpy`, planted fractional lags and a planted shift between two clocks, the refusals of `ape_frame_times` and
`ape_resample_truth` that need no device (all are made on the host; the capturing stream is refused in tests/test_resample_gpu.py), the
header and the binding.

Bounds.  The quaternion statement against the closed form `a (x) delta^w` and against scipy: 1e-14, room for another order of
operations and nothing more (measured figures: profiles/resample.md).  `refined` within 0.01 frame of the plant; the hand RMS
of the refined pass at most 0.1 x the integer-lag RMS; on two clocks the RMS at the planted shift at most 0.01 x the RMS at shift 0.
The builders and the host chain of `align(refine=True)` are shared with tests/test_resample_gpu.py."""
import ctypes as C
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from tests.test_score_lags_cpu import F, FPS, HIPS, LAGS, POS, SKIP, STARTS, WATCH, msgs_from_est, trajectory

REPO = Path(__file__).resolve().parents[1]
ENDS = STARTS[1:] + [F]
TIME_STARTS, TIME_F = [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 2049], 3000     # one-frame recordings, boundaries on wave and tile edges


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---------------- builders shared with the GPU tests -----------------------------------------------------------------------------------------
def exact_dt(n=TIME_F, seed=11):
    """float32 dt in [2^-8, 2^-3]: values on a grid of 2^-31 below 2^-3, so up to 2^16 of them add without rounding in float64"""
    return np.random.default_rng(seed).uniform(2.0 ** -8, 2.0 ** -3, size=n).astype(np.float32)


def partial_sums_are_exact(dt, starts):
    """every partial sum of every recording, as a fraction, is a float64: then any association gives the same bits"""
    ends = list(starts[1:]) + [len(dt)]
    for s, e in zip(starts, ends):
        assert e - s <= 2 ** 16
        total = Fraction(0)
        for v in dt[s + 1:e]:
            total += Fraction(float(v))
            if Fraction(float(total)) != total:
                return False
    return True


def jittered_dt(n, seed=5):
    """float32 sw_dt in [0.012, 0.03] s: a watch's jittered clock"""
    return np.random.default_rng(seed).uniform(0.012, 0.03, size=n).astype(np.float32)


def truth_clock(duration, hz=120.0, jitter=0.0, seed=9):
    """stamps of a mocap system at `hz` from 0 to past `duration`, each moved by up to `jitter` of a period (still strictly rising)"""
    n = int(np.ceil(duration * hz)) + 2
    t = np.arange(n, dtype=np.float64) / hz
    if jitter:
        t[1:] += np.random.default_rng(seed).uniform(-jitter, jitter, size=n - 1) / hz
    return t


def two_clock_case(layout=HIPS, n=F, shift=0.137, seed=0):
    """(msg [n, 25], frame times [n], dt float32 [n], truth est rows, truth times): the estimate is late by `shift` seconds"""
    from wear_mocap_ape_amd.score import frame_times_numpy
    dt = jittered_dt(n)
    tq = frame_times_numpy(dt)
    tt = truth_clock(tq[-1])
    truth = trajectory(tt * FPS, layout, seed)
    msg = msgs_from_est(trajectory((tq - shift) * FPS, layout, seed), layout)
    return msg, tq, dt, truth, tt


def hand_rms(msg, truth_est, layout, starts=None, skip=0):
    """per recording the RMS of the hand error over the scorable frames past `skip`, and their number"""
    from wear_mocap_ape_amd.score import accumulate_numpy, score_rows_numpy
    acc = accumulate_numpy(score_rows_numpy(msg, truth_est, layout), starts, skip)
    with np.errstate(all="ignore"):
        return np.sqrt(acc[:, 1] / acc[:, 15]), acc[:, 15]


def refined_chain_numpy(msg, truth, layout, lags, starts, skip, spread=None, shifts=None):
    """the host chain of `align(refine=True)` for est-kind truth: sweep, `best_lag`, the truth resampled at `refined` (or at `shifts`),
    scored and accumulated -> (best, rows [F, 7], acc [R, 25])"""
    from wear_mocap_ape_amd import score
    _, sweep = score.score_lags_numpy(msg, truth, layout, lags, starts, skip, spread)
    best = score.best_lag(sweep, lags)
    if shifts is None:
        shifts = [0.0 if b["lag"] is None else b["refined"] for b in best]
    moved = score.resample_truth_numpy(layout, truth, starts, None, None, truth.shape[0], starts, shifts)
    rows = score.score_rows_numpy(msg, moved, layout, spread)
    return best, rows, score.accumulate_numpy(rows, starts, skip)


# ---------------- 1: declarations --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_hip_binds_both_entries():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    want = {"ape_frame_times": ["const void* dt_dev", "int32_t dt_stride", "int32_t dt_dtype", "uint32_t flags", "int32_t F",
                                "const int32_t* seg_starts_host", "int32_t R", "double* times_dev", "void* stream"],
            "ape_resample_truth": ["int32_t layout", "const void* truth_dev", "int32_t truth_kind", "int32_t truth_dtype", "int32_t Ft",
                                   "const int32_t* truth_starts_host", "const double* truth_times_dev", "const double* times_dev",
                                   "int32_t F", "const int32_t* seg_starts_host", "int32_t R", "const double* shift_host", "double max_gap",
                                   "const double* bodies_host", "int32_t n_bodies", "void* out_dev", "int32_t out_dtype", "void* stream"]}
    for name, params in want.items():
        decl = text[text.index(f"\nint {name}(") + 1:]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        got = [" ".join(p.split()) for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
        assert got == params, (name, got)
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name) and len(_hip.SIGNATURES[name][1]) == len(params)
    assert _hip.SIGNATURES["ape_resample_truth"][1][12] is C.c_double
    assert "resample.hip" in (REPO / "arm-pose-estimation_amd" / "csrc" / "Makefile").read_text()
    for name in ("frame_times", "frame_times_numpy", "resample_truth", "resample_truth_numpy", "truth_on_frames", "align"):
        assert callable(getattr(score, name))
    import inspect
    assert inspect.signature(score.align).parameters["refine"].default is False
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    assert all("truth_on_frames" in vars(cls) for cls in (Estimator, WatchPhoneUarm, WatchPhonePocketKalman))


# ---------------- 2: the quaternion statement --------------------------------------------------------------------------------------------------
def _qmul(a, b):
    w1, x1, y1, z1 = (a[..., k] for k in range(4))
    w2, x2, y2, z2 = (b[..., k] for k in range(4))
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=-1)


def _pairs(n=20000, seed=21):
    """a, b = +-(a (x) delta), the closed form a (x) delta^w, the rotation angles of delta (log-uniform in [1e-9, 0.999 pi]) and w"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 4))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    phi = np.exp(rng.uniform(np.log(1e-9), np.log(0.999 * np.pi), size=n))
    phi[:4] = [1e-9, 0.999 * np.pi, 2e-6, 1.9e-6]                     # the ends, and the two sides of the chord / arc switch (theta = phi / 2)
    w = rng.uniform(0.0, 1.0, size=n)
    rot = lambda ang: np.concatenate([np.cos(ang / 2)[:, None], axis * np.sin(ang / 2)[:, None]], axis=1)     # noqa: E731
    b = _qmul(a, rot(phi)) * rng.choice([-1.0, 1.0], size=(n, 1))
    return a, b, _qmul(a, rot(w * phi)), phi, w


def _aligned_gap(q, ref):
    s = np.where((q * ref).sum(axis=1) < 0.0, -1.0, 1.0)[:, None]
    return np.abs(q - s * ref).max(axis=1)


def test_quaternion_statement_against_the_closed_form_and_scipy():
    from scipy.spatial.transform import Rotation, Slerp
    from wear_mocap_ape_amd.score import _slerp
    a, b, closed, phi, w = _pairs()
    q = _slerp(a, b, w)
    assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() <= 4e-16
    gap = _aligned_gap(q, closed)
    print(f"statement vs closed form: max {gap.max():.3e} over {len(w)} pairs, angles {phi.min():.1e} .. {phi.max():.4f}")
    assert gap.max() <= 1e-14
    # unnormalised inputs are normalised first; the ends return the ends
    scale = np.random.default_rng(3).uniform(0.5, 2.0, size=(len(w), 2))
    assert _aligned_gap(_slerp(a * scale[:, :1], b * scale[:, 1:], w), closed).max() <= 1e-14
    assert _aligned_gap(_slerp(a, b, np.zeros_like(w)), a).max() <= 1e-15 and _aligned_gap(_slerp(a, b, np.ones_like(w)), b).max() <= 1e-15
    # scipy's Slerp for angles >= 1e-3, one object per pair on the key times 0 and 1 (one long key axis would state the weight as
    # 2 k + w and lose its last digits: 1e-12 at k ~ 7000)
    big = np.flatnonzero(phi >= 1e-3)
    xyzw = [1, 2, 3, 0]
    got = np.stack([Slerp([0.0, 1.0], Rotation.from_quat(np.stack([a[k, xyzw], b[k, xyzw]])))([w[k]]).as_quat()[0] for k in big])
    gap = _aligned_gap(q[big], got[:, [3, 0, 1, 2]])
    print(f"statement vs scipy Slerp: max {gap.max():.3e} over {len(big)} pairs")
    assert gap.max() <= 1e-14


# ---------------- 3: the seven rules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_integer_shifts_on_the_index_clock_give_the_rows_themselves(layout):
    from wear_mocap_ape_amd.score import resample_truth_numpy
    truth = trajectory(np.arange(F), layout)
    truth[[10, 100, 400], [1, 7, 13]] = np.nan                          # an exact hit returns the row as it is, NaN included
    shifts = [0, 3, -2, 7, 1, -40]
    out = resample_truth_numpy(layout, truth, STARTS, None, None, F, STARTS, shifts)
    assert out.shape == truth.shape
    for (s, e), l in zip(zip(STARTS, ENDS), shifts):
        f = np.arange(s, e)
        inside = (f - l >= s) & (f - l < e)
        assert same(out[f[inside]], truth[f[inside] - l]) and np.isnan(out[f[~inside]]).all(), (s, l)
        assert inside.sum() == max(0, e - s - abs(l))
    assert np.isnan(out[13, 1]) and np.isfinite(out[13, 0]) and np.isnan(out[STARTS[1]:STARTS[1] + 3]).all()      # truth row 10 at lag 3
    # one shift for all recordings, no shift, and a float32 truth widened exactly
    assert same(resample_truth_numpy(layout, truth, STARTS, None, None, F, STARTS, 0.0), truth)
    assert same(resample_truth_numpy(layout, truth, STARTS, None, None, F, STARTS), truth)
    t32 = truth.astype(np.float32)
    assert same(resample_truth_numpy(layout, t32, STARTS, None, None, F, STARTS, shifts), out.astype(np.float32).astype(np.float64))


def test_rules_one_case_each():
    from wear_mocap_ape_amd.score import _slerp, resample_truth_numpy
    truth = trajectory(np.arange(8))
    tt = np.array([0.0, 0.1, 0.2, 0.2, 0.2, 0.5, 0.6, 0.7])           # duplicate stamps at rows 2-4, a dropout between rows 4 and 5
    run = lambda tq, t=truth, **kw: resample_truth_numpy(HIPS, t, None, tt, np.asarray(tq, dtype=np.float64), **kw)      # noqa: E731
    # 1: a non-finite query
    out = run([np.nan, np.inf, -np.inf, 0.1])
    assert np.isnan(out[:3]).all() and same(out[3], truth[1])
    # 2: nothing at or before the query
    assert np.isnan(run([-1e-9])).all() and same(run([0.0])[0], truth[0])
    # 3, 4: an exact hit on the last sample is kept, anything past it is NaN
    out = run([0.7, np.nextafter(0.7, 1.0), 5.0])
    assert same(out[0], truth[7]) and np.isnan(out[1:]).all()
    # duplicate stamps take the last: an exact hit returns row 4, and the pair bridged after 0.2 is (4, 5)
    out = run([0.2, 0.35])
    assert same(out[0], truth[4])
    assert np.abs(out[1, :9] - (truth[4, :9] + 0.5 * (truth[5, :9] - truth[4, :9]))).max() <= 1e-15
    assert np.abs(out[1, 9:13] - _slerp(truth[4:5, 9:13], truth[5:6, 9:13], np.array([0.5]))[0]).max() <= 1e-15
    # ... and before it (3 is not used: the search ends on row 1 for a query inside (0.1, 0.2))
    w = (0.15 - tt[1]) / (tt[2] - tt[1])
    assert np.array_equal(run([0.15])[0, :9], truth[1, :9] + w * (truth[2, :9] - truth[1, :9]))
    # 5: max_gap -- the dropout of 0.3 s is not bridged at 0.25 but is at 0.35; ordinary gaps of 0.1 s pass; exact hits pass
    out = run([0.35, 0.05, 0.5, 0.2], max_gap=0.25)
    assert np.isnan(out[0]).all() and np.isfinite(out[1]).all() and same(out[2], truth[5]) and same(out[3], truth[4])
    assert np.isfinite(run([0.35], max_gap=0.35)).all() and np.isfinite(run([0.35], max_gap=0.0)).all()
    # 6: a NaN in either neighbour (any column, the shoulder origin included); 3: a NaN row returned as it is on an exact hit
    for row, col in ((5, 0), (6, 12), (5, 7), (6, 20)):
        bad = truth.copy()
        bad[row, col] = np.nan
        out = run([0.55, 0.65, 0.45, 0.5, 0.6], t=bad)
        assert np.isnan(out[0]).all() and np.isnan(out[1]).all() == (row == 6) and np.isnan(out[2]).all() == (row == 5)
        assert same(out[3], bad[5]) and same(out[4], bad[6]) and np.isnan(out[3:, col]).sum() == 1
    # 7: the weights, on a clock that is not uniform; every quaternion comes out normalised
    out = run([0.525, 0.69])
    assert np.array_equal(out[0, :9], truth[5, :9] + ((0.525 - 0.5) / (0.6 - 0.5)) * (truth[6, :9] - truth[5, :9]))
    for c in (9, 13, 17):
        assert np.abs(np.linalg.norm(out[:, c:c + 4], axis=1) - 1.0).max() <= 4e-16
    # frame times need not be monotonic; recordings search their own rows only
    out = resample_truth_numpy(HIPS, truth, [0, 5], np.array([0.0, 0.1, 0.2, 0.3, 0.4, 0.0, 0.1, 0.2]), np.array([0.2, 0.0, 0.1, 0.2, 9.0]),
                               None, [0, 2], [0.0, 0.1])
    assert same(out[0], truth[2]) and same(out[1], truth[0]) and same(out[2], truth[5]) and same(out[3], truth[6]) and np.isnan(out[4]).all()
    for bad in (lambda: resample_truth_numpy(HIPS, truth), lambda: resample_truth_numpy(3, truth, frames=8),
                lambda: resample_truth_numpy(WATCH, truth, frames=8), lambda: resample_truth_numpy(HIPS, truth, [0, 4], frames=8)):
        with pytest.raises(UserWarning):
            bad()


# ---------------- 4: the clock -------------------------------------------------------------------------------------------------------------------
def test_frame_times_statement_and_the_exactness_of_its_inputs():
    from wear_mocap_ape_amd.score import frame_times_numpy
    dt = exact_dt()
    assert dt.dtype == np.float32 and dt.min() >= 2.0 ** -8 and dt.max() <= 2.0 ** -3
    assert partial_sums_are_exact(dt, TIME_STARTS)
    long = exact_dt(2 ** 16, seed=12)
    assert partial_sums_are_exact(long, [0])                            # the longest recording the precondition is stated for
    assert not partial_sums_are_exact(np.full(4, 0.1, dtype=np.float64), [0])      # (the check itself can fail)
    t = frame_times_numpy(dt, TIME_STARTS)
    ends = TIME_STARTS[1:] + [TIME_F]
    for s, e in zip(TIME_STARTS, ends):
        assert t[s] == 0.0
        for f in (s + 1, (s + e) // 2, e - 1):
            if s < f < e:
                assert Fraction(float(t[f])) == sum((Fraction(float(v)) for v in dt[s + 1:f + 1]), Fraction(0)), (s, f)
    # the first row's dt is not read; a NaN stays inside its recording
    dt2 = dt.copy()
    dt2[TIME_STARTS] = np.nan
    assert np.array_equal(frame_times_numpy(dt2, TIME_STARTS), t)
    dt2 = dt.copy()
    dt2[300] = np.nan
    t2 = frame_times_numpy(dt2, TIME_STARTS)
    assert np.isnan(t2[300:1023]).all() and np.array_equal(np.delete(t2, np.arange(300, 1023)), np.delete(t, np.arange(300, 1023)))
    assert np.array_equal(frame_times_numpy(dt[:1]), [0.0]) and np.array_equal(frame_times_numpy(dt[:3]), [0.0, float(dt[1]), float(dt[1]) + float(dt[2])])


# ---------------- 5: refinement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", [2.5, 3.3, -1.75])
def test_refined_lag_removes_the_sampling_error(plant):
    idx = np.arange(F)
    truth = trajectory(idx)
    msg = msgs_from_est(trajectory(idx - plant), HIPS)
    best, rows, acc = refined_chain_numpy(msg, truth, HIPS, LAGS, STARTS, SKIP)
    assert best[0]["lag"] is None and acc[0, 15] == 0
    with np.errstate(all="ignore"):
        rms = np.sqrt(acc[:, 1] / acc[:, 15])
    for r in range(1, 6):
        print(f"plant {plant}, recording {r}: lag {best[r]['lag']}, refined {best[r]['refined']:.5f}, hand rms {1e3 * best[r]['rms']:.2f} mm at "
              f"the integer lag, {1e3 * rms[r]:.3f} mm refined ({rms[r] / best[r]['rms']:.3f})")
    for r in range(1, 6):
        assert abs(best[r]["refined"] - plant) <= 0.01, (r, best[r])
        assert acc[r, 15] >= ENDS[r] - STARTS[r] - SKIP - 4 and rms[r] <= 0.1 * best[r]["rms"], (r, rms[r], best[r]["rms"])


# ---------------- 6: two clocks ------------------------------------------------------------------------------------------------------------------------
def test_two_clocks_with_a_planted_shift_in_seconds():
    from wear_mocap_ape_amd.score import resample_truth_numpy
    shift = 0.137
    msg, tq, dt, truth, tt = two_clock_case(shift=shift)
    assert dt.dtype == np.float32 and dt.min() >= 0.012 and dt.max() <= 0.03 and abs(1.0 / np.diff(tt).mean() - 120.0) < 1e-9
    at0, n0 = hand_rms(msg, resample_truth_numpy(HIPS, truth, None, tt, tq), HIPS)
    at, n = hand_rms(msg, resample_truth_numpy(HIPS, truth, None, tt, tq, shifts=shift), HIPS)
    print(f"hand rms {1e3 * at0[0]:.1f} mm unshifted, {1e3 * at[0]:.3f} mm at the shift ({at[0] / at0[0]:.2e})")
    assert n0[0] == F and F - 12 <= n[0] < F                            # the first 0.137 s of frames lie before the truth
    assert at[0] <= 0.01 * at0[0]


# ---------------- 7: the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_frame_times_refusals_are_made_on_the_host():
    """every refusal include/ape_hip.h states but the capturing stream (tests/test_resample_gpu.py): APE_ERR_INVALID_ARG before any device
    call (the pointers are never read)"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy, other = C.c_void_p(256), C.c_void_p(4096)

    def call(dt=dummy, stride=1, dtype=_hip.F32, flags=0, F=10, starts=(0, 3, 7), out=other, R=None):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        return lib.ape_frame_times(dt, stride, dtype, flags, F, C.c_void_p(st.ctypes.data) if len(st) else None, len(st) if R is None else R, out, None)

    bad = [(dict(dt=None), b"NULL"), (dict(out=None), b"NULL"), (dict(starts=()), b"NULL"), (dict(F=0), b"F=0"), (dict(F=-3), b"F=-3"),
           (dict(R=0), b"recording starts"), (dict(R=-1), b"recording starts"), (dict(R=11), b"recording starts"),
           (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 10)), b"seg_starts[1]"),
           (dict(starts=(0, 7, 3)), b"seg_starts[2]"), (dict(stride=0), b"dt_stride"), (dict(stride=-55), b"dt_stride"),
           (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(flags=1), b"flags"), (dict(flags=0x101), b"flags"),
           (dict(flags=0x200), b"flags"), (dict(flags=_hip.PARSE_BIG_ENDIAN, dtype=_hip.F64), b"big-endian"), (dict(out=dummy), b"aliases")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)                            # APE_ERR_INVALID_ARG
        assert what in lib.ape_last_error() and b"frame_times" in lib.ape_last_error(), (kw, lib.ape_last_error())


def test_resample_truth_refusals_are_made_on_the_host():
    """every refusal include/ape_hip.h states but the capturing stream (tests/test_resample_gpu.py); bodies_host must be valid for either
    kind, as for ape_score_rows"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy, other, third, fourth = C.c_void_p(256), C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(12288)
    body = np.zeros((3, 9))

    def call(layout=0, truth=dummy, kind=1, td=_hip.F64, Ft=20, tstarts=(0, 6, 14), tt=third, tq=fourth, F=10, starts=(0, 3, 7), shifts=None,
             max_gap=0.0, bodies=body, nb=1, out=other, od=_hip.F64, R=None):
        st, tst = np.ascontiguousarray(starts, dtype=np.int32), np.ascontiguousarray(tstarts, dtype=np.int32)
        sh = None if shifts is None else np.ascontiguousarray(shifts, dtype=np.float64)
        return lib.ape_resample_truth(layout, truth, kind, td, Ft, C.c_void_p(tst.ctypes.data) if len(tst) else None, tt, tq, F,
                                      C.c_void_p(st.ctypes.data) if len(st) else None, len(st) if R is None else R,
                                      None if sh is None else C.c_void_p(sh.ctypes.data), max_gap,
                                      C.c_void_p(bodies.ctypes.data) if bodies is not None else None, nb, out, od, None)

    nan, inf = float("nan"), float("inf")
    bad = [(dict(truth=None), b"NULL"), (dict(out=None), b"NULL"), (dict(starts=()), b"NULL"), (dict(tstarts=()), b"NULL"), (dict(bodies=None), b"NULL"),
           (dict(layout=_hip.LAYOUT_NONE), b"layout"), (dict(layout=3), b"layout"), (dict(kind=2), b"truth kind"), (dict(kind=-1), b"truth kind"),
           (dict(td=2), b"dtype"), (dict(od=-1), b"dtype"),
           (dict(F=0), b"F=0"), (dict(R=0), b"recording starts"), (dict(R=-1), b"recording starts"), (dict(R=11), b"recording starts"),
           (dict(starts=(1, 3, 7)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 3, 10)), b"seg_starts[2]"),
           (dict(Ft=0), b"Ft=0"), (dict(Ft=-1), b"Ft=-1"), (dict(Ft=2, tstarts=(0, 1, 1)), b"truth rows"),
           (dict(tstarts=(1, 6, 14)), b"truth rows"), (dict(tstarts=(0, 6, 6)), b"truth rows"), (dict(tstarts=(0, 6, 20)), b"truth rows"),
           (dict(tstarts=(0, 14, 6)), b"truth rows"),
           (dict(nb=2), b"n_bodies"), (dict(nb=0), b"n_bodies"), (dict(max_gap=nan), b"max_gap"),
           (dict(shifts=(0.0, nan, 0.0)), b"shift 1"), (dict(shifts=(0.0, 0.0, inf)), b"shift 2"), (dict(shifts=(-inf, 0.0, 0.0)), b"shift 0"),
           (dict(out=dummy), b"aliases"), (dict(out=third), b"aliases"), (dict(out=fourth), b"aliases")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)                            # APE_ERR_INVALID_ARG
        assert what in lib.ape_last_error() and b"resample_truth" in lib.ape_last_error(), (kw, lib.ape_last_error())
