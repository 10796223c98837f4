"""Mocap truth on each frame's clock (`ape_frame_times`, `ape_resample_truth`) on the GPU.

References: `score.frame_times_numpy` and `score.resample_truth_numpy` (plain numpy) on the same inputs; NN targets are first taken
through the float64 oracle FK (the reference's "eigh" route).

Bounds.  `frame_times`: float32 dt from [2^-8, 2^-3] adds without rounding in float64 (proved on the test's own values with
`fractions.Fraction` first), so the device must give numpy's BITS whatever its association; float64 dt of mixed magnitude within the
contract `|t[f] - exact| <= (f - s_r) 2^-53 sum|dt|`.  `resample_truth`: the NaN pattern identical, finite float64 values within 1e-12
absolute (the project's figure for float64 fixture rules; both sides run the same IEEE operations apart from asin / sin), exact hits
bit for bit; a float32 output within one float32 ulp of max(1, |x|) of the float64 statement rounded to float32.  `align(refine=True)`:
tests/test_score_gpu.py's own tolerances (rows 1e-13, sums 16 n 2^-53 max(1, max term), counts and maxima exact) against the host chain
run at the shifts the device found; those shifts against the host's to 1e-6 frame, as tests/test_score_lags_gpu.py compares `refined`."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests.test_resample_cpu import (ENDS, TIME_F, TIME_STARTS, exact_dt, jittered_dt, partial_sums_are_exact, refined_chain_numpy, truth_clock)
from tests.test_score_gpu import TOL, check_acc, check_rows, dev, same
from tests.test_score_lags_cpu import F, FPS, HIPS, LAGS, POS, SKIP, STARTS, WATCH, msgs_from_est, spread_for, trajectory

pytestmark = pytest.mark.gpu

R = len(STARTS)
SHIFTS = [0.0, 0.05, -0.03, 1e3, 0.11, 0.02]               # seconds; recording 3 is pushed wholly before its truth


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def run_times(dt, starts=None, **kw):
    from wear_mocap_ape_amd import score
    return host(score.frame_times(dt if isinstance(dt, torch.Tensor) else dev(dt), starts, **kw))


def run_resample(layout, truth, kind="est", **kw):
    from wear_mocap_ape_amd import score
    for k in ("truth_times", "times"):
        if kw.get(k) is not None and not isinstance(kw[k], torch.Tensor):
            kw[k] = dev(np.asarray(kw[k], dtype=np.float64))
    return host(score.resample_truth(layout, truth if isinstance(truth, torch.Tensor) else dev(truth), kind, **kw))


def check_resampled(got, ref, what, exact=None):
    """the NaN pattern identical, finite values within 1e-12 (float32: one ulp of max(1, |x|) around the rounded statement), the rows
    `exact` bit for bit -> the worst deviation"""
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = np.isfinite(ref)
    if got.dtype == np.float32:
        want = ref.astype(np.float32)
        gap = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
        assert (gap <= 2.0 ** -23 * np.maximum(1.0, np.abs(ref[ok]))).all(), (what, float(gap.max(initial=0.0)))
        if exact is not None:
            assert same(got[exact], want[exact]), what
        return float(gap.max(initial=0.0))
    worst = float(np.abs(got[ok] - ref[ok]).max(initial=0.0))
    assert worst <= 1e-12, (what, worst)
    if exact is not None:
        assert same(got[exact], ref[exact]), what
    return worst


# ---- the clock -----------------------------------------------------------------------------------------------------------------------------------
def test_frame_times_gives_numpys_bits_on_exactly_summable_input():
    from wear_mocap_ape_amd.score import frame_times_numpy
    dt = exact_dt()
    assert partial_sums_are_exact(dt, TIME_STARTS)          # the precondition: any association gives these bits
    ref = frame_times_numpy(dt, TIME_STARTS)
    d = dev(dt)
    got = run_times(d, TIME_STARTS)
    assert got.dtype == np.float64 and got.shape == (TIME_F,) and np.array_equal(got, ref)
    assert (got[TIME_STARTS] == 0.0).all()
    assert np.array_equal(run_times(d, TIME_STARTS), got)   # two calls, the same bits
    # one recording over three tiles, one tile alone, one frame
    assert np.array_equal(run_times(d), frame_times_numpy(dt))
    assert np.array_equal(run_times(d[:1024]), frame_times_numpy(dt[:1024])) and np.array_equal(run_times(d[:1025]), frame_times_numpy(dt[:1025]))
    assert np.array_equal(run_times(d[:1]), [0.0]) and np.array_equal(run_times(d[5:6]), [0.0])
    # a column view of raw [F, 55] rows, and the same rows byte-swapped under the big-endian flag
    rows = np.random.default_rng(2).normal(size=(TIME_F, 55)).astype(np.float32)
    rows[:, 0] = dt
    rd = dev(rows)
    assert not rd[:, 0].is_contiguous() and np.array_equal(run_times(rd[:, 0], TIME_STARTS), got)
    swapped = dev(rows.view(np.uint32).byteswap().view(np.float32))
    assert np.array_equal(run_times(swapped[:, 0], TIME_STARTS, big_endian=True), got)
    assert np.array_equal(run_times(dev(dt.view(np.uint32).byteswap().view(np.float32)), TIME_STARTS, big_endian=True), got)
    # float64 storage of the same values
    assert np.array_equal(run_times(dev(dt.astype(np.float64)), TIME_STARTS), got)


def test_frame_times_past_256_tiles_where_the_carry_scan_takes_a_second_round():
    """F = 300 000 is 293 tiles of 1024 frames: the one workgroup that scans the tile aggregates takes them 256 at a time and hands its
    running sum from the first round to the second.  One recording lies across that hand-over (tiles 255 | 256), one starts exactly on
    it; the input adds without rounding, so numpy's bits are asked for"""
    from wear_mocap_ape_amd.score import frame_times_numpy
    n, edge = 300_000, 256 * 1024
    dt = exact_dt(n, seed=13)
    d = dev(dt)
    for starts in ([0, 65_000, 130_000, 195_000, 260_000, edge - 4, edge + 6], [0, 65_000, 130_000, 195_000, 260_000, edge - 1, edge, edge + 1, edge + 56]):
        ends = starts[1:] + [n]
        # the precondition, in integers: every dt is a multiple of 2^-31 and a recording's total stays below 2^53 of them
        units = dt.astype(np.float64) * 2.0 ** 31
        assert np.array_equal(units, np.rint(units)) and max(e - s for s, e in zip(starts, ends)) <= 2 ** 16
        assert all(int(units[s + 1:e].astype(np.int64).sum()) < 2 ** 53 for s, e in zip(starts, ends))
        got = run_times(d, starts)
        assert np.array_equal(got, frame_times_numpy(dt, starts)) and (got[starts] == 0.0).all() and got[edge + 3] > 0.0
    bad = dt.copy()
    bad[edge - 2] = np.nan                                  # in the recording that lies across the hand-over: to its end, not beyond
    got = run_times(bad, [0, 65_000, 130_000, 195_000, 260_000, edge - 4, edge + 6])
    ref = frame_times_numpy(dt, [0, 65_000, 130_000, 195_000, 260_000, edge - 4, edge + 6])
    assert np.isnan(got[edge - 2:edge + 6]).all() and np.array_equal(np.delete(got, np.arange(edge - 2, edge + 6)), np.delete(ref, np.arange(edge - 2, edge + 6)))


def test_frame_times_float64_of_mixed_magnitude_stays_within_the_bound():
    rng = np.random.default_rng(17)
    dt = 10.0 ** rng.uniform(-6.0, 2.0, size=TIME_F) * rng.choice([1.0, 1.0, 1.0, -1.0], size=TIME_F)
    got = run_times(dt, TIME_STARTS)
    worst = 0.0
    for s, e in zip(TIME_STARTS, TIME_STARTS[1:] + [TIME_F]):
        assert got[s] == 0.0
        exact, total = Fraction(0), Fraction(0)
        for f in range(s + 1, e):
            exact += Fraction(float(dt[f]))
            total += abs(Fraction(float(dt[f])))
            err = abs(Fraction(float(got[f])) - exact)
            assert err <= (f - s) * Fraction(1, 2 ** 53) * total, (s, f, float(err))
            worst = max(worst, float(err / total))
    print(f"float64 dt, mixed magnitude: worst |t - exact| / sum|dt| = {worst:.3e}")


def test_a_nan_dt_spoils_the_rest_of_its_own_recording_only():
    from wear_mocap_ape_amd.score import frame_times_numpy
    dt = exact_dt()
    ref = frame_times_numpy(dt, TIME_STARTS)
    for bad in (np.nan, np.inf):
        d = dt.copy()
        d[300] = bad
        got = run_times(d, TIME_STARTS)
        assert not np.isfinite(got[300:1023]).any()         # frames 300 .. 1022, the end of the recording [257, 1023)
        keep = np.r_[0:300, 1023:TIME_F]
        assert np.array_equal(got[keep], ref[keep])
    d = dt.copy()
    d[TIME_STARTS] = np.nan                                 # the first row's dt is not read
    assert np.array_equal(run_times(d, TIME_STARTS), ref)
    d[1023] = 1.0
    d[1022] = np.inf                                        # the last frame of a recording, the one before a tile edge
    got = run_times(d, TIME_STARTS)
    assert np.isinf(got[1022]) and np.array_equal(np.delete(got, 1022), np.delete(ref, 1022))


# ---- the rows ----------------------------------------------------------------------------------------------------------------------------------
def clocks(seed=5):
    """frame times of the six recordings (jittered float32 dt) and ~1700 truth stamps on a jittered 120 Hz clock of their own"""
    from wear_mocap_ape_amd.score import frame_times_numpy
    tq = frame_times_numpy(jittered_dt(F, seed), STARTS)
    tts = [truth_clock(tq[e - 1], jitter=0.3, seed=seed + r) for r, e in enumerate(ENDS)]
    tstarts = [0] + [int(v) for v in np.cumsum([len(t) for t in tts])[:-1]]
    return tq, np.concatenate(tts), tstarts


@pytest.fixture(scope="module")
def session(golden):
    """per layout the truth of the six recordings in both kinds: est rows of smooth trajectories; NN targets (the fixtures' rows, tiled)
    with the est rows the oracle FK makes of them, one body per recording"""
    tq, tt, tstarts = clocks()
    Ft = tt.shape[0]
    assert 1600 <= Ft <= 1900
    tends = tstarts[1:] + [Ft]
    d = {"tq": tq, "tt": tt, "tstarts": tstarts, "Ft": Ft}
    for layout in (HIPS, WATCH, POS):
        g = golden(f"fk_layout{layout}.npz")
        est = np.concatenate([trajectory(tt[a:b] * FPS + 40.0 * r, layout, seed=r) for r, (a, b) in enumerate(zip(tstarts, tends))])
        reps = -(-Ft // 300)
        preds = np.tile(g["preds_bd_N300"], (reps, 1))[:Ft]
        bodies = np.stack([g["body_bd"].reshape(9) if r % 2 == 0 else g["body_bo"].reshape(9) for r in range(R)])
        d[layout] = {"est": est, "targets": preds, "bodies": bodies}
    return d


def oracle_rows(preds, bodies, tstarts, layout):
    tends = list(tstarts[1:]) + [preds.shape[0]]
    return np.concatenate([orc.arm_pose_from_targets(preds[a:b], bodies[r], layout, route="eigh") for r, (a, b) in enumerate(zip(tstarts, tends))])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", ["est", "targets"])
@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_resampled_rows_equal_the_statement(session, layout, kind, dtype):
    from wear_mocap_ape_amd.score import resample_truth_numpy
    s = session
    td = dev(s[layout][kind], dtype)
    stored = td.cpu().numpy().astype(np.float64)            # what the device reads, widened exactly
    est = stored if kind == "est" else oracle_rows(stored, s[layout]["bodies"], s["tstarts"], layout)
    kw = dict(truth_starts=s["tstarts"], truth_times=s["tt"], times=s["tq"], starts=STARTS, shifts=SHIFTS)
    ref = resample_truth_numpy(layout, est, **kw)
    got = run_resample(layout, td, kind, bodies=s[layout]["bodies"], out_dtype=dtype, **kw)
    assert got.dtype == (np.float32 if dtype == torch.float32 else np.float64) and got.shape == (F, 14 if layout == WATCH else 21)
    nan_rows = np.isnan(ref).all(axis=1)
    # recording 3 lies wholly before its truth; 0: no shift; 4: the first 0.11 s of frames; 2: at most the last frames, 0.03 s past the truth
    assert nan_rows[STARTS[3]:ENDS[3]].all() and not nan_rows[STARTS[0]:ENDS[0]].any() and 3 <= nan_rows[STARTS[4]:ENDS[4]].sum() <= 10
    assert not nan_rows[STARTS[2]:ENDS[2] - 4].any()
    assert same(ref[0], est[0]) and np.isfinite(ref[~nan_rows]).all()              # u = 0 at a recording's first frame: an exact hit
    worst = check_resampled(got, ref, (layout, kind, dtype), exact=[0] if kind == "est" else None)
    print(f"layout {layout} {kind} {dtype}: max |device - numpy| = {worst:.3e} over {int((~nan_rows).sum())} rows")
    # the same inputs, the same bits
    assert same(got, run_resample(layout, td, kind, bodies=s[layout]["bodies"], out_dtype=dtype, **kw))
    if kind == "targets" and layout != POS:                 # the body is the recording's: one body for all changes the odd recordings alone
        one = run_resample(layout, td, kind, bodies=s[layout]["bodies"][0], out_dtype=dtype, **kw)
        assert same(one[STARTS[2]:ENDS[2]], got[STARTS[2]:ENDS[2]]) and not same(one[STARTS[1]:ENDS[1]], got[STARTS[1]:ENDS[1]])


@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_integer_shifts_on_the_index_clock_give_the_input_bits(layout):
    truth = trajectory(np.arange(F), layout)
    truth[[10, 100, 400], [1, 7, 13]] = np.nan              # an exact hit returns the row as it is
    shifts = [0, 3, -2, 7, 1, -40]
    got = run_resample(layout, truth, truth_starts=STARTS, frames=F, starts=STARTS, shifts=shifts)
    for (s, e), l in zip(zip(STARTS, ENDS), shifts):
        f = np.arange(s, e)
        inside = (f - l >= s) & (f - l < e)
        assert same(got[f[inside]], truth[f[inside] - l]) and np.isnan(got[f[~inside]]).all(), (s, l)
    assert np.isnan(got[13, 1]) and np.isfinite(got[13, 0])
    assert same(run_resample(layout, truth, truth_starts=STARTS, frames=F, starts=STARTS), truth)


def test_edges_of_waves_tiles_and_of_the_truth():
    """F in {1, 63, 64, 65, 255, 256, 257, 513} against Ft in {1, 2, F}: frames at half-row steps of the truth's index clock, so even
    frames hit a row exactly, odd ones lie between two, and everything past the last row is NaN"""
    from wear_mocap_ape_amd.score import resample_truth_numpy
    rows = trajectory(np.arange(513), HIPS, seed=4)
    td = dev(rows)
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        tq = np.arange(n, dtype=np.float64) / 2.0
        for nt in sorted({1, 2, n}):
            ref = resample_truth_numpy(HIPS, rows[:nt], times=tq)
            got = run_resample(HIPS, td[:nt], times=tq)
            hits = np.flatnonzero((np.arange(n) % 2 == 0) & (np.arange(n) // 2 < nt))
            check_resampled(got, ref, (n, nt), exact=hits)
            assert same(got[hits], rows[hits // 2]) and np.isnan(got[2 * nt - 1:]).all() and np.isfinite(got[:2 * nt - 1]).all()
            if nt == 1:
                assert np.isfinite(got).all(axis=1).sum() == 1         # only the exact hit


def test_gaps_nan_values_duplicate_stamps_and_non_finite_times(session):
    from wear_mocap_ape_amd.score import resample_truth_numpy
    s = session
    est, tt, tq = s[HIPS]["est"].copy(), s["tt"].copy(), s["tq"].copy()
    rng = np.random.default_rng(77)
    est[rng.choice(s["Ft"], 40, replace=False), rng.integers(0, 21, size=40)] = np.nan
    est[rng.choice(s["Ft"], 5, replace=False), 3] = np.inf
    ts2 = s["tstarts"][2]
    tt[ts2 + 5:ts2 + 9] = tt[ts2 + 5]                       # rows 5-8 of recording 2 share a stamp, rows 30 and 31 another
    tt[ts2 + 31] = tt[ts2 + 30]
    drop = s["tstarts"][3] + 20                             # a dropout: ten stamps pushed on by 0.1 s each side of it
    tt[drop:s["tstarts"][4]] += 0.1
    tq[[4, 90, 91, 300, 699]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    tq[[400, 401]] = tq[[401, 400]]                         # frame times need not be monotonic
    tq[STARTS[2] + 9] = tt[ts2 + 5]                         # an exact hit on equal stamps (recording 2 has no shift here): the last of them
    kw = dict(truth_starts=s["tstarts"], truth_times=tt, times=tq, starts=STARTS, shifts=[0.0, 0.05, 0.0, 0.11, 0.0, 0.02])
    for max_gap in (0.0, 1.5 / 120.0):
        ref = resample_truth_numpy(HIPS, est, max_gap=max_gap, **kw)
        got = run_resample(HIPS, est, max_gap=max_gap, **kw)
        worst = check_resampled(got, ref, max_gap)
        print(f"gaps, max_gap {max_gap:.4f}: {int(np.isnan(ref).all(axis=1).sum())} NaN rows, max |device - numpy| = {worst:.3e}")
        assert np.isnan(got[[4, 90, 91, 300, 699]]).all() and same(got[STARTS[2] + 9], est[ts2 + 8])
    lost = np.isnan(ref).all(axis=1) & ~np.isnan(resample_truth_numpy(HIPS, est, **kw)).all(axis=1)
    assert lost[STARTS[3]:ENDS[3]].any() and lost.sum() >= 1                 # max_gap drops frames the dropout would otherwise bridge
    # unsorted truth times are refused by the check (which waits) and taken without it: no read outside the recording's rows
    bad = tt.copy()
    bad[100], bad[101] = bad[101], bad[100]
    with pytest.raises(UserWarning):
        run_resample(HIPS, est, **dict(kw, truth_times=bad))
    with pytest.raises(UserWarning):
        run_resample(HIPS, est, **dict(kw, truth_times=np.where(np.arange(s["Ft"]) == 7, np.nan, tt)))
    loose = run_resample(HIPS, est, check_times=False, **dict(kw, truth_times=bad))
    assert loose.shape == ref.shape
    boundary = tt.copy()
    boundary[s["tstarts"][1]:] -= 5.0                       # a clock that starts again (or earlier) with the next recording is in order
    assert run_resample(HIPS, est, **dict(kw, truth_times=boundary)).shape == ref.shape


def test_rows_behind_the_output_are_untouched_and_refusals_write_nothing(session):
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    s = session
    W, pad = 21, 3
    truth, tt, tq = dev(s[HIPS]["est"]), dev(s["tt"]), dev(s["tq"])
    out = torch.full((F + pad, W), -7.0, dtype=torch.float64, device="cuda")
    times = torch.full((F + pad,), -7.0, dtype=torch.float64, device="cuda")
    body = np.zeros((1, 9))
    st, tst = np.asarray(STARTS, dtype=np.int32), np.asarray(s["tstarts"], dtype=np.int32)
    sh = np.asarray(SHIFTS, dtype=np.float64)
    p = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def resample(layout=HIPS, Ft=s["Ft"], n=F, max_gap=0.0, shifts=sh, o=out, kind=_hip.TRUTH_EST):
        return lib.ape_resample_truth(layout, p(truth), kind, _hip.F64, Ft, C.c_void_p(tst.ctypes.data), p(tt), p(tq), n, C.c_void_p(st.ctypes.data),
                                      R, C.c_void_p(shifts.ctypes.data), max_gap, C.c_void_p(body.ctypes.data), 1, p(o), _hip.F64, stream)

    def clock(n=F, stride=1, flags=0, dtype=_hip.F64, o=times):
        return lib.ape_frame_times(p(tq), stride, dtype, flags, n, C.c_void_p(st.ctypes.data), R, p(o), stream)

    bad_shift = sh.copy()
    bad_shift[2] = np.nan
    for rc in (resample(layout=3), resample(Ft=0), resample(Ft=s["tstarts"][-1]), resample(n=STARTS[-1]), resample(max_gap=float("nan")),
               resample(shifts=bad_shift), resample(o=truth), resample(o=tt), resample(o=tq), resample(kind=2),
               clock(n=0), clock(stride=0), clock(flags=0x100), clock(flags=2), clock(dtype=3), clock(o=tq)):
        assert rc == 1                                      # APE_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (times == -7.0).all()
    assert resample() == 0 and clock() == 0
    torch.cuda.synchronize()
    assert (out[F:] == -7.0).all() and not (out[:F] == -7.0).any() and (times[F:] == -7.0).all() and not (times[:F] == -7.0).any()
    from wear_mocap_ape_amd.score import frame_times_numpy, resample_truth_numpy
    kw = dict(truth_starts=s["tstarts"], truth_times=s["tt"], times=s["tq"], starts=STARTS, shifts=SHIFTS)
    check_resampled(out[:F].cpu().numpy(), resample_truth_numpy(HIPS, s[HIPS]["est"], **kw), "direct call")
    # float32 rows behind a float32 output of the narrow layout, F one past a wave
    n = 65
    o32 = torch.full((n + pad, 14), -7.0, dtype=torch.float32, device="cuda")
    t14 = dev(trajectory(np.arange(n), WATCH))
    one = np.zeros(1, dtype=np.int32)
    half = np.full(1, 0.5)
    assert lib.ape_resample_truth(WATCH, p(t14), _hip.TRUTH_EST, _hip.F64, n, C.c_void_p(one.ctypes.data), None, None, n, C.c_void_p(one.ctypes.data),
                                  1, C.c_void_p(half.ctypes.data), 0.0, C.c_void_p(body.ctypes.data), 1, p(o32), _hip.F32, stream) == 0
    torch.cuda.synchronize()
    assert (o32[n:] == -7.0).all() and torch.isnan(o32[0]).all() and torch.isfinite(o32[1:n]).all()
    assert np.allclose(times[:F].cpu().numpy(), frame_times_numpy(s["tq"], STARTS), rtol=0, atol=1e-9)


def test_a_capturing_stream_is_refused_by_both_entries(session):
    """both entries stage host arrays per call: on a stream that is capturing a graph they return APE_ERR_INVALID_ARG and write nothing"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    s = session
    truth, tt, tq = dev(s[HIPS]["est"]), dev(s["tt"]), dev(s["tq"])
    out = torch.full((F, 21), -7.0, dtype=torch.float64, device="cuda")
    times = torch.full((F,), -7.0, dtype=torch.float64, device="cuda")
    body = np.zeros((1, 9))
    st, tst = np.asarray(STARTS, dtype=np.int32), np.asarray(s["tstarts"], dtype=np.int32)
    sh = np.asarray(SHIFTS, dtype=np.float64)
    p = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731

    def resample(stream):
        return lib.ape_resample_truth(HIPS, p(truth), _hip.TRUTH_EST, _hip.F64, s["Ft"], C.c_void_p(tst.ctypes.data), p(tt), p(tq), F,
                                      C.c_void_p(st.ctypes.data), R, C.c_void_p(sh.ctypes.data), 0.0, C.c_void_p(body.ctypes.data), 1, p(out), _hip.F64,
                                      stream)

    def clock(stream):
        return lib.ape_frame_times(p(tq), 1, _hip.F64, 0, F, C.c_void_p(st.ctypes.data), R, p(times), stream)

    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros((4,), device="cuda")
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            handle = C.c_void_p(side.cuda_stream)
            rc_r, msg_r = resample(handle), lib.ape_last_error()
            rc_c, msg_c = clock(handle), lib.ape_last_error()
    torch.cuda.current_stream().wait_stream(side)
    assert rc_r == 1 and b"capturing" in msg_r and b"resample_truth" in msg_r, (rc_r, msg_r)
    assert rc_c == 1 and b"capturing" in msg_c and b"frame_times" in msg_c, (rc_c, msg_c)
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (times == -7.0).all()    # nothing was written
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert resample(stream) == 0 and clock(stream) == 0     # ... and the same arguments on a stream that is not capturing are taken
    torch.cuda.synchronize()
    assert not (out == -7.0).any() and not (times == -7.0).any()


# ---- the chains ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", [2.5, -1.75])
def test_align_refine_gives_the_host_chains_result(plant):
    from wear_mocap_ape_amd import score
    idx = np.arange(F)
    truth = trajectory(idx)
    msg = msgs_from_est(trajectory(idx - plant), HIPS)
    rec = spread_for(msg)
    md, td, sd = dev(msg), dev(truth), dev(rec)
    best, rows, acc = score.align(HIPS, md, td, LAGS, truth_kind="est", spread=sd, starts=STARTS, skip=SKIP, refine=True)
    rows, acc = host(rows), host(acc)
    want_best, _, want_acc = refined_chain_numpy(msg, truth, HIPS, LAGS, STARTS, SKIP, rec)
    assert best[0]["lag"] is None and want_best[0]["lag"] is None and not acc[0].any()
    for r in range(1, R):
        assert best[r]["lag"] == want_best[r]["lag"] and best[r]["scored"] == want_best[r]["scored"], r
        assert abs(best[r]["refined"] - want_best[r]["refined"]) <= 1e-6 and abs(best[r]["refined"] - plant) <= 0.01, (r, best[r])
    # rows and accumulators: the host chain at the shifts the device found (a shift 1e-9 frame off moves the truth by more than 1e-13)
    shifts = [0.0 if b["lag"] is None else b["refined"] for b in best]
    _, ref_rows, ref_acc = refined_chain_numpy(msg, truth, HIPS, LAGS, STARTS, SKIP, rec, shifts)
    worst = check_rows(rows, ref_rows, ("refined rows", plant))
    print(f"plant {plant}: max |device - host chain| columns 0-4 = {worst:.3e}")
    check_acc(acc, rows, STARTS, SKIP, ("refined acc", plant))
    assert np.array_equal(acc[:, [15, 16]], ref_acc[:, [15, 16]]) and np.array_equal(acc[:, [15, 16]], want_acc[:, [15, 16]])
    with np.errstate(all="ignore"):
        rms = np.sqrt(acc[:, 1] / acc[:, 15])
    assert all(rms[r] <= 0.1 * best[r]["rms"] for r in range(1, R))
    # refine=False is the path it was: the integer pass of score_lags
    b0, rows0, acc0 = score.align(HIPS, md, td, LAGS, truth_kind="est", spread=sd, starts=STARTS, skip=SKIP)
    found = [0 if b["lag"] is None else b["lag"] for b in b0]
    s1, a1 = score.score_lags(HIPS, md, td, (0, 0), "est", sd, STARTS, SKIP, None, found, per_frame=True)
    assert [b["lag"] for b in b0] == [b["lag"] for b in best] and same(host(rows0), host(s1)[:, 0]) and np.array_equal(host(acc0), host(a1)[:, 0])


def test_truth_on_frames_from_raw_big_endian_rows(session):
    from wear_mocap_ape_amd import score
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    s = session
    dt = jittered_dt(F, 5)
    rows = np.random.default_rng(8).normal(size=(F, 55)).astype(np.float32)
    rows[:, 0] = dt
    wire = dev(rows.view(np.uint32).byteswap().view(np.float32))
    truth, tt = dev(s[WATCH]["targets"]), dev(s["tt"])
    kw = dict(truth_starts=s["tstarts"], starts=STARTS, shifts=SHIFTS, max_gap=0.02)
    got = host(score.truth_on_frames(WATCH, wire, truth, tt, bodies=s[WATCH]["bodies"], big_endian=True, **kw))
    times = score.frame_times(wire[:, 0], STARTS, big_endian=True)
    by_hand = host(score.resample_truth(WATCH, truth, "targets", s["tstarts"], tt, times, None, STARTS, SHIFTS, 0.02, s[WATCH]["bodies"]))
    assert got.shape == (F, 14) and same(got, by_hand) and np.isfinite(got).any()
    assert np.abs(host(times) - s["tq"]).max() <= 1e-12     # the session's clock was made of the same dt (numpy's order of summation)
    assert same(host(score.truth_on_frames(WATCH, dev(rows), truth, tt, bodies=s[WATCH]["bodies"], **kw)), got)
    # the estimator's method supplies its layout and body; host rows are copied over
    est_obj = WatchPhoneUarm(smooth=5)
    mine = host(est_obj.truth_on_frames(rows, truth, tt, **kw))
    want = host(score.truth_on_frames(est_obj._layout, dev(rows), truth, tt, bodies=est_obj.body_measurements, **kw))
    assert est_obj._layout == WATCH and same(mine, want)
    # the result goes into the scorers as est-kind truth; what could not be resampled is counted as not scorable
    msg = dev(msgs_from_est(trajectory(np.arange(F), WATCH), WATCH))
    _, acc = score.score_rows(WATCH, msg, torch.as_tensor(got, device="cuda"), "est", starts=STARTS)
    acc = host(acc)
    lost = np.isnan(got).all(axis=1)
    assert np.array_equal(acc[:, 16], [lost[a:b].sum() for a, b in zip(STARTS, ENDS)]) and acc[3, 15] == 0 and acc[2, 15] > 0
