"""Joint angles of every frame and their errors against truth (`ape_joint_angles`) on the GPU.

Reference of every per-frame value: `score.joint_angles_numpy` (plain numpy, the header's operations in their order) on the same rows --
for float32 rows the statement of the rounded rows; of the accumulators: numpy sums over the call's own per-frame rows.

Setup of tests/test_motion_gpu.py: F = 1000 frames, recordings starting at 0, 37, 253, 256, 257, 300, 301 and 900 (three rows before, at
and one row past the edge of a 256-frame tile; a one-frame recording at 300, whose support is empty at skip = 2), poses of
`tests/test_frame_fit_cpu.walk_est`.  One NaN row and rows forced onto and into each singular band (a straight arm, an arm hanging and
straight up, a swing of pi of either joint) are planted in the rows and, elsewhere, in the truth.

Tolerances and where they come from (u = 2^-53):
* every angle is atan2 of two numbers made of +, -, *, /, sqrt only, each correctly rounded and in the statement's order, from
  quaternions that are copies of the rows or, for target rows, the float64 conversion that `score._pose_rows` restates operation for
  operation: the atan2 arguments are bit-identical, so the NaN pattern is the statement's exactly (the thresholds compare identical
  quantities) and only the two atan2 routines differ: allowed 8 u |value|, the allowance tests/test_motion_gpu.py grants its atan2 columns.
* an error is the difference of two such angles: allowed 8 u (|a_row| + |a_truth|), measured on the circle.
* sums within 16 n u max(1, max term) of numpy's sums of the call's own rows (the rule of tests/test_frame_fit_gpu.py); minima, maxima and
  counts exact.
The worst fraction of the allowance used is printed (profiles/joint_angles.md records it)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_frame_fit_cpu import msgs_from_est, qmul, walk_est
from tests.test_joint_angles_cpu import call_entry, check_sums, fore_in_upper, refusals, targets_of, twist_x, upper_in_thorax
from tests.test_motion_gpu import ENDS, F, SKIP, STARTS, WIDE, default_body, dev, same

pytestmark = pytest.mark.gpu

HIPS, WATCH, POS = 0, 1, 2
U = 2.0 ** -53
KINDS = ("msg", "est", "targets")
LAGS = [2, 0, -1, 1, 0, 0, -3, 5]
SUPPORT = [max(0, e - s - SKIP) for s, e in zip(STARTS, ENDS)]
PERIODIC = (1, 2, 4, 5, 6)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


_ROWS = {}


def planted_rows(layout, kind, seed, at):
    """float64 rows [F, w] of a kind stating the walk of this layout and seed with the singular cases planted at rows at .. at + 7 (made
    once): a straight arm, the elbow 0.02 rad inside the band, the arm hanging, 0.03 rad from straight up, a forearm swing of pi and one
    0.02 rad short of it, an upper-arm swing of pi and one 0.03 rad short of it"""
    if (layout, seed, at) not in _ROWS:
        est = walk_est(F, layout, seed=seed)
        ql, qu = (6, 10) if layout == WATCH else (9, 13)
        qh = est[at:at + 8, 17:21] if layout != WATCH else np.tile([1.0, 0.0, 0.0, 0.0], (8, 1))
        a = np.random.default_rng(seed).uniform(0.4, 2.6, size=(8, 6))            # flexion, azimuth, twist, elevation, plane, twist
        a[0, 0], a[1, 0], a[2, 3], a[3, 3] = 0.0, 0.02, 0.0, np.pi - 0.03
        e, s = fore_in_upper(a[:, 0], a[:, 1], a[:, 2]), upper_in_thorax(a[:, 3], a[:, 4], a[:, 5])
        pole = lambda b, t: qmul(np.array([np.sin(t / 2), 0.0, np.cos(t / 2) * np.cos(b), np.cos(t / 2) * np.sin(b)]), twist_x(np.array(0.4)))  # noqa: E731
        e[4], e[5], s[6], s[7] = pole(0.7, 0.0), pole(-2.0, 0.02), pole(-1.1, 0.0), pole(2.2, 0.03)
        est[at:at + 8, qu:qu + 4] = qmul(qh, s)
        est[at:at + 8, ql:ql + 4] = qmul(est[at:at + 8, qu:qu + 4], e)
        _ROWS[layout, seed, at] = {"est": est, "msg": msgs_from_est(est, layout), "targets": targets_of(est, layout)}
    return _ROWS[layout, seed, at][kind]


def rows_and_truth(layout, kind, tkind):
    """(rows, truth): the singular cases at rows 252 .. 259 (across the tile edge and three recording starts) and a NaN row at 510 of
    the rows; at 600 .. 607 and a NaN row at 38 of the truth"""
    rows = planted_rows(layout, kind, 3 + layout, 252).copy()
    truth = planted_rows(layout, tkind, 50 + layout, 600).copy()
    rows[510, {"msg": 15, "est": 11, "targets": 1}[kind]] = np.nan
    truth[38, {"msg": 8, "est": 12, "targets": 2}[tkind]] = np.nan
    return rows, truth


def run(layout, rows, kind, truth=None, tkind="est", lags=None, per_frame=True, **kw):
    from wear_mocap_ape_amd import score
    a, e, acc = score.joint_angles(layout, rows, kind, truth, tkind, STARTS, SKIP, lags, per_frame=per_frame, **kw)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return host(a), host(e), host(acc)


def circle(d):
    return np.abs(np.angle(np.exp(1j * d)))


def paired_truth_angles(tang):
    """the truth's angles of frame f - l_r, NaN where that leaves the recording"""
    out = np.full((F, 7), np.nan)
    for s, e, l in zip(STARTS, ENDS, LAGS):
        f = np.arange(s, e)
        ok = (f - l >= s) & (f - l < e)
        out[f[ok]] = tang[f[ok] - l]
    return out


def check_rows(got, ref, allow, what, on_circle=()):
    """the NaN pattern exactly, every finite value within its allowance -> worst fraction of the allowance used"""
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), (what, np.argwhere(np.isnan(got) != np.isnan(ref))[:5])
    diff = np.abs(got - ref)
    cols = list(on_circle)
    diff[:, cols] = circle(got[:, cols] - ref[:, cols])
    ok = np.isfinite(ref)
    assert (diff[ok] <= allow[ok]).all(), (what, float((diff[ok] / np.where(allow[ok] > 0, allow[ok], 1.0)).max()))
    nz = ok & (allow > 0)
    return float((diff[nz] / allow[nz]).max(initial=0.0))


# ---------------- 1: per-frame rows and accumulators against the statement -------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_rows_errors_and_sums_against_the_statement(layout, kind):
    from wear_mocap_ape_amd.score import joint_angles_numpy
    tkind = KINDS[(KINDS.index(kind) + 1 + layout) % 3]     # truth of the rows' kind for one layout in three, of another for two
    rows, truth = rows_and_truth(layout, kind, tkind)
    w, tw = rows.shape[1], truth.shape[1]
    body = default_body()
    worst_a = worst_e = 0.0
    for dtype, npdt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        stored, tstored = rows.astype(npdt), truth.astype(npdt)
        ref, ref_err, ref_acc = joint_angles_numpy(stored, layout, kind, tstored, tkind, STARTS, SKIP, LAGS, body)
        tang = joint_angles_numpy(tstored, layout, tkind, bodies=body)[0]
        # the statement's own NaN pattern is not trivial: the planted rows, the NaN rows, the frames a lag leaves unpaired
        assert np.isnan(ref[510]).all() and np.isnan(ref[252, 1]) and np.isnan(ref[253, 1]) and np.isnan(ref[254, 4]) and np.isnan(ref[255, 4])
        assert np.isnan(ref[256, 2]) and np.isnan(ref[257, 2]) and np.isnan(ref[258, 5]) and np.isnan(ref[259, 5])
        assert np.isnan(ref[252:260]).sum() == 8 and np.isnan(tang[600:608]).sum() == 8 and np.isnan(tang[38]).all()
        assert np.isnan(ref_err[[0, 1, 897, 899, 900, 904]]).all() and np.isfinite(ref_err[[2, 896, 905], 0]).all() and np.isnan(ref_err[38]).all()
        plain, tplain = dev(stored), dev(tstored)
        wide = torch.full((F, WIDE), float("nan"), dtype=dtype, device="cuda")
        wide[:, :w] = plain
        twide = torch.full((F, WIDE), float("nan"), dtype=dtype, device="cuda")
        twide[:, :tw] = tplain
        allow_a = 8 * U * np.abs(ref)
        allow_e = 8 * U * (np.abs(ref) + np.abs(paired_truth_angles(tang)))
        for name, view, tview in (("contiguous", plain, tplain), ("strided", wide[:, :w], twide[:, :tw])):
            what = (layout, kind, tkind, str(dtype), name)
            got, err, acc = run(layout, view, kind, tview, tkind, LAGS, out_dtype=torch.float64, bodies=body)
            worst_a = max(worst_a, check_rows(got, ref, allow_a, what, PERIODIC))
            worst_e = max(worst_e, check_rows(err, ref_err, allow_e, what, PERIODIC))
            check_sums(acc, got, err, STARTS, SKIP, what)
            assert np.array_equal(acc[:, 4:70:5], ref_acc[:, 4:70:5]) and np.array_equal(acc[:, 70], SUPPORT), what       # counts; [70]
            for r in (3, 5):                                # the one-frame recordings: an empty support gives the stated empties
                assert (acc[r, 2:35:5] == np.inf).all() and (acc[r, 3:35:5] == -np.inf).all(), what
                assert not np.delete(acc[r], [2, 3, 7, 8, 12, 13, 17, 18, 22, 23, 27, 28, 32, 33]).any(), what
            if layout == WATCH:
                ok = np.isfinite(got[:, 0])
                assert (got[ok, 6] == 0.0).all() and not np.delete(acc, [3, 5], axis=0)[:, [30, 31, 32, 33]].any(), what
        # without truth: the same angles, no errors, error sums all zeros; the accumulators do not depend on the rows being written
        only, none, acc_only = run(layout, plain, kind, out_dtype=torch.float64, bodies=body)
        assert none is None and same(only, got) and np.array_equal(acc_only[:, :35], acc[:, :35]) and not acc_only[:, 35:70].any()
        assert np.array_equal(acc_only[:, 70], acc[:, 70])
        a2, e2, acc2 = run(layout, plain, kind, tplain, tkind, LAGS, per_frame=False, bodies=body)
        assert a2 is None and e2 is None and np.array_equal(acc2, acc)
        # the default output type is the rows'; float32 outputs are the float64 values rounded once; two runs give the same bits
        own, own_err, acc3 = run(layout, plain, kind, tplain, tkind, LAGS, bodies=body)
        assert own.dtype == npdt and own_err.dtype == npdt and np.array_equal(acc, acc3)
        assert same(own, got.astype(npdt)) and same(own_err, err.astype(npdt))
        f32, f32_err, _ = run(layout, plain, kind, tplain, tkind, LAGS, out_dtype=torch.float32, bodies=body)
        assert f32.dtype == np.float32 and same(f32, got.astype(np.float32)) and same(f32_err, err.astype(np.float32))
    print(f"layout {layout}, {kind} rows against {tkind} truth: NaN patterns equal; worst fraction of the atan2 allowance used: "
          f"angles {worst_a:.3f}, errors {worst_e:.3f}")


def test_min_swing_zero_states_everything_and_a_body_per_recording():
    from wear_mocap_ape_amd.score import joint_angles_numpy
    rows, truth = rows_and_truth(HIPS, "targets", "targets")
    rows[510, 1] = 0.25                                     # (no NaN row here)
    truth[38, 2] = 0.25
    rng = np.random.default_rng(9)
    bodies = default_body()[None, :] * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, size=(len(STARTS), 9)))
    ref, ref_err, _ = joint_angles_numpy(rows, HIPS, "targets", truth, "targets", STARTS, SKIP, LAGS, bodies, 0.0)
    got, err, acc = run(HIPS, dev(rows), "targets", dev(truth), "targets", LAGS, bodies=bodies, min_swing=0.0)
    assert np.isfinite(got).all() and (acc[:, 4:35:5] == np.array(SUPPORT)[:, None]).all()
    check_rows(got, ref, 8 * U * np.abs(ref), "min_swing 0", PERIODIC)
    tang = joint_angles_numpy(truth, HIPS, "targets", bodies=bodies, starts=STARTS, min_swing=0.0)[0]
    check_rows(err, ref_err, 8 * U * (np.abs(ref) + np.abs(paired_truth_angles(tang))), "min_swing 0 errors", PERIODIC)
    check_sums(acc, got, err, STARTS, SKIP, "min_swing 0")


# ---------------- 2: sets --------------------------------------------------------------------------------------------------------------------
def test_sets_are_single_set_calls_bit_for_bit():
    from wear_mocap_ape_amd import score
    rows, truth = rows_and_truth(HIPS, "msg", "est")
    other = planted_rows(HIPS, "msg", 77, 100).copy()
    holed = rows.copy()
    holed[299] = np.nan                                     # the last row of the recording 257 .. 299
    sets, td = dev(np.stack([rows, other, holed])), dev(truth)
    ang, err, acc = run(HIPS, sets, "msg", td, "est", LAGS)
    assert ang.shape == (3, F, 7) and err.shape == (3, F, 7) and acc.shape == (3, len(STARTS), 71)
    for c in range(3):
        a1, e1, acc1 = run(HIPS, sets[c], "msg", td, "est", LAGS)
        assert same(ang[c], a1) and same(err[c], e1) and np.array_equal(acc[c], acc1), c
    again = run(HIPS, sets, "msg", td, "est", LAGS)
    assert same(again[0], ang) and same(again[1], err) and np.array_equal(again[2], acc)         # two runs: the same bits
    assert (acc[:, :, 70] == np.array(SUPPORT)[None, :]).all()
    assert acc[2, 4, 4] == acc[0, 4, 4] - 1 and np.array_equal(acc[2, 5:], acc[0, 5:])           # the NaN row reaches no other recording
    assert np.isnan(ang[2, 299]).all() and np.isfinite(ang[2, 260:299, 0]).all()
    # sets of wide rows further apart than F rows: strided both ways, no copy
    big = torch.full((3, F + 5, WIDE), float("nan"), dtype=torch.float64, device="cuda")
    big[:, :F, :25] = sets
    view = big[:, :F, :25]
    assert score._sets_view(view, 25, "rows")[0].data_ptr() == big.data_ptr()
    a2, e2, acc2 = run(HIPS, view, "msg", td, "est", LAGS)
    assert same(a2, ang) and same(e2, err) and np.array_equal(acc2, acc)
    with pytest.raises(UserWarning):
        score.joint_angles(HIPS, torch.zeros((65, 4, 25), dtype=torch.float64, device="cuda"))
    with pytest.raises(UserWarning):
        score.joint_angles(HIPS, sets, "msg", rec_lags=LAGS, starts=STARTS)                      # lags without truth


def test_a_frame_of_a_live_bank_is_the_same_call():
    """[S, 25] messages, R = 1, no accumulators: the C entry with acc_dev NULL"""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.score import joint_angles_numpy
    S = 300
    msg = planted_rows(HIPS, "msg", 3, 252)[200:200 + S]
    ptrs = {"rows": dev(msg), "angles": torch.full((S, 7), -7.0, dtype=torch.float64, device="cuda")}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = {k: C.c_void_p(t.data_ptr()) for k, t in ptrs.items()}
    rc = call_entry(vp, truth=None, errors=None, acc=None, F=S, starts=(0,), stream=stream)
    assert rc == 0, _hip.lib().ape_last_error()
    torch.cuda.synchronize()
    ref = joint_angles_numpy(msg, HIPS, "msg")[0]
    check_rows(ptrs["angles"].cpu().numpy(), ref, 8 * U * np.abs(ref), "bank frame", PERIODIC)


# ---------------- 3: the refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    n = 10
    bufs = {"rows": dev(planted_rows(HIPS, "msg", 3, 252)[:n]), "truth": dev(planted_rows(HIPS, "est", 50, 600)[:n]),
            "angles": torch.full((2, n, 7), -7.0, dtype=torch.float64, device="cuda"),
            "errors": torch.full((2, n, 7), -7.0, dtype=torch.float64, device="cuda"),
            "acc": torch.full((2, 3, 71), -7.0, dtype=torch.float64, device="cuda")}
    ptrs = {k: C.c_void_p(t.data_ptr()) for k, t in bufs.items()}
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kw, what in refusals():
        rc = call_entry(ptrs, stream=stream, **kw)
        assert rc == 1 and what in lib.ape_last_error(), (kw, rc, lib.ape_last_error())
    # a capturing stream: the entry stages host arrays per call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros((4,), device="cuda")
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            rc, msg = call_entry(ptrs, stream=C.c_void_p(side.cuda_stream)), lib.ape_last_error()
    torch.cuda.current_stream().wait_stream(side)
    assert rc == 1 and b"capturing" in msg and b"joint_angles" in msg, (rc, msg)
    torch.cuda.synchronize()
    for name in ("angles", "errors", "acc"):
        assert (bufs[name] == -7.0).all(), name             # nothing was written
    assert call_entry(ptrs, stream=stream) == 0             # the same arguments, accepted
    torch.cuda.synchronize()
    assert float(bufs["acc"][0, 0, 70]) == 3.0 and bool(torch.isfinite(bufs["angles"][0, :, 0]).all()) and bool((bufs["angles"][1] == -7.0).all())


# ---------------- 4: histograms over [angles | errors] -----------------------------------------------------------------------------------------
def test_hist_rows_over_angles_and_errors():
    from wear_mocap_ape_amd import score
    rows, truth = rows_and_truth(HIPS, "msg", "est")
    a, e, _ = score.joint_angles(HIPS, dev(rows), "msg", dev(truth), "est", STARTS, SKIP, LAGS)
    both = torch.cat([a, e], dim=1)
    edges = score.angle_edges()
    hist = score.hist_rows(both, edges, STARTS, SKIP)
    torch.cuda.synchronize()
    h = hist.cpu().numpy()
    assert h.shape == (len(STARTS), 14, 75) and (h.sum(axis=2) == np.array(SUPPORT)[:, None]).all()
    assert np.array_equal(h, score.hist_numpy(both.cpu().numpy(), edges, STARTS, SKIP))
    assert not h[:, :, 72:74].any() and h[:, 1, 74].sum() > 0 and h[:, 7, 74].sum() > 0          # nothing outside the ranges; NaNs counted
    # the share of the frames whose flexion error lies within 5 degrees, off the edges at -5 and +5 degrees (bins 35 and 37 of 72)
    lo, hi = edges[7, 35], edges[7, 37]
    assert abs(hi - np.radians(5.0)) <= 1e-15 and abs(lo + np.radians(5.0)) <= 1e-15
    share = score.fraction_within(h[6, 7:8], edges[7:8], [[lo, hi]])
    v = e[301 + SKIP:900, 0].cpu().numpy()
    v = v[np.isfinite(v)]
    assert share.shape == (1, 2) and abs((share[0, 1] - share[0, 0]) - ((v > lo) & (v <= hi)).sum() / v.shape[0]) <= 1e-12
    med = score.quantiles(h[:, 0:1], edges[0:1], [0.5])
    assert np.isfinite(med["value"][[0, 1, 6, 7]]).all()


# ---------------- 5: end to end ----------------------------------------------------------------------------------------------------------------
def test_angles_recording_pocket(golden, tmp_path_factory):
    from tests.test_post_sweep_gpu import pocket
    from tests.test_replay import _synthetic_rows
    from wear_mocap_ape_amd import score
    n, starts, seed = 150, [0, 3, 40, 41], 0x5EED
    est = pocket(tmp_path_factory.mktemp("angles"), 1, 25)
    rows = _synthetic_rows(golden, "pocket", n, 21)
    out, y = est.process_recording(rows, starts=starts, return_targets=True, seed=seed)
    truth = (y.double().mean(dim=1) * torch.as_tensor(est._yy_s, device=y.device) + torch.as_tensor(est._yy_m, device=y.device)).contiguous()
    skip = est.sequence_len - 1
    a1, e1, acc1 = est.angles_recording(out, truth, starts=starts, per_frame=True, rec_lags=[0, 0, 1, 0])
    a2, e2, acc2 = score.joint_angles(est._layout, out, "msg", truth, "targets", starts, skip, [0, 0, 1, 0], est.body_measurements, 0.05, True)
    torch.cuda.synchronize()
    assert torch.equal(acc1, acc2) and same(a1.cpu().numpy(), a2.cpu().numpy()) and same(e1.cpu().numpy(), e2.cpu().numpy())
    assert tuple(a1.shape) == (n, 7) and acc1[:, 70].tolist() == [float(max(0, k - skip)) for k in (3, 37, 1, 109)]
    none, nerr, acc3 = est.angles_recording(out, starts=starts)
    assert none is None and nerr is None and torch.equal(acc3[:, :35], acc1[:, :35]) and not bool(acc3[:, 35:70].any())
    # the truth here is the mean of the replay's own samples in target space: the errors are what averaging quaternions instead of
    # 6D targets leaves; the flexion is always stated, so all 109 - 5 frames of the last recording's support carry an error
    s = score.summarise_angles(acc1)[3]
    assert s["deg"]["elbow_flexion"]["error_count"] == 104 == s["frames"]
    print(f"pocket replay against its own targets: elbow flexion rmse {s['deg']['elbow_flexion']['rmse']:.2e} deg over "
          f"{s['deg']['elbow_flexion']['error_count']} frames, range of motion {s['deg']['elbow_flexion']['rom']:.1f} deg")
    t1 = est.truth_angles(truth, starts=starts)
    t2 = score.joint_angles(est._layout, truth, "targets", None, "est", starts, skip, None, est.body_measurements, 0.05, False)
    assert t1[0] is None and t1[1] is None and torch.equal(t1[2], t2[2])


def test_angles_recording_fk_only(golden):
    from wear_mocap_ape_amd import score
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    est_obj = WatchPhoneUarm(smooth=5)
    rows = np.tile(golden("stream_trace_uarm.npz")["rows"].astype(np.float32), (3, 1))[:60]
    starts = [0, 20, 40]
    out = est_obj.process_recording(rows, starts=starts)
    _, _, a1 = est_obj.angles_recording(out, starts=starts)
    _, _, a2 = score.joint_angles(est_obj._layout, out, "msg", None, "est", starts, 0, per_frame=False)
    assert torch.equal(a1, a2) and a1[:, 70].tolist() == [20.0, 20.0, 20.0] and a1[:, 4].tolist() == [20.0, 20.0, 20.0]
    _, _, a3 = est_obj.angles_recording(out, starts=starts, skip=4)
    assert a3[:, 70].tolist() == [16.0, 16.0, 16.0]
    est_rows = torch.zeros((60, 21 if est_obj._layout != WATCH else 14), dtype=torch.float64, device="cuda")
    ql = 6 if est_obj._layout == WATCH else 9
    est_rows[:, ql:ql + 4] = out[:, 7:11].double()
    est_rows[:, ql + 4:ql + 8] = out[:, 14:18].double()
    if est_obj._layout != WATCH:
        est_rows[:, 17:21] = out[:, 21:25].double()
    _, _, t1 = est_obj.truth_angles(est_rows, "est", starts=starts)
    assert t1[:, 70].tolist() == [20.0, 20.0, 20.0] and torch.equal(t1[:, :35], a1[:, :35])      # the same quaternions as est rows


def test_angles_recording_kalman(golden):
    from oracle import kalman_oracle as ko
    from tests.test_kalman_bank_gpu import _estimator, make_rows
    from wear_mocap_ape_amd import score
    E, W, smooth = 16, 4, 2
    est_obj = _estimator(ko.make_state_dict(W, 36), E, W, smooth=smooth)
    rows = make_rows(np.random.default_rng(36), 60)
    starts = [0, 20, 40]
    out, _, rec = est_obj.process_recording(rows, starts=starts, seed=4242, spread=True)
    _, _, a1 = est_obj.angles_recording(out, starts=starts)
    _, _, a2 = score.joint_angles(est_obj._layout, out, "msg", None, "est", starts, W + 1, per_frame=False)
    assert torch.equal(a1, a2) and a1[:, 70].tolist() == [20.0 - W - 1] * 3 and float(a1[:, 4].sum()) > 0
