"""Speed, acceleration and jerk of a replay (`ape_motion_sums`) on the GPU.

Reference of every per-frame value: `score.motion_sums_numpy` (plain numpy, the header's operations in their order) on the same rows --
for float32 rows the statement of the rounded rows; of the accumulators: numpy sums over the call's own per-frame rows.

F = 1000 frames, recordings starting at 0, 37, 253, 256, 257, 300, 301 and 900 (three rows before, at and one row past the edge of a
256-frame tile; a one-frame recording at 300), skip = 2, poses of `tests/test_frame_fit_cpu.walk_est`; one NaN row and, on the
jittered clock, one repeated stamp are planted so that the NaN pattern is not trivial.

Tolerances and where they come from (u = 2^-53):
* columns [0:6] are made of +, -, *, /, sqrt only, each correctly rounded and in the statement's order, from poses that are copies of
  the rows (messages, est rows) or, for target rows, the float64 forward kinematics that `score._pose_rows` restates operation for
  operation: the statement's bits are asserted.
* columns [6:12] differ from the statement by the two atan2 implementations, a few ulp of the angle.  An angular speed is
  |w| = 2 atan2(n, d.w) / h1: allowed 8 u |w|.  An angular acceleration differences two such velocities over the half span: allowed
  8 u (|w(f)| + |w(f-1)|) / half span, frame by frame, |w(f-1)| made from rows f-1 and f-2 by the statement's operations
  (`prev_speeds`).  The worst fraction of the allowance used is printed.
* sums within 16 n u max(1, max term) of numpy's sums of the call's own rows (the rule of tests/test_frame_fit_gpu.py); maxima and
  counts exact.
* planted noise.  The walk's own hand jerk (rms 0.12 per frame^3) would swamp 1 mm of noise, so here the hand moves on a slow smooth
  curve (0.3 m sinusoids of 400 - 530 frames: a jerk of 1e-6 per frame^3) under the walk's quaternions.  Hand positions p + e, e iid
  normal with sigma = 1 mm per component, on the index clock (h = 1).  The jerk vector becomes J + N with
  N = e(f) - 3 e(f-1) + 3 e(f-2) - e(f-3): E |N|^2 = 3 x 20 sigma^2 = 60 sigma^2 / h^6, so the mean square of the jerk rises by
  60 sigma^2 plus the mean of 2 J.N.  Sampling error: a component of N is Gaussian with autocovariance c = (20, -15, 6, -1) sigma^2 at
  lags 0 .. 3 inside a recording's support and 0 beyond, so Var sum N^2 = 2 sum_fg c(f-g)^2 per component (three of them) and
  Var sum 2 J.N = 4 sum_fg c(f-g) J(f).J(g) with the known J of the clean curve; the two are uncorrelated (odd moments).  `noise_sd`
  sums both over the pairs (f, g) of every support exactly.  Four standard deviations are asserted to be below a quarter of the
  effect (they are 16 % of it), and the rise within four of them.  The seed is one at which the numpy statement passes."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_frame_fit_cpu import msgs_from_est, qmat, walk_est

pytestmark = pytest.mark.gpu

HIPS, WATCH, POS = 0, 1, 2
U = 2.0 ** -53
F, STARTS, SKIP = 1000, [0, 37, 253, 256, 257, 300, 301, 900], 2
ENDS = STARTS[1:] + [F]
SUPPORT = [max(0, e - s - SKIP - 3) for s, e in zip(STARTS, ENDS)]
WIDE = 70
SIGMA, NOISE_SEED = 1e-3, 11


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def same(a, b):
    """bit-equal up to the NaN payload"""
    return np.array_equal(a, b, equal_nan=True)


def default_body():
    from wear_mocap_ape_amd.data_types.bone_map import body9_from_bonemap
    return body9_from_bonemap(None)


def targets_from_est(est, layout):
    """NN targets that state the est rows' pose: 6D rotations (the first two columns of the matrices, row by row), the hips yaw as
    (sin, cos), and for the layout that predicts them the positions"""
    ql, qu = (6, 10) if layout == WATCH else (9, 13)
    six = lambda q: qmat(q)[:, :, :2].reshape(-1, 6)        # noqa: E731
    cols = [six(est[:, ql:ql + 4]), six(est[:, qu:qu + 4])]
    if layout != WATCH:
        w, y = est[:, 17], est[:, 19]
        cols.append(np.stack([2.0 * w * y, w * w - y * y], axis=1))
    if layout == POS:
        cols = [est[:, 0:3], cols[0], est[:, 3:6], cols[1], cols[2]]
    return np.concatenate(cols, axis=1)


_ROWS = {}


def rows_of(layout, kind):
    """float64 rows [F, w] of a kind stating the walk of this layout (made once)"""
    if (layout, kind) not in _ROWS:
        est = walk_est(F, layout, seed=3 + layout)
        _ROWS[layout, "est"] = est
        _ROWS[layout, "msg"] = msgs_from_est(est, layout)
        _ROWS[layout, "targets"] = targets_from_est(est, layout)
    return _ROWS[layout, kind]


def jittered_clock():
    rng = np.random.default_rng(5)
    t = np.empty(F)
    for s, e in zip(STARTS, ENDS):
        dt = 0.02 * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=e - s))
        dt[0] = 0.0
        t[s:e] = np.cumsum(dt)
    t[700] = t[699]                                         # a repeated stamp
    return t


def run(layout, rows, kind, times=None, per_frame=True, **kw):
    from wear_mocap_ape_amd import score
    m, a = score.motion_sums(layout, rows, kind, STARTS, SKIP, None if times is None else dev(times), per_frame=per_frame, **kw)
    torch.cuda.synchronize()
    return (None if m is None else m.cpu().numpy()), a.cpu().numpy()


def half_spans(times):
    if times is None:
        return np.ones(F)
    h = np.ones(F)
    h[2:] = (times[2:] - times[:-2]) / 2.0
    return h


def prev_speeds(rows, layout, kind, times, bodies=None):
    """|w(f-1)| `[F, 3]` of the three joints: the angular velocity over the step into frame f - 1, by the statement's own operations
    on rows f - 1 and f - 2 (NaN in the first two rows; whatever the rows give where they are not of one recording)"""
    from wear_mocap_ape_amd import score
    rows = np.asarray(rows, dtype=np.float64)
    st = np.asarray(STARTS)
    rec = np.searchsorted(st, np.arange(F), side="right") - 1
    t = (np.arange(F) - st[rec]).astype(np.float64) if times is None else times
    body = None
    if kind == "targets":
        b = score._body_rows(bodies, len(STARTS), "bodies")
        body = b[rec] if b.shape[0] > 1 else np.broadcast_to(b, (F, 9))
    out = np.full((F, 3), np.nan)
    with np.errstate(all="ignore"):
        pose, _ = score._pose_rows(rows, layout, kind, body)
        for j in range(3):
            q = score._unit4(pose[:, 6 + 4 * j:10 + 4 * j])
            w = score._ang_vel(q[1:-1], q[:-2], t[1:-1] - t[:-2])
            out[2:, j] = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
    return out


def check_rows(got, ref, times, what, wprev):
    """the NaN pattern and columns [0:6] bit for bit, [6:12] within the atan2 allowance (`wprev`: `prev_speeds` of the rows) -> worst
    fraction of the allowance used"""
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = np.isfinite(ref[:, 0])
    assert np.array_equal(got[ok, :6], ref[ok, :6]), (what, float(np.abs(got[ok, :6] - ref[ok, :6]).max()))
    assert np.isfinite(wprev[ok]).all(), what
    allow = np.concatenate([8 * U * ref[ok, 6:9], 8 * U * (ref[ok, 6:9] + wprev[ok]) / half_spans(times)[ok, None]], axis=1)
    diff = np.abs(got[ok, 6:] - ref[ok, 6:])
    assert (diff <= allow).all(), (what, float((diff / np.where(allow > 0, allow, 1.0)).max()))
    nz = allow > 0
    return float((diff[nz] / allow[nz]).max(initial=0.0))


def check_acc(acc, rows, what):
    """the accumulators against numpy's sums of the call's own per-frame rows; maxima and counts exact"""
    assert acc.shape == (len(STARTS), 38), what
    for r, (s, e) in enumerate(zip(STARTS, ENDS)):
        seg = rows[min(s + SKIP + 3, e):e].astype(np.float64)
        use = seg[np.isfinite(seg[:, 0])]
        n = max(1, use.shape[0])
        assert acc[r, 36] == use.shape[0] and acc[r, 37] == seg.shape[0] - use.shape[0] and acc[r, 36] + acc[r, 37] == SUPPORT[r], (what, r)
        for k in range(12):
            top = float(use[:, k].max(initial=0.0))
            assert acc[r, 3 * k + 2] == top, (what, r, k)
            assert abs(acc[r, 3 * k] - use[:, k].sum()) <= 16 * n * U * max(1.0, top), (what, r, k)
            assert abs(acc[r, 3 * k + 1] - (use[:, k] * use[:, k]).sum()) <= 16 * n * U * max(1.0, top * top), (what, r, k)
    assert not acc[5].any()                                 # the one-frame recording


# ---------------- 1: per-frame rows and accumulators against the statement -------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["msg", "est", "targets"])
@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_rows_and_sums_against_the_statement(layout, kind):
    from wear_mocap_ape_amd.score import motion_sums_numpy
    rows = rows_of(layout, kind).copy()
    w = rows.shape[1]
    rows[510, {"msg": 12, "est": 4, "targets": 1}[kind]] = np.nan                        # blanks 510 .. 513, across the tile edge at 512
    body = default_body()
    kw = dict(bodies=body) if kind == "targets" else {}
    clock = jittered_clock()
    worst = 0.0
    for dtype, npdt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        stored = rows.astype(npdt)
        plain = dev(stored)
        wide = torch.full((F, WIDE), float("nan"), dtype=dtype, device="cuda")
        wide[:, :w] = plain
        for times in (None, clock):
            ref, ref_acc = motion_sums_numpy(stored, layout, kind, STARTS, SKIP, times, **kw)
            gone = np.isnan(ref[:, 0])
            want_gone = np.zeros(F, dtype=bool)
            for s in STARTS:
                want_gone[s:s + 3] = True
            want_gone[510:514] = True
            if times is not None:
                want_gone[700:703] = True
            assert np.array_equal(gone, want_gone[:F]), (layout, kind)                    # (the statement itself; tests/test_motion_cpu.py)
            wprev = prev_speeds(stored, layout, kind, times, **kw)
            for name, view in (("contiguous", plain), ("strided", wide[:, :w])):
                what = (layout, kind, str(dtype), name, times is not None)
                got, acc = run(layout, view, kind, times, out_dtype=torch.float64, **kw)
                worst = max(worst, check_rows(got, ref, times, what, wprev))
                check_acc(acc, got, what)
                assert np.array_equal(acc[:, 36:], ref_acc[:, 36:]), what
                if layout == WATCH:
                    ok = np.isfinite(got[:, 0])
                    assert (got[ok][:, [8, 11]] == 0.0).all() and not acc[:, [24, 25, 26, 33, 34, 35]].any(), what
            # the accumulators do not depend on the per-frame rows being written; the default output type is the rows'
            none, acc2 = run(layout, plain, kind, times, per_frame=False, **kw)
            assert none is None and np.array_equal(acc, acc2)
            own, acc3 = run(layout, plain, kind, times, **kw)
            assert own.dtype == npdt and np.array_equal(acc, acc3) and same(own, got.astype(npdt))
    print(f"layout {layout}, {kind} rows: columns [0:6] bit-equal; worst fraction of the atan2 allowance used in [6:12] = {worst:.3f}")


def test_a_body_per_recording():
    """target rows are converted with their own recording's body, the halo rows below a tile edge included"""
    from wear_mocap_ape_amd.score import motion_sums_numpy
    rows = rows_of(HIPS, "targets")
    rng = np.random.default_rng(9)
    bodies = default_body()[None, :] * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, size=(len(STARTS), 9)))
    ref, _ = motion_sums_numpy(rows, HIPS, "targets", STARTS, SKIP, bodies=bodies)
    got, acc = run(HIPS, dev(rows), "targets", bodies=bodies)
    check_rows(got, ref, None, "bodies", prev_speeds(rows, HIPS, "targets", None, bodies))
    check_acc(acc, got, "bodies")
    one, _ = run(HIPS, dev(rows), "targets", bodies=bodies[0])
    assert same(one[:37], got[:37]) and not same(one[37:], got[37:])


# ---------------- 2: sets --------------------------------------------------------------------------------------------------------------------
def noisy_sets():
    msg = rows_of(HIPS, "msg")
    noisy = msg.copy()
    noisy[:, 4:7] += SIGMA * np.random.default_rng(NOISE_SEED).normal(size=(F, 3))
    holed = msg.copy()
    holed[299] = np.nan                                     # the last row of the recording 257 .. 299
    return np.stack([msg, noisy, holed])


def test_sets_are_single_set_calls_bit_for_bit():
    from wear_mocap_ape_amd import score
    sets = dev(noisy_sets())
    clock = jittered_clock()
    for times in (None, clock):
        motion, acc = run(HIPS, sets, "msg", times)
        assert motion.shape == (3, F, 12) and acc.shape == (3, len(STARTS), 38)
        for c in range(3):
            m1, a1 = run(HIPS, sets[c], "msg", times)
            assert same(motion[c], m1) and np.array_equal(acc[c], a1), c
        again = run(HIPS, sets, "msg", times)
        assert same(again[0], motion) and np.array_equal(again[1], acc)                   # two runs: the same bits
        assert (acc[:, :, 36] + acc[:, :, 37] == np.array(SUPPORT)[None, :]).all()
        assert acc[2, 4, 37] == 1 and acc[2, 5, 37] == 0 and acc[2, 7, 37] == 0           # the NaN row reaches no other recording
        assert acc[2, 6, 37] == (0 if times is None else 3)                               # (the repeated stamp's three rows)
        assert np.isnan(motion[2, 299]).all() and np.isfinite(motion[2, 260:299]).all() and np.isfinite(motion[2, 304:700]).all()
    # sets of wide rows further apart than F rows: strided both ways, no copy
    big = torch.full((3, F + 5, WIDE), float("nan"), dtype=torch.float64, device="cuda")
    big[:, :F, :25] = sets
    view = big[:, :F, :25]
    assert score._sets_view(view, 25, "rows")[0].data_ptr() == big.data_ptr()
    m2, a2 = run(HIPS, view, "msg", clock)
    assert same(m2, motion) and np.array_equal(a2, acc)
    with pytest.raises(UserWarning):
        score.motion_sums(HIPS, torch.zeros((65, 4, 25), dtype=torch.float64, device="cuda"))


# ---------------- 3: planted noise -----------------------------------------------------------------------------------------------------------
STENCIL_COV = (20.0, -15.0, 6.0, -1.0)                     # autocovariance of e(f) - 3 e(f-1) + 3 e(f-2) - e(f-3) at lags 0 .. 3, in sigma^2


def calm_sets():
    """(clean, noisy) messages [2, F, 25]: the walk's quaternions, the hand on a slow smooth curve, and the same plus the planted noise"""
    clean = rows_of(HIPS, "msg").copy()
    f = np.arange(F, dtype=np.float64)
    clean[:, 4:7] = 0.3 * np.stack([np.sin(2 * np.pi * f / 400.0), np.cos(2 * np.pi * f / 530.0 + 1.0), np.sin(2 * np.pi * f / 470.0 + 2.0)], axis=1)
    noisy = clean.copy()
    noisy[:, 4:7] += SIGMA * np.random.default_rng(NOISE_SEED).normal(size=(F, 3))
    return np.stack([clean, noisy])


def noise_sd(hand):
    """one standard deviation of the rise of the mean square jerk over all supports, from the clean curve's own jerk vectors"""
    J = np.zeros((F, 3))
    J[3:] = hand[3:] - 3.0 * hand[2:-1] + 3.0 * hand[1:-2] - hand[:-3]
    var_nn = var_jn = 0.0
    for s, e in zip(STARTS, ENDS):
        a = min(s + SKIP + 3, e)
        for k, c in enumerate(STENCIL_COV):
            if e - a - k <= 0:
                continue
            twice = 1.0 if k == 0 else 2.0                  # the pairs (f, f + k) and (f + k, f)
            var_nn += 3 * 2.0 * twice * (e - a - k) * c * c * SIGMA ** 4
            var_jn += 4.0 * twice * c * float((J[a + k:e] * J[a:e - k]).sum()) * SIGMA ** 2
    return np.sqrt(var_nn + var_jn) / sum(SUPPORT)


def noise_rise(acc_clean, acc_noisy):
    """rise of the hand jerk's mean square over all recordings"""
    n = acc_clean[:, 36].sum()
    assert n == acc_noisy[:, 36].sum() == sum(SUPPORT)
    return acc_noisy[:, 7].sum() / n - acc_clean[:, 7].sum() / n


def test_planted_noise_raises_the_jerk_by_what_it_must():
    from wear_mocap_ape_amd.score import motion_sums_numpy
    sets = calm_sets()
    want, sd = 60.0 * SIGMA ** 2, noise_sd(sets[0][:, 4:7])
    assert 4 * sd <= 0.25 * want, (sd, want)                                              # the test resolves the effect: a rise of 0 fails
    ref = [motion_sums_numpy(sets[c], HIPS, "msg", STARTS, SKIP)[1] for c in (0, 1)]
    assert ref[0][:, 7].sum() / sum(SUPPORT) <= 1e-3 * want                               # the clean curve's own jerk is nothing beside it
    rise = noise_rise(*ref)
    assert abs(rise - want) <= 4 * sd, ("the numpy statement alone", rise, want, sd)
    _, acc = run(HIPS, dev(sets), "msg", per_frame=False)
    rise = noise_rise(acc[0], acc[1])
    print(f"planted noise of {SIGMA} m: the hand jerk's mean square rises by {rise:.4e}, expected {want:.4e} +- {sd:.2e} (one sd, "
          f"{(rise - want) / sd:+.2f} sd off)")
    assert abs(rise - want) <= 4 * sd, (rise, want, sd)
    assert np.array_equal(acc[0][:, 9:], acc[1][:, 9:])                                   # nothing but the hand's three values moves


# ---------------- 4: end to end --------------------------------------------------------------------------------------------------------------
def test_sweep_recording_carries_the_motion_sums(golden, tmp_path_factory):
    from tests.test_post_sweep_gpu import pocket
    from tests.test_replay import _synthetic_rows
    from wear_mocap_ape_amd import score
    n, starts, seed = 150, [0, 3, 40, 41], 0x5EED
    est = pocket(tmp_path_factory.mktemp("motion"), 1, 25)
    rows = _synthetic_rows(golden, "pocket", n, 21)
    out1, y = est.process_recording(rows, starts=starts, return_targets=True, seed=seed)
    configs = score.grid((1, 5, 10), (25,))
    out = est.repost(y, configs, starts=starts)
    _, acc = score.motion_sums(est._layout, out, "msg", starts, est.sequence_len - 1)
    truth = (y.double().mean(dim=1) * torch.as_tensor(est._yy_s, device=y.device) + torch.as_tensor(est._yy_m, device=y.device)).contiguous()
    res = est.sweep_recording(rows, truth, (1, 5, 10), (25,), starts=starts, seed=seed, motion=True)
    torch.cuda.synchronize()
    assert res["configs"] == configs and isinstance(res["motion"], np.ndarray) and res["motion"].shape == (3, 4, 38)
    assert np.array_equal(res["motion"], acc.cpu().numpy())
    plain = est.sweep_recording(rows, truth, (1, 5, 10), (25,), starts=starts, seed=seed)
    assert sorted(plain) == ["acc", "best", "configs"] and np.array_equal(plain["acc"], res["acc"])
    for c, cfg in enumerate(configs):
        s = score.summarise_motion(res["motion"][c])[3]
        print(f"smooth {cfg[0]:2d}: hand jerk rms over {s['scored']} frames of the 109-frame recording = {s['rms']['hand_jerk']:.4e} per frame^3")
    # motion_recording is motion_sums with the class's layout and skip; truth_motion the same for the truth
    m1, a1 = est.motion_recording(out1, starts=starts, per_frame=True)
    m2, a2 = score.motion_sums(est._layout, out1, "msg", starts, est.sequence_len - 1, per_frame=True)
    assert torch.equal(a1, a2) and same(m1.cpu().numpy(), m2.cpu().numpy()) and tuple(m1.shape) == (n, 12)
    assert np.array_equal(a1.cpu().numpy(), res["motion"][0])                             # configuration (1, 25) is the replay itself
    none, t1 = est.truth_motion(truth, starts=starts)
    t2 = score.motion_sums(est._layout, truth, "targets", starts, est.sequence_len - 1, bodies=est.body_measurements)[1]
    assert none is None and torch.equal(t1, t2)
    assert (t1[:, 36] + t1[:, 37]).tolist() == [float(max(0, k - 3 - (est.sequence_len - 1))) for k in (3, 37, 1, 109)]


def test_motion_recording_fk_only(golden):
    from wear_mocap_ape_amd import score
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    est_obj = WatchPhoneUarm(smooth=5)
    rows = np.tile(golden("stream_trace_uarm.npz")["rows"].astype(np.float32), (3, 1))[:60]
    starts = [0, 20, 40]
    out = est_obj.process_recording(rows, starts=starts)
    _, a1 = est_obj.motion_recording(out, starts=starts)
    _, a2 = score.motion_sums(est_obj._layout, out, "msg", starts, 0)
    assert torch.equal(a1, a2) and a1[:, 36].tolist() == [17.0, 17.0, 17.0] and not bool(a1[:, [24, 25, 26, 33, 34, 35]].any())
    _, a3 = est_obj.motion_recording(out, starts=starts, skip=4)
    assert a3[:, 36].tolist() == [13.0, 13.0, 13.0]


def test_motion_recording_kalman(golden):
    from oracle import kalman_oracle as ko
    from tests.test_kalman_bank_gpu import _estimator, make_rows
    from wear_mocap_ape_amd import score
    E, W, smooth = 16, 4, 2
    est_obj = _estimator(ko.make_state_dict(W, 36), E, W, smooth=smooth)
    rows = make_rows(np.random.default_rng(36), 60)
    starts = [0, 20, 40]
    out, _, rec = est_obj.process_recording(rows, starts=starts, seed=4242, spread=True)
    _, a1 = est_obj.motion_recording(out, starts=starts)
    _, a2 = score.motion_sums(est_obj._layout, out, "msg", starts, W + 1)
    assert torch.equal(a1, a2) and (a1[:, 36] + a1[:, 37]).tolist() == [20.0 - 3 - W - 1] * 3 and float(a1[:, 36].sum()) > 0


# ---------------- 5: a capturing stream ------------------------------------------------------------------------------------------------------
def test_a_capturing_stream_is_refused():
    """the entry stages host arrays per call: on a stream that is capturing a graph it returns APE_ERR_INVALID_ARG and writes nothing"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    n = 64
    msg = dev(rows_of(HIPS, "msg")[:n])
    acc = torch.full((1, 1, 38), -7.0, dtype=torch.float64, device="cuda")
    motion = torch.full((1, n, 12), -7.0, dtype=torch.float64, device="cuda")
    st = np.zeros(1, dtype=np.int32)
    ptr = lambda t: C.c_void_p(t.data_ptr())                # noqa: E731

    def call(stream):
        return lib.ape_motion_sums(HIPS, ptr(msg), _hip.ROWS_MSG, 25, _hip.F64, 1, 0, n, C.c_void_p(st.ctypes.data), 1, 0, None, None, 0,
                                   ptr(motion), _hip.F64, ptr(acc), stream)

    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros((4,), device="cuda")
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            rc, err = call(C.c_void_p(side.cuda_stream)), lib.ape_last_error()
    torch.cuda.current_stream().wait_stream(side)
    assert rc == 1 and b"capturing" in err and b"motion_sums" in err, (rc, err)
    torch.cuda.synchronize()
    assert (acc == -7.0).all() and (motion == -7.0).all()   # nothing was written
    assert call(C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0                # the same arguments on a stream that is not capturing
    torch.cuda.synchronize()
    assert float(acc[0, 0, 36]) == n - 3 and bool(torch.isfinite(motion[0, 3:]).all())
