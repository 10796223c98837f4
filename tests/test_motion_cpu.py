"""Speed, acceleration and jerk of a replay without a GPU: the numpy statement `score.motion_sums_numpy` against closed
forms on a jittered clock, its bookkeeping, the agreement of the row kinds, the header and the binding, and every refusal of
`ape_motion_sums` that needs no device (all are made on the host; the capturing stream is refused in tests/test_motion_gpu.py).

Tolerances and where they come from (u = 2^-53, h = 0.02 s the nominal step, steps drawn from h +- 30 %, P = max |p|):
* cubic positions.  A k-th divided difference is sum_i p_i / prod_{j != i} (t_i - t_j).  The rows hold p rounded to float64, an error of
  u P each, so the value moves by u P sum_i 1 / |prod|.  With steps of at least 0.7 h the sums are at most 2 / (0.7 h) = 2.9 / h,
  4.1 / h^2 and 3.9 / h^3; times the factors 1, 2 and 6 of speed, acceleration and jerk: 2.9 u P / h, 8.2 u P / h^2, 23.3 u P / h^3.  The
  float64 arithmetic of the statement adds roundings of the same size on the same terms.  Asserted: 16 u P / h, 32 u P / h^2 and
  64 u P / h^3, each plus 8 u |value| for the roundings of the result itself.
* constant-rate turn.  A stored unit quaternion is off by at most 3 u in norm (rounding of four components, the normalisation); the
  product of two is off by 2 x 3 u plus 3 u of its own roundings, the angle 2 atan2 by twice that: 18 u, over a step of at least
  0.7 h: 26 u / h.  Asserted: 64 u / h on the angular speed; the angular acceleration differences two such velocities over a half span of
  at least 0.7 h: 74 u / h^2, asserted 128 u / h^2.  The same two bounds hold the results of quaternions scaled by general factors
  to the unscaled ones (the scale only moves normalisation's rounding); sign flips and powers of two change no bit.
* tiny steps.  Below n = 1e-8 the statement takes s = 2 for (2 atan2(n, d.w)) / n.  With |d| = 1 to rounding the two differ by
  n^2 / 6 < u relative and by d.w's own rounding, u; the three float64 operations behind s add 3 u: asserted 8 u relative.
* kinds.  tests/test_score_gpu.py records 1e-13 between the two truth kinds (positions in metres, angles in radians) on these
  fixtures.  On the index clock a speed differences two rows (x 2), an acceleration 2 |d2| three rows with coefficients 1, 2, 1 (x 4), a
  jerk four rows with 1, 3, 3, 1 (x 8); an angular speed two quaternions (x 2), an angular acceleration two velocities over a half
  span of 1 (x 4)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests.test_frame_fit_cpu import msgs_from_est, walk_est

REPO = Path(__file__).resolve().parents[1]
HIPS, WATCH, POS = 0, 1, 2
U = 2.0 ** -53
H = 0.02
LD = np.longdouble


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def jittered_clock(n, seed=0):
    rng = np.random.default_rng(seed)
    dt = H * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=n))
    dt[0] = 0.0
    return np.cumsum(dt)


def still_msgs(n):
    """messages of a pose at rest: positions 0, identity quaternions"""
    m = np.zeros((n, 25))
    m[:, [0, 7, 14, 21]] = 1.0
    return m


def axis_turn(axis, angle):
    """unit quaternions [n, 4] of the turns by `angle [n]` about `axis`, in longdouble"""
    a = np.asarray(axis, dtype=LD)
    a = a / np.sqrt((a * a).sum())
    half = np.asarray(angle, dtype=LD) / 2
    return np.concatenate([np.cos(half)[:, None], np.sin(half)[:, None] * a[None, :]], axis=1)


# ---------------- 1: the statement against closed forms, on a jittered clock -----------------------------------------------------------------
def test_cubic_positions_give_the_closed_forms():
    from wear_mocap_ape_amd.score import motion_sums_numpy
    n = 400
    t = jittered_clock(n, 1)
    rng = np.random.default_rng(2)
    worst = np.zeros(3)
    for cols in ((4, 7), (11, 14)):
        c = rng.normal(size=(4, 3)) * np.array([0.3, 0.2, 0.1, 0.05])[:, None]          # c0 .. c3 per component
        tl = t.astype(LD)[:, None]
        p = c[0].astype(LD) + tl * (c[1].astype(LD) + tl * (c[2].astype(LD) + tl * c[3].astype(LD)))
        m = still_msgs(n)
        m[:, cols[0]:cols[1]] = p.astype(np.float64)
        got, _ = motion_sums_numpy(m, HIPS, "msg", times=t)
        k0 = 0 if cols[0] == 4 else 3
        assert np.isnan(got[:3]).all() and np.isfinite(got[3:]).all()
        P = float(np.abs(p).max())
        t0, t1, t2 = tl[3:], tl[2:-1], tl[1:-2]
        d1 = (p[3:] - p[2:-1]) / (t0 - t1)                                              # the exact difference, in longdouble
        speed = np.sqrt((d1 * d1).sum(axis=1)).astype(np.float64)
        a = 2 * c[2].astype(LD) + 2 * c[3].astype(LD) * (t0 + t1 + t2)                  # 2 c2 + 6 c3 t*, t* the mean of the three stamps
        accel = np.sqrt((a * a).sum(axis=1)).astype(np.float64)
        jerk = 6.0 * float(np.sqrt((c[3].astype(LD) ** 2).sum()))
        for j, (ref, mult, power) in enumerate(((speed, 16, 1), (accel, 32, 2), (jerk, 64, 3))):
            bound = mult * U * P / H ** power + 8 * U * np.abs(ref)
            frac = np.abs(got[3:, k0 + j] - ref) / bound
            worst[j] = max(worst[j], float(frac.max()))
            assert (frac <= 1.0).all(), (cols, j, float(frac.max()))
        assert (got[3:, (3 - k0):(6 - k0)] == 0.0).all() and (got[3:, 6:] == 0.0).all()    # the joint at rest, the quaternions at rest
    print(f"cubic positions: worst fraction of the bound used, speed / acceleration / jerk = {worst[0]:.3f} / {worst[1]:.3f} / {worst[2]:.3f}")


def turning_msgs(n, t, rates, axes, q0s):
    """the three joints turning at `rates` about `axes` from `q0s`: the products made in longdouble and rounded once"""
    from tests.test_frame_fit_cpu import qmul
    m = still_msgs(n)
    for k, c in enumerate((7, 14, 21)):
        m[:, c:c + 4] = qmul(axis_turn(axes[k], rates[k] * t.astype(LD)), np.asarray(q0s[k], dtype=LD)).astype(np.float64)
    return m


def test_a_constant_rate_turn_about_a_fixed_axis():
    from wear_mocap_ape_amd.score import motion_sums_numpy
    n = 400
    t = jittered_clock(n, 3)
    rates = (1.7, 0.4, 3.1)                                                              # rad / s
    axes = ((1.0, 2.0, -0.5), (0.0, 0.0, 1.0), (-1.0, 0.3, 0.2))
    q0s = [np.array(q) / np.linalg.norm(q) for q in ((0.9, 0.1, -0.3, 0.2), (0.2, 0.7, 0.1, -0.6), (1.0, 0.0, 0.0, 0.0))]
    m = turning_msgs(n, t, rates, axes, q0s)
    got, _ = motion_sums_numpy(m, HIPS, "msg", times=t)
    assert np.isnan(got[:3]).all() and np.isfinite(got[3:]).all() and (got[3:, :6] == 0.0).all()
    sb, ab = 64 * U / H, 128 * U / H ** 2
    fs = np.abs(got[3:, 6:9] - np.array(rates)) / sb
    fa = got[3:, 9:12] / ab
    print(f"constant-rate turn: worst fraction of the bound used, angular speed {fs.max():.3f}, angular acceleration {fa.max():.3f}")
    assert (fs <= 1.0).all() and (fa <= 1.0).all(), (float(fs.max()), float(fa.max()))

    # whole quaternions with their sign flipped, or scaled by a power of two: not a bit changes
    rng = np.random.default_rng(4)
    same = m.copy()
    for c in (7, 14, 21):
        same[:, c:c + 4] *= (rng.choice([-1.0, 1.0], size=n) * rng.choice([0.5, 1.0, 4.0], size=n))[:, None]
    again, _ = motion_sums_numpy(same, HIPS, "msg", times=t)
    assert np.array_equal(again, got, equal_nan=True)
    # general scale factors move normalisation's rounding only
    scaled = m.copy()
    for c in (7, 14, 21):
        scaled[:, c:c + 4] *= rng.uniform(0.1, 9.0, size=n)[:, None]
    other, _ = motion_sums_numpy(scaled, HIPS, "msg", times=t)
    assert np.array_equal(other[:, :6], got[:, :6], equal_nan=True)
    assert (np.abs(other[3:, 6:9] - got[3:, 6:9]) <= sb).all() and (np.abs(other[3:, 9:12] - got[3:, 9:12]) <= ab).all()


def test_tiny_steps_agree_with_the_atan2_branch_in_longdouble():
    from wear_mocap_ape_amd import score
    n = 200
    t = jittered_clock(n, 5)
    rng = np.random.default_rng(6)
    angle = np.cumsum(rng.uniform(2e-10, 1.5e-8, size=n))                                # steps of 1e-10 .. 7.5e-9 in n = sin(angle / 2)
    m = still_msgs(n)
    for k, c in enumerate((7, 14, 21)):
        m[:, c:c + 4] = axis_turn(((1.0, 2.0, -0.5), (0.0, 1.0, 0.0), (0.3, 0.2, 1.0))[k], angle).astype(np.float64)
    got, _ = score.motion_sums_numpy(m, HIPS, "msg", times=t)
    assert np.isfinite(got[3:]).all()
    h = np.diff(t)
    for k, c in enumerate((7, 14, 21)):
        q = score._unit4(m[:, c:c + 4])                                                  # the difference quaternion as the statement forms it
        d = score._qmul(q[1:], q[:-1] * np.array([1.0, -1.0, -1.0, -1.0]))
        d = np.where((d[:, 0] < 0.0)[:, None], -d, d)
        nn = np.sqrt((d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) + d[:, 3] * d[:, 3])
        assert (nn < 1e-8).all() and (nn > 0.0).all()                                     # every step takes the small branch
        dl = d.astype(LD)
        nl = np.sqrt(dl[:, 1] * dl[:, 1] + dl[:, 2] * dl[:, 2] + dl[:, 3] * dl[:, 3])
        w = (2 * np.arctan2(nl, dl[:, 0]) / nl)[:, None] * dl[:, 1:] / h.astype(LD)[:, None]         # w[i]: the step into frame i + 1
        speed = np.sqrt((w * w).sum(axis=1))
        ref_s = speed[2:].astype(np.float64)
        assert (np.abs(got[3:, 6 + k] - ref_s) <= 8 * U * ref_s).all(), k
        dw = w[2:] - w[1:-1]
        half = (t[3:] - t[1:-2]).astype(LD) / 2
        ref_a = (np.sqrt((dw * dw).sum(axis=1)) / half).astype(np.float64)
        allow = 8 * U * ((speed[2:] + speed[1:-1]) / half).astype(np.float64)
        assert (np.abs(got[3:, 9 + k] - ref_a) <= allow).all(), k


# ---------------- 2: bookkeeping ---------------------------------------------------------------------------------------------------------------
def walk_msgs(n, layout=HIPS, seed=0):
    return msgs_from_est(walk_est(n, layout, seed), layout)


def test_short_recordings_and_skip():
    from wear_mocap_ape_amd.score import motion_sums_numpy
    starts = [0, 1, 4, 8]                                                                # recordings of 1, 3, 4 and 5 frames
    m = walk_msgs(13)
    for skip, want in ((0, [0, 0, 1, 2]), (1, [0, 0, 0, 1]), (2, [0, 0, 0, 0]), (40, [0, 0, 0, 0])):
        motion, acc = motion_sums_numpy(m, HIPS, "msg", starts, skip)
        assert acc.shape == (4, 38) and motion.shape == (13, 12)
        assert acc[:, 36].tolist() == want and not acc[:, 37].any(), (skip, acc[:, 36:])
        finite = np.isfinite(motion).all(axis=1)
        assert finite.tolist() == [False] * 7 + [True] + [False] * 3 + [True] * 2       # frames 7, 11 and 12: three frames into their recording
        assert np.array_equal(np.isnan(motion).any(axis=1), ~finite)                    # a row is all or nothing
        for r in range(4):
            if want[r] == 0:
                assert not acc[r].any()
    motion, acc = motion_sums_numpy(m, HIPS, "msg", starts, 0)
    assert np.array_equal(acc[2, 0:36:3], motion[7]) and np.array_equal(acc[2, 2:36:3], motion[7]) and np.array_equal(acc[2, 1:36:3], motion[7] ** 2)
    assert np.array_equal(acc[3, 2:36:3], np.maximum(motion[11], motion[12]))


def test_a_nan_row_blanks_four_frames_of_its_own_recording():
    from wear_mocap_ape_amd.score import motion_sums_numpy
    starts, F = [0, 20], 40
    for layout, kind, rows in ((HIPS, "msg", walk_msgs(F)), (WATCH, "est", walk_est(F, WATCH)), (HIPS, "est", walk_est(F, HIPS))):
        clean, acc0 = motion_sums_numpy(rows, layout, kind, starts)
        assert np.isfinite(clean[3:20]).all() and np.isfinite(clean[23:]).all()
        pos = 4 if kind == "msg" else 0                                                   # the hand's x
        for f, col in ((10, pos), (18, pos), (10, {"msg": 15, "est": rows.shape[1] - 1}[kind])):   # mid-recording, two from its end; a quaternion value
            bad = rows.copy()
            bad[f, col] = np.nan
            got, acc = motion_sums_numpy(bad, layout, kind, starts)
            blank = np.zeros(F, dtype=bool)
            blank[f:min(f + 4, 20)] = True
            assert np.array_equal(np.isnan(got).all(axis=1), np.isnan(clean).all(axis=1) | blank), (kind, f, col)
            assert np.array_equal(got[~blank], clean[~blank], equal_nan=True)            # and reaches no other frame, no other recording
            assert acc[0, 37] == blank.sum() and acc[0, 36] == 17 - blank.sum() and np.array_equal(acc[1], acc0[1])
    # a message column the pose does not use is not looked at
    m = walk_msgs(F)
    m[10, [0, 1, 2, 3, 18, 19, 20]] = np.nan
    assert np.array_equal(motion_sums_numpy(m, HIPS, "msg", starts)[0], motion_sums_numpy(walk_msgs(F), HIPS, "msg", starts)[0], equal_nan=True)


def test_repeated_and_backward_stamps_blank_the_three_rows_that_use_them():
    from wear_mocap_ape_amd.score import motion_sums_numpy
    F = 30
    m = walk_msgs(F)
    t = jittered_clock(F, 7)
    clean, _ = motion_sums_numpy(m, HIPS, "msg", times=t)
    for name, stamp in (("repeated", t[11]), ("backward", t[11] - 0.004), ("nan", np.nan), ("inf", np.inf)):
        tt = t.copy()
        tt[12] = stamp
        got, acc = motion_sums_numpy(m, HIPS, "msg", times=tt)
        gone = np.isnan(got).all(axis=1)
        if name in ("repeated", "backward"):                                             # the step into frame 12 is used by frames 12, 13, 14
            assert np.flatnonzero(gone).tolist() == [0, 1, 2, 12, 13, 14], (name, np.flatnonzero(gone))
            assert np.array_equal(got[16:], clean[16:]) and np.array_equal(got[3:12], clean[3:12])
        else:                                                                            # a non-finite stamp spoils the steps on both sides: 12 .. 15
            assert np.flatnonzero(gone).tolist() == [0, 1, 2, 12, 13, 14, 15], (name, np.flatnonzero(gone))
        assert acc[0, 36] + acc[0, 37] == F - 3 and acc[0, 37] == gone.sum() - 3


def test_watch_only_hips_columns_are_exact_zeros_and_the_counts_add_up():
    from wear_mocap_ape_amd.score import motion_sums_numpy
    F, starts = 60, [0, 2, 30, 31]
    for kind, rows in (("msg", walk_msgs(F, WATCH)), ("est", walk_est(F, WATCH))):
        if kind == "msg":
            rows[:, 21:25] = np.nan                                                      # not read without hips
        got, acc = motion_sums_numpy(rows, WATCH, kind, starts, 1)
        ok = np.isfinite(got[:, 0])
        assert ok.sum() == 25 + 26 and (got[ok][:, [8, 11]] == 0.0).all() and (got[ok][:, [6, 7, 9, 10]] > 0.0).all()
        assert not acc[:, [24, 25, 26, 33, 34, 35]].any()
        ends = starts[1:] + [F]
        assert (acc[:, 36] + acc[:, 37]).tolist() == [max(0, e - s - 1 - 3) for s, e in zip(starts, ends)]


def test_merge_motion_of_two_pieces_is_the_whole_but_for_the_joint():
    from wear_mocap_ape_amd.score import merge_motion, motion_sums_numpy, summarise_motion, MOTION_NAMES
    F, cut = 120, 47
    m = walk_msgs(F)
    t = jittered_clock(F, 8)
    whole, acc = motion_sums_numpy(m, HIPS, "msg", times=t)
    _, a = motion_sums_numpy(m[:cut], HIPS, "msg", times=t[:cut])
    _, b = motion_sums_numpy(m[cut:], HIPS, "msg", times=t[cut:])
    merged = merge_motion(a, b)
    assert merged.shape == (1, 38) and merged[0, 36] == acc[0, 36] - 3 and merged[0, 37] == 0
    keep = np.r_[3:cut, cut + 3:F]                                                       # the three frames at the joint are in neither piece
    rows = whole[keep]
    assert np.array_equal(merged[0, 2:36:3], rows.max(axis=0))
    assert np.allclose(merged[0, 0:36:3], rows.sum(axis=0), rtol=1e-13, atol=0) and np.allclose(merged[0, 1:36:3], (rows * rows).sum(axis=0), rtol=1e-13, atol=0)
    with pytest.raises(UserWarning):
        merge_motion(a, np.zeros((2, 38)))
    s = summarise_motion(merged)[0]
    assert s["scored"] == F - 6 and s["left_out"] == 0 and set(s["mean"]) == set(MOTION_NAMES) == set(s["rms"]) == set(s["max"])
    assert s["mean"]["hand_jerk"] == merged[0, 6] / (F - 6) and s["rms"]["hand_jerk"] == np.sqrt(merged[0, 7] / (F - 6)) and s["max"]["hand_jerk"] == merged[0, 8]
    empty = summarise_motion(np.zeros((1, 38)))[0]
    assert empty["scored"] == 0 and np.isnan(empty["mean"]["hand_speed"])


# ---------------- 3: the kinds agree -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_targets_and_est_rows_give_the_same_values(golden, layout):
    from wear_mocap_ape_amd.score import motion_sums_numpy
    g = golden(f"fk_layout{layout}.npz")
    starts = [0, 1, 150]
    a, acc_a = motion_sums_numpy(g["preds_bd_N300"], layout, "targets", starts, bodies=g["body_bd"])
    b, acc_b = motion_sums_numpy(g["est_bd_N300"], layout, "est", starts)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.isfinite(b[:, 0]).sum() == 146 + 147
    amp = np.array([2, 4, 8, 2, 4, 8, 2, 2, 2, 4, 4, 4]) * 1e-13
    ok = np.isfinite(b[:, 0])
    frac = np.abs(a[ok] - b[ok]) / amp
    print(f"targets against est rows, layout {layout}: worst fraction of the allowance used per column {np.round(frac.max(axis=0), 3).tolist()}")
    assert (frac <= 1.0).all(), (layout, frac.max(axis=0))
    assert np.array_equal(acc_a[:, 36:], acc_b[:, 36:])
    # the messages that state the est rows give the est rows' bits
    c, _ = motion_sums_numpy(msgs_from_est(g["est_bd_N300"], layout), layout, "msg", starts)
    assert np.array_equal(c, b, equal_nan=True)


# ---------------- 4: header and binding --------------------------------------------------------------------------------------------------------
def test_header_declares_and_hip_binds_the_entry():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    for name, value in (("APE_MOTION_WIDTH", 12), ("APE_MOTION_ACC_WIDTH", 38), ("APE_ROWS_MSG", 0), ("APE_ROWS_EST", 1), ("APE_ROWS_TARGETS", 2)):
        assert re.search(rf"^#define {name}\s+{value}\b", text, flags=re.M), name
    assert (_hip.MOTION_WIDTH, _hip.MOTION_ACC_WIDTH) == (12, 38) == (score.MOTION_WIDTH, score.MOTION_ACC_WIDTH)
    assert (_hip.ROWS_MSG, _hip.ROWS_EST, _hip.ROWS_TARGETS) == (0, 1, 2) and len(score.MOTION_NAMES) == 12
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    params = ["int32_t layout", "const void* rows_dev", "int32_t rows_kind", "int32_t rows_stride", "int32_t rows_dtype", "int32_t n_sets",
              "int64_t set_stride", "int32_t F", "const int32_t* seg_starts_host", "int32_t R", "int32_t skip", "const double* times_dev",
              "const double* bodies_host", "int32_t n_bodies", "void* motion_dev", "int32_t out_dtype", "double* acc_dev", "void* stream"]
    decl = text[text.index("\nint ape_motion_sums(") + 1:]
    decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
    got = [" ".join(p.split()) for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
    assert got == params, got
    assert text.index("int ape_motion_sums(") > text.index("int ape_rebody_rows(")        # after the 4.37 block
    res, args = _hip.SIGNATURES["ape_motion_sums"]
    assert hasattr(_hip.lib(), "ape_motion_sums") and res is C.c_int and len(args) == len(params)
    for p, a in zip(params, args):                                                       # every ctypes argument is the declared one's
        want = C.c_void_p if "*" in p else (C.c_int64 if p.startswith("int64_t") else C.c_int32)
        assert a is want, (p, a)
    assert _hip.lib().ape_motion_sums.argtypes == args
    make = (REPO / "arm-pose-estimation_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS\s*:=(.*)$", make, flags=re.M).group(1).split()
    hazard = re.search(r"^HAZARD_SRCS\s*:=(.*)$", make, flags=re.M).group(1).split()
    assert "motion.hip" in srcs and "motion.hip" not in hazard
    for name in ("motion_sums", "motion_sums_numpy", "summarise_motion", "merge_motion"):
        assert callable(getattr(score, name))
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    import inspect
    for cls in (Estimator, WatchPhoneUarm, WatchPhonePocketKalman):
        assert "motion_recording" in vars(cls) and "truth_motion" in vars(cls)
    tail = list(inspect.signature(Estimator.sweep_recording).parameters.values())[-2:]
    assert [(p.name, p.default) for p in tail] == [("motion", False), ("times", None)]


# ---------------- 5: the refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_are_made_on_the_host():
    """every refusal include/ape_hip.h states but the capturing stream: APE_ERR_INVALID_ARG before any device call (the pointers are never read)"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    rows_p, times_p, motion_p, acc_p = C.c_void_p(256), C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(16384)

    def call(layout=0, rows=rows_p, kind=_hip.ROWS_MSG, rs=25, rd=_hip.F64, n_sets=1, ss=0, F=10, starts=(0, 3, 7), skip=0, times=None,
             bodies=None, nb=0, motion=motion_p, od=_hip.F64, acc=acc_p, R=None):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        b = None if bodies is None else np.ascontiguousarray(bodies, dtype=np.float64)
        return lib.ape_motion_sums(layout, rows, kind, rs, rd, n_sets, ss, F, C.c_void_p(st.ctypes.data) if len(st) else None,
                                   len(st) if R is None else R, skip, times, None if b is None else C.c_void_p(b.ctypes.data), nb, motion, od,
                                   acc, None)

    one = np.zeros((1, 9))
    bad = [(dict(rows=None), b"NULL"), (dict(starts=()), b"NULL"), (dict(acc=None), b"NULL"),
           (dict(F=0), b"F=0"), (dict(F=-1), b"F=-1"), (dict(R=0), b"recording starts"), (dict(R=-1), b"recording starts"), (dict(R=11), b"recording starts"),
           (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 10)), b"seg_starts[1]"),
           (dict(skip=-1), b"skip"),
           (dict(kind=3), b"rows kind"), (dict(kind=-1), b"rows kind"), (dict(rd=2), b"dtype"), (dict(od=-1), b"dtype"),
           (dict(layout=_hip.LAYOUT_NONE), b"layout"), (dict(layout=3), b"layout"),
           (dict(rs=24), b"rows_stride"), (dict(kind=_hip.ROWS_EST, rs=20), b"rows_stride"), (dict(kind=_hip.ROWS_EST, layout=WATCH, rs=13), b"rows_stride"),
           (dict(kind=_hip.ROWS_TARGETS, layout=POS, rs=19, bodies=one, nb=1), b"rows_stride"),
           (dict(kind=_hip.ROWS_TARGETS, layout=WATCH, rs=11, bodies=one, nb=1), b"rows_stride"),
           (dict(n_sets=0), b"n_sets"), (dict(n_sets=65, ss=250), b"n_sets"), (dict(n_sets=-3), b"n_sets"),
           (dict(n_sets=2, ss=249), b"set_stride"), (dict(n_sets=2, ss=0), b"set_stride"), (dict(n_sets=3, rs=30, ss=299), b"set_stride"),
           (dict(n_sets=2, ss=-(2 ** 40)), b"set_stride"),
           (dict(kind=_hip.ROWS_TARGETS, rs=14), b"bodies_host"), (dict(kind=_hip.ROWS_TARGETS, rs=14, bodies=np.zeros((2, 9)), nb=2), b"n_bodies"),
           (dict(kind=_hip.ROWS_TARGETS, rs=14, bodies=one, nb=0), b"n_bodies"),
           (dict(motion=rows_p), b"aliases"), (dict(acc=rows_p), b"aliases"), (dict(times=times_p, motion=times_p), b"aliases"),
           (dict(times=times_p, acc=times_p), b"aliases"), (dict(motion=acc_p), b"aliases")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)                            # APE_ERR_INVALID_ARG
        assert what in lib.ape_last_error() and b"motion_sums" in lib.ape_last_error(), (kw, lib.ape_last_error())
