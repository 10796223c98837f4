"""Each recording's arm lengths and shoulder origin against the truth without a GPU: the numpy statements
`score.body_sums_numpy` and `score.rebody_rows_numpy` held to hand-written numpy, `score.best_body` on planted cases, the refusals of
`ape_body_sums` and `ape_rebody_rows` that need no device (all are made on the host; the capturing stream is refused in
tests/test_body_fit_gpu.py), the header and the binding.

The planted case: the quaternions of `tests/test_frame_fit_cpu.walk_est`; the truth states them through a planted body per recording
(every one of the nine values 5 - 30 % off the default's, the vectors not parallel to the default's), the messages state the same
quaternions through the default body, 3 frames late.  The body tolerance is 1e-12 = 100 x what a float64 prototype of the formulas
measured (1.9e-14 m at condition numbers up to 612), the convention of tests/test_frame_fit_cpu.py; every case asserts its own
condition number below 1e4, so that the reference alone stays inside the allowance.  The builders are shared with
tests/test_body_fit_gpu.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests.test_frame_fit_cpu import msgs_from_est, qmat, qmul, random_walk_quats, walk_est, yaw_quat

REPO = Path(__file__).resolve().parents[1]
HIPS, WATCH, POS = 0, 1, 2
LAG, LAGS = 3, (-8, 8)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


# ---------------- builders (plain numpy, independent of the statements under test) ---------------------------------------------------------
def default_body():
    from wear_mocap_ape_amd.data_types.bone_map import body9_from_bonemap
    return body9_from_bonemap(None)


def planted_body(k=0):
    """a body whose nine values are 5 - 30 % off the default's (offsets of the zero components: that share of the bone's length)"""
    d = default_body()
    sl, su = (1.10, 0.85)[k % 2], (0.92, 1.25)[k % 2]
    so = np.array([[1.07, 0.9, 1.3], [0.8, 1.12, 0.75]][k % 2])
    return np.r_[d[0] * sl, 0.13 * d[0], -0.08 * d[0], d[3] * su, -0.1 * d[3], 0.21 * d[3], d[6:9] * so]


def est_quats(est, layout):
    """(lower-arm, upper-arm, hips) quaternions of est rows; without hips the identity"""
    if layout == WATCH:
        return est[:, 6:10], est[:, 10:14], np.tile([1.0, 0.0, 0.0, 0.0], (est.shape[0], 1))
    return est[:, 9:13], est[:, 13:17], est[:, 17:21]


def est_through(est, body, layout):
    """est rows with the same quaternions and the positions made through `body` (rotation matrices by qmat)"""
    lq, uq, hq = est_quats(est, layout)
    uo = np.einsum("nab,b->na", qmat(hq), body[6:9])
    elbow = np.einsum("nab,b->na", qmat(uq), body[3:6]) + uo
    hand = np.einsum("nab,b->na", qmat(lq), body[0:3]) + elbow
    if layout == WATCH:
        return np.concatenate([hand, elbow, lq, uq], axis=1)
    return np.concatenate([hand, elbow, uo, lq, uq, hq], axis=1)


def planted_case(n, layout, seed=0, lag=LAG, k=0):
    """(msg [n, 25], truth est rows, planted body): the truth goes through the planted body, the messages through the default one, `lag`
    frames late (the first row again where f - lag leaves the recording)"""
    base = walk_est(n, layout, seed)
    body = planted_body(k)
    truth = est_through(base, body, layout)
    idx = np.clip(np.arange(n) - lag, 0, n - 1)
    return msgs_from_est(base[idx], layout), truth, body


def sums_by_hand(msg, truth, layout, lags, starts=None, skip=0, rec_lags=None, from_truth=False):
    """the 46 sums by loops over the pairs; a quaternion that is zero or not finite, or a non-finite used truth value, leaves a pair out"""
    hips = layout != WATCH
    F = truth.shape[0]
    st = [0] if starts is None else list(starts)
    ends = st[1:] + [F]
    lo, hi = lags
    L = hi - lo + 1
    ql, qu = (9, 13) if hips else (6, 10)
    used = list(range(6)) + list(range(ql, ql + 4)) + list(range(qu, qu + 4)) + (list(range(17, 21)) if hips else [])

    def mats(row, cols):
        out = []
        for c in cols:
            q = row[c:c + 4]
            if not np.isfinite(q).all() or not q.any():
                return None
            out.append(qmat(q / np.linalg.norm(q)))
        return out + ([np.eye(3)] if not hips else [])

    acc = np.zeros((len(st), L, 46))
    for r, (s, e) in enumerate(zip(st, ends)):
        o = 0 if rec_lags is None else rec_lags[r]
        for j in range(L):
            l = o + lo + j
            for f in range(s, e):
                if f - s < skip or f - (o + hi) < s or f - (o + lo) >= e:
                    continue
                t = truth[f - l]
                R = mats(t, (ql, qu) + ((17,) if hips else ())) if from_truth else mats(msg[f], (7, 14) + ((21,) if hips else ()))
                if R is None or not np.isfinite(t[used]).all():
                    acc[r, j, 45] += 1
                    continue
                Rl, Ru, Rh = R
                th, te = t[0:3], t[3:6]
                acc[r, j, :44] += np.r_[(Rl.T @ Ru).ravel(), (Rl.T @ Rh).ravel(), (Ru.T @ Rh).ravel(), Rl.T @ th, Ru.T @ th, Rh.T @ th,
                                        Ru.T @ te, Rh.T @ te, th @ th, te @ te]
                acc[r, j, 44] += 1
    return acc


def check_sums(got, ref, bound, what):
    """columns 0:44 within 16 n 2^-53 max(1, max |t|^2), the two counts exact"""
    assert got.shape == ref.shape, what
    assert np.array_equal(got[..., 44:], ref[..., 44:]), (what, got[..., 44:], ref[..., 44:])
    allow = 16.0 * np.maximum(ref[..., 44:45], 1.0) * 2.0 ** -53 * bound
    d = np.abs(got[..., :44] - ref[..., :44])
    assert (d <= allow).all(), (what, float((d / allow).max()))
    assert not got[ref[..., 44] == 0][..., :44].any(), what
    return float((d / allow).max())


def truth_bound(truth):
    pos = np.concatenate([truth[:, 0:3], truth[:, 3:6]])
    pos = pos[np.isfinite(pos).all(axis=1)]
    return max(1.0, float((pos * pos).sum(axis=1).max(initial=0.0)))


# ---------------- 1: declarations ----------------------------------------------------------------------------------------------------------
def test_header_declares_and_hip_binds_both_entries():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    assert re.search(r"^#define APE_BODY_ACC_WIDTH\s+46\b", text, flags=re.M) and _hip.BODY_ACC_WIDTH == 46 == score.BODY_ACC_WIDTH
    assert re.search(r"^#define APE_BODY_ROT_MSG\s+0\b", text, flags=re.M) and re.search(r"^#define APE_BODY_ROT_TRUTH\s+1\b", text, flags=re.M)
    assert (_hip.BODY_ROT_MSG, _hip.BODY_ROT_TRUTH) == (0, 1)
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    want = {"ape_body_sums": ["int32_t layout", "const void* msg_dev", "int32_t msg_stride", "int32_t msg_dtype", "const void* truth_dev",
                              "int32_t truth_kind", "int32_t truth_dtype", "int32_t F", "const int32_t* seg_starts_host", "int32_t R",
                              "int32_t skip", "int32_t rot_source", "int32_t lag_min", "int32_t lag_max", "const int32_t* rec_lag_host",
                              "double* acc_dev", "void* stream"],
            "ape_rebody_rows": ["int32_t layout", "const void* msg_dev", "int32_t msg_stride", "int32_t msg_dtype", "int32_t F",
                                "const int32_t* seg_starts_host", "int32_t R", "const double* bodies_host", "int32_t n_bodies", "void* out_dev",
                                "int32_t out_dtype", "void* stream"]}
    for name, params in want.items():
        decl = text[text.index(f"\nint {name}(") + 1:]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        got = [" ".join(p.split()) for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
        assert got == params, (name, got)
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name) and len(_hip.SIGNATURES[name][1]) == len(params)
    for name in ("body_sums", "body_sums_numpy", "best_body", "bodies_of", "rebody_rows", "rebody_rows_numpy", "align_body"):
        assert callable(getattr(score, name))
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    assert "fit_bodies" in vars(Estimator) and "fit_bodies" in vars(WatchPhoneUarm) and "fit_bodies" in vars(WatchPhonePocketKalman)


# ---------------- 2: the sums statement against loops -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [HIPS, WATCH])
def test_sums_statement_against_loops(layout):
    from wear_mocap_ape_amd.score import body_sums_numpy
    n, starts, lags, skip, offs = 150, [0, 1, 40, 110], (-2, 3), 2, [0, 2, 1, -1]
    msg, truth, _ = planted_case(n, layout, seed=4)
    msg[:, 7:11] *= 1.7                                     # an unnormalised quaternion is the rotation it stands for
    hq = 17 if layout == HIPS else 10                       # (a truth quaternion either way)
    msg[60, 8], truth[70, 1], truth[80, hq:hq + 4], msg[90, 14:18], truth[95, 4] = np.nan, np.inf, 0.0, 0.0, np.nan
    msg[50, 5] = np.nan                                     # a message position: not read
    if layout == HIPS:
        truth[100, 6] = np.nan                              # the est shoulder origin: not read
    else:
        msg[55, 22] = np.nan                                # the message's hips quaternion: not read without hips
    bound = truth_bound(truth)
    got = body_sums_numpy(msg, truth, layout, lags, starts, skip, offs)
    ref = sums_by_hand(msg, truth, layout, lags, starts, skip, offs)
    assert got.shape == (4, 6, 46) and not got[0].any() and got[1:, :, 44].all()
    print(f"layout {layout}: worst deviation {check_sums(got, ref, bound, layout):.3f} of the allowance")
    assert (got[:, :, 44] + got[:, :, 45] == (got[:, :1, 44] + got[:, :1, 45])).all()
    # recording 2, frames [40, 110): message rows 60 and 90 are lost at every lag; truth rows 70 and 95 (values used) wherever they are
    # paired inside the support; the zero truth quaternion of row 80 loses nothing, the rotations being the message's
    a, b = 40 + max(skip, offs[2] + lags[1]), 110 + min(0, offs[2] + lags[0])
    lost = [2 + sum(a <= row + offs[2] + l < b and row + offs[2] + l not in (60, 90) for row in (70, 95)) for l in range(lags[0], lags[1] + 1)]
    assert got[2, :, 45].tolist() == lost and not got[1, :, 45].any() and not got[3, :, 45].any()
    if layout == WATCH:                                     # R_h = I: the block of R_l'R_h is the sum of R_l'
        lone = body_sums_numpy(msg[:1], truth[:1], WATCH, (0, 0))
        assert np.abs(lone[0, 0, 9:18].reshape(3, 3) - qmat(msg[0, 7:11] / np.linalg.norm(msg[0, 7:11])).T).max() <= 1e-15
        assert np.abs(lone[0, 0, 33:36] - truth[0, 0:3]).max() == 0.0
    # rotations from the truth: the single lag 0, the message is not read
    got_t = body_sums_numpy(None, truth, layout, (0, 0), starts, skip, rotations="truth")
    ref_t = sums_by_hand(None, truth, layout, (0, 0), starts, skip, from_truth=True)
    check_sums(got_t, ref_t, bound, (layout, "truth"))
    assert got_t[2, 0, 45] == 3 and ref_t[2, 0, 44] == 70 - skip - 3       # rows 70, 80 (its zero quaternion) and 95
    for bad in (lambda: body_sums_numpy(None, truth, layout, (0, 1), rotations="truth"),
                lambda: body_sums_numpy(None, truth, layout, (0, 0), starts, rec_lags=[0, 0, 0, 0], rotations="truth"),
                lambda: body_sums_numpy(msg, truth, layout, (0, 0), rotations="mocap")):
        with pytest.raises(UserWarning):
            bad()


# ---------------- 3: planted bodies -----------------------------------------------------------------------------------------------------------
def direct_rms(msg, truth, lag, support):
    a, b = support
    dh = msg[a:b, 4:7] - truth[a - lag:b - lag, 0:3]
    de = msg[a:b, 11:14] - truth[a - lag:b - lag, 3:6]
    return float(np.sqrt((dh * dh).sum(axis=1).mean())), float(np.sqrt((de * de).sum(axis=1).mean()))


@pytest.mark.parametrize("weights", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("layout", [HIPS, WATCH])
@pytest.mark.parametrize("n", [1000, 200, 40])
def test_planted_body_and_lag_are_found(n, layout, weights):
    from wear_mocap_ape_amd.score import best_body, body_sums_numpy, bodies_of
    msg, truth, body = planted_case(n, layout, seed=n, k=(n // 200) % 2)
    acc = body_sums_numpy(msg, truth, layout, LAGS)
    assert acc.shape == (1, 17, 46) and (acc[0, :, 44] == n - 16).all() and not acc[0, :, 45].any()
    b = best_body(acc, LAGS, "vectors", weights)[0]
    want = body.copy()
    if weights[0] == 0:
        want[0:3] = default_body()[0:3]                     # the forearm is not observable from the elbow: the prior's
    worst = np.abs(b["body"] - want).max()
    print(f"n {n} layout {layout} weights {weights}: lag {b['lag']}, cond {b['cond']:.1f}, max |body - plant| {worst:.3e}, "
          f"rms after hand {b['hand_rms_after']:.2e} elbow {b['elbow_rms_after']:.2e}")
    assert b["ok"] and b["cond"] < 1e4 and b["lag"] == LAG and b["pairs"] == n - 16 and b["residual"].shape == (17,)
    assert worst <= 1e-12
    assert int(np.nanargmin(b["residual"])) == LAG - LAGS[0]
    assert b["elbow_rms_after"] <= 1e-6 and (weights[0] == 0 or b["hand_rms_after"] <= 1e-6)
    hand0, elbow0 = direct_rms(msg, truth, LAG, (8, n - 8))
    assert abs(b["hand_rms_before"] - hand0) <= 1e-9 and abs(b["elbow_rms_before"] - elbow0) <= 1e-9 and hand0 > 0.01
    assert abs(b["larm_length"] - np.linalg.norm(want[0:3])) <= 1e-12 and abs(b["uarm_length"] - np.linalg.norm(want[3:6])) <= 1e-12
    assert np.array_equal(bodies_of([b, b]), np.stack([b["body"], b["body"]]))


@pytest.mark.parametrize("layout", [HIPS, WATCH])
def test_lengths_mode_recovers_planted_scales(layout):
    from wear_mocap_ape_amd.score import best_body, body_sums_numpy
    n, scales = 200, np.array([1.1, 0.8, 1.25])
    base = walk_est(n, layout, seed=7)
    prior = planted_body(1)                                 # any prior: the truth's body is its three vectors scaled
    truth = est_through(base, np.r_[prior[0:3] * scales[0], prior[3:6] * scales[1], prior[6:9] * scales[2]], layout)
    idx = np.clip(np.arange(n) - LAG, 0, n - 1)
    acc = body_sums_numpy(msgs_from_est(base[idx], layout), truth, layout, LAGS)
    for weights, free in (((1, 1), [0, 1, 2]), ((1, 0), [0, 1, 2]), ((0, 1), [1, 2])):
        b = best_body(acc, LAGS, "lengths", weights, prior=prior)[0]
        got = np.array([b["body"][3 * k:3 * k + 3] @ prior[3 * k:3 * k + 3] / (prior[3 * k:3 * k + 3] @ prior[3 * k:3 * k + 3]) for k in range(3)])
        want = np.where(np.isin(np.arange(3), free), scales, 1.0)
        print(f"layout {layout} weights {weights}: scales {got}, cond {b['cond']:.2f}")
        assert b["ok"] and b["lag"] == LAG and b["cond"] < 1e4 and np.abs(got - want).max() <= 1e-12
        assert np.abs(b["body"] - np.repeat(want, 3) * prior).max() <= 1e-12


# ---------------- 4: identifiability ------------------------------------------------------------------------------------------------------------
def test_an_upper_arm_rigid_against_the_hips_is_refused_in_vectors_mode_and_solved_in_lengths_mode():
    from wear_mocap_ape_amd.score import best_body, body_sums_numpy
    n, scales = 300, np.array([0.9, 1.2, 1.15])
    rng = np.random.default_rng(3)
    lq, hq = random_walk_quats(rng, n), yaw_quat(np.cumsum(0.03 * rng.normal(size=n)))
    c = np.array([0.8, 0.3, -0.4, 0.2])
    uq = qmul(hq, c / np.linalg.norm(c))                    # q_uarm = q_hips (x) c
    base = np.concatenate([np.zeros((n, 9)), lq, uq, hq], axis=1)
    prior = default_body()
    truth = est_through(base, np.repeat(scales, 3) * prior, HIPS)
    msg = msgs_from_est(est_through(base, prior, HIPS), HIPS)
    acc = body_sums_numpy(msg, truth, HIPS, (0, 0))
    b = best_body(acc, (0, 0), "vectors")[0]
    print(f"vectors: cond {b['cond']:.3e}")
    assert b["cond"] >= 1e12 and not b["ok"] and np.array_equal(b["body"], prior) and b["lag"] == 0 and b["pairs"] == n
    assert b["hand_rms_after"] == b["hand_rms_before"] > 0.01 and np.isnan(b["residual"]).all()
    s = best_body(acc, (0, 0), "lengths")[0]
    print(f"lengths: cond {s['cond']:.3f}, max |body - plant| {np.abs(s['body'] - np.repeat(scales, 3) * prior).max():.3e}")
    assert s["ok"] and s["cond"] < 1e4 and np.abs(s["body"] - np.repeat(scales, 3) * prior).max() <= 1e-12
    assert s["hand_rms_after"] <= 1e-6 and s["elbow_rms_after"] <= 1e-6


def test_too_few_pairs_an_empty_support_and_the_ridge():
    from wear_mocap_ape_amd.score import best_body, body_sums_numpy, bodies_of
    msg, truth, body = planted_case(200, HIPS, seed=9, lag=0)
    starts = [0, 5, 6]                                      # five frames, one frame, the rest
    acc = body_sums_numpy(msg, truth, HIPS, (-1, 1), starts)
    assert acc[:, 1, 44].tolist() == [3, 0, 192]
    f = best_body(acc, (-1, 1))
    assert not f[0]["ok"] and f[0]["pairs"] == 3 and f[0]["lag"] in (-1, 0, 1) and np.array_equal(f[0]["body"], default_body())
    assert f[0]["hand_rms_before"] > 0.01 and f[0]["hand_rms_after"] == f[0]["hand_rms_before"]
    assert not f[1]["ok"] and f[1]["lag"] is None and f[1]["pairs"] == 0 and np.array_equal(f[1]["body"], default_body())
    assert np.isnan(f[1]["hand_rms_before"]) and np.isnan(f[1]["residual"]).all()
    assert f[2]["ok"] and f[2]["lag"] == 0 and np.abs(f[2]["body"] - body).max() <= 1e-12
    assert bodies_of(f).shape == (3, 9) and bodies_of(f).dtype == np.float64 and np.array_equal(bodies_of(f)[1], default_body())
    # three frames carry three scales: the lengths form has enough pairs
    assert best_body(acc, (-1, 1), "lengths")[0]["pairs"] == 3
    # one prior per recording; the ridge pulls towards it, monotonically
    priors = np.stack([default_body(), planted_body(1), default_body()])
    assert np.array_equal(best_body(acc, (-1, 1), prior=priors)[1]["body"], priors[1])
    dist = [np.linalg.norm(best_body(acc, (-1, 1), ridge=rho)[2]["body"] - default_body()) for rho in (0.0, 0.01, 0.1, 1.0, 10.0, 1000.0)]
    print("distance to the prior over the ridge:", dist)
    assert all(a > b for a, b in zip(dist, dist[1:])) and dist[-1] < 0.05 * dist[0]
    for bad in (lambda: best_body(acc, (-1, 2)), lambda: best_body(acc, (-1, 1), "scales"), lambda: best_body(acc[:, :, :45], (-1, 1)),
                lambda: best_body(acc, (-1, 1), weights=(0, 0)), lambda: best_body(acc, (-1, 1), weights=(1, 1, 1)),
                lambda: best_body(acc, (-1, 1), ridge=-1.0), lambda: best_body(acc, (-1, 1), prior=np.zeros((2, 9))),
                lambda: best_body(acc, (-1, 1), rec_lags=[0, 1])):
        with pytest.raises(UserWarning):
            bad()


def test_ties_go_to_the_smaller_lag_magnitude():
    from wear_mocap_ape_amd.score import best_body, body_sums_numpy
    msg, truth, _ = planted_case(60, HIPS, seed=2, lag=0)
    one = body_sums_numpy(msg, truth, HIPS, (0, 0))
    acc = np.repeat(one, 5, axis=1)                         # the same record at every lag: every residual ties
    assert best_body(acc, (-2, 2))[0]["lag"] == 0
    assert best_body(acc, (1, 5))[0]["lag"] == 1
    assert best_body(acc, (0, 4), rec_lags=[-3])[0]["lag"] == 0
    assert best_body(acc[:, :4], (0, 3), rec_lags=[-3])[0]["lag"] == 0
    assert best_body(acc[:, :2], (0, 1), rec_lags=[-1])[0]["lag"] == 0
    assert best_body(np.repeat(one, 3, axis=1), (-1, 1), rec_lags=[0])[0]["lag"] == 0
    two = np.repeat(one, 2, axis=1)
    assert best_body(two, (0, 1), rec_lags=[-2])[0]["lag"] == -1 and best_body(two, (-1, 0), rec_lags=[2])[0]["lag"] == 1
    sym = np.repeat(one, 3, axis=1)
    sym[0, 1] *= np.nan                                     # lag 0 unusable: |-1| == |1|, the smaller lag
    sym[0, 1, 44:46] = 0.0
    assert best_body(sym, (-1, 1))[0]["lag"] == -1


# ---------------- 5: the rows statement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [HIPS, WATCH])
def test_rebody_rows_statement(layout):
    from wear_mocap_ape_amd.score import rebody_rows_numpy
    n, starts = 200, [0, 50, 51]
    base = walk_est(n, layout, seed=5)
    msg = msgs_from_est(base, layout)
    msg[:, 0:4] = random_walk_quats(np.random.default_rng(1), n)
    same = rebody_rows_numpy(msg, default_body(), layout)
    assert same.shape == (n, 25) and np.abs(same - msg).max() <= 1e-15
    bodies = np.stack([planted_body(0), planted_body(1), default_body()])
    which = np.searchsorted(starts, np.arange(n), side="right") - 1
    want = msg.copy()
    for r in range(3):
        rows = msgs_from_est(est_through(base, bodies[r], layout), layout)
        if layout == WATCH:
            rows[:, 18:21] = bodies[r, 6:9]                 # (msgs_from_est writes the default origin for this layout)
        want[which == r, 4:25] = rows[which == r, 4:25]
    got = rebody_rows_numpy(msg, bodies, layout, starts)
    assert np.abs(got - want).max() <= 1e-15 and np.array_equal(got[:, [0, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 17, 21, 22, 23, 24]],
                                                                msg[:, [0, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 17, 21, 22, 23, 24]])
    assert np.array_equal(rebody_rows_numpy(msg, bodies[1], layout, starts), rebody_rows_numpy(msg, bodies[1], layout))
    # a NaN in one quaternion reaches only the positions behind it; a NaN position of the input is made again
    bad = msg.copy()
    bad[7, 8], bad[9, 15], bad[11, 22], bad[13, 5], bad[15, 2] = np.nan, np.nan, np.nan, np.nan, np.nan
    out = rebody_rows_numpy(bad, bodies, layout, starts)
    assert np.isnan(out[7, 4:7]).all() and np.isfinite(out[7, 11:14]).all() and np.isfinite(out[7, 18:21]).all()
    assert np.isnan(out[9, 4:7]).all() and np.isnan(out[9, 11:14]).all() and np.isfinite(out[9, 18:21]).all()
    assert np.isnan(out[11, 4:7]).all() == (layout == HIPS) and np.isnan(out[11, 18:21]).all() == (layout == HIPS) and np.isnan(out[11, 22])
    assert np.array_equal(out[13], got[13]) and np.isnan(out[15, 2]) and np.array_equal(out[15, 4:], got[15, 4:])
    rest = np.delete(np.arange(n), [7, 9, 11, 13, 15])
    assert np.array_equal(out[rest], got[rest])
    for args in ((msg, np.zeros((2, 9)), layout, starts), (msg, np.zeros(8), layout), (msg, default_body(), POS)):
        with pytest.raises(UserWarning):
            rebody_rows_numpy(*args)


# ---------------- 6: the C ABI -------------------------------------------------------------------------------------------------------------------
def test_body_sums_refusals_are_made_on_the_host():
    """every refusal include/ape_hip.h states but the capturing stream: APE_ERR_INVALID_ARG before any device call (the pointers are never read)"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)

    def call(layout=0, msg=dummy, ms=25, md=_hip.F64, truth=dummy, kind=_hip.TRUTH_EST, td=_hip.F64, F=10, starts=(0, 3, 7), skip=0, rot=0,
             lo=-2, hi=2, offs=None, acc=dummy, R=None):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        of = None if offs is None else np.ascontiguousarray(offs, dtype=np.int32)
        return lib.ape_body_sums(layout, msg, ms, md, truth, kind, td, F, C.c_void_p(st.ctypes.data) if len(st) else None,
                                 len(st) if R is None else R, skip, rot, lo, hi, None if of is None else C.c_void_p(of.ctypes.data), acc, None)

    big = 2 ** 31 - 1
    bad = [(dict(msg=None), b"NULL"), (dict(truth=None), b"NULL"), (dict(acc=None), b"NULL"), (dict(truth=None, rot=1, lo=0, hi=0), b"NULL"),
           (dict(F=0), b"F=0"), (dict(starts=()), b"NULL"), (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"),
           (dict(starts=(0, 10)), b"seg_starts[1]"), (dict(ms=24), b"msg_stride"), (dict(skip=-1), b"skip"),
           (dict(layout=_hip.LAYOUT_NONE), b"layout"), (dict(layout=3), b"layout"), (dict(kind=2), b"truth kind"),
           (dict(md=2), b"dtype"), (dict(td=-1), b"dtype"), (dict(rot=2), b"rotation source"), (dict(rot=-1), b"rotation source"),
           (dict(kind=_hip.TRUTH_TARGETS, layout=0), b"body being fitted"), (dict(kind=_hip.TRUTH_TARGETS, layout=1), b"body being fitted"),
           (dict(rot=1), b"single lag 0"), (dict(rot=1, lo=0, hi=1), b"single lag 0"), (dict(rot=1, lo=1, hi=1), b"single lag 0"),
           (dict(rot=1, lo=0, hi=0, offs=(0, 0, 0)), b"rec_lag_host"),
           (dict(R=0), b"recording starts"), (dict(R=-1), b"recording starts"), (dict(R=11), b"recording starts"),
           (dict(lo=1, hi=0), b"lag_min"), (dict(lo=big, hi=-big), b"lag_min"), (dict(lo=0, hi=65), b"66 lags"), (dict(lo=-big, hi=big), b"lags in the sweep"),
           (dict(lo=129, hi=129), b"|lag|"), (dict(lo=-129, hi=-128), b"|lag|"), (dict(lo=100, hi=129), b"|lag|"),
           (dict(offs=(0, 127, 0)), b"recording 1"), (dict(offs=(0, 0, -127)), b"recording 2"), (dict(offs=(big, 0, 0)), b"recording 0"),
           (dict(offs=(0, -big - 1, 0)), b"recording 1"), (dict(lo=0, hi=0, offs=(0, 0, 129)), b"recording 2")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)                            # APE_ERR_INVALID_ARG
        assert what in lib.ape_last_error() and b"body_sums" in lib.ape_last_error(), (kw, lib.ape_last_error())


def test_rebody_rows_refusals_are_made_on_the_host():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy, other = C.c_void_p(256), C.c_void_p(4096)

    def call(layout=0, msg=dummy, ms=25, md=_hip.F64, F=10, starts=(0, 3, 7), bodies=np.zeros((1, 9)), nb=None, out=other, od=_hip.F64, R=None):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        b = None if bodies is None else np.ascontiguousarray(bodies, dtype=np.float64)
        return lib.ape_rebody_rows(layout, msg, ms, md, F, C.c_void_p(st.ctypes.data) if len(st) else None, len(st) if R is None else R,
                                   None if b is None else C.c_void_p(b.ctypes.data), (0 if b is None else len(b)) if nb is None else nb, out, od,
                                   None)

    bad = [(dict(msg=None), b"NULL"), (dict(out=None), b"NULL"), (dict(bodies=None, nb=1), b"NULL"), (dict(starts=()), b"NULL"),
           (dict(F=0), b"F=0"), (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 10)), b"seg_starts[1]"),
           (dict(R=0), b"recording starts"), (dict(R=11), b"recording starts"), (dict(ms=24), b"msg_stride"),
           (dict(layout=_hip.LAYOUT_NONE), b"layout"), (dict(layout=3), b"layout"), (dict(layout=POS), b"predicted"),
           (dict(md=2), b"dtype"), (dict(od=-1), b"dtype"),
           (dict(bodies=np.zeros((2, 9))), b"n_bodies"), (dict(nb=0), b"n_bodies"), (dict(bodies=np.zeros((4, 9))), b"n_bodies"),
           (dict(out=dummy), b"aliases")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)                            # APE_ERR_INVALID_ARG
        assert what in lib.ape_last_error() and b"rebody_rows" in lib.ape_last_error(), (kw, lib.ape_last_error())
