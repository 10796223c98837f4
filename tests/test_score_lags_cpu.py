"""Scoring over a sweep of time lags without a GPU: the numpy statement `score.score_lags_numpy` against a plain loop
over recordings, lags and gathered rows; the support arithmetic; `best_lag` on constructed accumulators; `merge` on `[R, L, 25]`; the
refusals of `ape_score_lags` (all made on the host); the header and the binding.  The base case of the feature -- smooth trajectories
with a planted lag per recording -- is built here and shared with tests/test_score_lags_gpu.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
HIPS, WATCH, POS = 0, 1, 2
FPS = 50.0

# the base case: a 3-frame recording (empty support), a boundary on a 256-frame tile edge, three boundaries inside a wave
F, STARTS, SKIP, LAGS = 700, [0, 3, 70, 256, 300, 650], 5, (-5, 9)
PLANTED = [0, 3, 0, -2, 3, -2]                             # the estimate of recording r is late by PLANTED[r] frames
SUPPORTS = [0, 53, 172, 30, 336, 36]                       # length - max(skip, 9) - 5


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def trajectory(n, layout=HIPS, seed=0):
    """est rows of the layout at the (possibly fractional) frame indices `n`, 50 Hz: positions are sums of two sines at 0.4-1.3 Hz,
    quaternions normalised sums of sines (about a constant, so the norm stays away from 0)"""
    rng = np.random.default_rng(seed)
    t = np.asarray(n, dtype=np.float64)[:, None] / FPS

    def sines(k, amp):
        hz, ph, a = rng.uniform(0.4, 1.3, size=(2, k)), rng.uniform(0.0, 2 * np.pi, size=(2, k)), amp * rng.uniform(0.5, 1.0, size=(2, k))
        return a[0] * np.sin(2 * np.pi * hz[0] * t + ph[0]) + a[1] * np.sin(2 * np.pi * hz[1] * t + ph[1])

    est = np.zeros((t.shape[0], 14 if layout == WATCH else 21))
    est[:, 0:3], est[:, 3:6] = sines(3, 0.3), sines(3, 0.2)
    for c in ((6, 10) if layout == WATCH else (9, 13, 17)):
        q = sines(4, 0.6) + np.array([1.5, 0.2, -0.3, 0.1])
        est[:, c:c + 4] = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    if layout != WATCH:
        est[:, 6:9] = [-0.2, 0.4, 0.01]
    return est


def msgs_from_est(est, layout):
    """one message per est row stating that row's pose (compose_msg.py:72-78 columns)"""
    qc = (6, 10) if layout == WATCH else (9, 13, 17)
    m = np.zeros((est.shape[0], 25))
    m[:, 21] = 1.0
    m[:, 4:7], m[:, 11:14] = est[:, 0:3], est[:, 3:6]
    for k, c in enumerate(qc):
        m[:, 7 + 7 * k:11 + 7 * k] = est[:, c:c + 4]
    m[:, 0:4] = m[:, 7:11]
    return m


def spread_for(msg, seed=3):
    """spread records near the message's origins with well-conditioned covariances D + u u' (condition number < 10)"""
    rng = np.random.default_rng(seed)
    n = msg.shape[0]
    rec = np.zeros((n, 21))
    for o, c in ((0, 4), (9, 11)):
        rec[:, o:o + 3] = msg[:, c:c + 3] + 0.02 * rng.normal(size=(n, 3))
        d, u = 0.01 * rng.uniform(0.5, 2.0, size=(n, 3)), 0.05 * rng.normal(size=(n, 3))
        S = u[:, :, None] * u[:, None, :]
        S[:, [0, 1, 2], [0, 1, 2]] += d
        rec[:, o + 3:o + 9] = S[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    rec[:, 18:21] = 0.01
    return rec


def planted_case(layout=HIPS, planted=PLANTED, starts=STARTS, n=F, seed=0):
    """(msg [n, 25], truth est rows [n, W], spread [n, 21]): msg[f] = truth(f - planted[r]) in recording r, exactly"""
    idx = np.arange(n)
    rec = np.searchsorted(np.asarray(starts), idx, side="right") - 1
    truth = trajectory(idx, layout, seed)
    msg = msgs_from_est(trajectory(idx - np.asarray(planted, dtype=np.float64)[rec], layout, seed), layout)
    return msg, truth, spread_for(msg)


def plain_loop(msg, truth, layout, lags, starts, skip, spread, rec_lags=None):
    """the statement of the feature, frame by frame: gathered pair rows through score_rows_numpy, the support through accumulate_numpy"""
    from wear_mocap_ape_amd.score import accumulate_numpy, score_rows_numpy
    n, L = msg.shape[0], lags[1] - lags[0] + 1
    ends = list(starts[1:]) + [n]
    score, acc = np.full((n, L, 7), np.nan), np.zeros((len(starts), L, 25))
    for r, (s, e) in enumerate(zip(starts, ends)):
        o = 0 if rec_lags is None else rec_lags[r]
        sup = np.array([f for f in range(s, e) if f - s >= skip and f - (o + lags[1]) >= s and f - (o + lags[0]) < e], dtype=np.int64)
        for j in range(L):
            l = o + lags[0] + j
            fs = np.array([f for f in range(s, e) if s <= f - l < e], dtype=np.int64)
            if fs.size:
                score[fs, j] = score_rows_numpy(msg[fs], truth[fs - l], layout, None if spread is None else spread[fs])
            if sup.size:
                acc[r, j] = accumulate_numpy(score[sup, j])[0]
    return score, acc


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---------------- the numpy statement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [HIPS, WATCH, POS])
def test_numpy_statement_equals_the_plain_loop(layout):
    from wear_mocap_ape_amd.score import score_lags_numpy
    msg, truth, rec = planted_case(layout)
    truth[[10, 100, 101, 400], 1] = np.nan
    msg[[50, 333], 9] = np.nan
    for spread, rec_lags, lags, skip in ((rec, None, LAGS, SKIP), (None, [0, 2, -3, 7, 0, 1], (-2, 2), 0), (rec, None, (0, 0), 5)):
        s, a = score_lags_numpy(msg, truth, layout, lags, STARTS, skip, spread, rec_lags)
        s_ref, a_ref = plain_loop(msg, truth, layout, lags, STARTS, skip, spread, rec_lags)
        assert s.shape == s_ref.shape and a.shape == a_ref.shape
        assert same(s, s_ref) and np.array_equal(a, a_ref), (layout, lags)
    # the sweep {0}: score_rows_numpy and accumulate_numpy themselves
    from wear_mocap_ape_amd.score import accumulate_numpy, score_rows_numpy
    s0, a0 = score_lags_numpy(msg, truth, layout, (0, 0), STARTS, SKIP, rec)
    rows = score_rows_numpy(msg, truth, layout, rec)
    assert same(s0[:, 0], rows) and np.array_equal(a0[:, 0], accumulate_numpy(rows, STARTS, SKIP))


def test_support_is_common_to_all_lags():
    from wear_mocap_ape_amd.score import score_lags_numpy
    msg, truth, rec = planted_case()
    gaps_t, gaps_m = [20, 90, 91, 280, 500], [40, 130, 600]
    truth[gaps_t, 0] = np.nan
    msg[gaps_m, 5] = np.nan
    s, a = score_lags_numpy(msg, truth, HIPS, LAGS, STARTS, SKIP, rec)
    total = a[:, :, 15] + a[:, :, 16]
    assert np.array_equal(total, np.repeat(np.array(SUPPORTS, dtype=np.float64)[:, None], 15, axis=1))
    assert not a[0].any()                                               # the 3-frame recording
    # a truth gap meets a different frame at every lag: truth row 90 is paired with frame 90 + l, inside the support of [70, 256)
    # (frames 79 .. 250) for every l of the sweep, so each lag loses rows 90 and 91
    assert (a[2, :, 16] == 3).all() and (a[2, :, 15] == 172 - 3).all()       # ... and the message gap at frame 130
    for j, l in enumerate(range(LAGS[0], LAGS[1] + 1)):
        assert np.isnan(s[90 + l, j]).all() and np.isnan(s[130, j]).all() and np.isfinite(s[89 + l, j, :5]).all()
    # truth row 20 is inside the support of [3, 70) (frames 12 .. 64) only for l >= -8 and l <= 44: every lag; row 280 in [256, 300):
    # support 265 .. 294, frame 280 + l: every lag
    assert (a[1, :, 16] == 2).all() and (a[3, :, 16] == 1).all()
    # pairs never cross a boundary: at lag 3 the first three frames of a recording have no pair, at lag -2 the last two
    for st, en in zip(STARTS, STARTS[1:] + [F]):
        assert np.isnan(s[st:min(st + 3, en), 8]).all() and np.isnan(s[max(en - 2, st):en, 3]).all()
    # recordings shorter than the span (or than skip) give an empty support
    _, short = score_lags_numpy(msg[:40], truth[:40], HIPS, (-5, 9), [0, 14, 28], 0, None)
    assert short.shape == (3, 15, 25) and not short.any()               # 14, 14 and 12 frames for a span of 14
    _, one = score_lags_numpy(msg[:40], truth[:40], HIPS, (-5, 9), [0, 14, 25], 0, None)
    assert (one[2, :, 15] == 1).all() and not one[:2].any()             # 15 frames: exactly one
    _, skipped = score_lags_numpy(msg[:40], truth[:40], HIPS, (-1, 1), [0], 39, None)
    assert not skipped.any()                                            # frame 39 is past the skip but has no pair at lag -1


@pytest.mark.parametrize("k", [3, 0, -2])
def test_base_case_finds_the_planted_lag(k):
    """msg[f] = truth(f - k) for every recording, and the per-recording plant the device test uses"""
    from wear_mocap_ape_amd.score import best_lag, score_lags_numpy
    for planted in ([k] * 6, PLANTED):
        msg, truth, rec = planted_case(planted=planted)
        _, a = score_lags_numpy(msg, truth, HIPS, LAGS, STARTS, SKIP, rec)
        best = best_lag(a, LAGS)
        assert best[0]["lag"] is None and best[0]["at_edge"] is None and best[0]["scored"] == 0 and np.isnan(best[0]["rms"])
        for r in range(1, 6):
            b = best[r]
            assert b["lag"] == planted[r] and b["rms"] == 0.0 and b["scored"] == SUPPORTS[r] and not b["at_edge"], (r, b)
            assert (b["rms_lag0"] == 0.0) == (planted[r] == 0) and (planted[r] == 0 or b["rms_lag0"] > 1e-3)
        for name in ("elbow_pos", "larm_rot", "uarm_rot", "hips_rot"):
            assert [b["lag"] for b in best_lag(a, LAGS, name)[1:]] == list(planted[1:])


def test_half_frame_plant_is_refined():
    from wear_mocap_ape_amd.score import best_lag, score_lags_numpy
    idx = np.arange(F)
    truth = trajectory(idx)
    msg = msgs_from_est(trajectory(idx - 3.4), HIPS)
    _, a = score_lags_numpy(msg, truth, HIPS, LAGS, STARTS, SKIP)
    best = best_lag(a, LAGS)
    print("refined:", [round(b["refined"], 4) for b in best[1:]])
    for b in best[1:]:
        assert b["lag"] == 3 and abs(b["refined"] - 3.4) <= 0.01, b
        assert b["rms"] < b["rms_lag0"]


# ---------------- best_lag on constructed accumulators --------------------------------------------------------------------------------------
def _acc_from_ms(ms, n=10.0):
    """[R, L, 25] accumulators whose hand mean squares are `ms` over n scored frames"""
    ms = np.asarray(ms, dtype=np.float64)
    a = np.zeros(ms.shape + (25,))
    a[..., 15] = np.where(np.isfinite(ms), n, 0.0)
    a[..., 1] = np.where(np.isfinite(ms), ms * n, 0.0)
    return a


def test_best_lag_ties_edges_clamping_and_offsets():
    from wear_mocap_ape_amd.score import best_lag
    nan = float("nan")
    ms = [[4.0, 1.0, 2.0, 1.0, 4.0],                       # lags -2 .. 2: a tie between -1 and 1 -> the smaller l
          [1.0, 2.0, 3.0, 1.0, 1.0],                       # a tie between -2, 1 and 2 -> the smaller |l|
          [0.5, 1.0, 2.0, 3.0, 4.0],                       # the minimum at the first lag of the sweep
          [4.0, 3.0, 2.0, 1.0, 0.5],                       # ... at the last
          [9.0, 4.0, 1.0, 0.0, 1.0],                       # a symmetric parabola about lag 1
          [9.0, 1.0, 1.0, 9.0, 16.0],                      # a tie with the left neighbour: lag 0, the vertex on the clamp l - 0.5
          [5.0, 2.0, 2.0, 2.0, 5.0],                       # flat: second difference 0, lag 0 by the tie rule, refined = lag
          [nan] * 5,                                       # an empty support
          [nan, 3.0, 1.0, nan, nan]]                       # a neighbour without scored frames
    a = _acc_from_ms(ms)
    b = best_lag(a, (-2, 2))
    assert [x["lag"] for x in b] == [-1, 1, -2, 2, 1, 0, 0, None, 0]
    assert [x["at_edge"] for x in b] == [False, False, True, True, False, False, False, None, False]
    assert b[2]["refined"] == -2.0 and b[3]["refined"] == 2.0
    assert b[4]["refined"] == 1.0 and b[4]["rms"] == 0.0 and b[4]["rms_lag0"] == 1.0
    assert b[0]["refined"] == -0.75 and b[1]["refined"] == 1.5          # -1 + (4 - 2) / (2 * 4);  1 + (3 - 1) / (2 * 2), on the clamp
    assert b[5]["refined"] == -0.5
    assert b[6]["refined"] == 0.0 and b[8]["refined"] == 0.0
    assert b[7] == {"lag": None, "refined": b[7]["refined"], "at_edge": None, "scored": 0, "rms": b[7]["rms"], "rms_lag0": b[7]["rms_lag0"]}
    assert all(np.isnan(b[7][k]) for k in ("refined", "rms", "rms_lag0"))
    assert all(x["scored"] == 10 for i, x in enumerate(b) if i != 7)
    # rec_lags shift the answer: index j of recording r stands for rec_lags[r] + lo + j
    off = [0, 3, -4, 10, 0, 0, 0, 0, 0]
    c = best_lag(a, (-2, 2), rec_lags=off)
    assert [x["lag"] for x in c][:4] == [-1, 3 - 2, -4 - 2, 12]          # row 1: |l| of lags 1, 4, 5 -> 1
    assert np.isnan(c[1]["rms_lag0"]) and np.isnan(c[3]["rms_lag0"]) and c[0]["rms_lag0"] == np.sqrt(2.0)
    assert c[3]["refined"] == 12.0 and c[3]["at_edge"]
    # another error column, torch-free input checks
    a2 = np.zeros((1, 3, 25))
    a2[0, :, 15], a2[0, :, 7] = 4.0, [8.0, 4.0, 16.0]
    d = best_lag(a2, (5, 7), "larm_rot")
    assert d[0]["lag"] == 6 and d[0]["rms"] == 1.0 and np.isnan(d[0]["rms_lag0"])
    for bad in (lambda: best_lag(a, (-2, 3)), lambda: best_lag(a, (-2, 2), "hand"), lambda: best_lag(a[:, 0], (0, 0)),
                lambda: best_lag(a, (-2, 2), rec_lags=[0, 1])):
        with pytest.raises(UserWarning):
            bad()


def test_merge_takes_sweeps():
    """a recording cut in two: the merged sweep is the sum over the two pieces' supports -- the whole support less the frames whose
    pairs straddle the cut"""
    from wear_mocap_ape_amd import score
    msg, truth, rec = planted_case(planted=[1] * 6)
    msg[:, 4:7] += 0.01 * np.random.default_rng(5).normal(size=(F, 3))
    lags, cut = (-2, 3), 400
    _, whole = score.score_lags_numpy(msg, truth, HIPS, lags, [0], 5, rec)
    _, a = score.score_lags_numpy(msg[:cut], truth[:cut], HIPS, lags, [0], 5, rec[:cut])
    _, b = score.score_lags_numpy(msg[cut:], truth[cut:], HIPS, lags, [0], 0, rec[cut:])
    m = score.merge(a, b)
    assert m.shape == (1, 6, 25)
    assert (whole[0, :, 15] == F - 5 - 2).all() and (m[0, :, 15] == F - 5 - 2 - 5).all()      # frames cut-2 .. cut+2 are in neither piece
    s, _ = score.score_lags_numpy(msg, truth, HIPS, lags, [0], 5, rec)
    keep = np.r_[5:cut - 2, cut + 3:F - 2]
    for j in range(6):
        ref = score.accumulate_numpy(s[keep, j])[0]
        counts, maxima = [15, 16, 17, 19, 20, 21, 23, 24], [2, 5, 8, 11, 14]
        assert np.array_equal(m[0, j, counts], ref[counts]) and np.array_equal(m[0, j, maxima], ref[maxima])
        sums = [c for c in range(25) if c not in counts + maxima]
        top = max(1.0, float(np.nanmax(s[keep, j])) ** 2)               # the largest term of any sum
        assert (np.abs(m[0, j, sums] - ref[sums]) <= 16 * keep.size * 2.0 ** -53 * top).all()
    assert score.summarise(m[:, 3])[0]["scored"] == F - 12 and score.best_lag(m, lags)[0]["lag"] == 1
    with pytest.raises(UserWarning):
        score.merge(a, b[:, :5])
    with pytest.raises(UserWarning):
        score.merge(a, b[:, 0])
    with pytest.raises(UserWarning):
        score.summarise(m)                                  # summarise keeps taking [R, 25]


# ---------------- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_refusals_are_made_on_the_host():
    """every refusal include/ape_hip.h states: APE_ERR_INVALID_ARG before any device call (the pointers are never read)"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)
    body = np.zeros((3, 9))

    def call(layout=0, msg=dummy, ms=25, spread=dummy, ss=21, md=_hip.F64, truth=dummy, kind=0, td=_hip.F64, F=10, starts=(0, 3, 7),
             skip=0, bodies=body, nb=1, lo=-2, hi=2, offs=None, score=dummy, sd=_hip.F64, acc=dummy, R=None):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        of = None if offs is None else np.ascontiguousarray(offs, dtype=np.int32)
        return lib.ape_score_lags(layout, msg, ms, spread, ss, md, truth, kind, td, F, C.c_void_p(st.ctypes.data) if len(st) else None,
                                  len(st) if R is None else R, skip, C.c_void_p(bodies.ctypes.data) if bodies is not None else None, nb,
                                  lo, hi, None if of is None else C.c_void_p(of.ctypes.data), score, sd, acc, None)

    big = 2 ** 31 - 1
    bad = [(dict(msg=None), b"NULL"), (dict(truth=None), b"NULL"), (dict(score=None, acc=None), b"both NULL"), (dict(F=0), b"F=0"),
           (dict(starts=()), b"NULL"), (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"),
           (dict(starts=(0, 10)), b"seg_starts[1]"), (dict(ms=24), b"msg_stride"), (dict(ss=20), b"spread_stride"),
           (dict(skip=-1), b"skip"), (dict(nb=2), b"n_bodies"), (dict(nb=0), b"n_bodies"), (dict(bodies=None), b"NULL"),
           (dict(layout=_hip.LAYOUT_NONE), b"layout"), (dict(layout=3), b"layout"), (dict(kind=2), b"truth kind"),
           (dict(md=2), b"dtype"), (dict(td=-1), b"dtype"), (dict(sd=7), b"dtype"),
           (dict(R=0), b"recording starts"), (dict(R=-1), b"recording starts"), (dict(R=11), b"recording starts"),
           # the sweep's own
           (dict(lo=1, hi=0), b"lag_min"), (dict(lo=big, hi=-big), b"lag_min"), (dict(lo=0, hi=65), b"66 lags"), (dict(lo=-big, hi=big), b"lags in the sweep"),
           (dict(lo=129, hi=129), b"|lag|"), (dict(lo=-129, hi=-128), b"|lag|"), (dict(lo=100, hi=129), b"|lag|"),
           (dict(offs=(0, 127, 0)), b"recording 1"), (dict(offs=(0, 0, -127)), b"recording 2"), (dict(offs=(big, 0, 0)), b"recording 0"),
           (dict(offs=(0, -big - 1, 0)), b"recording 1"), (dict(lo=0, hi=0, offs=(0, 0, 129)), b"recording 2")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)                            # APE_ERR_INVALID_ARG
        assert what in lib.ape_last_error() and b"score_lags" in lib.ape_last_error(), (kw, lib.ape_last_error())


def test_header_declares_and_hip_binds_the_entry():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    assert re.search(r"^#define APE_SCORE_MAX_LAG\s+128\b", text, flags=re.M) and re.search(r"^#define APE_SCORE_MAX_LAGS\s+65\b", text, flags=re.M)
    assert re.search(r"^int ape_score_lags\(int32_t layout, const void\* msg_dev, int32_t msg_stride,", text, flags=re.M)
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    assert (_hip.SCORE_MAX_LAG, _hip.SCORE_MAX_LAGS) == (128, 65)
    assert "ape_score_lags" in _hip.SIGNATURES and hasattr(_hip.lib(), "ape_score_lags")
    decl = text[text.index("int ape_score_lags("):]
    decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
    assert len(decl.split(",")) == len(_hip.SIGNATURES["ape_score_lags"][1]) == 22
    assert len(_hip.SIGNATURES["ape_score_rows"][1]) == 19
    for name in ("score_lags", "score_lags_numpy", "best_lag", "align"):
        assert callable(getattr(score, name))
