"""Error distributions per recording without a GPU: the host statement `score.hist_numpy` against a plain double loop,
`lag_trim` against `score_lags_numpy`, what `quantiles`, `fraction_within`, `merge_hist`, `pit_edges` and `pit` promise, the header and
the binding, and every refusal of `ape_score_hist` that needs no device (all are made on the host; the capturing stream is refused in
tests/test_score_hist_gpu.py).

Bounds and where they come from:
* `quantiles`: `lo <= np.quantile(x, q, method="inverted_cdf") <= hi` is a condition, not a tolerance: the value of rank ceil(q n) lies
  in the bin whose cumulative count first reaches that rank.
* `pit_edges`: the bisection ends at neighbouring float64 values, so an edge is within one ulp (1.4e-14 at x = 100, 9e-16 near 6) of the
  quantile; the CDF's slope is below 0.25, and erf, sqrt and exp add a few 2^-53 each: |CDF(edge) - level| <= 1e-12, as the issue states.
* `pit` of N chi^2(3) draws in 10 cells: a cell count is binomial(N, 0.1) with standard deviation sqrt(0.09 N); a deviation of 5 of
  them has probability 5.7e-7 per cell (two-sided normal tail), 5.7e-6 over the 10 cells.  The coverage at level p is binomial(N, p) / N:
  5 sqrt(p (1 - p) / N).  The seed is fixed, so the test either holds or does not."""
import ctypes as C
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def slot_by_hand(v, e):
    """the header's table, one comparison at a time"""
    B = len(e) - 1
    if v != v:
        return B + 2
    if v <= e[0]:
        return B
    if v > e[B]:
        return B + 1
    for b in range(B):
        if e[b] < v <= e[b + 1]:
            return b
    raise AssertionError((v, e))


def hist_by_hand(values, edges, starts, trims):
    F, W = values.shape
    B = edges.shape[1] - 1
    ends = list(starts[1:]) + [F]
    out = np.zeros((len(starts), W, B + 3), dtype=np.int64)
    for r, (s, e) in enumerate(zip(starts, ends)):
        for f in range(s + trims[r][0], e - trims[r][1]):
            for w in range(W):
                out[r, w, slot_by_hand(float(values[f, w]), edges[w])] += 1
    return out


def edge_case_values(e, rng, n):
    """n values of which the first ones are the cases that go wrong: exact edges, +-inf, NaN, -0.0, a subnormal, a widened float32"""
    third = float(np.float32(1.0) / np.float32(3.0))                                     # a float32 value, widened exactly
    special = list(e) + [np.inf, -np.inf, np.nan, -0.0, 0.0, 5e-324, -5e-324, third, np.nextafter(e[1], np.inf), np.nextafter(e[1], -np.inf)]
    v = rng.uniform(e[0] - 0.5, e[-1] + 0.5, size=n)
    v[:len(special)] = special
    return rng.permutation(v)


# ---------------- 1: the host statement ----------------------------------------------------------------------------------------------------------
def test_hist_numpy_against_a_double_loop():
    from wear_mocap_ape_amd.score import hist_numpy
    rng = np.random.default_rng(0)
    edges = np.stack([np.array([0.0, 0.25, float(np.float32(1.0) / np.float32(3.0)), 0.5, 1.0, 2.0]),
                      np.array([-1.0, -0.5, 0.0, 1e-300, 0.75, 3.0]), np.array([-2.0, -1.0, 0.0, 0.5, 0.6, 0.7])])
    F = 300
    vals = np.stack([edge_case_values(edges[w], rng, F) for w in range(3)], axis=1)
    assert np.isnan(vals).sum() == 3 and np.isinf(vals).sum() == 6
    starts, trims = [0, 1, 120], [(0, 0), (0, 0), (7, 11)]
    want = hist_by_hand(vals, edges, starts, trims)
    got = hist_numpy(vals, edges, starts, 0, trims)
    assert got.dtype == np.int64 and got.shape == (3, 3, 8) and np.array_equal(got, want)
    assert np.array_equal(got.sum(axis=2), np.array([[1] * 3, [119] * 3, [162] * 3]))   # every frame of a window in exactly one slot
    # where <= puts -0.0, -inf and the edges themselves
    one = hist_numpy(np.array([[-0.0], [0.0], [-np.inf], [np.inf], [np.nan], [0.25], [np.nextafter(0.25, 1.0)], [2.0], [5e-324]]), edges[0])
    assert one.shape == (1, 1, 8) and one[0, 0].tolist() == [2, 1, 0, 0, 1, 3, 1, 1]
    # skip is added to the head trim; one set of edges serves all columns; float32 goes in widened
    assert np.array_equal(hist_numpy(vals, edges, starts, 5, trims), hist_by_hand(vals, edges, starts, [(5, 0), (5, 0), (12, 11)]))
    v32 = vals.astype(np.float32)
    assert np.array_equal(hist_numpy(v32, edges[0], starts), hist_by_hand(v32.astype(np.float64), np.stack([edges[0]] * 3), starts, [(0, 0)] * 3))
    third = np.array([[np.float32(1.0) / np.float32(3.0)]], dtype=np.float32)            # float32(1 / 3) widened IS the edge: right-closed, bin 1
    assert float(third[0, 0]) == edges[0, 2] and hist_numpy(third, edges[0])[0, 0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    # empty and inverted windows are exact zeros; groups and sets are slices
    z = hist_numpy(vals, edges, starts, 0, [(1, 0), (60, 59), (100, 100)])
    assert not z.any()
    stack = np.stack([vals, vals[::-1]], axis=1)                                          # [F, 2, 3]
    g = hist_numpy(stack, edges, starts, 0, trims)
    assert g.shape == (3, 2, 3, 8) and np.array_equal(g[:, 0], want) and np.array_equal(g[:, 1], hist_numpy(vals[::-1], edges, starts, 0, trims))
    c = hist_numpy(np.stack([stack, stack[:, ::-1]]), edges, starts, 0, trims)
    assert c.shape == (2, 3, 2, 3, 8) and np.array_equal(c[0], g) and np.array_equal(c[1], g[:, ::-1])


def test_lag_trim_gives_the_common_support_of_a_sweep():
    from tests.test_motion_cpu import walk_msgs
    from tests.test_frame_fit_cpu import walk_est
    from wear_mocap_ape_amd import score
    F, starts = 60, [0, 3, 30, 34]                                                        # recordings of 3, 27, 4 and 26 frames
    msg, truth = walk_msgs(F, 0, 1), walk_est(F, 0, 2)
    truth[40] = np.nan                                                                    # unscorable pairs are counted too: [16]
    edges = score.default_edges("score", 16)
    for lags, rec_lags, skip in (((-2, 2), None, 0), ((-2, 2), [1, -3, 0, 2], 0), ((0, 0), [1, -3, 0, 2], 4), ((1, 5), [0, 0, 0, 0], 2)):
        rows, acc = score.score_lags_numpy(msg, truth, 0, lags, starts, skip, None, rec_lags)
        trim = score.lag_trim(starts, F, lags, skip, rec_lags)
        assert trim.dtype == np.int32 and trim.shape == (4, 2) and (trim >= 0).all()
        h = score.hist_numpy(rows, edges, starts, 0, trim)
        assert h.shape == (4, lags[1] - lags[0] + 1, 7, 19)
        total = acc[:, :, 15] + acc[:, :, 16]
        assert np.array_equal(h.sum(axis=3), np.broadcast_to(total[:, :, None], h.shape[:3])), (lags, rec_lags)
        assert np.array_equal(h[:, :, 0, -1], acc[:, :, 16])                             # the NaN slot: the pairs that could not be scored
        assert total[0].max() == 0 or lags == (0, 0)                                      # the 3-frame recording is shorter than the span
    assert score.lag_trim(starts, F, (-2, 2), 1, [1, -3, 0, 2]).tolist() == [[3, 1], [1, 5], [2, 2], [4, 0]]


# ---------------- 2: what is read off a histogram ------------------------------------------------------------------------------------------------
def test_quantiles_bracket_numpys_inverted_cdf():
    from wear_mocap_ape_amd.score import hist_numpy, quantiles
    rng = np.random.default_rng(3)
    qs = (0.0, 0.01, 0.25, 0.5, 0.9, 0.95, 0.999, 1.0)
    checked = 0
    for n in (1, 2, 7, 100, 1001):
        for edges in (np.linspace(-4.0, 4.0, 33), np.exp(np.linspace(np.log(1e-3), np.log(50.0), 65)), np.array([-0.5, 0.5]),
                      np.array([-3.0, -0.1, 0.0, 0.1, 0.3, 3.0])):
            for x in (rng.normal(size=n), rng.exponential(size=n), np.round(rng.normal(size=n), 1)):   # the last: many ties, many on edges
                h = hist_numpy(x[:, None], edges)
                res = quantiles(h, edges, qs)
                assert res["value"].shape == (1, 1, len(qs)) and res["n"].tolist() == [[n]]
                for k, q in enumerate(qs):
                    true = np.quantile(x, q, method="inverted_cdf")
                    lo, hi, val, clip = (res[key][0, 0, k] for key in ("lo", "hi", "value", "clipped"))
                    if clip is None:
                        assert lo <= true <= hi and lo <= val <= hi and lo < hi, (n, q, lo, true, hi)
                        checked += 1
                    elif clip == "below":
                        assert true <= edges[0] and lo == hi == val == edges[0]
                    else:
                        assert clip == "above" and true > edges[-1] and lo == hi == val == edges[-1]
    assert checked > 250                                                                  # (of 480; the rest is clipped)
    # the clipped and the empty cases, and NaN is not counted
    e = np.array([0.0, 1.0, 2.0])
    h = hist_numpy(np.array([[-1.0], [-1.0], [0.5], [5.0], [np.nan]]), e)
    res = quantiles(h, e, (0.25, 0.5, 0.75, 1.0))
    assert res["n"].tolist() == [[4]] and res["clipped"][0, 0].tolist() == ["below", "below", None, "above"]
    assert res["value"][0, 0].tolist() == [0.0, 0.0, 0.5, 2.0] and res["lo"][0, 0, 2] == 0.0 and res["hi"][0, 0, 2] == 1.0
    one = quantiles(h, e, 0.75)
    assert one["value"].shape == (1, 1) and one["value"][0, 0] == 0.5
    empty = quantiles(hist_numpy(np.array([[np.nan], [np.nan]]), e), e, (0.5,))
    assert empty["n"].tolist() == [[0]] and np.isnan(empty["value"]).all() and np.isnan(empty["lo"]).all() and empty["clipped"][0, 0, 0] is None
    with pytest.raises(UserWarning):
        quantiles(h, e, 1.5)
    with pytest.raises(UserWarning):
        quantiles(h, np.array([0.0, 1.0]), 0.5)                                           # edges of another histogram


def test_fraction_within_takes_edges_only():
    from wear_mocap_ape_amd.score import default_edges, fraction_within, hist_numpy
    rng = np.random.default_rng(4)
    x = np.abs(rng.normal(scale=0.06, size=(500, 2)))
    x[:7, 0] = np.nan
    edges = default_edges("score", 64)[:2]
    assert (edges == 0.05).sum() == 2 and (edges == 0.10).sum() == 2                      # the marks are edges, bit for bit
    h = hist_numpy(x, edges)
    got = fraction_within(h, edges, (0.05, 0.10))
    assert got.shape == (1, 2, 2)
    for w in range(2):
        ok = x[~np.isnan(x[:, w]), w]
        assert got[0, w].tolist() == [(ok <= 0.05).sum() / ok.shape[0], (ok <= 0.10).sum() / ok.shape[0]]
    per_column = fraction_within(h, edges, np.array([[0.05], [edges[1, 9]]]))
    assert per_column[0, 1, 0] == (x[:, 1] <= edges[1, 9]).sum() / 500
    for bad in (0.07, np.nextafter(0.05, 1.0), 0.05 + 1e-17 + 1e-9):
        with pytest.raises(UserWarning, match="not an edge"):
            fraction_within(h, edges, (bad,))
    with pytest.raises(UserWarning, match="not an edge"):
        fraction_within(hist_numpy(x, np.array([-1.0, 0.0, 1.0])), np.array([-1.0, 0.0, 1.0]), (-0.0,))   # bit for bit: -0.0 is not 0.0
    assert np.isnan(fraction_within(hist_numpy(np.full((3, 2), np.nan), edges), edges, (0.05,))).all()


def test_merge_hist_of_two_pieces_is_the_whole():
    from wear_mocap_ape_amd.score import hist_numpy, merge_hist, summarise_hist, default_edges
    rng = np.random.default_rng(5)
    F = 400
    x = np.abs(rng.normal(scale=0.2, size=(F, 7)))
    x[rng.integers(0, F, size=9), :] = np.nan
    edges = default_edges("score", 32)
    # two recordings, both cut: piece a holds frames [0, 100) + [200, 270), piece b the rest of each
    a = np.r_[x[0:100], x[200:270]]
    b = np.r_[x[100:200], x[270:400]]
    whole = hist_numpy(x, edges, [0, 200])
    merged = merge_hist(hist_numpy(a, edges, [0, 100]), hist_numpy(b, edges, [0, 100]))
    assert merged.dtype == np.int64 and np.array_equal(merged, whole)
    with pytest.raises(UserWarning):
        merge_hist(whole, whole[:1])
    with pytest.raises(UserWarning):
        merge_hist(whole.astype(np.float64), whole)
    s = summarise_hist(merged, edges)
    assert len(s) == 2 and s[0]["window"] == 200 and set(s[0]["median"]) == {"hand_pos", "elbow_pos", "larm_rot", "uarm_rot", "hips_rot", "hand_d2", "elbow_d2"}
    for r, rows in enumerate((x[:200], x[200:])):
        ok = rows[~np.isnan(rows[:, 0])]
        assert s[r]["nan"]["hand_pos"] == 200 - ok.shape[0]
        for key, q in (("median", 0.5), ("p90", 0.9), ("p95", 0.95)):
            lo, hi = s[r][key + "_bin"]["elbow_pos"]
            assert lo <= np.quantile(ok[:, 1], q, method="inverted_cdf") <= hi and lo <= s[r][key]["elbow_pos"] <= hi


def test_pit_edges_and_a_flat_pit():
    from wear_mocap_ape_amd import score
    e = score.pit_edges(10)
    assert e.shape == (10,) and e[0] == 0.0 and (np.diff(e) > 0).all()
    assert e[5] == score.CHI2_3_Q50 and e[9] == score.CHI2_3_Q90                          # the module's constants, bit for bit
    for cells in (2, 4, 10, 20, 65, 257):
        ec = score.pit_edges(cells)
        worst = max(abs(score.chi2_3_cdf(float(x)) - k / cells) for k, x in enumerate(ec))
        assert ec.shape == (cells,) and worst <= 1e-12, (cells, worst)
    # the closed form itself, against the series of the regularised incomplete gamma function P(3/2, x/2) in exact-enough arithmetic
    for x in (0.01, 0.7, 2.3659738843753377, 6.251388631170325, 20.0):
        t, term, total, k = x / 2.0, 1.0 / 1.5, 1.0 / 1.5, 0
        while term > 1e-18 * total:
            k += 1
            term *= t / (1.5 + k)
            total += term
        series = total * math.exp(-t) * t ** 1.5 / math.gamma(1.5)
        assert abs(score.chi2_3_cdf(x) - series) <= 1e-13, x
    # values drawn from chi^2(3) through the closed-form CDF: u = CDF(x) is uniform, so x is found by bisection on the same CDF
    N, cells = 20000, 10
    g = np.random.default_rng(6).normal(size=(N, 3))
    x = (g * g).sum(axis=1)                                                               # chi^2(3) by its definition
    u = np.array([score.chi2_3_cdf(float(v)) for v in x])
    h = score.hist_numpy(x[:, None], e)
    p = score.pit(h[0, 0])
    assert p["cells"].shape == (cells,) and p["cells"].sum() == N == p["n"] and np.array_equal(p["levels"], np.arange(1, cells) / cells)
    assert np.array_equal(p["cells"], np.bincount(np.minimum((u * cells).astype(int), cells - 1), minlength=cells))   # the cells ARE the PIT's
    dev = np.abs(p["cells"] - N / cells) / math.sqrt(N * 0.1 * 0.9)
    print(f"pit of {N} chi^2(3) draws: largest cell deviation {dev.max():.2f} standard deviations (bound 5)")
    assert dev.max() <= 5.0
    cov = np.abs(p["coverage"] - p["levels"]) / np.sqrt(p["levels"] * (1 - p["levels"]) / N)
    assert cov.max() <= 5.0 and np.array_equal(p["cumulative"], np.cumsum(p["cells"])[:-1])
    assert p["cumulative"][4] == (x <= score.CHI2_3_Q50).sum() and p["cumulative"][8] == (x <= score.CHI2_3_Q90).sum()
    # a spread record that is too narrow piles up in the last cell
    narrow = score.pit(score.hist_numpy(4.0 * x[:, None], e)[0, 0])
    assert narrow["cells"][-1] > 0.4 * N and narrow["coverage"][8] < 0.6
    assert np.isnan(score.pit(np.zeros(12, dtype=np.int64))["coverage"]).all()
    with pytest.raises(UserWarning):
        score.pit_edges(1)


def test_default_edges():
    from wear_mocap_ape_amd import score
    s = score.default_edges("score")
    assert s.shape == (7, 65) and s.dtype == np.float64 and (np.diff(s, axis=1) > 0).all() and np.isfinite(s).all()
    assert np.array_equal(s[5], score.pit_edges(65)) and np.array_equal(s[6], s[5])
    assert s[0, 0] == 1e-4 and s[0, -1] == 10.0 and s[2, 0] == 1e-5 and s[2, -1] > 2 * math.pi
    ratio = s[2, 1:] / s[2, :-1]
    assert np.allclose(ratio, ratio[0], rtol=1e-12)                                       # geometric
    m = score.default_edges("motion", 256)
    assert m.shape == (12, 257) and (np.diff(m, axis=1) > 0).all() and m[2, -1] == 1e6 and m[9, 0] == 1e-3
    for bad in (("other", 64), ("score", 4), ("motion", 257)):
        with pytest.raises(UserWarning):
            score.default_edges(*bad)


# ---------------- 3: header, binding, Makefile ---------------------------------------------------------------------------------------------------
def test_header_declares_and_hip_binds_the_entry():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    for name, value in (("APE_HIST_MAX_BINS", 256), ("APE_HIST_MAX_WIDTH", 16)):
        assert re.search(rf"^#define {name}\s+{value}\b", text, flags=re.M), name
    assert (_hip.HIST_MAX_BINS, _hip.HIST_MAX_WIDTH) == (256, 16) == (score.HIST_MAX_BINS, score.HIST_MAX_WIDTH)
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    params = ["const void* values_dev", "int32_t values_dtype", "int32_t width", "int32_t n_sets", "int64_t set_stride", "int32_t F",
              "int64_t frame_stride", "int32_t n_groups", "int64_t group_stride", "const int32_t* seg_starts_host", "int32_t R",
              "const int32_t* trim_host", "const double* edges_host", "int32_t n_bins", "int64_t* hist_dev", "void* stream"]
    decl = text[text.index("\nint ape_score_hist(") + 1:]
    decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
    got = [" ".join(p.split()) for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
    assert got == params, got
    assert text.index("int ape_score_hist(") > text.index("int ape_motion_sums(")        # after the 4.39 block
    res, args = _hip.SIGNATURES["ape_score_hist"]
    assert hasattr(_hip.lib(), "ape_score_hist") and res is C.c_int and len(args) == len(params)
    for p, a in zip(params, args):                                                       # every ctypes argument is the declared one's
        want = C.c_void_p if "*" in p else (C.c_int64 if p.startswith("int64_t") else C.c_int32)
        assert a is want, (p, a)
    assert _hip.lib().ape_score_hist.argtypes == args
    make = (REPO / "arm-pose-estimation_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS\s*:=(.*)$", make, flags=re.M).group(1).split()
    hazard = re.search(r"^HAZARD_SRCS\s*:=(.*)$", make, flags=re.M).group(1).split()
    assert "score_hist.hip" in srcs and "score_hist.hip" not in hazard
    source = (REPO / "arm-pose-estimation_amd" / "csrc" / "score_hist.hip").read_text()
    assert "asm" not in re.sub(r"//.*", "", source)                                       # plain HIP
    for name in ("hist_rows", "hist_numpy", "lag_trim", "merge_hist", "quantiles", "fraction_within", "default_edges", "pit_edges", "pit",
                 "summarise_hist"):
        assert callable(getattr(score, name)), name
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    want = ["self", "out", "truth", "spread", "starts", "skip", "bonemaps", "truth_kind", "rec_lags", "edges", "bins"]
    for cls in (Estimator, WatchPhoneUarm, WatchPhonePocketKalman):
        assert "error_distribution" in vars(cls) and list(inspect.signature(cls.error_distribution).parameters) == want
    assert inspect.signature(Estimator.error_distribution).parameters["bins"].default == 64


# ---------------- 4: the refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_are_made_on_the_host():
    """every refusal include/ape_hip.h states but the capturing stream: APE_ERR_INVALID_ARG before any device call.  The pointers are host
    memory here: a refused call reads no value and leaves the sentinel-filled output as it was"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    F, W, B = 10, 3, 4
    values = np.zeros((2, F, 2, W))
    hist = np.full((2, 3, 2, W, B + 3), -7, dtype=np.int64)
    good_edges = np.tile(np.arange(B + 1, dtype=np.float64), (W, 1))
    vp, hp = C.c_void_p(values.ctypes.data), C.c_void_p(hist.ctypes.data)

    def call(v=vp, dt=_hip.F64, w=W, n_sets=1, ss=0, F=F, fs=2 * W, G=1, gs=0, starts=(0, 3, 7), R=None, trim=None, edges=good_edges, B=B, h=hp):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        tr = None if trim is None else np.ascontiguousarray(trim, dtype=np.int32)
        e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
        return lib.ape_score_hist(v, dt, w, n_sets, ss, F, fs, G, gs, C.c_void_p(st.ctypes.data) if len(st) else None,
                                  len(st) if R is None else R, None if tr is None else C.c_void_p(tr.ctypes.data),
                                  None if e is None else C.c_void_p(e.ctypes.data), B, h, None)

    def edges_with(w, i, x):
        e = good_edges.copy()
        e[w, i] = x
        return e

    inside = C.c_void_p(values.ctypes.data + 8 * 5)                                       # an output that starts inside the values
    before = C.c_void_p(values.ctypes.data - 8 * 4)                                       # ... and one whose end reaches into them
    bad = [(dict(v=None), b"NULL"), (dict(starts=()), b"NULL"), (dict(edges=None), b"NULL"), (dict(h=None), b"NULL"),
           (dict(F=0), b"F=0"), (dict(F=-1), b"F=-1"), (dict(R=0), b"recording starts"), (dict(R=-1), b"recording starts"), (dict(R=11), b"recording starts"),
           (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 10)), b"seg_starts[1]"),
           (dict(trim=[(0, 0), (-1, 0), (0, 0)]), b"trim[1]"), (dict(trim=[(0, 0), (0, 0), (0, -5)]), b"trim[2]"),
           (dict(w=0), b"width"), (dict(w=17, fs=17), b"width"), (dict(w=-2), b"width"),
           (dict(B=0), b"n_bins"), (dict(B=257), b"n_bins"), (dict(B=-1), b"n_bins"),
           (dict(n_sets=0), b"n_sets"), (dict(n_sets=65, ss=60), b"n_sets"), (dict(n_sets=-3), b"n_sets"),
           (dict(G=0), b"n_groups"), (dict(G=66, gs=W), b"n_groups"), (dict(G=-1), b"n_groups"),
           (dict(fs=W - 1), b"frame_stride"), (dict(fs=0), b"frame_stride"), (dict(fs=-6), b"frame_stride"),
           (dict(G=2, gs=W - 1), b"group_stride"), (dict(G=2, gs=0), b"group_stride"), (dict(G=2, gs=-W), b"group_stride"),
           (dict(n_sets=2, ss=10 * 2 * W - 1), b"set_stride"), (dict(n_sets=2, ss=0), b"set_stride"), (dict(n_sets=2, ss=-(2 ** 40)), b"set_stride"),
           (dict(n_sets=2, fs=2 ** 61, ss=2 ** 62), b"set_stride"),
           (dict(fs=2 ** 62), b"extent"), (dict(G=2, gs=2 ** 62, fs=2 ** 59), b"extent"), (dict(n_sets=64, ss=2 ** 58), b"extent"),
           (dict(dt=2), b"dtype"), (dict(dt=-1), b"dtype"),
           (dict(v=C.c_void_p(values.ctypes.data + 4)), b"aligned"), (dict(h=C.c_void_p(hist.ctypes.data + 4)), b"aligned"),
           (dict(dt=_hip.F32, v=C.c_void_p(values.ctypes.data + 2)), b"aligned"),
           (dict(edges=edges_with(1, 2, np.nan)), b"edges[1][2]"), (dict(edges=edges_with(0, 4, np.inf)), b"edges[0][4]"),
           (dict(edges=edges_with(2, 0, -np.inf)), b"edges[2][0]"), (dict(edges=edges_with(1, 3, 2.0)), b"edges[1][3]"),
           (dict(edges=edges_with(2, 1, 5.0)), b"edges[2][2]"),
           (dict(n_sets=64, ss=200 * 65 * 16, G=65, gs=16, w=16, fs=65 * 16, F=200, B=256, starts=np.arange(130),
                 edges=np.tile(np.arange(257, dtype=np.float64), (16, 1))), b"output elements"),      # 64 * 130 * 65 * 16 * 259 > 2^31 - 1
           (dict(h=vp), b"overlaps"), (dict(h=inside), b"overlaps"), (dict(h=before), b"overlaps"),
           (dict(n_sets=2, ss=F * 2 * W, G=2, gs=W, h=C.c_void_p(values.ctypes.data + 8 * (F * 2 * W + 50))), b"overlaps")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc, lib.ape_last_error())                                    # APE_ERR_INVALID_ARG
        assert what in lib.ape_last_error() and b"score_hist" in lib.ape_last_error(), (kw, lib.ape_last_error())
    assert (hist == -7).all() and not values.any()
