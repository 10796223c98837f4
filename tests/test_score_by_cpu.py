"""Errors by condition (`ape_score_by`) without a GPU: the numpy statement `score.stats_by_numpy`, the host functions on
its records, the header, the binding and every refusal the entry makes before its first device call.

There is no tolerance on the statement: it is compared bit for bit with a plain Python loop that adds one term at a time in the stated
order (frames in order within a piece of 1024 frames counted from the window's first frame, pieces in order, both from +0.0).  The one
bound of this file is `merge_by`'s: two chained halves add the same n terms of a cell in another order, and the two sums lie within
n 2^-53 sum|x| of each other (each addition rounds by at most 2^-53 of a partial sum, which sum|x| bounds); n and the maximum are exact."""
import ctypes as C
import inspect
import re
import struct
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
U = 2.0 ** -53
PIECE = 1024


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    """equal shapes, NaN in the same places, the same bits everywhere else (a NaN's sign and payload are not part of the contract)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return bool(np.array_equal(bits(a)[keep], bits(b)[keep]))


def slot_by_hand(v, e):
    """include/ape_hip.h's table, one comparison at a time"""
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
    raise AssertionError(v)


def by_hand(keys, values, edges, starts, trims, one_chain=False):
    """[R, K, B + 3, V, 4] of keys [F, K] and values [F, V] by Python floats, one addition at a time in the stated order; one_chain: the
    whole window as one piece"""
    F, K = keys.shape
    V = values.shape[1]
    B = edges.shape[1] - 1
    ends = list(starts[1:]) + [F]
    out = np.zeros((len(starts), K, B + 3, V, 4))
    out[..., 3] = -np.inf
    for r, (s, e) in enumerate(zip(starts, ends)):
        lo, up = s + trims[r][0], e - trims[r][1]
        step = max(1, up - lo) if one_chain else PIECE
        for k in range(K):
            for p0 in range(lo, up, step):
                piece = np.zeros((B + 3, V, 3))
                for f in range(p0, min(up, p0 + step)):
                    sl = slot_by_hand(float(keys[f, k]), edges[k])
                    for v in range(V):
                        x = float(values[f, v])
                        if x != x:
                            continue
                        piece[sl, v, 0] += 1.0
                        piece[sl, v, 1] = float(piece[sl, v, 1]) + x
                        piece[sl, v, 2] = float(piece[sl, v, 2]) + x * x
                        out[r, k, sl, v, 3] = max(out[r, k, sl, v, 3], x)
                out[r, k, :, :, :3] = out[r, k, :, :, :3] + piece
    return out


EDGES = np.array([[-1.0, -0.5, 0.0, 0.5, 1.0], [0.0, 1.0, 2.0, 4.0, 8.0]])


# ---------------- 1: the statement ---------------------------------------------------------------------------------------------------------------
def test_statement_equals_a_plain_loop_on_tiny_inputs():
    from wear_mocap_ape_amd.score import stats_by_numpy
    rng = np.random.default_rng(1)
    F = 40
    keys = np.stack([rng.uniform(-1.3, 1.3, size=F), rng.uniform(-1.0, 9.0, size=F)], axis=1)
    keys[[3, 17], [0, 1]] = np.nan
    keys[5, 0], keys[6, 0], keys[7, 1] = -0.5, 1.0, 0.0                                   # on edges: right-closed bins, below
    values = rng.normal(size=(F, 3)) * 10.0 ** rng.integers(-3, 4, size=(F, 3))
    values[[2, 9], [0, 2]] = np.nan
    values[11, 1], values[12, 1], values[13, 2], values[14, 0] = np.inf, np.inf, -np.inf, -0.0
    starts, trims = [0, 9, 10, 30], [(0, 0), (0, 0), (2, 3), (4, 7)]
    got = stats_by_numpy(keys, values, EDGES, starts, 0, trims)
    want = by_hand(keys, values, EDGES, starts, trims)
    assert got.shape == (4, 2, 7, 3, 4) and same_bits(got, want)
    assert not got[3, ..., :3].any() and (got[3, ..., 3] == -np.inf).all()                # an inverted window: zeros and -inf
    # skip is added to the head trim; a shared side and a side with sets
    assert same_bits(stats_by_numpy(keys, values, EDGES, starts, 2, [(0, 0), (0, 0), (0, 3), (2, 7)]),
                     by_hand(keys, values, EDGES, starts, [(2, 0), (2, 0), (2, 3), (4, 7)]))
    sets = np.stack([values, values[::-1].copy()])
    both = stats_by_numpy(keys, sets, EDGES, starts, 0, trims)
    assert both.shape == (2, 4, 2, 7, 3, 4) and same_bits(both[0], got) and same_bits(both[1], by_hand(keys, sets[1], EDGES, starts, trims))
    ksets = np.stack([keys, keys[::-1].copy()])
    assert same_bits(stats_by_numpy(ksets, values, EDGES, starts, 0, trims)[1], by_hand(ksets[1], values, EDGES, starts, trims))
    assert stats_by_numpy(keys[None], values, EDGES, starts, 0, trims).shape == (1, 4, 2, 7, 3, 4)
    # float32 is widened exactly
    assert same_bits(stats_by_numpy(keys.astype(np.float32), values.astype(np.float32), EDGES, starts, 0, trims),
                     by_hand(keys.astype(np.float32).astype(np.float64), values.astype(np.float32).astype(np.float64), EDGES, starts, trims))
    for bad in (lambda: stats_by_numpy(keys[:30], values, EDGES), lambda: stats_by_numpy(keys, values, EDGES[:1]),
                lambda: stats_by_numpy(ksets, np.stack([values] * 3), EDGES), lambda: stats_by_numpy(keys, values, EDGES, skip=-1)):
        with pytest.raises(UserWarning):
            bad()


def test_minus_zero_and_the_start_from_plus_zero():
    """a cell whose only terms are -0.0 sums to +0.0 (the sum starts at +0.0); its maximum is a zero"""
    from wear_mocap_ape_amd.score import stats_by_numpy
    got = stats_by_numpy(np.full((3, 1), 0.25), np.full((3, 1), -0.0), EDGES[:1])
    cell = got[0, 0, 2, 0]
    assert cell[0] == 3.0 and bits(cell[1]) == bits(0.0) and bits(cell[2]) == bits(0.0) and cell[3] == 0.0
    assert struct.pack("<d", float(np.cumsum(np.array([-0.0]))[-1])) == struct.pack("<d", -0.0)      # what a cumsum without the +0.0 would give


def test_the_piece_order_is_the_statement():
    """2500 frames in one window, magnitudes over 16 decades: the sum by pieces of 1024 and the sum in one chain differ in bits, and the
    statement gives the former.  The pieces are counted from the window's first frame, wherever the window begins."""
    from wear_mocap_ape_amd.score import stats_by_numpy
    rng = np.random.default_rng(2)
    n = 2500
    x = (rng.normal(size=(n, 2)) * 10.0 ** rng.uniform(-8, 8, size=(n, 2)))
    keys = rng.uniform(-1.0, 1.0, size=(n, 1))
    got = stats_by_numpy(keys, x, EDGES[:1])
    pieces, chain = by_hand(keys, x, EDGES[:1], [0], [(0, 0)]), by_hand(keys, x, EDGES[:1], [0], [(0, 0)], one_chain=True)
    assert same_bits(got[0], pieces[0])
    assert not np.array_equal(bits(pieces[..., 1:3]), bits(chain[..., 1:3]))              # the order matters at these magnitudes
    assert np.array_equal(pieces[..., [0, 3]], chain[..., [0, 3]])
    # np.cumsum adds one by one; np.sum does not
    col = x[:, 0]
    one_by_one = 0.0
    for v in col:
        one_by_one = one_by_one + float(v)
    assert bits(np.cumsum(col)[-1]) == bits(one_by_one)
    # embedded at an offset that is no multiple of the piece: the same record
    pad = 700
    k2, x2 = np.concatenate([rng.uniform(-1, 1, size=(pad, 1)), keys]), np.concatenate([rng.normal(size=(pad, 2)), x])
    assert same_bits(stats_by_numpy(k2, x2, EDGES[:1], [0, pad])[1], got[0])
    assert same_bits(stats_by_numpy(k2, x2, EDGES[:1], [0], 0, [(pad, 0)])[0], got[0])      # a trim is a slice


def test_counts_are_the_histogram_of_the_keys():
    from wear_mocap_ape_amd.score import hist_numpy, stats_by_numpy
    rng = np.random.default_rng(3)
    F, starts, trim = 3000, [0, 100, 1300], [(0, 5), (3, 0), (10, 10)]
    keys = np.stack([rng.uniform(-1.2, 1.2, size=F), rng.uniform(-1.0, 9.0, size=F)], axis=1)
    keys[rng.integers(0, F, size=40), rng.integers(0, 2, size=40)] = np.nan
    values = rng.normal(size=(F, 3))
    by = stats_by_numpy(keys, values, EDGES, starts, 0, trim)
    h = hist_numpy(keys, EDGES, starts, 0, trim)
    for v in range(3):
        assert np.array_equal(by[..., v, 0], h.astype(np.float64))                        # [R, K, B + 3]
    values[rng.integers(0, F, size=60), 1] = np.nan
    by = stats_by_numpy(keys, values, EDGES, starts, 0, trim)
    ends = starts[1:] + [F]
    for r, (s, e) in enumerate(zip(starts, ends)):
        lo, up = s + trim[r][0], e - trim[r][1]
        for k in range(2):
            assert by[r, k, :, 1, 0].sum() == (up - lo) - np.isnan(values[lo:up, 1]).sum()    # the window less the NaN values
            assert by[r, k, :, 0, 0].sum() == up - lo


# ---------------- 2: the host functions on records ---------------------------------------------------------------------------------------------
def test_merge_by_of_chained_halves():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(4)
    F, starts = 5000, [0, 2600]
    keys = rng.uniform(-1.2, 1.2, size=(F, 1))
    x = rng.normal(size=(F, 2)) * 10.0 ** rng.uniform(-4, 4, size=(F, 2))
    whole = score.stats_by_numpy(keys, x, EDGES[:1], starts)
    ia, ib = np.r_[0:1111, 2600:3900], np.r_[1111:2600, 3900:5000]                      # neither cut lies on a piece border
    a = score.stats_by_numpy(keys[ia], x[ia], EDGES[:1], [0, 1111])
    b = score.stats_by_numpy(keys[ib], x[ib], EDGES[:1], [0, 1489])
    merged = score.merge_by(a, b)
    assert np.array_equal(merged[..., 0], whole[..., 0]) and np.array_equal(merged[..., 3], whole[..., 3])
    mag = score.stats_by_numpy(keys, np.abs(x), EDGES[:1], starts)
    n = whole[..., 0]
    assert (np.abs(merged[..., 1] - whole[..., 1]) <= n * U * mag[..., 1]).all()
    assert (np.abs(merged[..., 2] - whole[..., 2]) <= n * U * mag[..., 2]).all()
    assert score.merge_by(np.stack([a, a]), np.stack([b, b])).shape == (2, 2, 1, 7, 2, 4)
    with pytest.raises(UserWarning):
        score.merge_by(a, b[:1])


def test_pool_and_summarise_with_an_empty_cell():
    from wear_mocap_ape_amd import score
    keys = np.array([[0.25], [0.3], [0.75], [0.8], [0.9]])
    x = np.array([[3.0, 1.0], [4.0, np.nan], [-2.0, 2.0], [6.0, 2.0], [1.0, 2.0]])
    by = score.stats_by_numpy(keys, x, EDGES[:1], [0, 2])
    pooled = score.pool_by(by)
    assert pooled.shape == (1, 7, 2, 4) and same_bits(pooled, score.stats_by_numpy(keys, x, EDGES[:1])[0])
    assert score.pool_by(np.stack([by, by])).shape == (2, 1, 7, 2, 4)
    s = score.summarise_by(pooled, EDGES[:1], ["key"], ["a", "b"])
    assert s["n"].shape == (1, 7, 2) and s["key_names"] == ("key",) and s["value_names"] == ("a", "b")
    assert s["slots"][0] == ["(-1, -0.5]", "(-0.5, 0]", "(0, 0.5]", "(0.5, 1]", "below", "above", "nan"]
    assert s["n"][0, 2].tolist() == [2.0, 1.0] and s["mean"][0, 2].tolist() == [3.5, 1.0] and s["max"][0, 2].tolist() == [4.0, 1.0]
    assert s["rms"][0, 2, 0] == np.sqrt(12.5) and s["rms"][0, 3, 0] == np.sqrt(41.0 / 3.0) and s["mean"][0, 3, 1] == 2.0
    empty = s["n"][0, 0]                                                                  # nothing in (-1, -0.5]
    assert not empty.any() and np.isnan(s["mean"][0, 0]).all() and np.isnan(s["rms"][0, 0]).all() and (s["max"][0, 0] == -np.inf).all()
    assert not pooled[0, 0, :, :3].any() and (pooled[0, 0, :, 3] == -np.inf).all()
    per_recording = score.summarise_by(by, EDGES[:1])
    assert per_recording["mean"].shape == (2, 1, 7, 2) and per_recording["key_names"] == ("key0",) and np.isnan(per_recording["mean"][0, 0, 3, 0])
    with pytest.raises(UserWarning):
        score.summarise_by(by, EDGES[:1, :4])
    with pytest.raises(UserWarning):
        score.summarise_by(by, EDGES[:1], value_names=["a"])


def close_sigmas(got, want):
    """NaN in the same places; the angular spreads are copies, bit for bit; the two roots within 2 ulp: the traces are the same IEEE
    additions in the same order on both sides, and a square root routine is within one ulp of the root (numpy's, correctly rounded,
    within half; a vectorised one of torch's need not round correctly), so two of them lie within 2 ulp <= 2^-51 |root| of each other"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)) or not same_bits(got[..., 2:], want[..., 2:]):
        return False
    keep = ~np.isnan(want[..., :2])
    return bool((np.abs(got[..., :2][keep] - want[..., :2][keep]) <= 2.0 ** -51 * np.abs(want[..., :2][keep])).all())


def test_spread_sigma_against_numpy():
    import torch
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(5)
    rec = rng.uniform(0.0, 1.0, size=(50, 21))
    rec[3, 6], rec[4, 15] = np.nan, -5.0
    got = score.spread_sigma(torch.from_numpy(rec)).numpy()
    with np.errstate(all="ignore"):
        want = np.concatenate([np.sqrt((rec[:, 3] + rec[:, 6]) + rec[:, 8])[:, None], np.sqrt((rec[:, 12] + rec[:, 15]) + rec[:, 17])[:, None],
                               rec[:, 18:21]], axis=1)
    assert got.shape == (50, 5) and close_sigmas(got, want) and np.isnan(got[3, 0]) and np.isnan(got[4, 1]) and len(score.SIGMA_NAMES) == 5
    wide = np.concatenate([rec, rng.normal(size=(50, 4))], axis=1)                        # the record in the first 21 columns
    assert close_sigmas(score.spread_sigma(torch.from_numpy(wide)).numpy(), want)
    assert score.spread_sigma(torch.from_numpy(np.stack([rec, rec]))).shape == (2, 50, 5)
    with pytest.raises(UserWarning):
        score.spread_sigma(torch.zeros((4, 20)))


# ---------------- 3: header, binding, refusals ---------------------------------------------------------------------------------------------------
PARAMS = ["const void* keys_dev", "int32_t keys_dtype", "int32_t n_keys", "int64_t keys_set_stride", "int64_t keys_frame_stride",
          "const void* values_dev", "int32_t values_dtype", "int32_t n_values", "int64_t values_set_stride", "int64_t values_frame_stride",
          "int32_t n_sets", "int32_t F", "const int32_t* seg_starts_host", "int32_t R", "const int32_t* trim_host", "const double* edges_host",
          "int32_t n_bins", "double* by_dev", "void* stream"]


def test_header_declares_and_hip_binds_the_entry():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    for name, value in (("APE_BY_MAX_KEYS", 8), ("APE_BY_MAX_VALUES", 16), ("APE_BY_MAX_BINS", 125), ("APE_BY_PIECE", 1024)):
        assert re.search(rf"^#define {name}\s+{value}\b", text, flags=re.M), name
    assert (_hip.BY_MAX_KEYS, _hip.BY_MAX_VALUES, _hip.BY_MAX_BINS, _hip.BY_PIECE) == (8, 16, 125, 1024)
    assert (score.BY_MAX_KEYS, score.BY_MAX_VALUES, score.BY_MAX_BINS, score.BY_PIECE) == (8, 16, 125, 1024)
    assert score.angle_edges(72).shape[1] - 1 <= score.BY_MAX_BINS                        # the angle edges fit
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    decl = text[text.index("\nint ape_score_by(") + 1:]
    decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
    got = [" ".join(p.split()) for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
    assert got == PARAMS, got
    assert text.index("int ape_score_by(") > text.index("int ape_joint_angles(")          # after the 4.41 block
    res, args = _hip.SIGNATURES["ape_score_by"]
    assert hasattr(_hip.lib(), "ape_score_by") and res is C.c_int and len(args) == len(PARAMS)      # the library exports the symbol
    for p, a in zip(PARAMS, args):
        want = C.c_void_p if "*" in p else (C.c_int64 if p.startswith("int64_t") else C.c_int32)
        assert a is want, (p, a)
    assert _hip.lib().ape_score_by.argtypes == args
    make = (REPO / "arm-pose-estimation_amd" / "csrc" / "Makefile").read_text()
    assert "score_by.hip" in re.search(r"^SRCS\s*:=(.*)$", make, flags=re.M).group(1).split()
    for name in ("stats_by", "stats_by_numpy", "merge_by", "pool_by", "summarise_by", "spread_sigma"):
        assert callable(getattr(score, name))
    sig = inspect.signature(score.stats_by_numpy)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[3:]] == [("starts", None), ("skip", 0), ("trim", None)]
    assert list(inspect.signature(score.stats_by).parameters) == list(sig.parameters) == ["keys", "values", "edges", "starts", "skip", "trim"]
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    for cls in (Estimator, WatchPhoneUarm, WatchPhonePocketKalman):
        assert "errors_by" in vars(cls)
        sig = inspect.signature(cls.errors_by)
        assert [(p.name, p.default) for p in list(sig.parameters.values())[4:]] == [
            ("spread", None), ("starts", None), ("skip", None), ("bonemaps", None), ("truth_kind", "targets"), ("rec_lags", None),
            ("edges", None), ("bins", 36), ("times", None)]
        assert list(sig.parameters)[:4] == ["self", "out", "truth", "by"]


def call_entry(ptrs, keys="keys", kd=None, K=2, kss=0, kfs=2, values="values", vd=None, V=3, vss=0, vfs=3, n_sets=1, F=10, starts=(0, 3, 7),
               R=None, trim=None, edges="default", B=4, by="by", stream=None):
    """ape_score_by with the named pointers of `ptrs` (an output named after another buffer aliases it; an integer is an address)"""
    from wear_mocap_ape_amd import _hip
    st = np.ascontiguousarray(starts, dtype=np.int32)
    tr = None if trim is None else np.ascontiguousarray(trim, dtype=np.int32)
    if isinstance(edges, str):
        edges = np.tile(np.arange(max(B, 1) + 1, dtype=np.float64), (max(K, 1), 1))
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
    p = lambda name: None if name is None else (C.c_void_p(name) if isinstance(name, int) else ptrs[name])    # noqa: E731
    return _hip.lib().ape_score_by(p(keys), _hip.F64 if kd is None else kd, K, kss, kfs, p(values), _hip.F64 if vd is None else vd, V, vss, vfs,
                                   n_sets, F, C.c_void_p(st.ctypes.data) if len(st) else None, len(st) if R is None else R,
                                   None if tr is None else C.c_void_p(tr.ctypes.data), None if e is None else C.c_void_p(e.ctypes.data), B,
                                   p(by), stream)


BIG_PIECES = (10_000_000 + PIECE - 1) // PIECE * 8 * 128 * 16 * 4 * 8                     # bytes of piece records of the case below


def refusals():
    """(keyword overrides of `call_entry`, a word of the message) of every refusal include/ape_hip.h states but the capturing stream"""
    from wear_mocap_ape_amd import _hip
    bad_edges = np.tile(np.arange(5.0), (2, 1))
    nan_e, flat_e, inf_e = bad_edges.copy(), bad_edges.copy(), bad_edges.copy()
    nan_e[1, 2], flat_e[0, 3], inf_e[1, 4] = np.nan, 2.0, np.inf
    return [(dict(keys=None), b"NULL"), (dict(values=None), b"NULL"), (dict(starts=()), b"NULL"), (dict(edges=None), b"NULL"), (dict(by=None), b"NULL"),
            (dict(F=0), b"F=0"), (dict(R=0), b"recording starts"), (dict(R=11), b"recording starts"),
            (dict(starts=(1, 3)), b"seg_starts[0]"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 10)), b"seg_starts[1]"),
            (dict(trim=[(0, 0), (-1, 0), (0, 0)]), b"trim[1]"), (dict(trim=[(0, 0), (0, 0), (0, -2)]), b"trim[2]"),
            (dict(n_sets=0), b"n_sets"), (dict(n_sets=65, kss=20, vss=30), b"n_sets"),
            (dict(B=0), b"n_bins"), (dict(B=126), b"n_bins"), (dict(K=0), b"n_keys"), (dict(K=9, kfs=9), b"n_keys"),
            (dict(V=0), b"n_values"), (dict(V=17, vfs=17), b"n_values"),
            (dict(kd=2), b"keys dtype"), (dict(vd=-1), b"values dtype"),
            (dict(kfs=1), b"keys_frame_stride"), (dict(vfs=2), b"values_frame_stride"), (dict(kfs=-2), b"keys_frame_stride"),
            (dict(n_sets=2, kss=19, vss=30), b"keys_set_stride"), (dict(n_sets=2, kss=20, vss=29), b"values_set_stride"),
            (dict(n_sets=2, kss=-20, vss=0), b"keys_set_stride"), (dict(n_sets=2, kss=0, vss=1), b"values_set_stride"),
            (dict(kfs=2 ** 62), b"63 bits"), (dict(n_sets=3, vss=2 ** 62, vfs=3), b"63 bits"),
            (dict(keys=4096 + 4), b"keys_dev is not aligned"), (dict(values=8192 + 2, vd=_hip.F32), b"values_dev is not aligned"),
            (dict(by=(1 << 30) + 4), b"by_dev is not aligned"),
            (dict(edges=nan_e), b"edges[1][2]"), (dict(edges=flat_e), b"edges[0][3]"), (dict(edges=inf_e), b"edges[1][4]"),
            (dict(edges=bad_edges[:, ::-1]), b"edges[0][1]"),
            (dict(n_sets=64, kss=4800, vss=9600, K=8, kfs=8, V=16, vfs=16, B=125, F=600, starts=tuple(range(600))), b"output elements"),
            (dict(K=8, kfs=8, V=16, vfs=16, B=125, F=10_000_000, starts=(0,), by=1 << 40), str(BIG_PIECES).encode() + b" bytes of piece records"),
            (dict(by="keys"), b"overlaps keys_dev"), (dict(by="values"), b"overlaps values_dev"),
            (dict(by=4096 + 8 * 19), b"overlaps keys_dev"), (dict(keys=(1 << 30) + 8 * 100), b"overlaps keys_dev"),
            (dict(values=(1 << 30) + 8 * (3 * 2 * 7 * 3 * 4 - 1)), b"overlaps values_dev")]


def test_refusals_are_made_on_the_host():
    """APE_ERR_INVALID_ARG before any device call (the pointers are never read; this machine has no device to call)"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    ptrs = {"keys": C.c_void_p(4096), "values": C.c_void_p(8192), "by": C.c_void_p(1 << 30)}
    for kw, what in refusals():
        rc = call_entry(ptrs, **kw)
        assert rc == 1, (kw, rc)                            # APE_ERR_INVALID_ARG
        assert what in lib.ape_last_error() and b"score_by" in lib.ape_last_error(), (kw, lib.ape_last_error())
    assert BIG_PIECES > 2 ** 30
