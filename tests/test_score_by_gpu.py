"""Errors by condition (`ape_score_by`) on the GPU.

Reference of every number: `score.stats_by_numpy` on the same inputs.  There is no tolerance in this file: counts, sums and sums of
squares are compared bit for bit (a NaN sum -- a cell that holds +inf and -inf -- must be NaN on both sides; its sign and payload are not
stated), maxima by value.

The borders of the kernel's own tiling that the shapes sit on: a piece is 1024 frames of one window, counted from the window's first
frame (1023, 1024, 1025, 2049 frames; windows that begin at 1000 and 1030 of the batch); a workgroup takes its piece in sub-tiles of 256
frames, a lane per frame, each wave staging 64 rows (1, 255, 256, 257 frames); the four waves split the value columns, wave w taking
columns w, w + 4, ... (V = 1: three idle waves; 4: one column each; 5: wave 0 takes two; 16: four each); a lane owns slots `lane` and
`lane + 64`, and the second is compiled out up to 64 slots (B = 61: 64 slots; 62: 65; 125: 128); the fold kernel takes 256 accumulators
per workgroup (V = 16, B = 125: 32 chunks; V = 1, B = 1: a quarter of one) and a recording without a window gets its zeros there (70
one-frame recordings; trims that empty a window, invert one, and empty at the tail); more than 8 key columns go 8 to a call (the motion
keys of `errors_by`)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_score_by_cpu import call_entry, refusals, same_bits

pytestmark = pytest.mark.gpu

HIPS, WATCH = 0, 1


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def on_device(keys, values, edges, starts=None, skip=0, trim=None):
    from wear_mocap_ape_amd import score
    by = score.stats_by(keys if isinstance(keys, torch.Tensor) else dev(keys), values if isinstance(values, torch.Tensor) else dev(values),
                        edges, starts, skip, trim)
    torch.cuda.synchronize()
    assert by.dtype == torch.float64
    return by.cpu().numpy()


def same_record(got, ref):
    return got.shape == ref.shape and same_bits(got[..., :3], ref[..., :3]) and np.array_equal(got[..., 3], ref[..., 3])


def check(keys, values, edges, starts=None, skip=0, trim=None, what=""):
    """the device's record of numpy `keys` and `values` is the host statement's; -> the record"""
    from wear_mocap_ape_amd import score
    got = on_device(keys, values, edges, starts, skip, trim)
    ref = score.stats_by_numpy(keys, values, edges, starts, skip, trim)
    assert same_record(got, ref), (what, got.shape, ref.shape, np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:5])
    return got


def wide_values(rng, shape):
    """magnitudes over 12 decades, both signs: any other order of the additions shows in the bits"""
    return rng.normal(size=shape) * 10.0 ** rng.uniform(-6, 6, size=shape)


def keys_over(rng, F, edges):
    """keys [F, K] over and beyond each column's edges, every slot but NaN likely hit"""
    return np.stack([rng.uniform(e[0] - 0.1 * (e[-1] - e[0]), e[-1] + 0.1 * (e[-1] - e[0]), size=F) for e in edges], axis=1)


EDGES = np.stack([np.linspace(-1.0, 1.0, 5), np.linspace(0.0, 8.0, 5)])


# ---------------- 1: windows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,starts,trim", [
    (1, [0], None), (255, [0], None), (256, [0], None), (257, [0], None),                 # the sub-tile's borders
    (1023, [0], None), (1024, [0], None), (1025, [0], None), (2049, [0], None),           # the piece's borders
    (2100, [0, 1000, 1030], None),                                                        # windows that begin mid-piece of the batch
    (70, list(range(70)), None),                                                          # 70 one-frame recordings
    (300, [0, 100, 200], [(100, 0), (30, 71), (0, 100)]),                                 # trims that empty a window, invert one, empty at the tail
    (2300, [0, 100, 1200], [(3, 5), (0, 0), (70, 6)]),                                    # 1024 frames left of the last: exactly one piece
])
def test_windows_at_the_borders(F, starts, trim):
    rng = np.random.default_rng(F + len(starts))
    keys, values = keys_over(rng, F, EDGES), wide_values(rng, (F, 3))
    got = check(keys, values, EDGES, starts, 0, trim, (F, starts[:4]))
    ends = starts[1:] + [F]
    tr = trim if trim is not None else [(0, 0)] * len(starts)
    want = [max(0, (e - b) - (s + a)) for s, e, (a, b) in zip(starts, ends, tr)]
    assert got.shape == (len(starts), 2, 7, 3, 4)
    assert np.array_equal(got[..., 0].sum(axis=2), np.tile(np.array(want, dtype=np.float64)[:, None, None], (1, 2, 3)))      # every frame in one slot
    if trim is not None and trim[0] == (100, 0):
        assert not got[..., :3].any() and (got[..., 3] == -np.inf).all()                  # exact zeros and -inf maxima


def test_skip_is_added_to_the_head_trim():
    rng = np.random.default_rng(1)
    keys, values = keys_over(rng, 300, EDGES), wide_values(rng, (300, 2))
    a = check(keys, values, EDGES, [0, 100], 7, [(1, 2), (0, 4)])
    assert same_record(a, on_device(keys, values, EDGES, [0, 100], 0, [(8, 2), (7, 4)]))
    assert a[..., 0].sum(axis=2).tolist() == [[[90.0] * 2] * 2, [[189.0] * 2] * 2]


# ---------------- 2: the limits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 61, 62, 125])
@pytest.mark.parametrize("V", [1, 4, 5, 16])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_limits_with_edges_per_key_column(K, V, B):
    rng = np.random.default_rng(10000 * K + 100 * V + B)
    edges = np.stack([np.sort(rng.uniform(-1.0 - k, 2.0 + k, size=B + 1)) for k in range(K)])      # every column its own, unevenly spaced
    assert (np.diff(edges, axis=1) > 0).all()
    F = 1300                                                                              # two pieces of the second recording
    keys, values = keys_over(rng, F, edges), wide_values(rng, (F, V))
    keys[rng.integers(0, F, size=5), rng.integers(0, K, size=5)] = np.nan
    values[rng.integers(0, F, size=5), rng.integers(0, V, size=5)] = np.nan
    got = check(keys, values, edges, [0, 130], 0, None, (K, V, B))
    assert got.shape == (2, K, B + 3, V, 4)
    if K > 1:                                                                             # the columns' edges differ, and so do their records
        assert not np.array_equal(got[1, 0, :, 0, 0], got[1, K - 1, :, 0, 0])


# ---------------- 3: dtypes, views, sets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kd,vd", [(torch.float32, torch.float32), (torch.float32, torch.float64), (torch.float64, torch.float32),
                                   (torch.float64, torch.float64)])
def test_dtypes_on_each_side(kd, vd):
    rng = np.random.default_rng(7)
    F = 1100
    keys, values = dev(keys_over(rng, F, EDGES), kd), dev(wide_values(rng, (F, 5)), vd)
    from wear_mocap_ape_amd import score
    got = on_device(keys, values, EDGES, [0, 40])
    assert same_record(got, score.stats_by_numpy(keys.cpu().numpy(), values.cpu().numpy(), EDGES, [0, 40]))      # widened exactly


def test_column_slices_and_strided_frames_go_in_without_a_copy():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(8)
    F = 700
    rows = dev(np.concatenate([keys_over(rng, 2 * F, np.tile(EDGES, (5, 1))), wide_values(rng, (2 * F, 15))], axis=1))      # [2F, 25]
    keys, values = rows[:, 2:4], rows[:, 10:17]                                           # column slices of wider rows
    assert score._by_view(keys, "keys")[0].data_ptr() == keys.data_ptr() and score._by_view(values, "values")[0].data_ptr() == values.data_ptr()
    assert not keys.is_contiguous() and score._by_view(keys, "keys")[5] == 25
    got = on_device(keys, values, EDGES, [0, 1100])
    assert same_record(got, score.stats_by_numpy(keys.cpu().numpy(), values.cpu().numpy(), EDGES, [0, 1100]))
    k2, v2 = rows[::2, 2:4], rows[1::2, 10:17]                                            # every second frame: a frame stride of 50
    view = score._by_view(k2, "keys")
    assert view[0].data_ptr() == k2.data_ptr() and view[5] == 50 and score._by_view(v2, "values")[0].data_ptr() == v2.data_ptr()
    got = on_device(k2, v2, EDGES, [0, 300])
    assert same_record(got, score.stats_by_numpy(k2.cpu().numpy(), v2.cpu().numpy(), EDGES, [0, 300]))
    # sets as a view: [C, F, W] slices of [C, F, 25], the set stride that of the wider rows
    sets = dev(np.concatenate([keys_over(rng, 3 * F, np.tile(EDGES, (2, 1))), wide_values(rng, (3 * F, 21))], axis=1)).reshape(3, F, 25)
    ks, vs = sets[:, :, 0:2], sets[:, :, 4:9]
    view = score._by_view(ks, "keys")
    assert view[0].data_ptr() == ks.data_ptr() and view[4] == F * 25 and view[5] == 25
    got = on_device(ks, vs, EDGES, [0, 10])
    assert same_record(got, score.stats_by_numpy(ks.cpu().numpy(), vs.cpu().numpy(), EDGES, [0, 10]))
    # what the rules do not admit is copied, and counted all the same
    kt = rows[:F, 2:4].t().contiguous().t()                                               # the last dimension not contiguous
    assert score._by_view(kt, "keys")[0].data_ptr() != kt.data_ptr()
    assert same_record(on_device(kt, values[:F], EDGES), score.stats_by_numpy(kt.cpu().numpy(), values[:F].cpu().numpy(), EDGES))


@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("shared", ["keys", "values", "neither"])
def test_sets_shared_and_per_set_are_single_set_calls(C_, shared):
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(20 + C_)
    F, starts = 1500, [0, 20, 1100]
    kshape, vshape = ((F,) if shared == "keys" else (C_, F)), ((F,) if shared == "values" else (C_, F))
    keys = np.stack([keys_over(rng, F, EDGES) for _ in range(C_)]) if len(kshape) == 2 else keys_over(rng, F, EDGES)
    values = wide_values(rng, vshape + (6,))
    got = check(keys, values, EDGES, starts, 2, None, (C_, shared))
    assert got.shape == (C_, 3, 2, 7, 6, 4)
    for c in range(C_):                                                                   # each set has the bits of a call on that set alone
        alone = on_device(keys[c] if keys.ndim == 3 else keys, values[c] if values.ndim == 3 else values, EDGES, starts, 2)
        assert alone.shape == (3, 2, 7, 6, 4) and same_record(alone, got[c]), c
    if C_ == 3 and shared != "neither":
        with pytest.raises(UserWarning):
            score.stats_by(dev(np.zeros((2, F, 2))), dev(np.zeros((3, F, 6))), EDGES)


# ---------------- 4: values ----------------------------------------------------------------------------------------------------------------------
def test_nan_inf_zero_and_keys_on_edges():
    rng = np.random.default_rng(9)
    F, B = 1200, 4
    e = EDGES[:1]
    keys = keys_over(rng, F, e)
    values = wide_values(rng, (F, 4))
    keys[10:20, 0] = np.nan                                                               # NaN keys: slot B + 2
    keys[20:25, 0] = e[0]                                                                 # keys exactly on the edges: below, then the right-closed bins
    keys[25:30, 0], keys[30, 0], keys[31, 0] = -0.0, np.inf, -np.inf
    values[12, 0] = values[40, 0] = values[41, 1] = np.nan                                # NaN values: left out of their own cell only
    keys[50:54, 0] = 0.25
    values[50, 2], values[51, 2] = np.inf, np.inf                                         # +inf twice: an inf sum
    values[52, 3], values[53, 3] = np.inf, -np.inf                                        # both: a NaN sum, an inf sum of squares, max +inf
    keys[60:64, 0] = -0.75
    values[60:64, 1] = -0.0                                                               # -0.0 alone in a column's piece would sum to +0.0; here with others
    got = check(keys, values, e, [0], 0, None, "specials")
    assert got[0, 0, B + 2, 1, 0] == 10.0 and got[0, 0, B + 2, 0, 0] == 9.0               # the NaN keys' slot; one of its values is NaN
    assert got[0, 0, B, :, 0].min() >= 2.0                                                # e[0] and -inf lie below
    assert got[0, 0, 1, 0, 0] >= 5.0                                                      # -0.0 == e[2] = 0.0 lies in (e[1], e[2]]
    assert got[0, 0, 2, 2, 1] == np.inf and got[0, 0, 2, 2, 3] == np.inf
    assert np.isnan(got[0, 0, 2, 3, 1]) and got[0, 0, 2, 3, 2] == np.inf and got[0, 0, 2, 3, 3] == np.inf
    # a column of -0.0 only: +0.0 sums, a zero maximum, counted
    z = check(np.full((300, 1), 0.25), np.full((300, 2), -0.0), e, [0])
    assert z[0, 0, 2, 0].tolist()[:1] == [300.0] and not np.signbit(z[0, 0, 2, :, 1:3]).any() and (z[0, 0, 2, :, 3] == 0.0).all()
    # all frames in one slot; frames spread over all slots of 125 bins
    one = check(np.full((2500, 1), 0.6), wide_values(rng, (2500, 3)), e, [0], 0, None, "one slot")
    assert (one[0, 0, 3, :, 0] == 2500.0).all() and not np.delete(one[0, 0], 3, axis=0)[..., 0].any()
    e125 = np.linspace(-1.0, 1.0, 126)[None]
    k = keys_over(rng, 2500, e125)
    k[::100, 0] = np.nan
    spread = check(k, wide_values(rng, (2500, 3)), e125, [0], 0, None, "all slots")
    assert (spread[0, 0, :, 0, 0] > 0).all()                                              # all 128 slots hit


# ---------------- 5: the order is the contract -----------------------------------------------------------------------------------------------------
def test_a_recording_has_the_same_bits_wherever_it_lies():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(11)
    n = 2300
    keys, values = keys_over(rng, n, EDGES), wide_values(rng, (n, 5))
    alone = on_device(keys, values, EDGES, [0])
    assert same_record(alone, score.stats_by_numpy(keys, values, EDGES, [0]))
    again = on_device(keys, values, EDGES, [0])
    assert np.array_equal(alone.view(np.int64), again.view(np.int64))                     # two calls: the same bits, NaN or not
    for offset in (1, 700, 1024 + 333):                                                   # embedded among others at three offsets
        tail = 150
        k2 = np.concatenate([keys_over(rng, offset, EDGES), keys, keys_over(rng, tail, EDGES)])
        v2 = np.concatenate([wide_values(rng, (offset, 5)), values, wide_values(rng, (tail, 5))])
        got = on_device(k2, v2, EDGES, [0, offset, offset + n])
        assert np.array_equal(got[1].view(np.int64), alone[0].view(np.int64)), offset
        # a trim has the bits of a call on the sliced tensors
        cut = on_device(k2, v2, EDGES, [0], 0, [(offset, tail)])
        assert np.array_equal(cut[0].view(np.int64), alone[0].view(np.int64)), offset
        dk, dv = dev(k2), dev(v2)
        sliced = on_device(dk[offset:offset + n], dv[offset:offset + n], EDGES, [0])
        assert np.array_equal(sliced[0].view(np.int64), alone[0].view(np.int64)), offset


def test_merge_and_pool_on_device_records():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(12)
    F, starts = 2600, [0, 1200]
    keys, values = keys_over(rng, F, EDGES), wide_values(rng, (F, 2))
    whole = on_device(keys, values, EDGES, starts)
    ia, ib = np.r_[0:500, 1200:2000], np.r_[500:1200, 2000:2600]
    merged = score.merge_by(on_device(keys[ia], values[ia], EDGES, [0, 500]), on_device(keys[ib], values[ib], EDGES, [0, 700]))
    assert np.array_equal(merged[..., [0, 3]], whole[..., [0, 3]])
    mag = score.stats_by_numpy(keys, np.abs(values), EDGES, starts)
    for j in (1, 2):
        assert (np.abs(merged[..., j] - whole[..., j]) <= whole[..., 0] * 2.0 ** -53 * mag[..., j]).all()
    by = score.stats_by(dev(keys), dev(values), EDGES, starts)
    assert same_bits(score.pool_by(by), score.pool_by(whole)) and score.summarise_by(by, EDGES)["n"].shape == (2, 2, 7, 2)


# ---------------- 6: the refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_and_a_capturing_stream_leave_the_output_untouched():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    bufs = {"keys": dev(np.linspace(-1.0, 3.0, 40).reshape(2, 10, 2)), "values": dev(np.arange(60.0).reshape(2, 10, 3)),
            "by": torch.full((2, 3, 2, 7, 3, 4), -7.0, dtype=torch.float64, device="cuda")}
    ptrs = {k: C.c_void_p(t.data_ptr()) for k, t in bufs.items()}
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kw, what in refusals():
        if any(isinstance(kw.get(name), int) for name in ("keys", "values", "by")):
            continue                                        # (the cases with made-up addresses: the host-only test's)
        rc = call_entry(ptrs, stream=stream, **kw)
        assert rc == 1 and what in lib.ape_last_error(), (kw, rc, lib.ape_last_error())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros((4,), device="cuda")
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            rc, msg = call_entry(ptrs, stream=C.c_void_p(side.cuda_stream)), lib.ape_last_error()
    torch.cuda.current_stream().wait_stream(side)
    assert rc == 1 and b"capturing" in msg and b"score_by" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert (bufs["by"] == -7.0).all()                       # nothing was written
    assert call_entry(ptrs, stream=stream) == 0             # the same arguments, accepted: one set
    torch.cuda.synchronize()
    assert float(bufs["by"][0, :, 0, :, 0, 0].sum()) == 10.0 and bool((bufs["by"][1] == -7.0).all())
    assert call_entry(ptrs, stream=stream, n_sets=2, kss=20, vss=0) == 0      # keys per set, the values shared
    torch.cuda.synchronize()
    assert float(bufs["by"][1, :, 1, :, 2, 0].sum()) == 10.0


# ---------------- 7: the estimators' one-line method -------------------------------------------------------------------------------------------------
def _check_errors_by(est_obj, skip, layout, golden, with_spread):
    from tests.test_frame_fit_cpu import msgs_from_est
    from tests.test_score_hist_gpu import spread_records
    from wear_mocap_ape_amd import score
    g = golden(f"fk_layout{layout}.npz")
    rng = np.random.default_rng(17 + layout)
    F, starts = 240, [0, 80, 160]
    m = msgs_from_est(g["est_bo_N300"][60 + rng.permutation(240)[:F]], layout)
    out, truth = dev(m), dev(g["est_bd_N300"][60:60 + F])
    rec = dev(spread_records(rng, m)) if with_spread else None
    for rec_lags in (None, [2, -1, 0]):
        if rec_lags is None:
            rows, _ = est_obj.score_recording(out, truth, rec, starts, truth_kind="est")
        else:
            rows = est_obj.score_recording(out, truth, rec, starts, truth_kind="est", lags=(0, 0), rec_lags=rec_lags)[0][:, 0]
        trim = score.lag_trim(starts, F, (0, 0), skip, rec_lags)
        o = [0, 0, 0] if rec_lags is None else rec_lags
        want = [80 - max(skip, v, 0) - max(0, -v) for v in o]
        parts = {"angles": (lambda: est_obj.angles_recording(out, None, starts, truth_kind="est", per_frame=True)[0], score.angle_edges(36)[:7],
                            score.ANGLE_NAMES),
                 "motion": (lambda: est_obj.motion_recording(out, starts, per_frame=True)[0], score.default_edges("motion", 36), score.MOTION_NAMES)}
        if rec_lags is None:
            parts["truth_angles"] = (lambda: est_obj.truth_angles(truth, "est", starts, per_frame=True)[0], score.angle_edges(36)[:7],
                                     score.ANGLE_NAMES)
        if with_spread:
            parts["spread"] = (lambda: score.spread_sigma(rec), score.default_edges("score", 36)[:5], score.SIGMA_NAMES)
        for by, (keys_of, edges_of, names_of) in parts.items():
            got, edges, names = est_obj.errors_by(out, truth, by, rec, starts, truth_kind="est", rec_lags=rec_lags)
            keys = keys_of()
            hand = score.stats_by(keys, rows, edges_of, starts, 0, trim)
            torch.cuda.synchronize()
            K = int(keys.shape[1])
            assert tuple(got.shape) == (3, K, 39, 7, 4) and np.array_equal(edges, edges_of) and tuple(names) == tuple(names_of) and len(names) == K
            assert torch.equal(got.view(torch.int64), hand.view(torch.int64)), by       # the parts it is documented to compose
            h = got.cpu().numpy()
            assert same_record(h, score.stats_by_numpy(keys.cpu().numpy(), rows.cpu().numpy(), edges, starts, 0, trim)), by
            nan_rows = np.isnan(rows.cpu().numpy()[:, 0])
            ends = starts[1:] + [F]
            left = [int(nan_rows[s + t0:e - t1].sum()) for s, e, (t0, t1) in zip(starts, ends, trim.tolist())]
            assert h[:, :, :, 0, 0].sum(axis=2).tolist() == [[float(n - k)] * K for n, k in zip(want, left)] and min(want) > 0, by
            s = score.summarise_by(score.pool_by(got), edges, names, score.SCORE_HIST_NAMES)
            assert s["rms"].shape == (K, 39, 7) and np.isfinite(s["rms"][0, :, 0][s["n"][0, :, 0] > 0]).all()
        if rec_lags is not None:
            with pytest.raises(UserWarning):
                est_obj.errors_by(out, truth, "truth_angles", rec, starts, truth_kind="est", rec_lags=rec_lags)
    # keys of one's own, edges and bins, an explicit skip
    own = dev(np.stack([np.linspace(0.0, 1.0, F), np.cos(np.arange(F))], axis=1))
    e9 = np.stack([np.linspace(0.0, 1.0, 10), np.linspace(-1.0, 1.0, 10)])
    got, edges, names = est_obj.errors_by(out, truth, own, rec, starts, skip=1, truth_kind="est", edges=e9)
    assert tuple(got.shape) == (3, 2, 12, 7, 4) and np.array_equal(edges, e9) and names == ("key0", "key1")
    rows, _ = est_obj.score_recording(out, truth, rec, starts, 1, truth_kind="est")
    assert torch.equal(got.view(torch.int64), score.stats_by(own, rows, e9, starts, 1).view(torch.int64))
    assert tuple(est_obj.errors_by(out, truth, "angles", rec, starts, truth_kind="est", bins=8)[0].shape) == (3, 7, 11, 7, 4)
    for bad in (lambda: est_obj.errors_by(out, truth, own, rec, starts, truth_kind="est"),
                lambda: est_obj.errors_by(out, truth, "speed", rec, starts, truth_kind="est")):
        with pytest.raises(UserWarning):
            bad()
    if not with_spread:
        with pytest.raises(UserWarning):
            est_obj.errors_by(out, truth, "spread", None, starts, truth_kind="est")


def test_errors_by_pocket_nn(golden, tmp_path, monkeypatch):
    from tests.test_replay import _estimator
    est_obj = _estimator(tmp_path, monkeypatch, "pocket", 1, 0.2, smooth=1)
    assert est_obj.sequence_len == 6
    _check_errors_by(est_obj, est_obj.sequence_len - 1, HIPS, golden, True)


def test_errors_by_fk_only(golden):
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    _check_errors_by(WatchPhoneUarm(smooth=5), 0, WATCH, golden, False)


def test_errors_by_kalman(golden):
    from oracle import kalman_oracle as ko
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    W = 4
    sd = ko.make_state_dict(W, 36)
    est_obj = WatchPhonePocketKalman({k: torch.from_numpy(v) for k, v in sd.items()}, smooth=2, num_ensemble=16, window_size=W)
    _check_errors_by(est_obj, W + 1, HIPS, golden, True)
