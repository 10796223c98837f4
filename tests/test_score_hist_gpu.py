"""Error distributions per recording (`ape_score_hist`) on the GPU.

Reference of every count: `score.hist_numpy` (searchsorted + bincount) on the same inputs, with exact integer equality throughout -- there
is no tolerance in this file.  The kernel's tile is 256 frames, one lane per frame, four waves; a row of more than 8 columns is split
into two chunks; a tile that holds frames of more than 4 recordings adds to the output directly instead of through the LDS histogram;
neighbouring lanes of a wave with the same recording and slot are added as one run.  The shapes below sit on each of those borders."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HIPS, WATCH = 0, 1


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def on_device(values, edges, starts=None, skip=0, trim=None):
    from wear_mocap_ape_amd import score
    h = score.hist_rows(values if isinstance(values, torch.Tensor) else dev(values), edges, starts, skip, trim)
    torch.cuda.synchronize()
    assert h.dtype == torch.int64
    return h.cpu().numpy()


def check(values, edges, starts=None, skip=0, trim=None, what=""):
    """the device's counts of `values` (numpy) are the host statement's; -> the counts"""
    from wear_mocap_ape_amd import score
    got = on_device(values, edges, starts, skip, trim)
    ref = score.hist_numpy(values, edges, starts, skip, trim)
    assert got.shape == ref.shape and np.array_equal(got, ref), (what, np.argwhere(got != ref)[:5])
    return got


def spread_values(rng, F, W, e):
    """values over and beyond the edges e [B + 1], every slot hit"""
    return rng.uniform(e[0] - 0.1 * (e[-1] - e[0]), e[-1] + 0.1 * (e[-1] - e[0]), size=(F, W))


EDGES = np.linspace(-1.0, 1.0, 9)


# ---------------- 1: the smallest shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,starts,trim", [
    (1, [0], None),
    (257, [0], None),                                                                     # one more than a tile
    (70, list(range(70)), None),                                                          # 70 one-frame recordings: across a wave boundary, added directly
    (200, [0, 37], None),                                                                 # a recording boundary in the middle of a wave
    (600, [0], None),                                                                     # one recording across three tiles
    (300, [0, 50, 100, 150], None),                                                       # 4 recordings in a tile: the LDS route's most
    (300, [0, 50, 100, 150, 200], None),                                                  # 5: added directly; the second tile goes through LDS
    (700, [0] + list(range(200, 270)), None),                                             # a long recording and 70 short ones share a tile
    (520, [0, 255, 256, 257, 512], None),                                                 # recordings that begin on, before and after a tile's border
    (300, [0, 100, 200], [(100, 0), (30, 71), (0, 100)]),                                 # trims that empty a window, invert one, and empty at the tail
    (300, [0, 100, 200], [(3, 5), (0, 0), (99, 0)]),
])
def test_shapes_at_the_borders(F, starts, trim):
    rng = np.random.default_rng(F + len(starts))
    got = check(spread_values(rng, F, 3, EDGES), EDGES, starts, 0, trim, (F, starts[:6]))
    ends = starts[1:] + [F]
    tr = trim if trim is not None else [(0, 0)] * len(starts)
    want = [max(0, (e - b) - (s + a)) for s, e, (a, b) in zip(starts, ends, tr)]
    assert np.array_equal(got.sum(axis=2), np.tile(np.array(want)[:, None], (1, 3)))    # every frame of a window in exactly one slot
    if trim is not None and trim[0] == (100, 0):
        assert not got.any()                                                              # empty and inverted windows: exact zeros


def test_skip_is_added_to_the_head_trim():
    rng = np.random.default_rng(1)
    v = spread_values(rng, 300, 2, EDGES)
    a = check(v, EDGES, [0, 100], 7, [(1, 2), (0, 4)])
    assert np.array_equal(a, on_device(v, EDGES, [0, 100], 0, [(8, 2), (7, 4)])) and a.sum(axis=2).tolist() == [[90, 90], [189, 189]]


# ---------------- 2: widths, bins, values ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 7, 8, 9, 12, 16])                                       # one chunk; 8: a full one; 9: 5 + 4; 12: 6 + 6; 16: 8 + 8
@pytest.mark.parametrize("B", [1, 64, 256])
def test_widths_and_bins_with_edges_per_column(W, B):
    rng = np.random.default_rng(100 * W + B)
    edges = np.stack([np.sort(rng.uniform(-1.0 - w, 2.0 + w, size=B + 1)) for w in range(W)])      # every column its own, unevenly spaced
    assert (np.diff(edges, axis=1) > 0).all()
    F = 300
    v = np.stack([rng.uniform(edges[w, 0] - 0.2, edges[w, -1] + 0.2, size=F) for w in range(W)], axis=1)
    v[rng.integers(0, F, size=5), rng.integers(0, W, size=5)] = np.nan
    got = check(v, edges, [0, 1, 258], 0, None, (W, B))
    assert got.shape == (3, W, B + 3)
    if W > 1:                                                                             # the columns' edges differ, and so do their counts
        assert not np.array_equal(got[2, 0], got[2, W - 1])


def slot_by_hand(v, e):
    """the header's table, one comparison at a time"""
    B = len(e) - 1
    if v != v:
        return B + 2
    if v <= e[0]:
        return B
    if v > e[B]:
        return B + 1
    return next(b for b in range(B) if e[b] < v <= e[b + 1])


def edge_case_values(e, rng, n):
    """exact edges, the values next to them, +-inf, NaN, -0.0, subnormals, a widened float32: planted at known frames, the first ones"""
    third = float(np.float32(1.0) / np.float32(3.0))
    special = list(e) + [np.nextafter(x, np.inf) for x in e] + [np.nextafter(x, -np.inf) for x in e] + \
        [np.inf, -np.inf, np.nan, -0.0, 0.0, 5e-324, -5e-324, third, 1e308, -1e308]
    v = rng.uniform(e[0] - 0.5, e[-1] + 0.5, size=n)
    v[:len(special)] = special
    return v, len(special)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_edge_case_values_in_both_dtypes(dtype):
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(2)
    third = float(np.float32(1.0) / np.float32(3.0))
    edges = np.stack([np.array([0.0, 0.25, third, 0.5, 1.0, 2.0]), np.array([-1.0, -0.5, 0.0, 1e-300, 0.75, 3.0]),
                      np.array([-2.0, -1.0, -0.0, 0.5, 0.625, 0.75])])
    cols = [edge_case_values(edges[w], rng, 300) for w in range(3)]
    v = np.stack([c[0] for c in cols], axis=1)
    if dtype == torch.float32:
        with np.errstate(over="ignore"):                                                  # (1e308 becomes inf, 1e-300 and the subnormals 0: the reference sees the same float32)
            v = v.astype(np.float32)
    got = check(v, edges, [0, 290], 0, None, dtype)
    # the planted frames, one by one, against the header's table
    n = cols[0][1]
    one = on_device(v[:n], edges, list(range(n)))                                         # a recording per frame: the slot of every planted value
    for f in range(n):
        for w in range(3):
            assert one[f, w].sum() == 1 and one[f, w, slot_by_hand(float(v[f, w]), edges[w])] == 1, (f, w, v[f, w])
    assert got[:, :, -1].sum() == 3 and score.hist_numpy(v, edges)[0, 0, 1] >= 2         # NaN once per column; the widened float32 sits on its edge


def test_a_column_sliced_row_strided_view_goes_in_without_a_copy():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(3)
    wide = rng.normal(scale=0.7, size=(400, 11))
    for dtype in (torch.float64, torch.float32):
        t = dev(wide, dtype)
        ref_in = t.cpu().numpy()
        view = t[:, 2:7]                                                                  # columns 2 .. 6 of rows 11 apart
        assert not view.is_contiguous() and score._hist_view(view)[0].data_ptr() == view.data_ptr()
        got = on_device(view, EDGES, [0, 130])
        assert np.array_equal(got, score.hist_numpy(ref_in[:, 2:7], EDGES, [0, 130]))
        every_other = t[::2, 1:4]                                                         # rows 22 apart
        assert score._hist_view(every_other)[6] == 22
        assert np.array_equal(on_device(every_other, EDGES, [0, 99]), score.hist_numpy(ref_in[::2, 1:4], EDGES, [0, 99]))
        turned = t.t()[:, :5]                                                             # the last dimension is not contiguous: copied
        assert turned.stride(1) != 1 and np.array_equal(on_device(turned, EDGES), score.hist_numpy(ref_in.T[:, :5], EDGES))


def test_maximum_contention_all_frames_in_one_bin():
    F = 5000
    v = np.full((F, 7), 0.3)
    got = check(v, EDGES, [0, 4000])
    b = 5                                                                                 # (0.25, 0.5]
    assert got[:, :, b].tolist() == [[4000] * 7, [1000] * 7] and got.sum() == 7 * F
    nan = check(np.full((F, 2), np.nan), EDGES)
    assert nan[0, :, -1].tolist() == [F, F] and nan.sum() == 2 * F


def test_runs_of_equal_neighbours_are_counted_whole():
    """runs of equal values of every length from 1 to beyond two waves, begun and ended anywhere in a wave, cut by recording boundaries,
    by the windows' ends and by NaN: a run is added once, with its length"""
    rng = np.random.default_rng(8)
    F = 1500
    cols = []
    for w in range(3):
        lengths = rng.integers(1, (4, 40, 140)[w], size=F)
        vals = rng.uniform(-1.2, 1.2, size=F)
        vals[rng.integers(0, F, size=F // 10)] = np.nan
        cols.append(np.repeat(vals, lengths)[:F])
    v = np.stack(cols, axis=1)
    starts, trim = [0, 333, 334, 900], [(5, 3), (0, 0), (0, 0), (64, 1)]
    got = check(v, EDGES, starts, 0, trim)
    assert got[:, :, -1].sum() > 100 and got.sum() == 3 * (1500 - 5 - 3 - 64 - 1)
    check(v, EDGES, list(range(0, F, 7)), 1)                                              # the same runs where every tile adds to the output directly
    check(v.astype(np.float32), EDGES, [0, 700], 0, [(0, 0), (100, 701)])


# ---------------- 3: sets and groups, the whole output, determinism ----------------------------------------------------------------------------------
def test_sets_and_groups_are_slices_of_single_calls():
    rng = np.random.default_rng(4)
    Cn, F, G, W = 2, 530, 3, 7
    v = spread_values(rng, Cn * F * G, W, EDGES).reshape(Cn, F, G, W)
    t = dev(v)
    starts, trim = [0, 3, 300], [(0, 0), (1, 0), (2, 9)]
    got = check(v, EDGES, starts, 0, trim)
    assert got.shape == (Cn, 3, G, W, 11)
    for c in range(Cn):
        for g in range(G):
            assert np.array_equal(got[c, :, g], on_device(t[c, :, g], EDGES, starts, 0, trim)), (c, g)      # [F, W] views, rows G * W apart
    assert np.array_equal(got[1], on_device(t[1], EDGES, starts, 0, trim))                # [F, G, W]
    # motion rows [C, F, 12] as [C, F, 1, 12]; and a group-major view [F, G, W] of [G, F, W] storage
    m = spread_values(rng, 3 * F, 12, EDGES).reshape(3, F, 12)
    assert np.array_equal(on_device(dev(m)[:, :, None], EDGES, starts)[:, :, 0], np.stack([check(m[c], EDGES, starts) for c in range(3)]))
    gm = dev(np.ascontiguousarray(v[0].transpose(1, 0, 2))).permute(1, 0, 2)
    assert not gm.is_contiguous() and np.array_equal(on_device(gm, EDGES, starts, 0, trim), got[0])


def direct_call(values, edges, starts, trim, hist, stream=None):
    from wear_mocap_ape_amd import _hip
    F, W = values.shape
    st = np.ascontiguousarray(starts, dtype=np.int32)
    tr = None if trim is None else np.ascontiguousarray(trim, dtype=np.int32)
    e = np.ascontiguousarray(np.broadcast_to(edges, (W, edges.shape[-1])), dtype=np.float64)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    return _hip.lib().ape_score_hist(C.c_void_p(values.data_ptr()), _hip.F64, W, 1, 0, F, int(values.stride(0)), 1, 0, C.c_void_p(st.ctypes.data),
                                     len(st), None if tr is None else C.c_void_p(tr.ctypes.data), C.c_void_p(e.ctypes.data), e.shape[1] - 1,
                                     C.c_void_p(hist.data_ptr()), stream)


def test_the_whole_output_is_written_and_two_calls_give_equal_bits():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(5)
    F, W = 1000, 7
    v = spread_values(rng, F, W, EDGES)
    t = dev(v)
    starts, trim = [0, 10, 11, 600], [(0, 0), (1, 0), (0, 0), (500, 0)]                   # an empty window and an inverted one among them
    ref = score.hist_numpy(v, EDGES, starts, 0, trim)
    a = torch.full((4, W, 11), -1, dtype=torch.int64, device="cuda")
    b = torch.full((4, W, 11), 2 ** 40 + 5, dtype=torch.int64, device="cuda")
    assert direct_call(t, EDGES, starts, trim, a) == 0 and direct_call(t, EDGES, starts, trim, b) == 0
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), ref) and torch.equal(a, b) and not ref[1].any() and not ref[3].any()
    # and on the many-recordings route
    many = list(range(0, F, 3))
    c = torch.full((len(many), W, 11), -1, dtype=torch.int64, device="cuda")
    assert direct_call(t, EDGES, many, None, c) == 0
    torch.cuda.synchronize()
    assert np.array_equal(c.cpu().numpy(), score.hist_numpy(v, EDGES, many)) and np.array_equal(on_device(t, EDGES, many), c.cpu().numpy())


# ---------------- 4: the tie to the scorers --------------------------------------------------------------------------------------------------------
def msgs_from_est(est, layout):
    """one message per est row stating that row's pose (compose_msg.py:72-78 columns)"""
    qc = (6, 10) if layout == WATCH else (9, 13, 17)
    m = np.zeros((est.shape[0], 25))
    m[:, 21] = 1.0
    m[:, 4:7], m[:, 11:14] = est[:, 0:3], est[:, 3:6]
    if layout != WATCH:
        m[:, 18:21] = est[:, 6:9]
    for k, c in enumerate(qc):
        m[:, 7 + 7 * k:11 + 7 * k] = est[:, c:c + 4]
    m[:, 0:4] = m[:, 7:11]
    return m


def spread_records(rng, msg, scale=0.05):
    """records whose means sit near the message's origins, with covariances A A' / 8 + a ridge (well conditioned)"""
    F = msg.shape[0]
    rec = np.zeros((F, 21))
    for o, c in ((0, 4), (9, 11)):
        rec[:, o:o + 3] = msg[:, c:c + 3] + scale * rng.normal(size=(F, 3))
        A = scale * 4 * rng.normal(size=(F, 3, 8))
        S = A @ A.transpose(0, 2, 1) / 8 + (0.1 * scale) ** 2 * np.eye(3)
        rec[:, o + 3:o + 9] = S[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    rec[:, 18:21] = 0.01
    return rec


@pytest.fixture(scope="module")
def planted(golden):
    """a pocket case of 300 frames in 3 recordings: messages from permuted est rows against est truth, with spread records; a truth row
    that cannot be scored and a few covariances that cannot be used"""
    g = golden("fk_layout0.npz")
    rng = np.random.default_rng(6)
    msg = msgs_from_est(g["est_bo_N300"][rng.permutation(300)], HIPS)
    truth = g["est_bd_N300"].copy()
    truth[[120, 280]] = np.nan
    rec = spread_records(rng, msg)
    rec[[10, 11, 200], 3:9] = 0.0                                                          # hand covariances without a usable inverse
    rec[[90], 12:18] = 0.0
    return dev(msg), dev(truth), dev(rec), [0, 40, 170]


def pit_edges_for_rows():
    from wear_mocap_ape_amd import score
    return np.stack([np.exp(np.linspace(np.log(1e-3), np.log(8.0), 10))] * 5 + [score.pit_edges(10)] * 2)


def check_tie(h, acc, what):
    """h [R, 7, 12] against acc [R, 25]: integers, exactly"""
    from wear_mocap_ape_amd import score
    B = 9
    assert np.array_equal(h[:, 0, :B + 2].sum(axis=1), acc[:, 15]) and np.array_equal(h[:, 0, B + 2], acc[:, 16]), what
    for k in (0, 1):
        p = score.pit(h[:, 5 + k])
        assert np.array_equal(p["n"], acc[:, 17 + 4 * k]), (what, k)
        assert np.array_equal(p["cumulative"][:, 4], acc[:, 19 + 4 * k]) and np.array_equal(p["cumulative"][:, 8], acc[:, 20 + 4 * k]), (what, k)
    assert (h.sum(axis=2) == (acc[:, 15] + acc[:, 16])[:, None]).all(), what


def test_counts_tie_to_score_rows_accumulators(planted):
    from wear_mocap_ape_amd import score
    msg, truth, rec, starts = planted
    edges = pit_edges_for_rows()
    for skip in (0, 6):
        rows, acc = score.score_rows(HIPS, msg, truth, "est", rec, starts, skip)
        h = on_device(rows, edges, starts, skip)
        acc = acc.cpu().numpy()
        assert h.shape == (3, 7, 12) and acc[:, 16].sum() == 2 and acc[0, 17] == acc[0, 15] - 2 and 0 < acc[:, 19].sum() < acc[:, 20].sum()
        check_tie(h, acc, skip)
        assert np.array_equal(h, score.hist_numpy(rows.cpu().numpy(), edges, starts, skip))


def test_counts_tie_to_score_lags_accumulators_at_every_lag(planted):
    from wear_mocap_ape_amd import score
    msg, truth, rec, starts = planted
    edges = pit_edges_for_rows()
    for rec_lags, skip in ((None, 0), ([1, -2, 0], 3)):
        rows, acc = score.score_lags(HIPS, msg, truth, (-2, 2), "est", rec, starts, skip, None, rec_lags, per_frame=True)
        trim = score.lag_trim(starts, 300, (-2, 2), skip, rec_lags)
        h = on_device(rows, edges, starts, 0, trim)
        acc = acc.cpu().numpy()
        assert h.shape == (3, 5, 7, 12) and (acc[:, :, 15] + acc[:, :, 16] > 30).all()
        for j in range(5):
            check_tie(h[:, j], acc[:, j], (rec_lags, j))
        assert np.array_equal(h, score.hist_numpy(rows.cpu().numpy(), edges, starts, 0, trim))


# ---------------- 5: the estimators' one-line method -------------------------------------------------------------------------------------------------
def _by_hand(est_obj, skip, out, truth, rec, starts, rec_lags, edges):
    from wear_mocap_ape_amd import score
    if rec_lags is None:
        rows, acc = est_obj.score_recording(out, truth, rec, starts, truth_kind="est")
    else:
        rows, acc = est_obj.score_recording(out, truth, rec, starts, truth_kind="est", lags=(0, 0), rec_lags=rec_lags)
        rows, acc = rows[:, 0], acc[:, 0]
    trim = score.lag_trim(starts, int(rows.shape[0]), (0, 0), skip, rec_lags)
    return score.hist_rows(rows, edges, starts, 0, trim), acc


def _check_error_distribution(est_obj, skip, layout, golden, with_spread):
    from wear_mocap_ape_amd import score
    g = golden(f"fk_layout{layout}.npz")
    rng = np.random.default_rng(7 + layout)
    F, starts = 90, [0, 30, 60]
    m = msgs_from_est(g["est_bo_N300"][60 + rng.permutation(240)[:F]], layout)
    out, truth = dev(m), dev(g["est_bd_N300"][60:60 + F])
    rec = dev(spread_records(rng, m)) if with_spread else None
    for rec_lags in (None, [2, -1, 0]):
        hist, edges, acc = est_obj.error_distribution(out, truth, rec, starts, truth_kind="est", rec_lags=rec_lags)
        h2, a2 = _by_hand(est_obj, skip, out, truth, rec, starts, rec_lags, score.default_edges("score", 64))
        torch.cuda.synchronize()
        assert tuple(hist.shape) == (3, 7, 67) and np.array_equal(edges, score.default_edges("score", 64))
        assert torch.equal(hist, h2) and torch.equal(acc, a2)
        o = [0, 0, 0] if rec_lags is None else rec_lags
        want = [30 - max(skip, v, 0) - max(0, -v) for v in o]
        assert hist.sum(dim=2).cpu().tolist() == [[n] * 7 for n in want] and min(want) > 0
        s = score.summarise_hist(hist, edges)
        assert [d["window"] for d in s] == want and all(np.isfinite(d["median"]["hand_pos"]) for d in s)
    # given edges and bins, and an explicit skip
    e9 = pit_edges_for_rows()
    hist, edges, acc = est_obj.error_distribution(out, truth, rec, starts, skip=1, truth_kind="est", edges=e9)
    assert np.array_equal(edges, e9) and hist.sum(dim=2).cpu().tolist() == [[29] * 7] * 3
    check_tie(hist.cpu().numpy(), acc.cpu().numpy(), "given edges")
    assert tuple(est_obj.error_distribution(out, truth, rec, starts, truth_kind="est", bins=32)[0].shape) == (3, 7, 35)


def test_error_distribution_pocket_nn(golden, tmp_path, monkeypatch):
    from tests.test_replay import _estimator
    est_obj = _estimator(tmp_path, monkeypatch, "pocket", 1, 0.2, smooth=1)
    assert est_obj.sequence_len > 1
    _check_error_distribution(est_obj, est_obj.sequence_len - 1, HIPS, golden, True)


def test_error_distribution_fk_only(golden):
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    _check_error_distribution(WatchPhoneUarm(smooth=5), 0, WATCH, golden, False)


def test_error_distribution_kalman(golden):
    from oracle import kalman_oracle as ko
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    W = 4
    sd = ko.make_state_dict(W, 36)
    est_obj = WatchPhonePocketKalman({k: torch.from_numpy(v) for k, v in sd.items()}, smooth=2, num_ensemble=16, window_size=W)
    _check_error_distribution(est_obj, W + 1, HIPS, golden, True)


# ---------------- 6: a capturing stream ---------------------------------------------------------------------------------------------------------------
def test_a_capturing_stream_is_refused():
    """the entry stages host arrays per call: on a stream that is capturing a graph it returns APE_ERR_INVALID_ARG and writes nothing"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    n = 64
    v = dev(np.full((n, 2), 0.3))
    hist = torch.full((1, 2, 11), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros((4,), device="cuda")
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            rc, err = direct_call(v, EDGES, [0], None, hist, C.c_void_p(side.cuda_stream)), lib.ape_last_error()
    torch.cuda.current_stream().wait_stream(side)
    assert rc == 1 and b"capturing" in err and b"score_hist" in err, (rc, err)
    torch.cuda.synchronize()
    assert (hist == -7).all()                                                             # nothing was written
    assert direct_call(v, EDGES, [0], None, hist) == 0                                    # the same arguments on a stream that is not capturing
    torch.cuda.synchronize()
    assert hist[0, :, 5].tolist() == [n, n] and int(hist.sum()) == 2 * n
