"""Reaches and holds on the device: ape_segment_frames and ape_segment_runs are held to their numpy statements integer
for integer, ape_segment_stats to its statement bit for bit (the order of summation is part of the contract), over tile edges, recording
starts next to them, the longest minimum lengths and segments longer than a piece.  The planted reach-and-hold trajectory of
tests/test_post_select_cpu.py goes through Estimator.segment_recording and gives tests/golden/segments_planted.npz."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests.test_post_select_cpu import HIPS, reach_and_hold
from tests.test_segments_cpu import EST_RULE, FIXTURE, PILOT, TRUTH_RULE

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2500)
EDGES = (63, 64, 65, 255, 256, 257, 1024, 1025)             # recording starts next to wave, workgroup and tile edges


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def starts_of(F):
    return [0] + [s for s in EDGES if s < F]


def slow_keys(rng, S, F, nan=0.1):
    """keys around the thresholds 0.25 / 0.5 that change slowly (runs of every length), with NaN, infinities and the thresholds themselves"""
    k = 0.375 + 0.3 * np.sin(np.cumsum(rng.normal(size=(S, F)), axis=1) * 0.3) + 0.04 * rng.normal(size=(S, F))
    hit = rng.random((S, F)) < nan
    k[hit] = rng.choice(np.array([np.nan, np.nan, np.inf, -np.inf, 0.25, 0.5]), size=int(hit.sum()))
    return k


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want):
    """float64 arrays equal bit for bit; a NaN (inf - inf) equals any NaN: its sign is the adder's own"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


# ---------------- 1. labels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", SIZES)
def test_labels_equal_the_statement(F):
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(4500 + F)
    st = starts_of(F)
    keys = slow_keys(rng, 3, F)
    th3, mn3 = [(0.25, 0.5), (0.375, 0.375), (0.25, 0.5)], [(1, 1), (3, 5), (9, 4)]
    # float64 contiguous, a rule per set and one rule for all, both first labels
    for th, mn, first in ((th3, mn3, 0), (th3[0], mn3[2], 1), (th3[1], (1, 1), 1)):
        got = score.segment_frames(dev(keys), th, mn, st, first)
        assert got.dtype == torch.uint8 and got.shape == (3, F)
        assert np.array_equal(got.cpu().numpy(), score.segment_frames_numpy(keys, th, mn, st, first)), (F, th, mn, first)
    # column 0 of [3, F, 12] float32 rows, as motion rows go in: no copy is made
    rows = rng.normal(size=(3, F, 12)).astype(np.float32)
    rows[:, :, 0] = keys.astype(np.float32)
    rd = dev(rows)
    got = score.segment_frames(rd[:, :, 0], th3, mn3, st)
    assert np.array_equal(got.cpu().numpy(), score.segment_frames_numpy(rows[:, :, 0], th3, mn3, st))
    one = score.segment_frames(rd[1, :, 0], th3[1], mn3[1], st)
    assert one.shape == (F,) and torch.equal(one, got[1])


def test_an_undecided_run_across_tile_edges_and_an_all_nan_set():
    from wear_mocap_ape_amd import score
    F = 2500
    keys = np.full((4, F), 0.3)                             # between the thresholds: undecided
    keys[0, 1000], keys[0, 2400] = 0.9, 0.1                 # a move decided at 1000 holds over the tile edge 1024 ... until a recording starts
    keys[1, 900], keys[1, 2300] = 0.9, 0.1                  # ... and through the whole of tile 1 into tile 2
    keys[2] = np.nan                                        # nothing decides anywhere
    keys[3, 5], keys[3, 1023], keys[3, 1024], keys[3, 2047], keys[3, 2048] = 0.9, 0.1, np.nan, 0.9, np.inf
    for st, first in (([0, 1030], 0), ([0, 1030], 1), ([0], 0), ([0, 1024, 2048], 1), ([0, 1023, 1025, 2047, 2049], 0)):
        got = score.segment_frames(dev(keys), (0.25, 0.5), (1, 1), st, first).cpu().numpy()
        assert np.array_equal(got, score.segment_frames_numpy(keys, (0.25, 0.5), (1, 1), st, first)), (st, first)
        if st == [0, 1030]:
            assert got[0, 999] == first and got[0, 1000:1030].all() and (got[0, 1030:2400] == first).all() and not got[0, 2400:].any()
            assert (got[2] == first).all()
        if st == [0]:
            assert got[1, 900:2300].all() and not got[1, :900].any() and not got[1, 2300:].any()


def blocks(rng, F, lengths):
    """keys 0 / 1 in runs whose lengths are drawn from `lengths`"""
    out, f, v = np.zeros(F), 0, int(rng.integers(0, 2))
    while f < F:
        n = int(rng.choice(lengths))
        out[f:f + n] = v
        f, v = f + n, 1 - v
    return out


def test_runs_of_min_and_min_less_one_on_a_tile_edge():
    from wear_mocap_ape_amd import score
    F, mh, mm = 2500, 5, 6
    keys = np.zeros((4, F))
    keys[0, 1000:1022], keys[0, 1026:1100] = 1, 1           # a hold of 4 = min_hold - 1 over the edge 1024: filled
    keys[1, 1000:1022], keys[1, 1027:1100] = 1, 1           # a hold of 5 = min_hold: stays
    keys[2, 2045:2050], keys[2, 1021:1027] = 1, 1           # a move of 5 = min_move - 1 over the edge 2048: dropped; one of 6 over 1024: stays
    keys[3, 1020:1023], keys[3, 1025:1027] = 1, 1           # moves of 3 and 2 around a hold of 2: filled to 7, which stays
    got = score.segment_frames(dev(keys), (0.5, 0.5), (mh, mm)).cpu().numpy()
    assert np.array_equal(got, score.segment_frames_numpy(keys, (0.5, 0.5), (mh, mm)))
    assert got[0, 1000:1100].all() and not got[1, 1022:1027].any() and got[1, 1027]
    assert not got[2, 2040:2055].any() and got[2, 1021:1027].all() and got[2].sum() == 6
    assert got[3, 1020:1027].all() and got[3].sum() == 7
    # the same runs with a recording starting inside them: nothing is filled across it, and both halves are judged alone
    for st in ([0, 1024], [0, 1023, 2048], [0, 1025, 2047]):
        got = score.segment_frames(dev(keys), (0.5, 0.5), (mh, mm), st).cpu().numpy()
        assert np.array_equal(got, score.segment_frames_numpy(keys, (0.5, 0.5), (mh, mm), st)), st
    # every length around the minimum, everywhere
    rng = np.random.default_rng(451)
    keys = np.stack([blocks(rng, F, [1, 2, 3, 4, 5, 6, 7, 30]) for _ in range(3)])
    st = starts_of(F)
    got = score.segment_frames(dev(keys), (0.5, 0.5), [(5, 6), (6, 5), (2, 7)], st, 1).cpu().numpy()
    assert np.array_equal(got, score.segment_frames_numpy(keys, (0.5, 0.5), [(5, 6), (6, 5), (2, 7)], st, 1))


def test_the_longest_minimum_lengths():
    """min_hold = min_move = 256: what a frame becomes hangs on frames up to 510 away, half a neighbouring tile's worth"""
    from wear_mocap_ape_amd import score
    F = 2500
    rng = np.random.default_rng(452)
    keys = np.stack([blocks(rng, F, [254, 255, 256, 257, 1, 3]), blocks(rng, F, [255, 256, 100, 511, 2]), blocks(rng, F, [600, 255, 256, 7])])
    keys[0, 1024 - 128:1024 + 127] = 0                      # a hold of 255 centred on the edge between two long moves
    keys[0, 1024 - 400:1024 - 128], keys[0, 1024 + 127:1024 + 400] = 1, 1
    for st in ([0], [0, 1024], starts_of(F)):
        for mn in ((256, 256), [(256, 1), (1, 256), (255, 256)]):
            got = score.segment_frames(dev(keys), (0.5, 0.5), mn, st).cpu().numpy()
            assert np.array_equal(got, score.segment_frames_numpy(keys, (0.5, 0.5), mn, st)), (st, mn)
    assert score.segment_frames(dev(keys), (0.5, 0.5), (256, 256))[0, 1024 - 400:1024 + 400].all()


# ---------------- 2. runs ---------------------------------------------------------------------------------------------------------------------
def check_runs(labels, st):
    from wear_mocap_ape_amd import score
    sof, n, table = score.segment_runs(dev(labels), st)
    w_sof, w_n, w_tab = score.segment_runs_numpy(labels, st)
    assert sof.dtype == n.dtype == table.dtype == torch.int32
    assert np.array_equal(sof.cpu().numpy(), w_sof) and np.array_equal(n.cpu().numpy(), w_n)
    tabs = [w_tab] if labels.ndim == 1 else w_tab
    got = table.cpu().numpy()[None] if labels.ndim == 1 else table.cpu().numpy()
    assert got.shape[1] == max(len(t) for t in tabs)
    for s, t in enumerate(tabs):
        assert np.array_equal(got[s, :len(t)], t), s
    return sof, n, table


@pytest.mark.parametrize("F", SIZES)
def test_runs_equal_the_statement(F):
    rng = np.random.default_rng(4600 + F)
    lab = np.stack([blocks(rng, F, [1, 2, 5, 40]), blocks(rng, F, [1, 1, 2, 300, 1100]), rng.integers(0, 256, size=F), np.zeros(F)]).astype(np.uint8)
    lab[0, rng.random(F) < 0.05] = 255
    check_runs(lab, starts_of(F))
    check_runs(lab[1], [0])


def test_every_frame_a_segment_one_segment_and_a_short_table():
    from wear_mocap_ape_amd import _hip, score
    F = 2500
    each = (np.arange(F) % 251).astype(np.uint8)            # no two neighbours equal: F segments
    whole = np.full(F, 255, dtype=np.uint8)                 # one segment of F frames
    _, n, table = check_runs(np.stack([each, whole]), [0])
    assert n.tolist() == [F, 1] and table[1, 0].tolist() == [0, 0, F, 255] and table.shape == (2, F, 4)
    _, n, _ = check_runs(np.stack([each, whole]), [0, 1024, 1025])
    assert n.tolist() == [F, 3]
    # a table too short: the count is the true one, the rows below cap are the table's, nothing past them is written; no seg_of_frame
    lab, st, cap = dev(np.stack([each, whole])), np.array([0, 1024], dtype=np.int32), 1500
    full = score.segment_runs(lab, [0, 1024])[2]
    n = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    table = torch.full((2, cap + 8, 4), -7, dtype=torch.int32, device="cuda")
    short = table[:, :cap]                                  # (a view: set s begins at s * (cap + 8) rows, so each set is called alone)
    for s in range(2):
        _hip.check(_hip.lib().ape_segment_runs(C.c_void_p(lab[s].data_ptr()), 1, F, C.c_void_p(st.ctypes.data), 2, None, C.c_void_p(n[s:].data_ptr()),
                                               C.c_void_p(short[s].data_ptr()), cap, None), "ape_segment_runs")
    torch.cuda.synchronize()
    assert n.tolist() == [F, 2]
    assert torch.equal(table[0, :cap], full[0, :cap]) and (table[0, cap:] == -7).all()
    assert torch.equal(table[1, :2], full[1, :2]) and (table[1, 2:] == -7).all()
    # the wrapper with a cap does not slice
    sof, n2, t2 = score.segment_runs(lab, [0, 1024], cap=cap, seg_of_frame=False)
    assert sof is None and t2.shape == (2, cap, 4) and torch.equal(t2[0], full[0, :cap]) and torch.equal(t2[1, :2], full[1, :2]) and n2.tolist() == [F, 2]


# ---------------- 3. stats --------------------------------------------------------------------------------------------------------------------
LENGTHS = (1023, 1025, 1, 1024, 2049, 7, 300, 1024)        # the 1025 begins at frame 1023 of tile 0, the last 1024 is aligned to nothing


def lengths_labels(lengths):
    return np.concatenate([np.full(n, i % 2, dtype=np.uint8) for i, n in enumerate(lengths)])


def test_stats_equal_the_statement_bit_for_bit():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(470)
    lab = lengths_labels(LENGTHS)
    F = lab.shape[0]
    labels = np.stack([lab, np.roll(lab, 5)])               # the second set's segments lie elsewhere
    st = [0, 1023 + 1025 + 1 + 1024 + 2049]                 # a recording boundary between two segments
    sof, n, table = score.segment_runs(dev(labels), st)
    tabs = score.segment_runs_numpy(labels, st)[2]
    vals = rng.normal(size=(2, F, 16)) * np.exp(rng.normal(size=(2, F, 16)) * 3.0)
    vals[..., 1] = np.round(vals[..., 1])                   # maxima that repeat
    vals[..., 2][rng.random((2, F)) < 0.2] = np.nan
    vals[..., 3] = np.nan                                   # an empty column
    vals[..., 4][rng.random((2, F)) < 0.01] = np.inf
    vals[..., 5][rng.random((2, F)) < 0.01] = -np.inf
    vals[..., 6][rng.random((2, F)) < 0.001] = rng.choice([np.inf, -np.inf], size=1)
    vd = dev(vals)
    # a set of values per set, 16 columns
    got = score.segment_stats(vd, sof, n, table).cpu().numpy()
    assert got.shape == (2, table.shape[1], 16, 5)
    for s in range(2):
        assert same_bits(got[s, :len(tabs[s])], score.segment_stats_numpy(vals[s], tabs[s])), s
    # one set of values shared by both sets of segments; a strided single column; float32
    shared = score.segment_stats(vd[1], sof, n, table).cpu().numpy()
    for s in range(2):
        assert same_bits(shared[s, :len(tabs[s])], score.segment_stats_numpy(vals[1], tabs[s])), s
    col = score.segment_stats(vd[0, :, 2], sof[0], n[0], table[0]).cpu().numpy()
    assert col.shape == (table.shape[1], 1, 5) and same_bits(col[:len(tabs[0])], score.segment_stats_numpy(vals[0, :, 2], tabs[0]))
    pair = score.segment_stats(vd[:, :, 1::5], sof, n, table).cpu().numpy()         # columns 1, 6, 11: a column stride of 5
    assert same_bits(pair[0, :len(tabs[0])], score.segment_stats_numpy(vals[0][:, 1::5], tabs[0]))
    v32 = vals[0, :, :3].astype(np.float32)
    f32 = score.segment_stats(dev(v32), sof[0], n[0], table[0]).cpu().numpy()
    assert same_bits(f32[:len(tabs[0])], score.segment_stats_numpy(v32, tabs[0]))
    # the first of a repeated maximum, -inf and -1 for an empty cell
    first = got[0, :len(tabs[0])]
    assert (first[:, 3, 0] == 0).all() and (first[:, 3, 3] == -np.inf).all() and (first[:, 3, 4] == -1).all()
    for i, (_, a, m, _) in enumerate(tabs[0].tolist()):
        assert first[i, 1, 4] == a + int(np.argmax(vals[0, a:a + m, 1]))


def test_a_table_with_a_cap_and_untouched_rows():
    from wear_mocap_ape_amd import _hip, score
    lab = lengths_labels(LENGTHS)
    F = lab.shape[0]
    vals = np.random.default_rng(471).normal(size=(F, 2))
    ld, vd = dev(lab), dev(vals)
    sof, n, table = score.segment_runs(ld, cap=5)           # eight segments, room for five
    assert int(n) == 8
    want = score.segment_stats_numpy(vals, score.segment_runs_numpy(lab)[2])
    out = torch.full((7, 2, 5), -7.0, dtype=torch.float64, device="cuda")
    _hip.check(_hip.lib().ape_segment_stats(C.c_void_p(vd.data_ptr()), _hip.F64, 1, 0, 2, 1, 2, 1, F, C.c_void_p(sof.data_ptr()),
                                            C.c_void_p(table.data_ptr()), C.c_void_p(n.data_ptr()), 5, C.c_void_p(out.data_ptr()), None),
               "ape_segment_stats")
    torch.cuda.synchronize()
    assert same_bits(out[:5].cpu().numpy(), want[:5]) and (out[5:] == -7.0).all()
    # fewer segments than rows: the rows from n_segs on are not written
    sof, n, table = score.segment_runs(ld, cap=12)
    out = torch.full((12, 2, 5), -7.0, dtype=torch.float64, device="cuda")
    _hip.check(_hip.lib().ape_segment_stats(C.c_void_p(vd.data_ptr()), _hip.F64, 1, 0, 2, 1, 2, 1, F, C.c_void_p(sof.data_ptr()),
                                            C.c_void_p(table.data_ptr()), C.c_void_p(n.data_ptr()), 12, C.c_void_p(out.data_ptr()), None),
               "ape_segment_stats")
    torch.cuda.synchronize()
    assert same_bits(out[:8].cpu().numpy(), want) and (out[8:] == -7.0).all()


def test_the_maximum_is_the_value_at_its_frame():
    """+0.0 and -0.0 compare equal: the earlier one is the maximum, with its own sign, within a piece and across two"""
    from wear_mocap_ape_amd import score
    vals = np.full(1500, -1.0)
    vals[[3, 1030]], vals[[4, 1031, 1400]] = -0.0, 0.0
    lab = np.zeros(1500, dtype=np.uint8)
    lab[1030:1032], lab[1032:] = 1, 2                       # segments [0, 1030), [1030, 1032), [1032, 1500)
    sof, n, table = score.segment_runs(dev(lab))
    got = score.segment_stats(dev(vals), sof, n, table).cpu().numpy()
    assert same_bits(got, score.segment_stats_numpy(vals, table.cpu().numpy()))
    assert got[:, 0, 4].tolist() == [3, 1030, 1400] and np.signbit(got[:, 0, 3]).tolist() == [True, True, False]
    whole = score.segment_stats(dev(vals[1:]), *score.segment_runs(dev(np.zeros(1499, dtype=np.uint8)))).cpu().numpy()
    assert whole[0, 0, 4] == 2 and np.signbit(whole[0, 0, 3]) and whole[0, 0, 0] == 1499     # the second piece's +0.0 does not replace it


def test_a_segment_has_the_same_bits_wherever_its_recording_lies():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(472)
    recs = [(1500, [700, 800]), (1, [1]), (2349, [2049, 300]), (1024, [1024]), (1031, [3, 1025, 3])]
    parts = [(lengths_labels(ls), (rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-3, 4, size=(n, 3))).astype(np.float32)) for n, ls in recs]
    results = []
    for order in ([0, 1, 2, 3, 4], [4, 2, 0, 3, 1], [3, 1, 4, 0, 2]):
        lab = np.concatenate([parts[i][0] for i in order])
        vals = np.concatenate([parts[i][1] for i in order])
        st = np.cumsum([0] + [recs[i][0] for i in order])[:-1].tolist()
        sof, n, table = score.segment_runs(dev(lab), st)
        stats = score.segment_stats(dev(vals), sof, n, table).cpu().numpy()
        tab = table.cpu().numpy()
        assert same_bits(stats, score.segment_stats_numpy(vals, tab))
        per = {}
        for i, (r, a, m, _) in enumerate(tab.tolist()):
            rec = order[r]
            rel = stats[i].copy()
            rel[:, 4] -= st[r]                              # the frame of the maximum, counted from the recording's first
            per.setdefault(rec, []).append((a - st[r], m, rel))
        results.append(per)
    for other in results[1:]:
        for rec in range(len(recs)):
            assert len(other[rec]) == len(results[0][rec])
            for (a0, m0, s0), (a1, m1, s1) in zip(results[0][rec], other[rec]):
                assert (a0, m0) == (a1, m1) and same_bits(s0, s1), rec


def test_the_same_call_twice_gives_the_same_bytes():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(473)
    F = 2500
    kd, st = dev(slow_keys(rng, 3, F)), starts_of(F)
    vd = dev(rng.normal(size=(3, F, 4)))
    runs = []
    for _ in range(2):
        labels = score.segment_frames(kd, (0.25, 0.5), (7, 9), st)
        sof, n, table = score.segment_runs(labels, st)
        runs.append((labels, sof, n, table, score.segment_stats(vd, sof, n, table)))
    (l0, f0, n0, t0, s0), (l1, f1, n1, t1, s1) = runs
    assert torch.equal(l0, l1) and torch.equal(f0, f1) and torch.equal(n0, n1)
    for s, k in enumerate(n0.tolist()):                     # (rows from n_segs on are not written)
        assert k > 10 and torch.equal(t0[s, :k], t1[s, :k]) and torch.equal(s0[s, :k].view(torch.int64), s1[s, :k].view(torch.int64))


# ---------------- 4. the planted trajectory, on the estimator -----------------------------------------------------------------------------------
def test_segment_recording_on_the_planted_trajectory(norm_stats, tmp_path):
    from tests.test_post_sweep_gpu import pocket
    from wear_mocap_ape_amd import _hip, score
    from wear_mocap_ape_amd.estimate import nn_models
    yh, truth, _ = reach_and_hold()
    F = yh.shape[0]
    m = nn_models.DropoutLSTM(22, 256, 2, 14, dropout=0.2, device=0, target_layout=_hip.LAYOUT_ORI_CAL_LARM_UARM_HIPS)
    st = norm_stats["pocket"]
    m.set_norm_stats(st["xx_m"], st["xx_s"], np.zeros(14), np.ones(14))
    m.set_body(orc.DEFAULT_BODY)
    windows, _ = score.ladder(samples=yh.shape[1])
    raw, pilot = score.post_window(m, torch.from_numpy(yh).cuda(), [windows[0], windows[PILOT]])
    est = pocket(tmp_path, 3, yh.shape[1])
    td = dev(truth)
    res = est.segment_recording(raw, pilot_rows=pilot, thresholds=EST_RULE[0], mins=EST_RULE[1], truth=td, truth_kind="est",
                                truth_thresholds=TRUTH_RULE[0], truth_mins=TRUTH_RULE[1])
    with np.load(FIXTURE) as z:
        want = {k: z[k] for k in z.files}
    assert np.array_equal(res["labels"].cpu().numpy(), want["est_labels"]) and np.array_equal(res["table"].cpu().numpy(), want["est_table"])
    assert np.array_equal(res["truth"]["labels"].cpu().numpy(), want["truth_labels"])
    assert np.array_equal(res["truth"]["table"].cpu().numpy(), want["truth_table"])
    mt = res["match"]
    print(f"planted trajectory on the device: matched {mt['matched']}, missed {mt['missed']}, spurious {mt['spurious']}, onset "
          f"{mt['onset'].tolist()}, offset {mt['offset'].tolist()}")
    assert (mt["matched"], mt["missed"], mt["spurious"]) == (6, 0, 0) and np.abs(mt["onset"]).max() <= 2 and np.abs(mt["offset"]).max() <= 2
    # the records are the statement's over the same per-frame columns
    assert res["names"] == ["hand_speed", "path", "hand_pos", "elbow_pos"]
    speed = score.motion_sums(HIPS, pilot, "msg", per_frame=True)[0][:, 0]
    errors = score.score_rows(HIPS, raw, td, "est")[0]
    cols = torch.stack([speed, speed, errors[:, 0], errors[:, 1]], dim=1).cpu().numpy()
    assert same_bits(res["stats"].cpu().numpy(), score.segment_stats_numpy(cols, want["est_table"]))
    # the endpoint error of every hold of the truth: the distance between the two mean hand positions over its frames
    hold = res["hold_error"].cpu().numpy()
    rh = raw.cpu().numpy()[:, 4:7]
    for i, (_, a, n, lab) in enumerate(want["truth_table"].tolist()):
        if lab == 1:
            assert np.isnan(hold[i])
        else:
            d = np.linalg.norm(rh[a:a + n].mean(axis=0) - truth[a:a + n, 0:3].mean(axis=0))
            assert abs(hold[i] - d) < 1e-12, (i, hold[i], d)
    # the truth alone, on the FK estimator's method as well
    tr = est.truth_segments(td, "est", TRUTH_RULE[0], TRUTH_RULE[1])
    assert torch.equal(tr["table"], res["truth"]["table"]) and tr["names"] == ["hand_speed", "path"]
    rows = score.summarise_segments(res["table"], res["stats"], res["names"])
    assert [(r["recording"], r["label"], r["count"]) for r in rows] == [(0, 0, 6), (0, 1, 6)]
