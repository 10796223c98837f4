"""Per-stream smoothing lengths on the GPU: one bank, many clients, each with the ``smooth`` its estimator would have been
built with.

Against the reference: ``smooth_traces.npz`` (tests/golden/gen_smooths.py) holds the messages and tails of the reference estimators built
with smooth 1, 2, 3, 5 and 8; stream s of a bank of capacity 8 with ``smooths[s] = k`` must return those of k.  Product against product,
bit for bit: a stream of a table bank equals the same stream of a uniform bank built with ``smooth = smooths[s]`` (same S, samples, seed
and rows, so the Monte-Carlo draws agree) -- the yardstick is the code as it was, which is pinned to the reference; a table of all
``cap`` equals the bank before ``set_smooths``; subset schedules with cold starts and a changed length equal one-stream uniform banks;
host frames equal device frames; a stream moves between banks with its length; refused calls leave no trace; frames enqueued around a
``set_smooths`` see the old and the new table.

Not covered here: the re-issue of an aborted frame (``ape_model_recover``), as in tests/test_bodies_gpu.py.  A re-issued lockstep step goes
through ``ape_streams_step`` again (with the bank's step count set back), a re-issued subset frame through ``subset_regress_post``; both
launch the post-filter through ``ape_launch_stream_post_smooths`` / ``ape_launch_stream_post_subset_smooths``, which read the bank's
device table, and the subset frame's slots (taken mod k on the host) are still in the bank's descriptor buffer.  The existing hook under
tests/hooks/ was left as it is."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_replay import _estimator, _synthetic_rows

pytestmark = pytest.mark.gpu

TOL_MSG_LOOP = 5e-6     # tests/test_bodies_gpu.py, tests/test_hip_round4.py: the same traces
TOL_FK_REF = 1e-5       # tests/test_fk_only_gpu.py against the reference's fk_only traces


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


@pytest.fixture(scope="module")
def traces(golden):
    return golden("smooth_traces.npz")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _lockstep(bank, kind, rows_t, spread=True):
    """rows_t [F, S, width] -> datagram rows [F, S, w] on the host"""
    outs = []
    for rows in rows_t:
        bank.push_rows(torch.from_numpy(np.ascontiguousarray(rows)).cuda(), kind)
        outs.append(bank.step_datagrams(spread=spread).cpu().numpy().copy())
    return np.stack(outs)


def _check_row(r, u, k, M, cap, spread, where):
    """r: a table bank's datagram row of a stream of length k (stride of cap); u: the row of a uniform bank built with smooth = k"""
    N, NS, tail = k * M, cap * M, 21 if spread else 0
    assert r.shape == (25 + 6 * NS + tail,), where
    assert u.shape == ((25 + 6 * N if N > 1 else 25) + tail,), where
    live = 25 + 6 * N if N > 1 else 25
    assert _same(r[:live], u[:live]), where
    if N == 1:                                       # the one row's hand and elbow origins: what the message itself carries
        assert _same(r[25:31], np.concatenate([r[4:7], r[11:14]])), where
    if spread:
        assert _same(r[-21:], u[-21:]), where
    pad = r[25 + 6 * N:25 + 6 * NS]
    assert not _bits(pad).any(), where               # exact zeros, every frame


# ---------------- 1. against the reference fixture ----------------------------------------------------------------------------------
SMOOTHS_REF, CAP_REF = [1, 2, 3, 5, 8, 8, 5, 3, 2, 1], 8


@pytest.mark.parametrize("name", ["pocket", "watch", "uarm"])
def test_bank_with_a_smooth_per_stream_replays_the_reference(golden, traces, tmp_path, monkeypatch, name):
    from wear_mocap_ape_amd.streams import StreamBank
    g = golden(f"stream_trace_{name}.npz")
    S = len(SMOOTHS_REF)
    est = _estimator(tmp_path, monkeypatch, name, int(g["weights_seed"]), 0.0, smooth=CAP_REF, monte_carlo_samples=1)
    bank = StreamBank(est._hip_model(), S, est.sequence_len, smooth=CAP_REF, normalize=True, dtype=torch.float64)
    assert bank.smooths.tolist() == [CAP_REF] * S                       # before: S copies of the capacity
    bank.set_smooths(SMOOTHS_REF)
    assert bank.smooths.tolist() == SMOOTHS_REF and bank.smooths.dtype == np.int32
    assert bank.state_desc()["smooth"] == CAP_REF
    worst = 0.0
    for f, row in enumerate(g["rows"]):
        bank.push_rows(torch.from_numpy(np.tile(row.astype(np.float32), (S, 1))).cuda(), est._parse_kind)
        msg, tail = bank.step(with_tail=True)
        msg, tail = msg.cpu().numpy(), tail.cpu().numpy().reshape(S, -1)
        assert tail.shape[1] == 6 * CAP_REF
        for s, k in enumerate(SMOOTHS_REF):
            worst = max(worst, float(np.abs(msg[s] - traces[f"msg_{name}_s{k}"][f]).max()),
                        float(np.abs(tail[s, :6 * k] - traces[f"tail_{name}_s{k}"][f]).max()))
            assert not _bits(tail[s, 6 * k:]).any(), (f, s)
    print(f"{name}: worst |bank - reference| = {worst:.3e}")
    assert worst < TOL_MSG_LOOP, (name, worst)
    est._hip_model().check()


def test_fk_bank_with_a_smooth_per_stream_replays_the_reference(golden, traces):
    from wear_mocap_ape_amd.streams import FkStreamBank
    fk = golden("fk_only_trace.npz")
    rows = fk["rows"][:20].astype(np.float32)
    S = len(SMOOTHS_REF)
    bank = FkStreamBank(S, smooth=CAP_REF, dtype=torch.float64)
    assert bank.smooths.tolist() == [CAP_REF] * S
    bank.set_smooths(SMOOTHS_REF)
    assert bank.smooths.tolist() == SMOOTHS_REF and bank.datagram_lengths().tolist() == [25 + 6 * k if k > 1 else 25 for k in SMOOTHS_REF]
    worst = 0.0
    for f, row in enumerate(rows):
        out = bank.step_rows(np.tile(row, (S, 1))).cpu().numpy()
        for s, k in enumerate(SMOOTHS_REF):
            worst = max(worst, float(np.abs(out[s] - traces[f"msg_fk_s{k}"][f]).max()))
    print(f"fk: worst |bank - reference| = {worst:.3e}")
    assert worst < TOL_FK_REF, worst


# ---------------- 2. / 3. / 5. product against product, bit for bit -------------------------------------------------------------
SMOOTHS_8, CAP = [1, 2, 3, 5, 5, 3, 2, 1], 5


@pytest.fixture(scope="module")
def pocket_rows(golden):
    """12 frames x 8 streams of raw rows that differ per stream"""
    return _synthetic_rows(golden, "pocket", 12 * 8, 41).reshape(12, 8, -1)


def _pocket(tmp_path, monkeypatch, mc):
    est = _estimator(tmp_path, monkeypatch, "pocket", 5, 0.2, smooth=CAP, monte_carlo_samples=mc or 1)
    return est._hip_model(), est.sequence_len, est._parse_kind


@pytest.mark.parametrize("mc", [None, 25])
def test_table_streams_equal_uniform_banks_bit_for_bit(pocket_rows, tmp_path, monkeypatch, mc):
    """25 samples: stacks of 25 / 50 / 75 / 125 rows -- inside one 64-row chunk, two that cross it, in a bank that holds the split form's
    workspaces (chunks past a stream's rows arrive with zero partial sums); one sample: k = 1 meets the uniform bank's lane-per-stream
    form.  Also: a table of all ``cap`` equals the bank before ``set_smooths`` (no table, no change)."""
    from wear_mocap_ape_amd.streams import StreamBank
    model, T, kind = _pocket(tmp_path, monkeypatch, mc)
    S, M = 8, mc or 1
    mk = lambda k: StreamBank(model, S, T, smooth=k, normalize=True, dtype=torch.float32, monte_carlo_samples=mc, seed=77)   # noqa: E731
    tab = mk(CAP)
    tab.set_smooths(SMOOTHS_8)
    got = _lockstep(tab, kind, pocket_rows)
    # the table forms keep the grid of the capacity -- split over its chunks where the bank holds the workspaces
    assert tab.last_post_form() == ("split x2" if mc else "one workgroup")
    assert tab.datagram_lengths().tolist() == [25 + 6 * k * M if k * M > 1 else 25 for k in SMOOTHS_8]
    forms = {}
    for k in sorted(set(SMOOTHS_8)):
        bank = mk(k)
        uni = _lockstep(bank, kind, pocket_rows)
        forms[k] = bank.last_post_form()
        for s in [s for s, ks in enumerate(SMOOTHS_8) if ks == k]:
            for f in range(len(pocket_rows)):
                _check_row(got[f, s], uni[f, s], k, M, CAP, True, (mc, k, s, f))
        if k == CAP:                                 # no table, no change
            same = mk(CAP)
            same.set_smooths([CAP] * S)
            assert _same(_lockstep(same, kind, pocket_rows), uni)
            assert same.smooths.tolist() == [CAP] * S
    assert forms == ({1: "one workgroup", 2: "one workgroup", 3: "split x2", 5: "split x2"} if mc else
                     {1: "wide", 2: "one workgroup", 3: "one workgroup", 5: "one workgroup"})
    parts = tab.split_datagrams(got[-1])
    assert [p.shape[0] for p in parts] == tab.datagram_lengths().tolist()
    model.check()


@pytest.mark.parametrize("mc", [None, 25])
def test_host_frames_equal_device_frames(pocket_rows, tmp_path, monkeypatch, mc):
    """lockstep ``ape_streams_frame_host`` on a table bank: the bits of the device frames; one sample: also ``frame_host`` over all streams"""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    model, T, kind = _pocket(tmp_path, monkeypatch, mc)
    S, M = 8, mc or 1
    mk = lambda: StreamBank(model, S, T, smooth=CAP, normalize=True, dtype=torch.float32, monte_carlo_samples=mc, seed=77)   # noqa: E731
    dev = mk()
    dev.set_smooths(SMOOTHS_8)
    want = _lockstep(dev, kind, pocket_rows)
    host = mk()
    host.set_smooths(SMOOTHS_8)
    lib, st = _hip.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = np.empty((S, 25 + 6 * CAP * M + 21), dtype=np.float32)
    for f, rows in enumerate(pocket_rows):
        rows = np.ascontiguousarray(rows)
        _hip.check(lib.ape_streams_frame_host(host._handle, kind, C.c_void_p(rows.ctypes.data), _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_SPREAD,
                                              C.c_void_p(out.ctypes.data), _hip.F32, st), "ape_streams_frame_host")
        assert _same(out, want[f]), (mc, f)
    if mc is None:
        sub = mk()
        sub.set_smooths(SMOOTHS_8)
        for f, rows in enumerate(pocket_rows):
            got = sub.frame_host(np.ascontiguousarray(rows), np.arange(S), kind, datagrams=True, spread=True)
            assert _same(got, want[f]), f
    model.check()


# ---------------- 4. subset schedule ---------------------------------------------------------------------------------------------
def test_subset_schedule_with_cold_starts_and_a_changed_length(golden, tmp_path, monkeypatch):
    """per-stream mode, deterministic: stream j gets a row every (j % 3 + 1)-th tick through ``frame`` and ``frame_host`` alternately;
    stream 2 is cold-started at tick 11, stream 3 gets smooth 2 at tick 17.  Every row equals the row of a one-stream uniform bank of the
    stream's current length fed the same rows with the same cold starts; streams a call does not list keep their rings"""
    from wear_mocap_ape_amd.streams import StreamBank
    est = _estimator(tmp_path, monkeypatch, "pocket", 3, 0.0, smooth=CAP, monte_carlo_samples=1)
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    model.set_kernel("tile16")                        # (the regressor's bits must not depend on the number of rows in a launch)
    try:
        S, smooths = 6, [1, 2, 3, 5, 2, 3]
        pool = _synthetic_rows(golden, "pocket", 30 * S, 43).reshape(30, S, -1)
        mk = lambda n, k: StreamBank(model, n, T, smooth=k, normalize=True, dtype=torch.float32)   # noqa: E731
        tab = mk(S, CAP)
        tab.set_smooths(smooths)
        refs = [mk(1, k) for k in smooths]
        everyone = np.arange(S)

        def records():
            state, warm = tab.export_state(everyone)
            return state.cpu().numpy().copy(), warm.copy()

        def untouched(before, listed):
            after = records()
            rest = [s for s in range(S) if s not in listed]
            assert _same(before[0][rest], after[0][rest]) and np.array_equal(before[1][rest], after[1][rest]), listed

        seen = 0
        for t in range(30):
            if t == 11:
                before = records()
                tab.reset(streams=[2])
                refs[2].reset()
                untouched(before, [2])
                assert tab.export_state([2])[1].tolist() == [0]
            if t == 17:
                before = records()
                tab.set_smooths([2], streams=[3])
                smooths[3] = 2
                refs[3] = mk(1, 2)
                untouched(before, [3])
                assert tab.smooths.tolist() == smooths and tab.export_state([3])[1].tolist() == [0]
            listed = np.array([j for j in range(S) if t % (j % 3 + 1) == 0])
            rows = np.ascontiguousarray(pool[t, listed])
            before = records()
            if t % 2 == 0:
                got = tab.frame(rows, listed, kind, datagrams=True).cpu().numpy()
            else:
                got = tab.frame_host(rows, listed, kind, datagrams=True)
            untouched(before, list(listed))
            assert got.shape == (len(listed), 25 + 6 * CAP)
            for i, j in enumerate(listed):
                want = refs[j].frame(rows[i:i + 1], [0], kind, datagrams=True).cpu().numpy()[0]
                _check_row(got[i], want, smooths[j], 1, CAP, False, (t, j))
                seen += 1
        assert seen == 30 * 2 + 15 * 2 + 10 * 2
        assert tab.last_post_form() == "one workgroup"
        model.check()
    finally:
        model.set_kernel("auto")


# ---------------- 6. hand-over ---------------------------------------------------------------------------------------------------
def test_a_stream_moves_between_banks_with_its_length(golden, tmp_path, monkeypatch):
    from wear_mocap_ape_amd import stream_state as ss
    from wear_mocap_ape_amd.streams import StreamBank
    est = _estimator(tmp_path, monkeypatch, "pocket", 4, 0.0, smooth=CAP, monte_carlo_samples=1)
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    model.set_kernel("tile16")
    try:
        S = 4
        pool = _synthetic_rows(golden, "pocket", 13 * S, 44).reshape(13, S, -1)
        mk = lambda: StreamBank(model, S, T, smooth=CAP, normalize=True, dtype=torch.float32)   # noqa: E731
        a, b = mk(), mk()
        a.set_smooths([3, 5, 1, 2])
        for t in range(7):
            a.push_rows(torch.from_numpy(np.ascontiguousarray(pool[t])).cuda(), kind)
            a.step_datagrams()
        state, warm = a.export_state([0, 3])
        desc = a.state_desc()
        assert warm.tolist() == [3, 3] and desc["smooth"] == CAP
        for rec, k in zip(state.cpu().numpy(), (3, 2)):
            _, stack = ss.unpack(rec, desc)
            assert np.abs(stack[:k]).min() > 0 and not _bits(stack[k:]).any()       # k predictions oldest first, zeros behind them
        b.set_smooths([3, 2], streams=[1, 0])                  # first the length (a cold start of the slot) ...
        assert b.smooths.tolist() == [2, 3, CAP, CAP]
        b.import_state([1, 0], state, warm, desc)              # ... then the history
        back, _ = b.export_state([1, 0])
        assert _same(back.cpu().numpy(), state.cpu().numpy())
        for t in range(7, 13):
            a.push_rows(torch.from_numpy(np.ascontiguousarray(pool[t])).cuda(), kind)
            want = a.step_datagrams().cpu().numpy()
            got = b.frame(np.ascontiguousarray(pool[t, [0, 3]]), [1, 0], kind, datagrams=True).cpu().numpy()
            assert _same(got[0], want[0]) and _same(got[1], want[3]), t
            assert not _bits(got[0][25 + 18:]).any() and not _bits(got[1][25 + 12:]).any()
        model.check()
    finally:
        model.set_kernel("auto")


# ---------------- 7. the FK bank, product against product -----------------------------------------------------------------------
def test_fk_bank_streams_equal_uniform_banks_bit_for_bit():
    from tests.test_fk_only_gpu import _random_rows
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import FkStreamBank
    S, F = 8, 12
    rng = np.random.default_rng(45)
    pool = _random_rows(rng, 2 * F * S).reshape(2 * F, S, 55)
    mk = lambda k: FkStreamBank(S, smooth=k, dtype=torch.float64)   # noqa: E731
    schedule = [np.array([j for j in range(S) if (t + j) % 3 != 0]) for t in range(F)]

    def run(bank):
        """12 lockstep frames (device and host entry alternately), then 12 subset frames through frame / frame_host alternately"""
        lib, st = _hip.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
        outs = []
        for t in range(F):
            if t % 2 == 0:
                outs.append(bank.step_rows(pool[t]).cpu().numpy().copy())
            else:
                rows, out = np.ascontiguousarray(pool[t]), np.empty((S, 25), dtype=np.float64)
                _hip.check(lib.ape_fk_bank_frame_host(bank._handle, _hip.PARSE_WATCH_PHONE_UARM, C.c_void_p(rows.ctypes.data),
                                                      C.c_void_p(out.ctypes.data), _hip.F64, st), "ape_fk_bank_frame_host")
                outs.append(out)
        subs = []
        for t in range(F):
            rows = np.ascontiguousarray(pool[F + t, schedule[t]])
            got = bank.frame(rows, schedule[t]).cpu().numpy().copy() if t % 2 == 0 else bank.frame_host(rows, schedule[t])
            full = np.full((S, 25), np.nan)
            full[schedule[t]] = got
            subs.append(full)
        return np.stack(outs), np.stack(subs)

    tab = mk(CAP)
    tab.set_smooths(SMOOTHS_8)
    got = run(tab)
    for k in sorted(set(SMOOTHS_8)):
        uni = run(mk(k))
        cols = [s for s, ks in enumerate(SMOOTHS_8) if ks == k]
        assert _same(got[0][:, cols], uni[0][:, cols]) and _same(got[1][:, cols], uni[1][:, cols]), k
        if k == CAP:
            same = mk(CAP)
            same.set_smooths([CAP] * S)
            again = run(same)
            assert _same(again[0], uni[0]) and _same(again[1], uni[1])
    # hand-over: stream 1 (k = 2) and stream 2 (k = 3) leave for slots 6 and 0 of another bank
    state, warm = tab.export_state([1, 2])
    rec = state.cpu().numpy().view(np.float64).reshape(2, CAP, 8)
    assert np.abs(rec[0, :2]).max() > 0 and not rec[0, 2:].any() and np.abs(rec[1, :3]).max() > 0 and not rec[1, 3:].any()
    other = mk(CAP)
    other.set_smooths([2, 3], streams=[6, 0])
    other.import_state([6, 0], state, warm, tab.state_desc())
    more = _random_rows(rng, 4 * S).reshape(4, S, 55)
    for t in range(4):
        want = tab.step_rows(more[t]).cpu().numpy()
        out = other.frame(np.ascontiguousarray(more[t, [1, 2]]), [6, 0]).cpu().numpy()
        assert _same(out[0], want[1]) and _same(out[1], want[2]), t


# ---------------- 8. refusals ---------------------------------------------------------------------------------------------------
def test_refused_calls_leave_no_trace(pocket_rows, tmp_path, monkeypatch):
    from tests.test_fk_only_gpu import _random_rows
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import FkStreamBank, StreamBank
    model, T, kind = _pocket(tmp_path, monkeypatch, None)
    S = 8
    lib, st = _hip.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)   # noqa: E731
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
    # (list, K, values, what the message names)
    cases = [(i32([0, 1]), 2, i32([0, 1]), b"smooth 0"), (i32([0, 1]), 2, i32([1, CAP + 1]), b"smooth 6"), (i32([3, 3]), 2, i32([1, 1]), b"twice"),
             (i32([0, S]), 2, i32([1, 1]), b"outside"), (i32([0, -1]), 2, i32([1, 1]), b"outside"),
             (i32(list(range(S)) + [0]), S + 1, i32([1] * (S + 1)), b"K=9"), (None, S - 1, i32([1] * S), b"no stream list"),
             (i32([0]), -1, i32([1]), b"K=-1"), (i32([0]), 1, None, b"NULL")]

    def refuse(entry, getter, handle, expect):
        for lst, K, vals, word in cases:
            assert getattr(lib, entry)(handle, ptr(lst), K, ptr(vals), st) != 0, (entry, word)
            assert word in lib.ape_last_error(), (entry, word, lib.ape_last_error())
            out = np.zeros((S,), dtype=np.int32)
            _hip.check(getattr(lib, getter)(handle, C.c_void_p(out.ctypes.data)), getter)
            assert out.tolist() == expect, (entry, word)

    mk = lambda: StreamBank(model, S, T, smooth=CAP, normalize=True, dtype=torch.float32)   # noqa: E731
    clean, hit, never = mk(), mk(), mk()
    clean.set_smooths(SMOOTHS_8)
    hit.set_smooths(SMOOTHS_8)
    want = _lockstep(clean, kind, pocket_rows)
    got = []
    for f, rows in enumerate(pocket_rows):
        if f in (0, 5):
            refuse("ape_streams_set_smooths", "ape_streams_get_smooths", hit._handle, SMOOTHS_8)
        got.append(_lockstep(hit, kind, rows[None])[0])
    assert _same(np.stack(got), want)
    refuse("ape_streams_set_smooths", "ape_streams_get_smooths", never._handle, [CAP] * S)    # ... and a bank without a table stays without
    assert _same(_lockstep(never, kind, pocket_rows[:6]), _lockstep(mk(), kind, pocket_rows[:6]))
    assert never.last_post_form() == "one workgroup"

    rng = np.random.default_rng(46)
    rows = _random_rows(rng, 6 * S).reshape(6, S, 55)
    fmk = lambda: FkStreamBank(S, smooth=CAP, dtype=torch.float64)   # noqa: E731
    fclean, fhit = fmk(), fmk()
    fclean.set_smooths(SMOOTHS_8)
    fhit.set_smooths(SMOOTHS_8)
    for f in range(6):
        if f in (0, 3):
            refuse("ape_fk_bank_set_smooths", "ape_fk_bank_get_smooths", fhit._handle, SMOOTHS_8)
        assert _same(fhit.step_rows(rows[f]).cpu().numpy(), fclean.step_rows(rows[f]).cpu().numpy()), f
    model.check()


# ---------------- 9. order on the stream ----------------------------------------------------------------------------------------
def test_set_smooths_is_ordered_between_frames_on_one_stream(pocket_rows, tmp_path, monkeypatch):
    """frames f, f+1, set_smooths, frames f+2, f+3 enqueued back to back with no synchronisation: the first two carry the old table, the
    last two are a cold start at the new one.  The FK bank at 4096 streams (the frame is one launch), then the NN bank."""
    from tests.test_fk_only_gpu import _random_rows
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import FkStreamBank, StreamBank
    S = 4096
    rng = np.random.default_rng(47)
    old, new = rng.integers(1, CAP + 1, size=S).astype(np.int32), rng.integers(1, CAP + 1, size=S).astype(np.int32)
    rows = torch.from_numpy(_random_rows(rng, 7 * S).reshape(7, S, 55)).cuda()
    mk = lambda: FkStreamBank(S, smooth=CAP, dtype=torch.float64)   # noqa: E731
    bank, ref_old, ref_new = mk(), mk(), mk()
    bank.set_smooths(old)
    ref_old.set_smooths(old)
    ref_new.set_smooths(new)
    for t in range(3):
        bank.step_rows(rows[t])
        ref_old.step_rows(rows[t])
    out = torch.zeros((4, S, 25), dtype=torch.float64, device="cuda")
    lib, st = _hip.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kind = _hip.PARSE_WATCH_PHONE_UARM
    buf = new.copy()
    torch.cuda.synchronize()
    for t in range(4):
        if t == 2:
            _hip.check(lib.ape_fk_bank_set_smooths(bank._handle, None, S, C.c_void_p(buf.ctypes.data), st))
            buf[:] = -7                               # the caller's buffer is free on return
        _hip.check(lib.ape_fk_bank_frame(bank._handle, kind, C.c_void_p(rows[3 + t].data_ptr()), None, S, C.c_void_p(out[t].data_ptr()), _hip.F64, st))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for t in range(4):
        want = (ref_old if t < 2 else ref_new).step_rows(rows[3 + t]).cpu().numpy()
        assert _same(got[t], want), t
    assert np.array_equal(bank.smooths, new)

    model, T, pk = _pocket(tmp_path, monkeypatch, None)
    S = 8
    nmk = lambda: StreamBank(model, S, T, smooth=CAP, normalize=True, dtype=torch.float32)   # noqa: E731
    bank, ref_old, ref_new = nmk(), nmk(), nmk()
    new8 = SMOOTHS_8[::-1][:4] + [4, 4, 1, 5]
    bank.set_smooths(SMOOTHS_8)
    ref_old.set_smooths(SMOOTHS_8)
    ref_new.set_smooths(new8)
    dev_rows = torch.from_numpy(np.ascontiguousarray(pocket_rows)).cuda()
    for t in range(3):
        bank.push_rows(dev_rows[t], pk)
        bank.step_datagrams()
    want_old = _lockstep(ref_old, pk, pocket_rows[:5], spread=False)[3:]
    want_new = _lockstep(ref_new, pk, pocket_rows[5:7], spread=False)
    torch.cuda.synchronize()
    outs = []
    for t in range(3, 7):
        if t == 5:
            bank.set_smooths(new8)
        bank.push_rows(dev_rows[t], pk)
        outs.append(bank.step_datagrams().clone())    # (a copy on the same stream: nothing waits for the host)
    torch.cuda.synchronize()
    got = torch.stack(outs).cpu().numpy()
    assert _same(got[:2], want_old) and _same(got[2:], want_new)
    model.check()
