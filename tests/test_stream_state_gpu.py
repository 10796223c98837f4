"""Stream state hand-over on the device (``ape_streams_export`` / ``ape_streams_import``, the FK-only bank's trio, ``Estimator.get_state``
/ ``set_state``).  The criterion everywhere is equivalence to the uninterrupted run: a stream that left its bank and
came back, or moved to another slot of another bank, continues with the bits of a twin that was never touched (regressor pinned to
``tile16``), and streams that were not listed keep their bytes."""
from array import array

import numpy as np
import pytest
import torch

from tests.test_replay import _estimator, _synthetic_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def _bank(model, S, T, smooth, **kw):
    from wear_mocap_ape_amd.streams import StreamBank
    return StreamBank(model, S, T, smooth=smooth, normalize=True, dtype=torch.float64, **kw)


def _frame(bank, kind, rows, streams, datagrams=False):
    return bank.frame(np.ascontiguousarray(rows, dtype=np.float32), streams, kind, datagrams=datagrams).cpu().numpy().copy()


def _all(bank):
    state, warm = bank.export_state(np.arange(bank._n))
    return state.cpu().numpy().copy(), warm.copy()


def _schedule(S, t):
    """the streams of frame t: every stream skips some frames, so that rows and predictions since the cold start differ by stream"""
    return np.array([s for s in range(S) if (t + s) % 4 != 0])


def _round_trip(make_bank, kind, pool, S, listed, checkpoints, frames):
    """two banks fed the same subset frames; at every checkpoint the listed streams of one leave (export, cold start) and come back
    (import).  Every frame of both banks must be equal, and the streams that stayed must keep their bytes"""
    a, twin = make_bank(), make_bank()
    desc = a.state_desc()
    assert desc["words_per_stream"] % 4 == 0 and desc["words_per_stream"] >= desc["T"] * desc["I"] + desc["smooth"] * desc["n_mc"] * desc["O"]
    rest = np.array([s for s in range(S) if s not in listed])
    phases = set()
    for t in range(frames):
        streams = _schedule(S, t)
        rows = pool[t, streams]
        got, want = _frame(a, kind, rows, streams), _frame(twin, kind, rows, streams)
        assert np.array_equal(got, want), t
        if t + 1 in checkpoints:
            before, warm_before = _all(a)
            state, warm = a.export_state(listed)
            assert state.dtype == torch.float32 and tuple(state.shape) == (len(listed), desc["words_per_stream"]) and state.is_cuda
            assert warm.dtype == np.uint8 and warm.tolist() == [3] * len(listed)
            a.reset(streams=listed)
            assert a.export_state(listed)[1].tolist() == [0] * len(listed)
            a.import_state(listed, state, warm, desc)
            after, warm_after = _all(a)
            # the canonical form does not depend on the ring phase: listed streams read back equal although their slots moved;
            # for the others the phase is the same before and after, so equal records mean equal ring bytes
            assert np.array_equal(before.view(np.uint32), after.view(np.uint32)) and np.array_equal(warm_before, warm_after)
            assert np.array_equal(before[rest].view(np.uint32), _all(twin)[0][rest].view(np.uint32))
            phases.add(((t + 1) % desc["T"], (t + 1) % desc["smooth"]))
    return phases


def test_round_trip_within_a_bank(golden, tmp_path, monkeypatch):
    est = _estimator(tmp_path, monkeypatch, "pocket", 3, 0.0, smooth=5, add_mc_samples=True, monte_carlo_samples=1)
    model, kind = est._hip_model(), est._parse_kind
    model.set_kernel("tile16")
    S, T, smooth = 7, 6, 5
    pool = _synthetic_rows(golden, "pocket", S * 15, 5).reshape(15, S, -1)
    phases = _round_trip(lambda: _bank(model, S, T, smooth), kind, pool, S, [5, 0, 3], (4, 7, 13), 15)
    assert len(phases) == 3
    model.set_kernel("auto")


def test_migration_across_slot_phase(golden, tmp_path, monkeypatch):
    est = _estimator(tmp_path, monkeypatch, "pocket", 4, 0.0, smooth=5, add_mc_samples=True, monte_carlo_samples=1)
    model, kind = est._hip_model(), est._parse_kind
    model.set_kernel("tile16")
    T, smooth = 6, 5
    a, b = _bank(model, 7, T, smooth), _bank(model, 9, T, smooth)
    pool = _synthetic_rows(golden, "pocket", 7 * 12, 6).reshape(12, 7, -1)
    other = _synthetic_rows(golden, "pocket", 9 * 19, 7).reshape(19, 9, -1)
    for t in range(4):
        _frame(a, kind, pool[t], np.arange(7))
    for t in range(11):
        _frame(b, kind, other[t], np.arange(9))
    state, warm = a.export_state([2])
    untouched = _all(b)[0]
    b.import_state([6], state, warm, a.state_desc())
    now = _all(b)[0]
    keep = np.array([s for s in range(9) if s != 6])
    assert np.array_equal(untouched[keep].view(np.uint32), now[keep].view(np.uint32))
    assert np.array_equal(now[6].view(np.uint32), state.cpu().numpy()[0].view(np.uint32))
    for t in range(4, 12):
        want = _frame(a, kind, pool[t, 2:3], [2])[0]
        rows = np.stack([other[t + 7, 1], pool[t, 2], other[t + 7, 3]])
        got = _frame(b, kind, rows, [1, 6, 3])[1]
        assert np.array_equal(got, want), t
    model.set_kernel("auto")


def test_exports_back_to_back(golden, tmp_path, monkeypatch):
    """12 exports of two of three streams, each into its own buffer, with no host synchronisation in between: the pinned descriptor
    ring the hand-over shares with the subset frames (csrc/bank_host.h) wraps, and a slot rewritten before its copy had run would
    export another call's streams.  Bit-equal to the same calls with a device synchronisation after each and to the bank's full
    export; a twin that imports the last call's records continues with the bank's bits."""
    est = _estimator(tmp_path, monkeypatch, "pocket", 8, 0.0, smooth=5, add_mc_samples=True, monte_carlo_samples=1)
    model, kind = est._hip_model(), est._parse_kind
    model.set_kernel("tile16")
    S, T, smooth = 3, 6, 5
    pool = _synthetic_rows(golden, "pocket", S * 8, 8).reshape(8, S, -1)
    a = _bank(model, S, T, smooth)
    for t in range(7):                                      # every stream at a ring phase of its own
        _frame(a, kind, pool[t, _schedule(S, t)], _schedule(S, t))
    pairs = [[t % S, (t + 1 + t // S % 2) % S] for t in range(12)]

    def run(sync):
        torch.cuda.synchronize()
        res = []
        for p in pairs:
            res.append(a.export_state(p))
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return [(state.cpu().numpy(), warm.copy()) for state, warm in res]

    queued, synced = run(False), run(True)
    whole, warm_all = _all(a)
    for p, (sq, wq), (ss, ws) in zip(pairs, queued, synced):
        assert np.array_equal(sq.view(np.uint32), ss.view(np.uint32)) and np.array_equal(wq, ws), p
        assert np.array_equal(sq.view(np.uint32), whole[p].view(np.uint32)) and np.array_equal(wq, warm_all[p]), p
    b = _bank(model, S, T, smooth)
    b.import_state(pairs[-1], queued[-1][0], queued[-1][1], a.state_desc())
    rows = pool[7, pairs[-1]]
    assert np.array_equal(_frame(a, kind, rows, pairs[-1]), _frame(b, kind, rows, pairs[-1]))
    model.set_kernel("auto")


def test_cold_and_half_warm_streams(golden, tmp_path, monkeypatch):
    est = _estimator(tmp_path, monkeypatch, "pocket", 5, 0.0, smooth=5, add_mc_samples=True, monte_carlo_samples=1)
    model, kind = est._hip_model(), est._parse_kind
    model.set_kernel("tile16")
    T, smooth = 6, 5
    pool = _synthetic_rows(golden, "pocket", 60, 8).reshape(12, 5, -1)
    b = _bank(model, 5, T, smooth)
    for t in range(7):
        _frame(b, kind, pool[t], np.arange(5))
    # a never-fed stream: no warm bit, and the import is a cold start of the target
    fresh = _bank(model, 3, T, smooth)
    state, warm = fresh.export_state([1])
    assert warm.tolist() == [0] and not state.cpu().numpy().any()
    b.import_state([4], state, warm)
    want = _frame(fresh, kind, pool[7, 0:1], [1])[0]
    got = _frame(b, kind, pool[7, 0:2], [4, 2])[0]
    assert np.array_equal(got, want)
    # a lockstep bank between push_rows and step: the window is warm, the stack is not
    lock = _bank(model, 3, T, smooth)
    lock.push_rows(torch.from_numpy(pool[8, :3].copy()).cuda(), kind)
    state, warm = lock.export_state([1])
    assert warm.tolist() == [1]
    assert np.array_equal(state.cpu().numpy()[0, :T * 22].reshape(T, 22), np.tile(state.cpu().numpy()[0, :22], (T, 1)))
    assert not state.cpu().numpy()[0, T * 22:].any()
    b.import_state([0], state, warm)
    # uninterrupted: the next row, then the first prediction -- its window is [first row x 5, next row], and it fills the whole stack
    lock.push_rows(torch.from_numpy(pool[9, :3].copy()).cuda(), kind)
    want = lock.step().cpu().numpy()[1]
    got = _frame(b, kind, pool[9, 1:2], [0])[0]
    assert np.array_equal(got, want)
    model.set_kernel("auto")


def test_export_from_a_lockstep_bank(golden, tmp_path, monkeypatch):
    est = _estimator(tmp_path, monkeypatch, "pocket", 6, 0.0, smooth=5, add_mc_samples=True, monte_carlo_samples=1)
    model, kind = est._hip_model(), est._parse_kind
    model.set_kernel("tile16")
    S, T, smooth = 4, 6, 5
    pool = _synthetic_rows(golden, "pocket", S * 12, 9).reshape(12, S, -1)
    lock, sub = _bank(model, S, T, smooth), _bank(model, 6, T, smooth)
    for t in range(8):
        lock.push_rows(torch.from_numpy(pool[t].copy()).cuda(), kind)
        lock.step()
    state, warm = lock.export_state([3, 1])
    assert warm.tolist() == [3, 3]
    sub.import_state([0, 5], state, warm, lock.state_desc())
    for t in range(8, 12):                                   # the lockstep bank was only read: it carries on in lockstep
        lock.push_rows(torch.from_numpy(pool[t].copy()).cuda(), kind)
        want = lock.step().cpu().numpy()
        got = _frame(sub, kind, pool[t, [3, 1]], [0, 5])
        assert np.array_equal(got, want[[3, 1]]), t
    model.set_kernel("auto")


def test_monte_carlo_stream_takes_the_new_banks_draws(golden, tmp_path, monkeypatch):
    est = _estimator(tmp_path, monkeypatch, "pocket", 7, 0.2, smooth=3, add_mc_samples=True, monte_carlo_samples=3)
    model, kind = est._hip_model(), est._parse_kind
    model.set_kernel("tile16")
    S, T, smooth, mc = 4, 6, 3, 3
    kw = dict(monte_carlo_samples=mc, dropout=0.2, seed=99)
    a, b = _bank(model, S, T, smooth, **kw), _bank(model, S, T, smooth, **kw)
    pool = _synthetic_rows(golden, "pocket", S * 6, 11).reshape(6, S, -1)
    alt = _synthetic_rows(golden, "pocket", 5, 12)
    streams = [2, 0, 3]                                       # list position 1 = stream 0
    for t in range(5):
        rows = pool[t, streams]
        last_a = _frame(a, kind, rows, streams, datagrams=True)
        rows_b = rows.copy()
        rows_b[1] = alt[t]
        last_b = _frame(b, kind, rows_b, streams, datagrams=True)
    assert np.array_equal(last_a[[0, 2]], last_b[[0, 2]]) and np.abs(last_a[1] - last_b[1]).max() > 1e-4   # only that stream differs
    assert a.state_desc()["n_mc"] == mc
    state, warm = a.export_state([0])
    b.import_state([0], state, warm)
    want = _frame(a, kind, pool[5, streams], streams, datagrams=True)
    got = _frame(b, kind, pool[5, streams], streams, datagrams=True)
    assert want.shape == (3, 25 + 6 * smooth * mc)
    assert np.array_equal(got, want)                          # same bank position (seed, call counter), same list position, same state
    tail = want[1, 25:].reshape(smooth * mc, 6)
    assert np.std(tail[-mc:], axis=0).max() > 1e-3            # dropout is really on: the newest frame's samples differ
    model.set_kernel("auto")


def test_round_trip_monte_carlo_bank(golden, tmp_path, monkeypatch):
    est = _estimator(tmp_path, monkeypatch, "pocket", 15, 0.2, smooth=3, add_mc_samples=True, monte_carlo_samples=3)
    model, kind = est._hip_model(), est._parse_kind
    model.set_kernel("tile16")
    S = 5
    pool = _synthetic_rows(golden, "pocket", S * 10, 22).reshape(10, S, -1)
    _round_trip(lambda: _bank(model, S, 6, 3, monte_carlo_samples=3, dropout=0.2, seed=5), kind, pool, S, [4, 1], (3, 8), 10)
    model.set_kernel("auto")


@pytest.mark.parametrize("case", ["ff", "imupose", "watch"])
def test_round_trip_other_regressors(golden, tmp_path, monkeypatch, case):
    if case == "watch":
        est = _estimator(tmp_path, monkeypatch, "watch", 8, 0.0, smooth=5, add_mc_samples=True, monte_carlo_samples=1)
        name, T, kw = "watch", 8, {}
    else:
        from tests.test_regressor_banks_gpu import estimator
        est = estimator(tmp_path, monkeypatch, case, "pocket", seed=3, dropout=0.0, smooth=5, add_mc_samples=True, monte_carlo_samples=1)
        name, T, kw = "pocket", 6, dict(monte_carlo_samples=4, dropout=0.0)
    model, kind = est._hip_model(), est._parse_kind
    if case == "watch":
        model.set_kernel("tile16")
    S, smooth = 5, 5
    pool = _synthetic_rows(golden, name, S * 12, 13).reshape(12, S, -1)
    make = lambda: _bank(model, S, T, smooth, **kw)            # noqa: E731
    d = make().state_desc()
    assert d["T"] == (1 if case == "ff" else T)               # DropoutFF keeps the newest row only
    assert d["n_mc"] == (4 if case == "ff" else 1)            # ImuPoseLSTM ignores the sample count
    _round_trip(make, kind, pool, S, [4, 1], (3, 8, 11), 12)
    if case == "watch":
        model.set_kernel("auto")


def _fk_bank(S):
    from wear_mocap_ape_amd.streams import FkStreamBank
    return FkStreamBank(S, smooth=5, dtype=torch.float64)


def test_fk_only_bank_round_trip_and_migration(golden):
    pool = _synthetic_rows(golden, "uarm", 5 * 15, 14).reshape(15, 5, -1)
    a, twin = _fk_bank(5), _fk_bank(5)
    desc = a.state_desc()
    assert desc == {"version": 1, "T": 0, "I": 0, "smooth": 5, "n_mc": 1, "O": 8, "words_per_stream": 80}
    listed, rest = [4, 0, 2], [1, 3]
    for t in range(15):
        streams = _schedule(5, t)
        got = a.frame(pool[t, streams], streams).cpu().numpy().copy()
        want = twin.frame(pool[t, streams], streams).cpu().numpy().copy()
        assert np.array_equal(got, want), t
        if t + 1 in (4, 7, 13):
            before = a.export_state(np.arange(5))[0].cpu().numpy().copy()
            state, warm = a.export_state(listed)
            assert warm.tolist() == [3, 3, 3]
            a.reset(streams=listed)
            assert a.export_state(listed)[1].tolist() == [0, 0, 0]
            a.import_state(listed, state, warm, desc)
            after = a.export_state(np.arange(5))[0].cpu().numpy().copy()
            assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
            assert np.array_equal(before[rest].view(np.uint32), twin.export_state(rest)[0].cpu().numpy().view(np.uint32))
    # migration: stream 2 of a bank of 5 after 4 frames into stream 6 of a bank of 8 that has run 11 frames on other rows
    src, dst = _fk_bank(5), _fk_bank(8)
    other = _synthetic_rows(golden, "uarm", 8 * 19, 15).reshape(19, 8, -1)
    for t in range(4):
        src.step_rows(pool[t])
    for t in range(11):
        dst.step_rows(other[t])
    state, warm = src.export_state([2])
    dst.import_state([6], state, warm, src.state_desc())
    for t in range(4, 12):
        want = src.frame(pool[t, 2:3], [2]).cpu().numpy()[0].copy()
        got = dst.frame(np.stack([other[t + 7, 1], pool[t, 2]]), [1, 6]).cpu().numpy()[1].copy()
        assert np.array_equal(got, want), t
    # a never-fed stream exports cold and imports as a cold start
    state, warm = _fk_bank(2).export_state([1])
    assert warm.tolist() == [0]
    dst.import_state([6], state, warm)
    fresh = _fk_bank(1)
    assert np.array_equal(dst.frame(pool[12, 0:1], [6]).cpu().numpy(), fresh.frame(pool[12, 0:1], [0]).cpu().numpy())


def test_refusals_leave_the_bank_unchanged(golden, tmp_path, monkeypatch):
    from wear_mocap_ape_amd.streams import FkStreamBank
    est = _estimator(tmp_path, monkeypatch, "pocket", 9, 0.0, smooth=5, add_mc_samples=True, monte_carlo_samples=1)
    model, kind = est._hip_model(), est._parse_kind
    model.set_kernel("tile16")
    S, T, smooth = 4, 6, 5
    pool = _synthetic_rows(golden, "pocket", S * 6, 16).reshape(6, S, -1)
    bank, twin = _bank(model, S, T, smooth), _bank(model, S, T, smooth)
    for t in range(5):
        _frame(bank, kind, pool[t], np.arange(S))
        _frame(twin, kind, pool[t], np.arange(S))
    state, warm = bank.export_state([1, 2])
    junk = torch.full_like(state, 7.0)
    desc = bank.state_desc()
    with pytest.raises(UserWarning):                         # another T
        bank.import_state([1, 2], junk, warm, dict(desc, T=T + 1))
    with pytest.raises(UserWarning):                         # another n_mc
        bank.import_state([1, 2], junk, warm, dict(desc, n_mc=2))
    with pytest.raises(UserWarning):                         # a duplicate stream
        bank.import_state([1, 1], junk, warm)
    with pytest.raises(UserWarning):                         # K > S
        bank.import_state(np.arange(S + 1), torch.zeros((S + 1, desc["words_per_stream"]), device="cuda"), np.zeros(S + 1, np.uint8))
    with pytest.raises(UserWarning):
        bank.export_state([0, S])
    # the same checks in the library itself, behind the Python ones
    import ctypes as C
    from wear_mocap_ape_amd import _hip
    idx, w2 = np.array([1, 1], dtype=np.int32), np.array([3, 3], dtype=np.uint8)
    d = _hip.ApeStreamStateDesc(*[desc[k] for k in ("version", "T", "I", "smooth", "n_mc", "O", "words_per_stream")])
    rc = _hip.lib().ape_streams_import(bank._handle, C.byref(d), C.c_void_p(idx.ctypes.data), 2, C.c_void_p(junk.data_ptr()),
                                       C.c_void_p(w2.ctypes.data), None)
    assert rc != 0 and b"twice" in _hip.lib().ape_last_error()
    idx = np.arange(S + 1, dtype=np.int32)
    rc = _hip.lib().ape_streams_import(bank._handle, C.byref(d), C.c_void_p(idx.ctypes.data), S + 1, C.c_void_p(junk.data_ptr()),
                                       C.c_void_p(w2.ctypes.data), None)
    assert rc != 0 and b"K=" in _hip.lib().ape_last_error()
    fk = FkStreamBank(3, smooth=5, dtype=torch.float64)
    with pytest.raises(UserWarning):
        fk.import_state([0], torch.zeros((1, 80), device="cuda"), np.array([3], np.uint8), dict(fk.state_desc(), smooth=4))
    with pytest.raises(UserWarning):
        fk.import_state([0], torch.zeros((1, 80), device="cuda"), np.array([3], np.uint8), desc)
    assert np.array_equal(_frame(bank, kind, pool[5], np.arange(S)), _frame(twin, kind, pool[5], np.arange(S)))
    model.set_kernel("auto")


def test_estimator_hands_over_to_a_bank_and_back(golden, tmp_path, monkeypatch):
    """12 ``process_row`` frames on an estimator, its state into stream 4 of a bank, 8 more rows there: the rows ``process_row`` returns
    when it simply continues; then the bank's stream back into a fresh estimator"""
    from wear_mocap_ape_amd import stream_state as ss
    kw = dict(smooth=5, add_mc_samples=True, monte_carlo_samples=1)
    est = _estimator(tmp_path, monkeypatch, "pocket", 10, 0.0, **kw)
    model, kind = est._hip_model(), est._parse_kind
    model.set_kernel("tile16")
    est.msg_as_array = True
    rows = _synthetic_rows(golden, "pocket", 24, 17)
    assert est._frame_runner() is not None
    est.reset()
    for r in rows[:12]:
        est.process_row(array("f", r.tolist()))
    state = est.get_state()
    assert state["form"] == "device" and state["warm"] == 3 and state["window"].shape == (est.sequence_len, 22)
    desc, rec, warm = est.state_record(state)
    bank = _bank(model, 6, est.sequence_len, 5)
    assert desc == bank.state_desc()
    bank.import_state([4], rec, warm, desc)
    want = np.array([est.process_row(array("f", r.tolist())) for r in rows[12:20]])
    got = np.array([bank.frame(r[np.newaxis], [4], kind, datagrams=True).cpu().numpy()[0] for r in rows[12:20]])
    assert want.shape == got.shape
    # process_row's host frame (ape_streams_frame_host) is not a launch that set_kernel pins: the messages' tolerance under "auto" ...
    print("process_row (host frame) against the bank, max diff", float(np.abs(want - got).max()))
    assert np.abs(want - got).max() <= 5e-6
    # ... and bit for bit where both sides are subset frames: a fresh estimator continued from the same state
    est3 = _estimator(tmp_path, monkeypatch, "pocket", 10, 0.0, **kw)
    est3._hip_model().set_kernel("tile16")
    est3.msg_as_array = True
    est3.set_state(state)
    same = np.array([est3.process_row(array("f", r.tolist())) for r in rows[12:20]])
    assert np.array_equal(same.astype(np.float32), got)
    with pytest.raises(UserWarning):                         # another split of the same number of words is refused
        est3.set_state(dict(state, window=state["window"].reshape(22, 6)))
    # ... and back: the bank's stream continues in a fresh estimator (set_state: its frames then run as subset frames, the same bits)
    st, w = bank.export_state([4])
    window, stack = ss.unpack(st.cpu().numpy()[0], desc)
    est2 = _estimator(tmp_path, monkeypatch, "pocket", 10, 0.0, **kw)
    est2._hip_model().set_kernel("tile16")
    est2.msg_as_array = True
    est2.set_state({"desc": desc, "window": window, "stack": stack, "warm": int(w[0]), "form": "device"})
    back = np.array([est2.process_row(array("f", r.tolist())) for r in rows[20:24]])
    cont = np.array([bank.frame(r[np.newaxis], [4], kind, datagrams=True).cpu().numpy()[0] for r in rows[20:24]])
    assert np.array_equal(back.astype(np.float32), cont)
    model.set_kernel("auto")


# ---------------- resumable replay (ape_replay_resume) ------------------------------------------------------------------------------
def _chained(est, rows, cuts, n_mc, **kw):
    """one recording replayed over [cuts[i], cuts[i+1]) with each call's state chained into the next -> the rows, the last state"""
    outs, state, warm = [], None, None
    for a, b in zip(cuts[:-1], cuts[1:]):
        out, (state, warm) = est.process_recording(rows[a:b], state_in=state, warm_in=warm, return_state=True, sample_row_base=a * n_mc, **kw)
        assert warm.tolist() == [3]
        outs.append(out.cpu().numpy())
    return np.concatenate(outs), state, warm


@pytest.mark.parametrize("mc", [1, 4])
def test_chunked_replay_equals_the_one_call(golden, tmp_path, monkeypatch, mc):
    est = _estimator(tmp_path, monkeypatch, "pocket", 11, 0.2 if mc > 1 else 0.0, smooth=2, add_mc_samples=True, monte_carlo_samples=mc)
    est._hip_model().set_kernel("tile16")
    rows = _synthetic_rows(golden, "pocket", 40, 18)
    whole = est.process_recording(rows).cpu().numpy()
    cuts = [0, 1, 7, 23, 40]                                   # the first chunk is shorter than both T and smooth
    got, state, _ = _chained(est, rows, cuts, mc)
    assert got.shape == whole.shape and np.array_equal(got, whole)
    if mc > 1:
        tail = whole[:, 25:].reshape(40, 2 * mc, 6)
        assert np.std(tail[:, -mc:], axis=1).max() > 1e-3      # dropout is really on
    # the internal chunking crossing the external one
    got64, state64, _ = _chained(est, rows, cuts, mc, max_rows_per_launch=64 if mc > 1 else 16)
    assert np.array_equal(got64, whole) and torch.equal(state64, state)
    # the last state is the recording's last T rows and last `smooth` predictions
    from wear_mocap_ape_amd import stream_state as ss
    T = est.sequence_len
    window, stack = ss.unpack(state.cpu().numpy()[0], ss.make_desc(T, 22, 2, mc, 14))
    xx = est.parse_rows(rows).cpu().numpy()
    assert np.array_equal(window, xx[40 - T:])
    _, y = est.process_recording(rows, return_targets=True)
    assert np.array_equal(stack, y.cpu().numpy()[38:])
    est._hip_model().set_kernel("auto")


def test_chunked_replay_of_three_recordings(golden, tmp_path, monkeypatch):
    est = _estimator(tmp_path, monkeypatch, "pocket", 12, 0.0, smooth=2, add_mc_samples=True, monte_carlo_samples=1)
    est._hip_model().set_kernel("tile16")
    rows = _synthetic_rows(golden, "pocket", 40, 19)
    whole = est.process_recording(rows, starts=[0, 17, 18]).cpu().numpy()
    # split at row 20: all three recordings have rows in the first call, only the third in the second (the others are not listed)
    first, (state, warm) = est.process_recording(rows[:20], starts=[0, 17, 18], return_state=True)
    assert warm.tolist() == [3, 3, 3]
    second = est.process_recording(rows[20:], state_in=state[2:3], warm_in=warm[2:3])
    assert np.array_equal(np.concatenate([first.cpu().numpy(), second.cpu().numpy()]), whole)
    # the carried records are those of one-recording replays: recording 1 has one row, its window is that row T times
    one, (s1, _) = est.process_recording(rows[17:18], return_state=True)
    assert torch.equal(s1[0], state[1]) and np.array_equal(one.cpu().numpy(), whole[17:18])
    est._hip_model().set_kernel("auto")


def test_replay_to_bank_and_bank_to_replay(golden, tmp_path, monkeypatch):
    est = _estimator(tmp_path, monkeypatch, "pocket", 13, 0.0, smooth=5, add_mc_samples=True, monte_carlo_samples=1)
    model, kind = est._hip_model(), est._parse_kind
    model.set_kernel("tile16")
    rows = _synthetic_rows(golden, "pocket", 20, 20)
    whole = est.process_recording(rows).cpu().numpy()
    _, (state, warm) = est.process_recording(rows[:12], return_state=True)
    bank = _bank(model, 6, est.sequence_len, 5)
    bank.import_state([4], state, warm)
    # the payload both sides send (float32 datagrams) bit for bit; in float64 the bank's post-filter and the replay's message kernel are
    # different kernels that agree to the bound tests/test_streams_subset.py holds this pair to under tile16 (1e-12)
    whole32 = est.process_recording(rows, out_dtype=torch.float32).cpu().numpy()
    got32 = np.array([bank.frame(r[np.newaxis], [4], kind, datagrams=True).cpu().numpy()[0] for r in rows[12:]])
    print("replay -> bank, float32 payload max diff", float(np.abs(got32 - whole32[12:]).max()))
    assert np.array_equal(got32, whole32[12:])
    st64, w64 = bank.export_state([4])
    bank64 = _bank(model, 6, est.sequence_len, 5)
    bank64.import_state([4], state, warm)
    got = np.array([bank64.frame(r[np.newaxis], [4], kind).cpu().numpy()[0] for r in rows[12:]])    # float64 [25]
    print("replay -> bank, float64 max diff", float(np.abs(got - whole[12:, :25]).max()))
    assert np.abs(got - whole[12:, :25]).max() <= 1e-12
    assert torch.equal(bank64.export_state([4])[0], st64)
    # the reverse: 12 process_row frames, then the replay continues from the estimator's state
    est.msg_as_array = True
    est.reset()
    for r in rows[:12]:
        est.process_row(array("f", r.tolist()))
    desc, rec, w = est.state_record(est.get_state())
    cont = est.process_recording(rows[12:], state_in=rec, warm_in=w).cpu().numpy()
    live = np.array([est.process_row(array("f", r.tolist())) for r in rows[12:]])
    # (process_row's host frame is not a launch that set_kernel pins: the tolerance of the messages under "auto")
    print("process_row (host frame) against the resumed replay, max diff", float(np.abs(cont - live).max()))
    assert np.abs(cont - live).max() <= 5e-6
    # ... and bit for bit against the bank that took the same record
    bank2 = _bank(model, 2, est.sequence_len, 5)
    bank2.import_state([1], rec, w, desc)
    got2 = np.array([bank2.frame(r[np.newaxis], [1], kind, datagrams=True).cpu().numpy()[0] for r in rows[12:]])
    print("bank -> replay, float64 max diff", float(np.abs(got2 - cont).max()))
    assert np.array_equal(got2, cont.astype(np.float32))
    model.set_kernel("auto")


def test_existing_replay_entries_equal_the_new_entry_without_states(golden, tmp_path, monkeypatch):
    import ctypes as C
    from wear_mocap_ape_amd import _hip
    est = _estimator(tmp_path, monkeypatch, "pocket", 14, 0.2, smooth=3, add_mc_samples=True, monte_carlo_samples=4)
    model = est._hip_model()
    model.set_kernel("tile16")
    rows = _synthetic_rows(golden, "pocket", 30, 21)
    old = est.process_recording(rows, starts=[0, 11])                      # all-default new arguments: ape_replay_bodies
    rd = torch.from_numpy(rows).cuda()
    st = np.array([0, 11], dtype=np.int32)

    def call(entry, *extra):
        out = torch.empty((30, 25 + 6 * 12), dtype=torch.float64, device="cuda")
        _hip.check(getattr(_hip.lib(), entry)(model.handle, est._parse_kind, C.c_void_p(rd.data_ptr()), 30, C.c_void_p(st.ctypes.data), 2,
                                              est.sequence_len, 3, 4, float(model.dropout), 0x5EED,
                                              _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG, C.c_void_p(out.data_ptr()), _hip.F64, None, 0,
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream), None, *extra), entry)
        return out
    direct = call("ape_replay_bodies")
    new = call("ape_replay_resume", None, None, None, None, 0)
    assert torch.equal(old, direct) and torch.equal(direct, new)
    # cold records (no warm bit) are the cold start too
    words = 6 * 22 + 3 * 4 * 14
    cold = call("ape_replay_resume", C.c_void_p(torch.zeros((2, words), device="cuda").data_ptr()),
                C.c_void_p(np.zeros(2, np.uint8).ctypes.data), None, None, 0)
    assert torch.equal(cold, new)
    model.set_kernel("auto")
