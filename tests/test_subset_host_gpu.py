"""Host subset frames on the GPU (``ape_*_frame_subset_host`` / ``*.frame_host`` / ``streams.tick``).

The host entry runs the device subset frame's kernels on the same arithmetic, so twin banks -- one seed, one schedule, one fed by
``frame()`` from device rows, the other by ``frame_host()`` -- must agree in every BIT of every output row and of the exported states
(tolerance zero).  Against the reference's own traces the tolerances are the ones the existing trace tests apply: 5e-6 for the NN
bank (tests/test_replay.py::test_replay_reference_traces and the "auto" legs of tests/test_streams_subset.py), 1e-5 for the FK bank
(tests/test_fk_only_gpu.py::test_process_row_against_reference).  The recovery branch is staged like tests/hooks/poke_cases.py stages
it for ``ape_streams_frame_host`` and runs in a child process on the test-hooks library (tests/hooks/subset_host_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests.conftest import GOLDEN
from tests.test_replay import _estimator, _synthetic_rows

pytestmark = pytest.mark.gpu

S7 = 7
KS = (7, 3, 1, 7, 7, 3, 7, 1, 7, 7, 3, 7)          # 12 frames, K from {1, 3, 7}: every stream gets at least seven rows


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert _bits(a) == _bits(b), (what, float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))))


def _host(x):
    if isinstance(x, tuple):
        return tuple(_host(v) for v in x)
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _states_equal(dev, host, S, what):
    (sa, wa), (sb, wb) = dev.export_state(np.arange(S)), host.export_state(np.arange(S))
    _same(sa.cpu().numpy(), sb.cpu().numpy(), what + " states")
    _same(wa, wb, what + " warm / age")


def _twin_schedule(dev, host, S, pool, frame_dev, frame_host, big_endian, seed, what):
    """12 frames on both banks: K from KS, scrambled lists, a reset of stream 2 in the middle, set_bodies on two streams"""
    rng = np.random.default_rng(seed)
    used = 0
    for t, K in enumerate(KS):
        K = min(K, S)
        if t == 4:
            bodies = np.tile(np.asarray(orc.DEFAULT_BODY, dtype=np.float64), (2, 1)) * np.array([[1.1], [0.9]])
            for b in (dev, host):
                b.set_bodies(bodies, streams=[1, 5])
        if t == 6:
            for b in (dev, host):
                b.reset(streams=[2])
        streams = rng.permutation(S)[:K]
        rows = pool[used:used + K]
        used += K
        sent = np.ascontiguousarray(rows.byteswap() if big_endian else rows)
        a = _host(frame_dev(dev, torch.from_numpy(sent).cuda(), streams))
        b = _host(frame_host(host, sent, streams))
        if isinstance(a, tuple):
            for i, (x, y) in enumerate(zip(a, b)):
                _same(x, y, f"{what} frame {t} part {i}")
        else:
            _same(a, b, f"{what} frame {t}")
            assert np.all(np.isfinite(a)), (what, t)
    _states_equal(dev, host, S, what)


# ---------------- 1. bit-equality with the device subset frame -------------------------------------------------------------------------------
@pytest.mark.parametrize("case,big_endian", [("det", False), ("mc_packed", True), ("mc_packed_spread", False)])
def test_lstm_bank_twins(golden, tmp_path, monkeypatch, case, big_endian):
    from wear_mocap_ape_amd.streams import StreamBank
    mc = case != "det"
    est = _estimator(tmp_path, monkeypatch, "pocket", 3, 0.2 if mc else 0.0, smooth=1, add_mc_samples=True, monte_carlo_samples=1)
    model, kind = est._hip_model(), est._parse_kind
    kw = dict(smooth=2, monte_carlo_samples=3, dropout=0.2, seed=77) if mc else dict(smooth=1)
    dev, host = (StreamBank(model, S7, 6, normalize=True, dtype=torch.float64, **kw) for _ in range(2))
    opt = dict(datagrams=mc, spread=case.endswith("spread"), big_endian=big_endian)
    pool = _synthetic_rows(golden, "pocket", sum(KS), 5)

    def frame_dev(b, rows, streams):
        out = b.frame(rows, streams, kind, **opt).clone()
        b.recover()
        return out
    _twin_schedule(dev, host, S7, pool, frame_dev, lambda b, rows, streams: b.frame_host(rows, streams, kind, **opt), big_endian, 1, case)
    n = 2 * 3
    want_w = (25 + 6 * n if mc else 25) + (21 if opt["spread"] else 0)
    out = host.frame_host(pool[:2], [0, 1], kind, **opt)
    assert out.shape == (2, want_w) and out.dtype == (np.float32 if mc else np.float64)
    assert host.frame_host(pool[:0], [], kind, **opt).shape == (0, want_w)          # K = 0: a no-op


@pytest.mark.parametrize("model_name,big_endian", [("ff", False), ("imupose", True)])
def test_regressor_bank_twins(golden, tmp_path, monkeypatch, model_name, big_endian):
    from wear_mocap_ape_amd.streams import StreamBank
    from tests.test_regressor_banks_gpu import estimator
    smooth, mc = 3, 3                                                               # the sizes of tests/test_regressor_banks_gpu.py
    est = estimator(tmp_path, monkeypatch, model_name, "pocket", smooth=smooth, add_mc_samples=True, monte_carlo_samples=mc)
    m, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    dev, host = (StreamBank(m, S7, T, smooth=smooth, normalize=True, dtype=torch.float64, monte_carlo_samples=mc, dropout=0.2, seed=5)
                 for _ in range(2))
    pool = _synthetic_rows(golden, "pocket", sum(KS), 6)
    opt = dict(datagrams=True, big_endian=big_endian)

    def frame_dev(b, rows, streams):
        out = b.frame(rows, streams, kind, **opt).clone()
        b.recover()
        return out
    _twin_schedule(dev, host, S7, pool, frame_dev, lambda b, rows, streams: b.frame_host(rows, streams, kind, **opt), big_endian, 2, model_name)


@pytest.mark.parametrize("big_endian", [False, True])
def test_fk_bank_twins(big_endian):
    from wear_mocap_ape_amd.streams import FkStreamBank
    from tests.test_fk_only_gpu import _random_rows
    dev, host = (FkStreamBank(S7, smooth=5, dtype=torch.float64) for _ in range(2))
    pool = _random_rows(np.random.default_rng(3), sum(KS))
    _twin_schedule(dev, host, S7, pool, lambda b, rows, streams: b.frame(rows, streams, big_endian=big_endian).clone(),
                   lambda b, rows, streams: b.frame_host(rows, streams, big_endian=big_endian), big_endian, 3, "fk")
    # lockstep and subset frames mix freely on this bank: a lockstep frame on both, then one more host frame against the device's
    rows = _random_rows(np.random.default_rng(4), S7 + 3)
    _same(dev.step_rows(rows[:S7]).cpu().numpy(), host.step_rows(rows[:S7]).cpu().numpy(), "fk lockstep")
    _same(dev.frame(rows[S7:], [6, 0, 3]).cpu().numpy(), host.frame_host(rows[S7:], [6, 0, 3]), "fk after lockstep")


@pytest.mark.parametrize("big_endian", [False, True])
def test_kalman_bank_twins(norm_stats, big_endian):
    from tests.test_kalman import make_model
    from tests.test_kalman_bank_gpu import make_bank, make_rows, pocket_stats
    E, W = 16, 4                                                                    # a size of tests/test_kalman_bank_gpu.py; W + 1 = 5 < 7 rows
    m, _ = make_model(E, W, 22)
    dev, host = (make_bank(m, S7, 2, pocket_stats(norm_stats), seed=99) for _ in range(2))
    pool = make_rows(np.random.default_rng(9), sum(KS))
    opt = dict(datagrams=True, spread=True, big_endian=big_endian)

    def frame_dev(b, rows, streams):
        out, n = b.frame(rows, streams, **opt)
        return out.clone(), n.clone()
    _twin_schedule(dev, host, S7, pool, frame_dev, lambda b, rows, streams: b.frame_host(rows, streams, **opt), big_endian, 4, "kalman")
    out, n = host.frame_host(pool[:S7], np.arange(S7), **opt)
    assert out.shape == (S7, 25 + 6 * 2 * E + 21) and n.dtype == np.int32 and n.max() == 2 * E     # past the W + 1 boundary
    assert host.get_draw_position() == (dev.get_draw_position()[0], dev.get_draw_position()[1] + 1)   # one call, one key
    dev.check()


# ---------------- 2. / 3. against the reference's own traces ---------------------------------------------------------------------------------
def _staggered(n_rows, n_streams=3):
    """tick -> [(stream, index of its next trace row)]: stream j begins j ticks late and is not listed on every (j + 2)-th tick"""
    nxt = [0] * n_streams
    t = 0
    while min(nxt) < n_rows:
        listed = []
        for j in range(n_streams):
            if t >= j and (t - j + 1) % (j + 2) != 0 and nxt[j] < n_rows:
                listed.append((j, nxt[j]))
                nxt[j] += 1
        yield listed
        t += 1


def test_lstm_bank_against_the_reference_trace(golden, tmp_path, monkeypatch):
    from wear_mocap_ape_amd.streams import StreamBank
    g = golden("stream_trace_pocket.npz")
    rows = g["rows"].astype(np.float32)
    for smooth in (1, 5):
        est = _estimator(tmp_path, monkeypatch, "pocket", int(g["weights_seed"]), 0.0, smooth=smooth, add_mc_samples=True,
                         monte_carlo_samples=1)
        ref = g[f"msg_s{smooth}_mc1"]
        bank = StreamBank(est._hip_model(), 3, est.sequence_len, smooth=smooth, normalize=True, dtype=torch.float32)
        seen, worst = [0, 0, 0], 0.0
        for listed in _staggered(len(rows)):
            if not listed:
                continue
            streams = [j for j, _ in listed][::-1]                                  # (list order is free)
            idx = [k for _, k in listed][::-1]
            out = bank.frame_host(rows[idx], streams, est._parse_kind, datagrams=True)
            assert out.shape[1] == ref.shape[1]
            for o, j, k in zip(out, streams, idx):
                worst = max(worst, float(np.abs(o - ref[k]).max()))
                seen[j] += 1
        print(f"smooth {smooth}: max |frame_host - reference trace| = {worst:.3e}")
        assert seen == [len(rows)] * 3
        assert worst < 5e-6, (smooth, worst)


def test_fk_bank_against_the_reference_trace():
    from wear_mocap_ape_amd.streams import FkStreamBank
    t = np.load(GOLDEN / "fk_only_trace.npz")
    n = int(t["lengths"][0])                                                       # the first recording: one cold start per stream
    rows, want = t["rows"][:n].astype(np.float32), t["msg_s5"][:n]
    bank = FkStreamBank(3, smooth=5, dtype=torch.float64)
    seen, worst = [0, 0, 0], 0.0
    for listed in _staggered(n):
        if not listed:
            continue
        streams, idx = [j for j, _ in listed], [k for _, k in listed]
        out = bank.frame_host(rows[idx], streams)
        for o, j, k in zip(out, streams, idx):
            np.testing.assert_array_equal(np.isnan(o), np.isnan(want[k]))
            if not np.isnan(want[k]).all():
                worst = max(worst, float(np.nanmax(np.abs(o - want[k]))))
            seen[j] += 1
    print(f"max |frame_host - reference trace| = {worst:.3e}")
    assert seen == [n] * 3 and worst < 1e-5, (seen, worst)


# ---------------- 4. both completion paths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 65])
def test_completion_words_and_stream_wait(golden, tmp_path, monkeypatch, S):
    from wear_mocap_ape_amd.streams import StreamBank
    est = _estimator(tmp_path, monkeypatch, "pocket", 4, 0.0, smooth=3, add_mc_samples=True, monte_carlo_samples=1)
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    dev, host = (StreamBank(model, S, T, smooth=3, normalize=True, dtype=torch.float64) for _ in range(2))
    pool = _synthetic_rows(golden, "pocket", 4 * S, 8)
    rng = np.random.default_rng(S)
    host.frame_stats(reset=True)
    for t in range(4):
        streams = rng.permutation(S)
        rows = pool[t * S:(t + 1) * S]
        want = dev.frame(rows, streams, kind, datagrams=True).cpu().numpy()
        dev.recover()
        _same(want, host.frame_host(rows, streams, kind, datagrams=True), f"S {S} frame {t}")
    st = host.frame_stats()
    print({k: (v if np.isscalar(v) else np.round(v, 1).tolist()) for k, v in st.items()})
    assert st["frames"] == 4 and st["recovered"] == 0 and len(st["wait_us"]) == 4
    # S = 64: every frame was taken at its completion words.  S = 65: vacuous -- a frame without words cannot miss them, the counter only
    # moves on the words path; the stream-wait path cannot be told apart through the ABI, its check is the bit-equality above
    assert st["fallback_syncs"] == 0
    # a short list on the larger bank is back on the words
    _same(dev.frame(pool[:5], [S - 1, 3, 1, 0, 9], kind).cpu().numpy(), host.frame_host(pool[:5], [S - 1, 3, 1, 0, 9], kind), "short list")
    dev.recover()
    assert host.frame_stats()["fallback_syncs"] == 0


# ---------------- 5. untouched streams ---------------------------------------------------------------------------------------------------------
def test_unlisted_streams_keep_their_bits(golden, tmp_path, monkeypatch, norm_stats):
    from wear_mocap_ape_amd.streams import FkStreamBank, StreamBank
    from tests.test_fk_only_gpu import _random_rows
    from tests.test_kalman import make_model
    from tests.test_kalman_bank_gpu import make_bank, make_rows, pocket_stats
    est = _estimator(tmp_path, monkeypatch, "pocket", 5, 0.0, smooth=2, add_mc_samples=True, monte_carlo_samples=1)
    kind = est._parse_kind
    nn = StreamBank(est._hip_model(), S7, 6, smooth=2, normalize=True, dtype=torch.float64)
    fk = FkStreamBank(S7, smooth=5, dtype=torch.float64)
    kb = make_bank(make_model(16, 4, 25)[0], S7, 2, pocket_stats(norm_stats))
    p_nn, p_fk, p_kb = _synthetic_rows(golden, "pocket", 20, 9), _random_rows(np.random.default_rng(5), 20), make_rows(np.random.default_rng(6), 20)
    rest = [0, 2, 3, 6]
    for bank, pool, call in ((nn, p_nn, lambda r, s: nn.frame_host(r, s, kind)), (fk, p_fk, fk.frame_host), (kb, p_kb, kb.frame_host)):
        call(pool[:S7], np.arange(S7))                                              # every stream has a history
        call(pool[S7:S7 + 4], rest)
        before = bank.export_state(rest)
        out = call(pool[12:15], [5, 1, 4])
        after = bank.export_state(rest)
        assert np.all(np.isfinite(out))
        _same(before[0].cpu().numpy(), after[0].cpu().numpy(), type(bank).__name__)
        _same(before[1], after[1], type(bank).__name__)


# ---------------- 6. mode and refusals ---------------------------------------------------------------------------------------------------------
def test_mode_rules_and_refusals(golden, tmp_path, monkeypatch):
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    lib = _hip.lib()
    S = 5
    est = _estimator(tmp_path, monkeypatch, "pocket", 6, 0.0, smooth=2, add_mc_samples=True, monte_carlo_samples=1)
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    bank, twin = (StreamBank(model, S, T, smooth=2, normalize=True, dtype=torch.float64) for _ in range(2))
    pool = _synthetic_rows(golden, "pocket", 4 * S, 10)
    _same(twin.frame_host(pool[:3], [4, 0, 2], kind), bank.frame_host(pool[:3], [4, 0, 2], kind), "first frame")
    # per-stream mode: the lockstep entries are refused with APE_ERR_NOT_READY until reset()
    rows_d = torch.from_numpy(pool[:S]).cuda()
    host_out = np.zeros((S, 25 + 12))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    not_ready = 3                                                                   # APE_ERR_NOT_READY (include/ape_hip.h)
    rc = lib.ape_streams_frame_host(bank._handle, kind, C.c_void_p(pool[:S].ctypes.data), _hip.FLAG_NORMALIZE_INPUT, C.c_void_p(host_out.ctypes.data),
                                    _hip.F64, st)
    assert rc == not_ready and b"per-stream" in lib.ape_last_error()
    rc_push = lib.ape_streams_push_rows(bank._handle, kind, C.c_void_p(rows_d.data_ptr()), st)
    assert rc_push == rc and b"per-stream" in lib.ape_last_error()
    msg = torch.empty((S, 25), dtype=torch.float64, device="cuda")
    rc_step = lib.ape_streams_step(bank._handle, _hip.FLAG_NORMALIZE_INPUT, C.c_void_p(msg.data_ptr()), None, _hip.F64, st)
    assert rc_step == rc and b"per-stream" in lib.ape_last_error()
    # refused before any launch: nothing is pushed, no counter moves
    out = np.zeros((S + 1, 25))
    wide = np.zeros((S + 1, 55), dtype=np.float32)
    wide[:S] = pool[:S]

    def call(streams, K=None, k=kind, flags=_hip.FLAG_NORMALIZE_INPUT, rows=wide):
        idx = np.ascontiguousarray(streams, dtype=np.int32)
        return lib.ape_streams_frame_subset_host(bank._handle, k, C.c_void_p(rows.ctypes.data), C.c_void_p(idx.ctypes.data),
                                                 len(idx) if K is None else K, flags, C.c_void_p(out.ctypes.data), _hip.F64, st)
    for args, word in ((dict(streams=[1, 1]), b"twice"), (dict(streams=[0, S]), b"outside"), (dict(streams=[-1]), b"outside"),
                       (dict(streams=list(range(S)) + [0], K=S + 1), b"K="), (dict(streams=[0], k=_hip.PARSE_WATCH_ONLY), b"features"),
                       (dict(streams=[0], k=0x77), b"kind"), (dict(streams=[0], flags=_hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_ALL_STEPS), b"accepted")):
        assert call(**args) != 0, args
        assert word in lib.ape_last_error(), (args, lib.ape_last_error())
    with pytest.raises(UserWarning):
        bank.frame_host(torch.from_numpy(pool[:1]).cuda(), [0], kind)                # device rows belong to frame()
    with pytest.raises(UserWarning):
        bank.frame_host(pool[:2], [0, 1, 2], kind)
    _same(twin.frame_host(pool[5:10], [3, 1, 0, 4, 2], kind), bank.frame_host(pool[5:10], [3, 1, 0, 4, 2], kind), "after the refusals")
    _states_equal(twin, bank, S, "after the refusals")
    # frame() and frame_host() share counters, rings and tables: they mix
    _same(twin.frame_host(pool[10:12], [2, 3], kind), bank.frame(pool[10:12], [2, 3], kind).cpu().numpy(), "mixed entries")
    bank.recover()
    bank.reset()                                                                    # back to lockstep
    bank.push_rows(rows_d, kind)
    assert tuple(bank.step().shape) == (S, 25)
    bank.recover()


# ---------------- 7. tick ------------------------------------------------------------------------------------------------------------------------
def test_tick_equals_rounds_and_single_stream_banks(golden, tmp_path, monkeypatch):
    from wear_mocap_ape_amd.streams import StreamBank, tick, tick_rounds
    S = 4
    est = _estimator(tmp_path, monkeypatch, "pocket", 7, 0.0, smooth=3, add_mc_samples=True, monte_carlo_samples=1)
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    model.set_kernel("tile16")                       # one kernel whatever the list length: a stream's bits do not depend on its company
    bag, by_round = (StreamBank(model, S, T, smooth=3, normalize=True, dtype=torch.float64) for _ in range(2))
    pool = _synthetic_rows(golden, "pocket", 18, 11)
    ids = np.array([3, 1, 3, 3, 1, 0, 2, 2, 3])
    got = np.concatenate([tick(bag, pool[:9], ids, kind=kind, datagrams=True), tick(bag, pool[9:], ids[::-1], kind=kind, datagrams=True)])
    assert got.shape == (18, 25 + 18) and got.dtype == np.float32
    want = np.zeros_like(got)
    for base, bag_ids in ((0, ids), (9, ids[::-1])):
        for r in tick_rounds(bag_ids)[0]:
            want[base + r] = by_round.frame_host(pool[base + r], bag_ids[r], kind, datagrams=True)
    _same(got, want, "tick against its rounds")
    all_ids = np.concatenate([ids, ids[::-1]])
    for s in range(S):                               # deterministic: every stream equals a fresh bank that saw only its rows
        one = StreamBank(model, 1, T, smooth=3, normalize=True, dtype=torch.float64)
        mine = np.flatnonzero(all_ids == s)
        ref = np.concatenate([one.frame_host(pool[i:i + 1], [0], kind, datagrams=True) for i in mine])
        _same(got[mine], ref, f"stream {s} alone")
    model.set_kernel("auto")
    assert tick(bag, pool[:0], [], kind=kind, datagrams=True).shape == (0, 43)


# ---------------- 8. recovery ----------------------------------------------------------------------------------------------------------------------
def test_host_subset_hooks_cases_on_the_test_hooks_library():
    """the re-issue of an aborted host subset frame (status word staged with ape_debug_poke, nothing is made to give up) runs in a
    CHILD process on lib/diag/libape_hip_testhooks.so, like tests/hooks/subset_cases.py"""
    import os
    import subprocess
    import sys
    from tests.conftest import REPO
    lib = REPO / "arm-pose-estimation_amd" / "lib" / "diag" / "libape_hip_testhooks.so"
    assert lib.exists(), "make -C arm-pose-estimation_amd/csrc hooks"
    torch.cuda.synchronize()
    env = dict(os.environ, APE_HIP_LIB=str(lib))
    r = subprocess.run([sys.executable, "-m", "pytest", str(REPO / "tests" / "hooks" / "subset_host_cases.py"), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], env=env, cwd=str(REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
