"""Subset frames of the stream bank (``ape_streams_frame_subset`` / ``StreamBank.frame``): each listed stream does
what its own reference ``Estimator.process_row`` does with one row; unlisted streams are untouched; ``reset(streams=...)`` cold-starts
single streams.

CPU tests: argument refusals of the C ABI without a bank or device.
GPU tests: random schedules against offline replay of each stream's rows, all streams in order against the lockstep bank, the mode rules,
the kernel routes by list size, frames enqueued back to back.  The Monte-Carlo contract and the re-issue of an aborted frame need the
test-hooks library and run in a child process (tests/hooks/subset_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_replay import _estimator, _synthetic_rows


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


# ---------------- CPU: refusals ---------------------------------------------------------------------------------------
def test_subset_entries_refuse_null_arguments():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)                          # never dereferenced: every call below is refused first
    idx = np.arange(4, dtype=np.int32)
    ip = C.c_void_p(idx.ctypes.data)
    for bank, rows, streams, out in ((None, dummy, ip, dummy), (dummy, None, ip, dummy), (dummy, dummy, None, dummy),
                                     (dummy, dummy, ip, None)):
        rc = lib.ape_streams_frame_subset(bank, _hip.PARSE_WATCH_PHONE_POCKET, rows, streams, 4, 0, out, _hip.F32, None)
        assert rc != 0 and b"NULL" in lib.ape_last_error()
    for bank, streams in ((None, ip), (dummy, None)):
        rc = lib.ape_streams_reset_subset(bank, streams, 4)
        assert rc != 0 and b"NULL" in lib.ape_last_error()


def test_streambank_frame_is_bound():
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    for name in ("ape_streams_reset_subset", "ape_streams_frame_subset"):
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name)
    assert callable(StreamBank.frame)


# ---------------- GPU ---------------------------------------------------------------------------------------------------
def _frame_c(bank, kind, rows_dev, streams, flags, dtype, out=None):
    """ape_streams_frame_subset through the C ABI -> out [K, 25 | 25+6N] of dtype (packed with FLAG_PACKED_MSG and N > 1)"""
    from wear_mocap_ape_amd import _hip
    idx = np.ascontiguousarray(streams, dtype=np.int32)
    K, n = len(idx), bank._smooth * bank._n_mc
    if out is None:
        w = 25 + 6 * n if (flags & _hip.FLAG_PACKED_MSG) and n > 1 else 25
        out = torch.empty((K, w), dtype=dtype, device="cuda")
    rc = _hip.lib().ape_streams_frame_subset(bank._handle, kind, C.c_void_p(rows_dev.data_ptr()), C.c_void_p(idx.ctypes.data), K, flags,
                                             C.c_void_p(out.data_ptr()), _hip.F64 if dtype == torch.float64 else _hip.F32,
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _hip.check(rc, "ape_streams_frame_subset")
    return out


class _History:
    """per stream: the rows it received, the outputs it returned and where it was cold-started"""

    def __init__(self, S):
        self.rows = [[] for _ in range(S)]
        self.outs = [[] for _ in range(S)]
        self.starts = [[0] for _ in range(S)]

    def reset(self, streams):
        for s in streams:
            if len(self.rows[s]) and self.starts[s][-1] != len(self.rows[s]):
                self.starts[s].append(len(self.rows[s]))

    def add(self, streams, rows, out):
        for j, s in enumerate(streams):
            self.rows[s].append(rows[j])
            self.outs[s].append(out[j])

    def check_against_replay(self, est, tol, streams=None):
        """every stream's outputs against ONE replay of all streams' rows back to back (a recording start at every stream and
        at every one of its cold starts)"""
        rows, outs, starts = [], [], []
        for s in (range(len(self.rows)) if streams is None else streams):
            if not self.rows[s]:
                continue
            base = sum(len(r) for r in rows)
            starts += [base + a for a in self.starts[s] if a < len(self.rows[s])]      # (a cold start behind its last row: no row)
            rows.append(np.array(self.rows[s]))
            outs.append(np.array(self.outs[s]))
        ref = est.process_recording(np.concatenate(rows), starts=starts).cpu().numpy()
        got = np.concatenate(outs)
        assert ref.shape == got.shape
        err = float(np.abs(ref - got).max())
        assert err <= tol, err
        return err


def _pick(rng, S):
    u = rng.random()
    K = 0 if u < 0.05 else 1 if u < 0.15 else S if u < 0.25 else int(rng.integers(1, S + 1))
    return rng.permutation(S)[:K]


def _run_schedule(est, name, smooth, golden, S, ticks, seed, big_endian=False):
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    bank = StreamBank(model, S, T, smooth=smooth, normalize=True, dtype=torch.float64)
    rng = np.random.default_rng(seed)
    pool = _synthetic_rows(golden, name, S * ticks, seed + 1)
    hist = _History(S)
    for t in range(ticks):
        r = np.flatnonzero(rng.random(S) < 0.03)
        if len(r):
            bank.reset(streams=r)
            hist.reset(r)
        streams = _pick(rng, S)
        rows = pool[t * S + streams] if len(streams) else np.zeros((0, pool.shape[1]), np.float32)
        if len(streams) == 0:
            assert bank.frame(rows, streams, kind).shape[0] == 0
            continue
        sent = rows.byteswap() if big_endian else rows
        out = _frame_c(bank, kind | (_hip.PARSE_BIG_ENDIAN if big_endian else 0), torch.from_numpy(np.ascontiguousarray(sent)).cuda(),
                       streams, _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG, torch.float64)
        hist.add(streams, rows, out.cpu().numpy())
    return hist


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pocket", "watch", "uarm"])
@pytest.mark.parametrize("smooth", [1, 5])
def test_subset_random_schedule_against_replay(golden, tmp_path, monkeypatch, name, smooth):
    est = _estimator(tmp_path, monkeypatch, name, 3, 0.0, smooth=smooth, add_mc_samples=True, monte_carlo_samples=1)
    model = est._hip_model()
    for kernel, tol in (("tile16", 1e-12), ("auto", 5e-6)):
        model.set_kernel(kernel)
        hist = _run_schedule(est, name, smooth, golden, 37, 240, 100 + smooth)
        hist.check_against_replay(est, tol)
    model.set_kernel("auto")


@pytest.mark.gpu
def test_subset_random_schedule_big_endian(golden, tmp_path, monkeypatch):
    est = _estimator(tmp_path, monkeypatch, "pocket", 4, 0.0, smooth=5, add_mc_samples=True, monte_carlo_samples=1)
    est._hip_model().set_kernel("tile16")
    hist = _run_schedule(est, "pocket", 5, golden, 37, 120, 7, big_endian=True)
    hist.check_against_replay(est, 1e-12)
    est._hip_model().set_kernel("auto")


@pytest.mark.gpu
@pytest.mark.parametrize("mc", [None, 4])
def test_subset_all_streams_in_order_equal_lockstep(golden, tmp_path, monkeypatch, mc):
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    S, smooth, ticks = 37, 3, 12
    est = _estimator(tmp_path, monkeypatch, "pocket", 5, 0.2, smooth=smooth, add_mc_samples=True, monte_carlo_samples=1)
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    model.set_kernel("tile16")
    kw = dict(monte_carlo_samples=mc, dropout=0.2, seed=4242) if mc else {}
    lock = StreamBank(model, S, T, smooth=smooth, normalize=True, dtype=torch.float64, **kw)
    sub = StreamBank(model, S, T, smooth=smooth, normalize=True, dtype=torch.float64, **kw)
    pool = torch.from_numpy(_synthetic_rows(golden, "pocket", S * ticks, 21)).cuda()
    flags = _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG
    n = smooth * (mc or 1)
    for t in range(ticks):
        rows = pool[t * S:(t + 1) * S].contiguous()
        lock.push_rows(rows, kind)
        want = torch.empty((S, 25 + 6 * n), dtype=torch.float64, device="cuda")
        _hip.check(_hip.lib().ape_streams_step(lock._handle, flags, C.c_void_p(want.data_ptr()), None, _hip.F64,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ape_streams_step")
        got = _frame_c(sub, kind, rows, np.arange(S), flags, torch.float64)
        assert torch.equal(got, want), t
        # the Python entry: the bank's dtype, [K, 25], the same messages
        msg = sub.frame(rows.cpu().numpy(), np.arange(S), kind) if t == ticks - 1 else None
    assert msg.dtype == torch.float64 and tuple(msg.shape) == (S, 25)
    model.set_kernel("auto")


@pytest.mark.gpu
def test_subset_mode_rules_and_refusals(golden, tmp_path, monkeypatch):
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    S, smooth = 16, 3
    est = _estimator(tmp_path, monkeypatch, "pocket", 6, 0.0, smooth=smooth, add_mc_samples=True, monte_carlo_samples=1)
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    model.set_kernel("tile16")
    bank = StreamBank(model, S, T, smooth=smooth, normalize=True, dtype=torch.float64)
    pool = _synthetic_rows(golden, "pocket", S * 20, 31)
    hist = _History(S)
    flags = _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG
    for t in range(4):                                        # lockstep frames
        rows = pool[t * S:(t + 1) * S]
        bank.push_rows(torch.from_numpy(rows).cuda(), kind)
        out = torch.empty((S, 25 + 6 * smooth), dtype=torch.float64, device="cuda")
        _hip.check(_hip.lib().ape_streams_step(bank._handle, flags, C.c_void_p(out.data_ptr()), None, _hip.F64,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ape_streams_step")
        hist.add(range(S), rows, out.cpu().numpy())
    rng = np.random.default_rng(2)
    for t in range(4, 14):                                    # subset frames continue each stream's history
        streams = rng.permutation(S)[:int(rng.integers(1, S + 1))]
        rows = pool[t * S + streams]
        out = _frame_c(bank, kind, torch.from_numpy(rows).cuda(), streams, flags, torch.float64)
        hist.add(streams, rows, out.cpu().numpy())
    hist.check_against_replay(est, 1e-12)
    rows = torch.from_numpy(pool[:S]).cuda()
    with pytest.raises(UserWarning, match="per-stream"):
        bank.push_rows(rows, kind)
    with pytest.raises(UserWarning, match="per-stream"):
        bank.step()
    for bad in ([0, 0], [S], [-1]):
        with pytest.raises(UserWarning):
            bank.frame(pool[:len(bad)], bad, kind)
        with pytest.raises(UserWarning):
            bank.reset(streams=bad)
    # the C entry refuses them on its own
    for bad in ([0, 0], [S], [-1]):
        idx = np.array(bad, dtype=np.int32)
        out = torch.empty((len(bad), 25 + 6 * smooth), dtype=torch.float64, device="cuda")
        rc = _hip.lib().ape_streams_frame_subset(bank._handle, kind, C.c_void_p(rows.data_ptr()), C.c_void_p(idx.ctypes.data), len(bad),
                                                 flags, C.c_void_p(out.data_ptr()), _hip.F64, None)
        assert rc != 0 and (b"twice" in _hip.lib().ape_last_error() or b"outside" in _hip.lib().ape_last_error())
    with pytest.raises(UserWarning):                          # the width of the other message
        bank.frame(pool[:2, :28], [0, 1], _hip.PARSE_WATCH_ONLY)
    with pytest.raises(UserWarning):
        bank.frame(pool[:2], [0, 1, 2], kind)
    bank.reset()                                              # back to lockstep
    bank.push_rows(rows, kind)
    assert tuple(bank.step().shape) == (S, 25)
    model.set_kernel("auto")


@pytest.mark.gpu
def test_subset_routes_by_size(golden, tmp_path, monkeypatch):
    """S = 4096 on auto: K = 1 (latency kernel), 8 (small-batch), 100, 1024 (cluster kernels), 4096 -- each against replay"""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    S, smooth = 4096, 2
    est = _estimator(tmp_path, monkeypatch, "pocket", 8, 0.0, smooth=smooth, add_mc_samples=True, monte_carlo_samples=1)
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    bank = StreamBank(model, S, T, smooth=smooth, normalize=True, dtype=torch.float64)
    rng = np.random.default_rng(9)
    pool = _synthetic_rows(golden, "pocket", 3 * S, 41)
    used = 0
    hist = _History(S)
    kernels = set()
    for K in (1, 8, 100, 1024, 4096):
        for _ in range(2):
            streams = rng.permutation(S)[:K]
            rows = pool[used:used + K]
            used = (used + K) % (2 * S)
            out = _frame_c(bank, kind, torch.from_numpy(rows).cuda(), streams, _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG,
                           torch.float64)
            hist.add(streams, rows, out.cpu().numpy())
            bank.recover()
            kernels.add(model.last_kernel())
    hist.check_against_replay(est, 5e-6)
    assert len(kernels) >= 3, kernels


@pytest.mark.gpu
def test_subset_frames_back_to_back(golden, tmp_path, monkeypatch):
    """100 frames enqueued with no host synchronisation, each into its own output: the descriptor staging is never rewritten under a
    pending copy"""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    S, smooth, n = 64, 2, 100
    est = _estimator(tmp_path, monkeypatch, "pocket", 10, 0.0, smooth=smooth, add_mc_samples=True, monte_carlo_samples=1)
    model, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    bank = StreamBank(model, S, T, smooth=smooth, normalize=True, dtype=torch.float64)
    rng = np.random.default_rng(12)
    pool = _synthetic_rows(golden, "pocket", S * n, 51)
    pool_d = torch.from_numpy(pool).cuda()
    lists = [rng.permutation(S)[:int(rng.integers(1, S + 1))] for _ in range(n)]
    rows_d = [pool_d[t * S:t * S + len(lists[t])].contiguous() for t in range(n)]
    outs = [torch.full((len(lists[t]), 25 + 6 * smooth), float("nan"), dtype=torch.float64, device="cuda") for t in range(n)]
    torch.cuda.synchronize()
    for t in range(n):
        _frame_c(bank, kind, rows_d[t], lists[t], _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG, torch.float64, out=outs[t])
    torch.cuda.synchronize()
    bank.recover()
    hist = _History(S)
    for t in range(n):
        hist.add(lists[t], pool[t * S:t * S + len(lists[t])], outs[t].cpu().numpy())
    hist.check_against_replay(est, 5e-6)


@pytest.mark.gpu
def test_subset_hooks_cases_on_the_test_hooks_library():
    """the Monte-Carlo contract (targets read through a test hook) and the re-issue of an aborted subset frame (status word staged with
    ape_debug_poke) run in a CHILD process on lib/diag/libape_hip_testhooks.so, like tests/hooks/poke_cases.py"""
    import os
    import subprocess
    import sys
    from tests.conftest import REPO
    lib = REPO / "arm-pose-estimation_amd" / "lib" / "diag" / "libape_hip_testhooks.so"
    assert lib.exists(), "make -C arm-pose-estimation_amd/csrc hooks"
    torch.cuda.synchronize()
    env = dict(os.environ, APE_HIP_LIB=str(lib))
    r = subprocess.run([sys.executable, "-m", "pytest", str(REPO / "tests" / "hooks" / "subset_cases.py"), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], env=env, cwd=str(REPO), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
