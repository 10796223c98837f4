"""The Monte-Carlo spread record on the GPU: `ape_spread_reduce` on the reference-written est / msg rows, the
post-filter's SPR forms behind the banks' lockstep, subset and host frames, the replay's fused form, the estimator's switch.

Reference of every record: `estimate/_post.spread_rows` (plain numpy, two-pass covariance) of the frame's own stacked est rows.
A bank's stacked rows are the model outputs its smoothing ring holds after the step: `export_state` hands them out in time order
and `ape_fk` (de-normalising, float64) turns them into the est rows -- the same device functions the post-filter runs; their
`[:, 0:6]` must be the tail `step(with_tail=True)` of the same call returns.

Tolerances, derived: the record is sums of N float64 products of magnitude <= M = max(1, max |est[:, :6]|^2); means, covariances
and sin^2(angle / 2) agree to 16 N 2^-53 M absolute; the angle itself is compared where sin^2(angle / 2) > 1e-6, at 1e-6 relative."""
import ctypes as C
from array import array

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests.test_hip_parity import _synthetic_windows, make_model
from tests.test_replay import _estimator, _synthetic_rows

pytestmark = pytest.mark.gpu

SW = 21


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def bound(est, N):
    return 16.0 * N * 2.0 ** -53 * max(1.0, float(np.nanmax(np.abs(est[:, :6])) ** 2))


def check_record(got, ref, est, N, what):
    """-> the largest deviation (means / covariances / sin^2) in units of the bound"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = bound(est, N)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    ok = ~np.isnan(ref)
    d_lin = np.abs(got[:18] - ref[:18])[ok[:18]]
    s_got, s_ref = np.sin(got[18:] / 2) ** 2, np.sin(ref[18:] / 2) ** 2
    d_sin = np.abs(s_got - s_ref)[ok[18:]]
    worst = float(max(d_lin.max(initial=0.0), d_sin.max(initial=0.0)))
    assert worst <= tol, (what, worst, tol)
    big = ok[18:] & (s_ref > 1e-6)
    if big.any():
        rel = float((np.abs(got[18:] - ref[18:])[big] / ref[18:][big]).max())
        assert rel <= 1e-6, (what, rel)
    return worst / tol


def expected_form(S, N, n_cus):
    """what DESIGN.md 4.28 says a bank of S streams with N stacked rows runs; compared with what the bank reports it launched"""
    if N == 1 and S >= 8:
        return "wide"
    chunks = 1 if N <= 64 else 1 + (N - 64 + 62) // 63
    return f"split x{chunks}" if chunks > 1 and S * chunks <= n_cus else "one workgroup"


def stack_est(bank, model, layout, streams, bodies):
    """the stacked est rows [K][N, W] of the listed streams after a frame: ring -> export -> ape_fk (de-normalising)"""
    from wear_mocap_ape_amd import stream_state as ss
    from wear_mocap_ape_amd.estimate import _post
    desc = bank.state_desc()
    state, warm = bank.export_state(streams)
    state = state.cpu().numpy()
    out = []
    for j in range(len(streams)):
        assert warm[j] == 3
        _, stack = ss.unpack(state[j], desc)
        out.append(_post.fk_rows(model.handle, layout, 0, stack.reshape(-1, stack.shape[2]), bodies[j], denormalize=True))
    return out


# ---------------- ape_spread_reduce against the reference-written rows --------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_spread_reduce_on_reference_rows(golden, layout):
    from wear_mocap_ape_amd.estimate import _post
    g = golden(f"fk_layout{layout}.npz")
    ctx = _post.context(layout)
    for tag in ("bd", "bo"):
        for N in (1, 7, 300):
            est, msg = g[f"est_{tag}_N{N}"], g[f"msg_{tag}_N{N}"]
            if N == 7:
                assert np.isfinite(est).all() and np.isfinite(msg).all()      # equal_nan below cannot hide a failure here
            ref = _post.spread_rows(est, msg, layout)
            with ctx.lock:
                got = _post.spread_reduce(ctx.handle, layout, ctx.device, est, msg)
            u = check_record(got, ref, est, N, (layout, tag, N))
            print(f"spread_reduce layout {layout} {tag} N {N}: {u:.3f} of the bound {bound(est, N):.2e}")
            if N == 1:
                assert np.array_equal(got[[0, 1, 2, 9, 10, 11]], est[0, :6]) and not got[[3, 4, 5, 6, 7, 8, 12, 13, 14, 15, 16, 17, 18, 19, 20]].any()
            if layout == 1:
                assert got[20] == 0.0
    with pytest.raises(UserWarning):
        _post.spread_reduce(ctx.handle, layout, ctx.device, g["est_bd_N7"][:, :-1], g["msg_bd_N7"])


def test_spread_reduce_nan_row(golden):
    from wear_mocap_ape_amd.estimate import _post
    g = golden("fk_layout0.npz")
    est, msg = g["est_bd_N300"].copy(), g["msg_bd_N300"]
    est[270, 1] = np.nan                                   # a row of the second trip of the loop; hand y only
    ctx = _post.context(0)
    with ctx.lock:
        got = _post.spread_reduce(ctx.handle, 0, ctx.device, est, msg)
    ref = _post.spread_rows(est, msg, 0)
    assert np.isnan(ref[[1, 4, 6, 7]]).all() and np.isfinite(np.delete(ref, [1, 4, 6, 7])).all()
    check_record(got, ref, est, 300, "nan row")


# ---------------- lockstep banks ------------------------------------------------------------------------------------------------------------
def run_lockstep(m, cfg, stats, body, S, smooth, n_mc, frames, watch=(0,), dtype=torch.float64, seed=77, dropout=0.2, twin=True):
    """`frames` lockstep frames of a Monte-Carlo bank with the record; every watched stream against spread_rows of its own rows"""
    from wear_mocap_ape_amd.estimate import _post
    from wear_mocap_ape_amd.streams import StreamBank
    T, I, N = cfg["T"], cfg["I"], smooth * n_mc
    mk = lambda dt: StreamBank(m, S, T, smooth=smooth, normalize=stats is not None, dtype=dt,        # noqa: E731
                               monte_carlo_samples=n_mc if n_mc > 0 else None, dropout=dropout, seed=seed)
    N = smooth * max(n_mc, 1)
    bank = mk(dtype)
    plain = mk(dtype) if twin else None
    st = stats if stats is not None else {"xx_m": np.zeros(I), "xx_s": np.ones(I)}
    feats = _synthetic_windows(st, S, frames, I, 23)
    worst = 0.0
    for f in range(frames):
        x = torch.from_numpy(np.ascontiguousarray(feats[:, f])).cuda()
        bank.push_features(x)
        msg, tail, rec = bank.step(with_tail=True, with_spread=True)
        assert tuple(msg.shape) == (S, 25) and tuple(rec.shape) == (S, SW) and tuple(tail.shape) == (S, N, 6)
        msg, tail, rec = msg.cpu().numpy(), tail.cpu().numpy(), rec.cpu().numpy()
        if twin:                                           # the flag changes nothing else: message and tail bits
            plain.push_features(x)
            pm, pt = plain.step(with_tail=True)
            assert np.array_equal(pm.cpu().numpy(), msg) and np.array_equal(pt.cpu().numpy(), tail)
        ests = stack_est(bank, m, cfg["layout"], list(watch), [body] * len(watch))
        for s, est in zip(watch, ests):
            assert est.shape[0] == N and np.abs(est[:, :6] - tail[s]).max() <= 1e-15          # the rows of this very call
            ref = _post.spread_rows(est, msg[s], cfg["layout"])
            worst = max(worst, check_record(rec[s], ref, est, N, (S, smooth, n_mc, f, s)))
            if N > 1 and dropout > 0:
                assert rec[s][18] > 1e-4 and rec[s][3] > 0                                    # the samples do spread
    m.recover()
    return worst, bank.last_post_form()


@pytest.mark.parametrize("smooth,n_mc", [(1, 25), (4, 16), (5, 13), (1, 127), (2, 64)])
def test_lockstep_pocket_bank(golden, norm_stats, smooth, n_mc):
    """N = 25, 64, 65, 127, 128: the edges of the 64-row chunk, of the 63-row later chunks and of a third chunk; 8 frames, so cold
    and warm stacks both occur.  S = 3 runs the split form above 64 rows (S * chunks workgroups fit the chip); the same stack in a
    bank too large for it (S = n_cus // chunks + 1) runs the one-workgroup form's loop over the chunks"""
    g = golden("stream_trace_pocket.npz")
    stats, body = norm_stats["pocket"], g["body"]
    m, sd, cfg = make_model("pocket", int(g["weights_seed"]), stats)
    m.set_body(body)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = smooth * n_mc
    u, form = run_lockstep(m, cfg, stats, body, 3, smooth, n_mc, 8, watch=(0, 2))
    print(f"lockstep pocket S 3 N {N} [{form}]: {u:.3f} of the bound")
    assert form == expected_form(3, N, n_cus) == ("one workgroup" if N <= 64 else f"split x{2 if N <= 127 else 3}")      # as launched
    if N in (65, 128):
        chunks = 2 if N == 65 else 3
        S = n_cus // chunks + 1
        u, form = run_lockstep(m, cfg, stats, body, S, smooth, n_mc, 2, watch=(0, S - 1), twin=False)
        print(f"lockstep pocket S {S} N {N} [{form}]: {u:.3f} of the bound")
        assert form == "one workgroup"


def test_deterministic_bank_wide_form(golden, norm_stats):
    """S = 65, N = 1: the wide kernel, its second workgroup with one live lane.  The record is trivial, the message bits unchanged"""
    from wear_mocap_ape_amd.streams import StreamBank
    g = golden("stream_trace_pocket.npz")
    stats = norm_stats["pocket"]
    m, sd, cfg = make_model("pocket", int(g["weights_seed"]), stats)
    m.set_body(g["body"])
    S = 65
    a, b = StreamBank(m, S, cfg["T"], dtype=torch.float64), StreamBank(m, S, cfg["T"], dtype=torch.float64)
    assert a.last_post_form() == "none"
    feats = _synthetic_windows(stats, S, 2, cfg["I"], 5)
    for f in range(2):
        x = torch.from_numpy(np.ascontiguousarray(feats[:, f])).cuda()
        a.push_features(x)
        b.push_features(x)
        msg, tail, rec = a.step(with_tail=True, with_spread=True)
        msg, tail, rec = msg.cpu().numpy(), tail.cpu().numpy(), rec.cpu().numpy()
        assert np.array_equal(msg, b.step().cpu().numpy())
        assert np.array_equal(rec[:, 0:3], tail[:, 0, 0:3]) and np.array_equal(rec[:, 9:12], tail[:, 0, 3:6])
        assert np.array_equal(rec[:, 0:3], msg[:, 4:7]) and np.array_equal(rec[:, 9:12], msg[:, 11:14])      # N == 1: the message copies the row
        assert not rec[:, 3:9].any() and not rec[:, 12:21].any()
        assert a.last_post_form() == "wide" == b.last_post_form()
    m.recover()


@pytest.mark.parametrize("name", ["watch", "position"])
def test_other_layouts(golden, norm_stats, name):
    """the watch-only layout (no hips: column 20 exactly 0) and the O = 20 position layout, S = 2, N = 25"""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import nn_models
    if name == "watch":
        g = golden("stream_trace_watch.npz")
        stats, body = norm_stats["watch"], g["body"]
        m, sd, cfg = make_model("watch", int(g["weights_seed"]), stats)
    else:
        cfg = dict(I=22, H=256, L=2, O=20, T=6, layout=_hip.LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS)
        m = nn_models.DropoutLSTM(22, 256, 2, 20, dropout=0.2, device=0, target_layout=cfg["layout"])
        m.load_state_dict(orc.make_state_dict(22, 256, 2, 20, seed=4))
        st = norm_stats["pocket"]
        stats = {"xx_m": st["xx_m"], "xx_s": st["xx_s"], "yy_m": np.linspace(-0.2, 0.2, 20), "yy_s": np.full(20, 0.3)}
        m.set_norm_stats(stats["xx_m"], stats["xx_s"], stats["yy_m"], stats["yy_s"])
        body = orc.DEFAULT_BODY
    m.set_body(body)
    u, form = run_lockstep(m, cfg, stats, body, 2, 1, 25, 8, watch=(0, 1))
    print(f"lockstep {name} S 2 N 25 [{form}]: {u:.3f} of the bound")
    assert form == "one workgroup"


def test_float32_record_is_the_float64_record_rounded_once(golden, norm_stats):
    from wear_mocap_ape_amd.streams import StreamBank
    g = golden("stream_trace_pocket.npz")
    stats = norm_stats["pocket"]
    m, sd, cfg = make_model("pocket", int(g["weights_seed"]), stats)
    m.set_body(g["body"])
    S, smooth, n_mc = 3, 5, 13
    mk = lambda dt: StreamBank(m, S, cfg["T"], smooth=smooth, dtype=dt, monte_carlo_samples=n_mc, dropout=0.2, seed=9)      # noqa: E731
    a, b = mk(torch.float32), mk(torch.float64)
    feats = _synthetic_windows(stats, S, 3, cfg["I"], 31)
    for f in range(3):
        x = torch.from_numpy(np.ascontiguousarray(feats[:, f])).cuda()
        a.push_features(x)
        b.push_features(x)
        r32, r64 = a.step(with_spread=True)[1], b.step(with_spread=True)[1]
        assert r32.dtype == torch.float32 and torch.equal(r32, r64.to(torch.float32))
    m.recover()


def test_packed_spread_datagram_rows(golden, norm_stats):
    """PACKED_MSG | SPREAD: columns [:25 + 6N] are bit-equal to the unflagged packed rows of a twin bank; the record behind them is
    the float32 of the float64 bank's"""
    from wear_mocap_ape_amd.streams import StreamBank
    g = golden("stream_trace_pocket.npz")
    stats = norm_stats["pocket"]
    m, sd, cfg = make_model("pocket", int(g["weights_seed"]), stats)
    m.set_body(g["body"])
    S, smooth, n_mc = 3, 2, 40
    N = smooth * n_mc
    mk = lambda dt: StreamBank(m, S, cfg["T"], smooth=smooth, dtype=dt, monte_carlo_samples=n_mc, dropout=0.2, seed=11)     # noqa: E731
    a, b, c = mk(torch.float32), mk(torch.float32), mk(torch.float64)
    feats = _synthetic_windows(stats, S, 3, cfg["I"], 37)
    for f in range(3):
        x = torch.from_numpy(np.ascontiguousarray(feats[:, f])).cuda()
        for bank in (a, b, c):
            bank.push_features(x)
        rows = a.step_datagrams(spread=True)
        assert tuple(rows.shape) == (S, 25 + 6 * N + SW) and rows.dtype == torch.float32
        packed, rec = StreamBank.split_spread(rows)
        assert torch.equal(packed, b.step_datagrams())
        assert torch.equal(rec, c.step(with_spread=True)[1].to(torch.float32))
    m.recover()


# ---------------- subset frames, per-stream bodies -----------------------------------------------------------------------------------------
def test_subset_frame_and_bodies(golden, norm_stats):
    """K = 2 of S = 4: one listed stream freshly reset, one warm; then two different bodies -- each stream's record matches its own
    rows and the two differ"""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import _post
    from wear_mocap_ape_amd.streams import StreamBank
    g = golden("stream_trace_pocket.npz")
    stats, body = norm_stats["pocket"], g["body"]
    m, sd, cfg = make_model("pocket", int(g["weights_seed"]), stats)
    m.set_body(body)
    S, smooth, n_mc, kind = 4, 3, 30, _hip.PARSE_WATCH_PHONE_POCKET
    N = smooth * n_mc                                      # 90 rows: the split form (4 x 2 workgroups)
    bank = StreamBank(m, S, cfg["T"], smooth=smooth, dtype=torch.float64, monte_carlo_samples=n_mc, dropout=0.2, seed=3)
    plain = StreamBank(m, S, cfg["T"], smooth=smooth, dtype=torch.float64, monte_carlo_samples=n_mc, dropout=0.2, seed=3)
    rows = _synthetic_rows(golden, "pocket", 6 * S, 41).reshape(6, S, -1)
    bodies = np.repeat(np.asarray(body, dtype=np.float64).reshape(1, 9), S, axis=0)
    worst = 0.0
    for t in range(6):
        if t == 3:
            bank.reset(streams=[1])
            plain.reset(streams=[1])
        if t == 4:                                         # two different wearers from here on
            bodies[1] = bodies[1] * 1.25
            bodies[3] = bodies[3] * 0.8
            bank.set_bodies(bodies[[1, 3]], streams=[1, 3])
            plain.set_bodies(bodies[[1, 3]], streams=[1, 3])
        streams = [1, 3] if t >= 3 else [3, 0]
        out = bank.frame(rows[t][streams], streams, kind, spread=True)
        assert tuple(out.shape) == (2, 25 + SW) and out.dtype == torch.float64
        msg, rec = (v.cpu().numpy() for v in StreamBank.split_spread(out))
        assert np.array_equal(msg, plain.frame(rows[t][streams], streams, kind).cpu().numpy())      # the flag changes nothing else
        ests = stack_est(bank, m, cfg["layout"], streams, bodies[streams])
        m.set_body(body)                                   # (fk_rows set the handle's body; the bank's table does not read it)
        for j, est in enumerate(ests):
            ref = _post.spread_rows(est, msg[j], cfg["layout"])
            worst = max(worst, check_record(rec[j], ref, est, N, ("subset", t, j)))
        if t >= 4:
            assert np.abs(rec[0] - rec[1]).max() > 1e-3    # two wearers, two records
    # datagram rows of a subset frame: the packed row, then the record
    d = bank.frame(rows[5][[0, 2]], [0, 2], kind, datagrams=True, spread=True)
    p = plain.frame(rows[5][[0, 2]], [0, 2], kind, datagrams=True)
    assert tuple(d.shape) == (2, 25 + 6 * N + SW) and d.dtype == torch.float32
    assert torch.equal(StreamBank.split_spread(d)[0], p)
    print(f"subset K 2 of S 4, N {N} [{bank.last_post_form()}], bodies from tick 4: {worst:.3f} of the bound")
    assert bank.last_post_form() == "split x2" == plain.last_post_form()
    m.recover()


# ---------------- other regressors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["ff", "imupose"])
def test_other_regressors(golden, tmp_path, monkeypatch, model):
    """a DropoutFF bank (N = smooth x n_mc) and an ImuPoseLSTM bank (n_mc ignored: N = smooth)"""
    from tests.test_regressor_banks_gpu import estimator, shifted_rows
    from wear_mocap_ape_amd.estimate import _post
    from wear_mocap_ape_amd.streams import StreamBank
    S, smooth, mc, name = 3, 3, 5, "pocket"
    est_obj = estimator(tmp_path, monkeypatch, model, name, smooth=smooth, add_mc_samples=True, monte_carlo_samples=mc, dropout=0.2)
    m, T, kind, layout = est_obj._hip_model(), est_obj.sequence_len, est_obj._parse_kind, est_obj._layout
    body = est_obj.body_measurements
    N = smooth * (mc if model == "ff" else 1)
    rows = shifted_rows(golden, name, S, 5)
    bank = StreamBank(m, S, T, smooth=smooth, dtype=torch.float64, monte_carlo_samples=mc, seed=21)
    worst = 0.0
    for f in range(5):
        bank.push_rows(torch.from_numpy(rows[f]).cuda(), kind)
        msg, tail, rec = bank.step(with_tail=True, with_spread=True)
        assert tuple(tail.shape) == (S, N, 6)
        msg, tail, rec = msg.cpu().numpy(), tail.cpu().numpy(), rec.cpu().numpy()
        bank.recover()
        for s, est in enumerate(stack_est(bank, m, layout, list(range(S)), [body] * S)):
            assert np.abs(est[:, :6] - tail[s]).max() <= 1e-15
            worst = max(worst, check_record(rec[s], _post.spread_rows(est, msg[s], layout), est, N, (model, f, s)))
    print(f"lockstep {model} S 3 N {N}: {worst:.3f} of the bound")


# ---------------- replay ----------------------------------------------------------------------------------------------------------------
def test_replay_records(golden, tmp_path, monkeypatch):
    """F = 40, starts [0, 17], smooth 3, n_mc 4: every frame's record against spread_rows of the replay's own rows (its packed cloud
    for the origins, y_dev -> ape_fk for the quaternions); the recording in two pieces (cut at 9 and at 17) gives the same bits"""
    from wear_mocap_ape_amd.estimate import _post
    smooth, n_mc, F, starts = 3, 4, 40, [0, 17]
    N = smooth * n_mc
    est_obj = _estimator(tmp_path, monkeypatch, "pocket", 1, 0.2, smooth=smooth, add_mc_samples=True, monte_carlo_samples=n_mc)
    m, layout, body = est_obj._hip_model(), est_obj._layout, est_obj.body_measurements
    rows = _synthetic_rows(golden, "pocket", F, 13)
    plain = est_obj.process_recording(rows, starts=starts, seed=5).cpu().numpy()
    out, y, rec = est_obj.process_recording(rows, starts=starts, seed=5, return_targets=True, spread=True)
    assert tuple(out.shape) == (F, 25 + 6 * N) and tuple(rec.shape) == (F, SW) and rec.dtype == torch.float64
    out, y, rec = out.cpu().numpy(), y.cpu().numpy(), rec.cpu().numpy()
    assert np.array_equal(out, plain)                      # the flag changes nothing else
    E = _post.fk_rows(m.handle, layout, 0, y.reshape(F * n_mc, -1), body, denormalize=True).reshape(F, n_mc, -1)
    worst = 0.0
    for f in range(F):
        seg = 17 if f >= 17 else 0
        est = np.concatenate([E[max(seg, f - smooth + 1 + j)] for j in range(smooth)])
        assert np.array_equal(est[:, :6].reshape(-1), out[f, 25:])                           # the replay's own cloud
        worst = max(worst, check_record(rec[f], _post.spread_rows(est, out[f, :25], layout), est, N, ("replay", f)))
    print(f"replay F 40 N {N}: {worst:.3f} of the bound")
    # float32: the float64 record rounded once
    r32 = est_obj.process_recording(rows, starts=starts, seed=5, spread=True, out_dtype=torch.float32)[1]
    assert np.array_equal(r32.cpu().numpy(), rec.astype(np.float32))
    # one recording in pieces: chained states, sample_row_base = rows before the piece (TILE16 granule: 4 rows = one frame)
    m.set_kernel("tile16")
    one = est_obj.process_recording(rows[:30], seed=5, spread=True)[1].cpu().numpy()
    for cut in (9, 17):
        o1, r1, (st, warm) = est_obj.process_recording(rows[:cut], seed=5, spread=True, return_state=True)
        o2, r2 = est_obj.process_recording(rows[cut:30], seed=5, spread=True, state_in=st, warm_in=warm, sample_row_base=cut * n_mc)
        assert np.array_equal(np.concatenate([r1.cpu().numpy(), r2.cpu().numpy()]), one), cut
    m.set_kernel("auto")


# ---------------- estimator -------------------------------------------------------------------------------------------------------------
def test_estimator_spread_switch(golden, tmp_path, monkeypatch):
    """WatchPhonePocketNN with spread on.  The process_row list is bit-equal to a twin with it off.  get_last_spread() -- all 21
    values -- is the record of that frame: spread_rows of the estimator's own stack (get_state -> ape_fk, whose [:, :6] is the cloud
    the frame returned) and the frame's message; on the host-frame route, and on the subset route a set_state puts the frame on.
    process_recording(spread=True): every row against spread_rows of the replay's own rows (y -> ape_fk).  The staged methods:
    get_last_spread() is spread_rows(est, msg) of the very rows msg_from_pred reduced"""
    from wear_mocap_ape_amd.estimate import _post
    smooth, n_mc = 3, 4
    N = smooth * n_mc
    mk = lambda: _estimator(tmp_path, monkeypatch, "pocket", 1, 0.2, smooth=smooth, add_mc_samples=True, monte_carlo_samples=n_mc)   # noqa: E731
    on, off, staged = mk(), mk(), mk()
    m, layout, body = on._hip_model(), on._layout, on.body_measurements
    assert on.spread is False and on.get_last_spread() is None
    on.spread = True
    rows = _synthetic_rows(golden, "pocket", 12, 17)

    def frame_and_check(r, what):
        a, b = on.process_row(array("f", r.tolist())), off.process_row(array("f", r.tolist()))
        assert isinstance(a, list) and a == b and len(a) == 25 + 6 * N
        rec = on.get_last_spread()
        assert rec.shape == (SW,) and rec.dtype == np.float64 and off.get_last_spread() is None
        stack = on.get_state()["stack"]                    # [smooth, n_mc, O] float32: what the frame's stack held
        est = _post.fk_rows(m.handle, layout, 0, stack.reshape(N, -1), body, denormalize=True)
        assert np.abs(est[:, :6].reshape(-1) - np.asarray(a[25:])).max() <= 1e-15            # the rows of this very frame
        assert np.array_equal(on.get_last_msg(), np.asarray(a[:25]))
        u = check_record(rec, _post.spread_rows(est, on.get_last_msg(), layout), est, N, what)
        assert (rec[18:21] > 1e-4).all() and rec[3] > 0    # the samples do spread
        return u
    worst = max(frame_and_check(r, ("host frame", f)) for f, r in enumerate(rows[:8]))
    print(f"estimator host frames N {N}: {worst:.3f} of the bound")
    # a set_state puts the one-stream bank into per-stream mode: the frames then run as subset frames
    on.set_state(on.get_state())
    off.set_state(off.get_state())
    assert on._frame_runner()._per_stream
    worst = max(frame_and_check(r, ("subset frame", f)) for f, r in enumerate(rows[8:]))
    print(f"estimator subset frames N {N}: {worst:.3f} of the bound")
    # reset and switching off clear the record
    on.reset()
    assert on.get_last_spread() is None
    on.process_row(array("f", rows[0].tolist()))
    assert on.get_last_spread() is not None
    on.spread = False
    assert on.get_last_spread() is None
    on.spread = True
    # the replay of the same rows: row for row against its own rows, all 21 values
    out, y, rec_rp = on.process_recording(rows, spread=True, return_targets=True)
    assert tuple(rec_rp.shape) == (12, SW)
    out, y, rec_rp = out.cpu().numpy(), y.cpu().numpy(), rec_rp.cpu().numpy()
    E = _post.fk_rows(m.handle, layout, 0, y.reshape(12 * n_mc, -1), body, denormalize=True).reshape(12, n_mc, -1)
    worst = 0.0
    for f in range(12):
        est = np.concatenate([E[max(0, f - smooth + 1 + j)] for j in range(smooth)])
        assert np.array_equal(est[:, :6].reshape(-1), out[f, 25:])
        worst = max(worst, check_record(rec_rp[f], _post.spread_rows(est, out[f, :25], layout), est, N, ("process_recording", f)))
    print(f"estimator process_recording N {N}: {worst:.3f} of the bound")
    # the staged reference-style methods fill the record through spread_rows: the same function of the same rows, so equal bits
    staged.use_device_frame = False
    staged.spread = True
    for r in rows[:4]:
        pred = staged.add_xx_to_row_hist_and_make_prediction(staged.parse_row_to_xx(array("f", r.tolist())))
        msg = staged.msg_from_pred(pred, True)
        ctx = _post.context(layout)
        with ctx.lock:
            est, m25 = _post.fk_and_msg(ctx.handle, layout, ctx.device, pred, body)
        assert est.shape[0] == N and np.array_equal(m25, np.asarray(msg[:25])) and np.array_equal(m25, staged.get_last_msg())
        assert np.array_equal(staged.get_last_spread(), _post.spread_rows(est, m25, layout))
        assert (staged.get_last_spread()[18:21] > 1e-4).all()
    # not served: the FK-only estimator
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    with pytest.raises(UserWarning, match="spread"):
        WatchPhoneUarm(smooth=2).spread = True


def test_small_position_layout_bank_writes_every_target(norm_stats):
    """an UNFLAGGED Monte-Carlo bank of S = 2 streams over the 20-target position layout: every target of every sample, columns
    16..19 included, is what the general route (ape_lstm_forward over the repeated windows with the bank's Philox key) computes, and
    two banks with one seed agree bit for bit.  (The Monte-Carlo latency kernel's head serves 16 targets; such banks stay off it.)"""
    from wear_mocap_ape_amd import _hip, stream_state as ss
    from wear_mocap_ape_amd.estimate import nn_models
    from wear_mocap_ape_amd.streams import StreamBank
    S, T, I, O, n_mc, seed = 2, 6, 22, 20, 25, 1234
    m = nn_models.DropoutLSTM(I, 256, 2, O, dropout=0.2, device=0, target_layout=_hip.LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS)
    m.load_state_dict(orc.make_state_dict(I, 256, 2, O, seed=4))
    st = norm_stats["pocket"]
    m.set_norm_stats(st["xx_m"], st["xx_s"], np.linspace(-0.2, 0.2, O), np.full(O, 0.3))
    m.set_body(orc.DEFAULT_BODY)
    mk = lambda: StreamBank(m, S, T, smooth=1, dtype=torch.float64, monte_carlo_samples=n_mc, dropout=0.2, seed=seed)      # noqa: E731
    a, b = mk(), mk()
    feats = _synthetic_windows(st, S, T, I, 29)
    for f in range(T):
        x = torch.from_numpy(np.ascontiguousarray(feats[:, f])).cuda()
        ys = []
        for bank in (a, b):
            bank.push_features(x)
            msg = bank.step().cpu().numpy()
            state, warm = bank.export_state([0, 1])
            ys.append(np.stack([ss.unpack(v, bank.state_desc())[1][0] for v in state.cpu().numpy()]))      # [S, n_mc, O]
            assert np.isfinite(msg).all()
        assert np.array_equal(ys[0], ys[1])
        if f in (0, T - 1):                                # the cold window (the newest row T times) and the first full one
            win = np.repeat(feats[:, :1], T, axis=1) if f == 0 else feats
            xw = torch.from_numpy(np.ascontiguousarray(np.repeat(win, n_mc, axis=0))).cuda()
            y = torch.empty((S * n_mc, O), dtype=torch.float32, device="cuda")
            _hip.check(_hip.lib().ape_lstm_forward(m.handle, C.c_void_p(xw.data_ptr()), S * n_mc, T, _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_DROPOUT_PHILOX,
                                                   None, 0.2, seed + f, C.c_void_p(y.data_ptr()), None), "ape_lstm_forward")
            torch.cuda.synchronize()
            err = np.abs(ys[0] - y.cpu().numpy().reshape(S, n_mc, O)).max(axis=(0, 1))
            print(f"position-layout bank S 2 frame {f}: max |bank - forward| per target {err.max():.2e}, targets 16..19 {err[16:].max():.2e}")
            assert err.max() < 2e-5, err
    m.recover()


def test_entries_refuse_what_they_always_refused(golden, norm_stats):
    from wear_mocap_ape_amd import _hip
    g = golden("stream_trace_pocket.npz")
    m, sd, cfg = make_model("pocket", int(g["weights_seed"]), norm_stats["pocket"])
    x = torch.zeros((2, cfg["T"], cfg["I"]), dtype=torch.float32, device="cuda")
    y = torch.zeros((2, cfg["O"]), dtype=torch.float32, device="cuda")
    e = torch.zeros((2, 21), dtype=torch.float64, device="cuda")
    lib = _hip.lib()
    assert lib.ape_lstm_forward(m.handle, C.c_void_p(x.data_ptr()), 2, cfg["T"], _hip.FLAG_SPREAD, None, 0.0, 0, C.c_void_p(y.data_ptr()), None) != 0
    assert lib.ape_infer(m.handle, C.c_void_p(x.data_ptr()), 2, cfg["T"], _hip.FLAG_SPREAD, None, C.c_void_p(e.data_ptr()), _hip.F64, None) != 0
    assert lib.ape_spread_reduce(m.handle, C.c_void_p(e.data_ptr()), 0, C.c_void_p(e.data_ptr()), C.c_void_p(e.data_ptr()), None) != 0
