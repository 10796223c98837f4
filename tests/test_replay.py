"""Offline replay (``ape_replay`` / ``Estimator.process_recording``): the pose message of every frame of
whole recordings in one call, as a fresh estimator's ``process_row`` loop over each recording would return it.

CPU tests: argument refusals of the C ABI without a device, the Python refusal without a HIP regressor.
GPU tests: the reference's streaming traces, cold starts at every recording start, the float64 post-filter against the
oracle, the Monte-Carlo contract (one dropout forward over the repeated windows, independent of the chunking), scale."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def _replay_c(model, kind, rows, starts, T, smooth, n_mc, p, seed, flags, out_dtype, want_y=False, max_rows=0):
    """ape_replay through the C ABI on device tensors -> (out, y)"""
    from wear_mocap_ape_amd import _hip
    rd = torch.as_tensor(rows, dtype=torch.float32).cuda().contiguous()
    st = np.ascontiguousarray(starts, dtype=np.int32)
    F, N = int(rd.shape[0]), smooth * n_mc
    width = 25 + 6 * N if (flags & _hip.FLAG_PACKED_MSG) and N > 1 else 25
    out = torch.empty((F, width), dtype=torch.float64 if out_dtype == _hip.F64 else torch.float32, device="cuda")
    y = torch.empty((F, n_mc, model.output_size), dtype=torch.float32, device="cuda") if want_y else None
    _hip.check(_hip.lib().ape_replay(model.handle, kind, C.c_void_p(rd.data_ptr()), F, C.c_void_p(st.ctypes.data), len(st), T,
                                     smooth, n_mc, float(p), seed, flags, C.c_void_p(out.data_ptr()), out_dtype,
                                     C.c_void_p(y.data_ptr()) if y is not None else None, max_rows,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ape_replay")
    return out, y


def _seg_of(F, starts):
    s = np.zeros(F, dtype=np.int64)
    for a in starts:
        s[a:] = a
    return s


def _stack_msgs(E, seg_of, smooth, body, layout, packed, frames):
    """oracle messages: E f64 [F, n_mc, W] est rows; stack row i of frame f = sample i % n_mc of frame
    max(seg, f - smooth + 1 + i // n_mc) (estimator.py:112-118 after a cold start at seg)"""
    out = []
    for f in frames:
        stack = np.concatenate([E[max(seg_of[f], f - smooth + 1 + j)] for j in range(smooth)])
        msg = orc.msg_from_est(stack, body, layout)
        if packed and stack.shape[0] > 1:
            msg = np.concatenate([msg, stack[:, :6].reshape(-1)])
        out.append(msg)
    return np.array(out)


def _windows(xx, seg_of, T, frames):
    """the clamped-index windows of Estimator._push_padded: row t of frame f is feature row max(seg, f - T + 1 + t)"""
    return np.stack([xx[[max(seg_of[f], f - T + 1 + t) for t in range(T)]] for f in frames])


def _synthetic_rows(golden, name, F, seed):
    """raw rows near the reference's recorded trace: the trace tiled, with a little noise on every column"""
    base = golden(f"stream_trace_{name}.npz")["rows"].astype(np.float32)
    rng = np.random.default_rng(seed)
    rows = np.tile(base, ((F + len(base) - 1) // len(base), 1))[:F]
    rows += np.float32(1e-3) * rng.standard_normal(rows.shape, dtype=np.float32)
    return rows


# ---------------- CPU: refusals ---------------------------------------------------------------------------------------
def test_replay_refuses_bad_arguments_without_a_device():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy = C.c_void_p(256)                          # never dereferenced: every call below is refused first

    def call(kind=0, F=10, starts=(0,), seq=6, smooth=1, n_mc=1, p=0.0, flags=0, dtype=_hip.F64, max_rows=0, rows=dummy):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        return lib.ape_replay(None, kind, rows, F, C.c_void_p(st.ctypes.data), len(st), seq, smooth, n_mc, p, 7, flags, dummy,
                              dtype, None, max_rows, None)

    bad = [(dict(kind=9), b"kind"), (dict(kind=0x200), b"kind"), (dict(F=0), b"F=0"), (dict(starts=(1,)), b"seg_starts[0]"),
           (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 10)), b"seg_starts[1]"), (dict(starts=()), b"starts"),
           (dict(seq=0), b"seq_len"), (dict(smooth=65), b"smooth"), (dict(smooth=0), b"smooth"), (dict(n_mc=0), b"n_mc"),
           (dict(smooth=64, n_mc=65), b"n_mc"), (dict(F=2 ** 30, n_mc=2), b"2^31"), (dict(p=1.0), b"dropout_p"),
           (dict(flags=_hip.FLAG_ALL_STEPS), b"PACKED_MSG"), (dict(dtype=3), b"dtype"), (dict(max_rows=8), b"max_rows_per_launch"),
           (dict(rows=None), b"NULL")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc != 0, kw
        assert what in lib.ape_last_error(), (kw, lib.ape_last_error())
    # valid arguments, no model: a loud failure (no CPU fallback); with no gfx950 device at all it says so
    rc = call(kind=_hip.PARSE_WATCH_PHONE_POCKET | _hip.PARSE_BIG_ENDIAN, starts=(0, 3, 9), smooth=4, n_mc=25, p=0.2,
              flags=_hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG)
    assert rc != 0 and b"model" in lib.ape_last_error()
    if lib.ape_device_count() == 0:
        assert rc == 5                               # APE_ERR_NO_DEVICE
        with pytest.raises(UserWarning):
            _hip.check(rc, "ape_replay")


def test_process_recording_needs_a_hip_regressor():
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.utility.names import NNS_INPUTS, NNS_TARGETS

    class _NoRegressor(Estimator):
        def parse_row_to_xx(self, row):
            return np.zeros(22, np.float32)

        def make_prediction_from_row_hist(self, xx_hist):
            return np.zeros((1, 14))

    x_in, y_out = list(NNS_INPUTS)[0], list(NNS_TARGETS)[0]
    est = _NoRegressor(x_in, y_out, normalize=False, smooth=2, seq_len=6)
    with pytest.raises(UserWarning):
        est.process_recording(np.zeros((4, 55), np.float32))


# ---------------- GPU ---------------------------------------------------------------------------------------------------
def _estimator(tmp_path, monkeypatch, name, seed, dropout, **kw):
    from wear_mocap_ape_amd import config
    from wear_mocap_ape_amd.estimate.watch_only import WatchOnlyNN
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import WatchPhonePocketNN
    from wear_mocap_ape_amd.estimate.watch_phone_uarm_nn import WatchPhoneUarmNN
    from tests.test_hip_parity import _deploy_dir
    _estimator.calls += 1                                   # a fresh tree per estimator, copied from the shipped one
    monkeypatch.setitem(config.PATHS, "deploy", _estimator.shipped.setdefault("deploy", config.PATHS["deploy"]))
    deploy, h = _deploy_dir(tmp_path / f"e{_estimator.calls}", name, seed, dropout=dropout)
    monkeypatch.setitem(config.PATHS, "deploy", deploy)
    cls = {"pocket": WatchPhonePocketNN, "watch": WatchOnlyNN, "uarm": WatchPhoneUarmNN}[name]
    return cls(model_hash=h, **kw)


_estimator.calls, _estimator.shipped = 0, {}


def _targets_to_est(est, y):
    """normalised targets [F, n_mc, O] -> f64 est rows [F, n_mc, W] (estimator.py:108-109, then the oracle's FK)"""
    F, M, O = y.shape
    pred = y.reshape(-1, O).astype(np.float64) * est._yy_s + est._yy_m
    e = orc.arm_pose_from_targets(pred, est.body_measurements, est._layout, route="closed")
    return e.reshape(F, M, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pocket", "watch", "uarm"])
def test_replay_reference_traces(golden, tmp_path, monkeypatch, name):
    g = golden(f"stream_trace_{name}.npz")
    rows = g["rows"].astype(np.float32)
    be = rows.byteswap()                                 # the UDP payload as received: big-endian float32
    for smooth, mc in ((1, 1), (5, 1), (3, 4)):
        tag = f"s{smooth}_mc{mc}"
        est = _estimator(tmp_path, monkeypatch, name, int(g["weights_seed"]), 0.0, smooth=smooth, add_mc_samples=True,
                         monte_carlo_samples=mc)
        ref = g[f"msg_{tag}"]
        out = est.process_recording(rows)
        assert out.is_cuda and out.dtype == torch.float64
        n = smooth * mc
        assert tuple(out.shape) == (len(rows), 25 + 6 * n if n > 1 else 25) == ref.shape
        err = float(np.abs(out.cpu().numpy() - ref).max())
        assert err < 5e-6, (tag, err)
        out_be = est.process_recording(be, big_endian=True)
        assert torch.equal(out_be, out), tag
        out32 = est.process_recording(rows, out_dtype=torch.float32)
        assert out32.dtype == torch.float32 and np.abs(out32.cpu().numpy() - ref).max() < 5e-6


@pytest.mark.gpu
def test_replay_cold_start_at_every_recording(golden, tmp_path, monkeypatch):
    smooth, mc = 3, 2
    est = _estimator(tmp_path, monkeypatch, "pocket", 3, 0.0, smooth=smooth, add_mc_samples=True, monte_carlo_samples=mc)
    T = est.sequence_len
    lengths = [1, T - 1, T, smooth + 1, 257, 1000]
    np.random.default_rng(5).shuffle(lengths)
    rows = _synthetic_rows(golden, "pocket", sum(lengths), 11)
    starts = np.cumsum([0] + lengths[:-1])
    out = est.process_recording(rows, starts=starts).cpu().numpy()
    assert out.shape == (len(rows), 25 + 6 * smooth * mc)
    for a, n in zip(starts, lengths):
        alone = est.process_recording(rows[a:a + n]).cpu().numpy()
        assert np.abs(out[a:a + n] - alone).max() < 5e-6, n
        est.reset()                                      # a fresh estimator's loop over this recording
        loop = np.array([np.asarray(est.process_row(r), dtype=np.float64) for r in rows[a:a + n]])
        assert loop.shape == out[a:a + n].shape
        assert np.abs(out[a:a + n] - loop).max() < 5e-6, n


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pocket", "watch"])
def test_replay_post_filter_exact(golden, tmp_path, monkeypatch, name):
    """returned targets -> the oracle's FK + message over the clamped stacks: the float64 post-filter alone"""
    smooth, mc = 4, 70
    est = _estimator(tmp_path, monkeypatch, name, 2, 0.2, smooth=smooth, add_mc_samples=True, monte_carlo_samples=mc)
    rows = _synthetic_rows(golden, name, 24, 3)
    starts = [0, 5, 17]
    out, y = est.process_recording(rows, starts=starts, return_targets=True)
    E = _targets_to_est(est, y.cpu().numpy())
    ref = _stack_msgs(E, _seg_of(len(rows), starts), smooth, est.body_measurements, est._layout, True, range(len(rows)))
    assert out.shape == ref.shape == (24, 25 + 6 * smooth * mc)
    assert np.abs(out.cpu().numpy() - ref).max() < 1e-12


@pytest.mark.gpu
def test_replay_post_filter_exact_position_layout(golden, norm_stats):
    """the 20-target layout (hand and elbow positions are network outputs) through the C ABI"""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import nn_models
    sd = orc.make_state_dict(22, 256, 2, 20, seed=4)
    m = nn_models.DropoutLSTM(22, 256, 2, 20, dropout=0.2, device=0, target_layout=_hip.LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS)
    m.load_state_dict(sd)
    st = norm_stats["pocket"]
    yy_m, yy_s = np.linspace(-0.2, 0.2, 20), np.full(20, 0.3)
    m.set_norm_stats(st["xx_m"], st["xx_s"], yy_m, yy_s)
    m.set_body(orc.DEFAULT_BODY)
    rows = _synthetic_rows(golden, "pocket", 30, 9)
    starts, smooth, mc = [0, 11], 3, 8
    out, y = _replay_c(m, _hip.PARSE_WATCH_PHONE_POCKET, rows, starts, 6, smooth, mc, 0.2, 99,
                       _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG, _hip.F64, want_y=True)
    pred = y.cpu().numpy().reshape(-1, 20).astype(np.float64) * yy_s + yy_m
    E = orc.arm_pose_from_targets(pred, orc.DEFAULT_BODY, 2, route="closed").reshape(30, mc, 21)
    ref = _stack_msgs(E, _seg_of(30, starts), smooth, orc.DEFAULT_BODY, 2, True, range(30))
    assert np.abs(out.cpu().numpy() - ref).max() < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("n_mc", [4, 25, 70])
def test_replay_monte_carlo_contract(golden, tmp_path, monkeypatch, n_mc):
    """the samples are those of ONE ape_lstm_forward(DROPOUT_PHILOX, p, seed) over the repeated windows [F*n_mc, T, I]"""
    from wear_mocap_ape_amd import _hip
    smooth, seed, p = 2, 1234567, 0.2
    est = _estimator(tmp_path, monkeypatch, "pocket", 1, p, smooth=smooth, add_mc_samples=True, monte_carlo_samples=n_mc)
    model, T = est._hip_model(), est.sequence_len
    rows = _synthetic_rows(golden, "pocket", 40, n_mc)
    starts = [0, 17, 18]
    seg = _seg_of(40, starts)
    xx = est.parse_rows(rows).cpu().numpy()
    x = np.repeat(_windows(xx, seg, T, range(40)), n_mc, axis=0).astype(np.float32)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()

    def forward():
        yr = torch.empty((40 * n_mc, model.output_size), dtype=torch.float32, device="cuda")
        _hip.check(_hip.lib().ape_lstm_forward(model.handle, C.c_void_p(xd.data_ptr()), 40 * n_mc, T,
                                               _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_DROPOUT_PHILOX, None, p, seed,
                                               C.c_void_p(yr.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "ape_lstm_forward")
        model.recover()
        return yr.cpu().numpy().reshape(40, n_mc, -1)

    for kernel in ("tile16", "auto"):
        model.set_kernel(kernel)
        y_ref = forward()
        out, y = est.process_recording(rows, starts=starts, return_targets=True, seed=seed)
        out64, y64 = est.process_recording(rows, starts=starts, return_targets=True, seed=seed, max_rows_per_launch=64)
        y, y64 = y.cpu().numpy(), y64.cpu().numpy()
        assert np.std(y[:, 0] - y[:, 1]) > 1e-3                  # the samples differ: dropout is on
        if kernel == "tile16":
            assert np.array_equal(y, y_ref) and np.array_equal(y64, y_ref)
        else:
            assert np.abs(y - y_ref).max() < 1e-6 and np.abs(y64 - y_ref).max() < 1e-6
        assert np.abs(out.cpu().numpy() - out64.cpu().numpy()).max() < (1e-12 if kernel == "tile16" else 5e-6)
    model.set_kernel("auto")


@pytest.mark.gpu
def test_replay_scale(golden, tmp_path, monkeypatch, norm_stats):
    smooth = 3
    est = _estimator(tmp_path, monkeypatch, "pocket", 6, 0.0, smooth=smooth, add_mc_samples=True, monte_carlo_samples=1)
    T, sd = est.sequence_len, orc.make_state_dict(22, 256, 2, 14, 6)
    stats = {"xx_m": est._xx_m, "xx_s": est._xx_s, "yy_m": est._yy_m, "yy_s": est._yy_s}
    rng = np.random.default_rng(0)
    for F, sm, starts, n_check in ((100_000, smooth, [0, 40_000, 77_777], 2000), (1_000_000, 1, [0], 200)):
        est._smooth = sm
        rows = _synthetic_rows(golden, "pocket", F, F)
        out = est.process_recording(rows, starts=starts)
        assert tuple(out.shape) == (F, 25 + 6 * sm if sm > 1 else 25)
        assert bool(torch.isfinite(out).all())
        seg = _seg_of(F, starts)
        frames = np.sort(rng.choice(F, n_check, replace=False))
        need = sorted({max(seg[f], f - sm + 1 + j) for f in frames for j in range(sm)})
        xx = est.parse_rows(rows).cpu().numpy()
        _, e = orc.infer_windows(sd, stats, est.body_measurements, est._layout, _windows(xx, seg, T, need))
        E = np.zeros((F, 1, e.shape[1]))
        E[need, 0] = e
        ref = _stack_msgs(E, seg, sm, est.body_measurements, est._layout, True, frames)
        err = float(np.abs(out.cpu().numpy()[frames] - ref).max())
        assert err < 5e-6, (F, err)
        del out


@pytest.mark.gpu
def test_replay_refusals_on_a_model(golden, tmp_path, monkeypatch):
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import nn_models
    est = _estimator(tmp_path, monkeypatch, "pocket", 1, 0.0, smooth=2, monte_carlo_samples=3)
    model = est._hip_model()
    rows = _synthetic_rows(golden, "pocket", 12, 1)
    with pytest.raises(UserWarning):                        # 20 features (watch-only kind) for a 22-input model
        _replay_c(model, _hip.PARSE_WATCH_ONLY_PHONE_MSG, rows, [0], 6, 2, 3, 0.0, 1, _hip.FLAG_NORMALIZE_INPUT, _hip.F64)
    with pytest.raises(UserWarning):
        est.process_recording(rows[:, :28])                 # width of the other message
    model.set_precision("f16")
    with pytest.raises(UserWarning, match="fp16"):
        est.process_recording(rows)
    model.set_precision("f32")
    assert est.process_recording(rows).shape == (12, 25 + 6 * 6)
    ff = nn_models.DropoutFF(14, 256, 2, 22, dropout=0.2, device=0)
    with pytest.raises(UserWarning, match="LSTM"):
        _replay_c(ff, _hip.PARSE_WATCH_PHONE_POCKET, rows, [0], 6, 1, 1, 0.0, 1, 0, _hip.F64)
