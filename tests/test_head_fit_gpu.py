"""The output layer fitted to a wearer on the device: hidden features (`ape_lstm_features`, `ape_replay_features`), fit
sums on the float64 matrix cores (`ape_fit_sums`) and installing a head (`ape_model_set_head`).

Budgets.  Features and targets: max(1e-6, 4 e_ref), the project's own, e_ref being the float32 oracle's distance from the
float64 one on the same inputs.  Fit sums: 1.01 n 2^-53 sum|a_k b_k| per entry against `score.fit_sums_numpy` (n the pairs summed; the
bound of a float64 sum of n products in any order, which the MFMA's fused chain is), counts exact, symmetry and repeatability bit for bit.

End to end: 400 pocket frames in 4 recordings, 380 of them behind the 5 cold-start frames of a recording; the truth is a shifted head on
the frames' own features plus noise of sigma = 0.01 (normalised units).  The fit has 257 unknowns per column, so a plain least-squares
fit of this plant would leave sqrt(1 - 257 / 380) sigma = 0.57 sigma on the frames it saw and about sqrt(1 + 257 / 122) sigma = 1.76 sigma
on the 20 it did not; the ridge towards the present head trades some of that variance for bias in the directions the 380 frames do not
span.  numpy's own ridge fit of the same plant is held to the 1.5 sigma in the test itself: it stated 1.157 sigma over all 400 frames, the
device route 1.157 sigma, from 9.30 sigma before the fit (one MI355X).  380 pairs are
fewer than the 2 (P + 1) = 514 below which `best_head` refuses by default: the fit is made under a ridge of 1e-3 towards the present head
with `min_pairs` stated, and the test first shows that the default refuses and leaves the head as it was."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc

REPO = Path(__file__).resolve().parents[1]
U = 2.0 ** -53
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def _stats(name):
    raw = json.loads((REPO / "tests" / "golden" / "norm_stats.json").read_text())
    raw = raw[name] if name in raw else raw["pocket"]
    return {k: np.array(raw[k]) for k in ("xx_m", "xx_s", "yy_m", "yy_s")}


_MODELS = {}


def _model(name, seed=0, fresh=False, sd=None):
    """a DropoutLSTM of the config with seeded weights, body set (cached per (name, seed) unless `fresh`)"""
    from wear_mocap_ape_amd.estimate import nn_models
    key = (name, seed)
    if not fresh and sd is None and key in _MODELS:
        return _MODELS[key]
    cfg = orc.MODEL_CONFIGS[name]
    sd_ = orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], seed=seed) if sd is None else sd
    m = nn_models.DropoutLSTM(cfg["I"], cfg["H"], cfg["L"], cfg["O"], device=0)
    m.load_state_dict(sd_)
    m.set_body(orc.DEFAULT_BODY)
    if not fresh and sd is None:
        _MODELS[key] = (m, sd_)
    return m, sd_


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).tobytes()


# ---------------- features ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pocket", "uarm"])
@pytest.mark.parametrize("T", [1, 6])
def test_features_against_the_float64_recurrence_and_the_tile_kernel(name, T):
    from wear_mocap_ape_amd import _hip
    cfg = orc.MODEL_CONFIGS[name]
    assert T in (1, cfg["T"])
    model, sd = _model(name)
    H = cfg["H"]
    sd_id = dict(sd)
    sd_id["output_layer.weight"], sd_id["output_layer.bias"] = np.eye(H, dtype=np.float32), np.zeros(H, dtype=np.float32)
    x = np.random.default_rng(3 + T).standard_normal((33, T, cfg["I"])).astype(np.float32)
    h64 = orc.lstm_forward(sd_id, x, dtype=np.float64)[:, -1]
    h32 = orc.lstm_forward(sd_id, x, dtype=np.float32)[:, -1]
    y64, y32 = orc.lstm_forward(sd, x, dtype=np.float64)[:, -1], orc.lstm_forward(sd, x, dtype=np.float32)[:, -1]
    for B in (1, 15, 16, 17, 33):
        xd = torch.from_numpy(x[:B]).cuda()
        model.set_kernel("auto")
        h, y = model.features(xd)
        assert model.last_kernel() == "ape_lstm_tile16<hout>"
        torch.cuda.synchronize()
        assert tuple(h.shape) == (B, H) and tuple(y.shape) == (B, cfg["O"])
        e_ref = float(np.abs(h32[:B].astype(np.float64) - h64[:B]).max())
        err = float(np.abs(h.cpu().numpy().astype(np.float64) - h64[:B]).max())
        print(f"{name} T={T} B={B}: |h - h64| = {err:.3e}, e_ref = {e_ref:.3e}")
        assert err <= max(1e-6, 4 * e_ref), (B, err, e_ref)
        assert float(np.abs(y.cpu().numpy() - y64[:B]).max()) <= max(1e-6, 4 * float(np.abs(y32[:B].astype(np.float64) - y64[:B]).max()))
        # the same launch's head: the bits of the forward entry forced onto the batch-tile kernel
        model.set_kernel("tile16")
        y16 = model(xd, last_step_only=True)[:, 0]
        assert model.last_kernel() == "ape_lstm_tile16"
        assert _bits(y) == _bits(y16), B
        if B in (17, 33) and cfg["L"] > 1:               # once more with in-kernel dropout, one seed
            hd, yd = model.features(xd, dropout_p=0.2, seed=77)
            yd16 = model._run(xd, _hip.FLAG_DROPOUT_PHILOX, dropout_p=0.2, seed=77, last_step_only=True)[:, 0]
            assert model.last_kernel() == "ape_lstm_tile16"
            assert _bits(yd) == _bits(yd16) and _bits(yd) != _bits(y) and _bits(hd) != _bits(h)
    model.set_kernel("auto")
    model.recover()


def test_features_refusals_on_the_device():
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import nn_models
    model, _ = _model("pocket")
    lib = _hip.lib()
    x = torch.zeros((4, 6, 22), device="cuda")
    h, y = torch.zeros((4, 256), device="cuda"), torch.zeros((4, 14), device="cuda")
    call = lambda m, flags: lib.ape_lstm_features(m.handle, C.c_void_p(x.data_ptr()), 4, 6, flags, None, 0.0, 0, C.c_void_p(h.data_ptr()),   # noqa: E731
                                                  C.c_void_p(y.data_ptr()), None)
    assert call(model, _hip.FLAG_ALL_STEPS) == 1 and b"ALL_STEPS" in lib.ape_last_error()
    assert call(model, _hip.FLAG_BROADCAST_X) == 1
    assert call(model, _hip.FLAG_NORMALIZE_INPUT) == 3                                             # no norm stats on this handle
    assert call(model, _hip.FLAG_DROPOUT_MASKS | _hip.FLAG_DROPOUT_PHILOX) == 1
    model.set_precision("f16")
    assert call(model, 0) == 2 and b"fp16" in lib.ape_last_error()
    model.set_precision("f32")
    assert call(model, 0) == 0
    torch.cuda.synchronize()
    model.recover()
    ff = nn_models.DropoutFF(14, 128, 2, 22, device=0)
    imu = nn_models.ImuPoseLSTM(22, 256, 2, 14, device=0)
    for other in (ff, imu):
        assert call(other, 0) == 2 and b"DropoutLSTM" in lib.ape_last_error()


@pytest.mark.parametrize("name", ["pocket", "uarm"])
def test_replay_features_of_two_recordings(golden, tmp_path, monkeypatch, name):
    from tests.test_replay import _estimator, _seg_of, _synthetic_rows, _windows
    est = _estimator(tmp_path, monkeypatch, name, 4, 0.0, smooth=1, add_mc_samples=False, monte_carlo_samples=1)
    rows = _synthetic_rows(golden, name, 38, 9)
    starts = [0, 1]
    out, y = est.process_recording(rows, starts=starts, return_targets=True)
    h16, y16 = est.features_recording(rows, starts, max_rows_per_launch=16, return_targets=True)
    h0, y0 = est.features_recording(rows, starts, max_rows_per_launch=0, return_targets=True)
    assert tuple(h0.shape) == (38, est._hip_model().hidden_layer_size) and h0.dtype == torch.float32
    assert _bits(h16) == _bits(h0) and _bits(y16) == _bits(y0)
    assert _bits(est.features_recording(rows, starts)) == _bits(h0)
    # the budget from the oracle on the windows the replay builds
    sd = {k: v.numpy() for k, v in est._hip_model().state_dict().items()}
    xx = est.parse_rows(torch.from_numpy(rows).cuda(), out_dtype=torch.float32).cpu().numpy().astype(np.float64)    # (the replay's float32 rows)
    T = est.sequence_len
    win = _windows(xx, _seg_of(38, starts), T, range(38))
    xn = ((win - est._xx_m) / est._xx_s).astype(np.float32)
    y64, y32 = orc.lstm_forward(sd, xn, dtype=np.float64)[:, -1], orc.lstm_forward(sd, xn, dtype=np.float32)[:, -1]
    budget = max(1e-6, 4 * float(np.abs(y32.astype(np.float64) - y64).max()))
    err_replay = float(np.abs(y0.cpu().numpy().astype(np.float64) - y[:, 0].cpu().numpy().astype(np.float64)).max())
    err_oracle = float(np.abs(y0.cpu().numpy().astype(np.float64) - y64).max())
    print(f"{name}: |y_features - y_replay| = {err_replay:.3e}, |y_features - y64| = {err_oracle:.3e}, budget {budget:.3e}")
    assert err_replay <= budget and err_oracle <= budget
    sd_id = dict(sd)
    H = h0.shape[1]
    sd_id["output_layer.weight"], sd_id["output_layer.bias"] = np.eye(H, dtype=np.float32), np.zeros(H, dtype=np.float32)
    h64, h32 = orc.lstm_forward(sd_id, xn, dtype=np.float64)[:, -1], orc.lstm_forward(sd_id, xn, dtype=np.float32)[:, -1]
    assert float(np.abs(h0.cpu().numpy() - h64).max()) <= max(1e-6, 4 * float(np.abs(h32.astype(np.float64) - h64).max()))


# ---------------- fit sums ---------------------------------------------------------------------------------------------------------------------
def _fit_case(P, Q, seed):
    """the batch of the issue: recordings of 1, 3, 4, 5, L - 1, L, L + 1 and 2 L + 5 frames, skip 2, lags of both signs, one longer than
    its recording, NaN / Inf planted in x and t of known frames inside the supports"""
    from wear_mocap_ape_amd import score
    L = score.FIT_PIECE
    lengths = [1, 3, 4, 5, L - 1, L, L + 1, 2 * L + 5]
    lags = [0, 5, -1, 2, 3, -4, 0, 7]
    starts = np.cumsum([0] + lengths[:-1])
    F = int(sum(lengths))
    rng = np.random.default_rng(seed)
    x = np.tanh(rng.standard_normal((F, P)) * 1.5)
    t = rng.standard_normal((F, Q)) * 2.0 + 0.5
    s4, s5, s6, s7 = (int(v) for v in starts[4:8])
    x[s4 + 10, 3], x[s5 + 100, P - 1], x[s7 + L + 2, 17] = np.nan, np.inf, -np.inf
    t[s4 + 20, 0], t[s6 + L, Q - 1], t[s7 + 2 * L - 10, Q // 2] = np.inf, np.nan, np.nan
    shift, scale = rng.standard_normal(Q), np.exp(rng.standard_normal(Q)) * np.where(np.arange(Q) % 3 == 0, -1.0, 1.0)
    return x, t, starts, lags, shift, scale


def _bound(x, t, starts, skip, lags, shift, scale):
    """1.01 n u sum|a_k b_k| per entry and recording, over the pairs summed: [R, M, M]"""
    F, P, Q = x.shape[0], x.shape[1], t.shape[1]
    ends = list(starts[1:]) + [F]
    out = []
    for s, e, l in zip(starts, ends, lags):
        lo, up = int(s) + max(skip, l), int(e) + min(0, l)
        f = np.arange(lo, max(lo, up))
        tt = t[f - l].astype(np.float64)
        tz = (tt - (0.0 if shift is None else shift)) / (1.0 if scale is None else scale)
        with np.errstate(all="ignore"):
            ok = np.isfinite(x[f]).all(axis=1) & np.isfinite(tt).all(axis=1)
        Z = np.abs(np.concatenate([x[f].astype(np.float64), np.ones((f.shape[0], 1)), tz], axis=1)[ok])
        out.append(1.01 * ok.sum() * U * (Z.T @ Z))
    return np.stack(out)


@pytest.mark.parametrize("P", [128, 256])
@pytest.mark.parametrize("Q", [1, 14, 17, 32])
def test_fit_sums_against_the_statement(P, Q):
    from wear_mocap_ape_amd import score
    x, t, starts, lags, shift, scale = _fit_case(P, Q, 100 * P + Q)
    skip, M = 2, P + 1 + Q
    F = x.shape[0]
    for xdt, tdt, affine in ((np.float32, np.float64, True), (np.float64, np.float32, False), (np.float32, np.float32, True),
                             (np.float64, np.float64, True)):
        xh, th = x.astype(xdt), t.astype(tdt)
        sh, sc = (shift, scale) if affine else (None, None)
        want = score.fit_sums_numpy(xh, th, starts, skip, lags, sh, sc)
        bound = _bound(xh, th, starts, skip, lags, sh, sc)
        # x a strided view of wider rows, t strided
        xw = torch.full((F, P + 24), 7.0, dtype=torch.from_numpy(xh).dtype, device="cuda")
        tw = torch.full((F, Q + 3), -3.0, dtype=torch.from_numpy(th).dtype, device="cuda")
        xw[:, 8:8 + P], tw[:, 2:2 + Q] = torch.from_numpy(xh).cuda(), torch.from_numpy(th).cuda()
        xv, tv = xw[:, 8:8 + P], tw[:, 2:2 + Q]
        acc = score.fit_sums(xv, tv, starts, skip, lags, sh, sc)
        assert acc.is_cuda and acc.dtype == torch.float64 and tuple(acc.shape) == (len(starts), M * M + 2)
        got = acc.cpu().numpy()
        G, Gw = got[:, :M * M].reshape(-1, M, M), want[:, :M * M].reshape(-1, M, M)
        assert np.isfinite(got).all()
        over = np.abs(G - Gw) - bound
        print(f"P={P} Q={Q} {np.dtype(xdt).name}/{np.dtype(tdt).name}: max |diff| / bound = {float((np.abs(G - Gw) / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (over <= 0).all(), float(over.max())
        assert (got[:, M * M:] == want[:, M * M:]).all() and (G[:, P, P] == got[:, M * M]).all()
        assert got[:, M * M + 1].sum() == 6 and (got[:2] == 0).all()                            # six planted pairs; shorter than skip / its lag
        assert _bits(G) == _bits(np.ascontiguousarray(G.transpose(0, 2, 1)))
        assert _bits(score.fit_sums(xv, tv, starts, skip, lags, sh, sc)) == _bits(acc)           # the same bits on every run
        assert _bits(score.fit_sums(xv.contiguous(), tv.contiguous(), starts, skip, lags, sh, sc)) == _bits(acc)


def test_fit_sums_record_does_not_depend_on_the_batch_around_it():
    from wear_mocap_ape_amd import score
    L, P, Q = score.FIT_PIECE, 256, 14
    rng = np.random.default_rng(8)
    recs = [(np.tanh(rng.standard_normal((n, P))).astype(np.float32), rng.standard_normal((n, Q))) for n in (L + 37, 90, 2 * L + 1)]
    recs[0][0][50, 7], recs[0][1][L + 3, 2] = np.nan, np.inf
    lags = [3, -2, 1]
    records = []
    for order in ((0, 1, 2), (1, 0, 2), (1, 2, 0)):
        x = torch.from_numpy(np.concatenate([recs[i][0] for i in order])).cuda()
        t = torch.from_numpy(np.concatenate([recs[i][1] for i in order])).cuda()
        starts = np.cumsum([0] + [recs[i][0].shape[0] for i in order][:-1])
        acc = score.fit_sums(x, t, starts, 5, [lags[i] for i in order])
        records.append(acc[order.index(0)].cpu().numpy())
    assert records[0][-1] == 2 and records[0][-2] == L + 37 - 5 - 2
    assert records[0].tobytes() == records[1].tobytes() == records[2].tobytes()
    alone = score.fit_sums(torch.from_numpy(recs[0][0]).cuda(), torch.from_numpy(recs[0][1]).cuda(), None, 5, [3])
    assert alone[0].cpu().numpy().tobytes() == records[0].tobytes()


def test_fit_sums_of_a_recording_cut_at_a_piece_boundary_merge_to_the_whole():
    from wear_mocap_ape_amd import score
    L, P, Q = score.FIT_PIECE, 128, 17
    rng = np.random.default_rng(9)
    n = 2 * L + 5
    x, t = torch.from_numpy(np.tanh(rng.standard_normal((n, P)))).cuda(), torch.from_numpy(rng.standard_normal((n, Q)).astype(np.float32)).cuda()
    whole = score.fit_sums(x, t)
    parts = score.merge_fit(score.fit_sums(x[:2 * L], t[:2 * L]), score.fit_sums(x[2 * L:], t[2 * L:]))
    assert parts.tobytes() == whole.cpu().numpy().tobytes()
    assert whole[0, -2].item() == n and whole[0, -1].item() == 0


# ---------------- set_head ---------------------------------------------------------------------------------------------------------------------
def _new_head(sd, seed):
    rng = np.random.default_rng(seed)
    w = (sd["output_layer.weight"] + 0.05 * rng.standard_normal(sd["output_layer.weight"].shape)).astype(np.float32)
    b = (sd["output_layer.bias"] - 0.1 + 0.05 * rng.standard_normal(sd["output_layer.bias"].shape)).astype(np.float32)
    return w, b


def test_set_head_round_trip_and_refusals():
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import nn_models
    model, sd = _model("pocket", seed=5, fresh=True)
    w0, b0 = model.get_head()
    assert _bits(w0) == _bits(sd["output_layer.weight"]) and _bits(b0) == _bits(sd["output_layer.bias"])
    w, b = _new_head(sd, 1)
    model.set_head(w, b)
    w1, b1 = model.get_head()
    assert _bits(w1) == _bits(w) and _bits(b1) == _bits(b)
    kept = model.state_dict()
    assert _bits(kept["output_layer.weight"]) == _bits(w) and _bits(kept["output_layer.bias"]) == _bits(b)
    with pytest.raises(UserWarning):
        model.set_head(w[:, :-1], b)
    lib = _hip.lib()
    ff = nn_models.DropoutFF(14, 128, 2, 22, device=0)
    imu = nn_models.ImuPoseLSTM(22, 256, 2, 14, device=0)
    for other, H in ((ff, 128), (imu, 256)):
        wz, bz = np.zeros((14, H), np.float32), np.zeros(14, np.float32)
        for entry in (lib.ape_model_set_head, lib.ape_model_get_head):
            assert entry(other.handle, C.c_void_p(wz.ctypes.data), C.c_void_p(bz.ctypes.data)) == 2          # APE_ERR_UNSUPPORTED
        with pytest.raises(UserWarning):
            other.set_head(wz, bz)
    bare = nn_models.DropoutLSTM(22, 256, 2, 14, device=0)
    wz, bz = np.zeros((14, 256), np.float32), np.zeros(14, np.float32)
    assert lib.ape_model_set_head(bare.handle, C.c_void_p(wz.ctypes.data), C.c_void_p(bz.ctypes.data)) == 3   # APE_ERR_NOT_READY


def test_every_route_runs_the_installed_head():
    """finds a packed copy of the head, if a route keeps one: set_head on a loaded model against a model created fresh and loaded with
    the blob whose tail is the new head, bit for bit, on every kernel the planner can be forced onto at B = 33, T = 6"""
    cfg = orc.MODEL_CONFIGS["pocket"]
    a, sd = _model("pocket", seed=6, fresh=True)
    w, b = _new_head(sd, 2)
    sd2 = dict(sd)
    sd2["output_layer.weight"], sd2["output_layer.bias"] = w, b
    x = torch.from_numpy(np.random.default_rng(4).standard_normal((33, 6, cfg["I"])).astype(np.float32)).cuda()
    y_old = a.set_kernel("tile16")(x, last_step_only=True).clone()
    a.set_head(w, b)
    f, _ = _model("pocket", fresh=True, sd=sd2)
    seen = {}
    for choice, precision in (("auto", "f32"), ("tile16", "f32"), ("cluster", "f32"), ("cluster_gen1", "f32"), ("auto_gen1", "f32"),
                              ("auto", "f16"), ("auto", "f16_gen1"), ("cluster", "f16")):
        try:
            for m in (a, f):
                m.set_kernel(choice)
                m.set_precision(precision)
        except UserWarning:
            for m in (a, f):
                m.set_kernel("auto")
                m.set_precision("f32")
            continue                                     # a route this device refuses
        try:
            ya = a(x, last_step_only=True)
        except UserWarning:
            continue                                     # ... or refuses at this shape
        ka = a.last_kernel()
        yf = f(x, last_step_only=True)
        assert f.last_kernel() == ka
        a.recover()
        f.recover()
        assert _bits(ya) == _bits(yf), (choice, precision, ka)
        assert _bits(ya) != _bits(y_old)
        seen.setdefault(ka, []).append((choice, precision))
    print("routes:", seen)
    assert "ape_lstm_tile16" in seen and len(seen) >= 2
    for m in (a, f):
        m.set_kernel("auto")
        m.set_precision("f32")
    # one lockstep frame of a 16-stream bank, deterministic and with 25 Monte-Carlo samples
    from wear_mocap_ape_amd.streams import StreamBank
    st = _stats("pocket")
    for m in (a, f):
        m.set_norm_stats(st["xx_m"], st["xx_s"], st["yy_m"], st["yy_s"])
    xx = torch.from_numpy((st["xx_m"] + st["xx_s"] * np.random.default_rng(6).standard_normal((16, cfg["I"]))).astype(np.float32)).cuda()
    for n_mc in (None, 25):
        got = []
        for m in (a, f):
            bank = StreamBank(m, 16, cfg["T"], smooth=1, dtype=torch.float64, monte_carlo_samples=n_mc, dropout=0.2, seed=11)
            bank.push_features(xx)
            msg, tail = bank.step(with_tail=True)
            torch.cuda.synchronize()
            bank.check()
            got.append((msg.clone(), tail.clone(), m.last_kernel()))
            del bank
        assert got[0][2] == got[1][2]
        assert _bits(got[0][0]) == _bits(got[1][0]) and _bits(got[0][1]) == _bits(got[1][1]), (n_mc, got[0][2])
        assert np.isfinite(got[0][0].cpu().numpy()).all()


def test_fit_head_end_to_end(golden, tmp_path, monkeypatch):
    from tests.test_replay import _estimator, _synthetic_rows
    from wear_mocap_ape_amd import score
    sigma, ridge = 0.01, 1e-3
    est = _estimator(tmp_path, monkeypatch, "pocket", 7, 0.0, smooth=1, add_mc_samples=False, monte_carlo_samples=1)
    rows = _synthetic_rows(golden, "pocket", 400, 21)
    rows += np.float32(0.02) * np.random.default_rng(22).standard_normal(rows.shape).astype(np.float32)     # (frames that differ: a fit needs them)
    starts = [0, 100, 200, 300]
    h = est.features_recording(rows, starts)
    w0, b0 = est.head
    rng = np.random.default_rng(23)
    w_true = w0.astype(np.float64) + 0.05 * rng.standard_normal(w0.shape)
    b_true = b0.astype(np.float64) + 0.1
    hh = h.cpu().numpy().astype(np.float64)
    truth_n = hh @ w_true.T + b_true + sigma * rng.standard_normal((400, w0.shape[0]))                       # normalised units
    truth = torch.from_numpy(truth_n * est._yy_s + est._yy_m).cuda()                                        # as score_recording takes them
    rms = lambda a: float(np.sqrt((a * a).mean()))                                                            # noqa: E731
    _, y_before = est.process_recording(rows, starts=starts, return_targets=True)
    before = rms(y_before[:, 0].cpu().numpy().astype(np.float64) - truth_n)
    # the condition on the plant: numpy's own ridge fit of the same rows (the frames behind the cold starts) stays inside the bound
    keep = np.concatenate([np.arange(s + est.sequence_len - 1, s + 100) for s in starts])
    X1 = np.concatenate([hh, np.ones((400, 1))], axis=1)
    D = np.ones(X1.shape[1])
    D[-1] = 0.0
    theta0 = np.concatenate([w0.T.astype(np.float64), b0[None].astype(np.float64)])
    A = X1[keep].T @ X1[keep] + np.diag(ridge * keep.shape[0] * D)
    theta = np.linalg.solve(A, X1[keep].T @ truth_n[keep] + (ridge * keep.shape[0] * D)[:, None] * theta0)
    plant = rms(X1 @ theta - truth_n)
    w, b, report, sums = est.fit_head(rows, truth, starts=starts, ridge=ridge, install=True)                # 380 pairs < 2 (P + 1): refused
    assert report["refused"] and _bits(w) == _bits(w0.astype(np.float64)) and _bits(est.head[0]) == _bits(w0)
    w, b, report, sums = est.fit_head(rows, truth, starts=starts, ridge=ridge, install=True, min_pairs=256 + 2)
    assert not report["refused"] and report["pairs"] == keep.shape[0] and tuple(sums.shape) == (4, (256 + 1 + 14) ** 2 + 2)
    w1, b1 = est.head
    assert _bits(w1) == _bits(w.astype(np.float32)) and _bits(b1) == _bits(b.astype(np.float32))
    _, y_after = est.process_recording(rows, starts=starts, return_targets=True)
    after = rms(y_after[:, 0].cpu().numpy().astype(np.float64) - truth_n)
    print(f"before {before / sigma:.2f} sigma, numpy's fit {plant / sigma:.3f} sigma, after {after / sigma:.3f} sigma; report {report['rmse_prior'].mean():.4f} -> "
          f"{report['rmse_fit'].mean():.4f}, cond {report['cond']:.3e}")
    assert before > 5 * sigma
    assert plant <= 1.5 * sigma
    assert after <= 1.5 * sigma
    # process_row runs the installed head too
    est.reset()
    msg = np.asarray(est.process_row(rows[0]), dtype=np.float64)
    assert np.abs(msg - est.process_recording(rows[:1]).cpu().numpy()[0]).max() < 5e-6
    assert np.isfinite(score.sweep_ridge(sums, w0, b0, [1e-4, 1e-2], min_pairs=256 + 2)[0]).all()
