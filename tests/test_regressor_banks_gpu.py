"""DropoutFF and ImuPoseLSTM behind the one-call frames, the stream banks and the offline replay, on the GPU.

The reference's own messages for these models (tests/golden/regressor_traces.npz, written by gen_regressor_traces.py from the
reference estimators) pin `process_row`; banks, subset frames and replays are pinned against the single-stream estimator and the
oracle.  Tolerances are the ones the existing trace tests apply to `stream_trace_*` (imported, not invented here).  The cases that
need the test-hooks library (injected masks, the targets of a Philox bank) run in a child process: tests/hooks/regressor_cases.py."""
import ctypes as C
import json
import shutil
from array import array
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests.test_hip_round4 import TOL_MSG_LOOP
from tests.test_replay import _replay_c

pytestmark = pytest.mark.gpu

MODELS = ("ff", "imupose")
HASHES = {"pocket": "670b66fa7664252d1cfb3b5a8a362002ffeeba5c", "watch": "04f4ad63bfccb3668f7598c9375403e10b1fae2a"}
FF_H, FF_L = 256, 2
_shipped = {}
_calls = [0]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def state_dict(model, name, seed):
    cfg = orc.MODEL_CONFIGS[name]
    if model == "ff":
        return orc.make_ff_state_dict(cfg["I"], FF_H, FF_L, cfg["O"], seed)
    return orc.make_imupose_state_dict(cfg["I"], cfg["O"], seed)


def deploy_dir(tmp_path, monkeypatch, model, name, seed, dropout):
    """a deploy tree whose results.json names a DropoutFF / ImuPoseLSTM checkpoint, in the checkpoint format of
    tests/test_hip_parity._deploy_dir ((model_state, optimizer_state), nn_models.py:410)"""
    from wear_mocap_ape_amd import config
    src = Path(_shipped.setdefault("deploy", config.PATHS["deploy"]))
    _calls[0] += 1
    dst = tmp_path / f"deploy{_calls[0]}"
    shutil.copytree(src / "data_stats", dst / "data_stats", dirs_exist_ok=True)
    d = dst / "nn" / HASHES[name]
    d.mkdir(parents=True, exist_ok=True)
    p = json.loads((src / "nn" / HASHES[name] / "results.json").read_text())
    p["dropout"] = dropout
    p["model"] = "DropoutFF" if model == "ff" else "ImuPoseLSTM"
    if model == "ff":
        p["hidden_layer_size"], p["hidden_layer_count"] = FF_H, FF_L
    (d / "results.json").write_text(json.dumps(p))
    sd = state_dict(model, name, seed)
    torch.save(({k: torch.from_numpy(v) for k, v in sd.items()}, {"state": {}, "param_groups": []}), d / "checkpoint.pt")
    monkeypatch.setitem(config.PATHS, "deploy", dst)
    return HASHES[name]


def estimator(tmp_path, monkeypatch, model, name, seed=3, dropout=0.0, **kw):
    from wear_mocap_ape_amd.estimate import nn_models
    from wear_mocap_ape_amd.estimate.watch_only import WatchOnlyNN
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import WatchPhonePocketNN
    h = deploy_dir(tmp_path, monkeypatch, model, name, seed, dropout)
    est = {"pocket": WatchPhonePocketNN, "watch": WatchOnlyNN}[name](model_hash=h, **kw)
    assert isinstance(est._hip_model(), nn_models.DropoutFF if model == "ff" else nn_models.ImuPoseLSTM)
    return est


def stacked(model, smooth, mc):
    return smooth * (mc if model == "ff" else 1)


def shifted_rows(golden, name, S, frames):
    """S distinct phase-shifted copies of the fixture rows: stream s starts at row s of the (tiled) trace, a small per-stream offset on top"""
    base = golden(f"stream_trace_{name}.npz")["rows"].astype(np.float32)
    n = len(base)
    rows = np.stack([base[(np.arange(frames) + s) % n] for s in range(S)], axis=1)          # [frames, S, width]
    rows = rows + np.float32(1e-4) * np.arange(S, dtype=np.float32)[None, :, None]
    return np.ascontiguousarray(rows)


def single_stream_msgs(est, rows):
    """[frames, width]: one estimator's process_row over one stream's rows, from a cold start"""
    est.reset()
    est.msg_as_array = True
    return np.array([est.process_row(array("f", r.tolist())) for r in rows])


# ---------------- 1. process_row against the reference's messages ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pocket", "watch"])
@pytest.mark.parametrize("model", MODELS)
def test_process_row_replays_the_reference_messages(golden, tmp_path, monkeypatch, model, name):
    g, rows = golden("regressor_traces.npz"), golden(f"stream_trace_{name}.npz")["rows"]
    mc = int(g["mc_samples"])
    for smooth in (1, 5):
        ref = g[f"msg_{model}_{name}_s{smooth}"]
        n = stacked(model, smooth, mc)
        assert ref.shape[1] == (25 + 6 * n if n > 1 else 25)
        est = estimator(tmp_path, monkeypatch, model, name, seed=int(g["weights_seed"]), smooth=smooth, add_mc_samples=True,
                        monte_carlo_samples=mc)
        assert est._frame_runner() is not None, "the device-resident frame must be the path that runs"
        arr = estimator(tmp_path, monkeypatch, model, name, seed=int(g["weights_seed"]), smooth=smooth, add_mc_samples=True,
                        monte_carlo_samples=mc)
        arr.msg_as_array = True
        for rep in range(2):                             # second pass behind a reset: the same cold start
            worst = 0.0
            for f, row32 in enumerate(rows):
                msg = est.process_row(array("f", row32.tolist()))
                a = arr.process_row(array("f", row32.tolist()))
                assert isinstance(msg, list) and len(msg) == ref.shape[1]
                assert isinstance(a, np.ndarray) and a.shape == (ref.shape[1],) and np.array_equal(np.asarray(msg), a)
                worst = max(worst, float(np.abs(np.asarray(msg) - ref[f]).max()))
            print(f"process_row {model} {name} smooth {smooth} pass {rep}: max |msg - reference| = {worst:.3e}")
            assert worst < TOL_MSG_LOOP, (model, name, smooth, rep, worst)
            assert np.abs(est.get_last_msg() - ref[-1][:25]).max() < TOL_MSG_LOOP
            est.reset()
            arr.reset()
        # the staged methods (reference semantics, host histories) agree, and the consumer thread's loop is process_row
        st = estimator(tmp_path, monkeypatch, model, name, seed=int(g["weights_seed"]), smooth=smooth, add_mc_samples=True,
                       monte_carlo_samples=mc)
        st.use_device_frame = False
        for f, row32 in enumerate(rows[:8]):
            b = st.process_row(array("f", row32.tolist()))
            assert len(b) == ref.shape[1] and np.abs(np.asarray(b) - ref[f]).max() < TOL_MSG_LOOP


# ---------------- 2. lockstep banks against the single-stream estimator -------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_bank_lockstep_frames_equal_single_stream_estimators(golden, tmp_path, monkeypatch, model):
    from wear_mocap_ape_amd.streams import StreamBank
    S, frames, smooth, mc, name = 37, 12, 3, 3, "pocket"
    est = estimator(tmp_path, monkeypatch, model, name, smooth=smooth, add_mc_samples=True, monte_carlo_samples=mc)
    m, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    rows = shifted_rows(golden, name, S, frames)
    ref = np.stack([single_stream_msgs(est, rows[:, s]) for s in range(S)], axis=1)          # [frames, S, 25 + 6N]
    n = stacked(model, smooth, mc)
    assert ref.shape[2] == 25 + 6 * n
    for dtype in (torch.float32, torch.float64):
        bank = StreamBank(m, S, T, smooth=smooth, normalize=True, dtype=dtype, monte_carlo_samples=mc)
        assert bank._n_mc == (mc if model == "ff" else 1)
        for rep in range(2):                             # second pass: a cold start after reset()
            worst = 0.0
            for f in range(frames):
                bank.push_rows(torch.from_numpy(rows[f]).cuda(), kind)
                if f % 2 == 0:
                    msg, tail = bank.step(with_tail=True)
                    assert tuple(msg.shape) == (S, 25) and tuple(tail.shape) == (S, n, 6) and msg.dtype == dtype
                    got = np.concatenate([msg.cpu().numpy(), tail.cpu().numpy().reshape(S, -1)], axis=1)
                else:
                    d = bank.step_datagrams()
                    assert tuple(d.shape) == (S, 25 + 6 * n) and d.dtype == torch.float32
                    got = d.cpu().numpy()
                bank.recover()
                worst = max(worst, float(np.abs(got.astype(np.float64) - ref[f]).max()))
            print(f"lockstep {model} {dtype} pass {rep}: max |bank - estimator| = {worst:.3e}")
            assert worst < TOL_MSG_LOOP, (model, dtype, rep, worst)
            bank.reset()
        del bank


# ---------------- 3. subset frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_bank_subset_frames(golden, tmp_path, monkeypatch, model):
    from wear_mocap_ape_amd.streams import StreamBank
    S, ticks, smooth, mc, name = 37, 14, 3, 3, "pocket"
    est = estimator(tmp_path, monkeypatch, model, name, smooth=smooth, add_mc_samples=True, monte_carlo_samples=mc)
    m, T, kind = est._hip_model(), est.sequence_len, est._parse_kind
    rows = shifted_rows(golden, name, S, ticks)
    bank = StreamBank(m, S, T, smooth=smooth, normalize=True, dtype=torch.float64, monte_carlo_samples=mc)
    rng = np.random.default_rng(11)
    fed = [[] for _ in range(S)]           # per stream: rows since its cold start
    outs = [[] for _ in range(S)]
    for t in range(ticks):
        if t == 6:
            cold = rng.permutation(S)[:9]
            bank.reset(streams=cold)
            for s in cold:
                fed[s] = []
        streams = rng.permutation(S)[:int(rng.integers(1, S))]          # always at least one stream unlisted
        d = bank.frame(rows[t][streams], streams, kind, datagrams=True)
        assert tuple(d.shape) == (len(streams), 25 + 6 * stacked(model, smooth, mc))
        d = d.cpu().numpy()
        bank.recover()
        for j, s in enumerate(streams):
            fed[s].append(rows[t][s])
            outs[s].append((len(fed[s]), d[j]))
    worst = 0.0
    for s in range(S):
        if not fed[s]:
            continue
        ref = single_stream_msgs(est, np.array(fed[s]))                  # the stream's rows since its last cold start
        for k, got in outs[s][-len(fed[s]):]:
            worst = max(worst, float(np.abs(got - ref[k - 1]).max()))
    print(f"subset {model}: max |bank - estimator| = {worst:.3e}")
    assert worst < TOL_MSG_LOOP, worst
    # where the schedules coincide -- every stream, in order, every frame -- subset and lockstep frames give the same bits.  DropoutFF
    # once more at p = 0.2 and equal seeds: a lockstep row's mask is keyed by stream * n_mc + sample, a subset row's by list position *
    # n_mc + sample, both under seed + frame counter, so the masks coincide when the list is every stream in order -- and only then
    for p in ((0.0, 0.2) if model == "ff" else (0.0,)):
        a = StreamBank(m, S, T, smooth=smooth, normalize=True, dtype=torch.float64, monte_carlo_samples=mc, dropout=p, seed=5)
        b = StreamBank(m, S, T, smooth=smooth, normalize=True, dtype=torch.float64, monte_carlo_samples=mc, dropout=p, seed=5)
        c = StreamBank(m, S, T, smooth=smooth, normalize=True, dtype=torch.float64, monte_carlo_samples=mc, dropout=p, seed=6)
        for t in range(8):
            a.push_rows(torch.from_numpy(rows[t]).cuda(), kind)
            da = a.step_datagrams().cpu().numpy()
            db = b.frame(rows[t], np.arange(S), kind, datagrams=True).cpu().numpy()
            assert np.array_equal(da, db), (model, p, t, float(np.abs(da - db).max()))
            if p > 0.0:                                      # the dropout is live: the samples of a stream differ, and so do two seeds
                dc = c.frame(rows[t], np.arange(S), kind, datagrams=True).cpu().numpy()
                tail = da[:, 25:].reshape(S, -1, 6)
                assert np.abs(tail[:, 0] - tail[:, 1]).max() > 1e-4 and not np.array_equal(da, dc)
        if p > 0.0:                                          # list position keys the masks: the reversed list draws others for stream 0
            a.push_rows(torch.from_numpy(rows[8]).cuda(), kind)
            da = a.step_datagrams().cpu().numpy()
            db = b.frame(rows[8][::-1].copy(), np.arange(S)[::-1].copy(), kind, datagrams=True).cpu().numpy()[::-1]
            assert np.array_equal(da[S // 2], db[S // 2]) and not np.array_equal(da[0], db[0])
        del a, b, c
    m.recover()


# ---------------- 4. offline replay -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_process_recording(golden, tmp_path, monkeypatch, model):
    bt = golden("body_traces.npz")

    class BoneMapStandIn:                                   # the three attributes Estimator.__init__ reads from a BoneMap
        def __init__(self, i):
            self.left_lower_arm_length, self.left_upper_arm_length = (float(v) for v in bt["bm_lengths"][i])
            self.left_upper_arm_origin_rh = np.array(bt["bm_origins"][i], dtype=np.float64)
    name, smooth, mc = "pocket", 3, 3
    est = estimator(tmp_path, monkeypatch, model, name, smooth=smooth, add_mc_samples=True, monte_carlo_samples=mc)
    base = golden(f"stream_trace_{name}.npz")["rows"].astype(np.float32)
    rec = [base, base[::-1][:13].copy()]
    rows, starts = np.concatenate(rec), [0, len(base)]
    n_eff = mc if model == "ff" else 1
    ref = np.concatenate([single_stream_msgs(est, r) for r in rec])
    out, y = est.process_recording(rows, starts=starts, return_targets=True)
    assert tuple(out.shape) == (len(rows), 25 + 6 * smooth * n_eff) and out.dtype == torch.float64
    assert tuple(y.shape) == (len(rows), n_eff, est._hip_model().output_size) and y.dtype == torch.float32
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print(f"process_recording {model}: max |replay - process_row loop| = {err:.3e}")
    assert err < TOL_MSG_LOOP, err
    # several launches: the chunking changes nothing.  DropoutFF: a sample row's trunk and head do not depend on how the rows are cut
    # into launches, so the bits are the same.  ImuPoseLSTM: the launch size picks the LSTM route, so the routes' common bound holds.
    small = est.process_recording(rows, starts=starts, max_rows_per_launch=16)
    if model == "ff":
        assert torch.equal(small, out)
    else:
        assert np.abs(small.cpu().numpy() - ref).max() < TOL_MSG_LOOP
    f32 = est.process_recording(rows, starts=starts, out_dtype=torch.float32)
    assert f32.dtype == torch.float32 and np.abs(f32.cpu().numpy() - ref).max() < TOL_MSG_LOOP
    # one bonemap per recording against estimators BUILT with those bonemaps
    bms = [BoneMapStandIn(1), BoneMapStandIn(3)]
    got = est.process_recording(rows, starts=starts, bonemaps=bms).cpu().numpy()
    for r, (bm, lo) in enumerate(zip(bms, starts)):
        e2 = estimator(tmp_path, monkeypatch, model, name, smooth=smooth, add_mc_samples=True, monte_carlo_samples=mc, bonemap=bm)
        want = single_stream_msgs(e2, rec[r])
        assert np.abs(got[lo:lo + len(rec[r])] - want).max() < TOL_MSG_LOOP, (model, r)
        assert np.abs(want - ref[lo:lo + len(rec[r])]).max() > 1e-3          # the body does reach the messages


def test_ff_process_recording_under_dropout_does_not_see_the_chunking(golden, tmp_path, monkeypatch):
    """DropoutFF at p = 0.2: a replay's mask is keyed by the sample row's index in the whole call (row_base of the launch + row), so
    however the rows are cut into launches the same masks meet the same rows -- bit-equal messages and targets"""
    smooth, mc = 2, 3
    est = estimator(tmp_path, monkeypatch, "ff", "pocket", dropout=0.2, smooth=smooth, add_mc_samples=True, monte_carlo_samples=mc)
    base = golden("stream_trace_pocket.npz")["rows"].astype(np.float32)
    rows, starts = np.concatenate([base, base[::-1][:13]]), [0, len(base)]
    out, y = est.process_recording(rows, starts=starts, return_targets=True, seed=9)
    assert tuple(out.shape) == (len(rows), 25 + 6 * smooth * mc) and tuple(y.shape) == (len(rows), mc, est._hip_model().output_size)
    assert float((y[:, 0] - y[:, 1]).abs().max()) > 1e-3                 # the dropout is live: a frame's samples differ
    total = len(rows) * mc                                               # sample rows: what max_rows_per_launch counts
    for chunk in (16, 32):                                               # 16 is the smallest the entry takes; launches cut through frames
        assert total % chunk != 0 and chunk % mc != 0 and total > 2 * chunk
        o2, y2 = est.process_recording(rows, starts=starts, return_targets=True, seed=9, max_rows_per_launch=chunk)
        assert torch.equal(o2, out) and torch.equal(y2, y), chunk
    o3 = est.process_recording(rows, starts=starts, seed=10)
    assert not torch.equal(o3, out)                                      # another seed, other masks


# ---------------- 7. ImuPoseLSTM ignores the sample count -----------------------------------------------------------------------------------------
def test_imupose_ignores_the_sample_count(golden, tmp_path, monkeypatch):
    rows = golden("stream_trace_pocket.npz")["rows"]
    for smooth in (1, 4):
        a = estimator(tmp_path, monkeypatch, "imupose", "pocket", smooth=smooth, add_mc_samples=True, monte_carlo_samples=1)
        b = estimator(tmp_path, monkeypatch, "imupose", "pocket", smooth=smooth, add_mc_samples=True, monte_carlo_samples=25)
        for row32 in rows:
            ma, mb = a.process_row(array("f", row32.tolist())), b.process_row(array("f", row32.tolist()))
            assert len(ma) == len(mb) == (25 if smooth == 1 else 25 + 6 * smooth)
            assert ma == mb                                  # bit-equal
        ra, rb = a.process_recording(rows[:, :]), b.process_recording(rows[:, :])
        assert ra.shape == rb.shape and torch.equal(ra, rb)


# ---------------- 8. ImuPoseLSTM banks on both LSTM routes, against the oracle -------------------------------------------------------------------
@pytest.mark.parametrize("S", [5, 600])
def test_imupose_bank_against_the_oracle(S):
    """Both LSTM routes (first-generation wide cluster kernel at 5 streams, layer-split lstm_upper32 route at 600) and the ragged tile,
    run the way the estimator runs the bank: float64 z-score with the deployed statistics in front, float64 de-normalisation behind.

    The statistics matter to what the message bound means.  TOL_MSG_LOOP is the bound for a float32 regressor in front of the float64
    post-filter, whose first step normalises the 6D rotation columns of the DE-NORMALISED targets.  Fed the raw outputs of a
    seeded-weight model instead (small |y|, so some 6D vectors have a norm near zero), that normalisation would amplify a target error
    by the inverse of that norm and the bound would measure the inputs' conditioning; with the deployed yy_m / yy_s the vectors have the
    size the bound was made for.  The targets themselves are bounded directly below, at the tolerance the existing ImuPoseLSTM tests use."""
    from tests.test_hip_parity import TOL_Y_SHORT
    from wear_mocap_ape_amd.estimate import nn_models
    from wear_mocap_ape_amd.streams import StreamBank
    from wear_mocap_ape_amd.utility import data_stats
    from wear_mocap_ape_amd.utility.names import NNS_INPUTS, NNS_TARGETS
    cfg, T, frames = orc.MODEL_CONFIGS["pocket"], 6, 9
    I, O, layout = cfg["I"], cfg["O"], cfg["layout"]
    st = data_stats.get_norm_stats(x_inputs=NNS_INPUTS.WATCH_PHONE_CAL_HIP, y_targets=NNS_TARGETS.ORI_CAL_LARM_UARM_HIPS)
    xx_m, xx_s, yy_m, yy_s = (np.asarray(st[k], dtype=np.float64) for k in ("xx_m", "xx_s", "yy_m", "yy_s"))
    assert xx_m.shape == (I,) and yy_m.shape == (O,)
    sd = orc.make_imupose_state_dict(I, O, 8)
    m = nn_models.ImuPoseLSTM(input_size=I, hidden_layer_size=256, hidden_layer_count=2, output_size=O, device=0, target_layout=layout)
    m.load_state_dict(sd)
    m.set_body(orc.DEFAULT_BODY)
    m.set_norm_stats(xx_m, xx_s, yy_m, yy_s)
    bank = StreamBank(m, S, T, smooth=1, normalize=True, dtype=torch.float64, monte_carlo_samples=25)
    assert bank._n_mc == 1
    # raw features whose z-scores are standard normal
    x = (xx_m + xx_s * np.random.default_rng(S).normal(size=(frames, S, I))).astype(np.float32)
    worst = worst_y = 0.0
    for f in range(frames):
        bank.push_features(torch.from_numpy(x[f]).cuda())
        got = bank.step().cpu().numpy().copy()
        assert (m.last_kernel() == "ape_lstm_upper32") == (S > 512), m.last_kernel()      # the layer-split route above 512 windows
        bank.recover()                                      # a healthy model: nothing to re-issue, the outputs stay
        assert np.array_equal(bank._msg.cpu().numpy(), got)
        # the oracle's windows: the last T rows, padded with the first one on a cold start (estimator.py:96-97)
        win = np.stack([x[max(0, f - T + 1 + t)] for t in range(T)], axis=1)               # [S, T, I]
        xn = ((win.astype(np.float64) - xx_m) / xx_s).astype(np.float32)                    # estimator.py:103-104, then the f32 cast
        y = orc.imupose_forward(sd, xn)[:, -1]
        est = orc.arm_pose_from_targets(y.astype(np.float64) * yy_s + yy_m, orc.DEFAULT_BODY, layout, "closed")
        ref = np.stack([orc.msg_from_est(est[s:s + 1], orc.DEFAULT_BODY, layout) for s in range(S)])
        worst = max(worst, float(np.abs(got - ref).max()))
        # the normalised targets of the same windows on the same route, directly
        yd = m.forward(torch.from_numpy(win).cuda(), last_step_only=True, normalize_input=True).cpu().numpy()[:, 0]
        assert (m.last_kernel() == "ape_lstm_upper32") == (S > 512), m.last_kernel()
        m.recover()
        worst_y = max(worst_y, float(np.abs(yd - y).max()))
    print(f"imupose bank S={S}: max |bank - oracle| = {worst:.3e}, max |y - oracle| = {worst_y:.3e}")
    assert worst_y < TOL_Y_SHORT, worst_y
    assert worst < TOL_MSG_LOOP, worst
    assert m.stats()["aborted_checks"] == 0


# ---------------- 9. refusals that remain --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_refusals_that_remain(golden, tmp_path, monkeypatch, model):
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import nn_models
    lib = _hip.lib()
    est = estimator(tmp_path, monkeypatch, model, "pocket", smooth=2, monte_carlo_samples=3)
    m, rows = est._hip_model(), golden("stream_trace_pocket.npz")["rows"]
    # ape_replay keeps refusing a non-LSTM handle
    with pytest.raises(UserWarning, match="LSTM"):
        _replay_c(m, est._parse_kind, rows, [0], est.sequence_len, 2, 1, 0.0, 1, _hip.FLAG_NORMALIZE_INPUT, _hip.F64)
    # the fp16 precision switch (refused on these models before this feature too: pinned here so that it stays, not new behaviour)
    with pytest.raises(UserWarning):
        m.set_precision("f16")
    assert lib.ape_model_set_precision(m.handle, _hip.PRECISION_F16) != 0
    # a model without a target layout
    cfg = orc.MODEL_CONFIGS["pocket"]
    if model == "ff":
        bare = nn_models.DropoutFF(cfg["O"], FF_H, FF_L, cfg["I"], device=0, target_layout=_hip.LAYOUT_NONE)
    else:
        bare = nn_models.ImuPoseLSTM(cfg["I"], 256, 2, cfg["O"], device=0, target_layout=_hip.LAYOUT_NONE)
    bare.load_state_dict(state_dict(model, "pocket", 1))
    h = C.c_void_p()
    assert lib.ape_streams_create(bare.handle, 4, 6, 1, C.byref(h)) != 0 and b"target layout" in lib.ape_last_error()
    rd = torch.from_numpy(rows).cuda()
    st = np.zeros(1, dtype=np.int32)
    out = torch.empty((len(rows), 25), dtype=torch.float64, device="cuda")
    rc = lib.ape_replay_regressor(bare.handle, est._parse_kind, C.c_void_p(rd.data_ptr()), len(rows), C.c_void_p(st.ctypes.data), 1, 6, 1, 1,
                                  0.0, 1, 0, C.c_void_p(out.data_ptr()), _hip.F64, None, 0, None, None)
    assert rc != 0 and b"target layout" in lib.ape_last_error()
    # bad starts: refused like ape_replay refuses them
    st2 = np.array([0, 0], dtype=np.int32)
    rc = lib.ape_replay_regressor(m.handle, est._parse_kind, C.c_void_p(rd.data_ptr()), len(rows), C.c_void_p(st2.ctypes.data), 2, 6, 1, 1,
                                  0.0, 1, 0, C.c_void_p(out.data_ptr()), _hip.F64, None, 0, None, None)
    assert rc != 0 and b"seg_starts" in lib.ape_last_error()


def test_replay_regressor_serves_lstm_handles_like_replay_bodies(golden, tmp_path, monkeypatch):
    from tests.test_replay import _estimator
    from wear_mocap_ape_amd import _hip
    est = _estimator(tmp_path, monkeypatch, "pocket", 3, 0.2, smooth=2, add_mc_samples=True, monte_carlo_samples=4)
    m, rows = est._hip_model(), golden("stream_trace_pocket.npz")["rows"]
    flags = _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG
    a, _ = _replay_c(m, est._parse_kind, rows, [0, 7], est.sequence_len, 2, 4, 0.2, 99, flags, _hip.F64)
    rd = torch.from_numpy(rows).cuda()
    st = np.array([0, 7], dtype=np.int32)
    b = torch.empty_like(a)
    _hip.check(_hip.lib().ape_replay_regressor(m.handle, est._parse_kind, C.c_void_p(rd.data_ptr()), len(rows), C.c_void_p(st.ctypes.data), 2,
                                               est.sequence_len, 2, 4, 0.2, 99, flags, C.c_void_p(b.data_ptr()), _hip.F64, None, 0,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream), None), "ape_replay_regressor")
    assert torch.equal(a, b)


# ---------------- 5 / 6. FF dropout, exact and statistical: on the test-hooks library ------------------------------------------------------------------
def test_regressor_hooks_cases_on_the_test_hooks_library():
    """injected masks against the oracle and the Philox bank's distribution (targets read through a test hook) run in a CHILD process
    on lib/diag/libape_hip_testhooks.so, like tests/hooks/subset_cases.py"""
    import os
    import subprocess
    import sys
    from tests.conftest import REPO
    lib = REPO / "arm-pose-estimation_amd" / "lib" / "diag" / "libape_hip_testhooks.so"
    assert lib.exists(), "make -C arm-pose-estimation_amd/csrc hooks"
    torch.cuda.synchronize()
    env = dict(os.environ, APE_HIP_LIB=str(lib))
    r = subprocess.run([sys.executable, "-m", "pytest", str(REPO / "tests" / "hooks" / "regressor_cases.py"), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider", "-s"], env=env, cwd=str(REPO), capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
