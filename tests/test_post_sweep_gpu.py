"""Post-filter sweep (`ape_post_sweep`) on the GPU: one replay's targets re-smoothed at many (smooth, samples).

Base case: pocket model with seeded weights, dropout 0.2, M = 6 samples, F = 150 frames in recordings of 3, 37, 1 and 109 frames (two
shorter than every multi-frame stack, one boundary right behind another), seven configurations.  Where a configuration takes all M
samples the sweep must give the bits of the replay at that configuration; a configuration of m < M samples those of an m-sample replay
whose targets are the first m of every frame; every configuration the float64 statement `post_sweep_numpy`
(tests/test_post_sweep_cpu.py) within 1e-12 (messages, the figure of test_replay_post_filter_exact) and the tolerances of
tests/test_spread_gpu.py (records)."""
import ctypes as C
from array import array

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests.test_post_sweep_cpu import post_sweep_numpy
from tests.test_replay import _estimator, _replay_c, _seg_of, _stack_msgs, _synthetic_rows, _targets_to_est
from tests.test_spread_gpu import check_record

pytestmark = pytest.mark.gpu

F, M, STARTS, SEED = 150, 6, [0, 3, 40, 41], 0x5EED
CONFIGS = [(1, 1), (1, 6), (2, 1), (3, 6), (7, 6), (7, 4), (5, 2)]
MSG_TOL = 1e-12


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def pocket(tmp, smooth, mc, name="pocket", seed=2, **kw):
    """an estimator with seeded weights and dropout 0.2 (the deploy path is patched while it is built, no longer)"""
    with pytest.MonkeyPatch.context() as patch:
        return _estimator(tmp, patch, name, seed, 0.2, smooth=smooth, add_mc_samples=True, monte_carlo_samples=mc, **kw)


@pytest.fixture(scope="module")
def base(golden, tmp_path_factory):
    """the base case, made once: estimator (smooth 3, 6 samples), rows, its replay's y, the sweep and the numpy statement of it"""
    tmp = tmp_path_factory.mktemp("post_sweep")
    est = pocket(tmp, 3, M)
    rows = _synthetic_rows(golden, "pocket", F, 21)
    out3, y, rec3 = est.process_recording(rows, starts=STARTS, return_targets=True, spread=True, seed=SEED)
    out, spread = est.repost(y, CONFIGS, starts=STARTS, spread=True)
    torch.cuda.synchronize()
    ref = post_sweep_numpy(y.cpu().numpy(), est._yy_m, est._yy_s, est.body_measurements, est._layout, STARTS, CONFIGS)
    return {"tmp": tmp, "est": est, "rows": rows, "y": y, "out": out, "spread": spread, "ref": ref, "replay3": (out3, rec3)}


def against_numpy(est, y, starts, configs, out, spread, bodies=None, what=""):
    """test 3's check of a sweep against the float64 statement; -> (worst message deviation, worst record deviation in bounds)"""
    yh = y.cpu().numpy()
    body = est.body_measurements if bodies is None else bodies
    ref_out, ref_spread = post_sweep_numpy(yh, est._yy_m, est._yy_s, body, est._layout, starts, configs)
    return compare(yh, est, starts, configs, out, spread, ref_out, ref_spread, what)


def compare(yh, est, starts, configs, out, spread, ref_out, ref_spread, what=""):
    E = _targets_to_est(est, yh)                            # (only the magnitudes of est[:, :6] enter the records' bound)
    seg = _seg_of(yh.shape[0], starts)
    o, s = out.cpu().numpy(), spread.cpu().numpy()
    worst_msg, worst_rec = 0.0, 0.0
    for c, (sm, m) in enumerate(configs):
        worst_msg = max(worst_msg, float(np.abs(o[c] - ref_out[c]).max()))
        for f in range(yh.shape[0]):
            stack = np.concatenate([E[max(seg[f], f - sm + 1 + j), :m] for j in range(sm)])
            worst_rec = max(worst_rec, check_record(s[c, f], ref_spread[c, f], stack, sm * m, (what, c, f)))
    print(f"{what}: worst |msg - numpy| = {worst_msg:.3e} (bound {MSG_TOL:g}), worst record deviation = {worst_rec:.3f} of its bound")
    assert worst_msg <= MSG_TOL, (what, worst_msg)
    return worst_msg, worst_rec


# ---------------- 1. bits of the replay -----------------------------------------------------------------------------------------------------
def test_full_sample_configurations_give_the_bits_of_the_replay(base):
    from wear_mocap_ape_amd import score
    out, spread, y = base["out"], base["spread"], base["y"]
    assert tuple(out.shape) == (7, F, 25) and tuple(spread.shape) == (7, F, 21) and out.dtype == torch.float64 and out.is_cuda
    assert out.data_ptr() == spread.data_ptr() - 25 * 8                  # two views of one tensor
    plan = score.post_sweep_last()
    assert plan["passes"] == 1 and plan["chunk_frames"] == F and plan["lds"], plan       # the base case runs on LDS tiles
    for c, (smooth, m) in enumerate(CONFIGS):
        if m != M:
            continue
        if smooth == 3:
            ro, rr = base["replay3"]
        else:
            e = pocket(base["tmp"], smooth, M)
            ro, yr, rr = e.process_recording(base["rows"], starts=STARTS, return_targets=True, spread=True, seed=SEED)
            assert torch.equal(yr, y), smooth                            # the regressor does not see smooth
        assert torch.equal(ro[:, :25], out[c]) and torch.equal(rr, spread[c]), (smooth, m)
    # the unspread call writes the same messages
    plain = base["est"].repost(y, CONFIGS, starts=STARTS)
    assert tuple(plain.shape) == (7, F, 25) and plain.is_contiguous() and torch.equal(plain, out)


# ---------------- 2. prefix selection -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth,m", [(7, 4), (5, 2)])
def test_prefix_selection(base, smooth, m):
    e = pocket(base["tmp"], smooth, m)
    om, ym, rm = e.process_recording(base["rows"], starts=STARTS, return_targets=True, spread=True, seed=SEED)
    y_big = torch.full((F, M, ym.shape[2]), float("nan"), dtype=torch.float32, device=ym.device)
    y_big[:, :m] = ym
    out, spread = e.repost(y_big, [(1, M), (smooth, m)], starts=STARTS, spread=True)       # (1, M): all six rows are converted
    assert torch.equal(out[1], om[:, :25]) and torch.equal(spread[1], rm)                   # no row outside the prefix is read
    assert bool(out[0].isnan().any(dim=1).all())                                           # ... and the NaNs are there
    # the configuration alone: rows k >= m are not even converted
    out1, spread1 = e.repost(y_big, [(smooth, m)], starts=STARTS, spread=True)
    assert torch.equal(out1[0], om[:, :25]) and torch.equal(spread1[0], rm)


# ---------------- 3. the float64 statement --------------------------------------------------------------------------------------------------
def test_every_configuration_against_the_numpy_statement(base):
    yh = base["y"].cpu().numpy()
    compare(yh, base["est"], STARTS, CONFIGS, base["out"], base["spread"], *base["ref"], what="base case")


# ---------------- 4. at the limits ----------------------------------------------------------------------------------------------------------
def test_at_the_limits(base, golden):
    from wear_mocap_ape_amd import score
    n, starts, configs = 70, [0, 30], [(64, 64), (64, 1), (1, 64)]
    e = pocket(base["tmp"], 64, 64)
    rows = _synthetic_rows(golden, "pocket", n, 5)
    ro, y, rr = e.process_recording(rows, starts=starts, return_targets=True, spread=True, seed=SEED)
    out, spread = e.repost(y, configs, starts=starts, spread=True)
    plan = score.post_sweep_last()
    assert not plan["lds"] and plan["passes"] == 1, plan    # a frame's 64 rows x 64 frames of halo: far more than a CU's LDS
    assert torch.equal(out[0], ro[:, :25]) and torch.equal(spread[0], rr)
    against_numpy(e, y, starts, configs, out, spread, what="limits")
    # in several passes, the carried-over 63 frames longer than a pass
    rule = score.post_sweep_plan(e._layout, n, configs, 2 * (63 + 20) * 8 * 21 * 64)
    assert rule["passes"] == 4
    out2, spread2 = e.repost(y, configs, starts=starts, spread=True, workspace_bytes=2 * (63 + 20) * 8 * 21 * 64)
    assert score.post_sweep_last()["passes"] == 4 and torch.equal(out2, out) and torch.equal(spread2, spread)


# ---------------- 5. the workspace bound does not show --------------------------------------------------------------------------------------
def test_workspace_bound_does_not_show(base):
    from wear_mocap_ape_amd import score
    est, y = base["est"], base["y"]
    bound = 2 * (6 + 30) * 8 * 21 * 6                       # two buffers of 6 carried-over + 30 frames of 6 rows of 21 float64
    rule = score.post_sweep_plan(est._layout, F, CONFIGS, bound)
    assert rule["passes"] == 5 and rule["chunk_frames"] == 30
    out, spread = est.repost(y, CONFIGS, starts=STARTS, spread=True, workspace_bytes=bound)
    last = score.post_sweep_last()
    assert last["passes"] == 5 and last["chunk_frames"] == 30, last
    assert torch.equal(out, base["out"]) and torch.equal(spread, base["spread"])
    for tiny in (2 * 7 * 8 * 21 * 6, 2 * 9 * 8 * 21 * 6):  # one and three frames a pass: every pass shorter than the halo
        o, s = est.repost(y, CONFIGS, starts=STARTS, spread=True, workspace_bytes=tiny)
        assert score.post_sweep_last()["passes"] == score.post_sweep_plan(est._layout, F, CONFIGS, tiny)["passes"] >= 50
        assert torch.equal(o, base["out"]) and torch.equal(s, base["spread"]), tiny
    again, again_s = est.repost(y, CONFIGS, starts=STARTS, spread=True)
    assert torch.equal(again, base["out"]) and torch.equal(again_s, base["spread"])         # the same arguments, the same bits
    with pytest.raises(UserWarning, match="holds no frame"):
        est.repost(y, CONFIGS, starts=STARTS, workspace_bytes=2 * 7 * 8 * 21 * 6 - 1)
    # a single configuration leaves an LDS tile's lanes idle: the rows are read from the workspace, with the same bits
    o1, s1 = est.repost(y, [(7, 6)], starts=STARTS, spread=True)
    assert not score.post_sweep_last()["lds"] and torch.equal(o1[0], base["out"][4]) and torch.equal(s1[0], base["spread"][4])


# ---------------- 6. other layouts and models -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,smooth,m", [("watch", 10, 6), ("uarm", 4, 5)])
def test_other_estimators_against_their_replays(base, golden, name, smooth, m):
    e = pocket(base["tmp"], smooth, m, name=name, seed=4)
    rows = _synthetic_rows(golden, name, 60, 8)
    starts = [0, 7, 8]
    ro, y, rr = e.process_recording(rows, starts=starts, return_targets=True, spread=True, seed=11)
    configs = [(smooth, m), (1, 1), (smooth + 1, m - 1)] + [(2, 2)] * 6          # (a list long enough for LDS tiles)
    out, spread = e.repost(y, configs, starts=starts, spread=True)
    assert torch.equal(out[0], ro[:, :25]) and torch.equal(spread[0], rr)
    assert torch.equal(out[3], out[8]) and torch.equal(spread[3], spread[8])
    against_numpy(e, y, starts, configs[:4], out[:4], spread[:4], what=name)


def test_position_layout_through_the_c_abi(golden, norm_stats):
    """the 20-target layout, set up as test_replay_post_filter_exact_position_layout"""
    from wear_mocap_ape_amd import _hip, score
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
    ro, y = _replay_c(m, _hip.PARSE_WATCH_PHONE_POCKET, rows, starts, 6, smooth, mc, 0.2, 99, _hip.FLAG_NORMALIZE_INPUT, _hip.F64, want_y=True)
    configs = [(smooth, mc), (2, 5), (1, 1), (5, 3)] * 3
    out = score.post_sweep(m, y, configs, starts)
    assert score.post_sweep_last()["lds"]
    assert torch.equal(out[0], ro) and torch.equal(out[:4], out[4:8])
    pred = y.cpu().numpy().reshape(-1, 20).astype(np.float64) * yy_s + yy_m
    E = orc.arm_pose_from_targets(pred, orc.DEFAULT_BODY, 2, route="closed").reshape(30, mc, 21)
    worst = 0.0
    for c, (s, k) in enumerate(configs[:4]):
        ref = _stack_msgs(E[:, :k], _seg_of(30, starts), s, orc.DEFAULT_BODY, 2, False, range(30))
        worst = max(worst, float(np.abs(out[c].cpu().numpy() - ref).max()))
    print(f"position layout: worst |msg - oracle| = {worst:.3e}")
    assert worst < MSG_TOL
    o1 = score.post_sweep(m, y, configs[:1], starts)        # ... and read from the workspace
    assert not score.post_sweep_last()["lds"] and torch.equal(o1[0], ro)
    # what needs a model to be refused
    lib, dummy = _hip.lib(), C.c_void_p(256)
    cf, s0 = np.array([[64, 8]], dtype=np.int32), np.zeros(1, dtype=np.int32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(model, ws=0, stream=stream):
        return lib.ape_post_sweep(model.handle, C.c_void_p(y.data_ptr()), 30, mc, C.c_void_p(s0.ctypes.data), 1, C.c_void_p(cf.ctypes.data), 1, 0,
                                  None, 0, C.c_void_p(out.data_ptr()), _hip.F64, ws, stream)
    assert call(m, 2 * 64 * 8 * 21 * 8 - 1) == 1 and b"holds no frame" in lib.ape_last_error()
    bare = nn_models.DropoutLSTM(22, 256, 2, 20, dropout=0.2, device=0, target_layout=_hip.LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS)
    bare.load_state_dict(sd)
    assert call(bare) == 3 and b"norm stats" in lib.ape_last_error()                       # APE_ERR_NOT_READY
    none = nn_models.DropoutLSTM(22, 256, 2, 20, dropout=0.2, device=0, target_layout=_hip.LAYOUT_NONE)
    assert call(none) == 1 and b"target layout" in lib.ape_last_error()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    before, scratch = out.clone(), torch.zeros((4,), device="cuda")
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            rc = call(m, stream=C.c_void_p(side.cuda_stream))
            msg = lib.ape_last_error()
    torch.cuda.current_stream().wait_stream(side)
    assert rc == 1 and b"capturing" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(out, before)                         # nothing was written


@pytest.mark.parametrize("model", ["ff", "imupose"])
def test_other_regressors_against_their_replays(golden, tmp_path, monkeypatch, model):
    from tests.test_regressor_banks_gpu import estimator
    smooth, mc = 3, 3
    e = estimator(tmp_path, monkeypatch, model, "pocket", dropout=0.2 if model == "ff" else 0.0, smooth=smooth, add_mc_samples=True,
                  monte_carlo_samples=mc)
    base_rows = golden("stream_trace_pocket.npz")["rows"].astype(np.float32)
    rows, starts = np.concatenate([base_rows, base_rows[::-1][:13]]), [0, len(base_rows)]
    ro, y, rr = e.process_recording(rows, starts=starts, return_targets=True, spread=True, seed=9)
    n = mc if model == "ff" else 1
    assert y.shape[1] == n
    configs = [(smooth, n), (1, 1), (2, n)] * 4
    out, spread = e.repost(y, configs, starts=starts, spread=True)
    assert torch.equal(out[0], ro[:, :25]) and torch.equal(spread[0], rr)
    against_numpy(e, y, starts, configs[:3], out[:3], spread[:3], what=model)


def test_per_recording_bodies(base, golden):
    bt = golden("body_traces.npz")

    class BoneMapStandIn:
        def __init__(self, i):
            self.left_lower_arm_length, self.left_upper_arm_length = (float(v) for v in bt["bm_lengths"][i])
            self.left_upper_arm_origin_rh = np.array(bt["bm_origins"][i], dtype=np.float64)
    from wear_mocap_ape_amd.data_types.bone_map import bodies_from
    est = base["est"]
    bms = [BoneMapStandIn(1), None, BoneMapStandIn(3), BoneMapStandIn(2)]
    ro, y, rr = est.process_recording(base["rows"], starts=STARTS, return_targets=True, spread=True, seed=SEED, bonemaps=bms)
    assert torch.equal(y, base["y"]) and not torch.equal(ro[:, :25], base["replay3"][0][:, :25])
    out, spread = est.repost(y, CONFIGS, starts=STARTS, bonemaps=bms, spread=True)
    assert torch.equal(out[3], ro[:, :25]) and torch.equal(spread[3], rr)
    against_numpy(est, y, STARTS, CONFIGS, out, spread, bodies=bodies_from(bms, 4), what="bodies")
    one = est.repost(y, [(3, 6)], starts=STARTS, bonemaps=bodies_from(bms, 4))             # ... values, and read from the workspace
    assert torch.equal(one[0], ro[:, :25])


# ---------------- 7. a bad sample stays where it is -----------------------------------------------------------------------------------------
def test_a_bad_sample_stays_where_it_is(base):
    est, y = base["est"], base["y"].clone()
    y[60, 2, 3] = float("nan")
    out, spread = est.repost(y, CONFIGS, starts=STARTS, spread=True)
    for c, (smooth, m) in enumerate(CONFIGS):
        hit = np.zeros(F, dtype=bool)
        if m > 2:
            hit[60:60 + smooth] = True                      # frame 60 is in the stacks of frames 60 .. 60 + smooth - 1 (recording 41 ..)
        keep = torch.as_tensor(~hit, device=out.device)
        assert torch.equal(out[c][keep], base["out"][c][keep]) and torch.equal(spread[c][keep], base["spread"][c][keep]), (smooth, m)
        if hit.any():
            bad = torch.as_tensor(hit, device=out.device)
            assert bool(out[c][bad].isnan().any(dim=1).all()) and bool(spread[c][bad].isnan().any(dim=1).all()), (smooth, m)
    # sample 2 of recording 1's last frame (39): frames 40 (a recording of its own) and 41 .. do not see it
    y2 = base["y"].clone()
    y2[39, 5, :] = float("nan")
    o2, _ = est.repost(y2, CONFIGS, starts=STARTS, spread=True)
    assert torch.equal(o2[:, 40:], base["out"][:, 40:]) and torch.equal(o2[:, :39], base["out"][:, :39])
    assert bool(o2[4, 39].isnan().any()) and torch.equal(o2[0], base["out"][0])


# ---------------- 8. float32 output ---------------------------------------------------------------------------------------------------------
def test_float32_output_is_the_float64_result_rounded_once(base):
    o32, s32 = base["est"].repost(base["y"], CONFIGS, starts=STARTS, spread=True, out_dtype=torch.float32)
    assert o32.dtype == torch.float32 and torch.equal(o32, base["out"].float()) and torch.equal(s32, base["spread"].float())
    p32 = base["est"].repost(base["y"], [(7, 6)], starts=STARTS, out_dtype=torch.float32, workspace_bytes=2 * 36 * 8 * 21 * 6)
    assert torch.equal(p32[0], base["out"][4].float())


# ---------------- 9. end to end -------------------------------------------------------------------------------------------------------------
def test_sweep_recording_end_to_end(base):
    from wear_mocap_ape_amd import score
    est, rows, y = base["est"], base["rows"], base["y"]
    t = y.double().mean(dim=1) * torch.as_tensor(est._yy_s, device=y.device) + torch.as_tensor(est._yy_m, device=y.device)
    seg = _seg_of(F, STARTS)
    late = torch.as_tensor(np.maximum(seg, np.arange(F) - 2), device=y.device)
    truth = t[late].contiguous()                            # the truth trails by two frames inside every recording
    for r in rows[:4]:
        est.process_row(array("f", r.tolist()))
    before = est.get_state()
    lags, smooths, samples = (-3, 3), [1, 3, 7], [6, 2]
    res = est.sweep_recording(rows, truth, smooths, samples, starts=STARTS, lags=lags, seed=SEED)
    assert res["configs"] == score.grid(smooths, samples) and res["acc"].shape == (6, 4, 7, 25) and len(res["best"]) == 6
    assert est._smooth == 3 and est._frame_samples() == M
    after = est.get_state()
    assert after["desc"] == before["desc"] and after["warm"] == before["warm"]
    assert np.array_equal(after["window"], before["window"]) and np.array_equal(after["stack"], before["stack"])
    for c, (smooth, m) in enumerate(res["configs"]):
        assert repr(res["best"][c]) == repr(score.best_lag(res["acc"][c], lags))       # (repr: NaN fields of the empty supports)
        if m != M:
            continue
        e = est if smooth == 3 else pocket(base["tmp"], smooth, M)
        ro, rr = e.process_recording(rows, starts=STARTS, spread=True, seed=SEED)
        acc = score.score_lags(e._layout, ro, truth, lags, "targets", rr, STARTS, e.sequence_len - 1, e.body_measurements)[1]
        assert np.array_equal(res["acc"][c], acc.cpu().numpy()), (smooth, m)
    print("lags found in the 109-frame recording:", [(cfg, b[3]["lag"]) for cfg, b in zip(res["configs"], res["best"])])
