"""Windowed post-filter (`ape_post_window`) on the GPU: one replay's targets re-smoothed at windows that look ahead
and at tapered weights.

Base case: the sweep's (tests/test_post_sweep_gpu.py) -- pocket model with seeded weights, dropout 0.2, M = 6 samples, F = 150 frames in
recordings of 3, 37, 1 and 109 frames -- at ten windows: five causal uniform ones, which must give the bits of `repost` (and through it of
the replay), three uniform ones that look ahead, which must give `repost`'s bits of a later frame, and two tapered ones.  Every window
and frame is held to the float64 statement `score.post_window_numpy` within 1e-12 (messages) and the derived bound of
tests/test_spread_gpu.py (records); only that check reaches the last `ahead` frames of a recording and the 1- and 3-frame recordings
where both clamps act at once."""
import ctypes as C
from array import array

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests.test_post_sweep_gpu import MSG_TOL, pocket
from tests.test_post_window_cpu import LAGS, SKIP, planted
from tests.test_replay import _replay_c, _synthetic_rows, _targets_to_est
from tests.test_spread_gpu import check_record

pytestmark = pytest.mark.gpu

F, M, STARTS, SEED = 150, 6, [0, 3, 40, 41], 0x5EED
ENDS = STARTS[1:] + [F]


def windows_of(score):
    return [(0, 0, 1), (0, 0, 6), (2, 0, 6), (6, 0, 6), (6, 0, 4), (3, 3, 6), (0, 6, 4), (4, 2, 2),
            score.window(3, 3, 6, "triangle"), score.window(5, 1, 6, "hann")]


CAUSAL = {0: (1, 1), 1: (1, 6), 2: (3, 6), 3: (7, 6), 4: (7, 4)}        # window index -> repost's (smooth, samples)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


@pytest.fixture(scope="module")
def base(golden, tmp_path_factory):
    """the base case, made once: estimator, rows, its replay's y, the windows' result and the numpy statement of it"""
    from wear_mocap_ape_amd import score
    tmp = tmp_path_factory.mktemp("post_window")
    est = pocket(tmp, 3, M)
    rows = _synthetic_rows(golden, "pocket", F, 21)
    _, y = est.process_recording(rows, starts=STARTS, return_targets=True, seed=SEED)
    windows = windows_of(score)
    out, spread = est.repost_windows(y, windows, starts=STARTS, spread=True)
    last = score.post_window_last()
    torch.cuda.synchronize()
    ref = score.post_window_numpy(y.cpu().numpy(), est._yy_m, est._yy_s, est.body_measurements, est._layout, STARTS, windows)
    return {"tmp": tmp, "est": est, "rows": rows, "y": y, "windows": windows, "out": out, "spread": spread, "ref": ref, "last": last}


def compare(est, yh, starts, windows, out, spread, ref, what="", E=None):
    """a result against the float64 statement `ref`: messages within MSG_TOL, records within check_record's bound at the stack height"""
    from wear_mocap_ape_amd import score
    E = _targets_to_est(est, yh) if E is None else E         # (only the magnitudes of est[:, :6] enter the records' bound)
    n_frames = yh.shape[0]
    ends = list(starts[1:]) + [n_frames]
    o, s = out.cpu().numpy(), spread.cpu().numpy()
    worst_msg, worst_rec = 0.0, 0.0
    for c, (back, ahead, m, _) in enumerate(score._windows(windows)[0]):
        worst_msg = max(worst_msg, float(np.abs(o[c] - ref[0][c]).max()))
        for a, b in zip(starts, ends):
            for f in range(a, b):
                stack = np.concatenate([E[min(b - 1, max(a, f - back + j)), :m] for j in range(back + ahead + 1)])
                worst_rec = max(worst_rec, check_record(s[c, f], ref[1][c, f], stack, (back + ahead + 1) * m, (what, c, f)))
    print(f"{what}: worst |msg - numpy| = {worst_msg:.3e} (bound {MSG_TOL:g}), worst record deviation = {worst_rec:.3f} of its bound")
    assert worst_msg <= MSG_TOL, (what, worst_msg)


def against_numpy(est, y, starts, windows, out, spread, bodies=None, what=""):
    from wear_mocap_ape_amd import score
    yh = y.cpu().numpy()
    ref = score.post_window_numpy(yh, est._yy_m, est._yy_s, est.body_measurements if bodies is None else bodies, est._layout, starts, windows)
    compare(est, yh, starts, windows, out, spread, ref, what)


# ---------------- 1. bits of the causal sweep -----------------------------------------------------------------------------------------------
def test_causal_uniform_windows_give_the_bits_of_the_sweep(base):
    est, y, out, spread = base["est"], base["y"], base["out"], base["spread"]
    assert tuple(out.shape) == (10, F, 25) and tuple(spread.shape) == (10, F, 21) and out.dtype == torch.float64 and out.is_cuda
    assert out.data_ptr() == spread.data_ptr() - 25 * 8                  # two views of one tensor
    assert base["last"]["passes"] == 1 and base["last"]["chunk_frames"] == F and base["last"]["lds"], base["last"]
    so, ss = est.repost(y, list(CAUSAL.values()), starts=STARTS, spread=True)
    for k, c in enumerate(CAUSAL):
        assert torch.equal(out[c], so[k]) and torch.equal(spread[c], ss[k]), (c, CAUSAL[c])
    # ... and through it the replay's (smooth 3, all six samples)
    ro, rr = est.process_recording(base["rows"], starts=STARTS, spread=True, seed=SEED)
    assert torch.equal(out[2], ro[:, :25]) and torch.equal(spread[2], rr)
    # the unspread call writes the same messages
    plain = est.repost_windows(y, base["windows"], starts=STARTS)
    assert tuple(plain.shape) == (10, F, 25) and plain.is_contiguous() and torch.equal(plain, out)


# ---------------- 2. the shift identity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,ahead,config", [(5, 3, (7, 6)), (6, 6, (7, 4))])
def test_a_window_that_looks_ahead_is_the_sweep_at_a_later_frame(base, c, ahead, config):
    so, ss = base["est"].repost(base["y"], [config], starts=STARTS, spread=True)
    checked = 0
    for s, e in zip(STARTS, ENDS):
        if e - ahead > s:                                   # every f <= e - 1 - ahead
            assert torch.equal(base["out"][c, s:e - ahead], so[0, s + ahead:e]), (c, s)
            assert torch.equal(base["spread"][c, s:e - ahead], ss[0, s + ahead:e]), (c, s)
            checked += e - ahead - s
    assert checked == sum(max(0, e - s - ahead) for s, e in zip(STARTS, ENDS)) >= 100


# ---------------- 3. the float64 statement --------------------------------------------------------------------------------------------------
def test_every_window_against_the_numpy_statement(base):
    compare(base["est"], base["y"].cpu().numpy(), STARTS, base["windows"], base["out"], base["spread"], base["ref"], what="base case")


# ---------------- 4. at the limits ----------------------------------------------------------------------------------------------------------
def test_at_the_limits(base):
    from wear_mocap_ape_amd import score
    est = base["est"]
    n, starts, windows = 70, [0, 30], [(63, 0, 64), (0, 63, 64), (32, 31, 64), (0, 0, 64), (63, 0, 1)]
    y = torch.randn((n, 64, 14), generator=torch.Generator().manual_seed(7)).cuda()
    out, spread = est.repost_windows(y, windows, starts=starts, spread=True)
    plan = score.post_window_last()
    assert not plan["lds"] and plan["passes"] == 1, plan    # a frame's 64 rows x 126 frames of halo: far more than a CU's LDS
    so, ss = est.repost(y, [(64, 64), (64, 1)], starts=starts, spread=True)
    assert torch.equal(out[0], so[0]) and torch.equal(spread[0], ss[0]) and torch.equal(out[4], so[1]) and torch.equal(spread[4], ss[1])
    against_numpy(est, y, starts, windows, out, spread, what="limits")
    # in several passes, the carried-over 126 frames longer than a pass
    bound = 2 * (126 + 20) * 8 * 21 * 64
    assert score.post_window_plan(est._layout, n, windows, bound)["passes"] == 4
    out2, spread2 = est.repost_windows(y, windows, starts=starts, spread=True, workspace_bytes=bound)
    assert score.post_window_last()["passes"] == 4 and torch.equal(out2, out) and torch.equal(spread2, spread)


# ---------------- 5. the workspace bound does not show --------------------------------------------------------------------------------------
def test_workspace_bound_does_not_show(base):
    from wear_mocap_ape_amd import score
    est, y, windows = base["est"], base["y"], base["windows"]
    frame = 8 * 21 * 6                                      # 6 rows of 21 float64; H = A = 6
    for bound, passes, chunk in ((2 * (12 + 30) * frame, 5, 30), (2 * 15 * frame, 50, 3), (2 * 13 * frame, 150, 1)):
        rule = score.post_window_plan(est._layout, F, windows, bound)
        assert rule["passes"] == passes and rule["chunk_frames"] == chunk
        out, spread = est.repost_windows(y, windows, starts=STARTS, spread=True, workspace_bytes=bound)
        last = score.post_window_last()
        assert last["passes"] == passes and last["chunk_frames"] == chunk, last
        assert torch.equal(out, base["out"]) and torch.equal(spread, base["spread"]), bound
    again, again_s = est.repost_windows(y, windows, starts=STARTS, spread=True)
    assert torch.equal(again, base["out"]) and torch.equal(again_s, base["spread"])         # the same arguments, the same bits
    with pytest.raises(UserWarning, match="holds no frame"):
        est.repost_windows(y, windows, starts=STARTS, workspace_bytes=2 * 13 * frame - 1)
    # a single window leaves an LDS tile's lanes idle: rows and weights are read from the workspace, with the same bits
    for c in (5, 8, 9):
        o1, s1 = est.repost_windows(y, [windows[c]], starts=STARTS, spread=True)
        assert not score.post_window_last()["lds"] and torch.equal(o1[0], base["out"][c]) and torch.equal(s1[0], base["spread"][c]), c


# ---------------- 6. other layouts ----------------------------------------------------------------------------------------------------------
def test_watch_only_layout(base, golden):
    from wear_mocap_ape_amd import score
    e = pocket(base["tmp"], 10, 6, name="watch", seed=4)
    rows = _synthetic_rows(golden, "watch", 60, 8)
    starts = [0, 7, 8]
    ro, y, rr = e.process_recording(rows, starts=starts, return_targets=True, spread=True, seed=11)
    assert y.shape[2] == 12
    windows = [(9, 0, 6), (2, 2, 6), score.window(3, 1, 5, "hann")] + [(1, 1, 2)] * 6          # (a list long enough for LDS tiles)
    out, spread = e.repost_windows(y, windows, starts=starts, spread=True)
    assert score.post_window_last()["lds"]
    assert torch.equal(out[0], ro[:, :25]) and torch.equal(spread[0], rr)
    so, ss = e.repost(y, [(10, 6)], starts=starts, spread=True)
    assert torch.equal(out[0], so[0]) and torch.equal(spread[0], ss[0])
    assert torch.equal(out[3], out[8]) and torch.equal(spread[3], spread[8])
    assert bool((spread[:, :, 20] == 0).all())                          # no hips: the third angle is exactly 0
    against_numpy(e, y, starts, windows[:4], out[:4], spread[:4], what="watch")


def test_position_layout_through_the_c_abi(golden, norm_stats):
    """the 20-target layout, set up as tests/test_post_sweep_gpu.py::test_position_layout_through_the_c_abi; and what needs a model to
    be refused"""
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
    windows = [(2, 0, 8), (2, 2, 5), score.window(1, 3, 3, "triangle"), (0, 0, 1)] * 3
    out, spread = score.post_window(m, y, windows, starts, spread=True)
    assert score.post_window_last()["lds"]
    assert torch.equal(out[0], ro) and torch.equal(out[:4], out[4:8]) and torch.equal(spread[:4], spread[8:])
    assert torch.equal(out[0], score.post_sweep(m, y, [(3, 8)], starts)[0])
    yh = y.cpu().numpy()
    ref = score.post_window_numpy(yh, yy_m, yy_s, orc.DEFAULT_BODY, 2, starts, windows[:4])
    pred = yh.reshape(-1, 20).astype(np.float64) * yy_s + yy_m
    E = orc.arm_pose_from_targets(pred, orc.DEFAULT_BODY, 2, route="closed").reshape(30, mc, 21)
    compare(None, yh, starts, windows[:4], out[:4], spread[:4], ref, what="position layout", E=E)
    o1 = score.post_window(m, y, windows[1:2], starts)      # ... and read from the workspace
    assert not score.post_window_last()["lds"] and torch.equal(o1[0], out[1])
    # what needs a model to be refused
    lib = _hip.lib()
    wn, s0 = np.array([[31, 32, 8]], dtype=np.int32), np.zeros(1, dtype=np.int32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    before = out.clone()

    def call(model, ws=0, stream=stream):
        return lib.ape_post_window(model.handle, C.c_void_p(y.data_ptr()), 30, mc, C.c_void_p(s0.ctypes.data), 1, C.c_void_p(wn.ctypes.data), None, 1,
                                   0, None, 0, C.c_void_p(out.data_ptr()), _hip.F64, ws, stream)
    assert call(m, 2 * 64 * 8 * 21 * 8 - 1) == 1 and b"holds no frame" in lib.ape_last_error()
    assert str(2 * 64 * 8 * 21 * 8).encode() in lib.ape_last_error()   # ... and names the smallest bound that works
    bare = nn_models.DropoutLSTM(22, 256, 2, 20, dropout=0.2, device=0, target_layout=_hip.LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS)
    bare.load_state_dict(sd)
    assert call(bare) == 3 and b"norm stats" in lib.ape_last_error()                       # APE_ERR_NOT_READY
    none = nn_models.DropoutLSTM(22, 256, 2, 20, dropout=0.2, device=0, target_layout=_hip.LAYOUT_NONE)
    assert call(none) == 1 and b"target layout" in lib.ape_last_error()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros((4,), device="cuda")
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


# ---------------- 7. per-recording bodies ---------------------------------------------------------------------------------------------------
def test_per_recording_bodies(base, golden):
    bt = golden("body_traces.npz")

    class BoneMapStandIn:
        def __init__(self, i):
            self.left_lower_arm_length, self.left_upper_arm_length = (float(v) for v in bt["bm_lengths"][i])
            self.left_upper_arm_origin_rh = np.array(bt["bm_origins"][i], dtype=np.float64)
    from wear_mocap_ape_amd.data_types.bone_map import bodies_from
    est, y, windows = base["est"], base["y"], base["windows"]
    bms = [BoneMapStandIn(1), None, BoneMapStandIn(3), BoneMapStandIn(2)]              # three bodies and the default
    out, spread = est.repost_windows(y, windows, starts=STARTS, bonemaps=bms, spread=True)
    against_numpy(est, y, STARTS, windows, out, spread, bodies=bodies_from(bms, 4), what="bodies")
    # the quaternions do not see the body, the origins do
    assert torch.equal(out[:, :, 7:11], base["out"][:, :, 7:11]) and not torch.equal(out[:, :, 4:7], base["out"][:, :, 4:7])
    so = est.repost(y, [CAUSAL[3]], starts=STARTS, bonemaps=bms)
    assert torch.equal(out[3], so[0])
    one = est.repost_windows(y, [windows[8]], starts=STARTS, bonemaps=bodies_from(bms, 4))   # ... values, and read from the workspace
    assert torch.equal(one[0], out[8])


# ---------------- 8. a bad sample stays where it is -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,k", [(60, 2), (39, 5), (40, 0)])
def test_a_bad_sample_stays_where_it_is(base, h, k):
    """the NaN sample (h, k) changes exactly the frames whose clamped windows hold frame h and whose m > k: frames h - ahead .. h + back of
    h's recording -- and, where h is the recording's last (first) frame, every frame within `ahead` (`back`) of it"""
    from wear_mocap_ape_amd import score
    est, y = base["est"], base["y"].clone()
    y[h, k, 3] = float("nan")
    out, spread = est.repost_windows(y, base["windows"], starts=STARTS, spread=True)
    s, e = next((a, b) for a, b in zip(STARTS, ENDS) if a <= h < b)
    for c, (back, ahead, m, _) in enumerate(score._windows(base["windows"])[0]):
        hit = np.zeros(F, dtype=bool)
        if m > k:
            for f in range(s, e):
                hit[f] = any(min(e - 1, max(s, f - back + j)) == h for j in range(back + ahead + 1))
            assert hit[max(s, h - ahead):min(e, h + back + 1)].all() and hit.sum() == min(e, h + back + 1) - max(s, h - ahead)
        keep = torch.as_tensor(~hit, device=out.device)
        assert torch.equal(out[c][keep], base["out"][c][keep]) and torch.equal(spread[c][keep], base["spread"][c][keep]), (c, back, ahead, m)
        if hit.any():
            bad = torch.as_tensor(hit, device=out.device)
            assert bool(out[c][bad].isnan().any(dim=1).all()) and bool(spread[c][bad].isnan().any(dim=1).all()), (c, back, ahead, m)


# ---------------- 9. float32 output ---------------------------------------------------------------------------------------------------------
def test_float32_output_is_the_float64_result_rounded_once(base):
    est, windows = base["est"], base["windows"]
    o32, s32 = est.repost_windows(base["y"], windows, starts=STARTS, spread=True, out_dtype=torch.float32)
    assert o32.dtype == torch.float32 and torch.equal(o32, base["out"].float()) and torch.equal(s32, base["spread"].float())
    p32 = est.repost_windows(base["y"], [windows[9]], starts=STARTS, out_dtype=torch.float32, workspace_bytes=2 * 36 * 8 * 21 * 6)
    assert torch.equal(p32[0], base["out"][9].float())


# ---------------- 10. end to end ------------------------------------------------------------------------------------------------------------
def test_the_planted_trajectory_on_the_device(norm_stats):
    """the planted trajectory of tests/test_post_window_cpu.py: a centred window has no lag at the error the causal one only reaches
    after the truth has been shifted, and a taper keeps the curvature"""
    from wear_mocap_ape_amd import _hip, score
    from wear_mocap_ape_amd.estimate import nn_models
    yh, truth = planted()
    m = nn_models.DropoutLSTM(22, 256, 2, 14, dropout=0.2, device=0, target_layout=_hip.LAYOUT_ORI_CAL_LARM_UARM_HIPS)
    st = norm_stats["pocket"]
    m.set_norm_stats(st["xx_m"], st["xx_s"], np.zeros(14), np.ones(14))
    m.set_body(orc.DEFAULT_BODY)
    y, truth_d = torch.from_numpy(yh).cuda(), torch.from_numpy(truth).cuda()
    n = yh.shape[1]
    windows = [(0, 0, n), (8, 0, n), (4, 4, n), score.window(4, 4, n, "triangle"),
               (8, 8, n), score.window(8, 8, n, "triangle"), score.window(8, 8, n, "hann")]
    out = score.post_window(m, y, windows)
    res = score.score_windows(0, out, None, truth_d, windows, LAGS, "est", [0], SKIP, orc.DEFAULT_BODY)
    assert res["acc"].shape == (7, 1, 25, 25) and [w[:3] for w in res["configs"]] == [tuple(w[:3]) for w in windows]
    best = [b[0] for b in res["best"]]
    print("planted trajectory on the device, hand RMS at lag 0 [mm]:", [round(1e3 * b["rms_lag0"], 2) for b in best], "lags:", [b["lag"] for b in best])
    assert [b["lag"] for b in best] == [0, 4, 0, 0, 0, 0, 0]
    assert abs(best[2]["refined"]) < 0.5
    assert best[2]["rms_lag0"] < best[1]["rms_lag0"]
    assert best[6]["rms_lag0"] < best[5]["rms_lag0"] < best[4]["rms_lag0"]


def test_sweep_windows_end_to_end(base):
    from wear_mocap_ape_amd import score
    est, rows, y = base["est"], base["rows"], base["y"]
    truth = (y.double().mean(dim=1) * torch.as_tensor(est._yy_s, device=y.device) + torch.as_tensor(est._yy_m, device=y.device)).contiguous()
    for r in rows[:4]:
        est.process_row(array("f", r.tolist()))
    before = est.get_state()
    windows, lags = [(2, 0, M), (1, 1, M), score.window(2, 2, 2, "hann"), (0, 0, 1)], (-3, 3)
    res = est.sweep_windows(rows, truth, windows, starts=STARTS, lags=lags, seed=SEED, motion=True)
    assert [w[:3] for w in res["configs"]] == [(2, 0, M), (1, 1, M), (2, 2, 2), (0, 0, 1)]
    assert np.array_equal(res["configs"][2][3], score.window_weights("hann", 2, 2)) and res["configs"][0][3] is None
    assert res["acc"].shape == (4, 4, 7, 25) and len(res["best"]) == 4 and res["motion"].shape == (4, 4, 38)
    assert est._smooth == 3 and est._frame_samples() == M
    after = est.get_state()
    assert after["desc"] == before["desc"] and np.array_equal(after["window"], before["window"]) and np.array_equal(after["stack"], before["stack"])
    for c in range(4):
        assert repr(res["best"][c]) == repr(score.best_lag(res["acc"][c], lags))           # (repr: NaN fields of the empty supports)
    # window 0 is this estimator's own configuration: the accumulators of its replay
    ro, rr = est.process_recording(rows, starts=STARTS, spread=True, seed=SEED)
    acc = score.score_lags(est._layout, ro, truth, lags, "targets", rr, STARTS, est.sequence_len - 1, est.body_measurements)[1]
    assert np.array_equal(res["acc"][0], acc.cpu().numpy())
    assert "motion" not in est.sweep_windows(rows, truth, windows[:1], starts=STARTS, lags=lags, seed=SEED)
