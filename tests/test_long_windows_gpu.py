"""The longest window of every LSTM route, and the first one beyond it, against the float64 recurrence (the CPU half with the windows, the
references and their conditioning: tests/test_long_windows_cpu.py).

Each row of ROUTES pins the kernel that must serve the shape (`kernel_name(B, T)` where it can name it, `last_kernel()` always), runs the
call, calls `check()` and compares EVERY row of the batch -- row r holds window r mod 7 -- with the reference at the project's budget
max(1e-6, 4 e_ref), e_ref = max |float32 oracle - float64 reference| over all steps of the same windows.  The routes that can return every step
are compared at every step, so that a mistake in the middle of a window shows even where the recurrence has forgotten it by the last step
(test_how_far_back_the_last_step_sees records how far back that is).  No kernel is another kernel's yardstick.
Every test prints its line (prefix `FAREND|`); the record is profiles/far_ends.md."""
import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from oracle import philox as ph
from tests import philox_cases as pc
from tests import test_hostile_inputs_cpu as hi
from tests import test_long_windows_cpu as lw
from tests.test_hostile_inputs_gpu import _build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


# route id: (model, set_kernel, B, T, kernel_name(B, T) must contain, last_kernel() must equal, every step compared as well, cases)
#   the limits: lstm_level16.hip takes one row tile per cluster up to 4000 steps and two up to 48; lstm_cluster_small.hip up to T + L - 1 = 4095
#   phases (12-bit phase tags); ImuPose's layer-split route up to 1023 steps (32-bit sequence offsets); 4001 on the routes without a limit
BOTH, LONG4K_ONLY = lw.CASES, (hi.LONG4K_CASE,)
ROUTES = {
    "level16-one-tile-T4000": ("uarm", "auto", 37, 4000, "ape_lstm_level16<128, 3, 64>", "ape_lstm_level16", False, BOTH),
    "level16-past-T4001": ("uarm", "auto", 37, 4001, "ape_lstm_cluster<", "ape_lstm_cluster", False, BOTH),
    # (values at 48 and 49 steps are held by tests/test_hostile_inputs_gpu.py: the pair is here for the route pin and the x 4 weights)
    "level16-two-tiles-T48": ("uarm", "auto", 530, 48, "ape_lstm_level16<128, 3, 64>", "ape_lstm_level16", False, LONG4K_ONLY),
    "level16-two-tiles-past-T49": ("uarm", "auto", 530, 49, "ape_lstm_cluster16<128, 3, 64, 2>", "ape_lstm_cluster16", False, LONG4K_ONLY),
    "cluster_small-pocket-T4094": ("pocket", "auto", 3, 4094, "ape_lstm_cluster<", "ape_lstm_cluster_small", False, BOTH),
    "cluster_small-pocket-past-T4095": ("pocket", "auto", 3, 4095, "ape_lstm_cluster<", "ape_lstm_cluster", False, BOTH),
    "cluster_small-uarm-T4093": ("uarm", "auto", 3, 4093, "ape_lstm_cluster<", "ape_lstm_cluster_small", False, BOTH),
    "cluster_small-uarm-past-T4094": ("uarm", "auto", 3, 4094, "ape_lstm_cluster<", "ape_lstm_cluster", False, BOTH),
    "cluster32-long-T4001": ("pocket", "cluster", 513, 4001, "ape_lstm_cluster32<256, 2, 32, false>", "ape_lstm_cluster32", False, BOTH),
    "cluster16-T4001": ("uarm", "cluster", 513, 4001, "ape_lstm_cluster16<128, 3, 64, 2>", "ape_lstm_cluster16", False, BOTH),
    "tile16-T4001": ("pocket", "tile16", 37, 4001, "tile16", "ape_lstm_tile16", True, BOTH),
    "cluster_gen1-T4001": ("pocket", "cluster_gen1", 77, 4001, "ape_lstm_cluster<", "ape_lstm_cluster", True, BOTH),
    "imupose-split32-T1023": ("imupose", "auto", 513, 1023, "ape_lstm_upper32<32, true>", "ape_lstm_upper32", False, BOTH),
    "imupose-past-T1024": ("imupose", "auto", 513, 1024, "ape_lstm_cluster<256, 2, 256", "ape_lstm_cluster", False, BOTH),
}
ROUTE_CASES = [(r, c) for r in ROUTES for c in ROUTES[r][7]]


def test_the_cpu_half_conditions_every_shape_used_here():
    have = {(m, T, a) for m, T, a in lw.GPU_SHAPES}
    for model, _, _, T, _, _, all_steps, _ in ROUTES.values():
        assert (model, T, False) in have and (not all_steps or (model, T, True) in have), (model, T)
        assert T <= lw.T_MAX[model]


def _batch(x7, B, T):
    """device [B, T, I]: row r = the first T steps of window r mod 7"""
    xd = torch.from_numpy(np.ascontiguousarray(x7[:, :T])).cuda()
    return xd[torch.arange(B, device="cuda") % lw.N_WINDOWS].contiguous()


def _worst(y, ref7):
    """max |y[r] - ref7[r mod 7]| over all rows: y [B, ...], ref7 [7, ...]"""
    worst = 0.0
    for w in range(min(lw.N_WINDOWS, y.shape[0])):
        worst = max(worst, float(np.abs(y[w::lw.N_WINDOWS].astype(np.float64) - ref7[w]).max()))
    return worst


@pytest.mark.parametrize("route,case", ROUTE_CASES)
def test_longest_window_against_the_float64_reference(norm_stats, route, case):
    model, kernel, B, T, want_name, want_last, all_steps, _ = ROUTES[route]
    ref = lw.reference(norm_stats, model, case)
    bud = pc.budget(lw.e_ref(ref, T))
    m, sd, st = _build(norm_stats, model, hi.wscale_of(model, case))
    assert all(np.array_equal(sd[k], ref["sd"][k]) for k in sd)
    try:
        m.set_kernel(kernel)
        assert want_name in m.kernel_name(B, T), (route, m.kernel_name(B, T))
        xd = _batch(ref["x"], B, T)
        y = m(xd, last_step_only=True, normalize_input=True)
        assert m.last_kernel() == want_last, (route, m.last_kernel())
        m.check()
        y = y.cpu().numpy()[:, 0]
        assert y.shape == (B, ref["y64"].shape[2]) and np.isfinite(y).all()
        err = _worst(y, ref["y64"][:, T - 1])
        line = (f"FAREND|{route}|{want_last}|{model} {B}x{T}|{case}|e_ref {lw.e_ref(ref, T):.2e}|budget {bud:.2e}|last step err {err:.2e}|"
                f"ratio {err / bud:.2f}")
        if all_steps:
            ya = m(xd, last_step_only=False, normalize_input=True)
            assert m.last_kernel() == want_last, (route, m.last_kernel())
            m.check()
            ya = ya.cpu().numpy()
            assert ya.shape == (B, T, ref["y64"].shape[2]) and np.isfinite(ya).all()
            err_all = _worst(ya, ref["y64"][:, :T])
            line += f"|all steps err {err_all:.2e}|ratio {err_all / bud:.2f}"
            err = max(err, err_all)
        print("\n" + line)
        assert err <= bud, line
    finally:
        m.set_kernel("auto")
        del m                                  # (ImuPose at 513 x 1023: 1.1 GB of layer workspace goes with the handle)
        torch.cuda.empty_cache()


# ---------------- the Monte-Carlo latency kernel at the ends of its window range -----------------------------------------------------------
@pytest.mark.parametrize("case", lw.CASES)
@pytest.mark.parametrize("route", sorted(pc.LONG_LSTM_ROUTES))
def test_mc_small_forward_at_its_longest_window(norm_stats, route, case):
    """one shared window, 25 dropout samples, 64 steps (the Monte-Carlo latency kernel's last: its LDS masks are sized by T) and 65 (the
    first-generation dropout kernel): the replica's masks (oracle/philox.py) under the float64 recurrence, as pc.lstm_reference does"""
    model, set_kernel, B, T, mseed, want_last, shared = pc.LONG_LSTM_ROUTES[route]
    c = lw.mc_forward_case(norm_stats, route, case)              # (conditioned on the CPU: test_the_mc_forward_cases_are_conditioned)
    sd, xn, y64, e = c["sd"], c["xn"], c["y64"], c["e_ref"]
    bud = pc.budget(e)
    m, sd_m, _ = _build(norm_stats, model, hi.wscale_of(model, case))
    assert all(np.array_equal(sd[k], sd_m[k]) for k in sd)
    m.set_kernel(set_kernel)
    m.manual_seed(mseed)                                         # the call below is Monte-Carlo call 1: key (mseed << 20) + 1
    y = m.monte_carlo_predictions(B, torch.from_numpy(np.ascontiguousarray(xn)).cuda(), last_step_only=True).cpu().numpy()[:, 0]
    used = m.last_kernel()
    m.check()
    assert used == want_last, (route, used)
    assert y.shape == y64.shape and np.isfinite(y).all() and np.isfinite(y64).all()
    err = float(np.abs(y - y64).max())
    line = f"FAREND|{route}|{used}|{model} {B} samples x {T}|{case}|e_ref {e:.2e}|budget {bud:.2e}|err {err:.2e}|ratio {err / bud:.2f}"
    print("\n" + line)
    assert e <= lw.E_REF_CAP and err <= bud, line


@pytest.mark.parametrize("bank_id", sorted(pc.LONG_BANKS))
def test_bank_of_one_estimator_with_long_windows(norm_stats, bank_id):
    """S = 1 stream x 25 samples with windows of 32, 33, 64 and 65 frames: the cold start, a reset, a half-filled window, the first full one
    and the first that has dropped a row, through pc.bank_reference (the replica's masks, the float64 recurrence, the oracle's float64 FK)"""
    from tests.test_philox_routes_gpu import _lstm_model
    from wear_mocap_ape_amd.streams import StreamBank
    reg, name, S, n_mc, smooth, seed, T, F = pc.bank_dims(bank_id)
    want_last = pc.bank_entry(bank_id)[7]
    m = _lstm_model(norm_stats, name)
    bank = StreamBank(m, S, T, smooth=smooth, normalize=True, dtype=torch.float64, monte_carlo_samples=n_mc, dropout=pc.P, seed=seed)
    feats = pc.bank_features(norm_stats, bank_id)
    checked = pc.long_bank_frames(bank_id)
    assert checked[-1] == F - 1
    got, kernels = {}, set()
    for f in range(F):
        if f == pc.RESET_AT:
            bank.reset()
        bank.push_features(torch.from_numpy(np.ascontiguousarray(feats[f])).cuda())
        msg, tail = bank.step(with_tail=True)
        kernels.add(m.last_kernel())
        if f in checked:
            got[f] = (tail.cpu().numpy().copy(), msg.cpu().numpy().copy())
    m.check()
    assert kernels == {want_last}, kernels
    ref = pc.bank_reference(norm_stats, bank_id, frames=checked, with32=True)
    err = max(pc.quantity_error(got[f], ref[f][0]) for f in checked)
    e = max(pc.quantity_error(ref[f][1], ref[f][0]) for f in checked)
    bud = pc.budget(e)
    line = (f"FAREND|bank {bank_id}|{want_last}|{name} S={S} n_mc={n_mc} T={T}|frames {checked} of {F}, reset before {pc.RESET_AT}|e_ref {e:.2e}|"
            f"budget {bud:.2e}|err {err:.2e}|ratio {err / bud:.2f}")
    print("\n" + line)
    assert e <= lw.E_REF_CAP and err <= bud, line


@pytest.mark.parametrize("bank_id", ["mc_small-1x25-T32", "mc_small-1x25-T33"])
def test_host_frames_at_the_fused_feature_builders_limit(golden, norm_stats, bank_id):
    """the same banks through `ape_streams_frame_host` (raw message in, datagram out): up to 32 frames per window the Monte-Carlo latency
    kernel's extra workgroups build the row's features in the regressor's own launch (its LDS holds the mask bits of T steps beside them),
    from 33 on the feature builder's own launch runs in front.  The reference takes the features the device's builder makes of the rows."""
    import ctypes as C
    from tests.test_philox_routes_gpu import _device_features, _lstm_model
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    reg, name, S, n_mc, smooth, seed, T, F = pc.bank_dims(bank_id)
    want_last, N = pc.bank_entry(bank_id)[7], smooth * n_mc
    m = _lstm_model(norm_stats, name)
    bank = StreamBank(m, S, T, smooth=smooth, normalize=True, dtype=torch.float64, monte_carlo_samples=n_mc, dropout=pc.P, seed=seed)
    rows = pc.trace_rows(golden, F, lw.HOST_ROWS_SEED)
    feats = _device_features(rows).reshape(F, S, -1)
    checked = pc.long_bank_frames(bank_id)
    out, got, kernels = np.empty((25 + 6 * N,), dtype=np.float64), {}, set()
    for f in range(F):
        if f == pc.RESET_AT:
            bank.reset()
        row = np.ascontiguousarray(rows[f])
        _hip.check(_hip.lib().ape_streams_frame_host(bank._handle, _hip.PARSE_WATCH_PHONE_POCKET, C.c_void_p(row.ctypes.data), _hip.FLAG_NORMALIZE_INPUT,
                                                     C.c_void_p(out.ctypes.data), _hip.F64, None), "ape_streams_frame_host")
        kernels.add(m.last_kernel())
        if f in checked:
            got[f] = (out[25:].reshape(S, N, 6).copy(), out[:25].reshape(S, 25).copy())
    m.check()
    assert kernels == {want_last}, kernels
    assert bank.frame_stats()["recovered"] == 0
    ref = pc.bank_reference(norm_stats, bank_id, frames=checked, with32=True, feats=feats)
    err = max(pc.quantity_error(got[f], ref[f][0]) for f in checked)
    e = max(pc.quantity_error(ref[f][1], ref[f][0]) for f in checked)
    bud = pc.budget(e)
    line = (f"FAREND|host frames {bank_id}|{want_last}|{name} S={S} n_mc={n_mc} T={T}|frames {checked} of {F}, reset before {pc.RESET_AT}|e_ref {e:.2e}|"
            f"budget {bud:.2e}|err {err:.2e}|ratio {err / bud:.2f}")
    print("\n" + line)
    assert e <= lw.E_REF_CAP and err <= bud, line
