"""The longest windows every LSTM route accepts, the parts that need no GPU: the windows and float64 references the GPU half
(tests/test_long_windows_gpu.py) holds every route to, the proof that those cases are conditioned, how far back the last step of such a window
still sees, and a sweep of the planner over the limits of the kernels whose hand-over tags hold the phase in 12 bits.

Windows   : 7 distinct windows of T_MAX[model] steps per model (seed SEED_X, standard-normal z-scores); a window of T steps is the first T steps
            of one of them, so ONE evaluation of the recurrence per (model, case) is the reference of every length: step t of a causal
            recurrence from the zero state does not depend on what follows it.  Row r of a batch holds window r mod 7 -- 7 is coprime to
            the 16-row tiles and the 32-row clusters, a read of a wrong row gives another window.
Cases     : `benign` (weights x 1) and `long4k` (`lstm.*` tensors x 4: tests/test_hostile_inputs_cpu.LONG4K_SCALE).
Reference : `hi.forward64`; yardstick e_ref(T) = max |hi.forward32 - reference| over the 7 windows and ALL steps below T;
            budget `pc.budget(e_ref)` = max(1e-6, 4 e_ref), the project's rule.
Every test prints its line (prefix `FAREND|`); the record is profiles/far_ends.md."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import philox_cases as pc
from tests import test_hostile_inputs_cpu as hi

REPO = Path(__file__).resolve().parents[1]
CASES = ("benign", hi.LONG4K_CASE)
N_WINDOWS, SEED_X = 7, 21
# the longest window of a model in the GPU half: pocket on the latency kernel's far side (4095), uarm likewise (4094), ImuPose past split32 (1024)
T_MAX = {"pocket": 4095, "uarm": 4094, "imupose": 1024}
# (model, T, all steps compared) of every case of the GPU half: the conditioning test below walks exactly these
GPU_SHAPES = (("uarm", 4000, False), ("uarm", 4001, False), ("uarm", 48, False), ("uarm", 49, False), ("uarm", 4093, False), ("uarm", 4094, False),
              ("pocket", 4094, False), ("pocket", 4095, False), ("pocket", 4001, False), ("pocket", 4001, True),
              ("imupose", 1023, False), ("imupose", 1024, False))
E_REF_CAP = 1e-5
_REF = {}


def windows(norm_stats, model):
    """-> (raw float32 features [7, T_MAX, I] as the models take them, the float32 z-scores the recurrence sees)"""
    st = norm_stats[model if model != "imupose" else "pocket"]
    z = hi.case_z("benign", N_WINDOWS, T_MAX[model], hi.dims_of(model)[0], SEED_X)
    return hi.raw_and_normalised(st, z)


def reference(norm_stats, model, case):
    """one evaluation per (model, case): dict(x raw, xn, sd, y64 [7, T_MAX, O], err [T_MAX]: max |float32 oracle - y64| per step)"""
    if (model, case) not in _REF:
        x, xn = windows(norm_stats, model)
        sd = hi.state_dict(model, hi.wscale_of(model, case))
        y64 = hi.forward64(model, sd, xn)
        y32 = hi.forward32(model, sd, xn)
        y64.setflags(write=False)
        _REF[model, case] = dict(x=x, xn=xn, sd=sd, y64=y64, err=np.abs(y32 - y64).max(axis=(0, 2)))
    return _REF[model, case]


def e_ref(ref, T):
    return float(ref["err"][:T].max())


# ---------------- conditioning ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("model", sorted(T_MAX))
def test_the_long_cases_are_conditioned(norm_stats, model, case):
    """for every (model, T) of the GPU half: the float64 reference is finite and the float32 oracle stays within 1e-5 of it over all steps --
    otherwise 4 e_ref would hold nothing on outputs below one (at x 8 it is about 1: the recurrence is chaotic there)"""
    ref = reference(norm_stats, model, case)
    assert np.isfinite(ref["y64"]).all()
    for m, T, _ in GPU_SHAPES:
        if m != model:
            continue
        e = e_ref(ref, T)
        print(f"\nFAREND|cond|{model}|{case}|T {T}|e_ref {e:.2e}|budget {pc.budget(e):.2e}|max |y| {float(np.abs(ref['y64'][:, :T]).max()):.2f}")
        assert e <= E_REF_CAP, (model, case, T, e)


def test_a_window_is_the_prefix_of_a_longer_one(norm_stats):
    """what lets one evaluation serve every length: the recurrence over the first T steps alone gives steps 0 .. T-1 of the long one (to the
    float64 rounding of the head's matrix product, whose blocking follows the shape: 1e-13 against budgets of 1e-6)"""
    ref = reference(norm_stats, "uarm", hi.LONG4K_CASE)
    for T in (1, 48, 333):
        assert np.abs(hi.forward64("uarm", ref["sd"], ref["xn"][:, :T]) - ref["y64"][:, :T]).max() <= 1e-13


# ---------------- the Monte-Carlo cases of the GPU half -------------------------------------------------------------------------------------
def mc_forward_case(norm_stats, route, case):
    """one shared window x B dropout samples under the host replica's masks (pc.LONG_LSTM_ROUTES): -> dict(xn [1, T, I] the z-scores the call
    takes, y64 [B, O] of the last step, e_ref on it)"""
    from oracle import philox as ph
    model, _, B, T, mseed, _, shared = pc.LONG_LSTM_ROUTES[route]
    assert shared
    _, H, L, _ = hi.dims_of(model)
    ref = reference(norm_stats, model, case)
    xn = ref["xn"][3:4, :T]                                      # window 3 of the 7
    masks = list(ph.lstm_masks(ph.lstm_call_seed(mseed, 1), np.arange(B), T, H, L, pc.P))
    xr = np.repeat(xn, B, axis=0)
    y64 = hi.forward64(model, ref["sd"], xr, masks)[:, -1]
    return dict(xn=xn, sd=ref["sd"], y64=y64, e_ref=float(np.abs(hi.forward32(model, ref["sd"], xr, masks)[:, -1] - y64).max()))


def bank_e_ref(ref, frames):
    return max(pc.quantity_error(ref[f][1], ref[f][0]) for f in frames)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("route", sorted(pc.LONG_LSTM_ROUTES))
def test_the_mc_forward_cases_are_conditioned(norm_stats, route, case):
    c = mc_forward_case(norm_stats, route, case)
    print(f"\nFAREND|cond|{route}|{case}|e_ref {c['e_ref']:.2e}|budget {pc.budget(c['e_ref']):.2e}")
    assert np.isfinite(c["y64"]).all() and c["e_ref"] <= E_REF_CAP


@pytest.mark.parametrize("feats", ["bank_features", "host_features"])
@pytest.mark.parametrize("bank_id", sorted(pc.LONG_BANKS))
def test_the_long_bank_cases_are_conditioned(golden, norm_stats, bank_id, feats):
    """the banks of the GPU half on the frames it checks, on the quantity it compares (tails and messages through the float64 FK): on the
    drawn features of the lockstep frames, and -- the two banks the host frames run -- on the host builder's features of the raw messages
    (the GPU half takes the device builder's, which agree with these to float32 rounding: the conditioning is the case's, not the builder's)"""
    T = pc.LONG_BANKS[bank_id][8]
    if feats == "host_features" and T > 33:
        return                                                   # (host frames run at T = 32 and 33 only)
    frames = pc.long_bank_frames(bank_id)
    F = pc.bank_dims(bank_id)[7]
    f = None if feats == "bank_features" else pc.host_features(pc.trace_rows(golden, F, HOST_ROWS_SEED)).reshape(F, 1, -1)
    ref = pc.bank_reference(norm_stats, bank_id, frames=frames, with32=True, feats=f)
    e = bank_e_ref(ref, frames)
    print(f"\nFAREND|cond|bank {bank_id}|{feats}|frames {frames}|e_ref {e:.2e}|budget {pc.budget(e):.2e}")
    assert all(np.isfinite(q).all() for fr in frames for q in ref[fr][0]) and e <= E_REF_CAP


HOST_ROWS_SEED = 8                         # pc.trace_rows(golden, F, HOST_ROWS_SEED): the raw messages of the host-frame banks


# ---------------- what the last step sees -------------------------------------------------------------------------------------------------
def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _steps64(model, sd, xn, state=None, keep=0):
    """`hi.forward64` step by step (all layers of a step before the next step) so that it can start from a state: xn [B, n, I] ->
    (y [B, O] of the last step, final state, the states in front of each of the last `keep` steps).  A state is [(h, c)] per layer."""
    x = np.asarray(xn, dtype=np.float64)
    if model == "imupose":
        x = np.maximum(x @ sd["input_layer.weight"].astype(np.float64).T + sd["input_layer.bias"].astype(np.float64), 0.0)
    L = sum(1 for k in sd if k.startswith("lstm.weight_ih_l"))
    W = [(sd[f"lstm.weight_ih_l{k}"].astype(np.float64).T, sd[f"lstm.weight_hh_l{k}"].astype(np.float64).T,
          sd[f"lstm.bias_ih_l{k}"].astype(np.float64) + sd[f"lstm.bias_hh_l{k}"].astype(np.float64)) for k in range(L)]
    H = W[0][1].shape[0]
    B, n = x.shape[0], x.shape[1]
    st = [(np.zeros((B, H)), np.zeros((B, H))) for _ in range(L)] if state is None else [(h.copy(), c.copy()) for h, c in state]
    kept = []
    for t in range(n):
        if t >= n - keep:
            kept.append([(h.copy(), c.copy()) for h, c in st])
        inp = x[:, t]
        for k, (wi, wh, b) in enumerate(W):
            h, c = st[k]
            pre = inp @ wi + h @ wh + b
            c = _sig(pre[:, H:2 * H]) * c + _sig(pre[:, :H]) * np.tanh(pre[:, 2 * H:3 * H])
            h = _sig(pre[:, 3 * H:]) * np.tanh(c)
            st[k] = (h, c)
            inp = h
    y = st[-1][0] @ sd["output_layer.weight"].astype(np.float64).T + sd["output_layer.bias"].astype(np.float64)
    return y, st, kept


MEMORY_GRID = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 511)


def memory_length(norm_stats, model, case):
    """the largest k of MEMORY_GRID for which replacing the z-scores of step T-1-k by zeros (the mean feature vector) still moves the last
    step of the float64 reference by more than the case's budget, T = T_MAX[model] -> (k or -1, move at that k, budget)"""
    ref = reference(norm_stats, model, case)
    T, sd, xn = T_MAX[model], ref["sd"], ref["xn"]
    keep = MEMORY_GRID[-1] + 1
    y, _, kept = _steps64(model, sd, xn, keep=keep)          # kept[j]: the state in front of step T - keep + j
    assert np.abs(y - ref["y64"][:, -1]).max() <= 1e-12      # the step-major walk is the reference's recurrence
    bud = pc.budget(e_ref(ref, T))
    best, move = -1, 0.0
    for k in MEMORY_GRID:
        tail = xn[:, T - 1 - k:].copy()
        tail[:, 0] = 0.0
        d = float(np.abs(_steps64(model, sd, tail, state=kept[keep - 1 - k])[0] - y).max())
        if d > bud:
            best, move = k, d
    return best, move, bud


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("model", sorted(T_MAX))
def test_how_far_back_the_last_step_sees(norm_stats, model, case):
    """a record with one assertion: the newest step is seen (k = 0 moves the output), and the recurrence forgets inside the 512 newest steps --
    which is why the routes that can return every step are compared at every step"""
    k, move, bud = memory_length(norm_stats, model, case)
    print(f"\nFAREND|memory|{model}|{case}|T {T_MAX[model]}|last step moved beyond its budget {bud:.2e} by zeroed steps up to T-1-{k} (by {move:.2e} there)")
    assert 0 <= k < MEMORY_GRID[-1]


# ---------------- the planner at the limits of the 12-bit phase tags -------------------------------------------------------------------------
NONE, GEN1, C32, SMALL, C16, LV16, SPLIT32, MC_SMALL = range(8)
TAG_MAX_PHASES = 4095                      # csrc/ape_plan.h APE_TAG_MAX_PHASES: (launch number << 12) | (phase + 1), phase + 1 <= T + L - 1
SPLIT32_MAX_T = 1023                       # 128 * T * 32768 < 2^32: lstm_upper32.hip's 32-bit sequence offsets
SWEEP_CUS = (256, 128)
SWEEP_B = (1, 4, 5, 37, 512, 513, 1024, 1025)
SWEEP_T = (1, 64, 65, 1023, 1024, 4000, 4001, 4093, 4094, 4095, 4096, 4097, 10000)
# (I, H, L, O, layout, model kind name)
SWEEP_MODELS = {"pocket": (22, 256, 2, 14, 0, "MODEL_LSTM"), "watch": (20, 256, 2, 12, 1, "MODEL_LSTM"), "uarm": (38, 128, 3, 12, 1, "MODEL_LSTM"),
                "imupose": (22, 256, 2, 14, 0, "MODEL_IMUPOSE")}


def plan_sweep():
    """-> {(model, n_cus, B, T, cdrop, c32): route} from `ape_debug_plan2` of the built library (pure host arithmetic, csrc/ape_plan.h)"""
    import __graft_entry__ as entry
    entry.build()
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    lib.ape_debug_plan2.restype = C.c_int
    lib.ape_debug_plan2.argtypes = [C.POINTER(_hip.ApeDims), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 6)]
    out, res = (C.c_int * 6)(), {}
    for name, (I, H, L, O, layout, kind) in SWEEP_MODELS.items():
        dims = _hip.ApeDims(I, H, L, O, layout, 0, getattr(_hip, kind))
        for cus in SWEEP_CUS:
            for B in SWEEP_B:
                for T in SWEEP_T:
                    for cdrop in (0, 1):
                        for c32 in (0, 1):
                            assert lib.ape_debug_plan2(C.byref(dims), cus, B, T, cdrop, c32, C.byref(out)) == 0
                            res[name, cus, B, T, cdrop, c32] = out[5]
    return res


def check_sweep(res):
    """no route with 12-bit phase tags plans more than 4095 phases, split32 never plans T > 1023 -> how many plans took such a route"""
    tagged = 0
    for (name, cus, B, T, cdrop, c32), route in res.items():
        L = SWEEP_MODELS[name][2]
        if route in (SMALL, LV16, MC_SMALL):
            tagged += 1
            assert T + L - 1 <= TAG_MAX_PHASES, (name, cus, B, T, cdrop, c32, route)
        if route == SPLIT32:
            tagged += 1
            assert T <= SPLIT32_MAX_T, (name, cus, B, T, cdrop, c32)
    return tagged


def check_both_sides(res, lv16_two_tiles_max_t):
    """the limits are really reached: the last window on each route, and the first one beyond it on another"""
    assert res["uarm", 256, 37, 4000, 0, 1] == LV16 and res["uarm", 256, 37, 4001, 0, 1] == GEN1
    assert res["uarm", 256, 512, 4000, 0, 1] == LV16 and res["uarm", 256, 513, 4001, 0, 1] == C16
    assert res["pocket", 256, 4, 4094, 0, 1] == SMALL and res["pocket", 256, 4, 4095, 0, 1] == GEN1
    assert res["uarm", 256, 4, 4093, 0, 1] == SMALL and res["uarm", 256, 4, 4094, 0, 1] == GEN1
    assert res["uarm", 256, 1, 4093, 0, 0] == SMALL and res["uarm", 256, 1, 4094, 0, 0] == GEN1
    assert res["imupose", 256, 513, 1023, 0, 1] == SPLIT32 and res["imupose", 256, 513, 1024, 0, 1] == GEN1
    assert res["imupose", 128, 1025, 1023, 0, 1] == SPLIT32 and res["imupose", 128, 1025, 4000, 0, 1] == GEN1
    # two row tiles per cluster (513 .. 1024 rows): up to the threshold the override moves
    for T in SWEEP_T:
        assert (res["uarm", 256, 1024, T, 0, 1] == LV16) == (T <= lv16_two_tiles_max_t), (T, res["uarm", 256, 1024, T, 0, 1])


_CHILD = """
import json, sys
sys.path.insert(0, {repo!r})
from tests import test_long_windows_cpu as lw
res = lw.plan_sweep()
n = lw.check_sweep(res)
lw.check_both_sides(res, {two_tiles})
print("SWEEP " + json.dumps([len(res), n]))
"""
OVERRIDES = ("APE_LV16_MAX_T", "APE_LV16_MIN_ROWS", "APE_C16_MIN_T")


def _sweep_in_a_child(overrides, two_tiles):
    """the overrides are read once per process, so every sweep runs in a child of its own with exactly `overrides` set -> tagged plans"""
    env = {k: v for k, v in os.environ.items() if k not in OVERRIDES}
    env.update(overrides)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(repo=str(REPO), two_tiles=two_tiles)], env=env, cwd=str(REPO), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("SWEEP ")]
    assert line, r.stdout[-2000:]
    n_plans, tagged = json.loads(line[-1][6:])
    assert n_plans == len(SWEEP_MODELS) * len(SWEEP_CUS) * len(SWEEP_B) * len(SWEEP_T) * 4 and tagged > 0
    return n_plans, tagged


def test_no_route_with_12_bit_tags_plans_past_4095_phases():
    n_plans, tagged = _sweep_in_a_child({}, 48)
    print(f"\nFAREND|plan|default thresholds|{n_plans} plans, {tagged} on routes with 12-bit tags or 32-bit offsets|none beyond its limit")


@pytest.mark.parametrize("value,two_tiles", [("5000", 4000), ("2147483647", 4000), ("-7", 0), ("100", 100)])
def test_the_sweep_under_an_unclamped_override(value, two_tiles):
    """`APE_LV16_MAX_T=5000` used to send 1024 rows x 4096 steps to the level kernel, whose tag then spilt into the launch number; the planner
    clamps the value to the one-tile form's own limit (APE_LV16_MAX_T_SINGLE = 4000)"""
    n_plans, tagged = _sweep_in_a_child({"APE_LV16_MAX_T": value}, two_tiles)
    print(f"\nFAREND|plan|APE_LV16_MAX_T={value}|two row tiles up to T = {two_tiles}|{tagged} of {n_plans} plans tagged, none beyond its limit")


def test_the_other_overrides_are_clamped_too():
    """APE_LV16_MIN_ROWS = 0 and APE_C16_MIN_T = -5, values no comparison has a meaning for: the plans of the sweep are those of 1 and 1, and hold"""
    _sweep_in_a_child({"APE_LV16_MIN_ROWS": "0", "APE_C16_MIN_T": "-5"}, 48)


# ---------------- the launchers' refusal -----------------------------------------------------------------------------------------------------
def test_the_launchers_refuse_what_the_tags_cannot_hold():
    """`ape_debug_launch_refusal(kernel, T)` calls the launcher of the level kernel (0, three layers) or the latency kernel (1: two layers,
    2: three) with a window that does not fit the 12-bit phase count and returns its answer -- the launchers refuse in front of every HIP
    call, so no GPU is needed and nothing is launched; where the window fits the entry answers -1 WITHOUT calling the launcher.  Both
    sides of T + L - 1 = 4095, and the same comparison as the planner's gate (csrc/ape_plan.h plan_tag_phases_fit)."""
    import __graft_entry__ as entry
    entry.build()
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    lib.ape_debug_launch_refusal.restype = C.c_int
    lib.ape_debug_launch_refusal.argtypes = [C.c_int, C.c_int]
    INVALID_VALUE = 1                      # hipErrorInvalidValue
    for kernel, L in ((0, 3), (1, 2), (2, 3)):
        last = TAG_MAX_PHASES - L + 1      # the longest window: T + L - 1 = 4095
        for T in (1, 6, 4000, last):
            assert lib.ape_debug_launch_refusal(kernel, T) == -1, (kernel, T)
        for T in (last + 1, last + 2, 4096, 5000, 10000, 2 ** 31 - 1, 0, -1):
            assert lib.ape_debug_launch_refusal(kernel, T) == INVALID_VALUE, (kernel, T)
    assert lib.ape_debug_launch_refusal(3, 5000) == -2
    # the planner's gate is the same function: a window length near INT_MAX does not wrap into the latency kernel's range
    lib.ape_debug_plan2.restype = C.c_int
    lib.ape_debug_plan2.argtypes = [C.POINTER(_hip.ApeDims), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 6)]
    out = (C.c_int * 6)()
    for dims in (_hip.ApeDims(22, 256, 2, 14, 0, 0, _hip.MODEL_LSTM), _hip.ApeDims(38, 128, 3, 12, 1, 0, _hip.MODEL_LSTM)):
        for T in (2 ** 31 - 1, 2 ** 31 - 2, 2 ** 31 - 3):
            assert lib.ape_debug_plan2(C.byref(dims), 256, 1, T, 0, 1, C.byref(out)) == 0 and out[5] == GEN1, (T, out[5])
