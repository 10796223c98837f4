"""The cases of tests/test_philox_routes_gpu.py and the references they are held to, built on the CPU from `oracle/philox.py` (the host replica
of the device-side Philox draws) and the float64 recurrence of tests/test_hostile_inputs_cpu.py; tests/test_philox_cpu.py evaluates the same
cases under replica mutants.  No kernel runs here and no kernel result enters a reference.

Reference : `hi.forward64(model, sd, x, masks)` with the replica's masks (DropoutFF: `orc.ff_forward` on float64 weights).
Yardstick : `e_ref = max |hi.forward32(..., masks) - reference|` on the same case; budget `max(1e-6, 4 e_ref)`, the project's rule.
Banks     : only the messages and sample tails of a frame are visible, so the compared quantity is every sample row's tail (hand and elbow
            position) and every stream's message through the oracle's float64 FK, with e_ref taken on that quantity.
Rows of one LSTM call are independent, so a reference restricted to some global rows (`rows=`) equals those rows of the whole case: the
mutant proofs of the large cases use that."""
import numpy as np

from oracle import ape_oracle as orc
from oracle import philox as ph
from tests import test_hostile_inputs_cpu as hi

P = 0.2
W_SEED = 3                       # weights: tests/test_hip_parity.make_model(name, W_SEED, stats)
SEED_X = 21
MI355X_CUS = 256                 # the CU count the CPU proofs assume for the AUTO split (the GPU test reads the device's)
FLOOR, FACTOR = 1e-6, 4.0


def budget(e_ref):
    return max(FLOOR, FACTOR * e_ref)


def state_dict(name):
    c = orc.MODEL_CONFIGS[name]
    return orc.make_state_dict(c["I"], c["H"], c["L"], c["O"], W_SEED)


# ---------------- one LSTM call ------------------------------------------------------------------------------------------------------------
# route id: (model, set_kernel, B (None: one batch-tile wave + 37), T, manual_seed, last_kernel() must equal, one shared window)
#   the call's key is (manual_seed << 20) + 1: from manual_seed 4096 on it has a high word; 5, 7 and 9 leave the high word zero
LSTM_ROUTES = {
    "tile16-pocket": ("pocket", "tile16", 37, 6, 0x12345, "ape_lstm_tile16", False),
    "tile16-watch": ("watch", "tile16", 37, 8, 5, "ape_lstm_tile16", False),
    "tile16-uarm": ("uarm", "tile16", 37, 6, 0xABCDE, "ape_lstm_tile16", False),
    "cluster-pocket-60": ("pocket", "cluster", 60, 6, 0x23456, "ape_lstm_cluster", False),
    "cluster-pocket-400": ("pocket", "cluster", 400, 6, 7, "ape_lstm_cluster", False),
    "cluster-pocket-530": ("pocket", "cluster", 530, 6, 0x34567, "ape_lstm_cluster", False),
    "cluster-uarm-45": ("uarm", "cluster", 45, 6, 0x45678, "ape_lstm_cluster", False),
    "auto-split-pocket": ("pocket", "auto", None, 6, 0x56789, "ape_lstm_cluster", False),
    "mc_small-25": ("pocket", "auto", 25, 6, 0x6789A, "ape_lstm_mc_small", True),
    "mc_small-128": ("pocket", "auto", 128, 6, 9, "ape_lstm_mc_small", True),
}


# the Monte-Carlo latency kernel at the ends of its window range (tests/test_long_windows_gpu.py): lstm_mc_small.hip sizes its LDS masks by T
# and is gated at T <= 64 -- one step more and the first-generation dropout kernel serves the call (from the same counters)
LONG_LSTM_ROUTES = {
    "mc_small-T64": ("pocket", "auto", 25, 64, 0x6789B, "ape_lstm_mc_small", True),
    "mc_small-T65": ("pocket", "auto", 25, 65, 0x6789C, "ape_lstm_cluster", True),
}


def lstm_route(route):
    return LSTM_ROUTES[route] if route in LSTM_ROUTES else LONG_LSTM_ROUTES[route]


def wave_rows(n_cus):
    return 16 * n_cus


def lstm_inputs(norm_stats, route, n_cus=MI355X_CUS):
    """-> dict: raw x [nb,T,I] as the model takes it, float32 z-scores xn [B,T,I] per row, B, key"""
    model, kernel, B, T, mseed, last, shared = lstm_route(route)
    B = wave_rows(n_cus) + 37 if B is None else B
    I = orc.MODEL_CONFIGS[model]["I"]
    z = hi.case_z("benign", 1 if shared else B, T, I, SEED_X)
    x, xn = hi.raw_and_normalised(norm_stats[model], z)
    return dict(model=model, x=x, xn=np.repeat(xn, B, axis=0) if shared else xn, B=B, T=T, key=ph.lstm_call_seed(mseed, 1))


def lstm_reference(inp, variant=ph.CONTRACT, rows=None, with32=False):
    """NN targets of the last step, float64 [rows, O] (and the float32 oracle's), under the replica's masks"""
    c = orc.MODEL_CONFIGS[inp["model"]]
    sd = state_dict(inp["model"])
    r = np.arange(inp["B"]) if rows is None else np.asarray(rows)
    masks = ph.lstm_masks(inp["key"], r, inp["T"], c["H"], c["L"], P, v=variant)
    y64 = hi.forward64(inp["model"], sd, inp["xn"][r], list(masks))[:, -1]
    if not with32:
        return y64
    return y64, hi.forward32(inp["model"], sd, inp["xn"][r], list(masks))[:, -1]


# ---------------- DropoutFF --------------------------------------------------------------------------------------------------------------
FF_DIMS = (22, 256, 2, 14)       # tests/golden/ff.npz "pocket_like": I, H, hidden layers, O
FF_MC = (50, 0x789AB)            # samples, manual_seed


def ff_sd64(sd):
    return {k: v.astype(np.float64) for k, v in sd.items()}


def ff_inputs():
    I, H, n_hidden, O = FF_DIMS
    x = np.random.default_rng(SEED_X).normal(size=(1, 6, I)).astype(np.float32)
    return dict(sd=orc.make_ff_state_dict(I, H, n_hidden, O, W_SEED), x=x, n=FF_MC[0], key=ph.lstm_call_seed(FF_MC[1], 1))


def ff_reference(inp, variant=ph.CONTRACT, with32=False):
    """`monte_carlo_predictions(n, x, last_step_only=True)`: n rows of the window's newest step, row r under mask row r"""
    mask = ph.ff_mask(inp["key"], inp["n"], FF_DIMS[1], P, v=variant)
    xr = np.repeat(inp["x"][:, -1], inp["n"], axis=0)
    y64 = orc.ff_forward(ff_sd64(inp["sd"]), xr, mask=mask)
    assert y64.dtype == np.float64
    return (y64, orc.ff_forward(inp["sd"], xr, mask=mask)) if with32 else y64


# ---------------- stream banks -------------------------------------------------------------------------------------------------------------
# bank id: (regressor, model, S, n_mc, smooth, seed, set_kernel after the bank is planned, last_kernel() must equal)
#   frames: T + 2, reset() in front of frame RESET_AT; every frame is checked up to CHECK_ALL_ROWS sample rows, the last one above
BANKS = {
    "mc_small-3x25": ("lstm", "pocket", 3, 25, 1, 0x1_0000_0007, "auto", "ape_lstm_mc_small"),
    "fused-5x25-smooth5": ("lstm", "pocket", 5, 25, 5, 0xABCDE12345, "auto", "ape_lstm_cluster"),
    "upper32-one-layer-A-21x25": ("lstm", "pocket", 21, 25, 1, 0x2_0000_0000 + 11, "auto", "ape_lstm_upper32"),
    "upper32-seq-A-100x25": ("lstm", "pocket", 100, 25, 1, 77, "auto", "ape_lstm_upper32"),
    "upper128-21x50": ("lstm", "uarm", 21, 50, 1, 0x3_0000_0005, "auto", "ape_lstm_upper128"),
    "shared-tile16-330x25": ("lstm", "pocket", 330, 25, 1, 0x4_0123_4567, "tile16", "ape_lstm_tile16"),
    "ff-7x25": ("ff", "pocket", 7, 25, 1, 0x5_0000_0003, "auto", "ape_ff_bank_head"),
}
# one estimator's bank (S = 1) with windows of 32 .. 65 frames instead of the deployed 6: a ninth field, the window length.  The bank steps on
# the Monte-Carlo latency kernel up to 64 frames (up to 32 its extra workgroups could also build the features) and on the fused
# first-generation dropout kernel from 65 (tests/test_long_windows_gpu.py checks LONG_BANK_FRAMES of each)
LONG_BANKS = {
    "mc_small-1x25-T32": ("lstm", "pocket", 1, 25, 1, 0x8_0000_0020, "auto", "ape_lstm_mc_small", 32),
    "mc_small-1x25-T33": ("lstm", "pocket", 1, 25, 1, 0x8_0000_0021, "auto", "ape_lstm_mc_small", 33),
    "mc_small-1x25-T64": ("lstm", "pocket", 1, 25, 1, 0x8_0000_0040, "auto", "ape_lstm_mc_small", 64),
    "mc_small-1x25-T65": ("lstm", "pocket", 1, 25, 1, 0x8_0000_0041, "auto", "ape_lstm_cluster", 65),
}
RESET_AT = 2
CHECK_ALL_ROWS = 2600


def bank_entry(bank):
    return BANKS[bank] if bank in BANKS else LONG_BANKS[bank][:8]


def long_bank_frames(bank):
    """the checked frames of a LONG_BANKS entry: the cold start, the reset, a half-filled window, the first full window and the first
    frame whose window has dropped a row"""
    T = LONG_BANKS[bank][8]
    return [0, RESET_AT, RESET_AT + T // 2, RESET_AT + T - 1, RESET_AT + T]


def bank_dims(bank):
    reg, name, S, n_mc, smooth, seed, kernel, last = bank_entry(bank)
    T = LONG_BANKS[bank][8] if bank in LONG_BANKS else orc.MODEL_CONFIGS[name]["T"]
    return reg, name, S, n_mc, smooth, seed, T, T + (RESET_AT + 1 if bank in LONG_BANKS else 2)


def bank_checked_frames(bank):
    _, _, S, n_mc, _, _, _, F = bank_dims(bank)
    return list(range(F)) if S * n_mc <= CHECK_ALL_ROWS else [F - 1]


# the banks under their own draws at the magnitudes of tests/test_hostile_inputs_cpu.py (tests/test_hostile_banks_gpu.py): the `lstm.*` tensors
# scaled by `hi.wscale_of(model, case)` and z-scores from `hi.case_z`; the DropoutFF bank on the like-named case of tests/ff_cases.py
# (every layer but the output layer scaled).  The windows are 6 or 8 frames: `hi.LONG_SCALE`'s caveat about long windows does not apply
BANK_CASES = ("trained", "sat30", "z1e3")
FF_BANK_CASE = {"trained": "w16", "sat30": "sat30", "z1e3": "z1e3"}


def bank_state_dict(reg, name, case="benign"):
    """the weights of a bank's regressor on a case; `benign`: as drawn"""
    c = orc.MODEL_CONFIGS[name]
    if reg == "ff":
        sd = orc.make_ff_state_dict(c["I"], 256, 2, c["O"], W_SEED)
        if case == "benign":
            return sd
        from tests import ff_cases as fc
        s = np.float32(fc.CASE_WSCALE[FF_BANK_CASE[case]])
        return {k: v if k.startswith("_output_layer.") else (v * s).astype(np.float32) for k, v in sd.items()}
    return state_dict(name) if case == "benign" else hi.state_dict(name, hi.wscale_of(name, case), W_SEED)


def bank_features(norm_stats, bank, case="benign"):
    """float32 feature rows [F, S, I]: frame f of stream s (column 0 at 0.02 on every case)"""
    reg, name, S, n_mc, smooth, seed, T, F = bank_dims(bank)
    st, I = norm_stats[name], orc.MODEL_CONFIGS[name]["I"]
    if case == "benign":
        z = np.random.default_rng(1000 + S).normal(size=(F, S, I))
    else:
        z = hi.case_z(case, F, S, I, 1000 + S)
    x = st["xx_m"] + st["xx_s"] * z
    x[..., 0] = 0.02
    return x.astype(np.float32)


def _clamped(f, start, n):
    """the n newest frames up to f, clamped at the cold start: what a window (n = T) and a smoothing stack (n = smooth) hold"""
    return [max(start, f - n + 1 + j) for j in range(n)]


def frame_targets(norm_stats, reg, name, feats, windows, key, n_mc, variant, global_rows, with32, ff_base=0, case="benign"):
    """one regressor call of a bank, frame or replay: `windows` [K, T] feature-frame indices per listed window, `feats` [F, K, I] (or
    [F, I] shared by all windows: a replay); sample row k * n_mc + i of the call is global row `global_rows[k * n_mc + i]`
    -> de-normalised targets float64 [K * n_mc, O] (and the float32 oracle's)"""
    st, c = norm_stats[name], orc.MODEL_CONFIGS[name]
    K = len(windows)
    if feats.ndim == 3:
        w = np.stack([feats[windows[k], k] for k in range(K)])                    # [K, T, I]
    else:
        w = np.stack([feats[windows[k]] for k in range(K)])
    xn = ((w.astype(np.float64) - st["xx_m"]) / st["xx_s"]).astype(np.float32)
    xr = np.repeat(xn, n_mc, axis=0)
    sd = bank_state_dict(reg, name, case)
    if reg == "ff":
        mask = ph.ff_bank_mask(key, global_rows, 256, P, philox_base=ff_base, v=variant)
        ys = [orc.ff_forward(ff_sd64(sd), xr[:, -1], mask=mask)] + ([orc.ff_forward(sd, xr[:, -1], mask=mask)] if with32 else [])
    else:
        masks = list(ph.lstm_masks(key, global_rows, windows.shape[1], c["H"], c["L"], P, v=variant))
        ys = [hi.forward64(name, sd, xr, masks)[:, -1]] + ([hi.forward32(name, sd, xr, masks)[:, -1]] if with32 else [])
    return [y.astype(np.float64) * st["yy_s"] + st["yy_m"] for y in ys]


def post_filter(name, stacks):
    """the float64 FK and message of every stream: stacks [K, N, O] de-normalised targets, oldest entry first -> (tail [K, N, 6], msg [K, 25])"""
    layout = orc.MODEL_CONFIGS[name]["layout"]
    tails, msgs = [], []
    for rows in stacks:
        est = orc.arm_pose_from_targets(rows, orc.DEFAULT_BODY, layout, "eigh")
        tails.append(est[:, :6])
        msgs.append(orc.msg_from_est(est, orc.DEFAULT_BODY, layout))
    return np.array(tails), np.array(msgs)


def bank_reference(norm_stats, bank, frames=None, variant=ph.CONTRACT, streams=None, with32=False, feats=None, case="benign"):
    """lockstep frames of a bank: {frame: [(tail, msg) float64 reference, (tail, msg) of the float32 oracle]} for `frames` (default: the
    checked ones) and `streams` (default: all).  Frame f is Monte-Carlo call f of the bank whatever reset() did in between: key
    seed + f; sample row = stream * n_mc + sample.  `feats` float32 [F, S, I]: the frames' feature rows where they are not
    `bank_features` (host frames: what the device's feature builder made of the raw messages).  `case`: weights and features of BANK_CASES."""
    reg, name, S, n_mc, smooth, seed, T, F = bank_dims(bank)
    frames = bank_checked_frames(bank) if frames is None else frames
    streams = np.arange(S) if streams is None else np.asarray(streams)
    feats = (bank_features(norm_stats, bank, case) if feats is None else feats)[:, streams]
    rows = (streams[:, None] * n_mc + np.arange(n_mc)[None, :]).reshape(-1)
    start = lambda f: RESET_AT if f >= RESET_AT else 0
    need = sorted({g for f in frames for g in _clamped(f, start(f), smooth)})
    y = {}
    for g in need:
        win = np.array([_clamped(g, start(g), 1 if reg == "ff" else T)] * len(streams))
        y[g] = [t.reshape(len(streams), n_mc, -1) for t in
                frame_targets(norm_stats, reg, name, feats, win, ph.bank_call_seed(seed, g), n_mc, variant, rows, with32, case=case)]
    out = {}
    for f in frames:
        out[f] = [post_filter(name, np.concatenate([y[g][k] for g in _clamped(f, start(f), smooth)], axis=1)) for k in range(2 if with32 else 1)]
    return out


def quantity_error(got, ref):
    """max |difference| over (tail, msg)"""
    return max(float(np.abs(np.asarray(g, dtype=np.float64) - r).max()) for g, r in zip(got, ref))


# ---------------- subset frame -----------------------------------------------------------------------------------------------------------
SUBSET = dict(model="pocket", S=9, n_mc=25, smooth=2, seed=0x6_0000_0009, listed=[7, 2, 5, 0], reset=[2, 5])


def subset_reference(norm_stats, feats, variant=ph.CONTRACT, with32=False):
    """feats float32 [3, S, I]: two lockstep frames of all S streams (Monte-Carlo calls 0 and 1, rows stream * n_mc + sample), reset of
    SUBSET["reset"], then ONE subset frame of SUBSET["listed"]: call 2 of the bank, rows BY LIST POSITION.  A listed stream that was reset
    starts cold (window and stack hold the new row / prediction only); the others stack frame 1's prediction under frame 2's.
    -> [(tail [K, smooth * n_mc, 6], msg [K, 25]) reference, ... float32 oracle]"""
    q = SUBSET
    name, n_mc, listed, T = q["model"], q["n_mc"], np.array(q["listed"]), orc.MODEL_CONFIGS[q["model"]]["T"]
    K = len(listed)
    cold = np.array([s in q["reset"] for s in listed])
    f = feats[:, listed]
    win2 = np.array([_clamped(2, 2 if cold[k] else 0, T) for k in range(K)])
    y2 = frame_targets(norm_stats, "lstm", name, f, win2, ph.bank_call_seed(q["seed"], 2), n_mc, variant, np.arange(K * n_mc), with32)
    rows1 = (listed[:, None] * n_mc + np.arange(n_mc)[None, :]).reshape(-1)
    win1 = np.array([_clamped(1, 0, T)] * K)
    y1 = frame_targets(norm_stats, "lstm", name, f, win1, ph.bank_call_seed(q["seed"], 1), n_mc, variant, rows1, with32)
    out = []
    for a, b in zip(y1, y2):
        a, b = a.reshape(K, n_mc, -1), b.reshape(K, n_mc, -1)
        out.append(post_filter(name, np.stack([np.concatenate([b[k] if cold[k] else a[k], b[k]]) for k in range(K)])))
    return out


# ---------------- replay -------------------------------------------------------------------------------------------------------------------
REPLAY = dict(model="pocket", F=40, n_mc=25, smooth=2, seed=0x7_0000_0001, cut=16)


def replay_reference(stats, feats, variant=ph.CONTRACT, rows=None, with32=False):
    """one recording of F frames in one call: the normalised NN targets [F * n_mc, O] of one dropout forward over the repeated windows, sample
    row f * n_mc + i (pieces of a resumed replay add `sample_row_base`, so they name the same rows).  feats float32 [F, I]; `rows`: frames."""
    q = REPLAY
    name, n_mc, T = q["model"], q["n_mc"], orc.MODEL_CONFIGS[q["model"]]["T"]
    frames = np.arange(q["F"]) if rows is None else np.asarray(rows)
    win = np.array([_clamped(f, 0, T) for f in frames])
    g = (frames[:, None] * n_mc + np.arange(n_mc)[None, :]).reshape(-1)
    ns = {name: dict(stats, yy_m=np.zeros_like(stats["yy_m"]), yy_s=np.ones_like(stats["yy_s"]))}        # targets stay normalised
    return frame_targets(ns, "lstm", name, feats, win, q["seed"], n_mc, variant, g, with32)


def host_features(rows):
    """the pocket feature builder on the host, float32 [n, 22] (the GPU tests take the device builder's rows instead)"""
    from wear_mocap_ape_amd.data_types import messaging
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_nn import features_from_row
    return np.stack([np.asarray(features_from_row(r, messaging.WATCH_PHONE_IMU_LOOKUP), dtype=np.float32) for r in rows])


def trace_rows(golden, n, seed):
    """raw pocket messages near the recorded trace (tests/test_replay._synthetic_rows)"""
    base = golden("stream_trace_pocket.npz")["rows"].astype(np.float32)
    rng = np.random.default_rng(seed)
    rows = np.tile(base, ((n + len(base) - 1) // len(base), 1))[:n]
    return rows + np.float32(1e-3) * rng.standard_normal(rows.shape, dtype=np.float32)


# ---------------- Kalman forward with device draws -----------------------------------------------------------------------------------------
# (regime, (S, E, W)) of tests/kalman_cases.py; (1, 48, 10): 48-row signs of 140 / 256 / 512 columns -- sign columns beyond 128 (the second
# Philox call of a row) and all four words of a call
KALMAN_CASES = (("benign", (2, 24, 10)), ("spread10", (2, 24, 10)), ("benign", (5, 17, 2)), ("spread10", (5, 17, 2)), ("benign", (1, 48, 10)))
KALMAN_SEEDS = {(2, 24, 10): 0x9E3779B97F4A7C15, (5, 17, 2): 12345, (1, 48, 10): 0x1_0000_0000 + 3}      # 12345: low word only
_KALMAN = {}


def kalman_id(case):
    return f"{case[0]}-S{case[1][0]}E{case[1][1]}W{case[1][2]}"


def _moved(nz, seed):
    """the normal draws moved by +-2 float32 ulps with seeded random signs; the +-1 signs as they are"""
    rng = np.random.default_rng(seed)
    out = {}
    for name, d in nz.items():
        out[name] = dict(d)
        for k in ("eps_w", "eps_b"):
            a = d[k]
            s = np.where(rng.random(a.shape) < 0.5, -1.0, 1.0).astype(np.float32)
            out[name][k] = (a + s * np.float32(2.0) * np.spacing(np.abs(a))).astype(np.float32)
    return out


def kalman_case(case, call, variant=ph.CONTRACT):
    """call number `call` (1 or 2) after manual_seed(KALMAN_SEEDS[shape]) on the case's weights and inputs: the replica's draws, the float64
    reference, e_ref (float32 oracle with the kernel's Gauss-Jordan against the float64 one, as tests/kalman_cases.py) and e_draw"""
    from oracle import kalman_oracle as ko
    from tests import kalman_cases as kc
    if (case, call, variant) in _KALMAN:
        return _KALMAN[case, call, variant]
    regime, shape = case
    S, E, W = shape
    c = kc.make_case((regime, shape, kc.WEIGHT_SEEDS[0]))
    key = ph.kalman_call_seed(KALMAN_SEEDS[shape], call)
    nz = ph.kalman_noise(key, W, S * E, v=variant)
    args = (c["sd"], c["raw"], c["state"])
    ref = ko.kalman_forward(*args, nz, dtype=np.float64, inverse="inv64")
    out = dict(sd=c["sd"], raw=c["raw"], state=c["state"], S=S, E=E, W=W, key=key, nz=nz, ref=ref)
    if variant == ph.CONTRACT:
        gj = ko.kalman_forward(*args, nz, dtype=np.float64, inverse="gj")
        out["e_ref"] = kc.errors(ko.kalman_forward(*args, nz, dtype=np.float32, inverse="gj"), gj)
        out["e_draw"] = kc.errors(ko.kalman_forward(*args, _moved(nz, call), dtype=np.float64, inverse="inv64"), ref)
    _KALMAN[case, call, variant] = out
    return out
