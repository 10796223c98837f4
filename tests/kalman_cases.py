"""The cases of tests/test_kalman_numerics_cpu.py and tests/test_kalman_numerics_gpu.py, built once: inputs, weights, injected draws, the
float64 reference of ``oracle/kalman_oracle.py`` and the yardstick ``e_ref``; and the oracle variants ("mutants") that prove the cases can
tell a subtly wrong ``csrc/kalman.hip`` from a right one.

Reference : ``ko.kalman_forward(..., dtype=float64, inverse="gj")``.
Yardstick : ``e_ref[output] = max |ko.kalman_forward(..., dtype=float32, inverse="gj") - reference|`` -- float32 arithmetic of the kernel's own
            algorithm (Gauss-Jordan with partial pivoting), never a kernel's result.
Budget    : ``max(1e-6, 4 * e_ref)`` per output, the rule of tests/test_hostile_inputs_gpu.py (another summation order, fused multiply-adds).
A case is HELD when every ``e_ref <= 1e-5``; ``spread100`` and ``spread1000`` are record-only by construction (condition 6e3 / 7e5: float32
Gauss-Jordan itself is 1e-4 / 5e-3 off there)."""
import functools

import numpy as np

from oracle import kalman_oracle as ko
from tests.test_kalman import synthetic_inputs

OUTPUTS = ("state_corrected", "m_state_corrected", "m_state_pred", "z", "ensemble_z")
HELD_E_REF = 1e-5
FLOOR, FACTOR = 1e-6, 4.0

# (S, E, W): what the shape is there for
SHAPES = (
    (1, 2, 2),        # smallest everything: R = 2 inside one 16-row tile, K = 28 / 44 padded to 32 / 48, E - 1 = 1
    (5, 17, 2),       # R = 85: ragged last tile, streams straddle the tiles at odd offsets
    (3, 24, 10),      # straddling at the deployed window
    (2, 48, 10),      # the deployed ensemble
    (17, 16, 4),      # many update workgroups
    (1, 128, 22),     # both limits: K = 308 / 484 staging, MAXE rows in the update's LDS
)
WEIGHT_SEEDS = (4, 5)
REGIME_SHAPES = ((2, 24, 10), (5, 17, 2))
REGIMES = ("spread10", "spread100", "spread1000", "collapsed", "bigR", "loud_z")
RECORD_ONLY = ("spread100", "spread1000")

CASES = tuple(("benign", shape, seed) for shape in SHAPES for seed in WEIGHT_SEEDS) + \
    tuple((regime, shape, WEIGHT_SEEDS[0]) for shape in REGIME_SHAPES for regime in REGIMES)


def case_id(case):
    regime, (S, E, W), seed = case
    return f"{regime}-S{S}E{E}W{W}-w{seed}"


def is_held_by_design(case):
    return case[0] not in RECORD_ONLY


def budget(e_ref):
    return max(FLOOR, FACTOR * e_ref)


def apply_regime(regime, sd, raw, state, nz):
    """-> (sd, raw, state, nz) of the regime, the arguments left as they were"""
    sd, nz = dict(sd), {k: dict(v) for k, v in nz.items()}
    if regime.startswith("spread"):
        # rows of the last process layer 1 .. spread geometrically, two rows nearly parallel to their neighbours, a larger state: the innovation
        # P + R then has off-diagonal entries above its diagonal ones and Gauss-Jordan has to swap rows
        spread = float(regime[len("spread"):])
        scale = (spread ** (np.arange(ko.DIM_X) / (ko.DIM_X - 1.0))).astype(np.float32)
        for key in ("weight", "bias"):
            v = sd["process_model.bayes_m2." + key] * (scale[:, None] if key == "weight" else scale)
            v[1] = 10.0 * v[0] + 0.1 * v[1]
            v[5] = -3.0 * v[4] + 0.05 * v[5]
            sd["process_model.bayes_m2." + key] = v.astype(np.float32)
        state = (3.0 * state).astype(np.float32)
    elif regime == "collapsed":
        # one history for all members of a stream and no weight perturbation in the process model: every member predicts the same state
        state = np.repeat(state[:, :1], state.shape[1], axis=1).copy()
        for name in ("process_model.bayes1", "process_model.bayes3"):
            nz[name]["eps_w"] = np.zeros_like(nz[name]["eps_w"])
            nz[name]["eps_b"] = np.zeros_like(nz[name]["eps_b"])
    elif regime == "bigR":
        sd["observation_noise.fc2.bias"] = sd["observation_noise.fc2.bias"] + np.float32(1e4)
    elif regime == "loud_z":
        for key in ("mu_weight", "mu_bias"):
            sd["sensor_model.fc6." + key] = (np.float32(30.0) * sd["sensor_model.fc6." + key]).astype(np.float32)
    elif regime != "benign":
        raise ValueError(regime)
    return sd, raw, state, nz


def errors(got, ref):
    return [float(np.abs(np.asarray(g, np.float64) - r).max()) for g, r in zip(got, ref)]


@functools.lru_cache(maxsize=None)
def make_case(case):
    """everything the tests need of one case, computed once and never written to afterwards"""
    regime, (S, E, W), seed = case
    rng = np.random.default_rng(1000 * S + 10 * E + W)
    sd = ko.make_state_dict(W, seed)
    raw, state = synthetic_inputs(rng, S, E, W)
    nz = ko.draw_noise(rng, W, S * E)
    sd, raw, state, nz = apply_regime(regime, sd, raw, state, nz)
    info = {}
    ref = ko.kalman_forward(sd, raw, state, nz, dtype=np.float64, inverse="gj", info=info)
    info32 = {}
    f32 = ko.kalman_forward(sd, raw, state, nz, dtype=np.float32, inverse="gj", info=info32)
    e_ref = errors(f32, ref)
    for a in (raw, state, *ref, *sd.values(), *(v for d in nz.values() for v in d.values())):
        a.setflags(write=False)
    return dict(case=case, id=case_id(case), S=S, E=E, W=W, sd=sd, raw=raw, state=state, nz=nz, ref=ref, e_ref=e_ref,
                swaps=info["swaps"], swaps32=info32["swaps"], cond=info["cond"], held=max(e_ref) <= HELD_E_REF,
                magnitude=[float(np.abs(r).max()) for r in ref])


def line(c, gpu_err=None):
    """the record line of a case: `KALNUM|case|swaps|cond|held|output e_ref [gpu err] budget ...`"""
    parts = [f"KALNUM|{c['id']}|swaps {c['swaps']}|cond {c['cond']:.3g}|{'held' if c['held'] else 'record only'}"]
    for i, name in enumerate(OUTPUTS):
        gpu = "" if gpu_err is None else f" gpu {gpu_err[i]:.2e}"
        parts.append(f"{name} e_ref {c['e_ref'][i]:.2e}{gpu} budget {budget(c['e_ref'][i]):.2e}")
    return "|".join(parts)


# ---------------- oracle variants -------------------------------------------------------------------------------------------------------------
MUTANTS = (
    "no_1e-3",            # 1  observation noise without the + 1e-3
    "swap_left_half",     # 2  the row swap exchanges the 14 left columns only
    "P_over_E",           # 3  P = A^T A / E
    "no_bias_pert",       # 4  the flipout bias perturbation dropped
    "sign_out_row_mod16", # 5  sign_out of row r % 16 (the row inside the tile) instead of row r
    "sensor_row_div16",   # 6  the sensor model's input row read as r // 16 instead of r // E
    "gaussian_only",      # 7  the elimination skips the rows above the pivot
    "mean_Em1",           # 8  ensemble means over E - 1 members
)


def _flipout(x, sd, name, nz, dt, mutant):
    out = ko.linear(x, sd[name + ".mu_weight"], sd[name + ".mu_bias"], dt)
    dw = (ko.softplus(sd[name + ".rho_weight"], dt) * nz["eps_w"].astype(dt)).astype(dt)
    db = (ko.softplus(sd[name + ".rho_bias"], dt) * nz["eps_b"].astype(dt)).astype(dt)
    if mutant == "no_bias_pert":
        db = np.zeros_like(db)
    sign_out = nz["sign_out"]
    if mutant == "sign_out_row_mod16":
        sign_out = sign_out[np.arange(x.shape[0]) % 16]
    pert = ko.linear((x * nz["sign_in"]).astype(dt), dw, db, dt)
    return (out + pert * sign_out).astype(dt)


def _gauss_jordan(a, dt, mutant):
    n = a.shape[0]
    m = np.concatenate([a.astype(dt), np.eye(n, dtype=dt)], axis=1)
    for c in range(n):
        piv = c + int(np.argmax(np.abs(m[c:, c])))
        if piv != c:
            cols = slice(0, n) if mutant == "swap_left_half" else slice(None)
            m[[c, piv], cols] = m[[piv, c], cols]
        m[c] = m[c] / m[c, c]
        others = np.arange(n) > c if mutant == "gaussian_only" else np.arange(n) != c
        m[others] = m[others] - np.outer(m[others, c], m[c])
    return m[:, n:].copy()


def _mean(x, dt, mutant):
    """mean over the members (axis 1)"""
    return (x[:, :-1] if mutant == "mean_Em1" else x).mean(axis=1, dtype=dt)


def variant_forward(sd, raw, state, nz, dtype=np.float32, mutant=None):
    """``ko.kalman_forward(..., dtype, inverse="gj")`` restated with one switch per mutant; ``mutant=None`` is bit-equal to the oracle
    (asserted in tests/test_kalman_numerics_cpu.py), so a mutant differs from the oracle by its one change and nothing else"""
    assert mutant is None or mutant in MUTANTS, mutant
    dt = dtype
    S, E = state.shape[0], state.shape[1]
    lrelu = lambda v: ko.leaky_relu(v, dtype=dt)
    h = state.reshape(S * E, -1).astype(dt)
    h = lrelu(_flipout(h, sd, "process_model.bayes1", nz["process_model.bayes1"], dt, mutant))
    h = lrelu(_flipout(h, sd, "process_model.bayes3", nz["process_model.bayes3"], dt, mutant))
    pred = ko.linear(h, sd["process_model.bayes_m2.weight"], sd["process_model.bayes_m2.bias"], dt).reshape(S, E, ko.DIM_X)
    src = np.minimum(np.arange(S * E) // (16 if mutant == "sensor_row_div16" else E), S - 1)
    h = raw.reshape(S, -1)[src].astype(dt)
    h = lrelu(ko.linear(h, sd["sensor_model.fc2.weight"], sd["sensor_model.fc2.bias"], dt))
    h = lrelu(_flipout(h, sd, "sensor_model.fc3", nz["sensor_model.fc3"], dt, mutant))
    h = lrelu(_flipout(h, sd, "sensor_model.fc5", nz["sensor_model.fc5"], dt, mutant))
    ens_z = _flipout(h, sd, "sensor_model.fc6", nz["sensor_model.fc6"], dt, mutant).reshape(S, E, ko.DIM_X)
    state_m, z = _mean(pred, dt, mutant), _mean(ens_z, dt, mutant)
    h = np.maximum(ko.linear(z, sd["observation_noise.fc1.weight"], sd["observation_noise.fc1.bias"], dt), 0).astype(dt)
    h = ko.linear(h, sd["observation_noise.fc2.weight"], sd["observation_noise.fc2.bias"], dt)
    r_diag = (np.square(h + dt(0.0 if mutant == "no_1e-3" else 1e-3)) + dt(0.038729833)).astype(dt)
    corrected = np.empty_like(pred)
    for s in range(S):
        A = (pred[s] - state_m[s]).astype(dt)
        P = (dt(1.0 / (E if mutant == "P_over_E" else E - 1)) * (A.T @ A)).astype(dt)
        inv = _gauss_jordan((P + np.diag(r_diag[s])).astype(dt), dt, mutant)
        K = (P @ inv).astype(dt)
        corrected[s] = pred[s] + (K @ (ens_z[s].T - pred[s].T)).T.astype(dt)
    return (corrected, _mean(corrected, dt, mutant)[:, None, :], state_m[:, None, :], z[:, None, :].astype(dt), ens_z)
