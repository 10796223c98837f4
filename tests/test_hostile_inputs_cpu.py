"""Hostile inputs, the parts that need no GPU: the float64 reference the GPU file (tests/test_hostile_inputs_gpu.py) holds every LSTM
route to, the input cases, and the ring arithmetic of a poisoned stream.

The suite's usual data (`orc.make_state_dict` weights within +-1/sqrt(H), standard-normal z-scores) keeps every gate pre-activation a
fraction of one.  The cases here are what a trained checkpoint and a misbehaving sensor look like:
  trained       `lstm.*` tensors x 16 (TRAINED_SCALE: the scale at which a quarter of layer 0's gates saturate), standard inputs
  trained_long  the same at x 8, for windows of 48 steps and more: there x 16 makes the recurrence chaotic (see LONG_SCALE)
  sat30         inputs at +-30 standard deviations, weights x 4: |h| reaches 1
  z1e3          |z| uniform up to 1e3 (1e2 for the binary16 routes), weights x 1
  benign        the control: same shape and seed, weights x 1, standard inputs
  long4k        weights x 4 on standard inputs, for windows of thousands of steps (tests/test_long_windows_cpu.py): the largest scale at which
                the recurrence is still conditioned over 4000 steps (see LONG4K_SCALE)
They must be hostile to kernels, not to the mathematics: the float64 reference stays finite on all of them (asserted below)."""
import numpy as np
import pytest

from oracle import ape_oracle as orc

CASES = ("trained", "sat30", "z1e3", "benign")
LONG_CASE, LONG_T = "trained_long", 48
# the scale of case `trained` per model.  8, as in tests/test_c32_split_gpu._model(wscale=8), puts only 2.3 % (watch) .. 16.2 % (uarm) of the
# layer-0 gate pre-activations beyond |v| > 4 -- the uniform weights within +-1/sqrt(H) are that small -- and reaches the quarter for
# one model alone (64 inputs on 128 units: 26.3 %).  16 gives 29.1 % (watch) .. 49.7 % (uarm); test_case_trained_saturates_a_quarter_of_layer0
# holds the floor for every entry
TRAINED_SCALE = {"pocket": 16.0, "watch": 16.0, "uarm": 16.0, "imupose": 16.0, "one_22_256": 16.0, "one_32_256": 16.0, "one_38_128": 16.0,
            "one_64_128": 8.0}
# Windows of LONG_T steps and more.  At x 16 the three-layer recurrence is chaotic over 48 steps: rounding errors grow by a factor of about
# 3 per step, the float32 oracle ends 0.8 .. 1.2 away from the float64 reference on outputs of order one, and a budget of 4 e_ref holds
# nothing.  At x 8 the same recurrence is conditioned (e_ref about 1e-4 at step 48, so a budget of about 4e-4 on outputs of order one),
# with 16 % of layer 0's pre-activations beyond 4 and pre-activations of several units throughout: that is the case the long-window
# routes are HELD to; their `trained` row at x 16 is run and recorded.  test_the_long_case_is_conditioned holds e_ref <= 1e-3 for it.
LONG_SCALE = 8.0
# Windows of thousands of steps (the far ends of tests/test_long_windows_*.py).  At x 8 the recurrence is chaotic over 4000 steps (the float32
# oracle ends about 1 from the float64 reference); at x 4 it forgets: e_ref 4.9e-7 (pocket, 4094 steps) and 6.8e-7 (uarm, 4000 steps) over all
# steps on outputs up to 0.7, against 4e-8 at x 1.  tests/test_long_windows_cpu.py holds e_ref <= 1e-5 for every case its GPU half uses.
LONG4K_CASE, LONG4K_SCALE = "long4k", 4.0
CASE_WSCALE = {"sat30": 4.0, "z1e3": 1.0, "benign": 1.0, LONG_CASE: LONG_SCALE, LONG4K_CASE: LONG4K_SCALE}
ONE_LAYER = {"one_22_256": (22, 256, 14), "one_32_256": (32, 256, 12), "one_38_128": (38, 128, 12), "one_64_128": (64, 128, 6)}
SEED_W = 3            # tests/test_c32_split_gpu._model's default weight seed


def wscale_of(model, case):
    return TRAINED_SCALE[model] if case == "trained" else CASE_WSCALE[case]


def dims_of(model):
    """-> (I, H, L, O)"""
    if model in orc.MODEL_CONFIGS:
        c = orc.MODEL_CONFIGS[model]
        return c["I"], c["H"], c["L"], c["O"]
    if model == "imupose":
        return 22, orc.IMUPOSE_HIDDEN, orc.IMUPOSE_LAYERS, 14
    I, H, O = ONE_LAYER[model]
    return I, H, 1, O


def state_dict(model, wscale, seed=SEED_W):
    """the weights of tests/test_c32_split_gpu._model(name, st, wscale, seed): `lstm.*` tensors scaled, head (and ImuPose's input layer) as drawn"""
    I, H, L, O = dims_of(model)
    sd = orc.make_imupose_state_dict(I, O, seed) if model == "imupose" else orc.make_state_dict(I, H, L, O, seed)
    return {k: (v * np.float32(wscale)).astype(np.float32) if k.startswith("lstm.") else v for k, v in sd.items()}


def case_z(case, B, T, I, seed, zmax=1e3):
    """the z-scores of a case, float64 [B,T,I] (the raw features are xx_m + xx_s * z rounded to float32)"""
    rng = np.random.default_rng(seed)
    if case == "sat30":
        return 30.0 * np.sign(rng.normal(size=(B, T, I)))
    if case == "z1e3":
        return rng.uniform(-zmax, zmax, size=(B, T, I))
    return rng.normal(size=(B, T, I))


def raw_and_normalised(st, z):
    """-> (raw float32 features, the float32 z-scores the kernels compute from them: float64 z-score, rounded once)"""
    raw = (st["xx_m"] + st["xx_s"] * z).astype(np.float32)
    return raw, ((raw.astype(np.float64) - st["xx_m"]) / st["xx_s"]).astype(np.float32)


def _sigmoid64(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def lstm_forward64(sd, x, masks=None, pre0=None):
    """the LSTM recurrence and head of nn_models.py:180-189 in plain float64: float32 weights and float32 inputs in, every product, sum,
    exp and tanh in float64.  x [B,T,I] -> y [B,T,O].  `masks`: L-1 arrays [B,T,H] on the outputs of layers 0..L-2.  `pre0`: a list
    that receives layer 0's gate pre-activations [B,4H] of every step."""
    L = sum(1 for k in sd if k.startswith("lstm.weight_ih_l"))
    seq = np.asarray(x, dtype=np.float64)
    B, T, _ = seq.shape
    for k in range(L):
        w_ih, w_hh = sd[f"lstm.weight_ih_l{k}"].astype(np.float64), sd[f"lstm.weight_hh_l{k}"].astype(np.float64)
        b = sd[f"lstm.bias_ih_l{k}"].astype(np.float64) + sd[f"lstm.bias_hh_l{k}"].astype(np.float64)
        H = w_hh.shape[1]
        h, c, out = np.zeros((B, H)), np.zeros((B, H)), np.empty((B, T, H))
        for t in range(T):
            pre = seq[:, t] @ w_ih.T + h @ w_hh.T + b
            if k == 0 and pre0 is not None:
                pre0.append(pre)
            c = _sigmoid64(pre[:, H:2 * H]) * c + _sigmoid64(pre[:, :H]) * np.tanh(pre[:, 2 * H:3 * H])
            h = _sigmoid64(pre[:, 3 * H:]) * np.tanh(c)
            out[:, t] = h
        seq = out if masks is None or k == L - 1 else out * np.asarray(masks[k], dtype=np.float64)
    return seq @ sd["output_layer.weight"].astype(np.float64).T + sd["output_layer.bias"].astype(np.float64)


def forward64(model, sd, x, masks=None, pre0=None):
    """`lstm_forward64` behind ImuPoseLSTM's Linear + ReLU (nn_models.py:236-244) where the model has one"""
    x = np.asarray(x, dtype=np.float64)
    if model == "imupose":
        x = np.maximum(x @ sd["input_layer.weight"].astype(np.float64).T + sd["input_layer.bias"].astype(np.float64), 0.0)
    return lstm_forward64(sd, x, masks, pre0)


def forward32(model, sd, x, masks=None, storage=None):
    """the pinned float32 oracle of the same model"""
    if model == "imupose":
        assert masks is None and storage is None
        return orc.imupose_forward(sd, x)
    return orc.lstm_forward(sd, x, masks=masks, storage=storage)


def poisoned_frames(T, smooth):
    """Frames for which ONE non-finite row makes a bank stream's messages non-finite, the frame of the row included.
    The row sits in slot `frame mod T` of the window ring `xring[S][n_mc][T][I]` until the row T frames later overwrites it: the
    predictions of T frames see it.  Every prediction sits in slot `step mod smooth` of `yring[S][smooth][n_mc][O]` for `smooth`
    steps, and a message averages all of them: the last bad prediction leaves the message smooth - 1 frames after it was made.
    A bank without a window (the FK-only bank; a DropoutFF, which reads the newest row only) has T = 1."""
    if T < 1 or smooth < 1:
        raise ValueError("T and smooth count frames: both at least 1")
    return T + smooth - 1


def has_stats(model):
    """the deployed models (and ImuPose on the pocket features) take raw features; the one-layer models take z-scores as they are"""
    return model in orc.MODEL_CONFIGS or model == "imupose"


def case_xn(norm_stats, model, z):
    """the float32 inputs the recurrence sees"""
    if has_stats(model):
        return raw_and_normalised(norm_stats[model if model in orc.MODEL_CONFIGS else "pocket"], z)[1]
    return z.astype(np.float32)


# ---------------- the tests ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["pocket", "watch", "uarm", "imupose", "one_38_128"])
def test_float64_reference_agrees_with_the_oracle_on_the_benign_case(norm_stats, model):
    """<= 2e-6: the oracle's own stated distance from torch's LSTM (tests/test_oracle_golden.py)"""
    I = dims_of(model)[0]
    sd = state_dict(model, 1.0)
    xn = case_xn(norm_stats, model, case_z("benign", 37, 8, I, 1))
    e = float(np.abs(forward32(model, sd, xn) - forward64(model, sd, xn)).max())
    print(f"\n[{model}] benign 37x8: max |float32 oracle - float64 reference| = {e:.2e}")
    assert e <= 2e-6
    # with injected dropout masks (the Monte-Carlo routes' reference)
    if model in orc.MODEL_CONFIGS:
        L, H = dims_of(model)[2], dims_of(model)[1]
        masks = [(np.random.default_rng(2 + k).random((37, 8, H)) >= 0.2).astype(np.float32) / np.float32(0.8) for k in range(L - 1)]
        assert float(np.abs(forward32(model, sd, xn, masks) - forward64(model, sd, xn, masks)).max()) <= 2e-6


@pytest.mark.parametrize("model", sorted(TRAINED_SCALE))
def test_case_trained_saturates_a_quarter_of_layer0(norm_stats, model):
    """the condition of case `trained`, from the float64 reference alone: at least a quarter of layer 0's gate pre-activations beyond |v| > 4"""
    I = dims_of(model)[0]
    sd = state_dict(model, wscale_of(model, "trained"))
    z = case_z("trained", 64, 6, I, 21)
    xn = case_xn(norm_stats, model, z)
    pre0 = []
    forward64(model, sd, xn, pre0=pre0)
    share = float((np.abs(np.stack(pre0)) > 4.0).mean())
    print(f"\n[{model}] weights x {wscale_of(model, 'trained'):g}: {100 * share:.1f} % of layer-0 gate pre-activations beyond |v| > 4")
    assert share >= 0.25


@pytest.mark.parametrize("case", ["trained", "sat30", "z1e3"])
@pytest.mark.parametrize("model", ["pocket", "watch", "uarm", "imupose", "one_64_128"])
def test_the_cases_are_hostile_to_kernels_not_to_the_mathematics(norm_stats, model, case):
    I = dims_of(model)[0]
    sd = state_dict(model, wscale_of(model, case))
    z = case_z(case, 40, 9, I, 5)
    xn = case_xn(norm_stats, model, z)
    y = forward64(model, sd, xn)
    assert np.isfinite(y).all()
    if case == "sat30":            # what the case is for: hidden states at the top of their range
        pre0 = []
        forward64(model, sd, xn, pre0=pre0)
        assert float(np.abs(np.stack(pre0)).max()) > 30.0


@pytest.mark.parametrize("T", [48, 49])
def test_the_long_case_is_conditioned(norm_stats, T):
    """the case the long-window routes are held to: the float32 oracle stays within 1e-3 of the float64 reference (so 4 e_ref means something
    on outputs of order one), the gates are still driven hard, and the reference is finite; at x 16 the oracle itself is lost"""
    I = dims_of("uarm")[0]
    xn = case_xn(norm_stats, "uarm", case_z(LONG_CASE, 64, T, I, 21))
    sd = state_dict("uarm", wscale_of("uarm", LONG_CASE))
    pre0 = []
    y64 = forward64("uarm", sd, xn, pre0=pre0)[:, -1]
    e = float(np.abs(forward32("uarm", sd, xn)[:, -1] - y64).max())
    share = float((np.abs(np.stack(pre0)) > 4.0).mean())
    sd16 = state_dict("uarm", wscale_of("uarm", "trained"))
    e16x = float(np.abs(forward32("uarm", sd16, xn)[:, -1] - forward64("uarm", sd16, xn)[:, -1]).max())
    print(f"\n[uarm 64x{T}] x {LONG_SCALE:g}: e_ref {e:.2e}, {100 * share:.1f} % of layer-0 pre-activations beyond 4; x 16: e_ref {e16x:.2e}")
    assert np.isfinite(y64).all() and e <= 1e-3 and share >= 0.10
    assert e16x > 1e-2            # why the x 16 row of these routes is a record, not a check


def test_poisoned_frames_ring_arithmetic():
    """a brute-force walk of the two rings against the closed form"""
    for T in (1, 2, 6, 8):
        for smooth in (1, 2, 5):
            for f in (T, T + 3):                       # (past the cold start, which writes the first row into all T slots)
                xring, yring, bad = [False] * T, [False] * smooth, 0
                for frame in range(f + T + smooth + 4):
                    xring[frame % T] = frame == f
                    yring[frame % smooth] = any(xring)
                    bad += any(yring)
                    if frame == f + poisoned_frames(T, smooth):
                        assert not any(yring)
                assert bad == poisoned_frames(T, smooth) == T + smooth - 1
    with pytest.raises(ValueError):
        poisoned_frames(0, 1)
