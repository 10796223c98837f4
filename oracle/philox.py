"""Host replica of the device-side random numbers  --  TEST INFRASTRUCTURE, NOT PRODUCT.

Every Monte-Carlo kernel of this project draws from Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as easy as 1, 2, 3"),
a counter-based generator: a number is a pure function of a 128-bit counter and a 64-bit key.  The counters are plain functions of
(row, step, unit, layer) and the key is the call's seed (include/ape_hip.h, "Random numbers"), so the host can compute the very numbers
the device must draw, and a Monte-Carlo route can be held to a float64 reference exactly like an eval-mode one.

This file is written from that contract, not from a kernel: numpy only, vectorised, integers in uint64 with explicit masks.

    philox4x32_10        the generator
    lstm_masks           inter-layer dropout multipliers of the LSTM kernels
    ff_mask, ff_bank_mask   DropoutFF: the batch kernel's and the bank head's multipliers
    kalman_normals, kalman_signs, kalman_noise, kalman_init_noise      the Kalman filter's flipout and format_state draws
    lstm_call_seed, bank_call_seed, kalman_call_seed                    the per-call keys

`Variant` switches single details of the scheme to a wrong reading (tests/test_philox_cpu.py proves with it that the GPU tests can tell
each such reading from the right one); the default is the contract.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict

import numpy as np

from oracle import kalman_oracle as ko

F = np.float32
U64 = np.uint64
M32 = U64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = U64(0xD2511F53), U64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = U64(0x9E3779B9), U64(0xBB67AE85)
TAG_FF, TAG_FF_BANK = 0xFF, 0xFE
KALMAN_WORD, SIGN_WORD = 0x4B414C4D, 0x5349474E          # "KALM", "SIGN"
TAG_PERTURB, TAG_SIGN, TAG_INIT = 0x100, 0x200, 0x300
KALMAN_CALL_STEP = 0xD1342543DE82EF95
# blob order of the nine Kalman layers (include/ape_hip.h): the sign tags carry this index, the perturbation tags the flipout layer's rank
KALMAN_LAYER_INDEX = {"process_model.bayes1": 0, "process_model.bayes3": 1, "sensor_model.fc3": 4, "sensor_model.fc5": 5,
                      "sensor_model.fc6": 6}


@dataclass(frozen=True)
class Variant:
    """the contract (defaults) or one wrong reading of it"""
    rounds: int = 10
    swap_t_u: bool = False          # counter (b & ~3, u, t, l)
    row_unaligned: bool = False     # counter word 0 = b
    word_shift: int = 0             # word (b + word_shift) & 3
    drop_k1: bool = False           # key high word forced to 0
    layer_shift: int = 0            # counter word 3 = l + layer_shift
    mantissa_shift: int = 8         # uf from w >> mantissa_shift
    sign_bit_shift: int = 0         # sign bit (c >> sign_bit_shift) & 31
    sign_word_shift: int = 5        # sign word (c >> sign_word_shift) & 3
    swap_sin_cos: bool = False      # sine for even idx


CONTRACT = Variant()


def philox4x32_10(counters, seed: int, rounds: int = 10) -> np.ndarray:
    """counters [..., 4] (any integer type; taken mod 2^32), seed 64 bits: key (seed & 0xFFFFFFFF, seed >> 32) -> uint32 [..., 4];
    `rounds` other than 10 is no Philox4x32-10: the mutant tests use it"""
    c = np.asarray(counters).astype(U64) & M32
    if c.shape[-1] != 4:
        raise ValueError("counters must end in an axis of 4 words")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = U64(seed & 0xFFFFFFFF), U64(seed >> 32)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2            # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> U64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _philox(c0, c1, c2, c3, seed, v: Variant):
    """broadcasting front end -> uint32 [..., 4]"""
    b = np.broadcast_arrays(*(np.asarray(a, dtype=np.int64) for a in (c0, c1, c2, c3)))
    return philox4x32_10(np.stack(b, axis=-1), int(seed) & 0xFFFFFFFF if v.drop_k1 else seed, v.rounds)


def _select(words, which):
    """words [..., 4], which [...] in 0..3 -> [...]"""
    return np.take_along_axis(words, np.asarray(which, dtype=np.int64)[..., None] & 3, axis=-1)[..., 0]


def _row_index(rows, base: int = 0) -> np.ndarray:
    """`rows`: a count (rows base .. base + rows - 1) or the global row numbers themselves (any subset, any order)"""
    r = np.arange(int(rows), dtype=np.int64) if np.ndim(rows) == 0 else np.asarray(rows, dtype=np.int64).reshape(-1)
    return r + int(base)


def _keep_multiplier(w, p: float, v: Variant):
    """uf = float32(w >> 8) * 2^-24 (exact: 24 bits); keep iff uf >= float32(p); multiplier float32(1) / (float32(1) - float32(p))"""
    uf = (w >> np.uint32(v.mantissa_shift)).astype(F) * F(2.0 ** -24)
    return np.where(uf >= F(p), F(1.0) / (F(1.0) - F(p)), F(0.0)).astype(F)


def lstm_masks(seed: int, rows, T: int, H: int, L: int, p: float, row_base: int = 0, v: Variant = CONTRACT) -> np.ndarray:
    """multipliers on the outputs of model layers 0..L-2 for global rows row_base .. row_base + rows - 1 (or the listed global rows, see
    `_row_index`) -> float32 [L-1, rows, T, H]: counter (b & ~3, t, u, l), word b & 3"""
    l = np.arange(L - 1, dtype=np.int64)[:, None, None, None]
    b = _row_index(rows, row_base)[None, :, None, None]
    t = np.arange(T, dtype=np.int64)[None, None, :, None]
    u = np.arange(H, dtype=np.int64)[None, None, None, :]
    c0 = b if v.row_unaligned else b & ~3
    c1, c2 = (u, t) if v.swap_t_u else (t, u)
    w = _philox(c0, c1, c2, l + v.layer_shift, seed, v)
    return _keep_multiplier(_select(w, np.broadcast_to(b + v.word_shift, w.shape[:-1])), p, v)


def ff_mask(seed: int, rows, H: int, p: float, v: Variant = CONTRACT) -> np.ndarray:
    """DropoutFF's batch kernel (mlp_tile16): multipliers on the last hidden activation -> float32 [rows, H]:
    counter (row & ~3, 0, col, 0xFF), word row & 3"""
    r = _row_index(rows)[:, None]
    col = np.arange(H, dtype=np.int64)[None, :]
    c0 = r if v.row_unaligned else r & ~3
    c1, c2 = (col, 0) if v.swap_t_u else (0, col)
    w = _philox(c0, c1, c2, TAG_FF + v.layer_shift, seed, v)
    return _keep_multiplier(_select(w, np.broadcast_to(r + v.word_shift, w.shape[:-1])), p, v)


def ff_bank_mask(seed: int, rows, H: int, p: float, philox_base: int = 0, v: Variant = CONTRACT) -> np.ndarray:
    """the DropoutFF bank head (ff_bank): sample row r = stream * n_mc + sample -> float32 [rows, H]:
    counter (lo32(r + philox_base), hi32(r + philox_base), unit >> 2, 0xFE), word unit & 3"""
    r = _row_index(rows, philox_base)[:, None]
    unit = np.arange(H, dtype=np.int64)[None, :]
    c1, c2 = (unit >> 2, r >> 32) if v.swap_t_u else (r >> 32, unit >> 2)
    w = _philox(r & 0xFFFFFFFF, c1, c2, TAG_FF_BANK + v.layer_shift, seed, v)
    return _keep_multiplier(_select(w, np.broadcast_to(unit + v.word_shift, w.shape[:-1])), p, v)


# ---------------- Kalman -------------------------------------------------------------------------------------------------------------
def _box_muller_inputs(idx, tag: int, seed: int, v: Variant):
    """the float32 inputs of the four library calls, bit for bit: u in (0, 1] for the logarithm, the angle a for sine / cosine"""
    idx = np.asarray(idx, dtype=np.int64)
    w = _philox(idx >> 2, tag, KALMAN_WORD, 0, seed, v)
    pair = (idx >> 1) & 1
    w_r, w_a = _select(w, 2 * pair), _select(w, 2 * pair + 1)
    u = ((w_r >> np.uint32(v.mantissa_shift)).astype(F) + F(1.0)) * F(2.0 ** -24)          # exact
    a = (F(6.283185307179586) * w_a.astype(F)) * F(2.0 ** -32)                              # uint32 -> float32 rounds to nearest
    return u, a


def kalman_radius(idx, tag: int, seed: int, v: Variant = CONTRACT) -> np.ndarray:
    """Box-Muller radius sqrt(-2 log u) of draw idx, float64"""
    u, _ = _box_muller_inputs(idx, tag, seed, v)
    return np.sqrt(-2.0 * np.log(u.astype(np.float64)))


def kalman_normals(idx, tag: int, seed: int, v: Variant = CONTRACT) -> np.ndarray:
    """standard normal number idx of stream (tag, seed): counter (idx >> 2, tag, "KALM", 0), Box-Muller pair (idx >> 1) & 1, cosine for
    even idx.  float32 up to the inputs of log / sqrt / sin / cos as the device forms them; the transcendentals and the products behind
    them in float64; the result rounded to float32 (so the device's value differs by the rounding of its four float32 library calls
    and of the products behind them only)."""
    idx = np.asarray(idx, dtype=np.int64)
    u, a = _box_muller_inputs(idx, tag, seed, v)
    r = np.sqrt(-2.0 * np.log(u.astype(np.float64)))
    a = a.astype(np.float64)
    odd = (idx & 1) == (0 if v.swap_sin_cos else 1)
    return (r * np.where(odd, np.sin(a), np.cos(a))).astype(F)


def kalman_signs(R: int, N: int, tag: int, seed: int, v: Variant = CONTRACT) -> np.ndarray:
    """+-1 number (r, c) of sign stream tag -> float32 [R, N]: counter (c >> 7, r, tag, "SIGN"), word (c >> 5) & 3, bit c & 31, set = -1"""
    r = np.arange(R, dtype=np.int64)[:, None]
    c = np.arange(N, dtype=np.int64)[None, :]
    w = _philox(c >> 7, r, tag, SIGN_WORD, seed, v)
    word = _select(w, np.broadcast_to(c >> v.sign_word_shift, w.shape[:-1]))
    bit = (word >> ((c >> v.sign_bit_shift) & 31).astype(np.uint32)) & np.uint32(1)
    return np.where(bit == 1, F(-1), F(1)).astype(F)


def kalman_noise(seed: int, W: int, rows: int, v: Variant = CONTRACT) -> Dict[str, Dict[str, np.ndarray]]:
    """the `nz` dict of kalman_oracle.draw_noise, filled with what the device draws under key `seed` (rows = streams * ensemble):
    perturbation segments 2j (weights, row-major [N, K]) and 2j + 1 (bias) of flipout layer j under tag 0x100 + segment; signs of the
    layer with blob index i under tags 0x200 + 2i (in, [rows, K]) and 0x201 + 2i (out, [rows, N])"""
    nz = {}
    for j, name in enumerate(ko.FLIPOUT_LAYERS):
        n, k = ko.layer_shapes(W)[name]
        i = KALMAN_LAYER_INDEX[name]
        nz[name] = {"eps_w": kalman_normals(np.arange(n * k), TAG_PERTURB + 2 * j, seed, v).reshape(n, k),
                    "eps_b": kalman_normals(np.arange(n), TAG_PERTURB + 2 * j + 1, seed, v),
                    "sign_in": kalman_signs(rows, k, TAG_SIGN + 2 * i, seed, v),
                    "sign_out": kalman_signs(rows, n, TAG_SIGN + 2 * i + 1, seed, v)}
    return nz


def kalman_init_noise(seed: int, K: int, E: int, v: Variant = CONTRACT) -> np.ndarray:
    """format_state's (and the bank's init) standard-normal draws -> float32 [K, E, 14]: draw idx = flat index, tag 0x300"""
    return kalman_normals(np.arange(K * E * ko.DIM_X), TAG_INIT, seed, v).reshape(K, E, ko.DIM_X)


# ---------------- per-call keys ------------------------------------------------------------------------------------------------------
def lstm_call_seed(manual_seed: int, call: int) -> int:
    """nn_models.py: the key of Monte-Carlo call number `call` (1 for the first) after manual_seed()"""
    return ((int(manual_seed) << 20) + int(call)) & 0xFFFFFFFFFFFFFFFF


def bank_call_seed(seed: int, mc_calls: int) -> int:
    """stream banks: the key of a frame when `mc_calls` Monte-Carlo frames went before it (reset() does not rewind the count)"""
    return (int(seed) + int(mc_calls)) & 0xFFFFFFFFFFFFFFFF


def kalman_call_seed(seed: int, calls: int) -> int:
    """KalmanSmartwatchModel / KalmanStreamBank: the key of call number `calls` (1 for the first) after manual_seed(seed)"""
    return (int(seed) + KALMAN_CALL_STEP * int(calls)) & 0xFFFFFFFFFFFFFFFF
