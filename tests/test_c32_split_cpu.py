"""CPU tests of the f16 hi / lo split of lstm_cluster32.hip (no GPU: `ape_debug_pack_c32_split` is pure host code).

(a) the real host packer: every weight comes back from hi + lo to 2^-22 relative, in the 32x32x16 A-fragment order, the input
    columns of layer 0 stay f32 (times 2^S), and what cannot be scaled is refused;
(b) a numpy emulation of the kernel's product form -- layer 0's input columns on the f32 chain, every other product as
    W_hi h_hi + W_hi h_lo + W_lo h_hi of power-of-two scaled operands (each product exact, f32 sums), 2^-S folded into the gate
    constants, the head on the f32 h of the last step -- through the pocket and watch models, against the f32 oracle."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from oracle import ape_oracle as orc

REPO = Path(__file__).resolve().parents[1]
HSHIFT = 15          # APE_C32_HSHIFT


def _pack(w_ih, w_hh, KXl, kx_f32):
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    fn = lib.ape_debug_pack_c32_split
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    w_ih = np.ascontiguousarray(w_ih, dtype=np.float32)
    w_hh = np.ascontiguousarray(w_hh, dtype=np.float32)
    H = w_hh.shape[1]
    out = np.zeros(8 * 4 * ((KXl + H) // 2) * 64, dtype=np.uint32)
    S = fn(w_ih.ctypes.data, w_ih.shape[1], w_hh.ctypes.data, H, KXl, kx_f32, out.ctypes.data)
    return S, out


def _unpack(img, H, KXl, kx_f32, S):
    """image -> (Wcat as f32 from the f32 groups / 2^S, Wcat as hi + lo / 2^sw from the split groups, hi, lo) in [4H, K] order"""
    K = KXl + H
    NG = kx_f32 // 8 + 2 * ((K - kx_f32) // 16)
    v = img.reshape(8, 4, NG, 64, 4)
    sw = S - HSHIFT
    W = np.full((4 * H, K), np.nan)
    hi = np.full((4 * H, K), np.nan)
    lo = np.full((4 * H, K), np.nan)
    lane = np.arange(64)
    mcol, hh = lane & 31, lane >> 5
    for mem in range(8):
        for w in range(4):
            row = (mcol >> 3) * H + mem * 32 + w * 8 + (mcol & 7)
            for g in range(kx_f32 // 8):
                f = v[mem, w, g].view(np.float32)
                for j in range(4):
                    W[row, 8 * g + 4 * hh + j] = np.ldexp(f[:, j].astype(np.float64), -S)
            for s in range((K - kx_f32) // 16):
                gh, gl = kx_f32 // 8 + 2 * s, kx_f32 // 8 + 2 * s + 1
                fh = v[mem, w, gh].copy().view(np.float16).astype(np.float64)       # [lane][8 halves]
                fl = v[mem, w, gl].copy().view(np.float16).astype(np.float64)
                for e in range(8):
                    k = kx_f32 + 16 * s + 8 * hh + e
                    hi[row, k], lo[row, k] = fh[:, e], fl[:, e]
                    W[row, k] = np.ldexp(fh[:, e] + fl[:, e], -sw)
    return W, hi, lo


def _wcat(w_ih, w_hh, KXl):
    H = w_hh.shape[1]
    W = np.zeros((4 * H, KXl + H), dtype=np.float64)
    W[:, :w_ih.shape[1]] = w_ih
    W[:, KXl:] = w_hh
    return W


@pytest.mark.parametrize("scale", [1.0, 8.0, 1e-3])
def test_packer_round_trip(scale):
    cfg = orc.MODEL_CONFIGS["pocket"]
    sd = orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], seed=0)
    H = cfg["H"]
    for l, (KXl, kx) in enumerate([(32, 32), (H, 0)]):
        w_ih = sd[f"lstm.weight_ih_l{l}"] * np.float32(scale)
        w_hh = sd[f"lstm.weight_hh_l{l}"] * np.float32(scale)
        S, img = _pack(w_ih, w_hh, KXl, kx)
        Wc = _wcat(w_ih, w_hh, KXl)
        wmax = np.abs(Wc[:, kx:]).max()
        sw = S - HSHIFT
        assert 2.0 ** 14 <= wmax * 2.0 ** sw < 2.0 ** 15
        W, hi, lo = _unpack(img, H, KXl, kx, S)
        assert not np.isnan(W).any()                                     # every (row, k) exactly once
        np.testing.assert_array_equal(W[:, :kx], Wc[:, :kx])           # input columns: f32 times 2^S, exact
        err = np.abs(W[:, kx:] - Wc[:, kx:])
        assert (err <= 2.0 ** -22 * np.abs(Wc[:, kx:]) + 2.0 ** (-25 - sw)).all(), float((err / np.abs(Wc[:, kx:])).max())
        # hi is the rounded weight, lo the rounded residual
        np.testing.assert_array_equal(hi[:, kx:], np.ldexp(Wc[:, kx:], sw).astype(np.float16).astype(np.float64))
        assert (np.abs(hi[:, kx:]) < 65504).all()


def test_packer_refuses_what_it_cannot_scale():
    H = 256
    rng = np.random.default_rng(0)
    w_ih = rng.uniform(-0.06, 0.06, (4 * H, 22)).astype(np.float32)
    w_hh = rng.uniform(-0.06, 0.06, (4 * H, H)).astype(np.float32)
    assert _pack(w_ih, w_hh, 32, 32)[0] > 0
    bad = w_hh.copy()
    bad[3, 7] = np.nan
    assert _pack(w_ih, bad, 32, 32)[0] == -1
    bad[3, 7] = np.inf
    assert _pack(w_ih, bad, 32, 32)[0] == -1
    assert _pack(w_ih, w_hh * np.float32(1e12), 32, 32)[0] == -1       # scale below 2^0
    assert _pack(w_ih, w_hh * np.float32(1e-20), 32, 32)[0] == -1      # scale above 2^64


# ---- (b) the kernel's product form in numpy ---------------------------------------------------------------------------------

def _split(v):
    hi = v.astype(np.float16).astype(np.float32)
    lo = (v - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def _sig(v):
    return (1.0 / (1.0 + np.exp(-v))).astype(np.float32)


def _emulate(sd, xn, KX=32):
    B, T, I = xn.shape
    H = sd["lstm.weight_hh_l0"].shape[1]
    seq_in = np.zeros((B, T, KX), dtype=np.float32)
    seq_in[..., :I] = xn
    hs_prev = None
    for l in range(2):
        w_ih, w_hh = sd[f"lstm.weight_ih_l{l}"], sd[f"lstm.weight_hh_l{l}"]
        KXl, kx = (KX, KX) if l == 0 else (H, 0)
        S, img = _pack(w_ih, w_hh, KXl, kx)
        _, whi, wlo = _unpack(img, H, KXl, kx, S)
        whi, wlo = whi[:, kx:].astype(np.float32), wlo[:, kx:].astype(np.float32)
        wx = np.ldexp(_wcat(w_ih, w_hh, KXl)[:, :kx], S).astype(np.float32)
        b = ((sd[f"lstm.bias_ih_l{l}"] + sd[f"lstm.bias_hh_l{l}"]).astype(np.float32) * np.float32(2.0 ** S)).astype(np.float32)
        h = np.zeros((B, H), np.float32)
        c = np.zeros((B, H), np.float32)
        out = []
        for t in range(T):
            hsplit = _split(h * np.float32(2.0 ** HSHIFT))
            if l == 0:
                src = hsplit
                acc = b + seq_in[:, t] @ wx.T
            else:
                src = tuple(np.concatenate([a, r], axis=1) for a, r in zip(hs_prev[t], hsplit))
                acc = b + np.zeros((B, 4 * H), np.float32)
            acc = acc + src[0] @ whi.T + src[1] @ whi.T + src[0] @ wlo.T
            pre = (acc * np.float32(2.0 ** -S)).astype(np.float32)          # exact: the descale in the gate constants
            i, f, g, o = _sig(pre[:, :H]), _sig(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), _sig(pre[:, 3 * H:])
            c = (f * c + i * g).astype(np.float32)
            h = (o * np.tanh(c)).astype(np.float32)
            out.append(h)
        # what layer 1 reads of layer 0: the split of h * 2^HSHIFT; the head reads the f32 h of the top layer's last step
        hs_prev = [_split(hh * np.float32(2.0 ** HSHIFT)) for hh in out]
    return (h @ sd["output_layer.weight"].T + sd["output_layer.bias"]).astype(np.float32)


@pytest.mark.parametrize("name,B,T", [("pocket", 256, 64), ("watch", 256, 13), ("pocket", 256, 1), ("watch", 256, 6)])
def test_split_product_form_against_oracle(name, B, T):
    raw = json.loads((REPO / "tests" / "golden" / "norm_stats.json").read_text())[name]
    st = {k: np.array(raw[k]) for k in ("xx_m", "xx_s")}
    cfg = orc.MODEL_CONFIGS[name]
    sd = orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], seed=0)
    rng = np.random.default_rng(11)
    x = (st["xx_m"] + st["xx_s"] * rng.normal(size=(B, T, cfg["I"]))).astype(np.float32)
    xn = ((x.astype(np.float64) - st["xx_m"]) / st["xx_s"]).astype(np.float32)
    y = _emulate(sd, xn)
    y_ref = orc.lstm_forward(sd, xn)[:, -1]
    err = float(np.abs(y - y_ref).max())
    print(f"\n[{name} {B}x{T}] split emulation vs f32 oracle {err:.2e}")
    assert err <= 2.5e-7
