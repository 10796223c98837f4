"""DropoutFF banks on the test-hooks library (lib/diag/libape_hip_testhooks.so): the dropout in front of the output layer, exact under
injected masks (`ape_debug_set_bank_masks`) and statistical under the bank's own Philox draws, the targets read through
`ape_debug_bank_targets`.  Not collected with the suite: tests/test_regressor_banks_gpu.py runs this file in a child process whose
APE_HIP_LIB names that library."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests import mc_check
from tests.test_hip_parity import TOL_Y_SHORT
from tests.test_hip_round4 import TOL_MSG_LOOP
from tests.test_regressor_banks_gpu import estimator, shifted_rows, state_dict

pytestmark = pytest.mark.gpu


def _hook(lib, name, argtypes):
    assert hasattr(lib, name), "this file runs on the test-hooks library (APE_HIP_LIB)"
    f = getattr(lib, name)
    f.restype, f.argtypes = C.c_int, argtypes
    return f


def _targets(lib, bank, rows, O):
    get = _hook(lib, "ape_debug_bank_targets", [C.c_void_p, C.c_void_p])
    y = np.empty((rows, O), dtype=np.float32)
    assert get(bank._handle, C.c_void_p(y.ctypes.data)) == 0
    return y


@pytest.mark.parametrize("inputs", ["in_range", "trace"])
def test_ff_bank_under_injected_masks_is_the_oracle(golden, tmp_path, monkeypatch, inputs):
    """lockstep frames, p = 0.2, n_mc = 4, masks [S * n_mc, H] of 0 or 1/(1-p): targets = orc.ff_forward(sd, x, mask) over the repeated
    newest rows; messages = oracle de-normalisation, FK and message over each stream's four rows.

    in_range: feature rows inside the deployed statistics (z-scores standard normal, pushed with push_features): the targets are held to
    TOL_Y_SHORT as it stands, the bound of the existing DropoutFF parity tests (the oracle's own float32 error is about 1e-7 there).

    trace: the fixture's wire rows through push_rows.  They lie far outside the deployed statistics, the hidden activations are large, and
    the ORACLE's float32 evaluation is itself further than TOL_Y_SHORT from the float64 evaluation of the same float32 weights, inputs and
    masks (computed below on the host, printed per frame).  Two float32 evaluations in different summation orders may each be that far
    from the exact value, so the device is held to max(TOL_Y_SHORT, 2 x the oracle's own float32 error on that frame) there."""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    lib = _hip.lib()
    set_masks = _hook(lib, "ape_debug_set_bank_masks", [C.c_void_p, C.c_void_p])
    S, n_mc, p, frames, name = 37, 4, 0.2, 5, "pocket"
    est = estimator(tmp_path, monkeypatch, "ff", name, seed=3, dropout=p, smooth=1, add_mc_samples=True, monte_carlo_samples=n_mc)
    m, kind = est._hip_model(), est._parse_kind
    sd, cfg = state_dict("ff", name, 3), orc.MODEL_CONFIGS[name]
    H, O, layout = m.hidden_layer_size, cfg["O"], cfg["layout"]
    rows = shifted_rows(golden, name, S, frames)
    bank = StreamBank(m, S, est.sequence_len, smooth=1, normalize=True, dtype=torch.float64, monte_carlo_samples=n_mc, dropout=p)
    rng = np.random.default_rng(17)
    worst_y = worst_msg = 0.0
    sd64 = {k: v.astype(np.float64) for k, v in sd.items()}
    for f in range(frames):
        mask = ((rng.random((S * n_mc, H)) >= p) / (1.0 - p)).astype(np.float32)
        md = torch.from_numpy(mask).cuda()
        assert set_masks(bank._handle, C.c_void_p(md.data_ptr())) == 0
        if inputs == "trace":
            bank.push_rows(torch.from_numpy(rows[f]).cuda(), kind)
            feats = est.parse_rows(rows[f]).cpu().numpy()
        else:
            feats = (est._xx_m + est._xx_s * rng.normal(size=(S, cfg["I"]))).astype(np.float32)
            bank.push_features(torch.from_numpy(feats).cuda())
        got = bank.step_datagrams().cpu().numpy().astype(np.float64)
        y = _targets(lib, bank, S * n_mc, O)
        xn = ((feats.astype(np.float64) - est._xx_m) / est._xx_s).astype(np.float32)
        y_ref = orc.ff_forward(sd, np.repeat(xn, n_mc, axis=0), mask=mask)
        ref_err = float(np.abs(y_ref - orc.ff_forward(sd64, np.repeat(xn, n_mc, axis=0), mask=mask)).max())      # the oracle's own f32 error
        err_y = float(np.abs(y - y_ref).max())
        bound = TOL_Y_SHORT if inputs == "in_range" else max(TOL_Y_SHORT, 2.0 * ref_err)
        print(f"ff bank, injected masks, {inputs}, frame {f}: max |z| = {np.abs(xn).max():.1f}, max |y - oracle| = {err_y:.3e}, bound {bound:.3e} "
              f"(oracle f32 vs f64: {ref_err:.3e})")
        assert err_y < bound, (inputs, f, err_y, ref_err)
        worst_y = max(worst_y, err_y)
        pred = y_ref.astype(np.float64) * est._yy_s + est._yy_m
        for s in range(S):
            e = orc.arm_pose_from_targets(pred[s * n_mc:(s + 1) * n_mc], est.body_measurements, layout, "closed")
            ref = np.concatenate([orc.msg_from_est(e, est.body_measurements, layout), e[:, :6].reshape(-1)])
            worst_msg = max(worst_msg, float(np.abs(got[s] - ref).max()))
        assert np.abs(y.reshape(S, n_mc, O)[:, 0] - y.reshape(S, n_mc, O)[:, 1]).max() > 1e-3          # the masks reach the rows
    print(f"ff bank, injected masks, {inputs}: max |y - oracle| = {worst_y:.3e}, max |msg - oracle| = {worst_msg:.3e}")
    assert worst_msg < TOL_MSG_LOOP, worst_msg
    # subset mode keeps its refusal of injected masks
    with pytest.raises(UserWarning, match="injected masks"):
        bank.frame(rows[0][:3], [0, 1, 2], kind)
    assert set_masks(bank._handle, None) == 0
    # an eval bank (no set_mc) has no dropout for the masks to stand in for: refused, not ignored
    ev = StreamBank(m, S, est.sequence_len, smooth=1, normalize=True, dtype=torch.float32)
    assert set_masks(ev._handle, C.c_void_p(md.data_ptr())) == 0
    ev.push_rows(torch.from_numpy(rows[0]).cuda(), kind)
    with pytest.raises(UserWarning, match="injected masks"):
        ev.step_datagrams()
    assert set_masks(ev._handle, None) == 0
    ev.step_datagrams()


def test_ff_bank_philox_masks_match_the_reference_distribution(golden):
    """a Philox bank at p = 0.2: many samples of ONE row against the quantiles the reference drew for DropoutFF.monte_carlo_predictions
    (tests/golden/mc_stats.npz: x_ff, dims_ff) with the check tests/test_hip_round2 applies to the HIP model's own sampler"""
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import nn_models
    from wear_mocap_ape_amd.streams import StreamBank
    lib = _hip.lib()
    g = golden("mc_stats.npz")
    I, H, n_hidden, O = (int(v) for v in g["dims_ff"])
    n_ref = int(g["n_samples"])
    m = nn_models.DropoutFF(output_size=O, hidden_layer_size=H, hidden_layer_count=n_hidden, input_size=I, dropout=0.2, device=0)
    m.load_state_dict(orc.make_ff_state_dict(I, H, n_hidden, O, 0))
    m.set_body(orc.DEFAULT_BODY)
    S, n_mc = 240, 100
    assert S * n_mc == n_ref
    x = torch.from_numpy(np.tile(g["x_ff"].reshape(1, I), (S, 1)).astype(np.float32)).cuda()

    def frames(seed, n):
        bank = StreamBank(m, S, 6, smooth=1, normalize=False, dtype=torch.float64, monte_carlo_samples=n_mc, seed=seed)
        out = []
        for _ in range(n):
            bank.push_features(x)
            bank.step()
            out.append(_targets(lib, bank, S * n_mc, O))
        return out

    a = frames(7, 2)
    for f, y in enumerate(a):
        bad = mc_check.compare(y, g["y_mean_ff"][0], g["y_cov_ff"][0], g["y_quant_ff"][0], g["quantile_levels"], n_ref, what=f"ff bank frame {f}")
        assert not bad, bad
    assert not np.array_equal(a[0], a[1])                    # two frames draw different masks
    assert np.abs(a[0] - a[1]).max() > 1e-3
    b = frames(7, 2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])      # two banks with one seed draw the same ones
    assert not np.array_equal(frames(8, 1)[0], a[0])
    # the samples of one stream differ among themselves and from the next stream's (keyed by stream AND sample)
    y = a[0].reshape(S, n_mc, O)
    assert np.abs(y[0, 0] - y[0, 1]).max() > 1e-4 and not np.array_equal(y[0], y[1])
    # negative control: without the 1/(1-p) scale the means move by tens of standard errors
    assert mc_check.compare(a[0] * 0.8, g["y_mean_ff"][0], g["y_cov_ff"][0], g["y_quant_ff"][0], g["quantile_levels"], n_ref)
