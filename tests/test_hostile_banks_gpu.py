"""The Monte-Carlo stream banks under their OWN draws at hostile magnitudes: the bank kernels whose Philox masks cannot be injected
(`ape_lstm_upper32`, `ape_lstm_upper128`, the latency kernel, the fused first-generation step, the shared-layer-0 step on the batch-tile
kernel, the DropoutFF bank head) held to float64 at trained weight magnitudes, saturated hidden states and z-scores up to 1e3.

`oracle/philox.py` computes on the host the masks the kernels draw, so the reference is `hi.forward64` (DropoutFF: the float64 evaluation of
tests/philox_cases.py) under those masks, on the cases of tests/test_hostile_inputs_cpu.py (`pc.BANK_CASES`; the DropoutFF bank on `w16` /
`sat30` / `z1e3` of tests/ff_cases.py).  Frame schedule, compared quantity and budget are those of
tests/test_philox_routes_gpu.py::test_bank_frames_draw_the_replicas_masks: T + 2 lockstep frames with one reset, every sample row's tail and
every stream's message through the oracle's float64 FK, `max(1e-6, 4 e_ref)` with e_ref the float32 oracle's distance on that quantity
under the same masks.  The proof that each case still tells a wrong counter reading from the right one: tests/test_philox_cpu.py.
Every test prints its line (prefix `HOSTILE|D|`); the record is profiles/hostile_inputs.md."""
import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests import philox_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def _model(norm_stats, reg, name, case):
    from wear_mocap_ape_amd.estimate import nn_models
    c, st = orc.MODEL_CONFIGS[name], norm_stats[name]
    if reg == "ff":
        m = nn_models.DropoutFF(output_size=c["O"], hidden_layer_size=256, hidden_layer_count=2, input_size=c["I"], dropout=pc.P, device=0)
    else:
        m = nn_models.DropoutLSTM(c["I"], c["H"], c["L"], c["O"], dropout=pc.P, device=0)
    m.load_state_dict(pc.bank_state_dict(reg, name, case))
    m.set_norm_stats(st["xx_m"], st["xx_s"], st["yy_m"], st["yy_s"])
    m.set_body(orc.DEFAULT_BODY)
    return m


@pytest.mark.parametrize("case", pc.BANK_CASES)
@pytest.mark.parametrize("bank_id", sorted(pc.BANKS))
def test_bank_under_its_own_draws_against_the_float64_reference(norm_stats, bank_id, case):
    from wear_mocap_ape_amd.streams import StreamBank
    reg, name, S, n_mc, smooth, seed, T, F = pc.bank_dims(bank_id)
    kernel, last = pc.BANKS[bank_id][6:8]
    m = _model(norm_stats, reg, name, case)
    bank = StreamBank(m, S, T, smooth=smooth, normalize=True, dtype=torch.float64, monte_carlo_samples=n_mc, dropout=pc.P, seed=seed)
    if kernel != "auto":
        m.set_kernel(kernel)                                 # behind the bank's plan: the shared-layer-0 step on the batch-tile kernel
    feats = pc.bank_features(norm_stats, bank_id, case)
    checked = pc.bank_checked_frames(bank_id)
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
    m.set_kernel("auto")
    assert kernels == {last}, kernels
    ref = pc.bank_reference(norm_stats, bank_id, with32=True, case=case)
    assert all(np.isfinite(q).all() for f in checked for q in ref[f][0])
    assert all(got[f][0].shape == ref[f][0][0].shape and got[f][1].shape == ref[f][0][1].shape for f in checked)
    assert all(np.isfinite(q).all() for f in checked for q in got[f])
    err = max(pc.quantity_error(got[f], ref[f][0]) for f in checked)
    e_ref = max(pc.quantity_error(ref[f][1], ref[f][0]) for f in checked)
    bud = pc.budget(e_ref)
    what = pc.FF_BANK_CASE[case] if reg == "ff" else case
    line = (f"HOSTILE|D|{bank_id}|{last}|{name} S={S} n_mc={n_mc} smooth={smooth}|{what}|frames {checked[0]}..{checked[-1]} of {F}|"
            f"e_ref {e_ref:.2e}|err {err:.2e}|budget {bud:.2e}|ratio {err / bud:.2f}")
    print("\n" + line)
    assert err <= bud, line


# ---------------- the bank head's two-tile form ------------------------------------------------------------------------------------------
# `ape_ff_bank_head<2>` serves more than 16 outputs; the deployed DropoutFF has 14.  The 20-target layout (hand and elbow positions beside
# the orientations) is the one configuration of a bank that reaches it: 22 -> 2 x 256 -> 20 on the pocket features, targets de-normalised
# with statistics of its own
WIDE_HEAD = dict(I=22, H=256, n_hidden=2, O=20, layout=2, S=7, n_mc=25, T=6, seed=0x6_0000_0011)


def wide_head_case(norm_stats, case, variant=None):
    """-> (state dict, stats, features float32 [F, S, I], {frame: [(tail, msg) float64 reference, (tail, msg) float32 oracle]});
    `variant`: a wrong reading of the counter contract (tests/test_philox_cpu.py), default the contract"""
    from oracle import philox as ph
    from tests import ff_cases as fc
    from tests import test_hostile_inputs_cpu as hi
    q = WIDE_HEAD
    I, H, O, S, n_mc, F = q["I"], q["H"], q["O"], q["S"], q["n_mc"], q["T"] + 2
    s = np.float32(fc.CASE_WSCALE[pc.FF_BANK_CASE[case]])
    sd = {k: v if k.startswith("_output_layer.") else (v * s).astype(np.float32)
          for k, v in orc.make_ff_state_dict(I, H, q["n_hidden"], O, pc.W_SEED).items()}
    st = dict(xx_m=norm_stats["pocket"]["xx_m"], xx_s=norm_stats["pocket"]["xx_s"], yy_m=0.1 * np.arange(O) - 1.0, yy_s=1.0 + 0.05 * np.arange(O))
    x = st["xx_m"] + st["xx_s"] * hi.case_z(case, F, S, I, 2000 + S)
    x[..., 0] = 0.02
    feats = x.astype(np.float32)
    ref = {}
    for f in range(F):                                       # a DropoutFF reads the newest row only; smooth = 1: frame f is call f alone
        xn = ((feats[f].astype(np.float64) - st["xx_m"]) / st["xx_s"]).astype(np.float32)
        xr = np.repeat(xn, n_mc, axis=0)
        mask = ph.ff_bank_mask(ph.bank_call_seed(q["seed"], f), S * n_mc, H, pc.P, v=ph.CONTRACT if variant is None else variant)
        ref[f] = []
        for y in (fc.ff_forward64(sd, xr, mask), orc.ff_forward(sd, xr, mask=mask)):
            stacks = (y.astype(np.float64) * st["yy_s"] + st["yy_m"]).reshape(S, n_mc, O)
            ests = [orc.arm_pose_from_targets(rows, orc.DEFAULT_BODY, q["layout"], "eigh") for rows in stacks]
            ref[f].append((np.array([e[:, :6] for e in ests]), np.array([orc.msg_from_est(e, orc.DEFAULT_BODY, q["layout"]) for e in ests])))
    return sd, st, feats, ref


@pytest.mark.parametrize("case", pc.BANK_CASES)
def test_ff_bank_head_with_more_than_sixteen_outputs(norm_stats, case):
    from wear_mocap_ape_amd.estimate import nn_models
    from wear_mocap_ape_amd.streams import StreamBank
    q = WIDE_HEAD
    sd, st, feats, ref = wide_head_case(norm_stats, case)
    m = nn_models.DropoutFF(output_size=q["O"], hidden_layer_size=q["H"], hidden_layer_count=q["n_hidden"], input_size=q["I"], dropout=pc.P, device=0)
    assert m.target_layout == q["layout"]
    m.load_state_dict(sd)
    m.set_norm_stats(st["xx_m"], st["xx_s"], st["yy_m"], st["yy_s"])
    m.set_body(orc.DEFAULT_BODY)
    bank = StreamBank(m, q["S"], q["T"], smooth=1, normalize=True, dtype=torch.float64, monte_carlo_samples=q["n_mc"], dropout=pc.P, seed=q["seed"])
    got = {}
    for f in range(q["T"] + 2):
        if f == pc.RESET_AT:
            bank.reset()
        bank.push_features(torch.from_numpy(np.ascontiguousarray(feats[f])).cuda())
        msg, tail = bank.step(with_tail=True)
        assert m.last_kernel() == "ape_ff_bank_head"
        got[f] = (tail.cpu().numpy().copy(), msg.cpu().numpy().copy())
    m.check()
    assert all(np.isfinite(a).all() for f in ref for a in ref[f][0])
    assert all(got[f][0].shape == ref[f][0][0].shape and got[f][1].shape == ref[f][0][1].shape and np.isfinite(got[f][0]).all() for f in ref)
    err = max(pc.quantity_error(got[f], ref[f][0]) for f in ref)
    e_ref = max(pc.quantity_error(ref[f][1], ref[f][0]) for f in ref)
    bud = pc.budget(e_ref)
    line = (f"HOSTILE|D|ff-wide-head-7x25|ape_ff_bank_head|22-256-256-256-20 S={q['S']} n_mc={q['n_mc']} smooth=1|{pc.FF_BANK_CASE[case]}|"
            f"frames 0..{q['T'] + 1} of {q['T'] + 2}|e_ref {e_ref:.2e}|err {err:.2e}|budget {bud:.2e}|ratio {err / bud:.2f}")
    print("\n" + line)
    assert err <= bud, line
