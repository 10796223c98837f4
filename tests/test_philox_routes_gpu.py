"""Every Monte-Carlo route that draws its own numbers, against a float64 reference under the SAME numbers: `oracle/philox.py` computes on the host
what the device must draw (the counters are plain functions of row, step, unit, layer and the call's key: include/ape_hip.h, "Random numbers"),
`hi.forward64` evaluates the recurrence under those masks.  Budget `max(1e-6, 4 e_ref)`, `e_ref = max |float32 oracle - float64 reference|` on
the same case: the rule of tests/test_hostile_inputs_gpu.py, unchanged.  No kernel is another kernel's yardstick here, and no row is skipped:
all rows of every checked call or frame are compared.  The cases, their references and the proof that they can tell a wrong counter scheme
from the right one: tests/philox_cases.py, tests/test_philox_cpu.py.  Every test prints its line (prefix `PHILOX|`); the record is
profiles/philox_replica.md."""
import ctypes as C

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


def _line(what, kernel, err, e_ref):
    bud = pc.budget(e_ref)
    line = f"PHILOX|{what}|{kernel}|err {err:.2e}|e_ref {e_ref:.2e}|budget {bud:.2e}|ratio {err / bud:.2f}"
    print("\n" + line)
    return line, bud


def _lstm_model(norm_stats, name):
    from tests.test_hip_parity import make_model
    m, sd, _ = make_model(name, pc.W_SEED, norm_stats[name])
    want = pc.state_dict(name)
    assert all(np.array_equal(sd[k], want[k]) for k in want)
    m.set_body(orc.DEFAULT_BODY)
    return m


def _ff_model(norm_stats, name=None):
    from wear_mocap_ape_amd.estimate import nn_models
    I, H, n_hidden, O = pc.FF_DIMS
    m = nn_models.DropoutFF(output_size=O, hidden_layer_size=H, hidden_layer_count=n_hidden, input_size=I, dropout=pc.P, device=0)
    m.load_state_dict(orc.make_ff_state_dict(I, H, n_hidden, O, pc.W_SEED))
    if name is not None:
        st = norm_stats[name]
        m.set_norm_stats(st["xx_m"], st["xx_s"], st["yy_m"], st["yy_s"])
        m.set_body(orc.DEFAULT_BODY)
    return m


# ---------------- one call ---------------------------------------------------------------------------------------------------------------
def _call(m, route, inp, kernel=None):
    model, set_kernel, _, T, mseed, last, shared = pc.LSTM_ROUTES[route]
    m.set_kernel(set_kernel if kernel is None else kernel)
    m.manual_seed(mseed)                                     # the call below is Monte-Carlo call 1: key (mseed << 20) + 1
    if shared:                                               # one window, B dropout samples: the z-scores go in as they are
        y = m.monte_carlo_predictions(inp["B"], torch.from_numpy(np.ascontiguousarray(inp["xn"][:1])).cuda(), last_step_only=True)
    else:
        m.lstm.train()
        y = m(torch.from_numpy(inp["x"]).cuda(), last_step_only=True, normalize_input=True)
    y = y.cpu().numpy()[:, 0]
    used = m.last_kernel()
    m.check()
    m.set_kernel("auto")
    return y, used


@pytest.mark.parametrize("route", sorted(pc.LSTM_ROUTES))
def test_lstm_route_draws_the_replicas_masks(norm_stats, route):
    model, set_kernel, _, T, mseed, last, shared = pc.LSTM_ROUTES[route]
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    inp = pc.lstm_inputs(norm_stats, route, n_cus)
    y64, y32 = pc.lstm_reference(inp, with32=True)
    m = _lstm_model(norm_stats, model)
    y, used = _call(m, route, inp)
    assert used == last, (route, used)
    assert y.shape == y64.shape and np.isfinite(y).all()
    line, bud = _line(f"{route}|{model} {inp['B']}x{T}|key {inp['key']:#x}", used, float(np.abs(y - y64).max()), float(np.abs(y32 - y64).max()))
    assert float(np.abs(y - y64).max()) <= bud, line
    if route == "auto-split-pocket":
        # the split really happened: the wave in front holds the batch-tile kernel's bits, the rest does not
        wave = pc.wave_rows(n_cus)
        y16, used16 = _call(m, route, inp, "tile16")
        assert used16 == "ape_lstm_tile16" and np.array_equal(y[:wave], y16[:wave]) and not np.array_equal(y[wave:], y16[wave:])


def test_dropout_ff_draws_the_replicas_mask(norm_stats):
    inp = pc.ff_inputs()
    y64, y32 = pc.ff_reference(inp, with32=True)
    m = _ff_model(norm_stats).set_kernel("tile16")            # the tile kernel, the only one with the dropout
    m.manual_seed(pc.FF_MC[1])
    y = m.monte_carlo_predictions(inp["n"], torch.from_numpy(inp["x"]).cuda(), last_step_only=True).cpu().numpy()[:, 0]
    m.check()
    assert y.shape == y64.shape
    line, bud = _line(f"DropoutFF mc {inp['n']}|pocket_like|key {inp['key']:#x}", "ape_mlp_tile16", float(np.abs(y - y64).max()),
                      float(np.abs(y32 - y64).max()))
    assert float(np.abs(y - y64).max()) <= bud, line


# ---------------- bank frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bank_id", sorted(pc.BANKS))
def test_bank_frames_draw_the_replicas_masks(norm_stats, bank_id):
    """T + 2 lockstep frames with one reset() in between: frame f is keyed seed + f whatever the reset did; rows stream * n_mc + sample"""
    from wear_mocap_ape_amd.streams import StreamBank
    reg, name, S, n_mc, smooth, seed, T, F = pc.bank_dims(bank_id)
    kernel, last = pc.BANKS[bank_id][6:8]
    m = _ff_model(norm_stats, name) if reg == "ff" else _lstm_model(norm_stats, name)
    bank = StreamBank(m, S, T, smooth=smooth, normalize=True, dtype=torch.float64, monte_carlo_samples=n_mc, dropout=pc.P, seed=seed)
    if kernel != "auto":
        m.set_kernel(kernel)                                 # behind the bank's plan: the shared-layer-0 step on the batch-tile kernel
    feats = pc.bank_features(norm_stats, bank_id)
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
    ref = pc.bank_reference(norm_stats, bank_id, with32=True)
    err = max(pc.quantity_error(got[f], ref[f][0]) for f in checked)
    e_ref = max(pc.quantity_error(ref[f][1], ref[f][0]) for f in checked)
    assert all(got[f][0].shape == ref[f][0][0].shape and got[f][1].shape == ref[f][0][1].shape for f in checked)
    line, bud = _line(f"bank {bank_id}|{name} S={S} n_mc={n_mc} smooth={smooth}|seed {seed:#x}|frames {checked[0]}..{checked[-1]} of {F}, reset "
                      f"before {pc.RESET_AT}", last, err, e_ref)
    assert err <= bud, line


# ---------------- subset frame -----------------------------------------------------------------------------------------------------------
def _device_features(rows):
    from wear_mocap_ape_amd import _hip
    rd = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    xx = torch.empty((rows.shape[0], 22), dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().ape_parse_rows(_hip.PARSE_WATCH_PHONE_POCKET, C.c_void_p(rd.data_ptr()), rows.shape[0], C.c_void_p(xx.data_ptr()),
                                         _hip.F32, None), "ape_parse_rows")
    torch.cuda.synchronize()
    return xx.cpu().numpy()


def test_subset_frame_draws_by_list_position_under_the_banks_call_counter(golden, norm_stats):
    from tests.test_streams_subset import _frame_c
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.streams import StreamBank
    q = pc.SUBSET
    S, n_mc, smooth, listed = q["S"], q["n_mc"], q["smooth"], q["listed"]
    T = orc.MODEL_CONFIGS[q["model"]]["T"]
    m = _lstm_model(norm_stats, q["model"])
    bank = StreamBank(m, S, T, smooth=smooth, normalize=True, dtype=torch.float64, monte_carlo_samples=n_mc, dropout=pc.P, seed=q["seed"])
    rows = pc.trace_rows(golden, 3 * S, 5).reshape(3, S, -1)
    kind = _hip.PARSE_WATCH_PHONE_POCKET
    kernels = set()
    for f in range(2):
        bank.push_rows(torch.from_numpy(np.ascontiguousarray(rows[f])).cuda(), kind)
        bank.step()
        kernels.add(m.last_kernel())
    bank.reset(streams=q["reset"])
    out = _frame_c(bank, kind, torch.from_numpy(np.ascontiguousarray(rows[2][listed])).cuda(), listed,
                   _hip.FLAG_NORMALIZE_INPUT | _hip.FLAG_PACKED_MSG, torch.float64).cpu().numpy()
    kernels.add(m.last_kernel())
    m.check()
    assert kernels == {"ape_lstm_cluster"}, kernels
    K, N = len(listed), smooth * n_mc
    assert out.shape == (K, 25 + 6 * N)
    got = (out[:, 25:].reshape(K, N, 6), out[:, :25])
    feats = _device_features(rows.reshape(3 * S, -1)).reshape(3, S, -1)
    r64, r32 = pc.subset_reference(norm_stats, feats, with32=True)
    line, bud = _line(f"subset frame|pocket S={S}, K={K} listed {listed} after 2 lockstep frames and reset of {q['reset']}|seed {q['seed']:#x}",
                      "ape_lstm_cluster", pc.quantity_error(got, r64), pc.quantity_error(r32, r64))
    assert pc.quantity_error(got, r64) <= bud, line


# ---------------- replay -------------------------------------------------------------------------------------------------------------------
def test_replay_draws_the_masks_of_one_call_whole_and_in_two_resumed_pieces(golden, tmp_path, monkeypatch):
    from tests.test_replay import _estimator
    q = pc.REPLAY
    F, n_mc, cut, seed = q["F"], q["n_mc"], q["cut"], q["seed"]
    est = _estimator(tmp_path, monkeypatch, q["model"], pc.W_SEED, pc.P, smooth=q["smooth"], add_mc_samples=True, monte_carlo_samples=n_mc)
    model = est._hip_model()
    rows = pc.trace_rows(golden, F, 6)
    feats = est.parse_rows(rows).cpu().numpy().astype(np.float32)
    stats = {"xx_m": est._xx_m, "xx_s": est._xx_s, "yy_m": est._yy_m, "yy_s": est._yy_s}
    y64, y32 = pc.replay_reference(stats, feats, with32=True)
    e_ref = float(np.abs(y32 - y64).max())
    _, y = est.process_recording(rows, return_targets=True, seed=seed)
    used = model.last_kernel()
    y = y.cpu().numpy().reshape(F * n_mc, -1)
    _, ya, (state, warm) = est.process_recording(rows[:cut], return_targets=True, return_state=True, seed=seed)
    _, yb = est.process_recording(rows[cut:], return_targets=True, seed=seed, state_in=state, warm_in=warm, sample_row_base=cut * n_mc)
    pieces = np.concatenate([ya.cpu().numpy().reshape(cut * n_mc, -1), yb.cpu().numpy().reshape((F - cut) * n_mc, -1)])
    assert used == model.last_kernel() == "ape_lstm_cluster"
    for what, got in (("one call", y), (f"two pieces, sample_row_base {cut * n_mc}", pieces)):
        assert got.shape == y64.shape
        line, bud = _line(f"replay {what}|pocket F={F} n_mc={n_mc}|seed {seed:#x}", used, float(np.abs(got - y64).max()), e_ref)
        assert float(np.abs(got - y64).max()) <= bud, line
