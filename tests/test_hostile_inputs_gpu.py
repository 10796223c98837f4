"""Hostile inputs on every LSTM route, and a bad stream that stays in its own slot (the CPU half: tests/test_hostile_inputs_cpu.py).

Part A: every route of the dispatch at trained weight magnitudes, saturated hidden states and z-scores up to 1e3, against a plain float64
        evaluation of the recurrence.  Budget of a float32 route: max(1e-6, 4 * e_ref), e_ref = max |orc.lstm_forward - float64 reference| on
        the same case -- the pinned float32 oracle's own rounding error, with a factor 4 for another summation order and two ~1-ulp hardware
        transcendentals per gate.  Budget of a binary16 route: 2 * e16, e16 = max |binary16-storage emulation - float64 reference|, and the
        documented 1.2e-5 from the emulation on the benign control.  No kernel's error is anybody's yardstick.
Part B: one NaN / one +Inf in one window: every other window keeps its bits, `check()` stays clean.
Part C: twin banks, one NaN sensor value in one stream of one of them: every other stream keeps its bits on every frame, the bad stream is
        non-finite for exactly `poisoned_frames(T, smooth)` frames and bit-equal to its twin from the next frame on.
Measured figures: profiles/hostile_inputs.md (every test prints its line, prefix `HOSTILE|`)."""
import numpy as np
import pytest
import torch

from oracle import ape_oracle as orc
from tests import test_hostile_inputs_cpu as hi
from tests.test_c32_split_gpu import _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


# route id: (model, set_kernel, set_precision, B, T, kernel_name(B, T) must contain, last_kernel() must equal, extras)
#   `kernel_name` describes eval-mode batches; it cannot name the Monte-Carlo latency kernel (None: `last_kernel()` alone pins that route)
#   extras: "masks" = injected dropout masks, "rows" = one window shared by B sample rows (monte_carlo_predictions' broadcast)
# shapes: the smallest with two row tiles / clusters and a ragged last one; cluster32 just above its 512-row threshold
ROUTES = {
    "tile16-pocket": ("pocket", "tile16", "f32", 37, 6, "tile16", "ape_lstm_tile16", ()),
    "tile16-watch": ("watch", "tile16", "f32", 37, 8, "tile16", "ape_lstm_tile16", ()),
    "tile16-uarm": ("uarm", "tile16", "f32", 37, 6, "tile16", "ape_lstm_tile16", ()),
    "cluster_gen1": ("pocket", "cluster_gen1", "f32", 77, 6, "ape_lstm_cluster<", "ape_lstm_cluster", ()),
    "cluster-le512": ("watch", "cluster", "f32", 45, 8, "ape_lstm_cluster<", "ape_lstm_cluster", ()),
    "cluster32-short": ("pocket", "cluster", "f32", 513, 6, "ape_lstm_cluster32<256, 2, 32, true>", "ape_lstm_cluster32", ()),
    "cluster32-long": ("pocket", "cluster", "f32", 513, 9, "ape_lstm_cluster32<256, 2, 32, false>", "ape_lstm_cluster32", ()),
    "cluster16": ("uarm", "cluster", "f32", 513, 49, "ape_lstm_cluster16<128, 3, 64, 2>", "ape_lstm_cluster16", ()),
    "level16-T6": ("uarm", "auto", "f32", 530, 6, "ape_lstm_level16<128, 3, 64>", "ape_lstm_level16", ()),
    "level16-T48": ("uarm", "auto", "f32", 37, 48, "ape_lstm_level16<128, 3, 64>", "ape_lstm_level16", ()),
    "cluster_small": ("pocket", "auto", "f32", 3, 6, "ape_lstm_cluster<", "ape_lstm_cluster_small", ()),
    "mc_small-masks": ("pocket", "auto", "f32", 25, 6, None, "ape_lstm_mc_small", ("masks", "rows")),
    "cluster_gen1-masks": ("uarm", "cluster_gen1", "f32", 45, 6, "ape_lstm_cluster<", "ape_lstm_cluster", ("masks",)),
    "f16": ("watch", "auto", "f16", 289, 8, "ape_lstm_cluster_f16v2", "ape_lstm_cluster_f16v2", ()),
    "f16_gen1": ("pocket", "auto", "f16_gen1", 45, 6, "ape_lstm_cluster_f16", "ape_lstm_cluster_f16", ()),
    "imupose": ("imupose", "auto", "f32", 45, 6, "ape_lstm_cluster<256, 2, 256", "ape_lstm_cluster", ()),
    "imupose-upper32": ("imupose", "auto", "f32", 513, 5, "ape_lstm_upper32<32, true>", "ape_lstm_upper32", ()),
    "one_22_256": ("one_22_256", "auto", "f32", 37, 6, "tile16", "ape_lstm_tile16", ()),
    "one_32_256": ("one_32_256", "auto", "f32", 37, 6, "tile16", "ape_lstm_tile16", ()),
    "one_38_128": ("one_38_128", "auto", "f32", 37, 6, "tile16", "ape_lstm_tile16", ()),
    "one_64_128": ("one_64_128", "auto", "f32", 37, 6, "tile16", "ape_lstm_tile16", ()),
}
SEED_X = 21
# part A: every route on every case, and the routes with long windows on the conditioned long-window case as well (hi.LONG_SCALE)
ROUTE_CASES = [(r, c) for r in sorted(ROUTES) for c in hi.CASES + ((hi.LONG_CASE,) if ROUTES[r][4] >= hi.LONG_T else ())]
_CASES = {}


def _mid_row(B):
    """a window in the MIDDLE of its row tile, whatever the route's tile (16 or 32 rows): row 24 of a 32-row tile = row 8 of a 16-row one"""
    return (B // 2) // 32 * 32 + 24 if B >= 64 else 24 if B > 24 else 1


def _stats(norm_stats, model):
    return norm_stats[model if model in orc.MODEL_CONFIGS else "pocket"] if hi.has_stats(model) else None


def _build(norm_stats, model, wscale):
    """the HIP model of a route with its `lstm.*` tensors scaled, and the very state dict the CPU file's references take"""
    from wear_mocap_ape_amd.estimate import nn_models
    sd = hi.state_dict(model, wscale)
    st = _stats(norm_stats, model)
    if model in orc.MODEL_CONFIGS:
        m, sd_m, _ = _model(model, st, wscale, hi.SEED_W)
        assert all(np.array_equal(sd[k], sd_m[k]) for k in sd)
        return m, sd, st
    I, H, L, O = hi.dims_of(model)
    m = nn_models.ImuPoseLSTM(I, H, L, O, device=0) if model == "imupose" else nn_models.DropoutLSTM(I, H, L, O, dropout=0.2, device=0)
    m.load_state_dict(sd)
    if st is not None:
        m.set_norm_stats(st["xx_m"], st["xx_s"], st["yy_m"], st["yy_s"])
    return m, sd, st


def _masks(model, B, T):
    _, H, L, _ = hi.dims_of(model)
    rng = np.random.default_rng(9)
    return [(rng.random((B, T, H)) >= 0.2).astype(np.float32) / np.float32(0.8) for _ in range(L - 1)]


def _launch(route, m, x, masks=None):
    """one call on the route, the launched kernel asserted -> y [B,O] of the last step"""
    model, kernel, precision, B, T, want_name, want_last, extras = ROUTES[route]
    m.set_kernel(kernel)
    m.set_precision(precision)
    assert want_name is None or want_name in m.kernel_name(B, T), (route, m.kernel_name(B, T))
    kw = dict(last_step_only=True, normalize_input=hi.has_stats(model))
    if masks is not None:
        kw["masks"] = torch.from_numpy(np.stack(masks)).cuda()
    if "rows" in extras:
        kw["rows"] = B
    y = m(torch.from_numpy(np.ascontiguousarray(x)).cuda(), **kw).cpu().numpy()[:, 0]
    assert m.last_kernel() == want_last, (route, m.last_kernel())
    m.check()
    m.set_precision("f32")
    m.set_kernel("auto")
    return y


def _case(norm_stats, route, case):
    """inputs and CPU references of one (route, case), computed once: raw x, float32 inputs xn, masks, y64, yardstick, emulation"""
    if (route, case) not in _CASES:
        _CASES[route, case] = _make_case(norm_stats, route, case)
    return _CASES[route, case]


def _make_case(norm_stats, route, case):
    model, kernel, precision, B, T, _, _, extras = ROUTES[route]
    st = _stats(norm_stats, model)
    I = hi.dims_of(model)[0]
    f16 = precision != "f32"
    nb = 1 if "rows" in extras else B
    z = hi.case_z(case, nb, T, I, SEED_X, zmax=1e2 if f16 else 1e3)
    x, xn = hi.raw_and_normalised(st, z) if st is not None else (z.astype(np.float32),) * 2
    sd = hi.state_dict(model, hi.wscale_of(model, case))
    masks = _masks(model, B, T) if "masks" in extras else None
    xr = np.repeat(xn, B, axis=0) if "rows" in extras else xn
    y64 = hi.forward64(model, sd, xr, masks)[:, -1]
    y_emu = hi.forward32(model, sd, xr, masks, storage="f16")[:, -1] if f16 else None
    yard = float(np.abs((y_emu if f16 else hi.forward32(model, sd, xr, masks)[:, -1]) - y64).max())
    return x, xn, masks, y64, yard, y_emu


# ---------------- part A ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,case", ROUTE_CASES)
def test_route_against_the_float64_reference(norm_stats, route, case):
    """(on windows of 48 steps and more the `trained` row at x 16 is a record: the float32 oracle itself is ~1 from float64 there, its budget holds
    nothing; those routes are held by the `trained_long` row, conditioned on the CPU by test_the_long_case_is_conditioned)"""
    model, kernel, precision, B, T, want_name, want_last, extras = ROUTES[route]
    f16 = precision != "f32"
    x, xn, masks, y64, yard, y_emu = _case(norm_stats, route, case)
    m, sd, st = _build(norm_stats, model, hi.wscale_of(model, case))
    y = _launch(route, m, x, masks)
    assert y.shape == y64.shape and np.isfinite(y).all()
    e = float(np.abs(y - y64).max())
    budget = 2.0 * yard if f16 else max(1e-6, 4.0 * yard)
    line = f"HOSTILE|A|{route}|{want_last}|{model} {B}x{T}|{case}|{'e16' if f16 else 'e_ref'} {yard:.2e}|err {e:.2e}|budget {budget:.2e}"
    if f16:
        e_emu = float(np.abs(y - y_emu).max())
        line += f"|vs emulation {e_emu:.2e}"
    print("\n" + line)
    assert e <= budget, line
    if f16 and case == "benign":
        assert e_emu <= 1.2e-5, line
    if f16 and case == "z1e3":
        # one z-score beyond binary16's 65504: its own window may be anything the format makes of it, every other window keeps its bits
        bad = _mid_row(B)
        x2 = x.copy()
        x2[bad, T // 2, 3] = np.float32(st["xx_m"][3] + st["xx_s"][3] * 7.0e4)
        y2 = _launch(route, m, x2)
        xn2 = ((x2.astype(np.float64) - st["xx_m"]) / st["xx_s"]).astype(np.float32)
        with np.errstate(all="ignore"):
            emu2 = hi.forward32(model, sd, xn2[bad:bad + 1], storage="f16")[0, -1]
        rest = np.arange(B) != bad
        assert np.array_equal(y2[rest], y[rest])
        own = "non-finite" if not np.isfinite(y2[bad]).any() else f"vs emulation {float(np.abs(y2[bad] - emu2).max()):.2e}"
        print(f"HOSTILE|A|{route}|{want_last}|{model} {B}x{T}|z beyond 65504|own window {own}|others bit-equal")
        assert not np.isfinite(y2[bad]).any() or float(np.abs(y2[bad] - emu2).max()) <= 1.2e-5


# ---------------- part B ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_a_non_finite_window_stays_in_its_window(norm_stats, route):
    """benign windows, then one NaN (and separately one +Inf) at a middle step of (a) a window in the middle of a tile, (b) the last valid
    row of the ragged last tile, beside the padding rows the buffer descriptors read as zero.  No tolerances: the other windows are
    bit-equal to the clean run.  A NaN window is non-finite in every output.  A +Inf feature saturates layer 0's gates at exactly 0 / 1 /
    +-1 in the mathematics (sigmoid(+-inf), tanh(+-inf)), so the float64 reference of that window is FINITE: the window must then be
    non-finite throughout or agree with the reference within the route's part-A budget -- anything else is garbage.
    The route on one shared window (`rows`) has no second window: there the NaN reaches every sample row, and the next clean call is clean."""
    model, kernel, precision, B, T, want_name, want_last, extras = ROUTES[route]
    f16 = precision != "f32"
    x, xn, masks, y64, yard, y_emu = _case(norm_stats, route, "benign")
    m, sd, st = _build(norm_stats, model, 1.0)
    y_clean = _launch(route, m, x, masks)
    assert np.isfinite(y_clean).all()
    if "rows" in extras:
        xb = x.copy()
        xb[0, T // 2, 3] = np.nan
        assert not np.isfinite(_launch(route, m, xb, masks)).any()
        assert np.array_equal(_launch(route, m, x, masks), y_clean)
        print(f"\nHOSTILE|B|{route}|{want_last}|{model} {B}x{T}|NaN in the shared window: all {B} rows non-finite, next clean call bit-equal")
        return
    notes = []
    for bad in (_mid_row(B), B - 1):
        rest = np.arange(B) != bad
        for val in (np.nan, np.inf):
            xb = x.copy()
            xb[bad, T // 2, 3] = val
            y = _launch(route, m, xb, masks)
            assert np.array_equal(y[rest], y_clean[rest]), (route, bad, val)
            if np.isnan(val):
                assert not np.isfinite(y[bad]).any(), (route, bad, y[bad])
                continue
            xnb = xb[bad:bad + 1] if st is None else ((xb[bad:bad + 1].astype(np.float64) - st["xx_m"]) / st["xx_s"]).astype(np.float32)
            mk = None if masks is None else [k[bad:bad + 1] for k in masks]
            with np.errstate(all="ignore"):
                r64 = hi.forward64(model, sd, xnb, mk)[0, -1]
                r32 = hi.forward32(model, sd, xnb, mk, storage="f16" if f16 else None)[0, -1]
            if not np.isfinite(r64).all():
                assert not np.isfinite(y[bad]).any(), (route, bad, y[bad])
                notes.append(f"row {bad} +Inf: reference non-finite, window non-finite")
            elif not np.isfinite(y[bad]).any():
                notes.append(f"row {bad} +Inf: window non-finite")
            else:
                e, e_y = float(np.abs(y[bad] - r64).max()), float(np.abs(r32 - r64).max())
                notes.append(f"row {bad} +Inf: finite like the reference, err {e:.2e} (yardstick {e_y:.2e})")
                if f16:         # part A's two bounds: twice the storage format's own error, or the documented 1.2e-5 from the emulation
                    e_emu = float(np.abs(y[bad] - r32).max())
                    notes[-1] += f", vs emulation {e_emu:.2e}"
                    assert e <= 2.0 * e_y or e_emu <= 1.2e-5, (route, bad, e, e_y, e_emu)
                else:
                    assert e <= max(1e-6, 4.0 * e_y), (route, bad, e, e_y)
    assert np.array_equal(_launch(route, m, x, masks), y_clean)
    print(f"\nHOSTILE|B|{route}|{want_last}|{model} {B}x{T}|NaN windows non-finite, others bit-equal|" + "; ".join(notes))


# ---------------- part C: twin stream banks -----------------------------------------------------------------------------------------------
def _bank_rows(golden, name, S, frames):
    from tests.test_regressor_banks_gpu import shifted_rows
    return shifted_rows(golden, name, S, frames)


def _bank_model(norm_stats, kind, name):
    """-> (model with stats and body, T_eff: the frames a row stays in what the regressor reads)"""
    from wear_mocap_ape_amd.estimate import nn_models
    st, cfg = norm_stats[name], orc.MODEL_CONFIGS[name]
    if kind == "lstm":
        m = _model(name, st)[0]
        t_eff = cfg["T"]
    elif kind == "ff":
        m = nn_models.DropoutFF(output_size=cfg["O"], hidden_layer_size=256, hidden_layer_count=2, input_size=cfg["I"], dropout=0.2, device=0)
        m.load_state_dict(orc.make_ff_state_dict(cfg["I"], 256, 2, cfg["O"], 3))
        t_eff = 1                        # a row-wise MLP on the newest row (StreamBank's docstring)
    else:
        m = nn_models.ImuPoseLSTM(cfg["I"], 256, 2, cfg["O"], device=0)
        m.load_state_dict(orc.make_imupose_state_dict(cfg["I"], cfg["O"], 3))
        t_eff = cfg["T"]
    if kind != "lstm":
        m.set_norm_stats(st["xx_m"], st["xx_s"], st["yy_m"], st["yy_s"])
    m.set_body(orc.DEFAULT_BODY)
    return m, t_eff


# bank id: (regressor, model, S, smooth, n_mc, bad stream, frame mode, spread flag, kernel the step must launch, post form)
BANKS = {
    "wide-lane0-of-wg1": ("lstm", "pocket", 65, 1, None, 64, "lockstep", False, None, "wide"),
    "wide-lane63-of-wg0": ("lstm", "pocket", 65, 1, None, 63, "lockstep", False, None, "wide"),
    "mc_small": ("lstm", "pocket", 2, 1, 25, 1, "lockstep", True, "ape_lstm_mc_small", None),
    "upper32": ("lstm", "pocket", 170, 1, 25, 85, "lockstep", True, "ape_lstm_upper32", None),
    "upper128": ("lstm", "uarm", 100, 1, 50, 50, "lockstep", True, "ape_lstm_upper128", None),
    "split-post-N130": ("lstm", "pocket", 3, 5, 26, 1, "lockstep", True, None, "split"),
    "dropout_ff": ("ff", "pocket", 37, 3, 3, 18, "lockstep", False, None, None),
    "imupose": ("imupose", "pocket", 37, 3, None, 18, "lockstep", False, None, None),
    "subset": ("lstm", "watch", 21, 2, None, 9, "subset", False, None, None),
    "subset-mc": ("lstm", "pocket", 5, 2, 4, 2, "subset", True, None, None),
    "host-subset": ("lstm", "pocket", 21, 2, None, 9, "host", False, None, None),
    "host-tick": ("lstm", "pocket", 21, 2, None, 9, "tick", False, None, None),
}


@pytest.mark.parametrize("bank_id", sorted(BANKS))
def test_a_bad_stream_stays_in_its_slot_and_recovers(golden, norm_stats, bank_id):
    from wear_mocap_ape_amd import _hip, streams
    from wear_mocap_ape_amd.data_types import messaging
    reg, name, S, smooth, n_mc, s_bad, mode, spread, want_kernel, want_form = BANKS[bank_id]
    m, t_eff = _bank_model(norm_stats, reg, name)
    T = orc.MODEL_CONFIGS[name]["T"]
    kind = {"pocket": _hip.PARSE_WATCH_PHONE_POCKET, "watch": _hip.PARSE_WATCH_ONLY, "uarm": _hip.PARSE_WATCH_PHONE_UARM}[name]
    col = (messaging.WATCH_ONLY_IMU_LOOKUP if name == "watch" else messaging.WATCH_PHONE_IMU_LOOKUP)["sw_gyro_x"]
    n_bad = hi.poisoned_frames(t_eff, smooth)
    f_bad = T + 1                                                    # the bad stream's own frame count at the bad row: past its cold start
    own_frames = f_bad + n_bad + 3
    # subset modes: the bad stream listed first on its bad frame, last on every other frame, and not at all on the tick after the bad one
    ticks = own_frames + (1 if mode != "lockstep" else 0)
    rows = _bank_rows(golden, name, S, ticks)
    others = [s for s in range(S) if s != s_bad]

    def lists(t):
        if mode == "lockstep":
            return list(range(S))
        if t == f_bad:
            return [s_bad] + others
        if t == f_bad + 1:
            return others
        return others[t % 3:] + others[:t % 3] + [s_bad]

    def run(poison):
        bank = streams.StreamBank(m, S, T, smooth=smooth, normalize=True, dtype=torch.float32, monte_carlo_samples=n_mc, dropout=0.2, seed=77)
        out, forms, kernels = [], set(), set()
        for t in range(ticks):
            ids = lists(t)
            r = rows[t][ids].copy()
            if poison and t == f_bad:
                r[ids.index(s_bad), col] = np.nan
            if mode == "lockstep":
                bank.push_rows(torch.from_numpy(r).cuda(), kind)
                got = bank.step(with_tail=True, with_spread=True) if spread else bank.step(with_tail=True)
                got = np.concatenate([g.cpu().numpy().reshape(S, -1) for g in got], axis=1)
            elif mode == "subset":
                got = bank.frame(r, ids, kind, datagrams=True, spread=spread).cpu().numpy().copy()
            elif mode == "host":
                got = bank.frame_host(r, ids, kind, datagrams=True, spread=spread)
            else:
                got = streams.tick(bank, r, np.asarray(ids), kind=kind, datagrams=True, spread=spread)
            bank.recover()
            forms.add(bank.last_post_form())
            kernels.add(m.last_kernel())
            out.append({s: got[j] for j, s in enumerate(ids)})
        m.check()
        return out, forms, kernels

    a, forms, kernels = run(True)
    b, forms_b, kernels_b = run(False)
    assert forms == forms_b and kernels == kernels_b
    if want_kernel is not None:
        assert kernels == {want_kernel}, kernels
    if want_form is not None:
        assert len(forms) == 1 and next(iter(forms)).startswith(want_form), forms
    own, bad_seen = 0, []
    for t in range(ticks):
        assert a[t].keys() == b[t].keys()
        for s in a[t]:
            if s != s_bad:
                assert np.array_equal(a[t][s], b[t][s]), (bank_id, t, s)
                assert np.isfinite(b[t][s]).all()
        if s_bad in a[t]:
            ra, rb = a[t][s_bad], b[t][s_bad]
            if f_bad <= own < f_bad + n_bad:
                assert not np.isfinite(ra[0:7]).any(), (bank_id, t, own, ra[0:7])          # hand rotation and hand position: means over the stack
                bad_seen.append(own)
            else:
                assert np.array_equal(ra, rb), (bank_id, t, own)                                # before the row, and from the first frame behind it
            own += 1
    assert len(bad_seen) == n_bad and own == own_frames
    print(f"\nHOSTILE|C|{bank_id}|{name} S={S} smooth={smooth} n_mc={n_mc} {mode}|kernels {sorted(kernels)}|post {sorted(forms)}|"
          f"stream {s_bad} non-finite for {n_bad} frames (T {t_eff} + smooth {smooth} - 1), bit-equal to its twin before and after; others bit-equal")


def test_fk_bank_keeps_a_bad_stream_in_its_slot(golden):
    """FkStreamBank (no regressor, no window: the stack of `smooth` quaternion pairs alone): lockstep frames and subset frames"""
    from wear_mocap_ape_amd.data_types import messaging
    from wear_mocap_ape_amd.streams import FkStreamBank
    S, smooth, s_bad, f_bad = 70, 5, 64, 3
    n_bad = hi.poisoned_frames(1, smooth)
    frames = f_bad + n_bad + 3
    rows = _bank_rows(golden, "uarm", S, frames)
    col = messaging.WATCH_PHONE_IMU_LOOKUP["sw_rotvec_x"]
    for mode in ("lockstep", "subset", "host"):
        outs = []
        for poison in (True, False):
            bank = FkStreamBank(S, smooth=smooth, dtype=torch.float64)
            seq = []
            for f in range(frames):
                r = rows[f].copy()
                if poison and f == f_bad:
                    r[s_bad, col] = np.nan
                ids = list(range(S)) if f % 2 else [s_bad] + [s for s in range(S) if s != s_bad]
                if mode == "lockstep":
                    got, ids = bank.step_rows(r).cpu().numpy().copy(), list(range(S))
                elif mode == "subset":
                    got = bank.frame(r[ids], ids).cpu().numpy().copy()
                else:
                    got = bank.frame_host(np.ascontiguousarray(r[ids]), ids)
                seq.append(got[np.argsort(ids)])
            outs.append(np.array(seq))
        a, b = outs
        rest = np.arange(S) != s_bad
        assert np.isfinite(b).all() and np.array_equal(a[:, rest], b[:, rest])
        for f in range(frames):
            if f_bad <= f < f_bad + n_bad:
                assert not np.isfinite(a[f, s_bad, 0:4]).any(), (mode, f)
            else:
                assert np.array_equal(a[f, s_bad], b[f, s_bad]), (mode, f)
    print(f"\nHOSTILE|C|fk_bank|uarm rows S={S} smooth={smooth} lockstep/subset/host|stream {s_bad} non-finite for {n_bad} frames, then bit-equal")


def test_kalman_bank_tiles_that_straddle_streams(norm_stats):
    """S = 3 streams x E = 24 members, W = 4: 72 ensemble rows in 16-row `kf_linear_kernel` tiles, so the tiles at rows 16..31 and 48..63
    hold members of two streams.  (1) benign frames through the init phase and into the ensemble phase against oracle/kalman_oracle.py at
    2e-4 (tests/test_kalman.py's bound for one application of the model on injected draws); (2) a NaN row in stream 1: streams 0 and 2
    stay bit-equal to the twin bank; (3) the filter feeds its state back: stream 1 stays non-finite; (4) after reset(streams=[1]) it equals
    a cold-started twin bit for bit."""
    from oracle import kalman_oracle as ko
    from tests.test_kalman import make_model
    from tests.test_kalman_bank_gpu import make_bank, make_rows, new_oracle, pocket_stats, run_frame, slice_noise
    S, E, W, smooth = 3, 24, 4, 1
    stats = pocket_stats(norm_stats)
    m, sd = make_model(E, W, 31)
    a, b = make_bank(m, S, smooth, stats), make_bank(m, S, smooth, stats)
    oracles = [new_oracle(sd, E, W, smooth, stats) for _ in range(S)]
    rng = np.random.default_rng(24)
    worst = 0.0
    for f in range(W + 3):                                                        # W + 1 init frames, then two ensemble frames
        rows, nz, init = make_rows(rng, S), ko.draw_noise(rng, W, S * E), rng.standard_normal((S, E, 14)).astype(np.float32)
        oa, na, ya = run_frame(a, rows, None, nz, init)
        ob, nb, yb = run_frame(b, rows, None, nz, init)
        assert np.array_equal(oa, ob) and np.array_equal(na, nb)
        for s in range(S):
            oracles[s].check(rows[s], slice_noise(nz, s, E), init[s], ya[s], int(na[s]), oa[s], f"benign frame {f} stream {s}")
            ref = oracles[s].last_y
            worst = max(worst, float(np.abs(ya[s][:ref.shape[0]] - ref).max()))
    assert int(na[0]) == E                                                        # the ensemble phase was reached
    print(f"\nHOSTILE|C|kalman S={S} E={E} W={W}|benign frames vs oracle: worst target error {worst:.2e} (bound 2e-4)")
    assert worst <= 2e-4
    for f in range(4):
        rows, nz, init = make_rows(rng, S), ko.draw_noise(rng, W, S * E), rng.standard_normal((S, E, 14)).astype(np.float32)
        rows_a = rows.copy()
        if f == 0:
            rows_a[1, 10] = np.nan
        oa, na, ya = run_frame(a, rows_a, None, nz, init)
        ob, nb, yb = run_frame(b, rows, None, nz, init)
        for s in (0, 2):
            assert np.array_equal(oa[s], ob[s]) and na[s] == nb[s] and np.array_equal(ya[s], yb[s]), (f, s)
        assert np.isfinite(ob).all()
        assert not np.isfinite(oa[1][0:7]).any() and not np.isfinite(ya[1]).any(), (f, oa[1][0:7])
    a.reset(streams=[1])
    c = make_bank(m, S, smooth, stats)
    for f in range(W + 3):
        row, nz, init = make_rows(rng, 1), ko.draw_noise(rng, W, E), rng.standard_normal((1, E, 14)).astype(np.float32)
        (oa, na, ya), (oc, nc, yc) = run_frame(a, row, [1], nz, init), run_frame(c, row, [1], nz, init)
        assert np.array_equal(oa, oc) and np.array_equal(na, nc) and np.isfinite(oa).all(), f
        k = E if f > W else 1                                                     # (init frames: the prediction is row 0 of y)
        assert np.array_equal(ya[:, :k], yc[:, :k]), f
    a.check()
