"""The MLP regressor (DropoutFF) on every forward route against a plain float64 evaluation, at hostile inputs (the CPU half, which proves
that these cases can tell a subtly wrong kernel from a right one: tests/test_ff_numerics_cpu.py; cases and reference: tests/ff_cases.py).

Part A: every route of `fc.ROUTES` -- `ape_mlp_tile16` in its 16-row and 32-row forms at H = 128 and 256, every dims edge, all steps and the
        last step of a [B,T,I] input, the fused float64 z-score, the kernel's own Philox mask and an injected one, and `ape_mlp_pipe` at
        exact fill, ragged ends and the first and second wrap of its four-slot ring -- on every case of `fc.CASES`.  Every row of the
        output is held to `ff_forward64` within `max(1e-6, 4 e_ref)`, `e_ref = max |orc.ff_forward - ff_forward64|` on the same case;
        `last_kernel()` pins the route; `check()` is clean; the pipeline called twice gives the same bits.
Part B: one NaN / one +Inf in one input value: every other row keeps its bits, the NaN row is non-finite in every output, the +Inf row is
        non-finite or within the budget of a finite reference, and the next clean call has the first clean call's bits (the ring and the
        LDS hold the previous call's values).
Shapes follow the device's compute-unit count; a shape the device cannot form skips with the reason.  Every test prints its line (prefix
`FFNUM|`); the record is profiles/hostile_inputs.md."""
import numpy as np
import pytest
import torch

from tests import ff_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def _n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(norm_stats, route, case):
    n_cus = _n_cus()
    if fc.route_rows(route, n_cus) is None:
        pytest.skip(f"{route}: no MLP pipeline on a device of {n_cus} compute units")
    return fc.make_case(route, case, n_cus, norm_stats)


def _build(c):
    from wear_mocap_ape_amd.estimate import nn_models
    I, H, n_hidden, O = fc.MODELS[c["model"]]
    m = nn_models.DropoutFF(output_size=O, hidden_layer_size=H, hidden_layer_count=n_hidden, input_size=I, dropout=fc.P_DROP, device=0)
    m.load_state_dict(c["sd"])
    if c["st"] is not None:
        st = c["st"]
        m.set_norm_stats(st["xx_m"], st["xx_s"], np.zeros(O), np.ones(O))
    return m


def _run(m, c, x=None, mode=None):
    """one call on the case's route -> (y float32 [rows, O], last_kernel())"""
    mode = c["mode"] if mode is None else mode
    xt = torch.tensor(c["x"] if x is None else x).cuda()
    m.set_kernel(c["kernel"])
    if mode == "mc":
        m.manual_seed(fc.MC_SEED)                                # the call below is Monte-Carlo call 1: key (MC_SEED << 20) + 1
        y = m.monte_carlo_predictions(c["N"], xt, last_step_only=True)
    elif mode == "masks":
        y = m(xt, masks=torch.tensor(c["mask"]).cuda())
    elif mode in ("rows", "all"):
        y = m(xt)
    else:
        y = m(xt, last_step_only=True, normalize_input=mode == "zscore")
    y = y.cpu().numpy()
    used = m.last_kernel()
    m.check()
    m.set_kernel("auto")
    return y.reshape(-1, y.shape[-1]), used


# ---------------- part A ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.CASES)
@pytest.mark.parametrize("route", sorted(fc.ROUTES))
def test_route_against_the_float64_reference(norm_stats, route, case):
    c = _case(norm_stats, route, case)
    m = _build(c)
    y, used = _run(m, c)
    assert used == c["last"], (route, used)
    assert y.shape == c["ref"].shape and np.isfinite(y).all()
    err = float(np.abs(y - c["ref"]).max())                     # every row
    line = fc.line(c, used, err)
    print("\n" + line)
    assert err <= c["budget"], line
    if used == "ape_mlp_pipe":
        y2, used2 = _run(m, c)
        assert used2 == used and np.array_equal(y2, y), line
    if route == "steps/last":
        # the last step of the same windows out of an all-steps call: row_stride / row_offset pick the very values, so the very bits
        y_all, _ = _run(m, c, mode="all")
        assert np.array_equal(y_all.reshape(c["N"], c["T"], -1)[:, -1], y), line


# ---------------- part B ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["tile-1/pocket_like", "tile-2/W+17", "pipe/wrap1", "mc/pocket_like"])
def test_a_non_finite_row_stays_in_its_row(norm_stats, route):
    """A benign batch with one NaN (and separately one +Inf) in column `fc.BAD_COL` of (a) a row in the middle of a tile, (b) the last valid row
    of the last tile, (c) on the pipeline a row of a tile that lands in a ring slot used before.  No tolerances for the other rows.
    The Monte-Carlo route repeats ONE row: there the value reaches every sample row, and the next clean call is clean."""
    c = _case(norm_stats, route, "benign")
    m = _build(c)
    y_clean, used = _run(m, c)
    assert used == c["last"] and np.isfinite(y_clean).all()
    notes = []
    for bad in ([0] if c["mode"] == "mc" else fc.bad_rows(route, _n_cus())):
        for val in (np.nan, np.inf):
            xb = np.array(c["x"])
            if c["mode"] == "mc":
                xb[0, 0, fc.BAD_COL] = val
                own = np.arange(c["N"])
            else:
                xb[bad, fc.BAD_COL] = val
                own = np.array([bad])
            y, used = _run(m, c, xb)
            rest = np.setdiff1d(np.arange(c["N"]), own)
            assert used == c["last"] and np.array_equal(y[rest], y_clean[rest]), (route, bad, val)
            if np.isnan(val):
                assert not np.isfinite(y[own]).any(), (route, bad, y[own])
                continue
            seen = np.array(c["seen"][own])
            seen[:, fc.BAD_COL] = val
            r64 = fc.ff_forward64(c["sd"], seen, None if c["mask"] is None else c["mask"][own])
            if not np.isfinite(r64).all() or not np.isfinite(y[own]).any():
                assert not np.isfinite(y[own]).any(), (route, bad, y[own])
                notes.append(f"row {bad} +Inf: non-finite")
            else:
                e = float(np.abs(y[own] - r64).max())
                notes.append(f"row {bad} +Inf: finite like the reference, err {e:.2e}")
                assert e <= c["budget"], (route, bad, e, c["budget"])
    y_again, _ = _run(m, c)
    assert np.array_equal(y_again, y_clean)
    print(f"\nFFNUM|B|{route}|{used}|{c['model']}|N {c['N']}|NaN rows non-finite, every other row bit-equal, next clean call bit-equal|" + "; ".join(notes))
