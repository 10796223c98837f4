"""MLP regressor numerics, the CPU half: the cases of tests/ff_cases.py have teeth (the GPU half: tests/test_ff_numerics_gpu.py).

No kernel runs here.  These tests pin what the GPU half relies on, from the reference alone:
  * `ff_forward64` is the reference's DropoutFF.forward (checked against torch in float64 where torch is importable, and against the pinned
    float32 oracle within its stated 2e-6 on the benign case of every model);
  * it is finite on every (route, case), so the cases are hostile to kernels, not to the mathematics;
  * ten subtly wrong variants of the forward (tests/ff_cases.py `MUTANTS`, oracle variants, not product code) each move it by more than the
    kernels' budget `max(1e-6, 4 e_ref)` on a case of a route that could make the mistake -- a kernel with that defect fails the GPU half.
    One of them, padded input columns that read on into the next row, cannot show on finite inputs (the packed weights are zero there:
    0 * finite = 0): the case that catches it is the NaN row of the non-finite tests, whose neighbours must keep their bits.
The shapes are those of a device of `fc.PROOF_CUS` compute units.  Every test prints its figures (prefixes `FFNUM|`, `FFMUT|`)."""
import numpy as np
import pytest

from tests import ff_cases as fc

CUS = fc.PROOF_CUS
FINITE_MUTANTS = [m for m in fc.MUTANTS if m != "pad_reads_next_row"]


def test_reference_is_the_models_forward_in_float64():
    """against torch.nn.functional in float64 (Linear, leaky_relu with the float32 slope widened), injected mask included"""
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    for model in ("pocket_like", "least", "i33"):
        c = fc.make_case({"pocket_like": "masks", "least": "tile-1/least", "i33": "tile-1/i33"}[model], "w4", CUS)
        sd = {k: torch.from_numpy(v.astype(np.float64)) for k, v in c["sd"].items()}
        a = torch.from_numpy(c["seen"].astype(np.float64)[:64])
        a = F.leaky_relu(F.linear(a, sd["_input_layer.weight"], sd["_input_layer.bias"]), float(np.float64(fc.SLOPE)))
        for k in range(fc.n_hidden_of(c["sd"])):
            a = F.leaky_relu(F.linear(a, sd[f"_hidden_layers.{k}.weight"], sd[f"_hidden_layers.{k}.bias"]), float(np.float64(fc.SLOPE)))
        if c["mask"] is not None:
            a = a * torch.from_numpy(c["mask"].astype(np.float64)[:64])
        y = F.linear(a, sd["_output_layer.weight"], sd["_output_layer.bias"]).numpy()
        scale = max(1.0, float(np.abs(y).max()))
        assert np.abs(y - c["ref"][:64]).max() <= 1e-12 * scale, model


def test_the_variant_without_a_mutation_is_the_reference():
    for route in ("tile-1/pocket_like", "tile-1/least", "mc/most", "masks"):
        c = fc.make_case(route, "sat30", CUS)
        y = fc.variant_forward(c["sd"], c["seen"], c["mask"])
        assert y.dtype == np.float64 and np.array_equal(y, c["ref"]), route


def test_case_weights_and_inputs_are_what_they_claim():
    base, big = fc.state_dict("most", "benign"), fc.state_dict("most", "w16")
    assert all(np.array_equal(big[k], base[k]) == k.startswith("_output_layer.") for k in base)
    assert np.array_equal(big["_hidden_layers.6.bias"], base["_hidden_layers.6.bias"] * np.float32(16))
    assert len(base) == 2 * (7 + 2) and base["_input_layer.weight"].shape == (256, 64) and base["_output_layer.weight"].shape == (32, 256)
    z = fc.case_z("zeros", 11, 1, 5)
    assert not z[0].any() and not np.signbit(z[0]).any() and not z[2].any() and np.signbit(z[2]).all() and z[1].all()
    assert np.abs(fc.case_z("z1e3", 64, 1, 22)).max() > 900 and set(np.unique(fc.case_z("sat30", 9, 1, 3))) == {-30.0, 30.0}
    # the zero rows reach the input layer as zeros of both signs, and their pre-activation is the bias
    c = fc.make_case("tile-1/pocket_like", "zeros", CUS)
    assert not c["seen"][0].any() and np.signbit(c["seen"][2]).all()
    assert np.array_equal(c["ref"][0], c["ref"][5]) and np.array_equal(c["ref"][0], c["ref"][2])


def test_route_shapes_pin_their_edges():
    W, P = fc.wide_rows(256), fc.pipe_pairs(256)
    assert (W, P) == (16384, 128)
    rows = {r: fc.route_rows(r, 256) for r in fc.ROUTES}
    assert rows["tile-2/W+37"] % 32 == 5 and rows["tile-2/W+17"] % 32 == 17 and rows["tile-2-kx64"] == W
    assert rows["pipe/wrap1"] == 32 * P * 4 + 32 == W + 32 and rows["pipe/wrap2"] == 32 * P * 9 + 5
    assert all(n >= W for r, n in rows.items() if fc.ROUTES[r][5]) and all(fc.route_rows(r, 8) is None for r in fc.ROUTES if fc.ROUTES[r][5])
    # every model is run, and the pipeline's cases stay inside what the pipeline takes (H 256, two hidden layers, I <= 32, O <= 16)
    assert {fc.ROUTES[r][0] for r in fc.ROUTES} == set(fc.MODELS)
    for r, (model, kernel, _, mode, last, pipe) in fc.ROUTES.items():
        I, H, n_hidden, O = fc.MODELS[model]
        assert not pipe or (H == 256 and n_hidden == 2 and I <= 32 and O <= 16 and mode in ("rows", "zscore")), r
    # the poisoned rows: inside the batch, one of them the last row, and on the pipeline one in the first reused ring slot
    for r in ("tile-1/pocket_like", "tile-2/W+17", "pipe/wrap1", "mc/pocket_like"):
        bad = fc.bad_rows(r, 256)
        assert rows[r] - 1 in bad and all(0 <= b < rows[r] for b in bad)
    assert 32 * P * 4 + 8 in fc.bad_rows("pipe/wrap1", 256)


@pytest.mark.parametrize("case", fc.CASES)
@pytest.mark.parametrize("route", sorted(fc.ROUTES))
def test_case_is_finite_and_conditioned(norm_stats, route, case):
    """the float64 reference is finite on every held (route, case); `benign` has e_ref <= 2e-6, the oracle's stated distance"""
    c = fc.make_case(route, case, CUS, norm_stats)
    print("\n" + fc.line(c))
    assert c["ref"].dtype == np.float64 and c["ref"].shape == (c["seen"].shape[0], fc.MODELS[c["model"]][3])
    assert np.isfinite(c["ref"]).all()
    if case == "benign":
        assert c["e_ref"] <= 2e-6, (route, c["e_ref"])


def _shift(c, mutant):
    return float(np.abs(fc.mutant_output(c, mutant) - c["ref"]).max())


@pytest.mark.parametrize("mutant", FINITE_MUTANTS)
def test_mutant_exceeds_the_budget_on_a_held_case(norm_stats, mutant):
    """the float64 evaluation of the mutant against the float64 reference, per (route, case) that could make the mistake, as a multiple
    of the kernels' budget; a (route, case) that catches fewer mutants than `benign` does is named in test_cases_that_hold_less_than_benign"""
    worst = []
    for route in fc.mutant_routes(mutant):
        for case in fc.CASES:
            c = fc.make_case(route, case, CUS, norm_stats)
            e = _shift(c, mutant)
            worst.append((e / c["budget"], route, case, e, c["budget"]))
    caught = sorted((w for w in worst if w[0] > 1.0), reverse=True)
    top = caught[0] if caught else max(worst)
    print(f"\nFFMUT|{mutant}|caught by {len(caught)} of {len(worst)} (route, case)|clearest: {top[1]} {top[2]} moved {top[3]:.2e} budget {top[4]:.2e}"
          f"|missed by: {', '.join(sorted(f'{w[1]} {w[2]}' for w in worst if w[0] <= 1.0)) or 'none'}")
    assert caught, (mutant, max(worst))
    assert caught[0][0] > 10.0, (mutant, caught[0])          # and not by a hair


def test_cases_that_hold_less_than_benign(norm_stats):
    """Where the budget is large in absolute terms (w16: outputs up to 1e7, e_ref of several units) only the mutants show that it still holds
    something.  Per (route, case): how many of the route's mutants it catches, against the route's benign case.  Reported, and every route
    must catch on each of its cases at least one mutant: a case that catches nothing checks nothing."""
    less = []
    for route in sorted(fc.ROUTES):
        muts = [m for m in FINITE_MUTANTS if route in fc.mutant_routes(m)]
        if not muts:
            continue
        count = {case: sum(_shift(fc.make_case(route, case, CUS, norm_stats), m) > fc.make_case(route, case, CUS, norm_stats)["budget"] for m in muts)
                 for case in fc.CASES}
        for case in fc.CASES:
            assert count[case] >= 1, (route, case, count)
            if count[case] < count["benign"]:
                less.append(f"{route} {case}: {count[case]} of {len(muts)} (benign {count['benign']})")
    print("\nFFMUT|cases that catch fewer mutants than benign|" + ("; ".join(less) or "none"))


def test_padded_columns_that_read_on_show_only_on_a_nan_row():
    """`pad_reads_next_row`: invisible on every finite case (asserted: the distance is exactly 0), caught by the NaN placement of the GPU
    half's non-finite tests: the row in front of the poisoned one turns non-finite, where every other row must keep its bits"""
    for route in ("tile-1/pocket_like", "tile-1/least", "tile-1/i33", "pipe/wrap1", "pipe-dims/least"):
        for case in ("benign", "z1e3"):
            c = fc.make_case(route, case, CUS)
            assert _shift(c, "pad_reads_next_row") == 0.0, (route, case)
        c = fc.make_case(route, "benign", CUS)
        for bad in fc.bad_rows(route, CUS):
            x = c["seen"].copy()
            x[bad, fc.BAD_COL] = np.nan
            clean_rule = fc.ff_forward64(c["sd"], x)
            rest = np.arange(c["N"]) != bad
            assert np.array_equal(clean_rule[rest], c["ref"][rest]) and not np.isfinite(clean_rule[bad]).any()
            y = fc.mutant_output(c, "pad_reads_next_row", x)
            assert not np.array_equal(y[rest], c["ref"][rest]) and not np.isfinite(y[bad - 1]).any(), (route, bad)
        print(f"\nFFMUT|pad_reads_next_row|{route}|finite cases: distance 0|NaN in column {fc.BAD_COL} of rows {fc.bad_rows(route, CUS)}: the row in front turns non-finite")
    # a model without padded columns cannot make the mistake
    c = fc.make_case("tile-1/most", "benign", CUS)
    x = c["seen"].copy()
    x[24, fc.BAD_COL] = np.nan
    assert np.isfinite(fc.mutant_output(c, "pad_reads_next_row", x)[23]).all()


def test_float32_in_another_summation_order_stays_inside_the_budget():
    """the rule leaves a correct kernel room: a float32 evaluation with k ascending, the bias as the initial accumulator and separate multiply
    and add (none of which the oracle does) on the widest model and the largest weights"""
    def seq32(sd, x):
        def lin(a, W, b, bias_first=True):
            acc = np.broadcast_to(b, (a.shape[0], W.shape[0])).astype(np.float32).copy() if bias_first else np.zeros((a.shape[0], W.shape[0]), np.float32)
            for k in range(W.shape[1]):
                acc = (acc + a[:, k:k + 1] * W[None, :, k]).astype(np.float32)
            return acc if bias_first else (acc + b).astype(np.float32)
        act = lambda v: np.where(v > 0, v, fc.SLOPE * v).astype(np.float32)
        a = act(lin(x, sd["_input_layer.weight"], sd["_input_layer.bias"]))
        for k in range(fc.n_hidden_of(sd)):
            a = act(lin(a, sd[f"_hidden_layers.{k}.weight"], sd[f"_hidden_layers.{k}.bias"]))
        return lin(a, sd["_output_layer.weight"], sd["_output_layer.bias"], False)
    for route, case in (("tile-1/most", "w16"), ("tile-1/pocket_like", "benign"), ("tile-1/least", "z1e3")):
        c = fc.make_case(route, case, CUS)
        e = float(np.abs(seq32(c["sd"], c["seen"]) - c["ref"]).max())
        print(f"\nFFNUM|float32, another order|{route}|{case}|err {e:.2e}|budget {c['budget']:.2e}|ratio {e / c['budget']:.2f}")
        assert e <= c["budget"]
