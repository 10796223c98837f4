"""Kalman forward numerics, the CPU half: the cases of tests/kalman_cases.py have teeth (the GPU half: tests/test_kalman_numerics_gpu.py).

No kernel runs here.  These tests pin what the GPU half relies on:
  * the float32 oracle with the kernel's own Gauss-Jordan is within 1e-5 of the float64 reference on every case that is meant to hold the kernels
    (``e_ref``: the yardstick; budget of the kernels ``max(1e-6, 4 e_ref)``), so a budget never exceeds 4e-5 where outputs are 0.1 .. 14;
  * ``spread10`` makes Gauss-Jordan swap rows (the benign cases never do, condition number ~2.5);
  * eight subtly wrong variants of the forward (tests/kalman_cases.py ``MUTANTS``, oracle variants, not product code) each exceed that budget on
    a held case against the float64 reference -- a kernel with that defect fails tests/test_kalman_numerics_gpu.py.
Every test prints its figures (prefixes ``KALNUM|`` and ``KALMUT|``); the record is profiles/kalman_numerics.md."""
import numpy as np
import pytest

from oracle import kalman_oracle as ko
from tests import kalman_cases as kc

HELD = [c for c in kc.CASES if kc.is_held_by_design(c)]


def test_gauss_jordan_inverse_and_its_swap_count():
    """the numpy Gauss-Jordan against LAPACK in float64; a matrix that needs no swap and one that needs a known number"""
    rng = np.random.default_rng(0)
    a = rng.normal(size=(14, 14))
    spd = a @ a.T + 14 * np.eye(14)
    inv, swaps = ko.gauss_jordan_inverse(spd, np.float64)
    assert swaps == 0 and np.abs(inv - np.linalg.inv(spd)).max() < 1e-14
    inv, swaps = ko.gauss_jordan_inverse(a, np.float64)
    assert swaps > 0 and np.abs(inv @ a - np.eye(14)).max() < 1e-10
    anti = np.eye(14)[::-1] * np.arange(1.0, 15.0)           # every column's only entry is as far from the diagonal as can be
    inv, swaps = ko.gauss_jordan_inverse(anti, np.float64)
    assert swaps == 7 and np.array_equal(inv, np.linalg.inv(anti))
    inv32, _ = ko.gauss_jordan_inverse(spd, np.float32)
    assert inv32.dtype == np.float32 and np.abs(inv32 - np.linalg.inv(spd)).max() < 1e-7
    with pytest.raises(ValueError):
        ko.kalman_forward({}, None, np.zeros((1, 2, 2, 14), np.float32), {}, inverse="lu")


def test_default_evaluation_is_float32_with_the_float64_inverse():
    """``kalman_forward`` without the new arguments is the pinned checker: float32 results, ``inverse="inv64"``; "gj" differs from it by
    float32 rounding only on a benign case, and the float64 evaluations of both inverses agree to 1e-15"""
    c = kc.make_case(("benign", (3, 24, 10), 4))
    args = (c["sd"], c["raw"], c["state"], c["nz"])
    default = ko.kalman_forward(*args)
    explicit = ko.kalman_forward(*args, dtype=np.float32, inverse="inv64")
    assert all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(default, explicit))
    gj = ko.kalman_forward(*args, inverse="gj")
    assert max(kc.errors(gj, [d.astype(np.float64) for d in default])) < 5e-7
    ref_inv = ko.kalman_forward(*args, dtype=np.float64)
    assert all(r.dtype == np.float64 for r in c["ref"]) and max(kc.errors(ref_inv, c["ref"])) < 1e-15


@pytest.mark.parametrize("case", kc.CASES, ids=kc.case_id)
def test_case_is_conditioned_for_float32(case):
    """``e_ref <= 1e-5`` on every output of every case but ``spread100`` / ``spread1000`` (recorded, not held: their e_ref says float32 Gauss-Jordan
    itself is not conditioned there); the swap counts: >= 4 on ``spread10`` in the float64 evaluation, 0 on every benign case"""
    c = kc.make_case(case)
    print(kc.line(c))
    assert all(np.all(np.isfinite(r)) for r in c["ref"])
    if kc.is_held_by_design(case):
        assert max(c["e_ref"]) <= kc.HELD_E_REF and c["held"], (c["id"], c["e_ref"])
    if case[0] == "spread10":
        assert c["swaps"] >= 4, (c["id"], c["swaps"])
    if case[0] == "benign":
        assert c["swaps"] == 0 and c["cond"] < 10, (c["id"], c["swaps"], c["cond"])


def test_the_regimes_do_what_they_are_for():
    for shape in kc.REGIME_SHAPES:
        benign = kc.make_case(("benign", shape, kc.WEIGHT_SEEDS[0]))
        # collapsed: one prediction per stream, so A = 0, P = 0, no gain: corrected == pred, and the mean prediction is that prediction
        c = kc.make_case(("collapsed", shape, kc.WEIGHT_SEEDS[0]))
        corrected, m_corrected, m_pred = c["ref"][:3]
        assert np.abs(corrected - m_pred).max() < 1e-15 and np.abs(m_corrected - m_pred).max() < 1e-15
        assert np.ptp(c["ref"][4], axis=1).max() > 0.1                       # while the observations of the members still differ
        # bigR: R ~ 1e8 I, the gain vanishes and state_corrected is the process model's output, which differs from member to member
        c = kc.make_case(("bigR", shape, kc.WEIGHT_SEEDS[0]))
        assert c["cond"] < 1.0001 and np.abs(c["ref"][1] - c["ref"][2]).max() < 1e-8
        assert np.ptp(c["ref"][0], axis=1).max() > 0.05
        # loud_z: an innovation y - H X an order of magnitude above the benign one
        c = kc.make_case(("loud_z", shape, kc.WEIGHT_SEEDS[0]))
        assert c["magnitude"][4] > 10 * benign["magnitude"][4]


def test_the_variant_without_a_mutation_is_the_oracle():
    """``kc.variant_forward(mutant=None)`` is ``ko.kalman_forward(inverse="gj")`` bit for bit in both precisions, so that a mutant's distance from
    the reference is its one defect's doing"""
    for case in (("benign", (5, 17, 2), 4), ("spread10", (2, 24, 10), 4), ("benign", (1, 2, 2), 5)):
        c = kc.make_case(case)
        args = (c["sd"], c["raw"], c["state"], c["nz"])
        for dt in (np.float32, np.float64):
            a, b = kc.variant_forward(*args, dtype=dt), ko.kalman_forward(*args, dtype=dt, inverse="gj")
            assert all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b)), (c["id"], dt)


@pytest.mark.parametrize("mutant", kc.MUTANTS)
def test_mutant_exceeds_the_budget_on_a_held_case(mutant):
    """the float32 evaluation of the mutant against the float64 reference, per held case and output, as a multiple of the kernels' budget"""
    worst = []
    for case in HELD:
        c = kc.make_case(case)
        err = kc.errors(kc.variant_forward(c["sd"], c["raw"], c["state"], c["nz"], np.float32, mutant), c["ref"])
        ratio, i = max((e / kc.budget(r), i) for i, (e, r) in enumerate(zip(err, c["e_ref"])))
        worst.append((ratio, c["id"], kc.OUTPUTS[i], err[i], kc.budget(c["e_ref"][i])))
    caught = sorted((w for w in worst if w[0] > 1.0), reverse=True)
    top = caught[0] if caught else max(worst)
    print(f"KALMUT|{mutant}|caught by {len(caught)} of {len(worst)} held cases|clearest: {top[1]} {top[2]} err {top[3]:.2e} budget {top[4]:.2e}"
          f"|missed by: {', '.join(sorted(w[1] for w in worst if w[0] <= 1.0)) or 'none'}")
    assert caught, (mutant, max(worst))
    assert caught[0][0] > 10.0, (mutant, caught[0])          # and not by a hair: a clear order of magnitude over the budget somewhere
