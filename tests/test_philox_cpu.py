"""The host replica of the device-side Philox draws (oracle/philox.py), the part that needs no GPU: the generator's known answers, the builders'
shapes, and the proof that the cases of tests/test_philox_routes_gpu.py and tests/test_kalman_draws_gpu.py can tell a subtly wrong counter
scheme from the right one.

Mutants.  Ten wrong readings of the contract (`ph.Variant`), each applied to the REPLICA: the float64 reference of a case under the mutant's
draws is compared with the reference under the contract's draws.  A kernel with that defect computes (to rounding) the mutant's reference, so
a distance of 100 budgets and more means the GPU test of that case fails by two orders of magnitude.  Every mutant is asserted on every case
it can touch:
    t / u swapped, b for b & ~3, word (b + 1) & 3, layer l + 1, >> 9, 9 rounds     every LSTM, DropoutFF, bank, subset and replay case
                                                                                      (the bank head's row counter has no `& ~3`: not that one)
    k1 forced to 0                                                                  every such case whose key has a high word; on the keys
                                                                                      below 2^32 it is the contract itself (asserted equal)
    >> 9, 9 rounds, k1 = 0, sign bit c >> 1, sign word (c >> 6) & 3, sin <-> cos    every Kalman forward case
The mutants of the large cases are evaluated on some of their rows (rows of one call are independent: those rows of the whole reference),
the budget always on the whole case.

`uf > p` against `uf >= p` is NOT tested: uf = k * 2^-24 with integer k, and float32(0.2) = 13421773 * 2^-26 is no multiple of 2^-24, so no
draw equals p and the two comparisons keep the same units at p = 0.2f."""
import numpy as np
import pytest

from oracle import kalman_oracle as ko
from oracle import philox as ph
from tests import kalman_cases as kc
from tests import philox_cases as pc

MUTANTS = {
    "t_u_swapped": ph.Variant(swap_t_u=True),
    "row_unaligned": ph.Variant(row_unaligned=True),
    "word_b_plus_1": ph.Variant(word_shift=1),
    "k1_zero": ph.Variant(drop_k1=True),
    "layer_plus_1": ph.Variant(layer_shift=1),
    "shift_9": ph.Variant(mantissa_shift=9),
    "nine_rounds": ph.Variant(rounds=9),
    "sign_bit_c_shr_1": ph.Variant(sign_bit_shift=1),
    "sign_word_c_shr_6": ph.Variant(sign_word_shift=6),
    "sin_cos_exchanged": ph.Variant(swap_sin_cos=True),
}
MASK_MUTANTS = ("t_u_swapped", "row_unaligned", "word_b_plus_1", "k1_zero", "layer_plus_1", "shift_9", "nine_rounds")
KALMAN_MUTANTS = ("k1_zero", "shift_9", "nine_rounds", "sign_bit_c_shr_1", "sign_word_c_shr_6", "sin_cos_exchanged")
MIN_RATIO = 100.0


# ---------------- the generator and the builders -------------------------------------------------------------------------------------------
def test_known_answers():
    """Philox4x32-10 (Salmon et al. 2011): the three published vectors, counter; key -> output"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, (k0, k1), want in kat:
        got = ph.philox4x32_10(np.array(ctr), (k1 << 32) | k0)
        assert got.dtype == np.uint32 and got.tolist() == list(want)
    batch = ph.philox4x32_10(np.array([k[0] for k in kat[:1]] * 6).reshape(2, 3, 4), 0)          # leading axes are kept
    assert batch.shape == (2, 3, 4) and (batch == np.array(kat[0][2], dtype=np.uint32)).all()
    with pytest.raises(ValueError):
        ph.philox4x32_10(np.zeros(3), 0)


def test_shapes_and_dtypes_of_every_builder():
    m = ph.lstm_masks(5, 37, 6, 128, 3, 0.2)
    assert m.shape == (2, 37, 6, 128) and m.dtype == np.float32 and set(np.unique(m)) == {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(0.2))}
    assert ph.lstm_masks(5, 37, 6, 256, 1, 0.2).shape == (0, 37, 6, 256)
    for f in (ph.ff_mask(5, 50, 256, 0.2), ph.ff_bank_mask(5, 175, 256, 0.2), ph.ff_bank_mask(5, [3, 4], 256, 0.2, philox_base=2 ** 33)):
        assert f.ndim == 2 and f.shape[1] == 256 and f.dtype == np.float32
    n = ph.kalman_normals(np.arange(12).reshape(3, 4), 0x300, 9)
    assert n.shape == (3, 4) and n.dtype == np.float32 and np.isfinite(n).all()
    s = ph.kalman_signs(5, 300, 0x204, 9)
    assert s.shape == (5, 300) and s.dtype == np.float32 and set(np.unique(s)) == {-1.0, 1.0}
    W, rows = 4, 6
    nz, want = ph.kalman_noise(9, W, rows), ko.draw_noise(np.random.default_rng(0), W, rows)
    assert list(nz) == list(want)
    for name in want:
        assert {k: (v.shape, v.dtype) for k, v in nz[name].items()} == {k: (v.shape, v.dtype) for k, v in want[name].items()}
    i = ph.kalman_init_noise(9, 2, 3)
    assert i.shape == (2, 3, 14) and i.dtype == np.float32
    assert ph.lstm_call_seed(0x12345, 1) == 0x1234500001 and ph.bank_call_seed(2 ** 64 - 1, 2) == 1
    assert ph.kalman_call_seed(1, 2) == (1 + 2 * 0xD1342543DE82EF95) % 2 ** 64


def test_keep_rate_and_normal_moments():
    """keep rate of lstm_masks within 5.5 standard errors of 1 - p; the Box-Muller draws are standard normal, the signs fair"""
    for p in (0.2, 0.5):
        m = ph.lstm_masks(0x1_0000_0003, 64, 6, 256, 3, p)
        n = m.size
        assert abs(float((m > 0).mean()) - (1.0 - np.float32(p))) < 5.5 * np.sqrt(p * (1 - p) / n)
    x = ph.kalman_normals(np.arange(400_000), 0x101, 77).astype(np.float64)
    assert abs(x.mean()) < 5.5 / np.sqrt(x.size) and abs(x.var() - 1) < 5.5 * np.sqrt(2 / x.size)
    assert abs(np.corrcoef(x[0::2], x[1::2])[0, 1]) < 5.5 / np.sqrt(x.size / 2)                  # cosine and sine of one pair
    s = ph.kalman_signs(64, 512, 0x200, 77)
    assert abs(s.mean()) < 5.5 / np.sqrt(s.size)
    assert abs(np.mean(s[:, :384] * s[:, 128:])) < 5.5 / np.sqrt(s[:, 128:].size)               # no period of 128 columns


def test_rows_of_a_chunk_are_rows_of_the_one_call():
    whole = ph.lstm_masks(2 ** 40 + 5, 530, 3, 128, 3, 0.2)
    for r0 in (512, 16, 6):                                   # (6: a chunk that starts inside a row quad)
        assert np.array_equal(ph.lstm_masks(2 ** 40 + 5, 530 - r0, 3, 128, 3, 0.2, row_base=r0), whole[:, r0:])
    assert np.array_equal(ph.lstm_masks(2 ** 40 + 5, [529, 3, 77], 3, 128, 3, 0.2), whole[:, [529, 3, 77]])
    bank = ph.ff_bank_mask(7, 40, 256, 0.2)
    assert np.array_equal(ph.ff_bank_mask(7, 24, 256, 0.2, philox_base=16), bank[16:])
    assert not np.array_equal(ph.ff_bank_mask(7, 8, 256, 0.2, philox_base=2 ** 32), bank[:8])     # the high row word is read


def test_the_contract_variant_changes_nothing_and_each_mutant_changes_the_draws():
    base = ph.lstm_masks(2 ** 40 + 5, 16, 4, 128, 3, 0.2)
    assert np.array_equal(base, ph.lstm_masks(2 ** 40 + 5, 16, 4, 128, 3, 0.2, v=ph.Variant()))
    for name in MASK_MUTANTS:
        assert not np.array_equal(base, ph.lstm_masks(2 ** 40 + 5, 16, 4, 128, 3, 0.2, v=MUTANTS[name])), name
    nz = ph.kalman_noise(2 ** 40 + 5, 2, 6)
    for name in KALMAN_MUTANTS:
        other = ph.kalman_noise(2 ** 40 + 5, 2, 6, v=MUTANTS[name])
        assert any(not np.array_equal(nz[l][k], other[l][k]) for l in nz for k in nz[l]), name


# ---------------- the route cases under the mutants ------------------------------------------------------------------------------------------
_WHOLE = {}


def _whole(key, make):
    """the contract's reference and budget of a whole case, computed once"""
    if key not in _WHOLE:
        _WHOLE[key] = make()
    return _WHOLE[key]


def _some_rows(B):
    """up to 96 rows: the first and last row quads, a stretch around 512 (a second cluster launch) and around the batch-tile wave"""
    if B <= 96:
        return np.arange(B)
    picks = [np.arange(16), np.arange(B - 16, B)]
    for edge in (512, pc.wave_rows(pc.MI355X_CUS)):
        if edge + 8 < B:
            picks.append(np.arange(edge - 8, edge + 8))
    return np.unique(np.concatenate(picks))


def _applies(name, key):
    return name != "k1_zero" or (key >> 32) != 0


def _assert_moved(what, name, key, shift, bud):
    if _applies(name, key):
        ratio = shift / bud
        print(f"PHILOX|mutant|{name}|{what}|moves the float64 reference by {shift:.2e}|budget {bud:.2e}|ratio {ratio:.1e}")
        assert ratio >= MIN_RATIO, (what, name, shift, bud)
    else:
        print(f"PHILOX|mutant|{name}|{what}|key below 2^32: the contract itself")
        assert shift == 0.0, (what, name, shift)


@pytest.mark.parametrize("route", sorted(pc.LSTM_ROUTES))
def test_mutants_move_every_lstm_route_case(norm_stats, route):
    inp = pc.lstm_inputs(norm_stats, route)

    def whole():
        y64, y32 = pc.lstm_reference(inp, with32=True)
        return y64, pc.budget(float(np.abs(y32 - y64).max()))
    y64, bud = _whole(("lstm", route), whole)
    rows = _some_rows(inp["B"])
    for name in MASK_MUTANTS:
        shift = float(np.abs(pc.lstm_reference(inp, MUTANTS[name], rows) - y64[rows]).max())
        _assert_moved(route, name, inp["key"], shift, bud)


def test_mutants_move_the_dropout_ff_case():
    inp = pc.ff_inputs()
    y64, y32 = pc.ff_reference(inp, with32=True)
    bud = pc.budget(float(np.abs(y32 - y64).max()))
    for name in MASK_MUTANTS:
        _assert_moved("DropoutFF mc 50", name, inp["key"], float(np.abs(pc.ff_reference(inp, MUTANTS[name]) - y64).max()), bud)


@pytest.mark.parametrize("bank", sorted(pc.BANKS))
def test_mutants_move_every_bank_case(norm_stats, bank):
    reg, name, S, n_mc, smooth, seed, T, F = pc.bank_dims(bank)

    def whole():
        ref = pc.bank_reference(norm_stats, bank, with32=True)
        return ref, pc.budget(max(pc.quantity_error(r32, r64) for r64, r32 in ref.values()))
    ref, bud = _whole(("bank", bank), whole)
    streams = np.arange(S) if S * n_mc <= 600 else np.array([0, 1, S // 2, S - 1])
    last = F - 1
    want = [q[streams] for q in ref[last][0]]
    for mut in MASK_MUTANTS:
        if reg == "ff" and mut == "row_unaligned":
            continue                                        # the bank head's counter carries the row itself: nothing to misalign
        got = pc.bank_reference(norm_stats, bank, [last], MUTANTS[mut], streams)[last][0]
        _assert_moved(bank, mut, ph.bank_call_seed(seed, last), pc.quantity_error(got, want), bud)


@pytest.mark.parametrize("case", pc.BANK_CASES)
@pytest.mark.parametrize("bank", sorted(pc.BANKS))
def test_hostile_bank_cases_are_finite_and_still_tell_a_wrong_counter_reading(norm_stats, bank, case):
    """the cases of tests/test_hostile_banks_gpu.py: the float64 bank reference stays finite, and at least one wrong reading of the counter
    contract moves it by MIN_RATIO budgets.  Evaluated on the last frame of up to four streams (rows of one call are independent: those
    rows of the whole reference), the budget from the same rows; the factor MIN_RATIO covers the whole case's larger e_ref (the GPU test
    computes that one, and asserts the whole reference finite)"""
    reg, name, S, n_mc, smooth, seed, T, F = pc.bank_dims(bank)
    streams = np.arange(S) if S <= 4 else np.array([0, 1, S // 2, S - 1])
    last = F - 1
    r64, r32 = pc.bank_reference(norm_stats, bank, [last], streams=streams, with32=True, case=case)[last]
    assert all(np.isfinite(q).all() for q in r64)
    bud = pc.budget(pc.quantity_error(r32, r64))
    moved = {}
    for mut in MASK_MUTANTS:
        if (reg == "ff" and mut == "row_unaligned") or not _applies(mut, ph.bank_call_seed(seed, last)):
            continue
        got = pc.bank_reference(norm_stats, bank, [last], MUTANTS[mut], streams, case=case)[last][0]
        moved[mut] = pc.quantity_error(got, r64) / bud
    print(f"PHILOX|hostile bank|{bank}|{case}|budget {bud:.2e}|" + "|".join(f"{k} {v:.1e}" for k, v in moved.items()))
    assert max(moved.values()) >= MIN_RATIO, (bank, case, moved)


@pytest.mark.parametrize("case", pc.BANK_CASES)
def test_the_wide_head_bank_cases_tell_a_wrong_counter_reading(norm_stats, case):
    """the 20-output DropoutFF bank of tests/test_hostile_banks_gpu.py (`ape_ff_bank_head<2>`): whole case, all frames"""
    from tests.test_hostile_banks_gpu import wide_head_case
    ref = wide_head_case(norm_stats, case)[3]
    assert all(np.isfinite(q).all() for f in ref for q in ref[f][0])
    bud = pc.budget(max(pc.quantity_error(ref[f][1], ref[f][0]) for f in ref))
    moved = {}
    for mut in MASK_MUTANTS:
        if mut != "row_unaligned":
            other = wide_head_case(norm_stats, case, MUTANTS[mut])[3]
            moved[mut] = max(pc.quantity_error(other[f][0], ref[f][0]) for f in ref) / bud
    print(f"PHILOX|hostile bank|ff-wide-head-7x25|{case}|budget {bud:.2e}|" + "|".join(f"{k} {v:.1e}" for k, v in moved.items()))
    assert max(moved.values()) >= MIN_RATIO, (case, moved)


def test_the_default_bank_case_is_the_benign_one(norm_stats):
    """`case="benign"` of the bank helpers: the weights as drawn and the features of before, bit for bit"""
    for bank in ("mc_small-3x25", "ff-7x25"):
        reg, name, S, n_mc, smooth, seed, T, F = pc.bank_dims(bank)
        st, I = norm_stats[name], pc.orc.MODEL_CONFIGS[name]["I"]
        x = st["xx_m"] + st["xx_s"] * np.random.default_rng(1000 + S).normal(size=(F, S, I))
        x[..., 0] = 0.02
        assert np.array_equal(pc.bank_features(norm_stats, bank), x.astype(np.float32))
        assert np.array_equal(pc.bank_features(norm_stats, bank, "benign"), pc.bank_features(norm_stats, bank))
        assert not np.array_equal(pc.bank_features(norm_stats, bank, "z1e3"), pc.bank_features(norm_stats, bank))
    sd, sd16 = pc.bank_state_dict("lstm", "pocket"), pc.bank_state_dict("lstm", "pocket", "trained")
    assert all(np.array_equal(sd[k], pc.state_dict("pocket")[k]) for k in sd)
    assert all(np.array_equal(sd16[k], sd[k] * np.float32(16) if k.startswith("lstm.") else sd[k]) for k in sd)
    ff, ff16 = pc.bank_state_dict("ff", "pocket"), pc.bank_state_dict("ff", "pocket", "trained")
    assert all(np.array_equal(ff16[k], ff[k] if k.startswith("_output_layer.") else ff[k] * np.float32(16)) for k in ff)


def test_mutants_move_the_subset_frame_and_the_replay(golden, norm_stats):
    q = pc.SUBSET
    feats = pc.host_features(pc.trace_rows(golden, 3 * q["S"], 5)).reshape(3, q["S"], -1)
    r64, r32 = pc.subset_reference(norm_stats, feats, with32=True)
    bud = pc.budget(pc.quantity_error(r32, r64))
    for name in MASK_MUTANTS:
        got = pc.subset_reference(norm_stats, feats, MUTANTS[name])[0]
        _assert_moved("subset frame", name, q["seed"] + 2, pc.quantity_error(got, r64), bud)
    q = pc.REPLAY
    feats = pc.host_features(pc.trace_rows(golden, q["F"], 6))
    y64, y32 = pc.replay_reference(norm_stats["pocket"], feats, with32=True)
    bud = pc.budget(float(np.abs(y32 - y64).max()))
    frames = np.array([0, 1, q["cut"] - 1, q["cut"], 20, 21, q["F"] - 1])          # (the second cluster launch starts in frame 20)
    rows = (frames[:, None] * q["n_mc"] + np.arange(q["n_mc"])).reshape(-1)
    for name in MASK_MUTANTS:
        got = pc.replay_reference(norm_stats["pocket"], feats, MUTANTS[name], frames)[0]
        _assert_moved("replay", name, q["seed"], float(np.abs(got - y64[rows]).max()), bud)


# ---------------- the Kalman forward cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.KALMAN_CASES, ids=pc.kalman_id)
def test_kalman_cases_draw_error_stays_below_e_ref_and_mutants_move_them(case):
    """e_draw (the float64 reference on draws moved by +-2 float32 ulps: what the device's own log / sqrt / sin / cos may differ by) is added to
    e_ref in the GPU budget: it stays below e_ref on every case and call, so it cannot swallow a fault.  Then the six mutants."""
    for call in (1, 2):
        c = pc.kalman_case(case, call)
        print(f"PHILOX|kalman case|{pc.kalman_id(case)} call {call}|" +
              "|".join(f"{n} e_ref {r:.2e} e_draw {d:.2e}" for n, r, d in zip(kc.OUTPUTS, c["e_ref"], c["e_draw"])))
        assert all(d < r for d, r in zip(c["e_draw"], c["e_ref"])), (case, call, c["e_draw"], c["e_ref"])
    c = pc.kalman_case(case, 1)
    buds = [kc.budget(r + d) for r, d in zip(c["e_ref"], c["e_draw"])]
    for name in KALMAN_MUTANTS:
        m = pc.kalman_case(case, 1, MUTANTS[name])
        ratio, out = max((e / b, n) for e, b, n in zip(kc.errors(m["ref"], c["ref"]), buds, kc.OUTPUTS))
        if _applies(name, c["key"]):
            print(f"PHILOX|mutant|{name}|kalman {pc.kalman_id(case)}|clearest output {out}|ratio {ratio:.1e}")
            assert ratio >= MIN_RATIO, (case, name, out, ratio)
        else:
            assert ratio == 0.0


def test_consecutive_kalman_calls_use_different_keys():
    a, b = pc.kalman_case(pc.KALMAN_CASES[0], 1), pc.kalman_case(pc.KALMAN_CASES[0], 2)
    assert a["key"] != b["key"] and not np.array_equal(a["nz"]["sensor_model.fc6"]["eps_b"], b["nz"]["sensor_model.fc6"]["eps_b"])
    assert max(kc.errors(a["ref"], b["ref"])) > 1e-3
