"""Float64 geometry across the exponent range, the parts that need no GPU: the inputs of tests/test_fk_magnitudes_gpu.py, a numpy
transcription of csrc/angle_device.h, and the proof that the inputs can tell the identity route WITHOUT its safe band from the reference.

The hips quaternion is (cos(a/2), 0, sin(a/2), 0), a = atan2(sn, cs).  The device gets it from half-angle identities on
r = sqrt(cs^2 + sn^2), c = cs / r, |s| = |sn| / r where r lies in [1e-140, 1e140], and from atan2 -> cos / sin, the reference's own route,
everywhere else.  Until the band existed the identities ran for every positive finite r: for |sn|, |cs| around 1e-160 the squares are
subnormal, r keeps a few bits and the quaternion was off by up to 1e-3 -- on inputs only the float64 entries can be given (the smallest
float32 subnormal squared is 2e-90).  The expected values are the oracle's (`orc.arm_pose_from_targets(..., "closed")`), NaN exactly
where it has NaN, 1e-11 elsewhere: the project's bound for `ape_fk`."""
import numpy as np
import pytest

from oracle import ape_oracle as orc

TOL = 1e-11
BAND = (1e-140, 1e140)                     # csrc/angle_device.h plain_radius
TINY = 5e-324                              # the smallest subnormal


def scales():
    """10^e for every integer e of the float64 range (subnormals included), quarter decades where the squares underflow and overflow"""
    s = [float(f"1e{e}") for e in range(-323, 309)]
    s += [10.0 ** (e + q / 4.0) for e in range(-165, -150) for q in (1, 2, 3)]
    s += [10.0 ** (e + q / 4.0) for e in range(150, 155) for q in (1, 2, 3)]
    return np.array(sorted(s))


def unit_pairs():
    """16 (sin, cos) pairs: the four axes exactly, both sides of +-pi and of 0, and eight angles in the open quadrants"""
    near = [np.pi - 1e-7, -(np.pi - 1e-7), 1e-7, -1e-7]
    quad = [0.3, -0.3, 1.1, -1.1, 2.0, -2.0, 2.9, -2.9]
    return np.array([(0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0)] + [(np.sin(a), np.cos(a)) for a in near + quad])


MIXED = np.array([(1e-160, 1e-170), (1e-170, 1e-160), (-1e-160, 1e-170), (1e-170, -1e-160), (1e-161, -3e-162), (-1e-161, -1e-161),
                  (TINY, 0.0), (0.0, TINY), (-TINY, 0.0), (0.0, -TINY), (TINY, -0.0), (-0.0, TINY), (TINY, TINY), (1e-310, 1e-310), (3e-162, 1e-300),
                  (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0),
                  (1e-160, 1e10), (1e10, 1e-160), (1e200, 1e-200), (-1e-200, 1e200), (1e308, 1e308), (-1e308, 1e308), (1e150, -1e154), (1e154, 1e154),
                  (1.3e154, 1.3e154), (1e-140, 0.0), (0.0, -1e140), (9.9e-141, 1e-142), (7.1e139, 7.1e139), (np.inf, 1.0), (1.0, -np.inf),
                  (np.inf, -np.inf), (np.nan, 1.0), (1.0, np.nan)])


def hips_pairs():
    """every (sn, cs) of the sweep, float64 [N, 2]: scale x unit pair, then the mixed pairs"""
    s, u = scales(), unit_pairs()
    return np.concatenate([(s[:, None, None] * u[None, :, :]).reshape(-1, 2), MIXED])


def six_d_scales():
    """(scale of column 1, scale of column 2) of a 6D rotation: both at one scale over the decades, and 1e100 apart in both orders"""
    dec = [float(f"1e{e}") for e in range(-323, 309, 3)] + [10.0 ** (e + q / 4.0) for e in range(-165, -150, 2) for q in (0, 2)] + \
          [10.0 ** (e + 0.5) for e in range(150, 155)]
    out = [(d, d) for d in dec]
    for e in range(-320, 209, 8):
        lo, hi = float(f"1e{e}"), float(f"1e{e + 100}")
        out += [(lo, hi), (hi, lo)]
    return np.array(out)


def layout_columns(layout):
    """-> (first column of the lower arm's 6D, of the upper arm's, of the hips pair or None)"""
    return {0: (0, 6, 12), 1: (0, 6, None), 2: (3, 12, 18)}[layout]


def preds_of(layout):
    """float64 prediction rows of one layout -> (preds [N, O], n_hips: the leading rows that carry the hips sweep (0 without hips columns)).
    Part 1: ordinary 6D columns (and positions), the hips pair swept.  Part 2: an ordinary hips pair, the 6D columns of the lower arm (even
    rows) or the upper arm (odd rows) scaled per column."""
    O = orc.LAYOUT_NUM_TARGETS[layout]
    c_l, c_u, c_h = layout_columns(layout)
    rng = np.random.default_rng(40 + layout)
    hp = hips_pairs() if c_h is not None else np.zeros((0, 2))
    p1 = rng.normal(size=(len(hp), O))
    if c_h is not None:
        p1[:, c_h:c_h + 2] = hp
    sc = six_d_scales()
    p2 = rng.normal(size=(len(sc), O))
    with np.errstate(over="ignore"):               # (1e308 x a value above one: an infinite target, part of the sweep)
        for r, (s1, s2) in enumerate(sc):
            c = c_l if r % 2 == 0 else c_u
            p2[r, [c, c + 2, c + 4]] *= s1
            p2[r, [c + 1, c + 3, c + 5]] *= s2
    return np.concatenate([p1, p2]), len(hp)


def expected(preds, layout):
    with np.errstate(all="ignore"):
        return orc.arm_pose_from_targets(preds, orc.DEFAULT_BODY, layout, "closed")


def compare(got, ref):
    """-> (same NaN pattern, same infinities, largest |difference| elsewhere)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nan_ok = np.array_equal(np.isnan(got), np.isnan(ref))
    inf = np.isinf(ref)
    inf_ok = np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf])
    fin = np.isfinite(ref) & np.isfinite(got)
    return nan_ok, inf_ok, float(np.abs(got[fin] - ref[fin]).max(initial=0.0))


# ---------------- csrc/angle_device.h in numpy ------------------------------------------------------------------------------------------------
def half_of_atan2_numpy(y, x, band=BAND):
    """(cos(a/2), sin(a/2)) of a = atan2(y, x), the device's formula operation by operation.  `band=None`: the route choice before the
    band existed (every positive finite r takes the identities)"""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y)
        plain = (r > 0.0) & (r <= np.finfo(np.float64).max) if band is None else (r >= band[0]) & (r <= band[1])
        rs = np.where(plain, r, 1.0)
        c, sa = x / rs, np.abs(y) / rs
        big = np.sqrt(0.5 * (1.0 + np.abs(c)))
        small = sa / (2.0 * big)
        ci = np.where(c >= 0.0, big, small)
        si = np.copysign(np.where(c >= 0.0, small, big), y)
        h = 0.5 * np.arctan2(y, x)
        return np.where(plain, ci, np.cos(h)), np.where(plain, si, np.sin(h))


def est_with_transcribed_hips(preds, layout, band):
    """the oracle's est rows with the hips quaternion (and the shoulder it rotates) from the transcription"""
    c_h = layout_columns(layout)[2]
    est = expected(preds, layout)
    c, s = half_of_atan2_numpy(preds[:, c_h], preds[:, c_h + 1], band)
    q = np.stack([c, np.zeros_like(c), s, np.zeros_like(c)], axis=-1)
    with np.errstate(all="ignore"):
        uo = orc.quat_rotate(q, orc.DEFAULT_BODY[:, 6:9])
    old = est[:, 6:9].copy()
    est[:, 17:21], est[:, 6:9] = q, uo
    if layout == 0:                                 # the arm hangs off the shoulder
        est[:, 0:3] += uo - old
        est[:, 3:6] += uo - old
    return est


def _radius(preds, layout):
    c_h = layout_columns(layout)[2]
    with np.errstate(all="ignore"):
        return np.hypot(preds[:, c_h], preds[:, c_h + 1])


@pytest.mark.parametrize("layout", [0, 2])
def test_the_sweep_has_teeth(layout):
    """the identities without the band miss 1e-11 by a factor of 1e5 or more where both squares are subnormal, and pass where they are normal;
    with the band the transcription passes on every row of the sweep -- so the GPU test fails on the former device code and only there"""
    preds, n_hips = preds_of(layout)
    preds = preds[:n_hips]
    ref = expected(preds, layout)
    r = _radius(preds, layout)
    old = est_with_transcribed_hips(preds, layout, None)
    deep = (r >= 1e-161) & (r <= 1e-159)
    safe = (r >= BAND[0]) & (r <= BAND[1])
    assert deep.sum() >= 16 and safe.sum() >= 16 * 280
    e_deep = compare(old[deep], ref[deep])[2]
    nan_ok, inf_ok, e_safe = compare(old[safe], ref[safe])
    print(f"\nFAREND|fk|layout {layout}|identities without the band: err {e_deep:.2e} on r in [1e-161, 1e-159], {e_safe:.2e} on r in [1e-140, 1e140]")
    assert e_deep >= 1e5 * TOL
    assert nan_ok and inf_ok and e_safe <= TOL
    by_decade = {e: compare(old[(r >= 10.0 ** e) & (r < 10.0 ** (e + 1))], ref[(r >= 10.0 ** e) & (r < 10.0 ** (e + 1))])[2] for e in range(-163, -153)}
    print("FAREND|fk|identities without the band, err by decade of r: " + ", ".join(f"1e{e}: {v:.1e}" for e, v in by_decade.items()))
    new = est_with_transcribed_hips(preds, layout, BAND)
    nan_ok, inf_ok, e_new = compare(new, ref)
    print(f"FAREND|fk|layout {layout}|identities inside [1e-140, 1e140], atan2 outside: err {e_new:.2e} on all {len(preds)} rows")
    assert nan_ok and inf_ok and e_new <= TOL


def test_inside_the_band_the_route_is_the_identities():
    """no bit may change for in-band inputs: there the banded transcription IS the unbanded one"""
    preds, n_hips = preds_of(0)
    sn, cs = preds[:n_hips, 12], preds[:n_hips, 13]
    r = _radius(preds[:n_hips], 0)
    safe = (r >= BAND[0]) & (r <= BAND[1])
    a, b = half_of_atan2_numpy(sn[safe], cs[safe], BAND), half_of_atan2_numpy(sn[safe], cs[safe], None)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_sweep_covers_what_it_claims():
    s = scales()
    assert s[0] == 1e-323 and s[-1] == 1e308 and len(s) == 632 + 45 + 15 and len(unit_pairs()) == 16
    hp = hips_pairs()
    assert len(hp) == len(s) * 16 + len(MIXED)
    assert np.signbit(MIXED[:, 0][(MIXED == 0).all(axis=1)]).sum() == 2            # signed zeros in both columns
    for layout in (0, 1, 2):
        preds, n_hips = preds_of(layout)
        assert preds.shape[1] == orc.LAYOUT_NUM_TARGETS[layout] and (n_hips > 0) == (layout != 1)
        ref = expected(preds, layout)
        # the 6D part meets NaN and the finite side alike (an unscaled norm: squares that overflow or flush give what numpy gives)
        assert np.isnan(ref[n_hips:]).any() and np.isfinite(ref[n_hips:]).all(axis=1).sum() > 100
