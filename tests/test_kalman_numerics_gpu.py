"""Kalman forward numerics on the GPU: ``csrc/kalman.hip`` (``kf_perturb_kernel``, ``kf_linear_kernel<FLIP>``, ``kf_update_kernel``) through
``KalmanSmartwatchModel.forward`` with injected draws, all five outputs against the float64 evaluation of ``oracle/kalman_oracle.py``.

Budget per output ``max(1e-6, 4 e_ref)``, ``e_ref = max |float32 oracle with the kernel's Gauss-Jordan - float64 reference|`` on the same case (the
rule of tests/test_hostile_inputs_gpu.py; no kernel's error is anybody's yardstick).  The cases, why each is there and the proof that they can
tell a wrong kernel from a right one: tests/kalman_cases.py and tests/test_kalman_numerics_cpu.py.  ``spread100`` / ``spread1000`` are recorded
only (finite, ``check()`` clean): float32 is not conditioned there.  Every test prints its line (prefix ``KALNUM|``); the record is
profiles/kalman_numerics.md."""
import numpy as np
import pytest
import torch

from tests import kalman_cases as kc
from tests.test_kalman import pack_noise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def _forward(c, raw=None):
    """one forward call of a fresh model on the case's weights and injected draws -> (the five outputs as numpy, the model)"""
    from wear_mocap_ape_amd.estimate import kalman_models
    m = kalman_models.KalmanSmartwatchModel(c["E"], c["W"])
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in c["sd"].items()})
    blob = pack_noise(c["nz"])
    assert blob.size == m.noise_floats(c["S"])
    out = m.forward(torch.from_numpy(np.array(c["raw"] if raw is None else raw)), torch.from_numpy(np.array(c["state"])),
                    noise=torch.from_numpy(blob))
    return [t.cpu().numpy() for t in out], m


@pytest.mark.parametrize("case", kc.CASES, ids=kc.case_id)
def test_forward_against_the_float64_reference(case):
    c = kc.make_case(case)
    got, m = _forward(c)
    err = kc.errors(got, c["ref"])
    print(kc.line(c, err))
    for g, r in zip(got, c["ref"]):
        assert g.shape == r.shape and g.dtype == np.float32 and np.all(np.isfinite(g))
    m.check()
    if not kc.is_held_by_design(case):
        return                                    # recorded: float32 Gauss-Jordan itself is 1e-4 .. 5e-3 from float64 on these
    assert c["held"], (c["id"], c["e_ref"])       # (the CPU half asserts the same)
    for name, e, e_ref in zip(kc.OUTPUTS, err, c["e_ref"]):
        assert e <= kc.budget(e_ref), (c["id"], name, e, kc.budget(e_ref))
    if case[0] == "collapsed":
        # every member of a stream predicts the same state: no anomaly, no gain, the prediction comes back -- in every member the same bits
        corrected, m_pred = got[0], got[2]
        assert np.abs(corrected.astype(np.float64) - m_pred).max() <= kc.budget(c["e_ref"][0])
        assert np.array_equal(corrected, np.repeat(corrected[:, :1], c["E"], axis=1))


def test_a_nan_stream_stays_in_its_own_rows():
    """(5,17,2): R = 85, stream 2 owns rows 34..50, which share their 16-row tiles with streams 1 and 3 (and the five sensor rows share one tile).
    A NaN in stream 2's raw observation leaves every output of the other four streams bit-equal to the clean call; stream 2 is non-finite in
    all that depends on its observation; a NaN is no zero pivot, so ``check()`` has nothing to report"""
    c = kc.make_case(("benign", (5, 17, 2), kc.WEIGHT_SEEDS[0]))
    clean, m0 = _forward(c)
    raw = np.array(c["raw"])
    raw[2, 1, 0, 7] = np.nan
    bad, m1 = _forward(c, raw)
    others = [0, 1, 3, 4]
    for name, a, b in zip(kc.OUTPUTS, clean, bad):
        assert np.array_equal(a[others], b[others]), name
        if name == "m_state_pred":                # the process model never reads the observation
            assert np.array_equal(a[2], b[2])
        else:
            assert not np.any(np.isfinite(b[2])), name
    assert all(np.all(np.isfinite(a)) for a in clean)
    m0.check()
    m1.check()
    print(f"KALNUM|nan-isolation-S5E17W2|streams 0, 1, 3, 4 bit-equal in all five outputs|stream 2 non-finite in "
          f"{', '.join(n for n in kc.OUTPUTS if n != 'm_state_pred')}; m_state_pred bit-equal|check() clean")
