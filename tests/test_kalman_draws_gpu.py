"""The Kalman filter's device-side draws (Box-Muller normals and flipout sign bits on Philox words, csrc/kalman_device.h and csrc/kalman.hip)
against `oracle/philox.py`, the host replica of the same counters: `format_state`, `KalmanSmartwatchModel.forward` and the `KalmanStreamBank`
with NO injected draws, each against the oracle fed the numbers the device must have drawn.  The CPU half -- e_draw below e_ref on every case,
six replica mutants each 100 budgets away -- is tests/test_philox_cpu.py; every test prints its line (prefix `PHILOX|`), the record is
profiles/philox_replica.md."""
import numpy as np
import pytest
import torch

from oracle import kalman_oracle as ko
from oracle import philox as ph
from tests import kalman_cases as kc
from tests import philox_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def test_format_state_draws_the_replicas_normals():
    """(out - state) / sqrt(0.1f) against kalman_init_noise within 8 * 2^-24 * max(1, r), r the replica's Box-Muller radius of the draw: the
    inputs of logf, sqrtf and sinf / cosf are bit-reproducible, so only the rounding of those four float32 calls and of the product
    differs.  The state is zero, so that the sum adds no rounding of its own; two calls, two keys; k = 3 states x 48 members."""
    from tests.test_kalman import make_model
    E, K, seed = 48, 3, 0x2_0000_0000 + 77
    m, _ = make_model(E, 10, 6)
    m.manual_seed(seed)
    state = np.zeros((K, 14), np.float32)
    c = np.float64(np.float32(0.31622776601683794))
    worst = 0.0
    for call in (1, 2):
        key = ph.kalman_call_seed(seed, call)
        out = m.format_state(torch.from_numpy(state)).cpu().numpy().astype(np.float64).reshape(K, E, 14)
        want = ph.kalman_init_noise(key, K, E).astype(np.float64)
        r = ph.kalman_radius(np.arange(K * E * 14), ph.TAG_INIT, key).reshape(K, E, 14)
        ratio = np.abs(out / c - want) / (8.0 * 2.0 ** -24 * np.maximum(1.0, r))
        worst = max(worst, float(ratio.max()))
        assert np.isfinite(out).all() and float(np.abs(out).max()) > 0.5
    print(f"\nPHILOX|format_state|kf_format_state_kernel|{2 * K * E * 14} draws, keys seed + step * (1, 2)|worst |draw - replica| / "
          f"(8 * 2^-24 * max(1, r)) = ratio {worst:.2f}")
    assert worst <= 1.0


@pytest.mark.parametrize("case", pc.KALMAN_CASES, ids=pc.kalman_id)
def test_forward_draws_the_replicas_noise(case):
    """kf_perturb, kf_linear<FLIP> and kf_update on their own draws: all five outputs of two consecutive calls within
    max(1e-6, 4 (e_ref + e_draw)) of the float64 oracle on the replica's draws of that call's key"""
    from wear_mocap_ape_amd.estimate import kalman_models
    first = pc.kalman_case(case, 1)
    m = kalman_models.KalmanSmartwatchModel(first["E"], first["W"])
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in first["sd"].items()})
    m.manual_seed(pc.KALMAN_SEEDS[case[1]])
    for call in (1, 2):
        c = pc.kalman_case(case, call)
        got = [t.cpu().numpy() for t in m.forward(torch.from_numpy(np.array(c["raw"])), torch.from_numpy(np.array(c["state"])))]
        err = kc.errors(got, c["ref"])
        buds = [kc.budget(r + d) for r, d in zip(c["e_ref"], c["e_draw"])]
        line = f"PHILOX|kalman forward {pc.kalman_id(case)} call {call}|kf_perturb + kf_linear + kf_update|key {c['key']:#x}|" + \
            "|".join(f"{n} err {e:.2e} e_ref {r:.2e} e_draw {d:.2e} budget {b:.2e} ratio {e / b:.2f}"
                     for n, e, r, d, b in zip(kc.OUTPUTS, err, c["e_ref"], c["e_draw"], buds))
        print("\n" + line)
        for g, w in zip(got, c["ref"]):
            assert g.shape == w.shape and np.isfinite(g).all()
        assert all(e <= b for e, b in zip(err, buds)), line
    m.check()


def test_bank_frames_draw_the_replicas_noise(norm_stats):
    """2 streams, E = 24, W = 4, smooth 1, W + 3 lockstep frames from a cold start with device draws: every stream against its own
    `ko.KalmanFrameLogic` fed the replica's draws of call f + 1 (shared perturbation, signs and format_state draws by list position), at the
    chained-frame bound of tests/test_kalman.py (5e-4 on the normalised targets); the key progression and the draw position behind the run"""
    from tests.test_kalman import make_model
    from tests.test_kalman_bank_gpu import TOL_Y, make_bank, make_rows, new_oracle, pocket_stats, slice_noise
    S, E, W, smooth, seed = 2, 24, 4, 1, 0x3_0000_0000 + 5
    stats = pocket_stats(norm_stats)
    m, sd = make_model(E, W, 31)
    bank = make_bank(m, S, smooth, stats, seed=seed)
    oracles = [new_oracle(sd, E, W, smooth, stats) for _ in range(S)]
    rng = np.random.default_rng(7)
    worst = 0.0
    assert bank.get_draw_position() == (seed, 0)
    for f in range(W + 3):
        key = ph.kalman_call_seed(seed, f + 1)
        nz, init = ph.kalman_noise(key, W, S * E), ph.kalman_init_noise(key, S, E)
        rows = make_rows(rng, S)
        out, n, y = bank.step_rows(rows, datagrams=True, return_targets=True)
        out, n, y = out.cpu().numpy().copy(), n.cpu().numpy().copy(), y.cpu().numpy().copy()
        for s in range(S):
            oracles[s].check(rows[s], slice_noise(nz, s, E), init[s], y[s], int(n[s]), out[s], f"device draws frame {f} stream {s}")
            ref = oracles[s].last_y
            worst = max(worst, float(np.abs(y[s][:ref.shape[0]] - ref).max()))
        assert bank.get_draw_position() == (seed, f + 1)
    assert int(n[0]) == E                                     # the ensemble phase was reached
    bank.check()
    print(f"\nPHILOX|kalman bank S={S} E={E} W={W}|ape_kalman_bank_frame|seed {seed:#x}, calls 1..{W + 3}|err {worst:.2e}|bound {TOL_Y:.0e}|"
          f"ratio {worst / TOL_Y:.2f}")
    assert worst < TOL_Y
