"""Spectra of a replay (`ape_spectra`) on the GPU.

Reference: `score.spectra_numpy` (plain numpy, `np.fft.rfft` per segment) on the same rows; for float32 rows the statement of the rounded
rows.  Counts are asserted exactly.

Rows: `[F, 25]` messages whose six position columns (`score.pose_cols`) go in as a strided view, a truth of `[F, 21]` est rows.  Column 4
(hand x) carries an offset 1000 times its motion, so the detrend path has something to take off.  skip = 2.  For a plan (N, hop) the
recordings are, in order, of lengths N - 1 + skip (no segment), N + skip (exactly one), N + hop - 1 + skip (still one), N + hop + skip
(two), N + 15 hop + skip (exactly a tile of 16), one frame, N + 16 hop + skip (17: one past a tile) and N + 32 hop + skip (33: one past
two tiles), so F depends on the plan (786 frames at (64, 5) .. 4621 at (64, 64)).  N = 512 runs one recording of 4 segments.  N = 16
has one bin block; N = 64 and 512 are multiples of 32, where bin N/2 is summed off the matrix path; N = 48 is 16 times an odd number
with two blocks, the second padded with bins past N/2 that are computed and not written.

Tolerance, u = 2^-53.  A coefficient X(k) of a segment differs from the statement's by at most
    e_x = (N + 8) u sum_n |w_n| |x_n - m|            any summation order, fused or not, a half-ulp table entry, the roundings of a_n
        + N u max|x_n| sum_n w_n                     with detrend: the two means differ by at most N u max|x|, each a_n by w_n times that
(e_y likewise).  A term of the sums then differs by at most
    | |X'|^2 - |X|^2 |      <= 2 |X| e_x + e_x^2 + 4 u |X|^2
    | conj(Y') X' - conj(Y) X |  <= |Y| e_x + |X| e_y + e_x e_y + 4 u |X| |Y|        (each of its two parts)
(the last summand: the two products and the sum of a term, rounded separately), and a sum over J segments by the sum of its terms'
bounds (the triangle inequality) plus (J + 2) u sum |term| for the order of the additions on either side.  The worst fraction of the
allowance used is printed (`-s`)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SKIP = 2
COLS = (4, 5, 6, 11, 12, 13)
TCOLS = (0, 1, 2, 3, 4, 5)
WORST = {"fraction": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def layout_of(n, hop):
    lengths = [n - 1 + SKIP, n + SKIP, n + hop - 1 + SKIP, n + hop + SKIP, n + 15 * hop + SKIP, 1, n + 16 * hop + SKIP, n + 32 * hop + SKIP]
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(int).tolist()
    return starts, int(sum(lengths)), [0, 1, 1, 2, 16, 0, 17, 33]


def rows_of(F, seed, sets=1):
    """messages [sets, F, 25] and est-row truth [sets, F, 21], float64 on the host: smooth motion plus noise, the truth a little ahead"""
    rng = np.random.default_rng(seed)
    t = np.arange(F)[:, None]
    msg = rng.standard_normal((sets, F, 25)) * 0.02
    tru = rng.standard_normal((sets, F, 21)) * 0.01
    for c in range(sets):
        base = 0.3 * np.sin(2 * np.pi * t / (40.0 + 7 * np.arange(6)) + c) + np.cumsum(rng.standard_normal((F, 6)), axis=0) * 0.01
        msg[c][:, COLS] += base
        tru[c][:, TCOLS] += np.roll(base, -3, axis=0)
    msg[:, :, 4] += 1000.0 * 0.3
    tru[:, :, 0] += 1000.0 * 0.3
    return msg, tru


def allowance(x, y, n, hop, w, detrend, starts, F):
    """the docstring's bound for one set: [R, V, n/2 + 1, 1 | 4], from the statement's own per-segment coefficients"""
    R, V = len(starts), x.shape[1]
    out = np.zeros((R, V, n // 2 + 1, 1 if y is None else 4))
    mag = np.zeros_like(out)
    for r in range(R):
        s, e = starts[r], starts[r + 1] if r + 1 < R else F
        J = (e - s - SKIP - n) // hop + 1 if e - s - SKIP >= n else 0
        for j in range(J):
            f0 = s + SKIP + j * hop
            for v in range(V):
                segs = [x[f0:f0 + n, v]] + ([] if y is None else [y[f0:f0 + n, v]])
                if not all(np.isfinite(g).all() for g in segs):
                    continue
                X, E = [], []
                for g in segs:
                    m = g.mean() if detrend else 0.0
                    X.append(np.abs(np.fft.rfft(w * (g - m))))
                    E.append((n + 8) * U * (np.abs(w) * np.abs(g - m)).sum() + (n * U * np.abs(g).max() * np.abs(w).sum() if detrend else 0.0))
                out[r, v, :, 0] += 2 * X[0] * E[0] + E[0] ** 2 + 4 * U * X[0] ** 2
                mag[r, v, :, 0] += X[0] ** 2
                if y is not None:
                    out[r, v, :, 1] += 2 * X[1] * E[1] + E[1] ** 2 + 4 * U * X[1] ** 2
                    mag[r, v, :, 1] += X[1] ** 2
                    cross = X[1] * E[0] + X[0] * E[1] + E[0] * E[1] + 4 * U * X[0] * X[1]
                    out[r, v, :, 2] += cross
                    out[r, v, :, 3] += cross
                    mag[r, v, :, 2] += X[0] * X[1]
                    mag[r, v, :, 3] += X[0] * X[1]
        out[r] += (J + 2) * U * mag[r]
    return out


def held(acc, counts, x, y, n, hop, taper, detrend, starts, F, what):
    """one set's device record against the statement's, within the allowance; counts exactly"""
    from wear_mocap_ape_amd import score
    ref, rc = score.spectra_numpy(x, y, None, None, n, hop, taper, detrend, starts, SKIP)
    assert np.array_equal(counts, rc), what
    allow = allowance(x, y, n, hop, score.spectra_taper(taper, n), detrend, starts, F)
    diff = np.abs(acc - ref)
    none = allow == 0.0
    assert (diff[none] == 0.0).all(), what                 # a recording without a segment holds exact zeros
    frac = float((diff[~none] / allow[~none]).max()) if (~none).any() else 0.0
    WORST["fraction"] = max(WORST["fraction"], frac)
    print(f"{what}: worst fraction of the allowance {frac:.3f} (so far {WORST['fraction']:.3f})")
    assert frac <= 1.0, what


VARIANTS = [  # sets, truth ("shared" | "sets" | None), taper, detrend
    (1, "shared", "hann", True),
    (1, "sets", "hann", True),            # rows [1, F, 25] against truth [1, F, 21]: the three-dimensional route with one set
    (3, "sets", "boxcar", False),
    (3, "shared", "own", True),
    (1, None, "hann", True),
    (3, None, "own", False),
]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,hop", [(16, 16), (16, 8), (16, 5), (48, 24), (64, 64), (64, 32), (64, 5)])
def test_against_the_statement(n, hop, dtype):
    from wear_mocap_ape_amd import score
    starts, F, J = layout_of(n, hop)
    msg, tru = rows_of(F, 100 * n + hop, 3)
    npd = np.float32 if dtype == torch.float32 else np.float64
    msg_r, tru_r = msg.astype(npd).astype(np.float64), tru.astype(npd).astype(np.float64)
    dm, dt = dev(msg, dtype), dev(tru, dtype)
    own = 0.2 + np.random.default_rng(5).random(n)
    for sets, truth, taper, detrend in VARIANTS:
        tp = own if taper == "own" else taper
        rows = dm[:sets] if sets > 1 or truth == "sets" else dm[0]
        tr = None if truth is None else (dt[:sets] if truth == "sets" else dt[0])
        acc, counts = score.spectra(rows, tr, COLS, None if tr is None else TCOLS, n, hop, tp, detrend, starts, SKIP)
        acc, counts = acc.cpu().numpy(), counts.cpu().numpy()
        if rows.dim() == 2:
            acc, counts = acc[None], counts[None]
        assert acc.shape == (sets, len(starts), 6, n // 2 + 1, 1 if tr is None else 4)
        assert (counts[..., 0] == np.asarray(J)[None, :, None]).all() and (counts[..., 1] == 0).all()
        for c in range(sets):
            y = None if truth is None else tru_r[c if truth == "sets" else 0][:, TCOLS]
            held(acc[c], counts[c], msg_r[c][:, COLS], y, n, hop, tp, detrend, starts, F,
                 f"N={n} hop={hop} {npd.__name__} sets={sets} truth={truth} taper={taper} detrend={detrend} set {c}")


def test_n_512_in_a_single_tile():
    from wear_mocap_ape_amd import score
    n, hop = 512, 256
    F = n + 3 * hop + SKIP
    msg, tru = rows_of(F, 512)
    acc, counts = score.spectra(dev(msg[0]), dev(tru[0], torch.float32), COLS, TCOLS, n, hop, "hann", True, None, SKIP)
    assert counts[..., 0].tolist() == [[4] * 6]
    y = tru[0].astype(np.float32).astype(np.float64)[:, TCOLS]
    held(acc.cpu().numpy(), counts.cpu().numpy(), msg[0][:, COLS], y, n, hop, "hann", True, [0], F, "N=512 hop=256 f64 rows, f32 truth")


def test_a_nan_frame_leaves_its_segments_out_of_its_column_only():
    from wear_mocap_ape_amd import score
    n, hop = 64, 32
    starts, F, J = layout_of(n, hop)
    msg, tru = rows_of(F, 7)
    clean = score.spectra(dev(msg[0]), dev(tru[0]), COLS, TCOLS, n, hop, "hann", True, starts, SKIP)
    bad_m, bad_t = msg[0].copy(), tru[0].copy()
    f_x = starts[6] + SKIP + 3 * hop + 5                    # recording 6 (17 segments): in segments 2 and 3 of column 5
    f_y = starts[7] + SKIP + 20 * hop + 40                  # recording 7 (33 segments): in segments 20 and 21 of truth column 2, the third tile
    bad_m[f_x, 5] = np.nan
    bad_t[f_y, 2] = -np.inf
    acc, counts = score.spectra(dev(bad_m), dev(bad_t), COLS, TCOLS, n, hop, "hann", True, starts, SKIP)
    want = np.zeros((len(starts), 6, 2), dtype=np.int32)
    want[:, :, 0] = np.asarray(J)[:, None]
    want[6, 1] = (15, 2)
    want[7, 2] = (31, 2)
    assert np.array_equal(counts.cpu().numpy(), want)
    a, c = acc.cpu().numpy(), clean[0].cpu().numpy()
    assert np.isfinite(a).all()
    touched = np.zeros(a.shape[:2], dtype=bool)
    touched[6, 1] = touched[7, 2] = True
    assert np.array_equal(a[~touched], c[~touched])         # every other (recording, column) has the bits of the clean call
    assert (a[6, 1, :, 0] < c[6, 1, :, 0]).any() and (a[7, 2, :, 1] < c[7, 2, :, 1]).any()
    held(a, counts.cpu().numpy(), bad_m[:, COLS], bad_t[:, TCOLS], n, hop, "hann", True, starts, F, "N=64 hop=32 with a NaN and an inf")


def test_the_same_bits():
    from wear_mocap_ape_amd import score
    n, hop = 64, 5
    starts, F, _ = layout_of(n, hop)
    msg, tru = rows_of(F, 9, 3)
    dm, dt = dev(msg, torch.float32), dev(tru)
    both = score.spectra(dm, dt, COLS, TCOLS, n, hop, "hann", True, starts, SKIP)
    again = score.spectra(dm, dt, COLS, TCOLS, n, hop, "hann", True, starts, SKIP)
    assert torch.equal(both[0], again[0]) and torch.equal(both[1], again[1])                     # twice the same call
    alone = score.spectra(dm[1], dt[1], COLS, TCOLS, n, hop, "hann", True, starts, SKIP)
    assert torch.equal(alone[0], both[0][1]) and torch.equal(alone[1], both[1][1])               # a set alone against the set within three
    for r in (4, 7):                                                                             # a recording alone against the same one later in a batch
        a, b = starts[r], starts[r + 1] if r + 1 < len(starts) else F
        rec = score.spectra(dm[2, a:b], dt[2, a:b], COLS, TCOLS, n, hop, "hann", True, None, SKIP)
        assert torch.equal(rec[0][0], both[0][2, r]) and torch.equal(rec[1][0], both[1][2, r])
    plain = score.spectra(dm, None, COLS, None, n, hop, "hann", True, starts, SKIP)
    assert plain[0].shape[-1] == 1 and torch.equal(plain[0][..., 0], both[0][..., 0])            # W = 1 against [0] of W = 4
    assert torch.equal(plain[1], both[1])
    shared = score.spectra(dm, dt[0], COLS, TCOLS, n, hop, "hann", True, starts, SKIP)           # one truth for all sets
    assert torch.equal(shared[0][0], both[0][0]) and torch.equal(shared[0][..., 0], both[0][..., 0])


def test_refusals_and_a_capturing_stream_leave_the_outputs_untouched():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    n, F = 16, 200
    msg, tru = rows_of(F, 3)
    x, y = dev(msg[0]), dev(tru[0])
    acc = torch.full((1, 1, 6, n // 2 + 1, 4), -7.0, dtype=torch.float64, device="cuda")
    counts = torch.full((1, 1, 6, 2), -7, dtype=torch.int32, device="cuda")
    st, xc, yc, w = np.zeros(1, dtype=np.int32), np.asarray(COLS, dtype=np.int32), np.asarray(TCOLS, dtype=np.int32), np.ones(n)
    ptr = lambda t: C.c_void_p(t.data_ptr())                # noqa: E731
    hp = lambda a: C.c_void_p(a.ctypes.data)                # noqa: E731

    def call(stream, N=n, hop=8, fs=25, out=acc):
        return lib.ape_spectra(ptr(x), _hip.F64, 0, fs, hp(xc), ptr(y), _hip.F64, 0, 21, hp(yc), 6, 1, F, hp(st), 1, SKIP, N, hop, hp(w), 1,
                               ptr(out), ptr(counts), stream)

    torch.cuda.synchronize()
    now = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kw, word in ((dict(N=24), b"N 24"), (dict(hop=17), b"hop"), (dict(fs=13), b"column offset"), (dict(out=x), b"overlaps x_dev")):
        rc, err = call(now, **kw), lib.ape_last_error()
        assert rc == 1 and word in err, (kw, rc, err)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros((4,), device="cuda")
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            rc, err = call(C.c_void_p(side.cuda_stream)), lib.ape_last_error()
    torch.cuda.current_stream().wait_stream(side)
    assert rc == 1 and b"capturing" in err and b"spectra" in err, (rc, err)
    torch.cuda.synchronize()
    assert (acc == -7.0).all() and (counts == -7).all() and torch.equal(x, dev(msg[0]))          # nothing was written
    assert call(now) == 0                                   # the same arguments on a stream that is not capturing
    torch.cuda.synchronize()
    J = (F - SKIP - n) // 8 + 1
    assert counts[0, 0, :, 0].tolist() == [J] * 6 and bool(torch.isfinite(acc).all()) and bool((acc[..., :2] >= 0).all())


# ---------------- end to end: the estimators' entries ----------------------------------------------------------------------------------------------
def test_sweep_recording_carries_the_bandwidths(golden, tmp_path_factory):
    from tests.test_post_sweep_gpu import pocket
    from tests.test_replay import _synthetic_rows
    from wear_mocap_ape_amd import score
    n, starts, seed = 700, [0, 3, 40], 0x5EED
    est = pocket(tmp_path_factory.mktemp("spectra"), 1, 25)
    rows = _synthetic_rows(golden, "pocket", n, 21)
    out1, y = est.process_recording(rows, starts=starts, return_targets=True, seed=seed)
    configs = score.grid((1, 5, 10), (25,))
    out = est.repost(y, configs, starts=starts)
    skip = est.sequence_len - 1
    truth = (y.double().mean(dim=1) * torch.as_tensor(est._yy_s, device=y.device) + torch.as_tensor(est._yy_m, device=y.device)).contiguous()
    res = est.sweep_recording(rows, truth, (1, 5, 10), (25,), starts=starts, seed=seed, spectra=True)
    plain = est.sweep_recording(rows, truth, (1, 5, 10), (25,), starts=starts, seed=seed)
    assert sorted(plain) == ["acc", "best", "configs"] and sorted(res) == ["acc", "bandwidth", "best", "configs"]
    assert np.array_equal(plain["acc"], res["acc"]) and res["bandwidth"].shape == (3, 3, 6)
    # targets go through resample_truth's conversion to est rows: the same record as est rows given directly
    est_rows = score.resample_truth(est._layout, truth, "targets", starts, None, None, n, starts, None, 0.0, est.body_measurements)
    acc, counts = score.spectra(out, est_rows, score.pose_cols(est._layout, "msg"), score.pose_cols(est._layout, "est"), 256, 128, "hann", True,
                                starts, skip)
    J = max(0, (n - 40 - skip - 256) // 128 + 1)
    assert J >= 2 and counts[:, :, :, 0].cpu().numpy().tolist() == [[[0] * 6, [0] * 6, [J] * 6]] * 3
    want = score.bandwidth(score.summarise_spectra(acc, counts, "hann"))
    assert np.array_equal(res["bandwidth"], want, equal_nan=True) and np.isnan(want[:, :2]).all()
    # spectrum_recording: the class's skip, the replay's own rows; configuration (1, 25) is the replay itself
    a1, c1, s1 = est.spectrum_recording(out1, truth, starts=starts, truth_kind="targets", rate=50.0)
    assert torch.equal(a1, acc[0]) and torch.equal(c1, counts[0]) and s1["psd"].shape == (3, 6, 129) and s1["freqs"][-1] == 25.0
    a2, c2, s2 = est.spectrum_recording(out1, est_rows, starts=starts)
    assert torch.equal(a2, a1) and np.array_equal(s2["gain"], s1["gain"], equal_nan=True)
    a3, c3, s3 = est.spectrum_recording(out1, starts=starts, n=64, hop=16, taper="boxcar")
    assert a3.shape == (3, 6, 33, 1) and "gain" not in s3 and int(c3[1, 0, 0]) == 0 and int(c3[2, 0, 0]) == (n - 40 - skip - 64) // 16 + 1


def test_spectrum_recording_fk_only_and_kalman(golden):
    import oracle.kalman_oracle as ko
    from tests.test_kalman_bank_gpu import _estimator, make_rows
    from wear_mocap_ape_amd import score
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    fk = WatchPhoneUarm(smooth=5)
    rows = np.tile(golden("stream_trace_uarm.npz")["rows"].astype(np.float32), (3, 1))[:60]
    starts = [0, 20, 40]
    out = fk.process_recording(rows, starts=starts)
    a1, c1, _ = fk.spectrum_recording(out, starts=starts, n=16, hop=4)
    a2, c2 = score.spectra(out, None, score.pose_cols(fk._layout, "msg"), None, 16, 4, "hann", True, starts, 0)
    assert torch.equal(a1, a2) and torch.equal(c1, c2) and c1[:, :, 0].tolist() == [[2] * 6] * 3
    E, W = 16, 4
    kal = _estimator(ko.make_state_dict(W, 36), E, W, smooth=2)
    starts = [0, 30, 60]
    out, _, _ = kal.process_recording(make_rows(np.random.default_rng(36), 90), starts=starts, seed=4242, spread=True)
    a1, c1, _ = kal.spectrum_recording(out, starts=starts, n=16, hop=4)
    a2, c2 = score.spectra(out, None, score.pose_cols(kal._layout, "msg"), None, 16, 4, "hann", True, starts, W + 1)
    assert torch.equal(a1, a2) and torch.equal(c1, c2) and c1[:, :, 0].tolist() == [[3] * 6] * 3       # 30 - (W + 1) = 25 frames
