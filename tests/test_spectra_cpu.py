"""Spectra of a replay (`ape_spectra`): the ABI, the numpy statement and what the host reads off the raw sums.  No GPU.

`score.spectra_numpy` + `score.summarise_spectra` are held to `scipy.signal.welch` / `csd` at 1e-12 relative (of the largest density: both
sides sum the same |rfft|^2 in float64, in different orders), to Parseval's identity, and to the spectrum of x - y for `error_psd`.

The planted low-pass: the truth is white noise of 4096 frames and the estimate its causal mean over 10 frames, H(f) =
exp(-i pi 9 f) sin(10 pi f) / (10 sin(pi f)): |H| falls to 1 / sqrt(2) at 0.04449 cycles per frame and the delay is 4.5 frames.  A Welch
estimate of 31 half-overlapping Hann segments of 256 frames at a coherence above 0.9 has a relative standard error of H of about
sqrt((1 - C) / (2 C 17)) < 6 % per bin (17 effective averages), smaller where the coherence is higher; on three seeds the statement gave a
bandwidth within 1.5 % of the analytic one, delays of 4.39 - 4.78 frames below it and |H - H_analytic| <= 0.02 up to 0.09 cycles per
frame.  The delay divides the phase by 2 pi f, so the lowest bin (f = 1 / 256) turns that bin's phase error of about 0.015 rad into
0.6 frames: that bin is held to 4.5 +- 1.8 frames, three of those standard errors; from the second bin on the same error is 0.3 frames
and falling.  Asserted, on one fixed seed: 3 %, 4.2 - 5.0 frames from the second bin up to the bandwidth, 2.7 - 6.3 at the first,
and 0.04.  These are conditions on the planted input, not on a kernel."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


def rows_of(seed, F=900, W=3):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.standard_normal((F, W)), axis=0) * 0.01 + rng.standard_normal((F, W)) * 0.05


# ---------------- 1: header and binding ----------------------------------------------------------------------------------------------------------
def test_header_declares_and_hip_binds_the_entry():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    for name, value in (("APE_SPECTRA_DETREND", "0x1u"), ("APE_SPECTRA_MAX_N", "512"), ("APE_SPECTRA_MAX_COLS", "16")):
        assert re.search(rf"^#define {name}\s+{value}\b", text, flags=re.M), name
    assert (_hip.SPECTRA_DETREND, _hip.SPECTRA_MAX_N, _hip.SPECTRA_MAX_COLS) == (1, 512, 16)
    decl = text[text.index("\nint ape_spectra(") + 1:]
    decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
    params = [" ".join(p.split()) for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
    assert len(params) == 23 and params[0] == "const void* x_dev" and params[-1] == "void* stream"
    res, args = _hip.SIGNATURES["ape_spectra"]
    assert hasattr(_hip.lib(), "ape_spectra") and res is C.c_int and len(args) == len(params)
    for p, a in zip(params, args):
        want = C.c_void_p if "*" in p else (C.c_int64 if p.startswith("int64_t") else (C.c_uint32 if p.startswith("uint32_t") else C.c_int32))
        assert a is want, (p, a)
    make = (REPO / "arm-pose-estimation_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS\s*:=(.*)$", make, flags=re.M).group(1).split()
    hazard = re.search(r"^HAZARD_SRCS\s*:=(.*)$", make, flags=re.M).group(1).split()
    assert "spectra.hip" in srcs and "spectra.hip" not in hazard
    for name in ("spectra", "spectra_numpy", "summarise_spectra", "merge_spectra", "bandwidth", "band_power", "pose_cols"):
        assert callable(getattr(score, name))
    assert score.pose_cols(0, "msg") == (4, 5, 6, 11, 12, 13) and score.pose_cols(1, "est") == (0, 1, 2, 3, 4, 5)
    import inspect
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    for cls in (Estimator, WatchPhoneUarm, WatchPhonePocketKalman):
        assert "spectrum_recording" in vars(cls)
    for fn in (Estimator.sweep_recording, Estimator.sweep_windows):
        assert inspect.signature(fn).parameters["spectra"].default is False


def test_refusals_are_made_on_the_host():
    """every refusal include/ape_hip.h states but the capturing stream: APE_ERR_INVALID_ARG before any device call (the pointers are never read)"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    x_p, y_p, acc_p, cnt_p = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20)
    taper = np.ones(512)

    def call(x=x_p, xd=_hip.F64, xss=0, xfs=25, xc=(4, 5, 6), y=None, yd=_hip.F64, yss=0, yfs=21, yc=(0, 1, 2), V=3, n_sets=1, F=100,
             starts=(0, 30, 70), R=None, skip=0, N=16, hop=8, tp=taper, flags=1, acc=acc_p, cnt=cnt_p):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        xc_, yc_ = (None if c is None else np.ascontiguousarray(c, dtype=np.int32) for c in (xc, yc))
        ptr = lambda a: None if a is None or len(a) == 0 else C.c_void_p(a.ctypes.data)       # noqa: E731
        return lib.ape_spectra(x, xd, xss, xfs, ptr(xc_), y, yd, yss, yfs, ptr(yc_), V, n_sets, F, ptr(st), len(st) if R is None else R, skip, N,
                               hop, ptr(tp), flags, acc, cnt, None)

    bad = [(dict(x=None), b"NULL"), (dict(xc=None), b"NULL"), (dict(starts=()), b"NULL"), (dict(tp=None), b"NULL"), (dict(acc=None), b"NULL"),
           (dict(cnt=None), b"NULL"), (dict(y=y_p, yc=None), b"NULL"),
           (dict(F=0), b"F=0"), (dict(R=0), b"recording starts"), (dict(R=101), b"recording starts"), (dict(starts=(1, 3)), b"seg_starts[0]"),
           (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(0, 100)), b"seg_starts[1]"), (dict(skip=-1), b"skip"),
           (dict(N=0), b"N 0"), (dict(N=24), b"N 24"), (dict(N=528), b"N 528"), (dict(N=-16), b"N -16"),
           (dict(hop=0), b"hop"), (dict(hop=17), b"hop"), (dict(hop=-1), b"hop"),
           (dict(V=0), b"V 0"), (dict(V=17), b"V 17"), (dict(n_sets=0), b"n_sets"), (dict(n_sets=65, xss=2500), b"n_sets"),
           (dict(flags=2), b"flags"), (dict(xd=2), b"dtype"), (dict(y=y_p, yd=-1), b"dtype"), (dict(xfs=0), b"frame stride"),
           (dict(xc=(4, 5, 25)), b"column offset"), (dict(xc=(-1, 5, 6)), b"column offset"), (dict(y=y_p, yc=(0, 1, 21)), b"column offset"),
           (dict(n_sets=2, xss=2499), b"overlap"), (dict(n_sets=2, xss=0), b"overlap"), (dict(n_sets=2, xss=2500, y=y_p, yss=2099), b"overlap"),
           (dict(xfs=1 << 40, xc=(4, 5, 6), F=1 << 30, starts=(0, 30, 70)), b"63 bits"), (dict(n_sets=64, xss=1 << 61), b"63 bits"),
           (dict(acc=x_p), b"overlaps x_dev"), (dict(cnt=C.c_void_p((1 << 20) + 8)), b"overlaps x_dev"),
           (dict(y=y_p, acc=C.c_void_p((2 << 20) + 16)), b"overlaps y_dev"), (dict(cnt=acc_p), b"acc_dev overlaps counts_dev")]
    for kw, word in bad:
        rc = call(**kw)
        msg = lib.ape_last_error()
        assert rc == 1 and word in msg, (kw, rc, msg)


# ---------------- 2: the statement against scipy and against identities ----------------------------------------------------------------------
@pytest.mark.parametrize("n,hop,taper", [(64, 32, "hann"), (128, 128, "boxcar"), (48, 5, "hann")])
def test_statement_agrees_with_scipy_welch_and_csd(n, hop, taper):
    signal = pytest.importorskip("scipy.signal")
    from wear_mocap_ape_amd import score
    x, y = rows_of(1), rows_of(2)
    acc, counts = score.spectra_numpy(x, y, n=n, hop=hop, taper=taper)
    s = score.summarise_spectra(acc, counts, taper, rate=50.0)
    kw = dict(fs=50.0, window=taper, nperseg=n, noverlap=n - hop, detrend="constant", scaling="density")
    for v in range(x.shape[1]):
        f, pxx = signal.welch(x[:, v], **kw)
        _, pyy = signal.welch(y[:, v], **kw)
        _, pyx = signal.csd(y[:, v], x[:, v], **kw)             # conj(Y) X: from the truth to the estimate
        assert np.allclose(f, s["freqs"], rtol=1e-15, atol=0)
        assert np.abs(s["psd"][0, v] - pxx).max() <= 1e-12 * pxx.max()
        assert np.abs(s["truth_psd"][0, v] - pyy).max() <= 1e-12 * pyy.max()
        h = s["gain"][0, v] * np.exp(1j * s["phase"][0, v])
        ref = pyx[1:] / pyy[1:]
        assert np.abs(h[1:] - ref).max() <= 1e-12 * np.abs(ref).max()
        coh = np.abs(pyx[1:]) ** 2 / (pxx[1:] * pyy[1:])
        assert np.abs(s["coherence"][0, v, 1:] - coh).max() <= 1e-12
    assert int(counts[0, 0, 0]) == (x.shape[0] - n) // hop + 1


def test_parseval_with_a_boxcar_and_no_detrend():
    from wear_mocap_ape_amd import score
    x = rows_of(3, F=640)
    n = 64
    acc, counts = score.spectra_numpy(x, n=n, hop=n, taper="boxcar", detrend=False)
    assert acc.shape == (1, 3, n // 2 + 1, 1) and (counts[0, :, 0] == 10).all()
    side = np.full(n // 2 + 1, 2.0)
    side[0] = side[-1] = 1.0
    for v in range(3):
        assert np.isclose((acc[0, v, :, 0] * side).sum() / n, (x[:, v] ** 2).sum(), rtol=1e-13, atol=0)
    s = score.summarise_spectra(acc, counts, "boxcar", rate=1.0)          # the density integrates to the mean square
    assert np.allclose(score.band_power(s, 0.0, 1.0), (x ** 2).mean(axis=0), rtol=1e-13, atol=0)


def test_error_psd_is_the_spectrum_of_the_difference():
    from wear_mocap_ape_amd import score
    x, y = rows_of(4), rows_of(5)
    s = score.summarise_spectra(*score.spectra_numpy(x, y, n=64, hop=16), "hann")
    d = score.summarise_spectra(*score.spectra_numpy(x - y, n=64, hop=16), "hann")
    top = max(s["psd"].max(), s["truth_psd"].max())
    assert np.abs(s["error_psd"] - d["psd"]).max() <= 1e-12 * top


def test_counts_and_the_left_out_pattern_on_planted_nans():
    from wear_mocap_ape_amd import score
    F, n, hop, skip = 400, 32, 8, 3
    starts = [0, 30, 31, 100, 101 + 2 * n]
    x, y = rows_of(6, F=F), rows_of(7, F=F)
    x[150, 1] = np.nan                   # recording 3 ([100, 165)): segments at 103 + 8 j; those with 103 + 8 j <= 150 < 135 + 8 j: j = 2 .. 4 of J = 4 -> j = 2, 3
    y[300, 2] = np.inf
    acc, counts = score.spectra_numpy(x, y, n=n, hop=hop, starts=starts, skip=skip)
    ends = starts[1:] + [F]
    J = [max(0, (e - s - skip - n) // hop + 1) if e - s - skip >= n else 0 for s, e in zip(starts, ends)]
    assert J == [0, 0, 5, 4, 26] and (counts.sum(axis=2) == np.asarray(J)[:, None]).all()
    assert counts[3, :, 1].tolist() == [0, 2, 0] and counts[4, :, 1].tolist() == [0, 0, 4]
    assert (acc[:2] == 0.0).all() and np.isfinite(acc).all()
    clean = score.spectra_numpy(np.nan_to_num(x), np.nan_to_num(y, posinf=0.0), n=n, hop=hop, starts=starts, skip=skip)[0]
    assert np.array_equal(acc[:, 0], clean[:, 0]) and np.array_equal(acc[3, 2], clean[3, 2])      # the other columns are untouched
    a = score.spectra_numpy(x[:165], y[:165], n=n, hop=hop, starts=starts[:4], skip=skip)
    b = score.spectra_numpy(x[165:], y[165:], n=n, hop=hop, skip=skip)
    m_acc, m_counts = score.merge_spectra((a[0][3:], a[1][3:]), (np.zeros_like(b[0]), np.zeros_like(b[1])))
    assert np.array_equal(m_acc, acc[3:4]) and np.array_equal(m_counts, counts[3:4])
    assert np.array_equal(b[0][0], acc[4]) and np.array_equal(b[1][0], counts[4])


def test_a_planted_low_pass_is_read_back():
    from wear_mocap_ape_amd import score
    F, L, n = 4096, 10, 256
    rng = np.random.default_rng(0)
    y = rng.standard_normal(F)
    c = np.concatenate([[0.0], np.cumsum(y)])
    x = (c[1:] - c[np.maximum(np.arange(F) + 1 - L, 0)]) / L
    acc, counts = score.spectra_numpy(x[:, None], y[:, None], n=n, hop=n // 2, taper="hann")
    s = score.summarise_spectra(acc, counts, "hann")
    f = s["freqs"]
    with np.errstate(all="ignore"):
        H = np.exp(-1j * np.pi * f * (L - 1)) * np.sin(np.pi * f * L) / (L * np.sin(np.pi * f))
    H[0] = 1.0
    bw = float(score.bandwidth(s)[0, 0])
    print(f"bandwidth {bw:.5f} cycles per frame (analytic 0.04449)")
    assert abs(bw - 0.04449) <= 0.03 * 0.04449
    below = (f > 1.5 / n) & (f < bw)
    delay = s["delay"][0, 0, below]
    print(f"delay from the second bin up to the bandwidth {delay.min():.3f} .. {delay.max():.3f} frames (analytic 4.5)")
    assert below.sum() >= 9 and delay.min() >= 4.2 and delay.max() <= 5.0
    first = float(s["delay"][0, 0, 1])
    print(f"delay at the first bin {first:.3f} frames (analytic 4.5, standard error 0.6)")
    assert abs(first - 4.5) <= 1.8                          # three standard errors of that bin
    upto = (f > 0) & (f <= 0.09)
    got = s["gain"][0, 0] * np.exp(1j * s["phase"][0, 0])
    print(f"max |H - H_analytic| up to 0.09 cycles per frame {np.abs(got - H)[upto].max():.4f}")
    assert np.abs(got - H)[upto].max() <= 0.04
    assert s["coherence"][0, 0, below].min() > 0.9
    assert float(score.band_power(s, 0.0, 0.51, "truth_psd")[0, 0]) == pytest.approx(1.0, rel=0.1)       # white noise of unit variance
