"""Reaches and holds, the part that needs no device: the header block and the binding of ape_segment_frames,
ape_segment_runs and ape_segment_stats, their refusals through the C ABI, the numpy statements against brute force, the stated order of
segment_stats_numpy, match_segments on hand-made tables, and the planted reach-and-hold trajectory of tests/test_post_select_cpu.py
through the statements.

tests/golden/segments_planted.npz holds the planted trajectory's labels and tables as the numpy statements give them (record() writes it);
tests/test_segments_gpu.py holds the device to it."""
import ctypes as C
import functools
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import ape_oracle as orc
from tests.test_post_select_cpu import HIPS, reach_and_hold

REPO = Path(__file__).resolve().parents[1]
FIXTURE = REPO / "tests" / "golden" / "segments_planted.npz"
PILOT = 3                                                   # the rung whose hand speed is labelled: Hann, half-width 3
EST_RULE = ((0.004, 0.008), (4, 4))                         # (lo, hi) [m/frame], (min_hold, min_move) for estimate rows
TRUTH_RULE = ((0.002, 0.004), (1, 1))                       # ... for the truth
PLANTED = [(60 + 72 * k, min(72 + 72 * k, 432)) for k in range(6)]     # the generator's reaches, [first, end)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


# ---------------- 1. the C ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_hip_binds_the_entries():
    from wear_mocap_ape_amd import _hip, score
    text = (REPO / "include" / "ape_hip.h").read_text()
    for name, value, bound in (("APE_SEGMENT_MAX_MIN", 256, _hip.SEGMENT_MAX_MIN), ("APE_SEG_TABLE_WIDTH", 4, _hip.SEG_TABLE_WIDTH),
                               ("APE_SEG_MAX_VALUES", 16, _hip.SEG_MAX_VALUES), ("APE_SEG_STAT_WIDTH", 5, _hip.SEG_STAT_WIDTH),
                               ("APE_SEG_PIECE", 1024, _hip.SEG_PIECE)):
        assert re.search(rf"^#define {name}\s+{value}\b", text, flags=re.M) and bound == value, name
    assert (score.SEGMENT_MAX_MIN, score.SEG_TABLE_WIDTH, score.SEG_MAX_VALUES, score.SEG_STAT_WIDTH, score.SEG_PIECE) == (256, 4, 16, 5, 1024)
    assert re.search(r"^#define APE_ABI_VERSION 7\s*$", text, flags=re.M) and _hip.lib().ape_abi_version() == 7 and _hip.ABI_VERSION == 7
    block = text.index("DESIGN.md 4.45")
    assert text.index("DESIGN.md 4.44") < block < text.index("int ape_segment_frames(")     # the block stands after 4.44's
    assert re.search(r"^int ape_segment_frames\(const void\* keys_dev, int32_t keys_dtype,", text, flags=re.M)
    assert re.search(r"^int ape_segment_runs\(const uint8_t\* labels_dev", text, flags=re.M)
    assert re.search(r"^int ape_segment_stats\(const void\* values_dev, int32_t values_dtype,", text, flags=re.M)
    for name, n_args in (("ape_segment_frames", 14), ("ape_segment_runs", 10), ("ape_segment_stats", 15)):
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name)
        decl = text[text.index(f"int {name}("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert len(decl.split(",")) == len(_hip.SIGNATURES[name][1]) == n_args, name
    for name in ("segment_frames", "segment_frames_numpy", "segment_runs", "segment_runs_numpy", "segment_stats", "segment_stats_numpy",
                 "match_segments", "summarise_segments"):
        assert callable(getattr(score, name))
    mk = (REPO / "arm-pose-estimation_amd" / "csrc" / "Makefile").read_text()
    assert "segments.hip" in mk.split("SRCS", 1)[1].split("\n", 1)[0]
    assert "segments.hip" not in mk.split("HAZARD_SRCS :=", 1)[1].split("\n", 1)[0]
    src = (REPO / "arm-pose-estimation_amd" / "csrc" / "segments.hip").read_text()
    assert "asm" not in src and "hipLaunchCooperativeKernel" not in src and "hipMemset" not in src
    assert "#pragma clang fp contract(off)" in src
    assert re.findall(r"atomic\w*\(", src) == ["atomicAdd("] and "atomicAdd(&lcount, 1)" in src     # one LDS counter, nothing on device memory
    from wear_mocap_ape_amd.estimate.estimator import Estimator
    from wear_mocap_ape_amd.estimate.watch_phone_pocket_kalman import WatchPhonePocketKalman
    from wear_mocap_ape_amd.estimate.watch_phone_uarm import WatchPhoneUarm
    for cls in (Estimator, WatchPhoneUarm, WatchPhonePocketKalman):
        assert callable(cls.segment_recording) and callable(cls.truth_segments)


# ---------------- 2. refusals ---------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return C.c_void_p(a.ctypes.data) if len(a) else None


def test_segment_frames_refusals_are_made_on_the_host():
    """before any device call: the device pointers are never read"""
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    dummy, far = C.c_void_p(4096), C.c_void_p(1 << 30)

    def call(keys=dummy, dtype=_hip.F64, S=2, ss=100, F=10, fs=1, starts=(0, 3, 7), R=None, th=((0.1, 0.2),), mins=((1, 1),), P=None,
             first=0, labels=far):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        t = np.ascontiguousarray(th, dtype=np.float64).reshape(-1)
        m = np.ascontiguousarray(mins, dtype=np.int32).reshape(-1)
        return lib.ape_segment_frames(keys, dtype, S, ss, F, fs, _ptr(st), len(st) if R is None else R, _ptr(t), _ptr(m),
                                      len(t) // 2 if P is None else P, first, labels, None)

    inf, nan = float("inf"), float("nan")
    bad = [(dict(keys=None), b"NULL"), (dict(labels=None), b"NULL"), (dict(starts=()), b"NULL"), (dict(th=(), P=1), b"NULL"),
           (dict(mins=()), b"NULL"), (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"),
           (dict(F=0), b"F=0"), (dict(R=0), b"recording starts"), (dict(starts=(0, 5, 5)), b"seg_starts[2]"), (dict(starts=(1, 5)), b"seg_starts[0]"),
           (dict(S=0), b"S=0"), (dict(S=65), b"S=65"), (dict(P=0), b"P=0"), (dict(P=3), b"P=3"),
           (dict(th=((0.1, 0.2), (0.3, 0.1)), mins=((1, 1), (1, 1))), b"thresholds[1]"), (dict(th=((nan, 0.2),)), b"thresholds[0]"),
           (dict(th=((0.1, inf),)), b"thresholds[0]"), (dict(th=((-inf, 0.1),)), b"thresholds[0]"),
           (dict(mins=((0, 1),)), b"mins[0][0] = 0"), (dict(mins=((1, 257),)), b"mins[0][1] = 257"), (dict(mins=((-3, 1),)), b"mins[0][0] = -3"),
           (dict(first=2), b"first_label 2"), (dict(first=-1), b"first_label -1"),
           (dict(fs=0), b"frame_stride"), (dict(ss=9), b"set_stride"), (dict(fs=12, ss=108), b"set_stride"),
           (dict(fs=2 ** 62, S=1), b"63 bits"), (dict(fs=2 ** 59, S=1), b"63 bits"),
           (dict(keys=C.c_void_p(4100)), b"aligned"), (dict(keys=C.c_void_p(4098), dtype=_hip.F32), b"aligned"),
           (dict(labels=C.c_void_p(4096 + 500)), b"overlaps")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)
        assert what in lib.ape_last_error() and b"segment_frames" in lib.ape_last_error(), (kw, lib.ape_last_error())
    if lib.ape_device_count() == 0:
        # valid arguments, no device: a loud failure (there is no CPU fallback)
        for kw in (dict(), dict(S=1, ss=0), dict(th=((0.1, 0.1),)), dict(mins=((256, 256),)), dict(first=1), dict(fs=12, ss=109, dtype=_hip.F32),
                   dict(th=((0.1, 0.2), (0.0, 0.0)), mins=((1, 1), (4, 4)))):
            assert call(**kw) != 0, kw


def test_segment_runs_refusals_are_made_on_the_host():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    lab, sof, n, tab = C.c_void_p(4096), C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p(1 << 22)

    def call(labels=lab, S=2, F=10, starts=(0, 3, 7), R=None, sof=sof, n=n, table=tab, cap=10):
        st = np.ascontiguousarray(starts, dtype=np.int32)
        return lib.ape_segment_runs(labels, S, F, _ptr(st), len(st) if R is None else R, sof, n, table, cap, None)

    bad = [(dict(labels=None), b"NULL"), (dict(n=None), b"NULL"), (dict(table=None), b"NULL"), (dict(starts=()), b"NULL"),
           (dict(F=0), b"F=0"), (dict(R=0), b"recording starts"), (dict(starts=(0, 7, 3)), b"seg_starts[2]"),
           (dict(S=0), b"S=0"), (dict(S=65), b"S=65"), (dict(cap=0), b"cap=0"), (dict(cap=-5), b"cap=-5"),
           (dict(n=C.c_void_p((1 << 21) + 2)), b"aligned"), (dict(table=C.c_void_p((1 << 22) + 1)), b"aligned"),
           (dict(sof=C.c_void_p((1 << 20) + 3)), b"aligned"),
           (dict(n=C.c_void_p(4096 + 16)), b"overlaps labels_dev"), (dict(table=C.c_void_p(4096 - 64)), b"overlaps labels_dev"),
           (dict(sof=C.c_void_p(4096 + 4)), b"overlaps labels_dev"),
           (dict(n=C.c_void_p((1 << 22) + 8)), b"two outputs overlap"), (dict(sof=C.c_void_p((1 << 21) - 40)), b"two outputs overlap"),
           (dict(sof=C.c_void_p((1 << 22) + 300)), b"two outputs overlap")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)
        assert what in lib.ape_last_error() and b"segment_runs" in lib.ape_last_error(), (kw, lib.ape_last_error())
    if lib.ape_device_count() == 0:
        for kw in (dict(), dict(sof=None), dict(cap=1), dict(S=64, F=100, cap=3)):
            assert call(**kw) != 0, kw


def test_segment_stats_refusals_are_made_on_the_host():
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    val, sof, tab, n, out = C.c_void_p(4096), C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p(1 << 22), C.c_void_p(1 << 23)

    def call(values=val, dtype=_hip.F64, vs=2, ss=100, fs=3, cs=1, V=3, S=2, F=10, sof=sof, table=tab, n=n, cap=10, out=out):
        return lib.ape_segment_stats(values, dtype, vs, ss, fs, cs, V, S, F, sof, table, n, cap, out, None)

    bad = [(dict(values=None), b"NULL"), (dict(sof=None), b"NULL"), (dict(table=None), b"NULL"), (dict(n=None), b"NULL"), (dict(out=None), b"NULL"),
           (dict(dtype=2), b"dtype"), (dict(F=0), b"F=0"), (dict(S=0), b"S=0"), (dict(S=65), b"S=65"),
           (dict(vs=0), b"0 sets of values"), (dict(vs=3), b"3 sets of values"), (dict(V=0), b"V=0"), (dict(V=17), b"V=17"),
           (dict(cap=0), b"cap=0"), (dict(fs=0), b"frame_stride 0"), (dict(cs=0), b"col_stride 0"), (dict(cs=-1), b"col_stride -1"),
           (dict(ss=29), b"set_stride"), (dict(fs=1, cs=10, ss=29), b"set_stride"), (dict(fs=2 ** 61, vs=1), b"63 bits"),
           (dict(cs=2 ** 62, vs=1), b"63 bits"),
           (dict(values=C.c_void_p(4100)), b"values_dev is not aligned"), (dict(values=C.c_void_p(4098), dtype=_hip.F32), b"values_dev is not aligned"),
           (dict(out=C.c_void_p((1 << 23) + 4)), b"aligned"), (dict(sof=C.c_void_p((1 << 20) + 2)), b"aligned"),
           (dict(out=C.c_void_p(4096 + 8)), b"overlaps"), (dict(out=C.c_void_p((1 << 20) - 8)), b"overlaps"),
           (dict(out=C.c_void_p((1 << 21) + 16)), b"overlaps"), (dict(out=C.c_void_p(1 << 22)), b"overlaps")]
    for kw, what in bad:
        rc = call(**kw)
        assert rc == 1, (kw, rc)
        assert what in lib.ape_last_error() and b"segment_stats" in lib.ape_last_error(), (kw, lib.ape_last_error())
    if lib.ape_device_count() == 0:
        for kw in (dict(), dict(vs=1, ss=0), dict(V=16, fs=16, ss=160), dict(fs=1, cs=10, ss=30), dict(dtype=_hip.F32, V=1, fs=1, ss=10)):
            assert call(**kw) != 0, kw


def test_python_refusals_without_a_device():
    from wear_mocap_ape_amd import score
    k = np.zeros((3, 8))
    for kw in (dict(thresholds=(0.2, 0.1)), dict(thresholds=(0.1, float("nan"))), dict(thresholds=((0.1, 0.2),) * 2), dict(mins=(0, 1)),
               dict(mins=(1, 257)), dict(mins=((1, 1),) * 4), dict(first_label=2), dict(thresholds=(0.1, 0.2, 0.3))):
        with pytest.raises(UserWarning):
            score.segment_frames_numpy(k, **kw)
    for call in (lambda: score.segment_frames(k), lambda: score.segment_runs(k.astype(np.uint8)), lambda: score.segment_stats(k, k, k, k),
                 lambda: score.match_segments(np.zeros((2, 3)), np.zeros((2, 4))),
                 lambda: score.summarise_segments(np.zeros((2, 4)), np.zeros((2, 3, 5)), ["a"])):
        with pytest.raises(UserWarning):
            call()


# ---------------- 3. the statements against brute force ---------------------------------------------------------------------------------------
def _brute_labels(keys, lo, hi, min_hold, min_move, starts, first_label):
    """an independent statement for one set: the last decisive frame found by searching backwards, the two minimum-length steps as
    substitutions on each recording's string of labels"""
    F = keys.shape[0]
    out = np.zeros(F, dtype=np.uint8)
    for a, b in zip(starts, list(starts[1:]) + [F]):
        s = []
        for f in range(a, b):
            lab = first_label
            for g in range(f, a - 1, -1):
                if keys[g] > hi or keys[g] <= lo:
                    lab = 1 if keys[g] > hi else 0
                    break
            s.append(str(lab))
        s = "".join(s)
        s = re.sub(r"(?<=1)0+(?=1)", lambda m: ("1" if len(m.group()) < min_hold else "0") * len(m.group()), s)
        s = re.sub(r"1+", lambda m: ("0" if len(m.group()) < min_move else "1") * len(m.group()), s)
        out[a:b] = [int(c) for c in s]
    return out


def test_segment_frames_numpy_equals_brute_force():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(45)
    specials = np.array([np.nan, np.inf, -np.inf, 0.5, 0.25])
    seen = set()
    for case in range(240):
        F = int(rng.integers(1, 90)) if case % 8 else int(rng.integers(500, 700))
        R = int(rng.integers(1, min(F, 4) + 1))
        starts = [0] + sorted(rng.choice(np.arange(1, F), size=R - 1, replace=False).tolist()) if R > 1 else [0]
        lo = 0.25
        hi = lo if case % 3 == 0 else 0.5
        mins = [(1, 1), (256, 256), (1, 256), (256, 1)][case % 4] if case % 5 == 0 else tuple(int(m) for m in rng.integers(1, 8, size=2))
        first = case % 2
        # slow keys, so that runs of every length up to the minimum occur; then NaN, infinities and the thresholds themselves
        keys = 0.375 + 0.3 * np.sin(np.cumsum(rng.normal(size=F)) * 0.5) + 0.05 * rng.normal(size=F)
        hit = rng.random(F) < 0.15
        keys[hit] = rng.choice(specials, size=int(hit.sum()))
        if case % 2:
            keys = keys.astype(np.float32)
        got = score.segment_frames_numpy(keys, (lo, hi), mins, starts, first)
        want = _brute_labels(keys.astype(np.float64), lo, hi, mins[0], mins[1], starts, first)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (case, F, starts, mins)
        seen.add((lo == hi, first, mins in ((1, 1), (256, 256))))
    assert len(seen) == 8
    # sets with a rule each equal the sets one by one; one rule serves every set
    keys = rng.random((3, 70))
    th, mn = [(0.2, 0.6), (0.5, 0.5), (0.1, 0.9)], [(1, 1), (3, 2), (5, 7)]
    both = score.segment_frames_numpy(keys, th, mn, [0, 33], 1)
    for s in range(3):
        assert np.array_equal(both[s], score.segment_frames_numpy(keys[s], th[s], mn[s], [0, 33], 1))
    assert np.array_equal(score.segment_frames_numpy(keys, th[1], mn[1], [0, 33])[2], score.segment_frames_numpy(keys[2], th[1], mn[1], [0, 33]))
    # an all-NaN recording takes first_label, and the minimum length then applies to it
    assert score.segment_frames_numpy(np.full(5, np.nan), first_label=1).tolist() == [1] * 5
    assert score.segment_frames_numpy(np.full(5, np.nan), mins=(1, 6), first_label=1).tolist() == [0] * 5


def test_segment_runs_numpy_equals_groupby():
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(46)
    for case in range(60):
        F = int(rng.integers(1, 120))
        R = int(rng.integers(1, min(F, 5) + 1))
        starts = [0] + sorted(rng.choice(np.arange(1, F), size=R - 1, replace=False).tolist()) if R > 1 else [0]
        lab = rng.choice(np.array([0, 1, 7, 255], dtype=np.uint8), size=F, p=[0.4, 0.4, 0.1, 0.1])
        lab = np.repeat(lab, rng.integers(1, 4, size=F))[:F]
        rec = np.searchsorted(starts, np.arange(F), side="right") - 1
        want, f = [], 0
        for (r, v), grp in itertools.groupby(zip(rec.tolist(), lab.tolist())):
            n = len(list(grp))
            want.append((r, f, n, v))
            f += n
        sof, n, table = score.segment_runs_numpy(lab, starts)
        assert n == len(want) and table.dtype == np.int32 and table.tolist() == [list(w) for w in want]
        assert sof.dtype == np.int32 and sof.tolist() == [i for i, w in enumerate(want) for _ in range(w[2])]
    sof, n, tables = score.segment_runs_numpy(np.array([[0, 1, 1], [5, 5, 5]]), [0, 2])
    assert n.tolist() == [3, 2] and tables[0].tolist() == [[0, 0, 1, 0], [0, 1, 1, 1], [1, 2, 1, 1]] and tables[1].tolist() == [[0, 0, 2, 5], [1, 2, 1, 5]] and sof.tolist() == [[0, 1, 2], [0, 0, 1]]


def _plain(x):
    s = 0.0
    for v in x.tolist():
        s = s + v
    return s


def test_segment_stats_numpy_sums_piece_by_piece():
    """The order is part of the contract.  In a segment of 1025 frames the second piece is one value, and adding it as a piece or as the
    1025th term is the same addition: the two orders cannot differ there, and the statement is held to both.  From 1026 frames on they
    can: a segment of 1030 frames whose plain left-to-right sum differs from the piecewise one in the last bit must give the piecewise."""
    from wear_mocap_ape_amd import score
    rng = np.random.default_rng(47)
    found = None
    for _ in range(200):
        x = rng.random(1030) + 0.5
        piecewise = (0.0 + _plain(x[:1024])) + _plain(x[1024:])
        if piecewise != _plain(x) and abs(piecewise - _plain(x)) <= 2 * np.spacing(piecewise):
            found = x
            break
    assert found is not None                                # numpy shows the two orders differ: the test can tell them apart
    x = found
    table = np.array([[0, 3, 1030, 1]], dtype=np.int32)
    vals = np.concatenate([rng.random(3), x, rng.random(5)])
    got = score.segment_stats_numpy(vals, table)
    assert got.shape == (1, 1, 5)
    assert got[0, 0, 1] == (0.0 + _plain(x[:1024])) + _plain(x[1024:]) and got[0, 0, 1] != _plain(x)
    assert got[0, 0, 2] == (0.0 + _plain(x[:1024] * x[:1024])) + _plain(x[1024:] * x[1024:])
    assert got[0, 0, 0] == 1030 and got[0, 0, 3] == x.max() and got[0, 0, 4] == 3 + int(np.argmax(x))
    # 1025 frames: piecewise == plain, and the statement gives it; up to 1024 frames it is the plain sum
    for n in (1, 1024, 1025):
        got = score.segment_stats_numpy(vals, np.array([[0, 2, n, 0]]))
        seg = vals[2:2 + n]
        assert got[0, 0, 1] == _plain(seg) and got[0, 0, 2] == _plain(seg * seg)
    # pieces count from the segment's first frame, not from the batch's tiles: the same values elsewhere give the same bits
    moved = score.segment_stats_numpy(np.concatenate([rng.random(1000), x]), np.array([[0, 1000, 1030, 1]]))
    assert np.array_equal(moved[0, 0, :4], score.segment_stats_numpy(vals, table)[0, 0, :4]) and moved[0, 0, 4] == 1000 + int(np.argmax(x))
    # NaN is left out of its own cell only, infinities follow IEEE, the first of two maxima is named, float32 is widened
    v = np.array([[1.0, np.nan], [np.nan, np.nan], [3.0, np.nan], [3.0, np.nan], [-np.inf, 2.0], [np.inf, 2.0], [-np.inf, 2.0]], dtype=np.float32)
    got = score.segment_stats_numpy(v, np.array([[0, 0, 4, 0], [0, 4, 1, 1], [0, 5, 2, 0]]))
    assert got[0, 0].tolist() == [3.0, 7.0, 19.0, 3.0, 2.0] and got[0, 1].tolist() == [0.0, 0.0, 0.0, -np.inf, -1.0]
    assert got[1, 0].tolist() == [1.0, -np.inf, np.inf, -np.inf, 4.0] and got[1, 1].tolist() == [1.0, 2.0, 4.0, 2.0, 4.0]
    zero = score.segment_stats_numpy(np.array([-1.0, -0.0, 0.0, -0.0]), np.array([[0, 0, 4, 0], [0, 2, 2, 0]]))
    assert zero[0, 0, 4] == 1 and np.signbit(zero[0, 0, 3]) and zero[1, 0, 4] == 2 and not np.signbit(zero[1, 0, 3])     # the value at that frame
    assert got[2, 0, 0] == 2 and np.isnan(got[2, 0, 1]) and got[2, 0, 2] == np.inf and got[2, 0, 3] == np.inf and got[2, 0, 4] == 5


# ---------------- 4. matching -----------------------------------------------------------------------------------------------------------------
def _table(rows):
    """(recording, first, end, label) -> table rows"""
    return np.array([[r, a, b - a, lab] for r, a, b, lab in rows], dtype=np.int32)


def test_match_segments_missed_spurious_and_ties():
    from wear_mocap_ape_amd import score
    truth = _table([(0, 0, 10, 0), (0, 10, 20, 1), (0, 20, 40, 0), (0, 40, 50, 1), (0, 50, 70, 0), (0, 70, 80, 1), (0, 80, 100, 0),
                    (1, 100, 110, 0), (1, 110, 120, 1), (1, 120, 130, 0)])
    est = _table([(0, 0, 12, 0), (0, 12, 15, 1), (0, 15, 17, 0), (0, 17, 20, 1), (0, 20, 60, 0), (0, 60, 64, 1), (0, 64, 69, 0),
                  (0, 69, 83, 1), (0, 83, 100, 0), (1, 100, 130, 0)])
    m = score.match_segments(est, truth)
    # truth move 1 overlaps two estimate moves in three frames each: the earlier one; move 3 has none; the estimate's row 5 matches nothing;
    # recording 1's move has no partner in its own recording
    assert m["pairs"] == [(1, 1), (5, 7)] and (m["matched"], m["missed"], m["spurious"]) == (2, 2, 2)
    assert m["missed_rows"] == [3, 8] and m["spurious_rows"] == [3, 5]
    assert m["onset"].tolist() == [2, -1] and m["offset"].tolist() == [-5, 3] and "onset_s" not in m
    # a lag moves the estimate: 17..20 at lag 3 is 14..17 against the truth, still 3 frames, and 12..15 becomes 9..12: 2 frames
    m3 = score.match_segments(est, truth, lag=3)
    assert m3["pairs"][0] == (1, 3) and m3["onset"][0] == 4 and m3["offset"][0] == -3
    # an estimate move in another recording is never taken, however well it overlaps
    other = est.copy()
    other[:, 0] = 1
    m1 = score.match_segments(other, truth)
    assert (m1["matched"], m1["missed"], m1["spurious"]) == (0, 4, 4)
    # the holds, and seconds on a clock
    holds = score.match_segments(est, truth, label=0, times=np.arange(130) * 0.01)
    assert holds["pairs"] == [(0, 0), (2, 4), (4, 6), (6, 8), (7, 9)] and holds["missed"] == 1 and holds["spurious"] == 1
    assert np.allclose(holds["onset_s"], 0.01 * holds["onset"]) and np.allclose(holds["offset_s"], 0.01 * holds["offset"])
    # a move is matched once: the second truth move that overlaps only a taken one is missed
    m = score.match_segments(_table([(0, 0, 30, 1)]), _table([(0, 0, 10, 1), (0, 10, 12, 0), (0, 12, 30, 1)]))
    assert m["pairs"] == [(0, 0)] and m["missed_rows"] == [2] and m["spurious"] == 0


def test_summarise_segments():
    from wear_mocap_ape_amd import score
    table = _table([(0, 0, 4, 0), (0, 4, 6, 1), (0, 6, 10, 0), (1, 10, 13, 1)])
    vals = np.arange(13, dtype=np.float64)[:, None] * np.array([1.0, -1.0])
    vals[10:13, 1] = np.nan
    stats = score.segment_stats_numpy(vals, table)
    res = score.summarise_segments(table, stats, ["up", "down"])
    assert [(d["recording"], d["label"], d["count"]) for d in res] == [(0, 0, 2), (0, 1, 1), (1, 1, 1)]
    assert res[0]["mean_duration"] == 4.0 and res[0]["longest_duration"] == 4.0 and res[0]["mean"]["up"] == (1.5 + 7.5) / 2 and res[0]["max"]["up"] == 9.0
    assert res[0]["max"]["down"] == 0.0 and res[2]["mean"]["up"] == 11.0 and np.isnan(res[2]["mean"]["down"]) and np.isnan(res[2]["max"]["down"])
    timed = score.summarise_segments(table, stats, ["up", "down"], times=np.arange(13) * 0.5)
    assert timed[0]["mean_duration"] == 1.5 and timed[1]["longest_duration"] == 0.5


# ---------------- 5. the planted trajectory ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def planted_numpy():
    """the reach-and-hold trajectory of tests/test_post_select_cpu.py through the numpy statements -> a dict: the labels and tables of the
    pilot rung (est), of the unsmoothed rung (raw) and of the truth"""
    from wear_mocap_ape_amd import score
    y, truth, _ = reach_and_hold()
    windows, _ = score.ladder(samples=y.shape[1])
    out, _ = score.post_window_numpy(y, np.zeros(14), np.ones(14), orc.DEFAULT_BODY, HIPS, [0], [windows[0], windows[PILOT]])
    res = {}
    for name, rows, kind, (th, mins) in (("raw", out[0], "msg", EST_RULE), ("est", out[1], "msg", EST_RULE), ("truth", truth, "est", TRUTH_RULE)):
        speed = score.motion_sums_numpy(rows, HIPS, kind, [0])[0][:, 0]
        labels = score.segment_frames_numpy(speed, th, mins, [0])
        res[name + "_labels"], res[name + "_table"] = labels, score.segment_runs_numpy(labels, [0])[2]
    return res


def record(path=FIXTURE):
    p = planted_numpy()
    np.savez_compressed(path, **{k: p[k] for k in ("est_labels", "est_table", "truth_labels", "truth_table")})


def test_the_planted_reaches_are_found_through_the_pilot_rung():
    from wear_mocap_ape_amd import score
    p = planted_numpy()
    moves = lambda t: [(int(a), int(a + n)) for _, a, n, lab in t if lab == 1]
    print("planted reach-and-hold trajectory, moves [first, end):")
    for name in ("truth", "est", "raw"):
        print(f"  {name:5s}: {moves(p[name + '_table'])}")
    # the truth's own hand speed finds the generator's reaches (a reach's last step arrives at the pose: one frame past the planted end)
    assert len(moves(p["truth_table"])) == 6
    for (a, b), (pa, pb) in zip(moves(p["truth_table"]), PLANTED):
        assert abs(a - pa) <= 1 and pb <= b <= pb + 1
    m = score.match_segments(p["est_table"], p["truth_table"])
    print(f"  matched {m['matched']}, missed {m['missed']}, spurious {m['spurious']}, onset {m['onset'].tolist()}, offset {m['offset'].tolist()}")
    assert (m["matched"], m["missed"], m["spurious"]) == (6, 0, 0)
    assert np.abs(m["onset"]).max() <= 2 and np.abs(m["offset"]).max() <= 2
    # the unsmoothed rows at the same settings: noise keeps the hand speed above the thresholds, and the reaches run together
    assert len(moves(p["raw_table"])) < 6
    # the fixture the GPU file holds the device to is what the statements give
    with np.load(FIXTURE) as z:
        for k in ("est_labels", "est_table", "truth_labels", "truth_table"):
            assert np.array_equal(z[k], p[k]), k
