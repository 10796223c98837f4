"""Scoring and post-filter calls in flight: the staging contract of include/ape_hip.h on the GPU.

Every device entry since `ape_score_rows` promises that "the launches go on `stream` and the call does not wait for them" and that "the
host arrays have been consumed when it returns", with the mechanics beside it: up to 8 calls in flight per device, one more waits for
the oldest, a slot is taken again once the event behind its last call has completed, and the post-filter's one workspace per device
orders a call on another stream behind its last user.  A test that makes one call, synchronises and compares values sees none of
this.  Here every case is ONE deterministic arrangement behind a bounded blocker -- ordinary torch work (matrix products) enqueued on the
call's stream, its length calibrated with events, an event `done` behind it:

(a) per entry: the call is made behind the blocker with host arrays the test owns; `done.query()` must still be false when it returns
    (else the call waited for the stream), then every host array is overwritten in place with ANOTHER VALID argument of the same shape
    (a late read shows as different bits, never as an index out of range), and after one synchronise the outputs hold the bytes of the
    same call made alone.  Each poisoned array is first shown, alone, to change the bytes -- otherwise the case would prove nothing.
(b) 12 calls of different sizes round robin on three streams behind three blockers, for the three pools whose slot carries device
    scratch from a call's first launch to its second: every output has the bytes of its call made alone, and when the ninth call
    returns the first has completed ("one more waits for the oldest").
(c) the shared post-filter workspace: a sweep on an idle stream stays behind a window call that is behind a blocker on another stream.

A case whose blocker had already ended when the call under test was made, or came out shorter than required, is inconclusive and
FAILS with that word; it does not pass.  Nothing here can fault the GPU: every argument, poisoned or not, is a valid one.
The C ABI is called through `_hip.lib()` so that the test, not a wrapper, owns the host arrays."""
import ctypes as C
import json
import math
import time
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
F, R, M, O = 600, 3, 4, 14                               # frames (three 256-frame workgroups), recordings, samples, targets
STARTS, STARTS_P = [0, 190, 417], [0, 233, 380]           # the recordings' first frames, and the poison's
LAYOUT = 0                                               # APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS
F64, FLAG_SPREAD = 1, 0x40
TRUTH_TARGETS, TRUTH_EST, ROWS_EST, ROWS_TARGETS, ROT_MSG = 0, 1, 1, 2, 0
NW = 64                                                  # APE_POST_MAX_WINDOW
MIN_BLOCKER, TIMES_CALL = 0.050, 100                     # the blocker: at least 50 ms and 100 host durations of the call
BODY = np.array([-0.22, 0.0, 0.0, -0.26, 0.0, 0.0, -0.1704612, 0.4309841, -0.00670862])


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _host(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _sp(stream):
    return C.c_void_p(stream.cuda_stream)


def _snap(outs):
    """the bytes of a call's outputs (after a synchronise)"""
    return b"".join(t.cpu().numpy().tobytes() for t in outs)


def _i32(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _f64(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64))


def _taper(rows):
    """weights [len(rows), 64]: the first n entries of row c are rows[c] divided by its sum (they sum to 1 well within the entry's 1e-9)"""
    w = np.zeros((len(rows), NW))
    for c, shape in enumerate(rows):
        v = np.asarray(shape, dtype=np.float64)
        v = v / v.sum()
        w[c, :len(v)] = v
    return w


class Blocker:
    """Bounded torch work on a stream: products of two 4096 x 4096 float32 matrices, as many as the wanted length takes by a calibration
    with events, never more than MAX_PRODUCTS."""
    MAX_PRODUCTS = 4000

    def __init__(self, streams):
        g = torch.Generator(device="cuda").manual_seed(7)
        self.a = torch.randn((4096, 4096), device="cuda", generator=g)
        self.b = torch.randn((4096, 4096), device="cuda", generator=g)
        self.c = {s.cuda_stream: torch.empty((4096, 4096), device="cuda") for s in streams}
        for s in streams:                                   # (the BLAS workspace of every stream, before anything is timed)
            with torch.cuda.stream(s):
                for _ in range(3):
                    torch.mm(self.a, self.b, out=self.c[s.cuda_stream])
        torch.cuda.synchronize()
        s = streams[0]
        with torch.cuda.stream(s):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(40):
                torch.mm(self.a, self.b, out=self.c[s.cuda_stream])
            t1.record()
        torch.cuda.synchronize()
        self.per_product = t0.elapsed_time(t1) / 1e3 / 40

    def enqueue(self, stream, seconds):
        """-> (start, done, products): events around the work; 1.5 times the products the calibration asks for"""
        n = min(self.MAX_PRODUCTS, int(math.ceil(1.5 * seconds / self.per_product)) + 1)
        with torch.cuda.stream(stream):
            start, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(n):
                torch.mm(self.a, self.b, out=self.c[stream.cuda_stream])
            done.record()
        return start, done, n


class Entry:
    """One entry's smallest call that uses every host array it takes: `host` / `poison` name -> numpy array (same shape and dtype, both
    valid), `outs()` fresh zeroed outputs, `call(h, outs, stream) -> status`.  `inert`: host arrays that are staged but whose values
    cannot reach this call's outputs (they are poisoned like the rest and left out of the one-by-one proof)."""

    def __init__(self, name, host, poison, outs, call, inert=()):
        assert set(host) == set(poison) and all(host[k].shape == poison[k].shape and host[k].dtype == poison[k].dtype for k in host), name
        self.name, self.host, self.poison, self.outs, self.call, self.inert = name, host, poison, outs, call, tuple(inert)

    def fresh(self, poisoned=()):
        return {k: (self.poison[k] if k in poisoned else v).copy() for k, v in self.host.items()}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as entry
    entry.build()


@pytest.fixture(scope="module")
def world():
    """streams, the blocker, the model handle of the post-filter and the device arrays every case reads; made once, never written again"""
    from oracle import ape_oracle as orc
    from wear_mocap_ape_amd import _hip
    from wear_mocap_ape_amd.estimate import nn_models
    torch.cuda.set_device(0)
    lib = _hip.lib()
    cfg = orc.MODEL_CONFIGS["pocket"]
    assert cfg["O"] == O and cfg["layout"] == LAYOUT
    model = nn_models.DropoutLSTM(cfg["I"], cfg["H"], cfg["L"], cfg["O"], device=0)
    model.load_state_dict(orc.make_state_dict(cfg["I"], cfg["H"], cfg["L"], cfg["O"], seed=0))
    raw = json.loads((REPO / "tests" / "golden" / "norm_stats.json").read_text())["pocket"]
    model.set_norm_stats(*(np.array(raw[k]) for k in ("xx_m", "xx_s", "yy_m", "yy_s")))
    model.set_body(orc.DEFAULT_BODY)

    rng = np.random.default_rng(0xF117)
    big = 1100                                             # (b) takes slices of up to 1100 frames of the same arrays

    def unit(n):
        q = rng.normal(size=(n, 4))
        return q / np.linalg.norm(q, axis=1, keepdims=True)

    msg = rng.normal(size=(big, 25)) * 0.3
    for c in (0, 7, 14, 21):
        msg[:, c:c + 4] = unit(big)
    est = rng.normal(size=(big, 21)) * 0.3
    for c in (9, 13, 17):
        est[:, c:c + 4] = unit(big)
    spread = np.abs(rng.normal(size=(big, 21))) * 0.01
    for k in (0, 9):                                       # usable covariances: diagonal-dominant xx xy xz yy yz zz behind each mean
        spread[:, k + 3], spread[:, k + 6], spread[:, k + 8] = spread[:, k + 3] + 0.05, spread[:, k + 6] + 0.05, spread[:, k + 8] + 0.05
    f = np.arange(big)
    keys = np.stack([np.abs(np.sin(f / 17.0 + s)) + 0.05 * rng.normal(size=big) for s in range(2)])
    keys[:, 50:60], keys[:, 60:64], keys[:, 64:74] = 1.0, 0.0, 1.0          # a hold of 4 frames between two moves: the minimum hold decides it
    keys[:, 100:110], keys[:, 110:113], keys[:, 113:123] = 0.0, 1.0, 0.0     # a move of 3 frames between two holds: the minimum move does
    for b in STARTS[1:] + STARTS_P[1:]:                    # a fast stretch up to every boundary and an undecided one behind it: whether frame b
        keys[:, b - 6:b], keys[:, b:b + 8] = 1.0, 0.5      # starts a recording decides its label (segment_frames) and its cap (select_rungs)
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()       # noqa: E731
    w = {
        "lib": lib, "model": model, "handle": model.handle,
        "idle": torch.cuda.Stream(), "sides": [torch.cuda.Stream() for _ in range(3)],
        "msg": dev(msg), "est": dev(est), "spread": dev(spread), "tgt": dev(rng.normal(size=(big, O))),
        "y": dev(rng.normal(size=(big, M, O)), torch.float32), "y2": dev(rng.normal(size=(big, M, O)), torch.float32),
        "keys": dev(keys), "dt": dev(0.02 + 0.005 * rng.random(big)), "values": dev(rng.normal(size=(big, 3))),
        "sel": dev(rng.integers(0, 2, size=(2, big)), torch.uint8), "labels": dev(keys > 0.5, torch.uint8),
        "report": [],
    }
    w["blocker"] = Blocker(w["sides"] + [w["idle"]])
    torch.cuda.synchronize()
    print(f"\nblocker: {w['blocker'].per_product * 1e3:.3f} ms per 4096^3 float32 product")
    yield w
    print("\n" + "\n".join(w["report"]))


# ---- the entries of (a) ------------------------------------------------------------------------------------------------------------------
def _entries(w):
    lib, hd = w["lib"], w["handle"]
    msg, est, spread, tgt, y, values, dt = (w[k][:F].contiguous() for k in ("msg", "est", "spread", "tgt", "y", "values", "dt"))
    keys, sel, labels = (w[k][:, :F].contiguous() for k in ("keys", "sel", "labels"))
    Z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")      # noqa: E731
    bodies = _f64([BODY * (1.0 + 0.1 * r) for r in range(R)])
    common = {"starts": _i32(STARTS), "bodies": bodies}
    common_p = {"starts": _i32(STARTS_P), "bodies": bodies * 1.5}
    lags, lags_p = {"rec_lag": _i32([1, -2, 0])}, {"rec_lag": _i32([0, 1, -1])}
    trims, trims_p = {"trim": _i32([[1, 2], [0, 3], [4, 0]])}, {"trim": _i32([[2, 0], [5, 1], [0, 6]])}
    L = 6                                                   # lags -2 .. 3
    windows = {"windows": _i32([[3, 3, 4], [2, 0, 2]]), "weights": _taper([[1, 2, 3, 4, 3, 2, 1], [1, 2, 3]])}
    windows_p = {"windows": _i32([[2, 4, 3], [1, 1, 1]]), "weights": _taper([[1, 4, 6, 8, 6, 4, 1], [3, 2, 1]])}    # the same frames per window
    E = []

    E.append(Entry("ape_score_rows", dict(common), dict(common_p), lambda: [Z(F, 7), Z(R, 25)],
                   lambda h, o, s: lib.ape_score_rows(LAYOUT, _ptr(msg), 25, _ptr(spread), 21, F64, _ptr(tgt), TRUTH_TARGETS, F64, F, _host(h["starts"]), R, 2,
                                                      _host(h["bodies"]), R, _ptr(o[0]), F64, _ptr(o[1]), _sp(s))))
    E.append(Entry("ape_score_lags", {**common, **lags}, {**common_p, **lags_p}, lambda: [Z(F, L, 7), Z(R, L, 25)],
                   lambda h, o, s: lib.ape_score_lags(LAYOUT, _ptr(msg), 25, _ptr(spread), 21, F64, _ptr(tgt), TRUTH_TARGETS, F64, F, _host(h["starts"]), R, 2,
                                                      _host(h["bodies"]), R, -2, 3, _host(h["rec_lag"]), _ptr(o[0]), F64, _ptr(o[1]), _sp(s))))
    E.append(Entry("ape_post_sweep", {**common, "configs": _i32([[3, 4], [1, 2], [7, 1]])}, {**common_p, "configs": _i32([[2, 4], [4, 2], [5, 3]])},
                   lambda: [Z(3, F, 46)],
                   lambda h, o, s: lib.ape_post_sweep(hd, _ptr(y), F, M, _host(h["starts"]), R, _host(h["configs"]), 3, FLAG_SPREAD, _host(h["bodies"]), R,
                                                      _ptr(o[0]), F64, 0, _sp(s))))
    E.append(Entry("ape_post_window", {**common, **windows}, {**common_p, **windows_p}, lambda: [Z(2, F, 46)],
                   lambda h, o, s: lib.ape_post_window(hd, _ptr(y), F, M, _host(h["starts"]), R, _host(h["windows"]), _host(h["weights"]), 2, FLAG_SPREAD,
                                                       _host(h["bodies"]), R, _ptr(o[0]), F64, 0, _sp(s))))
    E.append(Entry("ape_post_select", {**common, **windows}, {**common_p, **windows_p}, lambda: [Z(2, F, 46)],
                   lambda h, o, s: lib.ape_post_select(hd, _ptr(y), F, M, _host(h["starts"]), R, _host(h["windows"]), _host(h["weights"]), 2, _ptr(sel), 2,
                                                       FLAG_SPREAD, _host(h["bodies"]), R, _ptr(o[0]), F64, 0, _sp(s))))
    E.append(Entry("ape_select_rungs",
                   {"starts": _i32(STARTS), "edges": _f64([0.3, 0.6, 0.85]), "rung_of_slot": _i32([2, 1, 0, 0]), "reach": _i32([0, 2, 5])},
                   {"starts": _i32(STARTS_P), "edges": _f64([0.2, 0.5, 0.75]), "rung_of_slot": _i32([2, 2, 1, 0]), "reach": _i32([0, 1, 3])},
                   lambda: [Z(2, F, dtype=torch.uint8)],
                   lambda h, o, s: lib.ape_select_rungs(_ptr(keys), F64, 2, F, F, 1, _host(h["starts"]), R, _host(h["edges"]), 3, _host(h["rung_of_slot"]), 1,
                                                        _host(h["reach"]), 3, 2, _ptr(o[0]), _sp(s))))
    E.append(Entry("ape_segment_frames",
                   {"starts": _i32(STARTS), "thresholds": _f64([[0.4, 0.6]]), "mins": _i32([[3, 2]])},
                   {"starts": _i32(STARTS_P), "thresholds": _f64([[0.25, 0.75]]), "mins": _i32([[7, 5]])},
                   lambda: [Z(2, F, dtype=torch.uint8)],
                   lambda h, o, s: lib.ape_segment_frames(_ptr(keys), F64, 2, F, F, 1, _host(h["starts"]), R, _host(h["thresholds"]), _host(h["mins"]), 1, 0,
                                                          _ptr(o[0]), _sp(s))))
    E.append(Entry("ape_segment_runs", {"starts": _i32(STARTS)}, {"starts": _i32(STARTS_P)},
                   lambda: [Z(2, F, dtype=torch.int32), Z(2, dtype=torch.int32), Z(2, F, 4, dtype=torch.int32)],
                   lambda h, o, s: lib.ape_segment_runs(_ptr(labels), 2, F, _host(h["starts"]), R, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), F, _sp(s))))
    # (ape_segment_stats takes device arrays alone: what ape_segment_runs wrote for the same labels)
    runs = [Z(2, F, dtype=torch.int32), Z(2, dtype=torch.int32), Z(2, F, 4, dtype=torch.int32)]
    assert lib.ape_segment_runs(_ptr(labels), 2, F, _host(_i32(STARTS)), R, _ptr(runs[0]), _ptr(runs[1]), _ptr(runs[2]), F, _sp(w["idle"])) == 0
    torch.cuda.synchronize()
    E.append(Entry("ape_segment_stats", {}, {}, lambda: [Z(2, F, 3, 5)],
                   lambda h, o, s: lib.ape_segment_stats(_ptr(values), F64, 1, 0, 3, 1, 3, 2, F, _ptr(runs[0]), _ptr(runs[2]), _ptr(runs[1]), F, _ptr(o[0]),
                                                         _sp(s))))
    E.append(Entry("ape_frame_sums", {**common, **lags}, {**common_p, **lags_p}, lambda: [Z(R, L, 51)],
                   lambda h, o, s: lib.ape_frame_sums(LAYOUT, _ptr(msg), 25, F64, _ptr(tgt), TRUTH_TARGETS, F64, F, _host(h["starts"]), R, 2, _host(h["bodies"]), R,
                                                      -2, 3, _host(h["rec_lag"]), _ptr(o[0]), _sp(s))))
    E.append(Entry("ape_rotate_rows", {"starts": _i32(STARTS), "quats": _f64([[1, 0.1, 0.2, 0.3], [0.5, -0.5, 0.4, 0.1], [0.2, 0.9, 0.0, -0.3]])},
                   {"starts": _i32(STARTS_P), "quats": _f64([[0.3, 0.2, -0.7, 0.1], [1.0, 0.0, 0.3, 0.0], [0.6, 0.1, 0.1, 0.8]])},
                   lambda: [Z(F, 46)],
                   lambda h, o, s: lib.ape_rotate_rows(LAYOUT, _ptr(msg), 25, _ptr(spread), 21, F64, F, _host(h["starts"]), R, _host(h["quats"]), R, _ptr(o[0]),
                                                       F64, _sp(s))))
    E.append(Entry("ape_frame_times", {"starts": _i32(STARTS)}, {"starts": _i32(STARTS_P)}, lambda: [Z(F)],
                   lambda h, o, s: lib.ape_frame_times(_ptr(dt), 1, F64, 0, F, _host(h["starts"]), R, _ptr(o[0]), _sp(s))))
    E.append(Entry("ape_resample_truth",
                   {**common, "truth_starts": _i32([0, 200, 405]), "shift": _f64([0.25, -0.5, 1.75])},
                   {**common_p, "truth_starts": _i32([0, 180, 420]), "shift": _f64([0.5, 0.25, -1.25])},
                   lambda: [Z(F, 21)],
                   lambda h, o, s: lib.ape_resample_truth(LAYOUT, _ptr(tgt), TRUTH_TARGETS, F64, F, _host(h["truth_starts"]), None, None, F, _host(h["starts"]), R,
                                                          _host(h["shift"]), 0.0, _host(h["bodies"]), R, _ptr(o[0]), F64, _sp(s))))
    E.append(Entry("ape_body_sums", {"starts": _i32(STARTS), **lags}, {"starts": _i32(STARTS_P), **lags_p}, lambda: [Z(R, L, 46)],
                   lambda h, o, s: lib.ape_body_sums(LAYOUT, _ptr(msg), 25, F64, _ptr(est), TRUTH_EST, F64, F, _host(h["starts"]), R, 2, ROT_MSG, -2, 3,
                                                     _host(h["rec_lag"]), _ptr(o[0]), _sp(s))))
    E.append(Entry("ape_rebody_rows", dict(common), dict(common_p), lambda: [Z(F, 25)],
                   lambda h, o, s: lib.ape_rebody_rows(LAYOUT, _ptr(msg), 25, F64, F, _host(h["starts"]), R, _host(h["bodies"]), R, _ptr(o[0]), F64, _sp(s))))
    E.append(Entry("ape_motion_sums", dict(common), dict(common_p), lambda: [Z(1, F, 12), Z(1, R, 38)],
                   lambda h, o, s: lib.ape_motion_sums(LAYOUT, _ptr(tgt), ROWS_TARGETS, O, F64, 1, 0, F, _host(h["starts"]), R, 2, None, _host(h["bodies"]), R,
                                                       _ptr(o[0]), F64, _ptr(o[1]), _sp(s))))
    edges3 = np.stack([np.linspace(-1.5, 1.5, 5) + 0.1 * c for c in range(3)])
    E.append(Entry("ape_score_hist", {"starts": _i32(STARTS), **trims, "edges": _f64(edges3)}, {"starts": _i32(STARTS_P), **trims_p, "edges": _f64(edges3 + 0.2)},
                   lambda: [Z(1, R, 1, 3, 7, dtype=torch.int64)],
                   lambda h, o, s: lib.ape_score_hist(_ptr(values), F64, 3, 1, 0, F, 3, 1, 0, _host(h["starts"]), R, _host(h["trim"]), _host(h["edges"]), 4,
                                                      _ptr(o[0]), _sp(s))))
    # (the rows are targets, so bodies_host is staged; the angles read the quaternions alone, which no body enters)
    E.append(Entry("ape_joint_angles", {**common, **lags}, {**common_p, **lags_p}, lambda: [Z(1, F, 7), Z(1, F, 7), Z(1, R, 71)],
                   lambda h, o, s: lib.ape_joint_angles(LAYOUT, _ptr(tgt), ROWS_TARGETS, O, F64, 1, 0, _ptr(est), ROWS_EST, 21, F64, _host(h["rec_lag"]), F,
                                                        _host(h["starts"]), R, 2, _host(h["bodies"]), R, 0.05, _ptr(o[0]), _ptr(o[1]), F64, _ptr(o[2]), _sp(s)),
                   inert=("bodies",)))
    E.append(Entry("ape_score_by", {"starts": _i32(STARTS), **trims, "edges": _f64(edges3[:2])}, {"starts": _i32(STARTS_P), **trims_p, "edges": _f64(edges3[:2] + 0.2)},
                   lambda: [Z(1, R, 2, 7, 3, 4)],
                   lambda h, o, s: lib.ape_score_by(_ptr(values), F64, 2, 0, 3, _ptr(values), F64, 3, 0, 3, 1, F, _host(h["starts"]), R, _host(h["trim"]),
                                                    _host(h["edges"]), 4, _ptr(o[0]), _sp(s))))
    return {e.name: e for e in E}


ENTRIES = ["ape_score_rows", "ape_score_lags", "ape_post_sweep", "ape_post_window", "ape_post_select", "ape_select_rungs", "ape_segment_frames",
           "ape_segment_runs", "ape_segment_stats", "ape_frame_sums", "ape_rotate_rows", "ape_frame_times", "ape_resample_truth", "ape_body_sums",
           "ape_rebody_rows", "ape_motion_sums", "ape_score_hist", "ape_joint_angles", "ape_score_by"]


def _check(w, status, what):
    assert status == 0, (what, status, w["lib"].ape_last_error().decode("utf-8", "replace"))


def _alone(w, entry, poisoned=()):
    """the bytes of the entry's call made alone on an idle stream"""
    outs = entry.outs()
    torch.cuda.synchronize()
    _check(w, entry.call(entry.fresh(poisoned), outs, w["idle"]), entry.name)
    torch.cuda.synchronize()
    return _snap(outs)


# ---- (a) consumed on return, and no wait -------------------------------------------------------------------------------------------------
def _behind_a_blocker(w, entry):
    name, side = entry.name, w["sides"][0]
    ref = _alone(w, entry)
    assert ref == _alone(w, entry), "the same call twice gives the same bytes"
    # what the poison is worth: every host array, alone and all together, changes the bytes when it is what the call is given
    for k in entry.host:
        if k not in entry.inert:
            assert _alone(w, entry, (k,)) != ref, f"{name}: the poisoned {k} alone gives the reference's bytes: it would prove nothing"
    if entry.host:
        assert _alone(w, entry, tuple(entry.host)) != ref
    # warm-up on the side stream with the same sizes, then the host duration of the call on the idle stream (no allocation is timed)
    outs = entry.outs()
    _check(w, entry.call(entry.fresh(), outs, side), name)
    torch.cuda.synchronize()
    h = entry.fresh()
    t0 = time.perf_counter()
    status = entry.call(h, outs, side)
    t_call = time.perf_counter() - t0
    torch.cuda.synchronize()
    _check(w, status, name)
    assert _snap(outs) == ref
    need = max(MIN_BLOCKER, TIMES_CALL * t_call)

    outs = entry.outs()
    h = entry.fresh()
    torch.cuda.synchronize()
    start, done, products = w["blocker"].enqueue(side, need)
    over_before = done.query()
    t0 = time.perf_counter()
    status = entry.call(h, outs, side)
    t_behind = time.perf_counter() - t0
    over_after = done.query()
    for k, a in h.items():                                  # in place: the memory the call was given now holds another valid argument
        a[...] = entry.poison[k]
    torch.cuda.synchronize()
    length = start.elapsed_time(done) / 1e3
    got = _snap(outs)
    w["report"].append(f"(a) {name}: host call {t_call * 1e6:.0f} us on an idle stream, {t_behind * 1e6:.0f} us behind a blocker of {length * 1e3:.1f} ms "
                       f"({products} products, needed {need * 1e3:.1f} ms): {'WAITED for the stream' if over_after else 'returned at once'}; "
                       f"outputs {'equal' if got == ref else 'DIFFER from'} the call made alone")
    print(w["report"][-1])
    _check(w, status, name)
    assert not over_before, f"inconclusive: {name}: the blocker had ended before the call was made"
    assert length >= need, f"inconclusive: {name}: the blocker took {length * 1e3:.1f} ms, under the {need * 1e3:.1f} ms required"
    assert not over_after, f"{name} waited for the stream: the blocker in front of it had completed when the call returned ({t_behind * 1e3:.1f} ms)"
    assert got == ref, f"{name}: the outputs differ from the call made alone: a host array was read after the call returned"


@pytest.mark.parametrize("name", ENTRIES)
def test_a_call_behind_a_blocker_returns_at_once_and_has_consumed_its_host_arrays(world, name):
    _behind_a_blocker(world, _entries(world)[name])


# ---- (b) more than 8 in flight, slots outgrown, three streams ------------------------------------------------------------------------------
SIZES = [1, 255, 256, 257, 700, 64, 1100, 300, 513, 1024, 33, 900]      # rising and falling: slots are outgrown and reused
RECS = [1, 2, 3, 1, 3, 2, 1, 3, 2, 3, 1, 2]


def _starts_of(frames, recs, k):
    """`recs` valid starts of `frames` frames, different for every k"""
    recs = min(recs, frames)
    if recs == 1:
        return _i32([0])
    cuts = sorted({max(1, min(frames - 1, (frames * (j + 1)) // recs - 3 * k - j)) for j in range(recs - 1)})
    return _i32([0] + cuts)


def _score_calls(w):
    lib, Z = w["lib"], lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")       # noqa: E731
    calls = []
    for k, (n, r) in enumerate(zip(SIZES, RECS)):
        st = _starts_of(n, r, k)
        r = len(st)
        bodies = _f64([BODY * (1.0 + 0.05 * k + 0.1 * j) for j in range(r)])
        skip = k % 4
        if k % 2 == 0:
            calls.append((lambda n=n, r=r: [Z(n, 7), Z(r, 25)],
                          lambda o, s, n=n, r=r, st=st, bodies=bodies, skip=skip: lib.ape_score_rows(
                              LAYOUT, _ptr(w["msg"]), 25, _ptr(w["spread"]), 21, F64, _ptr(w["tgt"]), TRUTH_TARGETS, F64, n, _host(st), r, skip, _host(bodies), r,
                              _ptr(o[0]), F64, _ptr(o[1]), _sp(s))))
        else:
            off = _i32([(k + j) % 3 - 1 for j in range(r)])
            lo, hi = -(k % 3), 1 + k % 2
            nl = hi - lo + 1
            calls.append((lambda n=n, r=r, nl=nl: [Z(n, nl, 7), Z(r, nl, 25)],
                          lambda o, s, n=n, r=r, st=st, bodies=bodies, skip=skip, off=off, lo=lo, hi=hi: lib.ape_score_lags(
                              LAYOUT, _ptr(w["msg"]), 25, _ptr(w["spread"]), 21, F64, _ptr(w["tgt"]), TRUTH_TARGETS, F64, n, _host(st), r, skip, _host(bodies), r,
                              lo, hi, _host(off), _ptr(o[0]), F64, _ptr(o[1]), _sp(s))))
    return calls


def _by_calls(w):
    lib, Z = w["lib"], lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")       # noqa: E731
    calls = []
    for k, (n, r) in enumerate(zip(SIZES, RECS)):
        st = _starts_of(n, r, k)
        r = len(st)
        nk, nv, bins = 1 + k % 2, 1 + k % 3, 3 + k % 5
        edges = _f64([np.linspace(-1.5, 1.5, bins + 1) + 0.07 * k + 0.1 * c for c in range(nk)])
        trim = _i32([[(k + j) % 3, (2 * k + j) % 4] for j in range(r)])
        calls.append((lambda r=r, nk=nk, nv=nv, bins=bins: [Z(1, r, nk, bins + 3, nv, 4)],
                      lambda o, s, n=n, r=r, st=st, nk=nk, nv=nv, bins=bins, edges=edges, trim=trim: lib.ape_score_by(
                          _ptr(w["values"]), F64, nk, 0, 3, _ptr(w["tgt"]), F64, nv, 0, O, 1, n, _host(st), r, _host(trim), _host(edges), bins, _ptr(o[0]), _sp(s))))
    return calls


def _stats_calls(w):
    """ape_segment_stats over tables ape_segment_runs made (alone, here) for labels that change every 1050 frames: the 1100-frame call has
    one recording, so its first segment is longer than APE_SEG_PIECE = 1024 and the fold launch has pieces to add"""
    lib = w["lib"]
    Z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")          # noqa: E731
    labels = ((torch.arange(1100, device="cuda") // 1050) % 2).to(torch.uint8)
    calls = []
    for k, (n, r) in enumerate(zip(SIZES, RECS)):
        st = _starts_of(n, r, k)
        r = len(st)
        lab = labels[:n].contiguous() if k % 2 == 0 else w["labels"][0, :n].contiguous()
        if n == 1100:
            assert r == 1 and k % 2 == 0
        runs = [Z(1, n, dtype=torch.int32), Z(1, dtype=torch.int32), Z(1, n, 4, dtype=torch.int32)]
        _check(w, lib.ape_segment_runs(_ptr(lab), 1, n, _host(st), r, _ptr(runs[0]), _ptr(runs[1]), _ptr(runs[2]), n, _sp(w["idle"])), "ape_segment_runs")
        nv = 1 + k % 3
        calls.append((lambda n=n, nv=nv: [Z(1, n, nv, 5)],
                      lambda o, s, n=n, nv=nv, runs=runs: lib.ape_segment_stats(_ptr(w["tgt"]), F64, 1, 0, O, 1, nv, 1, n, _ptr(runs[0]), _ptr(runs[2]), _ptr(runs[1]),
                                                                                n, _ptr(o[0]), _sp(s))))
    torch.cuda.synchronize()
    return calls


@pytest.mark.parametrize("pool", ["score_rows_and_lags", "score_by", "segment_stats"])
def test_b_twelve_calls_in_flight_on_three_streams(world, pool):
    w = world
    calls = {"score_rows_and_lags": _score_calls, "score_by": _by_calls, "segment_stats": _stats_calls}[pool](w)
    assert len(calls) == 12
    refs = []
    for make, call in calls:                                # every call alone
        outs = make()
        torch.cuda.synchronize()
        _check(w, call(outs, w["idle"]), pool)
        torch.cuda.synchronize()
        refs.append(_snap(outs))
    outs = [make() for make, _ in calls]
    torch.cuda.synchronize()
    # the first stream's blocker is the shortest, so that the oldest call is also the first to complete
    marks = [w["blocker"].enqueue(s, MIN_BLOCKER * (1 if i == 0 else 3)) for i, s in enumerate(w["sides"])]
    over_before = [m[1].query() for m in marks]
    first = torch.cuda.Event()
    status, blocked_at_ninth, first_done_after_ninth = [], None, None
    for k, (_, call) in enumerate(calls):
        s = w["sides"][k % 3]
        if k == 8:
            blocked_at_ninth = not first.query()            # the first call is still behind its blocker: eight calls are in flight
        status.append(call(outs[k], s))
        if k == 0:
            first.record(s)
        if k == 8:
            first_done_after_ninth = first.query()
    torch.cuda.synchronize()
    lengths = [m[0].elapsed_time(m[1]) / 1e3 for m in marks]
    w["report"].append(f"(b) {pool}: blockers of {', '.join(f'{x * 1e3:.1f}' for x in lengths)} ms; first call pending before the ninth: {blocked_at_ninth}, "
                       f"complete after it: {first_done_after_ninth}")
    print(w["report"][-1])
    for k, st in enumerate(status):
        _check(w, st, f"{pool} call {k}")
    assert not any(over_before), f"inconclusive: {pool}: a blocker had ended before the first call was made"
    assert min(lengths) >= MIN_BLOCKER, f"inconclusive: {pool}: a blocker took {min(lengths) * 1e3:.1f} ms"
    assert blocked_at_ninth, f"inconclusive: {pool}: the first call had completed before the ninth was made, so fewer than eight were in flight"
    assert first_done_after_ninth, f"{pool}: with eight calls in flight the ninth returned before the oldest had completed"
    for k in range(12):
        assert _snap(outs[k]) == refs[k], f"{pool}: call {k} (F = {SIZES[k]}) in flight differs from the same call made alone"


# ---- (c) the shared post-filter workspace --------------------------------------------------------------------------------------------------
def test_c_a_sweep_on_another_stream_stays_behind_the_window_call_that_holds_the_workspace(world):
    w = world
    lib, hd = w["lib"], w["handle"]
    s1, s2 = w["sides"][0], w["sides"][1]
    Z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")                       # noqa: E731
    st, bodies = _i32(STARTS), _f64([BODY * (1.0 + 0.1 * r) for r in range(R)])
    windows, weights = _i32([[3, 3, 4], [2, 0, 2]]), _taper([[1, 2, 3, 4, 3, 2, 1], [1, 2, 3]])
    configs = _i32([[3, 2], [1, 1]])                        # (no more samples and no longer windows than A: no larger workspace)
    ya, yb = w["y"][:F].contiguous(), w["y2"][:F].contiguous()

    def call_a(out, s, y=ya, n=F):
        return lib.ape_post_window(hd, _ptr(y), n, M, _host(st), R, _host(windows), _host(weights), 2, FLAG_SPREAD, _host(bodies), R, _ptr(out), F64, 0, _sp(s))

    def call_b(out, s):
        return lib.ape_post_sweep(hd, _ptr(yb), F, M, _host(st), R, _host(configs), 2, 0, _host(bodies), R, _ptr(out), F64, 0, _sp(s))

    ref_a, ref_b = Z(2, F, 46), Z(2, F, 25)
    torch.cuda.synchronize()
    _check(w, call_a(ref_a, s1), "A alone")
    torch.cuda.synchronize()
    _check(w, call_b(ref_b, s2), "B alone")
    torch.cuda.synchronize()
    ref_a, ref_b = _snap([ref_a]), _snap([ref_b])
    # t_B: B alone, from the call to its completion
    out_b = Z(2, F, 25)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _check(w, call_b(out_b, s2), "B timed")
    s2.synchronize()
    t_b = time.perf_counter() - t0
    assert _snap([out_b]) == ref_b
    window = max(0.005, 20 * t_b)
    need = max(MIN_BLOCKER, 4 * window)

    out_a, out_b = Z(2, F, 46), Z(2, F, 25)
    torch.cuda.synchronize()
    start, done, _ = w["blocker"].enqueue(s1, need)
    over_before = done.query()
    sa = call_a(out_a, s1)
    sb = call_b(out_b, s2)
    behind_b = torch.cuda.Event()
    behind_b.record(s2)
    polls, early, cut_short = 0, False, False
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < window:
        b_done = behind_b.query()
        if done.query():                                    # (asked second: B complete with the blocker still running is the finding)
            cut_short = True
            break
        early = early or b_done
        polls += 1
    torch.cuda.synchronize()
    length = start.elapsed_time(done) / 1e3
    w["report"].append(f"(c) t_B = {t_b * 1e6:.0f} us, polled {polls} times over {window * 1e3:.1f} ms behind a blocker of {length * 1e3:.1f} ms: "
                       f"B {'COMPLETED early' if early else 'stayed incomplete'}")
    print(w["report"][-1])
    _check(w, sa, "A")
    _check(w, sb, "B")
    assert not over_before and not cut_short and polls > 0, "inconclusive: the blocker ended inside the polling window"
    assert not early, "B completed while A, the last user of the workspace, was still behind its blocker: B is not ordered behind A"
    assert _snap([out_a]) == ref_a and _snap([out_b]) == ref_b

    # C needs a larger workspace (more frames, every sample) while A' is in flight behind another blocker: C may wait, no result may change
    n_c = 1100
    yc = w["y2"][:n_c].contiguous()
    st_c = _i32([0, 400, 777])
    win_c = _i32([[5, 5, 4], [0, 0, 1]])

    def call_c(out, s):
        return lib.ape_post_window(hd, _ptr(yc), n_c, M, _host(st_c), R, _host(win_c), None, 2, FLAG_SPREAD, _host(bodies), R, _ptr(out), F64, 0, _sp(s))

    out_a, out_c = Z(2, F, 46), Z(2, n_c, 46)
    torch.cuda.synchronize()
    start, done, _ = w["blocker"].enqueue(s1, MIN_BLOCKER)
    sa = call_a(out_a, s1)
    a_in_flight = not done.query()
    sc = call_c(out_c, s2)
    torch.cuda.synchronize()
    _check(w, sa, "A'")
    _check(w, sc, "C")
    assert a_in_flight, "inconclusive: the blocker in front of A' had ended before C was called"
    got_a, got_c = _snap([out_a]), _snap([out_c])
    ref_c = Z(2, n_c, 46)
    _check(w, call_c(ref_c, s2), "C alone")
    torch.cuda.synchronize()
    assert got_a == ref_a, "A' changed under a call that grew the workspace"
    assert got_c == _snap([ref_c]), "C, which grew the workspace while A' was in flight, differs from the same call made alone"


# ---- (a) once more, at the size where the runtime's own staging ends (last: it leaves the workspace larger than (c) wants to find it) -----
def test_a_post_window_with_host_arrays_past_a_megabyte(world):
    """The size at which the HIP runtime stops staging a copy from pageable memory by itself: with 20 000 recordings the table of bodies
    is 1.44 MB, and a `hipMemcpyAsync` straight from the caller's array made the call wait for everything queued on the stream
    (profiles/calls_in_flight.md: at once up to 295 KB, the blocker's whole 75 ms at 1.44 MB).  The same steps as every case of (a)."""
    w = world
    lib, hd = w["lib"], w["handle"]
    recs, frames = 20000, 60000
    g = torch.Generator(device="cuda").manual_seed(20000)
    y = torch.randn((frames, 2, O), device="cuda", generator=g)
    starts = _i32(np.arange(recs) * 3)
    shifted = starts.copy()
    shifted[1::2] += 1                                      # recordings of 4 and 2 frames where they were of 3
    bodies = _f64([BODY * (1.0 + 0.001 * (r % 97)) for r in range(recs)])
    windows = {"windows": _i32([[3, 3, 2], [2, 0, 1]]), "weights": _taper([[1, 2, 3, 4, 3, 2, 1], [1, 2, 3]])}
    windows_p = {"windows": _i32([[2, 4, 1], [1, 1, 2]]), "weights": _taper([[1, 4, 6, 8, 6, 4, 1], [3, 2, 1]])}
    entry = Entry("ape_post_window (20 000 recordings)", {"starts": starts, "bodies": bodies, **windows}, {"starts": shifted, "bodies": bodies * 1.5, **windows_p},
                  lambda: [torch.zeros((2, frames, 25), dtype=torch.float64, device="cuda")],
                  lambda h, o, s: lib.ape_post_window(hd, _ptr(y), frames, 2, _host(h["starts"]), recs, _host(h["windows"]), _host(h["weights"]), 2, 0,
                                                      _host(h["bodies"]), recs, _ptr(o[0]), F64, 0, _sp(s)))
    _behind_a_blocker(w, entry)
