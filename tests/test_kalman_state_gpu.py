"""The Kalman bank's state hand-over on the GPU (``ape_kalman_bank_export`` / ``_import``, the draw position, ``ape_kalman_replay_resume``;
DESIGN.md 4.27).  PARITY UNPINNED like the bank: what is proved is that a stream that left its bank continues bit for bit like one that
stayed, and -- through tests/test_kalman_bank_gpu.py's ``StreamOracle`` carried across the hand-over -- within that file's own tolerances
of the oracle chain (5e-4 on the normalised targets over at most 14 frames of feedback, 1e-12 on the float64 messages).

Every stream stays at or below 14 frames since its cold start.  Draws are injected, so bit-equality does not depend on the draw position,
except in the draw-position and replay cases, which use the device draws on purpose."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import kalman_oracle as ko
from tests.test_kalman import make_model
from tests.test_kalman_bank_gpu import _estimator, features, make_bank, make_rows, new_oracle, pocket_stats, run_frame

pytestmark = pytest.mark.gpu


def draws(rng, W, E, K=1):
    return ko.draw_noise(rng, W, K * E), rng.standard_normal((K, E, 14)).astype(np.float32)


def n_new(frames_before, W, E):
    """rows of the prediction of the frame a stream runs after `frames_before` frames since its cold start"""
    return 1 if frames_before <= W else E


def assert_same_frame(a, b, rows_new, what):
    """two run_frame results, bit for bit: packed messages, n_rows, and the specified rows of y (rows_new[j] of entry j)"""
    (oa, na, ya), (ob, nb, yb) = a, b
    np.testing.assert_array_equal(oa, ob, err_msg=what)
    np.testing.assert_array_equal(na, nb, err_msg=what)
    for j, k in enumerate(rows_new):
        np.testing.assert_array_equal(ya[j, :k], yb[j, :k], err_msg=what)
    assert np.all(np.isfinite(oa)) and all(np.all(np.isfinite(ya[j, :k])) for j, k in enumerate(rows_new)), what


# ---- 1. continuation ------------------------------------------------------------------------------------------------------------------
# W = 4: n = 2 init phase; 5 = W + 1, the first mature age (the next frame is the first ensemble frame); 6 a ragged stack of 1- and E-row
# entries at smooth 3; 9 all E.  W = 10: n = 3 and 12.
@pytest.mark.parametrize("smooth", [1, 3])
@pytest.mark.parametrize("E,W,n", [(16, 4, 2), (16, 4, 5), (16, 4, 6), (16, 4, 9), (48, 10, 3), (48, 10, 12)])
def test_an_exported_stream_continues_in_another_bank(norm_stats, E, W, n, smooth):
    stats = pocket_stats(norm_stats)
    m, sd = make_model(E, W, 31)
    a, b = make_bank(m, 3, smooth, stats), make_bank(m, 5, smooth, stats)
    so = new_oracle(sd, E, W, smooth, stats)
    rng = np.random.default_rng(1000 * E + 10 * n + smooth)
    later = min(14 - n, W + 3)
    rows = make_rows(rng, n + later)
    for f in range(n):
        nz, init = draws(rng, W, E)
        out, cnt, y = run_frame(a, rows[f:f + 1], [1], nz, init)
        so.check(rows[f], nz, init[0], y[0], int(cnt[0]), out[0], f"source frame {f}")
    state, age = a.export_state([1])
    assert age.dtype == np.int32 and age.tolist() == [min(n, W + 1)]
    assert tuple(state.shape) == (1, a.state_desc()["words_per_stream"]) and state.dtype == torch.float32
    b.import_state([3], state, age, desc=a.state_desc())
    for f in range(n, n + later):                       # the same rows and draws, both at list position 0
        nz, init = draws(rng, W, E)
        ra, rb = run_frame(a, rows[f:f + 1], [1], nz, init), run_frame(b, rows[f:f + 1], [3], nz, init)
        assert_same_frame(ra, rb, [n_new(f, W, E)], f"E {E} W {W} n {n} smooth {smooth} frame {f}")
        so.check(rows[f], nz, init[0], rb[2][0], int(rb[1][0]), rb[0][0], f"imported frame {f}")       # the oracle carried on from A
    assert b.export_state([3])[1].tolist() == [min(n + later, W + 1)]
    m.check()


# ---- 2. canonical form ----------------------------------------------------------------------------------------------------------------
def expected_counts(f, W, E, smooth):
    """stack entries oldest first after f frames: the last `smooth` frames, padded with the first; a frame's entry has 1 row while the
    stream is in its first W + 1 frames (test_one_stream_bank_against_the_oracle_chain's ragged sequence)"""
    return [1 if max(1, f - smooth + 1 + k) <= W + 1 else E for k in range(smooth)]


@pytest.mark.parametrize("E,W,smooth,n", [(16, 4, 3, 2), (16, 4, 3, 6), (16, 4, 3, 9), (48, 10, 1, 12), (16, 4, 2, 5)])
def test_the_record_is_canonical(norm_stats, E, W, smooth, n):
    from wear_mocap_ape_amd import stream_state as ss
    stats = pocket_stats(norm_stats)
    m, _ = make_model(E, W, 32)
    a, b = make_bank(m, 2, smooth, stats), make_bank(m, 4, smooth, stats)
    desc = a.state_desc()
    assert desc == ss.kalman_desc(E, W, smooth)
    rng = np.random.default_rng(50 * n + smooth)
    more = min(3, 14 - n)
    rows = make_rows(rng, n + more)
    # a cold stream: a zero record, age 0
    state, age = a.export_state([1, 0])
    assert age.tolist() == [0, 0] and not state.cpu().numpy().view(np.int32).any()
    first = None
    for f in range(1, n + 1):
        nz, init = draws(rng, W, E)
        out, cnt, y = run_frame(a, rows[f - 1:f], [1], nz, init)
        state, age = a.export_state([1])
        rec = state.cpu().numpy()[0]
        window, history, stack, counts, pad = ss.kalman_unpack(rec, desc)
        k = n_new(f - 1, W, E)
        assert age.tolist() == [min(f, W + 1)]
        assert counts.tolist() == expected_counts(f, W, E, smooth), (f, counts)
        assert int(cnt[0]) == int(counts.sum())
        np.testing.assert_array_equal(stack[-1, :k], y[0, :k])                  # the newest stack entry: the frame's returned y
        for e in range(smooth):                                                  # unused rows and the padding: zeros
            assert not stack[e, counts[e]:].view(np.int32).any(), (f, e)
        assert not pad.view(np.int32).any()
        if k == E:                                                               # an ensemble frame joins the history itself
            np.testing.assert_array_equal(history[:, W - 1], y[0])
        else:                                   # format_state: z + sqrt(0.1) * draw, one float32 rounding apart at the most
            want = y[0, 0][None, :] + np.float32(0.31622776601683794) * init[0]
            assert np.abs(history[:, W - 1] - want).max() < 1e-6
        assert not history[:, :max(0, W - f)].view(np.int32).any()              # entries that do not exist yet
        assert history[:, max(0, W - f):].any(axis=(0, 2)).all()
        # the window: the W rows the frame saw, oldest first, the first row repeated while the stream is younger than W
        xx = features(rows[f - 1])                      # (1e-6: test_parse_rows' bound of the device's float64 features on the host builder)
        assert np.abs(window[-1] - xx).max() < 1e-6
        first = window[-1].copy() if f == 1 else first
        for t in range(max(0, W - f + 1)):
            np.testing.assert_array_equal(window[t], first)
    # export(import(r)) == r, in another slot of another bank
    r0 = state.cpu().numpy().copy()
    b.import_state([2], state, age)
    back, age_b = b.export_state([2])
    np.testing.assert_array_equal(back.cpu().numpy().view(np.int32), r0.view(np.int32))
    assert age_b.tolist() == age.tolist()
    # ... and after the same frames in both (for a mature stream the ring phases of A and B differ) the records are still equal
    for f in range(n, n + more):
        nz, init = draws(rng, W, E)
        assert_same_frame(run_frame(a, rows[f:f + 1], [1], nz, init), run_frame(b, rows[f:f + 1], [2], nz, init), [n_new(f, W, E)], f"frame {f}")
    (sa, aa), (sb, ab) = a.export_state([1]), b.export_state([2])
    np.testing.assert_array_equal(sa.cpu().numpy().view(np.int32), sb.cpu().numpy().view(np.int32))
    assert aa.tolist() == ab.tolist() == [min(n + more, W + 1)]
    m.check()


def test_exports_back_to_back(norm_stats):
    """12 exports of two of three streams, each into its own buffer, with no host synchronisation in between: the hand-over's pinned
    descriptor ring (csrc/bank_host.h) wraps.  Bit-equal to the same calls with a device synchronisation after each, and every
    record is the canonical one of its stream (the checks of test_the_record_is_canonical)."""
    from wear_mocap_ape_amd import stream_state as ss
    E, W, S, smooth = 16, 4, 3, 2
    stats = pocket_stats(norm_stats)
    m, _ = make_model(E, W, 35)
    a = make_bank(m, S, smooth, stats)
    desc = a.state_desc()
    rng = np.random.default_rng(35)
    ages = [2, 6, 9]                                        # init phase, the first ensemble frame behind it, mature
    last = {}
    for s, n in enumerate(ages):
        rows = make_rows(rng, n)
        for f in range(n):
            nz, init = draws(rng, W, E)
            out, cnt, y = run_frame(a, rows[f:f + 1], [s], nz, init)
        last[s] = (rows[n - 1], int(cnt[0]), y[0])
    pairs = [[t % S, (t + 1 + t // S % 2) % S] for t in range(12)]

    def run(sync):
        torch.cuda.synchronize()
        res = []
        for p in pairs:
            res.append(a.export_state(p))
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return [(state.cpu().numpy(), age.copy()) for state, age in res]

    queued, synced = run(False), run(True)
    for p, (sq, aq), (sy, ay) in zip(pairs, queued, synced):
        np.testing.assert_array_equal(sq.view(np.int32), sy.view(np.int32), err_msg=str(p))
        assert aq.tolist() == ay.tolist() == [min(ages[s], W + 1) for s in p]
        for j, s in enumerate(p):
            row, cnt, y = last[s]
            window, history, stack, counts, pad = ss.kalman_unpack(sq[j], desc)
            k = n_new(ages[s] - 1, W, E)
            assert counts.tolist() == expected_counts(ages[s], W, E, smooth) and cnt == int(counts.sum()), (p, s)
            np.testing.assert_array_equal(stack[-1, :k], y[:k])
            assert np.abs(window[-1] - features(row)).max() < 1e-6           # (test_the_record_is_canonical's bound)
            assert not pad.view(np.int32).any()
    m.check()


# ---- 3. untouched streams -------------------------------------------------------------------------------------------------------------
def test_import_and_export_leave_other_streams_untouched(norm_stats):
    E, W, S, smooth = 16, 4, 5, 2
    stats = pocket_stats(norm_stats)
    m, _ = make_model(E, W, 33)
    p, q, donor = make_bank(m, S, smooth, stats), make_bank(m, S, smooth, stats), make_bank(m, 1, smooth, stats)
    rng = np.random.default_rng(5)
    frames = [0] * S                                    # frames since the cold start, per stream

    def both(order):
        idx = list(range(S)) if order is None else order
        rows, (nz, init) = make_rows(rng, len(idx)), draws(rng, W, E, len(idx))
        rp, rq = run_frame(p, rows, order, nz, init), run_frame(q, rows, order, nz, init)
        news = [n_new(frames[s], W, E) for s in idx]
        for s in idx:
            frames[s] += 1
        return rp, rq, news, idx

    for _ in range(3):
        rp, rq, news, _ = both(None)
        assert_same_frame(rp, rq, news, "before")
    for f in range(6):                                  # the donor: a mature stream with a ragged stack
        nz, init = draws(rng, W, E)
        run_frame(donor, make_rows(rng, 1), None, nz, init)
    state, age = donor.export_state([0])
    assert age.tolist() == [W + 1]
    p.import_state([3], state, age)                     # Q never imports
    p.export_state([0, 2, 3])                           # ... and never exports
    for order in ([0, 1, 2, 4], [4, 1], [2, 0, 4, 1]):
        rp, rq, news, _ = both(order)
        assert_same_frame(rp, rq, news, f"subset {order}")
    rp, rq, news, idx = both(None)                      # lockstep: stream 3 differs (mature in P, frame 4 of its init phase in Q)
    keep = [0, 1, 2, 4]
    assert_same_frame(tuple(v[keep] for v in rp), tuple(v[keep] for v in rq), [news[s] for s in keep], "lockstep after the import")
    assert int(rq[1][3]) == smooth and int(rp[1][3]) == 2 * E          # (the donor's stack was [1, E]: this frame makes it [E, E])
    assert p.export_state([3])[1].tolist() == [W + 1] and q.export_state([3])[1].tolist() == [4]
    # an age-0 import is reset(streams=): nothing is read from the record
    words = p.state_desc()["words_per_stream"]
    junk = torch.full((2, words), float("nan"), dtype=torch.float32, device="cuda")
    p.import_state([1, 3], junk, [0, 0])
    q.reset(streams=[1, 3])
    frames[1] = frames[3] = 0
    assert p.export_state([1, 3, 0])[1].tolist() == [0, 0, min(frames[0], W + 1)]
    for order in ([3, 0], None, [1, 2]):
        rp, rq, news, idx = both(order)
        assert_same_frame(rp, rq, news, f"after the cold import {order}")
    assert int(rp[1][0]) == smooth                      # stream 1 is in its init phase again
    m.check()


# ---- 4. draw position -----------------------------------------------------------------------------------------------------------------
def plain_frame(bank, row, s):
    out, n, y = bank.frame(row, [s], datagrams=True, return_targets=True)
    return out.cpu().numpy().copy(), n.cpu().numpy().copy(), y.cpu().numpy().copy()


@pytest.mark.parametrize("n", [3, 7])
def test_a_bank_continues_another_banks_draw_sequence(norm_stats, n):
    E, W, smooth, seed = 16, 4, 2, 777
    stats = pocket_stats(norm_stats)
    m, _ = make_model(E, W, 34)
    a, b, c = (make_bank(m, S, smooth, stats, seed=seed) for S in (2, 3, 3))
    rng = np.random.default_rng(n)
    rows = make_rows(rng, n + 4)
    assert a.get_draw_position() == (seed, 0)
    for f in range(n):
        plain_frame(a, rows[f:f + 1], 1)
    assert a.get_draw_position() == (seed, n)
    state, age = a.export_state([1])
    b.set_draw_position(*a.get_draw_position())
    b.import_state([2], state, age)
    c.set_draw_position(seed, n + 1)                    # one call off: other draws
    c.import_state([2], state, age)
    assert b.get_draw_position() == (seed, n) and c.get_draw_position() == (seed, n + 1)
    for f in range(n, n + 4):
        ra, rb, rc = (plain_frame(bank, rows[f:f + 1], s) for bank, s in ((a, 1), (b, 2), (c, 2)))
        k = n_new(f, W, E)
        assert_same_frame(ra, rb, [k], f"frame {f}")
        assert not np.array_equal(ra[2][0, :k], rc[2][0, :k]), f
        assert np.array_equal(ra[1], rc[1])
    assert a.get_draw_position() == b.get_draw_position() == (seed, n + 4)
    m.check()


# ---- 5. resumable replay --------------------------------------------------------------------------------------------------------------
CUTS = [0, 2, 5, 6, 13]


def host(*tensors):
    return [t.cpu().numpy().copy() for t in tensors]


def test_a_recording_replayed_in_pieces_equals_the_one_call():
    E, W, smooth, seed, F = 16, 4, 2, 4343, 13
    sd = ko.make_state_dict(W, 35)
    est = _estimator(sd, E, W, smooth=smooth)
    rng = np.random.default_rng(12)
    rows = make_rows(rng, F)
    out, n, y = host(*est.process_recording(rows, seed=seed, return_targets=True))
    assert n.tolist() == [smooth] * (W + 1) + [1 + E] + [2 * E] * (F - W - 2) and np.all(np.isfinite(out))
    state = age = None
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        o, nn, yy, state, age = est.process_recording(rows[a:b], seed=seed, return_targets=True, state_in=state, age_in=age,
                                                      return_state=True, call_base=a)
        o, nn, yy = host(o, nn, yy)
        np.testing.assert_array_equal(o, out[a:b])
        np.testing.assert_array_equal(nn, n[a:b])
        for f in range(a, b):
            k = n_new(f, W, E)
            np.testing.assert_array_equal(yy[f - a, :k], y[f, :k])
        assert age.tolist() == [min(b, W + 1)] and tuple(state.shape) == (1, 4 * ((2 * W * 22 + E * W * 14 + smooth * E * 14 + smooth + 3) // 4))
    # a piece that does not chain the state starts cold: other rows
    o, nn = host(*est.process_recording(rows[6:13], seed=seed, call_base=6))
    assert nn.tolist() == [smooth] * (W + 1) + [1 + E, 2 * E] and not np.array_equal(o, out[6:13])
    est.model.check()


def test_three_recordings_cut_at_the_same_offsets_equal_the_one_call():
    E, W, smooth, seed, F, R = 16, 4, 2, 4344, 13, 3
    sd = ko.make_state_dict(W, 36)
    est = _estimator(sd, E, W, smooth=smooth)
    rng = np.random.default_rng(13)
    rows = make_rows(rng, R * F).reshape(R, F, 55)
    out, n, y = host(*est.process_recording(rows.reshape(R * F, 55), starts=[0, F, 2 * F], seed=seed, return_targets=True))
    out, n, y = out.reshape(R, F, -1), n.reshape(R, F), y.reshape(R, F, E, 14)
    assert np.all(np.isfinite(out))
    state = age = None
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        L = b - a
        o, nn, yy, state, age = est.process_recording(np.ascontiguousarray(rows[:, a:b]).reshape(R * L, 55), starts=[0, L, 2 * L], seed=seed,
                                                      return_targets=True, state_in=state, age_in=age, return_state=True, call_base=a)
        o, nn, yy = host(o, nn, yy)
        np.testing.assert_array_equal(o.reshape(R, L, -1), out[:, a:b])
        np.testing.assert_array_equal(nn.reshape(R, L), n[:, a:b])
        for f in range(a, b):
            k = n_new(f, W, E)
            np.testing.assert_array_equal(yy.reshape(R, L, E, 14)[:, f - a, :k], y[:, f, :k])
        assert age.tolist() == [min(b, W + 1)] * R
    est.model.check()


def test_a_replays_state_continues_in_a_bank_and_an_estimators_in_another_estimator():
    from wear_mocap_ape_amd.streams import KalmanStreamBank, trim_packed
    E, W, smooth, seed, F, cut = 16, 4, 2, 4345, 13, 8
    sd = ko.make_state_dict(W, 37)
    est = _estimator(sd, E, W, smooth=smooth)
    rng = np.random.default_rng(14)
    rows = make_rows(rng, F)
    out, n, y = host(*est.process_recording(rows, seed=seed, return_targets=True))
    _, _, state, age = est.process_recording(rows[:cut], seed=seed, return_state=True)
    bank = KalmanStreamBank(est.model, 2, smooth=smooth, normalize=True, seed=seed)
    bank.set_draw_position(seed, cut)
    bank.import_state([1], state, age)
    for f in range(cut, F):
        o, nn, yy = plain_frame(bank, rows[f:f + 1], 1)
        np.testing.assert_array_equal(o[0], out[f])
        assert int(nn[0]) == int(n[f])
        np.testing.assert_array_equal(yy[0], y[f])
    # get_state -> set_state on a second estimator: process_row continues bit for bit (the dict carries the draw position)
    one, two = _estimator(sd, E, W, smooth=smooth), _estimator(sd, E, W, smooth=smooth)
    one.manual_seed(seed)
    for f in range(6):
        assert one.process_row(rows[f]) == trim_packed(out[f], n[f]).tolist()
    st = one.get_state()
    assert st["form"] == "kalman-device" and st["age"] == W + 1 and (st["seed"], st["calls"]) == (seed, 6)
    assert st["record"].shape == (st["desc"]["words_per_stream"],) and st["desc"]["E"] == E
    two.set_state(st)
    for f in range(6, F):
        got = two.process_row(rows[f])
        assert got == one.process_row(rows[f]) == trim_packed(out[f], n[f]).tolist()
    # the staged host path keeps no canonical record and says so
    staged = _estimator(sd, E, W, smooth=smooth)
    staged.use_device_frame = False
    with pytest.raises(UserWarning, match="use_device_frame"):
        staged.get_state()
    with pytest.raises(UserWarning, match="use_device_frame"):
        staged.set_state(st)
    est.model.check()


# ---- 6. refusals that need a bank -----------------------------------------------------------------------------------------------------
def test_refusals_that_need_a_bank(norm_stats):
    from wear_mocap_ape_amd import _hip
    lib = _hip.lib()
    E, W, S, smooth = 16, 4, 4, 2
    m, _ = make_model(E, W, 38)
    bank = make_bank(m, S, smooth, pocket_stats(norm_stats))
    rng = np.random.default_rng(15)
    for _ in range(2):
        nz, init = draws(rng, W, E, S)
        run_frame(bank, make_rows(rng, S), None, nz, init)
    own = bank.state_desc()
    words = own["words_per_stream"]
    state = torch.zeros((S + 1, words), dtype=torch.float32, device="cuda")
    null = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def arr(v):
        return np.asarray(v, dtype=np.int32)

    def export(idx, K, ptr=None, stream=null):
        a, age = arr(idx), np.zeros(max(len(idx), 1), np.int32)
        return lib.ape_kalman_bank_export(bank._handle, C.c_void_p(a.ctypes.data), K, C.c_void_p(ptr or state.data_ptr()), C.c_void_p(age.ctypes.data),
                                          stream)

    def imp(idx, K, ages, desc=own, ptr=None, stream=null):
        a, g = arr(idx), arr(ages)
        d = _hip.ApeKalmanStateDesc(*[int(desc[k]) for k in ("version", "E", "W", "smooth", "words_per_stream")])
        return lib.ape_kalman_bank_import(bank._handle, C.byref(d), C.c_void_p(a.ctypes.data), K, C.c_void_p(ptr or state.data_ptr()),
                                          C.c_void_p(g.ctypes.data), stream)

    def refused(status, word):
        return status == 1 and word in lib.ape_last_error()          # APE_ERR_INVALID_ARG
    for key in ("version", "E", "W", "smooth", "words_per_stream"):   # a descriptor that differs in any one field
        assert refused(imp([0], 1, [1], desc=dict(own, **{key: own[key] + (4 if key == "words_per_stream" else 1)})), b"records are"), key
    assert refused(imp([0], 1, [-1]), b"age") and refused(imp([0], 1, [W + 2]), b"age") and refused(imp([0, 1], 2, [1, W + 2]), b"age")
    assert refused(imp([1, 1], 2, [1, 1]), b"twice") and refused(export([2, 0, 2], 3), b"twice")
    assert refused(imp([S], 1, [1]), b"outside") and refused(export([-1], 1), b"outside")
    assert refused(imp([0, 1, 2, 3, 0], S + 1, [1] * (S + 1)), b"K=") and refused(export([0, 1, 2, 3, 0], S + 1), b"K=")
    assert refused(imp([0], -1, [1]), b"K=") and refused(export([0], -1), b"K=")
    assert refused(imp([0], 1, [1], ptr=state.data_ptr() + 4), b"aligned") and refused(export([0], 1, ptr=state.data_ptr() + 8), b"aligned")
    # a capturing stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros((4,), device="cuda")
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            sp = C.c_void_p(side.cuda_stream)
            got = [(export([0], 1, stream=sp), lib.ape_last_error()), (imp([0], 1, [1], stream=sp), lib.ape_last_error())]
    torch.cuda.current_stream().wait_stream(side)
    assert all(status == 1 and b"capturing" in msg for status, msg in got), got
    # the replay's own: a state without its ages, an age outside [0, W + 1], a misaligned record buffer
    est = _estimator(ko.make_state_dict(W, 38), E, W, smooth=smooth)
    rows = make_rows(rng, 3)
    with pytest.raises(UserWarning, match="age"):
        est.process_recording(rows, state_in=state[:1], age_in=[W + 2])
    with pytest.raises(UserWarning, match="aligned"):
        est.process_recording(rows, state_in=state.reshape(-1)[1:1 + words].reshape(1, words), age_in=[1])
    with pytest.raises(UserWarning, match="together"):
        est.process_recording(rows, state_in=state[:1])
    # K = 0 is a no-op, and after every refusal nothing was launched or changed: the ages stand, the bank's next frame equals a twin's
    assert export([], 0) == 0 and imp([], 0, []) == 0
    assert bank.export_state(list(range(S)))[1].tolist() == [2] * S
    twin = make_bank(m, S, smooth, pocket_stats(norm_stats))
    rng2 = np.random.default_rng(15)
    for _ in range(2):
        nz, init = draws(rng2, W, E, S)
        run_frame(twin, make_rows(rng2, S), None, nz, init)
    nz, init = draws(rng, W, E, S)
    rows = make_rows(rng, S)
    assert_same_frame(run_frame(bank, rows, None, nz, init), run_frame(twin, rows, None, nz, init), [1] * S, "after the refusals")
    m.check()
