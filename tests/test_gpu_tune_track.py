"""lsdr_tune_track, lsdr_derotate_batch, capi.TrackedDecoder and capi.RecordingDecoder(tune="pieces") on the GPU: captures whose carrier
moves by more than the batch decoders' tuning window.

  a the tracker against the float64 restatement (track_common.track) on the first eight frames of three captures whose carrier moves: the
    same bins and held flags, powers within 1e-4·c, tune within 1e-7 of the formula on the device's own powers (test_gpu_tune_est.py's
    bounds); frame 0 is TuneEstimator(blocks=4)'s record bit for bit;
  b a capture's records are the same bits alone, in a batch, in the reversed batch, across two runs, in cs8, cs16 (in_scale 2^-8), cu16 and
    cf32 forms of the same floats and through both load paths;
  c the tracker's refusals are LSDR_E_ARG with a message and leave a usable object; edges: n = blocks·N − 1 (no frame), blocks·N (one), an end frame that coincides with a hop frame, a length of 0 beside live captures,
    a capture whose middle third is noise (held frames, the gate resumes from the last accepted bin), span = 0;
  d the derotator equals the numpy restatement (track_common.derotate) bit for bit in all five formats: tracks of 0, 1, 2, 3, 31 and 200 knots (the last three samples apart),
    a knot on sample 0, knots only in the middle, a segment boundary inside one 16-byte piece, a falling segment; lengths 1, 7, 8, 4097 and
    20000 (more than one workgroup in every format); nothing behind item n − 1 is written; alone, in any place, with any batch-mates;
    every refusal is LSDR_E_ARG with a message and leaves a usable object;
  e the loop closed: drifted(capture(1000, 11, 7.5), 2e-3, n, 0) and a ramp from −1.5e-3 to +1.5e-3 on the default engine, the drifted
    noise-18 capture on the Viterbi engine, decoded by TrackedDecoder.decode with no tune given, against oracle/_ref/leandvb on the SAME
    bytes (no --tune; --viterbi for the weak capture) under batch_common.check_against_reference with the tuning tests' numbers — and the
    same drifted capture through CaptureBatch.decode_estimated returns fewer than half the reference's packets;
  f RecordingDecoder(tune="pieces") on capture(2500, 3, 7.5) with e's ramp, from −1.5e-3 to +1.5e-3, nine pieces of 1 000 000 samples
    overlapping by 500 000: every pair joins, the stitched TS is the reference's under test_gpu_recording.py's rule, tune=None returns
    fewer packets.  The ramp: 3e-3 over 4 896 023 samples is 6.1e-4 per piece behind the tune estimated at the piece's start, and 3e-3
    at the recording's end behind the one tune of tune=None — the static offset that test_gpu_tune_est.py's untuned decode loses whole.
Measured on an MI355X: powers within 6.7e-7·c, tune within 2.1e-10 of the formula; e: 946 of 946, 946 of 946 and 932 of 932 packets, the whole
TS identical to the reference's in all three, all 31 frames accepted (quality at least 500, 439, 216); decode_estimated on the drifted
capture: 162 of 946 packets (17 %); f: 2445 packets of the reference's 2446 with a tune per piece, the first common packet at 0 / 0.
The reference binary (oracle/_ref/leandvb) is required by e and f: where it is missing those tests FAIL.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import batch_common as bc
import numpy as np
import pytest
import track_common as trk
import tune_common as tc

pytestmark = pytest.mark.gpu

LSDR_E_ARG = -2
N = trk.N
HOP = 65536
HEAD = 7 * HOP + 4 * N                  # eight frames, the end frame on the eighth hop frame
OMEGA, N_ALL = 1.2, 1958423
MOVING = [(7.5, 2e-3, 0.0), (18.0, 2e-3, 1.0), (7.5, 4e-3, 0.0)]


def _gaussian(n, seed, std=30.0):
    """n cu8 samples of circular Gaussian noise: no carrier and, unlike noise that is uniform on a square, no line in its fourth power."""
    return np.clip(np.rint(np.random.default_rng(seed).normal(0.0, std, 2 * n) + 128), 0, 255).astype(np.uint8)


def _head(noise, A, phase, n=HEAD):
    return np.ascontiguousarray(trk.drifted_capture(noise, A, phase)[0][: 2 * n])


def _bits(t):
    """A capture's track as bytes and integers (floats compared by their bits)."""
    f32 = lambda v: np.array(v, np.float32).tobytes()
    return (t["accepted"], f32([t["tune_first"], t["tune_last"], t["tune_min"], t["tune_max"], t["quality_min"]]),
            [(f["center"], f["bin"], f["held"], f32([f["tune"], f["quality"], f["mean_power"]] + f["power"])) for f in t["frames"]])


def _track(capi, ctx, arrays, lengths=None, ptrs=None, **kw):
    bufs = [ctx.upload(a) if a is not None else None for a in arrays]
    kw.setdefault("max_frames", 32)
    tr = capi.TuneTracker(ctx, len(arrays), **kw)
    try:
        if lengths is None:
            lengths = [len(a) // 2 for a in arrays]
        return tr.track(ptrs(bufs) if ptrs else [b.ptr if b else None for b in bufs], lengths)
    finally:
        tr.close()
        for b in bufs:
            if b:
                b.free()


def _against_restatement(got, iq, name, **kw):
    want = trk.track(tc.to_complex(iq), **kw)
    assert len(got["frames"]) == len(want["frames"]) and got["accepted"] == want["accepted"], (name, got, want)
    d_pow = d_tune = 0.0
    for k, (g, w) in enumerate(zip(got["frames"], want["frames"])):
        assert (g["center"], g["bin"], g["held"]) == (w["center"], w["bin"], w["held"]), (name, k, g, w)
        c = w["power"][1]
        dp = max(abs(a - b) for a, b in zip(g["power"] + [g["mean_power"]], w["power"] + [w["mean_power"]])) / c
        dt = abs(g["tune"] - tc.tune_from_peak(g["bin"], *g["power"]))
        d_pow, d_tune = max(d_pow, dp), max(d_tune, dt)
        assert dp <= 1e-4, (name, k, dp)
        assert dt <= 1e-7, (name, k, dt)
        assert g["quality"] == pytest.approx(g["power"][1] / g["mean_power"], rel=1e-6)
    acc = [f for f in got["frames"] if not f["held"]]
    if acc:
        t = [f["tune"] for f in acc]
        assert (got["tune_first"], got["tune_last"], got["tune_min"], got["tune_max"]) == (t[0], t[-1], min(t), max(t)), name
        assert got["quality_min"] == min(f["quality"] for f in acc)
    return d_pow, d_tune


# ---- a -----------------------------------------------------------------------------------------------------------------------------
def test_tracker_against_the_restatement(capi, ctx):
    heads = [_head(*m) for m in MOVING]
    got = _track(capi, ctx, heads)
    d = [_against_restatement(g, iq, str(m)) for g, iq, m in zip(got, heads, MOVING)]
    print(f"device against the restatement: powers within {max(x[0] for x in d):.2e} of c, tune within {max(x[1] for x in d):.2e} of the formula")
    assert all(len(g["frames"]) == 8 and g["accepted"] == 8 for g in got)
    bufs = [ctx.upload(h) for h in heads]
    est = capi.TuneEstimator(ctx, len(heads), blocks=4)
    try:
        for e, g in zip(est.estimate([b.ptr for b in bufs], [HEAD] * len(heads)), got):
            f0 = g["frames"][0]
            same = lambda a, b: np.array(a, np.float32).tobytes() == np.array(b, np.float32).tobytes()
            assert e["blocks"] == 4 and f0["bin"] == e["bin"] and f0["center"] == 2 * N and f0["held"] == 0
            assert same([f0["tune"], f0["quality"], f0["mean_power"]] + f0["power"], [e["tune"], e["quality"], e["mean_power"]] + e["power"]), (f0, e)
    finally:
        est.close()
        for b in bufs:
            b.free()


# ---- b -----------------------------------------------------------------------------------------------------------------------------
def test_records_are_the_same_bits(capi, ctx):
    heads = [_head(*m) for m in MOVING]
    short = np.ascontiguousarray(heads[1][: 2 * (3 * HOP + 5 * N + 17)])
    arrays = heads + [short]
    bufs = [ctx.upload(a) for a in arrays]
    ptrs, lengths = [b.ptr for b in bufs], [len(a) // 2 for a in arrays]
    tr, one = capi.TuneTracker(ctx, 4, max_frames=8), capi.TuneTracker(ctx, 1, max_frames=8)
    try:
        got = [_bits(t) for t in tr.track(ptrs, lengths)]
        assert [len(g[2]) for g in got] == [8, 8, 8, 5] and got[1][2][:3] == got[3][2][:3] and got[0] != got[2]
        assert [_bits(t) for t in tr.track(ptrs, lengths)] == got                                   # two runs
        assert [_bits(t) for t in tr.track(ptrs[::-1], lengths[::-1])] == got[::-1]                 # the reversed batch
        for i in range(4):                                                                          # alone
            assert _bits(one.track([ptrs[i]], [lengths[i]])[0]) == got[i], i
        moved = ctx.upload(np.concatenate([np.zeros(2, np.uint8), heads[0]]))                       # item-aligned only: the item-wise loads
        try:
            assert _bits(one.track([moved.at(2)], [HEAD])[0]) == got[0]
        finally:
            moved.free()
    finally:
        tr.close()
        one.close()
        for b in bufs:
            b.free()
    u8 = heads[1]
    s8 = (u8.astype(np.int16) - 128).astype(np.int8)
    s16 = (s8.astype(np.int16) * 256).astype(np.int16)
    u16 = (s16.astype(np.int32) + 32768).astype(np.uint16)
    f32 = s8.astype(np.float32)
    for name, items, kw in (("cs8", s8, dict(in_format=capi.IN_CS8)), ("cs16 scaled", s16, dict(in_format=capi.IN_CS16, in_scale=2.0 ** -8)),
                            ("cu16 scaled", u16, dict(in_format=capi.IN_CU16, in_scale=2.0 ** -8)),
                            ("cf32", f32, dict(in_format=capi.IN_CF32, in_scale=1.0)), ("cu8 scale 1", u8, dict(in_scale=1.0))):
        assert _bits(_track(capi, ctx, [items], [HEAD], **kw)[0]) == got[1], name
        item = items.itemsize * 2                                                                  # … and through the item-wise loads
        padded = np.concatenate([np.zeros(2, items.dtype), items])
        assert _bits(_track(capi, ctx, [padded], [HEAD], ptrs=lambda b, item=item: [b[0].at(item)], **kw)[0]) == got[1], name


# ---- c -----------------------------------------------------------------------------------------------------------------------------
def test_edges(capi, ctx):
    iq = _head(7.5, 2e-3, 0.0)
    lengths = [4 * N - 1, 4 * N, 0, HEAD, HEAD - 1, HEAD + N, 4 * N + 4095]
    buf = ctx.upload(np.concatenate([iq, iq[: 2 * N]]))
    tr = capi.TuneTracker(ctx, len(lengths), max_frames=9)
    try:
        got = tr.track([buf.ptr if n else None for n in lengths], lengths)
        zero = dict(frames=[], accepted=0, tune_first=0.0, tune_last=0.0, tune_min=0.0, tune_max=0.0, quality_min=0.0)
        assert got[0] == zero and got[2] == zero
        assert [len(g["frames"]) for g in got] == [0, 1, 0, 8, 8, 9, 1]
        assert [f["center"] for f in got[3]["frames"]] == [k * HOP + 2 * N for k in range(8)]          # the end frame is the eighth hop frame: once
        assert [f["center"] for f in got[4]["frames"]][-2:] == [6 * HOP + 2 * N, 7 * HOP - N + 2 * N]  # one block earlier: a frame of its own
        assert [f["center"] for f in got[5]["frames"]][-2:] == [7 * HOP + 2 * N, 7 * HOP + N + 2 * N]
        assert _bits(got[1]) == _bits(got[6]) and _bits(got[1])[2] == _bits(got[3])[2][:1]
        with pytest.raises(capi.LsdrError) as refusal:                                                # ten frames where nine fit: refused, nothing queued
            tr.track([buf.ptr] * len(lengths), [HEAD + HOP + N] * len(lengths))
        assert "max_frames" in str(refusal.value) and str(LSDR_E_ARG) in str(refusal.value)
        assert [_bits(g) for g in tr.track([buf.ptr if n else None for n in lengths], lengths)] == [_bits(g) for g in got]
    finally:
        tr.close()
        buf.free()


def test_tracker_arguments(capi, ctx):
    lib = capi.lib
    iq = _head(7.5, 2e-3, 0.0, 2 * HOP)
    buf = ctx.upload(iq)
    tr = capi.TuneTracker(ctx, 2, max_frames=4)
    want = None

    def usable():
        nonlocal want
        got = [_bits(g) for g in tr.track([buf.ptr, None], [2 * HOP, 0])]
        assert len(got[0][2]) == 3 and got[1][2] == []
        want = want or got
        assert got == want

    def message(rc, word):
        msg = lib.lsdr_last_error().decode()
        assert rc == LSDR_E_ARG and "tune_track" in msg and word in msg, (word, rc, msg)
        usable()

    try:
        usable()
        ptrs, lens = tr._args([buf.ptr, None], [2 * HOP, 0])
        message(lib.lsdr_tune_track_wait(tr.h, tr._sum, tr._frames), "in flight")                   # wait with nothing in flight
        tr.run_async([buf.ptr, None], [2 * HOP, 0])
        rc = lib.lsdr_tune_track_run_async(tr.h, ptrs, lens)                                        # a second run_async before wait
        msg = lib.lsdr_last_error().decode()
        assert rc == LSDR_E_ARG and "tune_track" in msg and "in flight" in msg, (rc, msg)
        assert [_bits(g) for g in tr.wait()] == want
        bad, _ = tr._args([buf.ptr + 1, None], [2 * HOP, 0])
        message(lib.lsdr_tune_track_run_async(tr.h, bad, lens), "aligned")
        bad, lens1 = tr._args([buf.ptr, None], [2 * HOP, N])
        message(lib.lsdr_tune_track_run_async(tr.h, bad, lens1), "pointer")
        _, lens5 = tr._args([buf.ptr, None], [4 * HOP, 0])                                          # five frames where four fit
        message(lib.lsdr_tune_track_run_async(tr.h, ptrs, lens5), "max_frames")
        e32 = capi.TuneTracker(ctx, 1, in_format=capi.IN_CF32, max_frames=4)                        # cf32 items want 8 bytes
        try:
            p, n1 = e32._args([buf.ptr + 4], [4 * N])
            message(lib.lsdr_tune_track_run_async(e32.h, p, n1), "aligned")
        finally:
            e32.close()
        for what, word, change in (("n_captures 0", "n_captures", lambda c: setattr(c, "n_captures", 0)), ("n_captures 65536", "n_captures", lambda c: setattr(c, "n_captures", 65536)),
                                   ("scale -1", "in_scale", lambda c: setattr(c, "in_scale", -1.0)), ("quality -1", "min_quality", lambda c: setattr(c, "min_quality", -1.0)),
                                   ("reserved", "reserved", lambda c: c.reserved.__setitem__(3, 1))):
            cfg = capi.TuneTrackCfg()
            cfg.n_captures, cfg.in_format = 2, capi.IN_CU8
            change(cfg)
            h = C.c_void_p()
            rc = lib.lsdr_tune_track_create(ctx.h, C.byref(cfg), C.byref(h))
            assert not h.value, what
            message(rc, word)
    finally:
        tr.close()
        buf.free()


def test_held_frames_and_the_gate(capi, ctx):
    hop, frames = 4 * N, 24
    n = frames * hop
    iq = _head(7.5, 2e-3, 0.0, n).copy()
    iq[2 * (n // 3): 2 * (2 * n // 3)] = _gaussian(2 * n // 3 - n // 3, 5)
    got, free = _track(capi, ctx, [iq, iq], hop=hop)[0], _track(capi, ctx, [iq], hop=hop, span=0)[0]
    _against_restatement(got, iq, "noise in the middle third", hop=hop)
    _against_restatement(free, iq, "noise in the middle third, span 0", hop=hop, span=0)
    held = [f["held"] for f in got["frames"]]
    inside = [k for k, f in enumerate(got["frames"]) if f["center"] - 2 * N >= n // 3 and f["center"] + 2 * N <= 2 * n // 3]
    print("held:", held, "bins:", [f["bin"] for f in got["frames"]], "span 0 bins:", [f["bin"] for f in free["frames"]])
    assert len(got["frames"]) == frames and len(inside) >= 6 and all(held[k] for k in inside) and not any(held[:7]) and not any(held[-7:])
    last, nxt = max(k for k in range(inside[0]) if not held[k]), min(k for k in range(inside[-1], frames) if not held[k])
    b0, b1 = got["frames"][last]["bin"], got["frames"][nxt]["bin"]
    assert all((f["bin"] - b0 + 64) % N <= 128 for f in got["frames"][last:nxt + 1])              # held frames searched the gate around the last accepted bin
    assert 0 < (b1 - b0) % N <= 64 and got["accepted"] == frames - sum(held)
    assert any(abs((f["bin"] - b0 + N // 2) % N - N // 2) > 64 for f in free["frames"][inside[0]:inside[-1] + 1])   # (ungated, noise peaks anywhere)


# ---- d -----------------------------------------------------------------------------------------------------------------------------
TRACKS = {"no knots": [],
          "one knot, on sample 0": [(0, 0.013)],
          "two knots in the middle, rising, a boundary inside a piece": [(1003, -0.02), (3001, 0.031)],
          "three knots, falling, the first on sample 0": [(0, 0.05), (5, -0.04), (4090, -0.2)],
          "200 knots three samples apart (pieces that straddle many boundaries)": [(3 * i + 1, float(0.1 * np.sin(0.7 * i))) for i in range(200)],
          "31 knots": [(100 + 37 * i * i, float(0.12 * np.sin(i))) for i in range(31)]}
LENGTHS = [1, 7, 8, 4097, 20000]
GUARD = 16


def _forms(capi, u8):
    s8 = (u8.astype(np.int16) - 128).astype(np.int8)
    s16 = (s8.astype(np.int16) * 256 + 77).astype(np.int16)
    return [("cu8", u8, dict()), ("cs8", s8, dict(in_format=capi.IN_CS8, in_scale=0.5)), ("cs16", s16, dict(in_format=capi.IN_CS16, in_scale=2.0 ** -8)),
            ("cu16", (s16.astype(np.int32) + 32768).astype(np.uint16), dict(in_format=capi.IN_CU16, in_scale=2.0 ** -7)),
            ("cf32", (s8.astype(np.float32) * np.float32(1.37)), dict(in_format=capi.IN_CF32, in_scale=1.0))]


def _derotate(capi, ctx, items, cases, ptr_offset=0, **kw):
    """The outputs (with GUARD items of room behind them, pre-filled) of one batch of (length, knots) cases reading the same items."""
    B, cap = len(cases), max(n for n, _ in cases) + GUARD
    fill = np.full(cap, np.complex64(complex(-7.25, 1234.5)))
    buf, outs = ctx.upload(items), [ctx.upload(fill) for _ in cases]
    d = capi.DerotateBatch(ctx, B, max(n for n, _ in cases), max([len(k) for _, k in cases] + [1]), **kw)
    try:
        d.run([buf.at(ptr_offset) if n else None for n, _ in cases], [n for n, _ in cases], [k for _, k in cases], [o.ptr for o in outs])
        return [ctx.download(o, np.complex64, cap) for o in outs], fill
    finally:
        d.close()
        buf.free()
        for o in outs:
            o.free()


def test_derotator_is_the_restatement_bit_for_bit(capi, ctx):
    trig = capi.trig16()
    u8 = _head(7.5, 2e-3, 0.0, max(LENGTHS) + 1)
    cases = [(n, k) for k in TRACKS.values() for n in LENGTHS] + [(0, TRACKS["31 knots"])]
    for fmt, items, kw in _forms(capi, u8):
        got, fill = _derotate(capi, ctx, items, cases, **kw)
        for (n, knots), out in zip(cases, got):
            want = trk.derotate(items[: 2 * n], knots, trig, fmt, kw.get("in_scale", 1.0))
            assert out[n:].tobytes() == fill[n:].tobytes(), (fmt, n, "written behind item n - 1")
            if knots:
                assert out[:n].tobytes() == want.tobytes(), (fmt, n, knots[:3])
            else:                                         # (the multiplication by (1, 0) may flip a zero's sign: values, not bits)
                xr, xi = trk.convert(items[: 2 * n], fmt, kw.get("in_scale", 1.0))
                assert np.array_equal(out[:n].real, xr) and np.array_equal(out[:n].imag, xi) and np.array_equal(out[:n], want), (fmt, n)
        # the item-wise loads: the same samples behind a pointer that is only item-aligned
        item = items.itemsize * 2
        moved, _ = _derotate(capi, ctx, np.concatenate([np.zeros(2, items.dtype), items]), cases, ptr_offset=item, **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(moved, got)), fmt
    # the rotation does something: the 31-knot track turns the samples
    assert not np.array_equal(got[len(cases) - 2][:20000], got[4][:20000])


def test_derotator_composition(capi, ctx):
    u8 = _head(7.5, 2e-3, 0.0, max(LENGTHS) + 1)
    cases = [(n, k) for k in list(TRACKS.values())[1:] for n in (4097, 20000)]
    got, _ = _derotate(capi, ctx, u8, cases)
    back, _ = _derotate(capi, ctx, u8, cases[::-1])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, back[::-1]))
    for i in (0, 3, 7):
        alone, _ = _derotate(capi, ctx, u8, [cases[i]])
        mates, _ = _derotate(capi, ctx, u8, [(8, []), cases[i], (20000, TRACKS["31 knots"])])
        m = cases[i][0] + GUARD
        assert alone[0][:m].tobytes() == got[i][:m].tobytes() == mates[1][:m].tobytes(), i


def test_derotator_arguments(capi, ctx):
    lib = capi.lib
    u8 = _head(7.5, 2e-3, 0.0, 4097)
    buf, out = ctx.upload(u8), ctx.alloc(4097 * 8 + 16)
    d = capi.DerotateBatch(ctx, 1, 4097, 3)
    good = [(10, 0.01), (2000, -0.02)]
    want = None

    def usable():
        nonlocal want
        d.run([buf.ptr], [4097], [good], [out.ptr])
        got = ctx.download(out, np.complex64, 4097).tobytes()
        want = want or got
        assert got == want

    def refused(word, ptr=None, n=4097, knots=good, o=None):
        p, e, outs, keep = d._args([buf.ptr if ptr is None else ptr], [n], [knots], [out.ptr if o is None else o])
        rc = lib.lsdr_derotate_batch_run_async(d.h, p, e, outs)
        msg = lib.lsdr_last_error().decode()
        assert rc == LSDR_E_ARG and "derotate_batch" in msg and word in msg, (word, rc, msg)
        usable()

    try:
        usable()
        assert want == trk.derotate(u8, good, capi.trig16()).tobytes()
        refused("ascend", knots=[(10, 0.0), (9, 0.0)])
        refused("ascend", knots=[(10, 0.0), (10, 0.1)])
        refused("2^31", knots=[(1 << 31, 0.0)])
        refused("finite", knots=[(1, float("nan"))])
        refused("finite", knots=[(1, 0.1), (2, 0.5)])
        refused("finite", knots=[(1, -0.5)])
        refused("less than 0.5", knots=[(1, 0.3), (2, -0.3)])
        refused("aligned", ptr=buf.ptr + 1)
        refused("16 bytes", o=out.ptr + 8)
        refused("max_samples", n=4098)
        refused("max_knots", knots=[(1, 0.0), (2, 0.0), (3, 0.0), (4, 0.0)])
        refused("no pointer", ptr=0)
        p, e, outs, keep = d._args([buf.ptr], [4097], [good], [out.ptr])
        assert lib.lsdr_derotate_batch_wait(d.h) == LSDR_E_ARG and "in flight" in lib.lsdr_last_error().decode()
        d.run_async([buf.ptr], [4097], [good], [out.ptr])
        assert lib.lsdr_derotate_batch_run_async(d.h, p, e, outs) == LSDR_E_ARG and "in flight" in lib.lsdr_last_error().decode()
        d.wait()
        usable()
        for what, word, change in (("n_captures 0", "n_captures", lambda c: setattr(c, "n_captures", 0)), ("format 5", "in_format", lambda c: setattr(c, "in_format", 5)),
                                   ("max_knots 2^20 + 1", "max_knots", lambda c: setattr(c, "max_knots", (1 << 20) + 1)),
                                   ("a table of 2^22 + 8 segments", "table", lambda c: (setattr(c, "n_captures", 8), setattr(c, "max_knots", 1 << 19))),
                                   ("scale nan", "in_scale", lambda c: setattr(c, "in_scale", float("nan"))), ("reserved", "reserved", lambda c: c.reserved.__setitem__(3, 1))):
            cfg = capi.DerotateBatchCfg()
            cfg.n_captures, cfg.in_format, cfg.max_knots, cfg.max_samples = 1, capi.IN_CU8, 3, 4097
            change(cfg)
            h = C.c_void_p()
            assert lib.lsdr_derotate_batch_create(ctx.h, C.byref(cfg), C.byref(h)) == LSDR_E_ARG and word in lib.lsdr_last_error().decode() and not h.value, what
        for what, word, kw in (("blocks 17", "blocks", dict(blocks=17)), ("hop 1000", "hop", dict(hop=1000)), ("span 2048", "span", dict(span=2048)),
                               ("quality nan", "min_quality", dict(min_quality=float("nan"))), ("format 9", "in_format", dict(in_format=9))):
            with pytest.raises(capi.LsdrError) as r:
                capi.TuneTracker(ctx, 1, **kw)
            assert "tune_track" in str(r.value) and word in str(r.value) and str(LSDR_E_ARG) in str(r.value), what
        usable()
    finally:
        d.close()
        buf.free()
        out.free()


# ---- e -----------------------------------------------------------------------------------------------------------------------------
BATCH_KW = dict(tile_len=4096, tile_warmup=512)
# capture → (noise, the moving offset, engine, leandvb's extra arguments, what the reference returns for the clean capture, sent packets asked)
LOOP = {"drift 2e-3, noise 7.5": (7.5, ("drift", 2e-3), "default", ("--anf", "0"), 946, False),
        "ramp -1.5e-3 to 1.5e-3, noise 7.5": (7.5, ("ramp", 1.5e-3), "default", ("--anf", "0"), 946, False),
        "drift 2e-3, noise 18": (18.0, ("drift", 2e-3), "viterbi", ("--viterbi", "--anf", "0"), 932, True)}


def _moving(noise, how):
    iq = bc.capture(1000, 11, noise)[0]
    return trk.drifted_capture(noise, how[1], 0.0)[0] if how[0] == "drift" else trk.ramped(iq, -how[1], how[1])


@pytest.fixture(scope="module")
def loop_inputs():
    """name → (the moving capture's bytes, the reference's TS for them), the references eight processes at a time, once."""
    iqs = {name: _moving(c[0], c[1]) for name, c in LOOP.items()}
    with ThreadPoolExecutor(max_workers=8) as ex:
        refs = list(ex.map(lambda name: bc.run_reference(bc.REF_U8 + LOOP[name][3], iqs[name]), LOOP))
    return {name: (iqs[name], ref) for name, ref in zip(LOOP, refs)}


@pytest.fixture(scope="module")
def decoders(capi, ctx):
    made = {}

    def get(engine):
        if engine not in made:
            made[engine] = capi.TrackedDecoder(ctx, 2, N_ALL, OMEGA, viterbi=engine == "viterbi", anf=0, batch_kw=BATCH_KW)
        return made[engine]
    yield get
    for d in made.values():
        d.close()


@pytest.fixture(scope="module")
def plain_batch(capi, ctx):
    cb = capi.CaptureBatch(ctx, 2, N_ALL, OMEGA, anf=0, **BATCH_KW)
    yield cb
    cb.close()


@pytest.mark.parametrize("engine", ["default", "viterbi"])
def test_the_loop_closed(capi, ctx, loop_inputs, decoders, engine):
    names = [n for n, c in LOOP.items() if c[2] == engine]
    sent = {noise: bc.capture(1000, 11, noise)[1] for noise in (7.5, 18.0)}
    bufs = [ctx.upload(loop_inputs[n][0]) for n in names]
    try:
        dec = decoders(engine)
        ptrs, lengths = [b.ptr for b in bufs] + [None] * (2 - len(bufs)), [N_ALL] * len(bufs) + [0] * (2 - len(bufs))
        res, ts, tracks = dec.decode(ptrs, lengths)                                                   # tune NOT given
        for i, name in enumerate(names):
            noise, how, _, _, ref_packets, ask_sent = LOOP[name]
            t = tracks[i]
            print(f"{name}: {len(t['frames'])} frames, {t['accepted']} accepted, tune {t['tune_min']:.2e} ... {t['tune_max']:.2e}, quality at least {t['quality_min']:.0f}; "
                  f"{res[i]['ts_packets']} packets, reference {len(loop_inputs[name][1]) // 188}")
            assert len(t["frames"]) == 31 and t["accepted"] == 31
            bc.check_against_reference(ts[i], loop_inputs[name][1], sent[noise] if ask_sent else None, ref_packets - 10, f"{name} tracked", False)
            assert res[i]["locked"] == 1 and res[i]["seam_bad"] == 0, res[i]
        if len(names) < 2:
            assert tracks[1]["frames"] == [] and res[1]["ts_packets"] == 0
    finally:
        for b in bufs:
            b.free()


def test_without_the_tracker_the_drifted_capture_is_lost(capi, ctx, loop_inputs, plain_batch):
    """The test that fails without the feature: one tune per capture, estimated at its start, loses the capture.  A = 2e-3."""
    name = "drift 2e-3, noise 7.5"
    iq, ref = loop_inputs[name]
    assert len(ref) // 188 >= 936, f"invalid input: the reference returns {len(ref) // 188} packets"
    buf = ctx.upload(iq)
    try:
        res, ts, est = plain_batch.decode_estimated([buf.ptr, None], [N_ALL, 0])
        print(f"{name} through decode_estimated (tune {est[0]['tune']:.2e}, quality {est[0]['quality']:.0f}): {len(ts[0]) // 188} packets, reference {len(ref) // 188}")
        assert est[0]["quality"] >= capi.TUNE_MIN_QUALITY
        assert len(ts[0]) // 188 < len(ref) // 188 // 2
    finally:
        buf.free()


def test_a_capture_without_a_line_passes_through(capi, ctx, decoders):
    """A capture with no accepted frame is derotated by nothing: the decoder sees the converted samples."""
    n = 3 * HOP
    noise = _gaussian(n, 3)
    buf = ctx.upload(noise)
    try:
        dec = decoders("default")
        res, ts, tracks = dec.decode([buf.ptr, None], [n, 0])
        assert tracks[0]["accepted"] == 0 and len(tracks[0]["frames"]) == 4 and all(f["held"] for f in tracks[0]["frames"])
        xr, xi = trk.convert(noise)
        out = dec.outputs(0, n)
        assert np.array_equal(out.real, xr) and np.array_equal(out.imag, xi) and res[0]["ts_packets"] == 0
    finally:
        buf.free()


# ---- f -----------------------------------------------------------------------------------------------------------------------------
PIECE, OVERLAP = 1000000, 500000


def test_recording_with_a_tune_per_piece(capi, ctx):
    iq = trk.ramped(bc.capture(2500, 3, 7.5)[0], -1.5e-3, 1.5e-3)
    n = len(iq) // 2
    with ThreadPoolExecutor(max_workers=1) as ex:
        ref = ex.submit(bc.run_reference, bc.REF_U8, iq)
        buf = ctx.upload(iq)
        try:
            out = {}
            for tune in ("pieces", None):
                dec = capi.RecordingDecoder(ctx, PIECE, OVERLAP, 9, 1.2, tune=tune)
                try:
                    out[tune] = dec.decode(buf.ptr, n)
                finally:
                    dec.close()
        finally:
            buf.free()
        rpk = bc.packets(ref.result())
    ts, report = out["pieces"]
    pk = bc.packets(ts)
    print("tunes per piece:", [f"{t:.2e}" for t in report["tunes"]], "packets", len(pk), "reference", len(rpk), "with tune=None:", out[None][1]["packets"],
          "its tune", out[None][1]["tune"])
    assert report["tune"] == "pieces" and len(report["tunes"]) == 9 == len(report["pieces"]) and out[None][1]["tunes"] == [out[None][1]["tune"]] * 9
    starts = [p["first_sample"] for p in report["pieces"]]
    assert all(abs(t - (-1.5e-3 + 3e-3 * (s + 4 * N) / n)) <= tc.W8 * 8 for t, s in zip(report["tunes"], starts)), report["tunes"]
    assert all(j["joined"] == 1 for j in report["joins"]) and report["unjoined"] == [] and len(report["joins"]) == 8
    # test_gpu_recording.py's rule (d)
    assert len(rpk) > 2300, f"invalid input, the reference returns {len(rpk)} packets"
    where = {}
    for j, p in enumerate(rpk):
        where.setdefault(p, j)
    i0 = next(i for i, p in enumerate(pk) if p in where)
    j0 = where[pk[i0]]
    m = min(len(pk) - i0, len(rpk) - j0)
    print(f"pair at {i0} / {j0}, compared {m}, not reached {len(rpk) - j0 - m}")
    assert pk[i0:i0 + m] == rpk[j0:j0 + m], "differs from the whole capture's TS"
    assert len(pk) - i0 == m, f"{len(pk) - i0 - m} packets behind the reference's last"
    assert len(rpk) - j0 - m <= 8, f"{len(rpk) - j0 - m} of the reference's last packets not reached"
    assert i0 <= 8 and j0 <= 8, f"the first common packet is at {i0} / {j0}"
    assert out[None][1]["packets"] < report["packets"]
