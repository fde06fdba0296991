"""lsdr_tune_est on the GPU: every capture's carrier offset estimated from its raw samples, and the batch decoders run with the estimates.

  a the device against the float64 restatement (tune_common.estimate) and against the TRUE offset: 16 shifted captures in one batch;
  b the five sample formats of the same samples give the cu8 record bit for bit;
  c lengths and composition: whole blocks only, all-zero records where there is none, a capture's record does not depend on the batch it
    is in or on its place, two runs are equal, the longest grid (64 blocks), a pointer that is only item-aligned;
  d every refusal is LSDR_E_ARG with a message and leaves a usable object;
  e the loop closed: captures shifted by offsets the tiles cannot follow, decoded by decode_estimated with NO tune given, against
    `leandvb --tune` with the true offset — and, with tune 0 and no estimator, the 3e-3 capture loses more than half its packets.

Bounds: |tune − offset| ≤ W/8 (tune_common.W8 = 7.6e-6: an eighth of the narrowest tuning window); powers within 1e-4·c of the restatement's
(float32 FFT against float64); tune within 1e-7 of the formula evaluated in float64 on the device's own powers.  tune is not compared with
the restatement's directly: where l ≈ r the sign of δ may legitimately differ.
Measured on an MI355X: powers within 2.1e-7·c, tune within 2.8e-9 of the formula, max |tune − offset| 2.26e-6, quality 347 … 1380; untuned,
the 3e-3 capture returns 0 packets from all three decoders.
The reference binary (oracle/_ref/leandvb) is required by e: where it is missing that test FAILS.
"""
import ctypes as C

import numpy as np
import pytest
import tune_common as tc
from batch_common import REF_U8, capture, check_against_reference, references, shifted

pytestmark = pytest.mark.gpu

LSDR_E_ARG = -2
N = tc.N
# the shifted-capture constants of test_gpu_capture_each.py and test_gpu_hs_each.py
OMEGA = 1.2
FS = 2400e3
N_ALL = 1958423
FREQS = [0.0, 1e-3, -1e-3, 3e-3]
# decoder → (noise, leandvb's extra arguments, what the reference returns for every one of FREQS tuned, sent packets asked, from first compared)
DECODERS = {"default": (7.5, ("--anf", "0"), 946, False, False), "viterbi": (18.0, ("--viterbi", "--anf", "0"), 932, True, False),
            "hs": (7.5, ("--hs",), 956, True, True)}


def _same(a, b):
    """Two records bit for bit (floats compared by their bits)."""
    f = lambda r: (np.array([r["tune"], r["quality"], r["mean_power"]] + r["power"], np.float32).tobytes(), r["bin"], r["blocks"])
    return f(a) == f(b)


def _estimate(capi, ctx, arrays, lengths=None, **kw):
    """One batch of host arrays (None: no pointer), whole or their first lengths[i] items."""
    bufs = [ctx.upload(a) if a is not None else None for a in arrays]
    est = capi.TuneEstimator(ctx, len(arrays), **kw)
    try:
        if lengths is None:
            lengths = [len(a) // 2 for a in arrays]
        return est.estimate([b.ptr if b else None for b in bufs], lengths)
    finally:
        est.close()
        for b in bufs:
            if b:
                b.free()


# ---- a -----------------------------------------------------------------------------------------------------------------------------
def test_against_the_restatement_and_the_truth(capi, ctx):
    cases = tc.sixteen()
    got = _estimate(capi, ctx, [iq for _, _, iq in cases])
    d_pow = d_tune = d_true = 0.0
    quals = []
    for (noise, f, iq), g in zip(cases, got):
        w = tc.estimate(tc.to_complex(iq))
        name = f"noise {noise} offset {f}"
        assert g["blocks"] == 8 and g["bin"] == w["bin"], (name, g, w)
        c = w["power"][1]
        dp = max(abs(a - b) for a, b in zip(g["power"] + [g["mean_power"]], w["power"] + [w["mean_power"]])) / c
        dt = abs(g["tune"] - tc.tune_from_peak(g["bin"], *g["power"]))
        d_pow, d_tune, d_true = max(d_pow, dp), max(d_tune, dt), max(d_true, abs(g["tune"] - f))
        quals.append(g["quality"])
        assert dp <= 1e-4, (name, dp)
        assert dt <= 1e-7, (name, dt)
        assert abs(g["tune"] - f) <= tc.W8, (name, g["tune"])
        assert g["quality"] == pytest.approx(g["power"][1] / g["mean_power"], rel=1e-6)
    print(f"device against the restatement: powers within {d_pow:.2e} of c, tune within {d_tune:.2e} of the formula; "
          f"max |tune - offset| {d_true:.3e} (bound {tc.W8:.3e}); quality {min(quals):.0f} ... {max(quals):.0f}")


# ---- b -----------------------------------------------------------------------------------------------------------------------------
def test_formats_give_the_same_record(capi, ctx):
    u8 = tc.shifted_head(18.0, 3e-3)
    s8 = (u8.astype(np.int16) - 128).astype(np.int8)
    s16 = (s8.astype(np.int16) * 256).astype(np.int16)
    u16 = (s16.astype(np.int32) + 32768).astype(np.uint16)
    f32 = s8.astype(np.float32)
    base = _estimate(capi, ctx, [u8])[0]
    assert base["blocks"] == 8 and abs(base["tune"] - 3e-3) <= tc.W8
    for name, items, kw in (("cs8", s8, dict(in_format=capi.IN_CS8)), ("cs16 scaled", s16, dict(in_format=capi.IN_CS16, in_scale=2.0 ** -8)),
                            ("cu16 scaled", u16, dict(in_format=capi.IN_CU16, in_scale=2.0 ** -8)),
                            ("cf32", f32, dict(in_format=capi.IN_CF32, in_scale=1.0)), ("cu8 scale 1", u8, dict(in_scale=1.0))):
        got = _estimate(capi, ctx, [items], **kw)[0]
        assert _same(got, base), (name, got, base)
    raw = _estimate(capi, ctx, [s16], in_format=capi.IN_CS16)[0]           # 256 times larger: the normalisation takes it
    assert np.isfinite(raw["quality"]) and raw["quality"] > 100 and raw["bin"] == base["bin"] and abs(raw["tune"] - base["tune"]) <= 1e-7, (raw, base)


# ---- c -----------------------------------------------------------------------------------------------------------------------------
def test_composition_and_lengths(capi, ctx):
    iq = tc.shifted_head(7.5, 1e-3, 9)
    lengths = [8 * N, 8 * N + 4095, N, N - 1, 0, 3 * N + 1]
    B = len(lengths)
    buf = ctx.upload(iq)
    ptrs = [buf.ptr if n else None for n in lengths]
    zero = dict(tune=0.0, quality=0.0, bin=0, blocks=0, power=[0.0, 0.0, 0.0], mean_power=0.0)
    est = capi.TuneEstimator(ctx, B)
    one = capi.TuneEstimator(ctx, 1)
    try:
        got = est.estimate(ptrs, lengths)
        assert [g["blocks"] for g in got] == [8, 8, 1, 0, 0, 3]
        assert got[3] == zero and got[4] == zero
        assert _same(got[0], got[1]) and not _same(got[0], got[5])
        for g, n in zip(got, lengths):                                      # … and every one is the restatement's
            w = tc.estimate(tc.to_complex(iq[: 2 * n]))
            assert g["bin"] == w["bin"] and abs(g["power"][1] - w["power"][1]) <= 1e-4 * max(w["power"][1], 1.0), (n, g, w)
        again = est.estimate(ptrs, lengths)
        assert all(_same(a, b) for a, b in zip(got, again))
        back = est.estimate(ptrs[::-1], lengths[::-1])
        assert all(_same(a, b) for a, b in zip(got, back[::-1]))
        for i, n in enumerate(lengths):
            alone = one.estimate([ptrs[i]], [n])[0]
            assert _same(alone, got[i]), (n, alone, got[i])
        # a pointer that is item-aligned only (the item-wise loads): the same samples give the same record
        moved = ctx.upload(np.concatenate([np.zeros(2, np.uint8), iq]))
        try:
            assert _same(one.estimate([moved.at(2)], [8 * N])[0], got[0])
        finally:
            moved.free()
    finally:
        est.close()
        one.close()
        buf.free()


def test_the_longest_grid(capi, ctx):
    f = -0.05
    long_iq = tc.shifted_head(18.0, f, 64)
    got = _estimate(capi, ctx, [long_iq, long_iq], [64 * N, N], blocks=64)
    w64, w1 = tc.estimate(tc.to_complex(long_iq), 64), tc.estimate(tc.to_complex(long_iq[: 2 * N]), 64)
    assert [g["blocks"] for g in got] == [64, 1] and w64["blocks"] == 64
    assert got[0]["bin"] == w64["bin"] and got[1]["bin"] == w1["bin"]
    assert abs(got[0]["power"][1] - w64["power"][1]) <= 1e-4 * w64["power"][1] and abs(got[1]["power"][1] - w1["power"][1]) <= 1e-4 * w1["power"][1]
    assert abs(got[0]["tune"] - f) <= tc.W8, got[0]
    print(f"64 blocks: tune off by {abs(got[0]['tune'] - f):.3e}, quality {got[0]['quality']:.0f}; one block: off by {abs(got[1]['tune'] - f):.3e}, quality {got[1]['quality']:.0f}")


# ---- d -----------------------------------------------------------------------------------------------------------------------------
def test_arguments(capi, ctx):
    lib = capi.lib
    iq = tc.shifted_head(7.5, 1e-3)
    buf = ctx.upload(iq)
    est = capi.TuneEstimator(ctx, 2)
    want = None

    def usable():
        nonlocal want
        got = est.estimate([buf.ptr, None], [8 * N, 0])
        assert got[0]["blocks"] == 8 and got[1]["blocks"] == 0 and abs(got[0]["tune"] - 1e-3) <= tc.W8
        want = want or got
        assert all(_same(a, b) for a, b in zip(got, want))

    def message(rc, what):
        msg = lib.lsdr_last_error().decode()
        assert rc == LSDR_E_ARG and "tune_est" in msg, (what, rc, msg)
        return msg

    try:
        usable()
        for what, word, change in (("n_captures 0", "n_captures", lambda c: setattr(c, "n_captures", 0)),
                                   ("n_captures -1", "n_captures", lambda c: setattr(c, "n_captures", -1)),
                                   ("format 5", "in_format", lambda c: setattr(c, "in_format", 5)),
                                   ("format -1", "in_format", lambda c: setattr(c, "in_format", -1)),
                                   ("scale -1", "in_scale", lambda c: setattr(c, "in_scale", -1.0)),
                                   ("scale nan", "in_scale", lambda c: setattr(c, "in_scale", float("nan"))),
                                   ("scale inf", "in_scale", lambda c: setattr(c, "in_scale", float("inf"))),
                                   ("blocks 65", "blocks", lambda c: setattr(c, "blocks", 65)),
                                   ("reserved", "reserved", lambda c: c.reserved.__setitem__(3, 1))):
            cfg = capi.TuneEstCfg()
            cfg.n_captures, cfg.in_format, cfg.in_scale, cfg.blocks = 2, capi.IN_CU8, 0.0, 8
            change(cfg)
            h = C.c_void_p()
            assert word in message(lib.lsdr_tune_est_create(ctx.h, C.byref(cfg), C.byref(h)), what) and not h.value
            usable()
        # more captures than the grid's second dimension takes: refused in front of any allocation, and an estimator made afterwards works
        with pytest.raises(capi.LsdrError) as refusal:
            capi.TuneEstimator(ctx, 65536)
        assert str(refusal.value) == f"lsdr error {LSDR_E_ARG}: tune_est: n_captures must be 1 to 65535 (got 65536)"
        after = capi.TuneEstimator(ctx, 2)
        try:
            assert all(_same(a, b) for a, b in zip(after.estimate([buf.ptr, None], [8 * N, 0]), want))
        finally:
            after.close()
        usable()
        ptrs, lens = est._args([buf.ptr, None], [8 * N, 0])
        assert "in flight" in message(lib.lsdr_tune_est_wait(est.h, est._out), "wait with nothing in flight")
        usable()
        est.run_async([buf.ptr, None], [8 * N, 0])
        assert "in flight" in message(lib.lsdr_tune_est_run_async(est.h, ptrs, lens), "a second run_async before wait")
        assert all(_same(a, b) for a, b in zip(est.wait(), want))
        usable()
        bad, _ = est._args([buf.ptr + 1, None], [8 * N, 0])
        assert "aligned" in message(lib.lsdr_tune_est_run_async(est.h, bad, lens), "a misaligned pointer")
        usable()
        bad, lens1 = est._args([buf.ptr, None], [8 * N, N])
        assert "pointer" in message(lib.lsdr_tune_est_run_async(est.h, bad, lens1), "samples without a pointer")
        usable()
        # cf32 items want 8 bytes
        e32 = capi.TuneEstimator(ctx, 1, in_format=capi.IN_CF32)
        try:
            p, n1 = e32._args([buf.ptr + 4], [N])
            assert "aligned" in message(lib.lsdr_tune_est_run_async(e32.h, p, n1), "cf32 at 4 bytes")
        finally:
            e32.close()
        usable()
    finally:
        est.close()
        buf.free()


# ---- e -----------------------------------------------------------------------------------------------------------------------------
def _make(capi, ctx, decoder, n):
    if decoder == "hs":
        return capi.HsBatch(ctx, n, N_ALL, OMEGA, fastlock=0)
    return capi.CaptureBatch(ctx, n, N_ALL, OMEGA, anf=0, tile_len=4096, tile_warmup=512, viterbi=decoder == "viterbi")


@pytest.mark.parametrize("decoder", ["default", "viterbi", "hs"])
def test_the_loop_closed(capi, ctx, decoder):
    noise, extra, ref_packets, ask_sent, from_first = DECODERS[decoder]
    iq, sent = capture(1000, 11, noise)
    assert len(iq) == 2 * N_ALL
    refs = references([(REF_U8 + extra + ("--tune", repr(f * FS)), 1000, 11, noise, None, f) for f in FREQS])
    bufs = [ctx.upload(shifted(iq, f) if f else iq) for f in FREQS]
    obj = _make(capi, ctx, decoder, len(FREQS))
    try:
        res, ts, est = obj.decode_estimated([b.ptr for b in bufs], [N_ALL] * len(FREQS))       # tune NOT given
        for i, f in enumerate(FREQS):
            assert est[i]["blocks"] == 8 and est[i]["quality"] >= capi.TUNE_MIN_QUALITY and abs(est[i]["tune"] - f) <= tc.W8, (f, est[i])
            check_against_reference(ts[i], refs[i], sent if ask_sent else None, ref_packets - 10, f"{decoder} offset {f} estimated", from_first)
            assert res[i]["locked"] == 1 and res[i]["seam_bad"] == 0, res[i]
        # the test has teeth: untuned and without the estimator, the 3e-3 capture is lost
        res0, ts0 = obj.decode_each([b.ptr for b in bufs], [N_ALL] * len(FREQS), 0.0)
        print(f"{decoder}: offset 3e-3 decoded with tune 0: {res0[3]['ts_packets']} packets (reference, tuned: {len(refs[3]) // 188})")
        assert len(ts0[3]) // 188 < len(refs[3]) // 188 // 2
        # a capture with no line is decoded with tune 0: what decode_each gives for it
        low = obj.decode_estimated([b.ptr for b in bufs], [N_ALL] * len(FREQS), min_quality=1e9)
        assert low[1] == ts0 and low[0] == res0
    finally:
        obj.close()
        for b in bufs:
            b.free()
