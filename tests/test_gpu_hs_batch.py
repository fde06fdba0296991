"""lsdr_hs_batch: B independent cu8 captures, each from its first sample to TS by leandvb's `--hs` graph per capture
(fast_qpsk_receiver<u8> → dvb_deconvol_sync<u8> → mpeg_sync(deconv = NULL, fastlock) → deinterleaver → rs_decoder → derandomizer), in
shared launches with every count on the device.

  * whole job: every capture's TS against the reference BINARY's for the same IQ (`leandvb --u8 -f 2400e3 --sr 2000e3 --cr 1/2 --hs`),
    with and without --fastlock, with a carrier offset inside the tile window and with one that needs --tune;
  * receiver: the hard symbols against the oracle's exact serial receiver — tile 0 bit for bit, the count equal, the share of equal
    decisions at least 0.999 (the bound of tests/test_gpu_hs.py for this arithmetic);
  * deconvolver and tail: given the object's own symbols, bytes / mpeg bytes / TS / counters are what the one-block-per-call C ABI gives
    when the host drives it, bit for bit;
  * a capture's output does not depend on what else is in the batch, nor on what the object decoded before.

Captures: synth_dvbs.capture_u8(600 packets, 1.2 samples per symbol): 1 175 063 samples — no multiple of 128 —, about 1 150 tiles at the
default 1 024-sample tile, 1 912 deconvolver chunks, 59 resyncs at P = 32.
The reference binary (oracle/_ref/leandvb) is required: where it is missing these tests FAIL.
"""
import functools

import numpy as np
import pytest
from batch_common import REF_U8, HostTail, capture, check_against_reference, decode_batch, references, shifted, six_variants

pytestmark = pytest.mark.gpu

REF_ARGS = REF_U8 + ("--hs",)
FS = 2400e3
OMEGA = 1.2
CAPS = [(21, 6.0), (22, 9.0), (23, 12.0), (24, 7.5)]      # (seed, noise_std)
N_SAMPLES = 1175063


def _capture(seed, noise_std):
    iq, sent = capture(600, seed, noise_std)
    assert len(iq) == 2 * N_SAMPLES
    return iq, sent


def _decode(capi, ctx, iqs, n_samples, hb=None, **kw):
    """One batch on a (new, unless given) object: (object, results, TS per capture)."""
    return decode_batch(ctx, iqs, n_samples, lambda: capi.HsBatch(ctx, len(iqs), n_samples, OMEGA, **kw), hb)


@functools.lru_cache(maxsize=None)
def _batch_of_four(capi, ctx, fastlock, tile_len, tile_warmup):
    """The four captures in one batch (computed once, shared by the tests that need it): (results, TS, symbols of capture 2)."""
    hb, res, ts = _decode(capi, ctx, [_capture(*c)[0] for c in CAPS], N_SAMPLES, fastlock=fastlock, tile_len=tile_len, tile_warmup=tile_warmup)
    try:
        sym2 = hb.symbols(2, res[2]["symbols"]).tobytes()
        assert hb.symbols_ptr(4) is None and hb.symbols_ptr(-1) is None
    finally:
        hb.close()
    return res, ts, sym2


@pytest.mark.parametrize("tile_len,tile_warmup", [(0, 0), (2048, 512)])
@pytest.mark.parametrize("fastlock", [0, 1])
def test_captures_decode_to_the_reference_ts(capi, ctx, fastlock, tile_len, tile_warmup):
    extra = ("--fastlock",) if fastlock else ()
    refs = references([(REF_ARGS + extra, 600, s, nz) for s, nz in CAPS])
    res, ts, _ = _batch_of_four(capi, ctx, fastlock, tile_len, tile_warmup)
    for i, (s, nz) in enumerate(CAPS):
        check_against_reference(ts[i], refs[i], _capture(s, nz)[1], 540, f"seed {s} noise {nz} fastlock {fastlock} tile {tile_len}", True)
        r = res[i]
        assert r["locked"] == 1 and r["seam_bad"] == 0 and r["next_sync_calls"] == 0, r
        assert r["samples"] == (N_SAMPLES - 1) // 128 * 128 and r["ts_packets"] * 188 == len(ts[i])
        assert r["bytes_deconv"] == r["symbols"] // 512 * 64, r


def test_symbols_against_the_oracle(capi, ctx, oracle):
    picks = [(24, 7.5), (21, 6.0)]
    iqs = [_capture(*c)[0] for c in picks]
    hb, res, _ = _decode(capi, ctx, iqs, N_SAMPLES)
    try:
        for i, c in enumerate(picks):
            want = oracle.fast_qpsk(iqs[i], OMEGA)["sym"]
            r = res[i]
            got = hb.symbols(i, r["symbols"])
            assert r["samples"] == (N_SAMPLES - 1) // 128 * 128
            first = int(1024 / OMEGA) - 8                       # tile 0: the first max(tile, warm-up) = 1024 samples' worth
            assert got[:first].tobytes() == want[:first].tobytes(), f"{c}: tile 0 is not the reference's"
            assert len(got) == len(want), (c, len(got), len(want), r)
            same = float((got == want).mean())
            print(f"capture {c}: {len(got)} symbols, {r['tiles']} tiles, {int((got != want).sum())} decisions differ (share equal {same:.7f}), "
                  f"seams dup {r['seam_dup']} miss {r['seam_miss']} bad {r['seam_bad']}")
            assert same >= 0.999, (c, same)
            assert r["seam_bad"] == 0, r
    finally:
        hb.close()


def _stage_reference(capi, ctx, sym, P):
    """What the one-block-per-call C ABI makes of hard symbols when the host drives it: a fresh dvb_deconvol_sync in front of
    batch_common.HostTail with mpeg_sync(fastlock = 1, resync_period P)."""
    d = capi.HsDeconv(ctx, P)
    by = d.run_stream(sym)
    alignment = int(d.locked)
    d.close()
    t = HostTail(capi, ctx, len(by) + 4096, fastlock=1, resync_period=P, data=by)
    t.sync()
    want_bytes, want_mpeg, want_ts, st = t.finish()
    return want_bytes, want_mpeg, want_ts.tobytes(), dict(st, alignment=alignment)


def _assert_stages_exact(capi, ctx, hb, res, ts, names, P):
    for i, name in enumerate(names):
        r = res[i]
        sym = hb.symbols(i, r["symbols"])
        assert sym.max(initial=0) <= 3
        want_bytes, want_mpeg, want_ts, st = _stage_reference(capi, ctx, sym, P)
        got_bytes = hb.stage_bytes(i, "deconv", r["bytes_deconv"])
        got_mpeg = hb.stage_bytes(i, "mpeg", r["bytes_mpeg"])
        assert r["bytes_deconv"] == len(want_bytes) == r["symbols"] // 512 * 64, (name, r, len(want_bytes))
        assert got_bytes.tobytes() == want_bytes.tobytes(), name
        assert r["alignment"] == st["alignment"], (name, r, st)
        assert r["bytes_mpeg"] == len(want_mpeg) and got_mpeg.tobytes() == want_mpeg.tobytes(), name
        assert r["rs_packets"] == st["npk"] and r["locked"] == st["locked"] and r["rs_bit_errors"] == st["errs"], (name, r, st)
        assert r["next_sync_calls"] == 0, (name, r)
        assert ts[i] == want_ts, name


@pytest.mark.parametrize("fastlock", [0, 1])
def test_deconvolver_and_tail_are_exact_on_the_objects_own_symbols(capi, ctx, fastlock):
    P = 1 if fastlock else 32
    base = _capture(23, 12.0)[0]
    n = N_SAMPLES
    variants = six_variants(base, n, 100000)
    variants.insert(4, ("I/Q swapped", np.ascontiguousarray(base.reshape(-1, 2)[:, ::-1]).reshape(-1)))
    names = [v[0] for v in variants]
    hb, res, ts = _decode(capi, ctx, [v for _, v in variants], n, fastlock=fastlock)
    try:
        _assert_stages_exact(capi, ctx, hb, res, ts, names, P)
        print("packets:", [r["ts_packets"] for r in res], "alignments:", [r["alignment"] for r in res])
        assert all(res[i]["ts_packets"] >= 540 and res[i]["locked"] == 1 for i in range(5)), res
        assert len({res[i]["alignment"] for i in range(4)}) > 1
        assert 300 <= res[5]["ts_packets"] <= 550, res[5]
        assert res[6]["ts_packets"] == 0 and res[6]["locked"] == 0, res[6]
        # the first 300 000 samples on the same object
        _, res2, ts2 = _decode(capi, ctx, [v for _, v in variants], 300000, hb=hb)
        assert all(r["samples"] == (300000 - 1) // 128 * 128 for r in res2)
        assert res2[0]["ts_packets"] > 50, res2[0]
        _assert_stages_exact(capi, ctx, hb, res2, ts2, [f"short run, {nm}" for nm in names], P)
        # … and a run too short for one chunk
        _, res3, ts3 = _decode(capi, ctx, [v for _, v in variants], 100, hb=hb)
        for r in res3:
            assert all(r[k] == 0 for k in r if k != "first_lock_byte"), r
        assert all(t == b"" for t in ts3)
    finally:
        hb.close()


def test_neighbours_do_not_matter(capi, ctx):
    res4, ts4, sym4 = _batch_of_four(capi, ctx, 0, 0, 0)
    iq = _capture(23, 12.0)[0]
    hb1, res1, ts1 = _decode(capi, ctx, [iq], N_SAMPLES)
    try:
        sym1 = hb1.symbols(0, res1[0]["symbols"]).tobytes()
    finally:
        hb1.close()
    hbc, resc, tsc = _decode(capi, ctx, [iq] * 4, N_SAMPLES)
    try:
        symc = [hbc.symbols(i, resc[i]["symbols"]).tobytes() for i in range(4)]
    finally:
        hbc.close()
    assert len(ts1[0]) >= 540 * 188
    assert ts1[0] == ts4[2] and all(t == ts1[0] for t in tsc)
    assert sym1 == sym4 and all(s == sym1 for s in symc)
    assert res1[0]["bytes_deconv"] == res4[2]["bytes_deconv"] and all(r["bytes_deconv"] == res1[0]["bytes_deconv"] for r in resc)
    assert res1[0] == res4[2] and all(r == res1[0] for r in resc)


@pytest.mark.parametrize("force", ["0", "1"])
def test_both_tile_kernels_give_the_same_symbols(capi, ctx, monkeypatch, force):
    """The tile kernel keeps the receiver's `rect` table in LDS when a run is large enough and reads it from memory otherwise
    (LSDR_HSB_LDS_RECT forces one of them, read when the object is made): same arithmetic, so the same symbols and TS."""
    res4, ts4, sym4 = _batch_of_four(capi, ctx, 0, 0, 0)
    monkeypatch.setenv("LSDR_HSB_LDS_RECT", force)
    hb, res, ts = _decode(capi, ctx, [_capture(23, 12.0)[0], _capture(21, 6.0)[0]], N_SAMPLES)
    try:
        sym = hb.symbols(0, res[0]["symbols"]).tobytes()
    finally:
        hb.close()
    assert sym == sym4 and ts[0] == ts4[2] and ts[1] == ts4[0] and res[0] == res4[2] and res[1] == res4[0]


def test_carrier_offset(capi, ctx, oracle):
    """(a) an offset of half the tile window (4.07e-4 cycles per sample at omega 1.2), decoded untuned: the tiles pull in inside their
    warm-up; (b) 1e-3 cycles per sample, decoded with the matching bias (the reference: --tune)."""
    iq, sent = _capture(23, 12.0)
    fa, fb = 2e-4, 1e-3
    # the sign of `freq` is lsdr_fastqpsk_create's: the exact receiver ends at +f for a capture multiplied by exp(+j2π·f·n)
    o = oracle.fast_qpsk(shifted(iq, fb)[: 2 * 400000], OMEGA)
    assert abs(o["freqw"] / 65536.0 - fb) < 1e-4, o["freqw"]
    refs = references([(REF_ARGS, 600, 23, 12.0, None, fa), (REF_ARGS + ("--tune", str(fb * FS)), 600, 23, 12.0, None, fb)])
    for name, f, freq, ref in (("offset 2e-4 untuned", fa, 0.0, refs[0]), ("offset 1e-3 tuned", fb, fb, refs[1])):
        hb, res, ts = _decode(capi, ctx, [shifted(iq, f)], N_SAMPLES, freq=freq)
        hb.close()
        check_against_reference(ts[0], ref, sent, 540, name, True)
        assert res[0]["locked"] == 1 and res[0]["seam_bad"] == 0, res[0]


def test_arguments(capi, ctx):
    E = capi.LSDR_E_ARG if hasattr(capi, "LSDR_E_ARG") else None

    def refused(fn):
        with pytest.raises(capi.LsdrError) as e:
            fn()
        return e

    refused(lambda: capi.HsBatch(ctx, 0, 1 << 16, OMEGA))
    refused(lambda: capi.HsBatch(ctx, 2, 1 << 16, OMEGA, tile_len=1000))
    refused(lambda: capi.HsBatch(ctx, 2, 1 << 16, OMEGA, tile_warmup=100))
    cfg = capi.HsBatchCfg()
    cfg.n_captures, cfg.max_samples, cfg.omega = 2, 1 << 16, OMEGA
    cfg.reserved[3] = 1
    h = capi.vp()
    rc = capi.lib.lsdr_hs_batch_create(ctx.h, cfg, h)
    assert rc != 0 and (E is None or rc == E) and not h.value
    hb = capi.HsBatch(ctx, 2, 1 << 16, OMEGA)
    buf = ctx.alloc(2 << 16)
    capi.check(capi.lib.lsdr_memset(ctx.h, buf.ptr, 128, 2 << 16))
    try:
        refused(lambda: hb.wait())                               # nothing in flight
        refused(lambda: hb.run_async([buf.ptr, buf.ptr], (1 << 16) + 1))
        refused(lambda: hb.ts_download_async([buf.ptr, buf.ptr], 0))      # before wait
        hb.run_async([buf.ptr, buf.ptr], 1 << 16)
        refused(lambda: hb.run_async([buf.ptr, buf.ptr], 1 << 16))        # in flight
        res = hb.wait()
        assert len(res) == 2 and all(r["ts_packets"] == 0 and r["locked"] == 0 for r in res)
        refused(lambda: hb.wait())
        lib = capi.lib
        for fn in (lib.lsdr_hs_batch_ts_dev, lib.lsdr_hs_batch_symbols_dev, lib.lsdr_hs_batch_bytes_dev, lib.lsdr_hs_batch_mpeg_dev):
            assert fn(hb.h, 0) is not None and fn(hb.h, 1) is not None
            assert fn(hb.h, 2) is None and fn(hb.h, -1) is None
    finally:
        hb.close()
        buf.free()
