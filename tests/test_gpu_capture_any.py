"""lsdr_capture_any_create: the capture batch on cs8, cu16, cs16 and cf32 captures (leandvb --s8 / --u16 / --s16 / --f32 --float-scale),
converted and scaled in the kernels' loads.

  1. the converters bit for bit: the notched stream in front of the first detect point is float32(item − Z)·float32(scale);
  2. every format is the cu8 run: the same samples in another format give the cu8 object's results, decisions, stage bytes and TS;
  3. true 16-bit data against the oracle's exact chain (scaler → auto_notch → cstln_receiver), both engines;
  4. true 16-bit data against the reference BINARY (`leandvb --f32 --float-scale 2^-8` on float32(s16));
  5. the argument checks.

The reference binary (oracle/_ref/leandvb) is required for 4: where it is missing that test FAILS.
"""
import ctypes as C
import functools

import numpy as np
import pytest
from batch_common import check_against_reference, run_reference

pytestmark = pytest.mark.gpu

LSDR_E_ARG, LSDR_E_UNSUPPORTED = -2, -4
DEC = 64 * 4096                                   # auto_notch::decimation lowered: 3 detect points in 1 Mi samples
S8 = 0.00390625                                   # 2^-8


# ---- the same samples in every format ----------------------------------------------------------------------------------------------
def _formats(capi):
    """name → (in_format, in_scale, items of the cu8 capture u as that format)."""
    def s(u):
        return u.astype(np.int16) - 128
    return {
        "cs8": (capi.IN_CS8, 0.0, lambda u: s(u).astype(np.int8)),
        "cu16": (capi.IN_CU16, 0.0, lambda u: (s(u).astype(np.int32) + 32768).astype(np.uint16)),
        "cs16": (capi.IN_CS16, 0.0, lambda u: s(u)),
        "cs16 * 256, scale 2^-8": (capi.IN_CS16, S8, lambda u: (s(u).astype(np.int32) * 256).astype(np.int16)),
        "cf32": (capi.IN_CF32, 1.0, lambda u: s(u).astype(np.float32)),
        "cf32 / 64, scale 64": (capi.IN_CF32, 64.0, lambda u: s(u).astype(np.float32) / np.float32(64)),
    }


@functools.lru_cache(maxsize=None)
def _cu8_captures():
    from leansdr_amd import synth_dvbs
    n = 1000000
    a = synth_dvbs.capture_u8(600, seed=11)[0][: 2 * n]
    b = synth_dvbs.capture_u8(600, seed=12)[0][: 2 * n]
    ph = 2 * np.pi * 0.1234 * np.arange(n)
    x = b.reshape(-1, 2).astype(np.float64) - 128 + 14.0 * np.stack([np.cos(ph), np.sin(ph)], axis=1)
    b = np.clip(np.rint(x + 128), 0, 255).astype(np.uint8).reshape(-1)
    c = np.random.default_rng(3).integers(96, 160, 2 * n, dtype=np.uint8)
    return [np.ascontiguousarray(v) for v in (a, b, c)]


def _run(capi, ctx, cb, arrays, n):
    """One batch of the first n samples of `arrays` (two values per sample) on cb: everything the comparison looks at."""
    bufs = [ctx.upload(a[: 2 * n]) for a in arrays]
    try:
        res, ts = cb.decode([b.ptr for b in bufs], n)
        out = dict(res=res, ts=ts, bins=[cb.bins(i) for i in range(len(arrays))], sym=[], deconv=[], mpeg=[])
        for i, r in enumerate(res):
            if cb.viterbi:
                out["sym"].append(cb.soft(i, r["symbols"]).tobytes())
            else:
                out["sym"].append(cb.words(i, r["symbols"]).tobytes())
            out["deconv"].append(cb.stage_bytes(i, "deconv", r["bytes_deconv"]).tobytes())
            out["mpeg"].append(cb.stage_bytes(i, "mpeg", r["bytes_mpeg"]).tobytes())
    finally:
        for b in bufs:
            b.free()
    return out


def _same(got, want, name):
    for i, (g, w) in enumerate(zip(got["res"], want["res"])):
        for k in w:
            assert g[k] == w[k], f"{name}: capture {i}: result.{k} is {g[k]}, the cu8 object's {w[k]}"
    assert got["bins"] == want["bins"], name
    for k in ("sym", "deconv", "mpeg", "ts"):
        for i in range(len(want[k])):
            assert got[k][i] == want[k][i], f"{name}: capture {i}: {k} differs from the cu8 object's"


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
def _range_items(fmt, rng, n=8192):
    if fmt == "cs8":
        v = rng.integers(-128, 128, 2 * n).astype(np.int8); v[:4] = [-128, 127, 127, -128]; return v, 0
    if fmt == "cu16":
        v = rng.integers(0, 65536, 2 * n).astype(np.uint16); v[:4] = [0, 65535, 65535, 0]; return v, 32768
    if fmt == "cs16":
        v = rng.integers(-32768, 32768, 2 * n).astype(np.int16); v[:4] = [-32768, 32767, 32767, -32768]; return v, 0
    mag = np.exp(rng.uniform(np.log(1e-3), np.log(3e4), 2 * n))
    v = (mag * rng.choice([-1.0, 1.0], 2 * n)).astype(np.float32)
    v[:8] = [1e-3, -1e-3, 3e4, -3e4, -1e-3, 3e4, -3e4, 1e-3]
    return v, 0


@pytest.mark.parametrize("fmt", ["cs8", "cu16", "cs16", "cf32"])
def test_converters_bit_for_bit(capi, ctx, fmt):
    """8192 items over the format's whole range, anf = 1 at the default detect period: no detect point is reached, the notch passes its
    input through, and the notched stream is the converted, scaled stream — float32(item − Z)·float32(scale), one rounding."""
    n = 8192
    items, Z = _range_items(fmt, np.random.default_rng(7), n)
    if fmt == "cf32":
        conv = items.copy()
        assert np.abs(items).min() == np.float32(1e-3) and np.abs(items).max() == np.float32(3e4)
    else:
        conv = (items.astype(np.int32) - Z).astype(np.float32)
        assert conv.min() == {"cs8": -128, "cu16": -32768, "cs16": -32768}[fmt] and conv.max() == {"cs8": 127, "cu16": 32767, "cs16": 32767}[fmt]
    in_format = {"cs8": capi.IN_CS8, "cu16": capi.IN_CU16, "cs16": capi.IN_CS16, "cf32": capi.IN_CF32}[fmt]
    buf = ctx.upload(items)
    try:
        for scale in (0.0, 0.00390625, 3.0):
            cb = capi.CaptureBatch(ctx, 1, n, 1.2, anf=1, in_format=in_format, in_scale=scale)
            try:
                cb.run_async([buf.ptr], n)
                res = cb.wait()
                assert cb.bins(0) == [] and res[0]["samples"] == (n - 1) // 128 * 128
                got = cb.notched(0, n).view(np.float32)
            finally:
                cb.close()
            want = conv * np.float32(scale if scale else 1.0)
            assert want.dtype == np.float32
            assert got.tobytes() == want.tobytes(), (fmt, scale, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    finally:
        buf.free()


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("viterbi,anf,tile", [(False, 1, 4096), (False, 1, 2048), (False, 0, 4096), (True, 1, 4096), (True, 1, 2048), (True, 0, 4096)])
def test_every_format_is_the_cu8_run(capi, ctx, viterbi, anf, tile):
    """B = 3 × 1 000 000 samples (245 / 489 tiles: the last wavefront of 64 tiles is partial; n is no multiple of 128): the cu8 object
    made without the new arguments is the yardstick, every other format of the same samples must reproduce all of it.  Then a second,
    short batch on the same objects."""
    import bench_c1
    caps = _cu8_captures()
    kw = dict(anf=anf, tile_len=tile, tile_warmup=512, notch_decimation=DEC if anf else 0, viterbi=True if viterbi else None)
    n, n2 = 1000000, 70000
    parent = capi.CaptureBatch(ctx, 3, n, bench_c1.OMEGA, **kw)
    try:
        want = _run(capi, ctx, parent, caps, n)
        want2 = _run(capi, ctx, parent, caps, n2)
    finally:
        parent.close()
    res = want["res"]
    assert res[0]["tiles"] == (245 if tile == 4096 else 489)
    assert all(res[i]["locked"] == 1 and res[i]["ts_packets"] > 400 for i in (0, 1)), res
    assert res[2]["ts_packets"] == 0, res[2]
    if anf:
        assert len(want["bins"][1]) == 3
    for name, (in_format, in_scale, conv) in _formats(capi).items():
        arrays = [conv(c) for c in caps]
        cb = capi.CaptureBatch(ctx, 3, n, bench_c1.OMEGA, in_format=in_format, in_scale=in_scale, **kw)
        try:
            _same(_run(capi, ctx, cb, arrays, n), want, f"{name} ({'viterbi' if viterbi else 'default'}, anf {anf}, tile {tile})")
            _same(_run(capi, ctx, cb, arrays, n2), want2, f"{name}, second batch of {n2}")
        finally:
            cb.close()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _true_s16_with_cw():
    """capture_s16(600, seed 11) plus the front-end test's interferer at the 16-bit level: a CW of amplitude 14·256 that moves behind the
    second detect point.  Returns (cs16 items, the same signal rounded to cu8)."""
    from leansdr_amd import synth_dvbs
    n = 1 << 20
    s = synth_dvbs.capture_s16(600, seed=11)[0][: 2 * n]
    t = np.arange(n)
    f = np.where(t < 2 * DEC + 4096 * 5, 0.1234, -0.31)
    ph = 2 * np.pi * np.cumsum(f)
    x = s.reshape(-1, 2).astype(np.float64) + 14.0 * 256.0 * np.stack([np.cos(ph), np.sin(ph)], axis=1)
    s16 = np.clip(np.rint(x), -32768, 32767).astype(np.int16).reshape(-1)
    u8 = np.clip(np.rint(s16.astype(np.float64) / 256.0 + 128.0), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(s16), np.ascontiguousarray(u8)


_ORACLE = {}


def _oracle_chain(oracle, key, xf, viterbi):
    """auto_notch → cstln_receiver(linear, QPSK, omega 1.2) on the float stream xf, once per (input, engine)."""
    import bench_c1
    import pyoracle as po
    k = (key, viterbi)
    if k not in _ORACLE:
        bins_by_block = oracle.auto_notch_bins(xf, decimation=DEC)
        bins = [bins_by_block[b] for b in range(len(bins_by_block)) if (b + 1) * 4096 % DEC == 0 and (b + 1) * 4096 >= DEC]
        notched, _ = oracle.auto_notch(xf, 1, DEC)
        p = po.rx_params(sampler=1, cstln=1, omega=bench_c1.OMEGA, meas_decimation=1 << 20, **(dict(pll_adjustment=1.0 / 6.0) if viterbi else {}))
        _ORACLE[k] = (bins, oracle.rx(p, notched))
    return _ORACLE[k]


def _check_front_end(capi, cb, res, bins, o, viterbi, name):
    """Default engine: test_front_end_against_the_oracle_chain's rule; Viterbi engine: test_soft_symbols_against_the_oracle_chain's."""
    import bench_c1
    import pyoracle as po
    from leansdr_amd import tolerance
    assert cb.bins(0) == bins and len(set(bins)) >= 2, (name, cb.bins(0), bins)
    assert res["samples"] == o["consumed"], name
    first = int(512 / bench_c1.OMEGA) - 8
    stats = dict(tiles=res["tiles"], bad_seams=res["seam_bad"], dup=res["seam_dup"], miss=res["seam_miss"])
    if viterbi:
        sym = cb.soft(0, res["symbols"])
        assert not sym["pad"].any()
        rep = tolerance.check_tiled(sym, o["sym"], stats, first_exact=first)
        print(f"{name}: {rep}")
        assert rep["pass"], (name, rep)
        return sym.tobytes()
    got = cb.words(0, res["symbols"])
    sym = np.zeros(len(got), po.SOFTSYM); sym["symbol"] = got
    ref_sym = o["sym"].copy(); ref_sym["symbol"] &= 3
    sym["cost"] = ref_sym["cost"][: len(sym)] if len(sym) <= len(ref_sym) else 0      # (packed decisions carry no cost)
    rep = tolerance.check_tiled(sym, ref_sym, stats, first_exact=0)
    print(f"{name}: {rep}")
    assert rep["pass"], (name, rep)
    assert got[:first].tobytes() == (o["sym"]["symbol"][:first] & 3).tobytes(), f"{name}: tile 0 is not the oracle's"
    return got.tobytes()


@pytest.mark.parametrize("viterbi,tile", [(False, 4096), (False, 2048), (True, 4096), (True, 2048)])
def test_true_16_bit_data_against_the_oracle_chain(capi, ctx, oracle, viterbi, tile):
    """99.6 % of these cs16 values are no multiples of 256.  float32(s16) → scaler(2^-8) → auto_notch → cstln_receiver by the oracle against
    the batch on the cs16 items with in_scale 2^-8, under the project's tolerance (measured on cu8: the arithmetic behind the conversion
    is the same).  Condition on the input, asserted first: the cu8 object passes the same check on the same signal rounded to cu8."""
    import bench_c1
    s16, u8 = _true_s16_with_cw()
    n = 1 << 20
    assert np.mean(s16 % 256 != 0) > 0.99
    kw = dict(anf=1, tile_len=tile, tile_warmup=512, notch_decimation=DEC, viterbi=True if viterbi else None)

    def decode(items, **fmt):
        cb = capi.CaptureBatch(ctx, 1, n, bench_c1.OMEGA, **kw, **fmt)
        buf = ctx.upload(items)
        try:
            res, ts = cb.decode([buf.ptr], n)
        except Exception:
            cb.close()
            raise
        finally:
            buf.free()
        return cb, res[0], ts[0]

    # the condition: cu8
    bins8, o8 = _oracle_chain(oracle, "u8", oracle.cconverter_u8(u8), viterbi)
    cb, res, _ = decode(u8)
    try:
        _check_front_end(capi, cb, res, bins8, o8, viterbi, f"condition (cu8 rounding), tile {tile}")
    finally:
        cb.close()
    # cs16
    f32 = s16.astype(np.float32)
    xf = oracle.scaler(S8, f32.view(np.complex64))
    assert xf.tobytes() == (f32 * np.float32(S8)).tobytes()
    bins, o = _oracle_chain(oracle, "s16", xf, viterbi)
    cb, res, ts = decode(s16, in_format=capi.IN_CS16, in_scale=S8)
    try:
        sym = _check_front_end(capi, cb, res, bins, o, viterbi, f"cs16, tile {tile}")
    finally:
        cb.close()
    assert res["locked"] == 1 and res["ts_packets"] > 400, res
    # the same values as cu16 and as cf32: the cs16 run bit for bit
    for name, items, in_format in (("cu16", (s16.astype(np.int32) + 32768).astype(np.uint16), capi.IN_CU16), ("cf32", f32, capi.IN_CF32)):
        cb, res2, ts2 = decode(items, in_format=in_format, in_scale=S8)
        try:
            sym2 = (cb.soft(0, res2["symbols"]) if viterbi else cb.words(0, res2["symbols"])).tobytes()
        finally:
            cb.close()
        assert res2 == res and sym2 == sym and ts2 == ts, f"{name} differs from the cs16 run"


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
REF_CASES = [(600, 11, 7.5, False, 1, 500), (600, 12, 7.5, False, 0, 500), (1500, 23, 18.0, True, 0, 1400), (1500, 22, 15.0, True, 1, 1400)]


@functools.lru_cache(maxsize=None)
def _s16_capture(n_packets, seed, noise_std):
    from leansdr_amd import synth_dvbs
    iq, ts = synth_dvbs.capture_s16(n_packets=n_packets, seed=seed, noise_std=noise_std)
    return np.ascontiguousarray(iq), {bytes(p) for p in np.asarray(ts, np.uint8).reshape(-1, 188)}


@pytest.mark.parametrize("n_packets,seed,noise_std,viterbi,anf,min_ref", REF_CASES)
def test_true_16_bit_data_against_the_reference_binary(capi, ctx, n_packets, seed, noise_std, viterbi, anf, min_ref):
    """`leandvb --f32 --float-scale 2^-8` on float32(s16) against the batch on the cs16 items with in_scale 2^-8, tile 4096, by
    bench_c1.verify's rule; the Viterbi cases also: every packet of the batch was transmitted (the default graph's first packets include
    some that never were — the reference's own acquisition)."""
    import bench_c1
    s16, sent = _s16_capture(n_packets, seed, noise_std)
    n = len(s16) // 2
    args = ["--f32", "--float-scale", "0.00390625", "-f", "2400e3", "--sr", "2000e3", "--cr", "1/2"] + ([] if anf else ["--anf", "0"]) + (["--viterbi"] if viterbi else [])
    ref = run_reference(args, s16.astype(np.float32))
    name = f"{n_packets} packets seed {seed} noise {noise_std} {'--viterbi ' if viterbi else ''}anf {anf}"
    cb = capi.CaptureBatch(ctx, 1, n, bench_c1.OMEGA, anf=anf, tile_len=4096, tile_warmup=512, viterbi=True if viterbi else None,
                           in_format=capi.IN_CS16, in_scale=S8)
    buf = ctx.upload(s16)
    try:
        res, ts = cb.decode([buf.ptr], n)
    finally:
        cb.close()
        buf.free()
    check_against_reference(ts[0], ref, sent if viterbi else None, min_ref, name, False)
    assert res[0]["locked"] == 1 and res[0]["seam_bad"] == 0, res[0]


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------
def test_arguments(capi, ctx):
    import bench_c1
    lib = capi.lib

    def create(in_format, in_scale, max_samples=1 << 16, reserved=0, viterbi=False):
        cfg = capi.CaptureBatchCfg()
        cfg.n_captures, cfg.max_samples, cfg.omega, cfg.fec, cfg.anf = 1, max_samples, bench_c1.OMEGA, capi.FEC12, 0
        icfg = capi.CaptureInputCfg()
        icfg.in_format, icfg.in_scale = in_format, in_scale
        icfg.reserved[3] = reserved
        vcfg = capi.CaptureViterbiCfg()
        h = C.c_void_p()
        rc = lib.lsdr_capture_any_create(ctx.h, C.byref(cfg), C.byref(vcfg) if viterbi else None, C.byref(icfg), C.byref(h))
        assert (rc == 0) == bool(h.value), "a failed create returns no object"
        return rc, h

    for bad in (5, -1, 33):
        assert create(bad, 0.0)[0] == LSDR_E_ARG
    for bad in (-1.0, float("inf"), float("nan")):
        assert create(capi.IN_CS16, bad)[0] == LSDR_E_ARG
    assert create(capi.IN_CS16, 0.0, reserved=1)[0] == LSDR_E_ARG
    assert create(capi.IN_CU8, 2.0)[0] == LSDR_E_UNSUPPORTED
    assert create(capi.IN_CU16, 0.0, max_samples=1 << 30)[0] == LSDR_E_UNSUPPORTED
    assert create(capi.IN_CF32, 0.0, max_samples=1 << 29, viterbi=True)[0] == LSDR_E_UNSUPPORTED
    # cu8 with scale 0 or 1, and a null icfg, are the cu8 object; after all those failures a valid create works and decodes
    for scale in (0.0, 1.0):
        rc, h = create(capi.IN_CU8, scale)
        assert rc == 0
        lib.lsdr_capture_batch_destroy(h)
    n = 1 << 16
    s16 = (np.random.default_rng(1).integers(-20000, 20000, 2 * n + 8)).astype(np.int16)
    buf = ctx.upload(s16)
    rc, h = create(capi.IN_CS16, S8)
    assert rc == 0
    try:
        one = (C.c_void_p * 1)
        # the typed cu8 call on a cs16 object; a pointer that is not aligned to the 4-byte item
        assert lib.lsdr_capture_batch_run_async(h, one(buf.ptr), n) == LSDR_E_ARG
        assert lib.lsdr_capture_any_run_async(h, one(buf.ptr + 2), n) == LSDR_E_ARG
        assert lib.lsdr_capture_any_run_async(h, one(buf.ptr), n + 1) == LSDR_E_ARG          # more than max_samples
        assert lib.lsdr_capture_any_run_async(h, one(buf.ptr + 4), n) == 0  # item-aligned is enough without the notch
        res = (capi.CaptureResult * 1)()
        assert lib.lsdr_capture_batch_wait(h, res) == 0
        assert res[0].samples == (n - 1) // 128 * 128 and res[0].ts_packets == 0
    finally:
        lib.lsdr_capture_batch_destroy(h)
        buf.free()
