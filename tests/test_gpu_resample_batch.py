"""lsdr_resample_batch on the GPU: leandvb's --derotate --resample for many captures in one launch, and ResampledDecoder's loop around it.

  a bit for bit against the numpy float32 restatement (resample_common.resample): batches of six captures with different lengths and
    tunes, at six geometries (N, D), at every length where the kernel changes its path (with the tile M the library chose): N − 1, N,
    N + D − 1 (nothing), N + D (one output), one tile, one tile and one output, three tiles and an odd remainder, 0 with no pointer;
    nothing is written behind out[produced − 1];
  b tune 0 equals the oracle's fir_filter as values;
  c the five sample formats of the same samples give the cu8 output bit for bit;
  d composition: alone, in the batch, in the reversed batch, in a second run, from a pointer that is only item-aligned;
  e ifreq != 0 against the reference chain rotator → fir_filter within resample_common.REF_CHAIN_BOUND (test_resample_abi.py measures it);
  f every refusal carries its code and its message and leaves a usable object;
  g the loop closed: oversampled captures shifted by offsets the decoder cannot follow, decoded by ResampledDecoder.decode with NO tune
    given, against the reference binary run with --resample --derotate f·Fs — and, derotated and decoded with tune 0, the 0.01 capture
    loses more than half its packets, as the reference loses all of them without --derotate.

The taps of a are random (an asymmetric tap set tells a reversed tap order from the right one, a designed low-pass does not).
Bounds: a, c, d are bit for bit; b as values; e resample_common.REF_CHAIN_BOUND (4e-2 of the output's RMS); g batch_common.check_against_reference
with the reference returning at least 400 (default engine, noise 7.5) and 450 packets (Viterbi engine, noise 30), every estimate's quality at
least TUNE_MIN_QUALITY, the fine estimate within an eighth of the decoder's window 1/(2048·omega/D) of the true residual, locked, no
unreconciled seam.
Measured on an MI355X: e 1.7e-5, 2.1e-4, 3.5e-3, 9.0e-3 at tunes 0.01, −0.03, 0.1, −0.12 (the restatement's own figures); g the whole TS is the
reference's byte for byte in all nine decodes (418 packets on the default engine at 12 and 10 samples per symbol, 468 on the Viterbi engine), raw
quality 124 … 2394, fine quality 811 … 2311, fine estimate within 7.8e-6 of the residual (window/8: 1.5e-5); with tune 0 the 0.01 capture returns 0 packets.
The reference binary (oracle/_ref/leandvb) is required by g: where it is missing that test FAILS.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import resample_common as rc
from batch_common import check_against_reference, run_reference
from conftest import bits_equal

pytestmark = pytest.mark.gpu

LSDR_E_ARG, LSDR_E_UNSUPPORTED = -2, -4
TUNES = [0.0, 1e-3, 0.01, -0.03, 0.1, -0.12]
GEOMETRIES = [(5, 1), (27, 2), (33, 3), (87, 8), (313, 30), (1024, 64)]
SENTINEL = np.complex64(complex(-7777.0, 7777.0))


def _taps(N):
    return (np.random.default_rng(N).standard_normal(N) / np.sqrt(N)).astype(np.float32)


def _source():
    return rc.capture_sps(16, 12, 7.5)[0]


def _run(capi, ctx, rs, arrays, lengths, tunes, misalign=0):
    """One run of `rs` over host arrays (None: no pointer): ([outputs], results).  Every output buffer has 8 items of room behind cap_out,
    filled with a sentinel that must survive; misalign: bytes by which every input is moved off its allocation's start."""
    cap_out = max([rs.produced(n) for n in lengths] + [1])
    bufs, outs = [], []
    try:
        for a in arrays:
            if a is None:
                bufs.append(None)
                continue
            raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            bufs.append(ctx.upload(np.concatenate([np.zeros(misalign, np.uint8), raw]) if misalign else raw))
        outs = [ctx.upload(np.full(cap_out + 8, SENTINEL, np.complex64)) for _ in arrays]
        res = rs.run([b.ptr + misalign if b else None for b in bufs], lengths, tunes, [o.ptr for o in outs], cap_out)
        got = []
        for o, r in zip(outs, res):
            whole = ctx.download(o, np.complex64, cap_out + 8)
            assert np.all(whole[r["produced"]:] == SENTINEL), "written behind out[produced - 1]"
            got.append(whole[: r["produced"]].copy())
        return got, res
    finally:
        for b in bufs + outs:
            if b:
                b.free()


# ---- a -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", GEOMETRIES)
def test_bit_for_bit_against_the_restatement(capi, ctx, N, D):
    h, src = _taps(N), _source()
    rs = capi.ResampleBatch(ctx, 6, 1 << 20, h, D)
    try:
        M = rs.tile
        assert M in (32, 64, 128, 256, 512, 1024)
        long = N + (3 * M + 77) * D + (D - 1)
        batches = [([N + D - 1, N + D, N + M * D, N + (M + 1) * D, long, 0], TUNES),
                   ([N - 1, N, long, N + M * D, N + (M + 1) * D, N + D], TUNES[2:] + TUNES[:2])]
        for lengths, tunes in batches:
            arrays = [src[2000 * i: 2000 * i + 2 * n] if n else None for i, n in enumerate(lengths)]
            got, res = _run(capi, ctx, rs, arrays, lengths, tunes)
            for i, (n, t) in enumerate(zip(lengths, tunes)):
                want, consumed, f = rc.resample(arrays[i], t, h, D) if n else (np.empty(0, np.complex64), 0, rc.ifreq_of(t))
                name = f"N {N} D {D} M {M}: capture {i}, {n} items, tune {t}"
                assert len(want) == (max(0, n - N) // D)
                assert res[i] == dict(consumed=consumed, produced=len(want), ifreq=f, applied=f / 65536.0), (name, res[i])
                assert bits_equal(got[i], want), (name, int(np.sum(got[i] != want)))
    finally:
        rs.close()


# ---- b, e --------------------------------------------------------------------------------------------------------------------------
def test_tune_0_is_fir_filter_and_the_reference_chain(capi, ctx, oracle):
    iq = _source()[: 2 * rc.CHAIN_SAMPLES]
    d, order, fcut = rc.design(12.0)
    h = oracle.lowpass(order, fcut)
    x = oracle.cconverter_u8(iq)
    tunes = [0.0] + list(rc.CHAIN_TUNES)
    rs = capi.ResampleBatch(ctx, len(tunes), rc.CHAIN_SAMPLES, h, d)
    try:
        got, res = _run(capi, ctx, rs, [iq] * len(tunes), [rc.CHAIN_SAMPLES] * len(tunes), tunes)
    finally:
        rs.close()
    want, consumed = oracle.fir_filter(h, d, x)
    assert res[0]["consumed"] == consumed and rc.same_values(got[0], want)
    devs = []
    for g, r, t in zip(got[1:], res[1:], rc.CHAIN_TUNES):
        assert r["ifreq"] == rc.ifreq_of(t) != 0
        want, consumed = oracle.fir_filter(h, d, oracle.rotator(x, -r["ifreq"] / 65536.0))
        assert r["consumed"] == consumed and len(g) == len(want)
        rms = float(np.sqrt(np.mean(np.abs(want.astype(np.complex128)) ** 2)))
        devs.append(float(np.max(np.abs(g.astype(np.complex128) - want.astype(np.complex128)))) / rms)
    print("device against rotator -> fir_filter, max |difference| / RMS: " + ", ".join(f"tune {t}: {v:.3e}" for t, v in zip(rc.CHAIN_TUNES, devs)))
    assert max(devs) <= rc.REF_CHAIN_BOUND, devs


# ---- c -----------------------------------------------------------------------------------------------------------------------------
def test_formats_give_the_same_output(capi, ctx):
    h, D = _taps(33), 3
    lengths = [33 + 3 * 1024 + 5, 4001]
    u8 = [_source()[: 2 * lengths[0]], _source()[6000: 6000 + 2 * lengths[1]]]
    tunes = [0.01, -0.12]

    def run(arrays, **kw):
        rs = capi.ResampleBatch(ctx, 2, 1 << 16, h, D, **kw)
        try:
            return _run(capi, ctx, rs, arrays, lengths, tunes)[0]
        finally:
            rs.close()

    base = run(u8)
    for g, a, t in zip(base, u8, tunes):
        assert bits_equal(g, rc.resample(a, t, h, D)[0])
    assert all(bits_equal(a, b) for a, b in zip(run(u8, in_scale=1.0), base))
    variants = [rc.formats_of(a) for a in u8]
    for k, (name, _, fmt, scale) in enumerate(variants[0]):
        got = run([v[k][1] for v in variants], in_format=getattr(capi, fmt), in_scale=scale)
        assert all(bits_equal(a, b) for a, b in zip(got, base)), name
    # an unscaled 16-bit run is 256 times larger, exactly
    s16 = run([v[2][1] for v in variants], in_format=capi.IN_CS16)
    assert all(bits_equal(a, (b.view(np.float32) * np.float32(256)).view(np.complex64)) for a, b in zip(s16, base))


# ---- d -----------------------------------------------------------------------------------------------------------------------------
def test_composition(capi, ctx):
    h, D = _taps(87), 8
    src = _source()
    six = capi.ResampleBatch(ctx, 6, 1 << 16, h, D)
    one = capi.ResampleBatch(ctx, 1, 1 << 16, h, D)
    try:
        M = six.tile
        lengths = [87 + (2 * M + 3) * D + 5, 87 + D, 0, 87 + M * D, 87 + (M + 1) * D + 1, 86]
        arrays = [src[3000 * i: 3000 * i + 2 * n] if n else None for i, n in enumerate(lengths)]
        got, res = _run(capi, ctx, six, arrays, lengths, TUNES)
        again, _ = _run(capi, ctx, six, arrays, lengths, TUNES)
        back, rback = _run(capi, ctx, six, arrays[::-1], lengths[::-1], TUNES[::-1])
        moved, _ = _run(capi, ctx, six, arrays, lengths, TUNES, misalign=2)           # cu8 items want 2 bytes: the item-wise loads
        assert rback[::-1] == res
        for i in range(6):
            alone, ralone = _run(capi, ctx, one, [arrays[i]], [lengths[i]], [TUNES[i]])
            assert ralone[0] == res[i]
            for name, other in (("a second run", again[i]), ("reversed batch", back[5 - i]), ("item-aligned pointer", moved[i]), ("alone", alone[0])):
                assert bits_equal(other, got[i]), (i, name)
        # cf32 from a pointer aligned to 8 bytes only
        f32 = [None if a is None else (a.astype(np.float32) - 128) for a in arrays]
        c32 = capi.ResampleBatch(ctx, 6, 1 << 16, h, D, in_format=capi.IN_CF32)
        try:
            wide, _ = _run(capi, ctx, c32, f32, lengths, TUNES)
            narrow, _ = _run(capi, ctx, c32, f32, lengths, TUNES, misalign=8)
        finally:
            c32.close()
        assert all(bits_equal(a, b) and bits_equal(a, c) for a, b, c in zip(got, wide, narrow))
    finally:
        six.close()
        one.close()


# ---- f -----------------------------------------------------------------------------------------------------------------------------
def test_arguments(capi, ctx):
    lib = capi.lib
    h, D, n = _taps(33), 3, 4001
    iq = _source()[: 2 * n]
    want = rc.resample(iq, 0.01, h, D)[0]
    buf, out = ctx.upload(iq), ctx.alloc((len(want) + 4) * 8)
    rs = capi.ResampleBatch(ctx, 2, n, h, D)

    def usable():
        res = rs.run([buf.ptr, None], [n, 0], [0.01, 0.0], [out.ptr, None], len(want))
        assert [r["produced"] for r in res] == [len(want), 0]
        assert bits_equal(ctx.download(out, np.complex64, len(want)), want)

    def message(rc_, code, what, word):
        msg = lib.lsdr_last_error().decode()
        assert rc_ == code and "resample_batch" in msg and word in msg, (what, rc_, msg)

    try:
        usable()
        for what, code, word, change in (("n_captures 0", LSDR_E_ARG, "n_captures", lambda c: setattr(c, "n_captures", 0)),
                                         ("n_captures -1", LSDR_E_ARG, "n_captures", lambda c: setattr(c, "n_captures", -1)),
                                         ("format 5", LSDR_E_ARG, "in_format", lambda c: setattr(c, "in_format", 5)),
                                         ("format -1", LSDR_E_ARG, "in_format", lambda c: setattr(c, "in_format", -1)),
                                         ("scale -1", LSDR_E_ARG, "in_scale", lambda c: setattr(c, "in_scale", -1.0)),
                                         ("scale nan", LSDR_E_ARG, "in_scale", lambda c: setattr(c, "in_scale", float("nan"))),
                                         ("scale inf", LSDR_E_ARG, "in_scale", lambda c: setattr(c, "in_scale", float("inf"))),
                                         ("reserved", LSDR_E_ARG, "reserved", lambda c: c.reserved.__setitem__(5, 1)),
                                         ("no taps", LSDR_E_ARG, "coeffs_host", lambda c: setattr(c, "coeffs_host", None)),
                                         ("decim 0", LSDR_E_UNSUPPORTED, "decim", lambda c: setattr(c, "decim", 0)),
                                         ("decim 65", LSDR_E_UNSUPPORTED, "decim", lambda c: setattr(c, "decim", 65)),
                                         ("ncoeffs 1", LSDR_E_UNSUPPORTED, "ncoeffs", lambda c: setattr(c, "ncoeffs", 1)),
                                         ("ncoeffs 1025", LSDR_E_UNSUPPORTED, "ncoeffs", lambda c: setattr(c, "ncoeffs", 1025))):
            cfg = capi.ResampleBatchCfg()
            cfg.n_captures, cfg.max_samples, cfg.in_format, cfg.in_scale = 2, n, capi.IN_CU8, 0.0
            cfg.ncoeffs, cfg.coeffs_host, cfg.decim = len(h), h.ctypes.data, D
            change(cfg)
            hd = C.c_void_p()
            message(lib.lsdr_resample_batch_create(ctx.h, C.byref(cfg), C.byref(hd)), code, what, word)
            assert not hd.value
            usable()
        good = dict(ptrs=[buf.ptr, None], lengths=[n, 0], tune=[0.01, 0.0], outs=[out.ptr, None])
        for what, word, cap, change in (("n_samples > max_samples", "max_samples", len(want), dict(lengths=[n + 1, 0])),
                                        ("tune nan", "tune", len(want), dict(tune=[float("nan"), 0.0])),
                                        ("tune inf", "tune", len(want), dict(tune=[0.0, float("inf")])),
                                        ("tune 0.5", "tune", len(want), dict(tune=[0.5, 0.0])),
                                        ("tune -0.5", "tune", len(want), dict(tune=[0.0, -0.5])),
                                        ("a misaligned input", "aligned", len(want), dict(ptrs=[buf.ptr + 1, None])),
                                        ("a misaligned output", "aligned", len(want), dict(outs=[out.ptr + 8, None])),
                                        ("samples without a pointer", "pointer", len(want), dict(lengths=[n, 40])),
                                        ("outputs without an output pointer", "pointer", len(want), dict(outs=[None, None])),
                                        ("cap_out too small", "cap_out", len(want) - 1, {})):
            p, e, o = rs._args(**{**good, **change})
            message(lib.lsdr_resample_batch_run_async(rs.h, p, e, o, cap), LSDR_E_ARG, what, word)
            usable()
        p, e, o = rs._args(**good)
        e[1].reserved[4] = 1
        message(lib.lsdr_resample_batch_run_async(rs.h, p, e, o, len(want)), LSDR_E_ARG, "each.reserved", "reserved")
        usable()
        message(lib.lsdr_resample_batch_wait(rs.h, None), LSDR_E_ARG, "wait with nothing in flight", "in flight")
        usable()
        p, e, o = rs._args(**good)
        capi.check(lib.lsdr_resample_batch_run_async(rs.h, p, e, o, len(want)))
        message(lib.lsdr_resample_batch_run_async(rs.h, p, e, o, len(want)), LSDR_E_ARG, "a second run_async before wait", "in flight")
        assert rs.wait()[0]["produced"] == len(want)
        usable()
        # cf32 items want 8 bytes
        r32 = capi.ResampleBatch(ctx, 1, n, h, D, in_format=capi.IN_CF32)
        try:
            p, e, o = r32._args([buf.ptr + 4], [100], [0.0], [out.ptr])
            message(lib.lsdr_resample_batch_run_async(r32.h, p, e, o, len(want)), LSDR_E_ARG, "cf32 at 4 bytes", "aligned")
        finally:
            r32.close()
        usable()
    finally:
        rs.close()
        buf.free()
        out.free()


# ---- g -----------------------------------------------------------------------------------------------------------------------------
OFFSETS = [0.0, 0.01, -0.03, 0.1]
# engine → (noise, leandvb's extra arguments, the least the reference must return, transmitted-packet set asked)
ENGINES = {"default": (7.5, (), 400, False), "viterbi": (30.0, ("--viterbi",), 450, True)}


def _ref_args(sps, f, extra, derotate=True):
    fs = sps * 2000e3
    return ("--u8", "-f", repr(fs), "--sr", "2000e3", "--cr", "1/2", "--resample") + (("--derotate", repr(f * fs)) if derotate else ()) + ("--anf", "0") + extra


def _references(jobs):
    """run_reference(args, items) of every job, eight processes at a time."""
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(lambda j: run_reference(*j), jobs))


def _closed_loop(capi, ctx, engine, sps, offsets, teeth):
    noise, extra, min_ref, ask_sent = ENGINES[engine]
    base, sent = rc.capture_sps(480, sps, noise)
    n = len(base) // 2
    caps = [rc.shifted_sps(480, sps, noise, f) for f in offsets]
    jobs = [(_ref_args(sps, f, extra), iq) for f, iq in zip(offsets, caps)]
    if teeth:
        jobs.append((_ref_args(sps, 0.0, extra, derotate=False), caps[offsets.index(0.01)]))
    refs = _references(jobs)
    bufs = [ctx.upload(iq) for iq in caps]
    dec = capi.ResampledDecoder(ctx, len(offsets), n, float(sps), viterbi=engine == "viterbi", anf=0)
    try:
        ptrs, lengths = [b.ptr for b in bufs], [n] * len(offsets)
        res, ts, info = dec.decode(ptrs, lengths)                                   # tune NOT given
        window8 = 1.0 / (2048.0 * dec.omega_out) / 8
        for i, f in enumerate(offsets):
            name = f"{engine}, {sps} samples per symbol, offset {f}"
            print(f"{name}: raw {info[i]['raw']['tune']:+.6e} (quality {info[i]['raw']['quality']:.0f}), ifreq {info[i]['ifreq']}, "
                  f"fine {info[i]['fine']['tune']:+.3e} (quality {info[i]['fine']['quality']:.0f}), produced {info[i]['produced']}")
            assert info[i]["raw"]["quality"] >= capi.TUNE_MIN_QUALITY and info[i]["fine"]["quality"] >= capi.TUNE_MIN_QUALITY, info[i]
            assert info[i]["ifreq"] == rc.ifreq_of(info[i]["raw"]["tune"]) and info[i]["tune"] == info[i]["fine"]["tune"]
            assert abs(info[i]["fine"]["tune"] - (f - info[i]["applied"]) * dec.decim) <= window8, info[i]
            assert info[i]["produced"] == (n - len(dec.coeffs)) // dec.decim
            check_against_reference(ts[i], refs[i], sent if ask_sent else None, min_ref, name, False)
            assert res[i]["locked"] == 1 and res[i]["seam_bad"] == 0, (name, res[i])
        if teeth:
            k = offsets.index(0.01)
            assert len(refs[-1]) // 188 == 0, "the reference decodes the 0.01 capture without --derotate"
            res0, ts0, info0 = dec.decode(ptrs, lengths, tune=0.0, fine=False)
            print(f"{engine}: offset 0.01 resampled and decoded with tune 0: {res0[k]['ts_packets']} packets (reference, derotated: {len(refs[k]) // 188})")
            assert info0[k]["ifreq"] == 0 and info0[k]["tune"] == 0.0 and info0[k]["fine"] is None
            assert len(ts0[k]) // 188 < len(refs[k]) // 188 // 2
    finally:
        dec.close()
        for b in bufs:
            b.free()


@pytest.mark.parametrize("engine", ["default", "viterbi"])
def test_the_loop_closed_at_12_samples_per_symbol(capi, ctx, engine):
    _closed_loop(capi, ctx, engine, 12, OFFSETS, teeth=True)


def test_the_loop_closed_at_10_samples_per_symbol(capi, ctx):
    _closed_loop(capi, ctx, "default", 10, [0.01], teeth=False)
