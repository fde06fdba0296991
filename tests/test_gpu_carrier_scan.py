"""lsdr_carrier_scan on the GPU: the carriers of wideband captures found in their spectrum, and one wideband capture decoded to one TS per
carrier with nothing given but its samples.

  a B = 4 (mix A, mix B, a capture of 5·4096 + 17 samples, one of 100 samples): spectrum(i) against the float64 P; the records equal to the
    float32 restatement (scan_common.find(exact=True)) applied to the device's own P, bit for bit; all zeros for the 100 samples;
  b the same bits alone and at every place of the batch, from a pointer that is only item-aligned, and in the four other sample formats;
  c spread: the stride as defined, and nothing read behind the capture's end — a length one sample short of the last spread block moves
    every block, and the samples behind it do not matter;
  d max_carriers = 2 on mix A: found 3, listed 2, the first two in frequency order; every refusal of create and run_async is LSDR_E_ARG with
    a message naming carrier_scan and leaves a usable object;
  e the accuracy bounds of test_carrier_scan_abi.py on the device's records;
  f the loop closed: one cu8 capture of 6 267 071 samples with two carriers (320 packets at 12 samples per symbol on −0.11, 384 at 10 on
    +0.14) through WidebandDecoder.decode, each TS against the reference binary run with the TRUE parameters; and the same capture
    through ResampledDecoder(omega=12) with no tune given does not return the first carrier's TS.

Bounds: P within 1e-4 of its peak of the float64 P (test_gpu_tune_est.py's bound for the same transform); centre within
scan_common.CENTER_BOUND, omega within OMEGA_BOUND, level within 0.5 dB (test_carrier_scan_abi.py's docstring derives them: twice what the
float64 restatement measures, at most 2 bins and 3 %; the worst there, and here, is mix B's carrier at 4 samples per symbol, 3.7e-4 off
centre).
The reference binary (oracle/_ref/leandvb) is required by f: where it is missing that test FAILS.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import scan_common as sc
from batch_common import check_against_reference, run_reference
from resample_common import formats_of

pytestmark = pytest.mark.gpu

LSDR_E_ARG = -2
N = sc.N


def _scan(capi, ctx, arrays, lengths=None, spectra=False, **kw):
    """One batch of host arrays (None: no pointer), whole or their first lengths[i] items: the records (and every capture's P)."""
    bufs = [ctx.upload(a) if a is not None else None for a in arrays]
    s = capi.CarrierScan(ctx, len(arrays), **kw)
    try:
        if lengths is None:
            lengths = [len(a) // 2 for a in arrays]
        got = s.scan([b.ptr if b else None for b in bufs], lengths)
        return (got, [s.spectrum(i) for i in range(len(arrays))]) if spectra else got
    finally:
        s.close()
        for b in bufs:
            if b:
                b.free()


def _batch():
    a, b = sc.case(0)[3], sc.case(2)[3]
    return [a, b, np.ascontiguousarray(sc.case(1)[3][: 2 * (5 * N + 17)]), np.ascontiguousarray(a[:200])]


# ---- a -----------------------------------------------------------------------------------------------------------------------------
def test_against_the_restatement(capi, ctx):
    arrays = _batch()
    got, spectra = _scan(capi, ctx, arrays, spectra=True)
    assert [g["blocks"] for g in got] == [64, 64, 5, 0] and [g["stride"] for g in got] == [1, 1, 1, 0]
    for i, (iq, g, P) in enumerate(zip(arrays, got, spectra)):
        want_P, M, stride = sc.spectrum(sc.to_complex(iq), 64, True)
        if M == 0:
            assert g == sc.SUMMARY_ZERO and not P.any(), g
            continue
        d = np.abs(P.astype(np.float64) - want_P).max() / want_P.max()
        want = sc.find(P, M, stride, exact=True)
        print(f"capture {i}: P within {d:.2e} of its peak; {g['found']} carriers: " +
              ", ".join(f"{c['center']:+.5f} omega {c['omega']:.3f} {c['cnr_db']:.1f} dB" for c in g["carriers"]))
        assert d <= 1e-4, (i, d)
        assert g == want, (i, g, want)
        if M == 64:                                             # and the float64 scan of the samples finds the same runs
            f64 = sc.find(want_P, M, stride)
            assert [(c["first_bin"], c["bins"]) for c in g["carriers"]] == [(c["first_bin"], c["bins"]) for c in f64["carriers"]], (i, g, f64)
    assert got[0]["found"] == 3 and got[1]["found"] == 3


# ---- b -----------------------------------------------------------------------------------------------------------------------------
def test_same_bits_anywhere_and_in_every_format(capi, ctx):
    arrays = _batch()
    base = _scan(capi, ctx, arrays)
    for r in range(1, 4):                                       # every capture at every place
        order = [(i + r) % 4 for i in range(4)]
        got = _scan(capi, ctx, [arrays[i] for i in order])
        assert [got[k] for k in range(4)] == [base[i] for i in order], r
    for i, a in enumerate(arrays):
        assert _scan(capi, ctx, [a])[0] == base[i], i
    # a pointer that is item-aligned only (the item-wise loads)
    buf = ctx.upload(np.concatenate([np.zeros(2, np.uint8), arrays[1]]))
    s = capi.CarrierScan(ctx, 1)
    try:
        assert s.scan([buf.at(2)], [len(arrays[1]) // 2])[0] == base[1]
    finally:
        s.close()
        buf.free()
    for i in (1, 2):
        for name, items, fmt, scale in formats_of(arrays[i]):
            got = _scan(capi, ctx, [items], [len(arrays[i]) // 2], in_format=getattr(capi, fmt), in_scale=scale)[0]
            assert got == base[i], (name, i, got, base[i])
    assert _scan(capi, ctx, [arrays[1]], in_scale=1.0)[0] == base[1]


# ---- c -----------------------------------------------------------------------------------------------------------------------------
def test_spread(capi, ctx):
    iq = sc.case(2, 40)[3]                                     # mix B, 40 blocks
    z = sc.to_complex(iq)
    other = iq.copy()
    other[2 * 29 * N:] = 128                                   # the same up to the end of block 28, silence behind it
    lengths = [40 * N, 40 * N - 1, 40 * N - 1, 7 * N, 40 * N]
    (got, spectra), plain = _scan(capi, ctx, [iq, iq, other, iq, iq], lengths, spectra=True, blocks=8), _scan(capi, ctx, [iq], blocks=8, spread=False)[0]
    # 40 blocks: every fifth; 39 whole blocks: every fourth, the last one read is block 28; fewer than asked: stride 1
    assert [(g["blocks"], g["stride"]) for g in got] == [(8, 5), (8, 4), (8, 4), (7, 1), (8, 5)]
    assert (plain["blocks"], plain["stride"]) == (8, 1)
    for g, P, n in zip(got, spectra, lengths):
        want_P, M, stride = sc.spectrum(z[:n], 8, True)
        assert (M, stride) == (g["blocks"], g["stride"])
        assert np.abs(P.astype(np.float64) - want_P).max() <= 1e-4 * want_P.max()
        assert g == sc.find(P, M, stride, exact=True)
    assert got[1] == got[2] and np.array_equal(spectra[1], spectra[2])           # nothing behind block 28 was read
    assert got[0] == got[4] and got[0] != got[1] and got[0]["floor"] != plain["floor"]
    assert [g["found"] for g in got if g["blocks"] == 8] == [3, 3, 3, 3], got


# ---- d -----------------------------------------------------------------------------------------------------------------------------
def test_max_carriers_and_arguments(capi, ctx):
    lib = capi.lib
    iq = sc.case(0)[3]
    full = _scan(capi, ctx, [iq])[0]
    two = _scan(capi, ctx, [iq], max_carriers=2)[0]
    assert two["found"] == 3 and two["listed"] == 2 and two["carriers"] == full["carriers"][:2], (two, full)
    assert _scan(capi, ctx, [iq], min_bins=300)[0]["found"] == 2 and _scan(capi, ctx, [iq], threshold_db=40.0)[0]["found"] == 0
    buf = ctx.upload(iq)
    s = capi.CarrierScan(ctx, 2)

    def usable():
        got = s.scan([buf.ptr, None], [64 * N, 0])
        assert got[0] == full and got[1] == sc.SUMMARY_ZERO, got

    def message(rc_, what):
        msg = lib.lsdr_last_error().decode()
        assert rc_ == LSDR_E_ARG and "carrier_scan" in msg, (what, rc_, msg)
        return msg

    try:
        usable()
        for what, word, change in (("n_captures 0", "n_captures", lambda c: setattr(c, "n_captures", 0)),
                                   ("n_captures -1", "n_captures", lambda c: setattr(c, "n_captures", -1)),
                                   ("format 5", "in_format", lambda c: setattr(c, "in_format", 5)),
                                   ("scale -1", "in_scale", lambda c: setattr(c, "in_scale", -1.0)),
                                   ("scale nan", "in_scale", lambda c: setattr(c, "in_scale", float("nan"))),
                                   ("blocks 257", "blocks", lambda c: setattr(c, "blocks", 257)),
                                   ("smooth 65", "smooth", lambda c: setattr(c, "smooth", 65)),
                                   ("threshold -3", "threshold_db", lambda c: setattr(c, "threshold_db", -3.0)),
                                   ("threshold nan", "threshold_db", lambda c: setattr(c, "threshold_db", float("nan"))),
                                   ("threshold inf", "threshold_db", lambda c: setattr(c, "threshold_db", float("inf"))),
                                   ("threshold 400", "threshold_db", lambda c: setattr(c, "threshold_db", 400.0)),
                                   ("max_carriers 65", "max_carriers", lambda c: setattr(c, "max_carriers", 65)),
                                   ("reserved", "reserved", lambda c: c.reserved.__setitem__(2, 1))):
            cfg = capi.CarrierScanCfg()
            cfg.n_captures, cfg.in_format = 2, capi.IN_CU8
            change(cfg)
            h = C.c_void_p()
            assert word in message(lib.lsdr_carrier_scan_create(ctx.h, C.byref(cfg), C.byref(h)), what) and not h.value
            usable()
        ptrs, lens = s._args([buf.ptr, None], [64 * N, 0])
        assert "in flight" in message(lib.lsdr_carrier_scan_wait(s.h, s._sum, s._car), "wait with nothing in flight")
        usable()
        s.run_async([buf.ptr, None], [64 * N, 0])
        assert "in flight" in message(lib.lsdr_carrier_scan_run_async(s.h, ptrs, lens), "a second run_async before wait")
        assert s.wait()[0] == full
        usable()
        bad, _ = s._args([buf.ptr + 1, None], [64 * N, 0])
        assert "aligned" in message(lib.lsdr_carrier_scan_run_async(s.h, bad, lens), "a misaligned pointer")
        usable()
        bad, lens1 = s._args([buf.ptr, None], [64 * N, N])
        assert "pointer" in message(lib.lsdr_carrier_scan_run_async(s.h, bad, lens1), "samples without a pointer")
        usable()
        assert lib.lsdr_carrier_scan_spectrum_dev(s.h, 2) is None and lib.lsdr_carrier_scan_spectrum_dev(s.h, -1) is None
        # the defaults are the header's: all zeros in the configuration is 64 blocks, smooth 8, 3 dB, 32 carriers, no spread
        cfg = capi.CarrierScanCfg()
        cfg.n_captures, cfg.in_format = 1, capi.IN_CU8
        h = C.c_void_p()
        capi.check(lib.lsdr_carrier_scan_create(ctx.h, C.byref(cfg), C.byref(h)))
        try:
            out, car = (capi.ScanSummary * 1)(), (capi.ScanCarrier * 32)()
            p1, n1 = (C.c_void_p * 1)(buf.ptr), (C.c_size_t * 1)(64 * N)
            capi.check(lib.lsdr_carrier_scan_run_async(h, p1, n1))
            capi.check(lib.lsdr_carrier_scan_wait(h, out, car))
            assert dict(out[0].as_dict(), carriers=[car[j].as_dict() for j in range(out[0].listed)]) == full
        finally:
            lib.lsdr_carrier_scan_destroy(h)
    finally:
        s.close()
        buf.free()


# ---- e -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(sc.CASES)), ids=[c[0] for c in sc.CASES])
def test_the_accuracy_bounds(capi, ctx, k):
    name, spec, noise, iq = sc.case(k)
    g = _scan(capi, ctx, [iq])[0]
    assert g["blocks"] == 64 and g["found"] == g["listed"] == len(spec) and not g["saturated"], (name, g)
    assert all(not c["weak"] for c in g["carriers"]), (name, g)
    dc, do, dl = sc.errors(g["carriers"], spec, noise)
    print(f"{name}: |center - f| {dc:.3e} (bound {sc.CENTER_BOUND:.2e}), |omega/true - 1| {do:.4f} (bound {sc.OMEGA_BOUND:.3f}), level within {dl:.2f} dB")
    assert do <= sc.OMEGA_BOUND, f"{name}: omega off by {do:.4f}"
    assert dl <= sc.LEVEL_DB_BOUND, f"{name}: level off by {dl:.2f} dB"
    assert dc <= sc.CENTER_BOUND, f"{name}: centre off by {dc:.3e} > {sc.CENTER_BOUND:.2e}"


def test_noise_alone_has_no_carriers(capi, ctx):
    got = _scan(capi, ctx, [sc.noise_alone(64), sc.noise_alone(16), np.full(2 * 8 * N, 128, np.uint8)])
    assert [g["found"] for g in got] == [0, 0, 0] and [g["saturated"] for g in got] == [0, 0, 1], got      # (silence: no floor to speak of)


# ---- f -----------------------------------------------------------------------------------------------------------------------------
def _ref_args(sps, f):
    fs = sps * 2e6
    return ("--u8", "-f", repr(fs), "--sr", "2000e3", "--cr", "1/2", "--resample", "--derotate", repr(f * fs), "--anf", "0")


def test_the_loop_closed(capi, ctx):
    iq = sc.wideband()
    assert len(iq) == 2 * sc.WIDE_N
    with ThreadPoolExecutor(max_workers=2) as ex:               # the reference with the TRUE parameters, both carriers at once
        refs = list(ex.map(lambda c: run_reference(_ref_args(c[0], c[1]), iq), sc.WIDE))
    buf = ctx.upload(iq)
    try:
        dec = capi.WidebandDecoder(ctx, sc.WIDE_N)
        scan, carriers = dec.decode(buf.ptr, sc.WIDE_N)
        print(f"scan: {scan['blocks']} blocks, stride {scan['stride']}, " + ", ".join(f"{c['center']:+.5f} omega {c['omega']:.3f}" for c in scan["carriers"]))
        assert scan["stride"] == 23 and len(carriers) == 2, (scan, carriers)
        for c, (sps, f, _), ref in zip(carriers, sc.WIDE, refs):
            name = f"{sps} samples per symbol at {f:+.2f}"
            assert abs(c["center"] - f) <= sc.CENTER_CAP and abs(c["omega_scan"] / sps - 1) <= sc.OMEGA_CAP and c["omega"] is not None, (name, c)
            print(f"{name}: scan {c['center']:+.5f} / {c['omega_scan']:.3f}, decimated by {c['decim']}, omega {c['omega']:.5f}, tune {c['tune']:+.6f}, "
                  f"{len(c['ts']) // 188} packets (reference {len(ref) // 188})")
            check_against_reference(c["ts"], ref, None, 200, name, False)
        assert carriers[0]["ts"] != carriers[1]["ts"]
        # the test has teeth: one omega for the capture and no tune, and the first carrier's TS is not what comes back
        one = capi.ResampledDecoder(ctx, 1, sc.WIDE_N, 12.0, anf=0)
        try:
            _, ts, _ = one.decode([buf.ptr], [sc.WIDE_N])
        finally:
            one.close()
        want = {refs[0][i:i + 188] for i in range(0, len(refs[0]), 188)}
        hit = sum(ts[0][i:i + 188] in want for i in range(0, len(ts[0]), 188))
        print(f"ResampledDecoder(omega=12), no tune: {len(ts[0]) // 188} packets, {hit} of them the first carrier's")
        assert hit < len(want) // 2
    finally:
        buf.free()
