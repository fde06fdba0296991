"""lsdr_spectrum_batch on the GPU: leandvb's --cnr and --fd-spectrum for many captures in shared launches, bit for bit the reference's.

  1 CNR against the oracle's cnr_fft: three captures of lengths 0, 5·4096 + 17 and 40·4096 with centres 0, 0.005 and −0.03 in one batch,
    nfft 4096 with a value every 8192 samples, and dense at nfft 64 (bands of three slots that wrap around bin 0); the golden CNR as well;
  2 rows against the oracle's spectrum (nfft 1024) at (decimation, kavg) = (4096, 0.5), (3000, 0.1) and dense (1024, 0.5), on the golden
    capture as cf32 with its scale: tests/golden/spectrum.npz comes out;
  3 the existing single-stream objects (capi.CnrFft, capi.Spectrum) give the same bits;
  4 composition invariance: a capture alone equals its slot in a batch of three, in any order;
  5 slab independence: slab_rows 1, 3 and the default, and 1 to 4 stages per pass, give the same bits (avgpower is carried across slabs);
  6 the five sample formats of the same samples give the same bits;
  7 a second run on the same object starts from fresh state;
  8 every refusal is LSDR_E_ARG with a message and leaves a usable object;
  9 ResampledDecoder.decode(cnr=True): the TS is that of cnr=False, the CNR is the oracle's on the resampler's own output.
Everything is compared by bits_equal: the device's transform is cfft_engine's butterflies evaluated once each, the sums are serial, libm runs
on the host.
"""
import numpy as np
import pytest
import resample_common as rc
import spectrum_common as sc
from conftest import bits_equal, gold, iq16_to_cf32

pytestmark = pytest.mark.gpu

N4 = 4096
LENGTHS = [0, 5 * N4 + 17, 40 * N4]
CENTERS = [0.0, 0.005, -0.03]


@pytest.fixture(scope="module")
def three():
    """Three cu8 captures at 4 samples per symbol (noise 7.5, 18 and 7.5 from another place of the capture), LENGTHS items long."""
    a, b = rc.capture_sps(32, 4, 7.5)[0], rc.capture_sps(32, 4, 18.0)[0]
    assert len(a) // 2 >= 41 * N4
    return [None, np.ascontiguousarray(b[: 2 * LENGTHS[1]]), np.ascontiguousarray(a[2 * 777: 2 * (777 + LENGTHS[2])])]


@pytest.fixture(scope="module")
def golden_cf32():
    g = gold("auto_notch.npz")
    return iq16_to_cf32(g["iq"]), float(g["scale"])


def _run(capi, ctx, arrays, centers=None, lengths=None, **kw):
    """One batch over host arrays (None: no pointer, length 0): SpectrumBatch.run's list."""
    bufs = [ctx.upload(a) if a is not None else None for a in arrays]
    if lengths is None:                                      # complex64 arrays hold one item per element, the others interleaved components
        lengths = [0 if a is None else (len(a) if a.dtype == np.complex64 else len(a) // 2) for a in arrays]
    sb = capi.SpectrumBatch(ctx, len(arrays), max(lengths + [1]), **kw)
    try:
        return sb.run([b.ptr if b else None for b in bufs], lengths, centers)
    finally:
        sb.close()
        for b in bufs:
            if b:
                b.free()


def _same(a, b):
    """Two captures' results bit for bit."""
    return (a["consumed"], a["rows"], a["icf"]) == (b["consumed"], b["rows"], b["icf"]) and bits_equal(a["cnr"], b["cnr"]) and \
        ((a["rows_db"] is None and b["rows_db"] is None) or bits_equal(a["rows_db"], b["rows_db"]))


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,dec", [(4096, 8192), (64, 64)])
def test_cnr_is_the_oracles(capi, ctx, oracle, three, nfft, dec):
    got = _run(capi, ctx, three, CENTERS, nfft=nfft, decimation=dec, bandwidth=0.2, kavg=0.1)
    for i, (a, n, c) in enumerate(zip(three, LENGTHS, CENTERS)):
        x = oracle.cconverter_u8(a) if a is not None else np.empty(0, np.complex64)
        want = oracle.cnr_fft(x, 0.2, nfft, dec, c, 1.0)
        rows, consumed = sc.rows_of(n, nfft, dec)
        assert got[i]["consumed"] == consumed and got[i]["rows"] == rows == len(want), (i, got[i]["consumed"], got[i]["rows"], len(want))
        assert got[i]["icf"] == int(np.floor(float(np.float32(c) * np.float32(nfft)) + 0.5))
        assert bits_equal(got[i]["cnr"], want), (i, got[i]["cnr"][:4], want[:4])
        assert got[i]["rows_db"] is None
    assert got[2]["rows"] >= 7 and np.all(np.isfinite(got[2]["cnr"]))
    if nfft == 64:                                           # centre −0.03: icf −2, the carrier's band is bins −5 … 1
        assert got[2]["icf"] == -2 and int((0.2 / 4) * 64) == 3


def test_cnr_golden(capi, ctx, golden_cf32):
    x, scale = golden_cf32
    got = _run(capi, ctx, [x], [float(np.float32(0.01) * np.float32(0.5))], nfft=4096, decimation=8192, bandwidth=0.2, in_format=capi.IN_CF32,
               in_scale=scale)[0]
    assert got["consumed"] == len(x) and bits_equal(got["cnr"], gold("auto_notch.npz")["cnr"])


# ---- 2, 3 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec,kavg,key", [(4096, 0.5, "d4096_k05"), (3000, 0.1, "d3000_k01"), (1024, 0.5, None)])
def test_rows_are_the_oracles_and_the_single_stream_objects(capi, ctx, oracle, golden_cf32, dec, kavg, key):
    raw, scale = golden_cf32
    arrays = [raw, np.ascontiguousarray(raw[1000: 1000 + 7 * 1024 + 5]), np.ascontiguousarray(raw[:1023])]
    got = _run(capi, ctx, arrays, nfft=1024, decimation=dec, kavg=kavg, rows=True, in_format=capi.IN_CF32, in_scale=scale)
    for i, a in enumerate(arrays):
        x = oracle.scaler(scale, a)
        want = oracle.spectrum(x, dec, kavg)
        rows, consumed = sc.rows_of(len(a), 1024, dec)
        assert got[i]["rows"] == rows == len(want) and got[i]["consumed"] == consumed
        assert got[i]["rows_db"].shape == (rows, 1024) and bits_equal(got[i]["rows_db"], want), (i, dec, kavg)
        sp = capi.Spectrum(ctx, dec, kavg)
        try:
            out, cons = sp.run(x)
        finally:
            sp.close()
        assert cons == consumed and bits_equal(got[i]["rows_db"], out)
        assert len(got[i]["cnr"]) == 0
    if key:
        assert bits_equal(got[0]["rows_db"], gold("spectrum.npz")[key])
    assert got[2]["rows"] == 0


def test_cnr_is_the_single_stream_objects(capi, ctx, oracle, three):
    got = _run(capi, ctx, three, CENTERS, nfft=4096, decimation=8192, bandwidth=0.2)
    for i in (1, 2):
        c = capi.CnrFft(ctx, 0.2, 4096, 8192)
        try:
            out, cons = c.run(oracle.cconverter_u8(three[i]), CENTERS[i], 1.0)
        finally:
            c.close()
        assert cons == got[i]["consumed"] and bits_equal(got[i]["cnr"], out)


def test_linear_rows_on_the_device(capi, ctx, golden_cf32):
    raw, scale = golden_cf32
    buf = ctx.upload(raw)
    with capi.SpectrumBatch(ctx, 1, len(raw), nfft=1024, decimation=4096, kavg=0.5, rows=True, in_format=capi.IN_CF32, in_scale=scale) as sb:
        r = sb.run([buf.ptr], [len(raw)])[0]
        assert sb.rows_linear_dev(0)
        host = sb.rows_linear(0)
        assert host.shape == (8, 1024) and np.all(host > 0)
        db = (10 * np.log10(host.astype(np.float64))).astype(np.float32)         # FFT order, linear: the host's log10f and the swap remain
        assert np.allclose(np.concatenate([db[:, 512:], db[:, :512]], axis=1), r["rows_db"], atol=1e-4)
    assert sb.h is None
    buf.free()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
def test_composition_invariance(capi, ctx, three):
    kw = dict(nfft=1024, decimation=3000, bandwidth=0.2, kavg=0.3, rows=True)
    whole = _run(capi, ctx, three, CENTERS, **kw)
    for order in ([2, 0, 1], [1, 2, 0]):
        got = _run(capi, ctx, [three[k] for k in order], [CENTERS[k] for k in order], **kw)
        for slot, k in enumerate(order):
            assert _same(got[slot], whole[k]), (order, slot)
    for k in (1, 2):
        alone = _run(capi, ctx, [three[k]], [CENTERS[k]], **kw)[0]
        assert _same(alone, whole[k]), k
    assert whole[0]["rows"] == 0 and whole[2]["rows"] == (40 * N4) // 3000


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------
def test_slabs_and_stages_do_not_enter_the_result(capi, ctx, three):
    kw = dict(nfft=1024, decimation=1024, bandwidth=0.2, kavg=0.1, rows=True)
    arrays, centers = [three[1], np.ascontiguousarray(three[2][: 2 * 9 * 1024])], [0.005, -0.03]
    base = _run(capi, ctx, arrays, centers, **kw)
    assert base[0]["rows"] == 20 and base[1]["rows"] == 9
    for extra in (dict(slab_rows=1), dict(slab_rows=3), dict(slab_rows=5, stages_per_pass=3), dict(stages_per_pass=1), dict(stages_per_pass=2)):
        got = _run(capi, ctx, arrays, centers, **kw, **extra)
        assert all(_same(g, b) for g, b in zip(got, base)), extra
    # nfft 4096 in k_cfft's form (one stage per pass) and the default, slabs of two rows
    kw = dict(nfft=4096, decimation=4096, bandwidth=0.25)
    base = _run(capi, ctx, [three[2]], [0.0], **kw)
    assert base[0]["rows"] == 40
    for extra in (dict(stages_per_pass=1), dict(slab_rows=2), dict(slab_rows=7, stages_per_pass=2)):
        assert _same(_run(capi, ctx, [three[2]], [0.0], **kw, **extra)[0], base[0]), extra


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------
def test_formats_give_the_same_bits(capi, ctx, three):
    u8 = three[1]
    kw = dict(nfft=1024, decimation=2048, bandwidth=0.2, rows=True)
    base = _run(capi, ctx, [u8], [0.005], **kw)[0]
    assert base["rows"] == 10
    for name, items, fmt, scale in sc.formats_of(u8):
        got = _run(capi, ctx, [items], [0.005], lengths=[len(u8) // 2], in_format=getattr(capi, fmt), in_scale=scale if scale else 1.0, **kw)[0]
        assert _same(got, base), name
    # an item-aligned pointer (no 16-byte loads) reads the same values
    buf = ctx.upload(np.concatenate([np.zeros(2, np.uint8), u8]))
    with capi.SpectrumBatch(ctx, 1, len(u8) // 2, **kw) as sb:
        assert _same(sb.run([buf.at(2)], [len(u8) // 2], [0.005])[0], base)
    buf.free()


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------
def test_a_second_run_starts_fresh(capi, ctx, three):
    kw = dict(nfft=1024, decimation=1024, bandwidth=0.2, rows=True, slab_rows=4)
    bufs = [ctx.upload(three[1]), ctx.upload(three[2])]
    with capi.SpectrumBatch(ctx, 2, LENGTHS[2], **kw) as sb:
        first = sb.run([bufs[0].ptr, bufs[1].ptr], [LENGTHS[1], LENGTHS[2]], [0.0, 0.005])
        second = sb.run([bufs[1].ptr, bufs[0].ptr], [11 * 1024 + 3, 6 * 1024], [-0.03, 0.0])
    fresh = _run(capi, ctx, [np.ascontiguousarray(three[2][: 2 * (11 * 1024 + 3)]), np.ascontiguousarray(three[1][: 2 * 6 * 1024])], [-0.03, 0.0], **kw)
    assert first[0]["rows"] == 20 and second[0]["rows"] == 11 and second[1]["rows"] == 6
    assert all(_same(s, f) for s, f in zip(second, fresh))
    for b in bufs:
        b.free()


# ---- 8 -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_usable_object(capi, ctx, three):
    u8 = three[1]
    n = len(u8) // 2
    for kw, word in ((dict(nfft=1000), "power of two"), (dict(nfft=32, decimation=64), "64"), (dict(nfft=8192, decimation=8192), "4096"),
                     (dict(nfft=4096, decimation=4095), "decimation"), (dict(nfft=4096, decimation=4096, bandwidth=0.26), "Fsampling > 4x Fsignal"),
                     (dict(nfft=64, decimation=64, bandwidth=0.05), "no slot"), (dict(nfft=1024, decimation=1024, in_format=7), "in_format"),
                     (dict(nfft=1024, decimation=1024, stages_per_pass=5), "stages_per_pass")):
        with pytest.raises(capi.LsdrError, match=word):
            capi.SpectrumBatch(ctx, 1, n, **kw)
    cfg = capi.SpectrumBatchCfg()
    cfg.n_captures, cfg.max_samples, cfg.in_format, cfg.nfft, cfg.decimation = 1, n, capi.IN_CU8, 1024, 1024
    cfg.reserved[3] = 1
    h = capi.vp()
    assert capi.lib.lsdr_spectrum_batch_create(ctx.h, cfg, h) == -2 and b"reserved" in capi.lib.lsdr_last_error()
    kw = dict(nfft=1024, decimation=2048, bandwidth=0.2, rows=True)
    base = _run(capi, ctx, [u8], [0.005], **kw)[0]
    buf = ctx.upload(u8)
    with capi.SpectrumBatch(ctx, 1, n, **kw) as sb:
        with pytest.raises(capi.LsdrError, match="max_samples"):
            sb.run([buf.ptr], [n + 1], [0.005])
        with pytest.raises(capi.LsdrError, match="no pointer"):
            sb.run([None], [n], [0.005])
        with pytest.raises(capi.LsdrError, match="aligned"):
            sb.run([buf.at(1)], [n - 1], [0.005])
        with pytest.raises(capi.LsdrError, match="centre"):
            sb.run([buf.ptr], [n], [0.5])
        e = (capi.CaptureEach * 1)()
        e[0].n_samples, e[0].tune = n, 0.005
        e[0].reserved[0] = 1
        ptrs = (capi.vp * 1)(buf.ptr)
        assert capi.lib.lsdr_spectrum_batch_run_async(sb.h, ptrs, e) == -2 and b"reserved" in capi.lib.lsdr_last_error()
        with pytest.raises(capi.LsdrError, match="no run in flight"):
            sb.wait()
        with pytest.raises(capi.LsdrError, match="no finished run"):
            sb.cnr_db(0)
        sb.run_async([buf.ptr], [n], [0.005])
        with pytest.raises(capi.LsdrError, match="in flight"):
            sb.run_async([buf.ptr], [n], [0.005])
        with pytest.raises(capi.LsdrError, match="no finished run"):
            sb.rows_db(0)
        sb.wait()
        assert _same(sb.run([buf.ptr], [n], [0.005])[0], base)             # … and the object still runs a valid batch
    with capi.SpectrumBatch(ctx, 1, n, nfft=1024, decimation=2048) as plain:
        plain.run([buf.ptr], [n])
        with pytest.raises(capi.LsdrError, match="no CNR"):
            plain.cnr_db(0)
        with pytest.raises(capi.LsdrError, match="no rows"):
            plain.rows_db(0)
        assert not plain.rows_linear_dev(0)
    buf.free()


# ---- 9 -----------------------------------------------------------------------------------------------------------------------------
def test_resampled_decoder_measures_the_cnr(capi, ctx, oracle):
    offsets = [0.01, -0.03]
    caps = [rc.shifted_sps(16, 12, 7.5, f) for f in offsets]
    n = len(caps[0]) // 2
    bufs = [ctx.upload(iq) for iq in caps]
    dec = capi.ResampledDecoder(ctx, 2, n, 12.0, anf=0)
    try:
        ptrs = [b.ptr for b in bufs]
        res0, ts0, info0 = dec.decode(ptrs, [n, n])
        res1, ts1, info1 = dec.decode(ptrs, [n, n], cnr=True)
        assert "cnr" not in info0[0] and dec.omega_out == 4.0
        for i in range(2):
            assert ts1[i] == ts0[i] and res1[i]["ts_packets"] == res0[i]["ts_packets"] and info1[i]["tune"] == info0[i]["tune"]
            x = dec.outputs(i, info1[i]["produced"])
            want = oracle.cnr_fft(x, 0.25, 4096, dec.cnr_decimation, info1[i]["cnr_center"], 1.0)
            assert info1[i]["cnr_center"] == info1[i]["tune"]
            assert len(want) == (info1[i]["produced"] // 4096 * 4096) // dec.cnr_decimation >= 3
            assert bits_equal(info1[i]["cnr"], want), (i, info1[i]["cnr"], want)
            print(f"offset {offsets[i]}: CNR {info1[i]['cnr']} dB around {info1[i]['cnr_center']:+.3e}")
    finally:
        dec.close()
        for b in bufs:
            b.free()
