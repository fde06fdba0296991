"""Every block of the GPU transmit chain (leansdr_amd/csrc/tx.hip) by itself through the C ABI, bit for bit against the oracle's
function of the same name: all nine constellations, all seven code rates, the grid and wave edges (63 / 64 / 65 items), state carried
through one handle across uneven pieces, and every output-capacity gate.  Then the whole chain on the constellations and rates that
tests/golden/tx.npz does not hold, and the integer cconverters / misaligned elementwise maps (elementwise.hip)."""
import ctypes as C
import numpy as np
import pytest
from conftest import bits_equal
import modcod_common as mc

pytestmark = pytest.mark.gpu

GUARD = 64     # bytes of 0xEE behind every output buffer: must come back untouched


class Out:
    """A device output buffer of `nbytes` followed by a guard band, both filled with 0xEE."""

    def __init__(self, ctx, nbytes, offset=0):
        self.ctx, self.nbytes, self.offset = ctx, int(nbytes), offset
        self.buf = ctx.upload(np.full(offset + self.nbytes + GUARD, 0xEE, np.uint8))
        self.ptr = self.buf.at(offset)

    def take(self, dtype, count):
        """The first `count` items; asserts that nothing behind them (to the end of the guard band) or in front was written."""
        raw = self.ctx.download(self.buf, np.uint8, self.offset + self.nbytes + GUARD)
        self.buf.free()
        used = count * np.dtype(dtype).itemsize
        assert used <= self.nbytes
        assert (raw[:self.offset] == 0xEE).all() and (raw[self.offset + used:] == 0xEE).all(), "wrote outside its output"
        return raw[self.offset:self.offset + used].view(dtype).copy()


def run(capi, ctx, fn, first, x, n_in, cap, out_dtype, item=1):
    """One *_run(first, in, n_in, out, cap, &consumed, &produced) call on an uploaded array -> (output items, consumed, produced)."""
    din = ctx.upload(x)
    out = Out(ctx, max(cap, 1) * item * np.dtype(out_dtype).itemsize)
    cons, prod = C.c_size_t(), C.c_size_t()
    capi.check(fn(first, din.ptr, n_in, out.ptr, cap, C.byref(cons), C.byref(prod)))
    ctx.sync()
    din.free()
    assert prod.value <= cap
    return out.take(out_dtype, prod.value * item), cons.value, prod.value


def ts_input(n, seed=0):
    from leansdr_amd import synth_dvbs
    return synth_dvbs.ts_packets(n, start=seed)


# ---------------------------------------------------------------------------------------------- randomizer
def test_randomizer_pieces_and_capacity(capi, ctx, oracle):
    """40 packets in pieces of 1, 7, 8, 9 and 15: the position in the 8-packet (1504-byte) pattern is carried through every phase;
    then a call with room for fewer packets than it is given."""
    lib = capi.lib
    ts = ts_input(45)
    want = oracle.randomizer(ts)
    h = capi.vp()
    capi.check(lib.lsdr_randomizer_create(ctx.h, C.byref(h)))
    pos, got = 0, []
    for n in (1, 7, 8, 9, 15):
        y, cons, prod = run(capi, ctx, lib.lsdr_randomizer_run, h, ts[pos:pos + n], n, n, np.uint8, 188)
        assert cons == n and prod == n
        got.append(y)
        pos += n
    assert pos == 40
    y, cons, prod = run(capi, ctx, lib.lsdr_randomizer_run, h, ts[40:45], 5, 3, np.uint8, 188)     # cap_packets < n_packets
    assert cons == 3 and prod == 3
    got.append(y)
    y, cons, prod = run(capi, ctx, lib.lsdr_randomizer_run, h, ts[43:45], 2, 2, np.uint8, 188)     # the position moved by 3, not 5
    got.append(y)
    lib.lsdr_randomizer_destroy(h)
    assert bits_equal(np.concatenate(got).reshape(-1, 188), want)


# ---------------------------------------------------------------------------------------------- rs_encoder
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_rs_encoder_grid_edges(capi, ctx, oracle, n):
    """One thread per packet, 64 per block: packet counts around the block edge; all-zero, all-0xFF and random payloads."""
    rng = np.random.default_rng(957)
    for name, ts in (("zero", np.zeros((n, 188), np.uint8)), ("ff", np.full((n, 188), 0xFF, np.uint8)),
                     ("random", rng.integers(0, 256, (n, 188), dtype=np.uint8))):
        y, cons, prod = run(capi, ctx, capi.lib.lsdr_rs_encoder_run, ctx.h, ts, n, n, np.uint8, 204)
        assert cons == n and prod == n, name
        assert bits_equal(y.reshape(-1, 204), oracle.rs_encoder(ts)), name
    if n == 65:
        y, cons, prod = run(capi, ctx, capi.lib.lsdr_rs_encoder_run, ctx.h, ts, n, 64, np.uint8, 204)    # cap_packets < n_packets
        assert cons == 64 and prod == 64 and bits_equal(y.reshape(-1, 204), oracle.rs_encoder(ts[:64]))


# ---------------------------------------------------------------------------------------------- interleaver
@pytest.mark.parametrize("n", [11, 12, 13, 40])
def test_interleaver(capi, ctx, oracle, n):
    """n packets give n - 11 interleaved ones (nothing below 12); a capacity of 204·k + 100 bytes lets only k whole packets out."""
    pk = np.random.default_rng(899 + n).integers(0, 256, (n, 204), dtype=np.uint8)
    want = oracle.interleaver(pk)
    assert len(want) == max(0, n - 11) * 204
    y, cons, prod = run(capi, ctx, capi.lib.lsdr_interleaver_run, ctx.h, pk, n, n * 204, np.uint8)
    assert cons == max(0, n - 11) and prod == len(want) and bits_equal(y, want)
    k = min(5, max(0, n - 11))
    y, cons, prod = run(capi, ctx, capi.lib.lsdr_interleaver_run, ctx.h, pk, n, 204 * k + 100, np.uint8)
    assert cons == k and prod == 204 * k and bits_equal(y, want[:204 * k])


# ---------------------------------------------------------------------------------------------- dvb_convol
@pytest.mark.parametrize("rate,bps", mc.CONVOL_PAIRS)
def test_dvb_convol(capi, ctx, oracle, rate, bps):
    """Every code rate x every symbol width its puncturing period allows, one handle fed exactly one group (bits_in bytes: at rate
    1/2 a single byte, the one-byte path of the history carry), then 2 groups, 5 groups and the rest; then a capacity that admits
    less than the input: consumed stays a whole number of groups (dvb.h:589-598)."""
    lib = capi.lib
    data = mc.convol_input()
    want, _ = oracle.dvb_convol(data, rate, bps)
    bi, bo = mc.FEC_BITS[rate]
    h = capi.vp()
    capi.check(lib.lsdr_convol_create(ctx.h, rate, bps, C.byref(h)))
    pos, got = 0, []
    for groups in (1, 2, 5, len(data)):
        piece = data[pos:pos + groups * bi]
        y, cons, prod = run(capi, ctx, lib.lsdr_convol_run, h, piece, len(piece), len(piece) * 16 + 64, np.uint8)
        assert cons == len(piece) and prod == len(piece) * 8 // bi * bo // bps
        got.append(y)
        pos += cons
    lib.lsdr_convol_destroy(h)
    assert pos == len(data) and bits_equal(np.concatenate(got), want)
    # capacity gate, on a fresh handle: the reference's integer expression, evaluated left to right
    cap = 997
    count = min(len(data), cap * bps // bo * bi // 8) // bi * bi
    assert 0 < count < len(data)
    capi.check(lib.lsdr_convol_create(ctx.h, rate, bps, C.byref(h)))
    y, cons, prod = run(capi, ctx, lib.lsdr_convol_run, h, data, len(data), cap, np.uint8)
    lib.lsdr_convol_destroy(h)
    assert cons == count and cons % bi == 0 and prod == count * 8 // bi * bo // bps
    assert bits_equal(y, want[:prod])


def test_dvb_convol_illegal_pair(capi, ctx):
    h = capi.vp()
    with pytest.raises(capi.LsdrError):           # rate 1/2 puts out 2 bits per group: no whole number of 3-bit symbols
        capi.check(capi.lib.lsdr_convol_create(ctx.h, 0, 3, C.byref(h)))


# ---------------------------------------------------------------------------------------------- cstln_transmitter
def cstln_tx(capi, ctx, sym, cstln, rate):
    din = ctx.upload(sym)
    out = Out(ctx, len(sym) * 8)
    capi.check(capi.lib.lsdr_cstln_transmitter_run(ctx.h, cstln, rate, din.ptr, len(sym), out.ptr))
    ctx.sync()
    din.free()
    return out.take(np.complex64, len(sym))


@pytest.mark.parametrize("cstln,rate", mc.TX_PAIRS)
def test_cstln_transmitter(capi, ctx, oracle, cstln, rate):
    sym = mc.tx_symbols(cstln)                    # every symbol value once, then 1000 random ones
    assert bits_equal(cstln_tx(capi, ctx, sym, cstln, rate), oracle.cstln_transmitter(sym, cstln, rate))


def test_cstln_transmitter_illegal_pair(capi, ctx):
    with pytest.raises(capi.LsdrError):           # 16APSK has no radius ratio for rate 1/2
        cstln_tx(capi, ctx, np.zeros(4, np.uint8), 3, 0)


# ---------------------------------------------------------------------------------------------- fir_resampler
def resampler(capi, ctx, co, interp, freq):
    h = capi.vp()
    capi.check(capi.lib.lsdr_fir_resampler_create(ctx.h, len(co), co.ctypes.data_as(capi.vp), interp, C.byref(h)))
    if freq:
        capi.check(capi.lib.lsdr_fir_resampler_set_freq(h, freq))
    return h


@pytest.mark.parametrize("ncoeffs,interp,freq", mc.RESAMPLER_CASES + mc.RESAMPLER_DIVIDING)
def test_fir_resampler(capi, ctx, oracle, ncoeffs, interp, freq):
    """One shot == the oracle with a NaN sample lying right behind the n_in samples handed over (where interp divides ncoeffs the
    reference's count would read it); the stream in pieces, one of them too short to make progress, == the one shot; a capacity that
    is no multiple of interp (seven of the eight shapes: at interp = 1 there is none) lets only whole groups out."""
    lib = capi.lib
    co, x = mc.resampler_coeffs(ncoeffs), mc.resampler_input()
    n = len(x)
    want, wcons = oracle.fir_resampler(co, interp, x, freq)
    assert wcons == n - (ncoeffs + interp) // interp
    padded = np.concatenate([x, np.array([np.nan + 1j * np.nan], np.complex64)])
    h = resampler(capi, ctx, co, interp, freq)
    y, cons, prod = run(capi, ctx, lib.lsdr_fir_resampler_run, h, padded, n, n * interp, np.complex64)
    assert not np.isnan(y.view(np.float32)).any()
    assert cons == wcons and prod == wcons * interp and bits_equal(y, want)
    # pieces: the caller carries what a call leaves unconsumed
    hold, got = np.zeros(0, np.complex64), []
    for k, piece in enumerate((ncoeffs - 1, 100, 7, 1500, n)):
        buf = np.concatenate([hold, x[:piece]])
        x = x[piece:]
        y, cons, prod = run(capi, ctx, lib.lsdr_fir_resampler_run, h, np.concatenate([buf, padded[-1:]]), len(buf), n * interp, np.complex64)
        if k == 0:
            assert cons == 0 and prod == 0        # fewer than ncoeffs samples: no progress
        got.append(y)
        hold = buf[cons:]
    assert len(x) == 0 and len(hold) == n - wcons
    assert bits_equal(np.concatenate(got), want)
    # capacity gate
    cap = 10 * interp + interp // 2                # no multiple of interp, except at interp = 1 where every capacity is one
    assert cap % interp or interp == 1
    y, cons, prod = run(capi, ctx, lib.lsdr_fir_resampler_run, h, padded, n, cap, np.complex64)
    assert cons == 10 and prod == 10 * interp and bits_equal(y, want[:prod])
    lib.lsdr_fir_resampler_destroy(h)


# ---------------------------------------------------------------------------------------------- simple_agc
def agc_input(chunks, extra=50):
    """`chunks` chunks of 128 samples, the first three all zero (no estimate yet: gain 0), plus a tail that is not consumed."""
    rng = np.random.default_rng(238)
    n = chunks * 128 + extra
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (3 + np.arange(n) / 2000.0)).astype(np.complex64)
    x[:3 * 128] = 0
    return x


@pytest.mark.parametrize("chunks", [1, 63, 64, 65, 129, 200])
def test_simple_agc_block_edges(capi, ctx, oracle, chunks):
    """Chunk counts around the 64-chunk blocks of the gain kernel; the estimate starts at 0 and is seeded by the first non-zero chunk."""
    lib = capi.lib
    x = agc_input(chunks)
    want, _ = oracle.simple_agc(x, 0.7, 0.01)
    assert len(want) == chunks * 128 and not want[:min(chunks, 3) * 128].any() and (chunks <= 3 or want[3 * 128:].all())
    h = capi.vp()
    capi.check(lib.lsdr_simple_agc_create(ctx.h, 0.7, 0.01, C.byref(h)))
    y, cons, prod = run(capi, ctx, lib.lsdr_simple_agc_run, h, x, len(x), len(x), np.complex64)
    assert cons == chunks * 128 and prod == chunks * 128 and bits_equal(y, want)
    if chunks == 65:      # capacity gate on a fresh estimate: whole chunks only
        lib.lsdr_simple_agc_destroy(h)
        capi.check(lib.lsdr_simple_agc_create(ctx.h, 0.7, 0.01, C.byref(h)))
        y, cons, prod = run(capi, ctx, lib.lsdr_simple_agc_run, h, x, len(x), 128 * 5 + 100, np.complex64)
        assert cons == 640 and prod == 640 and bits_equal(y, want[:640])
    lib.lsdr_simple_agc_destroy(h)


@pytest.mark.parametrize("reset", [False, True])
def test_simple_agc_pieces(capi, ctx, oracle, reset):
    """200 chunks in pieces of 1, 63, 70 and 66 through one handle (the first call leaves the estimate at 0, the second seeds it in
    its third chunk) == one shot; with lsdr_simple_agc_set between two calls == the oracle given the new parameters there."""
    lib = capi.lib
    x = agc_input(200, extra=0)
    h = capi.vp()
    capi.check(lib.lsdr_simple_agc_create(ctx.h, 0.7, 0.01, C.byref(h)))
    pos, got, want, est, par = 0, [], [], 0.0, (0.7, 0.01)
    for k, chunks in enumerate((1, 63, 70, 66)):
        if reset and k == 2:
            par = (1.5, 0.05)
            capi.check(lib.lsdr_simple_agc_set(h, *par))
        piece = x[pos:pos + chunks * 128]
        y, cons, prod = run(capi, ctx, lib.lsdr_simple_agc_run, h, piece, len(piece), len(piece), np.complex64)
        assert cons == len(piece) and prod == len(piece)
        w, est = oracle.simple_agc(piece, par[0], par[1], est)
        got.append(y); want.append(w)
        pos += cons
    lib.lsdr_simple_agc_destroy(h)
    assert pos == len(x) and bits_equal(np.concatenate(got), np.concatenate(want))
    if not reset:
        assert bits_equal(np.concatenate(got), oracle.simple_agc(x, 0.7, 0.01)[0])


# ---------------------------------------------------------------------------------------------- the whole chain
@pytest.mark.parametrize("cstln,rate", [(0, 0), (1, 5), (4, 6), (5, 4), (6, 3), (7, 4), (8, 5)])
def test_tx_chain_modcods(capi, ctx, oracle, cstln, rate):
    """The constellations and code rates that tests/golden/tx.npz does not hold."""
    ts = ts_input(24)
    want = oracle.tx_chain(ts, interp=3, amp=75.0, cstln=cstln, rate=rate)
    tx = capi.TxChain(ctx, interp=3, amp=75.0, cstln=cstln, rate=rate)
    y = tx.run(ts)
    tx.close()
    assert len(want) > 1000 and len(y) == len(want) and bits_equal(y, want)


# ---------------------------------------------------------------------------------------------- elementwise maps
COUNTS = [0, 1, 2, 3, 5, 1025]
INT_FORMATS = [("cs8", np.int8, 0, -128, 127), ("cu16", np.uint16, 32768, 0, 65535), ("cs16", np.int16, 0, -32768, 32767)]


def int_input(dtype, lo, hi, n):
    iq = np.random.default_rng(40 + n).integers(lo, hi + 1, 2 * n).astype(dtype)
    iq[:4] = np.array([lo, hi, hi, lo], dtype)[:len(iq[:4])]          # the extremes of the type
    return iq


def int_want(iq, zero):
    return (iq.astype(np.int64) - zero).astype(np.float32).view(np.complex64)


@pytest.mark.parametrize("name,dtype,zero,lo,hi", INT_FORMATS, ids=[f[0] for f in INT_FORMATS])
def test_cconverter_int(capi, ctx, name, dtype, zero, lo, hi):
    """cconverter<s8,0>, <u16,32768>, <s16,0> -> f32 (dsp.h:40-50): (in - Zin) in integer arithmetic, then converted."""
    fmt = {"cs8": capi.IN_CS8, "cu16": capi.IN_CU16, "cs16": capi.IN_CS16}[name]
    for n in COUNTS:
        iq = int_input(dtype, lo, hi, n)
        assert bits_equal(ctx.cconverter_int(fmt, iq), int_want(iq, zero)), n


def offset_call(capi, ctx, launch, x, n, in_item, want):
    """`launch(in_ptr, n, out_ptr)` with both pointers one item into their allocations: the input is not 8- or 16-byte aligned, the
    output not 16-byte aligned.  Same values as `want`, nothing written in front of or behind the n outputs."""
    raw = np.concatenate([np.full(in_item, 0xEE, np.uint8), np.ascontiguousarray(x).view(np.uint8).reshape(-1)])
    din = ctx.upload(raw)
    out = Out(ctx, n * 8, offset=8)
    capi.check(launch(din.at(in_item), n, out.ptr))
    ctx.sync()
    din.free()
    assert bits_equal(out.take(np.complex64, n), want)


@pytest.mark.parametrize("n", COUNTS)
def test_elementwise_misaligned(capi, ctx, oracle, n):
    """The scalar branches of k_cconv_u8, k_scale and k_cconv_int: the same values as the aligned call, inside their n outputs only."""
    lib = capi.lib
    rng = np.random.default_rng(33 + n)
    u8 = rng.integers(0, 256, 2 * n, dtype=np.uint8)
    want = oracle.cconverter_u8(u8)
    assert bits_equal(ctx.cconverter_u8(u8), want)
    offset_call(capi, ctx, lambda i, k, o: lib.lsdr_cconverter_u8_run(ctx.h, i, k, o), u8, n, 2, want)
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 100).astype(np.complex64)
    want = oracle.scaler(0.0123, x)
    assert bits_equal(ctx.scaler(0.0123, x), want)
    offset_call(capi, ctx, lambda i, k, o: lib.lsdr_scaler_run(ctx.h, 0.0123, i, k, o), x, n, 8, want)
    for name, dtype, zero, lo, hi in INT_FORMATS:
        fmt = {"cs8": capi.IN_CS8, "cu16": capi.IN_CU16, "cs16": capi.IN_CS16}[name]
        iq = int_input(dtype, lo, hi, n)
        offset_call(capi, ctx, lambda i, k, o: lib.lsdr_cconverter_int_run(ctx.h, fmt, i, k, o), iq, n, 2 * np.dtype(dtype).itemsize,
                    int_want(iq, zero))


def test_decimator_capacity(capi, ctx, oracle):
    """decimator with room for fewer than n/d outputs: produced = cap, nothing behind them written."""
    x = mc.resampler_input(1000)
    din = ctx.upload(x)
    for d, cap in ((3, 100), (7, 1), (1, 999), (5, 0)):
        out = Out(ctx, cap * 8)
        prod = C.c_size_t()
        capi.check(capi.lib.lsdr_decimator_run(ctx.h, d, din.ptr, len(x), out.ptr, cap, C.byref(prod)))
        ctx.sync()
        assert prod.value == cap < len(x) // d
        assert bits_equal(out.take(np.complex64, cap), oracle.decimator(d, x)[:cap])
    din.free()
