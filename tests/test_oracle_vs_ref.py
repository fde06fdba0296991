"""The oracle against the REAL reference run here (oracle/_ref, built from
/root/reference by oracle/Makefile).  Skipped where oracle/_ref is absent —
the committed goldens (test_oracle_golden.py) cover that case."""
import numpy as np
import pytest
from conftest import bits_equal, gold
import pyoracle as po
import modcod_common as mc


@pytest.fixture(scope="module")
def sig():
    rng = np.random.default_rng(7)
    n = 30000
    # QPSK-like stream at 4 samples/symbol with noise, amplitude ~75 (enough to lock)
    syms = (rng.integers(0, 2, n // 4 + 8) * 2 - 1) + 1j * (rng.integers(0, 2, n // 4 + 8) * 2 - 1)
    up = np.zeros(len(syms) * 4, np.complex64)
    up[::4] = syms
    h = np.hanning(9).astype(np.float32)
    x = np.convolve(up, h)[:n] * 40 + (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 6
    return x.astype(np.complex64)


def test_tables_all_constellations(oracle, ref):
    assert bits_equal(oracle.trig16(), ref.trig16())
    for pre, fec in [(0, 0), (1, 0), (2, 1), (3, 1), (3, 3), (3, 8), (4, 3), (4, 8), (5, 0), (6, 0), (7, 0), (8, 0)]:
        a, b = oracle.cstln_lut(pre, fec), ref.cstln_lut(pre, fec)
        for k in ("symbols", "cost", "symbol", "phase_error"):
            assert bits_equal(a[k], b[k]), (pre, fec, k)
    for a in [-1.5, 70000.7, 0.0, -65536.5, 32767.9, -32768.2, 1e6, -1e6 + 0.3, 123456.7]:
        assert oracle.lib.lo_trig16_index(a) == ref.lib.ref_trig16_index(a)


@pytest.mark.parametrize("order,fcut", [(312, (2e6 / 2) * (1 + 0.35 / 2) / 240e6), (14, 0.4895), (40, 0.1), (1, 0.3), (99, 0.02)])
def test_lowpass(oracle, ref, order, fcut):
    assert bits_equal(oracle.lowpass(order, np.float32(fcut)), ref.lowpass(order, np.float32(fcut)))
    assert bits_equal(oracle.lowpass(order, np.float32(fcut), False), ref.lowpass(order, np.float32(fcut), False))


@pytest.mark.parametrize("order,fs,ro", [(166, 2e6 / (8e6 * 16), 0.35), (41, 0.25, 0.35), (64, 0.25, 0.25), (100, 0.5, 0.2), (33, 1 / 3.0, 0.35)])
def test_rrc(oracle, ref, order, fs, ro):
    assert bits_equal(oracle.rrc(order, np.float32(fs), np.float32(ro)), ref.rrc(order, np.float32(fs), np.float32(ro)))


def test_elementwise(oracle, ref, sig):
    rng = np.random.default_rng(1)
    u8 = rng.integers(0, 256, 2 * 5000, dtype=np.uint8)
    assert bits_equal(oracle.cconverter_u8(u8), ref.cconverter_u8(u8))
    assert bits_equal(oracle.scaler(0.0123, sig), ref.scaler(0.0123, sig))


@pytest.mark.parametrize("n,d,freq", [(313, 30, 0.0), (313, 30, 0.001), (313, 30, -0.0123), (21, 1, 0.0), (21, 7, 0.05), (2, 3, 0.2), (64, 64, 0.0)])
def test_fir_filter(oracle, ref, sig, n, d, freq):
    c = oracle.lowpass(n - 1, np.float32(0.4 / d))
    a, cons = oracle.fir_filter(c, d, sig, freq)
    b, sc = ref.fir_filter(c, d, sig, freq)
    assert bits_equal(oracle.fir_shift(c, freq), sc)
    assert bits_equal(a, b) and cons == len(a) * d


def test_fir_resampler(oracle, ref, sig):
    rr = oracle.rrc(41, np.float32(0.25), np.float32(0.35))
    for f in (0.0, 0.01):
        a, _ = oracle.fir_resampler(rr, 4, sig[:3000], f)
        assert bits_equal(a, ref.fir_resampler(rr, 4, sig[:3000], f))


def test_fft_notch_cnr(oracle, ref, sig):
    assert bits_equal(oracle.cfft(sig[:4096]), ref.cfft(sig[:4096]))
    assert bits_equal(oracle.cfft(sig[:1024], True), ref.cfft(sig[:1024], True))
    t = np.arange(4096 * 7)
    x = (np.resize(sig, len(t)) * 0.2 + 60 * np.exp(2j * np.pi * 0.123 * t) + 30 * np.exp(-2j * np.pi * 0.31 * t)).astype(np.complex64)
    for ns, sp in [(1, 0.0), (2, 0.0), (3, 0.0), (1, 30.0)]:
        a, ba = oracle.auto_notch(x, ns, 4096 * 3, setpoint=sp)
        b, bb = ref.auto_notch(x, ns, 4096 * 3, setpoint=sp)
        assert ba == [int(v) for v in bb] and bits_equal(a, b)
    assert bits_equal(oracle.cnr_fft(x, 0.2, 4096, 8192, 0.01, 0.5), ref.cnr_fft(x, 0.2, 4096, 8192, 0.01, 0.5))
    for dec, k in [(2048, 0.5), (5000, 0.1), (1024, 0.9)]:
        assert bits_equal(oracle.spectrum(x, dec, k), ref.spectrum(x, dec, k))


def same_rx(a, b):
    assert bits_equal(a["sym"]["cost"], b["sym"]["cost"]) and bits_equal(a["sym"]["symbol"], b["sym"]["symbol"])
    for k in ("freq", "ss", "mer", "cstln"):
        assert bits_equal(a[k], b[k]), k
    sa, sb = a["state"].as_dict(), b["state"].as_dict()
    for k in sa:
        if k == "hist":
            assert np.array(sa[k], np.float32).tobytes() == np.array(sb[k], np.float32).tobytes()
        elif k == "meas_count":
            assert sa[k] == sb[k]
        else:
            assert np.float32(sa[k]).tobytes() == np.float32(sb[k]).tobytes(), k


@pytest.mark.parametrize("kw", [
    dict(sampler=1, cstln=1, omega=4.0, meas_decimation=4096),
    dict(sampler=0, cstln=1, omega=4.0, meas_decimation=1000),
    dict(sampler=1, cstln=1, omega=4.0, freq=0.01, allow_drift=1, meas_decimation=4096),
    dict(sampler=1, cstln=1, omega=4.0, freq=-0.03, meas_decimation=4096),
    dict(sampler=1, cstln=2, fec=1, omega=4.0, meas_decimation=4096),
    dict(sampler=1, cstln=0, omega=4.0, meas_decimation=4096),
    dict(sampler=1, cstln=3, fec=3, omega=4.0, meas_decimation=4096),
    dict(sampler=1, cstln=1, omega=3.7, pll_adjustment=1 / 6.0, meas_decimation=256),
    dict(sampler=1, cstln=1, omega=4.0, kest=0.05, meas_decimation=4096),
], ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items() if a not in ("meas_decimation",)))
def test_cstln_receiver(oracle, ref, sig, kw):
    p = po.rx_params(**kw)
    same_rx(oracle.rx(p, sig), ref.rx(p, sig))


def test_cstln_receiver_fir_sampler(oracle, ref, sig):
    rr = oracle.rrc(int(10 * 8e6 * 16 / (22 * (2e6 / 2) * 0.35)), np.float32(2e6 / (8e6 * 16)), np.float32(0.35))
    p = po.rx_params(sampler=2, coeffs=rr, subsampling=16, cstln=1, omega=4.0, meas_decimation=4096)
    same_rx(oracle.rx(p, sig * np.float32(16)), ref.rx(p, sig * np.float32(16)))
    rr1 = oracle.rrc(40, np.float32(0.25), np.float32(0.35))
    p = po.rx_params(sampler=2, coeffs=rr1, subsampling=1, cstln=1, omega=4.0, meas_decimation=4096)
    same_rx(oracle.rx(p, sig), ref.rx(p, sig))


@pytest.mark.parametrize("case", mc.RX_SWEEP, ids=mc.case_id)
def test_cstln_receiver_modcods(oracle, ref, case):
    """Every constellation (with one code rate each) x five settings x nearest / linear, and the FIR sampler twice: what the GPU's exact
    receivers are held to (test_gpu_rx_modcods.py) is the compiled reference's output, bit for bit — and the inputs do exercise what
    they are meant to: the whole symbol table, and the !allow_drift reset of the frequency limits (sdr.h:895-898)."""
    c, r, v, s = case
    rrc = gold("tables.npz")["rrc_rx"] if s == 2 else None
    x = mc.rx_input(oracle, c, r, v, s)
    a = mc.oracle_rx(oracle, case, rrc)
    same_rx(a, ref.rx(po.rx_params(**mc.rx_kwargs(c, r, v, s, rrc)), x))
    assert len(a["sym"]) > 4000 and len(a["freq"]) >= 14
    distinct = len(np.unique(a["sym"]["symbol"]))
    n = mc.NSYMBOLS[c]
    assert distinct >= {64: 48, 256: 128}.get(n, n), distinct
    if v == "clamp" and c in (1, 2, 3, 4):
        assert (a["freq"][1:] == 0).any()
    if v == "sps3_loud_drift":
        assert np.abs(x.view(np.float32)).max() > 127


@pytest.mark.parametrize("cstln,rate", mc.TX_PAIRS)
def test_cstln_transmitter(oracle, ref, cstln, rate):
    sym = mc.tx_symbols(cstln)
    assert bits_equal(oracle.cstln_transmitter(sym, cstln, rate), ref.cstln_transmitter(sym, cstln, rate))


@pytest.mark.parametrize("rate,bps", mc.CONVOL_PAIRS)
def test_dvb_convol(oracle, ref, rate, bps):
    """Every code rate with every symbol width its puncturing period allows."""
    data = mc.convol_input()
    a, cons = oracle.dvb_convol(data, rate, bps)
    bi, bo = mc.FEC_BITS[rate]
    assert cons == len(data) and len(a) == len(data) * 8 // bi * bo // bps
    assert bits_equal(a, ref.dvb_convol(data, rate, bps))


def test_simple_agc_before_the_first_estimate(oracle, ref):
    """Leading all-zero chunks: no estimate, gain 0; the first non-zero chunk seeds it (sdr.h:253-273)."""
    x = mc.resampler_input(128 * 70)
    x[:3 * 128] = 0
    ya, ea = oracle.simple_agc(x, 0.7, 0.01)
    yb, eb = ref.simple_agc(x, 0.7, 0.01)
    assert bits_equal(ya, yb) and ea == eb and not ya[:3 * 128].any() and ya[3 * 128:].all()


@pytest.mark.parametrize("ncoeffs,interp,freq", mc.RESAMPLER_CASES)
def test_fir_resampler_shapes(oracle, ref, ncoeffs, interp, freq):
    co, x = mc.resampler_coeffs(ncoeffs), mc.resampler_input()
    a, cons = oracle.fir_resampler(co, interp, x, freq)
    assert cons == len(x) - -(-ncoeffs // interp) and len(a) == cons * interp
    assert bits_equal(a, ref.fir_resampler(co, interp, x, freq))


@pytest.mark.parametrize("ncoeffs,interp,freq", mc.RESAMPLER_DIVIDING)
def test_fir_resampler_interp_divides_ncoeffs(oracle, ref, ncoeffs, interp, freq):
    """Where interp divides ncoeffs the reference's last output group reads in[n_in], a pipe slot nobody has written.  The oracle
    (and the GPU block) hold that one input sample back: every other output is the reference's, no read leaves the input (a NaN
    behind it does not show), and the held-back group comes out of the next call, from real data."""
    co, x = mc.resampler_coeffs(ncoeffs), mc.resampler_input()
    padded = np.concatenate([x, np.array([np.nan + 1j * np.nan], np.complex64)])
    a, cons = oracle.fir_resampler(co, interp, padded[:len(x)], freq)
    b = ref.fir_resampler(co, interp, x, freq)
    assert cons == len(x) - ncoeffs // interp - 1 and len(a) == cons * interp and len(b) == len(a) + interp
    assert bits_equal(a, b[:len(a)]) and not np.isnan(a.view(np.float32)).any()
    more = np.concatenate([x, mc.resampler_input(64)[:50]])
    whole, _ = oracle.fir_resampler(co, interp, more, freq)
    nxt, _ = oracle.fir_resampler(co, interp, more[cons:], freq)
    assert bits_equal(np.concatenate([a, nxt]), whole)


def test_rotator(oracle, ref, sig):
    for f in (0.01, -0.123, 0.4999, 1e-5):
        assert bits_equal(oracle.rotator(sig, f, splits=(7, 3000)), ref.rotator(sig, f))


@pytest.mark.parametrize("nslots", [1, 2, 3])
def test_auto_notch_long_interferer_stream_pinned(oracle, ref, nslots):
    """(CPU) the stream the GPU's scan-mode notch is held against (tests/test_gpu_notch.py::test_scan_mode_vs_oracle: three CW
    interferers on noise, 300 blocks, detect every 100): the oracle's output and bins are the compiled reference's, bit for bit."""
    rng = np.random.default_rng(11)
    n = 4096 * 300
    t = np.arange(n)
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 12 + 70 * np.exp(2j * np.pi * 0.0713 * t)
         + 40 * np.exp(-2j * np.pi * 0.27 * t) + 25 * np.exp(2j * np.pi * 0.4 * t)).astype(np.complex64)
    a, ba = oracle.auto_notch(x, nslots, 4096 * 100)
    b, bb = ref.auto_notch(x, nslots, 4096 * 100)
    assert ba == [int(v) for v in bb] and bits_equal(a, b)
