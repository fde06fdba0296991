"""lsdr_resample_batch without a GPU: the C ABI (header as C99, struct sizes, exported symbols), the filter design against the oracle's
filtergen under leandvb's rule, the arithmetic's numpy float32 restatement (resample_common) against the oracle's blocks — what the device
is then held to bit for bit in test_gpu_resample_batch.py — and the two-stage carrier estimate in float64.

The restatement against the reference chain rotator<f32>(−ifreq/65536) → fir_filter (lo_rotator_new, lo_fir_filter).  With ifreq == 0 the
two are equal as values.  With ifreq != 0 they differ by the reference's phase noise: its table is cosf / sinf of an angle rounded to float
(up to 2π·65535·|ifreq|/65536 ≈ 5e4 rad, whose float spacing is 3.9e-3 rad), the restatement's phases are exact.  MEASURED on the first 40000
samples of the 12-samples-per-symbol capture (noise 7.5, D = 3, N = 33) at the ifreq of tunes 0.01, −0.03, 0.1 and −0.12: the largest
|difference| over the output's RMS is 1.7e-5, 2.1e-4, 3.5e-3 and 9.0e-3 (it grows with |ifreq|, as the angle's spacing does).  REF_CHAIN_BOUND
(resample_common) is four times the largest, rounded up to one digit: 4e-2; the margin covers other seeds and offsets.  The GPU test uses the same bound.

The two-stage estimate (tune_common.estimate, float64): the raw-rate estimate f0, derotation by (int)(f0·65536)/65536, the low-pass and
the decimation of the restatement, a second estimate on the decimated stream against the TRUE residual (f − ifreq/65536)·D, at 10, 12, 16 and
33 samples per symbol, noise 7.5 and 18, offsets 0, 0.01, −0.03, 0.1 and −0.12.  Bound: an eighth of the decoder's tuning window
1/(2048·omega/D) (1.2e-5 to 1.5e-5).  Measured here: the raw estimate within 3.8e-6 of the offset; the fine one within 1.6e-6 of the residual, but for one
case (12 samples per symbol, noise 18, offset −0.03: the residual sits at a bin's centre, where the interpolation's sign is a coin toss) at 7.5e-6.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import resample_common as rc
import tune_common as tc
from conftest import ROOT, bits_equal

SYMBOLS = ("lsdr_resample_design", "lsdr_resample_batch_create", "lsdr_resample_batch_destroy", "lsdr_resample_batch_tile",
           "lsdr_resample_batch_run_async", "lsdr_resample_batch_wait")
REF_CHAIN_BOUND, CHAIN_TUNES, CHAIN_SAMPLES = rc.REF_CHAIN_BOUND, rc.CHAIN_TUNES, rc.CHAIN_SAMPLES
OMEGAS = {9.6: (2, 25), 10.0: (2, 27), 12.0: (3, 33), 16.0: (4, 43), 33.0: (8, 87), 120.0: (30, 313)}


def test_header_is_c99_and_the_structs_have_their_sizes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "lsdr_hip.h"\n'
                   "typedef char result_is_32_bytes[sizeof(lsdr_resample_result) == 32 ? 1 : -1];\n"
                   "typedef char cfg_is_72_bytes[sizeof(lsdr_resample_batch_cfg) == 72 ? 1 : -1];\n"
                   "int main(void) { lsdr_resample_batch_cfg c; lsdr_resample_result r; c.reserved[5] = 0; r.pad[1] = 0; (void)c; (void)r;\n"
                   "  int (*w)(lsdr_resample_batch *, lsdr_resample_result *) = lsdr_resample_batch_wait; (void)w;\n"
                   "  int (*a)(lsdr_resample_batch *, const void *const *, const lsdr_capture_each *, lsdr_cf32 *const *, size_t) = lsdr_resample_batch_run_async;\n"
                   "  (void)a; return LSDR_ABI_VERSION == 2 ? LSDR_OK : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_resampler(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert ctypes.sizeof(capi.ResampleResult) == 32 and ctypes.sizeof(capi.ResampleBatchCfg) == 72
    assert capi.lib.lsdr_abi_version() == 2


@pytest.mark.parametrize("omega", sorted(OMEGAS))
def test_design_is_leandvbs_rule_over_the_oracles_filtergen(capi, oracle, omega):
    d, order, fcut = rc.design(omega)
    assert (d, order + 1) == OMEGAS[omega]
    want = oracle.lowpass(order, fcut)                       # lo_lowpass + lo_normalize_dcgain(1)
    got_d, got = capi.resample_design(omega)
    assert got_d == d and bits_equal(got, want), (omega, got_d, len(got))
    assert abs(float(got.astype(np.float64).sum()) - 1.0) < 1e-6
    # a given decimation is taken as it is; the taps do not depend on it
    d5, c5 = capi.resample_design(omega, decim=5)
    assert d5 == 5 and bits_equal(c5, want)


def test_design_arguments(capi):
    lib = capi.lib
    d, n = ctypes.c_uint(), ctypes.c_uint()
    buf = np.empty(8, np.float32)
    assert lib.lsdr_resample_design(12.0, 0.35, 10.0, 0, ctypes.byref(d), buf.ctypes.data, 8, ctypes.byref(n)) == -2
    assert (d.value, n.value) == (3, 33) and "33" in lib.lsdr_last_error().decode()
    for omega, rolloff, rej, word in ((0.5, 0.35, 10.0, "omega"), (float("nan"), 0.35, 10.0, "omega"), (12.0, 0.0, 10.0, "rolloff"), (12.0, 0.35, -1.0, "rej")):
        assert lib.lsdr_resample_design(omega, rolloff, rej, 0, ctypes.byref(d), None, 0, ctypes.byref(n)) == -2
        assert word in lib.lsdr_last_error().decode()


@pytest.fixture(scope="module")
def head12(oracle):
    """The head of the 12-sps capture, converted (the oracle's cconverter), with leandvb's filter for it."""
    iq = rc.capture_sps(16, 12, 7.5)[0][: 2 * CHAIN_SAMPLES]
    d, order, fcut = rc.design(12.0)
    return iq, oracle.cconverter_u8(iq), oracle.lowpass(order, fcut), d


def test_restatement_with_ifreq_0_is_fir_filter(oracle, head12):
    iq, x, h, d = head12
    for tune in (0.0, 1e-5, -1e-5):                          # |tune·65536| < 1 truncates to 0
        got, consumed, f = rc.resample(iq, tune, h, d)
        want, wcons = oracle.fir_filter(h, d, x)             # lo_fir_shift_coeffs(freq = 0) → lo_fir_filter
        assert f == 0 and consumed == wcons and len(got) == (CHAIN_SAMPLES - 33) // 3
        assert rc.same_values(got, want)
    # a scaled 16-bit format: the scaler behind the converter
    s16 = ((iq.astype(np.int16) - 128) * 256).astype(np.int16)
    got, _, _ = rc.resample(s16, 0.0, h, d, "cs16", 2.0 ** -8)
    assert bits_equal(got, rc.resample(iq, 0.0, h, d)[0])
    want, _ = oracle.fir_filter(h, d, oracle.scaler(2.0 ** -8, (s16[0::2].astype(np.float32) + 1j * s16[1::2].astype(np.float32)).astype(np.complex64)))
    assert rc.same_values(got, want)


def test_restatement_sizes():
    h = np.array([0.25, 0.5, 0.25, 0.125, -0.125], np.float32)
    iq = rc.capture_sps(16, 12, 7.5)[0]
    for n, want in ((0, 0), (4, 0), (5, 0), (6, 0), (7, 1), (8, 1), (9, 2)):
        out, consumed, _ = rc.resample(iq[: 2 * n], 0.01, h, 2)
        assert (len(out), consumed) == (want, 2 * want), n
    assert len(rc.resample(iq[:200], 0.0, h, 2, cap_out=3)[0]) == 3
    assert [rc.ifreq_of(t) for t in (0.01, -0.03, 0.1, -0.12, 0.49999, -1e-5)] == [655, -1966, 6553, -7864, 32767, 0]


def reference_chain_deviation(oracle, iq, x, h, d, tune):
    """max |restatement − rotator → fir_filter| over the RMS of the reference chain's output."""
    got, consumed, f = rc.resample(iq, tune, h, d)
    want, wcons = oracle.fir_filter(h, d, oracle.rotator(x, -f / 65536.0))
    assert f != 0 and consumed == wcons and len(got) == len(want)
    rms = float(np.sqrt(np.mean(np.abs(want.astype(np.complex128)) ** 2)))
    return float(np.max(np.abs(got.astype(np.complex128) - want.astype(np.complex128)))) / rms


def test_restatement_against_the_reference_chain(oracle, head12):
    iq, x, h, d = head12
    devs = [reference_chain_deviation(oracle, iq, x, h, d, t) for t in CHAIN_TUNES]
    print("restatement against rotator -> fir_filter, max |difference| / RMS: " + ", ".join(f"tune {t}: {v:.3e}" for t, v in zip(CHAIN_TUNES, devs)))
    assert max(devs) <= REF_CHAIN_BOUND, devs
    assert max(devs) > 1e-6                                   # … and the phase noise is there: the two are NOT the same arithmetic


@pytest.mark.parametrize("sps", [10, 12, 16, 33])
def test_two_stage_estimate(sps):
    d, order, fcut = rc.design(float(sps))
    from leansdr_amd import capi
    h = capi.lowpass(order, fcut)
    n = tc.N * tc.BLOCKS * d + order + 1 + d
    window8 = 1.0 / (2048.0 * sps / d) / 8
    worst_raw = worst_fine = hi_rms = 0.0
    lo_rms = 1e9
    for noise in (7.5, 18.0):
        for f in (0.0, 0.01, -0.03, 0.1, -0.12):
            iq = rc.shifted_sps(8, sps, noise, f, n)
            assert len(iq) == 2 * n
            e0 = tc.estimate(tc.to_complex(iq))
            assert e0["quality"] >= 100, (sps, noise, f, e0)
            out, _, ifreq = rc.resample(iq, e0["tune"], h, d)
            assert len(out) >= tc.N * tc.BLOCKS
            e1 = tc.estimate(out.astype(np.complex128))
            residual = (f - ifreq / 65536.0) * d
            worst_raw, worst_fine = max(worst_raw, abs(e0["tune"] - f)), max(worst_fine, abs(e1["tune"] - residual))
            assert e1["blocks"] == tc.BLOCKS and e1["quality"] >= 100, (sps, noise, f, e1)
            assert abs(e1["tune"] - residual) <= window8, (sps, noise, f, e1["tune"], residual)
            rms = float(np.sqrt(np.mean(np.abs(out.astype(np.complex128)) ** 2)))
            lo_rms, hi_rms = min(lo_rms, rms), max(hi_rms, rms)
            assert 65.0 <= rms <= 85.0, (sps, noise, f, rms)     # the level contract (RMS near 75; TS identical from 19 to 75, include/lsdr_hip.h)
    print(f"output RMS {lo_rms:.1f} ... {hi_rms:.1f} for a signal amplitude of 75")
    print(f"{sps} samples per symbol (D = {d}, N = {order + 1}): raw estimate within {worst_raw:.2e}, fine within {worst_fine:.2e} of the residual "
          f"(bound {window8:.2e})")
