"""lsdr_spectrum_batch without a GPU: the C ABI (header as C99, struct sizes, exported symbols), the row/block rule's restatement
(spectrum_common) against the oracle's cnr_fft and spectrum — what the device's row counts are then held to in test_gpu_spectrum_batch.py —
and a yardstick on physics from the oracle alone.

The yardstick: two synthetic DVB-S captures at 4 samples per symbol that differ in their noise only (7.5 and 18 on the cu8 scale), each
through oracle.cnr_fft(bandwidth 1/4, nfft 4096, a value every 8192 samples, centre 0), the twelve values of a capture averaged.  The noise
power differs by 20·log10(18/7.5) = 7.604 dB, and so should the two readings.  MEASURED here, seeds 11, 12, 13: 24.85 / 17.29, 24.92 / 17.38,
25.07 / 17.52 dB; gaps 7.559, 7.535, 7.552 dB — 0.05 dB below the ideal (the noise bands at ±3…4 bandwidth/4 still hold a little of the
signal's skirt, which weighs more against the lower floor), spread over the seeds 0.024 dB.  The test holds seed 11's gap within 0.15 dB of
7.604: the measured offset plus four times the spread.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import spectrum_common as sc
from conftest import ROOT

SYMBOLS = ("lsdr_spectrum_batch_create", "lsdr_spectrum_batch_destroy", "lsdr_spectrum_batch_max_rows", "lsdr_spectrum_batch_slab_rows",
           "lsdr_spectrum_batch_run_async", "lsdr_spectrum_batch_wait", "lsdr_spectrum_batch_cnr", "lsdr_spectrum_batch_rows_db",
           "lsdr_spectrum_batch_rows_dev")
GAP_DB = 20.0 * np.log10(18.0 / 7.5)
GAP_BOUND_DB = 0.15


def test_header_is_c99_and_the_structs_have_their_sizes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "lsdr_hip.h"\n'
                   "typedef char result_is_32_bytes[sizeof(lsdr_spectrum_result) == 32 ? 1 : -1];\n"
                   "typedef char cfg_is_72_bytes[sizeof(lsdr_spectrum_batch_cfg) == 72 ? 1 : -1];\n"
                   "int main(void) { lsdr_spectrum_batch_cfg c; lsdr_spectrum_result r; c.reserved[4] = 0; c.stages_per_pass = 0; r.pad[2] = 0; (void)c; (void)r;\n"
                   "  int (*w)(lsdr_spectrum_batch *, lsdr_spectrum_result *) = lsdr_spectrum_batch_wait; (void)w;\n"
                   "  int (*a)(lsdr_spectrum_batch *, const void *const *, const lsdr_capture_each *) = lsdr_spectrum_batch_run_async; (void)a;\n"
                   "  int (*q)(lsdr_spectrum_batch *, int, float *, size_t, size_t *) = lsdr_spectrum_batch_cnr; (void)q;\n"
                   "  q = lsdr_spectrum_batch_rows_db;\n"
                   "  const float *(*d)(const lsdr_spectrum_batch *, int) = lsdr_spectrum_batch_rows_dev; (void)d;\n"
                   "  return LSDR_ABI_VERSION == 2 ? LSDR_OK : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_spectrum_batch(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert ctypes.sizeof(capi.SpectrumResult) == 32 and ctypes.sizeof(capi.SpectrumBatchCfg) == 72
    assert capi.SpectrumBatchCfg.stages_per_pass.offset == 48 and capi.SpectrumBatchCfg.reserved.offset == 52
    assert capi.lib.lsdr_abi_version() == 2


def test_the_restated_rule_is_the_phase_counter():
    for nfft, decs in sc.DECIMATIONS.items():
        for dec in decs:
            for n in sc.lengths_around(nfft, dec):
                rows, consumed = sc.rows_of(n, nfft, dec)
                fetched = sc.fetched_blocks(n, nfft, dec)
                assert rows == len(fetched) and consumed == (n // nfft) * nfft, (nfft, dec, n)
                assert fetched == [sc.block_of_row(m, nfft, dec) for m in range(1, rows + 1)], (nfft, dec, n)


@pytest.mark.parametrize("nfft", [1024, 4096])
def test_row_counts_are_the_oracles(oracle, nfft):
    rng = np.random.default_rng(5)
    longest = max(max(sc.lengths_around(nfft, dec)) for dec in sc.DECIMATIONS[nfft])
    x = (rng.standard_normal(longest) + 1j * rng.standard_normal(longest)).astype(np.complex64)
    for dec in sc.DECIMATIONS[nfft]:
        for n in sc.lengths_around(nfft, dec):
            rows, _ = sc.rows_of(n, nfft, dec)
            assert len(oracle.cnr_fft(x[:n], 0.2, nfft, dec)) == rows, ("cnr_fft", nfft, dec, n)
            if nfft == 1024:
                assert len(oracle.spectrum(x[:n], dec, 0.5)) == rows, ("spectrum", dec, n)


def test_the_quieter_capture_reads_higher_by_the_noise_ratio(oracle):
    cnr = {noise: oracle.cnr_fft(oracle.cconverter_u8(sc.capture4(noise)), 0.25, 4096, 8192, 0.0, 1.0) for noise in (7.5, 18.0)}
    assert len(cnr[7.5]) == len(cnr[18.0]) == 12
    quiet, loud = float(np.mean(cnr[7.5])), float(np.mean(cnr[18.0]))
    print(f"CNR at noise 7.5: {quiet:.3f} dB, at noise 18: {loud:.3f} dB, gap {quiet - loud:.3f} dB (ideal {GAP_DB:.3f})")
    assert quiet > loud
    assert abs((quiet - loud) - GAP_DB) <= GAP_BOUND_DB
