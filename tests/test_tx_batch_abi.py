"""lsdr_tx_batch without a GPU: the C ABI — the header as C99 with the new section's types and signatures, the records' sizes (64 and 64
bytes), the exported symbols and the ctypes mirrors in capi — and the two host-only entry points: lsdr_tx_batch_plan against the lengths
of the oracle's blocks over a grid of stream lengths, resampling ratios, AGC and constellation / code-rate pairs, and
lsdr_db_to_amplitude against the oracle's.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("lsdr_tx_batch_create", "lsdr_tx_batch_destroy", "lsdr_tx_batch_run_async", "lsdr_tx_batch_wait", "lsdr_tx_batch_out_dev",
           "lsdr_tx_batch_results_dev", "lsdr_tx_batch_download_async", "lsdr_tx_batch_download_wait", "lsdr_tx_batch_stats",
           "lsdr_tx_batch_set_noise_margin", "lsdr_tx_batch_plan", "lsdr_db_to_amplitude")


def test_header_is_c99_and_the_records_have_64_bytes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "lsdr_hip.h"\n'
                   "typedef char each_is_64_bytes[sizeof(lsdr_tx_each) == 64 ? 1 : -1];\n"
                   "typedef char result_is_64_bytes[sizeof(lsdr_tx_result) == 64 ? 1 : -1];\n"
                   "typedef char cfg_is_80_bytes[sizeof(lsdr_tx_batch_cfg) == 80 ? 1 : -1];\n"
                   "int main(void) { lsdr_tx_batch_cfg c; lsdr_tx_each e; lsdr_tx_result r;\n"
                   "  c.n_streams = 1; c.max_packets = 1; c.cstln = LSDR_QPSK; c.interp = 2; c.decim = 1; c.rolloff = 0; c.rrc_rej = 0; c.agc = 0;\n"
                   "  c.out_format = LSDR_IN_CU8; c.reserved[7] = 0;\n"
                   "  e.n_packets = 0; e.fec = LSDR_FEC12; e.amp = e.scale = e.noise_stddev = 0; e.seeded = 0; e.reserved0 = 0; e.seed = 0;\n"
                   "  e.reserved[5] = 0;\n"
                   "  r.packets = r.bytes = r.symbols = r.samples = r.noise_state = 0; r.noise_rounds = 0; r.agc_estimated = 0; r.reserved[3] = 0;\n"
                   "  (void)c; (void)e; (void)r;\n"
                   "  int (*cr)(lsdr_ctx *, const lsdr_tx_batch_cfg *, lsdr_tx_batch **) = lsdr_tx_batch_create; (void)cr;\n"
                   "  void (*de)(lsdr_tx_batch *) = lsdr_tx_batch_destroy; (void)de;\n"
                   "  int (*ru)(lsdr_tx_batch *, const uint8_t *const *, const lsdr_tx_each *) = lsdr_tx_batch_run_async; (void)ru;\n"
                   "  int (*wa)(lsdr_tx_batch *, lsdr_tx_result *) = lsdr_tx_batch_wait; (void)wa;\n"
                   "  const void *(*ou)(const lsdr_tx_batch *, int) = lsdr_tx_batch_out_dev; (void)ou;\n"
                   "  const lsdr_tx_result *(*rd)(const lsdr_tx_batch *) = lsdr_tx_batch_results_dev; (void)rd;\n"
                   "  int (*da)(lsdr_tx_batch *, void *const *, size_t) = lsdr_tx_batch_download_async; (void)da;\n"
                   "  int (*dw)(lsdr_tx_batch *) = lsdr_tx_batch_download_wait; (void)dw;\n"
                   "  int (*st)(const lsdr_tx_batch *, unsigned *, unsigned long long *) = lsdr_tx_batch_stats; (void)st;\n"
                   "  int (*nm)(lsdr_tx_batch *, float) = lsdr_tx_batch_set_noise_margin; (void)nm;\n"
                   "  int (*pl)(const lsdr_tx_batch_cfg *, const lsdr_tx_each *, lsdr_tx_result *) = lsdr_tx_batch_plan; (void)pl;\n"
                   "  float (*db)(double) = lsdr_db_to_amplitude; (void)db;\n"
                   "  return LSDR_ABI_VERSION == 2 ? LSDR_OK : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_tx_batch(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert ctypes.sizeof(capi.TxEach) == 64 and ctypes.sizeof(capi.TxResult) == 64 and ctypes.sizeof(capi.TxBatchCfg) == 80
    assert capi.lib.lsdr_abi_version() == 2


# (constellation, code rate): QPSK at all five rates, 8PSK 2/3, 16APSK 3/4, BPSK 1/2
MODCODS = [(1, 0), (1, 1), (1, 3), (1, 4), (1, 5), (2, 1), (3, 3), (0, 0)]
BITS = {0: 1, 1: 2, 2: 3, 3: 4}


@pytest.mark.parametrize("cstln,rate", MODCODS)
def test_plan_equals_the_oracles_lengths(capi, oracle, cstln, rate):
    """The closed form against the blocks themselves: the interleaver's packets, the bytes the coder takes, its symbols, and the length of
    oracle.tx_chain, for every stream length around the interleaver's 12 packets, four resampling ratios, with and without AGC."""
    rng = np.random.default_rng(5)
    for n in (0, 1, 11, 12, 13, 24, 40):
        ts = rng.integers(0, 256, (n, 188), dtype=np.uint8)
        il = oracle.interleaver(oracle.rs_encoder(oracle.randomizer(ts))) if n else np.zeros(0, np.uint8)
        conv_rate = 2 if (rate == 1 and BITS[cstln] in (2, 6)) else rate
        sym, consumed = oracle.dvb_convol(il, conv_rate, BITS[cstln])
        for interp, decim in ((2, 1), (6, 5), (4, 1), (21, 5)):
            for agc in (False, True):
                want = len(oracle.tx_chain(ts, interp=interp, decim=decim, amp=3.0, agc=agc, cstln=cstln, rate=rate))
                tb = capi.TxBatch(None, 1, 40, interp=interp, decim=decim, cstln=cstln, agc=agc)
                got = tb.plan(dict(fec=rate, amp=3.0), n_packets=n)
                assert got == dict(packets=len(il) // 204, bytes=consumed, symbols=len(sym), samples=want), (n, interp, decim, agc)


def test_plan_refuses_what_dvb_convol_refuses(capi):
    for cstln, rate in ((2, 0), (3, 1), (1, 9), (1, -1)):                 # 8PSK 1/2, 16APSK 2/3 (3 coded bits into 4-bit symbols), no such rates
        tb = capi.TxBatch(None, 1, 40, cstln=cstln)
        e, r = tb.each(n_packets=20, fec=rate), capi.TxResult()
        assert capi.lib.lsdr_tx_batch_plan(ctypes.byref(tb.cfg), ctypes.byref(e), ctypes.byref(r)) == -2      # LSDR_E_ARG, as lsdr_convol_create
    for bad in (dict(interp=0), dict(decim=0), dict(out_format=2)):
        tb = capi.TxBatch(None, 1, 40, **bad)
        e, r = tb.each(n_packets=20), capi.TxResult()
        assert capi.lib.lsdr_tx_batch_plan(ctypes.byref(tb.cfg), ctypes.byref(e), ctypes.byref(r)) == -2


def test_db_to_amplitude_is_the_oracles(capi, oracle):
    oracle.lib.lo_db_to_amp.restype = ctypes.c_float
    oracle.lib.lo_db_to_amp.argtypes = [ctypes.c_double]
    for db in (-40.0, -12.5, -3.0, 0.0, 0.1, 8.5, 12.0, 15.0, 22.0, 37.5):
        assert np.float32(capi.db_to_amplitude(db)).tobytes() == np.float32(oracle.lib.lo_db_to_amp(db)).tobytes()
