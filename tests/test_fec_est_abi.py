"""lsdr_fec_est without a GPU: the C ABI — the header as C99 with the new section's types and signatures, the record's size, the exported
symbols and the ctypes mirrors in capi.  The record of include/lsdr_hip.h (int32 + 5 × uint32, uint64, 2 × float, 5 × 24-byte scores)
has 160 bytes under the C ABI's alignment rules.
"""
import ctypes
import os
import subprocess

from conftest import ROOT

SYMBOLS = ("lsdr_fec_est_create", "lsdr_fec_est_destroy", "lsdr_fec_est_run_async", "lsdr_fec_est_wait", "lsdr_fec_est_polys",
           "lsdr_fec_est_tile")


def test_header_is_c99_and_the_record_has_160_bytes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "lsdr_hip.h"\n'
                   "typedef char record_is_160_bytes[sizeof(lsdr_fec_estimate) == 160 ? 1 : -1];\n"
                   "typedef char score_is_24_bytes[sizeof(lsdr_fec_est_score) == 24 ? 1 : -1];\n"
                   "typedef char cfg_is_40_bytes[sizeof(lsdr_fec_est_cfg) == 40 ? 1 : -1];\n"
                   "typedef char formats[LSDR_HSYM_PACKED2 == 0 && LSDR_HSYM_U8 == 1 && LSDR_HSYM_SOFT == 2 ? 1 : -1];\n"
                   "int main(void) { lsdr_fec_est_cfg c; lsdr_fec_estimate e; c.reserved[4] = 0; c.max_symbols = 1; c.in_format = LSDR_HSYM_SOFT;\n"
                   "  e.fec = -1; e.locked = e.ambiguous = e.sync = e.skip = e.pad = 0; e.symbols = 0; e.error_rate = e.runner_up = 0;\n"
                   "  e.score[4].errors = e.score[4].checks = 0; e.score[4].sync = e.score[4].skip = 0; (void)c; (void)e;\n"
                   "  int (*cr)(lsdr_ctx *, const lsdr_fec_est_cfg *, lsdr_fec_est **) = lsdr_fec_est_create; (void)cr;\n"
                   "  void (*de)(lsdr_fec_est *) = lsdr_fec_est_destroy; (void)de;\n"
                   "  int (*ru)(lsdr_fec_est *, const void *const *, const uint64_t *, const uint64_t *) = lsdr_fec_est_run_async; (void)ru;\n"
                   "  int (*wa)(lsdr_fec_est *, lsdr_fec_estimate *) = lsdr_fec_est_wait; (void)wa;\n"
                   "  int (*po)(int, uint64_t *, uint64_t *, int *) = lsdr_fec_est_polys; (void)po;\n"
                   "  unsigned (*ti)(const lsdr_fec_est *) = lsdr_fec_est_tile; (void)ti;\n"
                   "  return LSDR_ABI_VERSION == 2 ? LSDR_OK : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_estimator(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert ctypes.sizeof(capi.FecEstimate) == 160 and ctypes.sizeof(capi.FecEstScore) == 24 and ctypes.sizeof(capi.FecEstCfg) == 40
    assert (capi.HSYM_PACKED2, capi.HSYM_U8, capi.HSYM_SOFT) == (0, 1, 2)
    assert capi.lib.lsdr_abi_version() == 2
