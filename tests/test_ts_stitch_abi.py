"""lsdr_ts_stitch without a GPU: the header's section as C99, the record sizes, the exported symbols, the ABI version."""
import ctypes
import os
import subprocess

from conftest import ROOT

SYMBOLS = ("lsdr_ts_stitch_create", "lsdr_ts_stitch_destroy", "lsdr_ts_stitch_run_async", "lsdr_ts_stitch_wait", "lsdr_ts_stitch_out_dev",
           "lsdr_ts_stitch_download_async", "lsdr_ts_stitch_download_wait")


def test_header_is_c99_and_the_records_have_24_bytes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "lsdr_hip.h"\n'
                   "typedef char join_is_24_bytes[sizeof(lsdr_ts_join) == 24 ? 1 : -1];\n"
                   "typedef char keep_is_24_bytes[sizeof(lsdr_ts_keep) == 24 ? 1 : -1];\n"
                   "typedef char cfg_is_56_bytes[sizeof(lsdr_ts_stitch_cfg) == 56 ? 1 : -1];\n"
                   "int main(void) { lsdr_ts_stitch_cfg c; lsdr_ts_join j; lsdr_ts_keep k; c.window = 0; c.min_run = 0; c.reserved[7] = 0;\n"
                   "  j.joined = 0; j.run = 0; j.end = 0; j.next_start = 0; k.start = 0; k.end = 0; k.out_offset = 0; (void)c; (void)j; (void)k;\n"
                   "  int (*r)(lsdr_ts_stitch *, const uint8_t *const *, const uint64_t *) = lsdr_ts_stitch_run_async; (void)r;\n"
                   "  int (*w)(lsdr_ts_stitch *, lsdr_ts_join *, lsdr_ts_keep *) = lsdr_ts_stitch_wait; (void)w;\n"
                   "  const uint8_t *(*o)(const lsdr_ts_stitch *) = lsdr_ts_stitch_out_dev; (void)o;\n"
                   "  int (*d)(lsdr_ts_stitch *, uint8_t *, size_t) = lsdr_ts_stitch_download_async; (void)d;\n"
                   "  return LSDR_ABI_VERSION == 2 ? LSDR_OK : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_stitch(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert ctypes.sizeof(capi.TsJoin) == 24 and ctypes.sizeof(capi.TsKeep) == 24 and ctypes.sizeof(capi.TsStitchCfg) == 56
    assert capi.lib.lsdr_abi_version() == 2
