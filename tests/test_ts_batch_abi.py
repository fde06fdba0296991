"""lsdr_ts_batch without a GPU: the C ABI — the header as C99 with the new section's types and signatures, the records' sizes (fourteen
uint64 and four 32-bit fields: 128 bytes; ten uint32 and two uint64: 56 bytes), the exported symbols and the ctypes mirrors in capi.
"""
import ctypes
import os
import subprocess

from conftest import ROOT

SYMBOLS = ("lsdr_ts_batch_create", "lsdr_ts_batch_destroy", "lsdr_ts_batch_run_async", "lsdr_ts_batch_wait", "lsdr_ts_batch_pids",
           "lsdr_ts_batch_out_dev", "lsdr_ts_batch_index_dev", "lsdr_ts_batch_download_async", "lsdr_ts_batch_download_wait",
           "lsdr_ts_batch_tile")


def test_header_is_c99_and_the_records_have_128_and_56_bytes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "lsdr_hip.h"\n'
                   "typedef char summary_is_128_bytes[sizeof(lsdr_ts_summary) == 128 ? 1 : -1];\n"
                   "typedef char pid_is_56_bytes[sizeof(lsdr_ts_pid) == 56 ? 1 : -1];\n"
                   "typedef char cfg_is_56_bytes[sizeof(lsdr_ts_batch_cfg) == 56 ? 1 : -1];\n"
                   "typedef char rule_is_32_bytes[sizeof(lsdr_ts_rule) == 32 ? 1 : -1];\n"
                   "typedef char drops[LSDR_TS_DROP_NULL == 1 && LSDR_TS_DROP_TEI == 2 && LSDR_TS_DROP_SYNC == 4 ? 1 : -1];\n"
                   "int main(void) { lsdr_ts_batch_cfg c; lsdr_ts_rule r; lsdr_ts_summary s; lsdr_ts_pid p;\n"
                   "  c.n_streams = 1; c.max_packets = 1; c.max_pids = 0; c.reserved[7] = 0; r.keep_pids = 0; r.drop = LSDR_TS_DROP_NULL;\n"
                   "  r.want_index = 0; r.reserved[3] = 0;\n"
                   "  s.packets = s.sync_errors = s.tei = s.null_packets = s.valid = s.cc_errors = s.cc_repeats = s.cc_missing = 0;\n"
                   "  s.discontinuities = s.kept = s.pcr_first = s.pcr_last = s.pcr_first_packet = s.pcr_last_packet = 0;\n"
                   "  s.pids_seen = s.pids_listed = s.pcr_count = 0; s.pcr_pid = -1;\n"
                   "  p.pid = p.packets = p.pusi = p.scrambled = p.cc_errors = p.cc_repeats = p.cc_missing = p.discontinuities = 0;\n"
                   "  p.pcr_count = p.pad = 0; p.first_packet = p.last_packet = 0; (void)c; (void)r; (void)s; (void)p;\n"
                   "  int (*cr)(lsdr_ctx *, const lsdr_ts_batch_cfg *, lsdr_ts_batch **) = lsdr_ts_batch_create; (void)cr;\n"
                   "  void (*de)(lsdr_ts_batch *) = lsdr_ts_batch_destroy; (void)de;\n"
                   "  int (*ru)(lsdr_ts_batch *, const uint8_t *const *, const uint64_t *, const lsdr_ts_rule *) = lsdr_ts_batch_run_async; (void)ru;\n"
                   "  int (*wa)(lsdr_ts_batch *, lsdr_ts_summary *) = lsdr_ts_batch_wait; (void)wa;\n"
                   "  int (*pi)(lsdr_ts_batch *, int, lsdr_ts_pid *, unsigned, unsigned *) = lsdr_ts_batch_pids; (void)pi;\n"
                   "  const uint8_t *(*ou)(const lsdr_ts_batch *, int) = lsdr_ts_batch_out_dev; (void)ou;\n"
                   "  const uint32_t *(*ix)(const lsdr_ts_batch *, int) = lsdr_ts_batch_index_dev; (void)ix;\n"
                   "  int (*da)(lsdr_ts_batch *, uint8_t *const *, size_t) = lsdr_ts_batch_download_async; (void)da;\n"
                   "  int (*dw)(lsdr_ts_batch *) = lsdr_ts_batch_download_wait; (void)dw;\n"
                   "  unsigned (*ti)(const lsdr_ts_batch *) = lsdr_ts_batch_tile; (void)ti;\n"
                   "  return LSDR_ABI_VERSION == 2 ? LSDR_OK : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_ts_batch(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert ctypes.sizeof(capi.TsSummary) == 128 and ctypes.sizeof(capi.TsPid) == 56
    assert ctypes.sizeof(capi.TsBatchCfg) == 56 and ctypes.sizeof(capi.TsRule) == 32
    assert (capi.TS_DROP_NULL, capi.TS_DROP_TEI, capi.TS_DROP_SYNC) == (1, 2, 4)
    assert capi.lib.lsdr_abi_version() == 2


def test_bitrate_from_a_summary(capi):
    s = dict(pcr_count=2, pcr_first=1000, pcr_last=1000 + 4000 * 50, pcr_first_packet=10, pcr_last_packet=60)
    assert capi.ts_bitrate(s) == 188 * 8 * 27e6 / 4000
    wrapped = dict(s, pcr_first=(1 << 33) * 300 - 4000 * 20, pcr_last=4000 * 30)          # the 33-bit base wrapped in between
    assert capi.ts_bitrate(wrapped) == 188 * 8 * 27e6 / 4000
    assert capi.ts_bitrate(dict(s, pcr_count=1)) is None and capi.ts_bitrate(dict(s, pcr_last=1000)) is None
