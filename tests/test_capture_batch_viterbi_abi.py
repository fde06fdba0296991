"""The capture batch's Viterbi engine in the C ABI (lsdr_capture_batch_create_viterbi, _soft_dev, _viterbi_stats): exported, declared in
plain C, and mirrored by the ctypes binding; the existing configuration record and the ABI version are what they were.
No compute: runs without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["lsdr_capture_batch_create_viterbi", "lsdr_capture_batch_soft_dev", "lsdr_capture_batch_viterbi_stats"]
OLD_SYMBOLS = ["lsdr_capture_batch_create", "lsdr_capture_batch_destroy", "lsdr_capture_batch_run_async", "lsdr_capture_batch_wait",
               "lsdr_capture_batch_ts_download_async", "lsdr_capture_batch_ts_wait", "lsdr_capture_batch_ts_dev",
               "lsdr_capture_batch_words_dev", "lsdr_capture_batch_bytes_dev", "lsdr_capture_batch_mpeg_dev", "lsdr_capture_batch_bins",
               "lsdr_capture_batch_notched", "lsdr_capture_batch_tile_time"]


def header_symbols():
    src = open(os.path.join(ROOT, "include", "lsdr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(lsdr_capture_batch_[a-z0-9_]+)\s*\(", src))


def c_layout(tmp_path, ctype, fields):
    """sizeof and field offsets of `ctype` as a C99 compiler sees include/lsdr_hip.h."""
    src = tmp_path / f"{ctype}.c"
    prints = "".join(f'  printf(" %zu", offsetof({ctype}, {f}));\n' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lsdr_hip.h"\n'
                   f'int main(void) {{\n  printf("%zu", sizeof({ctype}));\n' + prints + '  return LSDR_OK;\n}\n')
    exe = tmp_path / ctype
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def ctypes_layout(struct):
    return [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f, _ in struct._fields_]


def test_header_declares_the_entry_points():
    assert header_symbols() == set(NEW_SYMBOLS) | set(OLD_SYMBOLS)


def test_library_exports_the_entry_points(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    missing = [s for s in NEW_SYMBOLS + OLD_SYMBOLS if not hasattr(lib, s)]
    assert not missing, f"liblsdr_hip.so lacks: {missing}"


def test_abi_version_unchanged(capi):
    assert capi.lib.lsdr_abi_version() == 2


def test_capture_batch_cfg_unchanged(capi, tmp_path):
    """The configuration record both constructors take is the one bench_c1.py and tests/test_abi.py mirror."""
    fields = [f for f, _ in capi.CaptureBatchCfg._fields_]
    assert fields == ["n_captures", "max_samples", "omega", "fec", "anf", "tile_len", "tile_warmup", "notch_k", "notch_decimation",
                      "unlocked_window", "aux_cus"]
    assert c_layout(tmp_path, "lsdr_capture_batch_cfg", fields) == ctypes_layout(capi.CaptureBatchCfg)


def test_capture_result_unchanged(capi, tmp_path):
    fields = [f for f, _ in capi.CaptureResult._fields_]
    assert c_layout(tmp_path, "lsdr_capture_result", fields) == ctypes_layout(capi.CaptureResult)


def test_viterbi_cfg_matches_c(capi, tmp_path):
    fields = [f for f, _ in capi.CaptureViterbiCfg._fields_]
    assert fields == ["resync_period", "reserved"]
    assert c_layout(tmp_path, "lsdr_capture_viterbi_cfg", fields) == ctypes_layout(capi.CaptureViterbiCfg)


def test_viterbi_stats_match_c(capi, tmp_path):
    fields = [f for f, _ in capi.CaptureViterbiStats._fields_]
    assert {"rounds", "batch_rounds", "switches", "stalls", "tiles", "repaired", "current_sync", "symbols", "bytes"} <= set(fields)
    assert c_layout(tmp_path, "lsdr_capture_viterbi_stats", fields) == ctypes_layout(capi.CaptureViterbiStats)


def test_binding_accepts_viterbi(capi):
    assert "viterbi" in inspect.signature(capi.CaptureBatch.__init__).parameters
    for name in ("soft", "soft_ptr", "viterbi_stats", "run_async", "wait", "decode", "stage_bytes"):
        assert callable(getattr(capi.CaptureBatch, name))
    argtypes = capi.lib.lsdr_capture_batch_create_viterbi.argtypes
    assert len(argtypes) == 4 and argtypes[2] == ctypes.POINTER(capi.CaptureViterbiCfg)
