"""lsdr_hs_batch in the C ABI: declared in plain C, exported by the library and mirrored by the ctypes binding; purely additive — the ABI
version and lsdr_capture_result are what they were.  No compute: runs without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["lsdr_hs_batch_create", "lsdr_hs_batch_destroy", "lsdr_hs_batch_run_async", "lsdr_hs_batch_wait", "lsdr_hs_batch_ts_download_async",
           "lsdr_hs_batch_ts_wait", "lsdr_hs_batch_ts_dev", "lsdr_hs_batch_symbols_dev", "lsdr_hs_batch_bytes_dev", "lsdr_hs_batch_mpeg_dev"]


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
    src = open(os.path.join(ROOT, "include", "lsdr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\b(lsdr_hs_batch_[a-z0-9_]+)\s*\(", src)) == set(SYMBOLS)


def test_library_exports_the_entry_points(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, f"liblsdr_hip.so lacks: {missing}"


def test_abi_version_unchanged(capi):
    assert capi.lib.lsdr_abi_version() == 2


def test_hs_batch_cfg_matches_c(capi, tmp_path):
    fields = [f for f, _ in capi.HsBatchCfg._fields_]
    assert fields == ["n_captures", "max_samples", "omega", "freq", "allow_drift", "fastlock", "tile_len", "tile_warmup", "reserved"]
    assert capi.HsBatchCfg.reserved.size == 8 * ctypes.sizeof(ctypes.c_int)
    assert c_layout(tmp_path, "lsdr_hs_batch_cfg", fields) == ctypes_layout(capi.HsBatchCfg)


def test_capture_result_unchanged(capi, tmp_path):
    fields = [f for f, _ in capi.CaptureResult._fields_]
    assert fields == ["ts_packets", "rs_packets", "rs_bit_errors", "symbols", "samples", "bytes_deconv", "bytes_mpeg", "first_lock_byte",
                      "next_sync_calls", "locked", "alignment", "bitphase", "tiles", "seam_dup", "seam_miss", "seam_bad"]
    layout = c_layout(tmp_path, "lsdr_capture_result", fields)
    assert layout == ctypes_layout(capi.CaptureResult)
    assert layout[0] == 96 and layout[1:] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76, 80, 84, 88, 92]


def test_binding(capi):
    params = list(inspect.signature(capi.HsBatch.__init__).parameters)
    assert params == ["self", "ctx", "n_captures", "max_samples", "omega", "freq", "allow_drift", "fastlock", "tile_len", "tile_warmup"]
    for name in ("run_async", "wait", "decode", "ts_download_async", "ts_wait", "symbols", "symbols_ptr", "stage_bytes", "close"):
        assert callable(getattr(capi.HsBatch, name)), name
    argtypes = capi.lib.lsdr_hs_batch_create.argtypes
    assert len(argtypes) == 3 and argtypes[1] == ctypes.POINTER(capi.HsBatchCfg)
    assert capi.lib.lsdr_hs_batch_symbols_dev.restype == capi.vp
