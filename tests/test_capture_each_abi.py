"""Per-capture lengths and tunes in the C ABI (lsdr_capture_each, lsdr_capture_each_run_async, lsdr_hs_each_run_async): exported, declared in
plain C99, mirrored by the ctypes binding, the ABI version what it was.  No compute: runs without a GPU."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["lsdr_capture_each_run_async", "lsdr_hs_each_run_async"]


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "lsdr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\b(lsdr_(?:capture|hs)_each_[a-z0-9_]+)\s*\(", src)) == set(SYMBOLS)


def test_library_exports_the_entry_points(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, f"liblsdr_hip.so lacks: {missing}"


def test_abi_version_unchanged(capi):
    assert capi.lib.lsdr_abi_version() == 2


def test_each_matches_c_and_the_calls_are_plain_c99(capi, tmp_path):
    """sizeof / offsets of lsdr_capture_each as a C99 compiler sees the header, and the two prototypes used from C."""
    fields = [f for f, _ in capi.CaptureEach._fields_]
    assert fields == ["n_samples", "tune", "reserved"]
    prints = "".join(f'  printf(" %zu", offsetof(lsdr_capture_each, {f}));\n' for f in fields)
    src = tmp_path / "each.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lsdr_hip.h"\n'
                   'int (*p_cap)(lsdr_capture_batch *, const void *const *, const lsdr_capture_each *) = lsdr_capture_each_run_async;\n'
                   'int (*p_hs)(lsdr_hs_batch *, const lsdr_cu8 *const *, const lsdr_capture_each *) = lsdr_hs_each_run_async;\n'
                   'int main(void) {\n  lsdr_capture_each e = {1000, 0.001f, {0, 0, 0, 0, 0}};\n'
                   '  return (e.n_samples == 1000 && p_cap && p_hs) ? LSDR_OK : 1;\n}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "each.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # (run it without the library: the layout alone)
    src2 = tmp_path / "layout.c"
    src2.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lsdr_hip.h"\n'
                    'int main(void) {\n  printf("%zu", sizeof(lsdr_capture_each));\n' + prints + '  return LSDR_OK;\n}\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(capi.CaptureEach)] + [getattr(capi.CaptureEach, f).offset for f in fields]
    assert got == want == [32, 0, 8, 12]


def test_binding_has_the_each_calls(capi):
    for cls in (capi.CaptureBatch, capi.HsBatch):
        assert callable(getattr(cls, "run_each_async")) and callable(getattr(cls, "decode_each"))
    assert capi.lib.lsdr_capture_each_run_async.argtypes[2] == ctypes.POINTER(capi.CaptureEach)
    assert capi.lib.lsdr_hs_each_run_async.argtypes[2] == ctypes.POINTER(capi.CaptureEach)
    assert capi.lib.lsdr_capture_each_run_async is not capi.lib.lsdr_hs_each_run_async
