"""The capture batch's signal reports in the C ABI (lsdr_capture_reports_set, lsdr_capture_reports_get, lsdr_capture_report): exported,
declared in plain C99, mirrored by the ctypes binding, the ABI version what it was.  No compute: runs without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["lsdr_capture_reports_set", "lsdr_capture_reports_get"]


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "lsdr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\b(lsdr_capture_reports_[a-z0-9_]+)\s*\(", src)) == set(SYMBOLS)


def test_library_exports_the_entry_points(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, f"liblsdr_hip.so lacks: {missing}"


def test_abi_version_unchanged(capi):
    assert capi.lib.lsdr_abi_version() == 2


def test_report_record_matches_c_and_the_calls_are_plain_c99(capi, tmp_path):
    """sizeof / offsets of lsdr_capture_report as a C99 compiler sees the header, and the two prototypes used from C."""
    fields = [f for f, _ in capi.CaptureReport._fields_]
    assert fields == ["freq", "ss", "mer", "pad"]
    src = tmp_path / "reports.c"
    prints = "".join(f'  printf(" %zu", offsetof(lsdr_capture_report, {f}));\n' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lsdr_hip.h"\n'
                   'int (*p_set)(lsdr_capture_batch *, uint64_t) = lsdr_capture_reports_set;\n'
                   'int (*p_get)(lsdr_capture_batch *, int, lsdr_capture_report *, size_t, size_t *, lsdr_capture_report *) = lsdr_capture_reports_get;\n'
                   'int main(void) {\n  lsdr_capture_report r = {0.0f, 75.0f, 20.0f, 0u};\n'
                   '  return (r.ss == 75.0f && p_set && p_get) ? LSDR_OK : 1;\n}\n')
    obj = tmp_path / "reports.o"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # (run it without the library: the layout alone)
    src2 = tmp_path / "layout.c"
    src2.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lsdr_hip.h"\n'
                    'int main(void) {\n  printf("%zu", sizeof(lsdr_capture_report));\n' + prints + '  return LSDR_OK;\n}\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(capi.CaptureReport)] + [getattr(capi.CaptureReport, f).offset for f in fields]
    assert got == want == [16, 0, 4, 8, 12]


def test_capture_batch_cfg_keeps_its_layout(capi, tmp_path):
    fields = [f for f, _ in capi.CaptureBatchCfg._fields_]
    assert fields == ["n_captures", "max_samples", "omega", "fec", "anf", "tile_len", "tile_warmup", "notch_k", "notch_decimation",
                      "unlocked_window", "aux_cus"]


def test_binding_accepts_reports(capi):
    params = inspect.signature(capi.CaptureBatch.__init__).parameters
    assert "reports" in params and params["reports"].default == 0
    assert callable(capi.CaptureBatch.reports) and callable(capi.CaptureBatch.set_reports)
    assert capi.lib.lsdr_capture_reports_set.argtypes[1] == ctypes.c_uint64
    argtypes = capi.lib.lsdr_capture_reports_get.argtypes
    assert len(argtypes) == 6 and argtypes[2] == ctypes.POINTER(capi.CaptureReport) and argtypes[5] == ctypes.POINTER(capi.CaptureReport)


def test_freq_bounds_are_stated(capi):
    """The two bounds on FREQ exist, and neither passes a report of constant 0: each is below half the carrier offset the GPU test of
    its engine applies (tests/test_gpu_capture_batch_reports.py: 1e-4 and 2e-4 cycles per sample)."""
    from leansdr_amd import tolerance
    assert 0 < tolerance.TOL["freq_atol"] < 0.5 * 1e-4
    assert 0 < tolerance.LOW_SNR["freq_atol"] < 0.5 * 2e-4
