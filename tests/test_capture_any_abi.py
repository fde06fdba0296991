"""The capture batch's other sample formats in the C ABI (lsdr_capture_any_create, lsdr_capture_any_run_async, lsdr_capture_input_cfg):
exported, declared in plain C99, mirrored by the ctypes binding, the ABI version what it was; and synth_dvbs.capture_s16, the true
16-bit capture the GPU tests decode.  No compute: runs without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["lsdr_capture_any_create", "lsdr_capture_any_run_async"]


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "lsdr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\b(lsdr_capture_any_[a-z0-9_]+)\s*\(", src)) == set(SYMBOLS)


def test_library_exports_the_entry_points(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, f"liblsdr_hip.so lacks: {missing}"


def test_abi_version_unchanged(capi):
    assert capi.lib.lsdr_abi_version() == 2


def test_input_cfg_matches_c_and_the_calls_are_plain_c99(capi, tmp_path):
    """sizeof / offsets of lsdr_capture_input_cfg as a C99 compiler sees the header, and the two prototypes used from C."""
    fields = [f for f, _ in capi.CaptureInputCfg._fields_]
    assert fields == ["in_format", "in_scale", "reserved"]
    src = tmp_path / "any.c"
    prints = "".join(f'  printf(" %zu", offsetof(lsdr_capture_input_cfg, {f}));\n' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lsdr_hip.h"\n'
                   'int (*p_create)(lsdr_ctx *, const lsdr_capture_batch_cfg *, const lsdr_capture_viterbi_cfg *, const lsdr_capture_input_cfg *,\n'
                   '                lsdr_capture_batch **) = lsdr_capture_any_create;\n'
                   'int (*p_run)(lsdr_capture_batch *, const void *const *, size_t) = lsdr_capture_any_run_async;\n'
                   'int main(void) {\n  lsdr_capture_input_cfg c = {LSDR_IN_CS16, 0.00390625f, {0, 0, 0, 0, 0, 0}};\n'
                   '  int formats[5] = {LSDR_IN_CF32, LSDR_IN_CU8, LSDR_IN_CS8, LSDR_IN_CU16, LSDR_IN_CS16};\n'
                   '  printf("%zu", sizeof(lsdr_capture_input_cfg));\n' + prints +
                   '  return (c.in_format == formats[4] && p_create && p_run) ? LSDR_OK : 1;\n}\n')
    obj = tmp_path / "any.o"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # (run it without the library: the layout alone)
    src2 = tmp_path / "layout.c"
    src2.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lsdr_hip.h"\n'
                    'int main(void) {\n  printf("%zu", sizeof(lsdr_capture_input_cfg));\n' + prints + '  return LSDR_OK;\n}\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(capi.CaptureInputCfg)] + [getattr(capi.CaptureInputCfg, f).offset for f in fields]
    assert got == want == [32, 0, 4, 8]


def test_binding_accepts_the_formats(capi):
    params = inspect.signature(capi.CaptureBatch.__init__).parameters
    assert "in_format" in params and "in_scale" in params
    assert params["in_format"].default == capi.IN_CU8 and params["in_scale"].default == 0.0
    assert (capi.IN_CF32, capi.IN_CU8, capi.IN_CS8, capi.IN_CU16, capi.IN_CS16) == (0, 1, 2, 3, 4)
    argtypes = capi.lib.lsdr_capture_any_create.argtypes
    assert len(argtypes) == 5 and argtypes[3] == ctypes.POINTER(capi.CaptureInputCfg)
    assert len(capi.lib.lsdr_capture_any_run_async.argtypes) == 3


def test_capture_s16_is_capture_u8_quantised_finer():
    """The same analogue signal as capture_u8 with the same seed, 256 times finer, no offset.  Rounding it to 8 bits again gives
    capture_u8 wherever neither clips — except at the ties of the second rounding (s16 ≡ 128 mod 256, i.e. s16 / 256 exactly half way
    between two u8 values: the first rounding has moved the sample onto the tie, 0.4 % of the values), where it is within one step."""
    from leansdr_amd import synth_dvbs
    s, ts = synth_dvbs.capture_s16(600, seed=11)
    u, ts8 = synth_dvbs.capture_u8(600, seed=11)
    assert s.dtype == np.int16 and len(s) == 2 * 1175063 and len(u) == len(s)
    assert np.array_equal(np.asarray(ts), np.asarray(ts8))
    assert np.mean(s % 256 != 0) > 0.99
    r = np.rint(s.astype(np.float64) / 256.0 + 128.0)
    inside = (r > 0) & (r < 255) & (u > 0) & (u < 255) & (np.abs(s.astype(np.int32)) < 32767)
    tie = (s.astype(np.int32) % 256) == 128
    assert inside.mean() > 0.99
    assert np.array_equal(r[inside & ~tie], u[inside & ~tie].astype(np.float64))
    assert np.abs(r[inside & tie] - u[inside & tie]).max() <= 1 and tie.mean() < 0.006
    # the other arguments are capture_u8's; lsb is the step
    s2, _ = synth_dvbs.capture_s16(16, seed=3, lsb=64.0)
    s3, _ = synth_dvbs.capture_s16(16, seed=3, lsb=256.0)
    assert np.abs(s2.astype(np.float64) * 4 - s3).max() <= 2.5
