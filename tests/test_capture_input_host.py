"""leansdr_amd/csrc/capture_input.h without a GPU: the one header that knows the raw captures' sample formats, as a stand-alone host program
(tests/capture_input_host.hip, its own main) built with the library's float rule (-ffp-contract=off) under AddressSanitizer and UBSan.

The program holds, bit for bit and for in_scale 1 and 1/128, in_unpack = in_load = in_piece = float(item − Z)·in_scale on the extreme items
of all five formats; lsdr_in_describe's table (kind, item size 2/2/4/4/8, the flip for cu16 alone, in_scale 0 → 1) and its refusals (format −1
and 5; scale −1, NaN, ±inf); and lsdr_in_check_each's refusals with the words the owners' callers match.  It makes no GPU call.
"""
import os
import subprocess

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_capture_input_on_the_host(tmp_path):
    exe = tmp_path / "capture_input_host"
    build = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                            "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "leansdr_amd", "csrc"), os.path.join(ROOT, "tests", "capture_input_host.hip"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    checks, failed = (int(w) for w in run.stdout.split() if w.isdigit())
    assert failed == 0 and checks > 700, run.stdout[-500:]
