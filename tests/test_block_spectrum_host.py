"""leansdr_amd/csrc/block_spectrum.h without a GPU: the arithmetic under lsdr_tune_est and lsdr_rate_est, as a stand-alone host program
(tests/block_spectrum_host.hip, its own main) built with the library's float rule (-ffp-contract=off) under AddressSanitizer and UBSan.

The program holds: the six radix-4 stages and the digit reversal on one seeded block (a tone between two bins plus noise) against a float64
DFT, powers within 1e-4 of the peak power (the bound of test_gpu_tune_est.py; measured 1.9e-7); the reversal an involution on 0 … 4095;
te_peak_record and re_peak_record on hand-set peaks (l = r, c = 0, bin 0 and the wrap at N/2 for the tune, bin N/2 for the rate, both
candidates, one, neither) equal to the formulas of tune_common's and rate_common's docstrings rounded to float.  It makes no GPU call.
"""
import os
import subprocess

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_block_spectrum_on_the_host(tmp_path):
    exe = tmp_path / "block_spectrum_host"
    build = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                            "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "leansdr_amd", "csrc"), os.path.join(ROOT, "tests", "block_spectrum_host.hip"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    checks, failed = (int(w) for w in run.stdout.splitlines()[-1].split() if w.isdigit())
    assert failed == 0 and checks > 70, run.stdout[-500:]
