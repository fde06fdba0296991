"""leansdr_amd/csrc/carrier_scan_device.h without a GPU: the plain C++ of lsdr_carrier_scan as a stand-alone host program
(tests/carrier_scan_host.hip, its own main) built with the library's float rule (-ffp-contract=off) under AddressSanitizer and UBSan.

The program holds: the runs as the kernel finds them (its per-thread phases for the 256 thread indices, a loop standing for the prefix sums)
equal to a serial walk over the bins from −1/2 upward — on hand-set S with a run across the N−1 → 0 seam, a run across ±1/2 (listed
last), single bins, all above (saturated), none above, min_bins, max_carriers, 2048 runs, a NaN, and on 40 seeded random patterns;
cs_run_record on hand-set runs (plain, at the seam, across ±1/2, weak, an edge at the run's first bin, n = 1, 2, 3) equal to the formulas
of scan_common's docstring rounded to float; cs_smooth equal to its definition.  It makes no GPU call.
"""
import os
import subprocess

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_carrier_scan_on_the_host(tmp_path):
    exe = tmp_path / "carrier_scan_host"
    build = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                            "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "leansdr_amd", "csrc"), os.path.join(ROOT, "tests", "carrier_scan_host.hip"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    checks, failed = (int(w) for w in run.stdout.splitlines()[-1].split() if w.isdigit())
    assert failed == 0 and checks > 150, run.stdout[-500:]
