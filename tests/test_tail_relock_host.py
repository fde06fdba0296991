"""leansdr_amd/csrc/tail_relock.h without a GPU: the window and rewind arithmetic of the FEC tail's re-acquisition as a stand-alone host
program (tests/tail_relock_host.hip, its own main) under AddressSanitizer and UBSan.

The program holds, for the five code rates and the windows 2048 and 8192, against a brute-force loop of single windows (deconvol_sync::run's
sizes bit by bit, mpeg_sync's locked path taking whole packets with a byte of look-ahead): the split of a locked stretch into whole
windows and a windowed end — one call over the whole windows writes their bytes and leaves their counters, with the symbols or the byte
buffer ending first — and the rewind after a drop in the first, a middle and the last packet of a window and on a window boundary: the
number of windows that stand and the deconvolver's counters at that boundary.  It makes no GPU call.
"""
import os
import subprocess

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_tail_relock_arithmetic_on_the_host(tmp_path):
    exe = tmp_path / "tail_relock_host"
    build = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                            "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "leansdr_amd", "csrc"), os.path.join(ROOT, "tests", "tail_relock_host.hip"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    checks, failed = (int(w) for w in run.stdout.splitlines()[-1].split() if w.isdigit())
    assert failed == 0 and checks > 10000, run.stdout[-500:]
