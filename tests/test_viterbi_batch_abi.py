"""The batch Viterbi decoder's C ABI (lsdr_viterbi_batch_*): exported, declared in plain C, and mirrored by the ctypes binding.
No compute: runs without a GPU."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCH_SYMBOLS = ["lsdr_viterbi_batch_create", "lsdr_viterbi_batch_destroy", "lsdr_viterbi_batch_set_resync_period",
                 "lsdr_viterbi_batch_reset", "lsdr_viterbi_batch_run_async", "lsdr_viterbi_batch_wait",
                 "lsdr_viterbi_batch_results_dev", "lsdr_viterbi_batch_stats"]


def header_symbols():
    src = open(os.path.join(ROOT, "include", "lsdr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(lsdr_viterbi_batch_[a-z0-9_]+)\s*\(", src))


def test_header_declares_the_batch_entry_points():
    assert header_symbols() == set(BATCH_SYMBOLS)


def test_library_exports_the_batch_entry_points(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    missing = [s for s in BATCH_SYMBOLS if not hasattr(lib, s)]
    assert not missing, f"liblsdr_hip.so lacks: {missing}"


def test_abi_version_unchanged(capi):
    assert capi.lib.lsdr_abi_version() == 2


def test_binding_exists(capi):
    for name in ("run_async_dev", "wait", "reset", "stats", "close", "run_streams"):
        assert callable(getattr(capi.ViterbiBatch, name))


def test_result_record_size_matches_c(capi, tmp_path):
    """include/lsdr_hip.h with the new declarations compiles as C99, and sizeof / field offsets of lsdr_viterbi_batch_result in C are
    the ctypes structure's."""
    src = tmp_path / "s.c"
    fields = [f for f, _ in capi.ViterbiBatchResult._fields_]
    prints = "".join(f'  printf(" %zu", offsetof(lsdr_viterbi_batch_result, {f}));\n' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lsdr_hip.h"\n'
                   'int main(void) {\n  printf("%zu", sizeof(lsdr_viterbi_batch_result));\n' + prints + '  return LSDR_OK;\n}\n')
    exe = tmp_path / "s"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(capi.ViterbiBatchResult)] + [getattr(capi.ViterbiBatchResult, f).offset for f in fields]
    assert got == want, (got, want)
