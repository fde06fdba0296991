"""Re-acquisition in the C ABI (lsdr_capture_relock_set, lsdr_capture_relock_get, lsdr_capture_relock_stats): exported, declared in plain
C, the record 40 bytes and mirrored field for field by the ctypes binding; lsdr_capture_result and the ABI version are what they were.
No compute: runs without a GPU."""
import ctypes
import inspect
import os
import re

from test_capture_batch_viterbi_abi import c_layout, ctypes_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["lsdr_capture_relock_set", "lsdr_capture_relock_get"]
FIELDS = ["locks", "drops", "passes", "exhausted", "first_drop_byte", "last_lock_byte", "next_sync_behind_first_lock", "pad"]


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "lsdr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\b(lsdr_capture_relock_[a-z0-9_]+)\s*\(", src)) == set(SYMBOLS)
    assert re.search(r"int\s+lsdr_capture_relock_set\s*\(\s*lsdr_capture_batch\s*\*\s*\w+\s*,\s*unsigned\s+\w+\s*\)", src)
    assert re.search(r"int\s+lsdr_capture_relock_get\s*\(\s*const\s+lsdr_capture_batch\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*lsdr_capture_relock_stats\s*\*\s*\w+\s*\)", src)


def test_library_exports_the_entry_points(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    assert capi.lib.lsdr_abi_version() == 2


def test_stats_record_is_40_bytes_and_mirrored(capi, tmp_path):
    assert [f for f, _ in capi.CaptureRelockStats._fields_] == FIELDS
    c = c_layout(tmp_path, "lsdr_capture_relock_stats", FIELDS)
    assert c[0] == 40 and c == ctypes_layout(capi.CaptureRelockStats)
    assert c[1:] == [0, 4, 8, 12, 16, 24, 32, 36]


def test_capture_result_is_what_it_was(capi, tmp_path):
    fields = [f for f, _ in capi.CaptureResult._fields_]
    assert c_layout(tmp_path, "lsdr_capture_result", fields)[0] == ctypes.sizeof(capi.CaptureResult) == 96


def test_binding_takes_relock(capi):
    for cls in (capi.CaptureBatch, capi.ResampledDecoder, capi.WidebandDecoder):
        p = inspect.signature(cls.__init__).parameters
        assert "relock" in p and p["relock"].default == 0, cls
    assert callable(capi.CaptureBatch.relock_stats) and callable(capi.CaptureBatch.set_relock)
    assert capi.lib.lsdr_capture_relock_set.argtypes[1] == ctypes.c_uint
    assert capi.lib.lsdr_capture_relock_get.argtypes[2] == ctypes.POINTER(capi.CaptureRelockStats)
