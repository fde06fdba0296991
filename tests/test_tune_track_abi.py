"""lsdr_tune_track and lsdr_derotate_batch without a GPU: the C ABI (header as C99, struct sizes and fields, exported symbols) and the
signatures of their Python classes (leansdr_amd/capi.py)."""
import ctypes
import inspect
import os
import subprocess

from conftest import ROOT

SYMBOLS = ("lsdr_tune_track_create", "lsdr_tune_track_destroy", "lsdr_tune_track_max_frames", "lsdr_tune_track_run_async", "lsdr_tune_track_wait",
           "lsdr_derotate_batch_create", "lsdr_derotate_batch_destroy", "lsdr_derotate_batch_run_async", "lsdr_derotate_batch_wait")


def test_header_is_c99_and_the_structs_have_their_sizes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "lsdr_hip.h"\n'
                   "typedef char cfg_is_48_bytes[sizeof(lsdr_tune_track_cfg) == 48 ? 1 : -1];\n"
                   "typedef char frame_is_40_bytes[sizeof(lsdr_track_frame) == 40 && offsetof(lsdr_track_frame, tune) == 8 && offsetof(lsdr_track_frame, power) == 24 ? 1 : -1];\n"
                   "typedef char summary_is_28_bytes[sizeof(lsdr_track_summary) == 28 ? 1 : -1];\n"
                   "typedef char knot_is_16_bytes[sizeof(lsdr_track_knot) == 16 && offsetof(lsdr_track_knot, tune) == 8 ? 1 : -1];\n"
                   "typedef char dcfg_is_40_bytes[sizeof(lsdr_derotate_batch_cfg) == 40 && offsetof(lsdr_derotate_batch_cfg, max_samples) == 16 ? 1 : -1];\n"
                   "typedef char each_is_24_bytes[sizeof(lsdr_derotate_each) == 24 && offsetof(lsdr_derotate_each, n_knots) == 16 ? 1 : -1];\n"
                   "int main(void) { lsdr_tune_track_cfg c; lsdr_track_frame f; lsdr_track_summary s; lsdr_derotate_each e;\n"
                   "  c.hop = 0; c.span = 0; c.min_quality = 0; c.max_frames = 0; f.held = 0; f.center = 0; s.accepted = 0; s.quality_min = 0; e.knots = 0;\n"
                   "  (void)c; (void)f; (void)s; (void)e;\n"
                   "  int (*w)(lsdr_tune_track *, lsdr_track_summary *, lsdr_track_frame *) = lsdr_tune_track_wait; (void)w;\n"
                   "  int (*r)(lsdr_derotate_batch *, const void *const *, const lsdr_derotate_each *, lsdr_cf32 *const *) = lsdr_derotate_batch_run_async; (void)r;\n"
                   "  return LSDR_ABI_VERSION == 2 ? LSDR_OK : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_tracker_and_the_derotator(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []
    assert ctypes.sizeof(capi.TuneTrackCfg) == 48 and ctypes.sizeof(capi.TrackFrame) == 40 and ctypes.sizeof(capi.TrackSummary) == 28
    assert ctypes.sizeof(capi.TrackKnot) == 16 and ctypes.sizeof(capi.DerotateBatchCfg) == 40 and ctypes.sizeof(capi.DerotateEach) == 24
    assert [f[0] for f in capi.TrackFrame._fields_] == ["center", "tune", "quality", "bin", "held", "power", "mean_power"]
    assert [f[0] for f in capi.TrackSummary._fields_] == ["frames", "accepted", "tune_first", "tune_last", "tune_min", "tune_max", "quality_min"]
    assert capi.lib.lsdr_abi_version() == 2


def test_python_signatures(capi):
    params = lambda f: list(inspect.signature(f).parameters)
    t = inspect.signature(capi.TuneTracker.__init__).parameters
    assert list(t) == ["self", "ctx", "n_captures", "in_format", "in_scale", "blocks", "hop", "span", "min_quality", "max_frames"]
    assert (t["blocks"].default, t["hop"].default, t["span"].default, t["min_quality"].default) == (4, 65536, 64, capi.TUNE_MIN_QUALITY)
    assert params(capi.TuneTracker.track) == ["self", "ptrs", "lengths"]
    assert params(capi.DerotateBatch.__init__) == ["self", "ctx", "n_captures", "max_samples", "max_knots", "in_format", "in_scale"]
    assert params(capi.DerotateBatch.run) == ["self", "ptrs", "lengths", "knots", "outs"]
    d = params(capi.TrackedDecoder.__init__)
    assert d[:5] == ["self", "ctx", "n_captures", "max_samples", "omega"] and d[-1] == "tracker_kw"
    assert {"fec", "viterbi", "in_format", "in_scale", "relock", "anf"} <= set(d)
    assert params(capi.TrackedDecoder.decode) == ["self", "ptrs", "lengths"]
    frames = [dict(center=8192, tune=1e-3, held=0), dict(center=73728, tune=0.1, held=1), dict(center=139264, tune=2e-3, held=0)]
    assert capi.track_knots(frames) == [(8192, 1e-3), (139264, 2e-3)]
    # the recording decoder's constructor is unchanged: tune="pieces" is a value, not a parameter
    r = inspect.signature(capi.RecordingDecoder.__init__).parameters
    assert list(r) == ["self", "ctx", "piece_samples", "overlap_samples", "pieces_per_batch", "omega", "fec", "viterbi", "hs", "in_format", "in_scale",
                       "relock", "tune", "window", "min_run", "piece_ts", "batch_kw"] and r["tune"].default is None
