"""ctypes driver for liblsdr_hip.so (include/lsdr_hip.h).  No CPU fallback."""
import ctypes as C
import math
import os
import time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LSDR_HIP_LIB", os.path.join(HERE, "liblsdr_hip.so"))  # override: instrumented builds (tools/)

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(or `make -C leansdr_amd/csrc`). leansdr_amd has no CPU fallback.")

lib = C.CDLL(LIB_PATH)

c_f, c_sz, vp = C.c_float, C.c_size_t, C.c_void_p
psz = C.POINTER(c_sz)

SOFTSYM = np.dtype([("cost", "<i2"), ("symbol", "u1"), ("pad", "u1")])

(BPSK, QPSK, PSK8, APSK16, APSK32, APSK64E, QAM16, QAM64, QAM256) = range(9)
CSTLN_BITS = {BPSK: 1, QPSK: 2, PSK8: 3, APSK16: 4, APSK32: 5, APSK64E: 6, QAM16: 4, QAM64: 6, QAM256: 8}
(FEC12, FEC23, FEC46, FEC34, FEC56, FEC78, FEC45, FEC89, FEC910) = range(9)
IN_CF32, IN_CU8 = 0, 1
IN_CS8, IN_CU16, IN_CS16 = 2, 3, 4
SYM_SOFT, SYM_HARD2 = 0, 1
FIR_EXACT, FIR_FMA, FIR_MFMA, FIR_MFMA_BLK = 0, 1, 2, 3
SAMP_NEAREST, SAMP_LINEAR, SAMP_FIR = 0, 1, 2
RX_SERIAL, RX_TILED = 0, 1
NOTCH_EXACT, NOTCH_SCAN = 0, 1


class LsdrError(RuntimeError):
    pass


class FirCfg(C.Structure):
    _fields_ = [("ncoeffs", C.c_uint), ("coeffs_host", vp), ("decim", C.c_uint),
                ("in_format", C.c_int), ("in_scale", c_f), ("arith", C.c_int)]


class NotchFirCfg(C.Structure):
    _fields_ = [("ncoeffs", C.c_uint), ("coeffs_host", vp), ("decim", C.c_uint), ("in_scale", c_f), ("nslots", C.c_int),
                ("notch_decimation", C.c_int), ("k", c_f)]


class RxCfg(C.Structure):
    _fields_ = [("sampler", C.c_int), ("ncoeffs", C.c_int), ("coeffs_host", vp), ("subsampling", C.c_int),
                ("cstln", C.c_int), ("fec", C.c_int), ("harden", C.c_int), ("omega", c_f), ("freq", c_f),
                ("pll_adjustment", c_f), ("allow_drift", C.c_int), ("meas_decimation", C.c_ulong),
                ("kest", c_f), ("mode", C.c_int), ("tile_len", C.c_uint), ("tile_warmup", C.c_uint), ("in_format", C.c_int), ("out_format", C.c_int)]


class RxState(C.Structure):
    _fields_ = [("mu", c_f), ("phase", c_f), ("freqw", c_f), ("agc_gain", c_f), ("est_insp", c_f),
                ("est_sp", c_f), ("est_ep", c_f), ("freq_tap", c_f), ("min_freqw", c_f), ("max_freqw", c_f),
                ("meas_count", C.c_ulong), ("hist", c_f * 12)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "hist"}
        d["hist"] = list(self.hist)
        return d


def _sig(name, restype, argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = argtypes
    return fn


_sig("lsdr_abi_version", C.c_int, [])
# include/lsdr_hip.h LSDR_ABI_VERSION: 2 since lsdr_rx_run_multi_async writes one `consumed` PER receiver (round 5) — a caller
# built against version 1 passed one size_t there.  A stale liblsdr_hip.so is refused at import, not discovered through memory damage.
ABI_VERSION = 2
if lib.lsdr_abi_version() != ABI_VERSION:
    raise ImportError(f"liblsdr_hip.so reports ABI version {lib.lsdr_abi_version()}, leansdr_amd.capi is written for {ABI_VERSION}: "
                      "rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
_sig("lsdr_last_error", C.c_char_p, [])
_sig("lsdr_device_count", C.c_int, [])
_sig("lsdr_device_pci_bus_id", C.c_int, [C.c_int, C.c_char_p, C.c_int])


def device_pci_bus_id(device):
    buf = C.create_string_buffer(32)
    check(lib.lsdr_device_pci_bus_id(device, buf, 32))
    return buf.value.decode()
_sig("lsdr_ctx_create", C.c_int, [C.c_int, vp, C.POINTER(vp)])
_sig("lsdr_ctx_create_masked", C.c_int, [C.c_int, vp, C.c_uint, C.POINTER(vp)])
_sig("lsdr_ctx_destroy", None, [vp])
_sig("lsdr_ctx_sync", C.c_int, [vp])
_sig("lsdr_ctx_stream", vp, [vp])
_sig("lsdr_malloc", C.c_int, [vp, c_sz, C.POINTER(vp)])
_sig("lsdr_free", C.c_int, [vp, vp])
_sig("lsdr_malloc_host", C.c_int, [c_sz, C.POINTER(vp)])
PROBE_FN = C.CFUNCTYPE(C.c_int, vp, vp)
_sig("lsdr_arena_create", C.c_int, [vp, c_sz, C.POINTER(vp)])
_sig("lsdr_arena_destroy", None, [vp])
_sig("lsdr_arena_bytes", c_sz, [vp])
_sig("lsdr_arena_owns", C.c_int, [vp, vp])
_sig("lsdr_arena_place", C.c_int, [vp, c_sz, C.c_uint, C.c_uint, C.c_int, vp, vp, vp, C.POINTER(vp), C.POINTER(C.c_float)])
_sig("lsdr_arena_time", C.c_int, [vp, vp, vp, vp, C.POINTER(C.c_float)])
_sig("lsdr_arena_release", C.c_int, [vp, vp])
_sig("lsdr_arena_probe_log", C.c_int, [vp, C.POINTER(C.c_float), C.c_uint, C.POINTER(C.c_uint)])
_sig("lsdr_ctx_set_arena", C.c_int, [vp, vp])
_sig("lsdr_free_host", C.c_int, [vp])
_sig("lsdr_memcpy_h2d", C.c_int, [vp, vp, vp, c_sz])
_sig("lsdr_memcpy_d2h", C.c_int, [vp, vp, vp, c_sz])
_sig("lsdr_memcpy_d2d", C.c_int, [vp, vp, vp, c_sz])
_sig("lsdr_memset", C.c_int, [vp, vp, C.c_int, c_sz])
_sig("lsdr_timer_start", C.c_int, [vp])
_sig("lsdr_timer_stop_ms", C.c_int, [vp, C.POINTER(c_f)])
_sig("lsdr_event_create", C.c_int, [vp, C.POINTER(vp)])
_sig("lsdr_event_destroy", None, [vp])
_sig("lsdr_event_record", C.c_int, [vp])
_sig("lsdr_event_elapsed_ms", C.c_int, [vp, vp, C.POINTER(c_f)])
_sig("lsdr_ctx_wait_event", C.c_int, [vp, vp])
_sig("lsdr_filtergen_lowpass", C.c_int, [C.c_int, c_f, c_f, vp])
_sig("lsdr_filtergen_root_raised_cosine", C.c_int, [C.c_int, c_f, c_f, vp])
_sig("lsdr_filtergen_normalize_dcgain", None, [C.c_int, vp, c_f])
_sig("lsdr_filtergen_normalize_power", None, [C.c_int, vp, c_f])
_sig("lsdr_trig16_table", None, [vp])
_sig("lsdr_cstln_lut_build", C.c_int, [C.c_int, C.c_int, vp, vp, vp, vp, C.POINTER(C.c_int)])
_sig("lsdr_cconverter_u8_run", C.c_int, [vp, vp, c_sz, vp])
_sig("lsdr_scaler_run", C.c_int, [vp, c_f, vp, c_sz, vp])
_sig("lsdr_decimator_run", C.c_int, [vp, C.c_uint, vp, c_sz, vp, c_sz, psz])
_sig("lsdr_auto_notch_create", C.c_int, [vp, C.c_int, c_f, C.POINTER(vp)])
_sig("lsdr_auto_notch_destroy", None, [vp])
_sig("lsdr_auto_notch_set", C.c_int, [vp, C.c_int, c_f])
_sig("lsdr_auto_notch_slot_bin", C.c_int, [vp, C.c_int])
_sig("lsdr_auto_notch_set_mode", C.c_int, [vp, C.c_int])
_sig("lsdr_auto_notch_stats", C.c_int, [vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint)])
_sig("lsdr_auto_notch_scan_time", C.c_int, [vp, C.c_int, C.POINTER(c_f), C.POINTER(C.c_uint)])
if hasattr(lib, "lsdr_auto_notch_debug_poison"):       # the measure build only (make -C leansdr_amd/csrc measure)
    _sig("lsdr_auto_notch_debug_poison", C.c_int, [vp])
_sig("lsdr_auto_notch_set_overlap", C.c_int, [vp, C.c_int])
_sig("lsdr_auto_notch_check", C.c_int, [vp, C.POINTER(C.c_uint)])
_sig("lsdr_auto_notch_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_notch_fir_create", C.c_int, [vp, C.POINTER(NotchFirCfg), C.POINTER(vp)])
_sig("lsdr_notch_fir_destroy", None, [vp])
_sig("lsdr_notch_fir_set", C.c_int, [vp, C.c_int, c_f])
_sig("lsdr_notch_fir_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_notch_fir_slot_bin", C.c_int, [vp])
_sig("lsdr_notch_fir_set_overlap", C.c_int, [vp, C.c_int])
_sig("lsdr_notch_fir_set_freq", C.c_int, [vp, c_f])
_sig("lsdr_notch_fir_track", C.c_int, [vp, c_f, c_f, c_f, C.POINTER(C.c_int)])
_sig("lsdr_notch_fir_current_freq", c_f, [vp])
_sig("lsdr_notch_fir_time", C.c_int, [vp, C.c_int, C.POINTER(c_f), C.POINTER(C.c_uint)])
_sig("lsdr_cfft_host", C.c_int, [C.c_int, vp, C.c_int])
_sig("lsdr_cnr_fft_create", C.c_int, [vp, c_f, C.c_int, C.POINTER(vp)])
_sig("lsdr_cnr_fft_destroy", None, [vp])
_sig("lsdr_cnr_fft_set", C.c_int, [vp, C.c_int, c_f])
_sig("lsdr_cnr_fft_run", C.c_int, [vp, c_f, c_f, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_mpeg_sync_set_resync_period", C.c_int, [vp, C.c_int])
_sig("lsdr_fastqpsk_create", C.c_int, [vp, c_f, c_f, c_f, C.c_int, C.c_ulong, C.POINTER(vp)])
_sig("lsdr_fastqpsk_destroy", None, [vp])
_sig("lsdr_fastqpsk_get_state", C.c_int, [vp, C.POINTER(c_f), C.POINTER(C.c_uint), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)])
_sig("lsdr_fastqpsk_set_tiled", C.c_int, [vp, C.c_int, C.c_uint, C.c_uint])
_sig("lsdr_fastqpsk_tiled_stats", C.c_int, [vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint)])
_sig("lsdr_fastqpsk_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz, vp, c_sz, psz, vp, c_sz, psz])
_sig("lsdr_hsdeconv_create", C.c_int, [vp, C.c_int, C.POINTER(vp)])
_sig("lsdr_hsdeconv_destroy", None, [vp])
_sig("lsdr_hsdeconv_locked", C.c_int, [vp])
_sig("lsdr_hsdeconv_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_cfft_run", C.c_int, [vp, C.c_int, C.c_int, vp, vp])
_sig("lsdr_randomizer_create", C.c_int, [vp, C.POINTER(vp)])
_sig("lsdr_randomizer_destroy", None, [vp])
_sig("lsdr_randomizer_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_rs_encoder_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_interleaver_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_convol_create", C.c_int, [vp, C.c_int, C.c_int, C.POINTER(vp)])
_sig("lsdr_convol_destroy", None, [vp])
_sig("lsdr_convol_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_cstln_transmitter_run", C.c_int, [vp, C.c_int, C.c_int, vp, c_sz, vp])
_sig("lsdr_fir_resampler_create", C.c_int, [vp, C.c_uint, vp, C.c_uint, C.POINTER(vp)])
_sig("lsdr_fir_resampler_destroy", None, [vp])
_sig("lsdr_fir_resampler_set_freq", C.c_int, [vp, c_f])
_sig("lsdr_fir_resampler_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_simple_agc_create", C.c_int, [vp, c_f, c_f, C.POINTER(vp)])
_sig("lsdr_simple_agc_destroy", None, [vp])
_sig("lsdr_simple_agc_set", C.c_int, [vp, c_f, c_f])
_sig("lsdr_simple_agc_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_wgn_create", C.c_int, [vp, C.c_int, C.c_long, C.POINTER(vp)])
_sig("lsdr_wgn_destroy", None, [vp])
_sig("lsdr_wgn_get_state", C.c_int, [vp, C.POINTER(C.c_ulonglong)])
_sig("lsdr_wgn_set_state", C.c_int, [vp, C.c_ulonglong])
_sig("lsdr_wgn_run", C.c_int, [vp, c_f, vp, vp, c_sz])
_sig("lsdr_adder_run", C.c_int, [vp, vp, vp, c_sz, vp])
_sig("lsdr_cconverter_f32_u8_run", C.c_int, [vp, vp, c_sz, vp])
_sig("lsdr_cconverter_f32_s16_run", C.c_int, [vp, vp, c_sz, vp])
_sig("lsdr_drifter_create", C.c_int, [vp, C.POINTER(vp)])
_sig("lsdr_drifter_destroy", None, [vp])
_sig("lsdr_drifter_set_component", C.c_int, [vp, C.c_int, c_f, c_f])
_sig("lsdr_drifter_get_phases", C.c_int, [vp, C.c_longlong * 3])
_sig("lsdr_drifter_set_phases", C.c_int, [vp, C.c_longlong * 3])
_sig("lsdr_drifter_run", C.c_int, [vp, vp, c_sz, vp, c_sz])
_sig("lsdr_rotator_create", C.c_int, [vp, c_f, C.POINTER(vp)])
_sig("lsdr_rotator_destroy", None, [vp])
_sig("lsdr_rotator_run", C.c_int, [vp, vp, c_sz, vp])
_sig("lsdr_spectrum_create", C.c_int, [vp, C.POINTER(vp)])
_sig("lsdr_spectrum_destroy", None, [vp])
_sig("lsdr_spectrum_set", C.c_int, [vp, C.c_int, c_f])
_sig("lsdr_spectrum_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_fir_filter_create", C.c_int, [vp, C.POINTER(FirCfg), C.POINTER(vp)])
_sig("lsdr_fir_filter_destroy", None, [vp])
_sig("lsdr_fir_filter_set_freq", C.c_int, [vp, c_f])
_sig("lsdr_fir_filter_track", C.c_int, [vp, c_f, c_f, c_f, C.POINTER(C.c_int)])
_sig("lsdr_fir_filter_current_freq", c_f, [vp])
_sig("lsdr_fir_filter_get_shifted_coeffs", C.c_int, [vp, vp])
_sig("lsdr_fir_filter_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_fir_filter_run_multi", C.c_int, [vp, C.c_uint, C.POINTER(vp), c_sz, C.POINTER(vp), c_sz, psz, psz])
_sig("lsdr_rx_create", C.c_int, [vp, C.POINTER(RxCfg), C.POINTER(vp)])
_sig("lsdr_rx_destroy", None, [vp])
_sig("lsdr_rx_readahead", C.c_int, [vp])
_sig("lsdr_rx_get_state", C.c_int, [vp, C.POINTER(RxState)])
_sig("lsdr_rx_set_state", C.c_int, [vp, C.POINTER(RxState)])
_sig("lsdr_rx_tiled_stats", C.c_int, [vp] + [C.POINTER(C.c_uint)] * 4)
_sig("lsdr_deconv_create", C.c_int, [vp, C.c_int, C.c_int, C.POINTER(vp)])
_sig("lsdr_deconv_destroy", None, [vp])
_sig("lsdr_deconv_next_sync", C.c_int, [vp])
_sig("lsdr_deconv_reset", C.c_int, [vp])
_sig("lsdr_mpeg_sync_reset", C.c_int, [vp])
_sig("lsdr_derandomizer_reset", C.c_int, [vp])
_sig("lsdr_rx_reset", C.c_int, [vp])
_sig("lsdr_rx_tile_time", C.c_int, [vp, C.c_int, C.POINTER(c_f), C.POINTER(C.c_uint)])
_sig("lsdr_deconv_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_deconv_run_hs2", C.c_int, [vp, vp, c_sz, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_viterbi_create", C.c_int, [vp, C.c_int, C.c_int, C.POINTER(vp)])
_sig("lsdr_viterbi_destroy", None, [vp])
_sig("lsdr_viterbi_set_resync_period", C.c_int, [vp, C.c_int])
_sig("lsdr_viterbi_current_sync", C.c_int, [vp])
_sig("lsdr_viterbi_stats", C.c_int, [vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint)])
_sig("lsdr_viterbi_repair_stats", C.c_int, [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)])
_sig("lsdr_viterbi_q4_supported", C.c_int, [C.c_int, C.c_int])
_sig("lsdr_viterbi_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])


class ViterbiBatchResult(C.Structure):
    """lsdr_viterbi_batch_result"""
    _fields_ = [("consumed", C.c_uint64), ("produced", C.c_uint64), ("current_sync", C.c_uint32), ("resync_phase", C.c_uint32),
                ("switched", C.c_uint32), ("stalled", C.c_uint32), ("tiles", C.c_uint32), ("repaired", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


_sig("lsdr_viterbi_batch_create", C.c_int, [vp, C.c_int, C.c_int, C.c_int, c_sz, C.POINTER(vp)])
_sig("lsdr_viterbi_batch_destroy", None, [vp])
_sig("lsdr_viterbi_batch_set_resync_period", C.c_int, [vp, C.c_int])
_sig("lsdr_viterbi_batch_reset", C.c_int, [vp, C.c_int])
_sig("lsdr_viterbi_batch_run_async", C.c_int, [vp, C.POINTER(vp), psz, vp, C.POINTER(vp), c_sz])
_sig("lsdr_viterbi_batch_wait", C.c_int, [vp, C.POINTER(ViterbiBatchResult)])
_sig("lsdr_viterbi_batch_results_dev", vp, [vp])
_sig("lsdr_viterbi_batch_stats", C.c_int, [vp, C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)])
_sig("lsdr_mpeg_sync_create", C.c_int, [vp, C.c_int, C.POINTER(vp)])
_sig("lsdr_mpeg_sync_destroy", None, [vp])
_sig("lsdr_mpeg_sync_locked", C.c_int, [vp])
_sig("lsdr_mpeg_sync_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz, vp, C.POINTER(C.c_int), C.POINTER(C.c_ulong), C.POINTER(C.c_int)])
_sig("lsdr_deinterleaver_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_rs_decoder_run", C.c_int, [vp, vp, c_sz, vp, C.POINTER(C.c_long), C.POINTER(C.c_long)])
_sig("lsdr_derandomizer_create", C.c_int, [vp, C.POINTER(vp)])
_sig("lsdr_derandomizer_destroy", None, [vp])
_sig("lsdr_derandomizer_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_derandomizer_pattern", None, [vp])
_sig("lsdr_rs_tables", None, [vp, vp, vp])
_sig("lsdr_rx_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz, vp, vp, vp, c_sz, psz, vp, c_sz, psz])
_sig("lsdr_rx_run_async", C.c_int, [vp, vp, c_sz, vp, c_sz, psz])
_sig("lsdr_rx_run_multi_async", C.c_int, [C.POINTER(vp), C.c_uint, C.POINTER(vp), c_sz, C.POINTER(vp), c_sz, psz])
_sig("lsdr_rx_run_async_hs2", C.c_int, [vp, vp, c_sz, vp, c_sz, c_sz, psz])
_sig("lsdr_rx_wait", C.c_int, [vp, psz])
_sig("lsdr_rx_retired_freq_tap", C.c_float, [vp])
_sig("lsdr_fec_spec", C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), vp])
_sig("lsdr_cconverter_int_run", C.c_int, [vp, C.c_int, vp, c_sz, vp])
_sig("lsdr_copy_h2d_async", C.c_int, [vp, vp, vp, c_sz])
_sig("lsdr_copy_d2h_async", C.c_int, [vp, vp, vp, c_sz])
_sig("lsdr_copy_fence", C.c_int, [vp])
_sig("lsdr_copy_sync_d2h", C.c_int, [vp])
_sig("lsdr_copy_sync_all", C.c_int, [vp])
_sig("lsdr_rx_batch_create", C.c_int, [vp, C.POINTER(RxCfg), C.c_uint, C.POINTER(vp)])
_sig("lsdr_rx_batch_destroy", None, [vp])
_sig("lsdr_rx_batch_run", C.c_int, [vp, vp, c_sz, vp, c_sz, psz, psz])
_sig("lsdr_rx_batch_get_state", C.c_int, [vp, C.c_uint, C.POINTER(RxState)])
_sig("lsdr_rx_decision_mode", C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint)])
_sig("lsdr_rx_snapshot_async", C.c_int, [vp])
_sig("lsdr_rx_get_snapshot", C.c_int, [vp, C.POINTER(RxState)])
_sig("lsdr_rx_snapshot_async_slot", C.c_int, [vp, C.c_uint])
_sig("lsdr_rx_get_snapshot_slot", C.c_int, [vp, C.c_uint, C.POINTER(RxState)])


class CaptureBatchCfg(C.Structure):
    _fields_ = [("n_captures", C.c_int), ("max_samples", C.c_size_t), ("omega", C.c_float), ("fec", C.c_int), ("anf", C.c_int),
                ("tile_len", C.c_uint), ("tile_warmup", C.c_uint), ("notch_k", C.c_float), ("notch_decimation", C.c_int),
                ("unlocked_window", C.c_uint), ("aux_cus", C.c_uint)]


class CaptureResult(C.Structure):
    _fields_ = [("ts_packets", C.c_uint64), ("rs_packets", C.c_uint64), ("rs_bit_errors", C.c_uint64), ("symbols", C.c_uint64),
                ("samples", C.c_uint64), ("bytes_deconv", C.c_uint64), ("bytes_mpeg", C.c_uint64), ("first_lock_byte", C.c_uint64),
                ("next_sync_calls", C.c_uint32), ("locked", C.c_uint32), ("alignment", C.c_uint32), ("bitphase", C.c_uint32),
                ("tiles", C.c_uint32), ("seam_dup", C.c_uint32), ("seam_miss", C.c_uint32), ("seam_bad", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class CaptureViterbiCfg(C.Structure):
    _fields_ = [("resync_period", C.c_int), ("reserved", C.c_int * 7)]


class CaptureViterbiStats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("batch_rounds", C.c_uint32), ("switches", C.c_uint32), ("stalls", C.c_uint32),
                ("tiles", C.c_uint32), ("repaired", C.c_uint32), ("current_sync", C.c_uint32), ("pad", C.c_uint32),
                ("symbols", C.c_uint64), ("bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


_sig("lsdr_capture_batch_create", C.c_int, [vp, C.POINTER(CaptureBatchCfg), C.POINTER(vp)])
_sig("lsdr_capture_batch_create_viterbi", C.c_int, [vp, C.POINTER(CaptureBatchCfg), C.POINTER(CaptureViterbiCfg), C.POINTER(vp)])
class CaptureInputCfg(C.Structure):
    _fields_ = [("in_format", C.c_int), ("in_scale", C.c_float), ("reserved", C.c_int * 6)]


_sig("lsdr_capture_any_create", C.c_int, [vp, C.POINTER(CaptureBatchCfg), C.POINTER(CaptureViterbiCfg), C.POINTER(CaptureInputCfg), C.POINTER(vp)])
_sig("lsdr_capture_any_run_async", C.c_int, [vp, vp, c_sz])
_sig("lsdr_capture_batch_soft_dev", vp, [vp, C.c_int])
_sig("lsdr_capture_batch_viterbi_stats", C.c_int, [vp, C.c_int, C.POINTER(CaptureViterbiStats)])
class CaptureRelockStats(C.Structure):
    """lsdr_capture_relock_stats: capture i's re-acquisition record (40 bytes)."""
    _fields_ = [("locks", C.c_uint32), ("drops", C.c_uint32), ("passes", C.c_uint32), ("exhausted", C.c_uint32),
                ("first_drop_byte", C.c_uint64), ("last_lock_byte", C.c_uint64), ("next_sync_behind_first_lock", C.c_uint32), ("pad", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


_sig("lsdr_capture_relock_set", C.c_int, [vp, C.c_uint])
_sig("lsdr_capture_relock_get", C.c_int, [vp, C.c_int, C.POINTER(CaptureRelockStats)])
_sig("lsdr_capture_batch_destroy", None, [vp])
_sig("lsdr_capture_batch_run_async", C.c_int, [vp, vp, c_sz])
_sig("lsdr_capture_batch_wait", C.c_int, [vp, vp])
_sig("lsdr_capture_batch_ts_download_async", C.c_int, [vp, vp, c_sz])
_sig("lsdr_capture_batch_ts_wait", C.c_int, [vp])
_sig("lsdr_capture_batch_ts_dev", vp, [vp, C.c_int])
_sig("lsdr_capture_batch_words_dev", vp, [vp, C.c_int])
_sig("lsdr_capture_batch_bytes_dev", vp, [vp, C.c_int])
_sig("lsdr_capture_batch_mpeg_dev", vp, [vp, C.c_int])
_sig("lsdr_capture_batch_bins", C.c_int, [vp, C.c_int, vp, C.c_uint, C.POINTER(C.c_uint)])
_sig("lsdr_capture_batch_notched", C.c_int, [vp, C.c_int, vp, c_sz])
_sig("lsdr_capture_batch_tile_time", C.c_int, [vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint)])


class CaptureReport(C.Structure):
    _fields_ = [("freq", C.c_float), ("ss", C.c_float), ("mer", C.c_float), ("pad", C.c_uint32)]


_sig("lsdr_capture_reports_set", C.c_int, [vp, C.c_uint64])
_sig("lsdr_capture_reports_get", C.c_int, [vp, C.c_int, C.POINTER(CaptureReport), c_sz, psz, C.POINTER(CaptureReport)])


class HsBatchCfg(C.Structure):
    _fields_ = [("n_captures", C.c_int), ("max_samples", C.c_size_t), ("omega", C.c_float), ("freq", C.c_float), ("allow_drift", C.c_int),
                ("fastlock", C.c_int), ("tile_len", C.c_uint), ("tile_warmup", C.c_uint), ("reserved", C.c_int * 8)]


_sig("lsdr_hs_batch_create", C.c_int, [vp, C.POINTER(HsBatchCfg), C.POINTER(vp)])


class CaptureEach(C.Structure):
    """lsdr_capture_each: one capture's length and tune in an `each` run."""
    _fields_ = [("n_samples", C.c_size_t), ("tune", C.c_float), ("reserved", C.c_int * 5)]


_sig("lsdr_capture_each_run_async", C.c_int, [vp, vp, C.POINTER(CaptureEach)])
_sig("lsdr_hs_each_run_async", C.c_int, [vp, vp, C.POINTER(CaptureEach)])
_sig("lsdr_hs_batch_destroy", None, [vp])
_sig("lsdr_hs_batch_run_async", C.c_int, [vp, vp, c_sz])
_sig("lsdr_hs_batch_wait", C.c_int, [vp, vp])
_sig("lsdr_hs_batch_ts_download_async", C.c_int, [vp, vp, c_sz])
_sig("lsdr_hs_batch_ts_wait", C.c_int, [vp])
_sig("lsdr_hs_batch_ts_dev", vp, [vp, C.c_int])
_sig("lsdr_hs_batch_symbols_dev", vp, [vp, C.c_int])
_sig("lsdr_hs_batch_bytes_dev", vp, [vp, C.c_int])
_sig("lsdr_hs_batch_mpeg_dev", vp, [vp, C.c_int])


class TuneEstCfg(C.Structure):
    _fields_ = [("n_captures", C.c_int), ("in_format", C.c_int), ("in_scale", C.c_float), ("blocks", C.c_uint), ("reserved", C.c_int * 4)]


class TuneEstimate(C.Structure):
    """lsdr_tune_estimate: one capture's estimated carrier offset."""
    _fields_ = [("tune", C.c_float), ("quality", C.c_float), ("bin", C.c_uint32), ("blocks", C.c_uint32), ("power", C.c_float * 3),
                ("mean_power", C.c_float)]

    def as_dict(self):
        return dict(tune=float(self.tune), quality=float(self.quality), bin=int(self.bin), blocks=int(self.blocks),
                    power=[float(v) for v in self.power], mean_power=float(self.mean_power))


_sig("lsdr_tune_est_create", C.c_int, [vp, C.POINTER(TuneEstCfg), C.POINTER(vp)])
_sig("lsdr_tune_est_destroy", None, [vp])
_sig("lsdr_tune_est_run_async", C.c_int, [vp, vp, psz])
_sig("lsdr_tune_est_wait", C.c_int, [vp, C.POINTER(TuneEstimate)])


class TuneTrackCfg(C.Structure):
    _fields_ = [("n_captures", C.c_int), ("in_format", C.c_int), ("in_scale", C.c_float), ("blocks", C.c_uint), ("hop", C.c_uint),
                ("span", C.c_uint), ("min_quality", C.c_float), ("max_frames", C.c_uint), ("reserved", C.c_int * 4)]


class TrackFrame(C.Structure):
    """lsdr_track_frame: one frame of a capture's carrier track."""
    _fields_ = [("center", C.c_uint64), ("tune", C.c_float), ("quality", C.c_float), ("bin", C.c_uint32), ("held", C.c_uint32),
                ("power", C.c_float * 3), ("mean_power", C.c_float)]

    def as_dict(self):
        return dict(center=int(self.center), tune=float(self.tune), quality=float(self.quality), bin=int(self.bin), held=int(self.held),
                    power=[float(v) for v in self.power], mean_power=float(self.mean_power))


class TrackSummary(C.Structure):
    """lsdr_track_summary: a capture's track over its accepted frames."""
    _fields_ = [("frames", C.c_uint32), ("accepted", C.c_uint32), ("tune_first", C.c_float), ("tune_last", C.c_float),
                ("tune_min", C.c_float), ("tune_max", C.c_float), ("quality_min", C.c_float)]

    def as_dict(self):
        return dict(frames=int(self.frames), accepted=int(self.accepted), tune_first=float(self.tune_first), tune_last=float(self.tune_last),
                    tune_min=float(self.tune_min), tune_max=float(self.tune_max), quality_min=float(self.quality_min))


_sig("lsdr_tune_track_create", C.c_int, [vp, C.POINTER(TuneTrackCfg), C.POINTER(vp)])
_sig("lsdr_tune_track_destroy", None, [vp])
_sig("lsdr_tune_track_max_frames", C.c_uint, [vp])
_sig("lsdr_tune_track_run_async", C.c_int, [vp, vp, psz])
_sig("lsdr_tune_track_wait", C.c_int, [vp, C.POINTER(TrackSummary), C.POINTER(TrackFrame)])


class TrackKnot(C.Structure):
    """lsdr_track_knot: the carrier offset `tune` (cycles per sample) at `sample`."""
    _fields_ = [("sample", C.c_uint64), ("tune", C.c_double)]


class DerotateBatchCfg(C.Structure):
    _fields_ = [("n_captures", C.c_int), ("in_format", C.c_int), ("in_scale", C.c_float), ("max_knots", C.c_uint), ("max_samples", C.c_size_t),
                ("reserved", C.c_int * 4)]


class DerotateEach(C.Structure):
    _fields_ = [("n_samples", C.c_size_t), ("knots", C.POINTER(TrackKnot)), ("n_knots", C.c_uint), ("reserved", C.c_uint)]


_sig("lsdr_derotate_batch_create", C.c_int, [vp, C.POINTER(DerotateBatchCfg), C.POINTER(vp)])
_sig("lsdr_derotate_batch_destroy", None, [vp])
_sig("lsdr_derotate_batch_run_async", C.c_int, [vp, vp, C.POINTER(DerotateEach), vp])
_sig("lsdr_derotate_batch_wait", C.c_int, [vp])


class RateEstCfg(C.Structure):
    _fields_ = [("n_captures", C.c_int), ("in_format", C.c_int), ("in_scale", C.c_float), ("blocks", C.c_uint), ("omega_min", C.c_float),
                ("omega_max", C.c_float), ("reserved", C.c_int * 2)]


class RateEstimate(C.Structure):
    """lsdr_rate_estimate: one capture's estimated samples per symbol."""
    _fields_ = [("omega", C.c_float), ("other", C.c_float), ("line", C.c_float), ("quality", C.c_float), ("corr", C.c_float),
                ("bin", C.c_uint32), ("blocks", C.c_uint32), ("ambiguous", C.c_uint32), ("power", C.c_float * 3), ("floor", C.c_float)]

    def as_dict(self):
        return dict(omega=float(self.omega), other=float(self.other), line=float(self.line), quality=float(self.quality),
                    corr=float(self.corr), bin=int(self.bin), blocks=int(self.blocks), ambiguous=int(self.ambiguous),
                    power=[float(v) for v in self.power], floor=float(self.floor))


_sig("lsdr_rate_est_create", C.c_int, [vp, C.POINTER(RateEstCfg), C.POINTER(vp)])
_sig("lsdr_rate_est_destroy", None, [vp])
_sig("lsdr_rate_est_run_async", C.c_int, [vp, vp, psz])
_sig("lsdr_rate_est_wait", C.c_int, [vp, C.POINTER(RateEstimate)])


class CarrierScanCfg(C.Structure):
    _fields_ = [("n_captures", C.c_int), ("in_format", C.c_int), ("in_scale", C.c_float), ("blocks", C.c_uint), ("spread", C.c_int),
                ("smooth", C.c_uint), ("threshold_db", C.c_float), ("min_bins", C.c_uint), ("max_carriers", C.c_uint), ("reserved", C.c_int * 3)]


class ScanSummary(C.Structure):
    """lsdr_scan_summary: what the carrier scan found in one capture."""
    _fields_ = [("blocks", C.c_uint32), ("stride", C.c_uint32), ("found", C.c_uint32), ("listed", C.c_uint32), ("saturated", C.c_uint32),
                ("reserved", C.c_uint32), ("floor", C.c_float), ("threshold", C.c_float)]

    def as_dict(self):
        return dict(blocks=int(self.blocks), stride=int(self.stride), found=int(self.found), listed=int(self.listed),
                    saturated=int(self.saturated), floor=float(self.floor), threshold=float(self.threshold))


class ScanCarrier(C.Structure):
    """lsdr_scan_carrier: one carrier of a capture."""
    _fields_ = [("center", C.c_float), ("bandwidth", C.c_float), ("omega", C.c_float), ("level", C.c_float), ("plateau", C.c_float),
                ("first_bin", C.c_uint32), ("bins", C.c_uint32), ("weak", C.c_uint32)]

    def as_dict(self):
        level = float(self.level)
        return dict(center=float(self.center), bandwidth=float(self.bandwidth), omega=float(self.omega), level=level,
                    cnr_db=10.0 * math.log10(level) if level > 0 else float("-inf"), plateau=float(self.plateau),
                    first_bin=int(self.first_bin), bins=int(self.bins), weak=int(self.weak))


_sig("lsdr_carrier_scan_create", C.c_int, [vp, C.POINTER(CarrierScanCfg), C.POINTER(vp)])
_sig("lsdr_carrier_scan_destroy", None, [vp])
_sig("lsdr_carrier_scan_run_async", C.c_int, [vp, vp, psz])
_sig("lsdr_carrier_scan_wait", C.c_int, [vp, C.POINTER(ScanSummary), C.POINTER(ScanCarrier)])
_sig("lsdr_carrier_scan_spectrum_dev", vp, [vp, C.c_int])


HSYM_PACKED2, HSYM_U8, HSYM_SOFT = 0, 1, 2   # lsdr_fec_est's input formats


class FecEstCfg(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("max_symbols", C.c_size_t), ("in_format", C.c_int), ("reserved", C.c_int * 5)]


class FecEstScore(C.Structure):
    _fields_ = [("errors", C.c_uint64), ("checks", C.c_uint64), ("sync", C.c_uint32), ("skip", C.c_uint32)]


class FecEstimate(C.Structure):
    """lsdr_fec_estimate: one stream's estimated code rate."""
    _fields_ = [("fec", C.c_int32), ("locked", C.c_uint32), ("ambiguous", C.c_uint32), ("sync", C.c_uint32), ("skip", C.c_uint32),
                ("pad", C.c_uint32), ("symbols", C.c_uint64), ("error_rate", C.c_float), ("runner_up", C.c_float), ("score", FecEstScore * 5)]

    def as_dict(self):
        return dict(fec=int(self.fec), locked=int(self.locked), ambiguous=int(self.ambiguous), sync=int(self.sync), skip=int(self.skip),
                    symbols=int(self.symbols), error_rate=float(self.error_rate), runner_up=float(self.runner_up),
                    score=[dict(errors=int(s.errors), checks=int(s.checks), sync=int(s.sync), skip=int(s.skip)) for s in self.score])


_sig("lsdr_fec_est_create", C.c_int, [vp, C.POINTER(FecEstCfg), C.POINTER(vp)])
_sig("lsdr_fec_est_destroy", None, [vp])
_sig("lsdr_fec_est_tile", C.c_uint, [vp])
_sig("lsdr_fec_est_run_async", C.c_int, [vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
_sig("lsdr_fec_est_wait", C.c_int, [vp, C.POINTER(FecEstimate)])
_sig("lsdr_fec_est_polys", C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)])


class ResampleBatchCfg(C.Structure):
    _fields_ = [("n_captures", C.c_int), ("max_samples", C.c_size_t), ("in_format", C.c_int), ("in_scale", C.c_float), ("ncoeffs", C.c_uint),
                ("coeffs_host", vp), ("decim", C.c_uint), ("reserved", C.c_int * 6)]


class ResampleResult(C.Structure):
    """lsdr_resample_result: what one capture consumed and produced, and the derotation it got (ifreq / 65536 cycles per sample)."""
    _fields_ = [("consumed", C.c_uint64), ("produced", C.c_uint64), ("ifreq", C.c_int32), ("applied", C.c_float), ("pad", C.c_uint32 * 2)]


_sig("lsdr_resample_design", C.c_int, [c_f, c_f, c_f, C.c_uint, C.POINTER(C.c_uint), vp, C.c_uint, C.POINTER(C.c_uint)])
_sig("lsdr_resample_batch_create", C.c_int, [vp, C.POINTER(ResampleBatchCfg), C.POINTER(vp)])
_sig("lsdr_resample_batch_destroy", None, [vp])
_sig("lsdr_resample_batch_tile", C.c_uint, [vp])
_sig("lsdr_resample_batch_run_async", C.c_int, [vp, vp, C.POINTER(CaptureEach), vp, c_sz])
_sig("lsdr_resample_batch_wait", C.c_int, [vp, C.POINTER(ResampleResult)])


class SpectrumBatchCfg(C.Structure):
    _fields_ = [("n_captures", C.c_int), ("max_samples", C.c_size_t), ("in_format", C.c_int), ("in_scale", C.c_float), ("nfft", C.c_int),
                ("decimation", C.c_uint), ("kavg", C.c_float), ("bandwidth", C.c_float), ("emit_rows", C.c_int), ("slab_rows", C.c_uint),
                ("stages_per_pass", C.c_uint), ("reserved", C.c_int * 5)]


class SpectrumResult(C.Structure):
    """lsdr_spectrum_result: the whole blocks one capture consumed, its rows, and the bin of its band centre."""
    _fields_ = [("consumed", C.c_uint64), ("rows", C.c_uint64), ("icf", C.c_int32), ("pad", C.c_uint32 * 3)]


_sig("lsdr_spectrum_batch_create", C.c_int, [vp, C.POINTER(SpectrumBatchCfg), C.POINTER(vp)])
_sig("lsdr_spectrum_batch_destroy", None, [vp])
_sig("lsdr_spectrum_batch_max_rows", c_sz, [vp])
_sig("lsdr_spectrum_batch_slab_rows", C.c_uint, [vp])
_sig("lsdr_spectrum_batch_run_async", C.c_int, [vp, vp, C.POINTER(CaptureEach)])
_sig("lsdr_spectrum_batch_wait", C.c_int, [vp, C.POINTER(SpectrumResult)])
_sig("lsdr_spectrum_batch_cnr", C.c_int, [vp, C.c_int, vp, c_sz, psz])
_sig("lsdr_spectrum_batch_rows_db", C.c_int, [vp, C.c_int, vp, c_sz, psz])
_sig("lsdr_spectrum_batch_rows_dev", vp, [vp, C.c_int])


TS_DROP_NULL, TS_DROP_TEI, TS_DROP_SYNC = 1, 2, 4   # lsdr_ts_rule.drop


class TsBatchCfg(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("max_packets", C.c_size_t), ("max_pids", C.c_uint), ("reserved", C.c_int * 8)]


class TsRule(C.Structure):
    _fields_ = [("keep_pids", vp), ("drop", C.c_uint), ("want_index", C.c_int), ("reserved", C.c_int * 4)]


class TsSummary(C.Structure):
    """lsdr_ts_summary: one transport stream's census."""
    _fields_ = [(k, C.c_uint64) for k in ("packets", "sync_errors", "tei", "null_packets", "valid", "cc_errors", "cc_repeats", "cc_missing",
                                          "discontinuities", "kept", "pcr_first", "pcr_last", "pcr_first_packet", "pcr_last_packet")] + \
               [("pids_seen", C.c_uint32), ("pids_listed", C.c_uint32), ("pcr_pid", C.c_int32), ("pcr_count", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class TsPid(C.Structure):
    """lsdr_ts_pid: one PID of a stream's table."""
    _fields_ = [(k, C.c_uint32) for k in ("pid", "packets", "pusi", "scrambled", "cc_errors", "cc_repeats", "cc_missing", "discontinuities",
                                          "pcr_count", "pad")] + [("first_packet", C.c_uint64), ("last_packet", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


_sig("lsdr_ts_batch_create", C.c_int, [vp, C.POINTER(TsBatchCfg), C.POINTER(vp)])
_sig("lsdr_ts_batch_destroy", None, [vp])
_sig("lsdr_ts_batch_run_async", C.c_int, [vp, vp, C.POINTER(C.c_uint64), C.POINTER(TsRule)])
_sig("lsdr_ts_batch_wait", C.c_int, [vp, C.POINTER(TsSummary)])
_sig("lsdr_ts_batch_pids", C.c_int, [vp, C.c_int, C.POINTER(TsPid), C.c_uint, C.POINTER(C.c_uint)])
_sig("lsdr_ts_batch_out_dev", vp, [vp, C.c_int])
_sig("lsdr_ts_batch_index_dev", vp, [vp, C.c_int])
_sig("lsdr_ts_batch_download_async", C.c_int, [vp, vp, c_sz])
_sig("lsdr_ts_batch_download_wait", C.c_int, [vp])
_sig("lsdr_ts_batch_tile", C.c_uint, [vp])


class TsStitchCfg(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("max_packets", C.c_size_t), ("window", C.c_uint), ("min_run", C.c_uint), ("reserved", C.c_int * 8)]


class TsJoin(C.Structure):
    """lsdr_ts_join: where stream k + 1 continues stream k (24 bytes)."""
    _fields_ = [("joined", C.c_uint32), ("run", C.c_uint32), ("end", C.c_uint64), ("next_start", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class TsKeep(C.Structure):
    """lsdr_ts_keep: the packets [start, end) a stitch keeps of a stream, and their place in the output (24 bytes)."""
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64), ("out_offset", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


_sig("lsdr_ts_stitch_create", C.c_int, [vp, C.POINTER(TsStitchCfg), C.POINTER(vp)])
_sig("lsdr_ts_stitch_destroy", None, [vp])
_sig("lsdr_ts_stitch_run_async", C.c_int, [vp, vp, C.POINTER(C.c_uint64)])
_sig("lsdr_ts_stitch_wait", C.c_int, [vp, C.POINTER(TsJoin), C.POINTER(TsKeep)])
_sig("lsdr_ts_stitch_out_dev", vp, [vp])
_sig("lsdr_ts_stitch_download_async", C.c_int, [vp, vp, c_sz])
_sig("lsdr_ts_stitch_download_wait", C.c_int, [vp])


class TxBatchCfg(C.Structure):
    """lsdr_tx_batch_cfg"""
    _fields_ = [("n_streams", C.c_int), ("max_packets", C.c_size_t), ("cstln", C.c_int), ("interp", C.c_int), ("decim", C.c_int),
                ("rolloff", c_f), ("rrc_rej", c_f), ("agc", C.c_int), ("out_format", C.c_int), ("reserved", C.c_int * 8)]


class TxEach(C.Structure):
    """lsdr_tx_each: one stream of a run (64 bytes)."""
    _fields_ = [("n_packets", C.c_uint64), ("fec", C.c_int32), ("amp", c_f), ("scale", c_f), ("noise_stddev", c_f), ("seeded", C.c_int32),
                ("reserved0", C.c_int32), ("seed", C.c_int64), ("reserved", C.c_int32 * 6)]


class TxResult(C.Structure):
    """lsdr_tx_result (64 bytes)."""
    _fields_ = [(k, C.c_uint64) for k in ("packets", "bytes", "symbols", "samples", "noise_state")] + \
               [("noise_rounds", C.c_uint32), ("agc_estimated", c_f), ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


_sig("lsdr_tx_batch_create", C.c_int, [vp, C.POINTER(TxBatchCfg), C.POINTER(vp)])
_sig("lsdr_tx_batch_destroy", None, [vp])
_sig("lsdr_tx_batch_run_async", C.c_int, [vp, vp, C.POINTER(TxEach)])
_sig("lsdr_tx_batch_wait", C.c_int, [vp, C.POINTER(TxResult)])
_sig("lsdr_tx_batch_out_dev", vp, [vp, C.c_int])
_sig("lsdr_tx_batch_results_dev", vp, [vp])
_sig("lsdr_tx_batch_download_async", C.c_int, [vp, vp, c_sz])
_sig("lsdr_tx_batch_download_wait", C.c_int, [vp])
_sig("lsdr_tx_batch_stats", C.c_int, [vp, C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)])
_sig("lsdr_tx_batch_set_noise_margin", C.c_int, [vp, c_f])
_sig("lsdr_tx_batch_plan", C.c_int, [C.POINTER(TxBatchCfg), C.POINTER(TxEach), C.POINTER(TxResult)])
_sig("lsdr_db_to_amplitude", c_f, [C.c_double])

#: decode_estimated's default threshold on `quality`: the geometric mean of what Gaussian noise alone reaches (3.1) and the weakest of the
#: test captures (347), rounded
TUNE_MIN_QUALITY = 30.0

#: group_by_omega's default threshold on a rate estimate's `quality`: the geometric mean of what Gaussian noise alone reaches (2.3 with 16
#: blocks, 1.6 with 64) and the weakest of the test captures (47), rounded
RATE_MIN_QUALITY = 10.0

#: every symbol include/lsdr_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [n for n in dir(lib) if n.startswith("lsdr_")]


def check(rc):
    if rc != 0:
        raise LsdrError(f"lsdr error {rc}: {lib.lsdr_last_error().decode()}")


def _np(a):
    return a.ctypes.data_as(vp)


# ---- host-side table design (no GPU needed) --------------------------------
def lowpass(order, fcut, renormalize=True):
    """filtergen::lowpass (+ the extra normalize_dcgain of leandvb.cc:377-378)."""
    out = np.empty(order + 1, np.float32)
    n = lib.lsdr_filtergen_lowpass(order, fcut, 1.0, _np(out))
    if renormalize:
        lib.lsdr_filtergen_normalize_dcgain(n, _np(out), 1.0)
    return out[:n]


def root_raised_cosine(order, fs, rolloff):
    out = np.empty(order + 3, np.float32)
    n = lib.lsdr_filtergen_root_raised_cosine(order, fs, rolloff, _np(out))
    return out[:n].copy()


def normalize_power(coeffs, gain):
    c = np.ascontiguousarray(coeffs, np.float32).copy()
    lib.lsdr_filtergen_normalize_power(len(c), _np(c), gain)
    return c


def trig16():
    out = np.empty(65536, np.complex64)
    lib.lsdr_trig16_table(_np(out))
    return out


def cstln_lut(predef, fec=0):
    cost = np.empty(65536, np.int16)
    sym = np.empty(65536, np.uint8)
    pe = np.empty(65536, np.int16)
    symbols = np.zeros((256, 2), np.int8)
    nrot = C.c_int()
    n = lib.lsdr_cstln_lut_build(predef, fec, _np(cost), _np(sym), _np(pe), _np(symbols), C.byref(nrot))
    if n < 0:
        check(n)
    return dict(nsymbols=n, nrotations=nrot.value, symbols=symbols[:n].copy(), cost=cost, symbol=sym,
                phase_error=pe)


# ---- device side ------------------------------------------------------------
class DevBuf:
    """A device allocation (what a device-resident pipebuf owns)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = vp()
        check(lib.lsdr_malloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def free(self):
        if self.ptr:
            check(lib.lsdr_free(self.ctx.h, self.ptr))
            self.ptr = None

    def at(self, byte_offset):
        return vp(self.ptr + int(byte_offset))


class ArenaWindow:
    """A window of an Arena, with what a pipeline uses of a DevBuf; free() gives it back to the arena."""

    def __init__(self, arena, ptr, nbytes, probe_ms=None):
        self.arena, self.ptr, self.nbytes, self.probe_ms = arena, int(ptr), int(nbytes), probe_ms

    def at(self, byte_offset):
        return vp(self.ptr + int(byte_offset))

    def free(self):
        if self.ptr and self.arena.h:
            check(lib.lsdr_arena_release(self.arena.h, vp(self.ptr)))
        self.ptr = None


class Arena:
    """lsdr_arena (include/lsdr_hip.h): one large device allocation handed out in windows, the fastest ones first."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        h = vp()
        check(lib.lsdr_arena_create(ctx.h, int(nbytes), C.byref(h)))
        self.h = h
        self.nbytes = int(lib.lsdr_arena_bytes(h))

    def place(self, nbytes, n_best=1, max_windows=64, from_tail=False, fill_from=None, probe=None):
        """probe(window_ptr: int) queues the launch(es) to be timed on the context's stream (None: the built-in streaming read).
        Returns the n_best windows, fastest first (.probe_ms = ms per probe call)."""
        out = (vp * n_best)()
        ms = (C.c_float * n_best)()
        err = []

        def _cb(user, window):
            try:
                probe(int(window))
                return 0
            except BaseException as e:      # never unwinds through the C caller
                err.append(e)
                return -2
        cb = PROBE_FN(_cb) if probe is not None else C.cast(None, PROBE_FN)
        rc = lib.lsdr_arena_place(self.h, int(nbytes), n_best, max_windows, int(bool(from_tail)), vp(fill_from) if fill_from else None,
                                  C.cast(cb, vp), None, out, ms)
        if err:
            raise err[0]
        check(rc)
        return [ArenaWindow(self, out[k], nbytes, float(ms[k])) for k in range(n_best)]

    def time(self, ptr, probe):
        """ms per call of probe(ptr) over any device pointer, timed like a candidate window (3 untimed calls, 6 timed)."""
        ms = C.c_float()
        err = []

        def _cb(user, window):
            try:
                probe(int(window))
                return 0
            except BaseException as e:
                err.append(e)
                return -2
        cb = PROBE_FN(_cb)
        rc = lib.lsdr_arena_time(self.h, vp(int(ptr)), C.cast(cb, vp), None, C.byref(ms))
        if err:
            raise err[0]
        check(rc)
        return float(ms.value)

    def probe_log(self):
        n = C.c_uint()
        buf = (C.c_float * 4096)()
        check(lib.lsdr_arena_probe_log(self.h, buf, 4096, C.byref(n)))
        return [float(buf[i]) for i in range(min(n.value, 4096))]

    def attach(self, on=True):
        """lsdr_ctx_set_arena: lsdr_malloc of 1 MiB or more on this context is served from the arena from now on."""
        check(lib.lsdr_ctx_set_arena(self.ctx.h, self.h if on else None))

    def close(self):
        if self.h:
            lib.lsdr_ctx_set_arena(self.ctx.h, None)
            lib.lsdr_arena_destroy(self.h)
            self.h = None


class Ctx:
    def __init__(self, device=0, stream=None, cu_mask=None):
        """cu_mask: iterable of CU indices this context's stream may use (None: the whole GPU)."""
        h = vp()
        if cu_mask is None:
            check(lib.lsdr_ctx_create(device, stream, C.byref(h)))
        else:
            cus = sorted(set(int(c) for c in cu_mask))
            words = (max(cus) // 32 + 1) if cus else 1
            m = (C.c_uint32 * words)()
            for c in cus:
                m[c // 32] |= 1 << (c % 32)
            check(lib.lsdr_ctx_create_masked(device, m, words, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.lsdr_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        check(lib.lsdr_ctx_sync(self.h))

    def alloc(self, nbytes):
        return DevBuf(self, nbytes)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        b = DevBuf(self, max(arr.nbytes, 1))
        check(lib.lsdr_memcpy_h2d(self.h, b.ptr, _np(arr), arr.nbytes))
        self.sync()
        return b

    def download(self, buf, dtype, count, byte_offset=0):
        out = np.empty(count, dtype)
        check(lib.lsdr_memcpy_d2h(self.h, _np(out), buf.at(byte_offset), out.nbytes))
        self.sync()
        return out

    def event(self):
        e = vp()
        check(lib.lsdr_event_create(self.h, C.byref(e)))
        return e

    @staticmethod
    def event_record(e):
        check(lib.lsdr_event_record(e))

    @staticmethod
    def event_elapsed_ms(a, b):
        ms = c_f()
        check(lib.lsdr_event_elapsed_ms(a, b, C.byref(ms)))
        return ms.value

    def wait_event(self, e):
        check(lib.lsdr_ctx_wait_event(self.h, e))

    def timer_start(self):
        check(lib.lsdr_timer_start(self.h))

    def timer_stop_ms(self):
        ms = c_f()
        check(lib.lsdr_timer_stop_ms(self.h, C.byref(ms)))
        return ms.value

    # elementwise blocks on numpy arrays (test convenience)
    def cconverter_u8(self, u8):
        u8 = np.ascontiguousarray(u8, np.uint8).reshape(-1, 2)
        din = self.upload(u8)
        dout = self.alloc(len(u8) * 8)
        check(lib.lsdr_cconverter_u8_run(self.h, din.ptr, len(u8), dout.ptr))
        out = self.download(dout, np.complex64, len(u8))
        din.free(); dout.free()
        return out

    def cconverter_int(self, in_format, iq):
        """iq: interleaved re, im of int8 (IN_CS8), uint16 (IN_CU16) or int16 (IN_CS16)."""
        iq = np.ascontiguousarray(iq, {IN_CS8: np.int8, IN_CU16: np.uint16, IN_CS16: np.int16}[in_format]).reshape(-1, 2)
        din = self.upload(iq)
        dout = self.alloc(max(8, len(iq) * 8))
        check(lib.lsdr_cconverter_int_run(self.h, in_format, din.ptr, len(iq), dout.ptr))
        out = self.download(dout, np.complex64, len(iq))
        din.free(); dout.free()
        return out

    def scaler(self, scale, x):
        x = np.ascontiguousarray(x, np.complex64)
        din = self.upload(x)
        dout = self.alloc(x.nbytes)
        check(lib.lsdr_scaler_run(self.h, scale, din.ptr, len(x), dout.ptr))
        out = self.download(dout, np.complex64, len(x))
        din.free(); dout.free()
        return out

    def decimator(self, d, x):
        x = np.ascontiguousarray(x, np.complex64)
        din = self.upload(x)
        dout = self.alloc(x.nbytes)
        prod = c_sz()
        check(lib.lsdr_decimator_run(self.h, d, din.ptr, len(x), dout.ptr, len(x), C.byref(prod)))
        out = self.download(dout, np.complex64, prod.value)
        din.free(); dout.free()
        return out


class FirFilter:
    """fir_filter<cf32,float> (dsp.h:219-285) on the GPU."""

    def __init__(self, ctx, coeffs, decim=1, in_format=IN_CF32, in_scale=0.0, arith=FIR_EXACT):
        self.ctx = ctx
        self.coeffs = np.ascontiguousarray(coeffs, np.float32)
        self.decim = decim
        self.in_format = in_format
        cfg = FirCfg(len(self.coeffs), self.coeffs.ctypes.data, decim, in_format, in_scale, arith)
        h = vp()
        check(lib.lsdr_fir_filter_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.lsdr_fir_filter_destroy(self.h)
            self.h = None

    def set_freq(self, f):
        check(lib.lsdr_fir_filter_set_freq(self.h, f))

    def track(self, freq_tap, tap_multiplier, freq_tol):
        s = C.c_int()
        check(lib.lsdr_fir_filter_track(self.h, freq_tap, tap_multiplier, freq_tol, C.byref(s)))
        return bool(s.value)

    @property
    def current_freq(self):
        return lib.lsdr_fir_filter_current_freq(self.h)

    def shifted_coeffs(self):
        out = np.empty(len(self.coeffs), np.complex64)
        check(lib.lsdr_fir_filter_get_shifted_coeffs(self.h, _np(out)))
        return out

    def run_dev(self, in_ptr, n_in, out_ptr, cap_out):
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_fir_filter_run(self.h, in_ptr, n_in, out_ptr, cap_out, C.byref(cons), C.byref(prod)))
        return cons.value, prod.value

    def run_multi_dev(self, in_ptrs, n_in, out_ptrs, cap_out):
        """The same filter over several equal-length device buffers in one launch; returns (consumed, produced) per buffer."""
        n = len(in_ptrs)
        ins = (vp * n)(*[vp(p) if not isinstance(p, vp) else p for p in in_ptrs])
        outs = (vp * n)(*[vp(p) if not isinstance(p, vp) else p for p in out_ptrs])
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_fir_filter_run_multi(self.h, n, ins, n_in, outs, cap_out, C.byref(cons), C.byref(prod)))
        return cons.value, prod.value

    def run(self, x):
        """numpy in → (numpy out, consumed)."""
        if self.in_format == IN_CU8:
            x = np.ascontiguousarray(x, np.uint8).reshape(-1, 2)
        else:
            x = np.ascontiguousarray(x, np.complex64)
        n = len(x)
        cap = max(0, (n - len(self.coeffs)) // self.decim) + 1
        din = self.ctx.upload(x)
        dout = self.ctx.alloc(cap * 8)
        cons, prod = self.run_dev(din.ptr, n, dout.ptr, cap)
        out = self.ctx.download(dout, np.complex64, prod)
        din.free(); dout.free()
        return out, cons


class CstlnReceiver:
    """cstln_receiver<f32> (sdr.h:697-938) on the GPU."""

    def __init__(self, ctx, sampler=SAMP_LINEAR, coeffs=None, subsampling=1, cstln=QPSK, fec=FEC12, harden=0,
                 omega=4.0, freq=0.0, pll_adjustment=1.0, allow_drift=0, meas_decimation=1048576, kest=0.01,
                 mode=RX_SERIAL, tile_len=0, tile_warmup=0, in_format=0, out_format=0):
        """in_format = IN_CU8: cconverter<u8,128,f32,0,1,1> fused into the receiver's loads (input = cu8 items).
        out_format = SYM_HARD2 (tiled QPSK on cu8 only): packed 2-bit decisions instead of soft symbols."""
        self.ctx = ctx
        cfg = RxCfg()
        cfg.in_format, cfg.out_format = in_format, out_format
        cfg.sampler = sampler
        if coeffs is not None:
            self.coeffs = np.ascontiguousarray(coeffs, np.float32)
            cfg.ncoeffs = len(self.coeffs)
            cfg.coeffs_host = self.coeffs.ctypes.data
        cfg.subsampling = subsampling
        cfg.cstln, cfg.fec, cfg.harden = cstln, fec, harden
        cfg.omega, cfg.freq, cfg.pll_adjustment = omega, freq, pll_adjustment
        cfg.allow_drift, cfg.meas_decimation, cfg.kest = allow_drift, meas_decimation, kest
        cfg.mode, cfg.tile_len, cfg.tile_warmup = mode, tile_len, tile_warmup
        self.cfg = cfg
        h = vp()
        check(lib.lsdr_rx_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.lsdr_rx_destroy(self.h)
            self.h = None

    @property
    def readahead(self):
        return lib.lsdr_rx_readahead(self.h)

    def state(self):
        st = RxState()
        check(lib.lsdr_rx_get_state(self.h, C.byref(st)))
        return st

    def set_state(self, st):
        check(lib.lsdr_rx_set_state(self.h, C.byref(st)))

    def reset(self):
        """The loop state right after construction: the next run starts a new capture."""
        check(lib.lsdr_rx_reset(self.h))

    def tile_time(self, enable):
        """(mean ms, launches) of the k_rx_tiles launches of the runs retired since the last call; then set the switch."""
        ms, n = c_f(), C.c_uint()
        check(lib.lsdr_rx_tile_time(self.h, int(enable), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def decision_mode(self):
        a, d = C.c_int(), C.c_uint()
        check(lib.lsdr_rx_decision_mode(self.h, C.byref(a), C.byref(d)))
        return dict(arithmetic=bool(a.value), max_phase_error_delta=d.value)

    def snapshot_async(self, slot=0):
        """Copy the device-side loop state into one of the receiver's four pinned slots, in stream order (between queued runs)."""
        check(lib.lsdr_rx_snapshot_async_slot(self.h, slot))

    def snapshot(self, slot=0):
        st = RxState()
        check(lib.lsdr_rx_get_snapshot_slot(self.h, slot, C.byref(st)))
        return st

    def tiled_stats(self):
        v = [C.c_uint() for _ in range(4)]
        check(lib.lsdr_rx_tiled_stats(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("tiles", "dup", "miss", "bad_seams"), [x.value for x in v]))

    def run_async(self, in_ptr, n_in, out_ptr, cap_out):
        """Queue one tiled run on the receiver's stream; returns the samples it will consume."""
        cons = c_sz()
        check(lib.lsdr_rx_run_async(self.h, in_ptr, n_in, out_ptr, cap_out, C.byref(cons)))
        return cons.value

    @staticmethod
    def run_multi_async(rxs, in_ptrs, n_in, out_ptrs, cap_out):
        """lsdr_rx_run_multi_async: one tiled run of every receiver in `rxs` (equally long inputs) with shared launches; returns the
        LIST of samples each receiver will consume.  Each receiver is retired with its own wait()."""
        n = len(rxs)
        hs = (vp * n)(*[r.h for r in rxs])
        ins = (vp * n)(*[p if isinstance(p, vp) else vp(p) for p in in_ptrs])
        outs = (vp * n)(*[p if isinstance(p, vp) else vp(p) for p in out_ptrs])
        cons = (c_sz * n)()
        check(lib.lsdr_rx_run_multi_async(hs, n, ins, n_in, outs, cap_out, cons))
        return [int(v) for v in cons]

    def run_async_hs2(self, in_ptr, n_in, out_ptr, out_sym_offset, cap_out):
        """Queue one tiled run of a SYM_HARD2 receiver writing its packed symbols from symbol out_sym_offset of `out_ptr`."""
        cons = c_sz()
        check(lib.lsdr_rx_run_async_hs2(self.h, in_ptr, n_in, out_ptr, out_sym_offset, cap_out, C.byref(cons)))
        return cons.value

    def wait(self):
        """Retire the oldest queued run; returns its symbol count."""
        prod = c_sz()
        check(lib.lsdr_rx_wait(self.h, C.byref(prod)))
        return prod.value

    @property
    def retired_freq_tap(self):
        """freq_tap after the most recently retired queued run (cycles per sample)."""
        return lib.lsdr_rx_retired_freq_tap(self.h)

    def run_dev(self, in_ptr, n_in, out_ptr, cap_out, meas=True):
        cons, prod, nm, nc = c_sz(), c_sz(), c_sz(), c_sz()
        if meas:
            mcap = n_in // max(1, self.cfg.meas_decimation) + 8
            ccap = n_in // 128 + 8
            fr, ss, mer = (np.empty(mcap, np.float32) for _ in range(3))
            cst = np.empty(ccap, np.complex64)
            check(lib.lsdr_rx_run(self.h, in_ptr, n_in, out_ptr, cap_out, C.byref(cons), C.byref(prod),
                                  _np(fr), _np(ss), _np(mer), mcap, C.byref(nm), _np(cst), ccap, C.byref(nc)))
            return dict(consumed=cons.value, produced=prod.value, freq=fr[:nm.value], ss=ss[:nm.value],
                        mer=mer[:nm.value], cstln=cst[:nc.value])
        check(lib.lsdr_rx_run(self.h, in_ptr, n_in, out_ptr, cap_out, C.byref(cons), C.byref(prod),
                              None, None, None, 0, None, None, 0, None))
        return dict(consumed=cons.value, produced=prod.value)

    def run(self, x, meas=True):
        """x: complex64 samples, or (in_format = IN_CU8) a uint8 array of interleaved re, im."""
        if self.cfg.in_format == IN_CU8:
            x = np.ascontiguousarray(x, np.uint8).reshape(-1, 2)
        else:
            x = np.ascontiguousarray(x, np.complex64)
        cap = len(x) + 256
        din = self.ctx.upload(x)
        dout = self.ctx.alloc(cap * 4)
        r = self.run_dev(din.ptr, len(x), dout.ptr, cap, meas)
        r["sym"] = self.ctx.download(dout, SOFTSYM, r["produced"])
        r["state"] = self.state()
        din.free(); dout.free()
        return r


class RxBatch:
    """Exact cstln_receiver<f32>, one GPU lane per independent capture (lsdr_rx_batch_*)."""

    def __init__(self, ctx, n_streams, sampler=SAMP_LINEAR, cstln=QPSK, fec=FEC12, omega=4.0, freq=0.0, pll_adjustment=1.0,
                 allow_drift=0, meas_decimation=1048576, kest=0.01, in_format=0):
        self.ctx, self.n = ctx, n_streams
        cfg = RxCfg()
        cfg.in_format = in_format
        cfg.sampler, cfg.cstln, cfg.fec = sampler, cstln, fec
        cfg.omega, cfg.freq, cfg.pll_adjustment = omega, freq, pll_adjustment
        cfg.allow_drift, cfg.meas_decimation, cfg.kest = allow_drift, meas_decimation, kest
        cfg.subsampling = 1
        h = vp()
        check(lib.lsdr_rx_batch_create(ctx.h, C.byref(cfg), n_streams, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.lsdr_rx_batch_destroy(self.h)
            self.h = None

    def run_dev(self, in_ptrs, n_in, out_ptrs, cap_out):
        ins = (vp * self.n)(*[p if isinstance(p, vp) else vp(p) for p in in_ptrs])
        outs = (vp * self.n)(*[p if isinstance(p, vp) else vp(p) for p in out_ptrs])
        cons = c_sz()
        prod = (c_sz * self.n)()
        check(lib.lsdr_rx_batch_run(self.h, ins, n_in, outs, cap_out, C.byref(cons), prod))
        return cons.value, list(prod)

    def state(self, stream):
        st = RxState()
        check(lib.lsdr_rx_batch_get_state(self.h, stream, C.byref(st)))
        return st


class _BlockEstimator:
    """What TuneEstimator and RateEstimator share: one object per batch of n captures, (pointers, lengths) in, one record per capture out.
    A subclass names its entry points (lsdr_<_name>_create / _destroy / _run_async / _wait), its record type and its word in the error text."""
    _name = _word = _record = None

    def _create(self, ctx, cfg, n_captures, in_format, in_scale, blocks):
        self.ctx, self.n, self.h = ctx, int(n_captures), None
        cfg.n_captures, cfg.in_format, cfg.in_scale, cfg.blocks = self.n, int(in_format), float(in_scale), int(blocks)
        h = vp()
        check(self._fn("create")(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h
        self._out = (self._record * self.n)()

    def _fn(self, what):
        return getattr(lib, f"lsdr_{self._name}_{what}")

    def close(self):
        if self.h:
            self._fn("destroy")(self.h)
            self.h = None

    def _args(self, iq_ptrs, n_samples):
        n = [int(v) for v in n_samples]
        if len(n) != self.n or len(iq_ptrs) != self.n:
            raise LsdrError(f"{self._word} estimator: {len(iq_ptrs)} pointers and {len(n)} lengths for {self.n} captures")
        return (vp * self.n)(*[p if isinstance(p, vp) else vp(p) for p in iq_ptrs]), (c_sz * self.n)(*n)

    def run_async(self, iq_ptrs, n_samples):
        """Queues the estimate of every capture's first n_samples[i] items; a pointer may be None where the length is 0."""
        check(self._fn("run_async")(self.h, *self._args(iq_ptrs, n_samples)))

    def wait(self):
        check(self._fn("wait")(self.h, self._out))
        return [r.as_dict() for r in self._out]

    def estimate(self, iq_ptrs, n_samples):
        self.run_async(iq_ptrs, n_samples)
        return self.wait()


class TuneEstimator(_BlockEstimator):
    """lsdr_tune_est: the carrier offset of each of n_captures captures, estimated from the raw samples (QPSK: the spectral line of the
    fourth power, over the first `blocks` blocks of 4096 samples) — the number the batch decoders' per-capture tune wants."""
    _name, _word, _record = "tune_est", "tune", TuneEstimate

    def __init__(self, ctx, n_captures, in_format=IN_CU8, in_scale=0.0, blocks=8):
        self._create(ctx, TuneEstCfg(), n_captures, in_format, in_scale, blocks)

    def estimate(self, iq_ptrs, n_samples):
        """One run, synchronously: [dict(tune, quality, bin, blocks, power [l, c, r], mean_power)] per capture."""
        return super().estimate(iq_ptrs, n_samples)


class RateEstimator(_BlockEstimator):
    """lsdr_rate_est: the samples per symbol of each of n_captures captures, estimated from the raw samples (RRC-shaped PSK: the spectral
    line of the squared magnitude, over the first `blocks` blocks of 4096 samples) — the omega the batch objects want at construction."""
    _name, _word, _record = "rate_est", "rate", RateEstimate

    def __init__(self, ctx, n_captures, in_format=IN_CU8, in_scale=0.0, blocks=64, omega_min=0.0, omega_max=0.0):
        cfg = RateEstCfg()
        cfg.omega_min, cfg.omega_max = float(omega_min), float(omega_max)
        self._create(ctx, cfg, n_captures, in_format, in_scale, blocks)

    def estimate(self, iq_ptrs, n_samples):
        """One run, synchronously: [dict(omega, other, line, quality, corr, bin, blocks, ambiguous, power [l, c, r], floor)] per capture."""
        return super().estimate(iq_ptrs, n_samples)


def group_by_omega(estimates, rtol=1e-3, min_quality=RATE_MIN_QUALITY):
    """The captures of a job sorted by rate: ([(omega, [capture indices])], [indices left out]) from RateEstimator's records.  Taken in
    ascending omega, a record joins the group whose first member it is within rtol of, and a group's omega is the median of its members'
    — the caller makes one CaptureBatch / HsBatch / ResampledDecoder per group.  Left out, in their own list: records below min_quality
    (all-zero records among them) and `ambiguous` ones, whose two candidates are for the caller to try."""
    good = sorted((i for i, e in enumerate(estimates) if e["quality"] >= min_quality and not e["ambiguous"] and e["omega"] > 0),
                  key=lambda i: (estimates[i]["omega"], i))
    left = [i for i in range(len(estimates)) if i not in set(good)]
    groups = []
    for i in good:
        if groups and estimates[i]["omega"] <= estimates[groups[-1][0]]["omega"] * (1.0 + rtol):
            groups[-1].append(i)
        else:
            groups.append([i])
    out = []
    for g in groups:
        om = sorted(estimates[i]["omega"] for i in g)
        mid = len(om) // 2
        out.append((om[mid] if len(om) % 2 else 0.5 * (om[mid - 1] + om[mid]), sorted(g)))
    return out, left


class FecEstimator:
    """lsdr_fec_est: the code rate of each of n_streams streams of hard QPSK symbols, estimated from the first max_symbols of them — the
    fec the batch decoders want at construction.  The parity checks deconv[b] ^ deconv2[b] of deconvol_sync's --fastlock, swept over the
    five rates, every symbol phase of the puncturing pattern and the four alignments (include/lsdr_hip.h)."""

    def __init__(self, ctx, n_streams, max_symbols=16384, in_format=HSYM_PACKED2):
        self.ctx, self.n, self.h = ctx, int(n_streams), None
        cfg = FecEstCfg()
        cfg.n_streams, cfg.max_symbols, cfg.in_format = self.n, int(max_symbols), int(in_format)
        h = vp()
        check(lib.lsdr_fec_est_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h
        self.max_symbols, self.in_format = int(max_symbols), int(in_format)
        self._out = (FecEstimate * self.n)()

    def close(self):
        if self.h:
            lib.lsdr_fec_est_destroy(self.h)
            self.h = None

    @property
    def tile(self):
        """The symbols per workgroup tile of the score kernel."""
        return int(lib.lsdr_fec_est_tile(self.h))

    def run_async(self, ptrs, n, offsets=None):
        """Queues the estimate: ptrs device pointers (None where n is 0), n symbols per stream, offsets the first symbol's position in the
        stream at the pointer (None: zeros)."""
        n = [int(v) for v in n]
        off = [0] * self.n if offsets is None else [int(v) for v in offsets]
        if len(n) != self.n or len(ptrs) != self.n or len(off) != self.n:
            raise LsdrError(f"fec estimator: {len(ptrs)} pointers, {len(n)} lengths and {len(off)} offsets for {self.n} streams")
        p = (vp * self.n)(*[q if isinstance(q, vp) else vp(q) for q in ptrs])
        check(lib.lsdr_fec_est_run_async(self.h, p, (C.c_uint64 * self.n)(*off) if offsets is not None else None, (C.c_uint64 * self.n)(*n)))

    def wait(self):
        check(lib.lsdr_fec_est_wait(self.h, self._out))
        return [r.as_dict() for r in self._out]

    def estimate(self, ptrs, n, offsets=None):
        """One run, synchronously: [dict(fec, locked, ambiguous, sync, skip, symbols, error_rate, runner_up, score [5 × dict(errors, checks,
        sync, skip)])] per stream."""
        self.run_async(ptrs, n, offsets)
        return self.wait()


def fec_polys(rate):
    """(deconv, deconv2, punctperiod, punctweight) a rate is scored with: lsdr_fec_est_polys, what lsdr_deconv_create computes."""
    d, d2, pw = (C.c_uint64 * 8)(), (C.c_uint64 * 8)(), C.c_int()
    pp = lib.lsdr_fec_est_polys(int(rate), d, d2, C.byref(pw))
    if pp <= 0:
        raise LsdrError(f"lsdr_fec_est_polys: {lib.lsdr_last_error().decode()}")
    return [int(v) for v in d[:pp]], [int(v) for v in d2[:pp]], pp, int(pw.value)


def group_by_fec(estimates):
    """The captures of a job sorted by code rate: ([(fec, [capture indices])], [indices left out]) from FecEstimator's records, in the
    order 1/2, 2/3, 3/4, 5/6, 7/8 — the caller makes one CaptureBatch / HsBatch per group.  Left out, in their own list: records that
    are not `locked` (nothing scored among them) and `ambiguous` ones."""
    good = [i for i, e in enumerate(estimates) if e["locked"] and not e["ambiguous"] and e["fec"] >= 0]
    left = [i for i in range(len(estimates)) if i not in set(good)]
    groups = [(fec, [i for i in good if estimates[i]["fec"] == fec]) for fec in (FEC12, FEC23, FEC34, FEC56, FEC78)]
    return [g for g in groups if g[1]], left


class TsBatch:
    """lsdr_ts_batch: the census (packet classes, per-PID continuity counters, PCR) and the PID filter of n_streams transport streams in
    device memory, each with its own length, in shared launches (include/lsdr_hip.h).  The table of a stream holds its max_pids lowest
    PIDs."""

    def __init__(self, ctx, n_streams, max_packets, max_pids=64):
        self.ctx, self.n, self.h = ctx, int(n_streams), None
        cfg = TsBatchCfg()
        cfg.n_streams, cfg.max_packets, cfg.max_pids = self.n, int(max_packets), int(max_pids)
        h = vp()
        check(lib.lsdr_ts_batch_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h
        self.max_packets, self.max_pids = int(max_packets), int(max_pids) or 64
        self._sum = (TsSummary * max(self.n, 1))()
        self._tab = (TsPid * self.max_pids)()

    def close(self):
        if self.h:
            lib.lsdr_ts_batch_destroy(self.h)
            self.h = None

    @property
    def tile(self):
        """The packets per workgroup tile."""
        return int(lib.lsdr_ts_batch_tile(self.h))

    def keep_bitmap(self, keep_pids):
        """lsdr_ts_rule.keep_pids from a list of PIDs (for every stream) or a list of such lists, one per stream: uint8 [n][1024]."""
        per = list(keep_pids)
        if not per or np.isscalar(per[0]):
            per = [per] * self.n
        if len(per) != self.n:
            raise LsdrError(f"ts batch: {len(per)} PID lists for {self.n} streams")
        bm = np.zeros((self.n, 1024), np.uint8)
        for i, pids in enumerate(per):
            for p in pids:
                if not 0 <= int(p) < 8192:
                    raise LsdrError(f"ts batch: PID {p} is outside 0 … 8191")
                bm[i, int(p) >> 3] |= 1 << (int(p) & 7)
        return bm

    def run_async(self, ptrs, n_packets, rule=None):
        """Queues one run: ptrs device pointers (None where there are no packets), n_packets per stream, rule a TsRule or None (census)."""
        n = [int(v) for v in n_packets]
        if len(n) != self.n or len(ptrs) != self.n:
            raise LsdrError(f"ts batch: {len(ptrs)} pointers and {len(n)} lengths for {self.n} streams")
        p = (vp * self.n)(*[q if isinstance(q, vp) else vp(q) for q in ptrs])
        check(lib.lsdr_ts_batch_run_async(self.h, p, (C.c_uint64 * self.n)(*n), C.byref(rule) if rule is not None else None))

    def pids(self, i):
        """Stream i's table after a wait: [dict(pid, packets, pusi, scrambled, cc_errors, cc_repeats, cc_missing, discontinuities,
        pcr_count, first_packet, last_packet)], ascending in pid."""
        n = C.c_uint()
        check(lib.lsdr_ts_batch_pids(self.h, int(i), self._tab, self.max_pids, C.byref(n)))
        return [self._tab[k].as_dict() for k in range(n.value)]

    def wait(self):
        """[summary dict with "pids": the stream's table] per stream."""
        check(lib.lsdr_ts_batch_wait(self.h, self._sum))
        out = [s.as_dict() for s in self._sum[:self.n]]
        for i, s in enumerate(out):
            s["pids"] = self.pids(i)
        return out

    def census(self, ptrs, n_packets):
        """One run without a rule, synchronously."""
        self.run_async(ptrs, n_packets)
        return self.wait()

    def rule(self, keep_pids=None, drop_null=True, drop_tei=True, drop_sync=True, index=False):
        """(TsRule, the array its keep_pids points to: keep it alive until run_async has returned)."""
        r = TsRule()
        bm = None if keep_pids is None else self.keep_bitmap(keep_pids)
        r.keep_pids = None if bm is None else bm.ctypes.data
        r.drop = (TS_DROP_NULL if drop_null else 0) | (TS_DROP_TEI if drop_tei else 0) | (TS_DROP_SYNC if drop_sync else 0)
        r.want_index = 1 if index else 0
        return r, bm

    def out_ptr(self, i):
        return lib.lsdr_ts_batch_out_dev(self.h, int(i))

    def index_ptr(self, i):
        return lib.lsdr_ts_batch_index_dev(self.h, int(i))

    def download_async(self, host_arrays, cap_bytes=None):
        """Queues the copy of every stream's kept packets into host_arrays[i] (uint8 numpy arrays of cap_bytes, default the smallest)."""
        cap = min(a.nbytes for a in host_arrays) if cap_bytes is None else int(cap_bytes)
        check(lib.lsdr_ts_batch_download_async(self.h, (vp * self.n)(*[a.ctypes.data for a in host_arrays]), cap))

    def download_wait(self):
        check(lib.lsdr_ts_batch_download_wait(self.h))

    def filter(self, ptrs, n_packets, keep_pids=None, drop_null=True, drop_tei=True, drop_sync=True, index=False):
        """One run with a rule, synchronously: (summaries, [the kept packets' bytes per stream], [uint32 arrays of their indices in the
        input] or None).  keep_pids: None (every PID), a list of PIDs, or a list of such lists, one per stream."""
        r, bm = self.rule(keep_pids, drop_null, drop_tei, drop_sync, index)
        self.run_async(ptrs, n_packets, r)
        res = self.wait()
        cap = max([s["kept"] for s in res] + [1]) * 188
        bufs = [np.empty(cap, np.uint8) for _ in range(self.n)]
        self.download_async(bufs, cap)
        idx = None
        if index:
            idx = [np.empty(s["kept"], np.uint32) for s in res]
            for i, a in enumerate(idx):
                if len(a):
                    check(lib.lsdr_memcpy_d2h(self.ctx.h, _np(a), self.index_ptr(i), a.nbytes))
            self.ctx.sync()
        self.download_wait()
        return res, [b[:s["kept"] * 188].tobytes() for b, s in zip(bufs, res)], idx


class TsStitch:
    """lsdr_ts_stitch: n_streams transport streams in device memory, in recording order, each continuing the one before it somewhere
    inside an overlap, joined into one with every packet once (include/lsdr_hip.h has the definition: the join of a pair is the longest
    run of at least min_run byte-equal packets, enough of them not null, between the last `window` packets of one stream and the first
    `window` of the next)."""

    def __init__(self, ctx, n_streams, max_packets, window=4096, min_run=8):
        self.ctx, self.n, self.h = ctx, int(n_streams), None
        cfg = TsStitchCfg()
        cfg.n_streams, cfg.max_packets, cfg.window, cfg.min_run = self.n, int(max_packets), int(window), int(min_run)
        h = vp()
        check(lib.lsdr_ts_stitch_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h
        self.max_packets, self.window, self.min_run = int(max_packets), int(window) or 4096, int(min_run) or 8
        self._joins, self._keep = (TsJoin * max(self.n - 1, 1))(), (TsKeep * self.n)()
        self.packets = 0

    def close(self):
        if self.h:
            lib.lsdr_ts_stitch_destroy(self.h)
            self.h = None

    def run_async(self, ptrs, n_packets):
        """Queues one run: ptrs device pointers (None where there are no packets), n_packets per stream."""
        n = [int(v) for v in n_packets]
        if len(n) != self.n or len(ptrs) != self.n:
            raise LsdrError(f"ts stitch: {len(ptrs)} pointers and {len(n)} lengths for {self.n} streams")
        p = (vp * self.n)(*[q if isinstance(q, vp) else vp(q) for q in ptrs])
        check(lib.lsdr_ts_stitch_run_async(self.h, p, (C.c_uint64 * self.n)(*n)))

    def wait(self):
        """([dict(joined, run, end, next_start)] per pair, [dict(start, end, out_offset)] per stream); self.packets: the output's."""
        check(lib.lsdr_ts_stitch_wait(self.h, self._joins, self._keep))
        keep = [k.as_dict() for k in self._keep]
        self.packets = keep[-1]["out_offset"] + keep[-1]["end"] - keep[-1]["start"]
        return [j.as_dict() for j in self._joins[:self.n - 1]], keep

    def out_ptr(self):
        return lib.lsdr_ts_stitch_out_dev(self.h)

    def download(self):
        """The output of the run waited for (bytes), over the object's download stream."""
        a = np.empty(self.packets * 188, np.uint8)
        check(lib.lsdr_ts_stitch_download_async(self.h, _np(a), a.nbytes))
        check(lib.lsdr_ts_stitch_download_wait(self.h))
        return a.tobytes()

    def stitch_records(self, ptrs, n_packets):
        """One run, synchronously: (joins, keep); the stitched TS stays on the device (out_ptr(), self.packets packets)."""
        self.run_async(ptrs, n_packets)
        return self.wait()

    def stitch(self, ptrs, n_packets):
        """One run, synchronously: (joins, keep, the stitched TS's bytes)."""
        joins, keep = self.stitch_records(ptrs, n_packets)
        return joins, keep, self.download()


def unjoined(joins):
    """The indices k of the pairs (k, k + 1) a stitch could not join."""
    return [k for k, j in enumerate(joins) if not j["joined"]]


def recording_plan(n_samples, piece_samples, overlap_samples):
    """The pieces a recording of n_samples is decoded in, [(first sample, length)], in closed form: piece i starts at i·(piece − overlap),
    the last may be short, and there are max(1, ⌈(n − overlap) / (piece − overlap)⌉) of them.  Piece and overlap are multiples of 8 samples
    (overlap_for gives multiples of 4096), so every piece of a 16-byte aligned recording starts 16-byte aligned in every sample format.
    No GPU, no context."""
    n, piece, overlap = int(n_samples), int(piece_samples), int(overlap_samples)
    if piece % 8 or overlap % 8 or not 0 <= overlap < piece:
        raise LsdrError(f"recording: piece ({piece}) and overlap ({overlap}) must be multiples of 8 samples with 0 <= overlap < piece")
    stride = piece - overlap
    count = max(1, -(-(n - overlap) // stride))
    return [(i * stride, max(0, min(piece, n - i * stride))) for i in range(count)]


#: 2500 − the most packets the capture batch returned of the 2500 sent, plus the most it locked behind the reference (`late`), per code
#: rate: README.md's table "Acquisition, batch against reference" (tests/test_gpu_capture_batch_rates.py, 1.2 samples per symbol)
ACQUISITION_PACKETS = {FEC12: 2500 - 2443 + 0, FEC23: 2500 - 2426 + 64, FEC34: 2500 - 2458 + 72, FEC56: 2500 - 2425 + 46, FEC78: 2500 - 2473 + 56}
FEC_RATE = {FEC12: (1, 2), FEC23: (2, 3), FEC34: (3, 4), FEC56: (5, 6), FEC78: (7, 8)}


def overlap_for(fec, omega, packets=None, window=4096):
    """An overlap in samples for RecordingDecoder: `packets` RS packets of 204·8 bits at 2·rate bits per symbol and omega samples per
    symbol, packets·204·8 / (2·rate)·omega, rounded up to a multiple of 4096.
    packets None: ACQUISITION_PACKETS[fec] + window.  A piece returns nothing of its first ACQUISITION_PACKETS[fec] packets — the table
    above is what the README's rate table records: the packets missing from the best of nine 2500-packet captures per rate, which counts
    the few lost at the capture's end as well, plus the most the batch locked behind the reference there — and behind them the overlap
    then holds `window` packets, all that a join looks at.  Measured at 1.2 samples per symbol with the default engine only; the table
    has no entry for other rates, and this function refuses them."""
    if fec not in ACQUISITION_PACKETS:
        raise LsdrError(f"overlap_for: no acquisition figure for code rate {fec}")
    if packets is None:
        packets = ACQUISITION_PACKETS[fec] + int(window)
    num, den = FEC_RATE[fec]
    samples = int(packets) * 204 * 8 * den / (2 * num) * float(omega)
    return -(-int(math.ceil(samples)) // 4096) * 4096


def ts_bitrate(summary):
    """The stream's bit rate from its PCRs: the bits between the first and the last packet that carry one, over the time between the two
    values (27 MHz ticks, the 33-bit base wraps).  None with fewer than two PCRs or no difference."""
    if summary["pcr_count"] < 2:
        return None
    ticks = (summary["pcr_last"] - summary["pcr_first"]) % ((1 << 33) * 300)
    packets = summary["pcr_last_packet"] - summary["pcr_first_packet"]
    if not ticks or not packets:
        return None
    return packets * 188 * 8 * 27e6 / ticks


class _TailBatch:
    """What the objects in front of the device-resident FEC tail share (CaptureBatch, HsBatch): a batch of self.n captures through
    run_async / wait, the TS download, and fetching TS and stage bytes.  A subclass sets _what, its name in error texts, and _c, the
    prefix of its C entry points (<_c>_wait, _ts_download_async, _ts_wait, _ts_dev, _bytes_dev, _mpeg_dev and _destroy), and hands its
    handle, its run_async entry point and its `each` entry point (per-capture lengths and tunes, lsdr_capture_each) to _attach."""

    def _attach(self, h, run, run_each):
        self.h, self._run, self._run_each = h, run, run_each
        self._res = (CaptureResult * max(self.n, 1))()

    def _fn(self, name):
        return getattr(lib, f"{self._c}_{name}")

    def _ptrs(self, ptrs):
        return (vp * self.n)(*[p if isinstance(p, vp) else vp(p) for p in ptrs])

    def close(self):
        est = getattr(self, "_est", None)
        if est:
            est[1].close()
            self._est = None
        fest = getattr(self, "_fec_est", None)
        if fest:
            fest.close()
            self._fec_est = None
        tsb = getattr(self, "_ts_batch", None)
        if tsb:
            tsb.close()
            self._ts_batch = None
        tss = getattr(self, "_ts_stitch", None)
        if tss:
            tss.close()
            self._ts_stitch = None
        if self.h:
            self._fn("destroy")(self.h)
            self.h = None

    def _ts_object(self, results):
        """(the cached TsBatch, sized for the longest TS so far; every capture's TS pointer; its packets) after a wait."""
        n = [int(r["ts_packets"]) for r in results]
        tsb = getattr(self, "_ts_batch", None)
        if not tsb or tsb.max_packets < max(n + [1]):
            if tsb:
                tsb.close()
            self._ts_batch = tsb = TsBatch(self.ctx, self.n, max(n + [1]))
        return tsb, [self._fn("ts_dev")(self.h, i) if n[i] else None for i in range(self.n)], n

    def ts_census(self, results):
        """After a wait: the census of every capture's TS where the run left it on the device (TsBatch.census over ts_dev(i) and
        results[i]["ts_packets"]).  The decode is not touched."""
        tsb, ptrs, n = self._ts_object(results)
        return tsb.census(ptrs, n)

    def ts_filter(self, results, **rule):
        """After a wait: TsBatch.filter over every capture's TS on the device — (summaries, [kept bytes], [indices] or None); rule:
        keep_pids, drop_null, drop_tei, drop_sync, index."""
        tsb, ptrs, n = self._ts_object(results)
        return tsb.filter(ptrs, n, **rule)

    def ts_stitch(self, results, window=4096, min_run=8):
        """After a wait, where the batch's captures are the overlapping pieces of one recording in order: TsStitch.stitch over every
        capture's TS on the device — (joins, keep, the stitched TS's bytes).  The decode is not touched."""
        n = [int(r["ts_packets"]) for r in results]
        tss = getattr(self, "_ts_stitch", None)
        if not tss or tss.max_packets < max(n + [1]) or (tss.window, tss.min_run) != (int(window), int(min_run)):
            if tss:
                tss.close()
            self._ts_stitch = tss = TsStitch(self.ctx, self.n, max(n + [1]), window, min_run)
        return tss.stitch([self._fn("ts_dev")(self.h, i) if n[i] else None for i in range(self.n)], n)

    def estimate_fec(self, results, max_symbols=16384):
        """After a wait: every capture's code rate, estimated from the hard decisions the run left on the device (FecEstimator over the
        first max_symbols of results[i]["symbols"]) — what `fec` this object should have been made with.  Reads what the front end wrote;
        the decode is not touched."""
        fmt, ptr = self._fec_symbols()
        fest = getattr(self, "_fec_est", None)
        if not fest or fest.max_symbols != int(max_symbols) or fest.in_format != fmt:
            if fest:
                fest.close()
            self._fec_est = fest = FecEstimator(self.ctx, self.n, max_symbols, fmt)
        n = [int(r["symbols"]) for r in results]
        return fest.estimate([ptr(i) if n[i] else None for i in range(self.n)], n)

    def run_async(self, iq_ptrs, n_samples):
        check(self._run(self.h, self._ptrs(iq_ptrs), int(n_samples)))

    def each(self, n_samples, tune=None):
        """The lsdr_capture_each array of a batch: n_samples a list (one length per capture), tune None (the uniform call's: 0, or the
        hs batch's freq), a scalar for all captures or a list."""
        n = [int(v) for v in n_samples]
        if tune is None:
            tune = getattr(self, "freq", 0.0)
        t = [float(tune)] * self.n if np.isscalar(tune) else [float(v) for v in tune]
        if len(n) != self.n or len(t) != self.n:
            raise LsdrError(f"{self._what}: {len(n)} lengths and {len(t)} tunes for {self.n} captures")
        e = (CaptureEach * max(self.n, 1))()
        for i in range(self.n):
            e[i].n_samples, e[i].tune = n[i], t[i]
        return e

    def run_each_async(self, iq_ptrs, n_samples, tune=None):
        """run_async with a length (and a tune, leandvb's --tune as Ftune/Fs in cycles per sample) per capture; a pointer may be None where
        the length is 0."""
        check(self._run_each(self.h, self._ptrs(iq_ptrs), self.each(n_samples, tune)))

    def wait(self, results=True):
        check(self._fn("wait")(self.h, self._res if results else None))
        return [r.as_dict() for r in self._res[:self.n]] if results else None

    def ts_download_async(self, host_ptrs, cap_bytes):
        check(self._fn("ts_download_async")(self.h, self._ptrs(host_ptrs), int(cap_bytes)))

    def ts_wait(self):
        check(self._fn("ts_wait")(self.h))

    def _fetch(self, ptr, n, sync=True):
        """n bytes at the device pointer ptr (host; sync=False: there after the caller's ctx.sync())."""
        a = np.empty(int(n), np.uint8)
        if n:
            if ptr is None:
                raise LsdrError(f"{self._what}: no such capture")
            check(lib.lsdr_memcpy_d2h(self.ctx.h, _np(a), ptr, int(n)))
            if sync:
                self.ctx.sync()
        return a

    def decode(self, iq_ptrs, n_samples):
        """One batch, synchronously: (results, [TS bytes per capture])."""
        self.run_async(iq_ptrs, n_samples)
        return self._results_and_ts()

    def _results_and_ts(self):
        res = self.wait()
        out = [self._fetch(self._fn("ts_dev")(self.h, i), r["ts_packets"] * 188, sync=False) for i, r in enumerate(res)]
        self.ctx.sync()
        return res, [a.tobytes() for a in out]

    def decode_each(self, iq_ptrs, n_samples, tune=None):
        """decode with a length and a tune per capture (run_each_async)."""
        self.run_each_async(iq_ptrs, n_samples, tune)
        return self._results_and_ts()

    def decode_estimated(self, iq_ptrs, n_samples, blocks=8, min_quality=TUNE_MIN_QUALITY):
        """decode_each with every capture's tune ESTIMATED from its own samples (TuneEstimator in this object's sample format, over the
        first `blocks` blocks): (results, [TS bytes per capture], estimates).  A capture whose quality is below min_quality has no line
        worth tuning to and is decoded with tune 0.  QPSK, |offset| < 1/8 cycle per sample."""
        est = getattr(self, "_est", None)
        if not est or est[0] != int(blocks):
            if est:
                est[1].close()
            self._est = est = (int(blocks), TuneEstimator(self.ctx, self.n, getattr(self, "in_format", IN_CU8), getattr(self, "in_scale", 0.0), blocks))
        estimates = est[1].estimate(iq_ptrs, n_samples)
        tune = [e["tune"] if e["quality"] >= min_quality else 0.0 for e in estimates]
        res, ts = self.decode_each(iq_ptrs, n_samples, tune)
        return res, ts, estimates

    def stage_bytes(self, i, which, n):
        """The first n bytes in front of mpeg_sync ("deconv") or behind it ("mpeg") of capture i after a run (host)."""
        return self._fetch(self._fn("bytes_dev" if which == "deconv" else "mpeg_dev")(self.h, int(i)), n)


class CaptureBatch(_TailBatch):
    """lsdr_capture_batch: B independent cu8 captures, each from its first sample to TS (leandvb's default `--u8` graph per capture),
    in shared launches with the counts on the device.  viterbi=True (or a dict of lsdr_capture_viterbi_cfg fields): the `--viterbi` graph —
    soft symbols, viterbi_sync, mpeg_sync without a deconvolver.  in_format / in_scale (lsdr_capture_input_cfg): captures of IN_CS8,
    IN_CU16, IN_CS16 or IN_CF32 items, converted (and multiplied by in_scale) in the kernels' loads — leandvb's --s8 / --u16 / --s16 /
    --f32 --float-scale; the converted samples must have an RMS near 75 (the level contract, include/lsdr_hip.h).
    relock=R (default engine, 0 … 16): re-acquire up to R times after a lost lock — the deconvolver stays one unlocked_window ahead of
    mpeg_sync until the (R+1)-th lock (lsdr_capture_relock_set); relock_stats(i) after a wait."""
    _c, _what = "lsdr_capture_batch", "capture batch"

    def __init__(self, ctx, n_captures, max_samples, omega, fec=FEC12, anf=1, tile_len=0, tile_warmup=0, notch_k=0.0, notch_decimation=0,
                 unlocked_window=0, aux_cus=0, viterbi=None, in_format=IN_CU8, in_scale=0.0, reports=0, relock=0):
        self.ctx, self.n = ctx, int(n_captures)
        cfg = CaptureBatchCfg()
        cfg.n_captures, cfg.max_samples, cfg.omega, cfg.fec, cfg.anf = self.n, int(max_samples), omega, fec, anf
        cfg.tile_len, cfg.tile_warmup, cfg.notch_k, cfg.notch_decimation = tile_len, tile_warmup, notch_k, notch_decimation
        cfg.unlocked_window = unlocked_window
        cfg.aux_cus = aux_cus
        self.unlocked_window = unlocked_window or 8192
        h = vp()
        self.viterbi = bool(viterbi)
        self.in_format, self.in_scale = int(in_format), float(in_scale)
        self._any = self.in_format != IN_CU8 or self.in_scale != 0.0
        vcfg = CaptureViterbiCfg()
        if self.viterbi:
            vcfg.resync_period = int(viterbi.get("resync_period", 0)) if isinstance(viterbi, dict) else 0
        if self._any:
            icfg = CaptureInputCfg()
            icfg.in_format, icfg.in_scale = self.in_format, self.in_scale
            check(lib.lsdr_capture_any_create(ctx.h, C.byref(cfg), C.byref(vcfg) if self.viterbi else None, C.byref(icfg), C.byref(h)))
        elif self.viterbi:
            check(lib.lsdr_capture_batch_create_viterbi(ctx.h, C.byref(cfg), C.byref(vcfg), C.byref(h)))
        else:
            check(lib.lsdr_capture_batch_create(ctx.h, C.byref(cfg), C.byref(h)))
        self._attach(h, lib.lsdr_capture_any_run_async if self._any else lib.lsdr_capture_batch_run_async, lib.lsdr_capture_each_run_async)
        self.relock = 0
        try:
            if reports:
                self.set_reports(reports)
            if relock:
                self.set_relock(relock)
        except Exception:
            self.close()
            raise

    def set_relock(self, relocks):
        """Re-acquisitions of the batches queued from here on (0: off).  Not while a batch is in flight; not on a Viterbi object."""
        check(lib.lsdr_capture_relock_set(self.h, int(relocks)))
        self.relock = int(relocks)

    def relock_stats(self, i):
        """Capture i's re-acquisition record of the waited-for batch: dict(locks, drops, passes, exhausted, first_drop_byte,
        last_lock_byte, next_sync_behind_first_lock)."""
        st = CaptureRelockStats()
        check(lib.lsdr_capture_relock_get(self.h, int(i), C.byref(st)))
        return st.as_dict()

    def _fec_symbols(self):
        """estimate_fec's input: the soft symbols of a Viterbi object, the packed decisions otherwise."""
        if self.viterbi:
            return HSYM_SOFT, self.soft_ptr
        return HSYM_PACKED2, lambda i: lib.lsdr_capture_batch_words_dev(self.h, int(i))

    def words(self, i, nsym):
        """The packed decisions of capture i after a run, unpacked (host)."""
        nw = (int(nsym) + 15) // 16
        w = np.empty(nw, np.uint32)
        if nw:
            check(lib.lsdr_memcpy_d2h(self.ctx.h, _np(w), lib.lsdr_capture_batch_words_dev(self.h, i), nw * 4))
            self.ctx.sync()
        return hs2_unpack(w, int(nsym))

    def soft_ptr(self, i):
        """Device pointer of capture i's compacted soft symbols (Viterbi objects; None otherwise or for i out of range)."""
        return lib.lsdr_capture_batch_soft_dev(self.h, int(i))

    def soft(self, i, n):
        """The first n soft symbols of capture i after a run (Viterbi objects), as a SOFTSYM array (host)."""
        a = np.empty(int(n), SOFTSYM)
        p = self.soft_ptr(i)
        if p is None:
            raise LsdrError("capture batch: no soft symbols (not a Viterbi object, or no such capture)")
        if n:
            check(lib.lsdr_memcpy_d2h(self.ctx.h, _np(a), p, int(n) * 4))
            self.ctx.sync()
        return a

    def viterbi_stats(self, i):
        st = CaptureViterbiStats()
        check(lib.lsdr_capture_batch_viterbi_stats(self.h, int(i), C.byref(st)))
        return st.as_dict()

    def bins(self, i, cap=4096):
        b = (C.c_int * cap)()
        n = C.c_uint()
        check(lib.lsdr_capture_batch_bins(self.h, i, b, cap, C.byref(n)))
        return list(b[:min(n.value, cap)])

    def notched(self, i, n):
        """The notched stream of capture i as the tiles of the last run saw it (test hook), n complex64 items."""
        d = self.ctx.alloc(int(n) * 8)
        check(lib.lsdr_capture_batch_notched(self.h, i, d.ptr, int(n)))
        out = self.ctx.download(d, np.complex64, int(n))
        d.free()
        return out

    def set_reports(self, period_samples):
        """Signal reports once per period_samples (cstln_receiver::meas_decimation; 0: off).  Not while a batch is in flight."""
        check(lib.lsdr_capture_reports_set(self.h, int(period_samples)))

    def reports(self, i):
        """Capture i's reports of the last batch, oldest first: dict(freq, ss, mer: float32 arrays; last: the same three behind the
        capture's last chunk, as a float32 array [freq, ss, mer])."""
        n, last = c_sz(), CaptureReport()
        check(lib.lsdr_capture_reports_get(self.h, int(i), None, 0, C.byref(n), C.byref(last)))
        buf = (CaptureReport * max(1, n.value))()
        check(lib.lsdr_capture_reports_get(self.h, int(i), buf, n.value, C.byref(n), C.byref(last)))
        a = np.frombuffer(buf, np.float32).reshape(-1, 4)[:n.value]
        return dict(freq=a[:, 0].copy(), ss=a[:, 1].copy(), mer=a[:, 2].copy(), last=np.array([last.freq, last.ss, last.mer], np.float32))

    def tile_time(self, enable):
        ms, n = C.c_float(), C.c_uint()
        check(lib.lsdr_capture_batch_tile_time(self.h, 1 if enable else 0, C.byref(ms), C.byref(n)))
        return ms.value, n.value


class HsBatch(_TailBatch):
    """lsdr_hs_batch: B independent cu8 captures, each from its first sample to TS by leandvb's `--hs` graph (fast_qpsk_receiver →
    dvb_deconvol_sync → mpeg_sync(fastlock) → deinterleaver → rs_decoder → derandomizer), in shared launches with every count on the
    device.  freq: the receiver's frequency bias in cycles per sample (FastQpsk's convention)."""
    _c, _what = "lsdr_hs_batch", "hs batch"

    def __init__(self, ctx, n_captures, max_samples, omega, freq=0.0, allow_drift=0, fastlock=0, tile_len=0, tile_warmup=0):
        self.ctx, self.n = ctx, int(n_captures)
        cfg = HsBatchCfg()
        cfg.n_captures, cfg.max_samples, cfg.omega, cfg.freq = self.n, int(max_samples), omega, freq
        cfg.allow_drift, cfg.fastlock, cfg.tile_len, cfg.tile_warmup = int(allow_drift), int(fastlock), tile_len, tile_warmup
        h = vp()
        check(lib.lsdr_hs_batch_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.freq = float(freq)
        self._attach(h, lib.lsdr_hs_batch_run_async, lib.lsdr_hs_each_run_async)

    def _fec_symbols(self):
        return HSYM_U8, self.symbols_ptr

    def symbols_ptr(self, i):
        """Device pointer of capture i's hard symbols, one per byte (None for i out of range)."""
        return lib.lsdr_hs_batch_symbols_dev(self.h, int(i))

    def symbols(self, i, n):
        """The first n hard symbols of capture i after a run (host)."""
        return self._fetch(self.symbols_ptr(i), n)


IN_ITEM_BYTES = {IN_CU8: 2, IN_CS8: 2, IN_CU16: 4, IN_CS16: 4, IN_CF32: 8}


class RecordingDecoder:
    """A recording of any length from its raw samples to one TS: cut into pieces of piece_samples that overlap by overlap_samples
    (recording_plan), decoded pieces_per_batch at a time as the captures of one batch (CaptureBatch, in either engine, or HsBatch with
    hs=True — each piece acquires anew), and the pieces' TS joined on the device (TsStitch, with `window` and `min_run`), the join between
    the last piece of one batch and the first of the next included.  tune: leandvb's --tune as Ftune/Fs in cycles per sample for every
    piece; None: estimated once, from the first piece (TuneEstimator; 0 where its quality is below TUNE_MIN_QUALITY); "pieces": every
    piece gets its own, estimated from its own first blocks by one TuneEstimator run in front of each batch — a piece below
    TUNE_MIN_QUALITY takes its left neighbour's (the recording's first piece: 0) — for recordings whose carrier wanders from piece to piece;
    within a piece it must still stay inside the tiles' window.
    decode / decode_file return (the TS's bytes, report): report = dict(pieces: [dict(first_sample, n_samples, result, keep: [start, end)
    of the piece's TS, ts: its bytes with piece_ts=True, head_in_front: see below)], joins: [dict(joined, run, end, next_start)] per adjacent pair, unjoined: the
    indices of the pairs that did not join, tune, tunes: the tune of every piece, packets).  The TS is the stitch's output with one exception: where the left piece of a join is kept
    from its first packet and holds fewer packets in front of the run than the right piece (it acquired late, behind a fade, beside a
    neighbour that started in the clear), the right piece's packets in front of the run go out in place of the left piece's: the left
    piece's record gains head_in_front (the packets taken from its neighbour) and dropped_in_front (its own, left out)."""

    def __init__(self, ctx, piece_samples, overlap_samples, pieces_per_batch, omega, fec=FEC12, viterbi=None, hs=False, in_format=IN_CU8,
                 in_scale=0.0, relock=0, tune=None, window=4096, min_run=8, piece_ts=False, **batch_kw):
        self.ctx, self.piece, self.overlap, self.B = ctx, int(piece_samples), int(overlap_samples), int(pieces_per_batch)
        recording_plan(0, self.piece, self.overlap)                     # (checks the two)
        if self.B < 1:
            raise LsdrError("recording: pieces_per_batch must be at least 1")
        if hs and (in_format != IN_CU8 or in_scale != 0.0 or fec != FEC12 or viterbi or relock):
            raise LsdrError("recording: hs=True decodes cu8 samples at rate 1/2, without viterbi= and relock=")
        self.in_format, self.in_scale, self.item = int(in_format), float(in_scale), IN_ITEM_BYTES[int(in_format)]
        self.tune, self.piece_ts, self.window, self.min_run = tune, bool(piece_ts), int(window), int(min_run)
        num, den = (1, 2) if hs else FEC_RATE[fec]
        # a piece's packets: its symbols carry 2·rate bits each, a packet is 204·8 of them; 1 % and 64 packets of room (omega is nominal)
        self.max_packets = int(1.01 * self.piece / float(omega) * 2 * num / den / 1632) + 64
        self._parts, self._bufs, self._est, self._est_pieces = [], [], None, None
        try:
            if hs:
                self.batch = self._own(HsBatch(ctx, self.B, self.piece, omega, **batch_kw))
            else:
                self.batch = self._own(CaptureBatch(ctx, self.B, self.piece, omega, fec=fec, viterbi=viterbi, in_format=in_format,
                                                    in_scale=in_scale, relock=0 if viterbi else relock, **batch_kw))
            self._make_stitcher(self.max_packets)
        except Exception:
            self.close()
            raise

    def _own(self, part):
        self._parts.append(part)
        return part

    def _make_stitcher(self, max_packets):
        """The stitcher of a batch's pieces behind slot 0, which holds the last piece of the batch before (self._carry: its TS, copied)."""
        old = getattr(self, "stitcher", None)
        self.stitcher = self._own(TsStitch(self.ctx, self.B + 1, max_packets, self.window, self.min_run))
        carry = self.ctx.alloc(max(max_packets, 1) * 188)
        if old:
            check(lib.lsdr_memcpy_d2d(self.ctx.h, carry.ptr, self._carry.ptr, self.max_packets * 188))
            self.ctx.sync()
            self._parts.remove(old)
            old.close()
            self._carry.free()
        self._carry, self.max_packets = carry, int(max_packets)

    def close(self):
        for p in reversed(self._parts):
            p.close()
        for b in self._bufs + ([self._carry] if getattr(self, "_carry", None) else []):
            b.free()
        for p in getattr(self, "_pinned", []):
            lib.lsdr_free_host(p)
        for e in (self._est, self._est_pieces):
            if e:
                e.close()
        self._parts, self._bufs, self._pinned, self._carry, self._est, self._est_pieces = [], [], [], None, None, None

    def plan(self, n_samples):
        """recording_plan with this object's piece and overlap."""
        return recording_plan(n_samples, self.piece, self.overlap)

    def batch_span(self, pieces):
        """The samples [first, end) that a batch of consecutive pieces reads."""
        return pieces[0][0], pieces[-1][0] + pieces[-1][1]

    def _tune_of(self, ptr, n):
        if self.tune == "pieces":
            return "pieces"
        if self.tune is not None:
            return float(self.tune)
        if not self._est:
            self._est = TuneEstimator(self.ctx, 1, self.in_format, self.in_scale)
        e = self._est.estimate([ptr], [n])[0]
        return e["tune"] if e["quality"] >= TUNE_MIN_QUALITY else 0.0

    def _start(self):
        return dict(pieces=[], joins=[], unjoined=[], tune=None, tunes=[], packets=0), [], None

    def _piece_tunes(self, ptrs, lengths, left):
        """Every piece's own tune (one TuneEstimator run over the batch); a piece without a line takes its left neighbour's, the batch's
        first piece `left`."""
        if not self._est_pieces:
            self._est_pieces = TuneEstimator(self.ctx, self.B, self.in_format, self.in_scale)
        tunes = []
        for e in self._est_pieces.estimate(ptrs, lengths):
            left = e["tune"] if e["quality"] >= TUNE_MIN_QUALITY else left
            tunes.append(left)
        return tunes

    def _batch_async(self, base_ptr, first_sample, pieces, tune, report):
        """Queues the decode of consecutive pieces; base_ptr holds the recording from first_sample on."""
        ptrs = [vp(base_ptr + (s - first_sample) * self.item) if n else None for s, n in pieces] + [None] * (self.B - len(pieces))
        lengths = [n for _, n in pieces] + [0] * (self.B - len(pieces))
        if tune == "pieces":
            tune = self._piece_tunes(ptrs, lengths, report["tunes"][-1] if report["tunes"] else 0.0)
        self.batch.run_each_async(ptrs, lengths, tune)
        report["tunes"] += [float(t) for t in (tune[:len(pieces)] if isinstance(tune, list) else [tune] * len(pieces))]

    def _batch_finish(self, pieces, last, report, out, carry):
        """Waits for the batch, joins its pieces behind the carried one and appends what is final to `out`: everything in front of the
        batch's last piece, whose own end the next batch's first piece decides (last: there is none).  Returns the new carry,
        (its packets, the start of its kept range, its index among the pieces)."""
        res = self.batch.wait()[:len(pieces)]
        n = [int(r["ts_packets"]) for r in res]
        if max(n + [0]) > self.max_packets:
            self._make_stitcher(max(n))
        ts_dev = self.batch._fn("ts_dev")
        ptrs = [self._carry.ptr if carry and carry[0] else None] + [ts_dev(self.batch.h, i) if n[i] else None for i in range(len(pieces))]
        ptrs += [None] * (self.B - len(pieces))
        joins, keep = self.stitcher.stitch_records(ptrs, [carry[0] if carry else 0] + n + [0] * (self.B - len(pieces)))
        first = len(report["pieces"])
        for i, ((s, ns), r) in enumerate(zip(pieces, res)):
            rec = dict(first_sample=s, n_samples=ns, result=r, keep=[keep[i + 1]["start"], keep[i + 1]["end"]])
            if self.piece_ts:
                rec["ts"] = self.batch._fetch(ts_dev(self.batch.h, i), n[i] * 188).tobytes()
            report["pieces"].append(rec)
        skip = 0
        if carry:                                                        # slot 0 is kept from 0 there; its range starts where its own batch said
            skip = min(carry[1], keep[0]["end"])
            report["pieces"][carry[2]]["keep"] = [carry[1], max(carry[1], keep[0]["end"])]
        report["joins"] += joins[0 if carry else 1:len(pieces)]
        final = self.stitcher.packets if last else keep[len(pieces)]["out_offset"]
        # A join drops what the right piece holds in front of the run: the left piece holds it too — unless the left piece acquired late
        # (behind a fade) beside a right neighbour that started in the clear.  Where the left piece is kept from its first packet and has
        # fewer packets in front of the run than the right piece, the right piece's are the ones that go out there.
        starts, pos = [carry[1] if carry else 0] + [k["start"] for k in keep[1:]], skip
        for i in range(0 if carry else 1, len(pieces)):                  # the join of slot i and slot i + 1, which is piece i of the batch
            j = joins[i]
            head, mine = j["next_start"] - j["run"], j["end"] - j["run"]
            if j["joined"] and starts[i] == 0 and head > mine:
                at = keep[i]["out_offset"]
                if at > pos:
                    out.append(self.batch._fetch(vp(self.stitcher.out_ptr() + pos * 188), (at - pos) * 188).tobytes())
                out.append(self.batch._fetch(ts_dev(self.batch.h, i), head * 188).tobytes())
                report["pieces"][first + i - 1].update(head_in_front=head, dropped_in_front=mine)
                pos = at + mine
        if final > pos:
            out.append(self.batch._fetch(vp(self.stitcher.out_ptr() + pos * 188), (final - pos) * 188).tobytes())
        if last:
            return None
        k = len(pieces) - 1
        if n[k]:
            check(lib.lsdr_memcpy_d2d(self.ctx.h, self._carry.ptr, ts_dev(self.batch.h, k), n[k] * 188))
        return n[k], keep[k + 1]["start"], first + k

    def _finish(self, report, out, tune):
        ts = b"".join(out)
        report["unjoined"], report["tune"], report["packets"] = unjoined(report["joins"]), tune, len(ts) // 188
        return ts, report

    def decode(self, ptr, n_samples):
        """A recording of n_samples items resident in device memory at ptr (16-byte aligned): (TS bytes, report)."""
        ptr = ptr.value if isinstance(ptr, vp) else int(ptr)
        plan = self.plan(n_samples)
        report, out, carry = self._start()
        tune = self._tune_of(vp(ptr), plan[0][1])
        for g in range(0, len(plan), self.B):
            pieces = plan[g:g + self.B]
            self._batch_async(ptr, 0, pieces, tune, report)
            carry = self._batch_finish(pieces, g + self.B >= len(plan), report, out, carry)
        return self._finish(report, out, tune)

    def decode_file(self, path):
        """A recording in a file of in_format items, streamed through two pinned host buffers and two device buffers of one batch's
        samples each: while a batch decodes, the next one is read and uploaded on the context's upload stream; consecutive batches share
        overlap_samples of input.  One host thread.  (TS bytes, report)."""
        n_samples = os.path.getsize(path) // self.item
        plan = self.plan(n_samples)
        groups = [plan[g:g + self.B] for g in range(0, len(plan), self.B)]
        cap = max((self.B - 1) * (self.piece - self.overlap) + self.piece, 1) * self.item
        if not self._bufs:
            self._bufs = [self.ctx.alloc(cap) for _ in range(2)]
            self._pinned = []
            for _ in range(2):
                p = vp()
                check(lib.lsdr_malloc_host(cap, C.byref(p)))
                self._pinned.append(p)
        host = [np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (cap,)) for p in self._pinned]
        report, out, carry = self._start()
        with open(path, "rb", buffering=0) as f:
            def upload(g):
                first, end = self.batch_span(groups[g])
                nbytes = (end - first) * self.item
                f.seek(first * self.item)
                view, got = memoryview(host[g % 2])[:nbytes], 0
                while got < nbytes:
                    k = f.readinto(view[got:])
                    if not k:
                        break
                    got += k
                if got != nbytes:
                    raise LsdrError(f"recording: {path}: read {got} of {nbytes} bytes at sample {first}")
                check(lib.lsdr_copy_h2d_async(self.ctx.h, self._bufs[g % 2].ptr, self._pinned[g % 2], nbytes))
            upload(0)
            check(lib.lsdr_copy_fence(self.ctx.h))
            tune = self._tune_of(vp(self._bufs[0].ptr), plan[0][1])
            for g, pieces in enumerate(groups):
                check(lib.lsdr_copy_fence(self.ctx.h))
                self._batch_async(self._bufs[g % 2].ptr, pieces[0][0], pieces, tune, report)
                if g + 1 < len(groups):
                    upload(g + 1)                                        # (batch g − 1, the last reader of these two buffers, was waited for)
                carry = self._batch_finish(pieces, g + 1 == len(groups), report, out, carry)
        return self._finish(report, out, tune)


def resample_design(omega, rolloff=0.35, rej=10.0, decim=0):
    """leandvb's --resample filter for omega = Fs/Fm (lsdr_resample_design, leandvb.cc:353-378): (decim, coeffs).  decim 0: (int)(omega/4),
    at least 1."""
    d, n = C.c_uint(), C.c_uint()
    lib.lsdr_resample_design(omega, rolloff, rej, int(decim), C.byref(d), None, 0, C.byref(n))       # the size first
    if not n.value:
        raise LsdrError(f"lsdr error: {lib.lsdr_last_error().decode()}")
    out = np.empty(n.value, np.float32)
    check(lib.lsdr_resample_design(omega, rolloff, rej, int(decim), C.byref(d), _np(out), len(out), C.byref(n)))
    return d.value, out[:n.value]


class ResampleBatch:
    """lsdr_resample_batch: leandvb's --derotate --resample for n_captures captures in one launch — each capture of in_format items, with
    its own length and carrier offset, converted, derotated by (int)(tune·65536)/65536 cycles per sample, low-passed by the real taps
    `coeffs` and decimated by `decim` into a cf32 stream (what CaptureBatch(in_format=IN_CF32, in_scale=1) decodes)."""

    def __init__(self, ctx, n_captures, max_samples, coeffs, decim, in_format=IN_CU8, in_scale=0.0):
        self.ctx, self.n, self.h = ctx, int(n_captures), None
        self.coeffs = np.ascontiguousarray(coeffs, np.float32)
        self.decim = int(decim)
        cfg = ResampleBatchCfg()
        cfg.n_captures, cfg.max_samples, cfg.in_format, cfg.in_scale = self.n, int(max_samples), int(in_format), float(in_scale)
        cfg.ncoeffs, cfg.coeffs_host, cfg.decim = len(self.coeffs), self.coeffs.ctypes.data, self.decim
        h = vp()
        check(lib.lsdr_resample_batch_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h
        self.tile = lib.lsdr_resample_batch_tile(h)
        self._res = (ResampleResult * max(self.n, 1))()

    def close(self):
        if self.h:
            lib.lsdr_resample_batch_destroy(self.h)
            self.h = None

    def produced(self, n_samples):
        """What a capture of n_samples items produces: (n − N) // D, 0 below N."""
        return max(0, int(n_samples) - len(self.coeffs)) // self.decim

    def _args(self, ptrs, lengths, tune, outs):
        n = [int(v) for v in lengths]
        t = [float(tune)] * self.n if np.isscalar(tune) else [float(v) for v in tune]
        if not (len(n) == len(t) == len(ptrs) == len(outs) == self.n):
            raise LsdrError(f"resample batch: {len(ptrs)} pointers, {len(n)} lengths, {len(t)} tunes and {len(outs)} outputs for {self.n} captures")
        e = (CaptureEach * max(self.n, 1))()
        for i in range(self.n):
            e[i].n_samples, e[i].tune = n[i], t[i]
        as_vp = lambda ps: (vp * self.n)(*[p if isinstance(p, vp) else vp(p) for p in ps])
        return as_vp(ptrs), e, as_vp(outs)

    def run_async(self, ptrs, lengths, tune, outs, cap_out):
        """Queues the run: ptrs / outs device pointers per capture (None where there are no samples / no outputs), lengths in items, tune
        in cycles per sample (a scalar or one per capture), cap_out cf32 items of room behind every output pointer."""
        p, e, o = self._args(ptrs, lengths, tune, outs)
        check(lib.lsdr_resample_batch_run_async(self.h, p, e, o, int(cap_out)))

    def wait(self):
        """[dict(consumed, produced, ifreq, applied)] per capture."""
        check(lib.lsdr_resample_batch_wait(self.h, self._res))
        return [dict(consumed=int(r.consumed), produced=int(r.produced), ifreq=int(r.ifreq), applied=float(r.applied)) for r in self._res[:self.n]]

    def run(self, ptrs, lengths, tune, outs, cap_out):
        self.run_async(ptrs, lengths, tune, outs, cap_out)
        return self.wait()


class SpectrumBatch:
    """lsdr_spectrum_batch: leandvb's --cnr (cnr_fft, sdr.h:1273-1345) and --fd-spectrum (spectrum, sdr.h:1347-1404) for n_captures
    captures in shared launches — each capture of in_format items with its own length and band centre; whole blocks of nfft samples, a row
    every `decimation` samples (>= nfft; == nfft: every block).  bandwidth > 0 (Fm/Fs, at most 0.25): one CNR value in dB per row.
    rows=True: every row's averaged power is kept (rows_db on the host in dB, fftshifted; rows_linear_dev on the device)."""

    def __init__(self, ctx, n_captures, max_samples, nfft=4096, decimation=1048576, kavg=0.1, bandwidth=0.0, rows=False, in_format=IN_CU8,
                 in_scale=1.0, slab_rows=0, stages_per_pass=0):
        self.ctx, self.n, self.h = ctx, int(n_captures), None
        self.nfft, self.decimation, self.bandwidth, self.rows = int(nfft), int(decimation), float(bandwidth), bool(rows)
        cfg = SpectrumBatchCfg()
        cfg.n_captures, cfg.max_samples, cfg.in_format, cfg.in_scale = self.n, int(max_samples), int(in_format), float(in_scale)
        cfg.nfft, cfg.decimation, cfg.kavg, cfg.bandwidth = self.nfft, self.decimation, float(kavg), self.bandwidth
        cfg.emit_rows, cfg.slab_rows, cfg.stages_per_pass = int(self.rows), int(slab_rows), int(stages_per_pass)
        h = vp()
        check(lib.lsdr_spectrum_batch_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h
        self.max_rows = int(lib.lsdr_spectrum_batch_max_rows(h))
        self.slab_rows = int(lib.lsdr_spectrum_batch_slab_rows(h))
        self._res = (SpectrumResult * max(self.n, 1))()

    @classmethod
    def cnr(cls, ctx, n_captures, max_samples, omega, Fs_over_Finfo, **kw):
        """leandvb --cnr for omega = Fs/Fm: cnr_fft(bandwidth = Fm/Fs) with a value every decimation(Fs, 1 Hz) = (int)Fs samples
        (leandvb.cc:327-328); Fs_over_Finfo is Fs over the 1 Hz of information rate."""
        kw.setdefault("nfft", 4096)
        return cls(ctx, n_captures, max_samples, decimation=max(int(Fs_over_Finfo), 1), bandwidth=1.0 / float(omega), **kw)

    @classmethod
    def spectrum(cls, ctx, n_captures, max_samples, Fs_over_Finfo, **kw):
        """leandvb --fd-spectrum: spectrum<f32> (1024 bins) with kavg 0.5 and a row every (int)Fs samples (leandvb.cc:339-342)."""
        kw.setdefault("kavg", 0.5)
        return cls(ctx, n_captures, max_samples, nfft=1024, decimation=max(int(Fs_over_Finfo), 1), rows=True, **kw)

    def close(self):
        if self.h:
            lib.lsdr_spectrum_batch_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _args(self, ptrs, lengths, center):
        n = [int(v) for v in lengths]
        t = [0.0 if center is None else float(center)] * self.n if center is None or np.isscalar(center) else [float(v) for v in center]
        if not (len(n) == len(t) == len(ptrs) == self.n):
            raise LsdrError(f"spectrum batch: {len(ptrs)} pointers, {len(n)} lengths and {len(t)} centres for {self.n} captures")
        e = (CaptureEach * max(self.n, 1))()
        for i in range(self.n):
            e[i].n_samples, e[i].tune = n[i], t[i]
        return (vp * self.n)(*[p if isinstance(p, vp) else vp(p) for p in ptrs]), e

    def run_async(self, ptrs, lengths, center=None):
        """Queues the run: device pointers per capture (None where there are no samples), lengths in items, center the band centre in
        cycles per sample (a scalar or one per capture; None: 0)."""
        check(lib.lsdr_spectrum_batch_run_async(self.h, *self._args(ptrs, lengths, center)))

    def wait(self):
        """[dict(consumed, rows, icf)] per capture."""
        check(lib.lsdr_spectrum_batch_wait(self.h, self._res))
        return [dict(consumed=int(r.consumed), rows=int(r.rows), icf=int(r.icf)) for r in self._res[:self.n]]

    def cnr_db(self, i):
        """Capture i's CNR values in dB, one per row (float32)."""
        out, n = np.empty(max(int(self._res[i].rows), 1), np.float32), c_sz()
        check(lib.lsdr_spectrum_batch_cnr(self.h, int(i), _np(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def rows_db(self, i):
        """Capture i's rows in dB as spectrum<f32> writes them (float32 [rows, nfft])."""
        out, n = np.empty((max(int(self._res[i].rows), 1), self.nfft), np.float32), c_sz()
        check(lib.lsdr_spectrum_batch_rows_db(self.h, int(i), _np(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def rows_linear_dev(self, i):
        """Device pointer of capture i's rows as linear averaged power, [rows, nfft] float32 in FFT order (None without rows=True)."""
        return lib.lsdr_spectrum_batch_rows_dev(self.h, int(i))

    def rows_linear(self, i):
        """rows_linear_dev(i)'s rows of the last run on the host (float32 [rows, nfft])."""
        out = np.empty((int(self._res[i].rows), self.nfft), np.float32)
        if out.size:
            check(lib.lsdr_memcpy_d2h(self.ctx.h, _np(out), vp(self.rows_linear_dev(i)), out.nbytes))
            self.ctx.sync()
        return out

    def run(self, ptrs, lengths, center=None):
        """One run, synchronously: per capture dict(consumed, rows, icf, cnr: float32[rows] (empty without bandwidth), rows_db: float32[rows, nfft] | None)."""
        self.run_async(ptrs, lengths, center)
        res = self.wait()
        for i, r in enumerate(res):
            r["cnr"] = self.cnr_db(i) if self.bandwidth > 0 else np.empty(0, np.float32)
            r["rows_db"] = self.rows_db(i) if self.rows else None
        return res


class ResampledDecoder:
    """Oversampled captures (omega = Fs/Fm above the batch decoders' 8) from their raw samples to TS: estimate every capture's carrier
    offset (TuneEstimator on the raw samples), derotate + low-pass + decimate (ResampleBatch, leandvb's --derotate --resample with
    resample_design's filter), estimate what is left on the decimated streams (TuneEstimator(IN_CF32)), decode them
    (CaptureBatch(in_format=IN_CF32, in_scale=1) at omega / decim with the fine estimates as per-capture tunes).  QPSK; |offset| < 1/8 cycle
    per raw sample where it is estimated.  The converted samples must meet the level contract (RMS near 75): the taps have DC gain 1.
    The decoder's tiles default to 896 symbols of warm-up and eight times that per tile (tile_warmup= / tile_len= in decimated samples
    override them): the capture batch's own defaults count samples and are too short at omega 4 … 8.
    anf=1 runs the decoder's notch on the DECIMATED stream, where leandvb's auto_notch sees the raw one (it sits in front of the
    rotator): interferers the low-pass removed are not there to be found, and the notch's bins are those of the decimated rate."""

    def __init__(self, ctx, n_captures, max_samples, omega, in_format=IN_CU8, in_scale=0.0, fec=FEC12, viterbi=None, anf=0, blocks=8,
                 rolloff=0.35, rej=10.0, decim=0, cnr_decimation=8 * 4096, relock=0, **batch_kw):
        self.ctx, self.n, self.max_samples = ctx, int(n_captures), int(max_samples)
        if relock and not viterbi:                                       # (the Viterbi engine searches its alignment in front of the tail)
            batch_kw["relock"] = relock
        self.in_format, self.cnr_decimation, self.measure = in_format, int(cnr_decimation), None
        self.decim, self.coeffs = resample_design(omega, rolloff, rej, decim)
        self.omega_out = float(omega) / self.decim
        self.cap_out = max(1, (self.max_samples - len(self.coeffs)) // self.decim)
        # the decoder's tiles: 896 symbols of warm-up, tiles eight times that.  The capture batch's default of 512 samples is 64 … 128
        # symbols at omega_out 4 … 8 and leaves seams unreconciled there (DESIGN.md §4.9 has the measurements)
        warm = -(-int(896 * self.omega_out) // 128) * 128
        batch_kw.setdefault("tile_warmup", warm)
        batch_kw.setdefault("tile_len", -(-8 * batch_kw["tile_warmup"] // 2048) * 2048)
        self._parts, self._outs = [], []
        try:
            self.est_raw = self._own(TuneEstimator(ctx, self.n, in_format, in_scale, blocks))
            self.resampler = self._own(ResampleBatch(ctx, self.n, self.max_samples, self.coeffs, self.decim, in_format, in_scale))
            self.est_fine = self._own(TuneEstimator(ctx, self.n, IN_CF32, 1.0, blocks))
            self.batch = self._own(CaptureBatch(ctx, self.n, self.cap_out, self.omega_out, fec=fec, anf=anf, viterbi=viterbi, in_format=IN_CF32,
                                                in_scale=1.0, **batch_kw))
            self._outs = [ctx.alloc(self.cap_out * 8) for _ in range(self.n)]
        except Exception:
            self.close()
            raise

    def _own(self, part):
        self._parts.append(part)
        return part

    def close(self):
        for p in reversed(self._parts):
            p.close()
        for b in self._outs:
            b.free()
        self._parts, self._outs, self.measure = [], [], None

    def outputs(self, i, n):
        """The first n items of capture i's decimated stream after a decode (host, complex64)."""
        return self.ctx.download(self._outs[i], np.complex64, int(n))

    def decode(self, ptrs, lengths, tune=None, fine=True, min_quality=TUNE_MIN_QUALITY, cnr=False):
        """(results, [TS bytes per capture], info).  tune: None = estimated from the raw samples (0 where the quality is below min_quality),
        else cycles per raw sample, a scalar or one per capture.  fine=False, or a fine quality below min_quality: the decoder's tune is what
        the derotation left by construction, (tune − ifreq/65536)·decim.  info[i] = dict(raw: the raw estimate or None, tune_raw, ifreq,
        applied, fine: the fine estimate or None, tune: the decoder's, produced).
        cnr=True: the decimated streams are measured as well, in front of the decode and apart from it — SpectrumBatch, cnr_fft with
        bandwidth decim/omega around the decoder's tune, a value every cnr_decimation decimated samples; info[i] gains cnr (float32, dB,
        one value per row) and cnr_center.  It needs omega / decim >= 4 (cnr_fft's own limit)."""
        raw = [None] * self.n
        if tune is None:
            raw = self.est_raw.estimate(ptrs, lengths)
            t_raw = [e["tune"] if e["quality"] >= min_quality else 0.0 for e in raw]
        else:
            t_raw = [float(tune)] * self.n if np.isscalar(tune) else [float(v) for v in tune]
        outs = [b.ptr for b in self._outs]
        rs = self.resampler.run(ptrs, lengths, t_raw, outs, self.cap_out)
        produced = [r["produced"] for r in rs]
        t_dec = [(t - r["applied"]) * self.decim for t, r in zip(t_raw, rs)]
        est = [None] * self.n
        if fine:
            est = self.est_fine.estimate(outs, produced)
            t_dec = [e["tune"] if e["quality"] >= min_quality else t for e, t in zip(est, t_dec)]
        measured = None
        if cnr:
            if self.measure is None:
                self.measure = self._own(SpectrumBatch(self.ctx, self.n, self.cap_out, nfft=4096, decimation=self.cnr_decimation,
                                                       bandwidth=1.0 / self.omega_out, in_format=IN_CF32, in_scale=1.0))
            measured = self.measure.run(outs, produced, t_dec)
        res, ts = self.batch.decode_each(outs, produced, t_dec)
        info = [dict(raw=raw[i], tune_raw=t_raw[i], ifreq=rs[i]["ifreq"], applied=rs[i]["applied"], fine=est[i], tune=t_dec[i], produced=produced[i])
                for i in range(self.n)]
        if measured is not None:
            for i in range(self.n):
                info[i]["cnr"], info[i]["cnr_center"] = measured[i]["cnr"], t_dec[i]
        return res, ts, info


class TuneTracker:
    """lsdr_tune_track: the carrier offset of each of n_captures captures ALONG its length (QPSK: TuneEstimator's line of the fourth power
    on frames of `blocks` blocks every `hop` samples and at the capture's end, gated to ± span bins around the last accepted frame, frames
    below min_quality held).  max_frames: of one capture (0: 256)."""

    def __init__(self, ctx, n_captures, in_format=IN_CU8, in_scale=0.0, blocks=4, hop=65536, span=64, min_quality=TUNE_MIN_QUALITY, max_frames=0):
        self.ctx, self.n, self.h = ctx, int(n_captures), None
        cfg = TuneTrackCfg()
        cfg.n_captures, cfg.in_format, cfg.in_scale, cfg.blocks, cfg.hop = self.n, int(in_format), float(in_scale), int(blocks), int(hop)
        cfg.span, cfg.min_quality, cfg.max_frames = int(span), float(min_quality), int(max_frames)
        h = vp()
        check(lib.lsdr_tune_track_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h
        self.max_frames = int(lib.lsdr_tune_track_max_frames(h))
        self._sum = (TrackSummary * self.n)()
        self._frames = (TrackFrame * (self.n * self.max_frames))()

    def close(self):
        if self.h:
            lib.lsdr_tune_track_destroy(self.h)
            self.h = None

    def _args(self, ptrs, lengths):
        n = [int(v) for v in lengths]
        if len(n) != self.n or len(ptrs) != self.n:
            raise LsdrError(f"tune tracker: {len(ptrs)} pointers and {len(n)} lengths for {self.n} captures")
        return (vp * self.n)(*[p if isinstance(p, vp) else vp(p) for p in ptrs]), (c_sz * self.n)(*n)

    def run_async(self, ptrs, lengths):
        """Queues the track of every capture's first lengths[i] items; a pointer may be None where the length is 0."""
        check(lib.lsdr_tune_track_run_async(self.h, *self._args(ptrs, lengths)))

    def wait(self):
        check(lib.lsdr_tune_track_wait(self.h, self._sum, self._frames))
        out = []
        for i, s in enumerate(self._sum):
            d = s.as_dict()
            d["frames"] = [self._frames[i * self.max_frames + k].as_dict() for k in range(int(s.frames))]
            out.append(d)
        return out

    def track(self, ptrs, lengths):
        """One run, synchronously: [dict(accepted, tune_first, tune_last, tune_min, tune_max, quality_min, frames: [dict(center, tune,
        quality, bin, held, power [l, c, r], mean_power)])] per capture."""
        self.run_async(ptrs, lengths)
        return self.wait()


def track_knots(frames):
    """[(center, tune)] of a track's accepted frames: the knots DerotateBatch takes."""
    return [(f["center"], f["tune"]) for f in frames if not f["held"]]


class DerotateBatch:
    """lsdr_derotate_batch: a carrier track, GIVEN per capture as knots [(sample, tune)], taken out of n_captures captures in one launch:
    each capture of in_format items, with its own length, converted and multiplied by exp(−j2π·φ(n)) into a cf32 stream (what
    CaptureBatch(in_format=IN_CF32, in_scale=1) decodes with tune 0).  The frequency runs linearly between the knots, with the first and the
    last slope outside them; no knots: the capture passes through converted."""

    def __init__(self, ctx, n_captures, max_samples, max_knots, in_format=IN_CU8, in_scale=0.0):
        self.ctx, self.n, self.h = ctx, int(n_captures), None
        cfg = DerotateBatchCfg()
        cfg.n_captures, cfg.in_format, cfg.in_scale = self.n, int(in_format), float(in_scale)
        cfg.max_knots, cfg.max_samples = int(max_knots), int(max_samples)
        h = vp()
        check(lib.lsdr_derotate_batch_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.lsdr_derotate_batch_destroy(self.h)
            self.h = None

    def _args(self, ptrs, lengths, knots, outs):
        n = [int(v) for v in lengths]
        if not (len(n) == len(ptrs) == len(knots) == len(outs) == self.n):
            raise LsdrError(f"derotate batch: {len(ptrs)} pointers, {len(n)} lengths, {len(knots)} tracks and {len(outs)} outputs for {self.n} captures")
        e = (DerotateEach * self.n)()
        keep = []
        for i in range(self.n):
            k = (TrackKnot * max(len(knots[i]), 1))()
            for j, (s, t) in enumerate(knots[i]):
                k[j].sample, k[j].tune = int(s), float(t)
            keep.append(k)
            e[i].n_samples, e[i].knots, e[i].n_knots = n[i], k, len(knots[i])
        as_vp = lambda ps: (vp * self.n)(*[p if isinstance(p, vp) else vp(p) for p in ps])
        return as_vp(ptrs), e, as_vp(outs), keep

    def run_async(self, ptrs, lengths, knots, outs):
        """Queues the run: ptrs / outs device pointers per capture (None where there are no samples; outs 16-byte aligned with room for
        lengths[i] cf32 items), knots a list of (sample, tune) per capture."""
        p, e, o, keep = self._args(ptrs, lengths, knots, outs)
        check(lib.lsdr_derotate_batch_run_async(self.h, p, e, o))

    def wait(self):
        check(lib.lsdr_derotate_batch_wait(self.h))

    def run(self, ptrs, lengths, knots, outs):
        self.run_async(ptrs, lengths, knots, outs)
        self.wait()


class TrackedDecoder:
    """Captures whose carrier moves by more than the batch decoders' tuning window, from their raw samples to TS: track every capture's
    carrier (TuneTracker, with tracker_kw: blocks, hop, span, min_quality), take the track out of the samples (DerotateBatch, into cf32
    buffers of this object's: 8 bytes of device memory per sample), decode the result (CaptureBatch(in_format=IN_CF32, in_scale=1) in
    either engine, with tune 0; batch_kw: its further arguments; relock is the default engine's and is not passed on with viterbi=, which
    searches its alignment in front of the tail).  A capture with no accepted frame is derotated by nothing.  QPSK,
    |offset| < 1/8 cycle per sample; what the track leaves of the carrier must fit the tiles' window."""

    def __init__(self, ctx, n_captures, max_samples, omega, fec=FEC12, viterbi=None, in_format=IN_CU8, in_scale=0.0, relock=0, anf=1,
                 batch_kw=None, **tracker_kw):
        self.ctx, self.n, self.max_samples = ctx, int(n_captures), int(max_samples)
        blocks, hop = int(tracker_kw.get("blocks", 4)) or 4, int(tracker_kw.get("hop", 65536)) or 65536
        tracker_kw.setdefault("max_frames", max(1, max(0, self.max_samples - blocks * 4096) // hop + 2))
        batch_kw = dict(batch_kw or {})
        if relock and not viterbi:
            batch_kw["relock"] = relock
        self._parts, self._outs = [], []
        try:
            self.tracker = self._own(TuneTracker(ctx, self.n, in_format, in_scale, **tracker_kw))
            self.derotator = self._own(DerotateBatch(ctx, self.n, self.max_samples, self.tracker.max_frames, in_format, in_scale))
            self.batch = self._own(CaptureBatch(ctx, self.n, self.max_samples, omega, fec=fec, anf=anf, viterbi=viterbi, in_format=IN_CF32,
                                                in_scale=1.0, **batch_kw))
            self._outs = [ctx.alloc(max(self.max_samples, 2) * 8) for _ in range(self.n)]
        except Exception:
            self.close()
            raise

    def _own(self, part):
        self._parts.append(part)
        return part

    def close(self):
        for p in reversed(self._parts):
            p.close()
        for b in self._outs:
            b.free()
        self._parts, self._outs = [], []

    def outputs(self, i, n):
        """The first n items of capture i's derotated stream after a decode (host, complex64)."""
        return self.ctx.download(self._outs[i], np.complex64, int(n))

    def decode(self, ptrs, lengths):
        """(results, [TS bytes per capture], tracks): tracks[i] is TuneTracker.track's record of capture i."""
        tracks = self.tracker.track(ptrs, lengths)
        outs = [b.ptr for b in self._outs]
        self.derotator.run(ptrs, lengths, [track_knots(t["frames"]) for t in tracks], outs)
        res, ts = self.batch.decode_each(outs, lengths, 0.0)
        return res, ts, tracks


class CarrierScan:
    """lsdr_carrier_scan: the carriers of each of n_captures wideband captures, read from the averaged power spectrum (Hann-windowed blocks
    of 4096 samples, `blocks` of them, spread over the whole capture with spread=True): where they are, how wide, how far above the floor.
    The centres are what ResampleBatch's tune takes (the same pointer once per carrier), omega what resample_design takes."""

    def __init__(self, ctx, n_captures, in_format=IN_CU8, in_scale=0.0, blocks=64, spread=True, smooth=8, threshold_db=3.0, min_bins=0,
                 max_carriers=32):
        self.ctx, self.n, self.h = ctx, int(n_captures), None
        cfg = CarrierScanCfg()
        cfg.n_captures, cfg.in_format, cfg.in_scale, cfg.blocks, cfg.spread = self.n, int(in_format), float(in_scale), int(blocks), int(bool(spread))
        cfg.smooth, cfg.threshold_db, cfg.min_bins, cfg.max_carriers = int(smooth), float(threshold_db), int(min_bins), int(max_carriers)
        h = vp()
        check(lib.lsdr_carrier_scan_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h
        self.max_carriers = int(max_carriers) or 32
        self._sum = (ScanSummary * self.n)()
        self._car = (ScanCarrier * (self.n * self.max_carriers))()

    def close(self):
        if self.h:
            lib.lsdr_carrier_scan_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _args(self, ptrs, lengths):
        n = [int(v) for v in lengths]
        if len(n) != self.n or len(ptrs) != self.n:
            raise LsdrError(f"carrier scan: {len(ptrs)} pointers and {len(n)} lengths for {self.n} captures")
        return (vp * self.n)(*[p if isinstance(p, vp) else vp(p) for p in ptrs]), (c_sz * self.n)(*n)

    def run_async(self, ptrs, lengths):
        """Queues the scan of every capture's first lengths[i] items; a pointer may be None where the length is 0."""
        check(lib.lsdr_carrier_scan_run_async(self.h, *self._args(ptrs, lengths)))

    def wait(self):
        check(lib.lsdr_carrier_scan_wait(self.h, self._sum, self._car))
        out = []
        for i, s in enumerate(self._sum):
            d = s.as_dict()
            d["carriers"] = [self._car[i * self.max_carriers + j].as_dict() for j in range(d["listed"])]
            out.append(d)
        return out

    def scan(self, ptrs, lengths):
        """One run, synchronously: per capture dict(blocks, stride, found, listed, saturated, floor, threshold, carriers=[dict(center,
        bandwidth, omega, level, cnr_db, plateau, first_bin, bins, weak)]), the carriers by start frequency from −1/2 upward."""
        self.run_async(ptrs, lengths)
        return self.wait()

    def spectrum(self, i):
        """Capture i's summed power spectrum P of the last run (float32[4096], FFT order)."""
        ptr = lib.lsdr_carrier_scan_spectrum_dev(self.h, int(i))
        if not ptr:
            raise LsdrError("carrier scan: no such capture")
        out = np.empty(4096, np.float32)
        check(lib.lsdr_memcpy_d2h(self.ctx.h, _np(out), vp(ptr), out.nbytes))
        self.ctx.sync()
        return out


def group_carriers(carriers, rtol=0.05):
    """The carriers of one scan sorted by width: ([(omega, [carrier indices])], [indices of the weak ones]) from CarrierScan's records.
    Taken in ascending omega, a carrier joins the group whose first member it is within rtol of, and a group's omega is that member's — the
    caller makes one ResampleBatch (one filter, one decimation) per group.  Weak carriers, whose width is their run's and no symbol rate,
    come back in their own list."""
    good = sorted((i for i, c in enumerate(carriers) if not c["weak"] and c["omega"] > 0), key=lambda i: (carriers[i]["omega"], i))
    weak = [i for i in range(len(carriers)) if i not in set(good)]
    groups = []
    for i in good:
        if groups and carriers[i]["omega"] <= groups[-1][0] * (1.0 + rtol):
            groups[-1][1].append(i)
        else:
            groups.append((carriers[i]["omega"], [i]))
    return [(om, sorted(g)) for om, g in groups], weak


class WidebandDecoder:
    """One wideband capture holding several QPSK DVB-S carriers, from its raw samples to one TS per carrier, out of existing objects:
    CarrierScan finds the carriers; group_carriers sorts them by width; per group one ResampleBatch takes the same pointer once per carrier
    with the centres as tunes (resample_design's filter and decimation for the group's omega — also at decimation 1: the other carriers
    have to be filtered away); RateEstimator(IN_CF32) reads every decimated stream's symbol rate inside ±10 % of the scan's;
    group_by_omega sorts them again; per subgroup TuneEstimator(IN_CF32) and CaptureBatch(in_format=IN_CF32, in_scale=1) at the estimated
    omega decode them.  The objects are made per call and closed; every launch is shared by a group's carriers."""

    def __init__(self, ctx, max_samples, in_format=IN_CU8, in_scale=0.0, fec=FEC12, viterbi=None, max_carriers=8, relock=0, **scan_kw):
        self.ctx, self.max_samples, self.in_format, self.in_scale = ctx, int(max_samples), in_format, in_scale
        self.relock = 0 if viterbi else int(relock)                      # CaptureBatch(relock=), default engine only
        self.fec, self.viterbi, self.max_carriers, self.scan_kw = fec, viterbi, int(max_carriers), scan_kw
        self.steps = {}

    def _timed(self, step, t0):
        self.steps[step] = self.steps.get(step, 0.0) + time.perf_counter() - t0

    def decode(self, ptr, n, min_quality=TUNE_MIN_QUALITY):
        """(scan, [dict(center, omega_scan, decim, omega, tune, result, ts)]): CarrierScan's record of the capture, and one entry per listed
        carrier in the scan's order.  A carrier that was not decoded (weak, or no symbol-rate line worth believing on its stream) has
        decim, omega, tune and result None and an empty ts.  self.steps holds the seconds of the last call's steps (each ends in a wait)."""
        ctx, n = self.ctx, int(n)
        if n > self.max_samples:
            raise LsdrError(f"wideband decoder: {n} samples exceed max_samples {self.max_samples}")
        self.steps = {}
        t0 = time.perf_counter()
        with CarrierScan(ctx, 1, self.in_format, self.in_scale, max_carriers=self.max_carriers, **self.scan_kw) as sc:
            scan = sc.scan([ptr], [n])[0]
        self._timed("scan", t0)
        cars = scan["carriers"]
        out = [dict(center=c["center"], omega_scan=c["omega"], decim=None, omega=None, tune=None, result=None, ts=b"") for c in cars]
        groups, _ = group_carriers(cars)
        for omega_g, members in groups:
            G = len(members)
            decim, coeffs = resample_design(omega_g)
            cap_out = max(1, (n - len(coeffs)) // decim)
            parts, outs = [], []
            try:
                t0 = time.perf_counter()
                outs = [ctx.alloc(cap_out * 8) for _ in members]
                optr = [b.ptr for b in outs]
                rs_ = ResampleBatch(ctx, G, n, coeffs, decim, self.in_format, self.in_scale)
                parts.append(rs_)
                centres = [min(max(cars[i]["center"], -0.49998), 0.49998) for i in members]
                rs = rs_.run([ptr] * G, [n] * G, centres, optr, cap_out)
                produced = [r["produced"] for r in rs]
                self._timed("resample", t0)
                t0 = time.perf_counter()
                rate = RateEstimator(ctx, G, IN_CF32, 1.0, omega_min=max(0.9 * omega_g / decim, 1.016), omega_max=min(1.1 * omega_g / decim, 64.0))
                parts.append(rate)
                rates = rate.estimate(optr, produced)
                self._timed("rate", t0)
                for omega, sub in group_by_omega(rates)[0]:
                    S = len(sub)
                    sptr, sprod = [optr[k] for k in sub], [produced[k] for k in sub]
                    t0 = time.perf_counter()
                    fine = TuneEstimator(ctx, S, IN_CF32, 1.0)
                    parts.append(fine)
                    est = fine.estimate(sptr, sprod)
                    tunes = [e["tune"] if e["quality"] >= min_quality else (centres[k] - rs[k]["applied"]) * decim for e, k in zip(est, sub)]
                    self._timed("tune", t0)
                    t0 = time.perf_counter()
                    warm = -(-int(896 * omega) // 128) * 128              # ResampledDecoder's rule: 896 symbols of warm-up, tiles eight times that
                    batch = CaptureBatch(ctx, S, cap_out, omega, fec=self.fec, anf=0, viterbi=self.viterbi, in_format=IN_CF32, in_scale=1.0,
                                         tile_warmup=warm, tile_len=-(-8 * warm // 2048) * 2048, relock=self.relock)
                    parts.append(batch)
                    res, ts = batch.decode_each(sptr, sprod, tunes)
                    self._timed("decode", t0)
                    for j, k in enumerate(sub):
                        out[members[k]].update(decim=decim, omega=omega, tune=tunes[j], result=res[j], ts=ts[j])
            finally:
                for p in reversed(parts):
                    p.close()
                for b in outs:
                    b.free()
        return scan, out


def hs2_pack(symbols, offset=0):
    """Hard symbols (0..3) → the packed "hs2" stream (16 per uint32, MSB first), starting at symbol `offset` of word 0."""
    s = np.concatenate([np.zeros(offset, np.uint8), np.asarray(symbols, np.uint8) & 3])
    s = np.concatenate([s, np.zeros((-len(s)) % 16, np.uint8)]).reshape(-1, 16).astype(np.uint32)
    sh = (30 - 2 * np.arange(16)).astype(np.uint32)
    return np.bitwise_or.reduce(s << sh, axis=1).astype(np.uint32)


def hs2_unpack(words, n, offset=0):
    w = np.asarray(words, np.uint32)
    sh = (30 - 2 * np.arange(16)).astype(np.uint32)
    return ((w[:, None] >> sh) & 3).astype(np.uint8).reshape(-1)[offset:offset + n]


# ---- FEC tail -----------------------------------------------------------------------
def derandomizer_pattern():
    out = np.empty(1504, np.uint8)
    lib.lsdr_derandomizer_pattern(_np(out))
    return out


def rs_tables():
    e, l, g = np.empty(512, np.uint8), np.empty(256, np.uint8), np.empty(17, np.uint8)
    lib.lsdr_rs_tables(_np(e), _np(l), _np(g))
    return e, l, g


class Deconv:
    """deconvol_sync<u8,0> (dvb.h:122-513) on the GPU."""

    def __init__(self, ctx, rate=FEC12, fastlock=0):
        self.ctx = ctx
        h = vp()
        check(lib.lsdr_deconv_create(ctx.h, rate, fastlock, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.lsdr_deconv_destroy(self.h)
            self.h = None

    def next_sync(self):
        check(lib.lsdr_deconv_next_sync(self.h))

    def reset(self):
        check(lib.lsdr_deconv_reset(self.h))

    def run_dev(self, in_ptr, n_in, out_ptr, cap):
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_deconv_run(self.h, in_ptr, n_in, out_ptr, cap, C.byref(cons), C.byref(prod)))
        return cons.value, prod.value

    def run_dev_hs2(self, words_ptr, sym_offset, n_in, out_ptr, cap):
        """The same on packed hard symbols (SYM_HARD2): symbols [sym_offset, sym_offset + n_in) of the stream at words_ptr."""
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_deconv_run_hs2(self.h, words_ptr, sym_offset, n_in, out_ptr, cap, C.byref(cons), C.byref(prod)))
        return cons.value, prod.value

    def run_stream(self, sym, pipe=4096, room=8192):
        """Whole stream through repeated run() calls on windows of `pipe` symbols (like the reference pipes)."""
        sym = np.ascontiguousarray(sym, SOFTSYM)
        din = self.ctx.upload(sym)
        dout = self.ctx.alloc(len(sym) + 64)
        pos, nout = 0, 0
        while True:
            avail = min(pipe, len(sym) - pos)
            cons, prod = self.run_dev(din.at(pos * 4), avail, dout.at(nout), room)
            if not cons and not prod:
                break
            pos += cons
            nout += prod
        out = self.ctx.download(dout, np.uint8, nout)
        din.free(); dout.free()
        return out


class Viterbi:
    """viterbi_sync (dvb.h:1173-1416) on the GPU."""

    def __init__(self, ctx, cstln=QPSK, rate=FEC12, resync_period=0):
        self.ctx = ctx
        h = vp()
        check(lib.lsdr_viterbi_create(ctx.h, cstln, rate, C.byref(h)))
        self.h = h
        if resync_period:
            check(lib.lsdr_viterbi_set_resync_period(h, resync_period))

    def close(self):
        if self.h:
            lib.lsdr_viterbi_destroy(self.h)
            self.h = None

    @property
    def current_sync(self):
        return lib.lsdr_viterbi_current_sync(self.h)

    def stats(self):
        t, b = C.c_uint(), C.c_uint()
        check(lib.lsdr_viterbi_stats(self.h, C.byref(t), C.byref(b)))
        return dict(tiles=t.value, bad_seams=b.value)

    def repair_stats(self):
        d, h = C.c_ulonglong(), C.c_ulonglong()
        check(lib.lsdr_viterbi_repair_stats(self.h, C.byref(d), C.byref(h)))
        return dict(device_repaired=d.value, host_rounds=h.value)

    def run_dev(self, in_ptr, n_in, out_ptr, cap):
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_viterbi_run(self.h, in_ptr, n_in, out_ptr, cap, C.byref(cons), C.byref(prod)))
        return cons.value, prod.value

    def run_stream(self, sym, pipe=None):
        """Whole stream; repeated run() calls (a call stops early when the alignment switches)."""
        sym = np.ascontiguousarray(sym, SOFTSYM)
        din = self.ctx.upload(sym)
        dout = self.ctx.alloc(len(sym) + 64)
        pos, nout = 0, 0
        while True:
            avail = len(sym) - pos if pipe is None else min(pipe, len(sym) - pos)
            cons, prod = self.run_dev(din.at(pos * 4), avail, dout.at(nout), len(sym) + 64 - nout)
            if not cons and not prod:
                break
            pos += cons
            nout += prod
        out = self.ctx.download(dout, np.uint8, nout)
        din.free(); dout.free()
        return out, pos


class ViterbiBatch:
    """n_streams independent viterbi_sync decoders (dvb.h:1173-1416) behind one object: every stream's tiles in the same launches,
    seam repair, the alignment decision and all counts on the device (lsdr_viterbi_batch_*)."""

    def __init__(self, ctx, cstln, rate, n_streams, max_symbols, resync_period=0):
        self.ctx, self.n = ctx, int(n_streams)
        h = vp()
        check(lib.lsdr_viterbi_batch_create(ctx.h, cstln, rate, n_streams, max_symbols, C.byref(h)))
        self.h = h
        if resync_period:
            check(lib.lsdr_viterbi_batch_set_resync_period(h, resync_period))

    def close(self):
        if self.h:
            lib.lsdr_viterbi_batch_destroy(self.h)
            self.h = None

    def reset(self, i=-1):
        check(lib.lsdr_viterbi_batch_reset(self.h, i))

    def stats(self):
        l, r = C.c_uint(), C.c_ulonglong()
        check(lib.lsdr_viterbi_batch_stats(self.h, C.byref(l), C.byref(r)))
        return dict(launches_last_run=l.value, runs=r.value)

    @property
    def results_dev(self):
        return lib.lsdr_viterbi_batch_results_dev(self.h)

    def run_async_dev(self, in_ptrs, n_in, out_ptrs, cap_out, n_in_dev=None):
        """Queues one run.  in_ptrs / out_ptrs: device addresses per stream (int, c_void_p or None); n_in: symbols per stream;
        n_in_dev: device address of n_streams uint64 counts, or None."""
        def addr(p):
            return p.value if isinstance(p, vp) else p
        ins = (vp * self.n)(*[addr(p) for p in in_ptrs])
        outs = (vp * self.n)(*[addr(p) for p in out_ptrs])
        ns = (c_sz * self.n)(*[int(x) for x in n_in])
        check(lib.lsdr_viterbi_batch_run_async(self.h, ins, ns, n_in_dev, outs, int(cap_out)))

    def wait(self):
        res = (ViterbiBatchResult * self.n)()
        check(lib.lsdr_viterbi_batch_wait(self.h, res))
        return [r.as_dict() for r in res]

    def run_streams(self, syms, pipe=None, n_in_dev=None):
        """Whole streams: uploads, then repeats run -> wait with every stream advanced by its own `consumed` until no stream makes
        progress (a run stops a stream early behind an alignment switch or in front of a seam that did not verify).
        pipe: at most that many symbols of a stream per run.  n_in_dev: per-stream symbol counts that reach the decoder through
        device memory (written by a device copy queued just before every run, without a host synchronise): stream i ends there.
        Returns ([(bytes, consumed_total, current_sync) per stream], runs)."""
        assert len(syms) == self.n
        syms = [np.ascontiguousarray(s, SOFTSYM) for s in syms]
        cap = max(len(s) for s in syms) + 64
        dins = [self.ctx.upload(s) if len(s) else None for s in syms]
        douts = [self.ctx.alloc(cap) for _ in syms]
        limit = [len(s) for s in syms] if n_in_dev is None else [min(len(s), int(m)) for s, m in zip(syms, n_in_dev)]
        d_src = d_cnt = None
        if n_in_dev is not None:
            d_src, d_cnt = self.ctx.alloc(8 * self.n), self.ctx.alloc(8 * self.n)
        pos, nout, cur, runs = [0] * self.n, [0] * self.n, [0] * self.n, 0
        while True:
            n_in = [len(s) - p if pipe is None else min(pipe, len(s) - p) for s, p in zip(syms, pos)]
            cnt_ptr = None
            if n_in_dev is not None:
                left = np.array([max(l - p, 0) for l, p in zip(limit, pos)], np.uint64)
                check(lib.lsdr_memcpy_h2d(self.ctx.h, d_src.ptr, _np(left), left.nbytes))
                self.ctx.sync()
                check(lib.lsdr_memcpy_d2d(self.ctx.h, d_cnt.ptr, d_src.ptr, left.nbytes))     # queued; the run reads it on the device
                cnt_ptr = d_cnt.ptr
            self.run_async_dev([d.at(p * 4) if d is not None else None for d, p in zip(dins, pos)], n_in,
                               [d.at(o) for d, o in zip(douts, nout)], cap - max(nout), cnt_ptr)
            res = self.wait()
            runs += 1
            for i, r in enumerate(res):
                pos[i] += r["consumed"]
                nout[i] += r["produced"]
                cur[i] = r["current_sync"]
            if not any(r["consumed"] for r in res):
                break
        out = [(self.ctx.download(d, np.uint8, n) if n else np.empty(0, np.uint8), p, c) for d, n, p, c in zip(douts, nout, pos, cur)]
        for d in dins + douts + [d_src, d_cnt]:
            if d is not None:
                d.free()
        return out, runs


class MpegSync:
    """mpeg_sync<u8,0> (dvb.h:712-891) on the GPU."""

    def __init__(self, ctx, fastlock=0):
        self.ctx = ctx
        h = vp()
        check(lib.lsdr_mpeg_sync_create(ctx.h, fastlock, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.lsdr_mpeg_sync_destroy(self.h)
            self.h = None

    @property
    def locked(self):
        return bool(lib.lsdr_mpeg_sync_locked(self.h))

    def set_resync_period(self, period):
        check(lib.lsdr_mpeg_sync_set_resync_period(self.h, period))

    def reset(self):
        check(lib.lsdr_mpeg_sync_reset(self.h))

    def run_dev(self, in_ptr, n_in, out_ptr, cap):
        cons, prod = c_sz(), c_sz()
        ev = (C.c_int * 8)()
        nev, lt, cns = C.c_int(), C.c_ulong(), C.c_int()
        check(lib.lsdr_mpeg_sync_run(self.h, in_ptr, n_in, out_ptr, cap, C.byref(cons), C.byref(prod), ev, C.byref(nev),
                                     C.byref(lt), C.byref(cns)))
        return cons.value, prod.value, list(ev[:nev.value]), lt.value, cns.value

    def run_stream(self, data):
        data = np.ascontiguousarray(data, np.uint8)
        din = self.ctx.upload(data)
        dout = self.ctx.alloc(len(data) + 4096)
        pos, nout, events = 0, 0, []
        while True:
            cons, prod, ev, lt, cns = self.run_dev(din.at(pos), len(data) - pos, dout.at(nout), len(data) + 4096 - nout)
            events += ev
            if not cons and not prod:
                break
            pos += cons
            nout += prod
        out = self.ctx.download(dout, np.uint8, nout)
        din.free(); dout.free()
        return out, events


def deinterleaver(ctx, data):
    data = np.ascontiguousarray(data, np.uint8)
    din = ctx.upload(data)
    cap = len(data) // 204 + 1
    dout = ctx.alloc(cap * 204)
    cons, prod = c_sz(), c_sz()
    check(lib.lsdr_deinterleaver_run(ctx.h, din.ptr, len(data), dout.ptr, cap, C.byref(cons), C.byref(prod)))
    out = ctx.download(dout, np.uint8, prod.value * 204).reshape(-1, 204)
    din.free(); dout.free()
    return out, cons.value


def rs_decoder(ctx, packets):
    packets = np.ascontiguousarray(packets, np.uint8).reshape(-1, 204)
    din = ctx.upload(packets)
    dout = ctx.alloc(max(1, len(packets)) * 188)
    b, e = C.c_long(), C.c_long()
    check(lib.lsdr_rs_decoder_run(ctx.h, din.ptr, len(packets), dout.ptr, C.byref(b), C.byref(e)))
    out = ctx.download(dout, np.uint8, len(packets) * 188).reshape(-1, 188)
    din.free(); dout.free()
    return out, b.value, e.value


class Derandomizer:
    def __init__(self, ctx):
        self.ctx = ctx
        h = vp()
        check(lib.lsdr_derandomizer_create(ctx.h, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.lsdr_derandomizer_destroy(self.h)
            self.h = None

    def run(self, packets):
        packets = np.ascontiguousarray(packets, np.uint8).reshape(-1, 188)
        din = self.ctx.upload(packets)
        dout = self.ctx.alloc(max(1, len(packets)) * 188)
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_derandomizer_run(self.h, din.ptr, len(packets), dout.ptr, len(packets), C.byref(cons), C.byref(prod)))
        out = self.ctx.download(dout, np.uint8, prod.value * 188).reshape(-1, 188)
        din.free(); dout.free()
        return out


# ---- auto_notch / cnr_fft / cfft ------------------------------------------------------
def cfft_dev(ctx, x, reverse=False):
    """cfft_engine<float> on the GPU (k_cfft): upload one block, transform, spectrum back on the host."""
    x = np.ascontiguousarray(x, np.complex64)
    din = ctx.upload(x)
    out = np.empty_like(x)
    check(lib.lsdr_cfft_run(ctx.h, len(x), int(reverse), din.ptr, _np(out)))
    din.free()
    return out


def cfft_host(x, reverse=False):
    x = np.ascontiguousarray(x, np.complex64).copy()
    check(lib.lsdr_cfft_host(len(x), _np(x), int(reverse)))
    return x


class AutoNotch:
    """auto_notch<f32> (sdr.h:46-154) on the GPU."""

    def __init__(self, ctx, nslots=1, setpoint=0.0, decimation=1024 * 4096, k=0.002, mode=0):
        """mode: NOTCH_EXACT (0, bit-exact verified tiles) or NOTCH_SCAN (1, single-pass scan, device-side detect; tolerance)."""
        self.ctx, self.nslots = ctx, nslots
        h = vp()
        check(lib.lsdr_auto_notch_create(ctx.h, nslots, setpoint, C.byref(h)))
        self.h = h
        check(lib.lsdr_auto_notch_set(h, decimation, k))
        if mode:
            check(lib.lsdr_auto_notch_set_mode(h, mode))

    def close(self):
        if self.h:
            lib.lsdr_auto_notch_destroy(self.h)
            self.h = None

    def bins(self):
        return [lib.lsdr_auto_notch_slot_bin(self.h, s) for s in range(self.nslots)]

    def scan_time(self, enable=True):
        """(mean ms, launches) of the k_notch_scan launches recorded since the previous call; then switches recording."""
        ms, n = c_f(), C.c_uint()
        check(lib.lsdr_auto_notch_scan_time(self.h, int(enable), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def stats(self):
        t, b = C.c_uint(), C.c_uint()
        check(lib.lsdr_auto_notch_stats(self.h, C.byref(t), C.byref(b)))
        return dict(tiles=t.value, bad_seams=b.value)

    def run_dev(self, in_ptr, n, out_ptr, cap):
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_auto_notch_run(self.h, in_ptr, n, out_ptr, cap, C.byref(cons), C.byref(prod)))
        return cons.value, prod.value

    def run(self, x):
        x = np.ascontiguousarray(x, np.complex64)
        din = self.ctx.upload(x)
        dout = self.ctx.alloc(max(8, x.nbytes))
        cons, prod = self.run_dev(din.ptr, len(x), dout.ptr, len(x))
        out = self.ctx.download(dout, np.complex64, prod)
        din.free(); dout.free()
        return out


class NotchFir:
    """auto_notch<f32>(1 slot) fused into fir_filter<cf32,float> (leandvb's default graph, leandvb.cc:296-301): lsdr_notch_fir_*.
    Tolerance mode; LsdrError (LSDR_E_UNSUPPORTED) for geometries without the fused kernel — use AutoNotch + FirFilter then."""

    def __init__(self, ctx, coeffs, decim, in_scale=0.0, nslots=1, decimation=1024 * 4096, k=0.002):
        self.ctx = ctx
        self.coeffs = np.ascontiguousarray(coeffs, np.float32)
        self.decim = decim
        cfg = NotchFirCfg(len(self.coeffs), self.coeffs.ctypes.data, decim, in_scale, nslots, decimation, k)
        h = vp()
        check(lib.lsdr_notch_fir_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.lsdr_notch_fir_destroy(self.h)
            self.h = None

    def bin(self):
        return lib.lsdr_notch_fir_slot_bin(self.h)

    def set_freq(self, freq):
        """fir_filter::set_freq (dsp.h:271-280): shifted taps from the next run on."""
        check(lib.lsdr_notch_fir_set_freq(self.h, freq))

    def track(self, freq_tap, tap_multiplier, freq_tol):
        """fir_filter::run's tracking step (dsp.h:236-244); returns whether the taps were re-shifted."""
        did = C.c_int()
        check(lib.lsdr_notch_fir_track(self.h, freq_tap, tap_multiplier, freq_tol, C.byref(did)))
        return bool(did.value)

    @property
    def current_freq(self):
        return float(lib.lsdr_notch_fir_current_freq(self.h))

    def set_overlap(self, on=True):
        """Detect chain and filter pass of run k+1 on the block's own streams next to run k's tail (inputs must be complete at call time)."""
        check(lib.lsdr_notch_fir_set_overlap(self.h, int(on)))

    def pass_time(self, enable=True):
        """(mean ms, launches) of the filter pass (k_fir_mfma_stream, per-interval taps) since the previous call; then switches recording."""
        ms, n = c_f(), C.c_uint()
        check(lib.lsdr_notch_fir_time(self.h, int(enable), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def run_dev(self, in_ptr, n_in, out_ptr, cap_out):
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_notch_fir_run(self.h, in_ptr, n_in, out_ptr, cap_out, C.byref(cons), C.byref(prod)))
        return cons.value, prod.value

    def run(self, x, step=None):
        """The whole stream `x` through the block in runs of at most `step` samples (None: one run); returns (outputs, consumed)."""
        x = np.ascontiguousarray(x, np.complex64)
        din = self.ctx.upload(x) if len(x) else None
        cap = len(x) // self.decim + 16
        dout = self.ctx.alloc(cap * 8)
        pos = nout = 0
        while din is not None:
            avail = len(x) - pos if step is None else min(len(x) - pos, step)
            cons, prod = self.run_dev(din.at(pos * 8), avail, dout.at(nout * 8), cap - nout)
            if not prod:
                if step is None or avail == len(x) - pos:
                    break
                step *= 2          # a run needs a whole 4096-block beyond the filter's history: offer more
                continue
            pos += cons; nout += prod
        out = self.ctx.download(dout, np.complex64, nout)
        if din is not None:
            din.free()
        dout.free()
        return out, pos


class FastQpsk:
    """fast_qpsk_receiver<u8> (sdr.h:946-1189), the --hs receiver."""

    def __init__(self, ctx, omega, freq=0.0, pll_adjustment=1.0, allow_drift=0, meas_decimation=0, tiled=False, tile_len=0,
                 tile_warmup=0):
        self.ctx = ctx
        h = vp()
        check(lib.lsdr_fastqpsk_create(ctx.h, omega, freq, pll_adjustment, allow_drift, meas_decimation, C.byref(h)))
        self.h = h
        if tiled:
            check(lib.lsdr_fastqpsk_set_tiled(h, 1, tile_len, tile_warmup))

    def set_tiled(self, enable, tile_len=0, tile_warmup=0):
        check(lib.lsdr_fastqpsk_set_tiled(self.h, int(enable), tile_len, tile_warmup))

    def tiled_stats(self):
        t, d, m, b = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
        check(lib.lsdr_fastqpsk_tiled_stats(self.h, C.byref(t), C.byref(d), C.byref(m), C.byref(b)))
        return dict(tiles=t.value, dup=d.value, miss=m.value, bad_seams=b.value)

    def close(self):
        if self.h:
            lib.lsdr_fastqpsk_destroy(self.h)
            self.h = None

    def state(self):
        mu, ph, fw, mn, mx = c_f(), C.c_uint(), C.c_longlong(), C.c_longlong(), C.c_longlong()
        check(lib.lsdr_fastqpsk_get_state(self.h, C.byref(mu), C.byref(ph), C.byref(fw), C.byref(mn), C.byref(mx)))
        return dict(mu=mu.value, phase=ph.value, freqw=fw.value, min_freqw=mn.value, max_freqw=mx.value)

    def run_dev(self, in_ptr, n_in, out_ptr, cap):
        """Device pointers (cu8 in, one hard symbol per byte out); no FREQ/constellation reports.  → (consumed, produced)."""
        cons, prod, nf, nc = c_sz(), c_sz(), c_sz(), c_sz()
        check(lib.lsdr_fastqpsk_run(self.h, in_ptr, n_in, out_ptr, cap, C.byref(cons), C.byref(prod), None, 0, C.byref(nf), None, 0,
                                    C.byref(nc)))
        return cons.value, prod.value

    def run(self, iq_u8, meas=True):
        """Upload interleaved u8 I/Q, run once, download.  Returns dict(sym, consumed, freq, cstln)."""
        iq = np.ascontiguousarray(iq_u8, np.uint8)
        n = len(iq) // 2
        din = self.ctx.upload(iq)
        dout = self.ctx.alloc(n + 256)
        fo = np.empty(n // 64 + 16, np.float32)
        co = np.empty((n // 64 + 16, 2), np.uint8)
        cons, prod, nf, nc = c_sz(), c_sz(), c_sz(), c_sz()
        check(lib.lsdr_fastqpsk_run(self.h, din.ptr, n, dout.ptr, n + 256, C.byref(cons), C.byref(prod),
                                    _np(fo) if meas else None, len(fo), C.byref(nf), _np(co) if meas else None, len(co), C.byref(nc)))
        sym = self.ctx.download(dout, np.uint8, prod.value)
        din.free(); dout.free()
        return dict(sym=sym, consumed=cons.value, freq=fo[:nf.value].copy(), cstln=co[:nc.value].copy())


class HsDeconv:
    """dvb_deconvol_sync<u8> (dvb.h:612-707), the --hs deconvolver."""

    def __init__(self, ctx, resync_period=32):
        self.ctx = ctx
        h = vp()
        check(lib.lsdr_hsdeconv_create(ctx.h, resync_period, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.lsdr_hsdeconv_destroy(self.h)
            self.h = None

    @property
    def locked(self):
        return lib.lsdr_hsdeconv_locked(self.h)

    def run_dev(self, in_ptr, n_in, out_ptr, cap):
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_hsdeconv_run(self.h, in_ptr, n_in, out_ptr, cap, C.byref(cons), C.byref(prod)))
        return cons.value, prod.value

    def run_stream(self, symbols, pipe=None, room=None):
        sym = np.ascontiguousarray(symbols, np.uint8)
        din = self.ctx.upload(sym)
        dout = self.ctx.alloc(len(sym) // 8 + 64)
        pos = nout = 0
        while True:
            avail = len(sym) - pos if pipe is None else min(pipe, len(sym) - pos)
            cap = len(sym) // 8 + 64 - nout if room is None else min(room, len(sym) // 8 + 64 - nout)
            cons, prod = c_sz(), c_sz()
            check(lib.lsdr_hsdeconv_run(self.h, din.at(pos), avail, dout.at(nout), cap, C.byref(cons), C.byref(prod)))
            if not prod.value:
                break
            pos += cons.value
            nout += prod.value
        out = self.ctx.download(dout, np.uint8, nout)
        din.free(); dout.free()
        return out


class Rotator:
    """rotator<f32> (sdr.h:1226-1259)."""

    def __init__(self, ctx, freq):
        self.ctx = ctx
        h = vp()
        check(lib.lsdr_rotator_create(ctx.h, freq, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.lsdr_rotator_destroy(self.h)
            self.h = None

    def run(self, x):
        x = np.ascontiguousarray(x, np.complex64)
        din = self.ctx.upload(x)
        dout = self.ctx.alloc(max(8, len(x) * 8))
        check(lib.lsdr_rotator_run(self.h, din.ptr, len(x), dout.ptr))
        out = self.ctx.download(dout, np.complex64, len(x))
        din.free(); dout.free()
        return out


class Spectrum:
    """spectrum<f32> (sdr.h:1347-1404)."""

    def __init__(self, ctx, decimation=1048576, kavg=0.1):
        self.ctx = ctx
        h = vp()
        check(lib.lsdr_spectrum_create(ctx.h, C.byref(h)))
        self.h = h
        check(lib.lsdr_spectrum_set(h, decimation, kavg))

    def close(self):
        if self.h:
            lib.lsdr_spectrum_destroy(self.h)
            self.h = None

    def run(self, x):
        x = np.ascontiguousarray(x, np.complex64)
        din = self.ctx.upload(x)
        out = np.empty((len(x) // 1024 + 1, 1024), np.float32)
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_spectrum_run(self.h, din.ptr, len(x), _np(out), len(out), C.byref(cons), C.byref(prod)))
        din.free()
        return out[:prod.value].copy(), cons.value

    def run_dev(self, in_ptr, n_in):
        out = np.empty((n_in // 1024 // 64 + 4, 1024), np.float32)
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_spectrum_run(self.h, in_ptr, n_in, _np(out), len(out), C.byref(cons), C.byref(prod)))
        return out[:prod.value].copy(), cons.value


class CnrFft:
    """cnr_fft<f32> (sdr.h:1273-1345)."""

    def __init__(self, ctx, bandwidth, nfft=4096, decimation=1048576, kavg=0.1):
        self.ctx = ctx
        h = vp()
        check(lib.lsdr_cnr_fft_create(ctx.h, bandwidth, nfft, C.byref(h)))
        self.h = h
        check(lib.lsdr_cnr_fft_set(h, decimation, kavg))

    def close(self):
        if self.h:
            lib.lsdr_cnr_fft_destroy(self.h)
            self.h = None

    def run(self, x, freq_tap=0.0, tap_multiplier=1.0):
        x = np.ascontiguousarray(x, np.complex64)
        din = self.ctx.upload(x)
        out = np.empty(len(x) // 64 + 8, np.float32)
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_cnr_fft_run(self.h, freq_tap, tap_multiplier, din.ptr, len(x), _np(out), len(out), C.byref(cons), C.byref(prod)))
        din.free()
        return out[:prod.value].copy(), cons.value

    def run_dev(self, in_ptr, n_in, freq_tap=0.0, tap_multiplier=1.0):
        """One run() over a device buffer: (CNR values appended by this call, samples consumed)."""
        out = np.empty(n_in // 64 + 8, np.float32)
        cons, prod = c_sz(), c_sz()
        check(lib.lsdr_cnr_fft_run(self.h, freq_tap, tap_multiplier, in_ptr, n_in, _np(out), len(out), C.byref(cons), C.byref(prod)))
        return out[:prod.value].copy(), cons.value


# ---- channel simulator (leanchansim.cc:34-190) -------------------------------------------
class Wgn:
    """wgn_c<f32> (dsp.h:164-190) on glibc's drand48/logf; seed=None: the state of a process that never seeds."""

    def __init__(self, ctx, seed=None):
        self.ctx = ctx
        h = vp()
        check(lib.lsdr_wgn_create(ctx.h, 0 if seed is None else 1, seed or 0, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.lsdr_wgn_destroy(self.h)
            self.h = None

    @property
    def state(self):
        x = C.c_ulonglong()
        check(lib.lsdr_wgn_get_state(self.h, C.byref(x)))
        return x.value

    def run(self, n, stddev=1.0, add=None):
        dout = self.ctx.alloc(max(8, n * 8))
        dadd = self.ctx.upload(np.ascontiguousarray(add, np.complex64)) if add is not None else None
        check(lib.lsdr_wgn_run(self.h, stddev, dadd.ptr if dadd else None, dout.ptr, n))
        out = self.ctx.download(dout, np.complex64, n)
        dout.free()
        if dadd:
            dadd.free()
        return out


def adder(ctx, a, b):
    a = np.ascontiguousarray(a, np.complex64); b = np.ascontiguousarray(b, np.complex64)
    n = min(len(a), len(b))
    da, db, dout = ctx.upload(a), ctx.upload(b), ctx.alloc(max(8, n * 8))
    check(lib.lsdr_adder_run(ctx.h, da.ptr, db.ptr, n, dout.ptr))
    out = ctx.download(dout, np.complex64, n)
    da.free(); db.free(); dout.free()
    return out


def cconv_f32_u8(ctx, x):
    x = np.ascontiguousarray(x, np.complex64)
    din, dout = ctx.upload(x), ctx.alloc(max(8, len(x) * 2))
    check(lib.lsdr_cconverter_f32_u8_run(ctx.h, din.ptr, len(x), dout.ptr))
    out = ctx.download(dout, np.uint8, len(x) * 2).reshape(-1, 2)
    din.free(); dout.free()
    return out


def cconv_f32_s16(ctx, x):
    x = np.ascontiguousarray(x, np.complex64)
    din, dout = ctx.upload(x), ctx.alloc(max(8, len(x) * 4))
    check(lib.lsdr_cconverter_f32_s16_run(ctx.h, din.ptr, len(x), dout.ptr))
    out = ctx.download(dout, np.int16, len(x) * 2).reshape(-1, 2)
    din.free(); dout.free()
    return out


class Drifter:
    """drifter<float> (leanchansim.cc:34-88)."""

    def __init__(self, ctx, amp=(0, 0, 0), freq=(0, 0, 0)):
        self.ctx = ctx
        h = vp()
        check(lib.lsdr_drifter_create(ctx.h, C.byref(h)))
        self.h = h
        for i in range(3):
            check(lib.lsdr_drifter_set_component(h, i, amp[i], freq[i]))

    def close(self):
        if self.h:
            lib.lsdr_drifter_destroy(self.h)
            self.h = None

    @property
    def phases(self):
        a = (C.c_longlong * 3)()
        check(lib.lsdr_drifter_get_phases(self.h, a))
        return tuple(a)

    @phases.setter
    def phases(self, v):
        check(lib.lsdr_drifter_set_phases(self.h, (C.c_longlong * 3)(*v)))

    def run(self, x, chunk=4096):
        x = np.ascontiguousarray(x, np.complex64)
        din, dout = self.ctx.upload(x), self.ctx.alloc(max(8, len(x) * 8))
        check(lib.lsdr_drifter_run(self.h, din.ptr, len(x), dout.ptr, chunk))
        out = self.ctx.download(dout, np.complex64, len(x))
        din.free(); dout.free()
        return out


# ---- transmit chain (leandvbtx.cc:79-175) ------------------------------------------------
class TxChain:
    """randomizer → rs_encoder → interleaver → dvb_convol → cstln_transmitter → fir_resampler(RRC) → decimator [→ simple_agc]
    on one context, device-resident between the blocks.  `run(ts)` feeds a batch of TS packets and returns the baseband
    produced so far (state is carried: interleaver window, convolutional history, resampler history, AGC estimate)."""

    def __init__(self, ctx, interp=2, decim=1, amp=1.0, rolloff=0.35, rrc_rej=10.0, agc=False, cstln=QPSK, rate=FEC12):
        self.ctx, self.interp, self.decim, self.cstln, self.rate = ctx, interp, decim, cstln, rate
        self.rand = vp(); check(lib.lsdr_randomizer_create(ctx.h, C.byref(self.rand)))
        bps = CSTLN_BITS[cstln]
        conv_rate = FEC46 if (rate == FEC23 and bps in (2, 6)) else rate      # leandvbtx.cc:117-121
        self.conv = vp(); check(lib.lsdr_convol_create(ctx.h, conv_rate, bps, C.byref(self.conv)))
        order = int(interp * rrc_rej)
        co = root_raised_cosine(order, float(np.float32(1.0) / np.float32(interp)), rolloff)
        co = normalize_power(co, float(np.float32(amp) / np.float32(75.0)))
        self.coeffs = co
        self.res = vp(); check(lib.lsdr_fir_resampler_create(ctx.h, len(co), _np(co), interp, C.byref(self.res)))
        self.agc = None
        if agc:
            self.agc = vp()
            check(lib.lsdr_simple_agc_create(ctx.h, float(np.float32(amp) / np.sqrt(np.float32(np.float32(interp) / decim))),
                                             float(np.float32(0.001 * decim / interp)), C.byref(self.agc)))
        self.pk_hold = np.zeros((0, 204), np.uint8)      # interleaver window (host-side carry of unconsumed packets)
        self.il_hold = np.zeros(0, np.uint8)              # interleaved bytes short of a convolutional group
        self.iq_hold = np.zeros(0, np.complex64)          # resampler input not yet consumed
        self.dec_hold = np.zeros(0, np.complex64)         # decimator / AGC remainders
        self.agc_hold = np.zeros(0, np.complex64)

    def close(self):
        lib.lsdr_randomizer_destroy(self.rand); lib.lsdr_convol_destroy(self.conv); lib.lsdr_fir_resampler_destroy(self.res)
        if self.agc:
            lib.lsdr_simple_agc_destroy(self.agc)

    def _run2(self, fn, h, din, n_in, cap_items, out_dtype, item=1):
        """One *_run call; `cap_items` / produced are in the block's output items of `item` elements of out_dtype."""
        dout = self.ctx.alloc(max(16, cap_items * item * np.dtype(out_dtype).itemsize))
        cons, prod = c_sz(), c_sz()
        if h is None:
            check(fn(self.ctx.h, din.ptr, n_in, dout.ptr, cap_items, C.byref(cons), C.byref(prod)))
        else:
            check(fn(h, din.ptr, n_in, dout.ptr, cap_items, C.byref(cons), C.byref(prod)))
        out = self.ctx.download(dout, out_dtype, prod.value * item)
        dout.free()
        return out, cons.value

    def run(self, ts):
        ctx = self.ctx
        ts = np.ascontiguousarray(ts, np.uint8).reshape(-1, 188)
        d = ctx.upload(ts)
        r, _ = self._run2(lib.lsdr_randomizer_run, self.rand, d, len(ts), len(ts), np.uint8, 188); d.free()
        r = r.reshape(-1, 188)
        d = ctx.upload(r)
        pk, _ = self._run2(lib.lsdr_rs_encoder_run, None, d, len(r), len(r), np.uint8, 204); d.free()
        pk = np.concatenate([self.pk_hold, pk.reshape(-1, 204)])
        if len(pk) < 12:
            self.pk_hold = pk
            return np.zeros(0, np.complex64)
        d = ctx.upload(pk)
        il, cons = self._run2(lib.lsdr_interleaver_run, None, d, len(pk), len(pk) * 204, np.uint8); d.free()
        self.pk_hold = pk[cons:]
        il = np.concatenate([self.il_hold, il])                 # dvb_convol consumes whole groups of bits_in bytes
        d = ctx.upload(il)
        sym, cons = self._run2(lib.lsdr_convol_run, self.conv, d, len(il), len(il) * 16 + 64, np.uint8); d.free()
        self.il_hold = il[cons:]
        d = ctx.upload(sym)
        dq = ctx.alloc(max(16, len(sym) * 8))
        check(lib.lsdr_cstln_transmitter_run(ctx.h, self.cstln, self.rate, d.ptr, len(sym), dq.ptr)); d.free()
        iq = np.concatenate([self.iq_hold, ctx.download(dq, np.complex64, len(sym))]); dq.free()
        d = ctx.upload(iq)
        y, cons = self._run2(lib.lsdr_fir_resampler_run, self.res, d, len(iq), len(iq) * self.interp, np.complex64); d.free()
        self.iq_hold = iq[cons:]
        y = np.concatenate([self.dec_hold, y])
        nd = len(y) // self.decim
        self.dec_hold = y[nd * self.decim:]
        y = np.ascontiguousarray(y[:nd * self.decim:self.decim]) if self.decim > 1 else y
        if self.agc:
            y = np.concatenate([self.agc_hold, y])
            d = ctx.upload(y)
            z, cons = self._run2(lib.lsdr_simple_agc_run, self.agc, d, len(y), len(y), np.complex64); d.free()
            self.agc_hold = y[cons:]
            y = z
        return y


# ---- leandvbtx | leanchansim for many streams (lsdr_tx_batch) ----------------------------
def db_to_amplitude(db):
    """How leandvbtx --power and leanchansim --awgn read their argument: expf(logf(10)·db/20)."""
    return float(lib.lsdr_db_to_amplitude(float(db)))


class TxBatch:
    """lsdr_tx_batch: n_streams transport streams, each with its own length, code rate, power, scale, noise level and seed, become
    n_streams noisy captures in device memory in one set of launches; every capture is bit for bit what leandvbtx | leanchansim write
    for that stream alone (include/lsdr_hip.h).  `ptrs()` and `lengths()` are what the batch decoders and estimators take.
    ctx None: no device object, only `plan`."""

    def __init__(self, ctx, n_streams, max_packets, interp=2, decim=1, cstln=QPSK, agc=False, rolloff=0.35, rrc_rej=10.0,
                 out_format=IN_CF32):
        self.ctx, self.n, self.h = ctx, int(n_streams), None
        cfg = TxBatchCfg()
        cfg.n_streams, cfg.max_packets, cfg.cstln, cfg.interp, cfg.decim = self.n, int(max_packets), int(cstln), int(interp), int(decim)
        cfg.rolloff, cfg.rrc_rej, cfg.agc, cfg.out_format = rolloff, rrc_rej, 1 if agc else 0, int(out_format)
        self.cfg, self.out_format = cfg, int(out_format)
        self._res = (TxResult * max(self.n, 1))()
        self._last = []
        self._keep = []
        if ctx is not None:
            h = vp()
            check(lib.lsdr_tx_batch_create(ctx.h, C.byref(cfg), C.byref(h)))
            self.h = h

    def close(self):
        if self.h:
            lib.lsdr_tx_batch_destroy(self.h)
            self.h = None
        for d in self._keep:
            d.free()
        self._keep = []

    @staticmethod
    def each(n_packets=0, fec=FEC12, amp=None, power_db=None, scale=0.0, awgn_db=None, noise_stddev=None, seed=None):
        """One stream's lsdr_tx_each.  amp | power_db (default amp 1), noise_stddev | awgn_db (default 0), seed None: --deterministic."""
        e = TxEach()
        e.n_packets, e.fec, e.scale = int(n_packets), int(fec), scale
        e.amp = (1.0 if power_db is None else db_to_amplitude(power_db)) if amp is None else amp
        e.noise_stddev = (0.0 if awgn_db is None else db_to_amplitude(awgn_db)) if noise_stddev is None else noise_stddev
        e.seeded, e.seed = (0, 0) if seed is None else (1, int(seed))
        return e

    def plan(self, each, n_packets=None):
        """The four lengths of one stream (dict(packets, bytes, symbols, samples)), on the host: no GPU, no context."""
        e = each if isinstance(each, TxEach) else self.each(**each)
        if n_packets is not None:
            e.n_packets = int(n_packets)
        r = TxResult()
        check(lib.lsdr_tx_batch_plan(C.byref(self.cfg), C.byref(e), C.byref(r)))
        return {k: int(getattr(r, k)) for k in ("packets", "bytes", "symbols", "samples")}

    def set_noise_margin(self, sigmas):
        check(lib.lsdr_tx_batch_set_noise_margin(self.h, sigmas))

    def stats(self):
        a, b = C.c_uint(), C.c_ulonglong()
        check(lib.lsdr_tx_batch_stats(self.h, C.byref(a), C.byref(b)))
        return dict(launches_last_run=a.value, runs=b.value)

    def run_async(self, ts, each):
        """Queues one run.  ts: per stream a numpy array of 188-byte packets (uploaded here), or (device pointer, n_packets); each: per
        stream a TxEach or the keyword arguments of `each` (n_packets is taken from ts)."""
        if len(ts) != self.n or len(each) != self.n:
            raise LsdrError(f"tx batch: {len(ts)} streams and {len(each)} records for {self.n} streams")
        keep = []                                        # this run's uploads; the last run's are freed once this one is accepted
        arr = (TxEach * self.n)()
        ptrs = (vp * self.n)()
        for i, (t, e) in enumerate(zip(ts, each)):
            if isinstance(t, tuple):
                ptr, npk = t
                ptr = ptr.value if isinstance(ptr, vp) else ptr
            else:
                a = np.ascontiguousarray(t, np.uint8).reshape(-1, 188)
                npk, ptr = len(a), None
                if npk:
                    d = self.ctx.upload(a)
                    keep.append(d)
                    ptr = d.ptr.value if isinstance(d.ptr, vp) else d.ptr
            arr[i] = e if isinstance(e, TxEach) else self.each(**e)
            arr[i].n_packets = int(npk)
            ptrs[i] = ptr
        rc = lib.lsdr_tx_batch_run_async(self.h, ptrs, arr)
        for d in (keep if rc else self._keep):           # refused (a run may be in flight): the last run's uploads stay
            d.free()
        if not rc:
            self._keep = keep
        check(rc)

    def wait(self):
        check(lib.lsdr_tx_batch_wait(self.h, self._res))
        self._last = [r.as_dict() for r in self._res[:self.n]]
        return self._last

    def run(self, ts, each):
        self.run_async(ts, each)
        return self.wait()

    def ptrs(self):
        return [lib.lsdr_tx_batch_out_dev(self.h, i) for i in range(self.n)]

    def lengths(self):
        return [int(r["samples"]) for r in self._last]

    def results_ptr(self):
        return lib.lsdr_tx_batch_results_dev(self.h)

    def download_all(self):
        """Every stream of the last run: complex64 arrays, or uint8 [n, 2] with IN_CU8."""
        u8 = self.out_format == IN_CU8
        cap = max(self.lengths() + [1])
        bufs = [np.empty((cap, 2), np.uint8) if u8 else np.empty(cap, np.complex64) for _ in range(self.n)]
        check(lib.lsdr_tx_batch_download_async(self.h, (vp * self.n)(*[b.ctypes.data for b in bufs]), bufs[0].nbytes))
        check(lib.lsdr_tx_batch_download_wait(self.h))
        return [b[:n] for b, n in zip(bufs, self.lengths())]

    def download(self, i):
        return self.download_all()[i]
