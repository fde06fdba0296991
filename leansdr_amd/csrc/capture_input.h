// leansdr_amd/csrc/capture_input.h — the one place that knows the raw captures' sample formats (LSDR_IN_*, include/lsdr_hip.h), for every
// object that reads captures on the device: lsdr_capture_batch / lsdr_hs_batch (host side only: rxb_host.h, hsb_host.h, capture_batch.hip),
// lsdr_tune_est, lsdr_rate_est, lsdr_carrier_scan, lsdr_resample_batch, lsdr_spectrum_batch (host side and kernels).  Plain C++ on values, callable from a kernel and from
// the host:
//   the kinds, in_item / in_load / in_unpack / in_piece   an item converted: value = float(item − Z)·in_scale, one rounding per component
//   lsdr_in_describe, lsdr_in_check_each                   an object's format and scale at create, a run's per-capture arguments
//   in_dispatch                                            a kernel instantiation by kind
//   in_run, lsdr_in_free                                   what the objects above the formats repeat: records, event, flag; destroy
//
// The conversion is rxb_device.h's (rxb_in<K>) for the kernels outside the receiver; the receiver's own loads stay where bench.py measures
// them.  rxb_host.h ties the two enumerations together.  block_spectrum.h stands on this header: what lsdr_tune_est and lsdr_rate_est share
// above the formats (blocks of 4096 samples, their transform, the reductions, the host's frame of a run).
#ifndef LSDR_CAPTURE_INPUT_H
#define LSDR_CAPTURE_INPUT_H
#include <cmath>
#include <initializer_list>
#include <type_traits>
#include "lsdr_internal.h"

#define IN_HD __host__ __device__ __forceinline__

enum { kCapU8 = 0, kCapS8 = 1, kCap16 = 2, kCapF32 = 3 };                 // one kind per item size (cu16 / cs16 differ in `flip`)
template <int K> struct in_item { static constexpr unsigned kBytes = K == kCapF32 ? 8u : (K == kCap16 ? 4u : 2u); };

// item `i` of a capture at `src`, converted.  flip: 0x80008000 for cu16 (the bias 32768 is the item's top bit), 0 for cs16.
template <int K>
IN_HD float2 in_load(const unsigned char *src, size_t i, float sc, unsigned flip) {
  if constexpr (K == kCapU8) {
    const unsigned w = *reinterpret_cast<const unsigned short *>(src + 2 * i);
    return make_float2((float)((int)(w & 255u) - 128) * sc, (float)((int)(w >> 8) - 128) * sc);
  } else if constexpr (K == kCapS8) {
    const unsigned w = *reinterpret_cast<const unsigned short *>(src + 2 * i);
    return make_float2((float)(int)(signed char)w * sc, (float)(int)(signed char)(w >> 8) * sc);
  } else if constexpr (K == kCap16) {
    const unsigned w = *reinterpret_cast<const unsigned *>(src + 4 * i) ^ flip;
    return make_float2((float)(int)(short)(w & 0xffffu) * sc, (float)((int)w >> 16) * sc);
  } else {
    const float2 w = *reinterpret_cast<const float2 *>(src + 8 * i);
    return make_float2(w.x * sc, w.y * sc);
  }
}
// … the same from the four dwords of one 16-byte load: item q of 16 / kBytes
template <int K>
IN_HD float2 in_unpack(const unsigned (&ws)[4], unsigned q, float sc, unsigned flip) {
  if constexpr (K == kCapU8) {
    const unsigned w = (ws[q >> 1] >> (16u * (q & 1u))) & 0xffffu;
    return make_float2((float)((int)(w & 255u) - 128) * sc, (float)((int)(w >> 8) - 128) * sc);
  } else if constexpr (K == kCapS8) {
    const unsigned w = ws[q >> 1] >> (16u * (q & 1u));
    return make_float2((float)(int)(signed char)w * sc, (float)(int)(signed char)(w >> 8) * sc);
  } else if constexpr (K == kCap16) {
    const unsigned w = ws[q] ^ flip;
    return make_float2((float)(int)(short)(w & 0xffffu) * sc, (float)((int)w >> 16) * sc);
  } else {
    float re, im;
    __builtin_memcpy(&re, &ws[2 * q], 4); __builtin_memcpy(&im, &ws[2 * q + 1], 4);
    return make_float2(re * sc, im * sc);
  }
}
// One 16-byte piece of a capture, the 16 / kBytes items from item `i0` (a multiple of that) on, converted: one 16-byte load where `wide`
// (src + i0·kBytes is 16-byte aligned), item by item where the capture's pointer is only item-aligned: the same values.
template <int K>
IN_HD void in_piece(const unsigned char *src, size_t i0, bool wide, float sc, unsigned flip, float2 (&z)[16u / in_item<K>::kBytes]) {
  constexpr unsigned kB = in_item<K>::kBytes, kPer = 16u / kB;
  if (wide) {
    const uint4 w = *reinterpret_cast<const uint4 *>(src + i0 * kB);
    const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (unsigned q = 0; q < kPer; ++q) z[q] = in_unpack<K>(ws, q, sc, flip);
  } else {
#pragma unroll
    for (unsigned q = 0; q < kPer; ++q) z[q] = in_load<K>(src, i0 + q, sc, flip);
  }
}

// f(std::integral_constant<int, kind>): the way from an object's kind to a kernel instantiation
template <class F>
auto in_dispatch(int kind, F &&f) {
  switch (kind) {
    case kCapU8: return f(std::integral_constant<int, kCapU8>());
    case kCapS8: return f(std::integral_constant<int, kCapS8>());
    case kCap16: return f(std::integral_constant<int, kCap16>());
    default: return f(std::integral_constant<int, kCapF32>());
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// What an object keeps of its in_format / in_scale.  who: the owner's prefix in the error texts.
struct lsdr_in_desc { int kind; unsigned item_bytes, in_flip; float in_scale; };
inline int lsdr_in_describe(const char *who, int in_format, float in_scale, lsdr_in_desc *out) {
  lsdr_in_desc d = {kCapU8, 2u, 0u, in_scale == 0.f ? 1.0f : in_scale};   // (in_scale 0: none)
  switch (in_format) {
    case LSDR_IN_CU8: break;
    case LSDR_IN_CS8: d.kind = kCapS8; break;
    case LSDR_IN_CU16: d.kind = kCap16; d.item_bytes = 4; d.in_flip = 0x80008000u; break;
    case LSDR_IN_CS16: d.kind = kCap16; d.item_bytes = 4; break;
    case LSDR_IN_CF32: d.kind = kCapF32; d.item_bytes = 8; break;
    default: lsdr_set_error("%s: in_format %d is none of LSDR_IN_CU8, _CS8, _CU16, _CS16, _CF32", who, in_format); return LSDR_E_ARG;
  }
  if (!std::isfinite(in_scale) || in_scale < 0.f) { lsdr_set_error("%s: in_scale must be finite and not negative", who); return LSDR_E_ARG; }
  *out = d;
  return LSDR_OK;
}

// The arguments of one run, capture by capture: length against max_samples, tune (tune_word: what the owner calls it), the reserved
// fields, a pointer wherever there are samples, the pointer aligned to the item.  Lengths and tunes come from `each` (with its reserved
// fields), or, where `each` is null, from n_samples and tune (null: no tune to check).  Nothing is written: a refused run leaves its
// object as it was.
inline int lsdr_in_check_each(const char *who, const char *tune_word, unsigned B, const void *const *iq, const lsdr_capture_each *each,
                              const size_t *n_samples, const float *tune, size_t max_samples, unsigned item_bytes) {
  for (unsigned i = 0; i < B; ++i) {
    const size_t n = each ? each[i].n_samples : n_samples[i];
    const float f = each ? each[i].tune : (tune ? tune[i] : 0.f);
    if (n > max_samples) { lsdr_set_error("%s: capture %u: n_samples %zu exceeds max_samples %zu", who, i, n, max_samples); return LSDR_E_ARG; }
    if (!std::isfinite(f) || !(fabsf(f) < 0.5f)) {
      lsdr_set_error("%s: capture %u: %s must be finite and inside (-0.5, 0.5) cycles per sample", who, i, tune_word); return LSDR_E_ARG;
    }
    for (int k = 0; each && k < 5; ++k)
      if (each[i].reserved[k]) { lsdr_set_error("%s: capture %u: lsdr_capture_each.reserved must be 0", who, i); return LSDR_E_ARG; }
    if (!iq[i] && n) { lsdr_set_error("%s: capture %u has samples and no pointer", who, i); return LSDR_E_ARG; }
    if ((size_t)iq[i] % item_bytes) {
      lsdr_set_error("%s: capture %u: the pointer is not aligned to the item size (%u bytes)", who, i, item_bytes); return LSDR_E_ARG;
    }
  }
  return LSDR_OK;
}

// The per-capture records of a run (pinned, and the device copy the kernels read), the event behind the run's last operation, and the flag
// between run_async and wait — of lsdr_tune_est, lsdr_rate_est, lsdr_resample_batch and lsdr_spectrum_batch.  The device is the caller's to set.
template <class Cap>
struct in_run {
  Cap *h_caps = nullptr, *d_caps = nullptr;
  size_t n = 0;
  hipEvent_t ev_done = nullptr;
  bool in_flight = false;

  int create(size_t captures) {
    n = captures;
    LSDR_HIP(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming));
    LSDR_HIP(hipHostMalloc((void **)&h_caps, n * sizeof(Cap), hipHostMallocDefault));
    memset(h_caps, 0, n * sizeof(Cap));
    LSDR_HIP(hipMalloc((void **)&d_caps, n * sizeof(Cap)));
    return LSDR_OK;
  }
  int idle(const char *who, const char *wait_name) const {                 // (behind the argument checks, in front of anything written)
    if (in_flight) { lsdr_set_error("%s: a run is in flight (%s first)", who, wait_name); return LSDR_E_ARG; }
    return LSDR_OK;
  }
  int upload(hipStream_t s) {
    LSDR_HIP(hipMemcpyAsync(d_caps, h_caps, n * sizeof(Cap), hipMemcpyHostToDevice, s));
    return LSDR_OK;
  }
  int mark(hipStream_t s) {
    LSDR_HIP(hipEventRecord(ev_done, s));
    in_flight = true;
    return LSDR_OK;
  }
  int wait(const char *who) {
    if (!in_flight) { lsdr_set_error("%s: no run in flight", who); return LSDR_E_ARG; }
    LSDR_HIP(hipEventSynchronize(ev_done));
    in_flight = false;
    return LSDR_OK;
  }
  void destroy() {
    if (ev_done) (void)hipEventDestroy(ev_done);
    if (d_caps) (void)hipFree(d_caps);
    if (h_caps) (void)hipHostFree(h_caps);
  }
};
// the rest of an object's buffers at destroy (null: never allocated)
inline void lsdr_in_free(std::initializer_list<void *> device, std::initializer_list<void *> pinned) {
  for (void *p : device) if (p) (void)hipFree(p);
  for (void *p : pinned) if (p) (void)hipHostFree(p);
}
#endif
