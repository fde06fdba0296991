// leansdr_amd/csrc/block_spectrum.h — what the estimators on raw captures share (lsdr_tune_est: tune_est.hip, lsdr_rate_est: rate_est.hip,
// lsdr_carrier_scan: carrier_scan.hip):
// a capture is cut into whole blocks of 4096 samples, one workgroup of 256 turns a block into LDS, applies its own point-wise step, takes the
// 4096-point FFT and writes |X|² as a row of scratch; a second kernel, one workgroup per capture, sums the rows and finds the first maximum.
// An estimator adds its point-wise step, its row layout and its record; the samples' conversion is capture_input.h's.
//   kBsN, kBsLog4, bs_cmul, bs_fft_stage, bs_digit_reverse   plain C++ on values, callable from a kernel and from the host
//   bs_cap, bs_stage, bs_sum256, bs_fft, bs_first_max        the kernels' shared steps
//   bs_check_captures, bs_host                               the host side: buffers, twiddles, the frame of run_async, wait, destroy
#ifndef LSDR_BLOCK_SPECTRUM_H
#define LSDR_BLOCK_SPECTRUM_H
#include <vector>
#include "capture_input.h"

constexpr unsigned kBsN = 4096;          // samples per block, FFT length
constexpr unsigned kBsLog4 = 6;          // radix-4 stages

IN_HD float2 bs_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// Stage s (0 … 5) of the in-place radix-4 decimation-in-frequency FFT of x[4096], the share of thread `tid` of 256: four butterflies.
// Sub-transform length L = 4096 / 4^s, quarter q = L / 4; tw[i] = exp(−j2π·i/4096).  Output m of a butterfly goes to quarter m, so X[k]
// ends up where bs_digit_reverse(k) says.  A barrier belongs between two stages.
IN_HD void bs_fft_stage(float2 *x, const float2 *tw, unsigned s, unsigned tid) {
  const unsigned lq = 10u - 2u * s, q = 1u << lq;
  for (unsigned i = 0; i < 4; ++i) {
    const unsigned b = tid + 256u * i;                       // butterfly 0 … 1023
    const unsigned j = b & (q - 1u), base = ((b >> lq) << (lq + 2u)) + j;
    const unsigned tj = j << (2u * s);                       // j·4096/L
    const float2 a0 = x[base], a1 = x[base + q], a2 = x[base + 2u * q], a3 = x[base + 3u * q];
    const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y), t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
    const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y);
    const float2 t3 = make_float2(a1.y - a3.y, -(a1.x - a3.x));                  // −j·(a1 − a3)
    x[base] = make_float2(t0.x + t2.x, t0.y + t2.y);
    x[base + q] = bs_cmul(make_float2(t1.x + t3.x, t1.y + t3.y), tw[tj]);
    x[base + 2u * q] = bs_cmul(make_float2(t0.x - t2.x, t0.y - t2.y), tw[2u * tj]);
    x[base + 3u * q] = bs_cmul(make_float2(t1.x - t3.x, t1.y - t3.y), tw[3u * tj]);
  }
}
// where X[k] sits behind the six stages: k's base-4 digits reversed
IN_HD unsigned bs_digit_reverse(unsigned k) {
  unsigned p = 0;
  for (unsigned d = 0; d < kBsLog4; ++d) { p = (p << 2) | (k & 3u); k >>= 2; }
  return p;
}

// ---- the kernels' shared steps (a workgroup of 256) -------------------------------------------------------------------------------------
struct bs_cap { const unsigned char *in; unsigned blocks, pad; };          // one capture of a run: its samples, its whole blocks (at most the object's); pad: 0, or begin's spread

// Block `block` of the capture at `in`, converted, into x[4096]: one 16-byte piece per thread and pass (item-wise where the capture's pointer
// is only item-aligned: the same values).  The alignment is decided once, in front of the loop, and the loop stays rolled: the registers of
// the block kernels are the FFT's, and a workgroup's loads overlap with the FFTs of the others on its CU.  Ends behind its barrier.
template <int K>
__device__ __forceinline__ void bs_stage(const unsigned char *in, unsigned block, float in_scale, unsigned in_flip, float2 *x) {
  constexpr unsigned kB = in_item<K>::kBytes, kPer = 16u / kB;
  const unsigned t = threadIdx.x;
  const unsigned char *src = in + (size_t)block * kBsN * kB;
  auto stage = [&](auto wide) {
#pragma unroll 1
    for (unsigned l = 0; l < kBsN / (256u * kPer); ++l) {
      const unsigned s0 = (l * 256u + t) * kPer;
      float2 z[kPer];
      in_piece<K>(src, s0, wide(), in_scale, in_flip, z);
#pragma unroll
      for (unsigned q = 0; q < kPer; ++q) x[s0 + q] = z[q];
    }
  };
  if (((size_t)src & 15u) == 0) stage(std::true_type());     // (a block is a multiple of 16 bytes: the capture's own alignment decides)
  else stage(std::false_type());
  __syncthreads();
}

// Σ over the workgroup of Q values at once, the same in every thread: lanes by xor-shuffles, the four wavefronts in order.  Its barrier
// stands behind everything the workgroup read or wrote in front of it.
template <int Q>
__device__ __forceinline__ void bs_sum256(float (&v)[Q], float (*red)[4]) {
#pragma unroll
  for (int q = 0; q < Q; ++q) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[q] += __shfl_xor(v[q], d, 64);
    if ((threadIdx.x & 63u) == 0) red[q][threadIdx.x >> 6] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < Q; ++q) v[q] = ((red[q][0] + red[q][1]) + red[q][2]) + red[q][3];
}

// x[4096] in LDS to its transform, in place and in digit-reversed order: a barrier in front of every stage and one behind the last
__device__ __forceinline__ void bs_fft(float2 *x, const float2 *tw) {
  for (unsigned s = 0; s < kBsLog4; ++s) {
    __syncthreads();
    bs_fft_stage(x, tw, s, threadIdx.x);
  }
  __syncthreads();
}

// The first maximum of all threads' (best, bk) — the larger power, the smaller bin among equals; a thread without a bin holds −1 — and the
// sum of their `sum`, lanes by xor-shuffles, the four wavefronts in order: thread 0 leaves with the workgroup's three values.  The one
// barrier publishes what the caller wrote to LDS in front of the call as well.
struct bs_peak_lds { float red[4], bestv[4]; unsigned bestk[4]; };
__device__ __forceinline__ void bs_first_max(float &best, unsigned &bk, float &sum, bs_peak_lds &sh) {
  const unsigned t = threadIdx.x;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float ov = __shfl_xor(best, d, 64);
    const unsigned ok = (unsigned)__shfl_xor((int)bk, d, 64);
    if (ov > best || (ov == best && ok < bk)) { best = ov; bk = ok; }
    sum += __shfl_xor(sum, d, 64);
  }
  if ((t & 63u) == 0) { sh.bestv[t >> 6] = best; sh.bestk[t >> 6] = bk; sh.red[t >> 6] = sum; }
  __syncthreads();
  if (t == 0) {
    for (unsigned w = 1; w < 4; ++w)
      if (sh.bestv[w] > best || (sh.bestv[w] == best && sh.bestk[w] < bk)) { best = sh.bestv[w]; bk = sh.bestk[w]; }
    sum = ((sh.red[0] + sh.red[1]) + sh.red[2]) + sh.red[3];
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// gridDim.y is the capture: checked at create, in front of anything allocated.  who: the owner's prefix in the error texts.
inline int bs_check_captures(const char *who, int n_captures) {
  if (n_captures < 1 || n_captures > 65535) { lsdr_set_error("%s: n_captures must be 1 to 65535 (got %d)", who, n_captures); return LSDR_E_ARG; }
  return LSDR_OK;
}

// What an estimator's object holds beside its scratch, and the frame of its calls: create; begin, the owner's launches, end; wait; destroy.
template <class Rec>
struct bs_host {
  in_run<bs_cap> run;
  Rec *h_rec = nullptr, *d_rec = nullptr;                    // pinned / device, one per capture
  float2 *d_tw = nullptr;                                    // [4096] exp(−j2π·i/4096)
  unsigned blocks = 0;                                       // of a capture at most

  int create(lsdr_ctx *c, size_t captures, unsigned max_blocks) {
    blocks = max_blocks;
    LSDR_HIP(hipSetDevice(c->device));
    LSDR_TRY(run.create(captures));
    LSDR_HIP(hipHostMalloc((void **)&h_rec, captures * sizeof(Rec), hipHostMallocDefault));
    memset(h_rec, 0, captures * sizeof(Rec));
    LSDR_HIP(hipMalloc((void **)&d_rec, captures * sizeof(Rec)));
    LSDR_HIP(hipMalloc((void **)&d_tw, kBsN * sizeof(float2)));
    std::vector<float2> tw(kBsN);
    for (unsigned i = 0; i < kBsN; ++i) {
      const double a = -2.0 * M_PI * (double)i / (double)kBsN;
      tw[i] = make_float2((float)cos(a), (float)sin(a));
    }
    LSDR_HIP(hipMemcpy(d_tw, tw.data(), kBsN * sizeof(float2), hipMemcpyHostToDevice));
    return LSDR_OK;
  }
  // The arguments checked (a refused call leaves the object as it was), every capture's record filled and uploaded.  *longest: the most
  // blocks of any capture; the block kernel's grid is sized for it, and a shorter capture's workgroups leave at once.  spread (the carrier
  // scan's): the record's pad carries max(1, (n / 4096) / blocks), the distance in blocks between two blocks of a scan over the whole capture.
  int begin(lsdr_ctx *c, const char *who, const char *wait_name, const void *const *iq_dev, const size_t *n_samples, unsigned item_bytes, unsigned *longest,
            bool spread = false) {
    const unsigned B = (unsigned)run.n;
    LSDR_TRY(lsdr_in_check_each(who, "tune", B, iq_dev, nullptr, n_samples, nullptr, ~(size_t)0, item_bytes));   // (any length: whole blocks of its front are read)
    LSDR_TRY(run.idle(who, wait_name));
    LSDR_HIP(hipSetDevice(c->device));
    *longest = 0;
    for (unsigned i = 0; i < B; ++i) {
      const size_t whole = n_samples[i] / kBsN;
      bs_cap &cap = run.h_caps[i];
      cap.in = reinterpret_cast<const unsigned char *>(iq_dev[i]);
      cap.blocks = whole < blocks ? (unsigned)whole : blocks;
      cap.pad = spread ? (unsigned)(whole / blocks > 1 ? whole / blocks : 1) : 0;
      if (cap.blocks > *longest) *longest = cap.blocks;
    }
    return run.upload(c->stream);
  }
  int end(lsdr_ctx *c) {
    LSDR_HIP(hipGetLastError());
    LSDR_HIP(hipMemcpyAsync(h_rec, d_rec, run.n * sizeof(Rec), hipMemcpyDeviceToHost, c->stream));
    return run.mark(c->stream);
  }
  int wait(const char *who, void *out) {
    LSDR_TRY(run.wait(who));
    memcpy(out, h_rec, run.n * sizeof(Rec));
    return LSDR_OK;
  }
  void destroy(lsdr_ctx *c, std::initializer_list<void *> scratch) {      // scratch: the owner's device buffers (null: never allocated)
    (void)hipStreamSynchronize(c->stream);
    run.destroy();
    lsdr_in_free({d_rec, d_tw}, {h_rec});
    lsdr_in_free(scratch, {});
  }
};
#endif
