// leansdr_amd/csrc/tune_est.hip — lsdr_tune_est: every capture's carrier offset estimated from its raw samples, for the batch decoders'
// per-capture tune (lsdr_capture_each.tune, include/lsdr_hip.h).  No decode kernel is involved: the estimator reads the capture, the host
// reads B records, and the caller hands the numbers to lsdr_capture_each_run_async / lsdr_hs_each_run_async.
//
// The estimator (QPSK): the fourth power of a QPSK signal carries no modulation and has a spectral line at 4·f.  For one capture of n items,
// M = min(blocks, n / 4096) whole blocks of N = 4096 samples from its first sample; per block the converted samples are divided by the block's
// RMS (so level and format cannot overflow the fourth power; an all-zero block contributes zeros), w = z⁴, X = FFT_N(w) with a rectangular
// window; P[k] = Σ_blocks |X[k]|² in block order; the first arg-max of P with its two cyclic neighbours gives the fractional bin
// (tune_est_device.h: te_peak_record), tune = κ/(4N).
//
//   k_te_block<K>   blockIdx.y = capture, blockIdx.x = block, one workgroup of 256: 16-byte loads (item-wise where the capture's pointer is
//                   only item-aligned: the same values), the converted block in LDS (32 KB), its RMS, z⁴ in place, six radix-4 stages,
//                   |X|² in natural order as one row of 4096 floats of scratch
//   k_te_peak       one workgroup per capture: the rows summed in block order, first maximum, neighbours, mean; thread 0 writes the record
//
// Determinism: no atomics; every sum has a fixed order that depends on the sample's index alone (the samples reach LDS first, the RMS is
// then summed by a layout that does not know the item size: thread t takes samples t, t + 256, …), so a capture's record is a pure function
// of its converted samples — the same bits alone, in any batch, in any place of it, and for every format that converts to the same floats.
// Both kernels leave by the capture's own block count: nothing is read behind block M − 1 of a capture, and nothing at all of one with M = 0.
#include <cmath>
#include "capture_input.h"
#include "tune_est_device.h"

namespace {

struct te_cap { const unsigned char *in; unsigned blocks, pad; };
struct te_args {
  const te_cap *caps;
  const float2 *tw;                    // [4096] exp(−j2π·i/4096)
  float *rows;                         // [captures][row_cap][4096] |X|² of every block
  te_record *rec;                      // [captures]
  unsigned row_cap;
  float in_scale;
  unsigned in_flip;
};
static_assert(sizeof(te_record) == sizeof(lsdr_tune_estimate) && sizeof(te_record) == 32, "lsdr_tune_estimate is te_record");

// Σ over the workgroup of 256, the same value in every thread: lanes by xor-shuffles, the four wavefronts in order
__device__ __forceinline__ float te_sum256(float v, float *red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

template <int K>
__global__ __launch_bounds__(256) void k_te_block(te_args A) {
  const te_cap cap = A.caps[blockIdx.y];
  if (blockIdx.x >= cap.blocks) return;
  __shared__ float2 x[kTeN];
  __shared__ float red[4];
  constexpr unsigned kB = in_item<K>::kBytes, kPer = 16u / kB;
  const unsigned t = threadIdx.x;
  const unsigned char *src = cap.in + (size_t)blockIdx.x * kTeN * kB;
  // One 16-byte piece per thread and pass.  The alignment is decided once, in front of the loop, and the loop stays rolled: the registers
  // of this kernel are the FFT's, and a workgroup's loads overlap with the FFTs of the others on its CU.
  auto stage = [&](auto wide) {
#pragma unroll 1
    for (unsigned l = 0; l < kTeN / (256u * kPer); ++l) {
      const unsigned s0 = (l * 256u + t) * kPer;
      float2 z[kPer];
      in_piece<K>(src, s0, wide(), A.in_scale, A.in_flip, z);
#pragma unroll
      for (unsigned q = 0; q < kPer; ++q) x[s0 + q] = z[q];
    }
  };
  if (((size_t)src & 15u) == 0) stage(std::true_type());     // (a block is a multiple of 16 bytes: the capture's own alignment decides)
  else stage(std::false_type());
  __syncthreads();
  float p = 0.f;
  for (unsigned i = 0; i < kTeN / 256u; ++i) { const float2 z = x[t + 256u * i]; p += z.x * z.x + z.y * z.y; }
  const float sum = te_sum256(p, red);
  const float inv = sum > 0.f ? 1.0f / sqrtf(sum * (1.0f / (float)kTeN)) : 0.f;
  for (unsigned i = 0; i < kTeN / 256u; ++i) x[t + 256u * i] = te_pow4(x[t + 256u * i], inv);     // (each thread its own samples: no barrier in front)
  for (unsigned s = 0; s < kTeLog4; ++s) {
    __syncthreads();
    te_fft_stage(x, A.tw, s, t);
  }
  __syncthreads();
  float *row = A.rows + ((size_t)blockIdx.y * A.row_cap + blockIdx.x) * kTeN;
  for (unsigned i = 0; i < kTeN / 256u; ++i) {
    const unsigned k = t + 256u * i;
    const float2 v = x[te_digit_reverse(k)];
    row[k] = v.x * v.x + v.y * v.y;
  }
}

__global__ __launch_bounds__(256) void k_te_peak(te_args A) {
  const te_cap cap = A.caps[blockIdx.x];
  const unsigned t = threadIdx.x;
  if (cap.blocks == 0) {
    if (t == 0) A.rec[blockIdx.x] = te_record{};             // no whole block: all zeros
    return;
  }
  __shared__ float P[kTeN];
  __shared__ float red[4], bestv[4];
  __shared__ unsigned bestk[4];
  const float *rows = A.rows + (size_t)blockIdx.x * A.row_cap * kTeN;
  float sum = 0.f, best = -1.f;
  unsigned bk = 0;
  for (unsigned i = 0; i < kTeN / 256u; ++i) {
    const unsigned k = t + 256u * i;
    float p = 0.f;
    for (unsigned b = 0; b < cap.blocks; ++b) p += rows[(size_t)b * kTeN + k];
    P[k] = p; sum += p;
    if (p > best) { best = p; bk = k; }                      // ascending k: the first maximum of this thread's bins
  }
  // the first maximum of all: the larger power, the smaller bin among equals
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float ov = __shfl_xor(best, d, 64);
    const unsigned ok = (unsigned)__shfl_xor((int)bk, d, 64);
    if (ov > best || (ov == best && ok < bk)) { best = ov; bk = ok; }
  }
  if ((t & 63u) == 0) { bestv[t >> 6] = best; bestk[t >> 6] = bk; }
  const float total = te_sum256(sum, red);                   // (its barrier publishes P, bestv and bestk as well)
  if (t == 0) {
    for (unsigned w = 1; w < 4; ++w)
      if (bestv[w] > best || (bestv[w] == best && bestk[w] < bk)) { best = bestv[w]; bk = bestk[w]; }
    A.rec[blockIdx.x] = te_peak_record(bk, P[(bk + kTeN - 1u) & (kTeN - 1u)], P[bk], P[(bk + 1u) & (kTeN - 1u)], total, cap.blocks);
  }
}

}  // namespace

struct lsdr_tune_est {
  lsdr_ctx *ctx = nullptr;
  lsdr_tune_est_cfg cfg{};
  unsigned blocks = 0;                 // cfg.blocks with the default filled in
  lsdr_in_desc in{};
  te_args A{};
  in_run<te_cap> run;
  te_record *h_rec = nullptr, *d_rec = nullptr;       // pinned / device
  float2 *d_tw = nullptr;
  float *d_rows = nullptr;
};

extern "C" {

void lsdr_tune_est_destroy(lsdr_tune_est *e) {
  if (!e) return;
  (void)hipStreamSynchronize(e->ctx->stream);
  e->run.destroy();
  lsdr_in_free({e->d_rec, e->d_tw, e->d_rows}, {e->h_rec});
  delete e;
}

static int te_build(lsdr_tune_est *e) {
  lsdr_ctx *c = e->ctx;
  const size_t B = (size_t)e->cfg.n_captures;
  LSDR_HIP(hipSetDevice(c->device));
  LSDR_TRY(e->run.create(B));
  LSDR_HIP(hipHostMalloc((void **)&e->h_rec, B * sizeof(te_record), hipHostMallocDefault));
  memset(e->h_rec, 0, B * sizeof(te_record));
  LSDR_HIP(hipMalloc((void **)&e->d_rec, B * sizeof(te_record)));
  LSDR_HIP(hipMalloc((void **)&e->d_tw, kTeN * sizeof(float2)));
  LSDR_HIP(hipMalloc((void **)&e->d_rows, B * e->blocks * kTeN * sizeof(float)));
  std::vector<float2> tw(kTeN);
  for (unsigned i = 0; i < kTeN; ++i) {
    const double a = -2.0 * M_PI * (double)i / (double)kTeN;
    tw[i] = make_float2((float)cos(a), (float)sin(a));
  }
  LSDR_HIP(hipMemcpy(e->d_tw, tw.data(), kTeN * sizeof(float2), hipMemcpyHostToDevice));
  te_args &A = e->A;
  A.caps = e->run.d_caps; A.tw = e->d_tw; A.rows = e->d_rows; A.rec = e->d_rec; A.row_cap = e->blocks;
  A.in_scale = e->in.in_scale; A.in_flip = e->in.in_flip;
  return LSDR_OK;
}

int lsdr_tune_est_create(lsdr_ctx *c, const lsdr_tune_est_cfg *cfg, lsdr_tune_est **out) {
  LSDR_ARG(c && cfg && out);
  if (cfg->n_captures < 1) { lsdr_set_error("tune_est: n_captures must be at least 1 (got %d)", cfg->n_captures); return LSDR_E_ARG; }
  lsdr_in_desc in;
  LSDR_TRY(lsdr_in_describe("tune_est", cfg->in_format, cfg->in_scale, &in));
  if (cfg->blocks > kTeMaxBlocks) { lsdr_set_error("tune_est: blocks is %u, at most %u", cfg->blocks, kTeMaxBlocks); return LSDR_E_ARG; }
  for (int i = 0; i < 4; ++i)
    if (cfg->reserved[i]) { lsdr_set_error("tune_est: lsdr_tune_est_cfg.reserved must be 0"); return LSDR_E_ARG; }
  lsdr_tune_est *e = new lsdr_tune_est();
  e->ctx = c; e->cfg = *cfg; e->in = in;
  e->blocks = cfg->blocks ? cfg->blocks : 8u;
  const int rc = te_build(e);
  if (rc) { lsdr_tune_est_destroy(e); return rc; }
  *out = e;
  return LSDR_OK;
}

int lsdr_tune_est_run_async(lsdr_tune_est *e, const void *const *iq_dev, const size_t *n_samples) {
  LSDR_ARG(e && iq_dev && n_samples);
  const unsigned B = (unsigned)e->cfg.n_captures;
  LSDR_TRY(lsdr_in_check_each("tune_est", "tune", B, iq_dev, nullptr, n_samples, nullptr, ~(size_t)0, e->in.item_bytes));   // (any length: whole blocks of its front are read)
  LSDR_TRY(e->run.idle("tune_est", "lsdr_tune_est_wait"));
  lsdr_ctx *c = e->ctx;
  LSDR_HIP(hipSetDevice(c->device));
  unsigned longest = 0;                                      // the grid is sized for it; a shorter capture's workgroups leave at once
  for (unsigned i = 0; i < B; ++i) {
    const size_t whole = n_samples[i] / kTeN;
    te_cap &cap = e->run.h_caps[i];
    cap.in = reinterpret_cast<const unsigned char *>(iq_dev[i]);
    cap.blocks = whole < e->blocks ? (unsigned)whole : e->blocks;
    cap.pad = 0;
    if (cap.blocks > longest) longest = cap.blocks;
  }
  LSDR_TRY(e->run.upload(c->stream));
  if (longest)
    in_dispatch(e->in.kind, [&](auto K) { hipLaunchKernelGGL(k_te_block<K()>, dim3(longest, B), dim3(256), 0, c->stream, e->A); });
  hipLaunchKernelGGL(k_te_peak, dim3(B), dim3(256), 0, c->stream, e->A);
  LSDR_HIP(hipGetLastError());
  LSDR_HIP(hipMemcpyAsync(e->h_rec, e->d_rec, B * sizeof(te_record), hipMemcpyDeviceToHost, c->stream));
  return e->run.mark(c->stream);
}

int lsdr_tune_est_wait(lsdr_tune_est *e, lsdr_tune_estimate *out) {
  LSDR_ARG(e && out);
  LSDR_TRY(e->run.wait("tune_est"));
  memcpy(out, e->h_rec, (size_t)e->cfg.n_captures * sizeof(te_record));
  return LSDR_OK;
}

}  // extern "C"
