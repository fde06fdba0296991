// leansdr_amd/csrc/tune_est.hip — lsdr_tune_est: every capture's carrier offset estimated from its raw samples, for the batch decoders'
// per-capture tune (lsdr_capture_each.tune, include/lsdr_hip.h).  No decode kernel is involved: the estimator reads the capture, the host
// reads B records, and the caller hands the numbers to lsdr_capture_each_run_async / lsdr_hs_each_run_async.
//
// The estimator (QPSK): the fourth power of a QPSK signal carries no modulation and has a spectral line at 4·f.  For one capture of n items,
// M = min(blocks, n / 4096) whole blocks of N = 4096 samples from its first sample; per block the converted samples are divided by the block's
// RMS (so level and format cannot overflow the fourth power; an all-zero block contributes zeros), w = z⁴, X = FFT_N(w) with a rectangular
// window; P[k] = Σ_blocks |X[k]|² in block order; the first arg-max of P with its two cyclic neighbours gives the fractional bin
// (tune_est_device.h: te_peak_record), tune = κ/(4N).  The staging, the workgroup sums, the transform, the first maximum and the host's
// frame are block_spectrum.h's, shared with rate_est.hip; here are the fourth power, the full row and the record.
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
#include "tune_est_device.h"

namespace {

struct te_args {
  const bs_cap *caps;
  const float2 *tw;                    // [4096] exp(−j2π·i/4096)
  float *rows;                         // [captures][row_cap][4096] |X|² of every block
  te_record *rec;                      // [captures]
  unsigned row_cap;
  float in_scale;
  unsigned in_flip;
};
static_assert(sizeof(te_record) == sizeof(lsdr_tune_estimate) && sizeof(te_record) == 32, "lsdr_tune_estimate is te_record");

template <int K>
__global__ __launch_bounds__(256) void k_te_block(te_args A) {
  const bs_cap cap = A.caps[blockIdx.y];
  if (blockIdx.x >= cap.blocks) return;
  __shared__ float2 x[kTeN];
  __shared__ float red[1][4];
  const unsigned t = threadIdx.x;
  bs_stage<K>(cap.in, blockIdx.x, A.in_scale, A.in_flip, x);
  float p[1] = {0.f};
  for (unsigned i = 0; i < kTeN / 256u; ++i) { const float2 z = x[t + 256u * i]; p[0] += z.x * z.x + z.y * z.y; }
  bs_sum256(p, red);
  const float inv = p[0] > 0.f ? 1.0f / sqrtf(p[0] * (1.0f / (float)kTeN)) : 0.f;
  for (unsigned i = 0; i < kTeN / 256u; ++i) x[t + 256u * i] = te_pow4(x[t + 256u * i], inv);     // (each thread its own samples: no barrier in front)
  bs_fft(x, A.tw);
  float *row = A.rows + ((size_t)blockIdx.y * A.row_cap + blockIdx.x) * kTeN;
  for (unsigned i = 0; i < kTeN / 256u; ++i) {
    const unsigned k = t + 256u * i;
    const float2 v = x[bs_digit_reverse(k)];
    row[k] = v.x * v.x + v.y * v.y;
  }
}

__global__ __launch_bounds__(256) void k_te_peak(te_args A) {
  const bs_cap cap = A.caps[blockIdx.x];
  const unsigned t = threadIdx.x;
  if (cap.blocks == 0) {
    if (t == 0) A.rec[blockIdx.x] = te_record{};             // no whole block: all zeros
    return;
  }
  __shared__ float P[kTeN];
  __shared__ bs_peak_lds sh;
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
  bs_first_max(best, bk, sum, sh);                           // (its barrier publishes P as well)
  if (t == 0) A.rec[blockIdx.x] = te_peak_record(bk, P[(bk + kTeN - 1u) & (kTeN - 1u)], P[bk], P[(bk + 1u) & (kTeN - 1u)], sum, cap.blocks);
}

}  // namespace

struct lsdr_tune_est {
  lsdr_ctx *ctx = nullptr;
  lsdr_tune_est_cfg cfg{};
  lsdr_in_desc in{};
  te_args A{};
  bs_host<te_record> host;
  float *d_rows = nullptr;
};

extern "C" {

void lsdr_tune_est_destroy(lsdr_tune_est *e) {
  if (!e) return;
  e->host.destroy(e->ctx, {e->d_rows});
  delete e;
}

static int te_build(lsdr_tune_est *e, unsigned blocks) {
  LSDR_TRY(e->host.create(e->ctx, (size_t)e->cfg.n_captures, blocks));
  LSDR_HIP(hipMalloc((void **)&e->d_rows, (size_t)e->cfg.n_captures * blocks * kTeN * sizeof(float)));
  te_args &A = e->A;
  A.caps = e->host.run.d_caps; A.tw = e->host.d_tw; A.rows = e->d_rows; A.rec = e->host.d_rec; A.row_cap = blocks;
  A.in_scale = e->in.in_scale; A.in_flip = e->in.in_flip;
  return LSDR_OK;
}

int lsdr_tune_est_create(lsdr_ctx *c, const lsdr_tune_est_cfg *cfg, lsdr_tune_est **out) {
  LSDR_ARG(c && cfg && out);
  LSDR_TRY(bs_check_captures("tune_est", cfg->n_captures));
  lsdr_in_desc in;
  LSDR_TRY(lsdr_in_describe("tune_est", cfg->in_format, cfg->in_scale, &in));
  if (cfg->blocks > kTeMaxBlocks) { lsdr_set_error("tune_est: blocks is %u, at most %u", cfg->blocks, kTeMaxBlocks); return LSDR_E_ARG; }
  for (int i = 0; i < 4; ++i)
    if (cfg->reserved[i]) { lsdr_set_error("tune_est: lsdr_tune_est_cfg.reserved must be 0"); return LSDR_E_ARG; }
  lsdr_tune_est *e = new lsdr_tune_est();
  e->ctx = c; e->cfg = *cfg; e->in = in;
  const int rc = te_build(e, cfg->blocks ? cfg->blocks : 8u);
  if (rc) { lsdr_tune_est_destroy(e); return rc; }
  *out = e;
  return LSDR_OK;
}

int lsdr_tune_est_run_async(lsdr_tune_est *e, const void *const *iq_dev, const size_t *n_samples) {
  LSDR_ARG(e && iq_dev && n_samples);
  lsdr_ctx *c = e->ctx;
  const unsigned B = (unsigned)e->cfg.n_captures;
  unsigned longest = 0;
  LSDR_TRY(e->host.begin(c, "tune_est", "lsdr_tune_est_wait", iq_dev, n_samples, e->in.item_bytes, &longest));
  if (longest)
    in_dispatch(e->in.kind, [&](auto K) { hipLaunchKernelGGL(k_te_block<K()>, dim3(longest, B), dim3(256), 0, c->stream, e->A); });
  hipLaunchKernelGGL(k_te_peak, dim3(B), dim3(256), 0, c->stream, e->A);
  return e->host.end(c);
}

int lsdr_tune_est_wait(lsdr_tune_est *e, lsdr_tune_estimate *out) {
  LSDR_ARG(e && out);
  return e->host.wait("tune_est", out);
}

}  // extern "C"
