// leansdr_amd/csrc/rate_est.hip — lsdr_rate_est: every capture's samples per symbol estimated from its raw samples, for the batch decoders'
// omega (lsdr_capture_batch_cfg, lsdr_hs_batch_cfg, lsdr_resample_design).  No decode kernel is involved: the estimator reads the capture,
// the host reads B records, and the caller groups the captures by rate and makes one decoder per group.
//
// The estimator (PSK with root-raised-cosine shaping): the squared magnitude of such a signal has a spectral line at the symbol rate,
// wherever the carrier is.  For one capture of n items, M = min(blocks, n / 4096) whole blocks of N = 4096 samples from its first sample;
// per block s = mean |z|², p[n] = |z[n]|²/s − 1 (an all-zero block contributes zeros), X = FFT_N(p) with a rectangular window;
// P[k] = Σ_blocks |X[k]|² in block order; c₁ = Σ_blocks Σ_{n ≥ 1} z[n]·conj(z[n − 1]) / s.  The first arg-max of P over [k_lo, N/2] with its
// two neighbours above the floor gives the line; the lag-one correlation R = |c₁| / (M₁·(N − 1)) chooses between omega = 1/line and its
// alias 1/(1 − line) (rate_est_device.h: re_peak_record).  The staging, the workgroup sums, the transform, the first maximum and the host's
// frame are block_spectrum.h's, shared with tune_est.hip; here are the three sums, the half row, the blocks' stats and the record.
//
//   k_re_block<K>   blockIdx.y = capture, blockIdx.x = block, one workgroup of 256: 16-byte loads (item-wise where the capture's pointer is
//                   only item-aligned: the same values), the converted block in LDS (32 KB), Σ|z|² and the lag-one sum, p in place, the
//                   six radix-4 stages, |X|² of bins 0 … N/2 as one row of scratch, the block's (c₁/s, s) beside it
//   k_re_peak       one workgroup per capture: the rows and the blocks' c₁ summed in block order, first maximum, floor; thread 0 writes
//                   the record
//
// Determinism: no atomics; every sum has a fixed order that depends on the sample's or the bin's index alone (the samples reach LDS first:
// thread t takes samples t, t + 256, … whatever the item size), so a capture's record is a pure function of its converted samples — the same
// bits alone, in any batch, in any place of it, and for every format that converts to the same floats.  Both kernels leave by the capture's
// own block count: nothing is read behind block M − 1 of a capture, and nothing at all of one with M = 0.
#include <cmath>
#include "rate_est_device.h"

namespace {

struct re_args {
  const bs_cap *caps;
  const float2 *tw;                    // [4096] exp(−j2π·i/4096)
  float *rows;                         // [captures][row_cap][kReRow] |X|² of every block, bins 0 … N/2
  float4 *stats;                       // [captures][row_cap] (re c₁/s, im c₁/s, s, 1) of every block; all zeros for a block with s = 0
  re_record *rec;                      // [captures]
  unsigned row_cap, k_lo;
  float in_scale;
  unsigned in_flip;
  float omega_min, omega_max;
};
static_assert(sizeof(re_record) == sizeof(lsdr_rate_estimate) && sizeof(re_record) == 48, "lsdr_rate_estimate is re_record");

template <int K>
__global__ __launch_bounds__(256) void k_re_block(re_args A) {
  const bs_cap cap = A.caps[blockIdx.y];
  if (blockIdx.x >= cap.blocks) return;
  __shared__ float2 x[kReN];
  __shared__ float red[3][4];
  const unsigned t = threadIdx.x;
  bs_stage<K>(cap.in, blockIdx.x, A.in_scale, A.in_flip, x);
  // Σ|z|² and Σ_{n ≥ 1} z[n]·conj(z[n − 1]): thread t takes n = t, t + 256, …
  float v[3] = {0.f, 0.f, 0.f};
  for (unsigned i = 0; i < kReN / 256u; ++i) {
    const unsigned n = t + 256u * i;
    const float2 z = x[n];
    v[0] += z.x * z.x + z.y * z.y;
    if (n) {
      const float2 y = x[n - 1u];
      v[1] += z.x * y.x + z.y * y.y;
      v[2] += z.y * y.x - z.x * y.y;
    }
  }
  bs_sum256(v, red);                                         // (its barrier is behind every read of a neighbour's sample)
  const float s = v[0] * (1.0f / (float)kReN);
  const float inv = s > 0.f ? 1.0f / s : 0.f;
  for (unsigned i = 0; i < kReN / 256u; ++i) {
    const float2 z = x[t + 256u * i];
    x[t + 256u * i] = make_float2(s > 0.f ? (z.x * z.x + z.y * z.y) * inv - 1.0f : 0.f, 0.f);
  }
  bs_fft(x, A.tw);
  const size_t slot = (size_t)blockIdx.y * A.row_cap + blockIdx.x;
  float *row = A.rows + slot * kReRow;
  for (unsigned i = 0; i <= kReHalf / 256u; ++i) {
    const unsigned k = t + 256u * i;
    if (k <= kReHalf) {
      const float2 X = x[bs_digit_reverse(k)];
      row[k] = X.x * X.x + X.y * X.y;
    }
  }
  if (t == 0) A.stats[slot] = s > 0.f ? make_float4(v[1] * inv, v[2] * inv, s, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(256) void k_re_peak(re_args A) {
  const bs_cap cap = A.caps[blockIdx.x];
  const unsigned t = threadIdx.x;
  if (cap.blocks == 0) {
    if (t == 0) A.rec[blockIdx.x] = re_record{};             // no whole block: all zeros
    return;
  }
  __shared__ float P[kReHalf + 1u];
  __shared__ float4 st[kReMaxBlocks];
  __shared__ bs_peak_lds sh;
  const float *rows = A.rows + (size_t)blockIdx.x * A.row_cap * kReRow;
  if (t < cap.blocks) st[t] = A.stats[(size_t)blockIdx.x * A.row_cap + t];
  float sum = 0.f, best = -1.f;
  unsigned bk = 0;
  for (unsigned i = 0; i <= kReHalf / 256u; ++i) {
    const unsigned k = t + 256u * i;
    if (k > kReHalf) break;
    float p = 0.f;
    for (unsigned b = 0; b < cap.blocks; ++b) p += rows[(size_t)b * kReRow + k];
    P[k] = p;
    if (k >= A.k_lo) {
      sum += p;
      if (p > best) { best = p; bk = k; }                    // ascending k: the first maximum of this thread's bins
    }
  }
  bs_first_max(best, bk, sum, sh);                           // (a thread without a searched bin holds −1; its barrier publishes P and st as well)
  if (t == 0) {
    const float floor_ = sum / (float)(kReHalf - A.k_lo + 1u);
    double cre = 0.0, cim = 0.0;                             // (the blocks' c₁ in block order, in double like the rest of the record)
    unsigned m1 = 0;
    for (unsigned b = 0; b < cap.blocks; ++b) { cre += (double)st[b].x; cim += (double)st[b].y; m1 += st[b].w != 0.f ? 1u : 0u; }
    const float corr = m1 ? (float)(sqrt(cre * cre + cim * cim) / ((double)m1 * (double)(kReN - 1u))) : 0.f;
    // (k_lo ≥ 2: bin bk − 1 exists; behind N/2 the spectrum of a real sequence mirrors)
    A.rec[blockIdx.x] = re_peak_record(bk, P[bk - 1u], P[bk], bk == kReHalf ? P[bk - 1u] : P[bk + 1u], floor_, corr, cap.blocks, A.omega_min, A.omega_max);
  }
}

}  // namespace

struct lsdr_rate_est {
  lsdr_ctx *ctx = nullptr;
  lsdr_rate_est_cfg cfg{};
  lsdr_in_desc in{};
  re_args A{};
  bs_host<re_record> host;
  float *d_rows = nullptr;
  float4 *d_stats = nullptr;
};

extern "C" {

void lsdr_rate_est_destroy(lsdr_rate_est *e) {
  if (!e) return;
  e->host.destroy(e->ctx, {e->d_rows, e->d_stats});
  delete e;
}

static int re_build(lsdr_rate_est *e, unsigned blocks, float omega_min, float omega_max) {
  const size_t B = (size_t)e->cfg.n_captures;
  LSDR_TRY(e->host.create(e->ctx, B, blocks));
  LSDR_HIP(hipMalloc((void **)&e->d_rows, B * blocks * kReRow * sizeof(float)));
  LSDR_HIP(hipMalloc((void **)&e->d_stats, B * blocks * sizeof(float4)));
  re_args &A = e->A;
  A.caps = e->host.run.d_caps; A.tw = e->host.d_tw; A.rows = e->d_rows; A.stats = e->d_stats; A.rec = e->host.d_rec; A.row_cap = blocks;
  A.k_lo = re_k_lo(omega_min, omega_max);
  A.in_scale = e->in.in_scale; A.in_flip = e->in.in_flip;
  A.omega_min = omega_min; A.omega_max = omega_max;
  return LSDR_OK;
}

int lsdr_rate_est_create(lsdr_ctx *c, const lsdr_rate_est_cfg *cfg, lsdr_rate_est **out) {
  LSDR_ARG(c && cfg && out);
  LSDR_TRY(bs_check_captures("rate_est", cfg->n_captures));
  lsdr_in_desc in;
  LSDR_TRY(lsdr_in_describe("rate_est", cfg->in_format, cfg->in_scale, &in));
  if (cfg->blocks > kReMaxBlocks) { lsdr_set_error("rate_est: blocks is %u, at most %u", cfg->blocks, kReMaxBlocks); return LSDR_E_ARG; }
  const float lo = cfg->omega_min == 0.f ? kReOmegaMin : cfg->omega_min, hi = cfg->omega_max == 0.f ? kReOmegaMax : cfg->omega_max;
  if (!(lo >= kReOmegaMin && lo <= kReOmegaMax)) { lsdr_set_error("rate_est: omega_min must lie in [1.016, 64] (0: 1.016)"); return LSDR_E_ARG; }
  if (!(hi >= kReOmegaMin && hi <= kReOmegaMax)) { lsdr_set_error("rate_est: omega_max must lie in [1.016, 64] (0: 64)"); return LSDR_E_ARG; }
  if (lo > hi) { lsdr_set_error("rate_est: omega_min %g is above omega_max %g", (double)lo, (double)hi); return LSDR_E_ARG; }
  for (int i = 0; i < 2; ++i)
    if (cfg->reserved[i]) { lsdr_set_error("rate_est: lsdr_rate_est_cfg.reserved must be 0"); return LSDR_E_ARG; }
  lsdr_rate_est *e = new lsdr_rate_est();
  e->ctx = c; e->cfg = *cfg; e->in = in;
  const int rc = re_build(e, cfg->blocks ? cfg->blocks : 64u, lo, hi);
  if (rc) { lsdr_rate_est_destroy(e); return rc; }
  *out = e;
  return LSDR_OK;
}

int lsdr_rate_est_run_async(lsdr_rate_est *e, const void *const *iq_dev, const size_t *n_samples) {
  LSDR_ARG(e && iq_dev && n_samples);
  lsdr_ctx *c = e->ctx;
  const unsigned B = (unsigned)e->cfg.n_captures;
  unsigned longest = 0;
  LSDR_TRY(e->host.begin(c, "rate_est", "lsdr_rate_est_wait", iq_dev, n_samples, e->in.item_bytes, &longest));
  if (longest)
    in_dispatch(e->in.kind, [&](auto K) { hipLaunchKernelGGL(k_re_block<K()>, dim3(longest, B), dim3(256), 0, c->stream, e->A); });
  hipLaunchKernelGGL(k_re_peak, dim3(B), dim3(256), 0, c->stream, e->A);
  return e->host.end(c);
}

int lsdr_rate_est_wait(lsdr_rate_est *e, lsdr_rate_estimate *out) {
  LSDR_ARG(e && out);
  return e->host.wait("rate_est", out);
}

}  // extern "C"
