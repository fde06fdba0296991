// leansdr_amd/csrc/carrier_scan.hip — lsdr_carrier_scan: the carriers of every wideband capture found in its averaged power spectrum — where
// they are, how wide, how far above the floor — for the objects that take one carrier each (lsdr_resample_batch with the same pointer and
// B tunes, lsdr_rate_est and lsdr_tune_est on the decimated streams, lsdr_capture_batch).  The host reads B summaries and B·max_carriers
// records; include/lsdr_hip.h has the definition step by step.
//
// For one capture of n items: M = min(blocks, n / 4096) blocks of N = 4096 samples, block b from sample b·stride·N (stride 1, or spread over
// the capture); per block the Hann window (from the twiddle table), the FFT and |X|² of all bins; P = Σ_blocks in block order; S = the
// circular boxcar of P; floor = the value of rank N/8 of S, T = floor·factor; runs of bins with S ≥ T in frequency order, those of at least
// min_bins bins kept, the first max_carriers listed; per listed run the plateau, the half-power edges, centre and width
// (carrier_scan_device.h).  The staging, the transform and the host's frame are block_spectrum.h's.
//
//   k_cs_block<K>   blockIdx.y = capture, blockIdx.x = block, one workgroup of 256: bs_stage, the window in place, the six radix-4 stages,
//                   |X|² of bins 0 … N − 1 in natural order as one row of scratch
//   k_cs_find       one workgroup per capture: P (kept in global memory for lsdr_carrier_scan_spectrum_dev), S, a bitonic sort of S's bit
//                   patterns (non-negative floats order like their bits), the runs by two prefix sums over the threads' counts, one thread
//                   per listed run.  LDS: P, S and the sort buffer at 16 KB each; the run lists reuse the sort buffer.
//
// Determinism: no atomics; every sum has a fixed order that depends on the bin's or the block's index alone, the runs are found in
// integers, so a capture's records are a pure function of its converted samples — the same bits alone, in any batch, in any place of it, and
// for every format that converts to the same floats.  Both kernels leave by the capture's own block count: nothing is read behind the last
// used block of a capture, and nothing at all of one with M = 0.
#include <cmath>
#include "carrier_scan_device.h"

namespace {

struct cs_args {
  const bs_cap *caps;                  // (pad: the stride in blocks; 0 reads as 1)
  const float2 *tw;                    // [4096] exp(−j2π·i/4096)
  float *rows;                         // [captures][row_cap][4096] |X|² of every block
  float *spec;                         // [captures][4096] P
  cs_summary *sum;                     // [captures]
  cs_carrier *car;                     // [captures][max_carriers]
  unsigned row_cap, smooth, min_bins, max_carriers;
  float factor, in_scale;
  unsigned in_flip;
};
static_assert(sizeof(cs_summary) == sizeof(lsdr_scan_summary) && sizeof(cs_summary) == 32, "lsdr_scan_summary is cs_summary");
static_assert(sizeof(cs_carrier) == sizeof(lsdr_scan_carrier) && sizeof(cs_carrier) == 32, "lsdr_scan_carrier is cs_carrier");
static_assert(sizeof(lsdr_carrier_scan_cfg) == 48, "lsdr_carrier_scan_cfg");

__device__ __forceinline__ unsigned cs_stride(const bs_cap &cap) { return cap.pad ? cap.pad : 1u; }

template <int K>
__global__ __launch_bounds__(256) void k_cs_block(cs_args A) {
  const bs_cap cap = A.caps[blockIdx.y];
  if (blockIdx.x >= cap.blocks) return;
  __shared__ float2 x[kCsN];
  const unsigned t = threadIdx.x;
  bs_stage<K>(cap.in, blockIdx.x * cs_stride(cap), A.in_scale, A.in_flip, x);
  for (unsigned i = 0; i < kCsPerThread; ++i) {              // Hann: w[n] = 0.5 − 0.5·cos(2πn/N)
    const unsigned n = t + 256u * i;
    const float w = 0.5f - 0.5f * A.tw[n].x;
    const float2 z = x[n];
    x[n] = make_float2(z.x * w, z.y * w);
  }
  bs_fft(x, A.tw);
  float *row = A.rows + ((size_t)blockIdx.y * A.row_cap + blockIdx.x) * kCsN;
  for (unsigned i = 0; i < kCsPerThread; ++i) {
    const unsigned k = t + 256u * i;
    const float2 X = x[bs_digit_reverse(k)];
    row[k] = X.x * X.x + X.y * X.y;
  }
}

// The exclusive prefix sum of v over the workgroup's 256 threads, and the sum of all in *total: lanes by shuffles, the four wavefronts in
// order.  tot[4] is this call's own; its barrier publishes what the caller wrote to LDS in front of the call as well.
__device__ __forceinline__ unsigned cs_scan256(unsigned v, unsigned *tot, unsigned *total) {
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = (unsigned)__shfl_up((int)inc, d, 64);
    if (lane >= (unsigned)d) inc += o;
  }
  if (lane == 63u) tot[w] = inc;
  __syncthreads();
  unsigned base = 0;
  for (unsigned i = 0; i < w; ++i) base += tot[i];
  *total = tot[0] + tot[1] + tot[2] + tot[3];
  return base + inc - v;
}

__global__ __launch_bounds__(256) void k_cs_find(cs_args A) {
  const bs_cap cap = A.caps[blockIdx.x];
  const unsigned t = threadIdx.x;
  float *spec = A.spec + (size_t)blockIdx.x * kCsN;
  cs_carrier *car = A.car + (size_t)blockIdx.x * A.max_carriers;
  if (cap.blocks == 0) {                                     // no whole block: all zeros
    for (unsigned i = 0; i < kCsPerThread; ++i) spec[t + 256u * i] = 0.f;
    if (t < A.max_carriers) car[t] = cs_carrier{};
    if (t == 0) A.sum[blockIdx.x] = cs_summary{};
    return;
  }
  __shared__ float P[kCsN], S[kCsN];
  __shared__ unsigned srt[kCsN];
  __shared__ unsigned tot[2][4];
  const float *rows = A.rows + (size_t)blockIdx.x * A.row_cap * kCsN;
  float p[kCsPerThread];                                     // bins t, t + 256, …: every bin in block order, a row's sixteen loads in flight together
#pragma unroll
  for (unsigned i = 0; i < kCsPerThread; ++i) p[i] = 0.f;
  for (unsigned b = 0; b < cap.blocks; ++b) {
    const float *row = rows + (size_t)b * kCsN + t;
#pragma unroll
    for (unsigned i = 0; i < kCsPerThread; ++i) p[i] += row[256u * i];
  }
#pragma unroll
  for (unsigned i = 0; i < kCsPerThread; ++i) {
    P[t + 256u * i] = p[i];
    spec[t + 256u * i] = p[i];
  }
  __syncthreads();
  for (unsigned i = 0; i < kCsPerThread; ++i) {
    const unsigned k = t + 256u * i;
    const float s = cs_smooth(P, k, A.smooth);
    S[k] = s;
    srt[k] = __float_as_uint(s);
  }
  __syncthreads();
  for (unsigned size = 2; size <= kCsN; size <<= 1)
    for (unsigned j = size >> 1; j > 0; j >>= 1) {
      for (unsigned i = 0; i < kCsN / 512u; ++i) {
        const unsigned p = t + 256u * i;                     // pair 0 … 2047
        const unsigned lo = ((p & ~(j - 1u)) << 1) | (p & (j - 1u)), hi = lo | j;
        const unsigned a = srt[lo], b = srt[hi];
        if ((a > b) == ((lo & size) == 0u)) { srt[lo] = b; srt[hi] = a; }
      }
      __syncthreads();
    }
  const float floor_ = __uint_as_float(srt[kCsFloorRank]);
  const float T = floor_ * A.factor;
  __syncthreads();                                           // (every thread has its floor: the sort buffer becomes the run lists)
  unsigned short *start = reinterpret_cast<unsigned short *>(srt), *end = start + kCsMaxRuns;
  cs_run *list = reinterpret_cast<cs_run *>(end + kCsMaxRuns);            // [kCsMaxCarriers], 8 KB into the 16
  unsigned runs, found = 0;
  const unsigned edges = cs_count_edges(S, T, t);
  const unsigned ebase = cs_scan256(edges, tot[0], &runs);
  runs &= 0xffffu;                                           // (as many ends as starts)
  cs_list_edges(S, T, t, ebase, start, end);
  __syncthreads();
  if (runs) {
    const unsigned kept = cs_count_kept(start, end, runs, A.min_bins, t);
    const unsigned kbase = cs_scan256(kept, tot[1], &found);
    cs_list_kept(start, end, runs, A.min_bins, t, kbase, A.max_carriers, list);
    __syncthreads();
  }
  const unsigned listed = found < A.max_carriers ? found : A.max_carriers;
  if (t < A.max_carriers) car[t] = t < listed ? cs_run_record(S, list[t].first, list[t].bins, floor_, T) : cs_carrier{};
  if (t == 0) {
    cs_summary R{};
    R.blocks = cap.blocks; R.stride = cs_stride(cap); R.found = found; R.listed = listed;
    R.saturated = !runs && S[0] >= T ? 1u : 0u;
    R.floor = floor_; R.threshold = T;
    A.sum[blockIdx.x] = R;
  }
}

}  // namespace

struct lsdr_carrier_scan {
  lsdr_ctx *ctx = nullptr;
  lsdr_carrier_scan_cfg cfg{};
  lsdr_in_desc in{};
  cs_args A{};
  bs_host<cs_summary> host;
  float *d_rows = nullptr, *d_spec = nullptr;
  cs_carrier *d_car = nullptr, *h_car = nullptr;
  bool spread = false;
};

extern "C" {

void lsdr_carrier_scan_destroy(lsdr_carrier_scan *e) {
  if (!e) return;
  e->host.destroy(e->ctx, {e->d_rows, e->d_spec, e->d_car});
  lsdr_in_free({}, {e->h_car});
  delete e;
}

static int cs_build(lsdr_carrier_scan *e, unsigned blocks) {
  const size_t B = (size_t)e->cfg.n_captures;
  cs_args &A = e->A;
  LSDR_TRY(e->host.create(e->ctx, B, blocks));
  LSDR_HIP(hipMalloc((void **)&e->d_rows, B * blocks * kCsN * sizeof(float)));
  LSDR_HIP(hipMalloc((void **)&e->d_spec, B * kCsN * sizeof(float)));
  LSDR_HIP(hipMemset(e->d_spec, 0, B * kCsN * sizeof(float)));
  LSDR_HIP(hipMalloc((void **)&e->d_car, B * A.max_carriers * sizeof(cs_carrier)));
  LSDR_HIP(hipHostMalloc((void **)&e->h_car, B * A.max_carriers * sizeof(cs_carrier), hipHostMallocDefault));
  memset(e->h_car, 0, B * A.max_carriers * sizeof(cs_carrier));
  A.caps = e->host.run.d_caps; A.tw = e->host.d_tw; A.rows = e->d_rows; A.spec = e->d_spec; A.sum = e->host.d_rec; A.car = e->d_car;
  A.row_cap = blocks;
  A.in_scale = e->in.in_scale; A.in_flip = e->in.in_flip;
  return LSDR_OK;
}

int lsdr_carrier_scan_create(lsdr_ctx *c, const lsdr_carrier_scan_cfg *cfg, lsdr_carrier_scan **out) {
  LSDR_ARG(c && cfg && out);
  LSDR_TRY(bs_check_captures("carrier_scan", cfg->n_captures));
  lsdr_in_desc in;
  LSDR_TRY(lsdr_in_describe("carrier_scan", cfg->in_format, cfg->in_scale, &in));
  if (cfg->blocks > kCsMaxBlocks) { lsdr_set_error("carrier_scan: blocks is %u, at most %u", cfg->blocks, kCsMaxBlocks); return LSDR_E_ARG; }
  const unsigned smooth = cfg->smooth ? cfg->smooth : 8u;
  if (smooth > kCsMaxSmooth) { lsdr_set_error("carrier_scan: smooth is %u, at most %u", cfg->smooth, kCsMaxSmooth); return LSDR_E_ARG; }
  const float db = cfg->threshold_db == 0.f ? 3.0f : cfg->threshold_db;
  if (!std::isfinite(db) || !(db > 0.f)) { lsdr_set_error("carrier_scan: threshold_db must be finite and above 0 (0: 3 dB)"); return LSDR_E_ARG; }
  const float factor = (float)pow(10.0, (double)db / 10.0);
  if (!std::isfinite(factor)) { lsdr_set_error("carrier_scan: threshold_db %g is beyond what a float holds", (double)db); return LSDR_E_ARG; }
  if (cfg->max_carriers > kCsMaxCarriers) { lsdr_set_error("carrier_scan: max_carriers is %u, at most %u", cfg->max_carriers, kCsMaxCarriers); return LSDR_E_ARG; }
  for (int i = 0; i < 3; ++i)
    if (cfg->reserved[i]) { lsdr_set_error("carrier_scan: lsdr_carrier_scan_cfg.reserved must be 0"); return LSDR_E_ARG; }
  lsdr_carrier_scan *e = new lsdr_carrier_scan();
  e->ctx = c; e->cfg = *cfg; e->in = in;
  e->spread = cfg->spread != 0;
  e->A.smooth = smooth; e->A.factor = factor;
  e->A.min_bins = cfg->min_bins ? cfg->min_bins : 2u * smooth + 1u;
  e->A.max_carriers = cfg->max_carriers ? cfg->max_carriers : 32u;
  const int rc = cs_build(e, cfg->blocks ? cfg->blocks : 64u);
  if (rc) { lsdr_carrier_scan_destroy(e); return rc; }
  *out = e;
  return LSDR_OK;
}

int lsdr_carrier_scan_run_async(lsdr_carrier_scan *e, const void *const *iq_dev, const size_t *n_samples) {
  LSDR_ARG(e && iq_dev && n_samples);
  lsdr_ctx *c = e->ctx;
  const unsigned B = (unsigned)e->cfg.n_captures;
  for (unsigned i = 0; i < B; ++i)                           // (a block's number is 32 bits in the kernels)
    if (n_samples[i] / kCsN > 0xffffffffull) { lsdr_set_error("carrier_scan: capture %u: n_samples %zu is beyond 2^32 blocks", i, n_samples[i]); return LSDR_E_ARG; }
  unsigned longest = 0;
  LSDR_TRY(e->host.begin(c, "carrier_scan", "lsdr_carrier_scan_wait", iq_dev, n_samples, e->in.item_bytes, &longest, e->spread));
  if (longest)
    in_dispatch(e->in.kind, [&](auto K) { hipLaunchKernelGGL(k_cs_block<K()>, dim3(longest, B), dim3(256), 0, c->stream, e->A); });
  hipLaunchKernelGGL(k_cs_find, dim3(B), dim3(256), 0, c->stream, e->A);
  LSDR_HIP(hipMemcpyAsync(e->h_car, e->d_car, (size_t)B * e->A.max_carriers * sizeof(cs_carrier), hipMemcpyDeviceToHost, c->stream));
  return e->host.end(c);
}

int lsdr_carrier_scan_wait(lsdr_carrier_scan *e, lsdr_scan_summary *summaries, lsdr_scan_carrier *carriers) {
  LSDR_ARG(e && summaries && carriers);
  LSDR_TRY(e->host.wait("carrier_scan", summaries));
  memcpy(carriers, e->h_car, (size_t)e->cfg.n_captures * e->A.max_carriers * sizeof(cs_carrier));
  return LSDR_OK;
}

const float *lsdr_carrier_scan_spectrum_dev(lsdr_carrier_scan *e, int i) {
  if (!e || i < 0 || i >= e->cfg.n_captures) return nullptr;
  return e->d_spec + (size_t)i * kCsN;
}

}  // extern "C"
