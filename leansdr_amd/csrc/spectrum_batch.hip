// leansdr_amd/csrc/spectrum_batch.hip — lsdr_spectrum_batch: cnr_fft<f32> (sdr.h:1273-1345) and spectrum<f32> (sdr.h:1347-1404) for many
// captures in shared launches, each capture in its own sample format, with its own length and band centre.  No decode kernel is involved.
//
// Per slab of slab_rows rows (rows = fetched blocks), all captures at once (blockIdx.y = capture):
//   k_sb_power<K>   one workgroup of 256 per 4096 points (one row of nfft 4096, four of 1024, … 64 of 64): 16-byte loads of the raw items,
//                   converted, into LDS in bit-reversed order; cfft_engine<float>::inplace(data, true) as passes of up to four radix-2
//                   stages kept in registers (16 points per thread) between LDS exchanges; 1/n, re² + im²; one row of scratch each
//   k_sb_average    one thread per bin and capture walks the slab's rows in order: avgpower = avgpower·(1 − kavg) + power·kavg, the first
//                   row of a capture initialising avgpower with its power FIRST (sdr.h:1313-1320); avgpower carried in device memory from
//                   slab to slab; the averaged row goes to the kept rows when rows are emitted, else (CNR) it replaces the power in the scratch
//   k_sb_bands      (CNR) one thread per row and band: the serial sum of avgslots (sdr.h:1334-1338) over the averaged row, all rows of
//                   the slab side by side (a sum needs its own row only)
// The host finishes with libm: the CNR's quotients and logf from the three sums (wait), 10·log10f of the kept rows (the rows accessor).
// The scratch is [captures][slab_rows][nfft] floats whatever the captures' lengths.
//
// Determinism: no atomics; a butterfly, a power, an average and a band sum are each evaluated once, by an expression and in an order that
// depend on the sample's index alone — the same bits alone, in any batch, with any slab_rows and any number of stages per pass.
// Every kernel leaves by the capture's own row count: nothing behind a capture's last fetched block is read.
#include <cmath>
#include "capture_input.h"
#include "spectrum_batch_device.h"

namespace {
#include "notch_detect.h"             // notch_detect_twiddles: cfft_engine's table, built on the host with cosf/sinf

struct sb_cap { const unsigned char *in; unsigned rows; int icf; };
struct sb_args {
  const sb_cap *caps;
  const float2 *om;                    // [nfft] cfft_engine's reverse twiddles
  float *scratch;                      // [captures][slab_rows][nfft] power, then averaged power, of the slab's rows
  float *avg;                          // [captures][nfft] avgpower behind the last row done
  float *rows;                         // [captures][max_rows][nfft] averaged power of every row (emit_rows), else null
  float *sums;                         // [captures][max_rows][3] band sums (CNR), else null
  unsigned long long max_rows;
  unsigned slab_rows, slab_base;       // this launch: rows slab_base … slab_base + slab_rows − 1 (0-based) of every capture
  unsigned logn, decimation, stages;
  int bwslots;
  float in_scale, kavg, invn;
  unsigned in_flip;
};

template <int K>
__global__ __launch_bounds__(kSbThreads) void k_sb_power(sb_args A) {
  const sb_cap cap = A.caps[blockIdx.y];
  const unsigned logn = A.logn, nfft = 1u << logn, per = kSbPoints >> logn;     // rows per workgroup
  const unsigned local0 = blockIdx.x * per;                                      // first row of this workgroup within the slab
  if (local0 >= A.slab_rows || (unsigned long long)A.slab_base + local0 >= cap.rows) return;
  unsigned valid = A.slab_rows - local0;                                         // rows of this workgroup that exist: 1 … per
  if ((unsigned long long)valid > (unsigned long long)cap.rows - A.slab_base - local0) valid = (unsigned)(cap.rows - A.slab_base - local0);
  if (valid > per) valid = per;
  extern __shared__ __attribute__((aligned(16))) char sb_smem[];
  float2 *d = reinterpret_cast<float2 *>(sb_smem), *w = d + kSbDataLds;
  constexpr unsigned kB = in_item<K>::kBytes, kPer = 16u / kB;
  const unsigned t = threadIdx.x;
  const bool vec = ((size_t)cap.in & 15u) == 0;              // (a block is a multiple of 16 bytes: the capture's own alignment decides)
  for (unsigned c = t; c < kSbPoints / kPer; c += kSbThreads) {
    const unsigned idx = c * kPer, u = idx >> logn, within = idx & (nfft - 1u);
    if (u >= valid) {
#pragma unroll
      for (unsigned q = 0; q < kPer; ++q) d[sb_dp(idx + q)] = make_float2(0.f, 0.f);
      continue;
    }
    const unsigned long long blk = sb_block_of_row((unsigned long long)A.slab_base + local0 + u + 1ull, logn, A.decimation);
    const unsigned char *src = cap.in + ((size_t)blk << logn) * kB;
    float2 z[kPer];
    in_piece<K>(src, within, vec, A.in_scale, A.in_flip, z);
#pragma unroll
    for (unsigned q = 0; q < kPer; ++q)                      // the bit-reversal permutation (dsp.h:84-92): position P holds in[brev(P)]
      d[sb_dp((u << logn) | (__brev(within + q) >> (32u - logn)))] = z[q];
  }
  for (unsigned i = t; i < nfft / 2u; i += kSbThreads) w[sb_tp(i)] = A.om[i];
  __syncthreads();
  for (unsigned st = 0; st < logn;) {
    unsigned S = logn - st;
    if (S > A.stages) S = A.stages;
    switch (S) {
      case 4: sb_pass<4>(d, w, st, logn, t); break;
      case 3: sb_pass<3>(d, w, st, logn, t); break;
      case 2: sb_pass<2>(d, w, st, logn, t); break;
      default: sb_pass<1>(d, w, st, logn, t); break;
    }
    st += S;
    __syncthreads();
  }
  float *out = A.scratch + (((size_t)blockIdx.y * A.slab_rows + local0) << logn);
  const float invn = A.invn;
  for (unsigned i = t; i < (valid << logn); i += kSbThreads) {
    float2 v = d[sb_dp(i)];
    v.x *= invn; v.y *= invn;                                // the reverse direction's 1/n (dsp.h:106-109)
    out[i] = v.x * v.x + v.y * v.y;
  }
}

__global__ __launch_bounds__(256) void k_sb_average(sb_args A) {
  const sb_cap cap = A.caps[blockIdx.y];
  const unsigned nfft = 1u << A.logn, bin = blockIdx.x * 256u + threadIdx.x;
  if (bin >= nfft || A.slab_base >= cap.rows) return;
  unsigned n = A.slab_rows;
  if (n > cap.rows - A.slab_base) n = cap.rows - A.slab_base;
  float *p = A.scratch + (((size_t)blockIdx.y * A.slab_rows) << A.logn) + bin;
  float *keep = A.rows ? A.rows + (((size_t)blockIdx.y * A.max_rows + A.slab_base) << A.logn) + bin : nullptr;
  float *carry = A.avg + ((size_t)blockIdx.y << A.logn) + bin;
  const float k = A.kavg, omk = 1 - k;
  const bool in_place = A.sums && !keep;                     // k_sb_bands reads the kept rows where there are any, else the scratch
  float a = A.slab_base ? *carry : 0.f;
  // sixteen rows' loads in flight per thread, then the recurrence over them in order: a wave per 64 bins is all the parallelism the
  // recurrence leaves, and one load at a time would pay the memory's latency per row
  constexpr unsigned kU = 16;
  for (unsigned r0 = 0; r0 < n; r0 += kU) {
    float pw[kU];
#pragma unroll
    for (unsigned u = 0; u < kU; ++u) pw[u] = r0 + u < n ? p[(size_t)(r0 + u) << A.logn] : 0.f;
#pragma unroll
    for (unsigned u = 0; u < kU; ++u) {
      if (r0 + u >= n) break;
      if (A.slab_base + r0 + u == 0) a = pw[u];              // `if (!avgpower) … memcpy(avgpower, power)`, and THEN the update like every row
      a = a * omk + pw[u] * k;
      if (in_place) p[(size_t)(r0 + u) << A.logn] = a;
      if (keep) keep[(size_t)(r0 + u) << A.logn] = a;
    }
  }
  *carry = a;
}

__global__ __launch_bounds__(64) void k_sb_bands(sb_args A) {
  const sb_cap cap = A.caps[blockIdx.y];
  const unsigned q = blockIdx.x * 64u + threadIdx.x, r = q / 3u, band = q - 3u * r;
  if (r >= A.slab_rows || (unsigned long long)A.slab_base + r >= cap.rows) return;
  int i0, i1;
  sb_band((int)band, cap.icf, A.bwslots, &i0, &i1);
  const float *row = A.rows ? A.rows + (((size_t)blockIdx.y * A.max_rows + A.slab_base + r) << A.logn)
                            : A.scratch + (((size_t)blockIdx.y * A.slab_rows + r) << A.logn);
  A.sums[((size_t)blockIdx.y * A.max_rows + A.slab_base + r) * 3u + band] = sb_band_sum(row, i0, i1, 1u << A.logn);
}

}  // namespace

struct lsdr_spectrum_batch {
  lsdr_ctx *ctx = nullptr;
  lsdr_spectrum_batch_cfg cfg{};
  lsdr_in_desc in{};
  unsigned logn = 0;
  size_t max_rows = 0, rows_alloc = 0;            // rows_alloc: max_rows, at least 1 (the strides of rows / sums)
  float kavg = 0.f;
  sb_args A{};
  in_run<sb_cap> run;
  lsdr_spectrum_result *h_res = nullptr;          // pinned
  float *h_sums = nullptr, *d_sums = nullptr;     // pinned / device
  float2 *d_om = nullptr;
  float *d_scratch = nullptr, *d_avg = nullptr, *d_rows = nullptr;
  bool have = false;                              // a finished run's results are there for the accessors
};

extern "C" {

void lsdr_spectrum_batch_destroy(lsdr_spectrum_batch *b) {
  if (!b) return;
  (void)hipStreamSynchronize(b->ctx->stream);
  b->run.destroy();
  lsdr_in_free({b->d_sums, b->d_om, b->d_scratch, b->d_avg, b->d_rows}, {b->h_res, b->h_sums});
  delete b;
}

static int sb_build(lsdr_spectrum_batch *b) {
  lsdr_ctx *c = b->ctx;
  const size_t B = (size_t)b->cfg.n_captures, nfft = (size_t)b->cfg.nfft;
  LSDR_HIP(hipSetDevice(c->device));
  LSDR_TRY(b->run.create(B));
  LSDR_HIP(hipHostMalloc((void **)&b->h_res, B * sizeof(lsdr_spectrum_result), hipHostMallocDefault));
  memset(b->h_res, 0, B * sizeof(lsdr_spectrum_result));
  LSDR_HIP(hipMalloc((void **)&b->d_om, nfft * sizeof(float2)));
  LSDR_HIP(hipMalloc((void **)&b->d_scratch, B * b->cfg.slab_rows * nfft * sizeof(float)));
  LSDR_HIP(hipMalloc((void **)&b->d_avg, B * nfft * sizeof(float)));
  if (b->cfg.emit_rows) LSDR_HIP(hipMalloc((void **)&b->d_rows, B * b->rows_alloc * nfft * sizeof(float)));
  if (b->cfg.bandwidth > 0) {
    LSDR_HIP(hipMalloc((void **)&b->d_sums, B * b->rows_alloc * 3 * sizeof(float)));
    LSDR_HIP(hipHostMalloc((void **)&b->h_sums, B * b->rows_alloc * 3 * sizeof(float), hipHostMallocDefault));
  }
  std::vector<float2> om;
  notch_detect_twiddles((int)nfft, true, om);
  LSDR_HIP(hipMemcpy(b->d_om, om.data(), nfft * sizeof(float2), hipMemcpyHostToDevice));
  sb_args &A = b->A;
  A.caps = b->run.d_caps; A.om = b->d_om; A.scratch = b->d_scratch; A.avg = b->d_avg; A.rows = b->d_rows; A.sums = b->d_sums;
  A.max_rows = b->rows_alloc; A.slab_rows = b->cfg.slab_rows; A.slab_base = 0;
  A.logn = b->logn; A.decimation = b->cfg.decimation; A.stages = b->cfg.stages_per_pass;
  A.bwslots = (int)((b->cfg.bandwidth / 4) * b->cfg.nfft);
  A.in_scale = b->in.in_scale; A.in_flip = b->in.in_flip;
  A.kavg = b->kavg; A.invn = (float)(1.0 / (double)nfft);
  return LSDR_OK;
}

int lsdr_spectrum_batch_create(lsdr_ctx *c, const lsdr_spectrum_batch_cfg *cfg, lsdr_spectrum_batch **out) {
  LSDR_ARG(c && cfg && out);
  if (cfg->n_captures < 1 || cfg->n_captures > 65535) { lsdr_set_error("spectrum_batch: n_captures must be 1 … 65535 (got %d)", cfg->n_captures); return LSDR_E_ARG; }
  lsdr_in_desc in;
  LSDR_TRY(lsdr_in_describe("spectrum_batch", cfg->in_format, cfg->in_scale, &in));
  if (cfg->nfft < 64 || cfg->nfft > 4096 || (cfg->nfft & (cfg->nfft - 1))) {
    lsdr_set_error("spectrum_batch: nfft must be a power of two, 64 … 4096 (got %d)", cfg->nfft); return LSDR_E_ARG;
  }
  if (cfg->decimation < (unsigned)cfg->nfft) {
    lsdr_set_error("spectrum_batch: decimation %u is below nfft %d (at most one row per block)", cfg->decimation, cfg->nfft); return LSDR_E_ARG;
  }
  if (!std::isfinite(cfg->kavg) || !std::isfinite(cfg->bandwidth) || cfg->bandwidth < 0.f) {
    lsdr_set_error("spectrum_batch: kavg and bandwidth must be finite, bandwidth not negative"); return LSDR_E_ARG;
  }
  if (cfg->bandwidth > 0.25) { lsdr_set_error("CNR estimator requires Fsampling > 4x Fsignal"); return LSDR_E_ARG; }   // sdr.h:1282-1283
  if (cfg->bandwidth > 0 && (int)((cfg->bandwidth / 4) * cfg->nfft) == 0) {
    lsdr_set_error("spectrum_batch: bandwidth %g gives no slot at nfft %d ((int)(bandwidth/4·nfft) is 0: cnr_fft would emit nothing)", (double)cfg->bandwidth, cfg->nfft);
    return LSDR_E_ARG;
  }
  if (cfg->stages_per_pass > kSbMaxStages) { lsdr_set_error("spectrum_batch: stages_per_pass is %u, at most %u", cfg->stages_per_pass, kSbMaxStages); return LSDR_E_ARG; }
  for (int i = 0; i < 5; ++i)
    if (cfg->reserved[i]) { lsdr_set_error("spectrum_batch: lsdr_spectrum_batch_cfg.reserved must be 0"); return LSDR_E_ARG; }
  lsdr_spectrum_batch *b = new lsdr_spectrum_batch();
  b->ctx = c; b->cfg = *cfg; b->in = in;
  for (int t = cfg->nfft; t > 1; t >>= 1) ++b->logn;
  b->kavg = cfg->kavg == 0.f ? (float)0.1 : cfg->kavg;
  if (!b->cfg.stages_per_pass) b->cfg.stages_per_pass = kSbMaxStages;
  b->max_rows = (size_t)sb_rows(cfg->max_samples >> b->logn, b->logn, cfg->decimation);
  if (b->max_rows > 0x7fffffffu) {
    lsdr_set_error("spectrum_batch: max_samples %zu gives %zu rows, at most 2^31 − 1", cfg->max_samples, b->max_rows);
    delete b;
    return LSDR_E_UNSUPPORTED;
  }
  b->rows_alloc = b->max_rows ? b->max_rows : 1;
  // the slab: 16 Mi floats of scratch over all captures unless the caller says otherwise, never more rows than a capture can have
  size_t slab = cfg->slab_rows ? cfg->slab_rows : ((size_t)1 << 24) / ((size_t)cfg->n_captures * (size_t)cfg->nfft);
  if (slab > b->rows_alloc) slab = b->rows_alloc;
  if (slab < 1) slab = 1;
  if (slab > 0x7fffffffu) slab = 0x7fffffffu;
  b->cfg.slab_rows = (unsigned)slab;
  const int rc = sb_build(b);
  if (rc) { lsdr_spectrum_batch_destroy(b); return rc; }
  *out = b;
  return LSDR_OK;
}

size_t lsdr_spectrum_batch_max_rows(const lsdr_spectrum_batch *b) { return b ? b->max_rows : 0; }
unsigned lsdr_spectrum_batch_slab_rows(const lsdr_spectrum_batch *b) { return b ? b->cfg.slab_rows : 0; }

int lsdr_spectrum_batch_run_async(lsdr_spectrum_batch *b, const void *const *iq_dev, const lsdr_capture_each *each) {
  LSDR_ARG(b && iq_dev && each);
  const unsigned B = (unsigned)b->cfg.n_captures;
  LSDR_TRY(lsdr_in_check_each("spectrum_batch", "the centre", B, iq_dev, each, nullptr, nullptr, b->cfg.max_samples, b->in.item_bytes));
  LSDR_TRY(b->run.idle("spectrum_batch", "lsdr_spectrum_batch_wait"));
  lsdr_ctx *c = b->ctx;
  LSDR_HIP(hipSetDevice(c->device));
  b->have = false;
  const int N = b->cfg.nfft;
  size_t longest = 0;                                        // the grids are sized for it; a shorter capture's workgroups leave at once
  for (unsigned i = 0; i < B; ++i) {
    const size_t blocks = each[i].n_samples >> b->logn;
    const size_t rows = (size_t)sb_rows(blocks, b->logn, b->cfg.decimation);
    const float center_freq = each[i].tune * 1.0f;           // *freq_tap * tap_multiplier
    const int icf = (int)floor((double)(center_freq * N) + 0.5);
    sb_cap &cap = b->run.h_caps[i];
    cap.in = reinterpret_cast<const unsigned char *>(iq_dev[i]);
    cap.rows = (unsigned)rows; cap.icf = icf;
    lsdr_spectrum_result &r = b->h_res[i];
    memset(&r, 0, sizeof r);
    r.consumed = (uint64_t)blocks << b->logn; r.rows = rows; r.icf = b->cfg.bandwidth > 0 ? icf : 0;
    if (rows > longest) longest = rows;
  }
  LSDR_TRY(b->run.upload(c->stream));
  const unsigned slab = b->cfg.slab_rows, per = kSbPoints >> b->logn;
  const size_t lds = ((size_t)kSbDataLds + sb_tw_lds((unsigned)N)) * sizeof(float2);
  for (size_t base = 0; base < longest; base += slab) {      // (over slabs, never over rows)
    sb_args A = b->A;
    A.slab_base = (unsigned)base;
    const unsigned here = longest - base < slab ? (unsigned)(longest - base) : slab;    // the longest capture's rows in this slab
    const dim3 grid((here + per - 1u) / per, B), wg(kSbThreads);
    in_dispatch(b->in.kind, [&](auto K) { hipLaunchKernelGGL(k_sb_power<K()>, grid, wg, lds, c->stream, A); });
    hipLaunchKernelGGL(k_sb_average, dim3(((unsigned)N + 255u) / 256u, B), dim3(256), 0, c->stream, A);
    if (b->d_sums) hipLaunchKernelGGL(k_sb_bands, dim3((here * 3u + 63u) / 64u, B), dim3(64), 0, c->stream, A);
  }
  LSDR_HIP(hipGetLastError());
  if (b->d_sums)
    for (unsigned i = 0; i < B; ++i)
      if (b->run.h_caps[i].rows)
        LSDR_HIP(hipMemcpyAsync(b->h_sums + (size_t)i * b->rows_alloc * 3, b->d_sums + (size_t)i * b->rows_alloc * 3,
                                (size_t)b->run.h_caps[i].rows * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  return b->run.mark(c->stream);
}

int lsdr_spectrum_batch_wait(lsdr_spectrum_batch *b, lsdr_spectrum_result *results) {
  LSDR_ARG(b);
  LSDR_TRY(b->run.wait("spectrum_batch"));
  b->have = true;
  if (results) memcpy(results, b->h_res, (size_t)b->cfg.n_captures * sizeof(lsdr_spectrum_result));
  return LSDR_OK;
}

static int sb_accessor(const lsdr_spectrum_batch *b, int i) {
  LSDR_ARG(b);
  if (i < 0 || i >= b->cfg.n_captures) { lsdr_set_error("spectrum_batch: capture %d of %d", i, b->cfg.n_captures); return LSDR_E_ARG; }
  if (b->run.in_flight || !b->have) { lsdr_set_error("spectrum_batch: no finished run (lsdr_spectrum_batch_wait first)"); return LSDR_E_ARG; }
  return LSDR_OK;
}

int lsdr_spectrum_batch_cnr(lsdr_spectrum_batch *b, int i, float *cnr_out, size_t cap, size_t *n) {
  LSDR_TRY(sb_accessor(b, i));
  LSDR_ARG(n);
  *n = 0;
  if (!b->d_sums) { lsdr_set_error("spectrum_batch: created with bandwidth 0: no CNR"); return LSDR_E_ARG; }
  const size_t rows = b->h_res[i].rows;
  if (rows > cap || (rows && !cnr_out)) { lsdr_set_error("spectrum_batch: capture %d has %zu CNR values, room for %zu", i, rows, cap); return LSDR_E_ARG; }
  const int bwslots = b->A.bwslots;
  const float *s = b->h_sums + (size_t)i * b->rows_alloc * 3;
  for (size_t r = 0; r < rows; ++r, s += 3) {                // sdr.h:1321-1332 from the three sums: `s / (i1 - i0 + 1)`, then the host's logf
    const float c2plusn2 = s[0] / (2 * bwslots + 1);
    const float n2 = (s[1] / (bwslots + 1) + s[2] / (bwslots + 1)) / 2;
    const float c2 = c2plusn2 - n2;
    cnr_out[r] = (c2 > 0 && n2 > 0) ? 10 * logf(c2 / n2) / logf(10) : -50;
  }
  *n = rows;
  return LSDR_OK;
}

const float *lsdr_spectrum_batch_rows_dev(const lsdr_spectrum_batch *b, int i) {
  if (!b || i < 0 || i >= b->cfg.n_captures || !b->d_rows) return nullptr;
  return b->d_rows + (((size_t)i * b->rows_alloc) << b->logn);
}

int lsdr_spectrum_batch_rows_db(lsdr_spectrum_batch *b, int i, float *rows_out, size_t cap_rows, size_t *n) {
  LSDR_TRY(sb_accessor(b, i));
  LSDR_ARG(n);
  *n = 0;
  if (!b->d_rows) { lsdr_set_error("spectrum_batch: created without emit_rows: no rows"); return LSDR_E_ARG; }
  const size_t rows = b->h_res[i].rows, N = (size_t)b->cfg.nfft;
  if (rows > cap_rows || (rows && !rows_out)) { lsdr_set_error("spectrum_batch: capture %d has %zu rows, room for %zu", i, rows, cap_rows); return LSDR_E_ARG; }
  if (!rows) return LSDR_OK;
  LSDR_HIP(hipSetDevice(b->ctx->device));
  LSDR_HIP(hipMemcpy(rows_out, lsdr_spectrum_batch_rows_dev(b, i), rows * N * sizeof(float), hipMemcpyDeviceToHost));
  for (size_t r = 0; r < rows; ++r) {                        // do_spectrum's output order (sdr.h:1391-1394), log10f on the host
    float *row = rows_out + r * N;
    for (size_t k = 0; k < N / 2; ++k) {
      const float lo = row[k], hi = row[N / 2 + k];
      row[k] = 10 * log10f(hi);
      row[N / 2 + k] = 10 * log10f(lo);
    }
  }
  *n = rows;
  return LSDR_OK;
}

}  // extern "C"
