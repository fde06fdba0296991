// leansdr_amd/csrc/resample_batch.hip — lsdr_resample_batch: leandvb's --derotate --resample in front of the batch decoders, for B captures
// in one launch.  Every capture, in any of the five sample formats, with its own length and its own carrier offset, is converted, derotated
// (rotator<f32>, sdr.h:1226-1259), low-passed by real taps and decimated (fir_filter<cf32,float>, dsp.h:246-262) into a cf32 stream that
// lsdr_capture_batch decodes as LSDR_IN_CF32.  include/lsdr_hip.h states the arithmetic; the kernel below is that arithmetic, one rounding
// per operation (-ffp-contract=off).
//
//   k_resample<K, R>  blockIdx.y = capture, blockIdx.x = tile of M outputs (M ≤ 256·R), one workgroup of 256.  The tile's (mv − 1)·D + N + 1
//                     input samples are loaded (16 bytes at a time where the capture's pointer is 16-byte aligned and the 16 bytes end inside
//                     the capture, item by item otherwise: the same values), converted, rotated ONCE by the table's phasor and written to LDS
//                     in polyphase layout: tile-local sample t sits at row t mod D, column t / D, rows S float2 apart (S odd).  The tap phase
//                     then reads, for tap i ↔ u = N − i = col·D + row, one float2 per output at row·S + col + (output's index): consecutive
//                     lanes read consecutive addresses.  Taps are visited i ascending; coefficient and place (row·S + col, a table built at
//                     create) are wave-uniform and come by scalar loads, eight taps at a time.
//
// A workgroup leaves by its own capture's `produced` before it forms any address; nothing behind item n − 1 of a capture is read (the last
// sample a tile needs is N + (produced − 1)·D ≤ n − 1, and a 16-byte load is used only where it ends inside the capture) and nothing behind
// out[produced − 1] is written.  All indexing of a capture is 64-bit; tile-local indices are below 2^17.  No atomics, no order that depends
// on scheduling: a capture's output is a pure function of its samples, its tune and the taps.
#include <cmath>
#include "capture_input.h"     // the formats' conversion: in_load / in_unpack = float(item − Z)·in_scale, as the capture batch's loads

namespace {

constexpr unsigned kRsThreads = 256;
constexpr unsigned kRsMaxDecim = 64, kRsMaxCoeffs = 1024;
constexpr size_t kRsLdsMax = 65536;            // per workgroup: two of them fit a CU's 160 KB at the largest tile
constexpr size_t kRsLdsWant = 32768;           // … and the largest tile at or under this is preferred (four and more per CU)

struct rs_cap {
  const unsigned char *in;
  float2 *out;
  unsigned long long produced;
  int ifreq;
  unsigned wide;                               // the capture's pointer is 16-byte aligned
};
static_assert(sizeof(rs_cap) == 32, "rs_cap is uploaded as an array");

struct rs_args {
  const rs_cap *caps;
  const float2 *tab;                           // [65536] (cos, sin)(2πj/65536)
  const float *taps;                           // [N]
  const unsigned *offs;                        // [N] tap i's place in the LDS tile: (u mod D)·S + u / D, u = N − i
  unsigned N, D, M, S;
  unsigned magic;                              // ceil(2^32 / D): t / D = umulhi(t, magic) for t < 2^32 / D (D = 1: handled apart)
  float in_scale;
  unsigned in_flip;
};

// sample j of the capture (tile-local t = j − j0), converted: rotate by the phase of index (−j·ifreq) mod 65536 and store at (t mod D, t / D)
__device__ __forceinline__ void rs_put(const rs_args &A, float2 *lds, unsigned long long j, unsigned t, int ifreq, float2 x) {
  const unsigned idx = (0u - (unsigned)j * (unsigned)ifreq) & 0xffffu;        // mod 2^16 commutes with the wrap of 32-bit arithmetic
  const float2 cs = A.tab[idx];
  const float2 y = make_float2(x.x * cs.x - x.y * cs.y, x.x * cs.y + x.y * cs.x);
  const unsigned q = A.D == 1u ? t : __umulhi(t, A.magic);
  lds[(t - q * A.D) * A.S + q] = y;
}

template <int K, int R>
__global__ __launch_bounds__(kRsThreads) void k_resample(rs_args A) {
  extern __shared__ __attribute__((aligned(16))) char rs_smem[];
  float2 *lds = reinterpret_cast<float2 *>(rs_smem);
  const rs_cap cap = A.caps[blockIdx.y];
  const unsigned long long m0 = (unsigned long long)blockIdx.x * A.M;
  if (m0 >= cap.produced) return;              // by the capture's own count, before any address of it is formed
  const unsigned long long rem = cap.produced - m0;
  const unsigned mv = rem < A.M ? (unsigned)rem : A.M;
  const unsigned N = A.N, D = A.D, l = threadIdx.x;
  constexpr unsigned kB = in_item<K>::kBytes, kPer = 16u / kB;
  const float sc = A.in_scale; const unsigned flip = A.in_flip;

  // ---- stage: tile-local t ∈ [0, T) ↔ sample j = j0 + t; the last one is N + (m0 + mv − 1)·D ≤ n − 1
  const unsigned T = (mv - 1u) * D + N + 1u;
  const unsigned long long j0 = m0 * D, jend = j0 + T;
  constexpr int NB = 4;
  if (cap.wide) {
    // 16-byte pieces c of the capture: items c·kPer … c·kPer + kPer − 1.  Every piece that holds a staged sample ends at or before
    // item jend − 1 … except the last, which is taken item by item when it reaches further (it may reach behind the capture's end).
    const unsigned long long c_first = j0 / kPer, c_last = (jend - 1u) / kPer;
    for (unsigned long long cb = c_first; cb <= c_last; cb += (unsigned long long)NB * kRsThreads) {
      uint4 w[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const unsigned long long c = cb + l + (unsigned)k * kRsThreads;
        if (c <= c_last && (c + 1u) * kPer <= jend) w[k] = *reinterpret_cast<const uint4 *>(cap.in + (size_t)c * 16u);
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const unsigned long long c = cb + l + (unsigned)k * kRsThreads;
        if (c > c_last) continue;
        if ((c + 1u) * kPer <= jend) {
          const unsigned ws[4] = {w[k].x, w[k].y, w[k].z, w[k].w};
#pragma unroll
          for (unsigned q = 0; q < kPer; ++q) {
            const unsigned long long j = c * kPer + q;
            if (j >= j0) rs_put(A, lds, j, (unsigned)(j - j0), cap.ifreq, in_unpack<K>(ws, q, sc, flip));
          }
        } else {
          for (unsigned q = 0; q < kPer; ++q) {
            const unsigned long long j = c * kPer + q;
            if (j >= j0 && j < jend) rs_put(A, lds, j, (unsigned)(j - j0), cap.ifreq, in_load<K>(cap.in, (size_t)j, sc, flip));
          }
        }
      }
    }
  } else {
    for (unsigned tb = 0; tb < T; tb += NB * kRsThreads) {
      float2 v[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const unsigned t = tb + l + (unsigned)k * kRsThreads;
        if (t < T) v[k] = in_load<K>(cap.in, (size_t)(j0 + t), sc, flip);
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const unsigned t = tb + l + (unsigned)k * kRsThreads;
        if (t < T) rs_put(A, lds, j0 + t, t, cap.ifreq, v[k]);
      }
    }
  }
  __syncthreads();

  // ---- taps: out[m0 + lm] = Σ_i h[i]·y[N + lm·D − i], i ascending; tile-local sample N + lm·D − i = (u / D + lm)·D + u mod D, u = N − i
  if (l >= A.M) return;                        // (tiles of fewer than 256 outputs: the other threads only staged)
  float accr[R], acci[R];
#pragma unroll
  for (int r = 0; r < R; ++r) { accr[r] = 0.f; acci[r] = 0.f; }
  // Eight taps at a time: their coefficients and their places in LDS (offs[i] = (u mod D)·S + u / D for u = N − i, built at create) are two
  // wide scalar loads, and their LDS reads do not depend on the sums, so they are in flight together; the sums themselves stay one chain
  // per output, i ascending.
  const float2 *base = lds + l;
  auto tap = [&](float h, unsigned off) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float2 x = base[off + (unsigned)r * kRsThreads];
      accr[r] = accr[r] + h * x.x;
      acci[r] = acci[r] + h * x.y;
    }
  };
  unsigned i = 0;
  for (; i + 8u <= N; i += 8u) {
    float h[8];
    unsigned o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { h[k] = A.taps[i + k]; o[k] = A.offs[i + k]; }
#pragma unroll
    for (int k = 0; k < 8; ++k) tap(h[k], o[k]);
  }
  for (; i < N; ++i) tap(A.taps[i], A.offs[i]);
  float2 *out = cap.out + m0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const unsigned lm = l + (unsigned)r * kRsThreads;
    if (lm < mv) out[lm] = make_float2(accr[r], acci[r]);
  }
}

// LDS row stride for a tile of M outputs: its N / D + 1 columns of halo behind M, made odd (consecutive rows land on different banks)
unsigned rs_stride(unsigned M, unsigned N, unsigned D) { return (M + N / D + 1u) | 1u; }
size_t rs_lds_bytes(unsigned M, unsigned N, unsigned D) { return (size_t)D * rs_stride(M, N, D) * sizeof(float2); }

// The tile: the largest of 1024, 512, 256 outputs whose LDS stays at or under kRsLdsWant; else the largest of 256, 128, 64, 32 that fits
// kRsLdsMax (two workgroups per CU).  D = 64, N = 1024 takes 64 outputs; D = 30, N = 313 takes 256 (64080 bytes).
unsigned rs_tile(unsigned N, unsigned D) {
  for (unsigned M = 1024; M >= 256; M >>= 1)
    if (rs_lds_bytes(M, N, D) <= kRsLdsWant) return M;
  for (unsigned M = 256; M >= 32; M >>= 1)
    if (rs_lds_bytes(M, N, D) <= kRsLdsMax) return M;
  return 0;
}

template <int K>
void rs_launch(unsigned M, dim3 grid, size_t lds, hipStream_t s, const rs_args &A) {
  const dim3 wg(kRsThreads);
  if (M > 512) hipLaunchKernelGGL((k_resample<K, 4>), grid, wg, lds, s, A);
  else if (M > 256) hipLaunchKernelGGL((k_resample<K, 2>), grid, wg, lds, s, A);
  else hipLaunchKernelGGL((k_resample<K, 1>), grid, wg, lds, s, A);
}

}  // namespace

struct lsdr_resample_batch {
  lsdr_ctx *ctx = nullptr;
  lsdr_resample_batch_cfg cfg{};
  lsdr_in_desc in{};
  unsigned M = 0;
  size_t lds = 0;
  rs_args A{};
  in_run<rs_cap> run;
  float2 *d_tab = nullptr;
  float *d_taps = nullptr;
  unsigned *d_offs = nullptr;
  std::vector<lsdr_resample_result> results;           // known at run_async: pure functions of the sizes
};

extern "C" {

int lsdr_resample_design(float omega, float rolloff, float rej, unsigned decim, unsigned *decim_out, float *coeffs_host, unsigned cap,
                         unsigned *ncoeffs) {
  LSDR_ARG(decim_out && ncoeffs);
  if (!std::isfinite(omega) || omega < 1.f) { lsdr_set_error("resample_design: omega must be finite and at least 1 (got %g)", (double)omega); return LSDR_E_ARG; }
  if (!std::isfinite(rolloff) || rolloff <= 0.f) { lsdr_set_error("resample_design: rolloff must be finite and positive"); return LSDR_E_ARG; }
  if (!std::isfinite(rej) || rej <= 0.f) { lsdr_set_error("resample_design: rej must be finite and positive"); return LSDR_E_ARG; }
  // leandvb.cc:353-378 with Fm = 1, Fs = omega, in the reference's floats
  int d = (int)decim;
  if (!d) {
    const float target_Fs = 4.f;
    d = (int)(omega / target_Fs);
    if (d < 1) d = 1;
  }
  const float transition = 0.5f * rolloff;
  const float forder = rej * omega / (22 * transition);
  if (!(forder < 1e6f)) { lsdr_set_error("resample_design: the order %g is out of range", (double)forder); return LSDR_E_ARG; }
  int order = (int)forder;
  order = ((order + 1) / 2) * 2;
  const float Fcut = 0.5f * (1 + rolloff / 2) / omega;
  *decim_out = (unsigned)d;
  *ncoeffs = (unsigned)order + 1u;
  if (!coeffs_host || cap < *ncoeffs) {
    lsdr_set_error("resample_design: cap is %u, the filter has %u coefficients", coeffs_host ? cap : 0u, *ncoeffs);
    return LSDR_E_ARG;
  }
  const int n = lsdr_filtergen_lowpass(order, Fcut, 1.f, coeffs_host);
  lsdr_filtergen_normalize_dcgain(n, coeffs_host, 1.f);
  *ncoeffs = (unsigned)n;
  return LSDR_OK;
}

void lsdr_resample_batch_destroy(lsdr_resample_batch *b) {
  if (!b) return;
  (void)hipStreamSynchronize(b->ctx->stream);
  b->run.destroy();
  lsdr_in_free({b->d_tab, b->d_taps, b->d_offs}, {});
  delete b;
}

static int rs_build(lsdr_resample_batch *b) {
  lsdr_ctx *c = b->ctx;
  const size_t B = (size_t)b->cfg.n_captures;
  const unsigned N = b->cfg.ncoeffs, D = b->cfg.decim;
  LSDR_HIP(hipSetDevice(c->device));
  LSDR_TRY(b->run.create(B));
  LSDR_HIP(hipMalloc((void **)&b->d_tab, 65536 * sizeof(float2)));
  LSDR_HIP(hipMalloc((void **)&b->d_taps, N * sizeof(float)));
  LSDR_HIP(hipMalloc((void **)&b->d_offs, N * sizeof(unsigned)));
  std::vector<float2> tab(65536);
  for (unsigned j = 0; j < 65536; ++j) {
    const double a = 2.0 * M_PI * (double)j / 65536.0;
    tab[j] = make_float2((float)cos(a), (float)sin(a));
  }
  LSDR_HIP(hipMemcpy(b->d_tab, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice));
  LSDR_HIP(hipMemcpy(b->d_taps, b->cfg.coeffs_host, N * sizeof(float), hipMemcpyHostToDevice));
  const unsigned S = rs_stride(b->M, N, D);
  std::vector<unsigned> offs(N);
  for (unsigned i = 0; i < N; ++i) offs[i] = ((N - i) % D) * S + (N - i) / D;
  LSDR_HIP(hipMemcpy(b->d_offs, offs.data(), N * sizeof(unsigned), hipMemcpyHostToDevice));
  b->cfg.coeffs_host = nullptr;                              // (the caller's array is not kept)
  rs_args &A = b->A;
  A.caps = b->run.d_caps; A.tab = b->d_tab; A.taps = b->d_taps; A.offs = b->d_offs;
  A.N = N; A.D = D; A.M = b->M; A.S = S;
  A.magic = D > 1u ? (unsigned)((0x100000000ull + D - 1u) / D) : 0u;
  A.in_scale = b->in.in_scale; A.in_flip = b->in.in_flip;
  return LSDR_OK;
}

int lsdr_resample_batch_create(lsdr_ctx *c, const lsdr_resample_batch_cfg *cfg, lsdr_resample_batch **out) {
  LSDR_ARG(c && cfg && out);
  if (cfg->n_captures < 1) { lsdr_set_error("resample_batch: n_captures must be at least 1 (got %d)", cfg->n_captures); return LSDR_E_ARG; }
  lsdr_in_desc in;
  LSDR_TRY(lsdr_in_describe("resample_batch", cfg->in_format, cfg->in_scale, &in));
  for (int i = 0; i < 6; ++i)
    if (cfg->reserved[i]) { lsdr_set_error("resample_batch: lsdr_resample_batch_cfg.reserved must be 0"); return LSDR_E_ARG; }
  if (!cfg->coeffs_host) { lsdr_set_error("resample_batch: coeffs_host is NULL"); return LSDR_E_ARG; }
  if (cfg->decim < 1 || cfg->decim > kRsMaxDecim) { lsdr_set_error("resample_batch: decim is %u, supported: 1 to %u", cfg->decim, kRsMaxDecim); return LSDR_E_UNSUPPORTED; }
  if (cfg->ncoeffs < 2 || cfg->ncoeffs > kRsMaxCoeffs) { lsdr_set_error("resample_batch: ncoeffs is %u, supported: 2 to %u", cfg->ncoeffs, kRsMaxCoeffs); return LSDR_E_UNSUPPORTED; }
  if (cfg->n_captures > 65535) { lsdr_set_error("resample_batch: n_captures is %d, supported: up to 65535 (one grid row per capture)", cfg->n_captures); return LSDR_E_UNSUPPORTED; }
  const unsigned M = rs_tile(cfg->ncoeffs, cfg->decim);
  if (!M) { lsdr_set_error("resample_batch: no tile of ncoeffs %u, decim %u fits LDS", cfg->ncoeffs, cfg->decim); return LSDR_E_UNSUPPORTED; }
  lsdr_resample_batch *b = new lsdr_resample_batch();
  b->ctx = c; b->cfg = *cfg; b->in = in; b->M = M;
  b->lds = rs_lds_bytes(M, cfg->ncoeffs, cfg->decim);
  b->results.assign((size_t)cfg->n_captures, lsdr_resample_result{});
  const int rc = rs_build(b);
  if (rc) { lsdr_resample_batch_destroy(b); return rc; }
  *out = b;
  return LSDR_OK;
}

unsigned lsdr_resample_batch_tile(const lsdr_resample_batch *b) { return b ? b->M : 0u; }

int lsdr_resample_batch_run_async(lsdr_resample_batch *b, const void *const *iq_dev, const lsdr_capture_each *each, lsdr_cf32 *const *out_dev,
                                  size_t cap_out) {
  LSDR_ARG(b && iq_dev && each && out_dev);
  const unsigned B = (unsigned)b->cfg.n_captures, N = b->cfg.ncoeffs, D = b->cfg.decim;
  LSDR_TRY(lsdr_in_check_each("resample_batch", "tune", B, iq_dev, each, nullptr, nullptr, b->cfg.max_samples, b->in.item_bytes));
  for (unsigned i = 0; i < B; ++i) {
    const lsdr_capture_each &e = each[i];
    if ((size_t)out_dev[i] % 16u) { lsdr_set_error("resample_batch: capture %u: the output pointer is not aligned to 16 bytes", i); return LSDR_E_ARG; }
    const size_t want = e.n_samples >= N ? (e.n_samples - N) / D : 0;
    if (want > cap_out) { lsdr_set_error("resample_batch: capture %u: cap_out is %zu, the capture produces %zu items", i, cap_out, want); return LSDR_E_ARG; }
    if (want && !out_dev[i]) { lsdr_set_error("resample_batch: capture %u produces %zu items and has no output pointer", i, want); return LSDR_E_ARG; }
  }
  LSDR_TRY(b->run.idle("resample_batch", "lsdr_resample_batch_wait"));
  lsdr_ctx *c = b->ctx;
  LSDR_HIP(hipSetDevice(c->device));
  unsigned long long longest = 0;                            // the grid is sized for it; a shorter capture's workgroups leave at once
  for (unsigned i = 0; i < B; ++i) {
    const lsdr_capture_each &e = each[i];
    const unsigned long long produced = e.n_samples >= N ? (e.n_samples - N) / D : 0;
    rs_cap &cap = b->run.h_caps[i];
    cap.in = reinterpret_cast<const unsigned char *>(iq_dev[i]);
    cap.out = reinterpret_cast<float2 *>(out_dev[i]);
    cap.produced = produced;
    cap.ifreq = (int)(e.tune * 65536);                       // C truncation: rotator's `int ifreq = freq * 65536`
    cap.wide = ((size_t)iq_dev[i] & 15u) == 0 ? 1u : 0u;
    lsdr_resample_result &r = b->results[i];
    r = lsdr_resample_result{};
    r.produced = produced; r.consumed = produced * D;
    r.ifreq = cap.ifreq; r.applied = (float)cap.ifreq / 65536.f;
    if (produced > longest) longest = produced;
  }
  const unsigned long long tiles = (longest + b->M - 1u) / b->M;
  if (tiles > 0x7fffffffull) { lsdr_set_error("resample_batch: %llu tiles exceed one launch", tiles); return LSDR_E_UNSUPPORTED; }
  LSDR_TRY(b->run.upload(c->stream));
  if (tiles) {
    in_dispatch(b->in.kind, [&](auto K) { rs_launch<K()>(b->M, dim3((unsigned)tiles, B), b->lds, c->stream, b->A); });
    LSDR_HIP(hipGetLastError());
  }
  return b->run.mark(c->stream);
}

int lsdr_resample_batch_wait(lsdr_resample_batch *b, lsdr_resample_result *results) {
  LSDR_ARG(b);
  LSDR_TRY(b->run.wait("resample_batch"));
  if (results) memcpy(results, b->results.data(), b->results.size() * sizeof(lsdr_resample_result));
  return LSDR_OK;
}

}  // extern "C"
