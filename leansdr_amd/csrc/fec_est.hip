// leansdr_amd/csrc/fec_est.hip — lsdr_fec_est: every stream's code rate estimated from its hard QPSK symbols, for the batch decoders' fec
// (lsdr_capture_batch_cfg.fec, leandvb's mandatory --cr).  The measurement is the reference's own: deconvol_sync inverts the
// convolutional code with two polynomials per output bit and readerrors() counts how often they disagree (dvb.h:225-265, 391-412);
// deconv[b] ^ deconv2[b] is a parity check of the punctured code — 0 on every error-free code word of the right rate at the right
// alignment and symbol phase, a coin flip on anything else.  Here it is swept over the five rates, every symbol phase of the puncturing
// pattern (skip) and the four alignments: 52 hypotheses per stream, many streams in one launch.  The definition: include/lsdr_hip.h.
//
//   k_fe_score<F>   blockIdx.y = stream, blockIdx.x = tile, one workgroup of 256.  The tile's symbols and the 48 in front of them go ONCE
//                   into LDS, normalised to packed 2-bit form (16 per word, MSB first) whatever the input format: coalesced loads, a
//                   funnel shift for a packed stream that starts inside a word.  Every thread then takes runs of 12 consecutive refill
//                   ENDS: a refill belongs to the tile that holds its last symbol, so each is counted exactly once at any tile size; its
//                   window is the 32 symbols up to that end — 64 bits funnel-shifted out of four packed LDS words.  12 = lcm of the
//                   halves (1, 3, 2, 3, 4 symbols per refill): inside a run every rate's skip is a compile-time constant and the 52
//                   counters stay in registers.  The alignments are not applied symbol by symbol: they are bit operations on the whole
//                   word, folded into the polynomial (fec_est_device.h: fe_polys), so a check is one popcll(w & x) & 1 and serves
//                   two alignments.  Counts: __shfl_down per wave, LDS across the four waves, one atomicAdd per workgroup and
//                   hypothesis with a nonzero count.
//   k_fe_pick       one wave per stream: lane r picks rate r's best hypothesis by exact 64-bit fraction comparisons, lane 0 writes the
//                   record (fec_est_device.h: fe_best_of_rate, fe_record).
//
// Both kernels leave by the stream's own count: nothing is read behind symbol n − 1 of a stream, nothing at all of one with n = 0.
// Integer sums: the atomics' order cannot change a count, so a record is a pure function of the stream's first min(n, max_symbols)
// symbols — the same alone, in any batch, at any tile size and in every input format.
#include <cstdlib>
#include "capture_input.h"
#include "fec_est_device.h"

namespace {

static_assert(sizeof(lsdr_fec_est_score) == 24 && sizeof(lsdr_fec_estimate) == 160, "lsdr_fec_estimate's layout");

// four symbols → one byte of the packed form, first symbol in the top bits
__device__ __forceinline__ unsigned fe_pack4(unsigned s0, unsigned s1, unsigned s2, unsigned s3) {
  return ((s0 & 3u) << 6) | ((s1 & 3u) << 4) | ((s2 & 3u) << 2) | (s3 & 3u);
}

// The tile's LDS image: word j holds the symbols base + 16·j … + 15 (base = tile start − 48, may be negative: zeros), zeros from symbol n on.
template <int F>
__device__ __forceinline__ void fe_stage(const fe_stream &S, long long base, unsigned words, unsigned *lds) {
  const unsigned t = threadIdx.x;
  if constexpr (F == LSDR_HSYM_PACKED2) {
    const unsigned *in = static_cast<const unsigned *>(S.sym);
    const unsigned long long last = (S.off + S.n - 1u) >> 4;             // the last word that holds a symbol of the stream
    for (unsigned j = t; j < words; j += kFeThreads) {
      const long long g0 = base + 16ll * j;
      unsigned w = 0;
      if (g0 >= 0 && (unsigned long long)g0 < S.n) {
        const unsigned long long bit = S.off + (unsigned long long)g0, wi = bit >> 4;
        const unsigned sh = 2u * (unsigned)(bit & 15u);
        const unsigned a = in[wi], b = sh && wi < last ? in[wi + 1] : 0u;
        w = sh ? (a << sh) | (b >> (32u - sh)) : a;
        const unsigned long long left = S.n - (unsigned long long)g0;      // symbols of the stream in this word
        if (left < 16u) w &= ~0u << (32u - 2u * (unsigned)left);
      }
      lds[j] = w;
    }
  } else {
    // one thread per four symbols: byte 3 − (q & 3) of word q >> 2 (MSB first in a little-endian word)
    unsigned char *lb = reinterpret_cast<unsigned char *>(lds);
    for (unsigned q = t; q < 4u * words; q += kFeThreads) {
      const long long g0 = base + 4ll * q;
      unsigned v = 0;
      if (g0 >= 0 && (unsigned long long)g0 < S.n) {
        const bool whole = (unsigned long long)g0 + 4u <= S.n;
        if constexpr (F == LSDR_HSYM_U8) {
          const unsigned char *p = static_cast<const unsigned char *>(S.sym) + (unsigned long long)g0;
          if (whole && ((size_t)p & 3u) == 0) {
            const unsigned x = *reinterpret_cast<const unsigned *>(p);
            v = fe_pack4(x, x >> 8, x >> 16, x >> 24);
          } else {
            unsigned s[4] = {0u, 0u, 0u, 0u};
            for (unsigned i = 0; i < 4u; ++i)
              if ((unsigned long long)g0 + i < S.n) s[i] = p[i];
            v = fe_pack4(s[0], s[1], s[2], s[3]);
          }
        } else {
          const unsigned *p = static_cast<const unsigned *>(S.sym) + (unsigned long long)g0;   // lsdr_softsymbol: symbol in byte 2
          if (whole && ((size_t)p & 15u) == 0) {
            const uint4 x = *reinterpret_cast<const uint4 *>(p);
            v = fe_pack4(x.x >> 16, x.y >> 16, x.z >> 16, x.w >> 16);
          } else {
            unsigned s[4] = {0u, 0u, 0u, 0u};
            for (unsigned i = 0; i < 4u; ++i)
              if ((unsigned long long)g0 + i < S.n) s[i] = p[i] >> 16;
            v = fe_pack4(s[0], s[1], s[2], s[3]);
          }
        }
      }
      lb[(q & ~3u) + 3u - (q & 3u)] = (unsigned char)v;
    }
  }
}

// the checks of one refill of rate R that ends at step `step` of a run (the run's first end e0 has (e0 − 31) ≡ 5 mod 12: tiles are
// multiples of 12): skip = (step + 5) mod half
template <unsigned R, unsigned STEP>
__device__ __forceinline__ void fe_refill(const fe_polys &P, unsigned long long w, unsigned (&acc)[kFeHyp]) {
  constexpr fe_rate_info ri = fe_rate(R);
  constexpr unsigned slot = ri.base + (STEP + 5u) % ri.half;
#pragma unroll
  for (unsigned b = 0; b < ri.pp; ++b) {
    const unsigned j = ri.pbase + b;
    const unsigned p = (unsigned)__popcll(w & P.x[j]), ps = (unsigned)__popcll(w & P.xs[j]);
    acc[slot * 4u + 0u] += (p ^ (P.flip[0] >> j)) & 1u;
    acc[slot * 4u + 1u] += (ps ^ (P.flip[1] >> j)) & 1u;
    acc[slot * 4u + 2u] += (p ^ (P.flip[2] >> j)) & 1u;
    acc[slot * 4u + 3u] += (ps ^ (P.flip[3] >> j)) & 1u;
  }
}
template <unsigned STEP>
__device__ __forceinline__ void fe_step(const fe_polys &P, unsigned long long hi, unsigned long long lo, unsigned so, unsigned long long e,
                                        unsigned long long n, unsigned (&acc)[kFeHyp]) {
  if (e >= 31u && e < n) {
    const unsigned s = 2u * (so + 1u + STEP);                            // 2 … 48: the window starts s/2 symbols into the four words
    const unsigned long long w = (hi << s) | (lo >> (64u - s));
    fe_refill<0, STEP>(P, w, acc); fe_refill<1, STEP>(P, w, acc); fe_refill<2, STEP>(P, w, acc);
    fe_refill<3, STEP>(P, w, acc); fe_refill<4, STEP>(P, w, acc);
  }
  if constexpr (STEP + 1u < kFeGroup) fe_step<STEP + 1u>(P, hi, lo, so, e + 1u, n, acc);
}

template <int F>
__global__ __launch_bounds__(kFeThreads) void k_fe_score(fe_args A) {
  const fe_stream S = A.st[blockIdx.y];
  const unsigned long long t0 = (unsigned long long)blockIdx.x * A.tile;
  if (t0 >= S.n) return;
  __shared__ unsigned lds[kFeMaxWords];
  __shared__ unsigned tot[kFeHyp];
  const unsigned t = threadIdx.x;
  if (t < kFeHyp) tot[t] = 0;
  fe_stage<F>(S, (long long)t0 - (long long)kFeHist, A.tile / 16u + 4u, lds);
  __syncthreads();
  unsigned acc[kFeHyp];
#pragma unroll
  for (unsigned h = 0; h < kFeHyp; ++h) acc[h] = 0;
#pragma unroll 1
  for (unsigned g = 0; g < A.groups; ++g) {
    const unsigned gi = g * kFeThreads + t;                                // run gi of the tile: ends t0 + 12·gi … + 11
    const unsigned long long e0 = t0 + (unsigned long long)kFeGroup * gi;
    if (e0 >= S.n) break;                                                  // (ascending in g)
    // the end e0 + step looks at the symbols e0 + step − 31 … e0 + step: LDS symbol 12·gi + 17 + step on (word 0 starts 48 in front of t0)
    const unsigned q = kFeGroup * gi + 16u, wi = q >> 4, so = q & 15u;
    const unsigned long long hi = ((unsigned long long)lds[wi] << 32) | lds[wi + 1u], lo = ((unsigned long long)lds[wi + 2u] << 32) | lds[wi + 3u];
    fe_step<0>(A.P, hi, lo, so, e0, S.n, acc);
  }
#pragma unroll
  for (unsigned h = 0; h < kFeHyp; ++h) {
    unsigned v = acc[h];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if ((t & 63u) == 0 && v) atomicAdd(&tot[h], v);
  }
  __syncthreads();
  if (t < kFeHyp && tot[t]) atomicAdd(A.counts + (size_t)blockIdx.y * kFeHyp + t, (unsigned long long)tot[t]);
}

__global__ __launch_bounds__(64) void k_fe_pick(fe_args A) {
  const fe_stream S = A.st[blockIdx.x];
  __shared__ lsdr_fec_est_score sc[kFeRates];
  const unsigned t = threadIdx.x;
  if (t < kFeRates) sc[t] = fe_best_of_rate(t, A.counts + (size_t)blockIdx.x * kFeHyp, S.n);
  __syncthreads();
  if (t == 0) {
    lsdr_fec_est_score all[kFeRates];
    for (unsigned r = 0; r < kFeRates; ++r) all[r] = sc[r];
    A.rec[blockIdx.x] = fe_record(all, S.n);
  }
}

// the alignment maps as swap + mask on packed symbols, from init_syncs' tables (dvb.h:308-360); false if one of them is not of that form
bool fe_affine(const unsigned char (&lut)[4], bool &swap, unsigned &mask2) {
  swap = ((lut[0] ^ lut[1]) & 3u) == 2u;
  mask2 = lut[0] & 3u;
  for (unsigned s = 0; s < 4; ++s) {
    const unsigned m = swap ? ((s >> 1) | ((s & 1u) << 1)) : s;
    if ((lut[s] & 3u) != (m ^ mask2)) return false;
  }
  return true;
}
unsigned long long fe_swap_pairs(unsigned long long x) {
  const unsigned long long M = 0x5555555555555555ull;
  return ((x >> 1) & M) | ((x & M) << 1);
}

}  // namespace

struct lsdr_fec_est {
  lsdr_ctx *ctx = nullptr;
  lsdr_fec_est_cfg cfg{};
  fe_args A{};
  in_run<fe_stream> run;
  unsigned long long *d_counts = nullptr;
  lsdr_fec_estimate *h_rec = nullptr, *d_rec = nullptr;                   // pinned / device
};

static int fe_rate_of(unsigned r) { return fe_rate(r).fec; }

extern "C" {

int lsdr_fec_est_polys(int rate, uint64_t deconv[8], uint64_t deconv2[8], int *punctweight) {
  bool known = false;
  for (unsigned r = 0; r < kFeRates; ++r) known = known || rate == fe_rate_of(r);
  if (!known || !deconv || !deconv2) { lsdr_set_error("fec_est: polys: rate %d is none of LSDR_FEC12, 23, 34, 56, 78, or a NULL array", rate); return 0; }
  lsdr_deconv_polys P;
  if (lsdr_deconv_polys_build(rate, &P)) return 0;
  for (int b = 0; b < 8; ++b) { deconv[b] = b < P.pp ? P.deconv[b] : 0; deconv2[b] = b < P.pp ? P.deconv2[b] : 0; }
  if (punctweight) *punctweight = P.pw;
  return P.pp;
}

void lsdr_fec_est_destroy(lsdr_fec_est *e) {
  if (!e) return;
  (void)hipStreamSynchronize(e->ctx->stream);
  e->run.destroy();
  lsdr_in_free({e->d_counts, e->d_rec}, {e->h_rec});
  delete e;
}

static int fe_build(lsdr_fec_est *e) {
  fe_polys &P = e->A.P;
  memset(&P, 0, sizeof(P));
  unsigned char luts[4][4];
  lsdr_deconv_luts(luts);
  bool swap[4]; unsigned mask2[4];
  for (int a = 0; a < 4; ++a)
    if (!fe_affine(luts[a], swap[a], mask2[a]) || swap[a] != ((a & 1) != 0)) { lsdr_set_error("fec_est: alignment %d is no swap-and-mask map", a); return LSDR_E_UNSUPPORTED; }
  for (unsigned r = 0; r < kFeRates; ++r) {
    const fe_rate_info ri = fe_rate(r);
    lsdr_deconv_polys H;
    LSDR_TRY(lsdr_deconv_polys_build(ri.fec, &H));
    if ((unsigned)H.pp != ri.pp || (unsigned)H.pw != 2u * ri.half) { lsdr_set_error("fec_est: rate %u: unexpected puncturing", r); return LSDR_E_UNSUPPORTED; }
    for (unsigned b = 0; b < ri.pp; ++b) {
      const unsigned long long x = H.deconv[b] ^ H.deconv2[b];
      if (!x) { lsdr_set_error("fec_est: rate %u: Alt polynomial not provided", r); return LSDR_E_UNSUPPORTED; }
      const unsigned j = ri.pbase + b;
      P.x[j] = x; P.xs[j] = fe_swap_pairs(x);
      for (int a = 0; a < 4; ++a)
        P.flip[a] |= (unsigned)__builtin_parityll((mask2[a] * 0x5555555555555555ull) & x) << j;
    }
  }
  lsdr_ctx *c = e->ctx;
  const size_t B = (size_t)e->cfg.n_streams;
  LSDR_HIP(hipSetDevice(c->device));
  LSDR_TRY(e->run.create(B));
  LSDR_HIP(hipHostMalloc((void **)&e->h_rec, B * sizeof(lsdr_fec_estimate), hipHostMallocDefault));
  memset(e->h_rec, 0, B * sizeof(lsdr_fec_estimate));
  LSDR_HIP(hipMalloc((void **)&e->d_rec, B * sizeof(lsdr_fec_estimate)));
  LSDR_HIP(hipMalloc((void **)&e->d_counts, B * kFeHyp * sizeof(unsigned long long)));
  // runs per thread: the tile is 3072 symbols times this.  LSDR_FEC_EST_GROUPS (1 … 8) is a tuning hook: the records do not depend on it
  unsigned groups = 1;
  if (const char *g = getenv("LSDR_FEC_EST_GROUPS")) {
    const int v = atoi(g);
    if (v >= 1 && v <= (int)kFeMaxGroups) groups = (unsigned)v;
  }
  e->A.st = e->run.d_caps; e->A.counts = e->d_counts; e->A.rec = e->d_rec;
  e->A.groups = groups; e->A.tile = kFeGroup * kFeThreads * groups;
  return LSDR_OK;
}

int lsdr_fec_est_create(lsdr_ctx *c, const lsdr_fec_est_cfg *cfg, lsdr_fec_est **out) {
  LSDR_ARG(c && cfg && out);
  if (cfg->n_streams < 1 || cfg->n_streams > 65535) { lsdr_set_error("fec_est: n_streams must be 1 to 65535 (got %d)", cfg->n_streams); return LSDR_E_ARG; }
  // (7·max_symbols checks at most: below 2^28 symbols the products of the exact fraction comparisons stay inside 64 bits)
  if (cfg->max_symbols == 0 || cfg->max_symbols > ((size_t)1 << 28)) { lsdr_set_error("fec_est: max_symbols must be 1 to 2^28 (got %zu)", cfg->max_symbols); return LSDR_E_ARG; }
  if (cfg->in_format != LSDR_HSYM_PACKED2 && cfg->in_format != LSDR_HSYM_U8 && cfg->in_format != LSDR_HSYM_SOFT) {
    lsdr_set_error("fec_est: in_format %d is none of LSDR_HSYM_PACKED2, _U8, _SOFT", cfg->in_format); return LSDR_E_ARG;
  }
  for (int i = 0; i < 5; ++i)
    if (cfg->reserved[i]) { lsdr_set_error("fec_est: lsdr_fec_est_cfg.reserved must be 0"); return LSDR_E_ARG; }
  lsdr_fec_est *e = new lsdr_fec_est();
  e->ctx = c; e->cfg = *cfg;
  const int rc = fe_build(e);
  if (rc) { lsdr_fec_est_destroy(e); return rc; }
  *out = e;
  return LSDR_OK;
}

unsigned lsdr_fec_est_tile(const lsdr_fec_est *e) { return e ? e->A.tile : 0u; }

int lsdr_fec_est_run_async(lsdr_fec_est *e, const void *const *sym_dev, const uint64_t *sym_offset, const uint64_t *n) {
  LSDR_ARG(e && sym_dev && n);
  const unsigned B = (unsigned)e->cfg.n_streams;
  const int F = e->cfg.in_format;
  const size_t align = F == LSDR_HSYM_U8 ? 1u : 4u;
  for (unsigned i = 0; i < B; ++i) {
    if (n[i] && !sym_dev[i]) { lsdr_set_error("fec_est: stream %u has symbols and no pointer", i); return LSDR_E_ARG; }
    if ((size_t)sym_dev[i] % align) { lsdr_set_error("fec_est: stream %u: the pointer is not aligned to %zu bytes", i, align); return LSDR_E_ARG; }
  }
  LSDR_TRY(e->run.idle("fec_est", "lsdr_fec_est_wait"));
  lsdr_ctx *c = e->ctx;
  LSDR_HIP(hipSetDevice(c->device));
  unsigned long long longest = 0;                                         // the grid is sized for it; a shorter stream's workgroups leave at once
  for (unsigned i = 0; i < B; ++i) {
    fe_stream &S = e->run.h_caps[i];
    const unsigned long long off = sym_offset ? sym_offset[i] : 0u;
    S.n = n[i] < e->cfg.max_symbols ? n[i] : e->cfg.max_symbols;
    if (F == LSDR_HSYM_PACKED2) { S.sym = sym_dev[i]; S.off = off; }
    else { S.sym = S.n ? static_cast<const unsigned char *>(sym_dev[i]) + off * (F == LSDR_HSYM_U8 ? 1u : 4u) : nullptr; S.off = 0; }
    if (S.n > longest) longest = S.n;
  }
  LSDR_TRY(e->run.upload(c->stream));
  LSDR_HIP(hipMemsetAsync(e->d_counts, 0, (size_t)B * kFeHyp * sizeof(unsigned long long), c->stream));
  if (longest) {
    const dim3 grid((unsigned)((longest + e->A.tile - 1u) / e->A.tile), B);
    if (F == LSDR_HSYM_PACKED2) hipLaunchKernelGGL(k_fe_score<LSDR_HSYM_PACKED2>, grid, dim3(kFeThreads), 0, c->stream, e->A);
    else if (F == LSDR_HSYM_U8) hipLaunchKernelGGL(k_fe_score<LSDR_HSYM_U8>, grid, dim3(kFeThreads), 0, c->stream, e->A);
    else hipLaunchKernelGGL(k_fe_score<LSDR_HSYM_SOFT>, grid, dim3(kFeThreads), 0, c->stream, e->A);
  }
  hipLaunchKernelGGL(k_fe_pick, dim3(B), dim3(64), 0, c->stream, e->A);
  LSDR_HIP(hipGetLastError());
  LSDR_HIP(hipMemcpyAsync(e->h_rec, e->d_rec, (size_t)B * sizeof(lsdr_fec_estimate), hipMemcpyDeviceToHost, c->stream));
  return e->run.mark(c->stream);
}

int lsdr_fec_est_wait(lsdr_fec_est *e, lsdr_fec_estimate *out) {
  LSDR_ARG(e && out);
  LSDR_TRY(e->run.wait("fec_est"));
  memcpy(out, e->h_rec, (size_t)e->cfg.n_streams * sizeof(lsdr_fec_estimate));
  return LSDR_OK;
}

}  // extern "C"
