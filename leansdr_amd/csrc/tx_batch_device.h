// leansdr_amd/csrc/tx_batch_device.h — what the generator side's files share: tx.hip and chan.hip (the one-stream blocks) and tx_batch.hip
// (lsdr_tx_batch).  The text of the device functions is the blocks' own, moved here unchanged:
//   drand48 as a 48-bit LCG with its O(log k) jump, glibc 2.35's logf restated, the x86 float → integer conversions (chan.hip);
//   the GF(256) tables of the RS encoder (tx.hip);
// and the records that tx_batch.hip's kernels and host code exchange.
#ifndef LSDR_TX_BATCH_DEVICE_H
#define LSDR_TX_BATCH_DEVICE_H
#include "lsdr_internal.h"

constexpr unsigned long long kLcgA = 0x5DEECE66DULL, kLcgC = 0xBULL, kLcgMask = 0xFFFFFFFFFFFFULL;

struct lcg_pow { unsigned long long a[48], c[48]; };               // X_{k+2^b} = a[b]·X_k + c[b]  (mod 2^48)
struct logf_tab { double invc[16], logc[16]; };
struct gf_tab { unsigned char exp[512], log[256], G[17]; };

__device__ __forceinline__ unsigned long long lcg_jump(const lcg_pow &p, unsigned long long x, unsigned long long k) {
  for (int b = 0; b < 48 && (k >> b); ++b)
    if ((k >> b) & 1) x = (p.a[b] * x + p.c[b]) & kLcgMask;
  return x;
}
__device__ __forceinline__ double lcg_next(unsigned long long &x) {
  x = (x * kLcgA + kLcgC) & kLcgMask;
  return (double)x * 0x1p-48;
}
// glibc 2.35 logf for positive normal x (sysdeps/ieee754/flt-32/e_logf.c)
__device__ __forceinline__ float glibc_logf(const logf_tab &t, float x) {
  const unsigned ix = __float_as_uint(x);
  if (ix == 0x3f800000u) return 0.f;
  const unsigned tmp = ix - 0x3f330000u;
  const int i = (tmp >> 19) % 16, k = (int)tmp >> 23;
  const unsigned iz = ix - (tmp & (0x1ffu << 23));
  const double z = (double)__uint_as_float(iz), r = z * t.invc[i] - 1, y0 = t.logc[i] + (double)k * 0x1.62e42fefa39efp-1, r2 = r * r;
  double y = 0x1.5575b0be00b6ap-2 * r + -0x1.ffffef20a4123p-2;
  y = -0x1.00ea348b88334p-2 * r2 + y;
  y = y * r2 + (y0 + r);
  return (float)y;
}

// cvttss2si / cvttsd2si: the "integer indefinite" value when the source is NaN or out of range
__device__ __forceinline__ int x86_f2i(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000; }
__device__ __forceinline__ long long x86_d2l(double v) {
  return (v >= -9223372036854775808.0 && v < 9223372036854775808.0) ? (long long)v : (long long)0x8000000000000000ULL;
}

// ---- host: the two tables of wgn_c
inline void lsdr_lcg_pow_fill(lcg_pow &p) {
  p.a[0] = kLcgA; p.c[0] = kLcgC;
  for (int b = 1; b < 48; ++b) {   // (a,c)∘(a,c): X → a·(a·X + c) + c
    p.a[b] = (p.a[b - 1] * p.a[b - 1]) & kLcgMask;
    p.c[b] = (p.a[b - 1] * p.c[b - 1] + p.c[b - 1]) & kLcgMask;
  }
}
inline void lsdr_logf_tab_fill(logf_tab &lt) {
  // glibc 2.35 sysdeps/ieee754/flt-32/e_logf_data.c (N = 16): {1/c, log c} for the 16 sub-intervals of [0.7, 1.4)
  static const double tab[16][2] = {
      {0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2}, {0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2},
      {0x1.49539f0f010bp+0, -0x1.01eae7f513a67p-2},  {0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3},
      {0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3}, {0x1.25e227b0b8eap+0, -0x1.1aa2bc79c81p-3},
      {0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4}, {0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4},
      {0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5}, {0x1p+0, 0x0p+0},
      {0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5},  {0x1.ca4b31f026aap-1, 0x1.c5e53aa362eb4p-4},
      {0x1.b2036576afce6p-1, 0x1.526e57720db08p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.bc2860d22477p-3},
      {0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2},  {0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2},
  };
  for (int i = 0; i < 16; ++i) { lt.invc[i] = tab[i][0]; lt.logc[i] = tab[i][1]; }
}
// glibc keeps the drand48 state in zeroed static storage: an unseeded process starts from X = 0; srand48(s): X = s<<16 | 0x330E
inline unsigned long long lsdr_drand48_start(int seeded, long long seed) {
  return seeded ? ((((unsigned long long)(unsigned)seed) << 16) | 0x330E) : 0ULL;
}

// ---- lsdr_tx_batch: the records of a run -----------------------------------------------------------------------------------------
constexpr unsigned kTxbThreads = 256;
constexpr unsigned kTxbTile = 2048;          // output samples per workgroup of the sample stage: 16 AGC chunks
constexpr unsigned kTxbMaxTaps = 1024;       // taps in LDS
constexpr unsigned kTxbMaxSpan = 16384;      // symbol bytes a sample tile may need, in LDS
constexpr unsigned kTxbNoisePairs = 16;      // candidate pairs per thread of the noise stage, 4096 per workgroup
constexpr unsigned kTxbNoiseBlock = kTxbThreads * kTxbNoisePairs;

// one stream of a run: uploaded by run_async (the noise fields again by every further round)
struct txb_stream {
  const unsigned char *ts;                   // n_packets · 188 bytes
  unsigned long long n_packets, il_packets, bytes, symbols, resampled, samples;   // lsdr_tx_batch_plan's lengths; resampled: before the AGC's chunks
  unsigned short rpolys[8];                  // the polynomials bit-reversed in 16 bits: newest input bit at bit 0 of the window
  int bits_in, bits_out, bps;
  unsigned point_set;                        // which of the run's point tables
  float scale, stddev, out_rms, bw;
  // noise stage
  unsigned long long x0, done0, npairs;      // state and outputs written at the round's start, the round's candidate pairs
  unsigned round, pad;
};
// what the noise stage leaves per stream (the host seeds it with {done0, x0} at every round)
struct txb_noise_out { unsigned long long done, state; };

struct txb_args {
  const txb_stream *st;
  unsigned char *rs;                         // [B][max_packets · 204]   randomized, RS-encoded packets
  unsigned char *sym;                        // [B][sym_stride]          one byte per symbol
  float2 *y;                                 // [B][y_stride]            resampled, decimated, before the AGC
  float *gain;                               // [B][chunk_stride]        chunk powers, then gains (AGC only)
  float *est;                                // [B]                      simple_agc::estimated
  const float2 *taps;                        // [B][kTxbMaxTaps]         this run's shifted taps (freq 0), per stream
  const float2 *points;                      // [point sets][256]
  unsigned *ncount;                          // [B][noise_blocks]
  unsigned long long *noff;                  // [B][noise_blocks + 1]
  txb_noise_out *nout;                       // [B]
  unsigned char *out;                        // [B][out_stride bytes]
  lsdr_tx_result *results;                   // [B]
  const gf_tab *gf;
  const unsigned char *pattern;              // the randomizer's 1504 bytes
  const lcg_pow *pw;
  const logf_tab *lt;
  size_t rs_stride, sym_stride, y_stride, chunk_stride, out_stride;
  unsigned noise_blocks;                     // per stream, the buffers' capacity
  unsigned n_streams, ncoeffs, interp, decim, latency, agc, out_u8;
};
#endif
