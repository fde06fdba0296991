// leansdr_amd/csrc/spectrum_batch_device.h — the arithmetic and the layouts of lsdr_spectrum_batch (include/lsdr_hip.h; kernels and host side
// in spectrum_batch.hip).  Plain C++ on values and arrays, callable from a kernel and from the host: which block a row is taken from, where
// a point and a twiddle sit in LDS, and a pass of consecutive radix-2 stages of cfft_engine<float>::inplace (dsp.h:78-110) kept in registers.
#ifndef LSDR_SPECTRUM_BATCH_DEVICE_H
#define LSDR_SPECTRUM_BATCH_DEVICE_H

#define SB_HD __host__ __device__ __forceinline__

constexpr unsigned kSbPoints = 4096;     // points per workgroup: one transform of 4096, four of 1024, … 64 of 64
constexpr unsigned kSbLogPoints = 12;
constexpr unsigned kSbThreads = 256;
constexpr unsigned kSbMaxStages = 4;     // radix-2 stages per pass at most: 16 points per thread

// THE ROW/BLOCK RULE (sdr.h:1292-1301, 1362-1371): run() adds nfft to `phase` per whole block and fetches the block with which phase
// reaches `decimation`, then subtracts decimation.  With decimation >= nfft at most one row per block: row m (1-based) is taken from block
// ceil(m·decimation / nfft) − 1, and J whole blocks give floor(J·nfft / decimation) rows.
SB_HD unsigned long long sb_rows(unsigned long long blocks, unsigned logn, unsigned decimation) { return (blocks << logn) / decimation; }
SB_HD unsigned long long sb_block_of_row(unsigned long long m, unsigned logn, unsigned decimation) {
  return ((m * decimation + ((1ull << logn) - 1ull)) >> logn) - 1ull;
}

// LDS layouts.  A point at index i sits at i + i/16: a thread's 16 consecutive points (first pass) are then 17 float2 from its neighbour's,
// and the 32 lanes of a half wave read 32 different pairs of banks.  Twiddle om[i] sits at i + i/8 + i/128: the strides k·2^j the later
// stages read with spread over the banks the same way.
SB_HD unsigned sb_dp(unsigned i) { return i + (i >> 4); }
SB_HD unsigned sb_tp(unsigned i) { return i + (i >> 3) + (i >> 7); }
constexpr unsigned kSbDataLds = kSbPoints + (kSbPoints >> 4);                 // float2
SB_HD unsigned sb_tw_lds(unsigned nfft) { return sb_tp(nfft / 2u) + 1u; }       // float2, for om[0 .. nfft/2)

// Stages st … st+S−1 of every transform in d[] (all of logn stages each; the transforms lie one behind the other in the index space of
// kSbPoints points, so a group of 2^S points never straddles two).  A group: the points whose index differs in bits [st, st+S) only.  The
// butterfly is the reference's expression (dsp.h:96-104), evaluated once per butterfly; which thread evaluates it, and when, does not
// enter its value, so S stages in registers give the bits of S passes through LDS.  A barrier belongs between two passes.
template <int S>
SB_HD void sb_pass(float2 *d, const float2 *w, unsigned st, unsigned logn, unsigned tid) {
  constexpr unsigned R = 1u << S;
  for (unsigned G = tid; G < (kSbPoints >> S); G += kSbThreads) {
    const unsigned low = G & ((1u << st) - 1u), base = ((G >> st) << (st + S)) | low;
    float2 v[R];
#pragma unroll
    for (unsigned r = 0; r < R; ++r) v[r] = d[sb_dp(base + (r << st))];
#pragma unroll
    for (unsigned s = 0; s < (unsigned)S; ++s) {
      const unsigned dom_shift = logn - 1u - (st + s);           // om[k·dom], dom = n / 2^(stage+1)
#pragma unroll
      for (unsigned b = 0; b < R / 2u; ++b) {
        const unsigned lo = b & ((1u << s) - 1u), r0 = ((b >> s) << (s + 1u)) | lo, r1 = r0 | (1u << s);
        const unsigned k = low | (lo << st);                     // the point's index within its half block of this stage
        const float2 ww = w[sb_tp(k << dom_shift)], dd = v[r1], dpv = v[r0];
        const float xr = ww.x * dd.x - ww.y * dd.y;
        const float xi = ww.x * dd.y + ww.y * dd.x;
        v[r1] = make_float2(dpv.x - xr, dpv.y - xi);
        v[r0] = make_float2(dpv.x + xr, dpv.y + xi);
      }
    }
#pragma unroll
    for (unsigned r = 0; r < R; ++r) d[sb_dp(base + (r << st))] = v[r];
  }
}

// the band sums of cnr_fft (sdr.h:1334-1338): a serial float sum in index order, indices wrapped into the transform
// (sixteen loads in flight, then their adds in index order: the sum is serial, the loads need not wait for it)
SB_HD float sb_band_sum(const float *avg, int i0, int i1, unsigned nfft) {
  float s = 0;
  int i = i0;
  for (; i + 15 <= i1; i += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = avg[(unsigned)(i + u) & (nfft - 1u)];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += v[u];
  }
  for (; i <= i1; ++i) s += avg[(unsigned)i & (nfft - 1u)];
  return s;
}
// band 0: the carrier's, icf ± bw; 1 and 2: the noise floors at −4bw … −3bw and +3bw … +4bw
SB_HD void sb_band(int band, int icf, int bw, int *i0, int *i1) {
  if (band == 0) { *i0 = icf - bw; *i1 = icf + bw; }
  else if (band == 1) { *i0 = icf - bw * 4; *i1 = icf - bw * 3; }
  else { *i0 = icf + bw * 3; *i1 = icf + bw * 4; }
}
#endif
