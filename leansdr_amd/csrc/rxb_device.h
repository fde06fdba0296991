// leansdr_amd/csrc/rxb_device.h — device side of the CAPTURE BATCH receiver (lsdr_capture_batch, include/lsdr_hip.h): the front end of
// leandvb's default graph for `--u8` input (leandvb.cc:211-217,296-301,476-510: cconverter<u8> → auto_notch(1 slot) → cstln_receiver with
// the linear sampler), for B independent captures decoded from their first sample, all of them in ONE set of launches.  Included inside
// cstln_receiver.hip's anonymous namespace (it reuses rx_tile_exact, the seam pass and the packed compaction of rx_tiling.h).
//
//   k_rxb_detect_fft / k_rxb_detect_peaks / k_rxb_iv   auto_notch::detect() (sdr.h:76-118) at every detect point of every capture: the
//                        reference's FFT bit for bit (notch_detect.h), first maximum, and per detect interval the notch's pole
//                        p = (1−k)·exp(j2π·bin/4096) and whether the estimator restarts there (sdr.h:94-103: only when the bin changes)
//   k_rxb_notch_pre      zero-start sums of the estimator recurrence over blocks of `pre_block` samples: a tile that starts in the
//                        middle of a capture gets its estimator from the few blocks in front of it ((1−k)^8192 < 1e-7)
//   (every kernel that reads a capture is instantiated per sample format — "sample formats" below: cu8 as it always was; cs8, cu16 / cs16
//    and cf32 with scaler's factor for lsdr_capture_any_create: leandvb --s8 / --u16 / --s16 / --f32 --float-scale, leandvb.cc:208-261)
//   k_rxb_tiles<NOTCH>   the tolerance tiles (one lane per tile, 64 consecutive tiles of one capture per wavefront, cu8 samples staged
//                        through LDS by buffer→LDS loads), packed 2-bit decisions out (rx_tiling.h "hs2")
//   k_rxb_seam / k_rxb_compact   rx_tiling.h's seam pass and packed compaction, blockIdx.y = capture
//   k_rxb_tiles_soft<NOTCH> / k_rxb_compact_soft   the same tiles with SOFT symbols out (leandvb --viterbi: viterbi_sync reads
//                        softsymbol{cost, symbol}, sdr.h:287-290): one 4-byte record per body symbol, staged transposed (row = symbol
//                        index, column = tile) and compacted through LDS into one contiguous lsdr_softsymbol array per capture
//   k_rxb_tiles_rep<NOTCH, SOFT, K> / k_rxb_reports   signal reports (lsdr_capture_reports_set: cstln_receiver's FREQ / SS / MER pipes,
//                        sdr.h:857-913): the same tiles with the estimators' affine map per tile and a slot per measurement instant, and the
//                        scan that composes a capture's maps from the constructed estimators (rxb_rep below).  Only objects that asked for
//                        reports launch them.
//
// The notch inside a tile.  sdr.h:119-138 with one slot is, per detect interval, estim[n] = (1−k)·estim[n−1] + k·x[n]·conj(e[n]),
// out[n] = x[n] − estim[n]·e[n], e[n] = exp(j2π·bin·n/4096) (n counted from the block start; 4096·bin/4096 is whole, so the phasor runs
// on across blocks).  With S[n] = estim[n]·e[n]:  S[n] = p·S[n−1] + k·x[n],  out[n] = x[n] − S[n] — one complex multiply-add per sample,
// no table.  TOLERANCE MODE like lsdr_notch_fir (float32 with exact phases, not the reference's table of cosf/sinf of a rounded angle):
// tests/test_gpu_capture_batch.py holds the notched samples against the oracle's auto_notch, and the TS against the reference binary's.
//
// The tile's symbol step.  Same loop as rx_tile_tol (sdr.h:790-916 per chunk: interpolate, AGC, slice, PLL, Mueller & Müller, estimators
// per chunk) restated for QPSK / linear sampler / packed decisions with about half the vector instructions per symbol — this kernel is
// bound by VALU issue, not by HBM:
//   * the linear sampler's two derotations (sdr.h:614-623) as ONE: s = (p0·(1−mu) + p1·e^{−jf}·mu)·e^{−j·phase}, e^{−jf} once per chunk
//     (sampler->update_freq is per chunk, sdr.h:790), e^{−j·phase} from v_cos/v_sin on the unquantised phase;
//   * decisions by arithmetic on the truncated coordinates (what cstln_lut<256> holds for QPSK, sdr.h:529-560): symbol = the two sign
//     bits, phase error = atan((|Q|−|I|)/(|Q|+|I|)) by an odd polynomial — atan2 − π/4 without the octant folding;
//   * fused multiply-adds throughout; the sample-skipping steps as one floor();
//   * the samples of the next symbol are fetched from LDS a whole symbol step ahead.
#ifndef LSDR_RXB_DEVICE_H
#define LSDR_RXB_DEVICE_H

struct rxb_iv { float pr, pi, k; int seg_block, bin, pad0, pad1, pad2; };   // one detect interval: pole, gain (0: no notch yet), first pre-block of its constant-bin segment, bin

struct rxb_cap {
  const unsigned char *in;             // cu8 items
  unsigned long long total_chunks;     // 128-sample chunks the receiver runs over
  unsigned n_tiles, n_det;
  unsigned *hstage; unsigned long long hpitch;
  rx_tile_info_h *hinfo;
  rx_tile_fix *fix; rx_seam_part *part;
  unsigned *out_words;
  rx_seam_result *res;                 // device memory: total symbols, seam statistics
  rx_state_dev *state_end;             // where the last tile leaves phase / freqw (rx_tiling.h reads freq_tap there)
  rx_ema_map *ema_scratch;             // [2]: what rx_tile_exact writes for the estimator scan nobody runs here
  rxb_iv *iv;                          // [n_det + 1]
  float2 *T;                           // [n_pre] zero-start block sums of S
  int *cand;                           // [n_det][kDetMaxSlots]
  float2 *halves;                      // [n_det][2][2048]
  // soft tiles only (null otherwise)
  unsigned *sstage;                    // body symbol k of tile j at sstage[k·hpitch + j]: cost in bits 15:0, symbol in bits 23:16 (lsdr_softsymbol)
  unsigned *spre;                      // [n_tiles] the warm-up's last symbol, as a soft record (the one a seam may re-insert)
  unsigned *out_soft;                  // the capture's compacted soft symbols
  unsigned long long *count_out;       // → the capture's entry of a contiguous uint64[n_captures]: symbols in out_soft
  const rx_state_dev *state0;          // the capture's loop state right after construction: set_freq(its tune) (lsdr_capture_each)
};

// Signal reports of one capture (`--fd-info`: cstln_receiver writes FREQ / SS / MER once per meas_decimation samples, sdr.h:857-913).
// The estimators behind them are EMAs with a constant pole (rx_ema_map, cstln_receiver.hip): a tile records the affine map of its body
// chunks, and for the chunk that holds a measurement instant a slot with the partial map up to there; k_rxb_reports composes the maps
// from the constructed estimators and turns the slots into values.
struct rxb_rep {
  rx_ema_map *map;                     // [n_tiles] the tile's map; behind k_rxb_reports the estimator VALUES in front of the tile (bi, bs, be)
  rx_meas *slot;                       // [reports + 1] one per measurement instant, oldest first; then the values behind the last chunk
};

struct rxb_args {
  const rxb_cap *caps;
  // both tables depend on the block index only: built for the longest capture of a launch, they are a prefix every shorter one reads its own part of
  const unsigned *iv_of_block;         // [blocks of 4096 samples] detect interval a block belongs to
  const unsigned *det_block;           // [n_det] block index of every detect point
  const float2 *om;                    // reverse-FFT twiddles (notch_detect.h)
  unsigned tile_chunks, warm_chunks;
  unsigned pre_block, pre_look;        // samples per pre-pass block; blocks a tile looks back
  float nk, l2omk;                     // auto_notch::k, log2(1 − k)
  rx_consts C;
  rx_tables T;
  float in_scale;                      // the converted formats (rxb_in below): scaler's factor (1: none), the 16-bit items' bias as an xor mask
  unsigned in_flip;
  // signal reports (lsdr_capture_reports_set; read by the REP tiles and k_rxb_reports only)
  const rxb_rep *rep;                  // [captures]
  unsigned rep_period;                 // cstln_receiver::meas_decimation in samples (0: no instant inside a capture, the final record only)
};


// ---- sample formats ----------------------------------------------------------------------------------------------------------------
// Every kernel that reads a capture converts in its loads: value = float(item − Z)·in_scale (cconverter<T,Z,f32,0,1,1>, dsp.h:40-50, exact;
// then scaler<float,cf32,cf32>, dsp.h:149-156, one rounding per component; in_scale = 1 is the identity).  One KIND per item size:
//   kRxbU8   cu8, no scale: the kernels of the cu8 objects, untouched (leandvb --u8, leandvb.cc:211-217)
//   kRxbS8   cs8 (--s8, leandvb.cc:218-227)
//   kRxb16   cu16 / cs16 (--u16 / --s16, leandvb.cc:228-248): the bias 32768 is the item's top bit, flipped by in_flip = 0x80008000
//   kRxbF32  cf32 (--f32 --float-scale, leandvb.cc:249-258)
// kStage is the tile kernel's LDS stage length in samples (rxb_stage).
enum { kRxbU8 = 0, kRxbS8 = 1, kRxb16 = 2, kRxbF32 = 3 };
__device__ __forceinline__ float rxb_u8f(unsigned w, int byte) {       // (float)((int)u8 − 128): flip the top bit, sign-extend
  return (float)(int)(signed char)((w ^ 0x8080u) >> (8 * byte));
}
__device__ __forceinline__ unsigned rxb_word(unsigned w) { return w; }
__device__ __forceinline__ unsigned rxb_word(const float2 &) { return 0u; }
template <int K> struct rxb_in;
template <> struct rxb_in<kRxbU8> {
  typedef unsigned item;
  static constexpr int kBytes = 2, kStage = 32, kTile0 = LSDR_IN_CU8;
  static __device__ __forceinline__ item ld(const void *p) { return *reinterpret_cast<const unsigned short *>(p); }
  static __device__ __forceinline__ float re(item w, float, unsigned) { return rxb_u8f(w, 0); }
  static __device__ __forceinline__ float im(item w, float, unsigned) { return rxb_u8f(w, 1); }
};
template <> struct rxb_in<kRxbS8> {
  typedef unsigned item;
  static constexpr int kBytes = 2, kStage = 32, kTile0 = kInS8;
  static __device__ __forceinline__ item ld(const void *p) { return *reinterpret_cast<const unsigned short *>(p); }
  static __device__ __forceinline__ float re(item w, float sc, unsigned) { return (float)(int)(signed char)w * sc; }
  static __device__ __forceinline__ float im(item w, float sc, unsigned) { return (float)(int)(signed char)(w >> 8) * sc; }
};
template <> struct rxb_in<kRxb16> {
  typedef unsigned item;
  static constexpr int kBytes = 4, kStage = 8, kTile0 = kIn16;
  static __device__ __forceinline__ item ld(const void *p) { return *reinterpret_cast<const unsigned *>(p); }
  static __device__ __forceinline__ float re(item w, float sc, unsigned flip) { return (float)(int)(short)((w ^ flip) & 0xffffu) * sc; }
  static __device__ __forceinline__ float im(item w, float sc, unsigned flip) { return (float)((int)(w ^ flip) >> 16) * sc; }
};
template <> struct rxb_in<kRxbF32> {
  typedef float2 item;
  static constexpr int kBytes = 8, kStage = 8, kTile0 = kInF32S;
  static __device__ __forceinline__ item ld(const void *p) { return *reinterpret_cast<const float2 *>(p); }
  static __device__ __forceinline__ float re(item w, float sc, unsigned) { return w.x * sc; }
  static __device__ __forceinline__ float im(item w, float sc, unsigned) { return w.y * sc; }
};

// ---- detect chain ----------------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(256) void k_rxb_detect_fft(rxb_args A) {
  typedef rxb_in<K> IN;
  const rxb_cap &cap = A.caps[blockIdx.y];
  if ((blockIdx.x >> 1) >= cap.n_det) return;
  const unsigned char *src = cap.in + (unsigned long long)IN::kBytes * kDetN * A.det_block[blockIdx.x >> 1];
  if constexpr (K == kRxbU8)
    cfft_half_body_t([&](unsigned i) { const uchar2 v = reinterpret_cast<const uchar2 *>(src)[i]; return cu8_to_cf32(v.x, v.y); }, A.om, cap.halves,
                     blockIdx.x);
  else {
    const float sc = A.in_scale; const unsigned flip = A.in_flip;
    cfft_half_body_t([&](unsigned i) { const typename IN::item w = IN::ld(src + (size_t)IN::kBytes * i); return make_float2(IN::re(w, sc, flip), IN::im(w, sc, flip)); },
                     A.om, cap.halves, blockIdx.x);
  }
}
__global__ __launch_bounds__(256) void k_rxb_detect_peaks(rxb_args A) {
  const rxb_cap &cap = A.caps[blockIdx.y];
  if (blockIdx.x >= cap.n_det) return;
  notch_peaks_body(cap.halves, A.om, (float)(1.0 / kDetN), 1, cap.cand, blockIdx.x);
}
// (1−k)^m·exp(j2π·bin·m/4096): exact angle reduction in integers, the magnitude through exp2
__device__ __forceinline__ float2 rxb_ppow(int bin, float l2omk, unsigned m) {
  const float mag = __builtin_exp2f(l2omk * (float)m);
  const float rev = (float)(((unsigned)bin * m) & 4095u) * (1.0f / 4096.0f);
  return make_float2(mag * __builtin_amdgcn_cosf(rev), mag * __builtin_amdgcn_sinf(rev));
}
// one thread per capture: the detect intervals' notch parameters (sdr.h:94-103: a slot restarts only when its bin changes)
__global__ __launch_bounds__(64) void k_rxb_iv(rxb_args A, unsigned n_caps) {
  const unsigned c = blockIdx.x * 64u + threadIdx.x;
  if (c >= n_caps) return;
  const rxb_cap &cap = A.caps[c];
  rxb_iv v; v.pr = v.pi = v.k = 0.f; v.seg_block = 0; v.bin = -1; v.pad0 = v.pad1 = v.pad2 = 0;
  cap.iv[0] = v;
  int bin_prev = -1;
  for (unsigned q = 0; q < cap.n_det; ++q) {
    const int bin = cap.cand[q * kDetMaxSlots];
    if (bin != bin_prev) v.seg_block = (int)(A.det_block[q] * (kDetN / A.pre_block));
    const double a = 2.0 * M_PI * (double)bin / kDetN, omk = 1.0 - (double)A.nk;
    v.pr = (float)(omk * cos(a)); v.pi = (float)(omk * sin(a)); v.k = A.nk; v.bin = bin;
    cap.iv[q + 1] = v;
    bin_prev = bin;
  }
}

// ---- estimator pre-pass ------------------------------------------------------------------------------------------------------------
// T[b] = Σ_{i in block b} k·p^(end−1−i)·(x[i]−128): what S is right behind block b if it was 0 in front of it.  One workgroup of 256 per
// block, 16 consecutive samples per thread (Horner), the threads' partial sums weighted by p^(16·(255−t)) and added up.
template <int K>
__global__ __launch_bounds__(256) void k_rxb_notch_pre(rxb_args A) {
  typedef rxb_in<K> IN;
  const rxb_cap &cap = A.caps[blockIdx.y];
  const unsigned PB = A.pre_block, per = PB / 256u;
  const unsigned long long pos = (unsigned long long)blockIdx.x * PB;
  if (pos + PB > cap.total_chunks * kChunk + 1) return;           // (only blocks in front of a tile start are ever read)
  const rxb_iv v = cap.iv[A.iv_of_block[pos >> 12]];
  __shared__ float2 red[4];
  float2 acc = make_float2(0.f, 0.f);
  if (v.k != 0.f) {
    const unsigned char *src = cap.in + IN::kBytes * (pos + (unsigned long long)threadIdx.x * per);
    if constexpr (K == kRxbU8) {
    for (unsigned i = 0; i < per; i += 8) {
      const uint4 w = *reinterpret_cast<const uint4 *>(src + 2 * i);   // 8 samples (a capture buffer is 16-byte aligned, blocks are multiples of 1024 samples)
      const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const unsigned s = ws[q] >> (16 * h);
          const float xr = (float)((int)(s & 255u) - 128), xi = (float)((int)((s >> 8) & 255u) - 128);
          const float nr = __builtin_fmaf(v.pr, acc.x, __builtin_fmaf(-v.pi, acc.y, v.k * xr));
          const float ni = __builtin_fmaf(v.pr, acc.y, __builtin_fmaf(v.pi, acc.x, v.k * xi));
          acc.x = nr; acc.y = ni;
        }
      }
    }
    } else {
      // the converted formats: 16 bytes per load as well (8, 4 or 2 samples), the items picked out of the four dwords
      constexpr unsigned kPer = 16u / (unsigned)IN::kBytes;
      const float sc = A.in_scale; const unsigned flip = A.in_flip;
      for (unsigned i = 0; i < per; i += kPer) {
        const uint4 w = *reinterpret_cast<const uint4 *>(src + IN::kBytes * i);
        const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (unsigned q = 0; q < kPer; ++q) {
          typename IN::item it;
          if constexpr (K == kRxbS8) it = ws[q >> 1] >> (16 * (q & 1u));
          else if constexpr (K == kRxb16) it = ws[q];
          else it = make_float2(__uint_as_float(ws[2 * q]), __uint_as_float(ws[2 * q + 1]));
          const float xr = IN::re(it, sc, flip), xi = IN::im(it, sc, flip);
          const float nr = __builtin_fmaf(v.pr, acc.x, __builtin_fmaf(-v.pi, acc.y, v.k * xr));
          const float ni = __builtin_fmaf(v.pr, acc.y, __builtin_fmaf(v.pi, acc.x, v.k * xi));
          acc.x = nr; acc.y = ni;
        }
      }
    }
    const float2 wgt = rxb_ppow(v.bin, A.l2omk, per * (255u - threadIdx.x));     // this thread's span ends that many samples in front of the block end
    acc = make_float2(acc.x * wgt.x - acc.y * wgt.y, acc.x * wgt.y + acc.y * wgt.x);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { acc.x += __shfl_xor(acc.x, d, 64); acc.y += __shfl_xor(acc.y, d, 64); }
  if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    cap.T[blockIdx.x] = make_float2(red[0].x + red[1].x + red[2].x + red[3].x, red[0].y + red[1].y + red[2].y + red[3].y);
}

// ---- tiles -------------------------------------------------------------------------------------------------------------------------
// a value every lane of the wavefront has, moved into a scalar register
__device__ __forceinline__ float rxb_uniform(float v) { return __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint(v))); }
// atan(u)·65536/2π for |u| ≤ 1, odd polynomial (max error 2e-6 rad = 0.02 table units)
__host__ __device__ __forceinline__ float rxb_atan_units(float u) {
  const float S = 10430.3784f;
  const float u2 = u * u;
  float p = -0.0117212f * S;
  p = __builtin_fmaf(p, u2, 0.05265332f * S);
  p = __builtin_fmaf(p, u2, -0.11643287f * S);
  p = __builtin_fmaf(p, u2, 0.19354346f * S);
  p = __builtin_fmaf(p, u2, -0.33262347f * S);
  p = __builtin_fmaf(p, u2, 0.99997726f * S);
  return p * u;
}
// the table's phase_error for the truncated coordinates (Ii, Qi), as a float (an integer value): sdr.h:548-556 for QPSK
__host__ __device__ __forceinline__ float rxb_phase_error(int Ii, int Qi) {
  const float a = __builtin_fabsf((float)Ii) + 1e-6f, b = __builtin_fabsf((float)Qi);   // (+1e-6: (0,0) gives u = −1, the table's atan2f(0,0) = 0)
#ifdef __HIP_DEVICE_COMPILE__
  const float u = (b - a) * __builtin_amdgcn_rcpf(b + a);
#else
  const float u = (b - a) / (b + a);
#endif
  const float at = rxb_atan_units(u);
  unsigned bits;
  __builtin_memcpy(&bits, &at, 4);
  bits ^= (unsigned)(Ii ^ Qi) & 0x80000000u;              // −pe where exactly one coordinate is negative
  float pe;
  __builtin_memcpy(&pe, &bits, 4);
  return __builtin_truncf(pe);                            // the table's (s32) cast
}

// ---- the notch's state for a lane that starts at sample `ws` (a multiple of pre_block) of its capture ----------------------------------
struct rxb_notch { float pr, pi, k, sr, si; unsigned ivm; };
__device__ __forceinline__ rxb_notch rxb_notch_start(const rxb_args &A, const rxb_cap &cap, unsigned long long ws) {
  rxb_notch N; N.pr = N.pi = N.k = N.sr = N.si = 0.f;
  N.ivm = A.iv_of_block[ws >> 12];
  const rxb_iv v = cap.iv[N.ivm];
  N.pr = v.pr; N.pi = v.pi; N.k = v.k;
  if (N.k != 0.f) {
    const long long b = (long long)(ws / A.pre_block);
    const float2 ppb = rxb_ppow(v.bin, A.l2omk, A.pre_block);             // p^pre_block
    for (int q = (int)A.pre_look - 1; q >= 0; --q) {
      const long long idx = b - 1 - q;
      if (idx < (long long)v.seg_block || idx < 0) continue;
      const float2 t = cap.T[idx];
      const float nr = N.sr * ppb.x - N.si * ppb.y + t.x, ni = N.sr * ppb.y + N.si * ppb.x + t.y;
      N.sr = nr; N.si = ni;
    }
  }
  return N;
}
// … at the first sample `pos` of a 4096-sample block: a detect point may start another interval there (sdr.h:64-75, 94-103)
__device__ __forceinline__ void rxb_notch_block(const rxb_args &A, const rxb_cap &cap, unsigned long long pos, rxb_notch &N) {
  const unsigned m = A.iv_of_block[pos >> 12];
  if (m == N.ivm) return;
  const rxb_iv v = cap.iv[m];
  if ((unsigned long long)v.seg_block * A.pre_block == pos) { N.sr = 0.f; N.si = 0.f; }     // the bin changed: the estimator restarts (sdr.h:99-101)
  N.pr = v.pr; N.pi = v.pi; N.k = v.k; N.ivm = m;
}
// S[n] = p·S[n−1] + k·x[n]
__device__ __forceinline__ void rxb_notch_step(float pr, float pi, float k, float sr, float si, float xr, float xi, float &tr, float &ti) {
  tr = __builtin_fmaf(pr, sr, __builtin_fmaf(-pi, si, k * xr));
  ti = __builtin_fmaf(pr, si, __builtin_fmaf(pi, sr, k * xi));
}
// Test kernel (lsdr_capture_batch_notched): the notched stream the tiles see, written out — one LANE per pre_block samples, the same
// start state, interval switches and recurrence as rxb_tile.
template <int K>
__global__ __launch_bounds__(64) void k_rxb_notch_dump(rxb_args A, unsigned cap_index, unsigned long long n_samples, float2 *out) {
  const rxb_cap &cap = A.caps[cap_index];
  const unsigned long long seg = (unsigned long long)blockIdx.x * 64u + threadIdx.x, ws = seg * A.pre_block;
  if (ws >= n_samples) return;
  rxb_notch N = rxb_notch_start(A, cap, ws);
  for (unsigned long long i = ws; i < ws + A.pre_block && i < n_samples; ++i) {
    if ((i & 4095ull) == 0) rxb_notch_block(A, cap, i, N);
    const typename rxb_in<K>::item w = rxb_in<K>::ld(cap.in + (unsigned long long)rxb_in<K>::kBytes * i);
    const float xr = rxb_in<K>::re(w, A.in_scale, A.in_flip), xi = rxb_in<K>::im(w, A.in_scale, A.in_flip);
    float tr, ti;
    rxb_notch_step(N.pr, N.pi, N.k, N.sr, N.si, xr, xi, tr, ti);
    N.sr = tr; N.si = ti;
    out[i] = make_float2(xr - tr, xi - ti);
  }
}

// The table's cost for the truncated coordinates (qpsk_decide's integer arithmetic, cstln_receiver.hip: nearest point by the signs, second
// nearest = flip the coordinate of smaller magnitude: d1 − min(d1 + 4·53·min(|I|,|Q|), 32767)) and the decision `sym`, as the 32 bits of an
// lsdr_softsymbol {int16 cost; uint8 symbol; uint8 pad = 0}.  |I|, |Q| ≤ 128: every product fits 24 bits.
__device__ __forceinline__ unsigned rxb_soft_word(int Ii, int Qi, unsigned sym) {
  const int a = Ii < 0 ? -Ii : Ii, b = Qi < 0 ? -Qi : Qi;
  const int da = a - 53, db = b - 53;
  const int d1 = __mul24(da, da) + __mul24(db, db);
  const int d2 = d1 + __mul24(212, a < b ? a : b);
  const int cost = d1 - (d2 > 32767 ? 32767 : d2);
  return ((unsigned)cost & 0xffffu) | (sym << 16);
}

// LDS staging of the lean tiles: 32 samples per stage + 16 of look-ahead (the next symbol's pair is read up to 3 samples ahead, a timing
// excursion walks up to omega + 2 ≤ 10): 112-byte rows, 7 KiB per wavefront — 22 wavefronts per CU where the 64-sample stages of
// rx_tile_tol (11 KiB) allow 14; this kernel lives on wavefronts per SIMD (VALU issue, a dependent chain per symbol).
// The wider items keep that row: 8-sample stages of 4-byte items are the same 112 bytes (cu16 / cs16: 7 KiB per wavefront, the cu8
// occupancy), of 8-byte items 208 bytes (cf32: 13 KiB per wavefront, 12 wavefronts per CU) — the look-ahead margin is what a row is made
// of, and it does not shrink with the stage.
constexpr float kSigPowerQpsk = 5618.0f;        // 53² + 53²: sig_power of every QPSK point (sdr.h:873-889)
template <int K> struct rxb_stage {
  static constexpr int kStage = rxb_in<K>::kStage, kMargin = 16, kRowBytes = rxb_in<K>::kBytes * (kStage + kMargin) + 16;
  static_assert(kRowBytes % 16 == 0 && kChunk % kStage == 0, "stage geometry");
};
static_assert(rxb_stage<kRxbU8>::kRowBytes == 112 && rxb_stage<kRxbS8>::kRowBytes == 112 && rxb_stage<kRxb16>::kRowBytes == 112 &&
              rxb_stage<kRxbF32>::kRowBytes == 208, "stage geometry");

// REP (signal reports, rxb_rep): per body chunk the estimator inputs of sdr.h:866-889 folded into the tile's map, and a slot where a
// measurement instant falls into the chunk.  insp does not depend on the gain and sig_power is 53² + 53²; ev_power = |s − c|² of the
// chunk's last symbol does: it is taken at the serial gain the soft tiles estimate (`pavg` / `crat` below, which the REP tiles of the
// default engine carry too), not at the tile's own, which starts from the constructed AGC.
template <bool NOTCH, bool SOFT, int K, bool REP = false>
__device__ __forceinline__ void rxb_tile(const rxb_args &A, const rxb_cap &cap, unsigned j0, int lane, char *lds) {
  constexpr bool GAIN = SOFT || REP;                                       // the second power estimator runs
  typedef rxb_stage<K> ST;
  typedef rxb_in<K> IN;
  typedef typename IN::item item_t;
  constexpr int kB = IN::kBytes;                                           // bytes per item
  const float isc = A.in_scale; const unsigned iflip = A.in_flip;          // (kRxbU8 reads neither)
  // (kRxbU8 calls rxb_u8f where it always did: through rxb_in the compiler flips the sign bit per byte, behind the sign extension — four
  // more instructions per symbol)
#define RXB_RE(w) (K == kRxbU8 ? rxb_u8f(rxb_word(w), 0) : IN::re(w, isc, iflip))
#define RXB_IM(w) (K == kRxbU8 ? rxb_u8f(rxb_word(w), 1) : IN::im(w, isc, iflip))
  constexpr int kStage = ST::kStage, kRowBytes = ST::kRowBytes, kStageLoads = ST::kRowBytes / 16;
  const bool valid = j0 + (unsigned)lane < cap.n_tiles;
  const unsigned j = valid ? j0 + (unsigned)lane : j0;
  const unsigned Lc = A.tile_chunks, Wc = A.warm_chunks;
  const unsigned long long cb = (unsigned long long)(j - 1) * Lc;          // first warm-up chunk; the body starts at chunk cb + Wc
  unsigned long long c1 = cb + Wc + Lc;
  if (c1 > cap.total_chunks) c1 = cap.total_chunks;
  const int nwarm = (int)Wc, nchunks = valid ? (int)(c1 - cb) : 0;
  const int wave_chunks = (int)(Wc + Lc);

  // LDS staging (rx_tile_tol's scheme): one row per lane, kStageLoads buffer→LDS loads of 1 KiB per 64-sample stage
  const unsigned long long addr = (unsigned long long)cap.in;
  const int delta = (int)(addr & 15ull);
  const unsigned long long cb0 = (unsigned long long)(j0 - 1) * Lc;         // first tile of the wavefront
  const unsigned long long bytes = ((cap.total_chunks * kChunk + 1ull) * (unsigned long long)kB + (unsigned)delta + 15ull) & ~15ull;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char *>(cap.in) - delta, 0,
                                                                         (int)(bytes > 0xffffffffull ? 0xffffffffu : (unsigned)bytes), 0x00020000);
  unsigned src_off[kStageLoads];
#pragma unroll
  for (int q = 0; q < kStageLoads; ++q) {
    const unsigned f = (unsigned)q * 1024u + (unsigned)lane * 16u, r = f / (unsigned)kRowBytes, col = f - r * (unsigned)kRowBytes;
    const unsigned long long tile_byte = (cb0 + (unsigned long long)r * Lc) * (unsigned long long)(kChunk * kB);
    src_off[q] = (j0 + r < cap.n_tiles && tile_byte + col < 0xfff00000ull) ? (unsigned)(tile_byte + col) : 0xfffffff0u;
  }
  const char *const row = lds + lane * kRowBytes + delta;                   // sample s0 of the stage in flight sits here

  const rx_consts &C = A.C;
  // the capture's constructed state, read once through the pointer in its record and held in scalar registers (the same for every lane)
  const rx_state_dev *S0 = cap.state0;
  const float s0_freqw = rxb_uniform(S0->freqw), s0_insp = rxb_uniform(S0->est_insp), s0_mu = rxb_uniform(S0->mu);
  float freqw = s0_freqw, agc = rxb_uniform(S0->agc_gain), est_insp = s0_insp;
  const float min_f = rxb_uniform(S0->min_freqw), max_f = rxb_uniform(S0->max_freqw);
  float fwin = 65536.0f / C.omega / 2048.0f;
  if (fwin < 8.f) fwin = 8.f;
  const float f_lo = freqw - fwin, f_hi = freqw + fwin;
  const float kk = C.kest, k1 = 1 - C.kest;
  const float freq_alpha = C.freq_alpha, freq_beta = C.freq_beta, gain_mu = C.gain_mu, omega = C.omega;
  // symbol timing at the tile's first sample, predicted from the capture's first sample (mu = 0 there) at the nominal omega: see rx_tile_tol
  float mu = 0.f, phase = 0.f;
  {
    const double ws = (double)cb * kChunk - (double)s0_mu, om = (double)C.omega;
    const double r = ws - om * __builtin_floor(ws / om);
    mu = (float)(r > 0.0 ? om - r : 0.0);
    if (!(mu >= 0.f && mu < C.omega)) mu = 0.f;
  }
  float h1pr = 0.f, h1pi = 0.f, h1cr = 0.f, h1ci = 0.f, mmA = 0.f, mmB = 0.f;      // Mueller & Müller: the previous symbol; p1·c2 and c1·p2

  // notch: pole / gain of the interval the tile is in, S in front of the tile's first sample from the pre-pass sums
  float npr = 0.f, npi = 0.f, nkk = 0.f, sr = 0.f, si = 0.f;
  rxb_notch NS; NS.pr = NS.pi = NS.k = NS.sr = NS.si = 0.f; NS.ivm = 0;
  if (NOTCH && valid) {
    NS = rxb_notch_start(A, cap, cb * kChunk);
    npr = NS.pr; npi = NS.pi; nkk = NS.k; sr = NS.sr; si = NS.si;
  }

  unsigned hacc = 0, hcnt = 0, hwarm = 0, hnwarm = 0, got = 0;
  unsigned *const hcol = cap.hstage + j;
  // SOFT: body symbol k goes to byte 4·(k·hpitch + j) of sstage (one row of `hpitch` dwords per symbol step: the 64 lanes of the wavefront
  // are 64 consecutive tiles and write 64 consecutive dwords; a capture's staging is below 4 GiB, so k and 4·hpitch fit 24 bits:
  // lsdr_rxb_create_in)
  const unsigned srow = 4u * (unsigned)cap.hpitch;
  // SOFT: the amplitude the COSTS are taken at.  A cost is proportional to the sampled point's amplitude, so the soft records need the
  // gain the serial receiver has at this tile — its power estimate is an average over the last hundred chunks (kest = 0.01 per chunk,
  // sdr.h:867-870), which a warm-up of a few chunks cannot reproduce from the constructed state (the tile's own gain stays some per cent
  // off for its whole length: harmless for signs, a bias on every cost).  The estimator's input, |interpolated sample|², does not depend
  // on the gain: the tile averages it over the warm-up's symbols (`pavg`, a running mean of weight 1/128 per symbol: ≈ the last 250
  // symbols, the timing loop has settled by then) and starts, at the body's first sample, a second estimator from the EXPECTED serial
  // value after cb + Wc chunks, mean + (1 − kest)^(cb+Wc)·(constructed − mean), updated per chunk like the first (`pavg` again).  The
  // record's coordinates are the sampled point times crat = gain(second) / gain(first), folded and truncated like the table's index.
  // The LOOPS keep the first gain, so timing, carrier and the seam records are those of the packed tiles (whose sensitivity is measured,
  // DESIGN §4.5): run at the second gain they slipped a symbol at noise 20 where the reference does not.
  float pavg = est_insp, crat = 1.0f;
  auto soft_gain = [&](float est2) { crat = (est2 > 0.f) ? __builtin_sqrtf(est_insp * __builtin_amdgcn_rcpf(est2)) : 1.0f; };
  auto soft_record = [&](float svr, float svi) {
    float Is = svr * crat, Qs = svi * crat;
    if (__builtin_fmaxf(__builtin_fabsf(Is), __builtin_fabsf(Qs)) > 127.0f) lut_halve(Is, Qs);
    const int Ic = (int)Is, Qc = (int)Qs;
    return rxb_soft_word(Ic, Qc, (((unsigned)Ic >> 31) << 1) | ((unsigned)Qc >> 31));
  };
  // REP: the body's map est ↦ ma·est + b (the b of est_sp is 5618·(1 − ma): its input is constant); the measurement counter of
  // sdr.h:905-913 at the body's first chunk (meas_count = 0 at the capture's first sample) and the slot the next instant fills
  float ma = 1.f, mbi = 0.f, mbe = 0.f;
  unsigned mcount = 0, mslot = 0;
  if (REP && A.rep_period) {
    const unsigned long long pos = (cb + Wc) * (unsigned long long)kChunk, q = pos / A.rep_period;
    mslot = (unsigned)q; mcount = (unsigned)(pos - q * A.rep_period);
  }
  float mu_begin = 0.f, phase_begin = 0.f;
  int n = 0;                                     // sample of the next symbol (tile-relative)
  item_t x0w = item_t(), x1w = item_t();         // the items of samples n and n + 1
  bool fetched = false;

  for (int ci = 0; ci < wave_chunks; ++ci) {
    const bool active = ci < nchunks;
    const bool body = ci >= nwarm;
    if (active && ci == nwarm) {
      // the loop state AT the body's first sample (rx_tiling.h compares it with the previous tile's at the same sample): the next symbol
      // instant is n, `over` samples into the body
      const float over = (float)(n - ci * kChunk);
      mu_begin = mu + over; phase_begin = phase - over * freqw;
      got = hcnt; hwarm = hacc; hnwarm = hcnt < 16u ? hcnt : 16u; hcnt = 0;
      if (GAIN && got) {
        pavg = __builtin_fmaf(__builtin_exp2f((float)(cb + Wc) * __builtin_log2f(k1)), s0_insp - pavg, pavg);
        soft_gain(pavg);
      }
    }
    // sampler->update_freq(freqw), sdr.h:790: the partner sample's extra rotation e^{−j·freqw}, constant over the chunk
    const float frev = freqw * (-1.0f / 65536.0f);
    const float cf = __builtin_amdgcn_cosf(frev), sf = __builtin_amdgcn_sinf(frev);
    if (NOTCH && active) {                       // a detect point is the start of a 4096-sample block
      const unsigned long long pos = (cb + (unsigned long long)ci) * kChunk;
      if ((pos & 4095ull) == 0) {
        NS.sr = sr; NS.si = si;
        rxb_notch_block(A, cap, pos, NS);
        npr = NS.pr; npi = NS.pi; nkk = NS.k; sr = NS.sr; si = NS.si;
      }
    }
    const unsigned cnt0 = hcnt;
    const bool wlast = ci + 1 == nwarm;           // (SOFT: the last warm-up chunk; its symbols at the gain estimated so far)
    if (SOFT && active && wlast) soft_gain(__builtin_fmaf(__builtin_exp2f((float)(cb + Wc) * __builtin_log2f(k1)), s0_insp - pavg, pavg));
    float g0r = 0.f, g0i = 0.f;                  // last interpolated sample of the chunk, before derotation (|.|² feeds the AGC)
#pragma unroll 1
    for (int sb = 0; sb < kChunk / kStage; ++sb) {
      const int s0 = ci * kChunk + sb * kStage, send = s0 + kStage;
      {
        const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(s0 * kB);
#pragma unroll
        for (int q = 0; q < kStageLoads; ++q)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (rx_lds_ptr)(size_t)(unsigned)(unsigned long long)(lds + q * 1024), 16, src_off[q], soff, 0, 0);
#ifndef RXB_NOWAIT                                // (measurement variant: what the stage wait costs; garbage results)
        __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): the stage has landed (single-wave workgroup: no barrier)
#endif
        asm volatile("" ::: "memory");
      }
      const char *ap = row + kB * (n - s0);      // sample n in this lane's row
      if (active && !fetched) {
        x0w = IN::ld(ap); x1w = IN::ld(ap + kB);
        fetched = true;
      }
      auto symbol = [&](auto body_tag) {
        constexpr bool BODY = decltype(body_tag)::value;
        const float x0r = RXB_RE(x0w), x0i = RXB_IM(x0w), x1r = RXB_RE(x1w), x1i = RXB_IM(x1w);
        // the items two and three samples on: the next symbol's pair is (x1, r2) or (r2, r3)
        const item_t r2 = IN::ld(ap + 2 * kB), r3 = IN::ld(ap + 3 * kB);
        float o0r = x0r, o0i = x0i, o1r = x1r, o1i = x1i, t0r = 0.f, t0i = 0.f, t1r = 0.f, t1i = 0.f;
        if (NOTCH) {
          rxb_notch_step(npr, npi, nkk, sr, si, x0r, x0i, t0r, t0i);
          rxb_notch_step(npr, npi, nkk, t0r, t0i, x1r, x1i, t1r, t1i);
          o0r = x0r - t0r; o0i = x0i - t0i; o1r = x1r - t1r; o1i = x1i - t1i;
        }
        // linear_sampler::interp (sdr.h:614-623), one derotation
        const float q1r = __builtin_fmaf(o1r, cf, -(o1i * sf)), q1i = __builtin_fmaf(o1r, sf, o1i * cf);
        g0r = __builtin_fmaf(mu, q1r - o0r, o0r); g0i = __builtin_fmaf(mu, q1i - o0i, o0i);
        if (GAIN && !BODY) pavg = __builtin_fmaf(__builtin_fmaf(g0r, g0r, __builtin_fmaf(g0i, g0i, -pavg)), 1.0f / 128.0f, pavg);
        const float prev = phase * (-1.0f / 65536.0f);
        const float ear = __builtin_amdgcn_cosf(prev) * agc, eai = __builtin_amdgcn_sinf(prev) * agc;
        const float svr = __builtin_fmaf(g0r, ear, -(g0i * eai)), svi = __builtin_fmaf(g0r, eai, g0i * ear);
        // cstln_lut<256>::lookup (sdr.h:470-483): fold into range, truncate; the decision is the two sign bits
        float Ir = svr, Qr = svi;
        if (__builtin_fmaxf(__builtin_fabsf(svr), __builtin_fabsf(svi)) > 127.0f) lut_halve(Ir, Qr);     // (the exact test is lut_halve's own)
        const int Ii = (int)Ir, Qi = (int)Qr;
        hacc = __builtin_amdgcn_alignbit(hacc, (unsigned)Ii, 31);
        hacc = __builtin_amdgcn_alignbit(hacc, (unsigned)Qi, 31);
        const float pe = rxb_phase_error(Ii, Qi);
        phase = __builtin_fmaf(pe, freq_alpha, phase);                       // sdr.h:814-815
        freqw = __builtin_fmaf(pe, freq_beta, freqw);
        freqw = __builtin_amdgcn_fmed3f(freqw, f_lo, f_hi);
        // constellation point (±53, ±53) by the sign bits; modified Mueller & Müller, sdr.h:822-840
        float c0r, c0i;
        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(c0r) : "s"(0x80000000u), "v"(Ii), "v"(0x42540000u));      // 53.0 with the coordinate's sign
        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(c0i) : "s"(0x80000000u), "v"(Qi), "v"(0x42540000u));
        // muerr = (p0 − p2)·c1 − (c0 − c2)·p1 (dot products) = A0 − B1 − B0 + A1 with A_k = p_k·c_{k−1}, B_k = c_k·p_{k−1}: the symbol before
        // the previous one enters through two running products, not through four more history registers
        const float A0 = __builtin_fmaf(svi, h1ci, svr * h1cr), B0 = __builtin_fmaf(c0i, h1pi, c0r * h1pr);
        const float muerr = (A0 - mmB) + (mmA - B0);
        const float mucorr = __builtin_amdgcn_fmed3f(muerr * gain_mu, -0.1f, 0.1f);
        mmA = A0; mmB = B0;
        h1pr = svr; h1pi = svi; h1cr = c0r; h1ci = c0i;
        const float mu2 = (mu + mucorr) + omega;
        // the sample steps up to the next symbol instant: at least one (sdr.h:800-847: one symbol per sample step at most)
        const float kf = __builtin_amdgcn_fmed3f(__builtin_floorf(mu2), 1.0f, 1024.0f);
        const int ki = (int)kf;
        mu = mu2 - kf;
        phase = __builtin_fmaf(kf, freqw, phase);
        ++hcnt;
        if (SOFT) {
          if (BODY) *reinterpret_cast<unsigned *>(reinterpret_cast<char *>(cap.sstage) + (__umul24(hcnt - 1u, srow) + 4u * j)) = soft_record(svr, svi);
          else if (wlast) cap.spre[j] = soft_record(svr, svi);                 // (the last one written is the warm-up's last symbol)
        } else if (BODY) { if ((hcnt & 15u) == 0) hcol[(unsigned long long)((hcnt >> 4) - 1) * cap.hpitch] = hacc; }
        const bool one = ki == 1;
        x0w = one ? x1w : r2; x1w = one ? r2 : r3;
        if (NOTCH) { sr = one ? t0r : t1r; si = one ? t0i : t1i; }
        if (ki > 2) {                             // (omega > 2, or a timing excursion): walk the samples in between
          for (int i = 2; i < ki; ++i) {
            const item_t w = IN::ld(ap + kB * i);
            if (NOTCH) {
              const float xr = RXB_RE(w), xi = RXB_IM(w);
              float nr, ni;
              rxb_notch_step(npr, npi, nkk, sr, si, xr, xi, nr, ni);
              sr = nr; si = ni;
            }
          }
          x0w = IN::ld(ap + kB * ki); x1w = IN::ld(ap + kB * ki + kB);
        }
        n += ki; ap += kB * ki;
      };
      if (body) { while (active && n < send) symbol(std::true_type()); }
      else { while (active && n < send) symbol(std::false_type()); }
    }
    if (active) {
      phase = fmod65536(phase);                                              // sdr.h:855
      if (hcnt != cnt0) {                                                    // the chunk had a symbol: sdr.h:867-870
        const float insp = g0r * g0r + g0i * g0i;
        est_insp = __builtin_fmaf(insp, kk, est_insp * k1);
        if (est_insp) agc = kCstlnAmp / __builtin_sqrtf(est_insp);
        if (REP && body) {                                                   // sdr.h:873-889: the chunk's last symbol, at the gain it was sampled with
          const float evr = __builtin_fmaf(h1pr, crat, -h1cr), evi = __builtin_fmaf(h1pi, crat, -h1ci);
          ma *= k1;
          mbi = __builtin_fmaf(insp, kk, mbi * k1);
          mbe = __builtin_fmaf(__builtin_fmaf(evr, evr, evi * evi), kk, mbe * k1);
        }
        if (GAIN && body) { pavg = __builtin_fmaf(insp, kk, pavg * k1); soft_gain(pavg); }
      }
      if (!C.allow_drift) {                                                  // sdr.h:895-898
        if (freqw < min_f || freqw > max_f) freqw = (max_f + min_f) / 2;
      }
      if (REP && body && A.rep_period) {                                     // sdr.h:905-913 (a period is at least a chunk: one instant at most)
        mcount += (unsigned)kChunk;
        if (mcount >= A.rep_period) {
          mcount -= A.rep_period;
          rx_meas mm; mm.freqw = freqw; mm.a = ma; mm.est_insp = mbi; mm.est_sp = kSigPowerQpsk * (1.0f - ma); mm.est_ep = mbe; mm.tile = j;
          A.rep[blockIdx.y].slot[mslot++] = mm;
        }
      }
    }
  }
  if (valid) {
    if (nchunks <= nwarm) { mu_begin = mu; phase_begin = phase; got = hcnt; hwarm = hacc; hnwarm = hcnt < 16u ? hcnt : 16u; hcnt = 0; }   // (never: a tile has a body)
    const float over_end = (float)(n - nchunks * kChunk);     // … and AT the sample behind the tile's last one
    mu += over_end; phase -= over_end * freqw;
    if (!SOFT && (hcnt & 15u)) hcol[(unsigned long long)(hcnt >> 4) * cap.hpitch] = hacc << (2 * (16 - (hcnt & 15u)));
    rx_tile_info_h th;
    th.mu_begin = mu_begin; th.phase_begin = phase_begin; th.mu_end = mu; th.phase_end = phase;
    th.count = hcnt; th.has_pre = got ? 1u : 0u; th.n_warm = hnwarm; th.warm_tail = hwarm; th.body_tail = hacc;
    cap.hinfo[j] = th;
    if (j == cap.n_tiles - 1) { cap.state_end->phase = phase; cap.state_end->freqw = freqw; }
    if (REP) { rx_ema_map m; m.a = ma; m.bi = mbi; m.bs = kSigPowerQpsk * (1.0f - ma); m.be = mbe; A.rep[blockIdx.y].map[j] = m; }
  }
#undef RXB_RE
#undef RXB_IM
}

template <bool NOTCH, bool SOFT, int K, bool REP = false>
__device__ __forceinline__ void rxb_tiles_body(const rxb_args &A) {
  __shared__ __attribute__((aligned(16))) char lds[64 * rxb_stage<K>::kRowBytes];
  const rxb_cap &cap = A.caps[blockIdx.y];
  if (blockIdx.x == 0) {
    // tile 0: the reference's arithmetic from the constructed state over the first warm_chunks chunks (in front of the first detect
    // point the notch passes its input through: SURVEY A7)
    if (threadIdx.x == 0 && cap.n_tiles) {
      rx_tiled_args a;
      a.in = cap.in; a.total_chunks = cap.total_chunks; a.first_chunks = A.warm_chunks; a.tile_chunks = A.tile_chunks; a.warm_chunks = A.warm_chunks;
      a.n_tiles = cap.n_tiles; a.lanes_per_wave = 64; a.dbg = 0; a.stage_stride = 0; a.stage = nullptr; a.wstage = nullptr; a.wstride = 0;
      a.info = nullptr; a.hstage = cap.hstage; a.hpitch = cap.hpitch; a.hinfo = cap.hinfo; a.ema = cap.ema_scratch; a.ema_wave = cap.ema_scratch + 1;
      if (SOFT) a.stage = reinterpret_cast<lsdr_softsymbol *>(cap.sstage);
      a.state = cap.state0; a.state_next = cap.state_end; a.meas = nullptr; a.meas_base = 0; a.cstln = nullptr; a.C = A.C; a.T = A.T;
      if (REP) {                                 // tile 0 owns chunks [0, warm_chunks): its slots and its (constant) map hold exact values
        a.ema_wave = A.rep[blockIdx.y].map;
        if (A.rep_period) { a.meas = A.rep[blockIdx.y].slot; a.C.meas_decimation = A.rep_period; }
      }
      rx_tile_exact<1, rxb_in<K>::kTile0, true, SOFT>(a, A.in_scale, A.in_flip);
    }
    return;
  }
  const unsigned j0 = 1u + (blockIdx.x - 1u) * 64u;
  if (j0 >= cap.n_tiles) return;
  rxb_tile<NOTCH, SOFT, K, REP>(A, cap, j0, (int)threadIdx.x, lds);
}
template <bool NOTCH>
__global__ __launch_bounds__(64) void k_rxb_tiles(rxb_args A) { rxb_tiles_body<NOTCH, false, kRxbU8>(A); }
// the soft tiles: held to the packed tiles' five waves per SIMD (the notch variant's live values come to one register more)
template <bool NOTCH>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) void k_rxb_tiles_soft(rxb_args A) { rxb_tiles_body<NOTCH, true, kRxbU8>(A); }
// the converted formats (cu8 objects never run these): packed and soft tiles of kind K
template <bool NOTCH, bool SOFT, int K>
__global__ __launch_bounds__(64) void k_rxb_tiles_in(rxb_args A) { rxb_tiles_body<NOTCH, SOFT, K>(A); }
// … the soft tiles of the 2- and 4-byte items: held to five waves per SIMD like k_rxb_tiles_soft (same 7 KiB of LDS; one register over otherwise)
template <bool NOTCH, int K>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) void k_rxb_tiles_in_soft5(rxb_args A) { rxb_tiles_body<NOTCH, true, K>(A); }

// the tiles with signal reports (rxb_rep), every kind: objects that have not asked for reports never run these
template <bool NOTCH, bool SOFT, int K>
__global__ __launch_bounds__(64) void k_rxb_tiles_rep(rxb_args A) { rxb_tiles_body<NOTCH, SOFT, K, true>(A); }

// Scan of a capture's tile maps, one workgroup per capture (blockIdx.x), behind the tiles: rx_ema_body's scheme.  Thread t composes its
// run of consecutive tiles, the runs are scanned across the workgroup, and every thread walks its tiles again from the values in front of
// them — from the constructed estimators for tile 0 — leaving those values in map[] and, behind the last tile, the final record
// slot[n_rep] (with the freqw the last tile left).  Then every slot's partial map is applied to the values in front of its tile.
constexpr unsigned kRxbRepThreads = 256;
__global__ __launch_bounds__(kRxbRepThreads) void k_rxb_reports(rxb_args A) {
  const rxb_cap &cap = A.caps[blockIdx.x];
  const rxb_rep R = A.rep[blockIdx.x];
  const unsigned n_tiles = cap.n_tiles;
  if (!n_tiles) return;
  const unsigned n_rep = A.rep_period ? (unsigned)(cap.total_chunks * kChunk / A.rep_period) : 0u;
  __shared__ rx_ema_map s_wave[kRxbRepThreads / 64];
  const unsigned t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const unsigned per = (n_tiles + kRxbRepThreads - 1) / kRxbRepThreads;
  const unsigned lo = t * per < n_tiles ? t * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
  rx_ema_map m; m.a = 1.f; m.bi = m.bs = m.be = 0.f;
  for (unsigned i = lo; i < hi; ++i) m = ema_then(m, R.map[i]);
  rx_ema_map inc = m;                            // inclusive scan over the lanes of a wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    rx_ema_map o;
    o.a = __shfl_up(inc.a, d, 64); o.bi = __shfl_up(inc.bi, d, 64); o.bs = __shfl_up(inc.bs, d, 64); o.be = __shfl_up(inc.be, d, 64);
    if (lane >= (unsigned)d) inc = ema_then(o, inc);
  }
  if (lane == 63) s_wave[wv] = inc;
  __syncthreads();
  rx_ema_map pre; pre.a = 1.f; pre.bi = pre.bs = pre.be = 0.f;
  for (unsigned i = 0; i < wv; ++i) pre = ema_then(pre, s_wave[i]);
  rx_ema_map exl;                                // exclusive: lanes before this one in the wave
  exl.a = __shfl_up(inc.a, 1, 64); exl.bi = __shfl_up(inc.bi, 1, 64); exl.bs = __shfl_up(inc.bs, 1, 64); exl.be = __shfl_up(inc.be, 1, 64);
  if (lane == 0) { exl.a = 1.f; exl.bi = exl.bs = exl.be = 0.f; }
  pre = ema_then(pre, exl);
  const rx_state_dev *S0 = cap.state0;
  float vi = pre.a * S0->est_insp + pre.bi, vs = pre.a * S0->est_sp + pre.bs, ve = pre.a * S0->est_ep + pre.be;
  for (unsigned i = lo; i < hi; ++i) {
    const rx_ema_map mi = R.map[i];
    rx_ema_map v; v.a = 0.f; v.bi = vi; v.bs = vs; v.be = ve;
    R.map[i] = v;
    vi = mi.a * vi + mi.bi; vs = mi.a * vs + mi.bs; ve = mi.a * ve + mi.be;
  }
  if (lo < hi && hi == n_tiles) {
    rx_meas mm; mm.freqw = cap.state_end->freqw; mm.a = 0.f; mm.est_insp = vi; mm.est_sp = vs; mm.est_ep = ve; mm.tile = n_tiles - 1;
    R.slot[n_rep] = mm;
  }
  __syncthreads();
  for (unsigned q = t; q < n_rep; q += kRxbRepThreads) {
    rx_meas mm = R.slot[q];
    const rx_ema_map v = R.map[mm.tile < n_tiles ? mm.tile : 0u];
    mm.est_insp = mm.a * v.bi + mm.est_insp; mm.est_sp = mm.a * v.bs + mm.est_sp; mm.est_ep = mm.a * v.be + mm.est_ep;
    R.slot[q] = mm;
  }
}

__global__ __launch_bounds__(kSeamBlock) void k_rxb_seam(rxb_args A, float omega, int R, float quad, const uint8_t *relabel) {
  const rxb_cap &cap = A.caps[blockIdx.y];
  if (blockIdx.x * kSeamBlock >= cap.n_tiles) return;
  rx_seam_h_body(cap.hinfo, cap.fix, cap.n_tiles, omega, R, quad, cap.part, relabel);
}
constexpr unsigned kRxbCompactLanes = 4;      // lanes per tile in the compaction (rx_tiling.h)
__global__ __launch_bounds__(64) void k_rxb_compact(rxb_args A, int R, float quad, const uint8_t *relabel) {
  const rxb_cap &cap = A.caps[blockIdx.y];
  if (blockIdx.x * (64u / kRxbCompactLanes) >= cap.n_tiles) return;
  rx_compact_h_body<rx_state_dev, (int)kRxbCompactLanes>(cap.hstage, cap.hpitch, cap.hinfo, cap.fix, cap.part, relabel, cap.n_tiles, R, quad, cap.out_words, 0ull,
                                  cap.state_end, cap.res);
}

// Compaction of the soft tile columns.  One workgroup of 256 per (64 consecutive tiles × 64 symbol steps): the 64 × 64 dwords come out of
// the transposed staging row by row (64 consecutive dwords per row), turn in LDS, and leave tile by tile — each tile's 64 symbols are 256
// consecutive bytes of the output, relabelled by the tile's accumulated quadrant step (the symbol byte only: the cost does not depend on
// the quadrant).  blockIdx.x = tile group · row_blocks + row block; the row blocks behind a group's longest tile leave at once.  The 64
// tiles of a group lie in one seam block (kSeamBlock is a multiple of 64), so `base` is the total of the seam blocks in front of it.
// Tile group 0's first thread also leaves the capture's totals (rx_compact_h_body's duties) and the contiguous count viterbi_sync reads.
constexpr unsigned kRxbSoftTile = 64;
static_assert(kSeamBlock % kRxbSoftTile == 0, "the tiles of a soft compaction workgroup share their seam block");
__global__ __launch_bounds__(256) void k_rxb_compact_soft(rxb_args A, unsigned row_blocks, int R, float quad, const uint8_t *relabel) {
  const rxb_cap &cap = A.caps[blockIdx.y];
  const unsigned n_tiles = cap.n_tiles;
  const unsigned grp = blockIdx.x / row_blocks, rb = blockIdx.x - grp * row_blocks;
  const unsigned j0 = grp * kRxbSoftTile, k0 = rb * kRxbSoftTile;
  if (j0 >= n_tiles) return;
  const unsigned rmask = (unsigned)R - 1;
  const unsigned nparts = (n_tiles + kSeamBlock - 1) / kSeamBlock, mypart = j0 / kSeamBlock;
  const unsigned tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  if (blockIdx.x == 0 && tid == 0) {
    rx_seam_result sr; sr.total = 0; sr.rot_final = 0; sr.ndup = 0; sr.nmiss = 0; sr.nbad = 0; sr.freq_tap = rx_freq_tap(cap.state_end);
    for (unsigned i = 0; i < nparts; ++i) {
      sr.total += cap.part[i].cnt; sr.rot_final = (sr.rot_final + cap.part[i].rot) & rmask;
      sr.ndup += cap.part[i].ndup; sr.nmiss += cap.part[i].nmiss; sr.nbad += cap.part[i].nbad;
    }
    *cap.res = sr;
    *cap.count_out = sr.total;
    if (sr.rot_final) rx_rotate_back(cap.state_end, sr.rot_final, quad);
  }
  __shared__ unsigned s_cnt[kRxbSoftTile], s_skip[kRxbSoftTile], s_map[kRxbSoftTile], s_max;
  __shared__ long long s_Q[kRxbSoftTile];
  __shared__ unsigned s_t[kRxbSoftTile][kRxbSoftTile + 1];
  unsigned long long base = 0;
  unsigned brot = 0;
  for (unsigned i = 0; i < mypart; ++i) { base += cap.part[i].cnt; brot += cap.part[i].rot; }      // (uniform; a handful of records)
  if (tid == 0) s_max = 0;
  __syncthreads();
  if (tid < kRxbSoftTile) {
    unsigned cnt = 0, skip = 0, map4 = 0;
    long long Q = 0;
    if (j0 + tid < n_tiles) {
      const rx_tile_fix f = cap.fix[j0 + tid];
      cnt = cap.hinfo[j0 + tid].count;
      skip = f.drop_first ? 1u : 0u;
      const unsigned ins = f.insert_pre ? 1u : 0u;
      const long long D = (long long)(base + f.out_offset);
      Q = D + (long long)ins - (long long)skip;                         // body symbol k goes to out[Q + k]
      map4 = hs2_map4(relabel + ((f.rot + brot) & rmask) * 256);
      if (ins && rb == 0) {                                             // the warm-up's last symbol belongs to this tile
        const unsigned v = cap.spre[j0 + tid];
        cap.out_soft[D] = (v & 0xff00ffffu) | (((map4 >> (2 * ((v >> 16) & 3u))) & 3u) << 16);
      }
      atomicMax(&s_max, cnt);
    }
    s_cnt[tid] = cnt; s_skip[tid] = skip; s_map[tid] = map4; s_Q[tid] = Q;
  }
  __syncthreads();
  if (k0 >= s_max) return;                                              // (uniform)
  const unsigned cnt_l = s_cnt[lane];
#pragma unroll 4
  for (unsigned r = wv; r < kRxbSoftTile; r += 4) {                     // row k0 + r: 64 consecutive dwords
    const unsigned k = k0 + r;
    if (k < cnt_l) s_t[lane][r] = cap.sstage[(unsigned long long)k * cap.hpitch + j0 + lane];
  }
  __syncthreads();
  for (unsigned t = wv; t < kRxbSoftTile; t += 4) {                     // tile j0 + t: 64 consecutive symbols
    const unsigned k = k0 + lane;
    if (k < s_cnt[t] && k >= s_skip[t]) {
      const unsigned v = s_t[t][lane];
      cap.out_soft[s_Q[t] + (long long)k] = (v & 0xff00ffffu) | (((s_map[t] >> (2 * ((v >> 16) & 3u))) & 3u) << 16);
    }
  }
}

#endif  // LSDR_RXB_DEVICE_H
