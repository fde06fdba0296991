// leansdr_amd/csrc/tx_batch.hip — lsdr_tx_batch: leandvbtx | leanchansim (leandvbtx.cc:79-175, leanchansim.cc:115-189) for many transport
// streams in shared launches, each stream with its own length, code rate, power, scale, noise level and seed; the captures stay in device
// memory.  The definition: include/lsdr_hip.h.  Every grid is (tiles of the longest stream) × (streams); a workgroup leaves by its own
// stream's lengths, so nothing is read or written behind them.
//
//   k_txb_bytes    a lane per packet: randomizer (XOR with the 8-packet pattern) and rs_encoder (division by G, the tables in LDS) in one
//                  pass, 204 bytes per packet.  The interleaver is not a pass: the symbol stage gathers out[p][i] = in[p + 11 − i%12][i].
//   k_txb_symbols  a lane per 8 groups of the coder = bits_in bytes in, 8·bits_out/bps symbols out.  The input bits slide through a 64-bit
//                  window (newest at bit 0); a coded bit is the parity of the window's low 16 bits under the bit-reversed polynomial.
//   k_txb_samples  a workgroup per 2048 output samples: the tile's symbol bytes, the stream's point table and its taps are staged in LDS
//                  and only the kept 1/decim of fir_resampler's outputs are computed, x = x + c·p with k ascending (dsp.h:318-332).  The
//                  constellation points never exist as a cf32 stream.  With AGC the same workgroup sums its 16 chunks' powers from LDS,
//                  sample by sample like simple_agc.
//   k_txb_agc      a wave per stream: the EMA chain over the chunk powers on wave-uniform values fed by v_readlane, the gains in parallel.
//   k_txb_ncount, k_txb_nscan, k_txb_emit   wgn_c per stream by count → scan → emit over a candidate budget (chan.hip's scheme).  An emit
//                  workgroup owns 4096 candidate pairs and with them a contiguous run of outputs: it puts the accepted pairs' samples in
//                  output order into LDS, then applies gain, scale, + noise, the drifter's table entry 0 and the u8 conversion lane by
//                  lane, so that every output is written once and both sides are coalesced.
//   k_txb_report   the result records.
// A stream whose candidates ran out is finished by further rounds of the last four kernels, driven by lsdr_tx_batch_wait.
#include <cmath>
#include "capture_input.h"
#include "tx_batch_device.h"

namespace {

static_assert(sizeof(lsdr_tx_each) == 64 && sizeof(lsdr_tx_result) == 64, "lsdr_tx_batch's records");
constexpr unsigned kTS = 188, kRS = 204;
constexpr unsigned kYPad = kTxbTile + kTxbTile / 128;                     // a chunk's 128 samples start one LDS slot further: 16 banks

__global__ __launch_bounds__(64) void k_txb_bytes(txb_args A) {
  const txb_stream &S = A.st[blockIdx.y];
  const unsigned long long p = (unsigned long long)blockIdx.x * 64 + threadIdx.x;
  if (!S.il_packets || (unsigned long long)blockIdx.x * 64 >= S.n_packets) return;   // (uniform)
  __shared__ gf_tab g;
  __shared__ unsigned char pat[1504];
  for (unsigned i = threadIdx.x; i < sizeof(gf_tab); i += 64) ((unsigned char *)&g)[i] = ((const unsigned char *)A.gf)[i];
  for (unsigned i = threadIdx.x; i < 1504u; i += 64) pat[i] = A.pattern[i];
  __syncthreads();
  if (p >= S.n_packets) return;
  const unsigned char *pin = S.ts + p * kTS;
  const unsigned char *pp = pat + (unsigned)(p & 7u) * kTS;               // pattern[(188·p + d) % 1504]
  unsigned char *po = A.rs + (size_t)blockIdx.y * A.rs_stride + p * kRS;
  unsigned char r[17];                                                    // sliding remainder: r[0] pairs with message byte d
  unsigned char lg[17];
#pragma unroll
  for (int i = 0; i < 17; ++i) { r[i] = 0; lg[i] = g.log[g.G[i]]; }
  const unsigned inv0 = 255u - lg[0];
  for (unsigned d = 0; d < kTS; ++d) {
    const unsigned char m = pin[d] ^ pp[d];
    po[d] = m;
    const unsigned char top = m ^ r[0];
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = r[i + 1];
    r[16] = 0;
    if (top) {
      const unsigned char k = g.exp[g.log[top] + inv0];                   // gdiv(p[d], G[0]); never 0
      const unsigned lk = g.log[k];
#pragma unroll
      for (int i = 1; i <= 16; ++i) r[i - 1] ^= g.G[i] ? g.exp[lk + lg[i]] : (unsigned char)0;
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) po[kTS + i] = r[i];
}

// byte j of the interleaver's output (dvb.h:899-921) from the RS packets
__device__ __forceinline__ unsigned txb_il(const unsigned char *rs, unsigned long long j) {
  const unsigned long long p = j / kRS;
  const unsigned i = (unsigned)(j - p * kRS);
  return rs[(p + 11u - i % 12u) * kRS + i];
}

__global__ __launch_bounds__(kTxbThreads) void k_txb_symbols(txb_args A) {
  const txb_stream &S = A.st[blockIdx.y];
  const unsigned bi = (unsigned)S.bits_in, bo = (unsigned)S.bits_out, bps = (unsigned)S.bps;
  const unsigned long long t = (unsigned long long)blockIdx.x * kTxbThreads + threadIdx.x;
  if (t * bi >= S.bytes) return;                                          // bytes is a multiple of bits_in
  const unsigned char *rs = A.rs + (size_t)blockIdx.y * A.rs_stride;
  const unsigned long long j0 = t * bi;
  unsigned short rp[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) rp[p] = S.rpolys[p];
  // the 16 input bits in front of this lane's first (a fresh coder's history is 0)
  unsigned long long w = 0;
  if (j0 >= 2) w = (txb_il(rs, j0 - 2) << 8) | txb_il(rs, j0 - 1);
  else if (j0 == 1) w = txb_il(rs, 0);
  unsigned char *out = A.sym + (size_t)blockIdx.y * A.sym_stride + t * (8u * bo / bps);
  const unsigned mask = (1u << bps) - 1u;
  unsigned avail = 0, no = 0;
  for (unsigned i = 0; i < bi; ++i) {
    w = (w << 8) | txb_il(rs, j0 + i);
    avail += 8;
    while (avail >= bi) {
      avail -= bi;
      const unsigned win = (unsigned)(w >> avail) & 0xffffu;              // bit k: the input bit k places before the group's last
      unsigned ser = 0;
      for (unsigned p = 0; p < bo; ++p) ser = (ser << 1) | ((unsigned)__popc(win & rp[p]) & 1u);
      for (unsigned left = bo; left >= bps; left -= bps) out[no++] = (unsigned char)((ser >> (left - bps)) & mask);
    }
  }
}

__global__ __launch_bounds__(kTxbThreads) void k_txb_samples(txb_args A) {
  const unsigned si = blockIdx.y, t = threadIdx.x;
  const txb_stream &S = A.st[si];
  const unsigned long long q0 = (unsigned long long)blockIdx.x * kTxbTile;
  if (q0 >= S.samples) return;
  const unsigned cnt = S.samples - q0 < kTxbTile ? (unsigned)(S.samples - q0) : kTxbTile;
  // LDS as the object needs it (txb_samples_lds): taps | points | the tile's samples (AGC only) | symbol bytes
  extern __shared__ __attribute__((aligned(16))) unsigned char txb_lds[];
  const unsigned N = A.ncoeffs, I = A.interp, D = A.decim;
  float2 *s_taps = reinterpret_cast<float2 *>(txb_lds), *s_pts = s_taps + N, *s_y = s_pts + 256;
  unsigned char *s_sym = reinterpret_cast<unsigned char *>(s_y + (A.agc ? kYPad : 0u));
  const unsigned kback = (N - 1u) / I;                                    // the oldest symbol a group reads lies kback behind its newest
  const unsigned long long o_first = q0 * D, m_first = o_first / I;
  const unsigned rel0 = (unsigned)(o_first - m_first * I);
  const unsigned m_span = (rel0 + (cnt - 1u) * D) / I + 1u, span = m_span + kback;
  // symbol latency + m − k of the stream ↔ s_sym[(m − m_first) + kback − k]; latency ≥ kback + 1 and latency + m < symbols (the plan)
  const unsigned char *sym = A.sym + (size_t)si * A.sym_stride + (A.latency + m_first - kback);
  for (unsigned x = t; x < span; x += kTxbThreads) s_sym[x] = sym[x];
  for (unsigned x = t; x < N; x += kTxbThreads) s_taps[x] = A.taps[(size_t)si * N + x];
  s_pts[t] = A.points[(size_t)S.point_set * 256u + t];
  __syncthreads();
  float2 *y = A.y + (size_t)si * A.y_stride + q0;
#pragma unroll 2
  for (unsigned l = t; l < cnt; l += kTxbThreads) {
    const unsigned rel = rel0 + l * D, m = rel / I, i = rel - m * I;
    unsigned idx = m + kback;
    float xr = 0.f, xi = 0.f;
    for (unsigned c = i; c < N; c += I, --idx) {
      const float2 cc = s_taps[c], p = s_pts[s_sym[idx]];
      const float pr = cc.x * p.x - cc.y * p.y;                           // complex·complex, math.h:40-43
      const float pq = cc.x * p.y + cc.y * p.x;
      xr = xr + pr;
      xi = xi + pq;
    }
    const float2 v = make_float2(xr, xi);
    y[l] = v;
    if (A.agc) s_y[l + (l >> 7)] = v;
  }
  if (!A.agc) return;                                                     // (uniform)
  __syncthreads();
  if (t < cnt / 128u) {                                                   // with AGC `samples`, and so cnt, are whole chunks
    const float2 *p = s_y + t * 129u;
    float a = 0.f;
    for (int i = 0; i < 128; ++i) a += p[i].x * p[i].x + p[i].y * p[i].y;
    A.gain[(size_t)si * A.chunk_stride + q0 / 128u + t] = a / 128;
  }
}

// simple_agc's EMA over one stream's chunk powers → gains in place (tx.hip's k_agc_gains, a fresh block: estimated starts at 0)
__global__ __launch_bounds__(64) void k_txb_agc(txb_args A) {
  const unsigned si = blockIdx.x, lane = threadIdx.x;
  const txb_stream &S = A.st[si];
  const unsigned long long nchunks = S.samples / 128u;
  float *amp2_gain = A.gain + (size_t)si * A.chunk_stride;
  const float bw = S.bw, out_rms = S.out_rms;
  float est = 0.f;
  const float keep = 1 - bw;
  float nxt = lane < nchunks ? amp2_gain[lane] : 0.f;
  for (unsigned long long c0 = 0; c0 < nchunks; c0 += 64) {
    const float cur = nxt;
    const unsigned long long cn = c0 + 64 + lane;
    nxt = cn < nchunks ? amp2_gain[cn] : 0.f;
    const unsigned m = (unsigned)(nchunks - c0 < 64 ? nchunks - c0 : 64);
    float mine = 0.f;
    const float curbw = cur * bw;
    if (est != 0.f && m == 64) {
      // a whole step of the walk in two unrolled halves (all 64 at once keeps 64 lane reads in SGPRs and spills them): per chunk a
      // lane read, the chain's multiply and add, and the compare and select that leave the lane its own estimate
#pragma unroll 32
      for (unsigned i = 0; i < 64; ++i) {
        est = est * keep + __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(curbw), i));
        if (lane == i) mine = est;
      }
    } else if (est != 0.f) {
      for (unsigned i = 0; i < m; ++i) {
        est = est * keep + __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(curbw), i));
        if (lane == i) mine = est;
      }
    } else {
      for (unsigned i = 0; i < m; ++i) {
        const float a = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(cur), i));
        if (!est) est = a;
        est = est * keep + a * bw;
        if (lane == i) mine = est;
      }
    }
    if (lane < m) amp2_gain[c0 + lane] = mine ? out_rms / __builtin_sqrtf(mine) : 0.f;
  }
  if (lane == 0) A.est[si] = est;
}

// wgn_c (dsp.h:164-190), pass 1: the accepted pairs of every 4096 candidates of the stream's budget
__global__ __launch_bounds__(kTxbThreads) void k_txb_ncount(txb_args A) {
  const unsigned si = blockIdx.y;
  const txb_stream &S = A.st[si];
  if ((unsigned long long)blockIdx.x * kTxbNoiseBlock >= S.npairs) return;
  __shared__ unsigned red[kTxbThreads / 64];
  const unsigned long long first = ((unsigned long long)blockIdx.x * kTxbThreads + threadIdx.x) * kTxbNoisePairs;
  unsigned cnt = 0;
  if (first < S.npairs) {
    unsigned long long x = lcg_jump(*A.pw, S.x0, 2 * first);
    const unsigned m = (unsigned)((S.npairs - first) < kTxbNoisePairs ? (S.npairs - first) : kTxbNoisePairs);
    for (unsigned j = 0; j < m; ++j) {
      const float u = (float)(2 * lcg_next(x) - 1), v = (float)(2 * lcg_next(x) - 1);
      const float r2 = u * u + v * v;
      cnt += !(r2 == 0 || r2 >= 1);
    }
  }
  for (int o = 32; o; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) A.ncount[(size_t)si * A.noise_blocks + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// pass 2: the exclusive scan of one stream's counts, a workgroup per stream; the total at [nblocks]
__global__ __launch_bounds__(1024) void k_txb_nscan(txb_args A) {
  const unsigned si = blockIdx.x;
  const txb_stream &S = A.st[si];
  const unsigned nblocks = (unsigned)((S.npairs + kTxbNoiseBlock - 1) / kTxbNoiseBlock);
  const unsigned *block_count = A.ncount + (size_t)si * A.noise_blocks;
  unsigned long long *block_off = A.noff + (size_t)si * (A.noise_blocks + 1u);
  __shared__ unsigned long long part[1024];
  const unsigned per = (nblocks + 1023) / 1024, lo = threadIdx.x * per < nblocks ? threadIdx.x * per : nblocks, hi = lo + per < nblocks ? lo + per : nblocks;
  unsigned long long s = 0;
  for (unsigned i = lo; i < hi; ++i) s += block_count[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (unsigned o = 1; o < 1024; o <<= 1) {
    const unsigned long long v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  unsigned long long run = part[threadIdx.x] - s;
  for (unsigned i = lo; i < hi; ++i) { block_off[i] = run; run += block_count[i]; }
  if (threadIdx.x == 1023) block_off[nblocks] = part[1023];
}

// pass 3: regenerate the candidates, and write output done0 + i of the stream where the reference's i-th accepted pair falls:
// simple_agc's gain, scaler, + noise, the drifter's rotation by its table entry 0 (cosf(0), sinf(0)) = (1, 0), the u8 conversion
__global__ __launch_bounds__(kTxbThreads) void k_txb_emit(txb_args A) {
  const unsigned si = blockIdx.y;
  const txb_stream &S = A.st[si];
  if ((unsigned long long)blockIdx.x * kTxbNoiseBlock >= S.npairs) return;
  __shared__ unsigned wsum[kTxbThreads / 64];
  __shared__ logf_tab t;
  if (threadIdx.x < 16) { t.invc[threadIdx.x] = A.lt->invc[threadIdx.x]; t.logc[threadIdx.x] = A.lt->logc[threadIdx.x]; }
  const unsigned nblocks = (unsigned)((S.npairs + kTxbNoiseBlock - 1) / kTxbNoiseBlock);
  const unsigned long long *block_off = A.noff + (size_t)si * (A.noise_blocks + 1u);
  const unsigned long long n = S.samples - S.done0, base = block_off[blockIdx.x];
  if (base >= n) return;                                                  // the whole workgroup lies past the last output (uniform)
  const unsigned long long first = ((unsigned long long)blockIdx.x * kTxbThreads + threadIdx.x) * kTxbNoisePairs;
  __shared__ float2 s_nz[kTxbNoiseBlock];                                 // the workgroup's noise samples, in output order
  unsigned m = 0;
  unsigned long long x0 = 0;
  if (first < S.npairs) {
    x0 = lcg_jump(*A.pw, S.x0, 2 * first);
    m = (unsigned)((S.npairs - first) < kTxbNoisePairs ? (S.npairs - first) : kTxbNoisePairs);
  }
  // (a) this lane's accepted pairs, and from them its first place among the workgroup's outputs
  unsigned cnt = 0;
  unsigned long long x = x0;
  for (unsigned j = 0; j < m; ++j) {
    const float u = (float)(2 * lcg_next(x) - 1), v = (float)(2 * lcg_next(x) - 1);
    const float r2 = u * u + v * v;
    cnt += !(r2 == 0 || r2 >= 1);
  }
  unsigned incl = cnt;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = __shfl_up(incl, o);
    if ((int)(threadIdx.x & 63) >= o) incl += v;
  }
  if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
  __syncthreads();
  unsigned woff = 0, total = 0;
  for (unsigned w = 0; w < kTxbThreads / 64; ++w) {
    if (w < (threadIdx.x >> 6)) woff += wsum[w];
    total += wsum[w];
  }
  // (b) the candidates again: every accepted pair's sample goes to its place in LDS; x is the state behind the pair
  const float stddev = S.stddev;
  unsigned l = woff + incl - cnt;
  x = x0;
  for (unsigned j = 0; j < m; ++j) {
    const float u = (float)(2 * lcg_next(x) - 1), v = (float)(2 * lcg_next(x) - 1);
    const float r2 = u * u + v * v;
    if (!(r2 == 0 || r2 >= 1)) {
      if (base + l < n) {
        const float k = __builtin_sqrtf(-glibc_logf(t, r2) / r2) * stddev;
        s_nz[l] = make_float2(k * u, k * v);
        if (base + l == n - 1) A.nout[si] = txb_noise_out{S.samples, x};
      }
      ++l;
    }
  }
  // the candidates ran out before the last output: the owner of the very last pair reports what there is
  if (first < S.npairs && first + m == S.npairs && block_off[nblocks] < n) A.nout[si] = txb_noise_out{S.done0 + block_off[nblocks], x};
  __syncthreads();
  // (c) the workgroup's outputs base … base + lim of this round, lane by lane: both sides coalesced
  const unsigned lim = n - base < total ? (unsigned)(n - base) : total;
  const unsigned long long g0 = S.done0 + base;
  const float2 *y = A.y + (size_t)si * A.y_stride + g0;
  const float *gain = A.gain + (size_t)si * A.chunk_stride;
  unsigned char *out = A.out + (size_t)si * A.out_stride;
  const float scale = S.scale;
  const float2 rot = make_float2(1.0f, 0.0f);
  for (unsigned i = threadIdx.x; i < lim; i += kTxbThreads) {
    const unsigned long long g = g0 + i;
    float2 a = y[i];
    if (A.agc) { const float gn = gain[g >> 7]; a = make_float2(a.x * gn, a.y * gn); }
    a = make_float2(a.x * scale, a.y * scale);
    const float2 nz = s_nz[i];
    const float2 v = make_float2(a.x + nz.x, a.y + nz.y);
    const float2 o = make_float2(v.x * rot.x - v.y * rot.y, v.x * rot.y + v.y * rot.x);
    if (A.out_u8)
      reinterpret_cast<uchar2 *>(out)[g] = make_uchar2((unsigned char)x86_f2i(128 + (o.x - 0.f) * 1 / 1), (unsigned char)x86_f2i(128 + (o.y - 0.f) * 1 / 1));
    else
      reinterpret_cast<float2 *>(out)[g] = o;
  }
}

__global__ __launch_bounds__(kTxbThreads) void k_txb_report(txb_args A) {
  const unsigned si = blockIdx.x * kTxbThreads + threadIdx.x;
  if (si >= A.n_streams) return;
  const txb_stream &S = A.st[si];
  lsdr_tx_result R;
  memset(&R, 0, sizeof(R));
  R.packets = S.il_packets; R.bytes = S.bytes; R.symbols = S.symbols; R.samples = S.samples;
  R.noise_state = A.nout[si].state;
  // round 1 writes every stream (0 without samples); in a further round the host marks a stream that had finished with round 0
  R.noise_rounds = S.npairs ? S.round : (S.round ? 0u : A.results[si].noise_rounds);
  R.agc_estimated = A.agc ? A.est[si] : 0.f;
  A.results[si] = R;
}

const int kCstlnBits[9] = {1, 2, 3, 4, 5, 6, 4, 6, 8};                    // BPSK, QPSK, 8PSK, 16APSK, 32APSK, 64APSKe, 16/64/256QAM

struct txb_rate { int bits_in, bits_out, bps; uint16_t polys[8]; };
// leandvbtx.cc:112-121 and dvb_convol's constructor: the coder a constellation and a --cr give, or lsdr_convol_create's refusal
int txb_coder(int cstln, int fec, txb_rate *r) {
  if (cstln < 0 || cstln >= 9) { lsdr_set_error("tx_batch: cstln %d is no constellation", cstln); return LSDR_E_ARG; }
  r->bps = kCstlnBits[cstln];
  const int rate = (fec == LSDR_FEC23 && (r->bps == 2 || r->bps == 6)) ? LSDR_FEC46 : fec;   // "Handling rate 2/3 as 4/6"
  if (lsdr_fec_spec(rate, &r->bits_in, &r->bits_out, r->polys) != LSDR_OK) { lsdr_set_error("tx_batch: dvb_convol: Unexpected FEC"); return LSDR_E_ARG; }
  if (r->bits_out % r->bps) { lsdr_set_error("tx_batch: dvb_convol: Code rate not suitable for this constellation"); return LSDR_E_ARG; }
  return LSDR_OK;
}

int txb_check_cfg(const lsdr_tx_batch_cfg *cfg) {
  if (cfg->n_streams < 1 || cfg->n_streams > 65535) { lsdr_set_error("tx_batch: n_streams must be 1 to 65535 (got %d)", cfg->n_streams); return LSDR_E_ARG; }
  if (cfg->cstln < 0 || cfg->cstln >= 9) { lsdr_set_error("tx_batch: cstln %d is no constellation", cfg->cstln); return LSDR_E_ARG; }
  if (cfg->interp < 1 || cfg->decim < 1) { lsdr_set_error("tx_batch: interp and decim must be at least 1 (got %d/%d)", cfg->interp, cfg->decim); return LSDR_E_ARG; }
  if (cfg->out_format != LSDR_IN_CF32 && cfg->out_format != LSDR_IN_CU8) { lsdr_set_error("tx_batch: out_format %d is neither LSDR_IN_CF32 nor LSDR_IN_CU8", cfg->out_format); return LSDR_E_ARG; }
  if (!std::isfinite(cfg->rolloff) || cfg->rolloff < 0.f || !std::isfinite(cfg->rrc_rej) || cfg->rrc_rej < 0.f) { lsdr_set_error("tx_batch: rolloff and rrc_rej must be finite and not negative"); return LSDR_E_ARG; }
  for (int i = 0; i < 8; ++i)
    if (cfg->reserved[i]) { lsdr_set_error("tx_batch: lsdr_tx_batch_cfg.reserved must be 0"); return LSDR_E_ARG; }
  return LSDR_OK;
}
int txb_order(const lsdr_tx_batch_cfg *cfg) { return (int)((float)cfg->interp * (cfg->rrc_rej == 0.f ? 10.f : cfg->rrc_rej)); }   // leandvbtx.cc:133
unsigned txb_ncoeffs(const lsdr_tx_batch_cfg *cfg) { return (unsigned)((txb_order(cfg) + 1) | 1); }                              // filtergen.h:68-92

// the lengths of one stream, block by block (what every block consumes of a whole stream handed to it in one call)
void txb_plan(const lsdr_tx_batch_cfg *cfg, const txb_rate &r, unsigned long long n_packets, txb_stream *S) {
  const unsigned long long N = txb_ncoeffs(cfg), I = (unsigned)cfg->interp, D = (unsigned)cfg->decim;
  S->n_packets = n_packets;
  S->il_packets = n_packets >= 12 ? n_packets - 11 : 0;                                      // while in.readable() >= 12 (dvb.h:906)
  S->bytes = S->il_packets * kRS / (unsigned)r.bits_in * (unsigned)r.bits_in;                // whole groups (dvb.h:587-591)
  S->symbols = S->bytes * 8 / (unsigned)r.bits_in * (unsigned)r.bits_out / (unsigned)r.bps;
  unsigned long long count = 0;                                                              // lsdr_fir_resampler_run
  const unsigned long long n_in = S->symbols, latency = (N + I) / I;
  if (n_in >= N && n_in * I >= N && n_in > latency) {
    count = (n_in * I - N) / I;
    if (count > n_in - latency) count = n_in - latency;
  }
  S->resampled = count * I / D;                                                              // decimator (generic.h:256-262)
  S->samples = cfg->agc ? S->resampled / 128 * 128 : S->resampled;                           // simple_agc's chunks (sdr.h:253-273)
}

unsigned short txb_brev16(unsigned v) {
  unsigned r = 0;
  for (int k = 0; k < 16; ++k) r |= ((v >> k) & 1u) << (15 - k);
  return (unsigned short)r;
}

// the noise stage's candidate budget for `want` outputs: acceptance is π/4, the accepted count's deviation is sqrt(0.17·want) (chan.hip)
unsigned long long txb_budget(unsigned long long want, float sigmas) {
  if (!want) return 0;
  const double sd = sqrt((double)want * 0.17);
  double np = (double)want * 1.2732395447351628 + (double)sigmas * sd * 1.2732395447351628 + 64;
  if (np < 1) np = 1;
  return (unsigned long long)np;
}

}  // namespace

struct lsdr_tx_batch {
  lsdr_ctx *ctx = nullptr;
  lsdr_tx_batch_cfg cfg{};
  txb_args A{};
  in_run<txb_stream> run;
  std::vector<float> rrc;                                                 // root_raised_cosine before normalize_power
  float2 *h_taps = nullptr, *d_taps = nullptr;                            // pinned / device [B][ncoeffs]
  float2 *h_points = nullptr, *d_points = nullptr;                        // pinned / device [16 rates][256]
  int point_set_of[16];                                                   // code rate → set built in h_points, −1: not yet
  unsigned n_point_sets = 0;
  txb_noise_out *h_nout = nullptr;                                        // pinned [B]
  lsdr_tx_result *h_results = nullptr;                                    // pinned [B]
  void *d_tables = nullptr;                                               // gf_tab, pattern, lcg_pow, logf_tab
  unsigned long long max_samples = 0, max_symbols = 0, noise_cap = 0;
  float sigmas = 6.f;
  unsigned item = 8, launches = 0, samples_lds = 0;
  unsigned long long runs = 0;
  hipStream_t dl = nullptr;
  hipEvent_t ev_dl = nullptr;
  bool dl_pending = false, waited = false;
};

static void txb_launch_noise(lsdr_tx_batch *b, unsigned long long max_pairs) {
  hipStream_t s = b->ctx->stream;
  const unsigned B = (unsigned)b->cfg.n_streams;
  unsigned nb = (unsigned)((max_pairs + kTxbNoiseBlock - 1) / kTxbNoiseBlock);
  if (!nb) nb = 1;
  hipLaunchKernelGGL(k_txb_ncount, dim3(nb, B), dim3(kTxbThreads), 0, s, b->A);
  hipLaunchKernelGGL(k_txb_nscan, dim3(B), dim3(1024), 0, s, b->A);
  hipLaunchKernelGGL(k_txb_emit, dim3(nb, B), dim3(kTxbThreads), 0, s, b->A);
  hipLaunchKernelGGL(k_txb_report, dim3((B + kTxbThreads - 1) / kTxbThreads), dim3(kTxbThreads), 0, s, b->A);
  b->launches += 4;
}
static int txb_fetch(lsdr_tx_batch *b) {
  const size_t B = (size_t)b->cfg.n_streams;
  LSDR_HIP(hipGetLastError());
  LSDR_HIP(hipMemcpyAsync(b->h_results, b->A.results, B * sizeof(lsdr_tx_result), hipMemcpyDeviceToHost, b->ctx->stream));
  LSDR_HIP(hipMemcpyAsync(b->h_nout, b->A.nout, B * sizeof(txb_noise_out), hipMemcpyDeviceToHost, b->ctx->stream));
  return b->run.mark(b->ctx->stream);
}

extern "C" {

float lsdr_db_to_amplitude(double db) { return expf(logf(10) * db / 20); }

int lsdr_tx_batch_plan(const lsdr_tx_batch_cfg *cfg, const lsdr_tx_each *each, lsdr_tx_result *result) {
  LSDR_ARG(cfg && each && result);
  LSDR_TRY(txb_check_cfg(cfg));
  txb_rate r;
  LSDR_TRY(txb_coder(cfg->cstln, each->fec, &r));
  txb_stream S;
  txb_plan(cfg, r, each->n_packets, &S);
  memset(result, 0, sizeof(*result));
  result->packets = S.il_packets; result->bytes = S.bytes; result->symbols = S.symbols; result->samples = S.samples;
  return LSDR_OK;
}

void lsdr_tx_batch_destroy(lsdr_tx_batch *b) {
  if (!b) return;
  (void)hipStreamSynchronize(b->ctx->stream);
  if (b->dl) { (void)hipStreamSynchronize(b->dl); (void)hipStreamDestroy(b->dl); }
  if (b->ev_dl) (void)hipEventDestroy(b->ev_dl);
  b->run.destroy();
  lsdr_in_free({b->A.rs, b->A.sym, b->A.y, b->A.gain, b->A.est, b->d_taps, b->d_points, b->A.ncount, b->A.noff, b->A.nout, b->A.out, b->A.results, b->d_tables},
               {b->h_taps, b->h_points, b->h_nout, b->h_results});
  delete b;
}

static int txb_build(lsdr_tx_batch *b) {
  lsdr_ctx *c = b->ctx;
  const lsdr_tx_batch_cfg &cfg = b->cfg;
  txb_args &A = b->A;
  const size_t B = (size_t)cfg.n_streams;
  A.n_streams = (unsigned)B; A.interp = (unsigned)cfg.interp; A.decim = (unsigned)cfg.decim; A.agc = cfg.agc ? 1u : 0u;
  A.out_u8 = cfg.out_format == LSDR_IN_CU8; b->item = A.out_u8 ? 2u : 8u;
  A.ncoeffs = txb_ncoeffs(&cfg);
  A.latency = (A.ncoeffs + A.interp) / A.interp;
  if (A.ncoeffs > kTxbMaxTaps) { lsdr_set_error("tx_batch: %u taps (interp·rrc_rej), at most %u", A.ncoeffs, kTxbMaxTaps); return LSDR_E_UNSUPPORTED; }
  const unsigned long long span = ((unsigned long long)(A.interp - 1u) + (unsigned long long)(kTxbTile - 1u) * A.decim) / A.interp + 1u + (A.ncoeffs - 1u) / A.interp;
  if (span > kTxbMaxSpan) { lsdr_set_error("tx_batch: interp/decim %u/%u needs %llu symbols per sample tile, at most %u", A.interp, A.decim, span, kTxbMaxSpan); return LSDR_E_UNSUPPORTED; }
  b->samples_lds = (A.ncoeffs + 256u + (A.agc ? kYPad : 0u)) * (unsigned)sizeof(float2) + (((unsigned)span + 15u) & ~15u);   // k_txb_samples' LDS
  if ((unsigned long long)cfg.max_packets >= (1ull << 24)) { lsdr_set_error("tx_batch: max_packets must be below 2^24 (got %zu)", cfg.max_packets); return LSDR_E_UNSUPPORTED; }
  b->rrc.resize((size_t)txb_order(&cfg) + 3);
  const float Fm = 1.0 / cfg.interp;                                      // leandvbtx.cc:132-136
  const int nc = lsdr_filtergen_root_raised_cosine(txb_order(&cfg), Fm, cfg.rolloff == 0.f ? 0.35f : cfg.rolloff, b->rrc.data());
  if (nc != (int)A.ncoeffs) { lsdr_set_error("tx_batch: root_raised_cosine gave %d taps, expected %u", nc, A.ncoeffs); return LSDR_E_ARG; }
  // the buffers: max_packets at the rate that gives the most of each item
  bool any = false;
  for (int fec = 0; fec < 16; ++fec) {
    b->point_set_of[fec] = -1;
    txb_rate r;
    if (txb_coder(cfg.cstln, fec, &r) != LSDR_OK) continue;
    txb_stream S;
    txb_plan(&cfg, r, cfg.max_packets, &S);
    if (S.samples > b->max_samples) b->max_samples = S.samples;
    if (S.symbols > b->max_symbols) b->max_symbols = S.symbols;
    any = true;
  }
  if (!any) { lsdr_set_error("tx_batch: no code rate suits constellation %d", cfg.cstln); return LSDR_E_ARG; }
  A.rs_stride = (cfg.max_packets * kRS + 15u) & ~(size_t)15u; if (!A.rs_stride) A.rs_stride = 16;
  A.sym_stride = (b->max_symbols + 15u) & ~(size_t)15u; if (!A.sym_stride) A.sym_stride = 16;
  A.y_stride = b->max_samples ? b->max_samples : 1;
  A.chunk_stride = b->max_samples / 128u + 1u;
  A.out_stride = (b->max_samples * b->item + 15u) & ~(size_t)15u; if (!A.out_stride) A.out_stride = 16;
  b->noise_cap = txb_budget(b->max_samples, 8.f);                         // room for margins up to 8 σ; a larger one is clamped
  A.noise_blocks = (unsigned)((b->noise_cap + kTxbNoiseBlock - 1) / kTxbNoiseBlock) + 1u;
  b->noise_cap = (unsigned long long)(A.noise_blocks - 1u) * kTxbNoiseBlock;
  LSDR_HIP(hipSetDevice(c->device));
  LSDR_TRY(b->run.create(B));
  LSDR_HIP(hipStreamCreateWithFlags(&b->dl, hipStreamNonBlocking));
  LSDR_HIP(hipEventCreateWithFlags(&b->ev_dl, hipEventDisableTiming));
  LSDR_HIP(hipHostMalloc((void **)&b->h_taps, B * A.ncoeffs * sizeof(float2), hipHostMallocDefault));
  LSDR_HIP(hipHostMalloc((void **)&b->h_points, 16 * 256 * sizeof(float2), hipHostMallocDefault));
  LSDR_HIP(hipHostMalloc((void **)&b->h_nout, B * sizeof(txb_noise_out), hipHostMallocDefault));
  LSDR_HIP(hipHostMalloc((void **)&b->h_results, B * sizeof(lsdr_tx_result), hipHostMallocDefault));
  memset(b->h_points, 0, 16 * 256 * sizeof(float2));
  memset(b->h_results, 0, B * sizeof(lsdr_tx_result));
  LSDR_HIP(hipMalloc((void **)&A.rs, B * A.rs_stride));
  LSDR_HIP(hipMalloc((void **)&A.sym, B * A.sym_stride));
  LSDR_HIP(hipMalloc((void **)&A.y, B * A.y_stride * sizeof(float2)));
  LSDR_HIP(hipMalloc((void **)&A.gain, B * A.chunk_stride * sizeof(float)));
  LSDR_HIP(hipMalloc((void **)&A.est, B * sizeof(float)));
  LSDR_HIP(hipMalloc((void **)&b->d_taps, B * A.ncoeffs * sizeof(float2)));
  LSDR_HIP(hipMalloc((void **)&b->d_points, 16 * 256 * sizeof(float2)));
  LSDR_HIP(hipMalloc((void **)&A.ncount, B * A.noise_blocks * sizeof(unsigned)));
  LSDR_HIP(hipMalloc((void **)&A.noff, B * (A.noise_blocks + 1u) * sizeof(unsigned long long)));
  LSDR_HIP(hipMalloc((void **)&A.nout, B * sizeof(txb_noise_out)));
  LSDR_HIP(hipMalloc((void **)&A.out, B * A.out_stride));
  LSDR_HIP(hipMalloc((void **)&A.results, B * sizeof(lsdr_tx_result)));
  LSDR_HIP(hipMemset(A.results, 0, B * sizeof(lsdr_tx_result)));
  // the read-only tables, one block: gf_tab | pattern | lcg_pow | logf_tab, each 16-byte aligned
  struct tables { gf_tab gf; alignas(16) unsigned char pattern[1504]; alignas(16) lcg_pow pw; alignas(16) logf_tab lt; };
  tables *T = new tables();
  lsdr_rs_tables(T->gf.exp, T->gf.log, T->gf.G);
  lsdr_derandomizer_pattern(T->pattern);                                  // same precompute_pattern() (dvb.h:1074-1087 ≡ :1116-1129)
  lsdr_lcg_pow_fill(T->pw);
  lsdr_logf_tab_fill(T->lt);
  hipError_t e = hipMalloc(&b->d_tables, sizeof(tables));
  if (e == hipSuccess) e = hipMemcpy(b->d_tables, T, sizeof(tables), hipMemcpyHostToDevice);
  delete T;
  LSDR_HIP(e);
  tables *dT = reinterpret_cast<tables *>(b->d_tables);
  A.gf = &dT->gf; A.pattern = dT->pattern; A.pw = &dT->pw; A.lt = &dT->lt;
  A.taps = b->d_taps; A.points = b->d_points; A.st = b->run.d_caps;
  return LSDR_OK;
}

int lsdr_tx_batch_create(lsdr_ctx *c, const lsdr_tx_batch_cfg *cfg, lsdr_tx_batch **out) {
  LSDR_ARG(c && cfg && out);
  LSDR_TRY(txb_check_cfg(cfg));
  lsdr_tx_batch *b = new lsdr_tx_batch();
  b->ctx = c; b->cfg = *cfg;
  const int rc = txb_build(b);
  if (rc) { lsdr_tx_batch_destroy(b); return rc; }
  *out = b;
  return LSDR_OK;
}

int lsdr_tx_batch_set_noise_margin(lsdr_tx_batch *b, float sigmas) {
  LSDR_ARG(b && std::isfinite(sigmas));
  b->sigmas = sigmas;
  return LSDR_OK;
}

int lsdr_tx_batch_stats(const lsdr_tx_batch *b, unsigned *launches_last_run, unsigned long long *runs) {
  LSDR_ARG(b);
  if (launches_last_run) *launches_last_run = b->launches;
  if (runs) *runs = b->runs;
  return LSDR_OK;
}

int lsdr_tx_batch_run_async(lsdr_tx_batch *b, const uint8_t *const *ts_dev, const lsdr_tx_each *each) {
  LSDR_ARG(b && ts_dev && each);
  const lsdr_tx_batch_cfg &cfg = b->cfg;
  const unsigned B = (unsigned)cfg.n_streams;
  txb_args &A = b->A;
  for (unsigned i = 0; i < B; ++i) {
    const lsdr_tx_each &E = each[i];
    if (E.reserved0) { lsdr_set_error("tx_batch: stream %u: lsdr_tx_each.reserved must be 0", i); return LSDR_E_ARG; }
    for (int k = 0; k < 6; ++k)
      if (E.reserved[k]) { lsdr_set_error("tx_batch: stream %u: lsdr_tx_each.reserved must be 0", i); return LSDR_E_ARG; }
    if (E.n_packets > cfg.max_packets) { lsdr_set_error("tx_batch: stream %u: n_packets %llu exceeds max_packets %zu", i, (unsigned long long)E.n_packets, cfg.max_packets); return LSDR_E_ARG; }
    if (E.n_packets && !ts_dev[i]) { lsdr_set_error("tx_batch: stream %u has packets and no pointer", i); return LSDR_E_ARG; }
    if (!std::isfinite(E.amp) || !std::isfinite(E.scale) || !std::isfinite(E.noise_stddev)) { lsdr_set_error("tx_batch: stream %u: amp, scale and noise_stddev must be finite", i); return LSDR_E_ARG; }
    txb_rate r;
    LSDR_TRY(txb_coder(cfg.cstln, E.fec, &r));
    if (E.fec < 0 || E.fec >= 16) { lsdr_set_error("tx_batch: stream %u: fec %d", i, E.fec); return LSDR_E_ARG; }
    if (b->point_set_of[E.fec] < 0) {
      lsdr::cstln_tables tab;
      if (lsdr::build_cstln(cfg.cstln, E.fec, tab) < 0) { lsdr_set_error("tx_batch: stream %u: constellation/code rate not supported", i); return LSDR_E_ARG; }
    }
  }
  LSDR_TRY(b->run.idle("tx_batch", "lsdr_tx_batch_wait"));
  lsdr_ctx *c = b->ctx;
  LSDR_HIP(hipSetDevice(c->device));
  const float cs0 = cosf(0.f), sn0 = sinf(0.f);                           // fir_resampler::set_freq(0) (dsp.h:351-360)
  std::vector<float> co(A.ncoeffs);
  unsigned long long longest_pk = 0, longest_bytes = 0, longest_samples = 0, most_pairs = 0;
  for (unsigned i = 0; i < B; ++i) {
    const lsdr_tx_each &E = each[i];
    txb_stream &S = b->run.h_caps[i];
    memset(&S, 0, sizeof(S));
    txb_rate r;
    LSDR_TRY(txb_coder(cfg.cstln, E.fec, &r));
    txb_plan(&cfg, r, E.n_packets, &S);
    S.ts = E.n_packets ? ts_dev[i] : nullptr;
    S.bits_in = r.bits_in; S.bits_out = r.bits_out; S.bps = r.bps;
    for (int p = 0; p < 8; ++p) S.rpolys[p] = txb_brev16(r.polys[p]);
    if (b->point_set_of[E.fec] < 0) {                                     // make_dvbs2_constellation(cstln, the rate asked for) (leandvbtx.cc:112)
      lsdr::cstln_tables tab;
      if (lsdr::build_cstln(cfg.cstln, E.fec, tab) < 0) return LSDR_E_ARG;
      float2 *pts = b->h_points + (size_t)b->n_point_sets * 256u;
      for (int s = 0; s < tab.nsymbols; ++s) pts[s] = make_float2((float)(0 + tab.symbols[s][0]), (float)(0 + tab.symbols[s][1]));   // Zout + cp (sdr.h:1213-1214)
      b->point_set_of[E.fec] = (int)b->n_point_sets++;
    }
    S.point_set = (unsigned)b->point_set_of[E.fec];
    S.scale = E.scale == 0.f ? 1.0f : E.scale;
    S.stddev = E.noise_stddev;
    S.out_rms = E.amp / sqrtf((float)cfg.interp / cfg.decim);             // leandvbtx.cc:163-165
    S.bw = 0.001 * cfg.decim / cfg.interp;
    S.x0 = lsdr_drand48_start(E.seeded, E.seed);
    S.done0 = 0;
    S.npairs = txb_budget(S.samples, b->sigmas);
    if (S.npairs > b->noise_cap) S.npairs = b->noise_cap;
    S.round = 1;
    b->h_nout[i] = txb_noise_out{0, S.x0};
    // this stream's taps: normalize_power(amp / cstln_amp) (leandvbtx.cc:138), then the resampler's shift by frequency 0
    memcpy(co.data(), b->rrc.data(), A.ncoeffs * sizeof(float));
    lsdr_filtergen_normalize_power((int)A.ncoeffs, co.data(), E.amp / 75.0f);
    float2 *sc = b->h_taps + (size_t)i * A.ncoeffs;
    for (unsigned k = 0; k < A.ncoeffs; ++k) sc[k] = make_float2(co[k] * cs0, co[k] * sn0);
    if (S.il_packets && S.n_packets > longest_pk) longest_pk = S.n_packets;
    if (S.bytes / (unsigned)r.bits_in > longest_bytes) longest_bytes = S.bytes / (unsigned)r.bits_in;
    if (S.samples > longest_samples) longest_samples = S.samples;
    if (S.npairs > most_pairs) most_pairs = S.npairs;
  }
  hipStream_t s = c->stream;
  if (b->dl_pending) LSDR_HIP(hipStreamWaitEvent(s, b->ev_dl, 0));        // the emit pass writes what a pending download reads
  LSDR_TRY(b->run.upload(s));
  LSDR_HIP(hipMemcpyAsync(b->d_taps, b->h_taps, (size_t)B * A.ncoeffs * sizeof(float2), hipMemcpyHostToDevice, s));
  LSDR_HIP(hipMemcpyAsync(b->d_points, b->h_points, 16 * 256 * sizeof(float2), hipMemcpyHostToDevice, s));
  LSDR_HIP(hipMemcpyAsync(A.nout, b->h_nout, (size_t)B * sizeof(txb_noise_out), hipMemcpyHostToDevice, s));
  b->launches = 0;
  auto tiles = [](unsigned long long n, unsigned per) { return (unsigned)(n ? (n + per - 1) / per : 1); };
  hipLaunchKernelGGL(k_txb_bytes, dim3(tiles(longest_pk, 64), B), dim3(64), 0, s, A);
  hipLaunchKernelGGL(k_txb_symbols, dim3(tiles(longest_bytes, kTxbThreads), B), dim3(kTxbThreads), 0, s, A);
  hipLaunchKernelGGL(k_txb_samples, dim3(tiles(longest_samples, kTxbTile), B), dim3(kTxbThreads), b->samples_lds, s, A);
  b->launches += 3;
  if (A.agc) { hipLaunchKernelGGL(k_txb_agc, dim3(B), dim3(64), 0, s, A); ++b->launches; }
  txb_launch_noise(b, most_pairs);
  b->waited = false;
  ++b->runs;
  return txb_fetch(b);
}

int lsdr_tx_batch_wait(lsdr_tx_batch *b, lsdr_tx_result *results) {
  LSDR_ARG(b);
  LSDR_TRY(b->run.wait("tx_batch"));
  const unsigned B = (unsigned)b->cfg.n_streams;
  for (;;) {                                                              // further rounds for the streams whose candidates ran out
    unsigned long long most_pairs = 0;
    for (unsigned i = 0; i < B; ++i) {
      txb_stream &S = b->run.h_caps[i];
      const txb_noise_out &O = b->h_nout[i];
      S.npairs = 0;
      if (O.done >= S.samples) { S.round = 0; continue; }
      S.x0 = O.state; S.done0 = O.done; ++S.round;
      S.npairs = txb_budget(S.samples - S.done0, b->sigmas > 6.f ? b->sigmas : 6.f);
      if (S.npairs > b->noise_cap) S.npairs = b->noise_cap;
      if (S.npairs > most_pairs) most_pairs = S.npairs;
    }
    if (!most_pairs) break;
    LSDR_HIP(hipSetDevice(b->ctx->device));
    LSDR_TRY(b->run.upload(b->ctx->stream));
    txb_launch_noise(b, most_pairs);
    LSDR_TRY(txb_fetch(b));
    LSDR_TRY(b->run.wait("tx_batch"));
  }
  b->waited = true;
  if (results) memcpy(results, b->h_results, (size_t)B * sizeof(lsdr_tx_result));
  return LSDR_OK;
}

const void *lsdr_tx_batch_out_dev(const lsdr_tx_batch *b, int i) {
  return b && i >= 0 && i < b->cfg.n_streams ? b->A.out + (size_t)i * b->A.out_stride : nullptr;
}
const lsdr_tx_result *lsdr_tx_batch_results_dev(const lsdr_tx_batch *b) { return b ? b->A.results : nullptr; }

int lsdr_tx_batch_download_async(lsdr_tx_batch *b, void *const *host, size_t cap_bytes) {
  LSDR_ARG(b && host);
  if (b->run.in_flight || !b->waited) { lsdr_set_error("tx_batch: download before the lsdr_tx_batch_wait of a run"); return LSDR_E_ARG; }
  const unsigned B = (unsigned)b->cfg.n_streams;
  for (unsigned i = 0; i < B; ++i) {
    const size_t bytes = (size_t)b->h_results[i].samples * b->item;
    if (bytes > cap_bytes) { lsdr_set_error("tx_batch: stream %u has %zu bytes, the host buffer has %zu", i, bytes, cap_bytes); return LSDR_E_ARG; }
    if (bytes && !host[i]) { lsdr_set_error("tx_batch: stream %u has %zu bytes and no host pointer", i, bytes); return LSDR_E_ARG; }
  }
  LSDR_HIP(hipSetDevice(b->ctx->device));
  for (unsigned i = 0; i < B; ++i) {
    const size_t bytes = (size_t)b->h_results[i].samples * b->item;
    if (bytes) LSDR_HIP(hipMemcpyAsync(host[i], b->A.out + (size_t)i * b->A.out_stride, bytes, hipMemcpyDeviceToHost, b->dl));
  }
  LSDR_HIP(hipEventRecord(b->ev_dl, b->dl));
  b->dl_pending = true;
  return LSDR_OK;
}

int lsdr_tx_batch_download_wait(lsdr_tx_batch *b) {
  LSDR_ARG(b);
  if (b->dl_pending) LSDR_HIP(hipEventSynchronize(b->ev_dl));
  b->dl_pending = false;
  return LSDR_OK;
}

}  // extern "C"
