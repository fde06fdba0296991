// leansdr_amd/csrc/ts_stitch.hip — lsdr_ts_stitch: the transport streams of the overlapping pieces of one recording, joined on the
// device so that no packet stands twice.  It reads TS buffers and touches no decode kernel.  The definition: include/lsdr_hip.h.
//
// For the pair (k, k + 1), T is the last min(W, n_k) packets of stream k and H the first min(W, n_k+1) of stream k + 1; cell (b, a) of the
// match matrix is "T[b] and H[a] have the same 188 bytes"; diagonal e holds the cells with a − b = e − (|T| − 1).
//
//   k_stitch_keys    blockIdx = (tile of 64 packets, tail | head, stream).  The tile's bytes as 16-byte loads from the 16-byte boundary
//                    at or below its first byte (a packet is 4-byte aligned, no more; the dwords outside the tile are masked); every
//                    dword adds st_mix to its packet's key in LDS.  Out: a 64-bit key per packet, its bit 0 the null flag.
//   k_stitch_spans   blockIdx = (band of 256 diagonals, pair), one lane per diagonal.  The keys of 512 rows of T and of the 767 columns
//                    of H the band meets there are staged in LDS (the row's key is a broadcast, the columns' keys consecutive); every
//                    lane counts its diagonal's key runs and keeps the rows [first, last) spanned by those of at least M.  A run of
//                    equal bytes of at least M lies inside one of them.
//   k_stitch_verify  blockIdx = (group of 64 diagonals, pair).  For every diagonal with a span, 256 cells at a time: a thread's cell is
//                    equal where the keys are and then the 47 dwords are — the byte compare decides, a key collision cannot join —; the
//                    wave ballots give the chunk as bit masks, every run's first thread reads its length and its packets that are not
//                    null from the masks, a run that reaches the chunk's end is carried.  A run that qualifies goes, as st_pack, into
//                    the pair's maximum: the longest, then the smallest a, then the smallest b — whatever the order of arrival.
//   k_stitch_plan    one workgroup: the joins, the kept ranges and their offsets in the output (a running prefix sum).
//   k_stitch_gather  blockIdx.y = stream: the kept range into the output, 16-byte stores (dword stores up to the first and behind the
//                    last 16-byte boundary of the stream's part).
//
// Five launches whatever the number of streams, nothing read by the host in between.  Every kernel leaves by the stream's own count:
// nothing is read behind packet n − 1 of a stream except the rest of the 16-byte line its last byte stands in, nothing at all of one
// with n = 0.
#include <cstdlib>
#include "capture_input.h"
#include "ts_stitch_device.h"

namespace {

static_assert(sizeof(lsdr_ts_join) == 24 && sizeof(lsdr_ts_keep) == 24, "lsdr_ts_stitch's records");

__device__ __forceinline__ unsigned st_min(unsigned long long n, unsigned W) { return n < W ? (unsigned)n : W; }

__global__ __launch_bounds__(kStThreads) void k_stitch_keys(st_args A) {
  const unsigned si = blockIdx.z, head = blockIdx.y, t = threadIdx.x;
  const st_stream S = A.st[si];
  const unsigned nreg = st_min(S.n, A.W), p0 = blockIdx.x * kStKeyTile;
  if (p0 >= nreg) return;
  const unsigned cnt = nreg - p0 < kStKeyTile ? nreg - p0 : kStKeyTile;
  __shared__ unsigned long long s_key[kStKeyTile];
  __shared__ unsigned s_null[kStKeyTile];
  if (t < kStKeyTile) s_key[t] = 0;
  __syncthreads();
  const unsigned long long first = (head ? 0ull : S.n - nreg) + p0;
  const size_t addr = (size_t)S.ts + (size_t)first * kStPacket;
  const unsigned lead = (unsigned)(addr & 15u) >> 2, total = cnt * kStDwords;
  const uint4 *src = reinterpret_cast<const uint4 *>(addr & ~(size_t)15u);
  const unsigned nvec = (lead + total + 3u) >> 2;
  for (unsigned j = t; j < nvec; j += kStThreads) {
    const uint4 v = src[j];
    const unsigned ws[4] = {v.x, v.y, v.z, v.w};
    unsigned long long acc = 0;
    unsigned at = ~0u;
#pragma unroll
    for (unsigned c = 0; c < 4u; ++c) {
      const unsigned q = 4u * j + c;
      if (q < lead || q - lead >= total) continue;
      const unsigned rel = q - lead, p = rel / kStDwords, w = rel - p * kStDwords;
      if (p != at) {
        if (at != ~0u) atomicAdd(&s_key[at], acc);
        at = p; acc = 0;
      }
      acc += st_mix(ws[c], w);
      if (w == 0) s_null[p] = st_is_null(ws[c]);
    }
    if (at != ~0u) atomicAdd(&s_key[at], acc);
  }
  __syncthreads();
  if (t < cnt) A.keys[((size_t)si * 2u + head) * A.W + p0 + t] = ((A.const_key ? 0ull : s_key[t]) & ~1ull) | s_null[t];
}

__global__ __launch_bounds__(kStThreads) void k_stitch_spans(st_args A) {
  const unsigned pair = blockIdx.y, t = threadIdx.x;
  if (pair + 1u >= A.P) return;
  const unsigned nT = st_min(A.st[pair].n, A.W), nH = st_min(A.st[pair + 1u].n, A.W);
  if (!nT || !nH) return;
  const unsigned ndiag = nT + nH - 1u, e0 = blockIdx.x * kStThreads;
  if (e0 >= ndiag) return;
  const int dlo = (int)e0 - (int)(nT - 1u), d = dlo + (int)t;
  const unsigned long long *kT = A.keys + ((size_t)pair * 2u + 0u) * A.W, *kH = A.keys + ((size_t)(pair + 1u) * 2u + 1u) * A.W;
  // the rows this band meets: a = b + d inside [0, nH) for some d of the band
  const int b_begin = -(dlo + (int)kStThreads - 1) > 0 ? -(dlo + (int)kStThreads - 1) : 0;
  const int b_end = (int)nH - dlo < (int)nT ? (int)nH - dlo : (int)nT;
  __shared__ unsigned long long sT[kStChunk], sH[kStChunk + kStThreads];
  const unsigned M = A.M;
  unsigned kr = 0, last = 0;
  int firstb = -1;
  for (int b0 = b_begin; b0 < b_end; b0 += (int)kStChunk) {
    const unsigned cnt = (unsigned)(b_end - b0) < kStChunk ? (unsigned)(b_end - b0) : kStChunk;
    __syncthreads();
    for (unsigned i = t; i < cnt; i += kStThreads) sT[i] = kT[b0 + (int)i];
    for (unsigned i = t; i < cnt + kStThreads - 1u; i += kStThreads) {
      const int a = b0 + dlo + (int)i;
      sH[i] = a >= 0 && a < (int)nH ? kH[a] : 0ull;
    }
    __syncthreads();
    for (unsigned i = 0; i < cnt; ++i) {
      const int b = b0 + (int)i, a = b + d;
      const bool keq = a >= 0 && a < (int)nH && sT[i] == sH[i + t];
      if (keq) {
        ++kr;
      } else {
        if (kr >= M) {
          if (firstb < 0) firstb = b - (int)kr;
          last = (unsigned)b;
        }
        kr = 0;
      }
    }
  }
  if (kr >= M) {                                                          // a run that ends with T
    if (firstb < 0) firstb = b_end - (int)kr;
    last = (unsigned)b_end;
  }
  if (e0 + t < ndiag) A.span[(size_t)pair * 2u * A.W + e0 + t] = firstb < 0 ? make_uint2(0u, 0u) : make_uint2((unsigned)firstb, last);
}

// the lowest position p ≥ from whose bit is clear in the 256-bit mask, 256: none
__device__ __forceinline__ unsigned st_next_clear(const unsigned long long (&m)[4], unsigned from) {
  for (unsigned w = from >> 6; w < 4u; ++w) {
    unsigned long long inv = ~m[w];
    if (w == from >> 6) inv &= ~0ull << (from & 63u);
    if (inv) return w * 64u + (unsigned)__ffsll((long long)inv) - 1u;
  }
  return 256u;
}
// the set bits of the mask at the positions [lo, hi)
__device__ __forceinline__ unsigned st_count(const unsigned long long (&z)[4], unsigned lo, unsigned hi) {
  unsigned n = 0;
#pragma unroll
  for (unsigned w = 0; w < 4u; ++w) {
    const unsigned wl = w * 64u;
    if (hi <= wl || lo >= wl + 64u) continue;
    unsigned long long x = z[w];
    if (lo > wl) x &= ~0ull << (lo - wl);
    if (hi < wl + 64u) x &= (1ull << (hi - wl)) - 1ull;
    n += (unsigned)__popcll(x);
  }
  return n;
}

__global__ __launch_bounds__(kStThreads) void k_stitch_verify(st_args A) {
  const unsigned pair = blockIdx.y, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  if (pair + 1u >= A.P) return;
  const st_stream ST = A.st[pair], SH = A.st[pair + 1u];
  const unsigned nT = st_min(ST.n, A.W), nH = st_min(SH.n, A.W);
  if (!nT || !nH) return;
  const unsigned ndiag = nT + nH - 1u, e0 = blockIdx.x * kStDiags;
  if (e0 >= ndiag) return;
  const unsigned long long *kT = A.keys + ((size_t)pair * 2u + 0u) * A.W, *kH = A.keys + ((size_t)(pair + 1u) * 2u + 1u) * A.W;
  const unsigned *pT = reinterpret_cast<const unsigned *>(ST.ts) + (size_t)(ST.n - nT) * kStDwords;
  const unsigned *pH = reinterpret_cast<const unsigned *>(SH.ts);
  __shared__ uint2 s_span[kStDiags];
  __shared__ unsigned long long s_m[4], s_z[4];
  if (t < kStDiags) s_span[t] = e0 + t < ndiag ? A.span[(size_t)pair * 2u * A.W + e0 + t] : make_uint2(0u, 0u);
  __syncthreads();
  const unsigned M = A.M, need = (M + 1u) / 2u;
  unsigned long long best = 0;
  for (unsigned q = 0; q < kStDiags; ++q) {
    const uint2 sp = s_span[q];
    if (!sp.y) continue;                                                  // (uniform)
    const int d = (int)(e0 + q) - (int)(nT - 1u);
    unsigned carry_len = 0, carry_nn = 0, carry_start = 0;                // the run that reached the last chunk's end (the same in every thread)
    for (unsigned c0 = sp.x; c0 < sp.y; c0 += kStThreads) {
      const unsigned cnt = sp.y - c0 < kStThreads ? sp.y - c0 : kStThreads, b = c0 + t;
      bool eq = false, nz = false;
      if (t < cnt) {
        const unsigned a = (unsigned)((int)b + d);
        const unsigned long long kt = kT[b];
        if (kt == kH[a]) {
          const unsigned *x = pT + (size_t)b * kStDwords, *y = pH + (size_t)a * kStDwords;
          unsigned diff = 0;
#pragma unroll
          for (unsigned w = 0; w < kStDwords; ++w) diff |= x[w] ^ y[w];
          eq = diff == 0;
          nz = eq && !(kt & 1ull);
        }
      }
      const unsigned long long bm = __ballot(eq), bz = __ballot(nz);
      if (lane == 0) { s_m[wave] = bm; s_z[wave] = bz; }
      __syncthreads();
      const unsigned long long m[4] = {s_m[0], s_m[1], s_m[2], s_m[3]}, z[4] = {s_z[0], s_z[1], s_z[2], s_z[3]};
      const bool more = c0 + cnt < sp.y;                                  // (then cnt is 256)
      if (eq && (t == 0 || !((m[(t - 1u) >> 6] >> ((t - 1u) & 63u)) & 1ull))) {   // a run's first thread
        const unsigned end = st_next_clear(m, t + 1u);                    // (the bits from cnt on are clear)
        unsigned len = end - t, nn = st_count(z, t, end), start = b;
        if (t == 0 && carry_len) { len += carry_len; nn += carry_nn; start = carry_start; }
        if (!(more && end == kStThreads) && len >= M && nn >= need) {
          const unsigned long long v = st_pack(len, (unsigned)((int)start + d), start);
          if (v > best) best = v;
        }
      }
      if (t == 0 && !eq && carry_len >= M && carry_nn >= need) {          // the carried run ended with the last chunk
        const unsigned long long v = st_pack(carry_len, (unsigned)((int)carry_start + d), carry_start);
        if (v > best) best = v;
      }
      if (more && (m[3] >> 63)) {                                        // the chunk's last run goes on: carried
        unsigned s = 0;
        for (int w = 3; w >= 0; --w)
          if (~m[w]) { s = (unsigned)w * 64u + 64u - (unsigned)__clzll((long long)~m[w]); break; }
        const unsigned len = kStThreads - s, nn = st_count(z, s, kStThreads);
        if (s == 0 && carry_len) { carry_len += len; carry_nn += nn; }
        else { carry_len = len; carry_nn = nn; carry_start = c0 + s; }
      } else {
        carry_len = 0; carry_nn = 0;
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long o = __shfl_down(best, s, 64);
    if (o > best) best = o;
  }
  if (lane == 0 && best) atomicMax(A.best + pair, best);
}

__global__ __launch_bounds__(kStThreads) void k_stitch_plan(st_args A) {
  const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  __shared__ unsigned long long ws[4];
  unsigned long long before = 0;                                          // packets kept in front of this round's streams
  for (unsigned k0 = 0; k0 < A.P; k0 += kStThreads) {
    const unsigned k = k0 + t;
    unsigned long long len = 0, start = 0, end = 0;
    if (k < A.P) {
      const unsigned long long n = A.st[k].n;
      end = n;
      if (k > 0) {
        const unsigned long long v = A.best[k - 1u];
        if (v) start = st_a(v) + st_run(v);
      }
      if (k + 1u < A.P) {
        const unsigned long long v = A.best[k];
        lsdr_ts_join j;
        j.joined = v ? 1u : 0u; j.run = st_run(v); j.end = n; j.next_start = 0;
        if (v) {
          j.end = (n - st_min(n, A.W)) + st_b(v) + st_run(v);
          j.next_start = st_a(v) + st_run(v);
        }
        end = j.end;
        A.joins[k] = j;
      }
      if (end < start) end = start;
      len = end - start;
    }
    unsigned long long x = len;
#pragma unroll
    for (unsigned s = 1; s < 64u; s <<= 1) {
      const unsigned long long y = __shfl_up(x, s, 64);
      if (lane >= s) x += y;
    }
    __syncthreads();
    if (lane == 63u) ws[wave] = x;
    __syncthreads();
    unsigned long long base = before, sum = 0;
#pragma unroll
    for (unsigned w = 0; w < 4u; ++w) {
      if (w < wave) base += ws[w];
      sum += ws[w];
    }
    if (k < A.P) {
      lsdr_ts_keep r;
      r.start = start; r.end = end; r.out_offset = base + x - len;
      A.keep[k] = r;
    }
    before += sum;
  }
  if (t == 0) *A.total = before;
}

__global__ __launch_bounds__(kStThreads) void k_stitch_gather(st_args A) {
  const unsigned k = blockIdx.y, t = threadIdx.x;
  const lsdr_ts_keep r = A.keep[k];
  if (r.end <= r.start) return;
  const unsigned *src = reinterpret_cast<const unsigned *>(A.st[k].ts) + (size_t)r.start * kStDwords;
  unsigned *out = reinterpret_cast<unsigned *>(A.out);
  const unsigned long long q0 = r.out_offset * kStDwords, q1 = q0 + (r.end - r.start) * kStDwords;   // this stream's dwords of the output
  unsigned long long v0 = (q0 + 3ull) >> 2, v1 = q1 >> 2;                 // … and the whole 16-byte lines among them
  if (v1 < v0) v1 = v0;
  if (blockIdx.x == 0) {
    const unsigned long long h1 = v0 * 4ull < q1 ? v0 * 4ull : q1, t0 = v1 * 4ull > h1 ? v1 * 4ull : h1;
    if (q0 + t < h1) out[q0 + t] = src[t];
    if (t0 + t < q1) out[t0 + t] = src[t0 + t - q0];
  }
  const bool wide = (((size_t)src + (size_t)(v0 * 4ull - q0) * 4u) & 15u) == 0;   // (uniform: every line's source then is 16-byte aligned)
  uint4 *out4 = reinterpret_cast<uint4 *>(A.out);
  for (unsigned long long j = v0 + (unsigned long long)blockIdx.x * kStThreads + t; j < v1; j += (unsigned long long)gridDim.x * kStThreads) {
    const unsigned *s = src + (j * 4ull - q0);
    out4[j] = wide ? *reinterpret_cast<const uint4 *>(s) : make_uint4(s[0], s[1], s[2], s[3]);
  }
}

}  // namespace

struct lsdr_ts_stitch {
  lsdr_ctx *ctx = nullptr;
  lsdr_ts_stitch_cfg cfg{};
  st_args A{};
  in_run<st_stream> run;
  lsdr_ts_join *h_joins = nullptr;                                        // pinned: [max(P − 1, 1)] joins, then h_keep = [P] kept ranges, then the
  lsdr_ts_keep *h_keep = nullptr;                                         //         total: one block like A.joins / A.keep / A.total, one copy per run
  size_t rec_bytes = 0, out_bytes = 0;
  unsigned gather_blocks = 1;
  hipStream_t dl = nullptr;                                               // the download of the output
  hipEvent_t ev_dl = nullptr;
  bool dl_pending = false, waited = false;
};

extern "C" {

void lsdr_ts_stitch_destroy(lsdr_ts_stitch *b) {
  if (!b) return;
  (void)hipStreamSynchronize(b->ctx->stream);
  if (b->dl) { (void)hipStreamSynchronize(b->dl); (void)hipStreamDestroy(b->dl); }
  if (b->ev_dl) (void)hipEventDestroy(b->ev_dl);
  b->run.destroy();
  lsdr_in_free({b->A.keys, b->A.span, b->A.best, b->A.joins, b->A.out}, {b->h_joins});
  delete b;
}

static int st_build(lsdr_ts_stitch *b) {
  lsdr_ctx *c = b->ctx;
  st_args &A = b->A;
  const size_t P = (size_t)b->cfg.n_streams, J = P > 1 ? P - 1 : 1;
  A.P = (unsigned)P;
  A.W = b->cfg.window ? b->cfg.window : 4096u;
  A.M = b->cfg.min_run ? b->cfg.min_run : 8u;
  // LSDR_TS_STITCH_CONST_KEY=1 (read per create) is a test hook: every packet's key is its null flag alone, so that packets with other
  // bytes meet with equal keys and the byte compare has to tell them apart.  The joins do not depend on it.
  const char *g = getenv("LSDR_TS_STITCH_CONST_KEY");
  A.const_key = g && atoi(g) ? 1u : 0u;
  LSDR_HIP(hipSetDevice(c->device));
  LSDR_TRY(b->run.create(P));
  LSDR_HIP(hipStreamCreateWithFlags(&b->dl, hipStreamNonBlocking));
  LSDR_HIP(hipEventCreateWithFlags(&b->ev_dl, hipEventDisableTiming));
  b->rec_bytes = J * sizeof(lsdr_ts_join) + P * sizeof(lsdr_ts_keep) + sizeof(unsigned long long);
  LSDR_HIP(hipHostMalloc((void **)&b->h_joins, b->rec_bytes, hipHostMallocDefault));
  memset(b->h_joins, 0, b->rec_bytes);
  b->h_keep = reinterpret_cast<lsdr_ts_keep *>(b->h_joins + J);
  LSDR_HIP(hipMalloc((void **)&A.joins, b->rec_bytes));
  A.keep = reinterpret_cast<lsdr_ts_keep *>(A.joins + J);
  A.total = reinterpret_cast<unsigned long long *>(A.keep + P);
  LSDR_HIP(hipMalloc((void **)&A.keys, P * 2u * A.W * sizeof(unsigned long long)));
  LSDR_HIP(hipMalloc((void **)&A.span, J * 2u * A.W * sizeof(uint2)));
  LSDR_HIP(hipMalloc((void **)&A.best, J * sizeof(unsigned long long)));
  b->out_bytes = ((P * b->cfg.max_packets * kStPacket + 15u) & ~(size_t)15u) + 16u;
  LSDR_HIP(hipMalloc((void **)&A.out, b->out_bytes));
  const size_t lines = (b->cfg.max_packets * kStPacket + 15u) / 16u, blocks = (lines + 4u * kStThreads - 1u) / (4u * kStThreads);
  b->gather_blocks = (unsigned)(blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks));
  A.st = b->run.d_caps;
  return LSDR_OK;
}

int lsdr_ts_stitch_create(lsdr_ctx *c, const lsdr_ts_stitch_cfg *cfg, lsdr_ts_stitch **out) {
  LSDR_ARG(c && cfg && out);
  if (cfg->n_streams < 1 || cfg->n_streams > 65535) { lsdr_set_error("ts_stitch: n_streams must be 1 to 65535 (got %d)", cfg->n_streams); return LSDR_E_ARG; }
  if (cfg->window > kStMaxWindow) { lsdr_set_error("ts_stitch: window must be at most 65535 (got %u)", cfg->window); return LSDR_E_ARG; }
  if (cfg->min_run > (cfg->window ? cfg->window : 4096u)) { lsdr_set_error("ts_stitch: min_run %u exceeds the window", cfg->min_run); return LSDR_E_ARG; }
  for (int i = 0; i < 8; ++i)
    if (cfg->reserved[i]) { lsdr_set_error("ts_stitch: lsdr_ts_stitch_cfg.reserved must be 0"); return LSDR_E_ARG; }
  if ((unsigned long long)cfg->max_packets >= (1ull << 32)) { lsdr_set_error("ts_stitch: max_packets must be below 2^32 (got %zu)", cfg->max_packets); return LSDR_E_UNSUPPORTED; }
  lsdr_ts_stitch *b = new lsdr_ts_stitch();
  b->ctx = c; b->cfg = *cfg;
  const int rc = st_build(b);
  if (rc) { lsdr_ts_stitch_destroy(b); return rc; }
  *out = b;
  return LSDR_OK;
}

int lsdr_ts_stitch_run_async(lsdr_ts_stitch *b, const uint8_t *const *ts_dev, const uint64_t *n_packets) {
  LSDR_ARG(b && ts_dev && n_packets);
  st_args &A = b->A;
  const unsigned P = A.P, J = P > 1 ? P - 1 : 1;
  for (unsigned i = 0; i < P; ++i) {
    if (n_packets[i] > b->cfg.max_packets) { lsdr_set_error("ts_stitch: stream %u: n_packets %llu exceeds max_packets %zu", i, (unsigned long long)n_packets[i], b->cfg.max_packets); return LSDR_E_ARG; }
    if (n_packets[i] && !ts_dev[i]) { lsdr_set_error("ts_stitch: stream %u has packets and no pointer", i); return LSDR_E_ARG; }
    if (n_packets[i] && (size_t)ts_dev[i] % 4u) { lsdr_set_error("ts_stitch: stream %u: the pointer is not aligned to 4 bytes", i); return LSDR_E_ARG; }
  }
  LSDR_TRY(b->run.idle("ts_stitch", "lsdr_ts_stitch_wait"));
  lsdr_ctx *c = b->ctx;
  LSDR_HIP(hipSetDevice(c->device));
  for (unsigned i = 0; i < P; ++i) {
    st_stream &S = b->run.h_caps[i];
    S.n = n_packets[i];
    S.ts = S.n ? ts_dev[i] : nullptr;
  }
  LSDR_TRY(b->run.upload(c->stream));
  // the gather waits for a download of the last run's output that is still pending
  if (b->dl_pending) LSDR_HIP(hipStreamWaitEvent(c->stream, b->ev_dl, 0));
  LSDR_HIP(hipMemsetAsync(A.best, 0, (size_t)J * sizeof(unsigned long long), c->stream));
  const unsigned ndiag = 2u * A.W - 1u;
  hipLaunchKernelGGL(k_stitch_keys, dim3((A.W + kStKeyTile - 1u) / kStKeyTile, 2, P), dim3(kStThreads), 0, c->stream, A);
  hipLaunchKernelGGL(k_stitch_spans, dim3((ndiag + kStThreads - 1u) / kStThreads, J), dim3(kStThreads), 0, c->stream, A);
  hipLaunchKernelGGL(k_stitch_verify, dim3((ndiag + kStDiags - 1u) / kStDiags, J), dim3(kStThreads), 0, c->stream, A);
  hipLaunchKernelGGL(k_stitch_plan, dim3(1), dim3(kStThreads), 0, c->stream, A);
  hipLaunchKernelGGL(k_stitch_gather, dim3(b->gather_blocks, P), dim3(kStThreads), 0, c->stream, A);
  LSDR_HIP(hipGetLastError());
  LSDR_HIP(hipMemcpyAsync(b->h_joins, A.joins, b->rec_bytes, hipMemcpyDeviceToHost, c->stream));
  b->waited = false;
  return b->run.mark(c->stream);
}

int lsdr_ts_stitch_wait(lsdr_ts_stitch *b, lsdr_ts_join *joins, lsdr_ts_keep *keep) {
  LSDR_ARG(b);
  LSDR_TRY(b->run.wait("ts_stitch"));
  b->waited = true;
  if (joins && b->A.P > 1) memcpy(joins, b->h_joins, (size_t)(b->A.P - 1u) * sizeof(lsdr_ts_join));
  if (keep) memcpy(keep, b->h_keep, (size_t)b->A.P * sizeof(lsdr_ts_keep));
  return LSDR_OK;
}

const uint8_t *lsdr_ts_stitch_out_dev(const lsdr_ts_stitch *b) { return b ? b->A.out : nullptr; }

int lsdr_ts_stitch_download_async(lsdr_ts_stitch *b, uint8_t *host, size_t cap_bytes) {
  LSDR_ARG(b);
  if (b->run.in_flight || !b->waited) { lsdr_set_error("ts_stitch: download before the lsdr_ts_stitch_wait of a run"); return LSDR_E_ARG; }
  const lsdr_ts_keep &last = b->h_keep[b->A.P - 1u];
  const size_t bytes = (size_t)(last.out_offset + (last.end - last.start)) * kStPacket;
  if (bytes > cap_bytes) { lsdr_set_error("ts_stitch: the output has %zu bytes, the host buffer has %zu", bytes, cap_bytes); return LSDR_E_ARG; }
  if (bytes && !host) { lsdr_set_error("ts_stitch: the output has %zu bytes and there is no host pointer", bytes); return LSDR_E_ARG; }
  LSDR_HIP(hipSetDevice(b->ctx->device));
  if (bytes) LSDR_HIP(hipMemcpyAsync(host, b->A.out, bytes, hipMemcpyDeviceToHost, b->dl));
  LSDR_HIP(hipEventRecord(b->ev_dl, b->dl));
  b->dl_pending = true;
  return LSDR_OK;
}

int lsdr_ts_stitch_download_wait(lsdr_ts_stitch *b) {
  LSDR_ARG(b);
  if (b->dl_pending) LSDR_HIP(hipEventSynchronize(b->ev_dl));
  b->dl_pending = false;
  return LSDR_OK;
}

}  // extern "C"
