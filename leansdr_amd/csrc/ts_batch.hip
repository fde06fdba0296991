// leansdr_amd/csrc/ts_batch.hip — lsdr_ts_batch: the census (packet classes, per-PID continuity, PCR) and the PID filter of many finished
// transport streams in device memory, each with its own length, in shared launches.  It reads TS buffers and touches no decode kernel.
// The definition: include/lsdr_hip.h.
//
//   k_ts_scan     blockIdx.y = stream, blockIdx.x = tile of `tile` packets, one workgroup of 256.  One 8-byte load per packet (bytes 0 … 7)
//                 gives a 4-byte descriptor in LDS (ts_batch_device.h: ts_desc).  Every valid packet walks the descriptors backwards, four
//                 per LDS read, to its predecessor of the same PID inside the tile and applies the pair rule (ts_pair); the walks of one
//                 PID add up to at most the tile, so the cost is about PIDs present × tile.  A packet without a predecessor opens its
//                 PID's entry in LDS and sets the PID's bit in the stream's presence bitmap.  The packets' contributions are summed per
//                 wave and PID by ballots (a dominant video PID is 90 % of a stream) and added to the entry by one lane; the entries go to
//                 the global per-PID counters with one set of atomics per tile and PID, and {first, last descriptor} of every entry to
//                 the tile's list.  With a rule the same pass writes the places of the tile's kept packets, in order, and their number.
//   k_ts_stitch   one workgroup per stream holds last[8192] descriptors in LDS and walks the tile lists in order — the entries of one
//                 tile are distinct PIDs and are handled in parallel, eight tiles' entries are fetched at a time — and applies the pair
//                 rule across the seams, also to a predecessor several tiles back.  With a rule it sums the tiles' kept counts into
//                 their offsets in the output.
//   k_ts_report   one workgroup per stream: the bitmap's prefix popcount gives every PID its slot, the lowest max_pids go to the table,
//                 all of them to the totals; the two packets pcr_first_packet and pcr_last_packet of pcr_pid are re-read for their values.
//   k_ts_copy     tile × stream: the output as a flat dword array (188 bytes = 47 dwords), output dword q of the tile → kept packet q / 47
//                 → source dword; both sides coalesced.
//
// Every kernel leaves by the stream's own count: nothing is read behind packet n − 1 of a stream, nothing at all of one with n = 0.
// All sums are integers and every minimum and maximum is exact: the atomics' order cannot change a count, so a record is a pure function
// of the stream's bytes — the same alone, in any batch and at any tile size (LSDR_TS_BATCH_TILE, tests/test_gpu_ts_batch.py).
#include <cstdlib>
#include "capture_input.h"
#include "ts_batch_device.h"

namespace {

static_assert(sizeof(lsdr_ts_summary) == 128 && sizeof(lsdr_ts_pid) == 56, "lsdr_ts_batch's records");
static_assert(kTsStateWords % 2 == 0 && kTsStateTotals % 2 == 0, "the 64-bit totals are aligned");
static_assert(kTsDropNull == LSDR_TS_DROP_NULL && kTsDropTei == LSDR_TS_DROP_TEI && kTsDropSync == LSDR_TS_DROP_SYNC, "drop bits");

// a PID's entry in a tile (LDS): places are packets counted from the tile's first; the sums are two 16-bit counts per word (a tile has
// at most 1024 packets, cc_missing at most 15 per packet)
enum { kEFirst = 0, kELast, kEPacketsPusi, kEScrambledPcr, kEErrorsRepeats, kEMissingDisc, kEPcrFirst, kEPcrLast, kEWords };

// a packet's first two dwords as one load: the packets of a 4-byte aligned stream are 4-byte aligned, no more
struct __attribute__((packed, aligned(4))) ts_head { unsigned w0, w1; };

// exclusive prefix sum over the workgroup of 256, and the total; ws: four words of LDS
__device__ __forceinline__ unsigned ts_exscan(unsigned v, unsigned *ws, unsigned &total) {
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned x = v;
#pragma unroll
  for (unsigned s = 1; s < 64u; s <<= 1) {
    const unsigned y = __shfl_up(x, s, 64);
    if (lane >= s) x += y;
  }
  if (lane == 63u) ws[wave] = x;
  __syncthreads();
  unsigned base = 0;
  total = 0;
#pragma unroll
  for (unsigned w = 0; w < 4u; ++w) {
    if (w < wave) base += ws[w];
    total += ws[w];
  }
  __syncthreads();
  return base + x - v;
}

__device__ __forceinline__ unsigned *ts_counters(const ts_args &A, unsigned si, unsigned pid) {
  return A.state + (size_t)si * kTsStateWords + kTsStateCounters + (size_t)pid * kTsCounters;
}
// what a pair adds to its PID's counters
__device__ __forceinline__ void ts_count_pair(unsigned *C, unsigned r) {
  if (r & 1u) atomicAdd(C + kTsCDisc, 1u);
  if (r & 2u) atomicAdd(C + kTsCRepeats, 1u);
  if (r & 4u) { atomicAdd(C + kTsCErrors, 1u); atomicAdd(C + kTsCMissing, r >> 4); }
}

__global__ __launch_bounds__(kTsThreads) void k_ts_scan(ts_args A) {
  const unsigned si = blockIdx.y, T = A.tile;
  const ts_stream S = A.st[si];
  const unsigned long long p0 = (unsigned long long)blockIdx.x * T;
  if (p0 >= S.n) return;
  const unsigned cnt = S.n - p0 < T ? (unsigned)(S.n - p0) : T;
  __shared__ __attribute__((aligned(16))) unsigned d[kTsMaxTile];
  __shared__ unsigned short ent_of[kTsPids];
  __shared__ unsigned ent[kTsMaxTile * kEWords];
  __shared__ unsigned s_ne, s_sync, s_tei, s_pcr, s_keep[16];
  const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, ppt = T / kTsThreads;
  if (t == 0) { s_ne = 0; s_sync = 0; s_tei = 0; s_pcr = kTsNone; }
  if (t < 16u) s_keep[t] = 0;
  const unsigned *in = reinterpret_cast<const unsigned *>(S.ts) + p0 * kTsDwords;
  // bytes 0 … 7 of the thread's packets: one 8-byte load each (a packet is 4-byte aligned), all of them issued before the first is used
  ts_head hd[4];
#pragma unroll
  for (unsigned j = 0; j < 4u; ++j) {
    const unsigned l = j * kTsThreads + t;
    hd[j].w0 = 0; hd[j].w1 = 0;
    if (j < ppt && l < cnt) hd[j] = *reinterpret_cast<const ts_head *>(in + (size_t)l * kTsDwords);
  }
  unsigned mine[4];
#pragma unroll
  for (unsigned j = 0; j < 4u; ++j) {
    const unsigned l = j * kTsThreads + t;
    const unsigned v = j < ppt && l < cnt ? ts_desc(hd[j].w0, hd[j].w1) : (unsigned)kTsAbsent << kTsClassShift;
    mine[j] = v;
    if (j < ppt) d[l] = v;
  }
  __syncthreads();

  const unsigned char *keep = A.keep ? A.keep + (size_t)si * (kTsPids / 8u) : nullptr;
  unsigned res[4], kr[4];
#pragma unroll
  for (unsigned j = 0; j < 4u; ++j) {
    res[j] = 0; kr[j] = kTsNone;
    if (j >= ppt) continue;                                               // (uniform)
    const unsigned l = j * kTsThreads + t, v = mine[j], cls = ts_class(v);
    const unsigned long long bs = __ballot(cls == kTsSync), bt = __ballot(cls == kTsTei), bp = __ballot(cls == kTsValid && ts_pcr(v));
    if (lane == 0) {
      if (bs) atomicAdd(&s_sync, (unsigned)__popcll(bs));
      if (bt) atomicAdd(&s_tei, (unsigned)__popcll(bt));
      if (bp) atomicMin(&s_pcr, l + (unsigned)__ffsll((long long)bp) - 1u);
    }
    if (A.rule) {
      const bool kf = cls != kTsAbsent && ts_keeps(v, A.drop, keep);
      const unsigned long long bk = __ballot(kf);
      if (lane == 0) s_keep[j * 4u + wave] = (unsigned)__popcll(bk);
      if (kf) kr[j] = (unsigned)__popcll(bk & ((1ull << lane) - 1ull));
    }
    if (cls == kTsValid) {
      const unsigned pid = ts_pid(v);
      unsigned prev = kTsNone, k = l;
      while (k & 3u) {
        --k;
        if ((d[k] & kTsKeyMask) == pid) { prev = d[k]; break; }
      }
      if (prev == kTsNone) {
        while (k) {
          k -= 4u;
          const uint4 q = *reinterpret_cast<const uint4 *>(&d[k]);
          if ((q.w & kTsKeyMask) == pid) { prev = q.w; break; }
          if ((q.z & kTsKeyMask) == pid) { prev = q.z; break; }
          if ((q.y & kTsKeyMask) == pid) { prev = q.y; break; }
          if ((q.x & kTsKeyMask) == pid) { prev = q.x; break; }
        }
      }
      if (prev != kTsNone) {
        if (pid != kTsNullPid) res[j] = ts_pair(prev, v);
      } else {                                                            // the PID's first packet in the tile opens its entry
        const unsigned e = atomicAdd(&s_ne, 1u);
        ent_of[pid] = (unsigned short)e;
        unsigned *E = ent + e * kEWords;
        E[kEFirst] = l; E[kELast] = 0; E[kEPacketsPusi] = 0; E[kEScrambledPcr] = 0; E[kEErrorsRepeats] = 0; E[kEMissingDisc] = 0;
        E[kEPcrFirst] = 0xffffu; E[kEPcrLast] = 0;
        atomicOr(A.state + (size_t)si * kTsStateWords + (pid >> 5), 1u << (pid & 31u));
      }
    }
  }
  __syncthreads();

  // every packet's contribution to its PID's entry, summed per wave and PID: one lane adds
#pragma unroll
  for (unsigned j = 0; j < 4u; ++j) {
    if (j >= ppt) continue;
    const unsigned l = j * kTsThreads + t, v = mine[j], r = res[j], pid = ts_pid(v);
    const bool valid = ts_class(v) == kTsValid;
    unsigned long long todo = __ballot(valid);
    while (todo) {                                                        // (uniform)
      const unsigned leader = (unsigned)__ffsll((long long)todo) - 1u;
      const unsigned lp = (unsigned)__shfl((int)pid, (int)leader, 64);
      const bool same = valid && pid == lp;
      const unsigned long long m = __ballot(same), bpcr = __ballot(same && ts_pcr(v));
      const unsigned n_pusi = (unsigned)__popcll(__ballot(same && ts_pusi(v))), n_scr = (unsigned)__popcll(__ballot(same && ts_scrambled(v)));
      const unsigned n_disc = (unsigned)__popcll(__ballot(same && (r & 1u))), n_rep = (unsigned)__popcll(__ballot(same && (r & 2u)));
      const unsigned n_err = (unsigned)__popcll(__ballot(same && (r & 4u)));
      const unsigned n_miss = (unsigned)__popcll(__ballot(same && (r & 0x10u))) + 2u * (unsigned)__popcll(__ballot(same && (r & 0x20u))) +
                              4u * (unsigned)__popcll(__ballot(same && (r & 0x40u))) + 8u * (unsigned)__popcll(__ballot(same && (r & 0x80u)));
      if (lane == leader) {
        unsigned *E = ent + (unsigned)ent_of[lp] * kEWords;
        const unsigned base = l - lane;
        atomicAdd(E + kEPacketsPusi, (unsigned)__popcll(m) | (n_pusi << 16));
        if (n_scr | bpcr) atomicAdd(E + kEScrambledPcr, n_scr | ((unsigned)__popcll(bpcr) << 16));
        if (n_err | n_rep) atomicAdd(E + kEErrorsRepeats, n_err | (n_rep << 16));
        if (n_miss | n_disc) atomicAdd(E + kEMissingDisc, n_miss | (n_disc << 16));
        atomicMax(E + kELast, base + 63u - (unsigned)__clzll((long long)m));
        if (bpcr) {
          atomicMin(E + kEPcrFirst, base + (unsigned)__ffsll((long long)bpcr) - 1u);
          atomicMax(E + kEPcrLast, base + 63u - (unsigned)__clzll((long long)bpcr));
        }
      }
      todo &= ~m;
    }
  }
  __syncthreads();

  const size_t tile_at = (size_t)si * A.max_tiles + blockIdx.x;
  const unsigned ne = s_ne;
  for (unsigned e = t; e < ne; e += kTsThreads) {
    const unsigned *E = ent + e * kEWords;
    const unsigned fl = E[kEFirst], ll = E[kELast], fd = d[fl], ld = d[ll];
    A.list[tile_at * T + e] = make_uint2(fd, ld);
    unsigned *C = ts_counters(A, si, ts_pid(fd));
    const unsigned pp = E[kEPacketsPusi], sp = E[kEScrambledPcr], er = E[kEErrorsRepeats], md = E[kEMissingDisc];
    atomicAdd(C + kTsCPackets, pp & 0xffffu);
    if (pp >> 16) atomicAdd(C + kTsCPusi, pp >> 16);
    if (sp & 0xffffu) atomicAdd(C + kTsCScrambled, sp & 0xffffu);
    if (er & 0xffffu) atomicAdd(C + kTsCErrors, er & 0xffffu);
    if (er >> 16) atomicAdd(C + kTsCRepeats, er >> 16);
    if (md & 0xffffu) atomicAdd(C + kTsCMissing, md & 0xffffu);
    if (md >> 16) atomicAdd(C + kTsCDisc, md >> 16);
    atomicMax(C + kTsCNotFirst, ~(unsigned)(p0 + fl));
    atomicMax(C + kTsCLast, (unsigned)(p0 + ll));
    if (sp >> 16) {
      atomicAdd(C + kTsCPcrCount, sp >> 16);
      atomicMax(C + kTsCNotPcrFirst, ~(unsigned)(p0 + E[kEPcrFirst]));
      atomicMax(C + kTsCPcrLast, (unsigned)(p0 + E[kEPcrLast]));
    }
  }
  unsigned kept = 0;
  if (A.rule) {
    unsigned before[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (unsigned x = 0; x < 16u; ++x) {
      const unsigned c = s_keep[x];
#pragma unroll
      for (unsigned j = 0; j < 4u; ++j)
        if (x < j * 4u + wave) before[j] += c;
      kept += c;
    }
#pragma unroll
    for (unsigned j = 0; j < 4u; ++j)
      if (kr[j] != kTsNone) A.klist[tile_at * T + before[j] + kr[j]] = (unsigned short)(j * kTsThreads + t);
  }
  if (t == 0) {
    A.hdr[tile_at] = make_uint2(ne, kept);
    unsigned long long *tot = reinterpret_cast<unsigned long long *>(A.state + (size_t)si * kTsStateWords + kTsStateTotals);
    if (s_sync) atomicAdd(tot + kTsTSync, (unsigned long long)s_sync);
    if (s_tei) atomicAdd(tot + kTsTTei, (unsigned long long)s_tei);
    if (kept) atomicAdd(tot + kTsTKept, (unsigned long long)kept);
    if (s_pcr != kTsNone) atomicMax(tot + kTsTNotPcrKey, ~(((p0 + s_pcr) << 13) | ts_pid(d[s_pcr])));
  }
}

__global__ __launch_bounds__(kTsThreads) void k_ts_stitch(ts_args A) {
  const unsigned si = blockIdx.x, T = A.tile, t = threadIdx.x;
  const ts_stream S = A.st[si];
  const unsigned ntiles = (unsigned)((S.n + T - 1u) / T);
  __shared__ unsigned last[kTsPids];
  __shared__ unsigned hn[kTsThreads], ws[4];
  for (unsigned p = t; p < kTsPids; p += kTsThreads) last[p] = kTsNone;
  unsigned long long kept_run = 0;
  // what one list entry adds: the pair (the PID's last packet so far, the PID's first packet in this tile)
  auto seam = [&](uint2 en) {
    const unsigned pid = ts_pid(en.x), prev = last[pid];
    if (prev != kTsNone && pid != kTsNullPid) {
      const unsigned r = ts_pair(prev, en.x);
      if (r) ts_count_pair(ts_counters(A, si, pid), r);
    }
    last[pid] = en.y;
  };
  for (unsigned c0 = 0; c0 < ntiles; c0 += kTsThreads) {
    __syncthreads();
    const unsigned tile = c0 + t;
    const uint2 h = tile < ntiles ? A.hdr[(size_t)si * A.max_tiles + tile] : make_uint2(0u, 0u);
    hn[t] = h.x;
    if (A.rule) {
      unsigned total;
      const unsigned ex = ts_exscan(h.y, ws, total);
      if (tile < ntiles) A.koff[(size_t)si * A.max_tiles + tile] = (unsigned)(kept_run + ex);
      kept_run += total;
    }
    __syncthreads();
    const unsigned m = ntiles - c0 < kTsThreads ? ntiles - c0 : kTsThreads;
    for (unsigned jj = 0; jj < m; jj += 8u) {
      uint2 en[8];
#pragma unroll
      for (unsigned u = 0; u < 8u; ++u) {
        const unsigned tl = jj + u;
        en[u] = make_uint2(kTsNone, kTsNone);
        if (tl < m && t < hn[tl]) en[u] = A.list[((size_t)si * A.max_tiles + c0 + tl) * T + t];
      }
#pragma unroll
      for (unsigned u = 0; u < 8u; ++u) {
        const unsigned tl = jj + u;
        if (tl < m) {                                                     // (uniform)
          if (en[u].x != kTsNone) seam(en[u]);
          for (unsigned e = t + kTsThreads; e < hn[tl]; e += kTsThreads) seam(A.list[((size_t)si * A.max_tiles + c0 + tl) * T + e]);
          __syncthreads();
        }
      }
    }
  }
}

__global__ __launch_bounds__(kTsThreads) void k_ts_report(ts_args A) {
  const unsigned si = blockIdx.x, t = threadIdx.x;
  const ts_stream S = A.st[si];
  const unsigned *st = A.state + (size_t)si * kTsStateWords;
  __shared__ unsigned ws[4];
  __shared__ unsigned long long tot[6];
  if (t < 6u) tot[t] = 0;
  unsigned b = st[t], seen;
  unsigned slot = ts_exscan((unsigned)__popc(b), ws, seen);
  unsigned long long a[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};       // valid, null, errors, repeats, missing, discontinuities
  while (b) {
    const unsigned pid = t * 32u + (unsigned)__ffs((int)b) - 1u;
    b &= b - 1u;
    const unsigned *C = st + kTsStateCounters + (size_t)pid * kTsCounters;
    a[0] += C[kTsCPackets];
    if (pid == kTsNullPid) a[1] += C[kTsCPackets];
    a[2] += C[kTsCErrors]; a[3] += C[kTsCRepeats]; a[4] += C[kTsCMissing]; a[5] += C[kTsCDisc];
    if (slot < A.max_pids) {
      lsdr_ts_pid r;
      r.pid = pid; r.packets = C[kTsCPackets]; r.pusi = C[kTsCPusi]; r.scrambled = C[kTsCScrambled]; r.cc_errors = C[kTsCErrors];
      r.cc_repeats = C[kTsCRepeats]; r.cc_missing = C[kTsCMissing]; r.discontinuities = C[kTsCDisc]; r.pcr_count = C[kTsCPcrCount]; r.pad = 0;
      r.first_packet = ~C[kTsCNotFirst]; r.last_packet = C[kTsCLast];
      A.pids[(size_t)si * A.max_pids + slot] = r;
    }
    ++slot;
  }
#pragma unroll
  for (unsigned k = 0; k < 6u; ++k) {
    unsigned long long v = a[k];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s, 64);
    if ((t & 63u) == 0 && v) atomicAdd(&tot[k], v);
  }
  __syncthreads();
  if (t == 0) {
    const unsigned long long *g = reinterpret_cast<const unsigned long long *>(st + kTsStateTotals);
    lsdr_ts_summary s;
    memset(&s, 0, sizeof(s));
    s.packets = S.n; s.sync_errors = g[kTsTSync]; s.tei = g[kTsTTei]; s.kept = g[kTsTKept];
    s.valid = tot[0]; s.null_packets = tot[1]; s.cc_errors = tot[2]; s.cc_repeats = tot[3]; s.cc_missing = tot[4]; s.discontinuities = tot[5];
    s.pids_seen = seen; s.pids_listed = seen < A.max_pids ? seen : A.max_pids;
    s.pcr_pid = -1;
    if (g[kTsTNotPcrKey]) {
      const unsigned pid = (unsigned)(~g[kTsTNotPcrKey]) & kTsPidMask;
      const unsigned *C = st + kTsStateCounters + (size_t)pid * kTsCounters;
      s.pcr_pid = (int)pid; s.pcr_count = C[kTsCPcrCount];
      s.pcr_first_packet = ~C[kTsCNotPcrFirst]; s.pcr_last_packet = C[kTsCPcrLast];
      s.pcr_first = ts_pcr_value(S.ts + s.pcr_first_packet * kTsPacket);
      s.pcr_last = ts_pcr_value(S.ts + s.pcr_last_packet * kTsPacket);
    }
    A.sum[si] = s;
  }
}

__global__ __launch_bounds__(kTsThreads) void k_ts_copy(ts_args A) {
  const unsigned si = blockIdx.y, T = A.tile, t = threadIdx.x;
  const ts_stream S = A.st[si];
  const unsigned long long p0 = (unsigned long long)blockIdx.x * T;
  if (p0 >= S.n) return;
  const size_t tile_at = (size_t)si * A.max_tiles + blockIdx.x;
  const unsigned kept = A.hdr[tile_at].y;
  if (!kept) return;
  const unsigned off = A.koff[tile_at];
  __shared__ unsigned short kl[kTsMaxTile];
  for (unsigned r = t; r < kept; r += kTsThreads) kl[r] = A.klist[tile_at * T + r];
  __syncthreads();
  const unsigned *in = reinterpret_cast<const unsigned *>(S.ts) + p0 * kTsDwords;
  unsigned *out = reinterpret_cast<unsigned *>(A.out + (size_t)si * A.out_stride) + (size_t)off * kTsDwords;
  const unsigned total = kept * kTsDwords;
  for (unsigned q = t; q < total; q += kTsThreads) {
    const unsigned r = q / kTsDwords, w = q - r * kTsDwords;
    out[q] = in[(unsigned)kl[r] * kTsDwords + w];
  }
  if (A.index)
    for (unsigned r = t; r < kept; r += kTsThreads) A.index[(size_t)si * A.max_packets + off + r] = (unsigned)(p0 + kl[r]);
}

}  // namespace

struct lsdr_ts_batch {
  lsdr_ctx *ctx = nullptr;
  lsdr_ts_batch_cfg cfg{};
  ts_args A{};
  in_run<ts_stream> run;
  lsdr_ts_summary *h_sum = nullptr;                                       // pinned: [B] summaries, then h_pids = [B][max_pids] records,
  lsdr_ts_pid *h_pids = nullptr;                                          //         one block like A.sum / A.pids: one copy per run
  size_t rec_bytes = 0;
  unsigned char *h_keep = nullptr, *d_keep = nullptr;                     // pinned / device: the rule's PID bitmaps
  unsigned *d_index = nullptr;
  hipStream_t dl = nullptr;                                               // downloads of the kept packets
  hipEvent_t ev_dl = nullptr;
  bool dl_pending = false, run_rule = false, run_index = false, filtered = false;   // filtered: the last run waited for had a rule
};

extern "C" {

void lsdr_ts_batch_destroy(lsdr_ts_batch *b) {
  if (!b) return;
  (void)hipStreamSynchronize(b->ctx->stream);
  if (b->dl) { (void)hipStreamSynchronize(b->dl); (void)hipStreamDestroy(b->dl); }
  if (b->ev_dl) (void)hipEventDestroy(b->ev_dl);
  b->run.destroy();
  lsdr_in_free({b->A.state, b->A.hdr, b->A.list, b->A.sum, b->d_keep, b->A.klist, b->A.koff, b->A.out, b->d_index}, {b->h_sum, b->h_keep});
  delete b;
}

static int tb_build(lsdr_ts_batch *b) {
  lsdr_ctx *c = b->ctx;
  ts_args &A = b->A;
  const size_t B = (size_t)b->cfg.n_streams;
  // packets per tile.  LSDR_TS_BATCH_TILE (256, 512, 768 or 1024; read per create) is a tuning and test hook: the records do not depend on it
  A.tile = kTsMaxTile;
  if (const char *g = getenv("LSDR_TS_BATCH_TILE")) {
    const int v = atoi(g);
    if (v >= (int)kTsThreads && v <= (int)kTsMaxTile && v % (int)kTsThreads == 0) A.tile = (unsigned)v;
  }
  A.max_packets = b->cfg.max_packets;
  A.max_tiles = (unsigned)((b->cfg.max_packets + A.tile - 1u) / A.tile);
  if (!A.max_tiles) A.max_tiles = 1;
  A.max_pids = b->cfg.max_pids ? b->cfg.max_pids : 64u;
  LSDR_HIP(hipSetDevice(c->device));
  LSDR_TRY(b->run.create(B));
  LSDR_HIP(hipStreamCreateWithFlags(&b->dl, hipStreamNonBlocking));
  LSDR_HIP(hipEventCreateWithFlags(&b->ev_dl, hipEventDisableTiming));
  b->rec_bytes = B * sizeof(lsdr_ts_summary) + B * A.max_pids * sizeof(lsdr_ts_pid);
  LSDR_HIP(hipHostMalloc((void **)&b->h_sum, b->rec_bytes, hipHostMallocDefault));
  memset(b->h_sum, 0, b->rec_bytes);
  b->h_pids = reinterpret_cast<lsdr_ts_pid *>(b->h_sum + B);
  LSDR_HIP(hipMalloc((void **)&A.state, B * kTsStateWords * sizeof(unsigned)));
  LSDR_HIP(hipMalloc((void **)&A.hdr, B * A.max_tiles * sizeof(uint2)));
  LSDR_HIP(hipMalloc((void **)&A.list, B * A.max_tiles * A.tile * sizeof(uint2)));
  LSDR_HIP(hipMalloc((void **)&A.sum, b->rec_bytes));
  A.pids = reinterpret_cast<lsdr_ts_pid *>(A.sum + B);
  A.st = b->run.d_caps;
  return LSDR_OK;
}

// the filter's buffers, at the first run with a rule (a census-only object never pays for them)
static int tb_filter_buffers(lsdr_ts_batch *b, bool want_index) {
  ts_args &A = b->A;
  const size_t B = (size_t)b->cfg.n_streams;
  if (!A.out) {
    A.out_stride = (A.max_packets * kTsPacket + 255u) & ~(size_t)255u;
    if (!A.out_stride) A.out_stride = 256;
    LSDR_HIP(hipHostMalloc((void **)&b->h_keep, B * (kTsPids / 8u), hipHostMallocDefault));
    LSDR_HIP(hipMalloc((void **)&b->d_keep, B * (kTsPids / 8u)));
    LSDR_HIP(hipMalloc((void **)&A.klist, B * A.max_tiles * A.tile * sizeof(unsigned short)));
    LSDR_HIP(hipMalloc((void **)&A.koff, B * A.max_tiles * sizeof(unsigned)));
    LSDR_HIP(hipMalloc((void **)&A.out, B * A.out_stride));
  }
  if (want_index && !b->d_index) LSDR_HIP(hipMalloc((void **)&b->d_index, B * (A.max_packets ? A.max_packets : 1u) * sizeof(unsigned)));
  return LSDR_OK;
}

int lsdr_ts_batch_create(lsdr_ctx *c, const lsdr_ts_batch_cfg *cfg, lsdr_ts_batch **out) {
  LSDR_ARG(c && cfg && out);
  if (cfg->n_streams < 1 || cfg->n_streams > 65535) { lsdr_set_error("ts_batch: n_streams must be 1 to 65535 (got %d)", cfg->n_streams); return LSDR_E_ARG; }
  if (cfg->max_pids > kTsPids) { lsdr_set_error("ts_batch: max_pids must be at most 8192 (got %u)", cfg->max_pids); return LSDR_E_ARG; }
  for (int i = 0; i < 8; ++i)
    if (cfg->reserved[i]) { lsdr_set_error("ts_batch: lsdr_ts_batch_cfg.reserved must be 0"); return LSDR_E_ARG; }
  // (packet indices and the per-PID counters are 32 bits wide)
  if ((unsigned long long)cfg->max_packets >= (1ull << 32)) { lsdr_set_error("ts_batch: max_packets must be below 2^32 (got %zu)", cfg->max_packets); return LSDR_E_UNSUPPORTED; }
  lsdr_ts_batch *b = new lsdr_ts_batch();
  b->ctx = c; b->cfg = *cfg;
  const int rc = tb_build(b);
  if (rc) { lsdr_ts_batch_destroy(b); return rc; }
  *out = b;
  return LSDR_OK;
}

unsigned lsdr_ts_batch_tile(const lsdr_ts_batch *b) { return b ? b->A.tile : 0u; }

int lsdr_ts_batch_run_async(lsdr_ts_batch *b, const uint8_t *const *ts_dev, const uint64_t *n_packets, const lsdr_ts_rule *rule) {
  LSDR_ARG(b && ts_dev && n_packets);
  const unsigned B = (unsigned)b->cfg.n_streams;
  for (unsigned i = 0; i < B; ++i) {
    if (n_packets[i] > b->cfg.max_packets) { lsdr_set_error("ts_batch: stream %u: n_packets %llu exceeds max_packets %zu", i, (unsigned long long)n_packets[i], b->cfg.max_packets); return LSDR_E_ARG; }
    if (n_packets[i] && !ts_dev[i]) { lsdr_set_error("ts_batch: stream %u has packets and no pointer", i); return LSDR_E_ARG; }
    if (n_packets[i] && (size_t)ts_dev[i] % 4u) { lsdr_set_error("ts_batch: stream %u: the pointer is not aligned to 4 bytes", i); return LSDR_E_ARG; }
  }
  if (rule) {
    if (rule->drop & ~(unsigned)(LSDR_TS_DROP_NULL | LSDR_TS_DROP_TEI | LSDR_TS_DROP_SYNC)) { lsdr_set_error("ts_batch: unknown drop bits 0x%x", rule->drop); return LSDR_E_ARG; }
    for (int k = 0; k < 4; ++k)
      if (rule->reserved[k]) { lsdr_set_error("ts_batch: lsdr_ts_rule.reserved must be 0"); return LSDR_E_ARG; }
  }
  LSDR_TRY(b->run.idle("ts_batch", "lsdr_ts_batch_wait"));
  lsdr_ctx *c = b->ctx;
  ts_args &A = b->A;
  LSDR_HIP(hipSetDevice(c->device));
  if (rule) LSDR_TRY(tb_filter_buffers(b, rule->want_index != 0));
  unsigned long long longest = 0;                                         // the grids are sized for it; a shorter stream's workgroups leave at once
  for (unsigned i = 0; i < B; ++i) {
    ts_stream &S = b->run.h_caps[i];
    S.n = n_packets[i];
    S.ts = S.n ? ts_dev[i] : nullptr;
    if (S.n > longest) longest = S.n;
  }
  LSDR_TRY(b->run.upload(c->stream));
  A.rule = rule ? 1u : 0u;
  A.drop = rule ? rule->drop : 0u;
  A.keep = nullptr;
  A.index = rule && rule->want_index ? b->d_index : nullptr;
  if (rule && rule->keep_pids) {
    memcpy(b->h_keep, rule->keep_pids, (size_t)B * (kTsPids / 8u));       // (the last run was waited for: its copy has left h_keep)
    LSDR_HIP(hipMemcpyAsync(b->d_keep, b->h_keep, (size_t)B * (kTsPids / 8u), hipMemcpyHostToDevice, c->stream));
    A.keep = b->d_keep;
  }
  // the kernels that write the output wait for a download of the last run's that is still pending
  if (rule && b->dl_pending) LSDR_HIP(hipStreamWaitEvent(c->stream, b->ev_dl, 0));
  LSDR_HIP(hipMemsetAsync(A.state, 0, (size_t)B * kTsStateWords * sizeof(unsigned), c->stream));
  const dim3 grid((unsigned)((longest + A.tile - 1u) / A.tile), B);
  if (longest) {
    hipLaunchKernelGGL(k_ts_scan, grid, dim3(kTsThreads), 0, c->stream, A);
    hipLaunchKernelGGL(k_ts_stitch, dim3(B), dim3(kTsThreads), 0, c->stream, A);
  }
  hipLaunchKernelGGL(k_ts_report, dim3(B), dim3(kTsThreads), 0, c->stream, A);
  if (rule && longest) hipLaunchKernelGGL(k_ts_copy, grid, dim3(kTsThreads), 0, c->stream, A);
  LSDR_HIP(hipGetLastError());
  LSDR_HIP(hipMemcpyAsync(b->h_sum, A.sum, b->rec_bytes, hipMemcpyDeviceToHost, c->stream));
  b->run_rule = rule != nullptr;
  b->run_index = rule && rule->want_index;
  b->filtered = false;
  return b->run.mark(c->stream);
}

int lsdr_ts_batch_wait(lsdr_ts_batch *b, lsdr_ts_summary *out) {
  LSDR_ARG(b);
  LSDR_TRY(b->run.wait("ts_batch"));
  b->filtered = b->run_rule;
  if (out) memcpy(out, b->h_sum, (size_t)b->cfg.n_streams * sizeof(lsdr_ts_summary));
  return LSDR_OK;
}

int lsdr_ts_batch_pids(lsdr_ts_batch *b, int i, lsdr_ts_pid *out, unsigned cap, unsigned *n) {
  LSDR_ARG(b && n);
  if (i < 0 || i >= b->cfg.n_streams) { lsdr_set_error("ts_batch: no stream %d (n_streams %d)", i, b->cfg.n_streams); return LSDR_E_ARG; }
  LSDR_TRY(b->run.idle("ts_batch", "lsdr_ts_batch_wait"));
  const unsigned listed = b->h_sum[i].pids_listed;
  *n = listed;
  if (listed > cap || (listed && !out)) { lsdr_set_error("ts_batch: stream %d lists %u PIDs, the table given has room for %u", i, listed, cap); return LSDR_E_ARG; }
  if (listed) memcpy(out, b->h_pids + (size_t)i * b->A.max_pids, (size_t)listed * sizeof(lsdr_ts_pid));
  return LSDR_OK;
}

const uint8_t *lsdr_ts_batch_out_dev(const lsdr_ts_batch *b, int i) {
  return b && b->A.out && i >= 0 && i < b->cfg.n_streams ? b->A.out + (size_t)i * b->A.out_stride : nullptr;
}

const uint32_t *lsdr_ts_batch_index_dev(const lsdr_ts_batch *b, int i) {
  return b && b->run_index && b->d_index && i >= 0 && i < b->cfg.n_streams ? b->d_index + (size_t)i * b->A.max_packets : nullptr;
}

int lsdr_ts_batch_download_async(lsdr_ts_batch *b, uint8_t *const *host, size_t cap_bytes) {
  LSDR_ARG(b && host);
  if (b->run.in_flight || !b->filtered) { lsdr_set_error("ts_batch: download before the lsdr_ts_batch_wait of a run with a rule"); return LSDR_E_ARG; }
  const unsigned B = (unsigned)b->cfg.n_streams;
  for (unsigned i = 0; i < B; ++i) {
    const size_t bytes = (size_t)b->h_sum[i].kept * kTsPacket;
    if (bytes > cap_bytes) { lsdr_set_error("ts_batch: stream %u keeps %zu bytes, the host buffer has %zu", i, bytes, cap_bytes); return LSDR_E_ARG; }
    if (bytes && !host[i]) { lsdr_set_error("ts_batch: stream %u keeps %zu bytes and has no host pointer", i, bytes); return LSDR_E_ARG; }
  }
  LSDR_HIP(hipSetDevice(b->ctx->device));
  for (unsigned i = 0; i < B; ++i) {
    const size_t bytes = (size_t)b->h_sum[i].kept * kTsPacket;
    if (bytes) LSDR_HIP(hipMemcpyAsync(host[i], b->A.out + (size_t)i * b->A.out_stride, bytes, hipMemcpyDeviceToHost, b->dl));
  }
  LSDR_HIP(hipEventRecord(b->ev_dl, b->dl));
  b->dl_pending = true;
  return LSDR_OK;
}

int lsdr_ts_batch_download_wait(lsdr_ts_batch *b) {
  LSDR_ARG(b);
  if (b->dl_pending) LSDR_HIP(hipEventSynchronize(b->ev_dl));
  b->dl_pending = false;
  return LSDR_OK;
}

}  // extern "C"
