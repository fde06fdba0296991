// leansdr_amd/csrc/hsb_device.h — device side of lsdr_hs_batch (include/lsdr_hip.h): leandvb's `--hs` graph for B independent cu8 captures in
// shared launches (included inside hs.hip's anonymous namespace, behind fq_chunk / hs_word / rx_tiling.h).  blockIdx.y = capture everywhere;
// every capture starts from the constructed state, so no state is carried and nothing is read back between the kernels.  cu8 only, and it
// stays so: `--hs requires --u8` in the reference too (leandvb.cc:773-774); the other sample formats belong to lsdr_capture_any_create.
//
//   k_hsb_reset     clears the per-capture records (a second batch sees nothing of the first)
//   k_hsb_tiles     fast_qpsk_receiver<u8> time-tiled, one lane per tile, fq_chunk's arithmetic.  Tile 0 (a block of its own) runs the
//                   reference's receiver from its constructed state: its symbols are the reference's.  Tile j ≥ 1 starts `warm` chunks
//                   early at mu = phase = 0 with the constructed frequency word, clamped to ± freq_window.  Body symbols are staged
//                   TRANSPOSED, four to a dword: dword r of tile j at stage[r·pitch + j] — the 64 tiles of a wavefront reach "four more
//                   symbols" within a few iterations of each other, so their stores fall into the same 256 bytes.  The last 16 warm-up
//                   and body symbols ride in the tile's record for the seam vote (rx_tile_info_h).
//   k_hsb_seam      rx_seam_h_body per capture
//   k_hsb_compact   64 tiles × 64 staging rows per workgroup: the rows come in coalesced, turn in LDS, and every tile's symbols leave as
//                   consecutive bytes of the capture's symbol array, relabelled by the accumulated quadrant step; the capture's total
//                   and seam counters go to its record in device memory
//   k_hsb_score     dvb_deconvol_sync::run's alignment search on the chunks ≡ 0 (mod P): the four error counts of a resync chunk use only
//                   the second half of its words (convolutional.h:184), i.e. no carried history — a wavefront half per chunk reduces them and
//                   writes the first arg-min.  For a freshly constructed object the alignment in force while chunk c is decoded is then
//                       c == 0 ? 0 : best[(c − 1) / P]
//                   a pure function of the symbol stream (dvb.h:632-657: `locked` changes behind a resync chunk, where all four ran).
//   k_hsb_decode    one thread per 32-bit output word with that alignment, straight into the FEC tail's byte buffer; the first thread of
//                   a capture leaves {bytes, alignment at the end} in the tail's record.
#ifndef LSDR_HSB_DEVICE_H
#define LSDR_HSB_DEVICE_H

struct hsb_rec {                   // per capture, device memory; copied to pinned memory in front of the tail (which only reads it)
  unsigned long long total;        // symbols in the capture's array (the tail's `nsym`)
  unsigned ndup, nmiss, nbad, pad;
  unsigned long long chunks;       // deconvolver chunks decoded
};

struct hsb_each {                  // per capture and run, device memory (uploaded by run_async): what lsdr_capture_each sets
  unsigned long long total_chunks; // 128-sample chunks of this capture
  unsigned n_tiles, pad;
  long long freqw, min_freqw, max_freqw;   // the constructed fq_state under set_freq(its tune)
};

struct hsb_args {
  fq_tiled_args t;                 // tables, loop constants, tile lengths, freq_window (in / stage / info / state / total_chunks / n_tiles unused)
  fq_state st0;                    // fast_qpsk_receiver as constructed, but for what set_freq sets (hsb_each)
  const hsb_each *each;            // [B]
  const unsigned char *const *in;  // [B] cu8 captures
  unsigned *stage;                 // [B][rows][pitch] dwords
  unsigned rows, pitch;
  rx_tile_info_h *info; rx_tile_fix *fix; rx_seam_part *part;
  unsigned tiles_cap, parts_cap;   // records per capture
  unsigned char *sym;              // [B][sym_stride] compacted symbols
  unsigned long long sym_stride, sym_cap;
  hsb_rec *rec;
  const uint8_t *relabel;
  // deconvolver
  unsigned char *best;             // [B][best_stride] first arg-min of every resync chunk
  unsigned long long best_stride;
  unsigned char *const *bytes;     // [B] the tail's byte buffers
  unsigned long long byte_room;
  lsdr_tail_vit *vit;              // [B] the tail's records
  int P;
};

__global__ __launch_bounds__(64) void k_hsb_reset(hsb_args A, unsigned n) {
  const unsigned i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  hsb_rec z; z.total = 0; z.ndup = z.nmiss = z.nbad = z.pad = 0; z.chunks = 0;
  A.rec[i] = z;
  lsdr_tail_vit v; v.bytes = 0; v.alignment = 0; v.pad = 0;
  A.vit[i] = v;
}

// LDSRECT: the 128 KiB `rect` table in LDS, one workgroup of kHsbLdsWaves wavefronts (four per SIMD) per CU (measured experiment, profiles/hs_batch/NOTES.md)
constexpr int kHsbLdsWaves = 16;
template <bool LDSRECT>
__device__ __forceinline__ void hsb_tiles_body(const hsb_args &A, const unsigned short *rect_lds) {
  const fq_tiled_args &a0 = A.t;
  const unsigned cap = blockIdx.y;
  unsigned j;
  if (LDSRECT) {
    // tile 0 is lane 0 of block 0's first wavefront; the other lanes of block 0 take tiles 1 … as everywhere else
    j = blockIdx.x * (unsigned)(kHsbLdsWaves * 64) + threadIdx.x;
  } else {
    if (blockIdx.x == 0) { if (threadIdx.x != 0) return; j = 0; }
    else j = 1u + (blockIdx.x - 1u) * 64u + threadIdx.x;
  }
  const hsb_each each = A.each[cap];
  if (j >= each.n_tiles) return;
  fq_tiled_args a = a0;
  if (LDSRECT) a.rect = rect_lds;
  const unsigned long long first = a.first_chunks, Lc = a.tile_chunks, Wc = a.warm_chunks, total = each.total_chunks;
  unsigned long long cb, c0, c1;
  if (j == 0) { cb = 0; c0 = 0; c1 = first; }
  else { c0 = first + (unsigned long long)(j - 1) * Lc; c1 = c0 + Lc; cb = c0 - Wc; }
  if (c1 > total) c1 = total;
  fq_state s = A.st0;
  s.freqw = each.freqw; s.min_freqw = each.min_freqw; s.max_freqw = each.max_freqw;
  rx_tile_info_h ti;
  ti.has_pre = 0; ti.n_warm = 0; ti.warm_tail = 0; ti.body_tail = 0; ti.mu_begin = ti.phase_begin = 0.f;
  const long long f_lo = s.freqw - a.freq_window, f_hi = s.freqw + a.freq_window;
  unsigned *po = A.stage + (unsigned long long)cap * A.rows * A.pitch + j;
  const unsigned rows = A.rows;
  const unsigned long long pitch = A.pitch;
  unsigned cnt = 0, got = 0, sacc = 0, tail = 0;
  const unsigned short *in16 = reinterpret_cast<const unsigned short *>(A.in[cap]);
  for (unsigned long long c = cb; c < c1; ++c) {
    const bool body = c >= c0;
    if (c == c0) {
      ti.mu_begin = s.mu; ti.phase_begin = (float)(s.phase & 0xffffu);
      ti.warm_tail = tail; ti.n_warm = got < 16u ? got : 16u; ti.has_pre = got ? 1u : 0u;
    }
    auto emit = [&](unsigned char v) {
      tail = (tail << 2) | (unsigned)(v & 3u);
      if (body) {
        sacc |= (unsigned)v << (8u * (cnt & 3u));
        if ((cnt & 3u) == 3u) { if ((cnt >> 2) < rows) po[(unsigned long long)(cnt >> 2) * pitch] = sacc; sacc = 0u; }
        ++cnt;
      }
    };
    const int avail = (int)((total - c) * kChunk + 1 < 1024 ? (total - c) * kChunk + 1 : 1024);
    const int n = j == 0 ? fq_chunk<false>(a, s, in16 + c * kChunk, avail, emit) : fq_chunk<true>(a, s, in16 + c * kChunk, avail, emit, f_lo, f_hi);
    if (!body) got += (unsigned)n;
  }
  if ((cnt & 3u) && (cnt >> 2) < rows) po[(unsigned long long)(cnt >> 2) * pitch] = sacc;
  if (cnt > rows * 4u) cnt = rows * 4u;        // (cannot happen: a chunk emits at most sym_per_chunk symbols)
  ti.mu_end = s.mu; ti.phase_end = (float)(s.phase & 0xffffu); ti.count = cnt; ti.body_tail = tail;
  A.info[(unsigned long long)cap * A.tiles_cap + j] = ti;
}

__global__ __launch_bounds__(64) void k_hsb_tiles(hsb_args A) { hsb_tiles_body<false>(A, nullptr); }

__global__ __launch_bounds__(kHsbLdsWaves * 64) void k_hsb_tiles_lds(hsb_args A) {
  extern __shared__ __attribute__((aligned(16))) unsigned short s_rect[];      // [65536]
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(A.t.rect);
    uint4 *dst = reinterpret_cast<uint4 *>(s_rect);
    for (unsigned i = threadIdx.x; i < 65536u * 2u / 16u; i += kHsbLdsWaves * 64) dst[i] = src[i];
  }
  __syncthreads();
  hsb_tiles_body<true>(A, s_rect);
}

__global__ __launch_bounds__(kSeamBlock) void k_hsb_seam(hsb_args A) {
  const unsigned cap = blockIdx.y, n_tiles = A.each[cap].n_tiles;
  if (blockIdx.x * kSeamBlock >= n_tiles) return;
  rx_seam_h_body(A.info + (unsigned long long)cap * A.tiles_cap, A.fix + (unsigned long long)cap * A.tiles_cap, n_tiles, A.t.omega, 4,
                 16384.0f, A.part + (unsigned long long)cap * A.parts_cap, A.relabel);
}

constexpr unsigned kHsbTile = 64;            // tiles and staging rows per compaction workgroup
static_assert(kSeamBlock % kHsbTile == 0, "the tiles of a compaction workgroup share their seam block");
__global__ __launch_bounds__(256) void k_hsb_compact(hsb_args A, unsigned row_blocks) {
  const unsigned cap = blockIdx.y, n_tiles = A.each[cap].n_tiles;
  const unsigned grp = blockIdx.x / row_blocks, rb = blockIdx.x - grp * row_blocks;
  const unsigned j0 = grp * kHsbTile, r0 = rb * kHsbTile;
  if (j0 >= n_tiles) return;
  const rx_tile_info_h *info = A.info + (unsigned long long)cap * A.tiles_cap;
  const rx_tile_fix *fix = A.fix + (unsigned long long)cap * A.tiles_cap;
  const rx_seam_part *part = A.part + (unsigned long long)cap * A.parts_cap;
  const unsigned *stage = A.stage + (unsigned long long)cap * A.rows * A.pitch;
  unsigned char *out = A.sym + (unsigned long long)cap * A.sym_stride;
  const unsigned nparts = (n_tiles + kSeamBlock - 1) / kSeamBlock, mypart = j0 / kSeamBlock;
  const unsigned tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  if (blockIdx.x == 0 && tid == 0) {
    hsb_rec r; r.total = 0; r.ndup = r.nmiss = r.nbad = r.pad = 0; r.chunks = 0;
    for (unsigned i = 0; i < nparts; ++i) { r.total += part[i].cnt; r.ndup += part[i].ndup; r.nmiss += part[i].nmiss; r.nbad += part[i].nbad; }
    if (r.total > A.sym_cap) r.total = A.sym_cap;
    A.rec[cap] = r;
  }
  __shared__ unsigned s_cnt[kHsbTile], s_skip[kHsbTile], s_map[kHsbTile], s_max;
  __shared__ long long s_Q[kHsbTile];
  __shared__ unsigned s_t[kHsbTile][kHsbTile + 1];
  unsigned long long base = 0;
  unsigned brot = 0;
  for (unsigned i = 0; i < mypart; ++i) { base += part[i].cnt; brot += part[i].rot; }      // (uniform; a handful of records)
  if (tid == 0) s_max = 0;
  __syncthreads();
  if (tid < kHsbTile) {
    unsigned cnt = 0, skip = 0, map4 = 0;
    long long Q = 0;
    if (j0 + tid < n_tiles) {
      const rx_tile_fix f = fix[j0 + tid];
      const rx_tile_info_h ti = info[j0 + tid];
      cnt = ti.count;
      skip = f.drop_first ? 1u : 0u;
      const unsigned ins = f.insert_pre ? 1u : 0u;
      const long long D = (long long)(base + f.out_offset);
      Q = D + (long long)ins - (long long)skip;                         // body symbol k goes to out[Q + k]
      map4 = hs2_map4(A.relabel + ((f.rot + brot) & 3u) * 256);
      if (ins && rb == 0 && (unsigned long long)D < A.sym_cap)          // the warm-up's last symbol belongs to this tile
        out[D] = (unsigned char)((map4 >> (2 * (ti.warm_tail & 3u))) & 3u);
      atomicMax(&s_max, cnt);
    }
    s_cnt[tid] = cnt; s_skip[tid] = skip; s_map[tid] = map4; s_Q[tid] = Q;
  }
  __syncthreads();
  if (r0 * 4u >= s_max) return;                                         // (uniform)
  const unsigned cnt_l = s_cnt[lane];
#pragma unroll 4
  for (unsigned r = wv; r < kHsbTile; r += 4) {                         // staging row r0 + r: 64 consecutive dwords
    const unsigned row = r0 + r;
    if (row * 4u < cnt_l) s_t[lane][r] = stage[(unsigned long long)row * A.pitch + j0 + lane];
  }
  __syncthreads();
  for (unsigned t = wv; t < kHsbTile; t += 4) {                         // tile j0 + t: 256 consecutive symbols, 64 bytes per store
    const unsigned cnt = s_cnt[t], skip = s_skip[t], map4 = s_map[t];
    const long long Q = s_Q[t];
#pragma unroll
    for (unsigned u = 0; u < 4; ++u) {
      const unsigned kl = u * 64u + lane, k = r0 * 4u + kl;
      if (k < cnt && k >= skip) {
        const unsigned v = (s_t[t][kl >> 2] >> (8u * (kl & 3u))) & 3u;
        const long long d = Q + (long long)k;
        if (d >= 0 && (unsigned long long)d < A.sym_cap) out[d] = (unsigned char)((map4 >> (2 * v)) & 3u);
      }
    }
  }
}

// ---- dvb_deconvol_sync<u8>, batched
__device__ __forceinline__ unsigned long long hsb_chunks(const hsb_args &A, unsigned cap) {
  unsigned long long chunks = A.rec[cap].total / kDcSyms;              // while in.readable() >= 512 && out.writable() >= 64, dvb.h:634-635
  const unsigned long long room = A.byte_room / kDcBytes;
  return chunks < room ? chunks : room;
}

// the I and Q bit streams (after the alignment's symbol map) of 32 symbols held in two uint4: oldest symbol in bit 31
__device__ __forceinline__ void hsb_iq32(const uint4 &lo, const uint4 &hi, unsigned mI, unsigned mQ, unsigned &I, unsigned &Q) {
  const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  I = 0; Q = 0;
#pragma unroll
  for (int d = 0; d < 8; ++d) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const unsigned s = (w[d] >> (8 * b)) & 3u;
      I = (I << 1) | ((mI >> s) & 1u);
      Q = (Q << 1) | ((mQ >> s) & 1u);
    }
  }
}
// hs_word on bit streams: histI after the symbol that produces output bit `bit` is the 32-symbol window ending there, (I64 >> bit)
__device__ __forceinline__ void hsb_word(unsigned long long I64, unsigned long long Q64, unsigned &wd, unsigned &we) {
  const unsigned long long PD = 0x3baull, PE = 0x38f70ull;
  wd = 0; we = 0;
#pragma unroll
  for (int bit = 0; bit < 32; ++bit) {
    if (PD & (2ull << (2 * bit))) wd ^= (unsigned)(I64 >> bit);
    if (PD & (1ull << (2 * bit))) wd ^= (unsigned)(Q64 >> bit);
    if (PE & (2ull << (2 * bit))) we ^= (unsigned)(I64 >> bit);
    if (PE & (1ull << (2 * bit))) we ^= (unsigned)(Q64 >> bit);
  }
}
__device__ __forceinline__ void hsb_masks(int s, unsigned &mI, unsigned &mQ) {
  mI = 0; mQ = 0;
#pragma unroll
  for (int v = 0; v < 4; ++v) { const unsigned iq = c_hs_lut[s][v]; mI |= (iq >> 1) << v; mQ |= (iq & 1u) << v; }
}
// word w of chunk c with alignment s; first: the stream's first word (history as constructed: zero)
__device__ __forceinline__ void hsb_word_at(const unsigned char *sym, unsigned long long c, int w, int s, bool first, unsigned &wd, unsigned &we) {
  const uint4 *p = reinterpret_cast<const uint4 *>(sym + c * kDcSyms + (unsigned)w * 32u);      // (32-byte aligned)
  unsigned mI, mQ, hI = 0, hQ = 0, I, Q;
  hsb_masks(s, mI, mQ);
  if (!first) hsb_iq32(p[-2], p[-1], mI, mQ, hI, hQ);
  hsb_iq32(p[0], p[1], mI, mQ, I, Q);
  hsb_word(((unsigned long long)hI << 32) | I, ((unsigned long long)hQ << 32) | Q, wd, we);
}

__global__ __launch_bounds__(256) void k_hsb_score(hsb_args A) {
  const unsigned cap = blockIdx.y;
  const unsigned long long chunks = hsb_chunks(A, cap);
  const unsigned long long n_resync = (chunks + (unsigned)A.P - 1) / (unsigned)A.P;
  if ((unsigned long long)blockIdx.x * 8 >= n_resync) return;
  const unsigned char *sym = A.sym + (unsigned long long)cap * A.sym_stride;
  unsigned char *best = A.best + (unsigned long long)cap * A.best_stride;
  const unsigned sub = threadIdx.x & 31u;                               // (alignment, word 8 … 15) of one resync chunk: half a wavefront
  const int s = (int)(sub >> 3), w = 8 + (int)(sub & 7u);
  const unsigned long long groups = ((n_resync + 7) / 8) * 8;           // whole workgroups: every lane reaches the shuffles
  for (unsigned long long r = (unsigned long long)blockIdx.x * 8 + (threadIdx.x >> 5); r < groups; r += (unsigned long long)gridDim.x * 8) {
    int e = 0;
    if (r < n_resync) {
      unsigned wd, we;
      hsb_word_at(sym, r * (unsigned)A.P, w, s, false, wd, we);          // w ≥ 8: the 32 symbols before the word are inside the chunk
      e = __popc(we);
    }
    e += __shfl_xor(e, 1, 64); e += __shfl_xor(e, 2, 64); e += __shfl_xor(e, 4, 64);
    const int e0 = __shfl(e, (int)(threadIdx.x & 32u) + 0, 64), e1 = __shfl(e, (int)(threadIdx.x & 32u) + 8, 64);
    const int e2 = __shfl(e, (int)(threadIdx.x & 32u) + 16, 64), e3 = __shfl(e, (int)(threadIdx.x & 32u) + 24, 64);
    if (sub == 0 && r < n_resync) {
      int b = 0, eb = e0;                                               // first arg-min, dvb.h:646
      if (e1 < eb) { eb = e1; b = 1; }
      if (e2 < eb) { eb = e2; b = 2; }
      if (e3 < eb) { eb = e3; b = 3; }
      best[r] = (unsigned char)b;
    }
  }
}

__global__ __launch_bounds__(256) void k_hsb_decode(hsb_args A) {
  const unsigned cap = blockIdx.y;
  const unsigned long long chunks = hsb_chunks(A, cap);
  const unsigned char *best = A.best + (unsigned long long)cap * A.best_stride;
  const unsigned P = (unsigned)A.P;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    lsdr_tail_vit v;
    v.bytes = chunks * kDcBytes; v.alignment = chunks ? best[(chunks - 1) / P] : 0u; v.pad = 0;
    A.vit[cap] = v;
    A.rec[cap].chunks = chunks;
  }
  if ((unsigned long long)blockIdx.x * 256 >= chunks * 16) return;
  const unsigned char *sym = A.sym + (unsigned long long)cap * A.sym_stride;
  unsigned *out = reinterpret_cast<unsigned *>(A.bytes[cap]);
  for (unsigned long long idx = (unsigned long long)blockIdx.x * 256 + threadIdx.x; idx < chunks * 16; idx += (unsigned long long)gridDim.x * 256) {
    const unsigned long long c = idx >> 4;
    const int w = (int)(idx & 15);
    const int s = c ? (int)best[(c - 1) / P] : 0;
    unsigned wd, we;
    hsb_word_at(sym, c, w, s, idx == 0, wd, we);
    out[idx] = __builtin_bswap32(wd);                                   // bytes MSB first (convolutional.h:186-190)
  }
}

#endif  // LSDR_HSB_DEVICE_H
