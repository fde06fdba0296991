// leansdr_amd/csrc/ts_stitch_device.h — what lsdr_ts_stitch's kernels and its host side share (ts_stitch.hip): a packet's 64-bit key, the
// packing of a run into one comparable word, and the kernels' arguments.  Plain C++ on values.  The definition: include/lsdr_hip.h.
#ifndef LSDR_TS_STITCH_DEVICE_H
#define LSDR_TS_STITCH_DEVICE_H
#include "lsdr_internal.h"

#define ST_HD __host__ __device__ __forceinline__

constexpr unsigned kStPacket = 188, kStDwords = 47, kStNullPid = 0x1fff, kStThreads = 256;
constexpr unsigned kStKeyTile = 64;                                       // packets per workgroup of the key pass
constexpr unsigned kStChunk = 512;                                        // rows of the match matrix per LDS stage of the span pass
constexpr unsigned kStDiags = 64;                                         // diagonals per workgroup of the verify pass
constexpr unsigned kStMaxWindow = 65535;                                  // (a run's two places are 16 bits each in st_pack)

// What dword w (0 … 46) of a packet adds to its key: splitmix64's finaliser over (w + 1, value).  The key is the sum over the packet's
// dwords — any order, so the pieces of a packet that two lanes hold add up — with bit 0 replaced by the null flag.  Equal bytes give
// equal keys; the reverse is never assumed (k_stitch_verify compares the bytes).
ST_HD unsigned long long st_mix(unsigned v, unsigned w) {
  unsigned long long x = ((unsigned long long)(w + 1u) << 32) | v;
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}
// a packet's first dword (little-endian: bytes 0 … 3) → whether its PID is 0x1fff
ST_HD unsigned st_is_null(unsigned w0) { return ((((w0 >> 8) & 0x1fu) << 8) | ((w0 >> 16) & 255u)) == kStNullPid ? 1u : 0u; }

// A run (L, a, b) as one word whose maximum is the join: the longest, then the smallest a, then the smallest b.  0: none.
ST_HD unsigned long long st_pack(unsigned L, unsigned a, unsigned b) {
  return ((unsigned long long)L << 32) | ((unsigned long long)(0xffffu - a) << 16) | (unsigned long long)(0xffffu - b);
}
ST_HD unsigned st_run(unsigned long long v) { return (unsigned)(v >> 32); }
ST_HD unsigned st_a(unsigned long long v) { return 0xffffu - ((unsigned)(v >> 16) & 0xffffu); }
ST_HD unsigned st_b(unsigned long long v) { return 0xffffu - ((unsigned)v & 0xffffu); }

struct st_stream {
  const unsigned char *ts;         // 4-byte aligned; null where n is 0
  unsigned long long n;            // packets
};
struct st_args {
  const st_stream *st;             // [P]
  unsigned long long *keys;        // [P][2][W]: the keys of every stream's last min(W, n) packets, then of its first min(W, n)
  uint2 *span;                     // [P − 1][2W]: per diagonal of a pair, the rows [x, y) that hold its key runs of at least M; y = 0: none
  unsigned long long *best;        // [P − 1]: st_pack of the pair's join, zeroed in front of every run
  lsdr_ts_join *joins;             // [P − 1]
  lsdr_ts_keep *keep;              // [P]
  unsigned long long *total;       // packets kept
  unsigned char *out;
  unsigned P, W, M, const_key;
};
#endif
