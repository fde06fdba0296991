// leansdr_amd/csrc/ts_batch_device.h — what lsdr_ts_batch's kernels and its host side share (ts_batch.hip): a packet's 4-byte descriptor,
// the continuity rule on a pair of descriptors, the layout of the per-PID counters and the kernels' arguments.  Plain C++ on values: the
// rules are callable from a kernel and from the host.  The definition: include/lsdr_hip.h.
#ifndef LSDR_TS_BATCH_DEVICE_H
#define LSDR_TS_BATCH_DEVICE_H
#include "lsdr_internal.h"

#define TS_HD __host__ __device__ __forceinline__

constexpr unsigned kTsPacket = 188, kTsDwords = 47, kTsPids = 8192, kTsNullPid = 0x1fff, kTsBitmapWords = kTsPids / 32u;
constexpr unsigned kTsThreads = 256, kTsMaxTile = 1024, kTsNone = 0xffffffffu;

// A packet's descriptor, from its bytes 0 … 5 (two dwords, little-endian):
//   bits 0-12 pid, 13-16 cc, 17 payload, 18 disc, 19 pusi, 20 scrambled, 21 pcr, 22-23 class (0 valid, 1 bad sync byte, 2 TEI, 3 no packet).
// Of a packet that is not valid only the class is set: nothing else is read from it.
enum { kTsValid = 0, kTsSync = 1, kTsTei = 2, kTsAbsent = 3 };
constexpr unsigned kTsPidMask = 0x1fffu, kTsClassShift = 22, kTsKeyMask = kTsPidMask | (3u << kTsClassShift);
TS_HD unsigned ts_desc(unsigned w0, unsigned w1) {
  const unsigned b0 = w0 & 255u, b1 = (w0 >> 8) & 255u, b2 = (w0 >> 16) & 255u, b3 = w0 >> 24, b4 = w1 & 255u, b5 = (w1 >> 8) & 255u;
  if (b0 != 0x47u) return (unsigned)kTsSync << kTsClassShift;
  if (b1 & 0x80u) return (unsigned)kTsTei << kTsClassShift;
  const unsigned afc = (b3 >> 4) & 3u, af = afc >> 1, af_len = af ? b4 : 0u;
  const unsigned disc = af && af_len > 0u && (b5 & 0x80u) ? 1u : 0u, pcr = af && af_len >= 7u && (b5 & 0x10u) ? 1u : 0u;
  return ((b1 & 0x1fu) << 8) | b2 | ((b3 & 15u) << 13) | ((afc & 1u) << 17) | (disc << 18) | (((b1 >> 6) & 1u) << 19) |
         ((b3 & 0xc0u ? 1u : 0u) << 20) | (pcr << 21);
}
TS_HD unsigned ts_pid(unsigned d) { return d & kTsPidMask; }
TS_HD unsigned ts_class(unsigned d) { return d >> kTsClassShift; }
TS_HD unsigned ts_cc(unsigned d) { return (d >> 13) & 15u; }
TS_HD unsigned ts_payload(unsigned d) { return (d >> 17) & 1u; }
TS_HD unsigned ts_disc(unsigned d) { return (d >> 18) & 1u; }
TS_HD unsigned ts_pusi(unsigned d) { return (d >> 19) & 1u; }
TS_HD unsigned ts_scrambled(unsigned d) { return (d >> 20) & 1u; }
TS_HD unsigned ts_pcr(unsigned d) { return (d >> 21) & 1u; }

// The continuity rule on two consecutive valid packets of one PID (never the null PID): what `cur` adds behind `prev`.
//   bit 0 discontinuities, bit 1 cc_repeats, bit 2 cc_errors, bits 4-7 cc_missing
TS_HD unsigned ts_pair(unsigned prev, unsigned cur) {
  if (ts_disc(cur)) return 1u;
  const unsigned expected = (ts_cc(prev) + ts_payload(cur)) & 15u;
  if (ts_cc(cur) == expected) return 0u;
  if (ts_payload(cur) && ts_cc(cur) == ts_cc(prev)) return 2u;
  return 4u | (((ts_cc(cur) - expected) & 15u) << 4);
}

// The 42-bit PCR of a packet whose descriptor has `pcr`, from its bytes 6 … 11: base·300 + ext in 27 MHz ticks
TS_HD unsigned long long ts_pcr_value(const unsigned char *b) {
  const unsigned long long base = ((unsigned long long)b[6] << 25) | ((unsigned long long)b[7] << 17) | ((unsigned long long)b[8] << 9) |
                                  ((unsigned long long)b[9] << 1) | (unsigned long long)(b[10] >> 7);
  const unsigned ext = ((unsigned)(b[10] & 1u) << 8) | b[11];
  return base * 300ull + ext;
}

// Per stream and PID, twelve 32-bit counters, zeroed in front of every run.  The minima are kept as maxima of the complement: zero means
// "none" for every field.
enum { kTsCPackets = 0, kTsCPusi, kTsCScrambled, kTsCErrors, kTsCRepeats, kTsCMissing, kTsCDisc, kTsCPcrCount,
       kTsCNotFirst /* ~first_packet */, kTsCLast, kTsCNotPcrFirst /* ~first packet with a PCR */, kTsCPcrLast, kTsCounters };
// Per stream, 64-bit: bad sync bytes, TEI packets, kept packets, and ~(index << 13 | pid) of the first valid packet with a PCR (a maximum)
enum { kTsTSync = 0, kTsTTei, kTsTKept, kTsTNotPcrKey, kTsTotals };

// One stream's words in the zeroed state: the presence bitmap, the totals, the counters
constexpr size_t kTsStateWords = kTsBitmapWords + 2u * kTsTotals + (size_t)kTsPids * kTsCounters;
constexpr size_t kTsStateTotals = kTsBitmapWords, kTsStateCounters = kTsBitmapWords + 2u * kTsTotals;

enum { kTsDropNull = 1u, kTsDropTei = 2u, kTsDropSync = 4u };

struct ts_stream {
  const unsigned char *ts;         // 4-byte aligned; null where n is 0
  unsigned long long n;            // packets
};
struct ts_args {
  const ts_stream *st;
  unsigned *state;                 // [streams][kTsStateWords]
  uint2 *hdr;                      // [streams][max_tiles] {PIDs in the tile's list, packets the tile keeps}
  uint2 *list;                     // [streams][max_tiles][tile] {first descriptor, last descriptor} of every PID present in the tile
  lsdr_ts_summary *sum;            // [streams]
  lsdr_ts_pid *pids;               // [streams][max_pids]
  // the filter (rule != 0)
  const unsigned char *keep;       // [streams][1024] bit pid & 7 of byte pid >> 3, or null: every PID
  unsigned short *klist;           // [streams][max_tiles][tile] the kept packets' places in their tile, ascending
  unsigned *koff;                  // [streams][max_tiles] kept packets in front of the tile
  unsigned char *out;              // [streams][out_stride]
  unsigned *index;                 // [streams][max_packets], or null
  size_t out_stride, max_packets;
  unsigned tile, max_tiles, max_pids, rule, drop;
};

// whether the rule keeps a packet with descriptor d
TS_HD bool ts_keeps(unsigned d, unsigned drop, const unsigned char *keep) {
  const unsigned c = ts_class(d);
  if (c == kTsSync) return !(drop & kTsDropSync);
  if (c == kTsTei) return !(drop & kTsDropTei);
  if (c != kTsValid) return false;
  const unsigned pid = ts_pid(d);
  if (pid == kTsNullPid && (drop & kTsDropNull)) return false;
  return !keep || ((keep[pid >> 3] >> (pid & 7u)) & 1u);
}
#endif
