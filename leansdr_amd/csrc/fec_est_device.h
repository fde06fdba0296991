// leansdr_amd/csrc/fec_est_device.h — what lsdr_fec_est's two kernels and its host side share (fec_est.hip): the table of the 52
// hypotheses, the kernels' arguments, and the integer rules that turn the counts into a record.  Plain C++ on values: the rules are
// callable from a kernel and from the host.
#ifndef LSDR_FEC_EST_DEVICE_H
#define LSDR_FEC_EST_DEVICE_H
#include "lsdr_internal.h"

#define FE_HD __host__ __device__ __forceinline__

// The five rates in the record's order, 2/3 handled as 4/6 (dvb.h:491-495).  half = punctweight/2: the symbols one refill shifts in and
// the number of skips; pp = punctperiod: the checks per refill.  A (rate, skip) pair is a SLOT (13 of them, a rate's in a row from
// base); hypothesis = slot·4 + alignment (52); polynomial index = pbase + b (20).
constexpr unsigned kFeRates = 5, kFeSlots = 13, kFeHyp = 52, kFePolys = 20;
struct fe_rate_info { unsigned half, pp, base, pbase; int fec; };
__host__ __device__ constexpr fe_rate_info fe_rate(unsigned r) {
  switch (r) {
    case 0: return {1u, 1u, 0u, 0u, LSDR_FEC12};
    case 1: return {3u, 4u, 1u, 1u, LSDR_FEC23};
    case 2: return {2u, 3u, 4u, 5u, LSDR_FEC34};
    case 3: return {3u, 5u, 6u, 8u, LSDR_FEC56};
    default: return {4u, 7u, 9u, 13u, LSDR_FEC78};
  }
}

// A tile is kFeGroup·256·groups symbols: every thread of a workgroup of 256 takes `groups` runs of 12 consecutive refill ends (12 is
// the least common multiple of the halves: inside a run the skip of every rate is known at compile time).  In front of the tile the
// workgroup keeps kFeHist symbols of history (three packed words: a refill that ends on the tile's first symbol looks back 31).
constexpr unsigned kFeGroup = 12, kFeThreads = 256, kFeHist = 48, kFeMaxGroups = 8;
constexpr unsigned kFeMaxWords = kFeGroup * kFeThreads * kFeMaxGroups / 16u + 4u;   // the tile, the history, one word behind

// The check polynomials as the score kernel uses them.  deconv[b] ^ deconv2[b] = x; the four alignments (init_syncs, dvb.h:308-360) map
// a packed word of symbols by "swap the two bits of every symbol or not, then XOR a constant", so
//   parity(map_a(w) & x) = parity(w & (swap_a ? xs : x)) ^ parity(mask_a & x):   xs = x with the bits of every pair swapped, and the
// second term one constant bit per (alignment, polynomial): bit (pbase + b) of flip[a].  Alignments 0 and 2 share x, 1 and 3 share xs.
struct fe_polys {
  unsigned long long x[kFePolys], xs[kFePolys];
  unsigned flip[4];
};

struct fe_stream {
  const void *sym;                 // packed: the 4-byte aligned word that holds bit 0 of the stream; else the first symbol's item
  unsigned long long off, n;       // packed: symbol 0 is symbol `off` of the words at sym; n: the symbols scored
};
struct fe_args {
  const fe_stream *st;
  unsigned long long *counts;      // [streams][kFeHyp] errors, zeroed in front of the score kernel
  lsdr_fec_estimate *rec;          // [streams]
  unsigned groups, tile;           // runs per thread; symbols per tile = 12·256·groups
  fe_polys P;
};

// R·punctperiod for (rate, skip) on n symbols
FE_HD unsigned long long fe_checks(const fe_rate_info &ri, unsigned k, unsigned long long n) {
  return n >= 32u + k ? ((n - k - 32u) / ri.half + 1u) * ri.pp : 0u;
}
// E1/C1 < E2/C2, exactly; a hypothesis without checks never wins
FE_HD bool fe_less(unsigned long long e1, unsigned long long c1, unsigned long long e2, unsigned long long c2) {
  if (c1 == 0) return false;
  if (c2 == 0) return true;
  return e1 * c2 < e2 * c1;
}
// the best hypothesis of one rate: the first, alignment outer and skip inner, with the smallest fraction
FE_HD lsdr_fec_est_score fe_best_of_rate(unsigned r, const unsigned long long *counts, unsigned long long n) {
  const fe_rate_info ri = fe_rate(r);
  lsdr_fec_est_score s = {0, 0, 0, 0};
  for (unsigned a = 0; a < 4; ++a)
    for (unsigned k = 0; k < ri.half; ++k) {
      const unsigned long long e = counts[(ri.base + k) * 4u + a], c = fe_checks(ri, k, n);
      if (fe_less(e, c, s.errors, s.checks)) { s.errors = e; s.checks = c; s.sync = a; s.skip = k; }
    }
  return s;
}
// the record from the five rates' best hypotheses
FE_HD lsdr_fec_estimate fe_record(const lsdr_fec_est_score (&sc)[kFeRates], unsigned long long n) {
  lsdr_fec_estimate o;
  memset(&o, 0, sizeof(o));
  o.fec = -1;
  unsigned win = 0, locks = 0;
  for (unsigned r = 1; r < kFeRates; ++r)
    if (fe_less(sc[r].errors, sc[r].checks, sc[win].errors, sc[win].checks)) win = r;
  if (sc[win].checks == 0) return o;                                      // nothing scored: all zeros, fec −1
  int other = -1;
  for (unsigned r = 0; r < kFeRates; ++r) {
    locks += sc[r].checks > 0 && 3u * sc[r].errors <= sc[r].checks ? 1u : 0u;   // the reference's own criterion, dvb.h:449-453
    if (r != win && (other < 0 || fe_less(sc[r].errors, sc[r].checks, sc[other].errors, sc[other].checks))) other = (int)r;
    o.score[r] = sc[r];
  }
  o.fec = fe_rate(win).fec;
  o.locked = 3u * sc[win].errors <= sc[win].checks ? 1u : 0u;
  o.ambiguous = o.locked && locks > 1u ? 1u : 0u;
  o.sync = sc[win].sync; o.skip = sc[win].skip;
  o.symbols = n;
  o.error_rate = (float)((double)sc[win].errors / (double)sc[win].checks);
  o.runner_up = sc[other].checks ? (float)((double)sc[other].errors / (double)sc[other].checks) : 0.f;
  return o;
}
#endif
