// leansdr_amd/csrc/derotate_batch_device.h — the phase arithmetic of lsdr_derotate_batch (include/lsdr_hip.h; kernel and host side in
// derotate_batch.hip).  Plain C++ on values, callable from a kernel and from the host: the knots of a track turned into segments
// (Φ, F, S) by the host, and a sample's phase from its segment in O(1) on the device.  Everything is an integer in units of 2^-64 cycle and
// wraps modulo 2^64: the arithmetic is done in uint64_t (two's complement), so no step depends on rounding or on the order of evaluation.
//   dr_freq_word, dr_floor_div, dr_tri, dr_phase, dr_freq   values
//   dr_build                                                a capture's knots checked and turned into its segments (host)
//   dr_find                                                 the segment of a sample, by binary search
#ifndef LSDR_DEROTATE_BATCH_DEVICE_H
#define LSDR_DEROTATE_BATCH_DEVICE_H
#include <cmath>
#include <cstdint>
#include "capture_input.h"

struct dr_knot { uint64_t sample; double tune; };                          // = lsdr_track_knot
// One segment: from sample `start` on (to the next segment's start, the last one to the capture's end) the phase of sample n is
// phi + F·m + S·m(m − 1)/2 with m = n − start; F and S are signed numbers kept as their two's complement.
struct dr_seg { uint64_t start, phi, F, S; };
static_assert(sizeof(dr_seg) == 32, "dr_seg is uploaded as an array");

constexpr uint64_t kDrMaxSample = 1ull << 31;                              // a knot's sample lies below it

// F = tune·2^64 rounded to nearest, for |tune| < 0.5 (above 2^-11 the product is a whole number already)
inline int64_t dr_freq_word(double tune) { return (int64_t)llrint(ldexp(tune, 64)); }

// floor(a / d) for d > 0
IN_HD int64_t dr_floor_div(int64_t a, int64_t d) {
  int64_t q = a / d;
  if (a % d != 0 && a < 0) --q;
  return q;
}

// m(m − 1)/2 modulo 2^64, exact for every m: the even one of the two factors is halved first
IN_HD uint64_t dr_tri(uint64_t m) { return (m & 1u) ? m * ((m - 1u) >> 1) : (m >> 1) * (m - 1u); }

// the phase and the frequency word of sample n ≥ g.start in segment g
IN_HD uint64_t dr_phase(const dr_seg &g, uint64_t n) {
  const uint64_t m = n - g.start;
  return g.phi + g.F * m + g.S * dr_tri(m);
}
IN_HD uint64_t dr_freq(const dr_seg &g, uint64_t n) { return g.F + g.S * (n - g.start); }

// The segment of sample n: the last one whose start is at or before n (segs[0].start is 0; count ≥ 1).
IN_HD unsigned dr_find(const dr_seg *segs, unsigned count, uint64_t n) {
  unsigned lo = 0, hi = count;                                             // segs[lo].start ≤ n < segs[hi].start
  while (hi - lo > 1u) {
    const unsigned mid = lo + (hi - lo) / 2u;
    if (segs[mid].start <= n) lo = mid; else hi = mid;
  }
  return lo;
}

// A capture's knots checked and turned into segments: segs has room for n_knots + 1.  *count: the segments written, at least 1 (no knots:
// one segment of frequency 0).  Returns 0, or the number of the rule that is broken, with *bad the knot it is broken at:
//   1 a sample at or above 2^31   2 samples not strictly ascending   3 a tune not finite or outside (−0.5, 0.5)
//   4 a step between neighbours of 0.5 cycle per sample or more
// Nothing is written to segs then.
inline int dr_build(const dr_knot *knots, unsigned n_knots, dr_seg *segs, unsigned *count, unsigned *bad) {
  for (unsigned i = 0; i < n_knots; ++i) {
    *bad = i;
    if (knots[i].sample >= kDrMaxSample) return 1;
    if (i && knots[i].sample <= knots[i - 1].sample) return 2;
    if (!std::isfinite(knots[i].tune) || !(fabs(knots[i].tune) < 0.5)) return 3;
    if (i) {
      const __int128 d = (__int128)dr_freq_word(knots[i].tune) - (__int128)dr_freq_word(knots[i - 1].tune);
      if (!(fabs(knots[i].tune - knots[i - 1].tune) < 0.5) || d >= ((__int128)1 << 63) || d <= -((__int128)1 << 63)) return 4;
    }
  }
  *bad = 0;
  if (n_knots == 0) {
    segs[0] = dr_seg{0, 0, 0, 0};
    *count = 1;
    return 0;
  }
  unsigned c = 0;
  auto slope = [&](unsigned i) -> uint64_t {                               // of the segment behind knot i; the last knot takes the one in front of it
    if (n_knots == 1) return 0;
    if (i + 1 == n_knots) --i;
    return (uint64_t)dr_floor_div(dr_freq_word(knots[i + 1].tune) - dr_freq_word(knots[i].tune), (int64_t)(knots[i + 1].sample - knots[i].sample));
  };
  if (knots[0].sample > 0) {                                               // the knot the library puts at sample 0: the first slope, run back
    const uint64_t S = slope(0);
    segs[c++] = dr_seg{0, 0, (uint64_t)dr_freq_word(knots[0].tune) - S * knots[0].sample, S};
  }
  for (unsigned i = 0; i < n_knots; ++i) {
    const uint64_t phi = c ? dr_phase(segs[c - 1], knots[i].sample) : 0;   // Φ is continuous at every knot
    segs[c++] = dr_seg{knots[i].sample, phi, (uint64_t)dr_freq_word(knots[i].tune), slope(i)};
  }
  *count = c;
  return 0;
}
#endif
