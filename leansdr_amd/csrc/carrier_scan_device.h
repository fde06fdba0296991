// leansdr_amd/csrc/carrier_scan_device.h — the arithmetic of the carrier scan (lsdr_carrier_scan, include/lsdr_hip.h; kernels and host side
// in carrier_scan.hip).  Plain C++ on values, callable from a kernel and from the host: the smoothed spectrum, the runs of bins above the
// threshold in frequency order, and the record of one run.  The blocks, the transform and the host's frame are block_spectrum.h's, the
// samples' conversion capture_input.h's.
//
// The runs are found by 256 threads in phases, each a function of the thread's index like bs_fft_stage; between two phases stands an
// exclusive prefix sum over the threads' counts (cs_scan256 in the kernel, a loop in tests/carrier_scan_host.hip):
//   cs_count_edges   thread t looks at positions 16t … 16t + 15 of the frequency order (position p is bin (p + N/2) mod N, −1/2 upward) and
//                    counts the runs that start and the runs that end there, packed as starts | ends << 16
//   cs_list_edges    … and writes their bins to start[] / end[] from its own ordinals on
//   cs_run_of        run j: start[j] and the end that belongs to it (the next one when the first end lies in front of the first start: a run
//                    across ±1/2, which is then the last), its length
//   cs_count_kept    thread t takes runs 8t … 8t + 7 and counts those of at least min_bins bins;  cs_list_kept writes the first max_carriers
//   cs_run_record    one listed run's record, in double on the float values of S
#ifndef LSDR_CARRIER_SCAN_DEVICE_H
#define LSDR_CARRIER_SCAN_DEVICE_H
#include "block_spectrum.h"

constexpr unsigned kCsN = kBsN;                    // samples per block, FFT length, bins
constexpr unsigned kCsMask = kCsN - 1u;
constexpr unsigned kCsMaxBlocks = 256;
constexpr unsigned kCsMaxSmooth = 64;
constexpr unsigned kCsMaxCarriers = 64;
constexpr unsigned kCsFloorRank = kCsN / 8u;       // the floor is the value of this rank (from 0) among the 4096 of S
constexpr unsigned kCsMaxRuns = kCsN / 2u;         // a run needs a bin below the threshold behind it
constexpr unsigned kCsPerThread = kCsN / 256u, kCsRunsPerThread = kCsMaxRuns / 256u;

struct cs_summary { unsigned blocks, stride, found, listed, saturated, reserved; float floor, threshold; };              // = lsdr_scan_summary
struct cs_carrier { float center, bandwidth, omega, level, plateau; unsigned first_bin, bins, weak; };                  // = lsdr_scan_carrier
struct cs_run { unsigned first, bins; };

// S[k] = (Σ_{j = −smooth … +smooth} P[(k + j) mod N]) / (float)(2·smooth + 1): float, j ascending, one division
IN_HD float cs_smooth(const float *P, unsigned k, unsigned smooth) {
  float acc = 0.f;
  for (unsigned j = 0; j <= 2u * smooth; ++j) acc += P[(k + kCsN - smooth + j) & kCsMask];
  return acc / (float)(2u * smooth + 1u);
}

IN_HD unsigned cs_bin_of(unsigned position) { return (position + kCsN / 2u) & kCsMask; }
IN_HD unsigned cs_position_of(unsigned bin) { return (bin + kCsN / 2u) & kCsMask; }

IN_HD unsigned cs_count_edges(const float *S, float T, unsigned tid) {
  unsigned packed = 0;
  for (unsigned i = 0; i < kCsPerThread; ++i) {
    const unsigned k = cs_bin_of(tid * kCsPerThread + i);
    if (!(S[k] >= T)) continue;
    if (!(S[(k - 1u) & kCsMask] >= T)) packed += 1u;
    if (!(S[(k + 1u) & kCsMask] >= T)) packed += 1u << 16;
  }
  return packed;
}
// base: the starts (low half) and ends (high half) of the threads in front of this one
IN_HD void cs_list_edges(const float *S, float T, unsigned tid, unsigned base, unsigned short *start, unsigned short *end) {
  unsigned ns = base & 0xffffu, ne = base >> 16;
  for (unsigned i = 0; i < kCsPerThread; ++i) {
    const unsigned k = cs_bin_of(tid * kCsPerThread + i);
    if (!(S[k] >= T)) continue;
    if (!(S[(k - 1u) & kCsMask] >= T)) start[ns++] = (unsigned short)k;
    if (!(S[(k + 1u) & kCsMask] >= T)) end[ne++] = (unsigned short)k;
  }
}
// run j of `runs` (≥ 1) in the order of the starts
IN_HD cs_run cs_run_of(const unsigned short *start, const unsigned short *end, unsigned runs, unsigned j) {
  const unsigned shift = cs_position_of(end[0]) < cs_position_of(start[0]) ? 1u : 0u;
  unsigned e = j + shift;
  if (e >= runs) e -= runs;
  cs_run r;
  r.first = start[j];
  r.bins = (((unsigned)end[e] - r.first) & kCsMask) + 1u;
  return r;
}
IN_HD unsigned cs_count_kept(const unsigned short *start, const unsigned short *end, unsigned runs, unsigned min_bins, unsigned tid) {
  unsigned kept = 0;
  for (unsigned i = 0; i < kCsRunsPerThread; ++i) {
    const unsigned j = tid * kCsRunsPerThread + i;
    if (j < runs && cs_run_of(start, end, runs, j).bins >= min_bins) ++kept;
  }
  return kept;
}
// base: the kept runs of the threads in front of this one; list[max_carriers]
IN_HD void cs_list_kept(const unsigned short *start, const unsigned short *end, unsigned runs, unsigned min_bins, unsigned tid, unsigned base,
                        unsigned max_carriers, cs_run *list) {
  for (unsigned i = 0; i < kCsRunsPerThread; ++i) {
    const unsigned j = tid * kCsRunsPerThread + i;
    if (j >= runs) break;
    const cs_run r = cs_run_of(start, end, runs, j);
    if (r.bins < min_bins) continue;
    if (base < max_carriers) list[base] = r;
    ++base;
  }
}

// Step 7 for the run of n bins from bin a on (unwrapped: [a, a + n − 1], S indexed mod N).  One thread per run; every float of the record
// is the one nearest to the double value.
IN_HD cs_carrier cs_run_record(const float *S, unsigned a, unsigned n, float floor_, float T) {
  const unsigned b = a + n - 1u, q = n / 4u;
  double sum = 0.0;
  for (unsigned k = a + q; k <= b - q; ++k) sum += (double)S[k & kCsMask];
  const double plateau = sum / (double)(n - 2u * q);
  const double L = plateau - (double)floor_, H = (double)floor_ + L / 2.0;
  unsigned i = a, j = b;
  bool weak = H < (double)T;
  if (!weak) {
    while (i <= b && !((double)S[i & kCsMask] >= H)) ++i;
    weak = i > b;                                            // (not with finite values: the plateau's largest bin is at least H)
  }
  double lo, hi;
  if (weak) {
    lo = (double)a - 0.5; hi = (double)b + 0.5;
  } else {
    while (!((double)S[j & kCsMask] >= H)) --j;              // (ends at i at the latest)
    const double si = (double)S[i & kCsMask], sj = (double)S[j & kCsMask];
    lo = (double)i - (si - H) / (si - (double)S[(i + kCsN - 1u) & kCsMask]);
    hi = (double)j + (sj - H) / (sj - (double)S[(j + 1u) & kCsMask]);
  }
  const double c = (lo + hi) / (2.0 * (double)kCsN), bw = (hi - lo) / (double)kCsN;
  cs_carrier R;
  R.center = (float)(c - floor(c + 0.5));
  R.bandwidth = (float)bw;
  R.omega = (float)(1.0 / bw);
  R.level = (float)(L / (double)floor_);
  R.plateau = (float)plateau;
  R.first_bin = a; R.bins = n; R.weak = weak ? 1u : 0u;
  return R;
}
#endif
