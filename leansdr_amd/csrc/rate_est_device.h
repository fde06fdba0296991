// leansdr_amd/csrc/rate_est_device.h — the arithmetic of the symbol-rate estimator (lsdr_rate_est, include/lsdr_hip.h; kernels and host
// side in rate_est.hip).  Plain C++ on values, callable from a kernel and from the host: the layout of a block's row, and the record of one
// capture from its summed spectrum.  The blocks, the transform and the reductions are block_spectrum.h's, the samples' conversion
// capture_input.h's.
#ifndef LSDR_RATE_EST_DEVICE_H
#define LSDR_RATE_EST_DEVICE_H
#include "block_spectrum.h"

constexpr unsigned kReN = kBsN;                    // samples per block, FFT length
constexpr unsigned kReHalf = kReN / 2u;            // the last bin searched: P is symmetric
constexpr unsigned kReRow = kReHalf + 16u;         // floats per block row: bins 0 … N/2, padded to whole 64-byte lines
constexpr unsigned kReMaxBlocks = 256;
constexpr float kReOmegaMin = 1.016f, kReOmegaMax = 64.0f;

struct re_record { float omega, other, line, quality, corr; unsigned bin, blocks, ambiguous; float power[3], floor; };   // = lsdr_rate_estimate

// k_lo = max(2, ⌊N/omega_max⌋): the first bin searched.  With omega_max < 2 that lies behind N/2 and only candidate b is admissible, whose
// lowest line is 1 − 1/omega_min: k_lo = max(2, ⌊N·(1 − 1/omega_min)⌋) then.
IN_HD unsigned re_k_lo(float omega_min, float omega_max) {
  const double lowest = omega_max < 2.f ? 1.0 - 1.0 / (double)omega_min : 1.0 / (double)omega_max;
  const unsigned k = (unsigned)floor((double)kReN * lowest);
  return k < 2u ? 2u : k;
}
IN_HD double re_abs_sinc(double x) {
  const double a = 3.14159265358979323846 * x;
  return a == 0.0 ? 1.0 : fabs(sin(a) / a);
}

// Steps 5 to 8 for one capture, in double: peak bin k0 with power c, neighbours l and r, the floor (mean of P over the searched bins),
// corr = R, the blocks M.  One thread per capture runs this once; every float of the record is the one nearest to the formula's value.
IN_HD re_record re_peak_record(unsigned k0, float l, float c, float r, float floor_, float corr, unsigned blocks, float omega_min, float omega_max) {
  re_record R{};                                             // all zeros: c = 0, or no admissible candidate
  if (!(c > 0.f)) return R;
  const double lp = (double)l - (double)floor_ > 0.0 ? (double)l - (double)floor_ : 0.0;
  const double rp = (double)r - (double)floor_ > 0.0 ? (double)r - (double)floor_ : 0.0;
  const double m = sqrt((lp > rp ? lp : rp) / (double)c), d = m / (1.0 + m);
  double line = ((double)k0 + (rp >= lp ? d : -d)) / (double)kReN;
  if (line > 0.5) line = 1.0 - line;
  const double a = 1.0 / line, b = 1.0 / (1.0 - line);
  const bool ok_a = a >= (double)omega_min && a <= (double)omega_max, ok_b = b >= (double)omega_min && b <= (double)omega_max;
  if (!ok_a && !ok_b) return R;
  const bool pick_a = ok_a && ok_b ? fabs((double)corr - re_abs_sinc(line)) < fabs((double)corr - re_abs_sinc(1.0 - line)) : ok_a;
  R.omega = (float)(pick_a ? a : b);
  R.other = ok_a && ok_b ? (float)(pick_a ? b : a) : 0.f;
  R.line = (float)line;
  R.quality = c / floor_;
  R.corr = corr;
  R.bin = k0; R.blocks = blocks;
  R.ambiguous = ok_a && ok_b && line > 0.4 ? 1u : 0u;
  R.power[0] = l; R.power[1] = c; R.power[2] = r;
  R.floor = floor_;
  return R;
}
#endif
