// leansdr_amd/csrc/tune_est_device.h — the arithmetic that is the carrier-offset estimator's own (lsdr_tune_est, include/lsdr_hip.h; kernels
// and host side in tune_est.hip).  Plain C++ on values, callable from a kernel and from the host: the fourth power and the peak's
// interpolation.  The blocks, the transform and the reductions are block_spectrum.h's, the samples' conversion capture_input.h's.
#ifndef LSDR_TUNE_EST_DEVICE_H
#define LSDR_TUNE_EST_DEVICE_H
#include "block_spectrum.h"

constexpr unsigned kTeN = kBsN;          // samples per block, FFT length
constexpr unsigned kTeMaxBlocks = 64;

// z ↦ (z·inv)⁴: the fourth power of the normalised sample removes QPSK's modulation (every point of the constellation has the same z⁴)
IN_HD float2 te_pow4(float2 z, float inv) {
  const float2 u = make_float2(z.x * inv, z.y * inv), u2 = bs_cmul(u, u);
  return bs_cmul(u2, u2);
}

// The record of one capture from its summed spectrum: peak bin k0 with power c, cyclic neighbours l and r, Σ P.  In double: one thread per
// capture runs this once, and tune (|tune| ≤ 1/8) is then the float nearest to the formula's value.
struct te_record { float tune, quality; unsigned bin, blocks; float power[3], mean_power; };      // = lsdr_tune_estimate
IN_HD te_record te_peak_record(unsigned k0, float l, float c, float r, float sum, unsigned blocks) {
  te_record R;
  R.bin = k0; R.blocks = blocks; R.power[0] = l; R.power[1] = c; R.power[2] = r;
  R.mean_power = sum * (1.0f / (float)kTeN);
  R.tune = 0.f; R.quality = 0.f;
  if (c > 0.f) {                                             // (an all-zero capture has no peak: tune and quality stay 0)
    const double m = sqrt((double)(l > r ? l : r) / (double)c), d = m / (1.0 + m);
    double kappa = (double)k0 + (r >= l ? d : -d);
    if (kappa >= 0.5 * kTeN) kappa -= (double)kTeN;
    R.tune = (float)(kappa / (4.0 * kTeN));
    R.quality = c / R.mean_power;
  }
  return R;
}
#endif
