// leansdr_amd/csrc/tune_est_device.h — the arithmetic of the carrier-offset estimator (lsdr_tune_est, include/lsdr_hip.h; kernels and host
// side in tune_est.hip).  Everything here is plain C++ on values and arrays, callable from a kernel and from the host: the fourth
// power, one radix-4 stage of the 4096-point FFT, the order its output comes out in, and the peak's interpolation.  The samples' conversion
// is capture_input.h's, as for every object that reads raw captures.
#ifndef LSDR_TUNE_EST_DEVICE_H
#define LSDR_TUNE_EST_DEVICE_H

#define TE_HD __host__ __device__ __forceinline__

constexpr unsigned kTeN = 4096;          // samples per block, FFT length
constexpr unsigned kTeLog4 = 6;          // radix-4 stages
constexpr unsigned kTeMaxBlocks = 64;

TE_HD float2 te_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// z ↦ (z·inv)⁴: the fourth power of the normalised sample removes QPSK's modulation (every point of the constellation has the same z⁴)
TE_HD float2 te_pow4(float2 z, float inv) {
  const float2 u = make_float2(z.x * inv, z.y * inv), u2 = te_cmul(u, u);
  return te_cmul(u2, u2);
}

// Stage s (0 … 5) of the in-place radix-4 decimation-in-frequency FFT of x[4096], the share of thread `tid` of 256: four butterflies.
// Sub-transform length L = 4096 / 4^s, quarter q = L / 4; tw[i] = exp(−j2π·i/4096).  Output m of a butterfly goes to quarter m, so X[k]
// ends up where te_digit_reverse(k) says.  A barrier belongs between two stages.
TE_HD void te_fft_stage(float2 *x, const float2 *tw, unsigned s, unsigned tid) {
  const unsigned lq = 10u - 2u * s, q = 1u << lq;
  for (unsigned i = 0; i < 4; ++i) {
    const unsigned b = tid + 256u * i;                       // butterfly 0 … 1023
    const unsigned j = b & (q - 1u), base = ((b >> lq) << (lq + 2u)) + j;
    const unsigned tj = j << (2u * s);                       // j·4096/L
    const float2 a0 = x[base], a1 = x[base + q], a2 = x[base + 2u * q], a3 = x[base + 3u * q];
    const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y), t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
    const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y);
    const float2 t3 = make_float2(a1.y - a3.y, -(a1.x - a3.x));                  // −j·(a1 − a3)
    x[base] = make_float2(t0.x + t2.x, t0.y + t2.y);
    x[base + q] = te_cmul(make_float2(t1.x + t3.x, t1.y + t3.y), tw[tj]);
    x[base + 2u * q] = te_cmul(make_float2(t0.x - t2.x, t0.y - t2.y), tw[2u * tj]);
    x[base + 3u * q] = te_cmul(make_float2(t1.x - t3.x, t1.y - t3.y), tw[3u * tj]);
  }
}
// where X[k] sits behind the six stages: k's base-4 digits reversed
TE_HD unsigned te_digit_reverse(unsigned k) {
  unsigned p = 0;
  for (unsigned d = 0; d < kTeLog4; ++d) { p = (p << 2) | (k & 3u); k >>= 2; }
  return p;
}

// The record of one capture from its summed spectrum: peak bin k0 with power c, cyclic neighbours l and r, Σ P.  In double: one thread per
// capture runs this once, and tune (|tune| ≤ 1/8) is then the float nearest to the formula's value.
struct te_record { float tune, quality; unsigned bin, blocks; float power[3], mean_power; };      // = lsdr_tune_estimate
TE_HD te_record te_peak_record(unsigned k0, float l, float c, float r, float sum, unsigned blocks) {
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
