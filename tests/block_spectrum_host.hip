// tests/block_spectrum_host.hip — the arithmetic under lsdr_tune_est and lsdr_rate_est on the host (leansdr_amd/csrc/block_spectrum.h,
// tune_est_device.h, rate_est_device.h), built and run by tests/test_block_spectrum_host.py (host side only, -ffp-contract=off,
// AddressSanitizer and UBSan).  No GPU call is made.
//
// The transform: bs_fft_stage for the 256 thread indices of each of the six stages, read out through bs_digit_reverse, on one seeded block
// (a tone between two bins plus noise), against a float64 DFT — powers within 1e-4 of the peak power, the estimators' own bound.  The
// reversal is an involution on 0 … 4095.  te_peak_record and re_peak_record on hand-set peaks against the formulas of the docstrings of
// tests/tune_common.py and tests/rate_common.py, written out here in double.
#include <cstdint>
#include <vector>
#include "tune_est_device.h"
#include "rate_est_device.h"

void lsdr_set_error(const char *, ...) {}

static unsigned g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) { ++g_failed; printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
  } while (0)

static const double kPi = 3.14159265358979323846;

static void check_transform() {
  std::vector<float2> x(kBsN), tw(kBsN);
  std::vector<double> cs(kBsN), sn(kBsN);
  for (unsigned i = 0; i < kBsN; ++i) {
    cs[i] = cos(-2.0 * kPi * (double)i / (double)kBsN); sn[i] = sin(-2.0 * kPi * (double)i / (double)kBsN);
    tw[i] = make_float2((float)cs[i], (float)sn[i]);                       // (the table the estimators upload)
  }
  uint64_t seed = 0x9e3779b97f4a7c15ull;
  auto uniform = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0 - 0.5; };
  for (unsigned n = 0; n < kBsN; ++n) {                                    // a tone at bin 300.5 plus noise of a third of its amplitude
    const double a = 2.0 * kPi * 300.5 * (double)n / (double)kBsN;
    x[n] = make_float2((float)(cos(a) + 0.66 * uniform()), (float)(sin(a) + 0.66 * uniform()));
  }
  std::vector<double> want(kBsN);
  double peak = 0.0;
  for (unsigned k = 0; k < kBsN; ++k) {
    double re = 0.0, im = 0.0;
    for (unsigned n = 0; n < kBsN; ++n) {
      const unsigned i = (k * n) & (kBsN - 1u);
      re += (double)x[n].x * cs[i] - (double)x[n].y * sn[i];
      im += (double)x[n].x * sn[i] + (double)x[n].y * cs[i];
    }
    want[k] = re * re + im * im;
    if (want[k] > peak) peak = want[k];
  }
  for (unsigned s = 0; s < kBsLog4; ++s)
    for (unsigned tid = 0; tid < 256u; ++tid) bs_fft_stage(x.data(), tw.data(), s, tid);
  double worst = 0.0;
  unsigned worst_k = 0;
  for (unsigned k = 0; k < kBsN; ++k) {
    const float2 v = x[bs_digit_reverse(k)];
    const float p = v.x * v.x + v.y * v.y;
    const double d = fabs((double)p - want[k]) / peak;
    if (d > worst) { worst = d; worst_k = k; }
  }
  printf("transform: powers within %.3e of the peak power %.6e (bound 1e-4), the largest distance at bin %u\n", worst, peak, worst_k);
  CHECK(peak > 1e6, "the tone stands out: peak %g", peak);
  CHECK(worst <= 1e-4, "bin %u is off by %g of the peak power", worst_k, worst);
}

static void check_reversal() {
  std::vector<unsigned char> seen(kBsN, 0);
  unsigned bad = 0;
  for (unsigned k = 0; k < kBsN; ++k) {
    const unsigned p = bs_digit_reverse(k);
    if (p >= kBsN || bs_digit_reverse(p) != k || seen[p < kBsN ? p : 0]) ++bad;
    if (p < kBsN) seen[p] = 1;
  }
  CHECK(bad == 0, "%u of 4096 indices do not come back", bad);
  CHECK(bs_digit_reverse(1) == 1024 && bs_digit_reverse(4) == 256 && bs_digit_reverse(4095) == 4095 && bs_digit_reverse(0x1b) == 0xe40, "known values");
}

// tests/tune_common.py, step 5
static double tune_want(unsigned k0, double l, double c, double r) {
  if (!(c > 0)) return 0.0;
  const double m = sqrt((l > r ? l : r) / c), d = m / (1.0 + m);
  double kappa = (double)k0 + (r >= l ? d : -d);
  if (kappa >= kBsN / 2.0) kappa -= (double)kBsN;
  return kappa / (4.0 * kBsN);
}
static void check_tune_records() {
  static const struct { const char *name; unsigned k0; float l, c, r; } peaks[] = {
      {"r above l", 100, 10.f, 1000.f, 250.f}, {"l above r", 100, 250.f, 1000.f, 10.f}, {"l = r", 777, 40.f, 900.f, 40.f},
      {"bin 0", 0, 5.f, 500.f, 125.f},         {"bin 0, l above r", 0, 125.f, 500.f, 5.f}, {"the last bin", 4095, 1.f, 64.f, 16.f},
      {"bin N/2", 2048, 3.f, 300.f, 30.f},     {"bin N/2 - 1, r above l", 2047, 3.f, 300.f, 299.f}, {"c = 0", 0, 0.f, 0.f, 0.f}};
  for (const auto &p : peaks) {
    const float sum = 8192.f;
    const te_record R = te_peak_record(p.k0, p.l, p.c, p.r, sum, 8);
    const double want = tune_want(p.k0, p.l, p.c, p.r);
    CHECK(R.tune == (float)want, "%s: tune %a, the formula gives %a", p.name, R.tune, (float)want);
    CHECK(R.tune >= -0.125f && R.tune < 0.125f, "%s: tune %g lies in [-1/8, 1/8)", p.name, R.tune);
    CHECK(R.bin == p.k0 && R.blocks == 8 && R.power[0] == p.l && R.power[1] == p.c && R.power[2] == p.r && R.mean_power == 2.0f, "%s: the record's copies", p.name);
    CHECK(R.quality == (p.c > 0.f ? p.c / 2.0f : 0.f), "%s: quality %g", p.name, R.quality);
  }
  CHECK(te_peak_record(777, 40.f, 900.f, 40.f, 1.f, 1).tune > (float)(777.0 / (4.0 * kBsN)), "l = r: the fraction is added");
  CHECK(te_peak_record(0, 125.f, 500.f, 5.f, 1.f, 1).tune < 0.f && te_peak_record(2048, 3.f, 300.f, 30.f, 1.f, 1).tune < -0.12f, "bins wrap into [-N/2, N/2)");
}

// tests/rate_common.py, steps 5 and 6: false where the record is all zeros
struct rate_want { double omega, other, line; unsigned ambiguous; };
static bool rate_formula(unsigned k0, double l, double c, double r, double floor_, double corr, float omega_min, float omega_max, rate_want *w) {
  if (!(c > 0)) return false;
  const double lo = (double)omega_min, hi = (double)omega_max;
  const double lp = l - floor_ > 0 ? l - floor_ : 0.0, rp = r - floor_ > 0 ? r - floor_ : 0.0;
  const double m = sqrt((lp > rp ? lp : rp) / c), d = m / (1.0 + m);
  double line = ((double)k0 + (rp >= lp ? d : -d)) / (double)kBsN;
  if (line > 0.5) line = 1.0 - line;
  const double a = 1.0 / line, b = 1.0 / (1.0 - line);
  const bool ok_a = lo <= a && a <= hi, ok_b = lo <= b && b <= hi;
  if (!ok_a && !ok_b) return false;
  auto sinc = [](double v) { return v == 0.0 ? 1.0 : fabs(sin(kPi * v) / (kPi * v)); };
  const bool pick_a = ok_a && ok_b ? fabs(corr - sinc(line)) < fabs(corr - sinc(1.0 - line)) : ok_a;
  w->omega = pick_a ? a : b;
  w->other = pick_a ? (ok_b ? b : 0.0) : (ok_a ? a : 0.0);
  w->line = line;
  w->ambiguous = ok_a && ok_b && line > 0.4 ? 1u : 0u;
  return true;
}
static void check_rate_records() {
  static const struct { const char *name; unsigned k0; float l, c, r, floor_, corr, lo, hi; int zero, other, ambiguous; } peaks[] = {
      // (zero: the record is all zeros; other: a second candidate is reported)
      {"omega 4, only a admissible", 1024, 30.f, 4000.f, 900.f, 20.f, 0.9f, 2.0f, 64.f, 0, 0, 0},
      {"both admissible, corr picks a", 1024, 900.f, 4000.f, 30.f, 20.f, 0.9f, 1.016f, 64.f, 0, 1, 0},
      {"both admissible, corr picks b", 1024, 30.f, 4000.f, 900.f, 20.f, 0.3f, 1.016f, 64.f, 0, 1, 0},
      {"both admissible and ambiguous", 1900, 50.f, 2000.f, 500.f, 40.f, 0.6f, 1.016f, 64.f, 0, 1, 1},
      {"only b admissible", 1365, 300.f, 3000.f, 100.f, 10.f, 0.4f, 1.016f, 1.9f, 0, 0, 0},
      {"neither admissible", 1024, 30.f, 4000.f, 900.f, 20.f, 0.9f, 8.f, 64.f, 1, 0, 0},
      {"l = r", 512, 400.f, 5000.f, 400.f, 25.f, 0.97f, 1.016f, 64.f, 0, 1, 0},
      {"both neighbours under the floor", 512, 10.f, 5000.f, 20.f, 25.f, 0.97f, 1.016f, 64.f, 0, 1, 0},
      {"bin N/2, the mirrored neighbour", 2048, 700.f, 2500.f, 700.f, 30.f, 0.64f, 1.016f, 64.f, 0, 1, 1},
      {"c = 0", 2, 0.f, 0.f, 0.f, 0.f, 0.f, 1.016f, 64.f, 1, 0, 0}};
  for (const auto &p : peaks) {
    const re_record R = re_peak_record(p.k0, p.l, p.c, p.r, p.floor_, p.corr, 64, p.lo, p.hi);
    rate_want w = {0.0, 0.0, 0.0, 0u};
    const bool some = rate_formula(p.k0, p.l, p.c, p.r, p.floor_, p.corr, p.lo, p.hi, &w);
    CHECK(some == !p.zero && (w.other != 0.0) == (p.other != 0) && w.ambiguous == (unsigned)p.ambiguous, "%s: the case is the one its name says", p.name);
    if (!some) {
      const re_record Z{};
      CHECK(memcmp(&R, &Z, sizeof R) == 0, "%s: the record is all zeros", p.name);
      continue;
    }
    CHECK(R.omega == (float)w.omega && R.other == (float)w.other && R.line == (float)w.line && R.ambiguous == w.ambiguous,
          "%s: omega %a other %a line %a ambiguous %u, the formulas give %a %a %a %u", p.name, R.omega, R.other, R.line, R.ambiguous, (float)w.omega,
          (float)w.other, (float)w.line, w.ambiguous);
    CHECK(R.line > 0.f && R.line <= 0.5f, "%s: line %g lies in (0, 0.5]", p.name, R.line);
    CHECK(R.quality == p.c / p.floor_ && R.corr == p.corr && R.bin == p.k0 && R.blocks == 64 && R.power[0] == p.l && R.power[1] == p.c && R.power[2] == p.r &&
              R.floor == p.floor_, "%s: the record's copies", p.name);
  }
  CHECK(re_peak_record(2048, 700.f, 2500.f, 700.f, 30.f, 0.64f, 64, 1.016f, 64.f).line < 0.5f, "bin N/2 with equal neighbours: the line folds back under 0.5");
  CHECK(re_k_lo(1.016f, 64.f) == 64u && re_k_lo(1.016f, 1.9f) == (unsigned)floor(4096.0 * (1.0 - 1.0 / (double)1.016f)) && re_k_lo(1.016f, 4096.f * 4.f) == 2u, "k_lo");
}

int main() {
  check_transform();
  check_reversal();
  check_tune_records();
  check_rate_records();
  printf("%u checks, %u failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
