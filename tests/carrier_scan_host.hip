// tests/carrier_scan_host.hip — the plain C++ of the carrier scan on the host (leansdr_amd/csrc/carrier_scan_device.h), built and run by
// tests/test_carrier_scan_host.py (host side only, -ffp-contract=off, AddressSanitizer and UBSan).  No GPU call is made.
//
// The runs: cs_count_edges, cs_list_edges, cs_count_kept and cs_list_kept for the 256 thread indices, a loop standing for the kernel's
// prefix sums, against a serial walk over the bins in frequency order — on hand-set S (a run across the N−1 → 0 seam, a run across ±1/2
// that has to come last, single bins, all above, none above, min_bins, max_carriers) and on seeded random patterns.  cs_run_record on
// hand-set runs (a plain one, one at the seam, weak, an edge at the run's first bin, n < 4) against the formulas of
// tests/scan_common.py's docstring, written out here in double.  cs_smooth against its definition.
#include <cstdint>
#include <vector>
#include "carrier_scan_device.h"

void lsdr_set_error(const char *, ...) {}

static unsigned g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) { ++g_failed; printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
  } while (0)

struct scan_out { unsigned runs, found, listed; bool saturated; std::vector<cs_run> list; };

// the kernel's phases, thread by thread
static scan_out by_phases(const std::vector<float> &S, float T, unsigned min_bins, unsigned max_carriers) {
  std::vector<unsigned short> start(kCsMaxRuns), end(kCsMaxRuns);
  std::vector<unsigned> count(256), base(256);
  unsigned total = 0;
  for (unsigned t = 0; t < 256; ++t) { count[t] = cs_count_edges(S.data(), T, t); base[t] = total; total += count[t]; }
  scan_out o;
  o.runs = total & 0xffffu;
  CHECK((total >> 16) == o.runs, "as many ends (%u) as starts (%u)", total >> 16, o.runs);
  CHECK(o.runs <= kCsMaxRuns, "%u runs", o.runs);
  for (unsigned t = 0; t < 256; ++t) cs_list_edges(S.data(), T, t, base[t], start.data(), end.data());
  o.found = 0;
  o.list.assign(max_carriers, cs_run{0xffffffffu, 0xffffffffu});
  if (o.runs) {
    for (unsigned t = 0; t < 256; ++t) { count[t] = cs_count_kept(start.data(), end.data(), o.runs, min_bins, t); base[t] = o.found; o.found += count[t]; }
    for (unsigned t = 0; t < 256; ++t) cs_list_kept(start.data(), end.data(), o.runs, min_bins, t, base[t], max_carriers, o.list.data());
  }
  o.listed = o.found < max_carriers ? o.found : max_carriers;
  o.list.resize(o.listed);
  o.saturated = !o.runs && S[0] >= T;
  return o;
}
// step 6 as it is written: a walk over the bins from −1/2 upward
static scan_out serially(const std::vector<float> &S, float T, unsigned min_bins, unsigned max_carriers) {
  scan_out o{0, 0, 0, true, {}};
  for (unsigned k = 0; k < kCsN; ++k) o.saturated = o.saturated && S[k] >= T;
  if (o.saturated) return o;
  for (unsigned p = 0; p < kCsN; ++p) {
    const unsigned s = (p + kCsN / 2u) % kCsN;
    if (!(S[s] >= T) || S[(s + kCsN - 1u) % kCsN] >= T) continue;
    unsigned n = 1;
    while (S[(s + n) % kCsN] >= T) ++n;
    ++o.runs;
    if (n < min_bins) continue;
    if (o.found < max_carriers) o.list.push_back(cs_run{s, n});
    ++o.found;
  }
  o.listed = (unsigned)o.list.size();
  return o;
}
static void compare(const char *name, const std::vector<float> &S, float T, unsigned min_bins, unsigned max_carriers, const scan_out *want) {
  const scan_out a = by_phases(S, T, min_bins, max_carriers), b = serially(S, T, min_bins, max_carriers);
  bool same = a.runs == b.runs && a.found == b.found && a.listed == b.listed && a.saturated == b.saturated && a.list.size() == b.list.size();
  for (size_t i = 0; same && i < a.list.size(); ++i) same = a.list[i].first == b.list[i].first && a.list[i].bins == b.list[i].bins;
  CHECK(same, "%s: the phases give %u runs, %u found, %u listed, saturated %d; the walk %u, %u, %u, %d", name, a.runs, a.found, a.listed, (int)a.saturated,
        b.runs, b.found, b.listed, (int)b.saturated);
  if (want) {
    bool as_said = a.found == want->found && a.saturated == want->saturated && a.list.size() == want->list.size();
    for (size_t i = 0; as_said && i < a.list.size(); ++i) as_said = a.list[i].first == want->list[i].first && a.list[i].bins == want->list[i].bins;
    CHECK(as_said, "%s: %u found, %zu listed, saturated %d", name, a.found, a.list.size(), (int)a.saturated);
  }
}
static void compare(const char *name, const std::vector<float> &S, float T, unsigned min_bins, unsigned max_carriers, const scan_out &want) {
  compare(name, S, T, min_bins, max_carriers, &want);
}
static void fill(std::vector<float> &S, unsigned first, unsigned bins, float v) {
  for (unsigned i = 0; i < bins; ++i) S[(first + i) % kCsN] = v;
}

static void check_runs() {
  std::vector<float> S(kCsN, 1.f);
  const float T = 2.f;
  compare("none above", S, T, 1, 8, scan_out{0, 0, 0, false, {}});
  std::fill(S.begin(), S.end(), 3.f);
  compare("all above", S, T, 1, 8, scan_out{0, 0, 0, true, {}});
  S[100] = 1.f;
  compare("all above but one bin", S, T, 1, 8, scan_out{1, 1, 1, false, {{101, kCsN - 1u}}});
  std::fill(S.begin(), S.end(), 1.f);
  fill(S, 4090, 20, 5.f);                                    // across the N−1 → 0 seam: in the middle of the frequency order
  fill(S, 3000, 30, 5.f);                                    // −0.27
  fill(S, 1000, 40, 5.f);                                    // +0.24
  compare("a run at the seam", S, T, 1, 8, scan_out{3, 3, 3, false, {{3000, 30}, {4090, 20}, {1000, 40}}});
  fill(S, 2040, 16, 5.f);                                    // across ±1/2: starts at +0.498, comes last
  compare("a run across +-1/2", S, T, 1, 8, scan_out{4, 4, 4, false, {{3000, 30}, {4090, 20}, {1000, 40}, {2040, 16}}});
  compare("min_bins", S, T, 25, 8, scan_out{4, 2, 2, false, {{3000, 30}, {1000, 40}}});
  compare("max_carriers", S, T, 1, 2, scan_out{4, 4, 2, false, {{3000, 30}, {4090, 20}}});
  compare("min_bins above every run", S, T, 41, 8, scan_out{4, 0, 0, false, {}});
  std::fill(S.begin(), S.end(), 1.f);
  S[2048] = 5.f; S[2047] = 5.f;                              // the first position of the order and the last
  compare("two bins across +-1/2", S, T, 1, 8, scan_out{1, 1, 1, false, {{2047, 2}}});
  S[2047] = 1.f; S[0] = 5.f; S[4095] = 1.f;
  compare("single bins", S, T, 1, 8, scan_out{2, 2, 2, false, {{2048, 1}, {0, 1}}});
  for (unsigned k = 0; k < kCsN; ++k) S[k] = (k & 1u) ? 5.f : 1.f;          // the most runs there can be
  compare("every other bin", S, T, 1, kCsMaxCarriers, nullptr);
  CHECK(by_phases(S, T, 1, kCsMaxCarriers).found == kCsMaxRuns, "2048 runs");
  S[17] = NAN;
  compare("a NaN is not above", S, T, 1, kCsMaxCarriers, nullptr);
  uint64_t seed = 0x9e3779b97f4a7c15ull;
  auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(seed >> 40); };
  for (unsigned round = 0; round < 40; ++round) {           // random run lengths, random levels around the threshold
    unsigned k = next() % kCsN;
    for (unsigned done = 0; done < kCsN;) {
      const unsigned n = 1u + next() % (round < 20 ? 40u : 700u);
      const float v = (next() & 1u) ? 2.f + (float)(next() % 8u) : 1.f;     // (2.0 itself is above)
      for (unsigned i = 0; i < n && done < kCsN; ++i, ++done) S[(k + done) % kCsN] = v;
    }
    char name[32];
    snprintf(name, sizeof name, "random pattern %u", round);
    compare(name, S, T, 1u + next() % 30u, 1u + next() % kCsMaxCarriers, nullptr);
  }
}

// tests/scan_common.py, step 7
struct want_rec { double center, bandwidth, omega, level, plateau; unsigned weak; };
static want_rec formula(const std::vector<float> &S, unsigned a, unsigned n, double floor_, double T) {
  const long b = (long)a + n - 1, q = n / 4;
  auto s = [&](long k) { return (double)S[(size_t)((k % (long)kCsN + kCsN) % kCsN)]; };
  double sum = 0.0;
  for (long k = a + q; k <= b - q; ++k) sum += s(k);
  want_rec w;
  w.plateau = sum / (double)(n - 2 * q);
  const double L = w.plateau - floor_, H = floor_ + L / 2.0;
  double lo, hi;
  w.weak = H < T ? 1u : 0u;
  if (w.weak) {
    lo = a - 0.5; hi = b + 0.5;
  } else {
    long i = a, j = b;
    while (s(i) < H) ++i;
    while (s(j) < H) --j;
    lo = (double)i - (s(i) - H) / (s(i) - s(i - 1));
    hi = (double)j + (s(j) - H) / (s(j) - s(j + 1));
  }
  const double c = (lo + hi) / (2.0 * kCsN);
  w.center = c - floor(c + 0.5);
  w.bandwidth = (hi - lo) / kCsN;
  w.omega = 1.0 / w.bandwidth;
  w.level = L / floor_;
  return w;
}
static void check_record(const char *name, const std::vector<float> &S, unsigned a, unsigned n, float floor_, float T, unsigned weak) {
  const cs_carrier R = cs_run_record(S.data(), a, n, floor_, T);
  const want_rec w = formula(S, a, n, (double)floor_, (double)T);
  CHECK(w.weak == weak, "%s: the case is the one its name says", name);
  CHECK(R.center == (float)w.center && R.bandwidth == (float)w.bandwidth && R.omega == (float)w.omega && R.level == (float)w.level && R.plateau == (float)w.plateau,
        "%s: center %a bandwidth %a omega %a level %a plateau %a, the formulas give %a %a %a %a %a", name, R.center, R.bandwidth, R.omega, R.level, R.plateau,
        (float)w.center, (float)w.bandwidth, (float)w.omega, (float)w.level, (float)w.plateau);
  CHECK(R.first_bin == a && R.bins == n && R.weak == weak, "%s: first_bin %u bins %u weak %u", name, R.first_bin, R.bins, R.weak);
  CHECK(R.center >= -0.5f && R.center <= 0.5f && R.bandwidth > 0.f, "%s: center %g bandwidth %g", name, R.center, R.bandwidth);
}
// a carrier with sloping edges: `edge` bins up, `top` bins of the plateau (with a ripple), `edge` bins down, all of it above T
static unsigned shape(std::vector<float> &S, unsigned a, unsigned edge, unsigned top, float T, float peak) {
  unsigned k = a;
  for (unsigned i = 0; i < edge; ++i) S[k++ % kCsN] = T + (peak - T) * (float)(i + 1) / (float)(edge + 1) * 0.97f;
  for (unsigned i = 0; i < top; ++i) S[k++ % kCsN] = peak * (1.f + 0.013f * (float)((int)(i * 7u % 11u) - 5));
  for (unsigned i = 0; i < edge; ++i) S[k++ % kCsN] = T + (peak - T) * (float)(edge - i) / (float)(edge + 1) * 0.93f;
  return k - a;
}
static void check_records() {
  const float floor_ = 1.f, T = 2.f;
  std::vector<float> S(kCsN, 1.1f);
  unsigned n = shape(S, 700, 30, 200, T, 40.f);
  check_record("a plain run", S, 700, n, floor_, T, 0);
  const cs_carrier R = cs_run_record(S.data(), 700, n, floor_, T);
  CHECK(fabsf(R.center - (700.f + 0.5f * (float)(n - 1u)) / (float)kCsN) < 2.f / (float)kCsN && R.bandwidth < (float)n / (float)kCsN, "a plain run: center %g, bandwidth %g", R.center, R.bandwidth);
  std::fill(S.begin(), S.end(), 1.1f);
  n = shape(S, 4000, 25, 150, T, 30.f);                      // bins 4000 … 103: the unwrapped indices pass N
  check_record("a run at the seam", S, 4000, n, floor_, T, 0);
  CHECK(cs_run_record(S.data(), 4000, n, floor_, T).center > 0.f && cs_run_record(S.data(), 4000, n, floor_, T).center < 0.002f, "a run at the seam: the centre is just above 0");
  std::fill(S.begin(), S.end(), 1.1f);
  n = shape(S, 1990, 20, 90, T, 30.f);                       // across ±1/2: the centre wraps into [−1/2, 1/2)
  check_record("a run across +-1/2", S, 1990, n, floor_, T, 0);
  CHECK(cs_run_record(S.data(), 1990, n, floor_, T).center < -0.49f, "a run across +-1/2: the centre is negative");
  std::fill(S.begin(), S.end(), 1.1f);
  fill(S, 300, 40, 2.6f);                                    // plateau 2.6: H = 1.8 < T
  check_record("weak", S, 300, 40, floor_, T, 1);
  const cs_carrier W = cs_run_record(S.data(), 300, 40, floor_, T);
  CHECK(W.bandwidth == 40.f / (float)kCsN && W.center == (float)(319.5 / kCsN), "weak: the edges are the run's");
  std::fill(S.begin(), S.end(), 1.1f);
  fill(S, 500, 60, 20.f);                                    // a brick: S[a] is above H already, the edge lies between a − 1 and a
  check_record("an edge at the run's first bin", S, 500, 60, floor_, T, 0);
  S[499] = 1.9f; S[560] = 1.99f;
  check_record("an edge at the run's first bin, neighbours just under T", S, 500, 60, floor_, T, 0);
  for (unsigned len = 1; len < 4; ++len) {
    std::fill(S.begin(), S.end(), 1.1f);
    for (unsigned i = 0; i < len; ++i) S[(4095u + i) % kCsN] = 9.f + (float)i;
    char name[32];
    snprintf(name, sizeof name, "n = %u at the seam", len);
    check_record(name, S, 4095, len, floor_, T, 0);
  }
  std::fill(S.begin(), S.end(), 1.1f);
  S[0] = 2.5f;
  check_record("n = 1 and weak", S, 0, 1, floor_, T, 1);
}

static void check_smooth() {
  std::vector<float> P(kCsN);
  for (unsigned k = 0; k < kCsN; ++k) P[k] = (float)((k * 2654435761u) >> 20) * 0.37f;
  unsigned bad = 0;
  for (unsigned smooth : {1u, 8u, 64u})
    for (unsigned k : {0u, 1u, 63u, 64u, 2048u, 4031u, 4032u, 4095u}) {
      float acc = 0.f;
      for (int j = -(int)smooth; j <= (int)smooth; ++j) acc = acc + P[(size_t)(((int)k + j + (int)kCsN) % (int)kCsN)];
      if (cs_smooth(P.data(), k, smooth) != acc / (float)(2u * smooth + 1u)) ++bad;
    }
  CHECK(bad == 0, "%u smoothed values differ from their definition", bad);
}

int main() {
  check_runs();
  check_records();
  check_smooth();
  printf("%u checks, %u failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
