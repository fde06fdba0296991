// tests/tail_relock_host.hip — the window and rewind arithmetic of the FEC tail's re-acquisition on the host (leansdr_amd/csrc/tail_relock.h),
// built and run by tests/test_tail_relock_host.py (host side only, AddressSanitizer and UBSan).  No GPU call is made.
//
// For the five code rates (punctperiod, punctweight of make_deconvol_sync_simple, dvb.h:480-513) and the windows 2048 and 8192, against a
// brute-force loop of SINGLE windows — deconvol_sync::run's sizes written out here from dvb.h:419-470, mpeg_sync's locked path taking
// whole packets with one byte of look-ahead (dvb.h:842-846):
//   · the split: relock_whole_windows counts no window the loop does not write whole, misses at most one, and ONE call with K·window bytes
//     of room writes K·window bytes and leaves the counters of K single windows; with room for the bytes running out as well;
//   · the rewind: for a drop in the first, a middle and the last packet a window makes readable, and for a packet whose look-ahead byte
//     is the last byte of a window (and the case one byte short of it), relock_drop_windows is the number of windows the loop has run
//     when mpeg_sync reaches the packet, and relock_plan_call / relock_after over those windows give the loop's counters there.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "tail_relock.h"

static unsigned g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) { ++g_failed; printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
  } while (0)

typedef unsigned long long u64;
struct dec { u64 pos, bw; int n_in, n_out; };

// deconvol_sync::run with `room` bytes writable (dvb.h:419-470), sizes only: returns the bytes it writes
static u64 run_once(int pp, int pw, u64 nsym, dec &d, u64 room) {
  const u64 readable = nsym - d.pos;
  if (readable < 64) return 0;
  long long maxrd = (long long)((readable - 64) / (u64)(pw / 2) * (u64)pp / 8);
  long long n = maxrd < (long long)room ? maxrd : (long long)room;
  if (n < 32) return 0;
  u64 used = 0;
  for (long long b = 0; b < n; ++b) {                      // readbyte, dvb.h:386-394: refill while fewer than 8 bits are pending
    while (d.n_out < 8) {
      while (d.n_in < 64) { ++used; d.n_in += 2; }         // one symbol = two bits into the shift register
      d.n_in -= pw; d.n_out += pp;
    }
    d.n_out -= 8;
  }
  d.pos += used; d.bw += (u64)n;
  return (u64)n;
}
static bool same(const dec &a, const relock_dec &b) { return a.pos == b.pos && a.bw == b.bw && a.n_in == b.n_in && a.n_out == b.n_out; }

static void check_stretch(int pp, int pw, u64 window, u64 nsym, u64 byte_cap, const dec &d0, const char *what) {
  const relock_dec s0 = {d0.pos, d0.bw, d0.n_in, d0.n_out};
  // the loop of single windows, until one is not whole
  std::vector<dec> after;                                  // after[j]: counters behind window j
  dec d = d0;
  while (true) {
    u64 room = byte_cap - d.bw;
    if (room > window) room = window;
    dec t = d;
    if (run_once(pp, pw, nsym, t, room) != window) break;
    d = t;
    after.push_back(d);
  }
  const u64 brute = after.size();
  const u64 K = relock_whole_windows(pp, pw, nsym, byte_cap, window, s0);
  CHECK(K <= brute && K + 1 >= brute, "%s pp %d window %llu nsym %llu: %llu whole windows, the loop writes %llu", what, pp, window, nsym, K, brute);
  for (u64 j = 0; j <= brute; ++j)
    CHECK(relock_window_whole(pp, pw, nsym, byte_cap, window, s0, j) == (j < brute), "%s pp %d window %llu nsym %llu: window %llu", what, pp, window, nsym, j);
  if (!K || K > brute) return;
  {
    const relock_call c = relock_plan_call(pp, pw, nsym, s0, K * window);
    CHECK(c.n == K * window, "%s pp %d window %llu: one call writes %llu of %llu bytes", what, pp, window, c.n, K * window);
    CHECK(same(after[K - 1], relock_after(pw, s0, c)), "%s pp %d window %llu nsym %llu: counters behind %llu windows", what, pp, window, nsym, K);
    dec one = d0;
    CHECK(run_once(pp, pw, nsym, one, K * window) == K * window && same(one, relock_after(pw, s0, c)), "%s pp %d: the one call itself", what, pp);
  }
  // drops: mpeg_sync is locked with `lead` bytes deconvolved and not yet taken
  for (u64 lead = 0; lead <= 204; lead += (lead == 0 || lead == 203) ? 1 : 101) {
    // packets readable behind window j: whole packets with one byte of look-ahead
    std::vector<u64> upto(K);
    for (u64 j = 0; j < K; ++j) { const u64 have = lead + (j + 1) * window; upto[j] = have >= 205 ? (have - 1) / 204 : 0; }
    auto drop = [&](u64 drop_at, const char *where) {
      u64 keep = 0;
      while (keep < K && upto[keep] <= drop_at) ++keep;    // the loop runs windows until the packet has been taken
      ++keep;
      if (keep > K) return;                                // (not a packet of this stretch)
      const u64 got = relock_drop_windows(drop_at, lead, window);
      CHECK(got == keep, "%s pp %d window %llu lead %llu drop at %llu (%s): %llu windows stand, the loop has run %llu", what, pp, window, lead, drop_at, where, got, keep);
      const relock_call c = relock_plan_call(pp, pw, nsym, s0, got * window);
      CHECK(got <= K && same(after[keep - 1], relock_after(pw, s0, c)), "%s pp %d window %llu lead %llu drop at %llu (%s): rewound counters", what, pp, window, lead, drop_at, where);
    };
    for (u64 j = 0; j < K; j = j < 2 ? j + 1 : (j + 1 < K - 1 ? K - 1 : j + 1)) {      // windows 0, 1, 2 and the last
      const u64 lo = j ? upto[j - 1] : 0, hi = upto[j];
      if (hi == lo) continue;
      drop(lo, "first packet of a window");
      drop(lo + (hi - lo) / 2, "a middle packet");
      drop(hi - 1, "last packet of a window");
      if (hi) drop(hi, "first packet behind the window");
    }
  }
  // a packet whose look-ahead byte is the last byte of window j: the lead that makes it so, and one byte less
  for (u64 j = 0; j < K && j < 3; ++j)
    for (u64 lead = 1; lead <= 204; ++lead) {
      const u64 have = lead + (j + 1) * window;
      if ((have - 1) % 204) continue;
      const u64 p = (have - 1) / 204 - 1;
      CHECK(relock_drop_windows(p, lead, window) == j + 1, "pp %d window %llu: look-ahead byte at the end of window %llu", pp, window, j);
      CHECK(relock_drop_windows(p, lead - 1, window) == j + 2, "pp %d window %llu: look-ahead byte one behind the end of window %llu", pp, window, j);
    }
}

int main() {
  const int rates[5][2] = {{1, 2}, {4, 6}, {3, 4}, {5, 6}, {7, 8}};        // 1/2, 2/3, 3/4, 5/6, 7/8: punctperiod, punctweight
  const u64 windows[2] = {2048, 8192};
  for (const auto &r : rates) {
    const int pp = r[0], pw = r[1];
    for (u64 window : windows) {
      const u64 sym_per_window = window * 8 / (u64)pp * (u64)(pw / 2);
      for (u64 extra = 0; extra < 5 * sym_per_window / 4; extra += sym_per_window / 16 + 1) {
        const u64 nsym = 6 * sym_per_window + extra;
        // a freshly constructed deconvolver
        check_stretch(pp, pw, window, nsym, 1ull << 40, dec{0, 0, 0, 0}, "fresh");
        // … and one that has run: a first window, three short calls (other bit counts), a symbol skipped
        dec d{0, 0, 0, 0};
        run_once(pp, pw, nsym, d, window);
        for (u64 odd : {33ull, 47ull, 101ull}) run_once(pp, pw, nsym, d, odd);
        d.pos += 1;
        check_stretch(pp, pw, window, nsym, 1ull << 40, d, "running");
        // the byte buffer ends first
        check_stretch(pp, pw, window, nsym, d.bw + 3 * window + 100, d, "room ends");
        check_stretch(pp, pw, window, nsym, d.bw + window - 1, d, "no room");
      }
      // around the sizes at which one more window becomes whole, symbol by symbol
      for (u64 nsym = 3 * sym_per_window - 40; nsym < 3 * sym_per_window + 140; ++nsym) check_stretch(pp, pw, window, nsym, 1ull << 40, dec{0, 0, 0, 0}, "edge");
    }
  }
  printf("tail_relock_host: %u checks, %u failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
