// tests/track_host.hip — the integer arithmetic of lsdr_derotate_batch and the frame plan of lsdr_tune_track on the host
// (leansdr_amd/csrc/derotate_batch_device.h, tune_track_device.h), built and run by tests/test_tune_track_host.py (host side only,
// AddressSanitizer and UBSan).  No GPU call is made.
//
// It reads cases from its standard input and answers on its standard output; the test compares the answers with Python integers.
//   "K k q" then k lines "sample tune" (tune as a C99 hex float), then q samples to ask for:
//        → "rule bad", and where rule is 0: "count", count lines "start phi F S", q lines "segment phase freq"
//   "F n blocks hop_blocks" → "frames" and the frames' first blocks on one line
//   "R center k0 l c r sum blocks min_quality" (floats as hex floats) → "held bin tune quality mean_power" (floats as hex floats)
#include <cinttypes>
#include <cstdio>
#include <vector>
#include "derotate_batch_device.h"
#include "tune_track_device.h"

void lsdr_set_error(const char *, ...) {}

int main() {
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'K') {
      unsigned k, q;
      if (scanf("%u %u", &k, &q) != 2) return 2;
      std::vector<dr_knot> knots(k);
      for (unsigned i = 0; i < k; ++i)
        if (scanf("%" SCNu64 " %la", &knots[i].sample, &knots[i].tune) != 2) return 2;
      std::vector<uint64_t> ask(q);
      for (unsigned i = 0; i < q; ++i)
        if (scanf("%" SCNu64, &ask[i]) != 1) return 2;
      std::vector<dr_seg> segs(k + 1u, dr_seg{~0ull, ~0ull, ~0ull, ~0ull});
      unsigned count = 0, bad = 0;
      const int rule = dr_build(knots.data(), k, segs.data(), &count, &bad);
      printf("%d %u\n", rule, bad);
      if (rule) {
        for (const dr_seg &g : segs)
          if (g.start != ~0ull || g.S != ~0ull) return 3;                  // (a refused track writes nothing)
        continue;
      }
      printf("%u\n", count);
      for (unsigned i = 0; i < count; ++i) printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", segs[i].start, segs[i].phi, segs[i].F, segs[i].S);
      for (uint64_t n : ask) {
        const unsigned si = dr_find(segs.data(), count, n);
        printf("%u %" PRIu64 " %" PRIu64 "\n", si, dr_phase(segs[si], n), dr_freq(segs[si], n));
      }
    } else if (kind == 'F') {
      unsigned long long n;
      unsigned blocks, hop_blocks;
      if (scanf("%llu %u %u", &n, &blocks, &hop_blocks) != 3) return 2;
      const tt_plan p = tt_frames(n, blocks, hop_blocks);
      printf("%llu\n", p.frames);
      for (unsigned long long f = 0; f < p.frames; ++f) printf("%llu ", tt_frame_block(p, f, hop_blocks));
      printf("\n");
    } else if (kind == 'R') {
      uint64_t center;
      unsigned k0, blocks;
      float l, c, r, sum, minq;
      if (scanf("%" SCNu64 " %u %a %a %a %a %u %a", &center, &k0, &l, &c, &r, &sum, &blocks, &minq) != 8) return 2;
      const tt_record R = tt_frame_record(center, k0, l, c, r, sum, blocks, minq);
      const te_record E = te_peak_record(k0, l, c, r, sum, blocks);
      if (R.center != center || R.tune != E.tune || R.quality != E.quality || R.bin != E.bin || R.power[0] != l || R.power[1] != c || R.power[2] != r ||
          R.mean_power != E.mean_power)
        return 4;                                                          // (field for field lsdr_tune_est's record of the same powers)
      printf("%u %u %a %a %a\n", R.held, R.bin, (double)R.tune, (double)R.quality, (double)R.mean_power);
    } else
      return 2;
  }
  return 0;
}
