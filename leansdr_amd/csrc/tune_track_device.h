// leansdr_amd/csrc/tune_track_device.h — the arithmetic that is the carrier tracker's own (lsdr_tune_track, include/lsdr_hip.h; kernels and
// host side in tune_track.hip).  Plain C++ on values, callable from a kernel and from the host: where a capture's frames lie, and a frame's
// record.  The fourth power and the peak's interpolation are tune_est_device.h's, the blocks and the transform block_spectrum.h's.
#ifndef LSDR_TUNE_TRACK_DEVICE_H
#define LSDR_TUNE_TRACK_DEVICE_H
#include <cstdint>
#include "tune_est_device.h"

constexpr unsigned kTtMaxBlocks = 16, kTtMaxSpan = kTeN / 2u - 1u;

// The frames of a capture of n items, in blocks of kTeN samples: frame k < hop_frames starts at block k·hop_blocks; where end_block lies
// behind the last of them, one more frame starts there (frames = hop_frames + 1), so that the track reaches the capture's end.
struct tt_plan { unsigned long long frames, hop_frames, end_block; };
IN_HD tt_plan tt_frames(unsigned long long n, unsigned blocks, unsigned hop_blocks) {
  tt_plan p = {0, 0, 0};
  const unsigned long long whole = n / kTeN;
  if (whole < blocks) return p;                                            // n < blocks·N: no frame
  p.end_block = whole - blocks;                                            // ⌊(n − blocks·N)/N⌋
  p.hop_frames = p.end_block / hop_blocks + 1u;
  p.frames = p.hop_frames + (p.end_block > (p.hop_frames - 1u) * hop_blocks ? 1u : 0u);
  return p;
}
IN_HD unsigned long long tt_frame_block(const tt_plan &p, unsigned long long k, unsigned hop_blocks) { return k < p.hop_frames ? k * hop_blocks : p.end_block; }

struct tt_record { uint64_t center; float tune, quality; unsigned bin, held; float power[3], mean_power; };      // = lsdr_track_frame
struct tt_summary { unsigned frames, accepted; float tune_first, tune_last, tune_min, tune_max, quality_min; };  // = lsdr_track_summary

// A frame's record from its peak: lsdr_tune_est's record of the same powers, field for field
IN_HD tt_record tt_frame_record(uint64_t center, unsigned k0, float l, float c, float r, float sum, unsigned blocks, float min_quality) {
  const te_record e = te_peak_record(k0, l, c, r, sum, blocks);
  tt_record R;
  R.center = center; R.tune = e.tune; R.quality = e.quality; R.bin = e.bin;
  R.held = e.quality >= min_quality ? 0u : 1u;
  R.power[0] = e.power[0]; R.power[1] = e.power[1]; R.power[2] = e.power[2]; R.mean_power = e.mean_power;
  return R;
}
// the summary over the accepted frames, in frame order
IN_HD void tt_summarise(tt_summary &s, const tt_record &R) {
  ++s.frames;
  if (R.held) return;
  if (!s.accepted) { s.tune_first = s.tune_min = s.tune_max = R.tune; s.quality_min = R.quality; }
  s.tune_last = R.tune;
  if (R.tune < s.tune_min) s.tune_min = R.tune;
  if (R.tune > s.tune_max) s.tune_max = R.tune;
  if (R.quality < s.quality_min) s.quality_min = R.quality;
  ++s.accepted;
}
#endif
