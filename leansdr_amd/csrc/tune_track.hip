// leansdr_amd/csrc/tune_track.hip — lsdr_tune_track: every capture's carrier offset ALONG its length, for captures whose carrier moves by
// more than the batch decoders' tuning window.  lsdr_tune_est's estimator (the line of the fourth power, tune_est.hip) is run on frames of
// `blocks` blocks every `hop` samples and once more at the capture's end; a gate of ± span bins around the last accepted frame's peak keeps
// the walk on the carrier, and a frame whose quality is below min_quality is held: recorded, but no knot of the track and no move of the
// gate.  The records are what lsdr_derotate_batch's knots are made of (derotate_batch.hip).  No decode kernel is involved.
//
//   k_tt_block<K>   blockIdx.y = capture, blockIdx.x = frame·blocks + block, one workgroup of 256: k_te_block's steps on block `block` of
//                   the frame — 16-byte loads (item-wise where the capture's pointer is only item-aligned), the converted block in LDS, its
//                   RMS, z⁴ in place, six radix-4 stages, |X|² in natural order as one row of 4096 floats of scratch
//   k_tt_sum        blockIdx.y = capture, blockIdx.x = frame: the frame's rows summed in block order into its first row (P), the first
//                   maximum over all bins and Σ P — k_te_peak's steps, for every frame at once
//   k_tt_walk       one workgroup per capture walks its frames in order — the gate makes that serial, so only the gate is left to it: an
//                   ungated frame takes k_tt_sum's peak, a gated one the first maximum of the gate's 2·span + 1 bins of P in their order
//                   b − span … b + span; neighbours, mean; thread 0 writes the record, keeps the summary and the gate's bin, which the
//                   workgroup reads behind the frame's last barrier.  (With the sums inside the walk, 32 captures of 129 frames took
//                   6.9 ms)
//
// Determinism: no atomics; every sum has a fixed order that depends on the sample's index alone, and the gate is a function of the frames
// in front of it — a capture's records are a pure function of its converted samples: the same bits alone, in any batch, in any place of it,
// and for every format that converts to the same floats.  Frame 0 is lsdr_tune_est's record of the same capture with the same `blocks`,
// bit for bit: the same steps in the same order.  All three kernels leave by the capture's own frame count: nothing behind a capture's last
// whole block is read, and nothing at all of one without a frame.
#include <cmath>
#include <vector>
#include "tune_track_device.h"

namespace {

struct tt_cap { const unsigned char *in; unsigned long long n; };          // one capture of a run
static_assert(sizeof(tt_cap) == 16, "tt_cap is uploaded as an array");

struct tt_peak { unsigned bin; float sum; };

struct tt_args {
  const tt_cap *caps;
  const float2 *tw;                    // [4096] exp(−j2π·i/4096)
  float *rows;                         // [captures][max_frames][blocks][4096] |X|² of every block of every frame; k_tt_sum leaves P in a frame's first row
  tt_record *rec;                      // [captures][max_frames]
  tt_summary *sum;                     // [captures]
  tt_peak *peaks;                      // [captures][max_frames] every frame's first maximum over all bins and Σ P
  unsigned blocks, hop_blocks, span, max_frames;
  float min_quality;
  float in_scale;
  unsigned in_flip;
};
static_assert(sizeof(tt_record) == sizeof(lsdr_track_frame) && sizeof(tt_record) == 40, "lsdr_track_frame is tt_record");
static_assert(sizeof(tt_summary) == sizeof(lsdr_track_summary) && sizeof(tt_summary) == 28, "lsdr_track_summary is tt_summary");

template <int K>
__global__ __launch_bounds__(256) void k_tt_block(tt_args A) {
  const tt_cap cap = A.caps[blockIdx.y];
  const tt_plan plan = tt_frames(cap.n, A.blocks, A.hop_blocks);
  const unsigned frame = blockIdx.x / A.blocks, j = blockIdx.x - frame * A.blocks;
  if (frame >= plan.frames) return;                                        // by the capture's own frames, before any address of it is formed
  __shared__ float2 x[kTeN];
  __shared__ float red[1][4];
  const unsigned t = threadIdx.x;
  bs_stage<K>(cap.in, (unsigned)(tt_frame_block(plan, frame, A.hop_blocks) + j), A.in_scale, A.in_flip, x);
  float p[1] = {0.f};
  for (unsigned i = 0; i < kTeN / 256u; ++i) { const float2 z = x[t + 256u * i]; p[0] += z.x * z.x + z.y * z.y; }
  bs_sum256(p, red);
  const float inv = p[0] > 0.f ? 1.0f / sqrtf(p[0] * (1.0f / (float)kTeN)) : 0.f;
  for (unsigned i = 0; i < kTeN / 256u; ++i) x[t + 256u * i] = te_pow4(x[t + 256u * i], inv);     // (each thread its own samples: no barrier in front)
  bs_fft(x, A.tw);
  float *row = A.rows + (((size_t)blockIdx.y * A.max_frames + frame) * A.blocks + j) * kTeN;
  for (unsigned i = 0; i < kTeN / 256u; ++i) {
    const unsigned k = t + 256u * i;
    const float2 v = x[bs_digit_reverse(k)];
    row[k] = v.x * v.x + v.y * v.y;
  }
}

// A frame's rows summed in block order into its first row, P; the first maximum over all bins and Σ P, as k_te_peak takes them.
__global__ __launch_bounds__(256) void k_tt_sum(tt_args A) {
  const tt_cap cap = A.caps[blockIdx.y];
  const tt_plan plan = tt_frames(cap.n, A.blocks, A.hop_blocks);
  if (blockIdx.x >= plan.frames) return;
  const unsigned t = threadIdx.x;
  __shared__ bs_peak_lds sh;
  float *rows = A.rows + ((size_t)blockIdx.y * A.max_frames + blockIdx.x) * A.blocks * kTeN;
  float sum = 0.f, best = -1.f;
  unsigned bk = 0;
  for (unsigned i = 0; i < kTeN / 256u; ++i) {
    const unsigned k = t + 256u * i;
    float p = 0.f;
    for (unsigned j = 0; j < A.blocks; ++j) p += rows[(size_t)j * kTeN + k];
    rows[k] = p; sum += p;                                   // (in place: this thread alone reads and writes bin k)
    if (p > best) { best = p; bk = k; }                      // ascending k: the first maximum of this thread's bins
  }
  bs_first_max(best, bk, sum, sh);
  if (t == 0) A.peaks[(size_t)blockIdx.y * A.max_frames + blockIdx.x] = tt_peak{bk, sum};
}

// One workgroup per capture walks its frames in order.  What is serial is small: an ungated frame takes k_tt_sum's peak, a gated one the
// first maximum of the gate's 2·span + 1 bins of P.
__global__ __launch_bounds__(256) void k_tt_walk(tt_args A) {
  const tt_cap cap = A.caps[blockIdx.x];
  const tt_plan plan = tt_frames(cap.n, A.blocks, A.hop_blocks);
  const unsigned t = threadIdx.x;
  __shared__ bs_peak_lds sh;
  __shared__ unsigned gate[2];                                             // {a frame was accepted, its bin}: thread 0 writes between a frame's two barriers, all read between frames
  tt_summary S = {};
  if (t == 0) { gate[0] = 0u; gate[1] = 0u; }
  __syncthreads();
  for (unsigned f = 0; f < (unsigned)plan.frames; ++f) {
    const float *P = A.rows + ((size_t)blockIdx.x * A.max_frames + f) * A.blocks * kTeN;
    const tt_peak pk = A.peaks[(size_t)blockIdx.x * A.max_frames + f];
    const bool gated = A.span != 0u && gate[0] != 0u;
    const unsigned b = gate[1];
    __syncthreads();                                         // every thread holds the gate in registers before thread 0 may write it: one decision for the workgroup
    unsigned bk = pk.bin;
    if (gated) {                                             // the gate's bins in their order: position q ↔ bin b − span + q (mod N)
      float best = -1.f, unused = 0.f;
      bk = 0;
      for (unsigned q = t; q <= 2u * A.span; q += 256u) {
        const float p = P[(b + kTeN - A.span + q) & (kTeN - 1u)];
        if (p > best) { best = p; bk = q; }                  // ascending q: the first maximum of this thread's positions
      }
      bs_first_max(best, bk, unused, sh);                    // (among equals the smaller position)
      bk = (b + kTeN - A.span + bk) & (kTeN - 1u);           // (thread 0's is the workgroup's)
    }
    if (t == 0) {
      const uint64_t center = (tt_frame_block(plan, f, A.hop_blocks) * kTeN) + (uint64_t)A.blocks * (kTeN / 2u);
      const tt_record R = tt_frame_record(center, bk, P[(bk + kTeN - 1u) & (kTeN - 1u)], P[bk], P[(bk + 1u) & (kTeN - 1u)], pk.sum, A.blocks, A.min_quality);
      A.rec[(size_t)blockIdx.x * A.max_frames + f] = R;
      tt_summarise(S, R);
      if (!R.held) { gate[0] = 1u; gate[1] = R.bin; }
    }
    __syncthreads();                                         // thread 0 has read sh and written the gate: the next frame may read the one and overwrite the other
  }
  if (t == 0) A.sum[blockIdx.x] = S;                         // (no frame: all zeros)
}

}  // namespace

struct lsdr_tune_track {
  lsdr_ctx *ctx = nullptr;
  lsdr_tune_track_cfg cfg{};                                 // with the defaults filled in
  lsdr_in_desc in{};
  tt_args A{};
  in_run<tt_cap> run;
  float2 *d_tw = nullptr;
  float *d_rows = nullptr;
  tt_record *h_rec = nullptr, *d_rec = nullptr;
  tt_summary *h_sum = nullptr, *d_sum = nullptr;
  tt_peak *d_peaks = nullptr;
};

extern "C" {

void lsdr_tune_track_destroy(lsdr_tune_track *e) {
  if (!e) return;
  (void)hipStreamSynchronize(e->ctx->stream);
  e->run.destroy();
  lsdr_in_free({e->d_tw, e->d_rows, e->d_rec, e->d_sum, e->d_peaks}, {e->h_rec, e->h_sum});
  delete e;
}

static int tt_build(lsdr_tune_track *e) {
  lsdr_ctx *c = e->ctx;
  const size_t B = (size_t)e->cfg.n_captures, F = e->cfg.max_frames;
  LSDR_HIP(hipSetDevice(c->device));
  LSDR_TRY(e->run.create(B));
  LSDR_HIP(hipHostMalloc((void **)&e->h_rec, B * F * sizeof(tt_record), hipHostMallocDefault));
  LSDR_HIP(hipHostMalloc((void **)&e->h_sum, B * sizeof(tt_summary), hipHostMallocDefault));
  memset(e->h_rec, 0, B * F * sizeof(tt_record));
  memset(e->h_sum, 0, B * sizeof(tt_summary));
  LSDR_HIP(hipMalloc((void **)&e->d_rec, B * F * sizeof(tt_record)));
  LSDR_HIP(hipMalloc((void **)&e->d_sum, B * sizeof(tt_summary)));
  LSDR_HIP(hipMalloc((void **)&e->d_peaks, B * F * sizeof(tt_peak)));
  LSDR_HIP(hipMemcpy(e->d_rec, e->h_rec, B * F * sizeof(tt_record), hipMemcpyHostToDevice));      // (zeros: the records behind a capture's last frame are never written)
  LSDR_HIP(hipMalloc((void **)&e->d_rows, B * F * e->cfg.blocks * kTeN * sizeof(float)));
  LSDR_HIP(hipMalloc((void **)&e->d_tw, kTeN * sizeof(float2)));
  std::vector<float2> tw(kTeN);
  for (unsigned i = 0; i < kTeN; ++i) {                      // (bs_host's table)
    const double a = -2.0 * M_PI * (double)i / (double)kTeN;
    tw[i] = make_float2((float)cos(a), (float)sin(a));
  }
  LSDR_HIP(hipMemcpy(e->d_tw, tw.data(), kTeN * sizeof(float2), hipMemcpyHostToDevice));
  tt_args &A = e->A;
  A.caps = e->run.d_caps; A.tw = e->d_tw; A.rows = e->d_rows; A.rec = e->d_rec; A.sum = e->d_sum; A.peaks = e->d_peaks;
  A.blocks = e->cfg.blocks; A.hop_blocks = e->cfg.hop / kTeN; A.span = e->cfg.span; A.max_frames = e->cfg.max_frames;
  A.min_quality = e->cfg.min_quality; A.in_scale = e->in.in_scale; A.in_flip = e->in.in_flip;
  return LSDR_OK;
}

int lsdr_tune_track_create(lsdr_ctx *c, const lsdr_tune_track_cfg *cfg_in, lsdr_tune_track **out) {
  LSDR_ARG(c && cfg_in && out);
  lsdr_tune_track_cfg cfg = *cfg_in;
  LSDR_TRY(bs_check_captures("tune_track", cfg.n_captures));
  lsdr_in_desc in;
  LSDR_TRY(lsdr_in_describe("tune_track", cfg.in_format, cfg.in_scale, &in));
  if (cfg.blocks > kTtMaxBlocks) { lsdr_set_error("tune_track: blocks is %u, at most %u", cfg.blocks, kTtMaxBlocks); return LSDR_E_ARG; }
  if (cfg.hop % kTeN) { lsdr_set_error("tune_track: hop is %u, it must be a multiple of %u samples", cfg.hop, kTeN); return LSDR_E_ARG; }
  if (cfg.span > kTtMaxSpan) { lsdr_set_error("tune_track: span is %u bins, at most %u", cfg.span, kTtMaxSpan); return LSDR_E_ARG; }
  if (!std::isfinite(cfg.min_quality) || cfg.min_quality < 0.f) { lsdr_set_error("tune_track: min_quality must be finite and not negative"); return LSDR_E_ARG; }
  for (int i = 0; i < 4; ++i)
    if (cfg.reserved[i]) { lsdr_set_error("tune_track: lsdr_tune_track_cfg.reserved must be 0"); return LSDR_E_ARG; }
  if (!cfg.blocks) cfg.blocks = 4;
  if (!cfg.hop) cfg.hop = 65536;
  if (cfg.min_quality == 0.f) cfg.min_quality = 30.f;
  if (!cfg.max_frames) cfg.max_frames = 256;
  if ((unsigned long long)cfg.max_frames * cfg.blocks > 0x7fffffffull) { lsdr_set_error("tune_track: max_frames %u times blocks %u exceeds one launch", cfg.max_frames, cfg.blocks); return LSDR_E_ARG; }
  lsdr_tune_track *e = new lsdr_tune_track();
  e->ctx = c; e->cfg = cfg; e->in = in;
  const int rc = tt_build(e);
  if (rc) { lsdr_tune_track_destroy(e); return rc; }
  *out = e;
  return LSDR_OK;
}

int lsdr_tune_track_run_async(lsdr_tune_track *e, const void *const *iq_dev, const size_t *n_samples) {
  LSDR_ARG(e && iq_dev && n_samples);
  lsdr_ctx *c = e->ctx;
  const unsigned B = (unsigned)e->cfg.n_captures;
  LSDR_TRY(lsdr_in_check_each("tune_track", "tune", B, iq_dev, nullptr, n_samples, nullptr, ~(size_t)0, e->in.item_bytes));
  unsigned long long longest = 0;
  for (unsigned i = 0; i < B; ++i) {                         // (before anything is queued)
    if (n_samples[i] / kTeN > 0xffffffffull) { lsdr_set_error("tune_track: capture %u: n_samples %zu exceeds 2^44", i, n_samples[i]); return LSDR_E_ARG; }
    const tt_plan p = tt_frames(n_samples[i], e->A.blocks, e->A.hop_blocks);
    if (p.frames > e->cfg.max_frames) { lsdr_set_error("tune_track: capture %u: %llu frames exceed max_frames %u", i, p.frames, e->cfg.max_frames); return LSDR_E_ARG; }
    if (p.frames > longest) longest = p.frames;
  }
  LSDR_TRY(e->run.idle("tune_track", "lsdr_tune_track_wait"));
  LSDR_HIP(hipSetDevice(c->device));
  for (unsigned i = 0; i < B; ++i) {
    e->run.h_caps[i].in = reinterpret_cast<const unsigned char *>(iq_dev[i]);
    e->run.h_caps[i].n = n_samples[i];
  }
  LSDR_TRY(e->run.upload(c->stream));
  if (longest) {
    in_dispatch(e->in.kind, [&](auto K) { hipLaunchKernelGGL(k_tt_block<K()>, dim3((unsigned)longest * e->A.blocks, B), dim3(256), 0, c->stream, e->A); });
    hipLaunchKernelGGL(k_tt_sum, dim3((unsigned)longest, B), dim3(256), 0, c->stream, e->A);
  }
  hipLaunchKernelGGL(k_tt_walk, dim3(B), dim3(256), 0, c->stream, e->A);
  LSDR_HIP(hipGetLastError());
  LSDR_HIP(hipMemcpyAsync(e->h_rec, e->d_rec, (size_t)B * e->cfg.max_frames * sizeof(tt_record), hipMemcpyDeviceToHost, c->stream));
  LSDR_HIP(hipMemcpyAsync(e->h_sum, e->d_sum, (size_t)B * sizeof(tt_summary), hipMemcpyDeviceToHost, c->stream));
  return e->run.mark(c->stream);
}

int lsdr_tune_track_wait(lsdr_tune_track *e, lsdr_track_summary *summary, lsdr_track_frame *frames) {
  LSDR_ARG(e && summary);
  LSDR_TRY(e->run.wait("tune_track"));
  memcpy(summary, e->h_sum, e->run.n * sizeof(tt_summary));
  if (frames) memcpy(frames, e->h_rec, e->run.n * e->cfg.max_frames * sizeof(tt_record));
  return LSDR_OK;
}

unsigned lsdr_tune_track_max_frames(const lsdr_tune_track *e) { return e ? e->cfg.max_frames : 0u; }

}  // extern "C"
