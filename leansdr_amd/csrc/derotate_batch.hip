// leansdr_amd/csrc/derotate_batch.hip — lsdr_derotate_batch: a carrier track, GIVEN by the caller as knots (sample, tune), taken out of B
// captures in one launch, in front of the batch decoders.  Every capture, in any of the five sample formats, with its own length and its own
// knots, is converted and multiplied by exp(−j·2π·φ(n)/2^64) into a cf32 stream that lsdr_capture_batch decodes as LSDR_IN_CF32 with tune 0.
// include/lsdr_hip.h states the arithmetic; derotate_batch_device.h is that arithmetic (the host turns the knots into segments (Φ, F, S)
// there and uploads them with the run), one rounding per float operation (-ffp-contract=off).
//
//   k_derotate<K>  blockIdx.y = capture, blockIdx.x = a contiguous span of 256·kDrPieces 16-byte pieces of the capture, one workgroup of
//                  256.  A thread's 16-byte loads are issued first, all in flight together.  The span's first segment is found once, by
//                  binary search (the same in every thread: scalar loads); a piece that ends in front of that segment's end takes it
//                  from registers, any other steps on from there.  Inside a piece the phase goes from sample to sample by φ += f, f += S — exact, since
//                  everything wraps modulo 2^64 — and is taken anew from the next segment where a boundary falls inside the piece.
//                  One 16-byte load per piece where the capture's pointer is 16-byte aligned and the piece ends inside the capture, item
//                  by item otherwise: the same values.  Two samples leave in one 16-byte store — through LDS within a wavefront, so that
//                  neighbouring lanes store neighbouring addresses — a capture's odd last sample in one of 8.
//
// Memory-bound: 2 to 8 bytes read and 8 written per sample, plus the 512 KB table (L2-resident; neighbouring samples read neighbouring
// entries).  A workgroup leaves by its own capture's length before it forms any address; nothing behind item n − 1 is read or written.
// No atomics, no order that depends on scheduling: a capture's output is a pure function of its samples and its knots.
#include <vector>
#include "derotate_batch_device.h"

namespace {

constexpr unsigned kDrThreads = 256, kDrPieces = 4;                        // pieces per thread
constexpr unsigned kDrMaxKnots = 1u << 20;                                 // of one capture
constexpr unsigned long long kDrMaxTable = 1ull << 22;                     // segments of all captures of an object: 128 MB, pinned and on the device

struct dr_cap {
  const unsigned char *in;
  float2 *out;
  unsigned long long n;
  unsigned seg0, segs;                                                     // its segments: [seg0, seg0 + segs) of the table
};
static_assert(sizeof(dr_cap) == 32, "dr_cap is uploaded as an array");

struct dr_args {
  const dr_cap *caps;
  const dr_seg *table;
  const float2 *tab;                                                       // [65536] (cos, sin)(2πj/65536): lsdr_trig16_table
  float in_scale;
  unsigned in_flip;
};

template <int K>
__global__ __launch_bounds__(kDrThreads) void k_derotate(dr_args A) {
  constexpr unsigned kB = in_item<K>::kBytes, kPer = 16u / kB;
  constexpr unsigned long long kSpan = (unsigned long long)kDrThreads * kDrPieces * kPer;
  const dr_cap cap = A.caps[blockIdx.y];
  const unsigned long long n0 = (unsigned long long)blockIdx.x * kSpan;
  if (n0 >= cap.n) return;                                                 // by the capture's own length, before any address of it is formed
  const dr_seg *segs = A.table + cap.seg0;
  const bool wide = ((size_t)cap.in & 15u) == 0;
  // the span's first segment, once: the same in every thread (scalar loads), and the one most pieces lie in whole
  const unsigned s0 = dr_find(segs, cap.segs, n0);
  const dr_seg g0 = segs[s0];
  const unsigned long long next0 = s0 + 1u < cap.segs ? segs[s0 + 1u].start : ~0ull;
  // the pieces' loads first, all in flight together: piece p of this thread starts at item i0(p); 16 bytes where the pointer is 16-byte
  // aligned and the piece ends inside the capture
  uint4 w[kDrPieces];
#pragma unroll
  for (unsigned p = 0; p < kDrPieces; ++p) {
    const unsigned long long i0 = n0 + ((unsigned long long)p * kDrThreads + threadIdx.x) * kPer;
    if (wide && i0 + kPer <= cap.n) w[p] = *reinterpret_cast<const uint4 *>(cap.in + (size_t)i0 * kB);
  }
  // The outputs leave through LDS, wavefront by wavefront: a thread holds kPer/2 16-byte pairs that are 8·kPer bytes apart from its
  // neighbour's, and a store should find neighbouring lanes at neighbouring addresses.  A wavefront's 64·kPer/2 pairs go to its own
  // region (one pair of padding per 16: the threads' strided writes then meet no bank twice) and come back lane by lane.  No workgroup
  // barrier: a wavefront reads only what it wrote itself, in program order.
  constexpr unsigned kH = kPer / 2u, kPairs = 64u * kH;
  __shared__ float4 tr[kDrThreads / 64u][kPairs + kPairs / 16u];
  const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
#pragma unroll
  for (unsigned p = 0; p < kDrPieces; ++p) {
    const unsigned long long c0 = n0 + ((unsigned long long)p * kDrThreads + wv * 64u) * kPer;      // the wavefront's first item of this pass
    if (c0 >= cap.n) break;                                                // (the same in the whole wavefront; later passes are behind the end too)
    const unsigned long long i0 = c0 + (unsigned long long)lane * kPer;
    float2 y[kPer];
    if (i0 < cap.n) {
    const bool whole = i0 + kPer <= cap.n;
    float2 z[kPer];
    if (wide && whole) {
      const unsigned ws[4] = {w[p].x, w[p].y, w[p].z, w[p].w};
#pragma unroll
      for (unsigned q = 0; q < kPer; ++q) z[q] = in_unpack<K>(ws, q, A.in_scale, A.in_flip);
    } else {
#pragma unroll
      for (unsigned q = 0; q < kPer; ++q) z[q] = i0 + q < cap.n ? in_load<K>(cap.in, (size_t)(i0 + q), A.in_scale, A.in_flip) : make_float2(0.f, 0.f);
    }
    // the piece's segment: the span's first one where the piece ends in front of the next boundary (no memory read), else stepped to
    dr_seg g = g0;
    unsigned long long next = next0;
    unsigned si = s0;
    if (i0 + kPer > next0) {
      si += dr_find(segs + si, cap.segs - si, i0);                         // (segs[s0].start ≤ n0 ≤ i0: a search, however dense the knots)
      g = segs[si];
      next = si + 1u < cap.segs ? segs[si + 1u].start : ~0ull;
    }
    uint64_t phi = dr_phase(g, i0), f = dr_freq(g, i0);
#pragma unroll
    for (unsigned q = 0; q < kPer; ++q) {
      if (q) {
        if (i0 + q >= next) {                                              // a boundary inside the piece: the next segment from its own start
          ++si;
          g = segs[si];
          next = si + 1u < cap.segs ? segs[si + 1u].start : ~0ull;
          phi = dr_phase(g, i0 + q); f = dr_freq(g, i0 + q);
        } else { phi += f; f += g.S; }
      }
      const float2 cs = A.tab[(unsigned)(phi >> 48)];
      y[q] = make_float2(z[q].x * cs.x + z[q].y * cs.y, z[q].y * cs.x - z[q].x * cs.y);
    }
    }
    float2 *out = cap.out + c0;
    if constexpr (kH == 1u) {                                              // cf32: a thread's pair is its lane's place already
      if (i0 + 1u < cap.n) *reinterpret_cast<float4 *>(out + 2u * lane) = make_float4(y[0].x, y[0].y, y[1].x, y[1].y);
      else if (i0 < cap.n) out[2u * lane] = y[0];
    } else {
      if (i0 < cap.n) {
#pragma unroll
        for (unsigned k = 0; k < kH; ++k) {
          const unsigned s = lane * kH + k;                                // pair s of the wavefront: items c0 + 2s, c0 + 2s + 1
          tr[wv][s + s / 16u] = make_float4(y[2 * k].x, y[2 * k].y, y[2 * k + 1].x, y[2 * k + 1].y);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (unsigned j = 0; j < kH; ++j) {
        const unsigned s = j * 64u + lane;
        const unsigned long long i = c0 + 2ull * s;
        if (i < cap.n) {                                                   // (its writer's piece begins at or before item i: it was written)
          const float4 v = tr[wv][s + s / 16u];
          if (i + 1u < cap.n) *reinterpret_cast<float4 *>(out + 2u * s) = v;
          else out[2u * s] = make_float2(v.x, v.y);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                // (the next pass writes the region again)
      __builtin_amdgcn_wave_barrier();
    }
  }
}

}  // namespace

struct lsdr_derotate_batch {
  lsdr_ctx *ctx = nullptr;
  lsdr_derotate_batch_cfg cfg{};
  lsdr_in_desc in{};
  dr_args A{};
  in_run<dr_cap> run;
  float2 *d_tab = nullptr;
  dr_seg *h_table = nullptr, *d_table = nullptr;                           // room for [captures][max_knots + 1]; a run's segments stand packed, capture behind capture
  std::vector<dr_seg> staged;                                              // a run's table while its arguments are checked
  std::vector<unsigned> counts;
};
static_assert(sizeof(dr_knot) == sizeof(lsdr_track_knot) && sizeof(dr_knot) == 16, "lsdr_track_knot is dr_knot");

extern "C" {

void lsdr_derotate_batch_destroy(lsdr_derotate_batch *b) {
  if (!b) return;
  (void)hipStreamSynchronize(b->ctx->stream);
  b->run.destroy();
  lsdr_in_free({b->d_tab, b->d_table}, {b->h_table});
  delete b;
}

static int dr_create(lsdr_derotate_batch *b) {
  lsdr_ctx *c = b->ctx;
  const size_t B = (size_t)b->cfg.n_captures, rows = B * ((size_t)b->cfg.max_knots + 1u);
  LSDR_HIP(hipSetDevice(c->device));
  LSDR_TRY(b->run.create(B));
  LSDR_HIP(hipMalloc((void **)&b->d_tab, 65536 * sizeof(float2)));
  LSDR_HIP(hipHostMalloc((void **)&b->h_table, rows * sizeof(dr_seg), hipHostMallocDefault));
  LSDR_HIP(hipMalloc((void **)&b->d_table, rows * sizeof(dr_seg)));
  std::vector<lsdr_cf32> tab(65536);
  lsdr_trig16_table(tab.data());
  LSDR_HIP(hipMemcpy(b->d_tab, tab.data(), tab.size() * sizeof(lsdr_cf32), hipMemcpyHostToDevice));
  b->staged.resize(rows);
  b->counts.assign(B, 0u);
  dr_args &A = b->A;
  A.caps = b->run.d_caps; A.table = b->d_table; A.tab = b->d_tab; A.in_scale = b->in.in_scale; A.in_flip = b->in.in_flip;
  return LSDR_OK;
}

int lsdr_derotate_batch_create(lsdr_ctx *c, const lsdr_derotate_batch_cfg *cfg, lsdr_derotate_batch **out) {
  LSDR_ARG(c && cfg && out);
  if (cfg->n_captures < 1 || cfg->n_captures > 65535) { lsdr_set_error("derotate_batch: n_captures must be 1 to 65535 (got %d)", cfg->n_captures); return LSDR_E_ARG; }
  lsdr_in_desc in;
  LSDR_TRY(lsdr_in_describe("derotate_batch", cfg->in_format, cfg->in_scale, &in));
  if (cfg->max_knots > kDrMaxKnots) { lsdr_set_error("derotate_batch: max_knots is %u, at most %u", cfg->max_knots, kDrMaxKnots); return LSDR_E_ARG; }
  if ((unsigned long long)cfg->n_captures * (cfg->max_knots + 1ull) > kDrMaxTable) {
    lsdr_set_error("derotate_batch: n_captures %d times max_knots + 1 (%u) exceeds the table's %llu segments", cfg->n_captures, cfg->max_knots + 1u, kDrMaxTable);
    return LSDR_E_ARG;
  }
  for (int i = 0; i < 4; ++i)
    if (cfg->reserved[i]) { lsdr_set_error("derotate_batch: lsdr_derotate_batch_cfg.reserved must be 0"); return LSDR_E_ARG; }
  lsdr_derotate_batch *b = new lsdr_derotate_batch();
  b->ctx = c; b->cfg = *cfg; b->in = in;
  const int rc = dr_create(b);
  if (rc) { lsdr_derotate_batch_destroy(b); return rc; }
  *out = b;
  return LSDR_OK;
}

int lsdr_derotate_batch_run_async(lsdr_derotate_batch *b, const void *const *iq_dev, const lsdr_derotate_each *each, lsdr_cf32 *const *out_dev) {
  LSDR_ARG(b && iq_dev && each && out_dev);
  const unsigned B = (unsigned)b->cfg.n_captures;
  size_t used = 0;                                                         // segments of the captures in front: the table is packed, and only what a run uses is copied
  for (unsigned i = 0; i < B; ++i) {
    const lsdr_derotate_each &e = each[i];
    if (e.n_samples > b->cfg.max_samples) { lsdr_set_error("derotate_batch: capture %u: n_samples %zu exceeds max_samples %zu", i, e.n_samples, b->cfg.max_samples); return LSDR_E_ARG; }
    if (e.reserved) { lsdr_set_error("derotate_batch: capture %u: lsdr_derotate_each.reserved must be 0", i); return LSDR_E_ARG; }
    if (!iq_dev[i] && e.n_samples) { lsdr_set_error("derotate_batch: capture %u has samples and no pointer", i); return LSDR_E_ARG; }
    if ((size_t)iq_dev[i] % b->in.item_bytes) { lsdr_set_error("derotate_batch: capture %u: the pointer is not aligned to the item size (%u bytes)", i, b->in.item_bytes); return LSDR_E_ARG; }
    if (!out_dev[i] && e.n_samples) { lsdr_set_error("derotate_batch: capture %u has samples and no output pointer", i); return LSDR_E_ARG; }
    if ((size_t)out_dev[i] % 16u) { lsdr_set_error("derotate_batch: capture %u: the output pointer is not aligned to 16 bytes", i); return LSDR_E_ARG; }
    if (e.n_knots > b->cfg.max_knots) { lsdr_set_error("derotate_batch: capture %u: %u knots exceed max_knots %u", i, e.n_knots, b->cfg.max_knots); return LSDR_E_ARG; }
    if (e.n_knots && !e.knots) { lsdr_set_error("derotate_batch: capture %u has %u knots and no knot pointer", i, e.n_knots); return LSDR_E_ARG; }
    unsigned bad = 0;
    const int rule = dr_build(reinterpret_cast<const dr_knot *>(e.knots), e.n_knots, b->staged.data() + used, &b->counts[i], &bad);
    if (rule) {
      static const char *const what[] = {"", "its sample must lie below 2^31", "the samples must ascend strictly", "its tune must be finite and inside (-0.5, 0.5) cycles per sample",
                                         "the tune must change by less than 0.5 cycles per sample between neighbours"};
      lsdr_set_error("derotate_batch: capture %u: knot %u: %s", i, bad, what[rule]);
      return LSDR_E_ARG;
    }
    used += b->counts[i];
  }
  LSDR_TRY(b->run.idle("derotate_batch", "lsdr_derotate_batch_wait"));     // (the pinned table and records belong to the run in flight until then)
  lsdr_ctx *c = b->ctx;
  LSDR_HIP(hipSetDevice(c->device));
  unsigned long long longest = 0;
  unsigned seg0 = 0;
  for (unsigned i = 0; i < B; ++i) {
    dr_cap &cap = b->run.h_caps[i];
    cap.in = reinterpret_cast<const unsigned char *>(iq_dev[i]);
    cap.out = reinterpret_cast<float2 *>(out_dev[i]);
    cap.n = each[i].n_samples;
    cap.seg0 = seg0; cap.segs = b->counts[i];
    seg0 += b->counts[i];
    if (cap.n > longest) longest = cap.n;
  }
  memcpy(b->h_table, b->staged.data(), used * sizeof(dr_seg));
  const unsigned long long span = (unsigned long long)kDrThreads * kDrPieces * (16u / b->in.item_bytes);
  const unsigned long long groups = (longest + span - 1u) / span;
  if (groups > 0x7fffffffull) { lsdr_set_error("derotate_batch: %llu workgroups exceed one launch", groups); return LSDR_E_UNSUPPORTED; }
  LSDR_TRY(b->run.upload(c->stream));
  LSDR_HIP(hipMemcpyAsync(b->d_table, b->h_table, used * sizeof(dr_seg), hipMemcpyHostToDevice, c->stream));
  if (groups) {
    in_dispatch(b->in.kind, [&](auto K) { hipLaunchKernelGGL(k_derotate<K()>, dim3((unsigned)groups, B), dim3(kDrThreads), 0, c->stream, b->A); });
    LSDR_HIP(hipGetLastError());
  }
  return b->run.mark(c->stream);
}

int lsdr_derotate_batch_wait(lsdr_derotate_batch *b) {
  LSDR_ARG(b);
  return b->run.wait("derotate_batch");
}

}  // extern "C"
