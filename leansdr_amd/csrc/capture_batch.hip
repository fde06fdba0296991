// leansdr_amd/csrc/capture_batch.hip — lsdr_capture_batch (include/lsdr_hip.h): B independent cu8 captures from their first sample to TS,
// one set of launches for all of them, counts on the device.  Host-side glue only: the front end is cstln_receiver.hip's lsdr_rxb
// (rxb_device.h / rxb_host.h), the FEC tail fec.hip's lsdr_tail (tail_device.h / tail_host.h).
//
// Replaces, per capture, one `leandvb --u8 -f Fs --sr Fm --cr R` process of the reference (leandvb.cc:157-600: its default graph).
//
// The VITERBI engine (lsdr_capture_batch_create_viterbi) is `leandvb --u8 … --viterbi`: the front end writes soft symbols, one
// lsdr_viterbi_batch (a stream per capture) decodes them straight into the tail's byte buffers, and the tail runs without deconvol_sync.
// lsdr_viterbi_batch commits a prefix per call, so a batch takes several ROUNDS: run_async queues the front end and round 1 (symbol counts
// from device memory), wait drives the remaining rounds — one host read of B records each, every round shared by all captures — and then
// queues the tail.
//
// Other sample formats (lsdr_capture_any_create): `leandvb --s8 / --u16 / --s16 / --f32 --float-scale S` (leandvb.cc:208-261) in place of
// `--u8`.  Format and scale only select the front end's kernels (rxb_device.h converts in its loads); everything here is format-blind.
//
// Signal reports (lsdr_capture_reports_set / _get): leandvb's --fd-info per capture — FREQ, SS, MER once per meas_decimation samples
// (sdr.h:857-913).  The front end records and scans the estimators in its own launches (rxb_device.h); here only the libm scalars.
#include "capture_input.h"

struct lsdr_capture_batch {
  lsdr_ctx *ctx;                   // the context the front end's tiles run on: the caller's, or (aux_cus) an own one on the tile partition
  lsdr_ctx *ctx_aux;               // aux_cus: the own context of the auxiliary partition (null: everything on ctx)
  lsdr_ctx *own_main;              // aux_cus: ctx is ours
  lsdr_capture_batch_cfg cfg;
  lsdr_rxb *rx;
  lsdr_tail *tail;
  bool in_flight;
  std::vector<size_t> consumed;    // per capture, of the last batch
  // the Viterbi engine (vb != null)
  lsdr_viterbi_batch *vb;
  size_t soft_cap, byte_cap;
  std::vector<lsdr_capture_viterbi_stats> vstats;
  int in_format; float in_scale;   // lsdr_capture_input_cfg (cu8, 0 by default)
  lsdr_in_desc in;                 // … and what they come to
};

// one more round of the Viterbi stage: stream i continues behind what it has committed.  first: the symbol counts are still on the device.
static int capture_batch_viterbi_round(lsdr_capture_batch *b, bool first, const std::vector<unsigned long long> &total,
                                       const std::vector<unsigned long long> &done, const std::vector<unsigned long long> &bytes) {
  const int n = b->cfg.n_captures;
  std::vector<const lsdr_softsymbol *> in(n);
  std::vector<uint8_t *> out(n);
  std::vector<size_t> n_in(n);
  unsigned long long most = 0;
  for (int i = 0; i < n; ++i) {
    in[i] = lsdr_rxb_soft(b->rx, (unsigned)i) + done[i];
    out[i] = const_cast<uint8_t *>(lsdr_tail_bytes_dev(b->tail, (unsigned)i)) + bytes[i];
    n_in[i] = (size_t)(first ? b->soft_cap : total[i] - done[i]);
    if (bytes[i] > most) most = bytes[i];
  }
  return lsdr_viterbi_batch_run_async(b->vb, in.data(), n_in.data(), first ? reinterpret_cast<const uint64_t *>(lsdr_rxb_counts_dev(b->rx)) : nullptr,
                                      out.data(), b->byte_cap - (size_t)most);
}


extern "C" {

void lsdr_capture_batch_destroy(lsdr_capture_batch *b) {
  if (!b) return;
  if (b->ctx) (void)hipStreamSynchronize(b->ctx->stream);
  if (b->ctx_aux) (void)hipStreamSynchronize(b->ctx_aux->stream);
  lsdr_viterbi_batch_destroy(b->vb);
  lsdr_tail_destroy(b->tail);
  lsdr_rxb_destroy(b->rx);
  if (b->ctx_aux) lsdr_ctx_destroy(b->ctx_aux);
  if (b->own_main) lsdr_ctx_destroy(b->own_main);
  delete b;
}

// compute-unit masks of the two partitions: mask bit i = CU i % 32 of XCD i / 32 (8 XCDs of 32 CUs); the auxiliary partition takes the
// first aux/8 CUs of every XCD, the tiles the rest
static int capture_batch_partition(lsdr_capture_batch *b, lsdr_ctx *caller) {
  const unsigned aux = b->cfg.aux_cus, ncu = (unsigned)caller->num_cu;
  if (aux % 8 || aux >= ncu || ncu % 8 || ncu > 1024) { lsdr_set_error("capture_batch: aux_cus must be a multiple of 8 below the device's %u CUs (got %u)", ncu, aux); return LSDR_E_ARG; }
  const unsigned per = ncu / 8, words = (ncu + 31) / 32;
  std::vector<uint32_t> m_aux(words, 0u), m_main(words, 0u);
  for (unsigned i = 0; i < ncu; ++i) ((i % per) < aux / 8 ? m_aux : m_main)[i / 32] |= 1u << (i % 32);
  LSDR_TRY(lsdr_ctx_create_masked(caller->device, m_main.data(), words, &b->own_main));
  LSDR_TRY(lsdr_ctx_create_masked(caller->device, m_aux.data(), words, &b->ctx_aux));
  b->ctx = b->own_main;
  return LSDR_OK;
}

static int capture_batch_build(lsdr_capture_batch *b, const lsdr_capture_viterbi_cfg *vcfg) {
  LSDR_TRY(lsdr_rxb_describe_in(b->in_format, b->in_scale, &b->in));     // (refused before anything is allocated)
  LSDR_HIP(hipSetDevice(b->ctx->device));
  lsdr_ctx *const caller = b->ctx;
  int vrate = b->cfg.fec;
  if (vcfg) {
    // what viterbi_sync cannot decode is refused before anything is allocated, with lsdr_viterbi_batch_create's own code
    if (vrate == LSDR_FEC23) vrate = LSDR_FEC46;                        // "QPSK 2/3 is handled as 4/6", leandvb.cc:533-537
    LSDR_ARG(vcfg->resync_period >= 0);
    lsdr_viterbi_batch *probe = nullptr;
    LSDR_TRY(lsdr_viterbi_batch_create(caller, LSDR_QPSK, vrate, 1, 4096, &probe));
    lsdr_viterbi_batch_destroy(probe);
  }
  if (b->cfg.aux_cus) LSDR_TRY(capture_batch_partition(b, b->ctx));
  lsdr_ctx *c = b->ctx;
  lsdr_ctx *const ct = b->ctx_aux ? b->ctx_aux : c;                     // the context the tail (and the Viterbi stage) runs on
  const unsigned window = b->cfg.unlocked_window ? b->cfg.unlocked_window : 8192u;
  size_t stride = 0;
  if (vcfg) {
    LSDR_TRY(lsdr_rxb_create_in(c, &b->cfg, 1, 1.0f / 6.0f, b->in_format, b->in_scale, &b->rx));   // cstln_receiver::pll_adjustment behind viterbi_sync, leandvb.cc:498-501
    b->soft_cap = lsdr_rxb_soft_cap(b->rx);
    LSDR_TRY(lsdr_viterbi_batch_create(ct, LSDR_QPSK, vrate, b->cfg.n_captures, b->soft_cap, &b->vb));
    if (vcfg->resync_period > 0) LSDR_TRY(lsdr_viterbi_batch_set_resync_period(b->vb, vcfg->resync_period));
    // viterbi_sync writes less than two bits per QPSK symbol at any rate
    LSDR_TRY(lsdr_tail_create_ex(ct, (unsigned)b->cfg.n_captures, b->soft_cap, b->cfg.fec, window, 1, b->soft_cap / 4 + 64, "capture_batch", &b->tail));
    b->byte_cap = lsdr_tail_byte_cap(b->tail);
    const void *counts = lsdr_rxb_results_dev(b->rx, &stride);
    LSDR_TRY(lsdr_tail_bind(b->tail, nullptr, counts, stride));
    lsdr_capture_viterbi_stats z;
    memset(&z, 0, sizeof(z));
    b->vstats.assign(b->cfg.n_captures, z);
  } else {
    LSDR_TRY(lsdr_rxb_create_in(c, &b->cfg, 0, 1.0f, b->in_format, b->in_scale, &b->rx));
    const size_t sym_cap = lsdr_rxb_words_cap(b->rx) * 16;
    LSDR_TRY(lsdr_tail_create_ex(ct, (unsigned)b->cfg.n_captures, sym_cap, b->cfg.fec, window, 0, 0, "capture_batch", &b->tail));
    std::vector<const uint32_t *> words(b->cfg.n_captures);
    for (int i = 0; i < b->cfg.n_captures; ++i) words[i] = lsdr_rxb_words(b->rx, (unsigned)i);
    const void *counts = lsdr_rxb_results_dev(b->rx, &stride);
    LSDR_TRY(lsdr_tail_bind(b->tail, words.data(), counts, stride));
  }
  return LSDR_OK;
}

int lsdr_capture_any_create(lsdr_ctx *c, const lsdr_capture_batch_cfg *cfg, const lsdr_capture_viterbi_cfg *vcfg, const lsdr_capture_input_cfg *icfg,
                            lsdr_capture_batch **out) {
  LSDR_ARG(c && cfg && out);
  lsdr_capture_viterbi_cfg v;
  memset(&v, 0, sizeof(v));
  if (vcfg) v = *vcfg;
  int in_format = LSDR_IN_CU8; float in_scale = 0.f;
  if (icfg) {
    for (int i = 0; i < 6; ++i) LSDR_ARG(icfg->reserved[i] == 0);
    in_format = icfg->in_format; in_scale = icfg->in_scale;
  }
  lsdr_capture_batch *b = new lsdr_capture_batch();
  b->ctx = c; b->cfg = *cfg; b->in_format = in_format; b->in_scale = in_scale;
  const int rc = capture_batch_build(b, vcfg ? &v : nullptr);
  if (rc) { lsdr_capture_batch_destroy(b); return rc; }
  *out = b;
  return LSDR_OK;
}

int lsdr_capture_batch_create(lsdr_ctx *c, const lsdr_capture_batch_cfg *cfg, lsdr_capture_batch **out) {
  return lsdr_capture_any_create(c, cfg, nullptr, nullptr, out);
}

int lsdr_capture_batch_create_viterbi(lsdr_ctx *c, const lsdr_capture_batch_cfg *cfg, const lsdr_capture_viterbi_cfg *vcfg, lsdr_capture_batch **out) {
  lsdr_capture_viterbi_cfg v;
  memset(&v, 0, sizeof(v));
  return lsdr_capture_any_create(c, cfg, vcfg ? vcfg : &v, nullptr, out);
}

// one batch, capture i over its first n_samples[i] items with set_freq(tune[i]): what every run_async entry point comes to
static int capture_batch_run(lsdr_capture_batch *b, const void *const *iq_dev, const size_t *n_samples, const float *tune) {
  if (b->in_flight) { lsdr_set_error("capture_batch: a batch is in flight (lsdr_capture_batch_wait first)"); return LSDR_E_ARG; }
  if (b->vb) LSDR_TRY(lsdr_viterbi_batch_reset(b->vb, -1));              // every capture: a freshly constructed viterbi_sync
  std::vector<size_t> consumed(b->cfg.n_captures, 0);
  // (the front end checks every capture's arguments before it queues anything: a refused batch leaves the object usable)
  LSDR_TRY(lsdr_rxb_launch(b->rx, iq_dev, n_samples, tune, consumed.data(), b->ctx_aux ? b->ctx_aux->stream : nullptr));
  b->consumed = consumed;
  if (b->vb) {
    const std::vector<unsigned long long> zero(b->cfg.n_captures, 0ull);
    LSDR_TRY(capture_batch_viterbi_round(b, true, zero, zero, zero));
    lsdr_tail_stale(b->tail);                                           // (the tail is launched in wait)
  } else {
    LSDR_TRY(lsdr_tail_launch(b->tail));
  }
  b->in_flight = true;
  return LSDR_OK;
}

int lsdr_capture_any_run_async(lsdr_capture_batch *b, const void *const *iq_dev, size_t n_samples) {
  LSDR_ARG(b && iq_dev);
  for (int i = 0; i < b->cfg.n_captures; ++i) LSDR_ARG(iq_dev[i]);
  const std::vector<size_t> n(b->cfg.n_captures, n_samples);
  const std::vector<float> tune(b->cfg.n_captures, 0.f);
  return capture_batch_run(b, iq_dev, n.data(), tune.data());
}

int lsdr_capture_each_run_async(lsdr_capture_batch *b, const void *const *iq_dev, const lsdr_capture_each *each) {
  LSDR_ARG(b && iq_dev && each);
  const int B = b->cfg.n_captures;
  LSDR_TRY(lsdr_in_check_each("capture_batch", "tune", (unsigned)B, iq_dev, each, nullptr, nullptr, b->cfg.max_samples, b->in.item_bytes));
  std::vector<size_t> n(B);
  std::vector<float> tune(B);
  for (int i = 0; i < B; ++i) { n[i] = each[i].n_samples; tune[i] = each[i].tune; }
  return capture_batch_run(b, iq_dev, n.data(), tune.data());
}

int lsdr_capture_batch_run_async(lsdr_capture_batch *b, const lsdr_cu8 *const *iq_dev, size_t n_samples) {
  LSDR_ARG(b && iq_dev);
  if (b->in_format != LSDR_IN_CU8) {                                     // (a cu8 pointer is never read as wider items)
    lsdr_set_error("capture_batch: this object reads in_format %d: lsdr_capture_any_run_async", b->in_format); return LSDR_E_ARG;
  }
  return lsdr_capture_any_run_async(b, reinterpret_cast<const void *const *>(iq_dev), n_samples);
}

int lsdr_capture_batch_wait(lsdr_capture_batch *b, lsdr_capture_result *results) {
  LSDR_ARG(b);
  if (!b->in_flight) { lsdr_set_error("capture_batch: no batch in flight"); return LSDR_E_ARG; }
  if (b->vb) {
    // the remaining rounds of the Viterbi stage, then the tail
    const int n = b->cfg.n_captures;
    std::vector<lsdr_viterbi_batch_result> vr(n);
    std::vector<unsigned long long> total(n, 0ull), done(n, 0ull), bytes(n, 0ull);
    std::vector<unsigned> align(n, 0u);
    lsdr_capture_viterbi_stats z;
    memset(&z, 0, sizeof(z));
    b->vstats.assign(n, z);
    b->in_flight = false;                                               // (an error below leaves the object idle)
    for (unsigned round = 1;; ++round) {
      LSDR_TRY(lsdr_viterbi_batch_wait(b->vb, vr.data()));               // synchronises the stream: the front end's totals are on the host now
      bool moved = false;
      for (int i = 0; i < n; ++i) {
        if (round == 1) LSDR_TRY(lsdr_rxb_seam_stats(b->rx, (unsigned)i, &total[i], nullptr, nullptr, nullptr));
        lsdr_capture_viterbi_stats &s = b->vstats[i];
        done[i] += vr[i].consumed; bytes[i] += vr[i].produced; align[i] = vr[i].current_sync;
        if (vr[i].consumed) { moved = true; ++s.rounds; s.tiles += vr[i].tiles; s.repaired += vr[i].repaired; }
        s.switches += vr[i].switched; s.stalls += vr[i].stalled;
        s.batch_rounds = round; s.symbols = done[i]; s.bytes = bytes[i]; s.current_sync = align[i];
      }
      if (!moved) break;
      LSDR_TRY(capture_batch_viterbi_round(b, false, total, done, bytes));
    }
    LSDR_TRY(lsdr_tail_set_bytes(b->tail, bytes.data(), align.data()));
    LSDR_TRY(lsdr_tail_launch(b->tail));
  }
  LSDR_TRY(lsdr_tail_wait(b->tail, results));
  b->in_flight = false;
  for (int i = 0; results && i < b->cfg.n_captures; ++i) {
    lsdr_capture_result &r = results[i];
    r.samples = b->consumed[i];
    r.tiles = lsdr_rxb_tiles(b->rx, (unsigned)i);
    unsigned long long tot = 0; unsigned d = 0, m = 0, bad = 0;
    LSDR_TRY(lsdr_rxb_seam_stats(b->rx, (unsigned)i, &tot, &d, &m, &bad));
    r.seam_dup = d; r.seam_miss = m; r.seam_bad = bad;
  }
  return LSDR_OK;
}

int lsdr_capture_batch_ts_download_async(lsdr_capture_batch *b, uint8_t *const *ts_host, size_t cap_bytes) {
  LSDR_ARG(b);
  return lsdr_tail_ts_download_async(b->tail, ts_host, cap_bytes);
}

int lsdr_capture_batch_ts_wait(lsdr_capture_batch *b) {
  LSDR_ARG(b);
  return lsdr_tail_ts_wait(b->tail);
}

static bool capture_index_ok(const lsdr_capture_batch *b, int i) { return b && i >= 0 && i < b->cfg.n_captures; }
const uint8_t *lsdr_capture_batch_ts_dev(const lsdr_capture_batch *b, int i) { return capture_index_ok(b, i) ? lsdr_tail_ts_dev(b->tail, (unsigned)i) : nullptr; }
const uint32_t *lsdr_capture_batch_words_dev(const lsdr_capture_batch *b, int i) { return capture_index_ok(b, i) ? lsdr_rxb_words(b->rx, (unsigned)i) : nullptr; }
const uint8_t *lsdr_capture_batch_bytes_dev(const lsdr_capture_batch *b, int i) { return capture_index_ok(b, i) ? lsdr_tail_bytes_dev(b->tail, (unsigned)i) : nullptr; }
const uint8_t *lsdr_capture_batch_mpeg_dev(const lsdr_capture_batch *b, int i) { return capture_index_ok(b, i) ? lsdr_tail_mpeg_dev(b->tail, (unsigned)i) : nullptr; }
const lsdr_softsymbol *lsdr_capture_batch_soft_dev(const lsdr_capture_batch *b, int i) { return capture_index_ok(b, i) ? lsdr_rxb_soft(b->rx, (unsigned)i) : nullptr; }

int lsdr_capture_batch_viterbi_stats(const lsdr_capture_batch *b, int i, lsdr_capture_viterbi_stats *out) {
  LSDR_ARG(b && out && i >= 0 && i < b->cfg.n_captures);
  if (!b->vb) { lsdr_set_error("capture_batch: not a Viterbi object (lsdr_capture_batch_create_viterbi)"); return LSDR_E_ARG; }
  *out = b->vstats[i];
  return LSDR_OK;
}

// Re-acquisition after a lost lock (include/lsdr_hip.h; tail_relock.h, tail_device.h: k_tail_relock): the tail's own switch
int lsdr_capture_relock_set(lsdr_capture_batch *b, unsigned relocks) {
  LSDR_ARG(b);
  if (b->vb) { lsdr_set_error("capture_batch: re-acquisition belongs to the default engine (a Viterbi object searches the alignment in front of the tail)"); return LSDR_E_UNSUPPORTED; }
  if (b->in_flight) { lsdr_set_error("capture_batch: a batch is in flight (lsdr_capture_batch_wait first)"); return LSDR_E_ARG; }
  return lsdr_tail_relock_set(b->tail, relocks);
}
int lsdr_capture_relock_get(const lsdr_capture_batch *b, int i, lsdr_capture_relock_stats *s) {
  LSDR_ARG(b && s);
  if (b->vb) { lsdr_set_error("capture_batch: re-acquisition belongs to the default engine (a Viterbi object searches the alignment in front of the tail)"); return LSDR_E_UNSUPPORTED; }
  if (i < 0 || i >= b->cfg.n_captures) { lsdr_set_error("capture_batch: capture %d of %d", i, b->cfg.n_captures); return LSDR_E_ARG; }
  return lsdr_tail_relock_stats(b->tail, (unsigned)i, s);
}

int lsdr_capture_batch_bins(lsdr_capture_batch *b, int i, int *bins, unsigned cap, unsigned *n) {
  LSDR_ARG(b && i >= 0 && i < b->cfg.n_captures);
  return lsdr_rxb_bins(b->rx, (unsigned)i, bins, cap, n);
}
int lsdr_capture_batch_notched(lsdr_capture_batch *b, int i, lsdr_cf32 *out_dev, size_t n) {
  LSDR_ARG(b && i >= 0 && i < b->cfg.n_captures);
  if (b->in_flight) { lsdr_set_error("capture_batch: a batch is in flight (lsdr_capture_batch_wait first)"); return LSDR_E_ARG; }
  return lsdr_rxb_notched(b->rx, (unsigned)i, out_dev, n);
}
// Signal reports: what leandvb's --fd-info prints per capture (cstln_receiver's FREQ / SS / MER pipes, sdr.h:857-913, leandvb.cc:428-430,
// 465, 502, 600-605).  The estimators come from the front end's launches (rxb_device.h: REP tiles, k_rxb_reports); the libm scalars of
// sdr.h:907-911 are taken here, as rx_run_tiled takes them.
static lsdr_capture_report capture_report(const lsdr_rxb_report &m) {
  lsdr_capture_report r;
  r.freq = m.freqw / 65536;
  r.ss = sqrtf(m.est_insp);
  r.mer = m.est_ep ? 10 * logf(m.est_sp / m.est_ep) / logf(10) : 0;
  r.pad = 0;
  return r;
}
int lsdr_capture_reports_set(lsdr_capture_batch *b, uint64_t period_samples) {
  LSDR_ARG(b);
  if (b->in_flight) { lsdr_set_error("capture_batch: a batch is in flight (lsdr_capture_batch_wait first)"); return LSDR_E_ARG; }
  if (b->ctx_aux) LSDR_HIP(hipStreamSynchronize(b->ctx_aux->stream));
  return lsdr_rxb_set_reports(b->rx, period_samples);
}
int lsdr_capture_reports_get(lsdr_capture_batch *b, int i, lsdr_capture_report *out, size_t cap, size_t *n, lsdr_capture_report *last) {
  LSDR_ARG(b && n && i >= 0 && i < b->cfg.n_captures && (out || !cap));
  if (b->in_flight) { lsdr_set_error("capture_batch: a batch is in flight (lsdr_capture_batch_wait first)"); return LSDR_E_ARG; }
  if (!lsdr_rxb_reports_on(b->rx)) { lsdr_set_error("capture_batch: reports are off (lsdr_capture_reports_set)"); return LSDR_E_ARG; }
  const lsdr_rxb_report *slots = nullptr;
  lsdr_rxb_report fin;
  size_t have = 0;
  LSDR_TRY(lsdr_rxb_reports(b->rx, (unsigned)i, &slots, &have, &fin));
  if (!lsdr_tail_waited(b->tail)) have = 0;                                // (no batch yet)
  for (size_t q = 0; q < have && q < cap; ++q) out[q] = capture_report(slots[q]);
  *n = have;
  if (last) *last = capture_report(fin);
  return LSDR_OK;
}
int lsdr_capture_batch_tile_time(lsdr_capture_batch *b, int enable, float *avg_ms, unsigned *launches) {
  LSDR_ARG(b);
  return lsdr_rxb_tile_time(b->rx, enable, avg_ms, launches);
}

}  // extern "C"
