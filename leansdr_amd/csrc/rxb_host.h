// leansdr_amd/csrc/rxb_host.h — host side of the capture-batch receiver (rxb_device.h); included at the end of cstln_receiver.hip.
// Internal API (lsdr_internal.h) of lsdr_capture_batch (capture_batch.hip): create / launch / accessors / destroy.
#ifndef LSDR_RXB_HOST_H
#define LSDR_RXB_HOST_H

// geometry of one capture's run over its n_samples
struct rxb_geom { unsigned long long chunks; unsigned n_tiles, n_det, n_pre, n_blocks; };

struct lsdr_rxb {
  lsdr_ctx *ctx;
  lsdr_rx *proto;                  // tables, loop constants, the constructed loop state, the relabel maps
  unsigned n;
  size_t max_samples;
  int anf;
  unsigned Lc, Wc, pre_block, pre_look;
  float nk;
  int notch_decimation;
  // capacities (for max_samples)
  unsigned max_tiles, max_det, max_pre, max_blocks, hwords;
  unsigned long long hpitch;
  size_t words_cap;                // 32-bit words of packed decisions per capture
  std::vector<rxb_cap> caps;       // host copy (buffer pointers are fixed at create; in / geometry per launch)
  rxb_cap *h_caps, *d_caps;        // pinned staging, device array
  rx_seam_result *d_res, *h_res; rx_state_dev *d_state_end; rx_ema_map *d_ema;   // h_res: pinned copy of d_res, filled behind every launch
  rx_state_dev *d_state0, *h_state0;                                             // [n] every capture's constructed state (its tune), pinned staging
  std::vector<float> tune_dev; bool tune_valid;                                  // the tunes d_state0 holds
  unsigned *d_iv_of_block, *d_det_block; float2 *d_om;
  std::vector<void *> owned;       // every per-capture device allocation
  size_t geom_samples;             // n_samples the detect-point tables on the device were built for: the longest capture's (a prefix for the others)
  std::vector<rxb_geom> geo;      // the last launch, per capture
  std::vector<size_t> cap_samples;
  bool any_det;                    // … ran the detect chain
  hipEvent_t tev0, tev1; bool timing; double time_ms; unsigned time_n; bool tev_pending;
  bool soft;                       // soft symbols out (the Viterbi engine): sstage / spre / out_soft instead of hstage / out_words
  unsigned srows;                  // rows (symbol steps) of a capture's transposed soft staging
  size_t soft_cap;                 // soft symbols per capture in out_soft
  unsigned long long *d_counts;    // [n] contiguous: soft symbols of every capture after the launch
  hipEvent_t ev_pre, ev_tiles;      // hand-overs between the tile stream and the auxiliary stream (lsdr_rxb_launch with aux)
  lsdr_in_desc in;                 // the captures' items (lsdr_capture_input_cfg): the kernels' kind (rxb_device.h: kRxbU8 …) and what goes with it
  // signal reports (lsdr_rxb_set_reports; off: rep_on false, nothing allocated, the kernels and launches of an object without them)
  bool rep_on;
  unsigned long long rep_period;   // as given
  unsigned rep_period_k;           // what the kernels count with (0: the period is longer than any capture of this object)
  size_t rep_pitch;                // slots per capture, the final record included
  rxb_rep *d_rep; rx_meas *d_slots, *h_slots;   // [n] records, [n·rep_pitch] slots, their pinned copy (filled behind every launch)
  std::vector<void *> rep_owned;   // the captures' map arrays
};

static int rxb_alloc(lsdr_rxb *b, void **p, size_t bytes) {
  LSDR_HIP(hipMalloc(p, bytes ? bytes : 16));
  b->owned.push_back(*p);
  return LSDR_OK;
}

static rxb_geom rxb_geometry(const lsdr_rxb *b, size_t n_samples) {
  rxb_geom g;
  const size_t usable = b->anf ? n_samples / kDetN * kDetN : n_samples;      // auto_notch::run moves whole 4096-sample blocks (sdr.h:64-75)
  g.chunks = usable >= (size_t)(kChunk + 1) ? (usable - 1) / kChunk : 0;     // cstln_receiver::run: chunk_size + readahead readable (sdr.h:783)
  g.n_tiles = g.chunks ? 1u : 0u;
  if (g.chunks > b->Wc) g.n_tiles += (unsigned)((g.chunks - b->Wc + b->Lc - 1) / b->Lc);
  g.n_blocks = (unsigned)(usable / kDetN);
  g.n_det = 0;
  if (b->anf) {                                                              // `phase += fft.n; if (phase >= decimation) { phase -= decimation; detect(); }`
    // decimation ≥ fft.n (lsdr_rxb_create_in): phase stays in [0, decimation), so after n blocks it is n·4096 − detects·decimation —
    // counted per capture and launch, hence not by walking the blocks
    if (b->notch_decimation >= kDetN) g.n_det = (unsigned)((unsigned long long)g.n_blocks * kDetN / (unsigned long long)b->notch_decimation);
    else {
      long long phase = 0;
      for (unsigned blk = 0; blk < g.n_blocks; ++blk) { phase += kDetN; if (phase >= b->notch_decimation) { phase -= b->notch_decimation; ++g.n_det; } }
    }
  }
  g.n_pre = b->anf ? (unsigned)(usable / b->pre_block) : 0u;
  return g;
}

// rxb_device.h's kinds are capture_input.h's, so lsdr_in_desc::kind selects the kernels as it stands
static_assert(kRxbU8 == kCapU8 && kRxbS8 == kCapS8 && kRxb16 == kCap16 && kRxbF32 == kCapF32, "one numbering of the kinds");

// An object's in_format / in_scale (lsdr_capture_input_cfg) with the front end's own rule: cu8 without a scale has its own kernels, and
// those have no scaler.
int lsdr_rxb_describe_in(int in_format, float in_scale, lsdr_in_desc *out) {
  LSDR_TRY(lsdr_in_describe("capture_batch", in_format, in_scale, out));
  if (out->kind == kRxbU8 && out->in_scale != 1.0f) {
    lsdr_set_error("capture_batch: cu8 captures take no in_scale (got %g): the cu8 kernels have no scaler", (double)in_scale); return LSDR_E_UNSUPPORTED;
  }
  return LSDR_OK;
}

// soft != 0: lsdr_softsymbol records out (rxb_device.h's soft tiles); pll_adjustment: cstln_receiver::pll_adjustment (sdr.h:777: divides
// freq_beta only), 1 in leandvb's default graph, 6 behind viterbi_sync (leandvb.cc:498-501) — given here as the factor 1/6
// in_format / in_scale: lsdr_capture_input_cfg (checked here).  cu8 without a scale has its own kernels.
int lsdr_rxb_create_in(lsdr_ctx *c, const lsdr_capture_batch_cfg *cfg, int soft, float pll_adjustment, int in_format, float in_scale, lsdr_rxb **out) {
  LSDR_ARG(c && cfg && out && cfg->n_captures >= 1 && cfg->n_captures <= 4096 && cfg->max_samples >= 4096);
  LSDR_ARG(cfg->anf == 0 || cfg->anf == 1);
  lsdr_in_desc in;
  LSDR_TRY(lsdr_rxb_describe_in(in_format, in_scale, &in));
  lsdr_rx_cfg rc;
  memset(&rc, 0, sizeof(rc));
  rc.sampler = LSDR_SAMP_LINEAR; rc.cstln = LSDR_QPSK; rc.fec = cfg->fec; rc.omega = cfg->omega; rc.freq = 0.f;
  rc.meas_decimation = 1048576; rc.pll_adjustment = pll_adjustment; rc.allow_drift = 0; rc.kest = 0.01f; rc.mode = LSDR_RX_TILED;
  rc.in_format = LSDR_IN_CU8; rc.out_format = LSDR_SYM_HARD2;
  if (!(cfg->omega >= 1.0f && cfg->omega <= 8.0f)) { lsdr_set_error("capture_batch: omega (samples per symbol) must be in [1, 8], got %g", (double)cfg->omega); return LSDR_E_UNSUPPORTED; }
  const unsigned L = cfg->tile_len ? cfg->tile_len : 4096u, W = cfg->tile_warmup ? cfg->tile_warmup : 512u;
  if (L % 2048u || W % kChunk || W < (unsigned)kChunk || (float)L / (cfg->omega + 0.1f) < 34.f) {
    lsdr_set_error("capture_batch: tile_len must be a multiple of 2048 samples and tile_warmup a multiple of 128 (got %u / %u)", L, W);
    return LSDR_E_ARG;
  }
  rc.tile_len = L; rc.tile_warmup = W;
  if (in.kind != kRxbU8) {
    // the tiles address a capture with 32-bit byte offsets (rxb_tile: src_off below 0xfff00000, plus the offset inside the tile)
    if ((unsigned long long)cfg->max_samples * in.item_bytes >= 0xfff00000ull || ((unsigned long long)L + W) * in.item_bytes >= 0x100000ull) {
      lsdr_set_error("capture_batch: %zu samples of %u bytes (tile_len %u) are beyond the tiles' 32-bit buffer offsets", cfg->max_samples, in.item_bytes, L);
      return LSDR_E_UNSUPPORTED;
    }
  }
  lsdr_rx *proto = nullptr;
  LSDR_TRY(lsdr_rx_create(c, &rc, &proto));
  lsdr_rxb *b = new lsdr_rxb();
  b->ctx = c; b->proto = proto; b->n = (unsigned)cfg->n_captures; b->max_samples = cfg->max_samples; b->anf = cfg->anf;
  b->Lc = L / kChunk; b->Wc = W / kChunk;
  b->soft = soft != 0;
  b->in = in;
  b->pre_block = (L % 4096u) ? 2048u : 4096u;
  b->nk = cfg->notch_k > 0.f ? cfg->notch_k : 0.002f;                          // sdr.h:56
  b->notch_decimation = cfg->notch_decimation > 0 ? cfg->notch_decimation : 1024 * kDetN;
  {
    const double omk = (double)(1.0f - b->nk);
    unsigned q = 1;
    while (pow(omk, (double)q * b->pre_block) > 1e-7 && q < 64) ++q;
    b->pre_look = q;
  }
  *out = b;                                                                    // (from here on the caller destroys on error)
  LSDR_HIP(hipSetDevice(c->device));
  if (b->anf && (long long)b->Wc * kChunk > (long long)b->notch_decimation - kDetN) {
    lsdr_set_error("capture_batch: the first detect point must lie behind the first tile"); return LSDR_E_UNSUPPORTED;
  }
  const rxb_geom g = rxb_geometry(b, b->max_samples);
  b->max_tiles = g.n_tiles ? g.n_tiles : 1; b->max_det = g.n_det; b->max_pre = g.n_pre; b->max_blocks = g.n_blocks ? g.n_blocks : 1;
  const unsigned sym_per_chunk = (unsigned)(kChunk / (cfg->omega - 0.1f)) + 2;
  const unsigned stage_stride = (b->Wc > b->Lc ? b->Wc : b->Lc) * sym_per_chunk;
  b->hwords = stage_stride / 16 + 2;
  b->hpitch = ((unsigned long long)b->max_tiles + 63) & ~63ull;
  b->words_cap = (size_t)((unsigned long long)g.chunks * sym_per_chunk / 16 + b->max_tiles + 64);
  // soft staging: a symbol step moves at least one sample on, so a tile body of Lc (tile 0: Wc) chunks holds at most that many samples' symbols
  b->srows = (b->Wc > b->Lc ? b->Wc : b->Lc) * (unsigned)kChunk + 1u;
  b->soft_cap = (size_t)((unsigned long long)g.chunks * sym_per_chunk + b->max_tiles + 64);
  if (b->soft && b->hpitch * b->srows * sizeof(unsigned) >= (1ull << 32)) {       // (the soft tiles address a capture's staging with 32 bits)
    lsdr_set_error("capture_batch: %zu samples per capture are too many for the soft staging at tile_len %u", b->max_samples, L); return LSDR_E_UNSUPPORTED;
  }
  b->caps.assign(b->n, rxb_cap());
  LSDR_HIP(hipMalloc((void **)&b->d_caps, b->n * sizeof(rxb_cap)));
  LSDR_HIP(hipHostMalloc((void **)&b->h_caps, b->n * sizeof(rxb_cap), hipHostMallocDefault));
  LSDR_HIP(hipMalloc((void **)&b->d_res, b->n * sizeof(rx_seam_result)));
  LSDR_HIP(hipMemset(b->d_res, 0, b->n * sizeof(rx_seam_result)));
  LSDR_HIP(hipHostMalloc((void **)&b->h_res, b->n * sizeof(rx_seam_result), hipHostMallocDefault));
  memset(b->h_res, 0, b->n * sizeof(rx_seam_result));
  LSDR_HIP(hipMalloc((void **)&b->d_state_end, b->n * sizeof(rx_state_dev)));
  LSDR_HIP(hipMalloc((void **)&b->d_state0, b->n * sizeof(rx_state_dev)));
  LSDR_HIP(hipHostMalloc((void **)&b->h_state0, b->n * sizeof(rx_state_dev), hipHostMallocDefault));
  for (unsigned i = 0; i < b->n; ++i) b->h_state0[i] = proto->st_initial;
  b->tune_dev.assign(b->n, 0.f); b->tune_valid = false;
  b->geo.assign(b->n, rxb_geom()); b->cap_samples.assign(b->n, 0); b->any_det = false;
  LSDR_HIP(hipMalloc((void **)&b->d_ema, 2 * b->n * sizeof(rx_ema_map)));
  LSDR_HIP(hipMalloc((void **)&b->d_counts, b->n * sizeof(unsigned long long)));
  LSDR_HIP(hipMemset(b->d_counts, 0, b->n * sizeof(unsigned long long)));
  LSDR_HIP(hipMalloc((void **)&b->d_iv_of_block, (size_t)b->max_blocks * sizeof(unsigned)));
  LSDR_HIP(hipMalloc((void **)&b->d_det_block, (size_t)(b->max_det + 1) * sizeof(unsigned)));
  {
    std::vector<float2> om;
    notch_detect_twiddles(kDetN, true, om);
    LSDR_HIP(hipMalloc((void **)&b->d_om, kDetN * sizeof(float2)));
    LSDR_HIP(hipMemcpy(b->d_om, om.data(), kDetN * sizeof(float2), hipMemcpyHostToDevice));
  }
  for (unsigned i = 0; i < b->n; ++i) {
    rxb_cap &cp = b->caps[i];
    memset(&cp, 0, sizeof(cp));
    LSDR_TRY(rxb_alloc(b, (void **)&cp.hstage, b->soft ? 0 : (size_t)b->hpitch * b->hwords * sizeof(unsigned)));
    LSDR_TRY(rxb_alloc(b, (void **)&cp.hinfo, (size_t)b->max_tiles * sizeof(rx_tile_info_h)));
    LSDR_TRY(rxb_alloc(b, (void **)&cp.fix, (size_t)b->max_tiles * sizeof(rx_tile_fix)));
    LSDR_TRY(rxb_alloc(b, (void **)&cp.part, (size_t)((b->max_tiles + kSeamBlock - 1) / kSeamBlock) * sizeof(rx_seam_part)));
    LSDR_TRY(rxb_alloc(b, (void **)&cp.out_words, b->soft ? 0 : b->words_cap * sizeof(unsigned)));
    if (b->soft) {
      LSDR_TRY(rxb_alloc(b, (void **)&cp.sstage, (size_t)b->hpitch * b->srows * sizeof(unsigned)));
      LSDR_TRY(rxb_alloc(b, (void **)&cp.spre, (size_t)b->max_tiles * sizeof(unsigned)));
      LSDR_TRY(rxb_alloc(b, (void **)&cp.out_soft, b->soft_cap * sizeof(unsigned)));
    }
    cp.count_out = b->d_counts + i;
    cp.res = b->d_res + i; cp.state_end = b->d_state_end + i; cp.ema_scratch = b->d_ema + 2 * i;
    cp.hpitch = b->hpitch; cp.state0 = b->d_state0 + i;
    if (b->anf) {
      LSDR_TRY(rxb_alloc(b, (void **)&cp.iv, (size_t)(b->max_det + 1) * sizeof(rxb_iv)));
      LSDR_TRY(rxb_alloc(b, (void **)&cp.T, (size_t)(b->max_pre + 1) * sizeof(float2)));
      LSDR_TRY(rxb_alloc(b, (void **)&cp.cand, (size_t)(b->max_det + 1) * kDetMaxSlots * sizeof(int)));
      LSDR_TRY(rxb_alloc(b, (void **)&cp.halves, (size_t)(b->max_det + 1) * kDetN * sizeof(float2)));
    }
  }
  b->geom_samples = 0;
  LSDR_HIP(hipEventCreate(&b->tev0)); LSDR_HIP(hipEventCreate(&b->tev1));
  LSDR_HIP(hipEventCreateWithFlags(&b->ev_pre, hipEventDisableTiming)); LSDR_HIP(hipEventCreateWithFlags(&b->ev_tiles, hipEventDisableTiming));
  b->timing = false; b->time_ms = 0; b->time_n = 0; b->tev_pending = false;
  return LSDR_OK;
}

static void rxb_reports_free(lsdr_rxb *b) {
  for (void *p : b->rep_owned) (void)hipFree(p);
  b->rep_owned.clear();
  if (b->d_rep) (void)hipFree(b->d_rep);
  if (b->d_slots) (void)hipFree(b->d_slots);
  if (b->h_slots) (void)hipHostFree(b->h_slots);
  b->d_rep = nullptr; b->d_slots = nullptr; b->h_slots = nullptr;
  b->rep_on = false; b->rep_period = 0; b->rep_period_k = 0; b->rep_pitch = 0;
}

// period_samples = cstln_receiver::meas_decimation; 0: off.  The previous launch of this object must have completed.  Buffers for max_samples.
int lsdr_rxb_set_reports(lsdr_rxb *b, unsigned long long period_samples) {
  LSDR_ARG(b);
  if (period_samples && period_samples < (unsigned long long)kChunk) {
    lsdr_set_error("capture_batch: a report period below %d samples (got %llu) is several reports per chunk", kChunk, period_samples); return LSDR_E_ARG;
  }
  LSDR_HIP(hipSetDevice(b->ctx->device));
  LSDR_HIP(hipStreamSynchronize(b->ctx->stream));
  rxb_reports_free(b);
  if (!period_samples) return LSDR_OK;
  const size_t reports = (size_t)((unsigned long long)b->max_samples / period_samples);
  if (reports && period_samples >= (1ull << 31)) {                              // (the tiles count samples up to the next instant in 32 bits)
    lsdr_set_error("capture_batch: a report period of %llu samples is beyond the tiles' 32-bit counter", period_samples); return LSDR_E_UNSUPPORTED;
  }
  b->rep_period = period_samples; b->rep_period_k = reports ? (unsigned)period_samples : 0u;
  b->rep_pitch = reports + 1;
  std::vector<rxb_rep> recs(b->n);
  LSDR_HIP(hipMalloc((void **)&b->d_slots, b->n * b->rep_pitch * sizeof(rx_meas)));
  LSDR_HIP(hipMemset(b->d_slots, 0, b->n * b->rep_pitch * sizeof(rx_meas)));
  LSDR_HIP(hipHostMalloc((void **)&b->h_slots, b->n * b->rep_pitch * sizeof(rx_meas), hipHostMallocDefault));
  memset(b->h_slots, 0, b->n * b->rep_pitch * sizeof(rx_meas));
  for (unsigned i = 0; i < b->n; ++i) {
    void *p = nullptr;
    LSDR_HIP(hipMalloc(&p, (size_t)b->max_tiles * sizeof(rx_ema_map)));
    b->rep_owned.push_back(p);
    recs[i].map = static_cast<rx_ema_map *>(p); recs[i].slot = b->d_slots + (size_t)i * b->rep_pitch;
  }
  LSDR_HIP(hipMalloc((void **)&b->d_rep, b->n * sizeof(rxb_rep)));
  LSDR_HIP(hipMemcpy(b->d_rep, recs.data(), b->n * sizeof(rxb_rep), hipMemcpyHostToDevice));
  b->rep_on = true;
  return LSDR_OK;
}
int lsdr_rxb_reports_on(const lsdr_rxb *b) { return b && b->rep_on ? 1 : 0; }
// capture i's estimator records of the last launch (valid once the stream has passed it): *n of them at *slots, then the final record
int lsdr_rxb_reports(const lsdr_rxb *b, unsigned i, const lsdr_rxb_report **slots, size_t *n, lsdr_rxb_report *last) {
  LSDR_ARG(b && i < b->n && slots && n && last && b->rep_on);
  static_assert(sizeof(lsdr_rxb_report) == sizeof(rx_meas) && offsetof(lsdr_rxb_report, est_ep) == offsetof(rx_meas, est_ep), "lsdr_rxb_report mirrors rx_meas");
  const rx_meas *s = b->h_slots + (size_t)i * b->rep_pitch;
  const unsigned long long chunks = b->geo[i].chunks;                          // (none: the capture's constructed estimators are the final record)
  const size_t rep_n = chunks && b->rep_period ? (size_t)(chunks * kChunk / b->rep_period) : 0;
  *slots = reinterpret_cast<const lsdr_rxb_report *>(s); *n = rep_n;
  if (!chunks) {
    const rx_state_dev &st = b->h_state0[i];
    last->freqw = st.freqw; last->est_insp = st.est_insp; last->est_sp = st.est_sp; last->est_ep = st.est_ep; last->a = 0.f; last->tile = 0;
  } else
    memcpy(last, s + rep_n, sizeof(*last));
  return LSDR_OK;
}

void lsdr_rxb_destroy(lsdr_rxb *b) {
  if (!b) return;
  (void)hipStreamSynchronize(b->ctx->stream);
  rxb_reports_free(b);
  for (void *p : b->owned) (void)hipFree(p);
  (void)hipFree(b->d_caps); if (b->h_caps) (void)hipHostFree(b->h_caps);
  (void)hipFree(b->d_res); if (b->h_res) (void)hipHostFree(b->h_res); (void)hipFree(b->d_state_end); (void)hipFree(b->d_state0); if (b->h_state0) (void)hipHostFree(b->h_state0); (void)hipFree(b->d_ema); (void)hipFree(b->d_counts);
  (void)hipFree(b->d_iv_of_block); (void)hipFree(b->d_det_block); (void)hipFree(b->d_om);
  if (b->tev0) (void)hipEventDestroy(b->tev0);
  if (b->tev1) (void)hipEventDestroy(b->tev1);
  if (b->ev_pre) (void)hipEventDestroy(b->ev_pre);
  if (b->ev_tiles) (void)hipEventDestroy(b->ev_tiles);
  lsdr_rx_destroy(b->proto);
  delete b;
}

static void rxb_fill_args(const lsdr_rxb *b, rxb_args &A) {
  A.caps = b->d_caps; A.iv_of_block = b->d_iv_of_block; A.det_block = b->d_det_block; A.om = b->d_om;
  A.tile_chunks = b->Lc; A.warm_chunks = b->Wc; A.pre_block = b->pre_block; A.pre_look = b->pre_look;
  A.nk = b->nk; A.l2omk = (float)log2((double)(1.0f - b->nk));
  rx_fill_consts(b->proto, A.C, A.T);
  A.in_scale = b->in.in_scale; A.in_flip = b->in.in_flip;
  A.rep = b->d_rep; A.rep_period = b->rep_period_k;
}

// the kernels of the object's kind (cu8: its own instantiations, the ones it had before there were other formats)
typedef void (*rxb_kernel_t)(rxb_args);
typedef void (*rxb_dump_kernel_t)(rxb_args, unsigned, unsigned long long, float2 *);
template <int K> static rxb_kernel_t rxb_tiles_of(bool notch, bool soft) {
  if (soft) {
    if constexpr (K == kRxbF32) return notch ? k_rxb_tiles_in<true, true, K> : k_rxb_tiles_in<false, true, K>;
    else return notch ? k_rxb_tiles_in_soft5<true, K> : k_rxb_tiles_in_soft5<false, K>;
  }
  return notch ? k_rxb_tiles_in<true, false, K> : k_rxb_tiles_in<false, false, K>;
}
// … with signal reports
template <int K> static rxb_kernel_t rxb_tiles_rep_of(bool notch, bool soft) {
  if (soft) return notch ? k_rxb_tiles_rep<true, true, K> : k_rxb_tiles_rep<false, true, K>;
  return notch ? k_rxb_tiles_rep<true, false, K> : k_rxb_tiles_rep<false, false, K>;
}
static rxb_kernel_t rxb_kernel_tiles_rep(int kind, bool notch, bool soft) {
  return in_dispatch(kind, [&](auto K) { return rxb_tiles_rep_of<K()>(notch, soft); });
}
static rxb_kernel_t rxb_kernel_tiles(int kind, bool notch, bool soft) {
  return in_dispatch(kind, [&](auto K) -> rxb_kernel_t {
    if constexpr (K() != kRxbU8) return rxb_tiles_of<K()>(notch, soft);
    else if (soft) return notch ? k_rxb_tiles_soft<true> : k_rxb_tiles_soft<false>;
    else return notch ? k_rxb_tiles<true> : k_rxb_tiles<false>;
  });
}
static rxb_kernel_t rxb_kernel_detect(int kind) { return in_dispatch(kind, [](auto K) -> rxb_kernel_t { return k_rxb_detect_fft<K()>; }); }
static rxb_kernel_t rxb_kernel_pre(int kind) { return in_dispatch(kind, [](auto K) -> rxb_kernel_t { return k_rxb_notch_pre<K()>; }); }
static rxb_dump_kernel_t rxb_kernel_dump(int kind) { return in_dispatch(kind, [](auto K) -> rxb_dump_kernel_t { return k_rxb_notch_dump<K()>; }); }

// capture i's constructed loop state under set_freq(tune): what lsdr_rx_create leaves for cfg.freq = tune (sdr.h:745-770; leandvb calls
// set_freq only for a nonzero --tune, leandvb.cc:483-487)
static rx_state_dev rxb_state_of(lsdr_rx *r, float tune) {
  if (!tune) return r->st_initial;
  const rx_state_dev keep = r->st;
  r->st = r->st_initial;
  rx_set_freq(r, tune, true);
  const rx_state_dev s = r->st;
  r->st = keep;
  return s;
}

// Queues the whole front end of a batch: detect chain, estimator pre-pass, tiles, seam pass, compaction.  aux == nullptr: everything on
// the context's stream.  aux: the TILES on the context's stream, everything else on `aux` (the caller's stream for the memory-bound
// kernels — on its own compute units, lsdr_capture_batch_cfg::aux_cus), handed over by events; what follows the compaction (the FEC tail)
// belongs on `aux` then.  The previous launch of this object must have completed (the argument records are single-buffered).
// n_samples[i], tune[i]: capture i's length and set_freq (lsdr_capture_each); consumed[i]: the samples its receiver runs over.  Every
// capture has its own geometry in its rxb_cap; the grids are sized for the longest one and a kernel leaves by the capture's own counts.
int lsdr_rxb_launch(lsdr_rxb *b, const void *const *iq, const size_t *n_samples, const float *tune, size_t *consumed, hipStream_t aux) {
  LSDR_ARG(b && iq && n_samples && tune && consumed);
  lsdr_ctx *c = b->ctx;
  lsdr_rx *r = b->proto;
  // everything is checked before anything of the previous launch is overwritten
  size_t longest = 0;
  rxb_geom gmax; memset(&gmax, 0, sizeof(gmax));
  std::vector<rxb_geom> geo(b->n);
  LSDR_TRY(lsdr_in_check_each("capture_batch", "tune", b->n, iq, nullptr, n_samples, tune, b->max_samples, b->in.item_bytes));
  for (unsigned i = 0; i < b->n; ++i) {
    const rxb_geom g = rxb_geometry(b, n_samples[i]);
    geo[i] = g;
    if (n_samples[i] > longest) longest = n_samples[i];
    if (g.chunks > gmax.chunks) gmax.chunks = g.chunks;
    if (g.n_tiles > gmax.n_tiles) gmax.n_tiles = g.n_tiles;
    if (g.n_det > gmax.n_det) gmax.n_det = g.n_det;
    if (g.n_pre > gmax.n_pre) gmax.n_pre = g.n_pre;
    if (g.n_blocks > gmax.n_blocks) gmax.n_blocks = g.n_blocks;
  }
  const bool notch = b->anf && gmax.n_det > 0;                               // the NOTCH tiles run when any capture has a detect point
  if (notch)
    for (unsigned i = 0; i < b->n; ++i)
      if (((unsigned long long)iq[i] & 15ull) != 0) { lsdr_set_error("capture_batch: with the notch the captures must be 16-byte aligned"); return LSDR_E_ARG; }
  LSDR_HIP(hipSetDevice(c->device));
  if (b->tev_pending) LSDR_TRY(lsdr_rxb_tile_time(b, -1, nullptr, nullptr));   // (the previous launch has completed: collect its events)
  if (b->anf && b->geom_samples != longest) {                                 // detect points up to the longest capture's length
    std::vector<unsigned> ivb(gmax.n_blocks ? gmax.n_blocks : 1, 0u), det(gmax.n_det + 1, 0u);
    long long phase = 0;
    unsigned m = 0;
    for (unsigned blk = 0; blk < gmax.n_blocks; ++blk) {
      phase += kDetN;
      if (phase >= b->notch_decimation) { phase -= b->notch_decimation; det[m++] = blk; }
      ivb[blk] = m;
    }
    LSDR_HIP(hipStreamSynchronize(c->stream));
    if (aux) LSDR_HIP(hipStreamSynchronize(aux));
    LSDR_HIP(hipMemcpy(b->d_iv_of_block, ivb.data(), ivb.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    LSDR_HIP(hipMemcpy(b->d_det_block, det.data(), det.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    b->geom_samples = longest;
  }
  bool retune = !b->tune_valid, idle = false;
  for (unsigned i = 0; i < b->n; ++i) {
    const rxb_geom &g = geo[i];
    consumed[i] = (size_t)g.chunks * kChunk;
    b->cap_samples[i] = n_samples[i];
    rxb_cap &cp = b->caps[i];
    cp.in = static_cast<const unsigned char *>(iq[i]);
    cp.total_chunks = g.chunks; cp.n_tiles = g.n_tiles; cp.n_det = g.n_det;
    b->h_caps[i] = cp;
    if (!g.chunks) idle = true;
    if (b->tune_dev[i] != tune[i]) { retune = true; b->tune_dev[i] = tune[i]; b->h_state0[i] = rxb_state_of(r, tune[i]); }
  }
  b->geo = geo; b->any_det = notch;
  const hipStream_t sa = aux ? aux : c->stream, st = c->stream;      // auxiliary kernels / tiles
  LSDR_HIP(hipMemcpyAsync(b->d_caps, b->h_caps, b->n * sizeof(rxb_cap), hipMemcpyHostToDevice, sa));
  if (retune) {                                                      // (a batch tuned like the one before it uploads nothing)
    LSDR_HIP(hipMemcpyAsync(b->d_state0, b->h_state0, b->n * sizeof(rx_state_dev), hipMemcpyHostToDevice, sa));
    b->tune_valid = true;
  }
  if (idle) {                                                        // a capture without a chunk is left by every kernel: its records are cleared here
    LSDR_HIP(hipMemsetAsync(b->d_res, 0, b->n * sizeof(rx_seam_result), sa));
    LSDR_HIP(hipMemsetAsync(b->d_counts, 0, b->n * sizeof(unsigned long long), sa));
  }
  if (!gmax.chunks) {                                                // no capture has a chunk
    LSDR_HIP(hipMemcpyAsync(b->h_res, b->d_res, b->n * sizeof(rx_seam_result), hipMemcpyDeviceToHost, sa));
    return LSDR_OK;
  }
  rxb_args A;
  rxb_fill_args(b, A);
  if (notch) {
    hipLaunchKernelGGL(rxb_kernel_detect(b->in.kind), dim3(2 * gmax.n_det, b->n), dim3(256), 0, sa, A);
    hipLaunchKernelGGL(k_rxb_detect_peaks, dim3(gmax.n_det, b->n), dim3(256), 0, sa, A);
    hipLaunchKernelGGL(k_rxb_iv, dim3((b->n + 63) / 64), dim3(64), 0, sa, A, b->n);
    hipLaunchKernelGGL(rxb_kernel_pre(b->in.kind), dim3(gmax.n_pre, b->n), dim3(256), 0, sa, A);
    LSDR_HIP(hipGetLastError());
  }
  const unsigned blocks = 1 + (gmax.n_tiles - 1 + 63) / 64;
  if (aux) { LSDR_HIP(hipEventRecord(b->ev_pre, sa)); LSDR_HIP(hipStreamWaitEvent(st, b->ev_pre, 0)); }
  if (b->timing) { LSDR_HIP(hipEventRecord(b->tev0, st)); }
  hipLaunchKernelGGL(b->rep_on ? rxb_kernel_tiles_rep(b->in.kind, notch, b->soft) : rxb_kernel_tiles(b->in.kind, notch, b->soft), dim3(blocks, b->n), dim3(64), 0, st, A);
  if (b->timing) { LSDR_HIP(hipEventRecord(b->tev1, st)); b->tev_pending = true; }
  if (aux) { LSDR_HIP(hipEventRecord(b->ev_tiles, st)); LSDR_HIP(hipStreamWaitEvent(sa, b->ev_tiles, 0)); }
  const int R = r->tabs.nrotations;
  const float quad = 65536.0f / R;
  hipLaunchKernelGGL(k_rxb_seam, dim3((gmax.n_tiles + kSeamBlock - 1) / kSeamBlock, b->n), dim3(kSeamBlock), 0, sa, A, r->omega, R, quad,
                     (const uint8_t *)r->d_relabel);
  if (b->soft) {
    const unsigned row_blocks = (b->srows + kRxbSoftTile - 1) / kRxbSoftTile;
    hipLaunchKernelGGL(k_rxb_compact_soft, dim3(((gmax.n_tiles + kRxbSoftTile - 1) / kRxbSoftTile) * row_blocks, b->n), dim3(256), 0, sa, A, row_blocks, R, quad,
                       (const uint8_t *)r->d_relabel);
  } else
    hipLaunchKernelGGL(k_rxb_compact, dim3((gmax.n_tiles * kRxbCompactLanes + 63) / 64, b->n), dim3(64), 0, sa, A, R, quad, (const uint8_t *)r->d_relabel);
  if (b->rep_on) hipLaunchKernelGGL(k_rxb_reports, dim3(b->n), dim3(kRxbRepThreads), 0, sa, A);
  LSDR_HIP(hipGetLastError());
  LSDR_HIP(hipMemcpyAsync(b->h_res, b->d_res, b->n * sizeof(rx_seam_result), hipMemcpyDeviceToHost, sa));
  if (b->rep_on) LSDR_HIP(hipMemcpyAsync(b->h_slots, b->d_slots, b->n * b->rep_pitch * sizeof(rx_meas), hipMemcpyDeviceToHost, sa));
  return LSDR_OK;
}

const uint32_t *lsdr_rxb_words(const lsdr_rxb *b, unsigned i) { return b && !b->soft && i < b->n ? b->caps[i].out_words : nullptr; }
size_t lsdr_rxb_words_cap(const lsdr_rxb *b) { return b ? b->words_cap : 0; }
// the soft engine: capture i's compacted soft symbols, their capacity, and the contiguous device array [n] of their counts
const lsdr_softsymbol *lsdr_rxb_soft(const lsdr_rxb *b, unsigned i) { return b && b->soft && i < b->n ? reinterpret_cast<const lsdr_softsymbol *>(b->caps[i].out_soft) : nullptr; }
size_t lsdr_rxb_soft_cap(const lsdr_rxb *b) { return b && b->soft ? b->soft_cap : 0; }
const unsigned long long *lsdr_rxb_counts_dev(const lsdr_rxb *b) { return b ? b->d_counts : nullptr; }
// device array [n]: .total = packed decisions of capture i after the launch (struct rx_seam_result: 8-byte total first)
const void *lsdr_rxb_results_dev(const lsdr_rxb *b, size_t *stride) { if (stride) *stride = sizeof(rx_seam_result); return b ? b->d_res : nullptr; }
unsigned lsdr_rxb_tiles(const lsdr_rxb *b, unsigned i) { return b && i < b->n ? b->geo[i].n_tiles : 0; }
// debugging / tests: the detected bins of capture i (synchronous)
int lsdr_rxb_bins(lsdr_rxb *b, unsigned i, int *bins, unsigned cap, unsigned *n) {
  LSDR_ARG(b && i < b->n && n);
  const unsigned n_det = b->anf ? b->geo[i].n_det : 0;                        // the capture's own detect points
  *n = n_det;
  if (!*n || !bins) return LSDR_OK;
  LSDR_HIP(hipStreamSynchronize(b->ctx->stream));
  std::vector<int> cand((size_t)n_det * kDetMaxSlots);
  LSDR_HIP(hipMemcpy(cand.data(), b->caps[i].cand, cand.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (unsigned q = 0; q < n_det && q < cap; ++q) bins[q] = cand[(size_t)q * kDetMaxSlots];
  return LSDR_OK;
}
// seam statistics of capture i's last launch; valid once the stream has passed the launch (the caller has waited for an event behind it)
int lsdr_rxb_seam_stats(lsdr_rxb *b, unsigned i, unsigned long long *total, unsigned *dup, unsigned *miss, unsigned *bad) {
  LSDR_ARG(b && i < b->n);
  const rx_seam_result sr = b->h_res[i];
  if (total) *total = sr.total;
  if (dup) *dup = sr.ndup;
  if (miss) *miss = sr.nmiss;
  if (bad) *bad = sr.nbad;
  return LSDR_OK;
}
// tests: the notched stream of capture i as the tiles of the LAST launch saw it (n cf32 items to device memory `out`); synchronous
int lsdr_rxb_notched(lsdr_rxb *b, unsigned i, lsdr_cf32 *out_dev, size_t n) {
  LSDR_ARG(b && i < b->n && out_dev);
  if (!b->anf || !b->geom_samples) { lsdr_set_error("capture_batch: no notch in this batch (or no run yet)"); return LSDR_E_ARG; }
  const size_t usable = b->cap_samples[i] / kDetN * kDetN;
  if (n > usable) n = usable;
  if (!n) return LSDR_OK;
  rxb_args A;
  rxb_fill_args(b, A);
  // (a run without a detect point launched no detect chain: the pass-through interval 0 is written here)
  if (!b->any_det) hipLaunchKernelGGL(k_rxb_iv, dim3((b->n + 63) / 64), dim3(64), 0, b->ctx->stream, A, b->n);
  const unsigned segs = (unsigned)((n + b->pre_block - 1) / b->pre_block);
  hipLaunchKernelGGL(rxb_kernel_dump(b->in.kind), dim3((segs + 63) / 64), dim3(64), 0, b->ctx->stream, A, i, (unsigned long long)n, reinterpret_cast<float2 *>(out_dev));
  LSDR_HIP(hipGetLastError());
  LSDR_HIP(hipStreamSynchronize(b->ctx->stream));
  return LSDR_OK;
}
int lsdr_rxb_tile_time(lsdr_rxb *b, int enable, float *avg_ms, unsigned *launches) {
  LSDR_ARG(b);
  if (b->tev_pending) {
    float ms = 0.f;
    if (hipEventSynchronize(b->tev1) == hipSuccess && hipEventElapsedTime(&ms, b->tev0, b->tev1) == hipSuccess) { b->time_ms += ms; ++b->time_n; }
    b->tev_pending = false;
  }
  if (avg_ms) *avg_ms = b->time_n ? (float)(b->time_ms / b->time_n) : 0.f;
  if (launches) *launches = b->time_n;
  if (enable < 0) return LSDR_OK;      // (collect only)
  b->time_ms = 0; b->time_n = 0; b->timing = enable != 0;
  return LSDR_OK;
}

#endif  // LSDR_RXB_HOST_H
