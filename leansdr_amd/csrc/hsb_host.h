// leansdr_amd/csrc/hsb_host.h — host side of lsdr_hs_batch (hsb_device.h); included at the end of hs.hip.  The FEC tail is fec.hip's
// lsdr_tail in its form without deconvol_sync, with mpeg_sync constructed as leandvb --hs constructs it (fastlock = true, resync_period).
// run_async queues everything on the caller's context stream and reads nothing back; wait is one event synchronisation (the tail's).
#ifndef LSDR_HSB_HOST_H
#define LSDR_HSB_HOST_H

struct lsdr_hs_batch {
  lsdr_ctx *ctx;
  lsdr_hs_batch_cfg cfg;
  lsdr_tail *tail;
  hsb_args A;
  unsigned Wc, Lc, first, sym_per_chunk, max_tiles;
  size_t max_chunks;
  unsigned *d_polar; unsigned short *d_rect, *d_sincos;
  const unsigned char **d_in, **h_in;        // [B] capture pointers: device copy, pinned staging
  unsigned char **d_bytes;
  hsb_rec *d_rec, *h_rec;                    // h_rec pinned
  hsb_each *d_each, *h_each;                 // [B] per-capture geometry and tuning of a run: device copy, pinned staging
  float max_omega;
  bool in_flight;
  int lds_rect;                              // tile kernel with the rect table in LDS: 1 / 0 forced, −1 by the size of the run
  std::vector<size_t> consumed; std::vector<unsigned> tiles;   // per capture, of the last run
  std::vector<void *> owned;
};

static int hsb_alloc(lsdr_hs_batch *b, void **p, size_t bytes) {
  LSDR_HIP(hipMalloc(p, bytes ? bytes : 16));
  b->owned.push_back(*p);
  return LSDR_OK;
}

// tile geometry of a run over `chunks` 128-sample chunks (fq_run_tiled's)
static unsigned hsb_tiles_of(const lsdr_hs_batch *b, size_t chunks) {
  if (!chunks) return 0;
  unsigned n = 1;
  if (chunks > b->first) n += (unsigned)((chunks - b->first + b->Lc - 1) / b->Lc);
  return n;
}

// fast_qpsk_receiver::set_freq (sdr.h:981-986): the frequency word and the limits update_freq_limits puts around it
static void hsb_set_freq(const lsdr_hs_batch *b, float freq, long long &freqw, long long &min_freqw, long long &max_freqw) {
  freqw = (long long)(freq * 65536);
  min_freqw = (long long)((float)freqw - 65536 / b->max_omega / 8);
  max_freqw = (long long)((float)freqw + 65536 / b->max_omega / 8);
}

static int hsb_build(lsdr_hs_batch *b) {
  lsdr_ctx *c = b->ctx;
  const lsdr_hs_batch_cfg &cfg = b->cfg;
  LSDR_HIP(hipSetDevice(c->device));
  const int B = cfg.n_captures;
  const float omega = cfg.omega;
  // fast_qpsk_receiver as leandvb constructs it: set_omega, set_freq, allow_drift (sdr.h:975-992; pll_adjustment 1)
  fq_state st;
  memset(&st, 0, sizeof(st));
  const float tol = 10e-6, max_omega = omega * (1 + tol);
  b->max_omega = max_omega;
  hsb_set_freq(b, cfg.freq, st.freqw, st.min_freqw, st.max_freqw);
  const long long freq_beta = (long long)(0.0012 * 256 * 65536 / (double)omega * 1.0);
  if (freq_beta == 0) { lsdr_set_error("fast_qpsk_receiver: Excessive oversampling"); return LSDR_E_ARG; }
  // geometry: lsdr_fastqpsk_set_tiled's defaults
  b->Wc = cfg.tile_warmup ? cfg.tile_warmup / kChunk : (unsigned)((400.0f * omega + kChunk - 1) / kChunk);
  if (b->Wc < 1) b->Wc = 1;
  b->Lc = cfg.tile_len ? cfg.tile_len / kChunk : 2 * b->Wc;
  b->first = b->Lc > b->Wc ? b->Lc : b->Wc;
  unsigned spc = omega > 1.1f ? (unsigned)(kChunk / (omega - 0.1f)) + 2 : (unsigned)kChunk;   // mu advances by ≥ omega − 0.1 per symbol; one symbol per sample at most
  if (spc > (unsigned)kChunk) spc = kChunk;
  b->sym_per_chunk = spc;
  b->max_chunks = cfg.max_samples ? (cfg.max_samples - 1) / kChunk : 0;
  b->max_tiles = hsb_tiles_of(b, b->max_chunks);
  const unsigned tiles_cap = b->max_tiles ? b->max_tiles : 1;
  const unsigned parts_cap = (tiles_cap + kSeamBlock - 1) / kSeamBlock;
  const unsigned rows = (b->first * spc + 3) / 4 + 1, pitch = (tiles_cap + 63u) & ~63u;
  const size_t sym_cap = (size_t)(spc + 1) * b->max_chunks + 64;
  const size_t sym_stride = (sym_cap + 512 + 255) & ~(size_t)255;
  const size_t byte_room = sym_cap / 8 + 64;
  const unsigned P = cfg.fastlock ? 1u : 32u;                            // leandvb.cc:853, 863

  LSDR_TRY(lsdr_tail_create_ex(c, (unsigned)B, sym_cap, LSDR_FEC12, 8192, 1, byte_room, "hs_batch", &b->tail));
  LSDR_TRY(lsdr_tail_set_mpeg_sync(b->tail, 1, (int)P));

  std::vector<unsigned> polar(65536);
  std::vector<unsigned short> rect(65536), sincos(65536);
  lsdr::build_fastqpsk_tables(polar.data(), rect.data(), sincos.data());
  LSDR_TRY(hsb_alloc(b, (void **)&b->d_polar, polar.size() * 4));
  LSDR_TRY(hsb_alloc(b, (void **)&b->d_rect, rect.size() * 2));
  LSDR_TRY(hsb_alloc(b, (void **)&b->d_sincos, sincos.size() * 2));
  LSDR_HIP(hipMemcpy(b->d_polar, polar.data(), polar.size() * 4, hipMemcpyHostToDevice));
  LSDR_HIP(hipMemcpy(b->d_rect, rect.data(), rect.size() * 2, hipMemcpyHostToDevice));
  LSDR_HIP(hipMemcpy(b->d_sincos, sincos.data(), sincos.size() * 2, hipMemcpyHostToDevice));
  uint8_t *d_relabel = nullptr;
  {
    // quadrant step K of a tile's carrier frame against tile 0's (fq_run_tiled): symbols are quadrant_to_symbol[] = {0,2,3,1} (sdr.h:1067)
    static const unsigned char q2s[4] = {0, 2, 3, 1}, s2q[4] = {0, 3, 1, 2};
    std::vector<uint8_t> rel(4 * 256, 0);
    for (int K = 0; K < 4; ++K) for (int sy = 0; sy < 4; ++sy) rel[K * 256 + sy] = q2s[(s2q[sy] + K) & 3];
    LSDR_TRY(hsb_alloc(b, (void **)&d_relabel, rel.size()));
    LSDR_HIP(hipMemcpy(d_relabel, rel.data(), rel.size(), hipMemcpyHostToDevice));
  }

  hsb_args &A = b->A;
  memset(&A, 0, sizeof(A));
  A.t.polar = b->d_polar; A.t.rect = b->d_rect; A.t.sincos = b->d_sincos;
  A.t.omega = omega;
  A.t.gain_mu = (float)(0.02 / (double)(75.0f * 75.0f) * 2);             // sdr.h:1004
  A.t.freq_alpha = (long long)(0.04 * 65536);                            // sdr.h:999
  A.t.freq_beta = freq_beta;                                             // sdr.h:1000
  A.t.meas_decimation = 1048576;
  A.t.allow_drift = cfg.allow_drift ? 1 : 0;
  A.t.freq_window = (long long)(65536.0f / omega / 2048.0f);
  if (A.t.freq_window < 8) A.t.freq_window = 8;
  A.t.first_chunks = b->first; A.t.tile_chunks = b->Lc; A.t.warm_chunks = b->Wc;
  A.st0 = st;
  A.rows = rows; A.pitch = pitch; A.tiles_cap = tiles_cap; A.parts_cap = parts_cap;
  A.sym_stride = sym_stride; A.sym_cap = sym_cap;
  A.relabel = d_relabel;
  A.byte_room = byte_room;
  A.P = (int)P;
  A.best_stride = byte_room / kDcBytes + 64;
  LSDR_TRY(hsb_alloc(b, (void **)&A.stage, (size_t)B * rows * pitch * 4));
  LSDR_TRY(hsb_alloc(b, (void **)&A.info, (size_t)B * tiles_cap * sizeof(rx_tile_info_h)));
  LSDR_TRY(hsb_alloc(b, (void **)&A.fix, (size_t)B * tiles_cap * sizeof(rx_tile_fix)));
  LSDR_TRY(hsb_alloc(b, (void **)&A.part, (size_t)B * parts_cap * sizeof(rx_seam_part)));
  LSDR_TRY(hsb_alloc(b, (void **)&A.sym, (size_t)B * sym_stride));
  LSDR_TRY(hsb_alloc(b, (void **)&A.best, (size_t)B * A.best_stride));
  LSDR_TRY(hsb_alloc(b, (void **)&b->d_rec, (size_t)B * sizeof(hsb_rec)));
  LSDR_TRY(hsb_alloc(b, (void **)&b->d_in, (size_t)B * sizeof(void *)));
  LSDR_TRY(hsb_alloc(b, (void **)&b->d_bytes, (size_t)B * sizeof(void *)));
  LSDR_HIP(hipMemset(b->d_rec, 0, (size_t)B * sizeof(hsb_rec)));
  LSDR_HIP(hipHostMalloc((void **)&b->h_in, (size_t)B * sizeof(void *), hipHostMallocDefault));
  LSDR_HIP(hipHostMalloc((void **)&b->h_rec, (size_t)B * sizeof(hsb_rec), hipHostMallocDefault));
  LSDR_TRY(hsb_alloc(b, (void **)&b->d_each, (size_t)B * sizeof(hsb_each)));
  LSDR_HIP(hipMemset(b->d_each, 0, (size_t)B * sizeof(hsb_each)));
  LSDR_HIP(hipHostMalloc((void **)&b->h_each, (size_t)B * sizeof(hsb_each), hipHostMallocDefault));
  memset(b->h_each, 0, (size_t)B * sizeof(hsb_each));
  b->consumed.assign(B, 0); b->tiles.assign(B, 0);
  memset(b->h_rec, 0, (size_t)B * sizeof(hsb_rec));
  A.in = b->d_in; A.rec = b->d_rec; A.bytes = b->d_bytes; A.each = b->d_each;
  A.vit = lsdr_tail_vit_dev(b->tail);
  {
    std::vector<unsigned char *> bytes(B);
    for (int i = 0; i < B; ++i) bytes[i] = const_cast<unsigned char *>(lsdr_tail_bytes_dev(b->tail, (unsigned)i));
    LSDR_HIP(hipMemcpy(b->d_bytes, bytes.data(), (size_t)B * sizeof(void *), hipMemcpyHostToDevice));
  }
  if (lsdr_tail_byte_cap(b->tail) < byte_room) { lsdr_set_error("hs_batch: the tail's byte buffers are too small"); return LSDR_E_NOMEM; }
  // the tail reads every capture's symbol count from its record
  LSDR_TRY(lsdr_tail_bind(b->tail, nullptr, &b->d_rec[0].total, sizeof(hsb_rec)));
  // The tile kernel with the `rect` table in LDS (k_hsb_tiles_lds) gives the same symbols; measured on 8 Mi-sample captures it takes 3.3 ms
  // against 4.4 for B = 32 and the same 2.5 ms for B = 16 (profiles/hs_batch/NOTES.md), so a run takes it when it has at least half a
  // workgroup of tiles per CU, the plain kernel below that.  LSDR_HSB_LDS_RECT = 0 / 1 (tuning hook) forces one of them.
  const char *e = getenv("LSDR_HSB_LDS_RECT");
  b->lds_rect = e && *e ? (atoi(e) != 0 ? 1 : 0) : -1;
  LSDR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_hsb_tiles_lds), hipFuncAttributeMaxDynamicSharedMemorySize, 65536 * 2));
  return LSDR_OK;
}

extern "C" {

void lsdr_hs_batch_destroy(lsdr_hs_batch *b) {
  if (!b) return;
  (void)hipStreamSynchronize(b->ctx->stream);
  lsdr_tail_destroy(b->tail);
  for (void *p : b->owned) (void)hipFree(p);
  if (b->h_in) (void)hipHostFree(b->h_in);
  if (b->h_rec) (void)hipHostFree(b->h_rec);
  if (b->h_each) (void)hipHostFree(b->h_each);
  delete b;
}

int lsdr_hs_batch_create(lsdr_ctx *c, const lsdr_hs_batch_cfg *cfg, lsdr_hs_batch **out) {
  LSDR_ARG(c && cfg && out);
  LSDR_ARG(cfg->n_captures >= 1 && cfg->omega > 0);
  LSDR_ARG(cfg->tile_len % kChunk == 0 && cfg->tile_warmup % kChunk == 0);
  for (int i = 0; i < 8; ++i) LSDR_ARG(cfg->reserved[i] == 0);
  lsdr_hs_batch *b = new lsdr_hs_batch();
  b->ctx = c; b->cfg = *cfg;
  const int rc = hsb_build(b);
  if (rc) { lsdr_hs_batch_destroy(b); return rc; }
  *out = b;
  return LSDR_OK;
}

// one batch, capture i over its first n_samples[i] items with set_freq(tune[i]): what both run_async entry points come to
static int hsb_run(lsdr_hs_batch *b, const lsdr_cu8 *const *iq_dev, const size_t *n_samples, const float *tune) {
  const unsigned B = (unsigned)b->cfg.n_captures;
  // (cu8: items of 2 bytes; the tune is the object's own where it is not lsdr_hs_each_run_async's, which has checked it)
  LSDR_TRY(lsdr_in_check_each("hs_batch", "tune", B, reinterpret_cast<const void *const *>(iq_dev), nullptr, n_samples, nullptr, b->cfg.max_samples, 2));
  if (b->in_flight) { lsdr_set_error("hs_batch: a batch is in flight (lsdr_hs_batch_wait first)"); return LSDR_E_ARG; }
  lsdr_ctx *c = b->ctx;
  LSDR_HIP(hipSetDevice(c->device));
  unsigned n_tiles = 0;                                                  // the longest capture's: the grids are sized for it
  unsigned long long sum_tiles = 0;
  for (unsigned i = 0; i < B; ++i) {
    const size_t chunks = n_samples[i] >= (size_t)(kChunk + 1) ? (n_samples[i] - 1) / kChunk : 0;      // 129 samples for a chunk, sdr.h:1010-1013
    hsb_each &e = b->h_each[i];
    e.total_chunks = chunks; e.n_tiles = hsb_tiles_of(b, chunks); e.pad = 0;
    hsb_set_freq(b, tune[i], e.freqw, e.min_freqw, e.max_freqw);
    b->consumed[i] = chunks * kChunk; b->tiles[i] = e.n_tiles;
    if (e.n_tiles > n_tiles) n_tiles = e.n_tiles;
    sum_tiles += e.n_tiles;
    b->h_in[i] = reinterpret_cast<const unsigned char *>(iq_dev[i]);
  }
  const hsb_args &A = b->A;
  hipLaunchKernelGGL(k_hsb_reset, dim3((B + 63) / 64), dim3(64), 0, c->stream, A, B);
  if (n_tiles) {
    LSDR_HIP(hipMemcpyAsync(b->d_in, b->h_in, B * sizeof(void *), hipMemcpyHostToDevice, c->stream));
    LSDR_HIP(hipMemcpyAsync(b->d_each, b->h_each, B * sizeof(hsb_each), hipMemcpyHostToDevice, c->stream));
    const bool lds = b->lds_rect >= 0 ? b->lds_rect != 0 : sum_tiles >= (unsigned long long)c->num_cu * (kHsbLdsWaves * 64 / 2);
    if (lds)
      hipLaunchKernelGGL(k_hsb_tiles_lds, dim3((n_tiles + kHsbLdsWaves * 64 - 1) / (kHsbLdsWaves * 64), B), dim3(kHsbLdsWaves * 64), 65536 * 2, c->stream, A);
    else
      hipLaunchKernelGGL(k_hsb_tiles, dim3(1 + (n_tiles - 1 + 63) / 64, B), dim3(64), 0, c->stream, A);
    hipLaunchKernelGGL(k_hsb_seam, dim3((n_tiles + kSeamBlock - 1) / kSeamBlock, B), dim3(kSeamBlock), 0, c->stream, A);
    const unsigned longest = (b->first > b->Lc ? b->first : b->Lc) * b->sym_per_chunk;
    const unsigned row_blocks = ((longest + 3) / 4 + kHsbTile - 1) / kHsbTile;
    hipLaunchKernelGGL(k_hsb_compact, dim3(((n_tiles + kHsbTile - 1) / kHsbTile) * row_blocks, B), dim3(256), 0, c->stream, A, row_blocks);
  }
  // whole-chip kernels sized for max_samples, shared by the captures; a workgroup with nothing to do leaves at once
  unsigned wide = (unsigned)c->num_cu * 8u / B;
  if (wide < 16) wide = 16;
  hipLaunchKernelGGL(k_hsb_score, dim3(wide, B), dim3(256), 0, c->stream, A);
  hipLaunchKernelGGL(k_hsb_decode, dim3(wide, B), dim3(256), 0, c->stream, A);
  LSDR_HIP(hipGetLastError());
  // the records go to the host in front of the tail, whose kernels only read them: the tail's "batch done" event is behind everything wait reads
  LSDR_HIP(hipMemcpyAsync(b->h_rec, b->d_rec, B * sizeof(hsb_rec), hipMemcpyDeviceToHost, c->stream));
  LSDR_TRY(lsdr_tail_launch(b->tail));
  b->in_flight = true;
  return LSDR_OK;
}

int lsdr_hs_batch_run_async(lsdr_hs_batch *b, const lsdr_cu8 *const *iq_dev, size_t n_samples) {
  LSDR_ARG(b && iq_dev);
  LSDR_ARG(n_samples <= b->cfg.max_samples);
  const std::vector<size_t> n(b->cfg.n_captures, n_samples);
  const std::vector<float> tune(b->cfg.n_captures, b->cfg.freq);
  return hsb_run(b, iq_dev, n.data(), tune.data());
}

int lsdr_hs_each_run_async(lsdr_hs_batch *b, const lsdr_cu8 *const *iq_dev, const lsdr_capture_each *each) {
  LSDR_ARG(b && iq_dev && each);
  const int B = b->cfg.n_captures;
  LSDR_TRY(lsdr_in_check_each("hs_batch", "tune", (unsigned)B, reinterpret_cast<const void *const *>(iq_dev), each, nullptr, nullptr, b->cfg.max_samples, 2));
  std::vector<size_t> n(B);
  std::vector<float> tune(B);
  for (int i = 0; i < B; ++i) { n[i] = each[i].n_samples; tune[i] = each[i].tune; }
  return hsb_run(b, iq_dev, n.data(), tune.data());
}

int lsdr_hs_batch_wait(lsdr_hs_batch *b, lsdr_capture_result *results) {
  LSDR_ARG(b);
  if (!b->in_flight) { lsdr_set_error("hs_batch: no batch in flight"); return LSDR_E_ARG; }
  LSDR_TRY(lsdr_tail_wait(b->tail, results));
  b->in_flight = false;
  for (int i = 0; results && i < b->cfg.n_captures; ++i) {
    lsdr_capture_result &r = results[i];
    r.samples = b->consumed[i];
    r.tiles = b->tiles[i];
    r.seam_dup = b->h_rec[i].ndup; r.seam_miss = b->h_rec[i].nmiss; r.seam_bad = b->h_rec[i].nbad;
  }
  return LSDR_OK;
}

int lsdr_hs_batch_ts_download_async(lsdr_hs_batch *b, uint8_t *const *ts_host, size_t cap_bytes) {
  LSDR_ARG(b);
  return lsdr_tail_ts_download_async(b->tail, ts_host, cap_bytes);
}

int lsdr_hs_batch_ts_wait(lsdr_hs_batch *b) {
  LSDR_ARG(b);
  return lsdr_tail_ts_wait(b->tail);
}

static bool hsb_index_ok(const lsdr_hs_batch *b, int i) { return b && i >= 0 && i < b->cfg.n_captures; }
const uint8_t *lsdr_hs_batch_ts_dev(const lsdr_hs_batch *b, int i) { return hsb_index_ok(b, i) ? lsdr_tail_ts_dev(b->tail, (unsigned)i) : nullptr; }
const uint8_t *lsdr_hs_batch_symbols_dev(const lsdr_hs_batch *b, int i) { return hsb_index_ok(b, i) ? b->A.sym + (size_t)i * b->A.sym_stride : nullptr; }
const uint8_t *lsdr_hs_batch_bytes_dev(const lsdr_hs_batch *b, int i) { return hsb_index_ok(b, i) ? lsdr_tail_bytes_dev(b->tail, (unsigned)i) : nullptr; }
const uint8_t *lsdr_hs_batch_mpeg_dev(const lsdr_hs_batch *b, int i) { return hsb_index_ok(b, i) ? lsdr_tail_mpeg_dev(b->tail, (unsigned)i) : nullptr; }

}  // extern "C"

#endif  // LSDR_HSB_HOST_H
