// leansdr_amd/csrc/tail_host.h — host side of the device-resident FEC tail (tail_device.h); included at the end of fec.hip.
// Internal API (lsdr_internal.h) of lsdr_capture_batch (capture_batch.hip) and lsdr_hs_batch (hsb_host.h).  The tail owns its output side:
// the "batch done" event behind its last kernel, the result records, and the TS download on a stream of its own.
#ifndef LSDR_TAIL_HOST_H
#define LSDR_TAIL_HOST_H

struct lsdr_tail {
  lsdr_ctx *ctx;
  unsigned n;
  size_t sym_cap, byte_cap, pk_cap;
  lsdr_deconv *dec;                 // the polynomials / alignment tables of deconvol_sync, built once by its own constructor
  lsdr_derandomizer *der;           // the PRBS pattern on the device
  tail_args A;
  std::vector<tail_cap> caps;       // host copy (pointers)
  tail_cap *d_caps;
  tail_result *h_res, *h_res_dev;   // pinned, [n]
  std::vector<void *> owned;
  bool nodeconv;                    // the Viterbi engine's tail: `bytes` is filled by viterbi_sync (k_tail_acquire_bytes)
  tail_vit *h_vit, *d_vit;          // nodeconv: [n] pinned staging and device records
  const char *who;                  // the owner's prefix in error texts ("capture_batch" / "hs_batch")
  hipEvent_t ev_done, ev_dl;        // behind the last kernel of a launch; behind the last TS download
  hipStream_t dl;                   // TS downloads
  bool dl_pending, waited;          // waited: between lsdr_tail_wait and the next launch — results and TS are stable
  unsigned relocks, ran_relocks;    // re-acquisitions asked for (0: off); what the last launch ran with
  tail_relock_rec *h_rl, *h_rl_dev; // pinned, [n]
};

static int tail_alloc(lsdr_tail *t, void **p, size_t bytes) {
  LSDR_HIP(hipMalloc(p, bytes ? bytes : 16));
  t->owned.push_back(*p);
  return LSDR_OK;
}

// nodeconv (bytes_per_capture != 0): the tail behind viterbi_sync — no deconvol_sync; every capture's `bytes` buffer takes that many bytes.
// who: the owner's prefix in error texts (a string literal).
int lsdr_tail_create_ex(lsdr_ctx *c, unsigned n, size_t sym_cap, int rate, unsigned window, int nodeconv, size_t bytes_per_capture, const char *who,
                        lsdr_tail **out) {
  LSDR_ARG(c && out && who && n >= 1 && sym_cap >= 1 && window >= 2048);      // (mpeg_sync's search needs 204·8 + 1 bytes in one call)
  LSDR_ARG(!nodeconv || bytes_per_capture >= 1);
  LSDR_HIP(hipSetDevice(c->device));
  lsdr_tail *t = new lsdr_tail();
  t->ctx = c; t->n = n; t->sym_cap = sym_cap; t->nodeconv = nodeconv != 0; t->h_vit = nullptr; t->d_vit = nullptr; t->who = who;
  *out = t;                                                             // (from here on the caller destroys on error)
  LSDR_HIP(hipEventCreateWithFlags(&t->ev_done, hipEventDisableTiming));
  LSDR_HIP(hipEventCreateWithFlags(&t->ev_dl, hipEventDisableTiming));
  LSDR_HIP(hipStreamCreateWithFlags(&t->dl, hipStreamNonBlocking));
  if (!t->nodeconv) LSDR_TRY(lsdr_deconv_create(c, rate, 0, &t->dec));
  LSDR_TRY(lsdr_derandomizer_create(c, &t->der));
  gf_tables *tab = rs_device_tables(c);
  if (!tab) { lsdr_set_error("%s: cannot allocate GF tables", who); return LSDR_E_NOMEM; }
  memset(&t->A, 0, sizeof(t->A));
  if (t->nodeconv) {
    t->byte_cap = (bytes_per_capture + 65536 + 3) & ~(size_t)3;
    LSDR_HIP(hipMalloc((void **)&t->d_vit, n * sizeof(tail_vit)));
    LSDR_HIP(hipMemset(t->d_vit, 0, n * sizeof(tail_vit)));
    LSDR_HIP(hipHostMalloc((void **)&t->h_vit, n * sizeof(tail_vit), hipHostMallocDefault));
  } else {
    const deconv_host &H = t->dec->H;
    // bytes out of sym_cap symbols (rate pp/(pw/2) bits per symbol) with slack; packets of 204 bytes
    t->byte_cap = (size_t)((unsigned long long)sym_cap * (unsigned)H.pp / (unsigned)(H.pw / 2) / 8) + 65536;
    for (int b = 0; b < 8; ++b) t->A.D.deconv[b] = b < H.pp ? H.deconv[b] : 0;
    t->A.D.pp = H.pp; t->A.D.pw = H.pw;
    for (int a = 0; a < 4; ++a) for (int s = 0; s < 4; ++s) t->A.luts[a][s] = t->dec->luts[a][s];
  }
  t->pk_cap = t->byte_cap / kRS + 64;
  memset(&t->A.ms0, 0, sizeof(t->A.ms0));
  t->A.ms0.scan_syncs = 8; t->A.ms0.want_syncs = 4; t->A.ms0.lock_timeout = 4; t->A.ms0.resync_period = 1;      // dvb.h:727-731
  t->A.gtab = tab;
  t->A.window = window;
  {
    uint8_t G[17];
    lsdr_rs_tables(nullptr, nullptr, G);                                // G[i] = coefficient of x^(16−i) (rs.h:93-105); G[0] = 1
    for (int m = 0; m < 16; ++m) t->A.rs_g[m] = G[1 + m];
  }
  t->A.pattern = t->der->d_pattern;
  t->caps.assign(n, tail_cap());
  LSDR_HIP(hipMalloc((void **)&t->d_caps, n * sizeof(tail_cap)));
  LSDR_HIP(hipHostMalloc((void **)&t->h_res, n * sizeof(tail_result), hipHostMallocDefault));
  LSDR_HIP(hipHostGetDevicePointer((void **)&t->h_res_dev, t->h_res, 0));
  memset(t->h_res, 0, n * sizeof(tail_result));
  LSDR_HIP(hipHostMalloc((void **)&t->h_rl, n * sizeof(tail_relock_rec), hipHostMallocDefault));
  LSDR_HIP(hipHostGetDevicePointer((void **)&t->h_rl_dev, t->h_rl, 0));
  memset(t->h_rl, 0, n * sizeof(tail_relock_rec));
  for (unsigned i = 0; i < n; ++i) {
    tail_cap &tc = t->caps[i];
    memset(&tc, 0, sizeof(tc));
    LSDR_TRY(tail_alloc(t, (void **)&tc.bytes, t->byte_cap + 64));
    LSDR_TRY(tail_alloc(t, (void **)&tc.mpeg, t->byte_cap + 64));
    LSDR_TRY(tail_alloc(t, (void **)&tc.rs, (t->pk_cap + kRsChunk) * kRS + 64));        // (k_tail_rs stages 16-byte pieces: room behind the last packet)
    LSDR_TRY(tail_alloc(t, (void **)&tc.rts, t->pk_cap * kTS));
    LSDR_TRY(tail_alloc(t, (void **)&tc.ts, t->pk_cap * kTS));
    LSDR_TRY(tail_alloc(t, (void **)&tc.first, t->pk_cap + kRsChunk));
    LSDR_TRY(tail_alloc(t, (void **)&tc.pkt_pos, t->pk_cap * sizeof(int)));
    LSDR_TRY(tail_alloc(t, (void **)&tc.pkt_dst, t->pk_cap * sizeof(long long)));
    tc.byte_cap = t->byte_cap; tc.pk_cap = t->pk_cap;
    tc.res = t->h_res_dev + i;
    tc.rl = t->h_rl_dev + i;
    if (t->nodeconv) tc.vit = t->d_vit + i;
  }
  t->A.caps = t->d_caps;
  return LSDR_OK;
}

void lsdr_tail_destroy(lsdr_tail *t) {
  if (!t) return;
  if (t->dl) (void)hipStreamSynchronize(t->dl);
  (void)hipStreamSynchronize(t->ctx->stream);
  for (void *p : t->owned) (void)hipFree(p);
  (void)hipFree(t->d_caps);
  if (t->h_res) (void)hipHostFree(t->h_res);
  if (t->h_rl) (void)hipHostFree(t->h_rl);
  (void)hipFree(t->d_vit);
  if (t->h_vit) (void)hipHostFree(t->h_vit);
  if (t->dec) lsdr_deconv_destroy(t->dec);
  lsdr_derandomizer_destroy(t->der);
  if (t->ev_done) (void)hipEventDestroy(t->ev_done);
  if (t->ev_dl) (void)hipEventDestroy(t->ev_dl);
  if (t->dl) (void)hipStreamDestroy(t->dl);
  delete t;
}

// Inputs of capture i: its packed decisions and where their count will be (device memory, 8 bytes).  Uploads the records.
int lsdr_tail_bind(lsdr_tail *t, const uint32_t *const *words, const void *counts_dev, size_t count_stride) {
  LSDR_ARG(t && (words || t->nodeconv) && counts_dev);
  for (unsigned i = 0; i < t->n; ++i) {
    t->caps[i].words = words ? words[i] : nullptr;
    t->caps[i].nsym = reinterpret_cast<const unsigned long long *>(static_cast<const char *>(counts_dev) + i * count_stride);
  }
  LSDR_HIP(hipMemcpy(t->d_caps, t->caps.data(), t->n * sizeof(tail_cap), hipMemcpyHostToDevice));
  return LSDR_OK;
}

// nodeconv: what viterbi_sync committed for every capture (bytes already in lsdr_tail_bytes_dev(i)) and its alignment; queued on the
// context's stream in front of the next lsdr_tail_launch.  The previous launch must have completed (single-buffered staging).
int lsdr_tail_set_bytes(lsdr_tail *t, const unsigned long long *bytes, const unsigned *alignment) {
  LSDR_ARG(t && t->nodeconv && bytes && alignment);
  LSDR_HIP(hipSetDevice(t->ctx->device));
  for (unsigned i = 0; i < t->n; ++i) { t->h_vit[i].bytes = bytes[i]; t->h_vit[i].alignment = alignment[i]; t->h_vit[i].pad = 0; }
  LSDR_HIP(hipMemcpyAsync(t->d_vit, t->h_vit, t->n * sizeof(tail_vit), hipMemcpyHostToDevice, t->ctx->stream));
  return LSDR_OK;
}

int lsdr_tail_set_mpeg_sync(lsdr_tail *t, int fastlock, int resync_period) {
  LSDR_ARG(t && resync_period >= 1);
  t->A.ms0.fastlock = fastlock ? 1 : 0; t->A.ms0.resync_period = resync_period;
  return LSDR_OK;
}
lsdr_tail_vit *lsdr_tail_vit_dev(lsdr_tail *t) { return t && t->nodeconv ? reinterpret_cast<lsdr_tail_vit *>(t->d_vit) : nullptr; }

// Queues the tail of every capture on the context's stream, and the "batch done" event behind it.  The kernel that WRITES the TS buffers
// waits for a pending download of the previous batch's TS.
int lsdr_tail_launch(lsdr_tail *t) {
  LSDR_ARG(t);
  lsdr_ctx *c = t->ctx;
  LSDR_HIP(hipSetDevice(c->device));
  const dim3 one(1, t->n);
  // whole-chip kernels: enough workgroups for the largest capture, shared by the captures (a workgroup with nothing to do leaves at once)
  unsigned wide = (unsigned)c->num_cu * 8u / t->n;
  if (wide < 16) wide = 16;
  wide = (wide + 7) / 8 * 8;
  const dim3 grid(wide, t->n);
  t->ran_relocks = t->nodeconv ? 0u : t->relocks;
  if (t->ran_relocks) {
    // R + 2 steps of the window loop, a whole-chip call between two of them; nothing is read in between (a capture with nothing to do
    // leaves every kernel at once)
    const unsigned R = t->ran_relocks;
    hipLaunchKernelGGL(k_tail_relock, one, dim3(256), 0, c->stream, t->A, R, 1, 0);
    for (unsigned p = 0; p <= R; ++p) {
      hipLaunchKernelGGL(k_tail_deconv, grid, dim3(256), 0, c->stream, t->A);
      hipLaunchKernelGGL(k_tail_realign, grid, dim3(256), 0, c->stream, t->A);
      hipLaunchKernelGGL(k_tail_relock, one, dim3(256), 0, c->stream, t->A, R, 0, p == R ? 1 : 0);
    }
  } else {
    if (t->nodeconv) {
      hipLaunchKernelGGL(k_tail_acquire_bytes, one, dim3(256), 0, c->stream, t->A);
    } else {
      hipLaunchKernelGGL(k_tail_acquire, one, dim3(256), 0, c->stream, t->A);
      hipLaunchKernelGGL(k_tail_deconv, grid, dim3(256), 0, c->stream, t->A);
    }
    hipLaunchKernelGGL(k_tail_realign, grid, dim3(256), 0, c->stream, t->A);
    hipLaunchKernelGGL(k_tail_book, one, dim3(256), 0, c->stream, t->A);
  }
  hipLaunchKernelGGL(k_tail_deint, grid, dim3(256), 0, c->stream, t->A);
  hipLaunchKernelGGL(k_tail_rs, grid, dim3(256), 0, c->stream, t->A);
  hipLaunchKernelGGL(k_tail_derand_scan, one, dim3(1024), 0, c->stream, t->A);
  LSDR_HIP(hipGetLastError());
  if (t->dl_pending) LSDR_HIP(hipStreamWaitEvent(c->stream, t->ev_dl, 0));
  hipLaunchKernelGGL(k_tail_derand_apply, grid, dim3(256), 0, c->stream, t->A);
  LSDR_HIP(hipGetLastError());
  LSDR_HIP(hipEventRecord(t->ev_done, c->stream));
  t->waited = false;
  return LSDR_OK;
}

// Waits for the last launch.  results (may be null): every record zeroed, then the tail's fields; samples, tiles and seam_* are the owner's.
int lsdr_tail_wait(lsdr_tail *t, lsdr_capture_result *results) {
  LSDR_ARG(t);
  LSDR_HIP(hipEventSynchronize(t->ev_done));
  t->waited = true;
  for (unsigned i = 0; results && i < t->n; ++i) {
    const tail_result &tr = t->h_res[i];
    lsdr_capture_result &r = results[i];
    memset(&r, 0, sizeof(r));
    r.ts_packets = tr.n_ts; r.rs_packets = tr.n_rs; r.rs_bit_errors = tr.rs_bit_errors; r.symbols = tr.symbols;
    r.bytes_deconv = tr.bytes_deconv; r.bytes_mpeg = tr.bytes_mpeg; r.first_lock_byte = tr.first_lock_byte;
    r.next_sync_calls = tr.next_sync_calls; r.locked = tr.locked_at_end; r.alignment = tr.alignment; r.bitphase = tr.bitphase;
  }
  return LSDR_OK;
}
// Re-acquisitions of the NEXT launches (0: off, the tail as it is without this call); the owner refuses the call while a batch is in flight.
int lsdr_tail_relock_set(lsdr_tail *t, unsigned relocks) {
  LSDR_ARG(t);
  if (t->nodeconv) { lsdr_set_error("%s: re-acquisition belongs to the default engine's tail (deconvol_sync)", t->who); return LSDR_E_UNSUPPORTED; }
  if (relocks > kRelockMax) { lsdr_set_error("%s: relocks is %u, at most %u", t->who, relocks, kRelockMax); return LSDR_E_ARG; }
  t->relocks = relocks;
  return LSDR_OK;
}
// Capture i's record of the waited-for batch; a batch that ran with re-acquisition off leaves it zero with both offsets ~0.
int lsdr_tail_relock_stats(const lsdr_tail *t, unsigned i, lsdr_capture_relock_stats *s) {
  LSDR_ARG(t && s && i < t->n);
  if (t->nodeconv) { lsdr_set_error("%s: re-acquisition belongs to the default engine's tail (deconvol_sync)", t->who); return LSDR_E_UNSUPPORTED; }
  if (!t->waited) { lsdr_set_error("%s: relock stats before lsdr_%s_wait", t->who, t->who); return LSDR_E_ARG; }
  memset(s, 0, sizeof(*s));
  s->first_drop_byte = s->last_lock_byte = ~0ull;
  if (t->ran_relocks) memcpy(s, &t->h_rl[i], sizeof(*s));
  return LSDR_OK;
}
bool lsdr_tail_waited(const lsdr_tail *t) { return t && t->waited; }
// a batch is under way in front of the tail (the Viterbi engine launches the tail only in its wait): the last batch's output is no longer current
void lsdr_tail_stale(lsdr_tail *t) { if (t) t->waited = false; }

// Every capture's TS of the waited-for batch to ts_host[i] (cap_bytes each), on the download stream; the next launch's TS writes wait for it.
int lsdr_tail_ts_download_async(lsdr_tail *t, uint8_t *const *ts_host, size_t cap_bytes) {
  LSDR_ARG(t && ts_host);
  if (!t->waited) { lsdr_set_error("%s: TS download before lsdr_%s_wait", t->who, t->who); return LSDR_E_ARG; }
  for (unsigned i = 0; i < t->n; ++i) {
    const size_t bytes = (size_t)t->h_res[i].n_ts * kTS;
    if (bytes > cap_bytes) { lsdr_set_error("%s: capture %d has %zu TS bytes, the host buffer %zu", t->who, (int)i, bytes, cap_bytes); return LSDR_E_ARG; }
    if (bytes) LSDR_HIP(hipMemcpyAsync(ts_host[i], t->caps[i].ts, bytes, hipMemcpyDeviceToHost, t->dl));
  }
  LSDR_HIP(hipEventRecord(t->ev_dl, t->dl));
  t->dl_pending = true;
  return LSDR_OK;
}

int lsdr_tail_ts_wait(lsdr_tail *t) {
  LSDR_ARG(t);
  if (t->dl_pending) LSDR_HIP(hipEventSynchronize(t->ev_dl));
  t->dl_pending = false;
  return LSDR_OK;
}

const uint8_t *lsdr_tail_ts_dev(const lsdr_tail *t, unsigned i) { return t && i < t->n ? t->caps[i].ts : nullptr; }
// tests: the deconvolved bytes / the mpeg_sync output of capture i (device pointers; counts in the result record)
size_t lsdr_tail_byte_cap(const lsdr_tail *t) { return t ? t->byte_cap : 0; }
const uint8_t *lsdr_tail_bytes_dev(const lsdr_tail *t, unsigned i) { return t && i < t->n ? t->caps[i].bytes : nullptr; }
const uint8_t *lsdr_tail_mpeg_dev(const lsdr_tail *t, unsigned i) { return t && i < t->n ? t->caps[i].mpeg : nullptr; }

static_assert(sizeof(lsdr_capture_relock_stats) == 40 && sizeof(tail_relock_rec) == 40 &&
              offsetof(lsdr_capture_relock_stats, first_drop_byte) == offsetof(tail_relock_rec, first_drop_byte) &&
              offsetof(lsdr_capture_relock_stats, next_sync_behind_first_lock) == offsetof(tail_relock_rec, next_sync_behind_first_lock),
              "include/lsdr_hip.h's lsdr_capture_relock_stats mirrors tail_device.h's tail_relock_rec");
static_assert(sizeof(lsdr_tail_vit) == sizeof(tail_vit) && offsetof(lsdr_tail_vit, alignment) == offsetof(tail_vit, alignment),
              "lsdr_internal.h mirrors tail_device.h's tail_vit");

#endif  // LSDR_TAIL_HOST_H
