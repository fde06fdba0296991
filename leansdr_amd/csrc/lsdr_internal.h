// leansdr_amd/csrc/lsdr_internal.h — shared internals of liblsdr_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/lsdr_hip.h"

struct lsdr_arena;
struct lsdr_ctx {
  int device;
  hipStream_t stream;
  bool own_stream;
  hipEvent_t ev0, ev1;
  int num_cu;
  void *bounce;          // scratch of lsdr_memcpy_d2d for overlapping ranges (pipebuf::pack)
  size_t bounce_cap;
  // copy engine (lsdr_copy_*): one upload and one download stream next to the compute stream, created on first use
  hipStream_t up, down;
  hipEvent_t ev_up, ev_compute;
  bool copy_ready;
  // rs_decoder (fec.hip): GF(256) tables and the corrected-bits counter of THIS context (two contexts on one device decode
  // concurrently on their own streams)
  void *rs_tables;
  unsigned long long *rs_counter;
  // Pinned bounce arena for per-call bookkeeping transfers (lsdr_stage_*): see below.
  char *stage_base;
  size_t stage_cap, stage_used;
  struct stage_pend { void *dst; const char *src; size_t bytes; };
  std::vector<stage_pend> stage_pending;   // D2H results to hand to their host destinations at the next lsdr_stage_sync
  std::vector<char *> stage_retired;       // outgrown arenas, still referenced by copies in flight
  // placed stream buffers (arena.hip): lsdr_malloc serves requests of 1 MiB or more from here while set (lsdr_ctx_set_arena)
  lsdr_arena *arena;
};
int lsdr_arena_malloc(lsdr_arena *a, size_t bytes, void **p);      // (arena.hip; LSDR_E_NOMEM when the arena has no free window)

struct lsdr_event {
  lsdr_ctx *ctx;
  hipEvent_t ev;
};

// Environment hooks come in two kinds.  Tuning / test hooks (plain getenv in the sources; INTEGRATION.md §6 lists them) choose
// among kernels and launch parameters that ALL give the documented results.  Measurement hooks skip or corrupt work (no filter
// launch, no receiver kernels, timing-only tiles, poisoned hand-off buffers): they exist only in the `make measure` build
// (-DLSDR_MEASURE → tools/variants/liblsdr_hip_measure.so); in the shipped library the macro does not even keep the name.
#ifdef LSDR_MEASURE
#define LSDR_MEASURE_ENV(name) getenv(name)
#else
#define LSDR_MEASURE_ENV(name) ((const char *)nullptr)
#endif

void lsdr_set_error(const char *fmt, ...);
int lsdr_hip_fail(hipError_t e, const char *what, const char *file, int line);

#define LSDR_HIP(call)                                                  \
  do {                                                                  \
    hipError_t e__ = (call);                                            \
    if (e__ != hipSuccess) return lsdr_hip_fail(e__, #call, __FILE__, __LINE__); \
  } while (0)

#define LSDR_TRY(call)                                                  \
  do {                                                                  \
    const int rc__ = (call);                                            \
    if (rc__) return rc__;                                              \
  } while (0)

#define LSDR_ARG(cond)                                                  \
  do {                                                                  \
    if (!(cond)) {                                                      \
      lsdr_set_error("%s:%d: bad argument: %s", __FILE__, __LINE__, #cond); \
      return LSDR_E_ARG;                                                \
    }                                                                   \
  } while (0)

// Bookkeeping transfers between the compute stream and ordinary (pageable) host memory — job lists, per-tile states, totals.
// hipMemcpyAsync on a pageable buffer of 128 KiB or more makes the runtime pin the caller's pages for the transfer; when that
// buffer (a std::vector) is freed afterwards, the unmap invalidates the pinned range and the driver suspends and restores
// every queue of the process: the next submission waits ~25 ms (measured: the 8PSK 2/3 chain ran 8x slower for it).  These
// go through one pinned arena per context instead:
//   lsdr_stage_h2d: the bytes are copied into the arena first, so `src_host` may be freed as soon as the call returns;
//   lsdr_stage_d2h: lands in the arena; `dst_host` holds the bytes after the next lsdr_stage_sync;
//   lsdr_stage_sync: hipStreamSynchronize(c->stream), then delivers every pending D2H and empties the arena.
int lsdr_stage_h2d(lsdr_ctx *c, void *dst_dev, const void *src_host, size_t bytes);
int lsdr_stage_d2h(lsdr_ctx *c, void *dst_host, const void *src_dev, size_t bytes);
int lsdr_stage_sync(lsdr_ctx *c);

// fir_filter.hip: the matrix-pipe pass of the fused auto_notch + fir_filter block (notch.hip)
int lsdr_fir_stream_iv_launch(lsdr_ctx *c, const void *in, size_t n_in, lsdr_cf32 *out, size_t count, unsigned align_n, unsigned D, unsigned nq,
                              const float *iv_tabs, const unsigned *iv_tile_first, unsigned n_iv, int wpc, unsigned *outputs_per_tile, hipStream_t stream = nullptr);

// ---- capture batch (capture_batch.hip): its two halves
// cstln_receiver.hip (rxb_host.h): the front end — auto_notch + cstln_receiver of every capture in shared launches, packed decisions out
struct lsdr_rxb;
struct lsdr_in_desc;                                                      // capture_input.h
int lsdr_rxb_describe_in(int in_format, float in_scale, lsdr_in_desc *out);   // what lsdr_rxb_create_in makes of them, or its refusal
int lsdr_rxb_create_in(lsdr_ctx *c, const lsdr_capture_batch_cfg *cfg, int soft, float pll_adjustment, int in_format, float in_scale, lsdr_rxb **out);
void lsdr_rxb_destroy(lsdr_rxb *b);
int lsdr_rxb_launch(lsdr_rxb *b, const void *const *iq, const size_t *n_samples /* [n] */, const float *tune /* [n] */, size_t *consumed /* [n] */,
                    hipStream_t aux = nullptr);
const uint32_t *lsdr_rxb_words(const lsdr_rxb *b, unsigned i);
size_t lsdr_rxb_words_cap(const lsdr_rxb *b);
const lsdr_softsymbol *lsdr_rxb_soft(const lsdr_rxb *b, unsigned i);
size_t lsdr_rxb_soft_cap(const lsdr_rxb *b);
const unsigned long long *lsdr_rxb_counts_dev(const lsdr_rxb *b);
const void *lsdr_rxb_results_dev(const lsdr_rxb *b, size_t *stride);
unsigned lsdr_rxb_tiles(const lsdr_rxb *b, unsigned i);
int lsdr_rxb_bins(lsdr_rxb *b, unsigned i, int *bins, unsigned cap, unsigned *n);
int lsdr_rxb_seam_stats(lsdr_rxb *b, unsigned i, unsigned long long *total, unsigned *dup, unsigned *miss, unsigned *bad);
int lsdr_rxb_tile_time(lsdr_rxb *b, int enable, float *avg_ms, unsigned *launches);
int lsdr_rxb_notched(lsdr_rxb *b, unsigned i, lsdr_cf32 *out_dev, size_t n);
// signal reports: the estimators at a measurement instant (cstln_receiver.hip's rx_meas); `a` and `tile` are the scan's own
struct lsdr_rxb_report { float freqw, est_insp, est_sp, est_ep, a; unsigned tile; };
int lsdr_rxb_set_reports(lsdr_rxb *b, unsigned long long period_samples);
int lsdr_rxb_reports_on(const lsdr_rxb *b);
int lsdr_rxb_reports(const lsdr_rxb *b, unsigned i, const lsdr_rxb_report **slots, size_t *n, lsdr_rxb_report *last);
// fec.hip (tail_host.h): the FEC tail of every capture, counts on the device, with its output side — the wait for a batch, the result
// records and the TS download.  who: the owner's prefix in error texts ("capture_batch" / "hs_batch").
struct lsdr_tail;
int lsdr_tail_create_ex(lsdr_ctx *c, unsigned n, size_t sym_cap, int rate, unsigned window, int nodeconv, size_t bytes_per_capture, const char *who,
                        lsdr_tail **out);
int lsdr_tail_set_bytes(lsdr_tail *t, const unsigned long long *bytes, const unsigned *alignment);
size_t lsdr_tail_byte_cap(const lsdr_tail *t);
void lsdr_tail_destroy(lsdr_tail *t);
int lsdr_tail_bind(lsdr_tail *t, const uint32_t *const *words, const void *counts_dev, size_t count_stride);
int lsdr_tail_launch(lsdr_tail *t);                                       // … and records "batch done" behind the last kernel
int lsdr_tail_wait(lsdr_tail *t, lsdr_capture_result *results);           // fills the tail's fields; samples, tiles, seam_* are the owner's
int lsdr_tail_relock_set(lsdr_tail *t, unsigned relocks);                 // re-acquisitions of the next launches (tail_relock.h); 0: off
int lsdr_tail_relock_stats(const lsdr_tail *t, unsigned i, lsdr_capture_relock_stats *s);   // after lsdr_tail_wait
bool lsdr_tail_waited(const lsdr_tail *t);                                // between lsdr_tail_wait and the next launch or lsdr_tail_stale
void lsdr_tail_stale(lsdr_tail *t);                                       // clears it ahead of a launch that comes later
int lsdr_tail_ts_download_async(lsdr_tail *t, uint8_t *const *ts_host, size_t cap_bytes);
int lsdr_tail_ts_wait(lsdr_tail *t);
const uint8_t *lsdr_tail_ts_dev(const lsdr_tail *t, unsigned i);
const uint8_t *lsdr_tail_bytes_dev(const lsdr_tail *t, unsigned i);
const uint8_t *lsdr_tail_mpeg_dev(const lsdr_tail *t, unsigned i);
// the tail without deconvol_sync (nodeconv) behind a producer that stays on the device (hs.hip's lsdr_hs_batch): mpeg_sync's public members
// fastlock / resync_period (dvb.h:716-717) as every capture's block is constructed, and the [n] device records {bytes, alignment} that
// k_tail_acquire_bytes reads — written by the producer's last kernel instead of lsdr_tail_set_bytes
struct lsdr_tail_vit { unsigned long long bytes; unsigned alignment, pad; };   // = tail_device.h's tail_vit
int lsdr_tail_set_mpeg_sync(lsdr_tail *t, int fastlock, int resync_period);
lsdr_tail_vit *lsdr_tail_vit_dev(lsdr_tail *t);

// fec.hip: what deconvol_sync's constructor derives for one code rate (dvb.h:122-293, 480-513) — the puncturing patterns, punctperiod (pp),
// punctweight (pw), the inverse polynomials deconv[0 … pp) and their alternates deconv2 (equal to deconv where the reference lists none).
// Host only.  lsdr_deconv_create and lsdr_fec_est_create (fec_est.hip) both take their polynomials from here.
struct lsdr_deconv_polys {
  unsigned conv[2], punct[2];
  int pp, pw;
  unsigned long long response[64], deconv[8], deconv2[8];
};
int lsdr_deconv_polys_build(int rate, lsdr_deconv_polys *P);
// … and init_syncs' four alignments (dvb.h:308-360): luts[alignment][symbol & 3] = the symbol's I/Q bits, I << 1 | Q
void lsdr_deconv_luts(unsigned char luts[4][4]);

// Host-side table builders (host_tables.cpp)
namespace lsdr {
void fir_shift_coeffs(unsigned ncoeffs, const float *coeffs, float freq, lsdr_cf32 *shifted);
struct cstln_tables {
  int nsymbols, nrotations;
  int8_t symbols[256][2];
  std::vector<int16_t> cost, phase_error;
  std::vector<uint8_t> symbol;
};
int build_cstln(int predef, int fec, cstln_tables &t);
// fast_qpsk_receiver::init_lookup_tables (sdr.h:1154-1171), packed: polar[re*256+im] = a | r<<16,
// rect[a*256+r] = re | im<<8, sincos[a] = re | im<<8.
void build_fastqpsk_tables(unsigned *polar, unsigned short *rect, unsigned short *sincos);
}  // namespace lsdr
