/* include/lsdr_hip.h — C ABI of the MI355X-native leandvb hot path.
 *
 * This is the drop-in boundary: the reference has no FFI layer,
 * a "block" is a C++ `runnable` whose run() moves items between pipebufs
 * (framework.h:124-131).  The host keeps that scheduler/pipebuf surface
 * (leansdr_amd/host headers, same class names and constructor signatures) and each
 * GPU-backed block's run() calls exactly one of the `*_run` entry points below.
 * Every entry point names the reference interface it replaces.
 *
 * Conventions
 *  - Plain C types only.  No torch / HIP types: a stream is passed as void*.
 *  - All `in`/`out` data pointers are DEVICE pointers (HBM) unless the name
 *    ends in `_host`.  lsdr_malloc/lsdr_memcpy_* exist so that a host without
 *    any HIP binding can own device pipebufs.
 *  - Every function returns 0 on success, <0 on error (LSDR_E_*); the message
 *    is available from lsdr_last_error().  The C++ shim maps !=0 to the
 *    reference's fail() (framework.h:33).  "Not enough input / no room" is not
 *    an error: *produced == 0, exactly like a reference run() that returns
 *    without progress (SURVEY §8b "Error convention").
 *  - One lsdr_ctx = one device + one HIP stream; all calls on a ctx (and on the
 *    blocks created on it) must come from one thread at a time (the scheduler
 *    thread, README.coding.md:29).  Different contexts may be driven from
 *    different threads concurrently (per-context tables, counters and staging;
 *    lsdr_last_error() is per thread): bench_more.py runs the front end and the
 *    FEC tail of one capture that way.
 *  - Work is enqueued on the ctx stream.  Functions whose outputs have a
 *    data-dependent size (cstln_receiver, the FEC tail) synchronise before
 *    returning so that the scheduler's progress hash (framework.h:96-113)
 *    never sees "no progress" while work is in flight.
 *  - Item layouts are the reference's: cf32 {float re,im} 8 B,
 *    cu8 {u8 re,im} 2 B, softsymbol {int16 cost; u8 symbol; u8 pad} 4 B,
 *    rspacket 204 B, tspacket 188 B.
 */
#ifndef LSDR_HIP_H
#define LSDR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSDR_ABI_VERSION 2

enum { LSDR_OK = 0, LSDR_E_HIP = -1, LSDR_E_ARG = -2, LSDR_E_NOMEM = -3, LSDR_E_UNSUPPORTED = -4 };

typedef struct { float re, im; } lsdr_cf32;
typedef struct { uint8_t re, im; } lsdr_cu8;
typedef struct { int16_t cost; uint8_t symbol; uint8_t pad; } lsdr_softsymbol; /* sdr.h:287-290 */

/* ------------------------------------------------------------------ context */
typedef struct lsdr_ctx lsdr_ctx;
int lsdr_abi_version(void);
/* PCI address of a device ("0000:c1:00.0", at least 16 bytes): lets the host pin a capture's threads to the GPU's NUMA node */
int lsdr_device_pci_bus_id(int device, char *buf, int len);
const char *lsdr_last_error(void);
/* stream == NULL: the ctx creates (and owns) a non-blocking HIP stream.
 *
 * PROCESS-WIDE SIDE EFFECT: the first context created in a process changes the C library's allocator policy for the WHOLE
 * process — mallopt(M_MMAP_THRESHOLD, 32 MiB) and mallopt(M_TRIM_THRESHOLD, 2 GiB), once, thread-safe (glibc only).  Reason: when
 * a host block of hundreds of KB is freed, glibc unmaps it; the amdgpu MMU notifier then suspends and restores every GPU queue of
 * the process, and the next submission waits 20-25 ms (measured: viterbi_sync 25 ms per call instead of 4.5).  Consequence for the
 * host application: freed host memory up to 32 MiB per block stays in the process heap instead of going back to the OS.  Set
 * LSDR_KEEP_MALLOC=1 in the environment before the first context to leave the allocator alone (and accept the stalls, or keep
 * your own large host buffers alive while GPU work is queued). */
int lsdr_ctx_create(int device, void *hip_stream, lsdr_ctx **ctx);
/* A context whose stream may only use the compute units set in cu_mask (bit i of word i/32 = CU i): lets two blocks
 * that would disturb each other (the HBM-streaming fir_filter and the latency-bound receiver tiles) own disjoint parts of
 * the chip.  Kernels size their grids for the masked CU count. */
int lsdr_ctx_create_masked(int device, const uint32_t *cu_mask, unsigned mask_words, lsdr_ctx **ctx);
void lsdr_ctx_destroy(lsdr_ctx *ctx);
int lsdr_ctx_sync(lsdr_ctx *ctx);
void *lsdr_ctx_stream(lsdr_ctx *ctx);
int lsdr_device_count(void);
/* Device pipebuf storage (replaces `new T[size]` of pipebuf, framework.h:141-143). */
int lsdr_malloc(lsdr_ctx *ctx, size_t bytes, void **dev_ptr);
int lsdr_free(lsdr_ctx *ctx, void *dev_ptr);
int lsdr_malloc_host(size_t bytes, void **pinned_ptr);   /* pinned staging for file_reader/writer */
int lsdr_free_host(void *pinned_ptr);
/* ---- placed stream buffers (arena.hip) ----
 * WHERE a resident buffer lands in HBM decides how fast a streaming kernel reads it (the same fir_filter launch: 0.37 ms over one 2 GiB
 * buffer, 0.42 ms over the next, reproducibly per buffer; it goes with the physical backing, and the windows of ONE large allocation are of
 * the fast kind far more often than separate allocations).  An arena is one device allocation handed out in 2 MiB-aligned windows, the
 * FASTEST free ones first: replaces, for the large stream buffers of a graph, the `new T[size]` of pipebuf (framework.h:141-143) that has no
 * such concern on a CPU.
 *   lsdr_arena_place   the n_best fastest of up to max_windows free candidate windows of `bytes` (from the arena's start, or from its end
 *                      downwards with from_tail).  "Fastest" under `probe` — it queues, on the context's stream, the launch whose speed
 *                      matters over the candidate it is given; the library times 6 calls after 3 untimed ones with events — or, with a null
 *                      probe, under a built-in streaming read of the window.  fill_from (device pointer, may be null): every candidate is
 *                      first filled with `bytes` bytes from there (a probe that reads samples needs samples).  The search ends early once
 *                      the n-th best candidate is 8 % under the median of at least five.  out[n_best], ms[n_best] (may be null): the
 *                      windows and their probe times, fastest first.  The arena REMEMBERS every probed window (time relative to its call's
 *                      median): later calls try free positions inside stretches known to be fast first, never-probed ones next, known-slow
 *                      ones last (the slow kind comes in stretches of GiBs; small buffers fit into a fast large window that was not taken).
 *   lsdr_arena_probe_log  the probe time of every candidate the last lsdr_arena_place tried, in the order tried.
 *   lsdr_ctx_set_arena    from now on lsdr_malloc(ctx, ≥ 1 MiB) is served from the arena (built-in probe, ≤ 12 candidates; an ordinary
 *                      allocation once the arena is full) and lsdr_free gives such windows back: a graph built on the host framework
 *                      gets placed device pipes unchanged.  Null detaches.  The arena must outlive what was allocated from it.
 * One thread per arena, like every object of a context. */
typedef struct lsdr_arena lsdr_arena;
typedef int (*lsdr_probe_fn)(void *user, void *candidate_window);
int lsdr_arena_create(lsdr_ctx *ctx, size_t bytes, lsdr_arena **arena);   /* LSDR_E_NOMEM: no such piece of device memory */
void lsdr_arena_destroy(lsdr_arena *arena);
size_t lsdr_arena_bytes(const lsdr_arena *arena);
int lsdr_arena_owns(const lsdr_arena *arena, const void *dev_ptr);
int lsdr_arena_place(lsdr_arena *arena, size_t bytes, unsigned n_best, unsigned max_windows, int from_tail, const void *fill_from,
                     lsdr_probe_fn probe, void *user, void **out, float *ms);
int lsdr_arena_time(lsdr_arena *arena, void *dev_ptr, lsdr_probe_fn probe, void *user, float *ms);   /* the probe over any buffer, timed like a candidate */
int lsdr_arena_release(lsdr_arena *arena, void *window);
int lsdr_arena_probe_log(const lsdr_arena *arena, float *ms, unsigned cap, unsigned *n);
int lsdr_ctx_set_arena(lsdr_ctx *ctx, lsdr_arena *arena);
int lsdr_memcpy_h2d(lsdr_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes); /* async on ctx stream */
int lsdr_memcpy_d2h(lsdr_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes); /* async on ctx stream */
int lsdr_memcpy_d2d(lsdr_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);  /* pipebuf::pack() memmove, framework.h:153-159 (overlap-safe) */
int lsdr_memset(lsdr_ctx *ctx, void *dst_dev, int value, size_t bytes);
/* Copy engine of a context — what a pipebuf with ends on both sides of PCIe uses (host framework.h; replaces the plain
 * `new T[size]` + in-place access of framework.h:133-183 for the file_reader → first GPU block and last GPU block →
 * file_writer edges of leandvb.cc:205-256,593).  Two side streams, one per direction; `src_host`/`dst_host` should be
 * pinned (lsdr_malloc_host).
 *   lsdr_copy_h2d_async  upload on the upload stream; returns at once.
 *   lsdr_copy_fence      later work on the compute stream waits (on the GPU) for every upload enqueued so far.
 *   lsdr_copy_d2h_async  download on the download stream, ordered after everything already on the compute stream.
 *   lsdr_copy_sync_d2h   the host waits for the downloads.
 *   lsdr_copy_sync_all   the host waits for uploads, compute stream and downloads (pipe compaction). */
int lsdr_copy_h2d_async(lsdr_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int lsdr_copy_d2h_async(lsdr_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int lsdr_copy_fence(lsdr_ctx *ctx);
int lsdr_copy_sync_d2h(lsdr_ctx *ctx);
int lsdr_copy_sync_all(lsdr_ctx *ctx);
/* Stream timing for bench.py (HIP events recorded on the ctx stream). */
int lsdr_timer_start(lsdr_ctx *ctx);
int lsdr_timer_stop_ms(lsdr_ctx *ctx, float *ms); /* synchronises on the stop event */
/* Free-standing HIP events on the ctx stream (per-kernel timing inside a timed region). */
typedef struct lsdr_event lsdr_event;
int lsdr_event_create(lsdr_ctx *ctx, lsdr_event **ev);
void lsdr_event_destroy(lsdr_event *ev);
int lsdr_event_record(lsdr_event *ev);
int lsdr_event_elapsed_ms(lsdr_event *start, lsdr_event *stop, float *ms); /* synchronises on `stop` */
/* Make all later work on `ctx` wait for `ev` (recorded on another ctx's stream): the edge between
 * two blocks that run on different HIP streams (e.g. fir_filter of batch k+1 ‖ cstln_receiver of batch k). */
int lsdr_ctx_wait_event(lsdr_ctx *ctx, lsdr_event *ev);

/* ----------------------------------------------------- host-side table design
 * Replaces filtergen.h (coefficients are *inputs* to the kernels and must be
 * numerically identical to the reference's), math.h trig16 and the
 * cstln_lut<256> constructor.  Pure host code using the same libm. */
int lsdr_filtergen_lowpass(int order, float Fcut, float gain, float *coeffs_host);               /* filtergen.h:45-62; returns ncoeffs */
int lsdr_filtergen_root_raised_cosine(int order, float Fs, float rolloff, float *coeffs_host);   /* filtergen.h:68-92; returns ncoeffs */
void lsdr_filtergen_normalize_dcgain(int n, float *coeffs_host, float gain);                      /* filtergen.h:34-40 */
void lsdr_filtergen_normalize_power(int n, float *coeffs_host, float gain);                       /* filtergen.h:26-32 */
void lsdr_trig16_table(lsdr_cf32 *lut_host /*[65536]*/);                                         /* math.h:95-106 */
enum { LSDR_BPSK, LSDR_QPSK, LSDR_PSK8, LSDR_APSK16, LSDR_APSK32, LSDR_APSK64E,
       LSDR_QAM16, LSDR_QAM64, LSDR_QAM256 };                                                    /* sdr.h:318-324 */
enum { LSDR_FEC12, LSDR_FEC23, LSDR_FEC46, LSDR_FEC34, LSDR_FEC56, LSDR_FEC78,
       LSDR_FEC45, LSDR_FEC89, LSDR_FEC910 };                                                    /* dvb.h:37-41 */
/* make_dvbs2_constellation (dvb.h:45-81) + cstln_lut<256> ctor (sdr.h:326-560).
 * Arrays are indexed [(u8)I*256 + (u8)Q]; symbols is [nsymbols][2] (re,im). */
int lsdr_cstln_lut_build(int predef, int fec, int16_t *cost_host, uint8_t *symbol_host,
                         int16_t *phase_error_host, int8_t *symbols_host, int *nrotations); /* returns nsymbols */

/* ------------------------------------------------------ elementwise blocks */
/* cconverter<u8,128,f32,0,1,1>::run, dsp.h:40-50 */
int lsdr_cconverter_u8_run(lsdr_ctx *ctx, const lsdr_cu8 *in, size_t n, lsdr_cf32 *out);
/* cconverter<s8,0,f32,0,1,1>, <u16,32768,f32,0,1,1>, <s16,0,f32,0,1,1>::run (dsp.h:40-50; leandvb --s8 / --u16 / --s16,
 * leandvb.cc:218-248): `in` is n complex items of the given integer format. */
enum { LSDR_IN_CS8 = 2, LSDR_IN_CU16 = 3, LSDR_IN_CS16 = 4 };   /* (LSDR_IN_CF32 = 0, LSDR_IN_CU8 = 1: fir_filter's fused formats) */
int lsdr_cconverter_int_run(lsdr_ctx *ctx, int in_format, const void *in, size_t n, lsdr_cf32 *out);
/* scaler<float,cf32,cf32>::run, dsp.h:149-156 */
int lsdr_scaler_run(lsdr_ctx *ctx, float scale, const lsdr_cf32 *in, size_t n, lsdr_cf32 *out);
/* decimator<cf32>::run, generic.h:256-262; *produced = min(n/d, cap), consumes produced*d */
int lsdr_decimator_run(lsdr_ctx *ctx, unsigned d, const lsdr_cf32 *in, size_t n, lsdr_cf32 *out,
                       size_t cap, size_t *produced);
/* rotator<f32> (sdr.h:1226-1259): out[i] = in[i]·(cos, sin)(2π·i·ifreq/65536), ifreq = (int)(freq·65536); the 16-bit table
 * index is carried across calls.  The table is built on the host with libm like the reference's constructor. */
typedef struct lsdr_rotator lsdr_rotator;
int lsdr_rotator_create(lsdr_ctx *ctx, float freq, lsdr_rotator **r);
void lsdr_rotator_destroy(lsdr_rotator *r);
int lsdr_rotator_run(lsdr_rotator *r, const lsdr_cf32 *in, size_t n, lsdr_cf32 *out);

/* -------------------------------------------------------------- auto_notch / cnr_fft / cfft
 * auto_notch<f32>, sdr.h:46-154: every `decimation` samples the `nslots` strongest bins of a 4096-point
 * spectrum are re-detected; every sample is cleaned by one first-order complex tracker per slot.
 * The per-sample recurrence runs on the GPU (time tiles with warm-up; every seam is verified bit for
 * bit against the previous tile's end state, unverified spans are redone sequentially → bit-exact);
 * detect() is a once-per-millions-of-samples control step: the block is fetched to the host and the
 * reference's FFT / hypotf / cosf / sinf sequence is evaluated there (exact libm). */
typedef struct lsdr_auto_notch lsdr_auto_notch;
int lsdr_auto_notch_create(lsdr_ctx *ctx, int nslots, float agc_rms_setpoint, lsdr_auto_notch **a);
void lsdr_auto_notch_destroy(lsdr_auto_notch *a);
int lsdr_auto_notch_set(lsdr_auto_notch *a, int decimation, float k);      /* public members, sdr.h:49-50 */
int lsdr_auto_notch_slot_bin(const lsdr_auto_notch *a, int slot);
/* LSDR_NOTCH_EXACT (default): the reference's sequential arithmetic in verified time tiles — bit-exact.
 * LSDR_NOTCH_SCAN: throughput mode — the estimator recurrence as a single-pass scan (one wavefront per 1024 samples,
 * decoupled look-back for the carry), detect() entirely on the device, no host synchronisation per run; tolerance-tested
 * (tests/test_gpu_notch.py), needs 1-4 slots and agc_rms_setpoint == 0 (leandvb's configuration, leandvb.cc:300-301). */
enum { LSDR_NOTCH_EXACT = 0, LSDR_NOTCH_SCAN = 1 };
int lsdr_auto_notch_set_mode(lsdr_auto_notch *a, int mode);
int lsdr_auto_notch_stats(const lsdr_auto_notch *a, unsigned *tiles, unsigned *bad_seams);
/* Measurement hook (bench_more.py's roofline of the scan kernel): HIP events on the block's stream around the k_notch_scan
 * launch of every LSDR_NOTCH_SCAN run while enabled.  Each call returns the mean over the (up to 16 most recent) launches
 * recorded since the previous call — after waiting for the stream — and then sets the switch. */
/* LSDR_NOTCH_SCAN, opt-in: a run's detect chain (FFTs of the detect points of its INPUT -> peaks -> phasor tables) on a side stream,
 * overlapping the previous run's scan kernel.  The caller promises that an input buffer is complete when lsdr_auto_notch_run is
 * called with it (the side stream does not wait for earlier work queued on the context).  Same results. */
int lsdr_auto_notch_set_overlap(lsdr_auto_notch *n, int on);
/* LSDR_NOTCH_SCAN's cross-workgroup look-back spins are bounded: *aborted_run = 0 while all were served, else the number of the
 * first run in which one gave up (the next lsdr_auto_notch_run then fails instead of continuing from garbage) */
int lsdr_auto_notch_check(lsdr_auto_notch *n, unsigned *aborted_run);
#ifdef LSDR_MEASURE
/* Measurement build only (make -C leansdr_amd/csrc measure; NOT in liblsdr_hip.so): garbage into the scan mode's hand-off buffers
 * (totals and flags); a correct hand-off never reads it (tools/notch_poison_stress.py) */
int lsdr_auto_notch_debug_poison(lsdr_auto_notch *n);
#endif
int lsdr_auto_notch_scan_time(lsdr_auto_notch *a, int enable, float *avg_ms, unsigned *launches);
/* run(), sdr.h:64-75: whole 4096-sample blocks; *consumed == *produced.  Synchronous. */
int lsdr_auto_notch_run(lsdr_auto_notch *a, const lsdr_cf32 *in, size_t n_in, lsdr_cf32 *out, size_t cap_out,
                        size_t *consumed, size_t *produced);

/* ---- notch_fir: auto_notch (one slot) FUSED into fir_filter — leandvb's default graph (`--anf 1`, leandvb.cc:103,296-301:
 * auto_notch<f32>(…, 1, 0) feeding fir_filter<cf32,float>) without the notched stream ever existing.  The notch of sdr.h:119-138 is, per
 * detect interval, the LTI filter (1 − k − p·z⁻¹)/(1 − p·z⁻¹), p = (1−k)·exp(j2π·bin/4096); composed with the decimating FIR it is ONE
 * complex-tap decimating FIR over the raw samples (matrix pipe, 8 B per sample) plus a first-order recurrence at the decimated rate;
 * detect() (FFT of the detect block, first maximum, sdr.h:76-118) runs on the device; outputs around a bin CHANGE are computed directly.
 * TOLERANCE MODE (float32 with exact phases, not the reference's rounding sequence): same bins as the reference; every output within
 * 2e-5 of the stream's full scale of fir_filter(auto_notch(x)) in the reference's arithmetic for bins below 2048 and within 1e-3 for
 * bins 2048…4095 (measured up to 3.8e-4), and within 1e-5 of the float64 restatement of the same filter for EVERY bin — the bounds
 * tests/test_gpu_notch_fir.py asserts.  (The larger figure is the reference's own doing: its phasor table is cosf/sinf of an angle
 * ROUNDED TO FLOAT, 2π·bin·i/4096 up to 25 736 rad for the negative-frequency bins, i.e. ±1e-3 rad of table noise that an exact-phase
 * formulation does not reproduce.)
 * Exists for nslots == 1, decim == 30, ncoeffs ≤ 330, cf32 input, agc set point 0; anything else: LSDR_E_UNSUPPORTED at create —
 * use the two blocks.  `in` is the RAW stream at fir_filter's read position (the block keeps the 32 samples in front of it).
 * One run = auto_notch::run over the whole 4096-sample blocks present, then fir_filter::run over what the notch released:
 * *produced = (A − F − ncoeffs)/decim with A the notch's frontier (a multiple of 4096 of the stream), *consumed = *produced·decim.
 * Queued on the context's stream.  cap_out must hold at least 150 outputs for the block to make progress. */
typedef struct lsdr_notch_fir lsdr_notch_fir;
typedef struct {
  unsigned ncoeffs; const float *coeffs_host;   /* fir_filter's prototype taps (dsp.h:221-231) */
  unsigned decim;
  float in_scale;                               /* a fused scaler in front (0 or 1: none); rides on the taps */
  int nslots;                                   /* auto_notch's slots: 1 */
  int notch_decimation;                         /* auto_notch::decimation (0: 1024·4096, sdr.h:56) */
  float k;                                      /* auto_notch::k (0: 0.002) */
} lsdr_notch_fir_cfg;
int lsdr_notch_fir_create(lsdr_ctx *ctx, const lsdr_notch_fir_cfg *cfg, lsdr_notch_fir **h);
void lsdr_notch_fir_destroy(lsdr_notch_fir *h);
int lsdr_notch_fir_set(lsdr_notch_fir *h, int decimation, float k);
/* fir_filter's carrier tracking (dsp.h:236-244,271-280) on the fused block: the taps are re-shifted (host libm, as lsdr_fir_filter_set_freq)
 * and take effect with the next run; the decimated-rate recurrence is re-anchored under the new taps. */
int lsdr_notch_fir_set_freq(lsdr_notch_fir *h, float freq);
int lsdr_notch_fir_track(lsdr_notch_fir *h, float freq_tap, float tap_multiplier, float freq_tol, int *shifted);
float lsdr_notch_fir_current_freq(const lsdr_notch_fir *h);
int lsdr_notch_fir_run(lsdr_notch_fir *h, const lsdr_cf32 *in, size_t n_in, lsdr_cf32 *out, size_t cap_out, size_t *consumed, size_t *produced);
int lsdr_notch_fir_slot_bin(lsdr_notch_fir *h);   /* waits for the stream; −1: nothing detected yet */
/* Opt-in: run k+1's detect chain and filter pass on ONE stream of the block's own, next to run k's tail (first output, fix-ups, recurrence,
 * state) on the context's stream; the output is complete in the order of the context's stream, as always.  The own stream does NOT wait
 * for earlier work queued on the context: the caller promises that an input buffer is complete when lsdr_notch_fir_run is called with
 * it and stays untouched until that run has completed on the context's stream.  Same results, bit for bit. */
int lsdr_notch_fir_set_overlap(lsdr_notch_fir *h, int on);
/* measurement hook: HIP events around the filter pass of every run while enabled (as lsdr_auto_notch_scan_time) */
int lsdr_notch_fir_time(lsdr_notch_fir *h, int enable, float *avg_ms, unsigned *launches);
/* cfft_engine<float>::inplace (dsp.h:56-116).  lsdr_cfft_run: the transform of one device block on the GPU (one workgroup,
 * in LDS, bit-identical butterflies) with the spectrum delivered to the host — what auto_notch::detect, cnr_fft and spectrum
 * use.  lsdr_cfft_host: the same arithmetic on host data (utility / cross-check). */
int lsdr_cfft_run(lsdr_ctx *ctx, int n, int reverse, const lsdr_cf32 *in_dev, lsdr_cf32 *out_host);
int lsdr_cfft_host(int n, lsdr_cf32 *data, int reverse);
/* cnr_fft<f32>, sdr.h:1273-1345: consumes whole nfft blocks; every `decimation` samples one block is
 * fetched and a CNR value (dB) is appended to cnr_out_host.  Synchronous only when a block is fetched. */
typedef struct lsdr_cnr_fft lsdr_cnr_fft;
int lsdr_cnr_fft_create(lsdr_ctx *ctx, float bandwidth, int nfft, lsdr_cnr_fft **c);
void lsdr_cnr_fft_destroy(lsdr_cnr_fft *c);
int lsdr_cnr_fft_set(lsdr_cnr_fft *c, int decimation, float kavg);         /* public members, sdr.h:1287-1288 */
int lsdr_cnr_fft_run(lsdr_cnr_fft *c, float freq_tap, float tap_multiplier, const lsdr_cf32 *in, size_t n_in,
                     float *cnr_out_host, size_t cap_out, size_t *consumed, size_t *produced);

/* spectrum<f32>, sdr.h:1347-1404 (nfft = 1024): consumes whole 1024-sample blocks; every `decimation` samples one
 * block is fetched, FFT'd on the host (cfft_engine), averaged (kavg) and written as one row of 1024 dB values,
 * fftshifted, to spectrum_out_host[cap_rows][1024].  Replaces spectrum::run / do_spectrum (sdr.h:1361-1396). */
typedef struct lsdr_spectrum lsdr_spectrum;
int lsdr_spectrum_create(lsdr_ctx *ctx, lsdr_spectrum **s);
void lsdr_spectrum_destroy(lsdr_spectrum *s);
int lsdr_spectrum_set(lsdr_spectrum *s, int decimation, float kavg);      /* public members, sdr.h:1358-1359 */
int lsdr_spectrum_run(lsdr_spectrum *s, const lsdr_cf32 *in, size_t n_in, float *spectrum_out_host, size_t cap_rows,
                      size_t *consumed, size_t *produced_rows);

/* -------------------------------------------------------------- fir_filter
 * fir_filter<cf32,float>, dsp.h:219-285 (decimating FIR, real prototype taps
 * frequency-shifted to complex).  The optional input stage fuses the block in
 * front of it in the leandvb graph so that its output never round-trips
 * through HBM: cconverter (u8 input, leandvb.cc:215) or scaler (f32 input,
 * leandvb.cc:255-256); results are bit-identical to running the two blocks
 * separately. */
enum { LSDR_IN_CF32 = 0, LSDR_IN_CU8 = 1 };
enum {
  LSDR_FIR_EXACT = 0, /* reference arithmetic: i-ascending accumulation, no FMA contraction → bit-exact */
  LSDR_FIR_FMA = 1,   /* same order, fused multiply-add (≤ 1 ulp/tap differences; tolerance-tested) */
  LSDR_FIR_MFMA = 2,  /* LSDR_FIR_FMA's arithmetic, bit for bit, on the f32 matrix pipe (v_mfma_f32_16x16x4_f32 is an exact
                       * k-ordered fmaf chain): the taps as a banded Toeplitz block, sixteen outputs per row group.  cf32 input
                       * at the decimations with a compile-time kernel; anything else runs LSDR_FIR_FMA's kernels (same bits). */
  LSDR_FIR_MFMA_BLK = 3 /* block-polyphase form on the matrix pipe (a dense product): the taps in blocks of `decim`, each block an
                       * fmaf chain from zero in tap order (complex taps, set_freq != 0: four taps at a time — their re-part products, then
                       * their im-part products), the block sums added in block order, in_scale multiplied into the taps (one
                       * rounding per tap) instead of the samples — its own stated arithmetic (oracle lo_fir_filter_blk), same
                       * error bound as LSDR_FIR_FMA.  cf32 input, every decimation 1 … 64 (whatever
                       * Fs / (4·Fm) leandvb.cc:353-378 computes), ncoeffs ≤ 16·decim; refused (LSDR_E_ARG) otherwise. */
};
typedef struct {
  unsigned ncoeffs;          /* fir_filter ctor _ncoeffs */
  const float *coeffs_host;  /* fir_filter ctor _coeffs (host) */
  unsigned decim;            /* fir_filter ctor _decim */
  int in_format;             /* LSDR_IN_* */
  float in_scale;            /* 0 = no fused scaler; else samples are multiplied by it first */
  int arith;                 /* LSDR_FIR_* */
} lsdr_fir_filter_cfg;
typedef struct lsdr_fir_filter lsdr_fir_filter;
/* Precondition of the matrix-pipe arithmetics (LSDR_FIR_MFMA, LSDR_FIR_MFMA_BLK): FINITE input samples.  Their K padding and the zero band of
 * the Toeplitz form multiply padding taps of 0.0 with real samples (fma(0, x, acc) = acc needs a finite x): one Inf or NaN sample reaches up to
 * 15·decim more outputs than in LSDR_FIR_EXACT / LSDR_FIR_FMA, where it stays inside its own tap window.  The same holds for what lies up to
 * 4 GiB behind the first tile of a stream longer than 4 GiB (read through a clamped buffer resource instead of zeros: finite, hence harmless). */
int lsdr_fir_filter_create(lsdr_ctx *ctx, const lsdr_fir_filter_cfg *cfg, lsdr_fir_filter **f);
void lsdr_fir_filter_destroy(lsdr_fir_filter *f);
/* set_freq(f), dsp.h:271-280 (host libm cosf/sinf, then upload). */
int lsdr_fir_filter_set_freq(lsdr_fir_filter *f, float freq);
/* The freq_tap prologue of run(), dsp.h:236-244: new=tap*mult; if |current-new|>tol → set_freq(new).
 * *shifted (may be NULL) reports whether a re-shift happened. */
int lsdr_fir_filter_track(lsdr_fir_filter *f, float freq_tap, float tap_multiplier, float freq_tol, int *shifted);
float lsdr_fir_filter_current_freq(const lsdr_fir_filter *f);
int lsdr_fir_filter_get_shifted_coeffs(const lsdr_fir_filter *f, lsdr_cf32 *shifted_host);
/* run() body, dsp.h:233-262.  in: n_in items of in_format.  Needs n_in >= ncoeffs;
 * *produced = min((n_in-ncoeffs)/decim, cap_out); *consumed = *produced*decim.
 * Output m = Σ_i sc[i]·in[ncoeffs + m·decim − i].  Asynchronous on the ctx stream. */
int lsdr_fir_filter_run(lsdr_fir_filter *f, const void *in, size_t n_in, lsdr_cf32 *out, size_t cap_out,
                        size_t *consumed, size_t *produced);
/* The same filter over n_streams (≤ 8) equal-length, independent buffers in ONE launch (no reference counterpart: the
 * reference has one fir_filter object per stream; this is the batched form of n_streams identical run() calls — same
 * consumed/produced for each, one prologue and one tail of the persistent kernel instead of n_streams). */
int lsdr_fir_filter_run_multi(lsdr_fir_filter *f, unsigned n_streams, const void *const *ins, size_t n_in,
                              lsdr_cf32 *const *outs, size_t cap_out, size_t *consumed, size_t *produced);

/* ---------------------------------------------------------- cstln_receiver
 * cstln_receiver<f32> + sampler_interface<f32>, sdr.h:589-938. */
enum { LSDR_SAMP_NEAREST = 0, LSDR_SAMP_LINEAR = 1, LSDR_SAMP_FIR = 2 }; /* sdr.h:600-689 */
enum { LSDR_SYM_SOFT = 0, LSDR_SYM_HARD2 = 1 };
enum {
  LSDR_RX_SERIAL = 0, /* one sequential pass, the reference's exact arithmetic → bit-exact soft symbols */
  LSDR_RX_TILED = 1   /* time-tiled with warm-up overlap (throughput mode; tolerance-tested).  The tolerance (leansdr_amd/tolerance.py)
                       * is stated and tested for BPSK, QPSK and 8PSK.  For 16-ary and denser constellations a tile's re-acquisition
                       * from phase = 0 is not reliable even with the reference's own arithmetic (restated with the serial oracle,
                       * 1024-sample tiles after 1024 of warm-up at 26 dB: 99.45 % of the serial decisions for 16QAM 3/4, 92.4 % for
                       * 16APSK 3/4; profiles/rx_tiled_constellations/emulation.txt): use LSDR_RX_SERIAL for those.  Nothing is refused. */
};
typedef struct {
  int sampler;               /* LSDR_SAMP_* */
  int ncoeffs;               /* fir_sampler(_ncoeffs,_coeffs,_subsampling), sdr.h:637-643 */
  const float *coeffs_host;
  int subsampling;
  int cstln, fec;            /* demod.cstln = make_dvbs2_constellation(cstln, fec), leandvb.cc:476 */
  int harden;                /* cstln->harden(), leandvb.cc:477-481 */
  float omega;               /* set_omega(Fs/Fm), leandvb.cc:482 */
  float freq;                /* set_freq(Ftune/Fs), leandvb.cc:483-487 (0: untouched) */
  float pll_adjustment;      /* public member; /=6 with --viterbi, leandvb.cc:498-501 */
  int allow_drift;           /* set_allow_drift() */
  unsigned long meas_decimation; /* public member, leandvb.cc:502 */
  float kest;                /* public member, default 0.01 */
  int mode;                  /* LSDR_RX_* */
  unsigned tile_len;         /* LSDR_RX_TILED: samples per tile (multiple of 128); 0 = default (twice the warm-up) */
  unsigned tile_warmup;      /* LSDR_RX_TILED: warm-up samples before each tile (multiple of 128); 0 = default (≈ 64 symbols) */
  int in_format;             /* LSDR_IN_CF32 (0, the reference's block) or LSDR_IN_CU8: the cconverter<u8,128,f32,0,1,1> in front
                              * of the receiver in the `leandvb --u8` graph (leandvb.cc:211-217, dsp.h:40-50) fused into the
                              * receiver's loads — `in` then points to lsdr_cu8 items and the converted cf32 stream never exists
                              * in HBM; results are bit-identical to running the two blocks separately */
  int out_format;            /* LSDR_SYM_SOFT (0): lsdr_softsymbol items.  LSDR_SYM_HARD2: LSDR_RX_TILED on QPSK only — the decisions
                              * alone, packed 16 per uint32 word, MSB first (symbol k of a run in word k/16, bits 31-2(k%16)..30-2(k%16)):
                              * what deconvol_sync, the next block of the default leandvb chain, reads of a softsymbol (`symbol & 3`,
                              * dvb.h:369-417); `out` then points to uint32 words and counts stay in symbols.  Needs cu8 input and the
                              * nearest or linear sampler. */
} lsdr_rx_cfg;
typedef struct {             /* the receiver's loop state, sdr.h:923-935 */
  float mu, phase, freqw, agc_gain, est_insp, est_sp, est_ep, freq_tap;
  float min_freqw, max_freqw;
  unsigned long meas_count;
  float hist[12];            /* hist[k] = {p.re,p.im,c.re,c.im}, k = 0..2 */
} lsdr_rx_state;
typedef struct lsdr_rx lsdr_rx;
int lsdr_rx_create(lsdr_ctx *ctx, const lsdr_rx_cfg *cfg, lsdr_rx **r);
void lsdr_rx_destroy(lsdr_rx *r);
int lsdr_rx_readahead(const lsdr_rx *r);                 /* sampler->readahead() */
int lsdr_rx_get_state(lsdr_rx *r, lsdr_rx_state *st);    /* includes freq_tap (sdr.h:918-921) */
int lsdr_rx_set_state(lsdr_rx *r, const lsdr_rx_state *st);
/* Back to the loop state lsdr_rx_create left (= a freshly constructed cstln_receiver, sdr.h:709-736 + leandvb.cc:476-487): the next
 * run starts a new capture.  Stream-ordered, no host wait; no queued runs may be outstanding. */
int lsdr_rx_reset(lsdr_rx *r);
/* LSDR_RX_TILED diagnostics of the last run: tiles, seams where a duplicated / lost symbol was
 * repaired, seams whose timing or carrier-phase mismatch exceeded the lock criterion. */
int lsdr_rx_tiled_stats(const lsdr_rx *r, unsigned *tiles, unsigned *dup, unsigned *miss, unsigned *bad_seams);
/* run(), sdr.h:772-916, over one buffer: consumes whole chunks of 128 samples while
 * n_in-pos >= 128+readahead and cap_out-produced >= 128 (and the measurement
 * outputs have room).  freq/ss/mer (meas_cap floats each, HOST pointers, may be
 * NULL) receive one value per meas_decimation samples; cstln_out_host (may be
 * NULL) one cf32 per chunk that produced a symbol.  Synchronous. */
int lsdr_rx_run(lsdr_rx *r, const void *in /* n_in items of cfg.in_format */, size_t n_in, lsdr_softsymbol *out, size_t cap_out,
                size_t *consumed, size_t *produced,
                float *freq_out_host, float *ss_out_host, float *mer_out_host, size_t meas_cap, size_t *n_meas,
                lsdr_cf32 *cstln_out_host, size_t cstln_cap, size_t *n_cstln);
/* Queued variant of lsdr_rx_run for LSDR_RX_TILED (no measurement outputs): puts the run on the context's stream and
 * returns at once with `consumed` (a pure function of the sizes); lsdr_rx_wait() retires the oldest queued run and
 * yields its symbol count.  Up to 8 runs may be queued; the loop state is carried on the device from run to run, so
 * the host never sits between two runs.  lsdr_rx_run / _set_state refuse to mix with outstanding queued runs. */
int lsdr_rx_run_async(lsdr_rx *rx, const void *in, size_t n_in, lsdr_softsymbol *out, size_t cap_out, size_t *consumed);
int lsdr_rx_wait(lsdr_rx *rx, size_t *produced);
/* lsdr_rx_run_async for n_rx independent captures at once (one receiver per capture — the reference has one cstln_receiver
 * object per stream, sdr.h:697-938, leandvb.cc:163): equally long inputs ins[i] → outs[i]; `consumed` is an ARRAY of n_rx
 * entries, consumed[i] = the samples receiver i takes (they differ only when the receivers are configured differently).  Every
 * run is planned before anything is queued: on an argument error no receiver has been queued.  Receivers
 * on ONE context with the same configuration share their launches (four per batch instead of four per capture); any other
 * combination is queued receiver by receiver.  Same results as n_rx separate lsdr_rx_run_async calls, bit for bit; each
 * receiver is retired with its own lsdr_rx_wait. */
int lsdr_rx_run_multi_async(lsdr_rx *const *rxs, unsigned n_rx, const void *const *ins, size_t n_in, lsdr_softsymbol *const *outs,
                            size_t cap_out, size_t *consumed);
/* The queued run of a LSDR_SYM_HARD2 receiver, writing its packed symbols from symbol position out_sym_offset of the stream
 * that starts at out_words[0] (symbols before it — a caller's unconsumed remainder of the previous run — are preserved, so
 * consecutive runs form one packed stream without a bit-shifting copy).  cap_out counts symbols after the offset. */
int lsdr_rx_run_async_hs2(lsdr_rx *rx, const void *in, size_t n_in, uint32_t *out_words, size_t out_sym_offset, size_t cap_out,
                          size_t *consumed);
/* freq_tap (sdr.h:919-921, cycles per sample) as of the end of the most recently retired queued run: lets the caller keep
 * fir_filter tracking the carrier (lsdr_fir_filter_track, dsp.h:236-244) from runs that have already completed while later
 * ones are still queued — the feedback of leandvb.cc:506-510 with a latency of the queue depth instead of a host wait. */
float lsdr_rx_retired_freq_tap(const lsdr_rx *rx);
/* Measurement hook (bench.py's roofline of the tile kernel): HIP events on the receiver's stream around the k_rx_tiles launch of
 * every queued run while enabled; each call returns the mean over the runs retired since the previous call, then sets the switch. */
int lsdr_rx_tile_time(lsdr_rx *rx, int enable, float *avg_ms, unsigned *launches);
/* Loop-state snapshot between queued runs: lsdr_rx_snapshot_async() puts a copy of the device-side loop state (the fields
 * of cstln_receiver<f32>, sdr.h:923-935) into a pinned slot in stream order, i.e. the state the NEXT queued run starts
 * from; lsdr_rx_get_snapshot() waits for the stream and returns it.  Lets a caller (bench.py's verification) replay one
 * queued run on a checker from exactly the state the device used, without putting the host between two runs.  Four slots
 * (`_slot` forms; the plain forms use slot 0), so that a batch in the middle of a long queue and the last one can both be kept. */
/* Exact receiver, one GPU LANE per independent capture: n_streams captures with the same parameters (BASELINE config 4's
 * shape), each with its own loop state, every lane running cstln_receiver<f32>::run's exact arithmetic (sdr.h:772-916) →
 * bit-exact soft symbols and state per capture, 64 captures per wavefront.  `in_dev` / `out_dev` are HOST arrays of
 * n_streams DEVICE pointers; every capture gets n_in samples and cap_out symbol slots; all consume the same *consumed. */
typedef struct lsdr_rx_batch lsdr_rx_batch;
int lsdr_rx_batch_create(lsdr_ctx *ctx, const lsdr_rx_cfg *cfg, unsigned n_streams, lsdr_rx_batch **b);
void lsdr_rx_batch_destroy(lsdr_rx_batch *b);
int lsdr_rx_batch_run(lsdr_rx_batch *b, const void *const *in_dev, size_t n_in, lsdr_softsymbol *const *out_dev, size_t cap_out,
                      size_t *consumed, size_t *produced /*[n_streams]*/);
int lsdr_rx_batch_get_state(lsdr_rx_batch *b, unsigned stream, lsdr_rx_state *st);
/* LSDR_RX_TILED, QPSK: whether the tolerance tiles take their decisions by arithmetic instead of the constellation-table
 * gather (only when lsdr_rx_create verified the arithmetic against all 65536 table entries: symbol/cost/point identical,
 * |phase_error difference| ≤ 2 table units — reported in *max_phase_error_delta). */
int lsdr_rx_decision_mode(const lsdr_rx *rx, int *arithmetic, unsigned *max_phase_error_delta);
int lsdr_rx_snapshot_async(lsdr_rx *rx);
int lsdr_rx_get_snapshot(lsdr_rx *rx, lsdr_rx_state *st);
int lsdr_rx_snapshot_async_slot(lsdr_rx *rx, unsigned slot);
int lsdr_rx_get_snapshot_slot(lsdr_rx *rx, unsigned slot, lsdr_rx_state *st);

/* ================================================================== DVB-S FEC tail
 * Item layouts: bytes are u8; RS packets 204 B (rspacket<u8>), TS packets 188 B (tspacket). */

/* ---- deconvol_sync<u8,0> via make_deconvol_sync_simple, dvb.h:122-513 (algebraic deconvolution).
 * `rate` is LSDR_FEC12/23/46/34/56/78.  fastlock (dvb.h:428-454) is not implemented on the device:
 * create fails with LSDR_E_UNSUPPORTED when requested. */
typedef struct lsdr_deconv lsdr_deconv;
int lsdr_deconv_create(lsdr_ctx *ctx, int rate, int fastlock, lsdr_deconv **d);
void lsdr_deconv_destroy(lsdr_deconv *d);
int lsdr_deconv_next_sync(lsdr_deconv *d);                       /* deconvol_sync::next_sync, dvb.h:185-193 */
int lsdr_deconv_reset(lsdr_deconv *d);                           /* the state of a freshly constructed block (a new stream begins); stream-ordered */
/* One run() call (run_decoding, dvb.h:419-470): skips `skip` symbols, needs >= 64 symbols of margin,
 * produces n = min(maxrd, cap_out) bytes when n >= 32.  Asynchronous (sizes are data-independent). */
int lsdr_deconv_run(lsdr_deconv *d, const lsdr_softsymbol *in, size_t n_in, uint8_t *out, size_t cap_out,
                    size_t *consumed, size_t *produced);

/* The same block on the packed hard symbols of a LSDR_SYM_HARD2 receiver (deconvol_sync reads `symbol & 3` only, dvb.h:373,396):
 * symbols [sym_offset, sym_offset + n_in) of the packed stream that starts at in_words[0]; same arithmetic, same outputs as
 * lsdr_deconv_run on the unpacked symbols.  No fastlock. */
int lsdr_deconv_run_hs2(lsdr_deconv *d, const uint32_t *in_words, size_t sym_offset, size_t n_in, uint8_t *out, size_t cap_out,
                        size_t *consumed, size_t *produced);

/* ---- viterbi_sync, dvb.h:1173-1416 (+ viterbi_dec / trellis / bitpath, viterbi.h).  Soft-decision Viterbi
 * with the reference's partial-metric update and its alignment search (conjugation x rotation x shift).
 * One run() call: all 128-block chunks that fit.  Bit-exact: the stream is decoded in tiles that start
 * from zero metrics a few chunks early; every seam is verified against the previous tile's end state
 * (all 64 path metrics and path registers) and anything unverified is re-decoded sequentially.
 * Synchronous. */
typedef struct lsdr_viterbi lsdr_viterbi;
int lsdr_viterbi_create(lsdr_ctx *ctx, int cstln, int rate, lsdr_viterbi **v);
void lsdr_viterbi_destroy(lsdr_viterbi *v);
int lsdr_viterbi_set_resync_period(lsdr_viterbi *v, int period);   /* public member resync_period (dvb.h:1232) */
int lsdr_viterbi_current_sync(const lsdr_viterbi *v);
/* diagnostics of the last run: tiles decoded, seams that failed verification (re-decoded serially) */
int lsdr_viterbi_stats(const lsdr_viterbi *v, unsigned *tiles, unsigned *bad_seams);
/* since create: seams re-decoded by the repair round that runs on the device behind the main launch (no host round trip), and the
 * launch -> readback rounds the host still had to add (a repaired tile whose end state changed fails the NEXT seam; anything that
 * does not settle is re-decoded sequentially: the output is exact either way) */
int lsdr_viterbi_repair_stats(const lsdr_viterbi *v, unsigned long long *device_repaired, unsigned long long *host_rounds);
/* host only (no GPU, no context): 1 if the trellis of (constellation, code rate) — built as trellis::init_convolutional does,
 * viterbi.h:59-92 — has the structure the four-lanes-per-tile kernel relies on (long inputs of QPSK 1/2 and 8PSK 2/3 then
 * use it; same bytes as every other kernel), 0 if not, -1 if viterbi_sync does not support the combination (dvb.h:1234-1331). */
int lsdr_viterbi_q4_supported(int cstln, int rate);
int lsdr_viterbi_run(lsdr_viterbi *v, const lsdr_softsymbol *in, size_t n_in, uint8_t *out, size_t cap_out,
                     size_t *consumed, size_t *produced);

/* ---- viterbi_sync for many streams at once: n_streams independent decoders (each one a viterbi_sync of its own, dvb.h:1173-1416)
 * behind one object.  Every stream's tiles ride in the same launches; seam repair, the alignment decision (dvb.h:1402-1411) and
 * every count stay on the device, and the host does nothing between run_async and wait (no synchronise, no readback, no launch that
 * depends on data).  The number of launches of a run does not depend on n_streams.
 * One call commits, per stream, a PREFIX of the stream's input: a whole number of 128-block chunks (dvb.h:1372-1373 decides how many
 * fit into n_in and cap_out), for which the bytes written and the decoder state afterwards are the reference's.  The prefix is shorter
 * than what fits only behind a resync chunk whose decision changed the alignment (`switched`: the rest belongs to the new alignment)
 * or in front of a seam that still failed verification after the device's repair rounds (`stalled`).  A stream with at least one chunk
 * available always commits at least one: continue with in + consumed, out + produced until consumed is 0.  The bytes do not depend on
 * how a stream is cut into calls, nor on what the other streams of the batch hold. */
typedef struct lsdr_viterbi_batch lsdr_viterbi_batch;
typedef struct {
  uint64_t consumed;        /* soft symbols of this call's input that are now decoded (whole chunks) */
  uint64_t produced;        /* bytes written to the stream's out pointer */
  uint32_t current_sync;    /* alignment in force after the call */
  uint32_t resync_phase;
  uint32_t switched;        /* 1: the prefix ends behind a resync chunk that changed the alignment (dvb.h:1402-1411) */
  uint32_t stalled;         /* 1: the prefix ends in front of a seam that did not verify after the device's repair rounds */
  uint32_t tiles, repaired; /* tiles planned for the stream; tiles the device decoded again */
} lsdr_viterbi_batch_result;
/* max_symbols: the most symbols one stream hands to one run (sizes the per-resync-chunk records).  Errors as lsdr_viterbi_create. */
int lsdr_viterbi_batch_create(lsdr_ctx *ctx, int cstln, int rate, int n_streams, size_t max_symbols, lsdr_viterbi_batch **vb);
void lsdr_viterbi_batch_destroy(lsdr_viterbi_batch *vb);
int lsdr_viterbi_batch_set_resync_period(lsdr_viterbi_batch *vb, int period);   /* all streams; not while a run is in flight */
/* stream i (all streams if i < 0) becomes a freshly constructed viterbi_sync; ordered on the context's stream; not while a run is in flight */
int lsdr_viterbi_batch_reset(lsdr_viterbi_batch *vb, int i);
/* in_dev / out_dev: HOST arrays of n_streams DEVICE pointers (out 4-byte aligned, else LSDR_E_ARG; in may be NULL where n_in is 0).
 * n_in: HOST array, symbols available per stream (<= max_symbols).  n_in_dev: NULL, or a DEVICE array of n_streams uint64 counts written
 * by earlier work on the context's stream; stream i then decodes min(n_in[i], n_in_dev[i]) symbols.  cap_out: bytes each out pointer can
 * take.  Queues everything and returns at once; one run is in flight per object (a second run_async before wait: LSDR_E_ARG). */
int lsdr_viterbi_batch_run_async(lsdr_viterbi_batch *vb, const lsdr_softsymbol *const *in_dev, const size_t *n_in,
                                 const uint64_t *n_in_dev, uint8_t *const *out_dev, size_t cap_out);
/* synchronises the context's stream once and copies n_streams records (results may be NULL) */
int lsdr_viterbi_batch_wait(lsdr_viterbi_batch *vb, lsdr_viterbi_batch_result *results);
/* the same records on the device ([n_streams], valid once the run's work on the stream is done), for a consumer kernel */
const lsdr_viterbi_batch_result *lsdr_viterbi_batch_results_dev(const lsdr_viterbi_batch *vb);
/* kernel launches queued by the last run_async; run_async calls since create */
int lsdr_viterbi_batch_stats(const lsdr_viterbi_batch *vb, unsigned *launches_last_run, unsigned long long *runs);

/* ---- mpeg_sync<u8,0>, dvb.h:712-891: bit alignment, polarity and 0x47/0xB8 sync search, lock tracking.
 * One run() call.  *call_next_sync = 1 when the reference would call deconv->next_sync() (dvb.h:771-779);
 * state_events (host, may be NULL) receives the values written to the lock-state pipe (0/1), at most 2.
 * *locktime receives the running count of packets since lock (the last value written to the locktime
 * pipe; one value per produced packet, consecutive).  Synchronous. */
typedef struct lsdr_mpeg_sync lsdr_mpeg_sync;
int lsdr_mpeg_sync_create(lsdr_ctx *ctx, int fastlock, lsdr_mpeg_sync **m);
void lsdr_mpeg_sync_destroy(lsdr_mpeg_sync *m);
int lsdr_mpeg_sync_run(lsdr_mpeg_sync *m, const uint8_t *in, size_t n_in, uint8_t *out, size_t cap_out,
                       size_t *consumed, size_t *produced, int *state_events_host, int *n_state_events,
                       unsigned long *locktime, int *call_next_sync);
int lsdr_mpeg_sync_locked(const lsdr_mpeg_sync *m);
int lsdr_mpeg_sync_reset(lsdr_mpeg_sync *m);                     /* a freshly constructed block (options kept); stream-ordered */
int lsdr_mpeg_sync_set_resync_period(lsdr_mpeg_sync *m, int period);   /* public member resync_period (dvb.h:717), used by --hs */

/* ---- deinterleaver<u8>::run, dvb.h:932-944 (Forney I=12, M=17 as a gather).  Needs 2448 bytes per
 * packet window; *produced packets of 204 B, *consumed = 204 * produced.  Asynchronous. */
int lsdr_deinterleaver_run(lsdr_ctx *ctx, const uint8_t *in, size_t n_in, uint8_t *out_packets, size_t cap_packets,
                           size_t *consumed, size_t *produced);

/* ---- rs_decoder<u8,0>::run + rs_engine, dvb.h:998-1053, rs.h:84-272.  in: n packets of 204 B (corrected in
 * place like the reference), out: n packets of 188 B (sync byte ^0x55 when uncorrectable).  `bits`/`errs`
 * are the values of the bitcount/errcount pipes for this call.  Synchronous (counters). */
int lsdr_rs_decoder_run(lsdr_ctx *ctx, uint8_t *in_packets, size_t n_packets, uint8_t *out_packets,
                        long *bits, long *errs);

/* ---- derandomizer, dvb.h:1107-1163: PRBS removal, resync on the inverted sync byte, drops packets whose
 * restored sync byte is not 0x47.  Synchronous (output count is data dependent). */
typedef struct lsdr_derandomizer lsdr_derandomizer;
int lsdr_derandomizer_create(lsdr_ctx *ctx, lsdr_derandomizer **d);
void lsdr_derandomizer_destroy(lsdr_derandomizer *d);
int lsdr_derandomizer_reset(lsdr_derandomizer *d);               /* a new stream begins (PRBS position 0) */
int lsdr_derandomizer_run(lsdr_derandomizer *d, const uint8_t *in_packets, size_t n_packets, uint8_t *out_packets,
                          size_t cap_packets, size_t *consumed, size_t *produced);
/* host-side tables for tests: PRBS pattern (dvb.h:1116-1129), GF(256) exp/log and RS generator (rs.h:47-105) */
void lsdr_derandomizer_pattern(uint8_t *pattern1504_host);
void lsdr_rs_tables(uint8_t *exp512_host, uint8_t *log256_host, uint8_t *G17_host);

/* -------------------------------------------------------------- `--hs` path (leandvb.cc:727-969)
 * fast_qpsk_receiver<u8> (sdr.h:946-1189): cu8 samples → hard QPSK symbols {0,1,2,3}; optional FREQ measurements
 * (one per meas_decimation samples) and one sampled constellation point per chunk, both to HOST buffers.
 * _create = ctor + set_omega(omega) + set_freq(freq) + the public members; _run = run() over one buffer (needs
 * 129 samples and room for 128 symbols).  Bit-exact incl. the carried loop state. */
typedef struct lsdr_fastqpsk lsdr_fastqpsk;
int lsdr_fastqpsk_create(lsdr_ctx *ctx, float omega, float freq, float pll_adjustment, int allow_drift,
                         unsigned long meas_decimation, lsdr_fastqpsk **r);
void lsdr_fastqpsk_destroy(lsdr_fastqpsk *r);
int lsdr_fastqpsk_get_state(const lsdr_fastqpsk *r, float *mu, unsigned *phase, long long *freqw, long long *min_freqw,
                            long long *max_freqw);
/* throughput mode (time-tiled like LSDR_RX_TILED; not bit-exact at the symbol level, no FREQ/constellation reports);
 * tile_len / tile_warmup in samples (multiples of 128), 0 = defaults (≈ 400 symbols of warm-up, tiles twice that) */
int lsdr_fastqpsk_set_tiled(lsdr_fastqpsk *r, int enable, unsigned tile_len, unsigned tile_warmup);
int lsdr_fastqpsk_tiled_stats(const lsdr_fastqpsk *r, unsigned *tiles, unsigned *dup, unsigned *miss, unsigned *bad_seams);
int lsdr_fastqpsk_run(lsdr_fastqpsk *r, const lsdr_cu8 *in, size_t n_in, uint8_t *out, size_t cap_out, size_t *consumed,
                      size_t *produced, float *freq_out_host, size_t freq_cap, size_t *n_freq, lsdr_cu8 *cstln_out_host,
                      size_t cstln_cap, size_t *n_cstln);
/* dvb_deconvol_sync<u8> (dvb.h:612-707) on deconvol_poly2 (convolutional.h:80-192): 512 hard symbols → 64 bytes per
 * chunk, the four alignments re-scored every resync_period chunks.
 * Both blocks are one call per buffer with a host read of their counts; the whole `--hs` graph for many captures at once, with every
 * count on the device, is lsdr_hs_batch (below, behind the capture batch). */
typedef struct lsdr_hsdeconv lsdr_hsdeconv;
int lsdr_hsdeconv_create(lsdr_ctx *ctx, int resync_period, lsdr_hsdeconv **d);
void lsdr_hsdeconv_destroy(lsdr_hsdeconv *d);
int lsdr_hsdeconv_locked(const lsdr_hsdeconv *d);
int lsdr_hsdeconv_run(lsdr_hsdeconv *d, const uint8_t *in, size_t n_in, uint8_t *out, size_t cap_out, size_t *consumed,
                      size_t *produced);

/* -------------------------------------------------------------- transmit chain (leandvbtx.cc:79-175)
 * Device pointers throughout; every *_run is the body of the reference block's run() over one buffer. */
typedef struct lsdr_randomizer lsdr_randomizer;          /* randomizer, dvb.h:1063-1102 (8-packet pattern position carried) */
int lsdr_randomizer_create(lsdr_ctx *ctx, lsdr_randomizer **r);
void lsdr_randomizer_destroy(lsdr_randomizer *r);
int lsdr_randomizer_run(lsdr_randomizer *r, const uint8_t *in_packets, size_t n_packets, uint8_t *out_packets, size_t cap_packets,
                        size_t *consumed, size_t *produced);
/* rs_encoder, dvb.h:957-980 + rs_engine::encode, rs.h:141-167: 188-byte packets → 204-byte packets */
int lsdr_rs_encoder_run(lsdr_ctx *ctx, const uint8_t *in_packets, size_t n_packets, uint8_t *out_packets, size_t cap_packets,
                        size_t *consumed, size_t *produced);
/* interleaver, dvb.h:899-921: needs 12 packets, consumes n−11 */
int lsdr_interleaver_run(lsdr_ctx *ctx, const uint8_t *in_packets, size_t n_packets, uint8_t *out_bytes, size_t cap_bytes,
                         size_t *consumed_packets, size_t *produced_bytes);
/* fec_specs[rate] (dvb.h:553-565): bits entering / leaving the convolutional coder and its generator polynomials. */
int lsdr_fec_spec(int rate, int *bits_in, int *bits_out, uint16_t polys_host[8]);
typedef struct lsdr_convol lsdr_convol;                  /* dvb_convol, dvb.h:567-604 (16-bit history carried) */
int lsdr_convol_create(lsdr_ctx *ctx, int rate, int bits_per_symbol, lsdr_convol **v);
void lsdr_convol_destroy(lsdr_convol *v);
int lsdr_convol_run(lsdr_convol *v, const uint8_t *in, size_t n_in, uint8_t *out, size_t cap_out, size_t *consumed, size_t *produced);
/* cstln_transmitter<f32,0>, sdr.h:1196-1222, with make_dvbs2_constellation(cstln, rate) */
int lsdr_cstln_transmitter_run(lsdr_ctx *ctx, int cstln, int rate, const uint8_t *sym, size_t n, lsdr_cf32 *out);
typedef struct lsdr_fir_resampler lsdr_fir_resampler;    /* fir_resampler<cf32,float>, dsp.h:290-364 (interpolator, decim = 1) */
int lsdr_fir_resampler_create(lsdr_ctx *ctx, unsigned ncoeffs, const float *coeffs_host, unsigned interp, lsdr_fir_resampler **f);
void lsdr_fir_resampler_destroy(lsdr_fir_resampler *f);
int lsdr_fir_resampler_set_freq(lsdr_fir_resampler *f, float freq);
/* *consumed = min((n_in·interp − ncoeffs)/interp, n_in − latency, cap_out/interp), latency = (ncoeffs + interp)/interp;
 * *produced = *consumed·interp.  The n_in − latency bound is the one place where the block deliberately departs from the
 * reference: it changes nothing unless interp divides ncoeffs, where the reference's last output group reads in[n_in] — a pipe
 * slot nobody has written, so its value there is arbitrary.  Here no read leaves in[0 … n_in); the held-back sample is consumed,
 * and its group produced, by the next call.  Carry the unconsumed input as with every other block. */
int lsdr_fir_resampler_run(lsdr_fir_resampler *f, const lsdr_cf32 *in, size_t n_in, lsdr_cf32 *out, size_t cap_out, size_t *consumed,
                           size_t *produced);
typedef struct lsdr_simple_agc lsdr_simple_agc;          /* simple_agc<f32>, sdr.h:238-274 (power estimate carried) */
int lsdr_simple_agc_create(lsdr_ctx *ctx, float out_rms, float bw, lsdr_simple_agc **a);
void lsdr_simple_agc_destroy(lsdr_simple_agc *a);
int lsdr_simple_agc_set(lsdr_simple_agc *a, float out_rms, float bw);
int lsdr_simple_agc_run(lsdr_simple_agc *a, const lsdr_cf32 *in, size_t n_in, lsdr_cf32 *out, size_t cap_out, size_t *consumed,
                        size_t *produced);

/* ---- channel simulator of leanchansim (leanchansim.cc:34-190): noise, adder, LO drift, f32 → u8 ------------------ */
typedef struct lsdr_wgn lsdr_wgn;                          /* wgn_c<f32>, dsp.h:164-190, on glibc's drand48()/logf() */
/* seeded = 0: the drand48 state of a process that never seeds (leanchansim --deterministic); else srand48(seed)
 * (leanchansim.cc:146-147 seeds with the pid). */
int lsdr_wgn_create(lsdr_ctx *ctx, int seeded, long seed, lsdr_wgn **w);
void lsdr_wgn_destroy(lsdr_wgn *w);
int lsdr_wgn_get_state(lsdr_wgn *w, unsigned long long *x48);
int lsdr_wgn_set_state(lsdr_wgn *w, unsigned long long x48);
/* the next n samples of wgn_c::run (stddev is its public member); add != NULL: out = add + noise (adder fused) */
int lsdr_wgn_run(lsdr_wgn *w, float stddev, const lsdr_cf32 *add, lsdr_cf32 *out, size_t n);
/* adder<cf32>::run, dsp.h:125-134 */
int lsdr_adder_run(lsdr_ctx *ctx, const lsdr_cf32 *a, const lsdr_cf32 *b, size_t n, lsdr_cf32 *out);
/* cconverter<f32,0,u8,128,1,1>::run, dsp.h:40-50 (x86 float → int32 → u8 truncation) */
int lsdr_cconverter_f32_u8_run(lsdr_ctx *ctx, const lsdr_cf32 *in, size_t n, lsdr_cu8 *out);
/* cconverter<f32,0,int16_t,0,32768,1>::run (leandvbtx --s16, leandvbtx.cc:179): out = interleaved (re, im) int16 */
int lsdr_cconverter_f32_s16_run(lsdr_ctx *ctx, const lsdr_cf32 *in, size_t n, int16_t *out);
typedef struct lsdr_drifter lsdr_drifter;                  /* drifter<float>, leanchansim.cc:34-88 */
int lsdr_drifter_create(lsdr_ctx *ctx, lsdr_drifter **d);
void lsdr_drifter_destroy(lsdr_drifter *d);
int lsdr_drifter_set_component(lsdr_drifter *d, int i, float amp, float freq);   /* public member drifts[i] */
int lsdr_drifter_get_phases(lsdr_drifter *d, long long a[3]);
int lsdr_drifter_set_phases(lsdr_drifter *d, const long long a[3]);
/* n samples as consecutive run() calls of `chunk` samples (0: one call).  run() restarts its phase accumulator at 0, so
 * the reference's output depends on how its 4096-sample pipes cut the stream; pass 4096 to reproduce leanchansim. */
int lsdr_drifter_run(lsdr_drifter *d, const lsdr_cf32 *in, size_t n, lsdr_cf32 *out, size_t chunk);

/* ------------------------------------------------------------ capture batch
 * BASELINE configs 1 and 4: B independent cu8 captures, each decoded from its FIRST SAMPLE to transport-stream packets by the blocks of
 * leandvb's default `--u8` graph, freshly constructed per capture (leandvb.cc:157-600: one scheduler per capture):
 *     cconverter<u8,128,f32,0,1,1> → auto_notch<f32>(anf slots, setpoint 0) → cstln_receiver<f32>(linear_sampler, QPSK) →
 *     deconvol_sync<u8,0> → mpeg_sync<u8,0> → deinterleaver<u8> → rs_decoder<u8,0> → derandomizer          (leandvb.cc:211-217,
 *     296-301, 425-510, 521-596; dsp.h:40-50, sdr.h:46-154, 697-938, dvb.h:122-513, 712-891, 926-948, 985-1058, 1107-1163)
 * All captures of a batch share every launch (blockIdx.y = capture) and every data-dependent count stays on the device — the symbols the
 * receiver produced, where mpeg_sync locked, the packets the derandomizer kept: the host reads one result record per capture and batch.
 *  * front end: the time-tiled receiver of LSDR_RX_TILED with packed decisions (tolerance mode, same seam reconciliation), restated for
 *    VALU issue (leansdr_amd/csrc/rxb_device.h), with the one-slot notch of sdr.h:119-138 INSIDE the tile's sample walk:
 *    S[n] = p·S[n−1] + k·x[n], out = x − S, p = (1−k)·exp(j2π·bin/4096) — float32 with exact phases (lsdr_notch_fir's tolerance class);
 *    detect() (sdr.h:76-118) is the reference's FFT bit for bit, at the reference's detect points, on the device.  auto_notch moves
 *    whole 4096-sample blocks: with anf = 1 a capture's last n mod 4096 samples are not demodulated (as in the reference).
 *  * FEC tail: the bit-exact blocks of this ABI, driven on the device the way a scheduler with `unlocked_window`-byte pipes drives them while
 *    mpeg_sync is unlocked (next_sync() included), then in one call each (leansdr_amd/csrc/tail_device.h).
 * anf ∈ {0, 1}; omega = Fs/Fm ∈ [1, 8]; tile_len a multiple of 2048 (0: 4096), tile_warmup a multiple of 128 (0: 512).
 * One batch in flight per object: run_async → wait → [ts_download_async → ts_wait]; the NEXT run_async may be queued while the
 * download is in flight (its last kernel waits for it).  Use two objects on two contexts to overlap one batch's tail with the other's
 * front end.
 *
 * The VITERBI engine (lsdr_capture_batch_create_viterbi) is the same object for `leandvb --u8 … --viterbi` (leandvb.cc:498-501, 532-540,
 * 558-596), the graph that decodes weak signals:
 *     cconverter<u8> → auto_notch → cstln_receiver(linear_sampler, QPSK, pll_adjustment / 6) → viterbi_sync → mpeg_sync(deconv = NULL) →
 *     deinterleaver → rs_decoder → derandomizer
 *  * front end: the same tiles with SOFT symbols out — per symbol one lsdr_softsymbol, `symbol` the two sign bits, `cost` the exact integer
 *    arithmetic of the constellation table on the tile's truncated coordinates; so cost and symbol are exact functions of the tile's own
 *    sampled point and only the loop trajectory is tolerance-class, as in the default engine (tile 0 is the reference's arithmetic).  A
 *    cost scales with the point's amplitude, and a tile cannot reproduce the serial AGC (an average over a hundred chunks) in its warm-up:
 *    the record's coordinates are taken at the gain of a second power estimator that the tile starts from the mean it measured over its
 *    warm-up, while timing and carrier loops run exactly as in the default engine (leansdr_amd/csrc/rxb_device.h).  The
 *    records are staged transposed (row = symbol step, column = tile: a wavefront's 64 tiles write 64 consecutive dwords) and compacted
 *    into one contiguous array per capture, its count in device memory.  Memory: 4 bytes per symbol, staged and compacted — about 7 bytes
 *    per input sample at 1.2 samples per symbol (the default engine: about 0.5).
 *  * Viterbi stage: one lsdr_viterbi_batch, a stream per capture, on the context the tail runs on; it reads the compacted soft symbols
 *    with their counts from device memory and writes straight into the tail's byte buffers.  lsdr_viterbi_batch commits a prefix per
 *    call and plans the next call on the host, so a batch takes several ROUNDS.  run_async queues the front end and round 1; WAIT DRIVES
 *    THE REMAINING ROUNDS (one host read of B records per round, every round shared by all captures: their number does not grow with B),
 *    then queues the tail and waits for it.  The bytes are viterbi_sync's whatever the number of rounds.
 *  * FEC tail: mpeg_sync's search runs over bytes that are already there (no deconvol_sync, no next_sync()); the rest is the same.  In the
 *    result, bytes_deconv is the number of bytes viterbi_sync committed, next_sync_calls is 0, alignment is viterbi_sync's current_sync.
 * cfg->fec is viterbi_sync's code rate, with leandvb's rule "QPSK 2/3 is handled as 4/6"; what lsdr_viterbi_batch_create refuses is
 * refused here with the same code.  Every other call works on both kinds of object; words_dev returns NULL on a Viterbi object, soft_dev
 * and viterbi_stats NULL / LSDR_E_ARG on a default one.  The accessors return NULL for i outside [0, n_captures). */
typedef struct lsdr_capture_batch lsdr_capture_batch;
typedef struct {
  int n_captures;            /* B */
  size_t max_samples;        /* per capture */
  float omega;               /* samples per symbol, cstln_receiver::set_omega(Fs/Fm), leandvb.cc:482 */
  int fec;                   /* LSDR_FEC12 … (deconvol_sync's rate, leandvb.cc:521-531) */
  int anf;                   /* auto_notch slots: 1 = leandvb's default (leandvb.cc:103), 0 = `--anf 0` */
  unsigned tile_len, tile_warmup;
  float notch_k;             /* auto_notch::k (0: 0.002, sdr.h:56) */
  int notch_decimation;      /* auto_notch::decimation in samples (0: 1024·4096, sdr.h:56) */
  unsigned unlocked_window;  /* bytes deconvol_sync hands mpeg_sync per call while mpeg_sync is not locked = the byte pipe between them
                              * (0: 8192 = leandvb's BUF_BYTES at its default --buf-factor 4, leandvb.cc:194); decides how far the
                              * deconvolver runs ahead of a next_sync() */
  unsigned aux_cus;          /* 0: every kernel on the context's stream.  N (a multiple of 8, < the device's CUs): the object runs on two
                              * streams of its own with disjoint compute-unit masks — the receiver's TILES (vector-issue-bound, they fill
                              * every wave slot they can get for milliseconds) on all CUs but N, everything else (the notch's detect chain
                              * and estimator pre-pass, seam pass, compaction, the whole FEC tail: memory-bound kernels) on N/8 CUs of
                              * every XCD, handed over by events.  Several objects made with the same N share the two partitions: one
                              * batch's tail then runs beside another's tiles instead of waiting for their wave slots. */
} lsdr_capture_batch_cfg;
typedef struct {
  uint64_t ts_packets;       /* packets in the capture's TS buffer */
  uint64_t rs_packets, rs_bit_errors;   /* rs_decoder: packets decoded, bits corrected (dvb.h:1007-1040) */
  uint64_t symbols;          /* decisions the receiver produced */
  uint64_t samples;          /* samples the receiver consumed */
  uint64_t bytes_deconv, bytes_mpeg, first_lock_byte;
  uint32_t next_sync_calls, locked, alignment, bitphase;     /* deconvol_sync::next_sync() calls; mpeg_sync locked at the end; alignment in force */
  uint32_t tiles, seam_dup, seam_miss, seam_bad;             /* receiver seams: duplicates dropped, symbols re-inserted, unreconciled */
} lsdr_capture_result;
typedef struct {
  int resync_period;         /* viterbi_sync::resync_period in chunks (0: 32, dvb.h:1232) */
  int reserved[7];           /* 0 */
} lsdr_capture_viterbi_cfg;
typedef struct {             /* the Viterbi stage of capture i in the last batch */
  uint32_t rounds;           /* lsdr_viterbi_batch calls in which this capture's stream committed symbols */
  uint32_t batch_rounds;     /* calls the batch made (the last one finds nothing left to commit in any stream) */
  uint32_t switches, stalls; /* calls that ended behind an alignment switch / in front of an unverified seam */
  uint32_t tiles, repaired;  /* Viterbi tiles planned; tiles the device decoded again */
  uint32_t current_sync, pad;
  uint64_t symbols, bytes;   /* soft symbols consumed, bytes committed */
} lsdr_capture_viterbi_stats;
int lsdr_capture_batch_create(lsdr_ctx *ctx, const lsdr_capture_batch_cfg *cfg, lsdr_capture_batch **b);
/* vcfg may be NULL (defaults) */
int lsdr_capture_batch_create_viterbi(lsdr_ctx *ctx, const lsdr_capture_batch_cfg *cfg, const lsdr_capture_viterbi_cfg *vcfg,
                                      lsdr_capture_batch **b);
void lsdr_capture_batch_destroy(lsdr_capture_batch *b);
/* iq_dev: HOST array of B DEVICE pointers to lsdr_cu8 items (16-byte aligned), n_samples each.  Queues everything; returns at once. */
int lsdr_capture_batch_run_async(lsdr_capture_batch *b, const lsdr_cu8 *const *iq_dev, size_t n_samples);
/* waits for the batch's kernels; results[B] (may be NULL) */
int lsdr_capture_batch_wait(lsdr_capture_batch *b, lsdr_capture_result *results);
/* after wait: copies every capture's TS (ts_packets·188 bytes) to ts_host[i] (pinned memory recommended) on a side stream */
int lsdr_capture_batch_ts_download_async(lsdr_capture_batch *b, uint8_t *const *ts_host, size_t cap_bytes);
int lsdr_capture_batch_ts_wait(lsdr_capture_batch *b);
const uint8_t *lsdr_capture_batch_ts_dev(const lsdr_capture_batch *b, int i);          /* device buffer of capture i's TS */
const uint32_t *lsdr_capture_batch_words_dev(const lsdr_capture_batch *b, int i);     /* its packed decisions (16 per word, MSB first) */
const uint8_t *lsdr_capture_batch_bytes_dev(const lsdr_capture_batch *b, int i);      /* deconvol_sync's output, mpeg_sync's output */
const uint8_t *lsdr_capture_batch_mpeg_dev(const lsdr_capture_batch *b, int i);
/* Viterbi objects: capture i's compacted soft symbols (result.symbols of them), the Viterbi stage's counters after wait */
const lsdr_softsymbol *lsdr_capture_batch_soft_dev(const lsdr_capture_batch *b, int i);
int lsdr_capture_batch_viterbi_stats(const lsdr_capture_batch *b, int i, lsdr_capture_viterbi_stats *stats);
/* the notch's detected bins of capture i after a run (tests): bins[0 … *n) */
int lsdr_capture_batch_bins(lsdr_capture_batch *b, int i, int *bins, unsigned cap, unsigned *n);
/* tests: the NOTCHED stream of capture i exactly as the tiles of the last run saw it — the same start state per tile (from the estimator
 * pre-pass), the same interval switches, the same recurrence — written to device memory as n cf32 items (anf = 1 only; synchronous) */
int lsdr_capture_batch_notched(lsdr_capture_batch *b, int i, lsdr_cf32 *out_dev, size_t n);
/* HIP events around the tile kernel of every run while enabled: mean duration since the previous call, then sets the switch */
int lsdr_capture_batch_tile_time(lsdr_capture_batch *b, int enable, float *avg_ms, unsigned *launches);

/* Re-acquisition after a lost lock (default engine).  Without it the tail walks the UNLOCKED phase in unlocked_window-byte calls of
 * deconvol_sync, mpeg_sync behind every one of them, and at the first lock deconvolves everything that is left in one call.  If the lock
 * drops inside that call — a fade, a burst — mpeg_sync searches the rest alone: the next_sync() it asks for (dvb.h:775-779) finds every
 * symbol deconvolved already (deconvol_sync::next_sync takes effect on the symbols run() has not read, dvb.h:185-193, 419-470), and a
 * capture whose carrier loop comes back on a rotation that needs another alignment loses everything behind the burst.  In the reference
 * the deconvolver is never more than one byte pipe ahead of mpeg_sync, so the request still reaches it.
 *
 * relocks = R > 0 keeps that schedule for the whole capture.  Capture i's tail output — the deconvolved bytes up to bytes_deconv, the mpeg
 * bytes, the RS counts, next_sync_calls, locked, alignment, bitphase, first_lock_byte and the TS — is what this loop makes of the
 * capture's packed decisions:
 *   1. deconvol_sync::run with at most unlocked_window bytes of room, at the alignment in force (its own sizes, dvb.h:419-470);
 *   2. mpeg_sync::run() until nothing moves (dvb.h:743-754);
 *   3. every next_sync() it asks for;
 *   4. again, until the deconvolver produces nothing;
 * with one exception: from the (R+1)-th lock on, a call made while mpeg_sync is locked has the whole remainder for room — the schedule
 * without re-acquisition, which R = 0 is exactly.  A capture whose lock drops behind such a call is `exhausted`: it ends like a capture
 * does today.  The locked stretches are still deconvolved and realigned by the whole chip, a stretch of whole windows per launch; that
 * changes no byte.  The device runs R + 1 such stretches at most, in a fixed sequence of launches with no host read in between; a
 * capture that needs fewer leaves the others at once.
 * Limits: R re-acquisitions per capture (at most 16); a search that does not finish before the capture ends gains nothing (mpeg_sync
 * tries 8 bit phases of 8 packets three times per alignment: up to 4·3·64 packets per round of the four alignments); the default engine
 * only — in the Viterbi and --hs graphs the alignment search sits in front of the tail.
 * lsdr_capture_relock_set: for the batches queued after it, every entry point and sample format.  LSDR_E_ARG: relocks > 16, a batch
 * in flight.  LSDR_E_UNSUPPORTED: a Viterbi object.
 * lsdr_capture_relock_get: capture i of the waited-for batch.  LSDR_E_ARG: i out of range, no batch waited for.
 * LSDR_E_UNSUPPORTED: a Viterbi object.  A batch that ran with relocks = 0 leaves the record zero, both byte offsets ~0. */
typedef struct {
  uint32_t locks, drops;          /* mpeg_sync: times it locked, times it lost the lock */
  uint32_t passes;                /* whole-chip stretches this capture used */
  uint32_t exhausted;             /* 1: the lock dropped behind a call that had the whole remainder for room */
  uint64_t first_drop_byte;       /* deconvolved-stream offset behind the packet at which the lock first dropped (~0: never) */
  uint64_t last_lock_byte;        /* … at which mpeg_sync locked last (~0: never), as first_lock_byte counts */
  uint32_t next_sync_behind_first_lock, pad;   /* next_sync() calls made after the first lock */
} lsdr_capture_relock_stats;      /* 40 bytes */
int lsdr_capture_relock_set(lsdr_capture_batch *b, unsigned relocks);   /* 0 = off (default) … 16 */
int lsdr_capture_relock_get(const lsdr_capture_batch *b, int i, lsdr_capture_relock_stats *s);   /* after wait */

/* Signal reports: per capture what `leandvb --fd-info` prints — cstln_receiver writes FREQ, SS and MER once per meas_decimation samples
 * (sdr.h:857-913: the estimators est_insp / est_sp / est_ep of sdr.h:866-889, freqw behind the drift clamp of sdr.h:895-898; leandvb.cc:428-430,
 * 465, 502, 600-605; leandvb's period is Fs/Finfo).  They tell a weak capture (MER) from a mistuned one (FREQ, held inside
 * ± 65536/omega/2048 table units per sample around the capture's tune — 0 in a uniform run, lsdr_capture_each below) and from one at the wrong level (SS: the LEVEL CONTRACT below asks for about 75).
 * Both engines, all sample formats, in the batch's own launches: the tiles fold each body chunk's estimator inputs into an affine map
 * per tile (a chunk belongs to exactly one tile's body; the error vector is taken at the serial gain the tile estimates, as the soft
 * records are), one more launch per batch composes the maps of every capture from the constructed estimators, and the records follow the
 * result records into pinned host memory — nothing is synchronised or read on the host between run_async and wait.  Reports inside tile 0
 * are the reference's bit for bit; the others hold leansdr_amd/tolerance.py's ss_rtol / mer_atol_db / capture_batch_freq_atol against
 * the serial receiver.  An object with reports off (the default) runs the kernels and launches it would run without this call.
 * LSDR_E_ARG: a period in (0, 128) (several reports per chunk), i outside [0, n_captures), a batch in flight, lsdr_capture_reports_get
 * with reports off.  LSDR_E_UNSUPPORTED: a period of 2^31 samples or more that still fits into max_samples. */
typedef struct { float freq, ss, mer; uint32_t pad; } lsdr_capture_report;   /* freq_tap in cycles per sample; sqrt(est_insp); dB */
/* period_samples = cstln_receiver::meas_decimation (leandvb: Fs/Finfo); 0 = off (the default).  Not while a batch is in flight.  Buffers
 * are sized for max_samples here. */
int lsdr_capture_reports_set(lsdr_capture_batch *b, uint64_t period_samples);
/* after wait: capture i's reports of the last batch, oldest first (result.samples / period_samples of them); *n = how many there are (may
 * exceed cap: cap are written); last (may be NULL) = the estimators behind the capture's last chunk */
int lsdr_capture_reports_get(lsdr_capture_batch *b, int i, lsdr_capture_report *out, size_t cap, size_t *n, lsdr_capture_report *last);

/* Other sample formats: the same object for captures that are not cu8.  leandvb reads five formats into the same graph (leandvb.cc:208-261);
 * here the format replaces the graph's first block(s), fused into every load that touches a capture — the converted, scaled stream never
 * exists in device memory:
 *     LSDR_IN_CU8   --u8   cconverter<u8,128,f32,0,1,1>         leandvb.cc:211-217   (the default; exactly lsdr_capture_batch_create[_viterbi])
 *     LSDR_IN_CS8   --s8   cconverter<s8,0,f32,0,1,1>           leandvb.cc:218-227
 *     LSDR_IN_CU16  --u16  cconverter<u16,32768,f32,0,1,1>      leandvb.cc:228-237
 *     LSDR_IN_CS16  --s16  cconverter<s16,0,f32,0,1,1>          leandvb.cc:238-248
 *     LSDR_IN_CF32  --f32 --float-scale in_scale                leandvb.cc:249-258: the raw items through scaler<float,cf32,cf32>
 * (dsp.h:40-50: float((int)item − Z), exact for all four integer types; dsp.h:149-156: re·scale, im·scale, one rounding each).  in_scale
 * behind an integer format is that scaler behind the converter — a block leandvb does not put there; it exists for the LEVEL CONTRACT:
 * tiles j ≥ 1 start from the constructed AGC (est_insp = 75², gain 1) and cannot re-measure the level in their warm-up (kest = 0.01 per
 * chunk), so THE CONVERTED, SCALED SAMPLES MUST HAVE AN RMS NEAR 75, which cu8 data has by construction and 16-bit or float data only if the
 * caller scales it (a power of two where bit-identity with another format matters: s16 = 256·s8 with in_scale 2^-8 is the s8 run bit for
 * bit).  Measured window (profiles/capture_batch_formats/level.txt: true 16-bit captures against `leandvb --f32 --float-scale` at the same
 * value): RMS 19 … 75 — the TS is the reference's, at noise 7.5 (both engines) and at noise 18 (Viterbi engine); RMS 150 — still at noise 7.5,
 * the weak capture loses 14 % of its packets; RMS 300 — the weak capture does not lock (seam_bad > 0).  When in doubt scale low.  Tile 0 is the reference's arithmetic
 * on the converted floats bit for bit, the detect FFT likewise; the rest is the tolerance class of the cu8 object.
 * Every other lsdr_capture_batch_* call works on an object made this way, except the typed lsdr_capture_batch_run_async, which returns
 * LSDR_E_ARG on a non-cu8 object (a cu8 pointer is never read as wider items).  All captures of a batch have the object's format.
 * LSDR_E_ARG: in_format outside the five, in_scale negative or not finite, nonzero reserved, a capture pointer not aligned to its item
 * size (2, 2, 4, 4, 8 bytes; 16 with anf = 1).  LSDR_E_UNSUPPORTED: LSDR_IN_CU8 with a scale other than 0 or 1 (the cu8 kernels have no
 * scaler); for the other formats max_samples × bytes per item ≥ 0xfff00000 (the tiles' 32-bit buffer offsets: 2^30 samples of a 16-bit
 * format, 2^29 of cf32, are too many). */
typedef struct {
  int in_format;     /* LSDR_IN_CU8 (default), LSDR_IN_CS8, LSDR_IN_CU16, LSDR_IN_CS16: cconverter<T,Z,f32,0,1,1> (leandvb.cc:208-248, dsp.h:40-50);
                        LSDR_IN_CF32: the raw cf32 items (leandvb.cc:249-258) */
  float in_scale;    /* 0 or 1: none.  Else every converted sample is multiplied by it, re and im, one rounding each: scaler<float,cf32,cf32>
                        (dsp.h:149-156) behind the converter; for cf32 it IS leandvb's --float-scale */
  int reserved[6];   /* 0 */
} lsdr_capture_input_cfg;
/* vcfg == NULL: the default engine; icfg == NULL: cu8, unscaled (then exactly lsdr_capture_batch_create[_viterbi]) */
int lsdr_capture_any_create(lsdr_ctx *ctx, const lsdr_capture_batch_cfg *cfg, const lsdr_capture_viterbi_cfg *vcfg,
                            const lsdr_capture_input_cfg *icfg, lsdr_capture_batch **b);
/* iq_dev: HOST array of B DEVICE pointers to n_samples items of the object's format, aligned to the item size (16 bytes with anf = 1) */
int lsdr_capture_any_run_async(lsdr_capture_batch *b, const void *const *iq_dev, size_t n_samples);

/* ------------------------------------------------------------ `--hs` batch
 * leandvb's "maximum throughput" graph (`leandvb --u8 --hs [--fastlock] [--tune F] [--drift]`, leandvb.cc:813-893) for B independent cu8
 * captures, each decoded from its FIRST SAMPLE to TS by freshly constructed blocks (cu8 only, and it stays so: `--hs requires --u8`,
 * leandvb.cc:773-774 — the other sample formats are lsdr_capture_any_create's):
 *     fast_qpsk_receiver<u8>(omega, set_freq, allow_drift) → dvb_deconvol_sync<u8>(resync_period = fastlock ? 1 : 32) →
 *     mpeg_sync<u8,0>(deconv = NULL, fastlock = true, resync_period = fastlock ? 1 : 32) → deinterleaver → rs_decoder → derandomizer
 * (sdr.h:946-1189, dvb.h:612-707, 712-891; rate 1/2 only, no notch).  All captures share every launch (blockIdx.y = capture).  run_async
 * queues everything on the context's stream and returns — captures uploaded with lsdr_memcpy_h2d on that context are ordered in front of
 * it; wait is one event synchronisation plus the read of B pinned records.  There are no rounds and no host read in between:
 *  * receiver: time-tiled as lsdr_fastqpsk_set_tiled does it (one lane per tile, the same seam reconciliation), body symbols staged
 *    transposed and compacted into one contiguous u8 array per capture, its count in device memory.  Tile 0 runs from the constructed
 *    state: its symbols are the reference's bit for bit.  Tile j ≥ 1 starts tile_warmup samples early at mu = phase = 0 with the
 *    CONSTRUCTED frequency word (`freq`) and is held within ± 65536 / omega / 2048 of it (4.07e-4 cycles per sample at omega 1.2) — the
 *    contract of both tiled receivers: A CAPTURE MUST BE TUNED TO WITHIN THAT WINDOW OF ITS CARRIER (`freq`, leandvb's --tune);
 *    per capture: lsdr_hs_each_run_async below.
 *  * dvb_deconvol_sync: all four alignments are scored on the chunks ≡ 0 (mod resync_period); the score uses the second half of a
 *    chunk's words only, so it carries no history, and for a freshly constructed block the alignment in force while chunk c is decoded is
 *    c == 0 ? 0 : first arg-min of the scores of chunk ((c − 1) / P)·P — a function of the symbol stream, evaluated per thread.
 *  * FEC tail: the capture batch's tail without deconvol_sync, mpeg_sync constructed with fastlock / resync_period as above.
 * lsdr_capture_result as for the capture batch: next_sync_calls is 0, alignment is the deconvolver's alignment at the end, bytes_deconv
 * is 64 × the chunks decoded, symbols the hard symbols produced, samples = (n_samples − 1) / 128 · 128.
 * One batch in flight per object: run_async → wait → [ts_download_async → ts_wait]; the next run_async may be queued while a download is
 * in flight.  LSDR_E_ARG: n_captures < 1, tile sizes that are no multiples of 128, nonzero reserved, n_samples > max_samples, run_async
 * while a batch is in flight, wait with nothing in flight.  n_samples < 129 is a valid batch that produces nothing.  The accessors
 * return NULL for i outside [0, n_captures). */
typedef struct lsdr_hs_batch lsdr_hs_batch;
typedef struct {
  int n_captures;            /* B */
  size_t max_samples;        /* per capture */
  float omega;               /* Fs/Fm, fast_qpsk_receiver::set_omega */
  float freq;                /* set_freq(Ftune/Fs), cycles per sample: lsdr_fastqpsk_create's convention */
  int allow_drift, fastlock;
  unsigned tile_len, tile_warmup;   /* samples, multiples of 128; 0 = lsdr_fastqpsk_set_tiled's defaults */
  int reserved[8];           /* 0 */
} lsdr_hs_batch_cfg;
int lsdr_hs_batch_create(lsdr_ctx *ctx, const lsdr_hs_batch_cfg *cfg, lsdr_hs_batch **b);
void lsdr_hs_batch_destroy(lsdr_hs_batch *b);
/* iq_dev: HOST array of B DEVICE pointers to lsdr_cu8 items (4-byte aligned), n_samples each.  Queues everything; returns at once. */
int lsdr_hs_batch_run_async(lsdr_hs_batch *b, const lsdr_cu8 *const *iq_dev, size_t n_samples);
int lsdr_hs_batch_wait(lsdr_hs_batch *b, lsdr_capture_result *results /* [B], may be NULL */);
/* after wait: copies every capture's TS (ts_packets·188 bytes) to ts_host[i] (pinned memory recommended) on a side stream */
int lsdr_hs_batch_ts_download_async(lsdr_hs_batch *b, uint8_t *const *ts_host, size_t cap_bytes);
int lsdr_hs_batch_ts_wait(lsdr_hs_batch *b);
const uint8_t *lsdr_hs_batch_ts_dev(const lsdr_hs_batch *b, int i);        /* device buffer of capture i's TS */
const uint8_t *lsdr_hs_batch_symbols_dev(const lsdr_hs_batch *b, int i);   /* its hard symbols, one per byte (result.symbols of them) */
const uint8_t *lsdr_hs_batch_bytes_dev(const lsdr_hs_batch *b, int i);     /* dvb_deconvol_sync's output, mpeg_sync's output */
const uint8_t *lsdr_hs_batch_mpeg_dev(const lsdr_hs_batch *b, int i);

/* ------------------------------------------------------------ per-capture lengths and --tune in one batch
 * The recordings of a job never have equal lengths, and a capture the reports show as mistuned (FREQ) needs leandvb's --tune
 * (demod.set_freq(Ftune/Fs), leandvb.cc:483-487, 817-821).  An EACH run gives every capture of a batch its own length and its own tune;
 * tune is GIVEN by the caller exactly as --tune is — nothing here estimates it; lsdr_tune_est (below) produces that number from the raw
 * capture, in front of the decode and apart from it.
 *  * Capture i of an each run is decoded as a freshly constructed graph with set_freq(each[i].tune) over its first each[i].n_samples items.
 *    wait, the TS download, the accessors, reports and viterbi_stats work as before; every result is per capture: in lsdr_capture_result
 *    samples, tiles, symbols and seam_* are that capture's own, as are the packed words / soft symbols, the report slots and the final
 *    record (result.samples / period reports), the detected bins (the detect points inside that capture) and the Viterbi bytes.
 *  * COMPOSITION INVARIANCE: what capture i produces does not depend on the other captures of the batch — bit for bit the TS, every field
 *    of lsdr_capture_result, packed words and soft symbols, report slots and final record, detected bins, Viterbi bytes.  (The launches
 *    are sized for the longest capture; every kernel leaves by the capture's own counts.  With anf = 1 the notch instantiation of the
 *    tiles runs when ANY capture has a detect point; a capture without one passes through it unchanged.)
 *  * The uniform entry points (lsdr_capture_batch_run_async, lsdr_capture_any_run_async, lsdr_hs_batch_run_async) are the each path with
 *    equal lengths and tune = 0 (capture batch) or tune = cfg.freq (hs batch); their outputs are what they were.
 *  * In the hs batch each[i].tune replaces cfg.freq for that capture.
 *  * iq_dev[i] may be NULL only where n_samples is 0 (a valid capture that decodes nothing).  Alignment per item, and 16 bytes with
 *    anf = 1, as for the uniform calls.  The non-cu8 objects (lsdr_capture_any_create) go through the same call: hence `void`.
 *  * THE TUNING CONTRACT with tune in it: tiles j >= 1 start from the frequency word constructed for tune and are held within
 *    +- 65536/omega/2048 table units per sample of it (4.07e-4 cycles per sample at omega 1.2), so THE CARRIER MUST LIE WITHIN THAT WINDOW
 *    OF tune; the hs batch has its own window of the same width around tune.  FREQ reports are held inside that window around tune, no
 *    longer around 0; the drift clamp (sdr.h:895-898) is the reference's, around tune as well.
 * LSDR_E_ARG, with a message, the object left usable: n_samples > max_samples, tune not finite or |tune| >= 0.5, nonzero reserved, a
 * batch in flight. */
typedef struct {
  size_t n_samples;   /* this capture's length, <= cfg.max_samples; 0 is valid (nothing decoded) */
  float  tune;        /* set_freq(Ftune/Fs) for this capture, cycles per sample, sign as lsdr_hs_batch_cfg.freq / lsdr_fastqpsk_create:
                         a capture multiplied by exp(+j2π·f·n) is tuned with +f */
  int    reserved[5]; /* 0 */
} lsdr_capture_each;   /* 32 bytes */
int lsdr_capture_each_run_async(lsdr_capture_batch *b, const void *const *iq_dev, const lsdr_capture_each *each /* [B], host */);
int lsdr_hs_each_run_async(lsdr_hs_batch *b, const lsdr_cu8 *const *iq_dev, const lsdr_capture_each *each /* [B], host */);

/* ------------------------------------------------------------ per-capture carrier offset, estimated (QPSK)
 * The number lsdr_capture_each.tune wants, from the raw capture: recordings whose carriers are off by more than the tiles' window (an
 * ordinary LNB or SDR offset is many times 4.07e-4 cycles per sample) are estimated here, then decoded with the estimates.  It runs in
 * front of the batch decoders and touches none of their kernels; the TUNING CONTRACT above is unchanged.
 *
 * THE ESTIMATOR.  The fourth power of a QPSK signal carries no modulation and has a spectral line at 4·f.  For one capture of n items let
 * M = min(blocks, n / 4096) whole blocks of N = 4096 samples, from the capture's first sample:
 *   1 convert the samples as the capture batch's loads do: float(item − Z)·in_scale (lsdr_capture_input_cfg);
 *   2 divide each block by its own RMS, so that level and format cannot overflow the fourth power; an all-zero block contributes zeros;
 *   3 w = z⁴, X = FFT_N(w), rectangular window;
 *   4 P[k] = Σ_blocks |X[k]|², summed in block order;
 *   5 k0 = the first arg-max of P, c = P[k0], l and r its cyclic neighbours; m = sqrt(max(l, r)/c), δ = ±m/(1 + m), + when r ≥ l;
 *     κ = k0 + δ taken into [−N/2, N/2); tune = κ/(4N) cycles per sample;
 *   6 the sign is lsdr_capture_each.tune's: a capture multiplied by exp(+j2π·f·n) yields +f;
 *   7 quality = c / mean(P);
 *   8 M == 0: the record is all zeros (blocks = 0).  (So is tune and quality of a capture whose blocks are all zero: c = 0.)
 * RANGE: |f| < 1/8 cycle per sample — the fourth power folds at 1/4.  QPSK only.  A narrow-band interferer stronger than the line wins the
 * peak, and quality does not tell the two apart.  The estimate is taken from the capture's start; a carrier that moves is --drift's job.
 * ACCURACY, measured on synthetic DVB-S captures (tests/test_tune_est_abi.py, tests/test_gpu_tune_est.py) with eight
 * blocks, at 1.2, 4 and 8 samples per symbol, noise 7.5 and 18 on the cu8 scale, offsets 0 … ±0.12: |tune − f| ≤ 2.3e-6 cycles per sample,
 * 0.6 % of the tuning window at omega 1.2 and 3.7 % of it at omega 8; the tests hold it to an eighth of the narrowest window (7.6e-6).
 * QUALITY reads as the line's height over the spectrum's mean: 350 … 2000 on those captures, at most 3.2 on Gaussian noise alone (eight
 * blocks); a capture below about 30 has no line worth tuning to.  The device works in float32 and agrees with a float64 restatement to
 * 1e-6 of the peak power.
 * A record is a pure function of the capture's own converted samples: no atomics, every sum in a fixed order — bit for bit the same alone,
 * in any batch, and in every format that converts to the same floats (cs16 = 256·cs8 with in_scale 2^-8 is the cs8 run).
 * run_async queues everything on the context's stream (behind lsdr_memcpy_h2d on that context) and returns: one launch over all blocks of
 * all captures, one over the captures, the records' copy to pinned memory; no host read in between.  wait is one event synchronisation and
 * the read of B records.  One run in flight per object.
 * iq_dev: HOST array of B DEVICE pointers, each aligned to its item size (2, 2, 4, 4, 8 bytes for cu8, cs8, cu16, cs16, cf32; a 16-byte
 * aligned capture is read by 16-byte loads), NULL only where n_samples[i] is 0.  Nothing behind block M − 1 of a capture is read.
 * LSDR_E_ARG, with a message, the object (if any) left usable: n_captures < 1 (or above 65535), in_format outside the five LSDR_IN_*, in_scale
 * negative or not finite, blocks > 64, nonzero reserved; a misaligned pointer, samples without a pointer, run_async with a run in flight, wait with none. */
typedef struct lsdr_tune_est lsdr_tune_est;
typedef struct {
  int n_captures;      /* B */
  int in_format;       /* LSDR_IN_CU8, _CS8, _CU16, _CS16, _CF32 */
  float in_scale;      /* as lsdr_capture_input_cfg.in_scale: 0 or 1 = none (the normalisation makes the estimate independent of it, up to rounding) */
  unsigned blocks;     /* blocks of 4096 samples per capture, at most 64; 0 = 8 */
  int reserved[4];     /* 0 */
} lsdr_tune_est_cfg;
typedef struct {
  float tune;          /* cycles per sample: what lsdr_capture_each.tune takes */
  float quality;       /* power[1] / mean_power */
  uint32_t bin;        /* k0, 0 … 4095 */
  uint32_t blocks;     /* M: the blocks that were used; 0 = no whole block, the record is all zeros */
  float power[3];      /* l, c, r: P at k0 − 1, k0, k0 + 1 (cyclic) */
  float mean_power;    /* mean(P) */
} lsdr_tune_estimate;  /* 32 bytes */
int lsdr_tune_est_create(lsdr_ctx *ctx, const lsdr_tune_est_cfg *cfg, lsdr_tune_est **e);
void lsdr_tune_est_destroy(lsdr_tune_est *e);
int lsdr_tune_est_run_async(lsdr_tune_est *e, const void *const *iq_dev, const size_t *n_samples /* [B], host */);
int lsdr_tune_est_wait(lsdr_tune_est *e, lsdr_tune_estimate *out /* [B] */);

/* ------------------------------------------------------------ per-capture samples per symbol, estimated (PSK, RRC shaping)
 * The number every batch object wants at create (lsdr_capture_batch_cfg.omega, lsdr_hs_batch_cfg.omega, lsdr_resample_design's omega),
 * from the raw capture: a job of recordings is not all at one symbol rate, and the reference has no block for this (--sr is mandatory).
 * It runs in front of the decoders, before or beside lsdr_tune_est, and touches none of their kernels.
 *
 * THE ESTIMATOR.  The squared magnitude of a root-raised-cosine PSK signal has a spectral line at the symbol rate, wherever the carrier
 * is.  For one capture of n items let M = min(blocks, n / 4096) whole blocks of N = 4096 samples, from the capture's first sample:
 *   1 convert the samples as the capture batch's loads do: float(item − Z)·in_scale (lsdr_capture_input_cfg);
 *   2 per block s = mean |z|² and p[n] = |z[n]|²/s − 1; a block with s = 0 contributes zeros to every sum below and is not counted in M₁;
 *   3 X = FFT_N(p + 0j), rectangular window (lsdr_tune_est's transform); P[k] += |X[k]|², summed in block order;
 *   4 in the same pass c₁ += Σ_{n=1…N−1} z[n]·conj(z[n−1]) / s, the sum inside the block in a fixed order; R = |c₁| / (M₁·(N − 1)), M₁ the
 *     number of nonzero blocks: the normalised lag-one autocorrelation magnitude, which no carrier offset moves;
 *   5 the bins searched are k ∈ [k_lo, N/2], k_lo = max(2, ⌊N/omega_max⌋) (P is symmetric, and the low bins hold the level's slow content;
 *     with omega_max < 2, where that lies behind N/2 and only candidate b below is admissible, k_lo = max(2, ⌊N·(1 − 1/omega_min)⌋));
 *     floor = mean of P over them; k0 = their first arg-max, c = P[k0]; l′ = max(P[k0−1] − floor, 0), r′ = max(P[k0+1] − floor, 0);
 *     m = sqrt(max(l′, r′)/c), δ = ±m/(1 + m), + when r′ ≥ l′; line = (k0 + δ)/N, folded into (0, 0.5] by line ↦ 1 − line where it
 *     exceeds 0.5;
 *   6 the candidates are omega_a = 1/line (≥ 2) and omega_b = 1/(1 − line) (in [1, 2]): the line of omega < 2 aliases onto that of some
 *     omega ≥ 2 (1.2 and 6 both put it at 1/6 cycle per sample).  A candidate outside [omega_min, omega_max] is dropped.  If both remain,
 *     a is chosen when |R − |sinc(line)|| < |R − |sinc(1 − line)||, else b, with sinc(x) = sin(πx)/(πx).  omega is the chosen candidate,
 *     other the other one, or 0 if it was dropped; ambiguous = 1 when both were admissible and line > 0.4 (omega in about (1.67, 2.5),
 *     where the two converge and R cannot be trusted to tell them apart);
 *   7 quality = c / floor;
 *   8 the record is all zeros when M = 0, when c = 0, or when no candidate is admissible.
 * LIMITS: QPSK/PSK with RRC shaping — the line's height follows the roll-off, and a roll-off near 0 has no line.  The estimate is taken
 * from the capture's start.  A periodic interferer in the magnitude can win the peak.  omega within [omega_min, omega_max] ⊆ [1.016, 64].
 * ACCURACY, measured on synthetic DVB-S captures (roll-off 0.35; tests/test_rate_est_abi.py, tests/test_gpu_rate_est.py; DESIGN.md
 * §4.11) with 64 blocks, at 6/5, 3/2, 3, 4, 8 and 12 samples per symbol, noise 7.5 and 18 on the cu8 scale, every capture 0.03 cycles
 * per sample off tune: |omega/true − 1| ≤ 3.0e-5; the tests hold it to 2.5e-4, a quarter of the 1e-3 by which the reference's --sr may be
 * off with its TS unchanged.  QUALITY reads as the line's height over the mean of the searched bins: 47 … 187 on those captures, at most
 * 1.6 on Gaussian noise alone with 64 blocks (2.3 with 16); a capture below about 10 has no line worth believing.
 * A record is a pure function of the capture's own converted samples: no atomics, every sum in a fixed order — bit for bit the same alone,
 * in any batch and at any place in it, run twice, and in every format that converts to the same floats.
 * run_async queues everything on the context's stream (behind lsdr_memcpy_h2d on that context) and returns: one launch over all blocks of
 * all captures, one over the captures, the records' copy to pinned memory; no host read in between.  wait is one event synchronisation and
 * the read of B records.  One run in flight per object.
 * iq_dev: HOST array of B DEVICE pointers, each aligned to its item size (2, 2, 4, 4, 8 bytes for cu8, cs8, cu16, cs16, cf32; a 16-byte
 * aligned capture is read by 16-byte loads), NULL only where n_samples[i] is 0.  Nothing behind block M − 1 of a capture is read.
 * LSDR_E_ARG, with a message naming rate_est, the object (if any) left usable: n_captures < 1 (or above 65535), in_format outside the five
 * LSDR_IN_*, in_scale negative or not finite, blocks > 256, omega_min or omega_max outside [1.016, 64] or omega_min > omega_max, nonzero
 * reserved; a misaligned pointer, samples without a pointer, run_async with a run in flight, wait with none. */
typedef struct lsdr_rate_est lsdr_rate_est;
typedef struct {
  int n_captures;      /* B */
  int in_format;       /* LSDR_IN_CU8, _CS8, _CU16, _CS16, _CF32 */
  float in_scale;      /* as lsdr_tune_est_cfg.in_scale: 0 or 1 = none (the normalisation makes the estimate independent of it, up to rounding) */
  unsigned blocks;     /* blocks of 4096 samples per capture, at most 256; 0 = 64 */
  float omega_min;     /* the smallest samples per symbol admitted; 0 = 1.016 */
  float omega_max;     /* the largest; 0 = 64 */
  int reserved[2];     /* 0 */
} lsdr_rate_est_cfg;   /* 32 bytes */
typedef struct {
  float omega;         /* samples per symbol: what the batch objects' omega takes; 0 = nothing found (the record is all zeros) */
  float other;         /* the candidate that was not chosen; 0 = it was not admissible */
  float line;          /* the line's frequency, cycles per sample, in (0, 0.5] */
  float quality;       /* power[1] / floor */
  float corr;          /* R */
  uint32_t bin;        /* k0, k_lo … 2048 */
  uint32_t blocks;     /* M: the blocks that were used */
  uint32_t ambiguous;  /* 1: both candidates admissible and line > 0.4 */
  float power[3];      /* P at k0 − 1, k0, k0 + 1 */
  float floor;         /* mean of P over the searched bins */
} lsdr_rate_estimate;  /* 48 bytes */
int lsdr_rate_est_create(lsdr_ctx *ctx, const lsdr_rate_est_cfg *cfg, lsdr_rate_est **e);
void lsdr_rate_est_destroy(lsdr_rate_est *e);
int lsdr_rate_est_run_async(lsdr_rate_est *e, const void *const *iq_dev, const size_t *n_samples /* [B], host */);
int lsdr_rate_est_wait(lsdr_rate_est *e, lsdr_rate_estimate *out /* [B] */);

/* ------------------------------------------------------------ the carriers of a wideband capture, found in its spectrum
 * The step in front of every object above: those take one carrier per capture, and in a recording of a whole transponder the strongest
 * carrier's lines win and the others are never seen.  The scan reads the averaged power spectrum the way a person reads
 * lsdr_spectrum_batch's picture: which carriers there are, where, and roughly how wide.  Behind it lsdr_resample_batch takes the same
 * pointer once per carrier with the centres as tunes, and lsdr_rate_est / lsdr_tune_est refine what the scan read on the decimated
 * streams.  The reference has no block for this (leansdrscan tries command lines).  It touches no other object's kernels.
 *
 * THE DEFINITION, for one capture of n items, N = 4096:
 *   1 M = min(blocks, n / N) whole blocks.  spread = 0: block b is the capture's b-th.  spread = 1: block b starts at sample b·stride·N,
 *     stride = max(1, (n / N) / blocks) in integer division — the scan sees the whole recording, not its start;
 *   2 per block: the samples converted as the capture batch's loads do, float(item − Z)·in_scale; the Hann window from the transform's
 *     own table, w[n] = 0.5f − 0.5f·(float)cos(2πn/N), z·w component-wise (no division by the RMS: powers stay absolute);
 *     X = FFT_N (lsdr_tune_est's transform); |X[k]|² of all N bins;
 *   3 P[k] = Σ_blocks |X[k]|², float, in block order (lsdr_carrier_scan_spectrum_dev, FFT order: bin k is frequency k/N, above N/2 negative);
 *   4 S[k] = (Σ_{j=−smooth…+smooth} P[(k+j) mod N]) / (float)(2·smooth + 1), float, j ascending: a circular boxcar;
 *   5 floor = the value of rank N/8 (from 0: the 513th smallest) among the N values of S; T = floor·factor, one float multiply,
 *     factor = (float)pow(10.0, threshold_db/10.0);
 *   6 above[k] = S[k] ≥ T.  A run starts at s where above[s] and not above[(s−1) mod N] and lasts while above holds, across the N−1 → 0
 *     seam if it has to.  Runs are taken in ascending (s + N/2) mod N: by start frequency from −1/2 upward, a run across ±1/2 last.
 *     All bins above: saturated = 1 and no carriers; none above: no carriers.  Runs of fewer than min_bins bins are dropped; found
 *     counts the rest, the first max_carriers of them are listed;
 *   7 per listed run [a, b] (unwrapped indices, S indexed mod N), n = b − a + 1, q = n / 4, in double on the float values of S:
 *     plateau = (Σ_{k=a+q…b−q} S[k]) / (n − 2q), ascending; L = plateau − floor; H = floor + L/2, the half-power level — a raised-cosine
 *     spectrum crosses it at ±Fm/2 whatever the roll-off, so the width measured there is the symbol rate.  H < T: weak = 1, lo = a − 0.5,
 *     hi = b + 0.5.  Otherwise i = the first k ≥ a with S[k] ≥ H, lo = i − (S[i] − H)/(S[i] − S[i−1]); j = the last k ≤ b with S[k] ≥ H,
 *     hi = j + (S[j] − H)/(S[j] − S[j+1]).  c = (lo + hi)/(2N), center = c − floor(c + 0.5): cycles per sample in [−1/2, 1/2), the sign of
 *     lsdr_capture_each.tune and of lsdr_spectrum_batch's centre.  bandwidth = (hi − lo)/N, omega = 1/bandwidth, level = L/floor (linear;
 *     10·log10 of it is the carrier's C/N in dB where the floor is the noise).  Every float is the one nearest to the double value;
 *   8 a capture with M = 0 gives records (and a spectrum) of all zeros; the unlisted carrier records of a capture are all zeros.
 * LIMITS.  The floor is a rank statistic of the smoothed spectrum: a front end whose passband droops at the edges, or a band that is more
 * than 7/8 occupied, biases it.  bandwidth is the symbol rate only for RRC-shaped carriers.  An unmodulated or narrow interferer is listed
 * like any carrier: `bins` near min_bins, and a later lsdr_rate_est quality below 10, tell it apart.  A weak carrier near the threshold
 * may come out in pieces.  The picture is of the blocks scanned, not of what happens between them.
 * ACCURACY, measured on sums of synthetic DVB-S carriers plus noise (tests/scan_common.py, tests/test_carrier_scan_abi.py; DESIGN.md
 * §4.15) with 64 blocks (16 in brackets): every carrier found and none in noise alone; |omega/true − 1| ≤ 1.7 % (3.4 %) — the boxcar and the
 * window widen every carrier by about 1 % —; level within 0.2 dB (0.4) of the carriers' C/N; |center − true| ≤ 1.5e-4 cycles per sample
 * (2.9e-4) for carriers of 8 … 24 samples per symbol 9 … 22 dB above the noise, and 3.7e-4, 1.5 bins (4.6e-4), for one of 4 samples per symbol
 * at 11.5 dB.  The half-power edges of a carrier 1024 bins wide with 358-bin skirts move with the ±4 % that 64 blocks and 17 bins leave on S:
 * over twelve other draws of the noise that carrier's centre had a standard deviation of 4.3e-4, up to 7.4e-4 off.  The centre is a coarse
 * value in any case: lsdr_tune_est on the decimated stream has the fine one.
 * A capture's records are a pure function of its own converted samples: no atomics, every sum in a fixed order, the runs found in
 * integers — bit for bit the same alone, in any batch and at any place in it, and in every format that converts to the same floats.
 * run_async queues everything on the context's stream and returns: one launch over all blocks of all captures, one over the captures,
 * the records' copies to pinned memory.  wait is one event synchronisation and the read of the records.  One run in flight per object.
 * iq_dev: as lsdr_rate_est_run_async's.  Nothing behind a capture's last used block is read.
 * LSDR_E_ARG, with a message naming carrier_scan, the object (if any) left usable: n_captures < 1 (or above 65535), in_format outside the
 * five LSDR_IN_*, in_scale negative or not finite, blocks > 256, smooth > 64, threshold_db negative or not finite, max_carriers > 64,
 * nonzero reserved; a misaligned pointer, samples without a pointer, run_async with a run in flight, wait with none. */
typedef struct lsdr_carrier_scan lsdr_carrier_scan;
typedef struct {
  int n_captures;        /* B */
  int in_format;         /* LSDR_IN_CU8, _CS8, _CU16, _CS16, _CF32 */
  float in_scale;        /* as lsdr_tune_est_cfg.in_scale: 0 or 1 = none; powers scale with its square, the records' ratios do not */
  unsigned blocks;       /* blocks of 4096 samples per capture, at most 256; 0 = 64 */
  int spread;            /* 0: the capture's first blocks; otherwise: blocks spread over the whole capture */
  unsigned smooth;       /* the boxcar's half width in bins, 1 … 64; 0 = 8 */
  float threshold_db;    /* the threshold above the floor, > 0; 0 = 3 */
  unsigned min_bins;     /* the shortest run kept; 0 = 2·smooth + 1 */
  unsigned max_carriers; /* the records per capture, at most 64; 0 = 32 */
  int reserved[3];       /* 0 */
} lsdr_carrier_scan_cfg; /* 48 bytes */
typedef struct {
  uint32_t blocks;       /* M: the blocks that were used; 0 = no whole block, everything is zero */
  uint32_t stride;       /* blocks between two used blocks (1 without spread) */
  uint32_t found;        /* runs of at least min_bins bins */
  uint32_t listed;       /* min(found, max_carriers): the records that are filled */
  uint32_t saturated;    /* 1: every bin is above the threshold (no floor to speak of) */
  uint32_t reserved;
  float floor;           /* the value of rank N/8 of S */
  float threshold;       /* T */
} lsdr_scan_summary;     /* 32 bytes */
typedef struct {
  float center;          /* cycles per sample in [−1/2, 1/2): what lsdr_capture_each.tune takes */
  float bandwidth;       /* cycles per sample between the half-power edges: Fm/Fs of an RRC-shaped carrier */
  float omega;           /* 1 / bandwidth: samples per symbol */
  float level;           /* (plateau − floor) / floor, linear */
  float plateau;         /* mean of S over the run's middle half */
  uint32_t first_bin;    /* a, 0 … 4095 */
  uint32_t bins;         /* n */
  uint32_t weak;         /* 1: the half-power level is under the threshold; the edges are the run's */
} lsdr_scan_carrier;     /* 32 bytes */
int lsdr_carrier_scan_create(lsdr_ctx *ctx, const lsdr_carrier_scan_cfg *cfg, lsdr_carrier_scan **e);
void lsdr_carrier_scan_destroy(lsdr_carrier_scan *e);
int lsdr_carrier_scan_run_async(lsdr_carrier_scan *e, const void *const *iq_dev, const size_t *n_samples /* [B], host */);
int lsdr_carrier_scan_wait(lsdr_carrier_scan *e, lsdr_scan_summary *summaries /* [B] */, lsdr_scan_carrier *carriers /* [B·max_carriers] */);
/* capture i's P of the last run: 4096 floats on the device, FFT order; valid until the next run_async or destroy (NULL: i out of range) */
const float *lsdr_carrier_scan_spectrum_dev(lsdr_carrier_scan *e, int i);

/* ------------------------------------------------------------ per-stream code rate, estimated from the hard symbols (QPSK)
 * The last constructor argument of the batch decoders that has to be known per capture: lsdr_capture_batch_cfg.fec, leandvb's mandatory
 * --cr.  A capture decoded at the wrong rate gives nothing back and says nothing about why.  The measurement is the reference's own:
 * deconvol_sync inverts the convolutional code with two different polynomials per output bit (deconv[b], deconv2[b], dvb.h:225-265) and
 * readerrors() (dvb.h:391-412) counts how often they disagree — --fastlock chooses among the four alignments by that count and gives an
 * alignment up above 1/3 (dvb.h:449-453).  deconv[b] ^ deconv2[b] is a parity check of the punctured code: 0 on every error-free code word
 * of the right rate at the right alignment and symbol phase, a coin flip on anything else.  This object sweeps it over all five rates,
 * every symbol phase of the puncturing pattern and the four alignments, for many streams at once.  It needs no tune, no MPEG framing and
 * no second decode: the receivers' QPSK decisions do not depend on fec, so one front-end pass feeds every hypothesis.
 *
 * THE DEFINITION.  All integers: every implementation agrees bit for bit.  One stream has n hard symbols s[0 … n), each `symbol & 3` as
 * deconvol_sync reads them (dvb.h:373,396); the first min(n, max_symbols) are scored.  A hypothesis is (rate r, alignment a, skip k):
 *   r in {1/2, 2/3, 3/4, 5/6, 7/8}; 2/3 is handled as 4/6 (dvb.h:491-495) and reported as LSDR_FEC23;
 *   a in 0 … 3: the lut of init_syncs (dvb.h:308-360);
 *   k in [0, punctweight/2): 1, 3, 2, 3, 4 values for the five rates — 13 (rate, skip) pairs, 52 hypotheses.
 * E(r,a,k) is what readerrors() of a freshly constructed deconvol_sync of rate r on alignment a counts over all complete refills of
 * s[k … n): R = (n − k >= 32) ? (n − k − 32)/(punctweight/2) + 1 : 0 refills; refill q looks at the 32 symbols that end in front of
 * symbol k + 32 + q·punctweight/2 (the newest in the window's low bits) and adds, for b = punctperiod − 1 … 0,
 * parity(w & deconv[b]) != parity(w & deconv2[b]).  C(r,a,k) = R·punctperiod.
 * Per rate the best hypothesis is the first, a outer and k inner, with the smallest E/C; fractions are compared exactly
 * (E1·C2 < E2·C1 in 64-bit integers) and a hypothesis with C = 0 never wins.  Per stream the winner is the first rate, in the order
 * above, with the smallest best fraction; locked = (C > 0 and 3·E <= C), the reference's own criterion; ambiguous = a second rate also
 * satisfies it.  No symbols, or fewer than 32: the record is all zeros with fec = −1.
 * WHAT THE FRACTION MEANS.  The check polynomials have w = 10 / 12 / 18 / 24 / 32 taps (1/2 … 7/8); at a channel bit error rate q the right
 * hypothesis reads (1 − (1 − 2q)^w)/2 and every wrong one about 1/2.  It stays under 1/3 up to q of about 5 % at rate 1/2 and 1.7 % at 7/8:
 * exactly where leandvb --fastlock itself holds an alignment.  Measured (tests/test_fec_est_host.py): synthetic captures at
 * 1.2 samples per symbol, noise 7.5 on the cu8 scale, 4096 symbols: 0.044 … 0.137 for the transmitted rate, at least 0.449 for every
 * other; uniformly random symbols 0.462.
 * LIMITS: QPSK only.  Hard decisions only: a weak capture that needs --viterbi reads near 1/2 for every rate and comes back locked = 0.
 * The estimate rests on the first max_symbols symbols, acquisition included.  The checks have even weight: a stretch of constant symbols
 * satisfies those of every rate, so a stream that is partly constant reads below 1/2 for the wrong rates too (`ambiguous` says so).
 * run_async queues everything on the context's stream and returns: a memset of the counters, one launch over all tiles of all streams,
 * one over the streams, the records' copy to pinned memory; nothing is synchronised or read on the host in between.  wait is one event
 * synchronisation and the read of n_streams records.  One run in flight per object.
 * LSDR_E_ARG, with a message naming fec_est, the object (if any) left usable: n_streams < 1 (or above 65535), max_symbols 0 (or above
 * 2^28), an unknown in_format, nonzero reserved; symbols without a pointer, a packed or soft pointer that is not 4-byte aligned,
 * run_async with a run in flight, wait with none. */
enum { LSDR_HSYM_PACKED2 = 0,   /* 16 per uint32, MSB first: lsdr_capture_batch_words_dev, LSDR_SYM_HARD2 */
       LSDR_HSYM_U8 = 1,        /* one per byte: lsdr_hs_batch_symbols_dev, lsdr_fastqpsk_run */
       LSDR_HSYM_SOFT = 2 };    /* lsdr_softsymbol, `symbol & 3`: lsdr_capture_batch_soft_dev, lsdr_rx_run */
typedef struct lsdr_fec_est lsdr_fec_est;
typedef struct { int n_streams; size_t max_symbols; int in_format; int reserved[5]; } lsdr_fec_est_cfg;
typedef struct { uint64_t errors, checks; uint32_t sync, skip; } lsdr_fec_est_score;   /* 24 bytes */
typedef struct {
  int32_t fec;                 /* LSDR_FEC12 / 23 / 34 / 56 / 78; −1: nothing scored */
  uint32_t locked, ambiguous, sync, skip, pad;
  uint64_t symbols;            /* symbols scored: min(n, max_symbols) */
  float error_rate, runner_up; /* (float)((double)E/C) of the winner and of the best other rate */
  lsdr_fec_est_score score[5]; /* per rate, in the order 1/2, 2/3, 3/4, 5/6, 7/8: its best hypothesis */
} lsdr_fec_estimate;           /* 160 bytes */
int lsdr_fec_est_create(lsdr_ctx*, const lsdr_fec_est_cfg*, lsdr_fec_est**);
void lsdr_fec_est_destroy(lsdr_fec_est*);
/* the symbols per workgroup tile: the lengths at which the score kernel changes its path are multiples of it */
unsigned lsdr_fec_est_tile(const lsdr_fec_est*);
/* sym_dev: HOST array of DEVICE pointers (may be NULL where n is 0); sym_offset (may be NULL: zeros): the first symbol's position in the
 * stream that starts at sym_dev[i] (packed streams: any value; the others: added to the pointer); n[i] symbols from there, of which the first
 * min(n[i], max_symbols) are scored.  Queues everything on the context's stream and returns. */
int lsdr_fec_est_run_async(lsdr_fec_est*, const void *const *sym_dev, const uint64_t *sym_offset, const uint64_t *n);
int lsdr_fec_est_wait(lsdr_fec_est*, lsdr_fec_estimate *out /* [n_streams] */);
/* host only, no context: the polynomials a rate is scored with (what lsdr_deconv_create computes); returns punctperiod, *punctweight
 * (0, with a message, for a rate that is none of the five) */
int lsdr_fec_est_polys(int rate, uint64_t deconv[8], uint64_t deconv2[8], int *punctweight);

/* ------------------------------------------------------------ resample batch: --derotate --resample for many captures
 * The batch decoders take omega = Fs/Fm in [1, 8] and have no filter in front of the receiver; a recording from an ordinary SDR is wider
 * (2.4 MS/s around a 250 kS/s carrier is omega 9.6).  leandvb puts rotator<f32> (--derotate, leandvb.cc:310-318, sdr.h:1226-1259) and a
 * decimating low-pass fir_filter<cf32,float> (--resample, leandvb.cc:353-384, dsp.h:219-285) there.  This is that front end for B captures
 * in ONE launch: any of the five sample formats in, each capture with its own length and its own carrier offset, cf32 streams out, which
 * lsdr_capture_any_create(LSDR_IN_CF32, in_scale 1) decodes unchanged at omega / decim (the taps have DC gain 1: a capture at the level
 * contract's RMS stays there).  The hs batch stays cu8 and is not served.
 *
 * THE ARITHMETIC, one float32 rounding per operation (no contraction).  For one capture of n items, N = ncoeffs, D = decim, taps h:
 *   1 x[k] = float(item − Z)·in_scale, exactly as the capture batch's loads convert (lsdr_capture_input_cfg; a scale of 0 or 1 multiplies
 *     by nothing);
 *   2 ifreq = (int)(tune·65536), C truncation (rotator's own `int ifreq = freq * 65536`).  Sample k has the phase index
 *     (−k·ifreq) mod 65536, taken into [0, 65536) with 64-bit k; (c, s) = T[index] with T[j] = ((float)cos(2πj/65536), (float)sin(2πj/65536))
 *     evaluated in double at create — one table for all captures;  y.re = x.re·c − x.im·s;  y.im = x.re·s + x.im·c.
 *     This is rotator<f32>(−ifreq/65536) with EXACT phases: the reference's table is cosf of an angle rounded to float, and that noise is
 *     not reproduced (the stance lsdr_notch_fir takes).  Measured against the reference chain: tests/test_resample_abi.py, DESIGN.md §4.9;
 *   3 out[m] = Σ_{i=0…N−1} h[i]·y[N + m·D − i], i ascending, re and im separately, each from 0 by acc = acc + h[i]·y: real taps in
 *     fir_filter's order (dsp.h:246-262);
 *   4 produced = n ≥ N ? min((n − N)/D, cap_out) : 0; consumed = produced·D.  Both are functions of the sizes, known at run_async: wait is
 *     one event synchronisation, nothing is counted on the device.
 * So: with ifreq == 0 the output equals cconverter / scaler → fir_filter in LSDR_FIR_EXACT as values (a −0 may come out as +0); and a
 * capture's output is a pure function of its own samples, its tune and the taps — bit for bit the same alone, in any batch, in any place
 * of it, from a 16-byte aligned pointer or an item-aligned one, and in every format that converts to the same floats.
 * tune has lsdr_capture_each's sign (a capture multiplied by exp(+j2πfn) is given +f) and is applied as ifreq/65536; what is left,
 * (f − ifreq/65536)·D cycles per decimated sample, is the decoder's tune (lsdr_tune_est on the decimated stream measures it).
 * LIMITS: decim 1 … 64, ncoeffs 2 … 1024, n_captures ≤ 65535; anything else is LSDR_E_UNSUPPORTED at create.
 * LSDR_E_ARG, with a message naming the field, the object (if any) left usable: n_captures < 1, in_format outside the five, in_scale
 * negative or not finite, nonzero reserved (cfg or each), coeffs_host NULL; n_samples > max_samples, tune not finite or |tune| ≥ 0.5, an
 * input pointer not aligned to its item (2, 2, 4, 4, 8 bytes), an output pointer not aligned to 16 bytes, samples without a pointer, outputs
 * without an output pointer, cap_out smaller than some capture's (n − N)/D (refused, never truncated), run_async with a run in flight, wait
 * with none.  n_samples < N + D is a valid capture that produces nothing; iq_dev[i] may be NULL only where n_samples is 0. */
/* host only: leandvb.cc:353-378 for omega = Fs/Fm.  decim 0: (int)(omega/4), at least 1.  order = (int)(rej*omega/(22*0.5*rolloff))
 * made even, Fcut = 0.5*(1+rolloff/2)/omega, filtergen::lowpass + normalize_dcgain(1) through lsdr_filtergen_*: the reference's floats.
 * *decim_out and *ncoeffs are always written; LSDR_E_ARG where cap < *ncoeffs (or coeffs_host is NULL): nothing is written to coeffs_host. */
int lsdr_resample_design(float omega, float rolloff, float rej, unsigned decim, unsigned *decim_out,
                         float *coeffs_host, unsigned cap, unsigned *ncoeffs);
typedef struct lsdr_resample_batch lsdr_resample_batch;
typedef struct { int n_captures; size_t max_samples; int in_format; float in_scale;   /* as lsdr_capture_input_cfg */
                 unsigned ncoeffs; const float *coeffs_host; unsigned decim; int reserved[6]; } lsdr_resample_batch_cfg;
typedef struct { uint64_t consumed, produced; int32_t ifreq; float applied; /* ifreq/65536 */ uint32_t pad[2]; } lsdr_resample_result;
int  lsdr_resample_batch_create(lsdr_ctx*, const lsdr_resample_batch_cfg*, lsdr_resample_batch**);
void lsdr_resample_batch_destroy(lsdr_resample_batch*);
/* the outputs per workgroup tile chosen for (ncoeffs, decim): the lengths at which the kernel changes its path are multiples of it */
unsigned lsdr_resample_batch_tile(const lsdr_resample_batch*);
/* each[i] = {n_samples, tune}: lsdr_capture_each, same sign (a capture multiplied by exp(+j2πfn) is given +f).
 * out_dev: HOST array of B DEVICE pointers, 16-byte aligned, cap_out cf32 items each (may be NULL where the capture produces nothing).
 * Queues one launch over all captures on the context's stream and returns; one run in flight per object. */
int  lsdr_resample_batch_run_async(lsdr_resample_batch*, const void *const *iq_dev, const lsdr_capture_each *each,
                                   lsdr_cf32 *const *out_dev, size_t cap_out);
int  lsdr_resample_batch_wait(lsdr_resample_batch*, lsdr_resample_result *results /* [B], may be NULL */);

/* ------------------------------------------------------------ spectrum batch: --cnr and --fd-spectrum for many captures
 * cnr_fft<f32> (sdr.h:1273-1345, leandvb --cnr) and spectrum<f32> (sdr.h:1347-1404, --fd-spectrum) for B captures in shared launches: any
 * of the five sample formats in, each capture with its own length and its own band centre.  One object serves both blocks; they differ in
 * nfft, kavg and what they emit.  It reads the raw capture, needs no lock and touches no decode kernel.  The single-stream objects
 * (lsdr_cnr_fft_*, lsdr_spectrum_*) stay what they are; a capture's results here are theirs bit for bit.
 *
 * THE CONTRACT: whole blocks of nfft samples only; decimation >= nfft (at most one row per block; == nfft is every block, a dense
 * waterfall); bandwidth <= 0.25; the centre is GIVEN by the caller (each[i].tune, cycles per sample: what *freq_tap·tap_multiplier is in
 * the reference — the array passed to lsdr_capture_each_run_async can be passed here unchanged); libm (logf, log10f) runs on the host.
 *
 * THE ARITHMETIC, one float32 rounding per operation (no contraction), for one capture of n items:
 *   1 J = n / nfft whole blocks; block j is the nfft samples at j·nfft.  run()'s phase counter adds nfft per block and fetches the block
 *     with which it reaches `decimation`: row m (1-based) is taken from block ceil(m·decimation/nfft) − 1, and there are
 *     floor(J·nfft/decimation) rows; consumed = J·nfft.  Both are functions of the sizes, known at run_async;
 *   2 x[k] = float(item − Z)·in_scale, exactly as the capture batch's loads convert (lsdr_capture_input_cfg);
 *   3 X = cfft_engine<float>::inplace(x, true): radix-2, the reference's butterfly (dsp.h:96-104) evaluated once per butterfly, with the
 *     host-built cosf/sinf table and the 1/n of the reverse direction — lsdr_cfft_dev's bits;
 *   4 power = re·re + im·im;  the first row sets avgpower = power and THEN, like every row, avgpower = avgpower·(1 − kavg) + power·kavg
 *     (sdr.h:1313-1320);
 *   5 bandwidth > 0: icf = floor(center·nfft + 0.5), bwslots = (int)((bandwidth/4)·nfft); the three avgslots sums (icf ± bwslots,
 *     icf − 4·bwslots … icf − 3·bwslots, icf + 3·bwslots … icf + 4·bwslots) are serial float sums in index order, indices & (nfft − 1)
 *     (sdr.h:1334-1338); the host then forms c2plusn2, n2, c2 and 10·logf(c2/n2)/logf(10), or −50 — one CNR value per row;
 *   6 emit_rows: every row's avgpower is kept in device memory (linear); the rows accessor returns 10·log10f of it, the two halves
 *     swapped as do_spectrum writes them (sdr.h:1391-1394).
 * A capture's results are a pure function of its own samples, its length and its centre — bit for bit the same alone, in any batch, in any
 * place of it, with any slab_rows and stages_per_pass, and in every format that converts to the same floats.  A run starts from fresh
 * state (a newly constructed block per capture); nothing is carried from one run to the next.
 * SLABS: the rows are worked off slab_rows at a time (three launches per slab, shared by all captures); the scratch is
 * n_captures·slab_rows·nfft floats whatever the captures' lengths, and avgpower is carried in device memory from slab to slab.
 * run_async queues everything on the context's stream and returns; wait is one event synchronisation.  One run in flight per object.
 * iq_dev: HOST array of B DEVICE pointers, each aligned to its item size (2, 2, 4, 4, 8 bytes; a 16-byte aligned capture is read by
 * 16-byte loads), NULL only where n_samples is 0.  Nothing behind a capture's last fetched block is read.
 * LSDR_E_ARG, with a message, the object (if any) left usable: n_captures outside 1 … 65535, in_format outside the five, in_scale negative
 * or not finite, nfft no power of two or outside 64 … 4096, decimation < nfft, bandwidth > 0.25 (cnr_fft's own message), negative or so
 * small that (int)((bandwidth/4)·nfft) is 0, stages_per_pass > 4, nonzero reserved (cfg or each); n_samples > max_samples, a centre not
 * finite or |centre| >= 0.5, a misaligned pointer, samples without a pointer, run_async with a run in flight, wait with none, an accessor
 * before a finished run or for what the object was not created to produce. */
typedef struct lsdr_spectrum_batch lsdr_spectrum_batch;
typedef struct {
  int n_captures;            /* B */
  size_t max_samples;        /* the longest capture a run may bring */
  int in_format;             /* LSDR_IN_CU8, _CS8, _CU16, _CS16, _CF32 */
  float in_scale;            /* as lsdr_capture_input_cfg.in_scale: 0 or 1 = none */
  int nfft;                  /* power of two, 64 … 4096 (cnr_fft: 4096, spectrum: 1024) */
  unsigned decimation;       /* samples between fetched blocks, >= nfft */
  float kavg;                /* 0: 0.1 */
  float bandwidth;           /* Fm/Fs of the CNR bands, <= 0.25; 0: no CNR */
  int emit_rows;             /* keep every row's averaged power */
  unsigned slab_rows;        /* rows per group of launches; 0: 16 Mi floats of scratch over all captures, at most a capture's rows */
  unsigned stages_per_pass;  /* radix-2 stages kept in registers between two LDS exchanges, 1 … 4; 0: 4.  The results do not depend on it */
  int reserved[5];           /* 0 */
} lsdr_spectrum_batch_cfg;   /* 72 bytes */
typedef struct {
  uint64_t consumed;         /* samples: the whole blocks */
  uint64_t rows;             /* rows produced (CNR values, kept rows) */
  int32_t icf;               /* the centre's bin, floor(center·nfft + 0.5); 0 without CNR */
  uint32_t pad[3];
} lsdr_spectrum_result;      /* 32 bytes */
int  lsdr_spectrum_batch_create(lsdr_ctx*, const lsdr_spectrum_batch_cfg*, lsdr_spectrum_batch**);
void lsdr_spectrum_batch_destroy(lsdr_spectrum_batch*);
size_t lsdr_spectrum_batch_max_rows(const lsdr_spectrum_batch*);     /* the rows of a capture of max_samples */
unsigned lsdr_spectrum_batch_slab_rows(const lsdr_spectrum_batch*);  /* slab_rows with the default filled in */
/* each[i] = {n_samples, tune}: lsdr_capture_each; tune is the band centre (read with bandwidth > 0 only, checked always) */
int  lsdr_spectrum_batch_run_async(lsdr_spectrum_batch*, const void *const *iq_dev, const lsdr_capture_each *each /* [B], host */);
int  lsdr_spectrum_batch_wait(lsdr_spectrum_batch*, lsdr_spectrum_result *results /* [B], may be NULL */);
/* after wait.  cnr: capture i's CNR values in dB, one per row (bandwidth > 0).  rows_db: its rows in dB, [rows][nfft], fftshifted
 * (emit_rows; copies the rows from the device, synchronously).  *n: what was written; LSDR_E_ARG where cap is too small.
 * rows_dev: the same rows as linear averaged power in device memory, [rows][nfft] in FFT order, valid until the next run_async; NULL
 * without emit_rows. */
int  lsdr_spectrum_batch_cnr(lsdr_spectrum_batch*, int i, float *cnr_out, size_t cap, size_t *n);
int  lsdr_spectrum_batch_rows_db(lsdr_spectrum_batch*, int i, float *rows_out, size_t cap_rows, size_t *n);
const float *lsdr_spectrum_batch_rows_dev(const lsdr_spectrum_batch*, int i);

/* ------------------------------------------------------------ TS batch: census and PID filter of many transport streams
 * What a decoded TS is worth, and the part of it a user wants, without downloading and parsing all of it.  The reference drops every
 * packet Reed-Solomon could not repair (derandomizer sets TEI and does not write it, dvb.h:1146-1156): a loss leaves no byte in the TS,
 * only a jump of the MPEG continuity counter of the PID it hit.  This object reads B finished TS buffers in device memory — the batch
 * decoders' *_ts_dev(i) or any uploaded TS, each with its own length — in shared launches and touches no decode kernel.
 *
 * THE DEFINITION (ISO 13818-1 §2.4.3).  All integers: every implementation agrees bit for bit, and a record is a pure function of the
 * stream's bytes — the same alone, in any batch and at any tile size.  Packet k of a stream is the bytes b[0 … 187] at 188·k.
 *   class    b[0] != 0x47: sync_errors, nothing else is read from the packet; else b[1] & 0x80: tei, nothing else is read (its PID cannot
 *            be trusted); else the packet is VALID.
 *   fields   of a valid packet: pid = (b[1]&0x1f)<<8 | b[2]; pusi = b[1]>>6 & 1; scrambled = (b[3]&0xc0) != 0; afc = b[3]>>4 & 3,
 *            payload = afc&1, af = afc>>1; cc = b[3]&15; af_len = af ? b[4] : 0; disc = af && af_len > 0 && (b[5]&0x80);
 *            pcr = af && af_len >= 7 && (b[5]&0x10); its value base·300 + ext, base = b[6]<<25 | b[7]<<17 | b[8]<<9 | b[9]<<1 | b[10]>>7,
 *            ext = (b[10]&1)<<8 | b[11].
 *   null     pid 0x1fff counts in null_packets and in its own record (packets, pusi, scrambled, pcr_count, first, last); it is never
 *            continuity-checked.
 *   continuity  per PID other than 0x1fff, over that PID's valid packets in stream order; the first is not judged.  For every later
 *            packet cur with predecessor prev: cur.disc → discontinuities++; otherwise expected = (prev.cc + cur.payload) & 15;
 *            cur.cc == expected is fine; else cur.payload && cur.cc == prev.cc → cc_repeats++ (the standard's legal duplicate, not
 *            judged further); else cc_errors++ and cc_missing += (cur.cc − expected) & 15.  The rule looks at the pair only.
 *   PCR      pcr_pid is the PID of the first valid packet in stream order with pcr set (−1: none); pcr_count, pcr_first, pcr_last
 *            (27 MHz ticks), pcr_first_packet and pcr_last_packet (indices among ALL packets of the stream) refer to that PID only.
 * The summary's four continuity totals run over ALL PIDs of the stream, listed or not.  The table of lsdr_ts_batch_pids holds the
 * min(pids_seen, max_pids) LOWEST PIDs in ascending order.
 * THE FILTER (a run with a rule).  A packet is kept iff `drop` does not drop it (sync-error and TEI packets by their class, null packets
 * by their PID) and it is a sync-error or TEI packet, or keep_pids is NULL, or its PID's bit is set; sync-error and TEI packets have no
 * PID, keep_pids does not apply to them.  The kept packets stand in stream order at lsdr_ts_batch_out_dev(i), kept·188 bytes; with
 * want_index, lsdr_ts_batch_index_dev(i) holds each one's index in the input.  `kept` is 0 after a run without a rule.
 * QUEUEING.  run_async queues everything on the context's stream and returns; one run in flight per object; wait is one synchronisation
 * and the read of pinned records.  download_async (after the wait of a run with a rule) copies kept·188 bytes per stream on a stream of
 * its own and may still be pending when the next run_async is queued: the kernels that write the output wait for it.
 * LIMITS: 188-byte packets only.  No PSI parsing: PAT and PMT are the user's to read from the filtered PID 0.  Continuity says how many
 * packets a PID lost modulo 16: cc_missing is a lower bound on the loss.  The per-PID counters are 32 bits wide.
 * LSDR_E_ARG, with a message naming ts_batch, the object (if any) left usable: n_streams < 1 (or above 65535), max_pids > 8192, nonzero
 * reserved, n_packets[i] > max_packets, a NULL or not 4-byte aligned pointer with packets, unknown drop bits, run_async with a run in
 * flight, wait with none, a download before the wait of a run with a rule or into cap_bytes smaller than some stream's kept bytes, i out
 * of range.  LSDR_E_UNSUPPORTED: max_packets ≥ 2^32. */
enum { LSDR_TS_DROP_NULL = 1, LSDR_TS_DROP_TEI = 2, LSDR_TS_DROP_SYNC = 4 };
typedef struct lsdr_ts_batch lsdr_ts_batch;
typedef struct { int n_streams; size_t max_packets; unsigned max_pids; /* 0: 64; at most 8192 */ int reserved[8]; } lsdr_ts_batch_cfg;
typedef struct {
  const uint8_t *keep_pids;  /* HOST; NULL: all PIDs; else n_streams × 1024 bytes, bit (pid & 7) of byte pid >> 3 of stream i's 1024 */
  unsigned drop;             /* LSDR_TS_DROP_NULL | _TEI | _SYNC */
  int want_index;
  int reserved[4];           /* 0 */
} lsdr_ts_rule;
typedef struct {
  uint64_t packets, sync_errors, tei, null_packets, valid, cc_errors, cc_repeats, cc_missing, discontinuities, kept,
           pcr_first, pcr_last, pcr_first_packet, pcr_last_packet;
  uint32_t pids_seen, pids_listed;
  int32_t pcr_pid;
  uint32_t pcr_count;
} lsdr_ts_summary;           /* 128 bytes */
typedef struct {
  uint32_t pid, packets, pusi, scrambled, cc_errors, cc_repeats, cc_missing, discontinuities, pcr_count, pad;
  uint64_t first_packet, last_packet;
} lsdr_ts_pid;               /* 56 bytes */
int  lsdr_ts_batch_create(lsdr_ctx*, const lsdr_ts_batch_cfg*, lsdr_ts_batch**);
void lsdr_ts_batch_destroy(lsdr_ts_batch*);
/* ts_dev: HOST array of DEVICE pointers, 4-byte aligned (may be NULL where n_packets is 0); n_packets: HOST; rule NULL: census only */
int  lsdr_ts_batch_run_async(lsdr_ts_batch*, const uint8_t *const *ts_dev, const uint64_t *n_packets, const lsdr_ts_rule *rule);
int  lsdr_ts_batch_wait(lsdr_ts_batch*, lsdr_ts_summary *out /* [n_streams], may be NULL */);
/* after wait: stream i's table, *n = pids_listed entries where cap allows (LSDR_E_ARG, nothing written, where it does not) */
int  lsdr_ts_batch_pids(lsdr_ts_batch*, int i, lsdr_ts_pid *out, unsigned cap, unsigned *n);
const uint8_t *lsdr_ts_batch_out_dev(const lsdr_ts_batch*, int i);     /* NULL before the first run with a rule, or i out of range */
const uint32_t *lsdr_ts_batch_index_dev(const lsdr_ts_batch*, int i);  /* NULL unless the last run's rule had want_index */
int  lsdr_ts_batch_download_async(lsdr_ts_batch*, uint8_t *const *host /* [n_streams] HOST pointers */, size_t cap_bytes);
int  lsdr_ts_batch_download_wait(lsdr_ts_batch*);
/* packets per workgroup tile: the lengths at which the kernels change their path are multiples of it */
unsigned lsdr_ts_batch_tile(const lsdr_ts_batch*);

/* ------------------------------------------------------------ TX batch: leandvbtx | leanchansim for many streams at once
 * The mirror image of lsdr_capture_batch: n_streams transport streams in device memory, each with its own length, code rate, power, noise
 * level and seed, become n_streams noisy captures in device memory in one set of launches.  Every stream is a pair of freshly started
 * processes (leandvbtx.cc:79-175, leanchansim.cc:115-189):
 *   randomizer → rs_encoder → interleaver → dvb_convol → cstln_transmitter(make_dvbs2_constellation) → fir_resampler(RRC,
 *   normalize_power(amp/75)) → decimator [→ simple_agc] | scaler(scale) → + wgn_c(stddev) → drifter with all components zero
 *   [→ cconverter<f32,0,u8,128,1,1>]
 * EXACT.  Stream i's output is bit for bit what the two programs write for that stream alone — the same alone, at any position of any
 * batch and on a reused object; a run carries nothing into the next one.  The order of operations is the reference's: AGC gain, scale,
 * + noise, the drifter's multiplication by its table entry 0 (1, 0).
 * PER STREAM.  fec: leandvbtx's rule "2/3 on QPSK and 64-ary runs as 4/6" applies; a rate the constellation cannot carry is refused with
 * the code of lsdr_convol_create.  amp: leandvbtx --power, linear.  scale: leanchansim --scale (0: 1).  noise_stddev: --awgn, linear (0 is
 * valid and still runs the adder).  seeded / seed: srand48(seed), or --deterministic's unseeded generator, as lsdr_wgn_create.
 * THE RESULT.  packets, bytes, symbols, samples: the items that left the interleaver, that the convolutional coder took, that the mapper
 * produced, that the object wrote.  noise_state: the drand48 state behind the last noise sample (the start state where samples is 0).
 * noise_rounds: the rounds of the noise stage the stream took part in (1 unless its candidates ran out, 0 without samples).
 * agc_estimated: simple_agc's estimate after the last chunk (0 without AGC).  lsdr_tx_batch_plan fills the four lengths on the host, in
 * closed form from the blocks' consumption rules (interleaver n − 11; whole groups of the coder; lsdr_fir_resampler_run's count; the
 * decimator; the AGC's whole 128-sample chunks), without a GPU or a context; run_async sizes its launches with it.
 * QUEUEING.  run_async queues everything on the context's stream and returns; between run_async and wait the host reads nothing and
 * synchronises nothing; one run in flight per object.  The number of kernel launches of a run does not depend on n_streams
 * (lsdr_tx_batch_stats).  NOISE: wgn_c's rejection step makes positions data dependent; every stream gets a candidate budget (n·4/π plus
 * `sigmas` standard deviations, 6 by default, lsdr_tx_batch_set_noise_margin) and a stream whose candidates run out is finished by further
 * rounds that wait drives; the bytes do not depend on the number of rounds.
 * OUTPUT.  The object owns the output buffers (lsdr_tx_batch_out_dev(i), 16-byte aligned, sized from max_packets at the slowest rate):
 * `samples` items of cf32 (LSDR_IN_CF32) or cu8 (LSDR_IN_CU8, leanchansim --ou8).  download_async / download_wait copy them to the host
 * on a stream of their own after wait; the next run's kernels wait for a pending download.
 * OUT OF SCOPE: the drift options (--lo, --ppm, --drift*), --s16, --fill, cu8 input of leanchansim, streams continued across runs, a
 * constellation or interp/decim per stream.
 * LSDR_E_ARG, with a message naming tx_batch, the object (if any) left usable: n_streams outside 1 … 65535, interp or decim < 1, an
 * out_format outside the two, rolloff or rrc_rej not finite or negative, nonzero reserved, n_packets > max_packets, a NULL pointer with
 * packets, amp / scale / noise_stddev not finite, a code rate the constellation cannot carry, run_async with a run in flight, wait with
 * none, a download before a wait or into too small a buffer.  LSDR_E_UNSUPPORTED: more than 1024 taps, or an interp/decim whose sample
 * tile needs more than 16384 symbols. */
typedef struct lsdr_tx_batch lsdr_tx_batch;
typedef struct {
  int n_streams;
  size_t max_packets;
  int cstln;                 /* every constellation lsdr_cstln_transmitter_run accepts */
  int interp, decim;
  float rolloff, rrc_rej;    /* 0: 0.35 and 10 */
  int agc;
  int out_format;            /* LSDR_IN_CF32 or LSDR_IN_CU8 */
  int reserved[8];           /* 0 */
} lsdr_tx_batch_cfg;
typedef struct {
  uint64_t n_packets;
  int32_t fec;
  float amp, scale, noise_stddev;
  int32_t seeded;
  int32_t reserved0;         /* 0 */
  int64_t seed;
  int32_t reserved[6];       /* 0 */
} lsdr_tx_each;              /* 64 bytes */
typedef struct {
  uint64_t packets, bytes, symbols, samples, noise_state;
  uint32_t noise_rounds;
  float agc_estimated;
  uint32_t reserved[4];
} lsdr_tx_result;            /* 64 bytes */
int  lsdr_tx_batch_create(lsdr_ctx*, const lsdr_tx_batch_cfg*, lsdr_tx_batch**);
void lsdr_tx_batch_destroy(lsdr_tx_batch*);
/* ts_dev: HOST array of n_streams DEVICE pointers (may be NULL where n_packets is 0); each: HOST [n_streams] */
int  lsdr_tx_batch_run_async(lsdr_tx_batch*, const uint8_t *const *ts_dev, const lsdr_tx_each *each);
int  lsdr_tx_batch_wait(lsdr_tx_batch*, lsdr_tx_result *results /* [n_streams], may be NULL */);
const void *lsdr_tx_batch_out_dev(const lsdr_tx_batch*, int i);            /* NULL: i out of range */
const lsdr_tx_result *lsdr_tx_batch_results_dev(const lsdr_tx_batch*);     /* [n_streams], valid after wait */
int  lsdr_tx_batch_download_async(lsdr_tx_batch*, void *const *host /* [n_streams] HOST pointers */, size_t cap_bytes);
int  lsdr_tx_batch_download_wait(lsdr_tx_batch*);
int  lsdr_tx_batch_stats(const lsdr_tx_batch*, unsigned *launches_last_run, unsigned long long *runs);
int  lsdr_tx_batch_set_noise_margin(lsdr_tx_batch*, float sigmas);         /* a negative value makes round 1 fall short (tests) */
int  lsdr_tx_batch_plan(const lsdr_tx_batch_cfg*, const lsdr_tx_each*, lsdr_tx_result*);   /* host only */
float lsdr_db_to_amplitude(double db);                                     /* expf(logf(10)*db/20): how both apps parse --power and --awgn */

/* ------------------------------------------------------------ TS stitch: the streams of a recording's overlapping pieces, joined
 * A recording longer than a batch decoder's max_samples is decoded in pieces that overlap; every piece acquires anew at its start, so
 * adjacent pieces' transport streams share a stretch of packets.  This object takes P transport streams in device memory, in recording
 * order — the batch decoders' *_ts_dev(i) or any uploaded TS, each with its own length; a length of 0 with a NULL pointer is valid —
 * finds where each continues the one before it and writes them, every packet once, into one device buffer.  It reads TS buffers and
 * touches no decode kernel.
 *
 * THE DEFINITION.  All integers: every implementation agrees bit for bit (tests/stitch_common.py restates it in numpy).
 *   the join of the pair (k, k+1).  T is the last min(W, n_k) packets of stream k, H the first min(W, n_k+1) packets of stream k+1.  A RUN
 *            is a maximal stretch of L consecutive pairs T[b+i], H[a+i] (i = 0 … L−1) whose 188 bytes are equal.  Equality is by bytes:
 *            the kernels pre-filter with a 64-bit key, a byte compare decides, a key collision can never join.  A run QUALIFIES if L ≥ M
 *            and at least ⌈M/2⌉ of its packets are not null packets (PID 0x1fff, (b[1]&0x1f)<<8 | b[2]).  The join is the longest
 *            qualifying run, ties to the smallest a, then the smallest b:
 *              joined = 1, run = L, end = (n_k − |T|) + b + L  (stream k is kept up to here), next_start = a + L  (stream k+1 from here).
 *            Without a qualifying run: joined = 0, run = 0, end = n_k, next_start = 0 — nothing is dropped and the caller is told.
 *   the kept range of stream k is [start, max(start, end)) with start = the join (k−1, k)'s next_start (0 for k = 0) and end = the join
 *            (k, k+1)'s end (n_k for k = P−1): a stream shorter than both of its overlaps keeps nothing.
 *   the output is the kept ranges one behind the other, stream 0 first: keep[k] = {start, end, out_offset}, out_offset in packets.
 * The join of a pair depends on the two streams alone: the same records alone, at any position of a larger batch and on a reused object.
 * QUEUEING.  run_async queues five launches on the context's stream — their number does not depend on P — and the records' copy, and
 * returns; the host reads nothing before wait, which is one synchronisation and the read of pinned records.  One run in flight per
 * object.  download_async (after wait) copies the output on a stream of its own and may still be pending when the next run_async is
 * queued: the kernel that writes the output waits for it.
 * The kernels read the 16-byte lines that hold a stream's first and last byte whole (a line never leaves the page its bytes are in).
 * LSDR_E_ARG, with a message naming ts_stitch, the object (if any) left usable: n_streams outside 1 … 65535, window above 65535, min_run
 * above the window, nonzero reserved, n_packets[i] > max_packets, a NULL or not 4-byte aligned pointer with packets, run_async with a run
 * in flight, wait with none, a download before a wait or into too small a buffer.  LSDR_E_UNSUPPORTED: max_packets ≥ 2^32. */
typedef struct lsdr_ts_stitch lsdr_ts_stitch;
typedef struct {
  int n_streams;
  size_t max_packets;        /* per stream; the output buffer holds n_streams × max_packets packets */
  unsigned window;           /* W; 0: 4096 */
  unsigned min_run;          /* M; 0: 8 */
  int reserved[8];           /* 0 */
} lsdr_ts_stitch_cfg;
typedef struct { uint32_t joined, run; uint64_t end, next_start; } lsdr_ts_join;   /* 24 bytes */
typedef struct { uint64_t start, end, out_offset; } lsdr_ts_keep;                  /* 24 bytes */
int  lsdr_ts_stitch_create(lsdr_ctx*, const lsdr_ts_stitch_cfg*, lsdr_ts_stitch**);
void lsdr_ts_stitch_destroy(lsdr_ts_stitch*);
/* ts_dev: HOST array of n_streams DEVICE pointers, 4-byte aligned (may be NULL where n_packets is 0); n_packets: HOST */
int  lsdr_ts_stitch_run_async(lsdr_ts_stitch*, const uint8_t *const *ts_dev, const uint64_t *n_packets);
int  lsdr_ts_stitch_wait(lsdr_ts_stitch*, lsdr_ts_join *joins /* [n_streams − 1], may be NULL */, lsdr_ts_keep *keep /* [n_streams], may be NULL */);
const uint8_t *lsdr_ts_stitch_out_dev(const lsdr_ts_stitch*);             /* (keep[P−1].out_offset + its length) × 188 bytes after wait */
int  lsdr_ts_stitch_download_async(lsdr_ts_stitch*, uint8_t *host, size_t cap_bytes);
int  lsdr_ts_stitch_download_wait(lsdr_ts_stitch*);

/* ------------------------------------------------------------ a carrier that moves: its track along the capture (QPSK)
 * The batch decoders hold every tile within ± 1/(2048·omega) cycles per sample of ONE tune per capture (the TUNING CONTRACT), and
 * lsdr_tune_est reads that one number from the capture's first blocks.  An oscillator that wanders or a pass that sweeps leaves that
 * window within the capture.  lsdr_tune_track reads the offset ALONG the capture; lsdr_derotate_batch (below) takes a track out of the
 * samples.  Both run in front of the decoders and touch none of their kernels.
 *
 * THE TRACKER.  For one capture of n items, with N = 4096:
 *   1 FRAMES.  Frame k starts at sample s_k = k·hop, for every k with s_k + blocks·N ≤ n.  If e = ⌊(n − blocks·N)/N⌋·N lies behind the
 *     last of them, one more frame starts at e: the track then reaches the capture's end.  n < blocks·N: no frame, an all-zero summary.
 *   2 SPECTRUM of a frame: steps 1 to 4 of lsdr_tune_est on the frame's `blocks` blocks — convert, divide each block by its own RMS,
 *     w = z⁴, X = FFT_N(w), P[k] = Σ_blocks |X[k]|² in block order.
 *   3 PEAK.  Frame 0, and every frame with no accepted frame in front of it, takes the first arg-max of P over all bins.  Every other frame
 *     takes the first maximum over the 2·span + 1 bins b − span … b + span (mod N), walked in that order, b the bin of the last accepted
 *     frame.  span = 0: every frame searches all bins.  c, l, r, the interpolation, tune and quality = c / mean(P over ALL bins) are
 *     lsdr_tune_est's step 5 and 7 on the peak's cyclic neighbours (which may lie outside the gate).
 *   4 ACCEPT OR HOLD.  A frame with quality ≥ min_quality is accepted.  Any other frame is held: its record is written with held = 1, it
 *     is no knot of the track, and it does not move b.
 * A frame's record carries center = s_k + blocks·N/2, the sample its tune belongs to.  The summary is taken over the accepted frames in
 * frame order.  With `blocks` equal on both sides, frame 0's record is lsdr_tune_est's record of the same capture, field for field and
 * bit for bit.  The accepted frames' (center, tune) are the knots lsdr_derotate_batch takes.
 * LIMITS: QPSK only; |f| < 1/8; a narrow-band interferer inside the gate wins the peak; the carrier should move by less than about one bin
 * of the fourth power per block inside a frame (1.5e-8 cycles per sample²), or the line smears over the frame's blocks.
 * A capture's records are a pure function of its converted samples: no atomics, every sum in a fixed order — bit for bit the same alone,
 * in any batch, at any place of it, and in every format that converts to the same floats.
 * run_async queues everything on the context's stream and returns: one launch over all blocks of all frames of all captures (one
 * workgroup per block; blocks × 16 KB of scratch per frame), one over the frames (a frame's rows summed in block order, its first maximum
 * over all bins), one over the captures (one workgroup walks a capture's frames in order: the gate makes that serial, and only the gate's
 * 2·span + 1 bins are read there), the records' copy to pinned memory.  wait is one event synchronisation and the read of the records.  One run in
 * flight per object.  Pointers as for lsdr_tune_est; nothing behind a capture's last whole block is read.
 * LSDR_E_ARG, with a message, the object (if any) left usable: n_captures outside 1 … 65535, in_format outside the five LSDR_IN_*,
 * in_scale or min_quality negative or not finite, blocks > 16, hop not a multiple of 4096, span > 2047, nonzero reserved; a capture with
 * more than max_frames frames (checked before anything is queued), a misaligned pointer, samples without a pointer, run_async with a run
 * in flight, wait with none. */
typedef struct lsdr_tune_track lsdr_tune_track;
typedef struct {
  int n_captures;      /* B */
  int in_format;       /* LSDR_IN_CU8, _CS8, _CU16, _CS16, _CF32 */
  float in_scale;      /* as lsdr_tune_est_cfg.in_scale */
  unsigned blocks;     /* blocks of 4096 samples per frame, at most 16; 0 = 4 */
  unsigned hop;        /* samples between two frames' starts, a multiple of 4096; 0 = 65536 */
  unsigned span;       /* the gate: ± span bins of 1/(4·4096) cycles per sample around the last accepted peak, at most 2047; 0 = no gate */
  float min_quality;   /* a frame below it is held; 0 = 30 */
  unsigned max_frames; /* of one capture; 0 = 256.  Scratch: n_captures × max_frames × blocks rows of 16 KB */
  int reserved[4];     /* 0 */
} lsdr_tune_track_cfg; /* 48 bytes */
typedef struct {
  uint64_t center;     /* s_k + blocks·4096/2: the sample the frame's tune belongs to */
  float tune;          /* cycles per sample, as lsdr_tune_estimate.tune */
  float quality;       /* power[1] / mean_power */
  uint32_t bin;        /* the peak's bin, 0 … 4095 */
  uint32_t held;       /* 1: quality < min_quality — no knot, the gate stays */
  float power[3];      /* l, c, r */
  float mean_power;    /* mean(P) over all bins */
} lsdr_track_frame;    /* 40 bytes */
typedef struct {
  uint32_t frames, accepted;
  float tune_first, tune_last, tune_min, tune_max, quality_min;   /* over the accepted frames; all zero where there is none */
} lsdr_track_summary;  /* 28 bytes */
int lsdr_tune_track_create(lsdr_ctx *ctx, const lsdr_tune_track_cfg *cfg, lsdr_tune_track **t);
void lsdr_tune_track_destroy(lsdr_tune_track *t);
unsigned lsdr_tune_track_max_frames(const lsdr_tune_track *t);      /* with the default filled in */
int lsdr_tune_track_run_async(lsdr_tune_track *t, const void *const *iq_dev, const size_t *n_samples /* [B], host */);
/* frames: [B][max_frames], capture i's records at frames[i·max_frames … + summary[i].frames); may be NULL */
int lsdr_tune_track_wait(lsdr_tune_track *t, lsdr_track_summary *summary /* [B] */, lsdr_track_frame *frames);

/* ------------------------------------------------------------ a track, given, taken out of the samples
 * lsdr_derotate_batch multiplies every capture by exp(−j·2π·φ(n)), φ the integral of a piecewise-linear frequency track, and writes cf32
 * items that lsdr_capture_batch decodes as LSDR_IN_CF32 (in_scale 1) with tune 0.  The track is GIVEN by the caller as knots
 * (sample, tune), exactly as lsdr_capture_each.tune is given: from lsdr_tune_track's accepted frames, from an orbit prediction, or from a
 * smoothing of either.  Per capture: samples strictly ascending and below 2^31, |tune| < 0.5, |Δtune| between neighbours < 0.5.
 *
 * THE DEFINITION.  All phase arithmetic is in integers, in units of 2^-64 cycle, wrapping modulo 2^64 (tests/track_common.py restates it
 * in Python integers):
 *   frequency word  F_i = (int64) of ldexp(tune_i, 64) rounded to nearest (for |tune| > 2^-11 the double is a whole number already);
 *   slope of segment i, between knot i and knot i + 1:  S_i = floor((F_{i+1} − F_i) / (sample_{i+1} − sample_i)), signed floor division;
 *   outside the knots the first segment's slope runs back to sample 0 and the last one's runs on to the end: where knot 0 is not on
 *     sample 0, the library puts a knot at sample 0 with F = F_0 − S_0·sample_0, and the last knot starts a segment with the slope in
 *     front of it.  One knot: a constant frequency.  No knots: F = 0, the capture passes through converted;
 *   phase  φ(n) = Φ_i + F_i·m + S_i·(m(m − 1)/2), m = n − sample_i, i the last knot at or before n; Φ at sample 0 is 0 and
 *     Φ_{i+1} = φ_i(sample_{i+1}): the phase is continuous, the frequency steps by less than sample_{i+1} − sample_i units at a knot;
 *   rotation  (c, s) = lsdr_trig16_table's entry φ(n) >> 48: cosf / sinf of 2π·index/65536;
 *   output  out.re = xr·c + xi·s, out.im = xi·c − xr·s in float32, every product and sum rounded on its own; x the converted sample,
 *     float(item − Z)·in_scale.
 * The sign is lsdr_capture_each.tune's: a capture multiplied by exp(+j2π·Σf) comes back with knots of +f.
 * The host turns a capture's knots into its (Φ, F, S) table and uploads it with the run; one launch covers all captures, every one with
 * its own length; 16-byte loads (where the capture's pointer is 16-byte aligned) and 16-byte stores.  Nothing behind item n − 1 is read
 * or written.  A capture's output is a pure function of its samples and its knots.  One run in flight per object.
 * The cf32 copy costs 8 bytes of device memory per sample.  What is left of the carrier after the derotation must still fit the decoder's
 * tuning window.
 * LSDR_E_ARG, with a message, the object left usable: knots out of order, a knot's sample ≥ 2^31, a tune not finite or outside
 * (−0.5, 0.5), a step of 0.5 or more between neighbours, a pointer not aligned to its item, an output pointer not aligned to 16 bytes,
 * samples without a pointer, n_samples above max_samples, more than max_knots knots, a table above 2^22 segments at create, nonzero
 * reserved, run_async with a run in flight, wait with none. */
typedef struct lsdr_derotate_batch lsdr_derotate_batch;
typedef struct { uint64_t sample; double tune; } lsdr_track_knot;   /* 16 bytes */
typedef struct {
  int n_captures;      /* B, 1 … 65535 */
  int in_format;       /* LSDR_IN_CU8, _CS8, _CU16, _CS16, _CF32 */
  float in_scale;      /* as lsdr_capture_input_cfg.in_scale: 0 or 1 = none */
  unsigned max_knots;  /* of one capture, at most 2^20; n_captures × (max_knots + 1) at most 2^22 (32 bytes of table each) */
  size_t max_samples;  /* of one capture */
  int reserved[4];     /* 0 */
} lsdr_derotate_batch_cfg;  /* 40 bytes */
typedef struct {
  size_t n_samples;
  const lsdr_track_knot *knots;   /* HOST, n_knots of them; read during run_async only */
  unsigned n_knots;
  unsigned reserved;   /* 0 */
} lsdr_derotate_each;  /* 24 bytes */
int lsdr_derotate_batch_create(lsdr_ctx *ctx, const lsdr_derotate_batch_cfg *cfg, lsdr_derotate_batch **b);
void lsdr_derotate_batch_destroy(lsdr_derotate_batch *b);
/* iq_dev, out_dev: HOST arrays of B DEVICE pointers; out_dev[i] 16-byte aligned with room for each[i].n_samples items */
int lsdr_derotate_batch_run_async(lsdr_derotate_batch *b, const void *const *iq_dev, const lsdr_derotate_each *each /* [B], host */,
                                  lsdr_cf32 *const *out_dev);
int lsdr_derotate_batch_wait(lsdr_derotate_batch *b);

#ifdef __cplusplus
}
#endif
#endif /* LSDR_HIP_H */
