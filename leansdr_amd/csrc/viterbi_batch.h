// leansdr_amd/csrc/viterbi_batch.h — lsdr_viterbi_batch: B independent viterbi_sync decoders (dvb.h:1173-1416) in shared launches.
// Included at the end of viterbi.hip (it uses that file's kernels, job format and tables).
//
// One run = a fixed sequence of launches on the context's stream, whatever the number of streams and whatever the data:
//   [k_vitb_prep]            only with device-side counts: clips every stream's chunk count
//   trellis                  every stream's tiles, the main alignment's and the other alignments', in ONE launch (BATCH kernels)
//   R × (verify, re-run)     seam check, then the job list once more with the flags as a predicate (vit_args::cond)
//   verify                   the flags the decision relies on
//   k_vitb_decide            one wavefront per stream: committable prefix, alignment decision, carried states, result record
// The host plans the tiles from LENGTHS only (and from the alignment / resync phase the previous wait returned) and reads nothing
// between run_async and wait.
//
// Exactness: tile 0 of a stream starts from the carried state; tile k is exact when tile k−1 is and its start state (recorded in
// begin_states[k], whatever it was read from) equals end_states[k−1] as it stands after the last launch.  The decision kernel
// commits the chunks in front of the first seam — of any alignment — that does not verify, or up to the first resync chunk whose
// decision changes the alignment (dvb.h:1402-1411), and carries exactly the decoder states of that point into the next call.
// Everything behind the prefix is decoded again by the next call; nothing unverified is ever committed, so no sequential path and no
// host-side repair exist here.

namespace {

constexpr int kVitbRounds = 2;   // device repair rounds per run.  One round settles every failed seam of the bench's and the tests' streams
                                 // at the default warm-up (viterbi.hip: "a call whose failed seams settle in one round"); a tile whose end
                                 // state changed in round 1 fails the NEXT seam, which round 2 repairs.  What is still open after that
                                 // stalls the stream there for this run (lsdr_viterbi_batch_result::stalled), it never costs a wrong byte.
constexpr int kVitbMaxRounds = 6;   // (what lsdr_viterbi_run allows; upper bound of the LSDR_VITB_ROUNDS hook)
constexpr unsigned kVitbWarmOthers = 12;   // warm-up (resync chunks) of the other alignments' tiles: "with 12 none [failed] in the bench's streams"

struct vitb_plan {               // one stream's part of the job list (host-planned), for the decision kernel
  unsigned main0, n_main;        // slots of the main alignment's tiles
  unsigned oth0, n_oth;          // slots of the other alignments' tiles
  unsigned long long r0;         // first resync chunk of the run
  unsigned nrs;                  // planned resync chunks
  int cur;                       // alignment in force
};

// device-side symbol counts → chunk counts (dvb.h:1372-1373), never more than the host planned
__global__ void k_vitb_prep(vit_bstream *streams, const unsigned long long *n_in_dev, unsigned n, unsigned sym_per_chunk, unsigned extra) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long m = n_in_dev[i];
  const unsigned long long ch = m < (unsigned long long)sym_per_chunk + extra ? 0ull : (m - extra) / sym_per_chunk;
  if (ch < streams[i].chunks) streams[i].chunks = ch;
}

// seam check of every job that continues its predecessor's slot (from_state < 0) and has work in this run
__global__ __launch_bounds__(64) void k_vitb_verify(const vit_job *jobs, const vit_bstream *streams, const vit_state *begin_states,
                                                    const vit_state *end_states, unsigned njobs, int *bad) {
  const unsigned j = blockIdx.x;
  if (j >= njobs) return;
  const int lane = threadIdx.x;
  const vit_job job = jobs[j];
  int flag = 0;
  if (j > 0 && job.from_state < 0 && job.first_chunk < streams[job.stream].chunks) {
    const bool same = begin_states[j].cost[lane] == end_states[j - 1].cost[lane] && begin_states[j].path[lane] == end_states[j - 1].path[lane];
    flag = __all(same) ? 0 : 1;
  }
  if (lane == 0) bad[j] = flag;
}

// One wavefront per stream.  bad: [rounds + 1][njobs] — the flags each repair round acted on, then the final ones.
__global__ __launch_bounds__(64) void k_vitb_decide(const vit_job *jobs, const vit_bstream *streams, const vitb_plan *plans, const int *bad,
                                                    unsigned njobs, int rounds, const vit_state *end_states, const int *r_totals,
                                                    const vit_state *r_states, vit_state *carried, int nsyncs, int period,
                                                    unsigned sym_per_chunk, unsigned bytes_per_chunk, lsdr_viterbi_batch_result *results) {
  const unsigned i = blockIdx.x;
  const int lane = threadIdx.x;
  const vit_bstream S = streams[i];
  const vitb_plan P = plans[i];
  const int *fin = bad + (size_t)rounds * njobs;
  const unsigned chunks = (unsigned)S.chunks;
  // ---- end of the verified work: the first seam that still fails, of the main alignment's tiles or of another alignment's
  unsigned E = chunks, repaired = 0;
  for (unsigned k = lane; k < P.n_main + P.n_oth; k += 64) {
    const unsigned slot = k < P.n_main ? P.main0 + k : P.oth0 + (k - P.n_main);
    if (fin[slot]) { const unsigned fc = (unsigned)jobs[slot].first_chunk; E = fc < E ? fc : E; }
    for (int r = 0; r < rounds; ++r) repaired += bad[(size_t)r * njobs + slot] ? 1u : 0u;
  }
  E = (unsigned)wave_min((int)E);
  for (int o = 32; o; o >>= 1) repaired += __shfl_xor(repaired, o, 64);
  // the prefix ends where a main tile starts (a failed seam of another alignment sits on a resync chunk, which starts a main tile
  // unless tile 0 was extended over it): the last tile start at or below E, and the slot of the tile in front of it
  unsigned last_first = 0, last_slot = P.main0;     // last tile that starts below the end of the prefix
  const bool stalled = E < chunks;
  if (stalled) {
    int best = 0;
    for (unsigned k = lane; k < P.n_main; k += 64) { const unsigned fc = (unsigned)jobs[P.main0 + k].first_chunk; if (fc <= E && (int)fc > best) best = (int)fc; }
    E = (unsigned)(-wave_min(-best));
  }
  {
    int best = 0;                                   // (tiles ascend with their first chunk: the highest index below E)
    for (unsigned k = lane; k < P.n_main; k += 64) if ((unsigned)jobs[P.main0 + k].first_chunk < E && (int)k > best) best = (int)k;
    best = -wave_min(-best);
    last_slot = P.main0 + (unsigned)best;
    last_first = (unsigned)jobs[last_slot].first_chunk;
  }
  (void)last_first;
  // ---- alignment decisions of the resync chunks below E, in order (dvb.h:1402-1411): ascending s from best = current, strict '>'
  unsigned n_r = 0;                                 // resync chunks below E
  if (P.nrs && P.r0 < E) { n_r = (unsigned)((E - 1 - P.r0) / (unsigned)period) + 1u; if (n_r > P.nrs) n_r = P.nrs; }
  int sw_r = -1, new_sync = P.cur;
  if (nsyncs > 1) {
    for (unsigned rb = 0; rb < n_r && sw_r < 0; rb += 64) {
      const unsigned r = rb + (unsigned)lane;
      int best = P.cur;
      if (r < n_r) {
        const int *t = r_totals + ((size_t)S.rbase + r) * (unsigned)nsyncs;
        int bt = t[P.cur];
        for (int s = 0; s < nsyncs; ++s) { const int ts = t[s]; if (ts > bt) { best = s; bt = ts; } }
      }
      const unsigned long long m = __ballot(best != P.cur);
      if (m) {
        const int l = __ffsll((long long)m) - 1;
        sw_r = (int)rb + l;
        new_sync = __shfl(best, l, 64);
      }
    }
  }
  // ---- result and carried states
  unsigned used = E;
  vit_state *mine = carried + (size_t)i * (unsigned)nsyncs;
  if (sw_r >= 0) {
    // everything behind this chunk belongs to the new alignment; every decoder as of the end of the deciding chunk
    used = (unsigned)(P.r0 + (unsigned long long)sw_r * (unsigned)period) + 1u;
    const vit_state *row = r_states + ((size_t)S.rbase + (unsigned)sw_r) * (unsigned)nsyncs;
    for (int s = 0; s < nsyncs; ++s) { mine[s].cost[lane] = row[s].cost[lane]; mine[s].path[lane] = row[s].path[lane]; }
  } else if (used) {
    mine[P.cur].cost[lane] = end_states[last_slot].cost[lane]; mine[P.cur].path[lane] = end_states[last_slot].path[lane];
    if (n_r && nsyncs > 1) {                        // the other alignments see the resync chunks only: their state after the last one
      const vit_state *row = r_states + ((size_t)S.rbase + (n_r - 1)) * (unsigned)nsyncs;
      for (int s = 0; s < nsyncs; ++s)
        if (s != P.cur) { mine[s].cost[lane] = row[s].cost[lane]; mine[s].path[lane] = row[s].path[lane]; }
    }
  }
  if (lane == 0) {
    lsdr_viterbi_batch_result R;
    R.consumed = (unsigned long long)used * sym_per_chunk;
    R.produced = (unsigned long long)used * bytes_per_chunk;
    R.current_sync = (unsigned)new_sync;
    R.resync_phase = (unsigned)(((unsigned long long)S.phase0 + used) % (unsigned)period);
    R.switched = sw_r >= 0 ? 1u : 0u;
    R.stalled = (sw_r < 0 && stalled) ? 1u : 0u;
    R.tiles = P.n_main + P.n_oth;
    R.repaired = repaired;
    results[i] = R;
  }
}

}  // namespace

struct lsdr_viterbi_batch {
  lsdr_ctx *ctx;
  lsdr_viterbi *v;                 // tables, alignment maps and the kernel checks of the single-stream decoder (its run path is not used)
  int n;
  size_t max_symbols, max_chunks;
  unsigned rows_per_stream;        // rows of r_totals / r_states per stream at the current resync period
  struct host_stream { int cur, phase; size_t budget; };
  std::vector<host_stream> hs;     // what the previous wait returned: alignment, resync phase; look-ahead budget
  vit_state *d_states;             // [n][nsyncs] carried decoder states
  vit_bstream *d_streams;
  vitb_plan *d_plans;
  lsdr_viterbi_batch_result *d_results;
  int *d_rtotals; vit_state *d_rstates;
  vit_job *d_jobs; vit_state *d_begin, *d_end; int *d_bad;
  size_t jobs_cap;
  bool in_flight;
  unsigned launches_last;
  unsigned long long runs;
  std::vector<vit_job> jobs;       // (kept between runs: no allocation on the submit path)
  std::vector<vit_bstream> streams;
  std::vector<vitb_plan> plans;
};

static int vitb_alloc_rows(lsdr_viterbi_batch *b) {
  lsdr_viterbi *v = b->v;
  (void)hipFree(b->d_rtotals); (void)hipFree(b->d_rstates);
  b->d_rtotals = nullptr; b->d_rstates = nullptr;
  b->rows_per_stream = (unsigned)(b->max_chunks / (size_t)v->resync_period + 2);
  const size_t rows = (size_t)b->rows_per_stream * (size_t)b->n * (size_t)v->nsyncs;
  LSDR_HIP(hipMalloc((void **)&b->d_rtotals, rows * sizeof(int)));
  LSDR_HIP(hipMalloc((void **)&b->d_rstates, rows * sizeof(vit_state)));
  return LSDR_OK;
}

extern "C" {

int lsdr_viterbi_batch_create(lsdr_ctx *c, int cstln, int rate, int n_streams, size_t max_symbols, lsdr_viterbi_batch **out) {
  LSDR_ARG(c && out && n_streams >= 1 && max_symbols >= 1);
  lsdr_viterbi *v = nullptr;
  LSDR_TRY(lsdr_viterbi_create(c, cstln, rate, &v));     // (the same error classes for unsupported constellations and rates)
  const size_t spc = (size_t)v->nshifts * kChunkBlocks;
  if (max_symbols / spc >= ((size_t)1 << 30)) { lsdr_viterbi_destroy(v); lsdr_set_error("viterbi_batch: max_symbols too large"); return LSDR_E_ARG; }
  lsdr_viterbi_batch *b = new lsdr_viterbi_batch();
  b->ctx = c; b->v = v; b->n = n_streams; b->max_symbols = max_symbols; b->max_chunks = max_symbols / spc;
  b->hs.assign(n_streams, {0, 0, (size_t)1 << 40});
  b->d_states = nullptr; b->d_streams = nullptr; b->d_plans = nullptr; b->d_results = nullptr; b->d_rtotals = nullptr; b->d_rstates = nullptr;
  b->d_jobs = nullptr; b->d_begin = b->d_end = nullptr; b->d_bad = nullptr; b->jobs_cap = 0;
  b->in_flight = false; b->launches_last = 0; b->runs = 0;
  int rc = LSDR_OK;
  auto alloc = [&]() -> int {
    const size_t ns = (size_t)n_streams * v->nsyncs * sizeof(vit_state);
    LSDR_HIP(hipMalloc((void **)&b->d_states, ns));
    LSDR_HIP(hipMemset(b->d_states, 0, ns));
    LSDR_HIP(hipMalloc((void **)&b->d_streams, n_streams * sizeof(vit_bstream)));
    LSDR_HIP(hipMalloc((void **)&b->d_plans, n_streams * sizeof(vitb_plan)));
    LSDR_HIP(hipMalloc((void **)&b->d_results, n_streams * sizeof(lsdr_viterbi_batch_result)));
    LSDR_HIP(hipMemset(b->d_results, 0, n_streams * sizeof(lsdr_viterbi_batch_result)));
    return vitb_alloc_rows(b);
  };
  rc = alloc();
  if (rc) { lsdr_viterbi_batch_destroy(b); return rc; }
  *out = b;
  return LSDR_OK;
}

void lsdr_viterbi_batch_destroy(lsdr_viterbi_batch *b) {
  if (!b) return;
  (void)hipStreamSynchronize(b->ctx->stream);
  if (b->in_flight) { b->ctx->stage_pending.clear(); b->in_flight = false; }
  (void)hipFree(b->d_states); (void)hipFree(b->d_streams); (void)hipFree(b->d_plans); (void)hipFree(b->d_results);
  (void)hipFree(b->d_rtotals); (void)hipFree(b->d_rstates);
  (void)hipFree(b->d_jobs); (void)hipFree(b->d_begin); (void)hipFree(b->d_end); (void)hipFree(b->d_bad);
  lsdr_viterbi_destroy(b->v);
  delete b;
}

int lsdr_viterbi_batch_set_resync_period(lsdr_viterbi_batch *b, int period) {
  LSDR_ARG(b && period >= 1);
  if (b->in_flight) { lsdr_set_error("viterbi_batch: a run is in flight (call lsdr_viterbi_batch_wait first)"); return LSDR_E_ARG; }
  LSDR_HIP(hipSetDevice(b->ctx->device));
  LSDR_HIP(hipStreamSynchronize(b->ctx->stream));
  b->v->resync_period = period;
  return vitb_alloc_rows(b);
}

int lsdr_viterbi_batch_reset(lsdr_viterbi_batch *b, int i) {
  LSDR_ARG(b && i < b->n);
  if (b->in_flight) { lsdr_set_error("viterbi_batch: a run is in flight (call lsdr_viterbi_batch_wait first)"); return LSDR_E_ARG; }
  LSDR_HIP(hipSetDevice(b->ctx->device));
  const size_t one = (size_t)b->v->nsyncs * sizeof(vit_state);
  if (i < 0) LSDR_HIP(hipMemsetAsync(b->d_states, 0, one * b->n, b->ctx->stream));
  else LSDR_HIP(hipMemsetAsync(b->d_states + (size_t)i * b->v->nsyncs, 0, one, b->ctx->stream));
  for (int k = 0; k < b->n; ++k) if (i < 0 || k == i) b->hs[k] = {0, 0, (size_t)1 << 40};
  return LSDR_OK;
}

int lsdr_viterbi_batch_run_async(lsdr_viterbi_batch *b, const lsdr_softsymbol *const *in_dev, const size_t *n_in, const uint64_t *n_in_dev,
                                 uint8_t *const *out_dev, size_t cap_out) {
  LSDR_ARG(b && in_dev && n_in && out_dev);
  if (b->in_flight) { lsdr_set_error("viterbi_batch: a run is in flight (call lsdr_viterbi_batch_wait first)"); return LSDR_E_ARG; }
  lsdr_viterbi *v = b->v;
  lsdr_ctx *c = b->ctx;
  const vit_code &C = v->C;
  const size_t spc = (size_t)v->nshifts * kChunkBlocks, bpc = (size_t)C.bits_in * kChunkBlocks / 8;
  const int P = v->resync_period, ns = v->nsyncs;
  // ---- chunks per stream, from the lengths (dvb.h:1372-1373) and the look-ahead budget (work behind an alignment switch is thrown away)
  b->streams.resize(b->n); b->plans.resize(b->n);
  size_t total_chunks = 0, total_rs = 0;
  for (int i = 0; i < b->n; ++i) {
    LSDR_ARG(n_in[i] <= b->max_symbols);
    size_t chunks = n_in[i] < spc + (size_t)(v->nshifts - 1) ? 0 : (n_in[i] - (size_t)(v->nshifts - 1)) / spc;
    if (chunks > cap_out / bpc) chunks = cap_out / bpc;
    if (chunks > b->hs[i].budget) chunks = b->hs[i].budget;
    LSDR_ARG(((uintptr_t)out_dev[i] & 3u) == 0);
    if (chunks) LSDR_ARG(in_dev[i] && out_dev[i]);
    vit_bstream &S = b->streams[i];
    S.in = in_dev[i]; S.out = out_dev[i]; S.states = b->d_states + (size_t)i * ns; S.chunks = chunks;
    S.phase0 = b->hs[i].phase; S.rbase = (unsigned)i * b->rows_per_stream;
    vitb_plan &pl = b->plans[i];
    pl.cur = b->hs[i].cur;
    pl.r0 = (unsigned long long)((P - S.phase0) % P);
    pl.nrs = pl.r0 < chunks ? (unsigned)((chunks - 1 - pl.r0) / (unsigned)P) + 1u : 0u;
    total_chunks += chunks; total_rs += pl.nrs;
  }
  LSDR_HIP(hipSetDevice(c->device));
  // ---- kernel and tile length, from the batch's total (viterbi_run_aligned's rules: see there)
  unsigned TL = (unsigned)P;
  if (P >= 8) { TL = 8; while (TL < 32 && P % (int)(TL * 2) == 0) TL *= 2; }
  const bool generic_only = getenv("LSDR_VIT_GENERIC") != nullptr, lane_only = getenv("LSDR_VIT_LANE") != nullptr;
  const bool q4 = v->q4 && !generic_only && !lane_only &&
                  (getenv("LSDR_VIT_Q4") != nullptr || total_chunks >= (size_t)c->num_cu * 4 / 2 * 12 * 8);
  {
    const int forced = getenv("LSDR_VIT_TL") ? atoi(getenv("LSDR_VIT_TL")) : 0;
    const size_t want = q4 ? (size_t)c->num_cu * 4 / 2 * 12 : (size_t)c->num_cu * 4 * 3 / 2;
    const unsigned tl_min = q4 ? 4u : 1u;
    if (forced > 0) TL = (unsigned)forced;
    else while (TL > tl_min && TL % 2 == 0 && total_chunks / TL < want) TL /= 2;
  }
  unsigned TLo = 4;
  for (unsigned t = 32; t >= 8; t /= 2)
    if ((size_t)(ns - 1) * ((total_rs + t - 1) / t) >= 1024) { TLo = t; break; }
  const int wo_env = getenv("LSDR_VIT_WO") ? atoi(getenv("LSDR_VIT_WO")) : 0;
  const unsigned Wo = wo_env > 0 ? (unsigned)wo_env : kVitbWarmOthers < (unsigned)kWarm ? (unsigned)kWarm : kVitbWarmOthers;
  if (q4) while (TLo > 4 && (TLo + Wo) * 23 > (TL + (unsigned)kWarm) * 22) TLo /= 2;
  int rounds = kVitbRounds;
  if (const char *e = getenv("LSDR_VITB_ROUNDS")) { rounds = atoi(e); if (rounds < 0) rounds = 0; if (rounds > kVitbMaxRounds) rounds = kVitbMaxRounds; }   // test hook, read per call
  // ---- jobs: every stream's main tiles first, then every stream's tiles of the other alignments (k_viterbi_q4 keeps the two
  // kinds in separate wavefronts).  slot = index in the list; a job with from_state < 0 continues the slot before it.
  std::vector<vit_job> &jobs = b->jobs;
  jobs.clear();
  for (int i = 0; i < b->n; ++i) {
    const size_t chunks = (size_t)b->streams[i].chunks;
    vitb_plan &pl = b->plans[i];
    pl.main0 = (unsigned)jobs.size();
    unsigned long long cstart = 0, next_rs = pl.r0;
    while (cstart < chunks) {
      while (next_rs <= cstart) next_rs += (unsigned)P;      // first resync chunk beyond cstart
      unsigned long long cend = cstart + TL;
      if (cend > next_rs) cend = next_rs;
      if (cend > chunks) cend = chunks;
      vit_job j;
      j.first_chunk = cstart; j.n_chunks = (unsigned)(cend - cstart);
      j.warm = cstart == 0 ? 0u : (unsigned)(cstart < (unsigned long long)kWarm ? cstart : (unsigned long long)kWarm);
      j.sync = pl.cur; j.from_state = cstart == 0 ? pl.cur : -1; j.emit = 1; j.chunk_step = 1; j.slot = (unsigned)jobs.size(); j.stream = (unsigned)i;
      if (cstart != 0 && j.warm < (unsigned)kWarm) jobs.back().n_chunks += j.n_chunks;      // cannot warm up fully: extends tile 0
      else jobs.push_back(j);
      cstart = cend;
    }
    pl.n_main = (unsigned)jobs.size() - pl.main0;
  }
  const size_t n_main_all = jobs.size();
  for (int i = 0; i < b->n; ++i) {
    vitb_plan &pl = b->plans[i];
    pl.oth0 = (unsigned)jobs.size();
    if (ns > 1)
      for (int s = 0; s < ns; ++s) {
        if (s == pl.cur) continue;
        unsigned r0 = 0;
        while (r0 < pl.nrs) {
          unsigned r1 = r0 + TLo;
          if (r0 == 0 && r1 < Wo + TLo) r1 = Wo + TLo;       // tile 0 is long enough for tile 1 to warm up fully
          if (r1 > pl.nrs) r1 = pl.nrs;
          vit_job j;
          j.first_chunk = pl.r0 + (unsigned long long)r0 * (unsigned)P; j.n_chunks = r1 - r0; j.warm = r0 == 0 ? 0u : Wo; j.sync = s;
          j.from_state = r0 == 0 ? s : -1; j.emit = 0; j.chunk_step = (unsigned)P; j.slot = (unsigned)jobs.size(); j.stream = (unsigned)i;
          jobs.push_back(j);
          r0 = r1;
        }
      }
    pl.n_oth = (unsigned)jobs.size() - pl.oth0;
  }
  const size_t nj = jobs.size();
  b->launches_last = 0;
  if (b->jobs_cap < nj + 1) {
    LSDR_HIP(hipStreamSynchronize(c->stream));
    (void)hipFree(b->d_jobs); (void)hipFree(b->d_begin); (void)hipFree(b->d_end); (void)hipFree(b->d_bad);
    b->d_jobs = nullptr; b->d_begin = b->d_end = nullptr; b->d_bad = nullptr; b->jobs_cap = 0;
    const size_t cap = nj + nj / 4 + 64;
    LSDR_HIP(hipMalloc((void **)&b->d_jobs, cap * sizeof(vit_job)));
    LSDR_HIP(hipMalloc((void **)&b->d_begin, cap * sizeof(vit_state)));
    LSDR_HIP(hipMalloc((void **)&b->d_end, cap * sizeof(vit_state)));
    LSDR_HIP(hipMalloc((void **)&b->d_bad, (size_t)(kVitbMaxRounds + 1) * cap * sizeof(int)));
    b->jobs_cap = cap;
  }
  LSDR_TRY(lsdr_stage_h2d(c, b->d_streams, b->streams.data(), (size_t)b->n * sizeof(vit_bstream)));
  LSDR_TRY(lsdr_stage_h2d(c, b->d_plans, b->plans.data(), (size_t)b->n * sizeof(vitb_plan)));
  LSDR_TRY(lsdr_stage_h2d(c, b->d_jobs, jobs.data(), nj * sizeof(vit_job)));
  if (n_in_dev) {
    hipLaunchKernelGGL(k_vitb_prep, dim3((unsigned)((b->n + 63) / 64)), dim3(64), 0, c->stream, b->d_streams,
                       (const unsigned long long *)n_in_dev, (unsigned)b->n, (unsigned)spc, (unsigned)(v->nshifts - 1));
    ++b->launches_last;
  }
  if (nj) {
    vit_args a;
    memset(&a, 0, sizeof(a));
    a.T = v->d_T; a.C = C; a.bits_per_symbol = v->bits_per_symbol; a.nshifts = v->nshifts;
    a.resync_period = P; a.maps = v->d_maps; a.shifts = v->d_shifts;
    a.jobs = b->d_jobs; a.njobs = (unsigned)nj;
    a.begin_states = b->d_begin; a.end_states = b->d_end;
    a.totals_stride = 1;
    a.q4_n_main = (unsigned)n_main_all; a.q4_main_waves = (a.q4_n_main + 15u) / 16u;
    a.streams = b->d_streams; a.r_totals = b->d_rtotals; a.r_states = b->d_rstates; a.nsyncs = ns;
    const dim3 grid((unsigned)((nj + kVitWaves - 1) / kVitWaves)), block(kVitWaves * 64);
    auto lane_launch = [&](const vit_args &x) {
      if (x.C.nus == 2 && x.C.bits_out == 2 && !generic_only) hipLaunchKernelGGL((k_viterbi<2, true>), grid, block, 0, c->stream, x);
      else if (x.C.nus == 4 && x.C.bits_out == 3 && !generic_only) hipLaunchKernelGGL((k_viterbi<4, true>), grid, block, 0, c->stream, x);
      else hipLaunchKernelGGL((k_viterbi<0, true>), grid, block, 0, c->stream, x);
    };
    if (q4) {
      const unsigned waves = a.q4_main_waves + (a.njobs - a.q4_n_main + 15u) / 16u;
      if (C.nus == 2) hipLaunchKernelGGL((k_viterbi_q4<2, true>), dim3(waves), dim3(64), 0, c->stream, a);
      else hipLaunchKernelGGL((k_viterbi_q4<4, true>), dim3(waves), dim3(64), 0, c->stream, a);
    } else lane_launch(a);
    ++b->launches_last;
    for (int r = 0; r <= rounds; ++r) {
      int *flags = b->d_bad + (size_t)r * nj;
      hipLaunchKernelGGL(k_vitb_verify, dim3((unsigned)nj), dim3(64), 0, c->stream, (const vit_job *)b->d_jobs, (const vit_bstream *)b->d_streams,
                         (const vit_state *)b->d_begin, (const vit_state *)b->d_end, (unsigned)nj, flags);
      ++b->launches_last;
      if (r == rounds) break;
      vit_args fa = a;
      fa.cond = flags;
      lane_launch(fa);
      ++b->launches_last;
    }
  }
  {   // (also when no stream has a chunk: the records on the device always describe the last run)
    const int rounds_run = nj ? rounds : 0;
    hipLaunchKernelGGL(k_vitb_decide, dim3((unsigned)b->n), dim3(64), 0, c->stream, (const vit_job *)b->d_jobs, (const vit_bstream *)b->d_streams,
                       (const vitb_plan *)b->d_plans, (const int *)b->d_bad, (unsigned)nj, rounds_run, (const vit_state *)b->d_end,
                       (const int *)b->d_rtotals, (const vit_state *)b->d_rstates, b->d_states, ns, P, (unsigned)spc, (unsigned)bpc, b->d_results);
    ++b->launches_last;
    LSDR_HIP(hipGetLastError());
  }
  b->in_flight = true;
  ++b->runs;
  return LSDR_OK;
}

int lsdr_viterbi_batch_wait(lsdr_viterbi_batch *b, lsdr_viterbi_batch_result *results) {
  LSDR_ARG(b);
  if (!b->in_flight) { lsdr_set_error("viterbi_batch: no run in flight"); return LSDR_E_ARG; }
  lsdr_ctx *c = b->ctx;
  LSDR_HIP(hipSetDevice(c->device));
  std::vector<lsdr_viterbi_batch_result> res(b->n);
  b->in_flight = false;
  {
    LSDR_TRY(lsdr_stage_d2h(c, res.data(), b->d_results, (size_t)b->n * sizeof(lsdr_viterbi_batch_result)));
    LSDR_TRY(lsdr_stage_sync(c));
    for (int i = 0; i < b->n; ++i) {
      lsdr_viterbi_batch::host_stream &h = b->hs[i];
      h.cur = (int)res[i].current_sync; h.phase = (int)res[i].resync_phase;
      // look-ahead: one resync period after a switch, doubling with every switch-free run
      if (res[i].switched) h.budget = (size_t)b->v->resync_period;
      else if (h.budget < ((size_t)1 << 40)) h.budget *= 2;
    }
  }
  if (results) memcpy(results, res.data(), (size_t)b->n * sizeof(lsdr_viterbi_batch_result));
  return LSDR_OK;
}

const lsdr_viterbi_batch_result *lsdr_viterbi_batch_results_dev(const lsdr_viterbi_batch *b) { return b ? b->d_results : nullptr; }

int lsdr_viterbi_batch_stats(const lsdr_viterbi_batch *b, unsigned *launches_last_run, unsigned long long *runs) {
  LSDR_ARG(b);
  if (launches_last_run) *launches_last_run = b->launches_last;
  if (runs) *runs = b->runs;
  return LSDR_OK;
}

}  // extern "C"
