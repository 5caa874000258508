// engine_aln.hip -- ibwa_batch_run and what reads its results.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <sys/mman.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>

#include "engine_ctx.h"

using namespace ibwa;

// ibwa_batch_run: its passes, each a function over the run's state (Run), in the order they run.
namespace {

// the pages a cooperative launch took from its pool (a bump counter: freed pages go to per-wave lists)
void note_coop_pages(ibwa_ctx *c, uint32_t pool_pages) {
  uint32_t used = 0;
  if (hipMemcpy(&used, c->coop.c_next.as<uint32_t>() + CNEXT_POOL, 4, hipMemcpyDeviceToHost) != hipSuccess) return;
  c->stats.coop_pages_peak = std::max<int64_t>(c->stats.coop_pages_peak, std::min<uint32_t>(used, pool_pages));
  c->stats.coop_pages_cap = std::max<int64_t>(c->stats.coop_pages_cap, pool_pages);  // the largest launch's pool
}

// Kernel arguments of the persistent gapped search shared by the first and retry passes;
// the caller fills the per-pass scratch and output pointers.
GapArgs gap_args(const ibwa_ctx *c, const AlnArgs &A, const AlnOpt &o, int64_t b0, int64_t cnt) {
  GapArgs G = {};
  G.ix[0] = c->index.ix[0];
  G.ix[1] = c->index.ix[1];
  G.o64[0] = c->index.o64[0].as<uint4>();
  G.o64[1] = c->index.o64[1].as<uint4>();
  G.seq = A.seq;
  G.off = A.off + b0;
  G.len = A.len + b0;
  G.ids = nullptr;
  G.n = cnt;
  G.maxdiff_tab = A.maxdiff_tab;
  G.wbuf = c->pass.d_wbuf.as<uint2>();
  G.wstride = A.wstride;
  G.wlen1 = A.wlen1;
  G.nN = c->pass.d_nN.as<uint16_t>();
  G.aln_next = counter(c, CTR_STREAM);
  G.lanes_per_wave = 64;
  G.o = o;
  return G;
}

int check_opt(const ibwa_gap_opt_t *o) {
  if (o->s_mm <= 0 || o->s_gapo <= 0 || o->s_gape <= 0)
    return fail(IBWA_EINVAL,
                "zero/negative penalties (-M %d -O %d -E %d) are unsupported: the reference reads uninitialised "
                "stack slots (bwtgap.c:60) or crashes on them",
                o->s_mm, o->s_gapo, o->s_gape);
  if (o->seed_len < 0 || o->max_gape < 0 || o->max_gapo < 0) return fail(IBWA_EINVAL, "negative option");
  return 0;
}

// Runs one pass of (width, search) over `lanes` reads.  ids == nullptr: the reads A.off / A.len start at.
int run_pass(ibwa_ctx *c, AlnArgs A, int64_t lanes, const int64_t *d_ids, float *ms_w, float *ms_s) {
  A.n = lanes;
  A.ids = d_ids;
  HIPCHK(hipEventRecord(c->ev[0], c->stream));
  HIPCHK(launch_width(A, c->block, c->stream));
  HIPCHK(hipEventRecord(c->ev[1], c->stream));
  HIPCHK(launch_search(A, c->block, c->stream));
  HIPCHK(hipEventRecord(c->ev[2], c->stream));
  HIPCHK(hipEventSynchronize(c->ev[2]));
  float a = 0, b = 0;
  HIPCHK(hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
  HIPCHK(hipEventElapsedTime(&b, c->ev[1], c->ev[2]));
  *ms_w += a;
  *ms_s += b;
  return 0;
}

// What the passes of one ibwa_batch_run share.
struct Run {
  ibwa_ctx *c = nullptr;
  const ibwa_gap_opt_t *opt = nullptr;
  std::chrono::steady_clock::time_point t0;
  AlnOpt o = {};  // batch-level local_opt (bwtaln.c:86-93)
  AlnArgs A = {};
  int64_t n = 0;
  int max_len = 0;
  int batch_md = 0;
  bool exact_path = false;
  bool v2 = false;             // persistent gapped search (gapped.hip)
  bool resume_states = false;  // the first pass left resume states (GapArgs::rdump)
  float ms_w = 0, ms_s = 0, ms_r = 0;
  float res_ms = 0, res_w = 0;  // the cooperative launches over resumed reads (after each chunk)
  int64_t res_ok = 0;           // reads they resolved
  // retry bookkeeping: the handed-on reads' statuses (rstat, as c->res.retry_ids), the reads still to
  // resolve and their slots in retry_ids, the pass that resolved each slot, the general kernels' sizes
  std::vector<uint32_t> rstat;
  std::vector<int64_t> todo, where;
  std::vector<uint8_t> found_by;
  std::vector<std::pair<int64_t, std::vector<uint4>>> patch;  // (read, hits) of the wide / general passes
  uint64_t cap = 0;
  uint32_t acap = 0;
  // host-phase timestamps (IBWA_VERBOSE)
  double since() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

size_t first_pass_lds(const Run &R);  // plan_first_pass's LDS bytes per workgroup

// Checks, the batch-level options, the per-length max_diff table and the arguments every pass shares;
// which path takes the batch.
int run_setup(Run &R, int batch_max_len) {
  ibwa_ctx *c = R.c;
  const ibwa_gap_opt_t *opt = R.opt;
  if (!c->index.loaded[0] || !c->index.loaded[1]) return fail(IBWA_ENOINDEX, "load both .bwt and .rbwt first");
  if (c->index.ix[0].seq_len != c->index.ix[1].seq_len) return fail(IBWA_EINVAL, ".bwt and .rbwt lengths differ");
  if (int rc = check_opt(opt)) return rc;
  c->res.fetched = false;
  HIPCHK(enter(c));
  memset(&c->stats, 0, sizeof(c->stats));
  g_alloc_ms = 0;
  c->pass.hpop_valid = false;  // set again by a gapped run that leaves resume states
  R.n = c->batch.n;
  const int max_len = R.max_len = std::max(batch_max_len, c->batch.max_len);

  // batch-level local_opt (bwtaln.c:86-93)
  AlnOpt &o = R.o;
  o.s_mm = opt->s_mm; o.s_gapo = opt->s_gapo; o.s_gape = opt->s_gape; o.mode = opt->mode;
  o.indel_end_skip = opt->indel_end_skip; o.max_del_occ = opt->max_del_occ; o.max_entries = opt->max_entries;
  o.fnr_pos = opt->fnr > 0.0f;
  const int batch_md = R.batch_md = o.fnr_pos ? ibwa_cal_maxdiff(max_len, 0.02, opt->fnr) : opt->max_diff;
  o.max_diff = opt->max_diff;
  o.max_gapo = batch_md < opt->max_gapo ? batch_md : opt->max_gapo;
  o.max_gape = opt->max_gape; o.max_seed_diff = opt->max_seed_diff; o.seed_len = opt->seed_len;
  o.max_top2 = opt->max_top2;
  o.n_stacks = (batch_md + 1) * o.s_mm + (o.max_gapo + 1) * o.s_gapo + (o.max_gape + 1) * o.s_gape;
  if (o.n_stacks <= 0 || o.n_stacks > (1 << 20)) return fail(IBWA_EINVAL, "invalid stack size %d", o.n_stacks);

  // per-length max_diff table
  std::vector<int16_t> tab(max_len + 1);
  for (int l = 0; l <= max_len; ++l) tab[l] = (int16_t)(o.fnr_pos ? ibwa_cal_maxdiff(l, 0.02, opt->fnr) : opt->max_diff);
  if (int rc = c->pass.d_tab.ensure(tab.size() * 2)) return rc;
  HIPCHK(hipMemcpyAsync(c->pass.d_tab.p, tab.data(), tab.size() * 2, hipMemcpyHostToDevice, c->stream));

  AlnArgs &A = R.A;
  A.ix[0] = c->index.ix[0];
  A.ix[1] = c->index.ix[1];
  A.seq = c->batch.v_seq;
  A.off = c->batch.v_off;
  A.len = c->batch.v_len;
  A.maxdiff_tab = c->pass.d_tab.as<int16_t>();
  A.wlen1 = (uint32_t)max_len + 1;
  A.wstride = 2ull * A.wlen1 + 2ull * ((uint64_t)std::max(opt->seed_len, 0) + 1);
  A.o = o;
  // k_width's one-row steps from the text (1: when SA / text are resident, 2: derive them)
  if (c->width_jump == 2 && !(c->exact_path && !o.fnr_pos && opt->max_diff == 0))
    if (int rc = ensure_jump(c)) return rc;
  if (c->width_jump && c->index.jump_ready) {
    for (int s = 0; s < 2; ++s) {
      A.jsa[s] = c->index.sa_full[s].as<uint32_t>();
      A.jtxt[s] = c->index.txt2[s].as<uint32_t>();
    }
  }

  R.exact_path = c->exact_path && !o.fnr_pos && opt->max_diff == 0 && opt->max_entries >= 2;
  c->stats.path = R.exact_path ? 1 : 0;
  if (R.exact_path) return 0;

  // persistent gapped search (gapped.hip) when the options fit its entry bit fields and the bucket
  // heads fit a workgroup's LDS: one lane's in the wide kernel (4 B heads: n_stacks <= 12 288) and 64
  // lanes' in the first pass (2 B heads, without the LDS widths one per bucket: n_stacks <= 480 with
  // the default page settings)
  R.v2 = c->gapped_v2 && batch_md + 1 <= 31 && o.max_gapo <= 7 && o.max_gape <= 15 &&
         gapped_lds_bytes(o.n_stacks, 64, true, 0, 0, 1, 4096) <= 65536 && max_len <= 65535;
  R.v2 = R.v2 && first_pass_lds(R) <= 65536;
  c->res.stream_out = R.v2;
  c->pass.hpop_valid = false;
  c->res.resumed_ids.clear();
  c->stats.n_resumed = 0;
  c->stats.resume_records = 0;
  c->stats.resume_records_peak = c->stats.resume_records_cap = 0;
  c->stats.coop_pages_peak = c->stats.coop_pages_cap = 0;
  c->stats.n_tail_jumps = 0;
  c->stats.n_width_tab_steps = 0;
  A.cap = c->stack_cap;
  return 0;
}

// max_diff == 0: the whole batch by k_exact.
int exact_pass(Run &R) {
  ibwa_ctx *c = R.c;
  AlnArgs &A = R.A;
  const int64_t n = R.n;
  const int max_len = R.max_len;
  c->res.stream_out = false;
  A.aln_cap = c->aln_cap;
  A.n = n;
  if (int rc = c->pass.d_aln.ensure(std::max<int64_t>(n, 1) * (uint64_t)A.aln_cap * 16)) return rc;
  if (int rc = c->pass.d_naln.ensure(std::max<int64_t>(n, 1) * 4)) return rc;
  if (int rc = c->pass.d_status.ensure(std::max<int64_t>(n, 1) * 4)) return rc;
  if (int rc = c->d_counter.ensure(64)) return rc;
  A.aln = c->pass.d_aln.as<uint4>();
  A.n_aln = c->pass.d_naln.as<int32_t>();
  A.status = c->pass.d_status.as<uint32_t>();
  if (int rc = ensure_kmer(c)) return rc;
  if (int rc = ensure_jump(c)) return rc;
  c->stats.kmer_k = c->index.kmer_K;
  HIPCHK(hipEventRecord(c->ev[0], c->stream));
  const uint32_t stride = exact_record_stride(max_len);
  if (int rc = c->d_rec.ensure(std::max<int64_t>(n, 1) * (uint64_t)stride * 16)) return rc;
  const uint32_t *jump[6] = {c->index.sa_full[0].as<uint32_t>(), c->index.sa_full[1].as<uint32_t>(),
                             c->index.isa_full[0].as<uint32_t>(), c->index.isa_full[1].as<uint32_t>(),
                             c->index.txt2[0].as<uint32_t>(), c->index.txt2[1].as<uint32_t>()};
  const bool use_jump = c->index.jump_ready && c->exact_jump;
  c->stats.path = use_jump ? 3 : 1;
  HIPCHK(launch_exact(A, c->index.o64[0].as<uint4>(), c->index.o64[1].as<uint4>(), c->index.kt[0].as<uint2>(),
                      c->index.kt[1].as<uint2>(), c->index.kmer_K, c->d_rec.as<uint4>(), stride,
                      counter(c, CTR_CLAIM), c->exact_blocks, c->ev[2], use_jump ? jump : nullptr,
                      c->stream));
  HIPCHK(hipEventRecord(c->ev[1], c->stream));
  HIPCHK(hipEventSynchronize(c->ev[1]));
  float ms_pack = 0, ms = 0;
  HIPCHK(hipEventElapsedTime(&ms_pack, c->ev[0], c->ev[2]));
  HIPCHK(hipEventElapsedTime(&ms, c->ev[2], c->ev[1]));
  c->stats.ms_width = ms_pack;  // the exact path's pre-pass: read packing
  c->stats.ms_search = ms;
  c->stats.n_launch_search = 1;
  c->res.aln_cap_used = A.aln_cap;
  c->res.h_naln.resize(n);
  c->res.h_status.clear();
  c->res.naln_on_host = false;  // results stay in HBM; ibwa_batch_fetch copies them
  c->res.retry_ids.clear();
  c->res.patch_ids.clear();
  c->res.patch_alns.clear();
  c->res.retry_pass.clear();
  c->res.resumed_ids.clear();
  c->stats.ms_total = R.since();
  c->stats.ms_alloc = g_alloc_ms;
  return 0;
}

// Cooperative launches (coop.hip): over the resumed reads of a first-pass chunk (coop_resumed_chunk)
// and in the retry rounds (coop_rounds).  Both size their scratch, order their reads and fill their
// arguments here; each sets only what it does differently.
constexpr uint32_t COOP_FREECAP = 4096, COOP_HCAP = 4096;
int coop_full_blocks(const ibwa_ctx *c) { return c->n_cus * c->coop_waves_per_cu; }
struct CoopScratch {
  uint32_t stg_log2 = 10, pool_pages = 0;
};
// Sizes and grows the scratch of a launch of `blocks` waves over `lanes` reads.  scaled_pool: the page
// pool in proportion to the launch's waves (at least 1 GiB), else the whole pool.
int coop_scratch(ibwa_ctx *c, int max_len, int64_t lanes, int blocks, bool scaled_pool, CoopScratch *S) {
  uint32_t stg_log2 = 10;
  while ((1u << stg_log2) < (uint32_t)c->coop_stg_room * (9u * (uint32_t)(max_len + 1) + 16u)) ++stg_log2;
  const int full_blocks = coop_full_blocks(c);
  const uint32_t freecap = COOP_FREECAP, hcap = COOP_HCAP;
  const uint64_t pool_bytes =
      !scaled_pool ? c->pool_bytes(max_len)
                   : std::min<uint64_t>(c->pool_bytes(max_len),
                                        std::max<uint64_t>(1ull << 30, c->pool_bytes(max_len) / full_blocks * blocks));
  const uint32_t pool_pages = c->coop_pool_pages ? c->coop_pool_pages : (uint32_t)(pool_bytes / (COOP_PG * 16ull));
  if (int rc = c->coop.c_stg.ensure((uint64_t)blocks * 64 * 16 << stg_log2)) return rc;
  if (int rc = c->coop.c_dir.ensure((uint64_t)blocks * COOP_NSTK * COOP_MAXP * 4)) return rc;
  if (int rc = c->coop.c_free.ensure((uint64_t)blocks * freecap * 4)) return rc;
  if (int rc = c->coop.c_hits.ensure((uint64_t)blocks * hcap * 16)) return rc;
  if (int rc = c->coop.c_recb.ensure((uint64_t)blocks * COOP_RREC * 16)) return rc;
  if (int rc = c->coop.c_pool.ensure((uint64_t)pool_pages * COOP_PG * 16)) return rc;
  if (int rc = c->coop.c_next.ensure(64)) return rc;
  if (int rc = c->pass.r_status.ensure(lanes * 4)) return rc;
  S->stg_log2 = stg_log2;
  S->pool_pages = pool_pages;
  return 0;
}
// The selection d_ids / d_selst [0, lanes) into d_ordids, largest first-pass stack first (its longest
// reads then do not start near the launch's end); d_ordi [0, lanes) holds the permutation.
int order_selection(ibwa_ctx *c, int64_t lanes) {
  size_t tb = 0;
  HIPCHK(order_heavy_first(nullptr, nullptr, lanes, nullptr, nullptr, nullptr, nullptr, &tb, c->stream));
  if (int rc = c->coop.d_ordk.ensure(lanes * 8)) return rc;
  if (int rc = c->coop.d_ordi.ensure(lanes * 8)) return rc;
  if (int rc = c->coop.d_ordids.ensure(lanes * 8)) return rc;
  if (int rc = c->coop.d_ordtmp.ensure(tb + 16)) return rc;
  HIPCHK(order_heavy_first(c->coop.d_selst.as<uint32_t>(), c->pass.d_ids.as<int64_t>(), lanes, c->coop.d_ordk.as<uint32_t>(),
                           c->coop.d_ordi.as<uint32_t>(), c->coop.d_ordids.as<int64_t>(), c->coop.d_ordtmp.p, &tb, c->stream));
  return 0;
}
// What every cooperative launch passes to k_coop; the caller adds its widths (wbuf, nN, wb_base) and
// whatever else it does differently.
CoopArgs coop_args(const Run &R, const int64_t *ids, int64_t lanes, const CoopScratch &S) {
  const ibwa_ctx *c = R.c;
  CoopArgs K = {};
  K.ix[0] = c->index.ix[0];
  K.ix[1] = c->index.ix[1];
  K.o64[0] = c->index.o64[0].as<uint4>();
  K.o64[1] = c->index.o64[1].as<uint4>();
  K.seq = R.A.seq;
  K.off = R.A.off;
  K.len = R.A.len;
  K.ids = ids;
  K.n = lanes;
  K.out_by_id = 1;  // n_aln / aln_off of the input read; status per launch read
  K.maxdiff_tab = R.A.maxdiff_tab;
  K.wstride = R.A.wstride;
  K.wlen1 = R.A.wlen1;
  K.stg = c->coop.c_stg.as<uint4>();
  K.stg_log2 = S.stg_log2;
  K.dir = c->coop.c_dir.as<uint32_t>();
  K.freel = c->coop.c_free.as<uint32_t>();
  K.freecap = COOP_FREECAP;
  K.pool = c->coop.c_pool.as<uint4>();
  K.pool_pages = S.pool_pages;
  K.pool_next = c->coop.c_next.as<uint32_t>() + CNEXT_POOL;
  K.hits = c->coop.c_hits.as<uint4>();
  K.recb = c->coop.c_recb.as<uint4>();
  K.hcap = COOP_HCAP;
  K.max_iters = 1u << 24;  // runaway guard; a read past it goes to the sequential kernel
  K.early = c->coop_early;
  // hits go on the first pass's stream (a read out of room there is flagged and re-run below)
  K.aln = c->pass.d_aln.as<uint4>();
  K.aln_total = c->res.stream_total;
  K.aln_next = counter(c, CTR_STREAM);
  K.aln_off = c->pass.d_aoff.as<uint64_t>();
  K.n_aln = c->pass.d_naln.as<int32_t>();
  K.status = c->pass.r_status.as<uint32_t>();
  K.o = R.o;
  return K;
}

// The reads of chunk [b0, b0 + cnt) that left a resume state go through the cooperative pass right
// after their chunk's first pass, so the state buffer holds one chunk's states at a time: a read
// it resolves is done (status 0), one it hands on starts over in the passes below.
// Selects the resumed reads of the chunk, orders them largest stack first, runs k_coop over them, then
// takes the reads it resolved and the state buffer's use, and sets the buffer's fill counter back to 0
// for the next chunk.
int coop_resumed_chunk(Run &R, int64_t b0, int64_t cnt) {
  ibwa_ctx *c = R.c;
  const int64_t n = R.n;
  size_t tb = 0;
  HIPCHK(select_resumed(c->pass.d_roff.as<uint64_t>(), b0, cnt, c->pass.d_status.as<uint32_t>(), nullptr, nullptr, nullptr,
                        nullptr, &tb, c->stream));
  if (int rc = c->coop.d_seltmp.ensure(tb + 16)) return rc;
  if (int rc = c->pass.d_ids.ensure(cnt * 8)) return rc;
  if (int rc = c->coop.d_selst.ensure(cnt * 4)) return rc;
  unsigned long long *d_cnt = counter(c, CTR_RESUMED);
  HIPCHK(select_resumed(c->pass.d_roff.as<uint64_t>(), b0, cnt, c->pass.d_status.as<uint32_t>(), c->pass.d_ids.as<int64_t>(),
                        c->coop.d_selst.as<uint32_t>(), d_cnt, c->coop.d_seltmp.p, &tb, c->stream));
  unsigned long long lanes_u = 0;
  HIPCHK(hipMemcpyAsync(&lanes_u, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const int64_t lanes = (int64_t)lanes_u;
  if (lanes > 0) {
    const int blocks = (int)std::min<int64_t>(coop_full_blocks(c), lanes);
    CoopScratch S;
    if (int rc = coop_scratch(c, R.max_len, lanes, blocks, true, &S)) return rc;
    // largest first-pass stack first, as in the retry rounds
    const int64_t *ids = c->pass.d_ids.as<int64_t>();
    if (lanes > 1) {
      if (int rc = order_selection(c, lanes)) return rc;
      ids = c->coop.d_ordids.as<int64_t>();
    }
    CoopArgs K = coop_args(R, ids, lanes, S);
    // The widths and N counts are the chunk's own first-pass rows, still in place (their gap_shadow
    // updates included): no k_width run.
    K.wbuf = c->pass.d_wbuf.as<uint2>();
    K.nN = c->pass.d_nN.as<uint16_t>();
    K.wb_base = b0;
    // every read of this launch left a state
    K.rdump = c->pass.d_rdump.as<uint4>();
    K.roff = c->pass.d_roff.as<uint64_t>();
    // as each read ends: done in the first pass's status if resolved, else its state dropped, so that the
    // later passes see it as any other handed-on read
    K.fix_status = c->pass.d_status.as<uint32_t>();
    K.fix_roff = c->pass.d_roff.as<uint64_t>();
    HIPCHK(hipEventRecord(c->ev[3], c->stream));
    HIPCHK(hipEventRecord(c->ev[5], c->stream));  // no width kernel: ms_coop_width gets ~0
    HIPCHK(launch_coop(K, counter(c, CTR_CLAIM), blocks, c->stream));
    HIPCHK(hipEventRecord(c->ev[4], c->stream));
    HIPCHK(hipEventSynchronize(c->ev[4]));
    note_coop_pages(c, S.pool_pages);
    float t_all = 0, t_w = 0;
    HIPCHK(hipEventElapsedTime(&t_all, c->ev[3], c->ev[4]));
    HIPCHK(hipEventElapsedTime(&t_w, c->ev[3], c->ev[5]));
    std::vector<uint32_t> rs(lanes);
    std::vector<int64_t> rid(lanes);
    HIPCHK(hipMemcpyAsync(rs.data(), c->pass.r_status.p, lanes * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(rid.data(), ids, lanes * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int64_t ok = 0;
    for (int64_t j = 0; j < lanes; ++j)
      if (rs[j] == 0) {
        ++ok;
        c->res.resumed_ids.push_back(rid[j]);
      }
    R.res_ms += t_all;
    R.res_w += t_w;
    R.res_ok += ok;
    if (c->verbose)
      fprintf(stderr, "[ibwa_amd] chunk at %lld: %lld resumed reads through the cooperative pass, %.1f ms\n",
              (long long)b0, (long long)lanes, t_all);
  }
  unsigned long long *rdn = c->pass.d_roff.as<unsigned long long>() + n;
  unsigned long long used = 0;
  HIPCHK(hipMemcpyAsync(&used, rdn, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->stats.resume_records += (int64_t)used;
  c->stats.resume_records_peak = std::max<int64_t>(c->stats.resume_records_peak, (int64_t)used);
  if (cnt >= 65536) c->resume_need = std::max(c->resume_need, (double)used / (double)cnt);
  HIPCHK(zero_async(rdn, 8, c->stream));
  return 0;
}

// Sizes of the persistent first pass: workgroup, LDS, pages, chunks, state buffer.
constexpr uint32_t LG = 13;  // log2 of a first-pass page's slots
struct FirstPassPlan {  // (in the order plan_first_pass returns them)
  int block, blocks;  // workgroup size, persistent grid
  uint64_t lanes;
  size_t lds;
  int per_cu;
  bool lw, resume;
  int max_pages, ppb, ppb_run;
  uint32_t P0r;
  int64_t chunk;
  uint32_t cw_rw, cw_sb, cw_words;
  uint64_t rd_cap, aln_total;
};
FirstPassPlan plan_first_pass(const Run &R) {
  const ibwa_ctx *c = R.c;
  const AlnOpt &o = R.o;
  const int64_t n = R.n;
  const int max_len = R.max_len, batch_md = R.batch_md;
  // equal chunks of at most gap_reads_per_chunk reads: every launch ends with a tail in which
  // only its slowest reads still run, so fewer (and balanced) launches waste less -- but no more
  // reads than an earlier run's resume states per read let the state buffer hold (150 bp at 2 %:
  // 3 chunks of 6.7 M instead of 2 of 10 M, whose overflowing states start over: 5160 -> 4972 ms
  // per 20 M reads in the round-4 footprint sweep)
  // LDS: bucket heads + free slots + page table per lane, the page bitmap per workgroup
  const uint32_t P0 = c->gap_cap1;
  const int max_pages = (int)std::min<uint32_t>(7, (65536u - P0) >> LG);
  auto ppb_of = [&](int blk) { return std::max(1, c->gap_pages_per_block * blk / 256); };
  // LDS widths (gapped.hip LW): bids clamped to max_diff + 1 in 3 bits and to max_seed_diff + 1
  // in 2, a ring of 16 bucket heads (the largest penalty <= 15), and 3 workgroups per CU still fit
  const int maxpen = std::max(o.s_mm, std::max(o.s_gapo, o.s_gape));
  const uint32_t cw_rw = (uint32_t)(max_len + 15) / 16;
  const uint32_t cw_sb = max_len > o.seed_len ? (uint32_t)o.seed_len + 1u : 0u;
  const uint32_t cw_words = 1u + cw_rw + ((uint32_t)max_len + 1u + cw_sb + 3u) / 4u;
  // The LDS rows grow with the read (100 bp: 208 B per lane, 3 workgroups of 256 lanes per CU); longer
  // reads take the workgroup size that keeps the most waves per CU (150 bp: 9 of 64 lanes) as long
  // as that is at least gap_lw_min_waves
  int lw_block = 256, lw_waves = 0;
  for (int blk : {256, 128, 64}) {
    const size_t b = gapped_lds_bytes(o.n_stacks, blk, false, max_pages, ppb_of(blk), 64, 0, (int)cw_words);
    if (b > 65536) continue;
    const int waves = std::min<int>(c->gap_blocks_per_cu * 4, (int)(160 * 1024 / b) * (blk / 64));
    if (waves > lw_waves) lw_waves = waves, lw_block = blk;
  }
  const bool lw = c->gap_lw && !c->diag && batch_md <= 6 && o.max_seed_diff >= 0 && o.max_seed_diff <= 2 && maxpen <= 15 &&
                  max_pages <= GAP_MAX_PAGES && lw_waves >= c->gap_lw_min_waves;
  auto lds_of = [&](int blk) {
    return gapped_lds_bytes(o.n_stacks, blk, false, max_pages, ppb_of(blk), 64, 0, lw ? (int)cw_words : 0);
  };
  const int block = lw ? lw_block : lds_of(256) <= 65536 ? 256 : lds_of(128) <= 65536 ? 128 : 64;
  const int ppb = ppb_of(block);
  const size_t lds = lds_of(block);
  const int per_cu = std::max<int>(
      1, std::min<int>(c->gap_blocks_per_cu * 256 / block, (int)(160 * 1024 / std::max<size_t>(lds, 1))));
  const bool resume = lw && c->gap_resume && c->gap_coop && max_len <= COOP_MAXLEN && o.n_stacks <= COOP_NSTK;
  // (Round 5 also overlapped a chunk's cooperative pass with the next chunk's first pass on a
  // second stream; measured 3-10 % slower at 50 M reads in both of its variants, it was removed in
  // round 6: DESIGN §4.4.1.)
  int64_t per_chunk = c->gap_reads_per_chunk;
  if (c->resume_need > 0)  // (the state buffer's bound no lower than 65 536 reads; gap_reads_per_chunk may be)
    per_chunk = std::min<int64_t>(per_chunk, std::max<int64_t>(65536, (int64_t)((double)(((uint64_t)c->gap_resume_gb << 30) / 16) /
                                                                                 (1.15 * c->resume_need))));
  const int64_t n_chunks = (std::max<int64_t>(n, 1) + per_chunk - 1) / per_chunk;
  const int64_t chunk = (std::max<int64_t>(n, 1) + n_chunks - 1) / n_chunks;
  // persistent grid: fills the chip, but a small batch gets only the lanes it can use, so
  // its per-lane scratch and page pools are sized by the batch, not the worst case
  const int blocks = (int)std::min<int64_t>((int64_t)c->n_cus * per_cu, (chunk + block - 1) / block);
  const uint64_t lanes = (uint64_t)blocks * block;
  const uint64_t aln_total = std::max<uint64_t>((uint64_t)n * c->gap_stream_per_read, c->gap_stream_min);
  // resume states of the early hand-offs: per read 1 + the state's offset (0: none), then per state
  // buffer its fill counter and the count of states stored
  uint64_t rd_cap = 0;
  if (resume) {
    // the buffer holds one first-pass chunk's states at a time (cleared after each chunk)
    const double per_read = std::max<double>(c->gap_resume_recs, 1.15 * c->resume_need);
    rd_cap = std::min<uint64_t>(((uint64_t)c->gap_resume_gb << 30) / 16, (uint64_t)((double)chunk * per_read) + (1u << 16));
    if (c->gap_resume_records > 0) rd_cap = (uint64_t)c->gap_resume_records;
  }
  // and smaller static slot regions (4096: 5859 -> 5840 ms per 50M-read step, hits identical,
  // profiles/r03_pool_cap_sweep.log; the page table and max_pages are the same for both sizes)
  const uint32_t P0r = resume ? std::min<uint32_t>(P0, c->gap_resume_cap1) : P0;
  // with resume states a read leaves the first pass by 2 000 iterations, so few stacks outgrow the
  // static slots: a smaller page pool (same time at 50M reads, profiles/r03_pool_chunk_sweep.log)
  const int ppb_run = resume ? std::min(ppb, std::max(1, c->gap_resume_ppb * block / 256)) : ppb;
  return {block, blocks, lanes, lds, per_cu, lw, resume, max_pages, ppb, ppb_run, P0r, chunk, cw_rw, cw_sb, cw_words,
          rd_cap, aln_total};
}

size_t first_pass_lds(const Run &R) { return plan_first_pass(R).lds; }

// IBWA_VERBOSE: a k_gapped launch's iterations per read (GapArgs::iters), b ms
int print_gapped_iters(const uint32_t *d_iters, int64_t cnt, float b) {
  std::vector<uint32_t> it(cnt);
  HIPCHK(hipMemcpy(it.data(), d_iters, cnt * 4, hipMemcpyDeviceToHost));
  uint64_t sum = 0;
  uint32_t mx = 0;
  for (uint32_t v : it) { sum += v; mx = std::max(mx, v); }
  std::sort(it.begin(), it.end());
  fprintf(stderr, "[ibwa_amd] k_gapped: %lld reads, %.3g lane-iterations (%.0f per read, p99 %u, p99.99 %u, "
          "max %u), %.1f ms -> %.3g lane-iterations/s\n", (long long)cnt, (double)sum, (double)sum / cnt,
          it[(size_t)(cnt * 0.99)], it[(size_t)(cnt * 0.9999)], mx, b, sum / (b * 1e-3));
  return 0;
}
// IBWA_PROF_PHASES: a k_gapped launch's phase counters (GapArgs::prof in d_prof)
int print_gapped_phases(const ibwa_ctx *c, int waves, int64_t cnt) {
  unsigned long long pf[23];
  HIPCHK(hipMemcpy(pf, c->d_prof.p, sizeof pf, hipMemcpyDeviceToHost));
  const char *nm[4] = {"claim", "pop", "wait", "rest"};
  double tot = (double)(pf[0] + pf[1] + pf[2] + pf[3]);
  fprintf(stderr, "[ibwa_amd] k_gapped phases (wave cycles, %d waves):", waves);
  for (int q = 0; q < 4; ++q) fprintf(stderr, " %s %.1f%%", nm[q], tot > 0 ? 100.0 * pf[q] / tot : 0.0);
  const double wi = pf[9] ? (double)pf[9] : 1.0;
  fprintf(stderr, "; per wave-iteration: exact %.3f push trips %.3f hits %.3f ends %.3f expansions %.3f "
          "claims %.3f (%llu wave-iterations)\n", pf[4] / wi, pf[5] / wi, pf[6] / wi, pf[7] / wi, pf[8] / wi,
          pf[10] / wi, pf[9]);
  const double li = pf[16] ? (double)pf[16] : 1.0;
  fprintf(stderr, "[ibwa_amd] k_gapped loads per live lane-iteration: block %.3f second block %.3f widths %.3f "
          "seed widths %.3f candidate %.3f; exact steps %.3f (unique interval %.3f) (%.3g live lane-iterations)\n",
          pf[11] / li, pf[12] / li, pf[13] / li, pf[14] / li, pf[15] / li, pf[17] / li, pf[18] / li, (double)pf[16]);
  fprintf(stderr, "[ibwa_amd] k_gapped tail jumps: %.2f per read (%.2f onto an empty entry), %.2f symbols per "
          "read; pure-match run steps %.3f per live lane-iteration (%llu)\n", (double)pf[19] / cnt,
          (double)pf[20] / cnt, (double)pf[21] / cnt, pf[22] / li, pf[22]);
  return 0;
}

// First pass by the persistent gapped kernel, in equal chunks; each chunk's resumed reads go through the
// cooperative pass right after it.
int first_pass_persistent(Run &R) {
  ibwa_ctx *c = R.c;
  AlnArgs &A = R.A;
  const AlnOpt &o = R.o;
  const int64_t n = R.n;
  if (int rc = ensure_kmer(c)) return rc;
  c->stats.path = 2;
  if (c->width_tab && c->index.ltab_K > 0 && c->index.ix[0].seq_len < LTAB_MARK) {  // k_width's leading steps
    A.ltab[0] = c->index.ltab[0].as<uint2>();
    A.ltab[1] = c->index.ltab[1].as<uint2>();
    A.tab_k = (uint32_t)c->index.ltab_K;
    A.tab_reset = c->width_tab == 2;
  }
  A.cw_stage = (uint32_t)c->width_rec_stage;
  const FirstPassPlan P = plan_first_pass(R);
  const bool lw = P.lw, resume = P.resume;
  c->stats.first_pass_lw = lw;
  c->stats.first_pass_block = P.block;
  const int64_t chunk = P.chunk;
  if (int rc = c->pass.d_wbuf.ensure(chunk * A.wstride * 8)) return rc;
  if (int rc = c->pass.d_nN.ensure(chunk * 2 + 2)) return rc;
  if (lw) {
    if (int rc = c->pass.d_cw.ensure(chunk * (uint64_t)P.cw_words * 4)) return rc;
    if (int rc = c->pass.d_ptabg.ensure(P.lanes * GAP_MAX_PAGES * 2)) return rc;
  }
  if (resume) {
    if (int rc = c->pass.d_rdump.ensure(P.rd_cap * 16)) return rc;
    c->stats.resume_records_cap = (int64_t)P.rd_cap;
    if (int rc = c->pass.d_roff.ensure(((uint64_t)n + 4) * 8)) return rc;
    HIPCHK(zero_async(c->pass.d_roff.p, ((uint64_t)n + 4) * 8, c->stream));
    if (int rc = c->pass.d_hpop.ensure(((uint64_t)n + 1) * 4)) return rc;
    HIPCHK(zero_async(c->pass.d_hpop.p, ((uint64_t)n + 1) * 4, c->stream));
    R.resume_states = true;
    c->pass.hpop_valid = true;
  }
  if (int rc = c->pass.d_ent.ensure(P.lanes * P.P0r * 16)) return rc;
  if (int rc = c->pass.d_pool.ensure((uint64_t)P.blocks * P.ppb_run * (16ull << LG))) return rc;
  if (int rc = c->pass.d_aln.ensure(P.aln_total * 16)) return rc;
  if (int rc = c->pass.d_aoff.ensure(std::max<int64_t>(n, 1) * 8)) return rc;
  if (int rc = c->pass.d_naln.ensure(std::max<int64_t>(n, 1) * 4)) return rc;
  if (int rc = c->pass.d_status.ensure(std::max<int64_t>(n, 1) * 4)) return rc;
  if (int rc = c->d_counter.ensure(64)) return rc;
  HIPCHK(zero_async(counter(c, CTR_STREAM), 8, c->stream));
  HIPCHK(zero_async(counter(c, CTR_TAIL_JUMPS), 8, c->stream));  // GapArgs::tail_jumps
  HIPCHK(zero_async(counter(c, CTR_WIDTH_TAB), 8, c->stream));   // AlnArgs::tab_steps (every k_width of the run)
  A.tab_steps = counter(c, CTR_WIDTH_TAB);
  c->res.diag_w.clear();
  c->res.diag_cw.clear();
  c->res.diag_shape[0] = c->res.diag_shape[1] = c->res.diag_shape[2] = 0;
  for (int64_t b0 = 0; b0 < n; b0 += chunk) {
    const int64_t cnt = std::min(chunk, n - b0);
    AlnArgs B = A;
    B.n = cnt;
    B.off = A.off + b0;
    B.len = A.len + b0;
    B.wbuf = c->pass.d_wbuf.as<uint2>();
    B.nN = c->pass.d_nN.as<uint16_t>();
    GapArgs G = gap_args(c, A, o, b0, cnt);
    G.wbuf = B.wbuf;
    G.nN = B.nN;
    if (lw) {
      B.cw = c->pass.d_cw.as<uint32_t>();
      B.cw_words = P.cw_words;
      B.cw_rw = P.cw_rw;
      G.cw = B.cw;
      G.cw_words = P.cw_words;
      G.cw_rw = P.cw_rw;
      G.ptab_g = c->pass.d_ptabg.as<uint16_t>();
    }
    G.ent = c->pass.d_ent.as<uint4>();
    if (lw && c->index.ltab_K > 0 && c->index.ix[0].seq_len < LTAB_MARK) {
      G.ltab[0] = c->index.ltab[0].as<uint2>();
      G.ltab[1] = c->index.ltab[1].as<uint2>();
      G.tab_k = (uint32_t)c->index.ltab_K;
      G.tail_tab = (uint32_t)c->gap_tail_tab;
      G.tail_jumps = counter(c, CTR_TAIL_JUMPS);
    }
    G.cap1 = P.P0r;
    G.hit_slots = std::min<uint32_t>(c->gap_hit_slots, P.P0r / 2);
    G.pool = c->pass.d_pool.as<uint4>();
    G.page_log2 = LG;
    G.max_pages = P.max_pages;
    G.pages_per_block = P.ppb_run;
    G.aln = c->pass.d_aln.as<uint4>();
    G.aln_total = P.aln_total;
    c->res.stream_total = P.aln_total;
    G.aln_off = c->pass.d_aoff.as<uint64_t>() + b0;
    G.n_aln = c->pass.d_naln.as<int32_t>() + b0;
    G.status = c->pass.d_status.as<uint32_t>() + b0;
    G.max_iters = c->gap_iter_budget;
    G.early_iters = resume ? c->gap_resume_iters : c->gap_early_iters;
    G.early_entries = resume ? c->gap_resume_entries : c->gap_early_entries;
    if (resume) {
      G.rdump = c->pass.d_rdump.as<uint4>();
      G.rd_next = c->pass.d_roff.as<unsigned long long>() + n;
      G.rd_cap = P.rd_cap;
      G.roff = c->pass.d_roff.as<uint64_t>() + b0;
      G.hpop = c->pass.d_hpop.as<uint32_t>() + b0;
      G.tail_lanes = c->gap_tail_lanes;
      G.tail_iters = c->gap_tail_iters;
    }
    if (c->verbose || c->diag) {
      if (int rc = c->pass.d_iters.ensure(std::max<int64_t>(n, 1) * 4)) return rc;
      G.iters = c->pass.d_iters.as<uint32_t>() + b0;
    }
    if (c->diag) {
      if (int rc = c->pass.d_feat.ensure(std::max<int64_t>(n, 1) * 8)) return rc;
      B.feat = c->pass.d_feat.as<uint16_t>() + b0 * 4;
    }
    if (c->prof_phases) {
      if (int rc = c->d_prof.ensure(256)) return rc;
      HIPCHK(hipMemsetAsync(c->d_prof.p, 0, 256, c->stream));
      G.prof = c->d_prof.as<unsigned long long>();
    }
    const bool keep_w = c->diag_width && b0 == 0;  // ibwa_batch_diag 3 / 4: the first chunk's k_width outputs
    if (keep_w) {
      // zeros where k_width writes nothing (past a read's length), so the copies compare byte for byte
      HIPCHK(hipMemsetAsync(B.wbuf, 0, (uint64_t)cnt * A.wstride * 8, c->stream));
      if (lw) HIPCHK(hipMemsetAsync(B.cw, 0, (uint64_t)cnt * P.cw_words * 4, c->stream));
    }
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    HIPCHK(launch_width(B, c->block, c->stream));
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    if (keep_w) {
      // before k_gapped: its gap_shadow rewrites the rows, and the later passes reuse the buffer
      c->res.diag_w.resize((uint64_t)cnt * A.wstride);
      c->res.diag_cw.resize(lw ? (uint64_t)cnt * P.cw_words : 0);
      c->res.diag_shape[0] = (uint64_t)cnt;
      c->res.diag_shape[1] = A.wstride;
      c->res.diag_shape[2] = lw ? P.cw_words : 0;
      HIPCHK(hipStreamSynchronize(c->stream));
      HIPCHK(hipMemcpy(c->res.diag_w.data(), B.wbuf, c->res.diag_w.size() * 8, hipMemcpyDeviceToHost));
      if (lw) HIPCHK(hipMemcpy(c->res.diag_cw.data(), B.cw, c->res.diag_cw.size() * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(launch_gapped(G, counter(c, CTR_CLAIM), P.blocks, P.block, false, c->stream));
    HIPCHK(hipEventRecord(c->ev[2], c->stream));
    HIPCHK(hipEventSynchronize(c->ev[2]));
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
    HIPCHK(hipEventElapsedTime(&b, c->ev[1], c->ev[2]));
    R.ms_w += a;
    R.ms_s += b;
    c->stats.n_launch_width++;
    c->stats.n_launch_search++;
    if (c->verbose)
      if (int rc = print_gapped_iters(G.iters, cnt, b)) return rc;
    if (c->prof_phases)
      if (int rc = print_gapped_phases(c, P.blocks * P.block / 64, cnt)) return rc;
    if (R.resume_states)
      if (int rc = coop_resumed_chunk(R, b0, cnt)) return rc;
  }
  return 0;
}

// First pass by the general kernels (options outside k_gapped's entry bit fields, or gapped_v2 = 0),
// in chunks of lanes_per_chunk reads.
int first_pass_legacy(Run &R) {
  ibwa_ctx *c = R.c;
  AlnArgs &A = R.A;
  const AlnOpt &o = R.o;
  const int64_t n = R.n;
  const int64_t chunk = std::min<int64_t>(std::max<int64_t>(n, 1), c->lanes_per_chunk);
  A.aln_cap = c->aln_cap;
  if (int rc = c->pass.d_wbuf.ensure(chunk * A.wstride * 8)) return rc;
  if (int rc = c->pass.d_heads.ensure(chunk * (uint64_t)o.n_stacks * 4)) return rc;
  if (int rc = c->pass.d_ent.ensure(chunk * (uint64_t)A.cap * 16)) return rc;
  if (int rc = c->pass.d_prev.ensure(chunk * (uint64_t)A.cap * 4)) return rc;
  if (int rc = c->pass.d_aln.ensure(std::max<int64_t>(n, 1) * (uint64_t)A.aln_cap * 16)) return rc;
  if (int rc = c->pass.d_naln.ensure(std::max<int64_t>(n, 1) * 4)) return rc;
  if (int rc = c->pass.d_status.ensure(std::max<int64_t>(n, 1) * 4)) return rc;
  A.wbuf = c->pass.d_wbuf.as<uint2>();
  A.heads = c->pass.d_heads.as<uint32_t>();
  A.ent = c->pass.d_ent.as<uint4>();
  A.prev = c->pass.d_prev.as<uint32_t>();
  for (int64_t b0 = 0; b0 < n; b0 += chunk) {
    int64_t lanes = std::min(chunk, n - b0);
    // lane-indexed inputs and outputs: shift the base pointers to this chunk
    AlnArgs B = A;
    B.off = A.off + b0;
    B.len = A.len + b0;
    B.aln = c->pass.d_aln.as<uint4>() + b0 * A.aln_cap;
    B.n_aln = c->pass.d_naln.as<int32_t>() + b0;
    B.status = c->pass.d_status.as<uint32_t>() + b0;
    if (int rc = run_pass(c, B, lanes, nullptr, &R.ms_w, &R.ms_s)) return rc;
    c->stats.n_launch_width++;
    c->stats.n_launch_search++;
  }
  return 0;
}

// After the first pass: its times, the reads it handed on (non-zero status) selected on the device,
// their status counts, and the retry bookkeeping the later passes work on.
int select_handed_on_reads(Run &R) {
  ibwa_ctx *c = R.c;
  const int64_t n = R.n;
  std::vector<uint32_t> &rstat = R.rstat;
  c->stats.ms_width = R.ms_w;
  c->stats.ms_search = R.ms_s;
  c->res.aln_cap_used = R.A.aln_cap;

  if (c->verbose) fprintf(stderr, "[ibwa_amd] t %.1f ms: first pass done\n", R.since());
  // results stay in HBM; the reads handed on (non-zero status) are selected on the device
  c->res.naln_on_host = false;
  c->res.h_status.clear();
  c->res.stream_len = 0;
  c->res.retry_ids.clear();
  c->res.patch_ids.clear();
  c->res.patch_alns.clear();
  c->res.retry_pass.clear();
  if (n) {
    size_t tb = 0;
    HIPCHK(select_handed_on(c->pass.d_status.as<uint32_t>(), n, nullptr, nullptr, nullptr, nullptr, &tb, c->stream));
    if (int rc = c->coop.d_seltmp.ensure(tb + 16)) return rc;
    if (int rc = c->pass.d_ids.ensure(n * 8)) return rc;
    if (int rc = c->coop.d_selst.ensure(n * 4)) return rc;
    if (int rc = c->d_counter.ensure(64)) return rc;
    unsigned long long *d_cnt = counter(c, CTR_HANDED_ON);
    HIPCHK(select_handed_on(c->pass.d_status.as<uint32_t>(), n, c->pass.d_ids.as<int64_t>(), c->coop.d_selst.as<uint32_t>(), d_cnt,
                            c->coop.d_seltmp.p, &tb, c->stream));
    unsigned long long cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->res.retry_ids.resize(cnt);
    rstat.resize(cnt);
    if (cnt) {
      HIPCHK(hipMemcpyAsync(c->res.retry_ids.data(), c->pass.d_ids.p, cnt * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(rstat.data(), c->coop.d_selst.p, cnt * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  for (size_t j = 0; j < rstat.size(); ++j) {
    const uint32_t s_ = rstat[j];
    if (s_ & ST_BAD_SCORE) return fail(IBWA_EINVAL, "read %lld: score outside the stack range", (long long)c->res.retry_ids[j]);
    c->stats.n_stack_overflow += (s_ & ST_STACK_OVERFLOW) != 0;
    c->stats.n_aln_overflow += (s_ & ST_ALN_OVERFLOW) != 0;
    c->stats.n_heavy += (s_ & ST_HEAVY) != 0;
  }
  if (R.resume_states) {
    unsigned long long rs[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(rs, c->pass.d_roff.as<unsigned long long>() + n, 32, hipMemcpyDeviceToHost));
    c->stats.n_resumed = (int64_t)(rs[1] + rs[3]);  // states stored in either buffer
    c->stats.n_heavy += R.res_ok;  // handed on and resolved by the per-chunk cooperative launches
    c->stats.n_coop += R.res_ok;
    c->stats.ms_coop += R.res_ms;
    c->stats.ms_coop_width += R.res_w;
  }
  if (c->verbose) fprintf(stderr, "[ibwa_amd] t %.1f ms: handed-on reads selected, %zu to retry\n", R.since(), c->res.retry_ids.size());
  // retry pass: larger stacks / hit arrays for the few reads that overflowed
  R.todo = c->res.retry_ids;
  R.cap = std::max<uint64_t>((uint64_t)c->stack_cap * 16, 65536);
  R.acap = std::max<uint32_t>(c->aln_cap * 64, 4096);
  R.found_by.assign(R.todo.size(), 0);
  R.where.resize(R.todo.size());
  for (size_t j = 0; j < R.todo.size(); ++j) R.where[j] = (int64_t)j;
  return 0;
}

// IBWA_PROF_PHASES: a k_coop launch's phase counters (CoopArgs::prof) and wave durations (wave_t)
int print_coop_phases(const ibwa_ctx *c, const CoopArgs &K, int blocks) {
  unsigned long long pf[40];
  HIPCHK(hipMemcpy(pf, c->d_prof.p, sizeof pf, hipMemcpyDeviceToHost));
  const char *nm[6] = {"barriers", "commits", "claims", "loads+consume", "levels", "read set-up"};
  double tot = 0;
  for (int q = 0; q < 6; ++q) tot += (double)pf[q];
  fprintf(stderr, "[ibwa_amd] k_coop phases (wave cycles):");
  for (int q = 0; q < 6; ++q) fprintf(stderr, " %s %.1f%%", nm[q], tot > 0 ? 100.0 * pf[q] / tot : 0.0);
  fprintf(stderr, "; %llu iterations (%.0f cycles each), %llu commits, %llu levels; lanes per iteration: "
          "%.1f running (%.1f fetching an entry, %.1f in an exact tail)\n", pf[6], pf[6] ? tot / pf[6] : 0.0, pf[7],
          pf[8], pf[6] ? (double)pf[9] / pf[6] : 0.0, pf[6] ? (double)pf[10] / pf[6] : 0.0,
          pf[6] ? (double)pf[11] / pf[6] : 0.0);
  const double it = pf[6] ? (double)pf[6] : 1.0;
  fprintf(stderr, "[ibwa_amd] k_coop idle lanes per iteration: barrier %.1f, level drained %.1f, ring %.1f, staging %.1f; "
          "chains %llu (%.0f per level), %llu discarded at %llu barriers, %llu children committed\n",
          pf[12] / it, pf[13] / it, pf[14] / it, pf[15] / it, pf[16], pf[8] ? (double)pf[16] / pf[8] : 0.0, pf[17],
          pf[18], pf[19]);
  fprintf(stderr, "[ibwa_amd] k_coop iterations (running lanes) by chains per level:");
  const char *nb[5] = {"<=2", "<=16", "<=64", "<=256", ">256"};
  for (int q = 0; q < 5; ++q)
    fprintf(stderr, " %s: %.1f%% (%.1f)", nb[q], 100.0 * pf[20 + q] / it, pf[20 + q] ? (double)pf[25 + q] / pf[20 + q] : 0.0);
  fprintf(stderr, "\n");
  fprintf(stderr, "[ibwa_amd] k_coop one-row lane-steps: expanding %.1f%%, exact tail %.1f%% of running; chains by steps:",
          100.0 * pf[30] / (pf[9] ? pf[9] : 1), 100.0 * pf[31] / (pf[9] ? pf[9] : 1));
  const char *cb[4] = {"<4", "<16", "<64", ">=64"};
  for (int q = 0; q < 4; ++q)
    fprintf(stderr, " %s: %llu (%.1f%% of steps)", cb[q], pf[32 + q], 100.0 * pf[36 + q] / (pf[9] ? pf[9] : 1));
  fprintf(stderr, "\n");
  // wave end times (shader clock) relative to the first wave start: the pass's tail
  std::vector<unsigned long long> wt((size_t)blocks * 2);
  HIPCHK(hipMemcpy(wt.data(), K.wave_t, wt.size() * 8, hipMemcpyDeviceToHost));
  // each wave's own duration (the clock is per XCD; the persistent grid starts together)
  std::vector<double> ends;
  for (int w = 0; w < blocks; ++w) ends.push_back((double)(wt[2 * w + 1] - wt[2 * w]));
  std::sort(ends.begin(), ends.end());
  const double last = ends.back() > 0 ? ends.back() : 1.0;
  fprintf(stderr, "[ibwa_amd] k_coop wave durations (fraction of the longest): p10 %.3f p50 %.3f p90 %.3f p99 %.3f\n",
          ends[ends.size() / 10] / last, ends[ends.size() / 2] / last, ends[ends.size() * 9 / 10] / last,
          ends[ends.size() * 99 / 100] / last);
  return 0;
}
// IBWA_VERBOSE: a cooperative round's iterations, hand-on reasons (rs: its statuses), pages and root chains;
// handed_on: the reads that run again in the next round, a: its ms
int print_coop_round(const CoopArgs &K, const std::vector<uint32_t> &rs, int blocks, size_t handed_on, float a) {
  const int64_t lanes = K.n;
  uint32_t mx = 0;
  if (K.iters) {
    std::vector<uint32_t> it(lanes);
    HIPCHK(hipMemcpy(it.data(), K.iters, lanes * 4, hipMemcpyDeviceToHost));
    mx = *std::max_element(it.begin(), it.end());
    double sum = 0;
    for (uint32_t v : it) sum += v;
    std::sort(it.begin(), it.end());
    fprintf(stderr, "[ibwa_amd] coop wave-iterations: sum %.3g (%.0f per wave of %d), p50 %u p99 %u p99.9 %u max %u\n",
            sum, sum / blocks, blocks, it[it.size() / 2], it[(size_t)(it.size() * 0.99)],
            it[(size_t)(it.size() * 0.999)], mx);
  }
  uint32_t pages = 0;
  HIPCHK(hipMemcpy(&pages, K.pool_next, 4, hipMemcpyDeviceToHost));
  int why[8] = {0};
  for (int64_t j = 0; j < lanes; ++j)
    if (rs[j]) ++why[(rs[j] >> 8) & 7];
  fprintf(stderr, "[ibwa_amd] coop hand-on reasons: len %d, max_entries %d, pool %d, bucket pages %d, guard %d\n",
          why[1], why[2], why[3], why[4], why[5]);
  fprintf(stderr, "[ibwa_amd] coop pass: %lld reads, %zu handed on, max %u wave iterations, %u pages, %.1f ms\n",
          (long long)lanes, handed_on, mx, pages, a);
  if (K.proot) {
    unsigned long long used = 0;
    HIPCHK(hipMemcpy(&used, K.pstore_next, 8, hipMemcpyDeviceToHost));
    std::vector<uint4> pr((size_t)lanes * 2);
    HIPCHK(hipMemcpy(pr.data(), K.proot, pr.size() * 16, hipMemcpyDeviceToHost));
    int64_t fl[3] = {0, 0, 0};
    for (const uint4 &q : pr) ++fl[(q.w & 0xFFu) < 3 ? (q.w & 0xFFu) : 2];
    fprintf(stderr, "[ibwa_amd] coop roots: %.1f children per chain stored (%llu of %llu entries), chains: %lld done, "
            "%lld hit, %lld skipped\n", (double)used / (double)pr.size(), used, (unsigned long long)K.pstore_cap,
            (long long)fl[0], (long long)fl[1], (long long)fl[2]);
  }
  return 0;
}

// heavy and overflowing reads: the wave-cooperative kernel first (exact; whatever it cannot
// hold is flagged and continues in the wide and general rounds)
int coop_rounds(Run &R) {
  ibwa_ctx *c = R.c;
  const AlnArgs &A = R.A;
  std::vector<int64_t> &todo = R.todo, &where = R.where;
  if (!(R.v2 && c->gap_coop && !todo.empty() && R.max_len <= COOP_MAXLEN && R.o.n_stacks <= COOP_NSTK)) return 0;
  std::vector<int64_t> wide_todo, wide_where;
  const int n_rounds = 4;
  for (int round = 0; round < n_rounds && !todo.empty(); ++round) {
    const int64_t lanes = (int64_t)todo.size();
    const size_t wide0 = wide_todo.size();
    // one heavy read per wave at a time: no more waves than heavy reads, and the page pool in
    // proportion (at least 1 GiB).  The reads that run out of pages run again with all of it,
    // shared by 8x fewer concurrent waves each round (the pool is taken page by page, so each of
    // them can grow into the room the others leave): a read whose stack outgrew its share of a
    // busy pool is still resolved cooperatively, instead of by the sequential wide kernel (at
    // coop_pool_gb=10, 150 bp reads at 2 %: minutes; now 1.07x the 16 GiB time, r05_sweep_mem150.jsonl)
    const int full_blocks = coop_full_blocks(c);
    const int blocks = (int)std::min<int64_t>(std::max(1, full_blocks >> (3 * round)), lanes);
    if (int rc = c->pass.d_ids.ensure(lanes * 8)) return rc;
    if (int rc = c->pass.d_wbuf.ensure(lanes * A.wstride * 8)) return rc;
    if (int rc = c->pass.d_nN.ensure(lanes * 2 + 2)) return rc;
    CoopScratch S;
    if (int rc = coop_scratch(c, R.max_len, lanes, blocks, round == 0, &S)) return rc;
    // k_coop_roots: two chain records per read, their children in a compact store (a chain that
    // finds it full leaves level 0 to k_coop).  A root chain stages ~190 children on a GRCh37-sized
    // genome, so the store takes the first pass's page pool when there is one: nothing in it is
    // live between the first pass and the retry passes, which set it up anew.
    uint4 *pstore = nullptr;
    uint64_t pcap = 0;
    if (c->coop_roots) {
      if (int rc = c->coop.c_proot.ensure((uint64_t)lanes * 2 * 16)) return rc;
      if (c->pass.d_pool.cap >= (1ull << 30)) {
        pstore = c->pass.d_pool.as<uint4>();
        pcap = std::min<uint64_t>(c->pass.d_pool.cap / 16, 0xFFFFFFFFull);
      } else {
        pcap = std::min<uint64_t>(1ull << 31, std::max<uint64_t>(1ull << 24, (uint64_t)lanes * 2 * 256));
        if (int rc = c->coop.c_pstore.ensure(pcap * 16)) return rc;
        pstore = c->coop.c_pstore.as<uint4>();
      }
    }
    if (int rc = c->d_counter.ensure(64)) return rc;
    // d_ids holds todo (select_handed_on, input order); the pass takes the reads with the largest
    // first-pass stacks first (its longest reads then do not start near its end) -- which pass or
    // which order resolves a read changes nothing in its results
    if (round) HIPCHK(hipMemcpy(c->pass.d_ids.p, todo.data(), lanes * 8, hipMemcpyHostToDevice));
    const int64_t *coop_ids = c->pass.d_ids.as<int64_t>();
    if (!round && lanes > 1) {
      if (int rc = order_selection(c, lanes)) return rc;
      std::vector<uint32_t> perm(lanes);
      HIPCHK(hipMemcpyAsync(perm.data(), c->coop.d_ordi.p, lanes * 4, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      for (int64_t j = 0; j < lanes; ++j) {
        todo[j] = c->res.retry_ids[perm[j]];
        where[j] = perm[j];
      }
      coop_ids = c->coop.d_ordids.as<int64_t>();
    }
    AlnArgs B = A;
    B.ids = coop_ids;
    B.n = lanes;
    B.wbuf = c->pass.d_wbuf.as<uint2>();
    B.nN = c->pass.d_nN.as<uint16_t>();
    CoopArgs K = coop_args(R, coop_ids, lanes, S);
    // widths from this launch's own k_width: the first pass's rows of these reads are gone
    K.wbuf = B.wbuf;
    K.nN = B.nN;
    K.wb_base = -1;
    // states only if the first pass left any: k_coop then looks up roff[id] (0: the read starts over,
    // as one whose state a per-chunk launch dropped).  No fix-up: the statuses are read on the host below
    if (R.resume_states) {
      K.rdump = c->pass.d_rdump.as<uint4>();
      K.roff = c->pass.d_roff.as<uint64_t>();
    }
    // level 0 by k_coop_roots: these reads start at their roots (a resumed chunk's start at their states)
    if (c->coop_roots) {
      K.proot = c->coop.c_proot.as<uint4>();
      K.pstore = pstore;
      K.pstore_next = c->coop.c_next.as<unsigned long long>() + CNEXT_PSTORE;
      K.pstore_cap = pcap;
    }
    // diagnostics of the retry rounds only
    if (c->verbose) {
      if (int rc = c->pass.d_iters.ensure(lanes * 4)) return rc;
      K.iters = c->pass.d_iters.as<uint32_t>();
    }
    if (c->prof_phases) {
      if (int rc = c->d_prof.ensure(512 + (uint64_t)blocks * 16)) return rc;
      HIPCHK(hipMemsetAsync(c->d_prof.p, 0, 512 + (uint64_t)blocks * 16, c->stream));
      K.prof = c->d_prof.as<unsigned long long>();
      K.wave_t = K.prof + 64;
    }
    HIPCHK(hipEventRecord(c->ev[3], c->stream));
    HIPCHK(launch_width(B, c->block, c->stream));
    HIPCHK(hipEventRecord(c->ev[5], c->stream));
    if (K.proot) HIPCHK(launch_coop_roots(K, counter(c, CTR_CLAIM), blocks, c->stream));
    HIPCHK(hipEventRecord(c->ev[6], c->stream));
    HIPCHK(launch_coop(K, counter(c, CTR_CLAIM), blocks, c->stream));
    HIPCHK(hipEventRecord(c->ev[4], c->stream));
    HIPCHK(hipEventSynchronize(c->ev[4]));
    note_coop_pages(c, S.pool_pages);
    if (c->verbose) fprintf(stderr, "[ibwa_amd] t %.1f ms: coop kernel done\n", R.since());
    if (c->prof_phases)
      if (int rc = print_coop_phases(c, K, blocks)) return rc;
    float a = 0;
    HIPCHK(hipEventElapsedTime(&a, c->ev[3], c->ev[4]));
    R.ms_r += a;
    std::vector<uint32_t> rs(lanes);
    HIPCHK(hipMemcpyAsync(rs.data(), c->pass.r_status.p, lanes * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // reads out of pool pages (reason 3: the pool is shared by the launch's waves) run again in a
    // launch of their own with the whole pool; the others go on to the wide kernel
    std::vector<int64_t> next, next_where;
    for (int64_t j = 0; j < lanes; ++j) {
      if (rs[j] & ST_BAD_SCORE) return fail(IBWA_EINVAL, "score outside the stack range");
      if (rs[j]) {
        const bool again = ((rs[j] >> 8) & 7u) == 3u && round < n_rounds - 1;
        (again ? next : wide_todo).push_back(todo[j]);
        (again ? next_where : wide_where).push_back(where[j]);
        continue;
      }
      R.found_by[where[j]] = 1;
    }
    if (c->verbose)
      if (int rc = print_coop_round(K, rs, blocks, next.size(), a)) return rc;
    if (c->verbose) fprintf(stderr, "[ibwa_amd] t %.1f ms: coop results on host\n", R.since());
    c->stats.n_coop += lanes - (int64_t)next.size() - (int64_t)(wide_todo.size() - wide0);
    c->stats.ms_coop += a;
    {
      float w = 0, rt = 0;
      HIPCHK(hipEventElapsedTime(&w, c->ev[3], c->ev[5]));
      HIPCHK(hipEventElapsedTime(&rt, c->ev[5], c->ev[6]));
      c->stats.ms_coop_width += w;
      c->stats.ms_coop_roots = rt;
    }
    todo.swap(next);
    where.swap(next_where);
  }
  todo.insert(todo.end(), wide_todo.begin(), wide_todo.end());
  where.insert(where.end(), wide_where.begin(), wide_where.end());
  return 0;
}

// IBWA_VERBOSE: a wide launch's longest read (GapArgs::iters in d_iters), a ms
int print_wide_launch(const ibwa_ctx *c, int64_t lanes, float a) {
  std::vector<uint32_t> it(lanes);
  HIPCHK(hipMemcpy(it.data(), c->pass.d_iters.p, lanes * 4, hipMemcpyDeviceToHost));
  const uint32_t mx = *std::max_element(it.begin(), it.end());
  fprintf(stderr, "[ibwa_amd]   wide launch: %lld reads, max %u iterations, %.1f ms (%.2f us/iteration)\n",
          (long long)lanes, mx, a, mx ? a * 1e3 / mx : 0.0);
  return 0;
}

// first two retry rounds: the persistent gapped kernel with 24-bit slot links and one
// large static region per read (4 MiB, then 64 MiB; reads < 4096 bp); then the general kernels
int wide_general_rounds(Run &R) {
  ibwa_ctx *c = R.c;
  const ibwa_gap_opt_t *opt = R.opt;
  const AlnArgs &A = R.A;
  const AlnOpt &o = R.o;
  std::vector<int64_t> &todo = R.todo, &where = R.where;
  uint64_t &cap = R.cap;
  uint32_t &acap = R.acap;
  float &ms_r = R.ms_r;
  int wide_rounds = R.v2 && R.max_len < 4096 ? 2 : 0;
  while (!todo.empty()) {
    const bool wide_round = wide_rounds > 0;
    const uint32_t wide_hits = 4096;
    // live entries never exceed max_entries + 9 (one expansion after the last check)
    const uint64_t need_cap =
        wide_round ? std::min<uint64_t>((uint64_t)opt->max_entries + 64 + wide_hits, wide_rounds == 2 ? 1u << 18 : 1u << 22)
                   : std::min<uint64_t>(cap, (uint64_t)opt->max_entries + 16);
    // keep each retry chunk within ~16 GiB (general kernels) / 48 GiB (gapped wide) of stack scratch
    const uint64_t budget = (wide_round ? 48ull : 16ull) << 30;
    int64_t per = std::max<int64_t>(1, (int64_t)(budget / (need_cap * 20 + acap * 16 + A.wstride * 8 + 64)));
    std::vector<int64_t> next;
    std::vector<int64_t> next_where;
    for (size_t b0 = 0; b0 < todo.size(); b0 += per) {
      int64_t lanes = std::min<int64_t>(per, (int64_t)todo.size() - (int64_t)b0);
      AlnArgs B = A;
      B.cap = (uint32_t)need_cap;
      B.aln_cap = acap;
      if (int rc = c->pass.d_ids.ensure(lanes * 8)) return rc;
      if (int rc = c->pass.d_wbuf.ensure(lanes * A.wstride * 8)) return rc;
      if (int rc = c->pass.d_ent.ensure(lanes * need_cap * 16)) return rc;
      if (!wide_round) {
        if (int rc = c->pass.d_heads.ensure(lanes * (uint64_t)o.n_stacks * 4)) return rc;
        if (int rc = c->pass.d_prev.ensure(lanes * need_cap * 4)) return rc;
      }
      const uint64_t r_total = wide_round ? (uint64_t)lanes * 64 + 65536 : (uint64_t)lanes * acap;
      if (int rc = c->pass.r_aln.ensure(r_total * 16)) return rc;
      if (int rc = c->pass.r_aoff.ensure(lanes * 8)) return rc;
      if (int rc = c->pass.r_naln.ensure(lanes * 4)) return rc;
      if (int rc = c->pass.r_status.ensure(lanes * 4)) return rc;
      HIPCHK(hipMemcpyAsync(c->pass.d_ids.p, todo.data() + b0, lanes * 8, hipMemcpyHostToDevice, c->stream));
      B.wbuf = c->pass.d_wbuf.as<uint2>();
      B.heads = c->pass.d_heads.as<uint32_t>();
      B.ent = c->pass.d_ent.as<uint4>();
      B.prev = c->pass.d_prev.as<uint32_t>();
      B.aln = c->pass.r_aln.as<uint4>();
      B.n_aln = c->pass.r_naln.as<int32_t>();
      B.status = c->pass.r_status.as<uint32_t>();
      float a = 0, b = 0;
      if (wide_round) {
        if (int rc = c->pass.d_nN.ensure(lanes * 2 + 2)) return rc;
        if (int rc = c->d_counter.ensure(64)) return rc;
        B.ids = c->pass.d_ids.as<int64_t>();
        B.n = lanes;
        B.nN = c->pass.d_nN.as<uint16_t>();
        GapArgs G = gap_args(c, A, o, 0, lanes);
        G.ids = B.ids;
        G.out_by_id = 0;
        G.ent = B.ent;
        G.cap1 = (uint32_t)need_cap;
        G.hit_slots = wide_hits;
        G.pool = nullptr;
        G.max_pages = 0;
        G.pages_per_block = 0;
        G.page_log2 = 13;
        G.aln = B.aln;
        G.aln_total = r_total;
        G.aln_next = counter(c, CTR_WIDE_STREAM);
        G.aln_off = c->pass.r_aoff.as<uint64_t>();
        G.n_aln = B.n_aln;
        G.status = B.status;
        if (c->verbose) {
          if (int rc = c->pass.d_iters.ensure(lanes * 4)) return rc;
          G.iters = c->pass.d_iters.as<uint32_t>();
        }
        HIPCHK(zero_async(G.aln_next, 8, c->stream));
        // one heavy read per wave: an iteration then costs only that read's path
        const int blk = 64;
        G.lanes_per_wave = 1;
        G.free_depth = 4096;  // 16 KiB of LDS per heavy read: freed slots are reused, not leaked
        HIPCHK(hipEventRecord(c->ev[3], c->stream));
        HIPCHK(launch_width(B, c->block, c->stream));
        HIPCHK(launch_gapped(G, counter(c, CTR_CLAIM), (int)lanes, blk, true, c->stream));
        HIPCHK(hipEventRecord(c->ev[4], c->stream));
        HIPCHK(hipEventSynchronize(c->ev[4]));
        HIPCHK(hipEventElapsedTime(&a, c->ev[3], c->ev[4]));
        if (c->verbose)
          if (int rc = print_wide_launch(c, lanes, a)) return rc;
      } else {
        if (int rc = run_pass(c, B, lanes, c->pass.d_ids.as<int64_t>(), &a, &b)) return rc;
      }
      ms_r += a + b;
      std::vector<int32_t> rn(lanes);
      std::vector<uint32_t> rs(lanes);
      std::vector<uint64_t> ro(lanes);
      std::vector<uint4> ra(r_total);
      HIPCHK(hipMemcpyAsync(rn.data(), c->pass.r_naln.p, lanes * 4, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(rs.data(), c->pass.r_status.p, lanes * 4, hipMemcpyDeviceToHost, c->stream));
      if (wide_round) HIPCHK(hipMemcpyAsync(ro.data(), c->pass.r_aoff.p, lanes * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(ra.data(), c->pass.r_aln.p, r_total * 16, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      for (int64_t j = 0; j < lanes; ++j) {
        int64_t slot = where[b0 + j];
        if (rs[j] & ST_BAD_SCORE) return fail(IBWA_EINVAL, "score outside the stack range");
        if (rs[j]) {
          next.push_back(todo[b0 + j]);
          next_where.push_back(slot);
          continue;
        }
        const uint64_t first = wide_round ? (rn[j] ? ro[j] : 0) : (uint64_t)j * acap;
        R.patch.emplace_back(todo[b0 + j], std::vector<uint4>(ra.begin() + first, ra.begin() + first + rn[j]));
        R.found_by[slot] = wide_round ? 2 : 3;
      }
    }
    if (c->verbose)
      fprintf(stderr, "[ibwa_amd] retry round (%s, cap %llu): %zu reads, %zu still overflow, %.1f ms so far\n",
              wide_round ? "gapped wide" : "general", (unsigned long long)need_cap, todo.size(), next.size(), ms_r);
    if (wide_round) {
      --wide_rounds;  // what still overflows goes to a larger round, then to the general kernels
      todo.swap(next);
      where.swap(next_where);
      continue;
    }
    if (!next.empty()) {
      if (cap >= (uint64_t)opt->max_entries + 16 && acap >= (1u << 20))
        return fail(IBWA_EOVERFLOW, "read %lld overflowed the large-capacity pass", (long long)next[0]);
      cap *= 16;
      acap = std::min<uint32_t>(acap * 16, 1u << 20);
    }
    todo.swap(next);
    where.swap(next_where);
  }
  return 0;
}

// The patch list for ibwa_batch_fetch and the run's final statistics.
int finish_run(Run &R) {
  ibwa_ctx *c = R.c;
  std::vector<std::pair<int64_t, std::vector<uint4>>> &patch = R.patch;
  // the reads the wide / general passes resolved, in input order, for ibwa_batch_fetch to patch in
  std::sort(patch.begin(), patch.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
  c->res.patch_ids.resize(patch.size());
  c->res.patch_alns.resize(patch.size());
  for (size_t j = 0; j < patch.size(); ++j) {
    c->res.patch_ids[j] = patch[j].first;
    c->res.patch_alns[j].swap(patch[j].second);
  }
  c->res.retry_pass.swap(R.found_by);
  // hit-stream records of the first and cooperative passes; a read whose hits did not fit advanced
  // the fill counter but wrote nothing (ST_ALN_OVERFLOW, re-run above): the records end at stream_total
  if (R.v2 && R.n) {
    HIPCHK(hipMemcpyAsync(&c->res.stream_len, counter(c, CTR_STREAM), 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->res.stream_len = std::min<unsigned long long>(c->res.stream_len, c->res.stream_total);
    unsigned long long tj = 0;
    HIPCHK(hipMemcpy(&tj, counter(c, CTR_TAIL_JUMPS), 8, hipMemcpyDeviceToHost));
    c->stats.n_tail_jumps = (int64_t)tj;
    if (R.A.tab_steps) {
      HIPCHK(hipMemcpy(&tj, counter(c, CTR_WIDTH_TAB), 8, hipMemcpyDeviceToHost));
      c->stats.n_width_tab_steps = (int64_t)tj;
    }
  }
  c->stats.ms_retry = R.ms_r + R.res_ms;
  c->stats.n_retry = (int64_t)c->res.retry_ids.size() + R.res_ok;
  c->stats.ms_total = R.since();
  c->stats.ms_alloc = g_alloc_ms;
  return 0;
}

}  // namespace

extern "C" {

int ibwa_batch_run(ibwa_ctx_t *c, const ibwa_gap_opt_t *opt, int batch_max_len) {
  Run R;
  R.c = c;
  R.opt = opt;
  R.t0 = std::chrono::steady_clock::now();
  if (int rc = run_setup(R, batch_max_len)) return rc;
  if (R.exact_path) return exact_pass(R);
  if (int rc = R.v2 ? first_pass_persistent(R) : first_pass_legacy(R)) return rc;
  if (int rc = select_handed_on_reads(R)) return rc;
  if (int rc = coop_rounds(R)) return rc;
  if (int rc = wide_general_rounds(R)) return rc;
  return finish_run(R);
}

int ibwa_batch_retry_info(const ibwa_ctx_t *c, int64_t *ids, uint8_t *pass, int64_t cap, int64_t *n) {
  const int64_t m0 = (int64_t)c->res.retry_ids.size(), m = m0 + (int64_t)c->res.resumed_ids.size();
  for (int64_t j = 0; j < std::min(m, cap); ++j) {
    if (ids) ids[j] = j < m0 ? c->res.retry_ids[j] : c->res.resumed_ids[j - m0];
    if (pass) pass[j] = j >= m0 ? 4 : j < (int64_t)c->res.retry_pass.size() ? c->res.retry_pass[j] : 0;
  }
  if (n) *n = m;
  return 0;
}

int ibwa_batch_diag(const ibwa_ctx_t *c, int what, void *out, uint64_t cap_bytes) {
  if (what >= 3 && what <= 5) {
    // the first-pass chunk's k_width outputs, kept by the run under option diag_width (the whole batch
    // when it ran as one chunk): 3 its width rows, 4 its compact records, 5 their shape {reads, wstride,
    // cw_words}
    const void *src = what == 3 ? (const void *)c->res.diag_w.data()
                      : what == 4 ? (const void *)c->res.diag_cw.data() : (const void *)c->res.diag_shape;
    const uint64_t need3 = what == 3 ? c->res.diag_w.size() * 8 : what == 4 ? c->res.diag_cw.size() * 4 : 24;
    if (cap_bytes < need3) return fail(IBWA_EINVAL, "diag buffer too small");
    if (need3) memcpy(out, src, need3);
    return 0;
  }
  if (what == 2) {
    const uint64_t need2 = (uint64_t)c->batch.n * 4;
    if (cap_bytes < need2) return fail(IBWA_EINVAL, "diag buffer too small");
    if (!c->pass.hpop_valid || c->pass.d_hpop.cap < need2) {  // no resume states in the last run
      memset(out, 0, need2);
      return 0;
    }
    if (c->batch.n == 0) return 0;
    HIPCHK(enter(c));
    HIPCHK(hipMemcpy(out, c->pass.d_hpop.p, need2, hipMemcpyDeviceToHost));
    return 0;
  }
  const uint64_t need = what == 0 ? (uint64_t)c->batch.n * 4 : (uint64_t)c->batch.n * 8;
  if (!c->diag || (what != 0 && what != 1)) return fail(IBWA_EINVAL, "set option diag=1 before the run; what = 0 or 1");
  if (cap_bytes < need) return fail(IBWA_EINVAL, "diag buffer too small");
  if (c->batch.n == 0) return 0;
  HIPCHK(enter(c));
  HIPCHK(hipMemcpy(out, (what == 0 ? c->pass.d_iters : c->pass.d_feat).p, need, hipMemcpyDeviceToHost));
  return 0;
}

// the batch's results to the host once (h_naln / h_aoff / h_aln), and per read its hit count with
// the wide / general passes' patches in (c->res.h_cnt)
// huge pages for a large host array (fewer faults, and fewer page tables to tear down at exit)
static void advise_huge(const void *p, size_t bytes) {
  const uintptr_t a = (reinterpret_cast<uintptr_t>(p) + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1);
  const uintptr_t e = (reinterpret_cast<uintptr_t>(p) + bytes) & ~(uintptr_t)((2u << 20) - 1);
  if (e > a) (void)madvise(reinterpret_cast<void *>(a), e - a, MADV_HUGEPAGE);
}

static int fetch_to_host(ibwa_ctx_t *c) {
  if (c->res.fetched) return 0;
  const int64_t n = c->batch.n;
  const uint32_t cap = c->res.aln_cap_used;
  const uint64_t n_slots = c->res.stream_out ? c->res.stream_len : (uint64_t)n * cap;
  if (c->res.h_aln.capacity() < n_slots) {
    std::vector<uint4>().swap(c->res.h_aln);
    c->res.h_aln.reserve(n_slots + n_slots / 8);  // not touched yet: huge pages advised first
    advise_huge(c->res.h_aln.data(), c->res.h_aln.capacity() * sizeof(uint4));
  }
  c->res.h_aln.resize(std::max<uint64_t>(n_slots, 1));
  if (n) {
    HIPCHK(enter(c));
    if (!c->res.naln_on_host) {
      c->res.h_naln.resize(n);
      HIPCHK(hipMemcpyAsync(c->res.h_naln.data(), c->pass.d_naln.p, n * 4, hipMemcpyDeviceToHost, c->stream));
      c->res.naln_on_host = true;
    }
    if (c->res.stream_out) {
      c->res.h_aoff.resize(n);
      HIPCHK(hipMemcpyAsync(c->res.h_aoff.data(), c->pass.d_aoff.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (n_slots) HIPCHK(hipMemcpyAsync(c->res.h_aln.data(), c->pass.d_aln.p, n_slots * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  c->res.h_cnt.assign(c->res.h_naln.begin(), c->res.h_naln.begin() + n);
  for (size_t j = 0; j < c->res.patch_ids.size(); ++j) c->res.h_cnt[c->res.patch_ids[j]] = (int32_t)c->res.patch_alns[j].size();
  c->res.fetched = true;
  return 0;
}

int ibwa_batch_fetch_sai(ibwa_ctx_t *c, void *dst, uint64_t cap_bytes, uint64_t *bytes, int64_t *n_total) {
  if (!c || !bytes) return fail(IBWA_EINVAL, "fetch_sai: bad arguments");
  if (int rc = fetch_to_host(c)) return rc;
  const int64_t n = c->batch.n;
  const uint32_t cap = c->res.aln_cap_used;
  const int32_t *cnt = c->res.h_cnt.data();
  // per range of reads (one per host thread): its bytes and hits, then the ranges' offsets
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(16, n >> 16));
  std::vector<uint64_t> bo(T + 1, 0), ho(T + 1, 0);
  auto ranges = [&](auto &&fn) {
    if (T == 1) { fn(0); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back(fn, t);
    for (auto &x : th) x.join();
  };
  ranges([&](int t) {
    uint64_t h = 0;
    for (int64_t i = n * t / T; i < n * (t + 1) / T; ++i) h += (uint64_t)cnt[i];
    ho[t + 1] = h;
    bo[t + 1] = h * 16 + (uint64_t)(n * (t + 1) / T - n * t / T) * 4;
  });
  for (int t = 0; t < T; ++t) {
    bo[t + 1] += bo[t];
    ho[t + 1] += ho[t];
  }
  *bytes = bo[T];
  if (n_total) *n_total = (int64_t)ho[T];
  if (!dst || cap_bytes < bo[T]) return 0;
  ranges([&](int t) {
    char *w = static_cast<char *>(dst) + bo[t];
    const int64_t lo = n * t / T;
    size_t rj = std::lower_bound(c->res.patch_ids.begin(), c->res.patch_ids.end(), lo) - c->res.patch_ids.begin();
    for (int64_t i = lo; i < n * (t + 1) / T; ++i) {
      const int32_t k = cnt[i];
      const uint4 *src;
      if (rj < c->res.patch_ids.size() && c->res.patch_ids[rj] == i) {
        src = c->res.patch_alns[rj].data();
        ++rj;
      } else {
        src = c->res.h_aln.data() + (c->res.stream_out ? (k ? c->res.h_aoff[i] : 0) : (uint64_t)i * cap);
      }
      memcpy(w, &k, 4);
      if (k) memcpy(w + 4, src, (size_t)k * 16);
      w += 4 + (size_t)k * 16;
    }
  });
  return 0;
}

int ibwa_batch_fetch(ibwa_ctx_t *c, int32_t *n_aln, ibwa_aln1_t **aln, int64_t *n_total) {
  const int64_t n = c->batch.n;
  const uint32_t cap = c->res.aln_cap_used;
  // first-pass hits (per-read slots n x cap, or the hit stream + per-read offsets) to the host, with
  // the reads the wide / general passes resolved patched in (the first and cooperative passes wrote
  // theirs into d_naln / d_aln)
  if (int rc = fetch_to_host(c)) return rc;
  const std::vector<int32_t> &cnt = c->res.h_cnt;
  std::vector<int64_t> at(n + 1, 0);  // output offset of read i
  for (int64_t i = 0; i < n; ++i) at[i + 1] = at[i] + cnt[i];
  const int64_t tot = at[n];
  ibwa_aln1_t *o = (ibwa_aln1_t *)malloc(std::max<int64_t>(tot, 1) * sizeof(ibwa_aln1_t));
  if (!o) return fail(IBWA_EINVAL, "out of host memory");
  // the records in input order, gathered by several host threads (patch_ids ascending)
  auto gather = [&](int64_t lo, int64_t hi) {
    size_t rj = std::lower_bound(c->res.patch_ids.begin(), c->res.patch_ids.end(), lo) - c->res.patch_ids.begin();
    for (int64_t i = lo; i < hi; ++i) {
      const uint4 *src;
      if (rj < c->res.patch_ids.size() && c->res.patch_ids[rj] == i) {
        src = c->res.patch_alns[rj].data();
        ++rj;
      } else {
        src = c->res.h_aln.data() + (c->res.stream_out ? (cnt[i] ? c->res.h_aoff[i] : 0) : i * cap);
      }
      memcpy(o + at[i], src, (size_t)cnt[i] * 16);
      if (n_aln) n_aln[i] = cnt[i];
    }
  };
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(16, n / 65536));
  if (nt == 1) {
    gather(0, n);
  } else {
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back(gather, n * t / nt, n * (t + 1) / nt);
    for (auto &x : th) x.join();
  }
  *aln = o;
  if (n_total) *n_total = tot;
  return 0;
}

int ibwa_ctx_prepare(ibwa_ctx_t *c, const ibwa_gap_opt_t *opt) {
  if (!c) return fail(IBWA_EINVAL, "null context");
  HIPCHK(enter(c));
  if (int rc = ensure_kmer(c)) return rc;
  // the condition of ibwa_batch_run's exact path
  if (opt && c->exact_path && !(opt->fnr > 0.0f) && opt->max_diff == 0 && opt->max_entries >= 2)
    if (int rc = ensure_jump(c)) return rc;
  return 0;
}

int ibwa_batch_stats(const ibwa_ctx_t *c, ibwa_run_stats_t *st) {
  *st = c->stats;
  return 0;
}

int ibwa_aln_batch(ibwa_ctx_t *c, const ibwa_gap_opt_t *opt, int64_t n, const uint8_t *seq, const uint64_t *off,
                   const uint32_t *len, int batch_max_len, int32_t *n_aln, ibwa_aln1_t **aln, int64_t *n_total) {
  if (int rc = ibwa_batch_stage(c, n, seq, off, len)) return rc;
  if (int rc = ibwa_batch_run(c, opt, batch_max_len)) return rc;
  return ibwa_batch_fetch(c, n_aln, aln, n_total);
}

}  // extern "C"
