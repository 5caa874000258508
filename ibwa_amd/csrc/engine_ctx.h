// engine_ctx.h -- what the host units of the C ABI (engine_*.hip) share: error reporting, the device
// buffer type, and the context.  Private to ibwa_amd/csrc.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "engine.h"
#include "ibwa_aln.h"

namespace ibwa {

// the message ibwa_last_error returns on this thread; fail() sets it and returns `code`
extern thread_local std::string g_err;
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIPCHK(x)                                                                                    \
  do {                                                                                               \
    hipError_t e_ = (x);                                                                             \
    if (e_ != hipSuccess) return fail(IBWA_EHIP, "%s:%d %s: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
  } while (0)

// hipMalloc wall time of this thread (a run reports what it spent: ibwa_run_stats_t.ms_alloc)
extern thread_local double g_alloc_ms;
// the stream of the context this thread's API call works on
extern thread_local hipStream_t g_stream;

// A growable device buffer (carved from the device's arena when one is reserved).  It owns what it
// holds: moving hands the range on, destruction returns it.  free_dev synchronises g_stream before it
// returns an arena range, so a context's buffers die while its stream is alive and g_stream names it.
struct DBuf {
  void *p = nullptr;
  size_t cap = 0;
  bool borrowed = false;  // another context's buffer (ibwa_ctx_share_index): never freed or grown here
  DBuf() = default;
  DBuf(const DBuf &) = delete;
  DBuf &operator=(const DBuf &) = delete;
  DBuf(DBuf &&o) noexcept : p(o.p), cap(o.cap), borrowed(o.borrowed) { o.forget(); }
  DBuf &operator=(DBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      cap = o.cap;
      borrowed = o.borrowed;
      o.forget();
    }
    return *this;
  }
  ~DBuf() { release(); }
  int ensure(size_t bytes);
  static void free_dev(void *q, size_t n);
  void release() {
    if (p && !borrowed) free_dev(p, cap);
    forget();
  }
  DBuf borrow() const {  // a non-owning view
    DBuf b;
    b.p = p;
    b.cap = cap;
    b.borrowed = true;
    return b;
  }
  template <class T> T *as() const { return (T *)p; }

 private:
  void forget() {
    p = nullptr;
    cap = 0;
    borrowed = false;
  }
};

// A FASTQ parse's device scratch (ibwa_fq_parse): the raw block, its line table, per-record lengths
// and scan keys.  Only the kept reads' codes, offsets and lengths outlive a parse, so the ingest
// contexts of one device that never parse at the same time share one scratch (ibwa_fq_share_scratch).
struct FqScratch {
  int refs = 1;
  const void *last = nullptr;  // the context whose block the line table holds (ibwa_fq_offset)
  DBuf raw, tile, nl, cnt, len, L, key, tmp;
  uint32_t *hinit = nullptr;  // pinned: the parse counters' initial values, then zeros for the padding
  // a block in pageable memory (the CLI's mapped file) goes to the device through two pinned
  // staging chunks, filled by host threads: left to the HIP runtime, a pageable copy locks the
  // file's pages, and unlocking GBs of them cost ~0.3 s at process exit (profiles/r05_e2e_g.json)
  static constexpr size_t kStage = 64u << 20;
  char *stage[2] = {nullptr, nullptr};
  hipEvent_t sev[2] = {nullptr, nullptr};
  FqScratch() = default;
  FqScratch(const FqScratch &) = delete;
  FqScratch &operator=(const FqScratch &) = delete;
  ~FqScratch() {
    if (hinit) (void)hipHostFree(hinit);
    for (int i = 0; i < 2; ++i) {
      if (stage[i]) (void)hipHostFree(stage[i]);
      if (sev[i]) (void)hipEventDestroy(sev[i]);
    }
  }
  void unref() {
    if (--refs == 0) delete this;
  }
  // src[0, n) to device dst on stream st
  hipError_t h2d(void *dst, const void *src, size_t n, hipStream_t st);
};

// A context's stream and events.  The context's base, so they are destroyed after every member:
// the buffers' release still synchronises the stream.
struct CtxQueue {
  hipStream_t stream = nullptr;
  hipEvent_t ev[8] = {};
  CtxQueue() = default;
  CtxQueue(const CtxQueue &) = delete;
  CtxQueue &operator=(const CtxQueue &) = delete;
  ~CtxQueue() {
    for (auto &x : ev)
      if (x) (void)hipEventDestroy(x);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// The index set a context searches: per strand the Occ blocks and everything derived from them, the
// state that says what is resident, and the packed reference(s).  ibwa_ctx_share_index lends it as a
// unit (borrow_index below).
struct IndexSet {
  DBuf idx[2];
  IndexView ix[2] = {};
  bool loaded[2] = {false, false};
  int build_rounds[2] = {0, 0};
  // bit-plane Occ layouts (occ64.hip) and K-mer interval tables for the exact-match path (kmer.hip)
  DBuf o64[2], kt[2];
  // level tables of the LW first pass (GapArgs::ltab): strings of length <= gap_tab_k + 1 (0: off;
  // -1: auto, floor(log4(n)) up to 13 -- 2 x 2.9 GB at GRCh37 size -- or 14 with room, ensure_kmer),
  // built with the K-mer tables
  // (ensure_kmer).  Measured at 50 M reads (profiles/r06_sweep_tab.jsonl, hits identical): k_gapped
  // 2 476 ms per step without, 2 149 / 2 027 / 1 947 ms with K = 10 / 12 / 13.
  DBuf ltab[2];
  int ltab_K = 0;   // tab_k of the built level tables
  int kmer_K = 0;   // K of the built tables
  bool kmer_valid = false;
  // sampled suffix arrays kept by ibwa_ctx_build_index
  DBuf sa_s[2];
  uint32_t sa_intv = 0;
  bool sa_loaded[2] = {false, false};  // sa_s[s] holds a sampled SA of the resident index
  // full SA / ISA and 2-bit texts of an index built here: the exact path's unique-interval jump
  DBuf sa_full[2], isa_full[2], txt2[2];
  bool sa_expanded = false;   // sa_full[0/1] derived from the sampled SA (ibwa_ctx_expand_sa)
  bool jump_ready = false;
  bool jump_derived = false;  // jump arrays derived from a loaded BWT (ensure_jump), not built here
  // the packed reference (ibwa_ctx_load_pac)
  DBuf pac;
  uint64_t pac_len = 0;  // the set's l_pac
  bool pac_loaded = false;
  // the nucleotide sequence of a colour-space set (ibwa_ctx_load_ntpac)
  DBuf ntpac;
  uint64_t ntpac_len = 0;
  bool ntpac_loaded = false;
};

// The staged batch: d_seq / d_off / d_len, or (ibwa_batch_stage_fq) a parsed block's kept reads.
struct Batch {
  DBuf d_seq, d_off, d_len;
  const uint8_t *v_seq = nullptr;
  const uint64_t *v_off = nullptr;
  const uint32_t *v_len = nullptr;
  int64_t n = 0;
  uint64_t seq_bytes = 0;
  int max_len = 0;
};

// Results of the last run: where they are, and the host's copy (fetch_to_host).
struct Results {
  std::vector<int32_t> h_naln;
  std::vector<uint32_t> h_status;
  std::vector<uint4> h_aln;      // n * aln_cap slots
  std::vector<int64_t> retry_ids;                   // every read a later pass resolved (input order)
  std::vector<int64_t> patch_ids;                   // ... of which the wide / general passes' (input order)
  std::vector<std::vector<uint4>> patch_alns;       // their hits (the coop pass writes into d_aln / d_naln)
  std::vector<uint8_t> retry_pass;  // per retry_ids entry: 1 coop, 2 wide, 3 general kernels
  std::vector<int64_t> resumed_ids; // reads the cooperative pass resolved from a resume state (retry_info pass 4)
  std::vector<uint64_t> h_aoff;
  std::vector<int32_t> h_cnt;  // per read its hits, patches included (fetch_to_host)
  uint32_t aln_cap_used = 0;
  bool stream_out = false;           // d_aln is a hit stream indexed by d_aoff
  unsigned long long stream_len = 0;  // hit-stream records written by the first pass (<= stream_total)
  unsigned long long stream_total = 0;  // hit-stream slots of the last first-pass launch
  bool naln_on_host = true;  // h_naln mirrors d_naln
  bool fetched = false;       // the batch's results are on the host (fetch_to_host; a run resets it)
  // option diag_width: the first-pass chunk's width rows and compact records as k_width wrote them
  // (ibwa_batch_diag 3 / 4), and their shape {reads, wstride, cw_words}
  std::vector<uint2> diag_w;
  std::vector<uint32_t> diag_cw;
  uint64_t diag_shape[3] = {0, 0, 0};
};

// Scratch and device outputs of the first pass, the wide pass and the general kernels.
struct PassScratch {
  DBuf d_wbuf, d_heads, d_ent, d_prev, d_aln, d_naln, d_status, d_tab, d_ids;
  DBuf r_aln, r_naln, r_status;  // retry pass outputs (r_status: the cooperative launches' too)
  DBuf d_nN, d_pool, d_aoff, r_aoff, d_iters;
  DBuf d_cw, d_ptabg;
  DBuf d_rdump, d_roff;
  DBuf d_hpop;           // per read: first-pass pops before its resume state (0: none; ibwa_batch_diag 2)
  bool hpop_valid = false;
  DBuf d_feat;           // option diag: k_width features
};

// Scratch of the wave-cooperative heavy-read pass (coop.hip).
struct CoopBufs {
  DBuf c_stg, c_dir, c_free, c_pool, c_hits, c_next, c_recb, c_proot, c_pstore;
  DBuf d_selst, d_seltmp;                           // statuses of the handed-on reads, select scratch
  DBuf d_ordk, d_ordi, d_ordids, d_ordtmp;          // the coop pass's order (largest first-pass stack first)
};

// sw_batch's buffers (kept between calls), under the names its functions use.  ibwa_refine_batch
// fills seq1 / off1 / len1 on the device and runs the same launch; ibwa_pac_extract borrows o1 (its
// output offsets) and s1 (its output bytes).
struct SwBufs {
  DBuf s1, s2, o1, o2, l1, l2;  // seq1, seq2, off1, off2, len1, len2
  DBuf sc, pl, nc, en, cg;      // score, path_len, n_cigar, ends, CIGAR rows
  DBuf scr, tbb;                // DP scratch, traceback
  DBuf cf, cc;                  // packed CIGARs: each row's first word, the words
};
// ibwa_stdaln_batch's and ibwa_extend_batch's buffers (kept between calls).  g0 / pos / dir: the
// extension's G0 per pair and ibwa_extend_seeds' positions and directions.
struct StdBufs {
  DBuf s1, s2, o1, o2, l1, l2, mat;
  DBuf g0, pos, dir;
  DBuf sc, su, pl, nc, en, cg;  // score, subo, path_len, n_cigar, ends, a chunk's CIGAR rows
  DBuf scr, tbb, cf, cc;        // DP scratch, traceback, packed CIGARs (first words, words)
};
// ibwa_bsw2_seed_batch's buffers (kept between calls).
struct SeedBufs {
  DBuf seq, off, len, strand, t, bw, ids, arena, res, out, ctr;
};
// the buffers of k_bsw2_extend's launches (ibwa_bsw2_aln1_batch, ibwa_bsw2_extend_left_batch; kept between calls).
struct Bsw2ExtBufs {
  DBuf qry, qoff, qlen, bw, rev, hoff, hits, htask, tgt, eh, status, ctr;
};
// ibwa_refine_batch's own buffers.  ibwa_pac_extract borrows them for its begins, lengths and got
// counts (dpos, dext, dout in that order).
struct RefineBufs {
  DBuf dpos, dext, dout;
};
// ibwa_md_batch's buffers.
struct MdBufs {
  DBuf dpos, dseq, doff, dlen, dnc, dco, dcg, dto, dnm, dtx, dtmp;
};
// Colour space.  din / dout_cs: ibwa_pac2cspac.  dbt: k_cs2nt's position-major scratch (cs2nt_run).
// The job arrays carry ibwa_cs2nt_batch's names; ibwa_cs2nt_rows borrows dseq / dq / doff / dsz / dout /
// dpos for its reference rows, colour rows, offsets, sizes, output and output offsets.
struct CsBufs {
  DBuf din, dout_cs;
  DBuf dbt;
  DBuf dseq, dq, doff, dsz, dout, dpos;
  DBuf dst, dlen, dnc, dco, dcg;
};

}  // namespace ibwa

struct ibwa_ctx : ibwa::CtxQueue {
  using DBuf = ibwa::DBuf;
  int device = 0;
  ibwa::IndexSet index;
  ibwa::Batch batch;
  ibwa::Results res;
  ibwa::PassScratch pass;
  ibwa::CoopBufs coop;
  DBuf d_rec;                // the exact path's packed reads
  DBuf d_counter, d_prof;    // every pass's: the device counters (CounterSlot), IBWA_PROF_PHASES counters
  DBuf h2p_in, h2p_out;      // staging of ibwa_sa2pos
  // post-alignment services
  ibwa::SwBufs sw;
  ibwa::StdBufs sd;
  ibwa::SeedBufs seed;
  ibwa::Bsw2ExtBufs bext;
  ibwa::RefineBufs rf;
  ibwa::MdBufs md;
  ibwa::CsBufs cs;
  ibwa_run_stats_t stats = {};
  // ibwa_ctx_share_index: the context whose index structures this one borrows, and how many
  // contexts borrow this one's; neither side may rebuild or replace them while shared
  ibwa_ctx *share_src = nullptr;
  int n_borrowers = 0;
  bool destroy_pending = false;  // destroyed while borrowed: freed with its last borrower
  // FASTQ ingest (fastq.hip, ibwa_fq_parse): the last parsed block and its kept reads
  DBuf fq_codes, fq_offk, fq_lenk;  // the last parsed block's kept reads (ibwa_batch_stage_fq's views)
  ibwa::FqScratch *fqs = nullptr;   // parse scratch, own or shared (ibwa_fq_share_scratch)
  int64_t fq_kept = 0;
  double fq_ms = 0;  // device time of the last parse (H2D copy + kernels), HIP events
  ~ibwa_ctx() {
    if (fqs) fqs->unref();
  }

  // options and tuning
  int coop_roots = 1;                               // option: level 0 of the heavy reads by k_coop_roots
  int jump_derive = 1;        // option: derive the jump arrays for a loaded index when HBM allows
  int exact_jump = 1;
  int width_tab = 2;           // option: k_width's steps from the level tables (1: a chain's first; 2: and after resets)
  int width_rec_stage = 1;     // option: k_width stages its compact records in LDS and stores them whole
  int diag_width = 0;          // option: keep the first-pass chunk's k_width outputs (ibwa_batch_diag 3 / 4)
  int gap_tail_tab = 1;        // option: exact tails of nodes stored by their strings jump by the level tables
  int width_jump = 1;         // option: k_width steps one-row intervals from the text (2: derive SA / text for it)
  int sa_walk = 0;                     // option: always walk the sampled SA (parity / low-memory)
  uint32_t stack_cap = 4096, aln_cap = 8;
  int block = 256;
  int64_t lanes_per_chunk = 1 << 18;
  int exact_path = 1;       // use k_exact when max_diff == 0
  int exact_blocks = 2048;  // persistent grid of k_exact (set from the CU count)
  int n_cus = 256;
  // persistent gapped search (gapped.hip)
  int gapped_v2 = 1;
  int gap_blocks_per_cu = 3;         // 134 VGPRs -> 3 waves per SIMD
  uint32_t gap_cap1 = 8192;          // per-lane static slots (stack + hit area)
  int gap_pages_per_block = 384;      // 128 KiB pages per 256-lane workgroup pool
  uint32_t gap_hit_slots = 256;      // hits a read may hold in the first pass
  int64_t gap_reads_per_chunk = 1 << 24;  // at most; a batch is cut into equal chunks (each chunk's last reads run alone)
  // early hand-off to the coop pass: a read past 3000 iterations whose stack holds > 1000 entries
  // (swept at 10M reads: 2.28 -> 2.14 s per step; budget 6000-16000 with it: within noise)
  uint32_t gap_early_iters = 3000, gap_early_entries = 1000;
  uint32_t gap_iter_budget = 8000;   // first-pass iterations per read before handing it to the coop pass (swept 1000-8000 at 50M reads: 8000 best)
  // wave-cooperative heavy-read pass (coop.hip)
  int gap_coop = 1;
  int coop_early = 1;                // k_coop issues a wave-iteration's claims and loads before its control section
  int gap_lw = 1;                    // first pass with its widths in LDS (gapped.hip LW) when they fit
  int gap_lw_min_waves = 8;          // ... in a workgroup size that keeps at least this many waves per CU
  int gap_resume = 1;                // early hand-offs leave their search state for the coop pass (LW)
  int gap_resume_gb = 48;            // state buffer: at most this many GiB ...
  // ... sized per read of a first-pass chunk: this many 16 B records (100 bp reads at 1 % need ~160
  // per read at the busiest chunk), or the most an earlier run's chunk needed (x 1.15) if more --
  // states that do not fit are not lost work only: their reads start over in the cooperative pass
  uint32_t gap_resume_recs = 192;
  double resume_need = 0;            // the most records per chunk read a run of this context requested
  int coop_stg_room = 1;             // k_coop's per-lane staging ring: this many chains' children (2: same time)
  int64_t gap_resume_records = 0;    // tests: state buffer of this many 16 B records (0: by gap_resume_gb)
  // the early hand-off rule when the read leaves a resume state (nothing is re-run, so it pays to hand
  // on earlier: swept at 50M reads, flat optimum, profiles/r03_resume_sweep*.log)
  uint32_t gap_resume_iters = 2000, gap_resume_entries = 300;
  // resume in a launch's tail (GapArgs::tail_lanes): 16 / 200 measured 5868 vs 5884 ms per 50M-read
  // step (profiles/r03_tail_sweep.log; 8, 32, 4 / 500 in between)
  uint32_t gap_tail_lanes = 16, gap_tail_iters = 200;
  // first-pass pages per 256-lane pool when states are left (<= gap_pages_per_block): 96 -> 48 cost
  // nothing measurable at 100 or 150 bp (profiles/r04_sweep_mem*.jsonl)
  int gap_resume_ppb = 48;
  uint32_t gap_resume_cap1 = 4096;   // first-pass static slots per lane when states are left (<= gap_cap1)
  int coop_waves_per_cu = 12;        // 13.3 KiB of LDS and 168 VGPRs per wave (3 waves per SIMD)
  // bucket page pool, GiB (0: by read length -- 10 up to 128 bp, 16 above: at 100 bp 10 GiB costs
  // nothing, 5 322 vs 5 316 ms per 50 M-read step; at 150 bp / 2 % it cost 7 %, profiles/r05_sweep_mem*.jsonl)
  int coop_pool_gb = 0;
  uint64_t pool_bytes(int max_len) const { return (uint64_t)(coop_pool_gb ? coop_pool_gb : max_len <= 128 ? 10 : 16) << 30; }
  uint32_t coop_pool_pages = 0;      // tests: the pool in pages (0: by coop_pool_gb)
  bool verbose = getenv("IBWA_VERBOSE") != nullptr;
  bool prof_phases = getenv("IBWA_PROF_PHASES") != nullptr;  // diagnostics kernel variant
  int sw_stop_after = getenv("IBWA_SW_STOP") ? atoi(getenv("IBWA_SW_STOP")) : 0;  // diagnostics
  int64_t stdaln_scratch_mb = 32768;  // option: device scratch of one ibwa_stdaln_batch launch, MiB
  int64_t stdaln_suba_rows = 8192;   // option: keep suba (one entry per row of seq2) up to this many rows
  int64_t stdaln_chunks = 0;         // launches the last ibwa_stdaln_batch took
  double stdaln_ms = 0;              // ... and their kernel time
  int64_t seed_arena_cells = 0;      // option: cells of a task's arena in k_bsw2_seed's first launch (0: by read length)
  int seed_waves_per_cu = 8;         // option: its persistent waves per CU (18 KiB of LDS each)
  int64_t seed_stats[8] = {};        // ibwa_bsw2_seed_stats
  int bsw2_ext_waves_per_cu = 0;     // option: k_bsw2_extend's persistent waves per CU (0: what the LDS admits, 8 at most)
  int64_t aln1_stats[8] = {};        // ibwa_bsw2_aln1_stats
  int64_t extend_no_band = 0;        // path-mode pairs of the last extension whose global fill stayed below the extension score
  int diag = 0;                      // option: keep per-read first-pass iterations and k_width features
  uint32_t gap_stream_per_read = 4;     // first-pass hit-stream slots per read
  uint64_t gap_stream_min = 1u << 20;   // ... and at least this many in total
  int gap_tab_k = -1;  // level tables' depth (IndexSet::ltab; -1: auto, 0: off)
  int kmer_k = -1;     // requested K (-1: auto from the genome size, 0: off)
};

namespace ibwa {

// What "borrow an index" (ibwa_ctx_share_index) copies: non-owning views of every index buffer of
// src, the state that describes them, and the options they were built or are searched with.  dst's
// own index buffers are released as the views replace them.
inline void borrow_index(ibwa_ctx *dst, const ibwa_ctx *src) {
  IndexSet &D = dst->index;
  const IndexSet &S = src->index;
  for (int s = 0; s < 2; ++s) {
    D.idx[s] = S.idx[s].borrow();
    D.o64[s] = S.o64[s].borrow();
    D.kt[s] = S.kt[s].borrow();
    D.ltab[s] = S.ltab[s].borrow();
    D.sa_s[s] = S.sa_s[s].borrow();
    D.sa_full[s] = S.sa_full[s].borrow();
    D.isa_full[s] = S.isa_full[s].borrow();
    D.txt2[s] = S.txt2[s].borrow();
    D.ix[s] = S.ix[s];
    D.loaded[s] = true;
    D.sa_loaded[s] = S.sa_loaded[s];
    D.build_rounds[s] = S.build_rounds[s];
  }
  D.pac = S.pac.borrow();
  D.pac_len = S.pac_len;
  D.pac_loaded = S.pac_loaded;
  D.ntpac = S.ntpac.borrow();
  D.ntpac_len = S.ntpac_len;
  D.ntpac_loaded = S.ntpac_loaded;
  D.kmer_K = S.kmer_K;
  D.ltab_K = S.ltab_K;
  D.kmer_valid = S.kmer_valid;
  D.sa_intv = S.sa_intv;
  D.sa_expanded = S.sa_expanded;
  D.jump_ready = S.jump_ready;
  D.jump_derived = S.jump_derived;
  dst->kmer_k = src->kmer_k;
  dst->gap_tab_k = src->gap_tab_k;
  dst->jump_derive = src->jump_derive;
  dst->exact_jump = src->exact_jump;
  dst->width_jump = src->width_jump;
  dst->width_tab = src->width_tab;
  dst->gap_tail_tab = src->gap_tail_tab;
}

// An API call's entry: the context's device, and its stream for the arena (DBuf::free_dev).
inline hipError_t enter(const ibwa_ctx *c) {
  g_stream = c->stream;
  return hipSetDevice(c->device);
}

inline unsigned long long *counter(const ibwa_ctx *c, CounterSlot s) { return c->d_counter.as<unsigned long long>() + s; }

// An operation that would rebuild or replace index structures shared by ibwa_ctx_share_index
// (borrowed buffers are written in place or cannot grow, and the other context may be aligning).
int refuse_shared(const ibwa_ctx *c, const char *what);
// (Re)build the K-mer and level tables for the resident index if needed (engine_index.hip).
int ensure_kmer(ibwa_ctx *c);
// The exact path's jump arrays for a loaded index, when HBM allows (engine_index.hip).
int ensure_jump(ibwa_ctx *c);
int derive_sa_locked(ibwa_ctx *c, uint32_t intv);

}  // namespace ibwa
