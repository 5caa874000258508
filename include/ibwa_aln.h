/*
 * ibwa_aln.h -- C ABI of the MI355X `ibwa aln` engine (libibwa_amd.so).
 *
 * Plain pointers and sizes only.  Each entry point names the reference
 * interface it replaces.  The drop-in that keeps the reference's own types
 * (`bwa_cal_sa_reg_gap` itself) is in ibwa_bwa_compat.h.
 *
 * Error convention: functions return 0 on success and a negative IBWA_E*
 * code on failure; ibwa_last_error() gives a message.  There is no CPU
 * fallback: without a usable gfx950 device every compute call fails.
 */
#ifndef IBWA_ALN_H
#define IBWA_ALN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
	IBWA_OK = 0,
	IBWA_EHIP = -1,      /* HIP runtime error (no device, OOM, launch failure) */
	IBWA_EINVAL = -2,    /* bad argument / unsupported option combination */
	IBWA_ENOINDEX = -3,  /* index not loaded */
	IBWA_EIO = -4,       /* file I/O */
	IBWA_EOVERFLOW = -5  /* a read exceeded even the large-capacity retry pass */
};

/* gap_opt_t (bwtaln.h:105-115); also the raw 64-byte .sai header (bwtaln.c:192) */
typedef struct {
	int s_mm, s_gapo, s_gape;
	int mode; /* bits 24-31: barcode length */
	int indel_end_skip, max_del_occ, max_entries;
	float fnr;
	int max_diff, max_gapo, max_gape;
	int max_seed_diff, seed_len;
	int n_threads;
	int max_top2;
	int trim_qual;
} ibwa_gap_opt_t;

/* bwt_aln1_t (bwtaln.h:34-38): one SA interval hit, 16 bytes, the .sai record */
typedef struct {
	uint32_t n_mm:8, n_gapo:8, n_gape:8, a:1;
	uint32_t k, l;
	int score;
} ibwa_aln1_t;

#define IBWA_MODE_GAPE     0x01 /* bwtaln.h:95-103 */
#define IBWA_MODE_COMPREAD 0x02
#define IBWA_MODE_LOGGAP   0x04
#define IBWA_MODE_NONSTOP  0x10
#define IBWA_MODE_BAM      0x20
#define IBWA_MODE_BAM_SE   0x40
#define IBWA_MODE_BAM_READ1 0x80
#define IBWA_MODE_BAM_READ2 0x100
#define IBWA_MODE_IL13     0x200

typedef struct ibwa_ctx ibwa_ctx_t;

const char *ibwa_last_error(void);
void ibwa_free(void *p);

/* gap_init_opt (bwtaln.c:21-37) */
void ibwa_gap_init_opt(ibwa_gap_opt_t *opt);
/* bwa_cal_maxdiff (bwtaln.c:39-51) */
int ibwa_cal_maxdiff(int len, double err, double thres);

/* One engine per GPU (device ordinal).  Owns a HIP stream and device buffers. */
int ibwa_ctx_create(int device, ibwa_ctx_t **out);
/* Visible HIP devices (the CLI's -G maps GPU slice g to device g mod this count). */
int ibwa_device_count(int *n);
/* Device memory the library's buffers hold now, and their high-water mark, in bytes, summed over
 * every context of the process (a context borrowing another's index counts only its own buffers).
 * No reference counterpart: the footprint report of bench.py and the CLI's stats line. */
int ibwa_device_bytes(int64_t *now, int64_t *peak);
/* Device arena: one allocation of `bytes` on `device`, made once, from which every later buffer of
 * the process's contexts on that device is carved (a buffer that does not fit is a plain
 * allocation).  Replaces the per-batch scratch allocation of bwa_cal_sa_reg_gap (bwtaln.c:88-97,
 * 139: gap_init_stack / gap_destroy_stack per thread) with memory taken once per process.  A
 * hipMalloc right after another process released much of the HBM waits for the driver to wipe it;
 * reserving the arena while the index loads pays that once, overlapped.  IBWA_EINVAL if the device
 * already has one (the arena lives until the process exits or ibwa_release). */
int ibwa_reserve(int device, uint64_t bytes);
/* Hand the arena of `device` back to the driver now, e.g. before a long host-only phase.  The
 * driver wipes freed memory on the copy engine (~33 GB/s) and an allocation made meanwhile -- by
 * any process -- waits behind that wipe: handing a large arena back right before exit made the next
 * process wait 3.5-5.2 s where an exit holding it often did not (profiles/r05_b2b_rel*.jsonl).  The
 * contexts that carved buffers from it are destroyed first: IBWA_EINVAL while any buffer is still
 * carved.  Afterwards ibwa_reserve may reserve a new arena. */
int ibwa_release(int device);
/* Free and total device memory of `device` (hipMemGetInfo), for sizing an arena. */
int ibwa_device_memory(int device, uint64_t *free_b, uint64_t *total_b);
/* The arena of `device`: its size, the bytes its buffers use now, and their high-water mark. */
int ibwa_arena_stats(int device, uint64_t *size, uint64_t *used, uint64_t *peak);
/* Frees a context.  A context whose index others still borrow (ibwa_ctx_share_index) is freed with
 * its last borrower, so the destroy order of a source and its borrowers does not matter. */
void ibwa_ctx_destroy(ibwa_ctx_t *ctx);

/*
 * Make an FM-index device-resident (replaces the host residency of
 * bwt_restore_bwt, bwtio.c:51-70, as used by bwa_aln_core bwtaln.c:184-189).
 * strand 0 = prefix.bwt, 1 = prefix.rbwt.  `bwt` is the reference's
 * interleaved array (bwt_t.bwt, bwt_size words); L2 = bwt_t.L2[1..4].
 */
int ibwa_ctx_load_bwt(ibwa_ctx_t *ctx, int strand, uint32_t primary, const uint32_t L2[4],
                      const uint32_t *bwt, uint64_t bwt_size);
int ibwa_ctx_load_bwt_file(ibwa_ctx_t *ctx, int strand, const char *path);
/* Copy the index of another context (same process) device-to-device (xGMI peer copy when possible). */
int ibwa_ctx_clone_index(ibwa_ctx_t *dst, const ibwa_ctx_t *src);
/* Use the index of another context on the same device without a copy: its BWT and the structures
 * ibwa_ctx_prepare built (call after it).  Two contexts then align different batches concurrently on
 * one GPU (the CLI's overlapped groups).  src must outlive dst.  While shared, neither context may
 * rebuild or replace the index (load_bwt, build_index, load_sa, clone_index into it, option kmer_k,
 * K-mer tables or a sampled SA the destination would have to build): those return IBWA_EINVAL. */
int ibwa_ctx_share_index(ibwa_ctx_t *dst, const ibwa_ctx_t *src);

/*
 * Batched aln over flat arrays -- the body of bwa_cal_sa_reg_gap
 * (bwtaln.c:80-140) for one batch of n_seqs reads.
 *   seq/off/len : bwa_seq_t.seq of read i (the read reversed, codes 0..5,
 *                 bwaseqio.c:183-191) at seq[off[i] .. off[i]+len[i])
 *   batch_max_len: 0, or the max read length of the *whole* reference batch
 *                 when this call processes only a slice of it (bwtaln.c:89-93
 *                 derive max_diff / max_gapo / stack size from it)
 *   n_aln       : out, per read hit count
 *   aln         : out, malloc'd concatenation of hits in read order (ibwa_free)
 */
int ibwa_aln_batch(ibwa_ctx_t *ctx, const ibwa_gap_opt_t *opt, int64_t n_seqs, const uint8_t *seq,
                   const uint64_t *off, const uint32_t *len, int batch_max_len, int32_t *n_aln,
                   ibwa_aln1_t **aln, int64_t *n_total);

/*
 * Device-resident form used for measurement: stage a batch into HBM once,
 * run the kernels (inputs already resident), then fetch the results.
 */
int ibwa_batch_stage(ibwa_ctx_t *ctx, int64_t n_seqs, const uint8_t *seq, const uint64_t *off,
                     const uint32_t *len);

/*
 * FASTQ ingest on the device -- bwa_read_seq (bwaseqio.c:145-208) over kseq_read (kseq.h:156-195)
 * for strict 4-line records ("@header", one line of sequence bytes: isgraph, none of '>' '+' '@';
 * a line starting with '+'; one line of quality bytes 33..127 as long as the sequence), with the
 * barcode strip (-B: mode >> 24), -I and bwa_trim_read (-q, :74-87), nst_nt4_table codes and the
 * reversal (:197).  raw[0, nbytes) must begin at a record.  Out: *n_rec strict records from its
 * start (at most cap), the *consumed bytes they span, *not_strict = 1 when the next complete
 * record is not strict (the serial kseq reader takes over there; else the block ended inside a
 * record, or *n_rec == cap: what follows the cap records is not reported on), per record the kept length (-1: not longer than the barcode, skipped as bwaseqio.c:162)
 * and the sequence line's length (rec_len / rec_L may be null).  The kept reads stay in the
 * context (one block at a time) for ibwa_batch_stage_fq.  raw may be pinned (ibwa_host_alloc).
 */
int ibwa_fq_parse(ibwa_ctx_t *ctx, const void *raw, uint64_t nbytes, int mode, int trim_qual, int64_t *n_rec,
                  uint64_t *consumed, int *not_strict, int32_t *rec_len, uint32_t *rec_L, int64_t cap);
/* byte offset (in the block) of record r of the last ibwa_fq_parse (r <= its n_rec); IBWA_EINVAL once
 * another context sharing the parse scratch has parsed since */
int ibwa_fq_offset(const ibwa_ctx_t *ctx, int64_t r, uint64_t *off);
/* dst's parses use src's parse scratch (the raw block, line table, per-record arrays: ~1.7x the
 * block; same device).  Only the kept reads (~0.75x the block) stay per context.  The contexts'
 * ibwa_fq_parse calls must not overlap (each returns with its device work done). */
int ibwa_fq_share_scratch(ibwa_ctx_t *dst, const ibwa_ctx_t *src);
/* kept reads and device time (H2D copy + kernels, ms) of the last ibwa_fq_parse */
int ibwa_fq_stats(const ibwa_ctx_t *ctx, int64_t *kept, double *ms);
/* Diagnostic accessor (tests): the kept reads [first, first + n) of ctx's last parsed block, copied to
 * the host as the device holds them -- len[n], off[n] (absolute offsets into the block's code array;
 * the kept reads lie there one behind the other from 0) and into codes the bytes they span,
 * off[n-1] + len[n-1] - off[0] of them (at most codes_cap, else IBWA_EINVAL; half the block's bytes
 * always suffice).  Waits for ctx's stream and launches nothing.  The kept reads are the context's own,
 * so this also holds after another context has parsed through a shared scratch.  IBWA_EINVAL for a
 * range outside the ibwa_fq_stats kept reads and for null pointers. */
int ibwa_fq_fetch(const ibwa_ctx_t *ctx, int64_t first, int64_t n, uint32_t *len, uint64_t *off, uint8_t *codes,
                  uint64_t codes_cap);
/* ibwa_batch_stage from src's last parsed block (same device): its kept reads [first, first + n),
 * max_len = their longest.  Nothing is copied: the batch is a view of src's block, which must not be
 * parsed over (ibwa_fq_parse on src) or destroyed while this context runs or fetches the batch. */
int ibwa_batch_stage_fq(ibwa_ctx_t *ctx, const ibwa_ctx_t *src, int64_t first, int64_t n, int max_len);
/* pinned host memory for the raw blocks */
int ibwa_host_alloc(uint64_t bytes, void **p);
int ibwa_host_free(void *p);
int ibwa_batch_run(ibwa_ctx_t *ctx, const ibwa_gap_opt_t *opt, int batch_max_len);
int ibwa_batch_fetch(ibwa_ctx_t *ctx, int32_t *n_aln, ibwa_aln1_t **aln, int64_t *n_total);
/* The batch's .sai records (bwtaln.c:227-231: per read its int n_aln, then n_aln bwt_aln1_t), in
 * input order, serialised by host threads straight into the caller's buffer.  *bytes = their size;
 * with dst == NULL or cap < *bytes nothing is written (call again with a buffer that large: the
 * device results are copied back once per batch).  *n_total = the hits (may be NULL). */
int ibwa_batch_fetch_sai(ibwa_ctx_t *ctx, void *dst, uint64_t cap, uint64_t *bytes, int64_t *n_total);

/*
 * ibwa_ctx_prepare: the per-index device structures the first ibwa_batch_run with
 * these options would otherwise build on the way (bit-plane Occ layouts and
 * K-mer tables; for max_diff = 0 the exact path's full SA / ISA / 2-bit text,
 * derived from a loaded BWT).  Optional: a caller (the CLI) runs it right
 * after loading the index, while it parses its first reads.  No reference
 * counterpart (bwt_restore_bwt, bwtaln.c:184-189, is the load it follows).
 */
int ibwa_ctx_prepare(ibwa_ctx_t *ctx, const ibwa_gap_opt_t *opt);

typedef struct {
	double ms_width;       /* width kernel (exact path: its read-packing pre-pass), HIP events */
	double ms_search;      /* search kernel (first pass; exact path: k_exact alone) */
	double ms_retry;       /* large-capacity retry pass (0 if none) */
	double ms_total;       /* ibwa_batch_run wall, device-synchronised */
	int64_t n_retry;       /* reads re-run in the large-capacity pass */
	int64_t n_launch_width, n_launch_search;
	int path;              /* 0: width + general search; 1: exact-match path (max_diff == 0);
	                          2: width + persistent gapped search; 3: exact path with the
	                          unique-interval jump (index built by ibwa_ctx_build_index) */
	int kmer_k;            /* K of the K-mer interval table the exact path used (0: none) */
	int64_t n_stack_overflow;  /* first-pass reads whose stack did not fit (re-run) */
	int64_t n_aln_overflow;    /* first-pass reads whose hits did not fit (re-run) */
	int64_t n_heavy;           /* first-pass reads over the iteration budget (re-run) */
	double ms_sw;              /* last ibwa_sw_batch kernel time */
	int64_t n_coop;            /* heavy reads the wave-cooperative pass resolved */
	double ms_coop;            /* its time (width + search), part of ms_retry */
	double ms_sa2pos;          /* last ibwa_sa2pos kernel time */
	int sa2pos_full;           /* 1: it gathered from a full SA, 0: it walked the sampled SA */
	double ms_coop_width;      /* of ms_coop: the heavy reads' widths (k_width) */
	double ms_coop_roots;      /* of ms_coop: their level 0 (k_coop_roots); the rest is k_coop */
	int64_t n_resumed;         /* heavy reads handed on with their search state (the cooperative
	                              pass resumes them instead of starting over) */
	int64_t resume_records;    /* 16 B records those states took (requested, incl. any that did not fit);
	                              the cooperative pass runs them chunk by chunk (part of ms_coop) */
	int64_t resume_records_peak; /* the most records one first-pass chunk's states requested (the
	                              state buffer holds one chunk's states at a time) */
	int64_t resume_records_cap;  /* the state buffer's capacity in 16 B records */
	int64_t coop_pages_peak;     /* the most bucket pages one cooperative launch took from its pool */
	int64_t coop_pages_cap;      /* the largest launch's pool in pages (COOP_PG 16 B entries each) */
	double ms_alloc;             /* wall time the run spent allocating device buffers (hipMalloc) */
	int64_t n_tail_jumps;        /* exact tails the first pass started from a level-table entry
	                                ("gap_tail_tab"; 0 when the option or the tables are off) */
	int64_t n_width_tab_steps;   /* steps k_width's chains took from a level-table entry after a reset
	                                ("width_tab" 2; 0 when the option or the tables are off), summed over
	                                the run's k_width launches */
	double ms_bsw2_seed;         /* last ibwa_bsw2_seed_batch: k_bsw2_seed kernel time, its retry launch included */
	int64_t n_bsw2_retry;        /* ... tasks that outgrew their arena or the output buffer and ran again */
	int64_t bsw2_arena_peak;     /* ... the largest arena a task used, in bytes */
	int first_pass_lw;           /* 1: the persistent first pass ran in its LDS-width variant (width records and a
	                                ring of 16 bucket heads in LDS), 0: it did not, or path != 2 */
	int first_pass_block;        /* its workgroup size, 256 / 128 / 64 (0: the persistent kernel did not run) */
} ibwa_run_stats_t;
int ibwa_batch_stats(const ibwa_ctx_t *ctx, ibwa_run_stats_t *st);

/* Named engine options:
 *   "exact_path" (0/1, default 1)  exact-match kernel when max_diff == 0
 *   "exact_jump" (0/1, default 1)  keep full SA / ISA / text at ibwa_ctx_build_index and let
 *                                  the exact path jump over a unique interval's remaining symbols
 *   "jump_derive" (0/1, default 1) for an index loaded from .bwt files, derive those arrays on
 *                                  the device from the BWT at the first -n 0 batch (HBM permitting)
 *   "width_jump" (0/1/2, default 1) k_width steps one-row intervals from the 2-bit text
 *                                  (1: when those arrays are resident; 2: derive them for a
 *                                  gapped batch too; 0: Occ steps only) -- same widths
 *   "width_tab" (0/1/2, default 2) k_width takes a chain's first steps (up to gap_tab_k + 1) from
 *                                  the level tables, one round trip for all; 2: also the steps after
 *                                  every reset (empty interval or N), one 8 B entry per step instead of
 *                                  two Occ blocks, down to the same depth -- same widths
 *   "width_rec_stage" (0/1, default 1) k_width builds a block's compact first-pass records in LDS and
 *                                  stores them as whole lines at the block's end (0, or when the
 *                                  staging would cost residency: each lane stores its own words
 *                                  along its walk) -- same records
 *   "gap_tail_tab" (0/1, default 1) first pass: the exact tail (bwt_match_exact_alt) of a node stored
 *                                  by its string takes its steps down to depth gap_tab_k + 1 from one
 *                                  level-table entry, one round trip for all (0: one Occ step per
 *                                  symbol) -- same hits
 *   "kmer_k" (-1 auto, 0 off, 1..16) K-mer interval table length
 *   "gap_tab_k" (-1 auto, 0 off, 1..14) level tables of the first pass: the SA interval of every
 *                                  string of length <= K + 1 per strand; nodes at depth <= K are
 *                                  stored by their strings and expanded from one 32 B load (auto:
 *                                  floor(log4(n)) up to 13, 14 when both tables fit 15 % of the free
 *                                  HBM; the CLI pins 13) -- same hits
 *   "exact_blocks", "lanes_per_chunk"
 *   "gapped_v2" (0/1, default 1)   persistent gapped-search kernel (else the general kernels)
 *   "gap_cap1", "gap_pages_per_block", "gap_hit_slots", "gap_blocks_per_cu", "gap_reads_per_chunk"
 *                                  its per-lane static slots, 128 KiB pages per workgroup pool,
 *                                  first-pass hit slots, residency and batch slice size
 *   "gap_lw" (0/1, default 1), "gap_lw_min_waves" (8)  first pass with its width records in LDS
 *                                  (and resume states), in the workgroup size that keeps the most
 *                                  waves per CU (100 bp: 12, 150 bp: 9) when that is at least the minimum
 *   "gap_iter_budget" (8000)       first-pass iterations before a read goes to the cooperative pass
 *   "gap_early_iters", "gap_early_entries" (3000, 1000)
 *                                  earlier hand-off of a read whose stack holds that many entries
 *   "gap_resume" (0/1, default 1), "gap_resume_gb" (48)  an early hand-off leaves the read's search
 *                                  state (at the next score-level boundary) for the cooperative pass,
 *                                  which resumes it instead of starting over; state buffer size cap
 *                                  ("gap_resume_records": the buffer in 16 B records, for tests)
 *   "gap_resume_recs" (192)        state buffer records per read of a first-pass chunk, or 1.15 x the
 *                                  most an earlier run of the context needed, if more (states that do
 *                                  not fit start over in the cooperative pass: same hits)
 *   "gap_resume_iters", "gap_resume_entries" (2000, 300)  the early hand-off rule when states are left
 *   "gap_resume_ppb" (48), "gap_resume_cap1" (4096)  first-pass pool pages per 256 lanes and static
 *                                  slots per lane when states are left (at most the values above)
 *   "gap_tail_lanes", "gap_tail_iters" (16, 200)  also leave a state when no read is left to claim and
 *                                  at most that many lanes of the wave are busy (0: off)
 *   "coop_waves_per_cu" (12), "coop_pool_gb" (16)  cooperative pass residency and page pool (reads
 *                                  that run out of its pages run again in up to two more launches with
 *                                  the whole pool, then the wide kernel; "coop_pool_pages": the pool
 *                                  in pages, for tests)
 *   "coop_stg_room" (1)            its per-lane staging ring holds this many chains' children (1..4)
 *   "coop_roots" (0/1, default 1)  level 0 of the heavy reads one root chain per lane (k_coop_roots)
 *   "gap_coop" (0/1, default 1)    the cooperative pass (0: heavy reads go to the wide kernel)
 *   "coop_early" (0/1, default 1)  its wave-iterations issue their claims and loads before the hit
 *                                  barrier and the commit (0: after them); same hits either way
 *   "sa_walk" (0/1, default 0)     SA -> coordinate by walking the sampled SA even when the full SA is
 *                                  resident
 *   "seed_arena_cells" (0), "seed_waves_per_cu" (8)  ibwa_bsw2_seed_batch: cells (64 B) of a task's arena in
 *                                  the first launch (0: from the read length; a task that does
 *                                  not fit runs again in a larger arena) and its persistent waves per CU
 *   "bsw2_ext_waves_per_cu" (0)    k_bsw2_extend's persistent waves per CU (0: as many as the LDS admits, 8 at most)
 *   Test and diagnostics hooks: "gap_stream_per_read" (4), "gap_stream_min" (1 << 20) the first
 *   pass's hit-stream size; "gap_resume_records", "coop_pool_pages" buffer sizes in records / pages;
 *   "diag" (0) per-read iterations and k_width features; "diag_width" (0) keep the first-pass
 *   chunk's k_width outputs for ibwa_batch_diag 3 / 4; "sw_stop" (0) stop k_sw after a pass. */
int ibwa_ctx_set_option(ibwa_ctx_t *ctx, const char *key, long value);

/* The sources this library was built from: the first 16 hex digits of the SHA-256 of the
 * ibwa_amd/csrc/ sources (cpp, h, hip) followed by the include/ headers, each list in byte order of
 * the file names (no reference counterpart; the Python loader refuses a stale build). */
const char *ibwa_build_id(void);

/*
 * The `aln` command line (bwa_aln's getopt loop, bwtaln.c:249-284; same option string and
 * semantics, plus -G INT = number of GPUs) into *opt, starting from gap_init_opt's defaults.
 * argv[0] is the command name.  Returns the index of the first positional argument, -1 on an
 * unknown option.  n_gpus / fn_out (-f) may be NULL.  Thread-safe (getopt is serialised).
 */
int ibwa_aln_parse_args(int argc, char *const *argv, ibwa_gap_opt_t *opt, int *n_gpus, const char **fn_out);
/*
 * ibwa_aln_parse_args plus -F FILE, the CLI's pair mode (`aln -f out1.sai -F out2.sai <prefix>
 * <in1.fq> <in2.fq>`: both ends of a pair aligned by one process, one .sai each).  *fn_out2 = -F's
 * argument, NULL when the option is absent; fn_out2 may be NULL (the option is then parsed and
 * dropped, as -f is with fn_out NULL -- which is what ibwa_aln_parse_args does).  No reference
 * counterpart: like -G, the letter is free in bwa_aln's option string (bwtaln.c:249).
 */
int ibwa_aln_parse_args2(int argc, char *const *argv, ibwa_gap_opt_t *opt, int *n_gpus, const char **fn_out,
                         const char **fn_out2);

/*
 * Reads of the last ibwa_batch_run that the first pass handed on, and the pass that resolved
 * each: 1 the wave-cooperative pass (coop.hip), 2 the sequential wide pass (gapped.hip, one
 * read per wave), 3 the general kernels (aln.hip), 4 the wave-cooperative pass resuming the first
 * pass's search state (after the read's chunk).  Writes min(cap, n) entries; *n = their count.
 */
int ibwa_batch_retry_info(const ibwa_ctx_t *ctx, int64_t *ids, uint8_t *pass, int64_t cap, int64_t *n);

/* Diagnostics of the last ibwa_batch_run with option "diag" = 1 (gapped path): what 0 = first-pass
 * iterations per read (uint32[n]); 1 = k_width's search-cost features per read (uint16[n][4]:
 * sum of log2 width over both full-length chains, the same over the seed chains, the smaller
 * restart count of the two full chains, of the two seed chains).  what 2 (no option needed): per
 * read the pops (bwtgap.c:129) the first pass made before leaving its resume state, 0 if it left
 * none (uint32[n]): the point where the read's search moves from k_gapped to k_coop.
 * With option "diag_width" = 1 (persistent gapped path), valid for a batch that ran as one chunk:
 * what 3 = the width rows of the first-pass chunk as k_width wrote them, before the search updates
 * them (uint2[n][wstride]: {width, bid} per position of the two full-length chains, wlen1 entries
 * each, then of the two seed chains; zeros where k_width writes nothing); 4 = its compact records
 * (uint32[n][cw_words]; empty when the first pass did not run with its widths in LDS); 5 = their
 * shape (uint64[3]: reads, wstride, cw_words). */
int ibwa_batch_diag(const ibwa_ctx_t *ctx, int what, void *out, uint64_t cap_bytes);

/* Tuning knobs (0 = default): per-lane stack entries, per-read hit slots, block size */
int ibwa_ctx_set_tuning(ibwa_ctx_t *ctx, int stack_cap, int aln_cap, int block);

/*
 * On-device index construction (bwa_index, bwtindex.c:42-186, for the BWT
 * part): `codes` is the packed reference (.pac content, one 2-bit code per
 * byte, N already replaced as bns_fasta2bntseq does -- see ibwa_pack_nt4),
 * n < 2^32 - 1.  Builds .bwt (text) and .rbwt (reversed text, bwtmisc.c:160)
 * straight into HBM; the result is bit-identical to `bwa index`.
 * sa_intv > 0 also keeps the sampled suffix arrays (.sa/.rsa, bwt_cal_sa).
 */
int ibwa_ctx_build_index(ibwa_ctx_t *ctx, const uint8_t *codes, uint64_t n, int sa_intv);
/* Geometry of a resident index: primary, L2[1..4], and bwt_size (reference words). */
int ibwa_ctx_bwt_info(const ibwa_ctx_t *ctx, int strand, uint32_t *primary, uint32_t L2[4], uint64_t *bwt_size);
/* Export a resident index in the reference's interleaved .bwt word layout
 * (bwt_dump_bwt, bwtio.c:7-15, after bwt_bwtupdate_core): words[bwt_size]. */
int ibwa_ctx_export_bwt(const ibwa_ctx_t *ctx, int strand, uint32_t *words, uint64_t cap);
/* Export the sampled SA kept by ibwa_ctx_build_index: out[(n+intv)/intv] with out[0] = (u32)-1
 * (bwt.c:56-66); entries 1.. are what bwt_dump_sa writes. */
int ibwa_ctx_export_sa(const ibwa_ctx_t *ctx, int strand, uint32_t *out, uint64_t cap);
/* Sort rounds the last ibwa_ctx_build_index took for a strand (prefix doubling: round r compares
 * 21 * 2^(r-1) symbols); an error for an index that was loaded, not built. */
int ibwa_ctx_build_rounds(const ibwa_ctx_t *ctx, int strand, int *rounds);

/*
 * Batched Smith-Waterman with path: aln_local_core (stdaln.c:529-760) with
 * aln_param_bwa and _thres = 1, as bwa_sw_core (bwasw.c:51) calls it for each
 * mate rescue, plus aln_path2cigar32 (stdaln.c:1010-1040).  Pair p aligns
 * seq1 = ref[off1[p] .. +len1[p]) (the reference window) against seq2 =
 * qry[off2[p] .. +len2[p]) (the read), codes 0..4.  Per pair: score (-1 if a
 * length is 0), path_len, ends[4p..4p+3] = start i, start j, end i, end j
 * (1-based, path[path_len-1] and path[0]), n_cigar; *cigar = malloc'd
 * concatenation of all CIGARs (len << 4 | op, op 0 M, 1 I, 2 D; ibwa_free).
 * Requires min(len1, len2) * 11 <= 32000 (the reference's score rebasing is
 * then unreachable); IBWA_EINVAL otherwise.
 */
int ibwa_sw_batch(ibwa_ctx_t *ctx, int64_t n, const uint8_t *ref, const uint64_t *off1, const uint32_t *len1,
                  const uint8_t *qry, const uint64_t *off2, const uint32_t *len2, int32_t *score,
                  int32_t *path_len, int32_t *ends, int32_t *n_cigar, uint32_t **cigar, int64_t *n_cigar_total);

/*
 * SA -> coordinate.
 *
 * ibwa_ctx_load_sa: make a sampled suffix array device-resident, as
 * bwt_restore_sa (bwtio.c:29-49) loads it into bwt_t: sa[0..n_sa) with
 * sa[0] = (u32)-1, n_sa = (seq_len + sa_intv) / sa_intv; strand 0 = prefix.sa,
 * 1 = prefix.rsa.  ibwa_ctx_load_sa_file reads the .sa/.rsa file itself and
 * applies bwt_restore_sa's primary / seq_len consistency checks (IBWA_EINVAL).
 * An index built by ibwa_ctx_build_index(sa_intv > 0) already has both.
 *
 * ibwa_ctx_expand_sa: derive the full SA of both strands on the device from
 * the sampled ones (one LF walk per sampled row, seq_len steps in all;
 * 2 x 4 B per base of HBM) so that ibwa_sa2pos is one gather per hit.
 *
 * ibwa_sa2pos: bwtdb_sa2seq (dbset.c:240-246) over n hits, i.e. bwt_sa
 * (bwt.c:69-79) on bwt[0] for strand 1 and seq_len - (bwt_sa(bwt[1], k) + len)
 * (u32 arithmetic) for strand 0, plus `offset` (bwtdb_t.offset; 0 for a single
 * database).  Replaces the per-hit calls of bwa_cal_pac_pos (bwase.c:133,
 * :146, :157), bwa_cal_pac_pos_pe (bwape.c:347, :400) and saiset.c:136, :147.
 * Uses the full SA when resident (option "sa_walk" = 1 forces the walk).
 */
int ibwa_ctx_load_sa(ibwa_ctx_t *ctx, int strand, uint32_t sa_intv, const uint32_t *sa, uint64_t n_sa);
int ibwa_ctx_load_sa_file(ibwa_ctx_t *ctx, int strand, const char *path);
int ibwa_ctx_expand_sa(ibwa_ctx_t *ctx);
/* The sampled SA of both strands (bwt_cal_sa's values at interval sa_intv, what `bwa index`
 * writes to .sa / .rsa, bwt.c:48-67) derived on the device from the resident BWT alone. */
int ibwa_ctx_derive_sa(ibwa_ctx_t *ctx, uint32_t sa_intv);
int ibwa_sa2pos(ibwa_ctx_t *ctx, int64_t n, const uint8_t *strand, const uint32_t *k, const uint32_t *len,
                uint64_t offset, uint64_t *pos);

/*
 * Batched banded global alignment: aln_global_core (stdaln.c:345-525) with aln_param_bwa's
 * scores (gap open 26, extend 9, aln_sm_maq) and the given band_width / gap_end, as
 * refine_gapped_core (bwase.c:167-199) calls it with band 50, gap_end 5 for each gapped read.
 * Pair p aligns seq1 = ref[off1[p] .. +len1[p]) against seq2 = qry[off2[p] .. +len2[p]).
 * Per pair: score (0 and path_len 0 if a length is 0), path_len, n_cigar; *cigar = malloc'd
 * concatenation of the CIGARs in aln_path2cigar32 encoding (len << 4 | op: 0 M, 1 I, 2 D).
 */
int ibwa_global_batch(ibwa_ctx_t *ctx, int64_t n, const uint8_t *ref, const uint64_t *off1, const uint32_t *len1,
                      const uint8_t *qry, const uint64_t *off2, const uint32_t *len2, int band, int gap_end,
                      int32_t *score, int32_t *path_len, int32_t *n_cigar, uint32_t **cigar, int64_t *n_cigar_total);

/*
 * The reference sequence in HBM, and bwa_refine_gapped (bwase.c:333-416) as two batched stages.
 *
 * ibwa_ctx_load_pac: dbset_load_pac (dbset.c): the n_db references of a set, each 2-bit packed
 * from its own base 0 (base x at bits 7-6 .. 1-0 of byte x / 4, bntseq.c; (l_pac[i] + 3) / 4 bytes
 * are read of pac[i]), laid back to back as dbset_restore lays them (db[i]->offset = sum of the
 * earlier l_pac, dbset.c:146-151) into one device array of sum(l_pac) / 4 bytes.  Loading again
 * replaces the sequence.  ibwa_ctx_share_index lends it with the index; a context that borrows or
 * lends its index refuses the call (IBWA_EINVAL).  The three calls below fail with IBWA_ENOINDEX
 * while no sequence is loaded.
 *
 * ibwa_pac_extract: dbset_extract_sequence (dbset.c:306-325) for n windows: the codes of
 * [beg[i], beg[i] + len[i]) clipped at the total l_pac, 1 B per base at out + out_off[i];
 * got[i] = bases written (0 for beg[i] >= l_pac).  out is written over [0, max(out_off[i] +
 * len[i])): the bytes no window covers, and those past got[i], are 0 (the reference callocs them).
 *
 * ibwa_refine_batch: refine_gapped_core (bwase.c:167-221) with is_end_correct = 1 for n hits on
 * references without a remap table.  Job i: the hit position pos[i], ext[i] = (strand ? 1 : -1) *
 * gaps as at bwase.c:354 / :363, and the read's codes seq[off[i] .. +len[i]) in the orientation
 * bwa_refine_gapped passes (seq after its seq_reverse, or rseq for a reverse-strand hit).  On the
 * device: the window rule of bwase.c:185-192, the window's bases from the resident sequence,
 * aln_global_core with aln_param_bwa (band 50, gap_end 5), bwa_aln_path2cigar, and the position
 * and end fix-ups of bwase.c:201-218.  pos_out[i] = the refined position, n_cigar[i], and *cigar =
 * malloc'd concatenation of the CIGARs as bwa_cigar_t (op << 29 | len; op 0 M, 1 I, 2 D, 3 S;
 * ibwa_free).  A job with pos > l_pac fails the whole call with IBWA_EINVAL (the message names
 * the job, the position and l_pac, bwase.c:179-181) before anything is written.  translate_cigar
 * of a remapped alternate (bwase.c:223-238) is the caller's, applied to this output.
 *
 * ibwa_md_batch: bwa_cal_md1 (bwase.c:243-295) for n reads.  Read i: pos[i], its codes in the
 * hit's orientation, len[i], and n_cigar[i] bwa_cigar_t's (S allowed) taken in read order from
 * `cigar`, or n_cigar[i] < 0 for none (n_cigar == NULL: no read has one).  nm[i] is unmasked (the
 * caller keeps bwa_seq_t.nm's & 0xfff).  The MD texts come NUL-terminated and compact in read
 * order: read i's starts at (*md)[(*md_off)[i]], (*md_off)[n] is the total size.  Offsets and
 * texts are one allocation: release *md_off with ibwa_free (*md points into it).
 */
int ibwa_ctx_load_pac(ibwa_ctx_t *ctx, int n_db, const uint8_t *const *pac, const uint64_t *l_pac);
int ibwa_pac_extract(ibwa_ctx_t *ctx, int64_t n, const uint64_t *beg, const uint32_t *len, const uint64_t *out_off,
                     uint8_t *out, uint32_t *got);
int ibwa_refine_batch(ibwa_ctx_t *ctx, int64_t n, const uint64_t *pos, const int32_t *ext, const uint8_t *seq,
                      const uint64_t *off, const uint32_t *len, uint64_t *pos_out, int32_t *n_cigar, uint32_t **cigar,
                      int64_t *n_cigar_total);
int ibwa_md_batch(ibwa_ctx_t *ctx, int64_t n, const uint64_t *pos, const uint8_t *seq, const uint64_t *off,
                  const uint32_t *len, const int32_t *n_cigar, const uint32_t *cigar, int32_t *nm, uint64_t **md_off,
                  const char **md);

/*
 * Colour space: the colour sequence of a nucleotide .pac, and bwa_cs2nt_core (cs2nt.c:113-196), which
 * turns the colours of a mapped read into bases and base qualities.
 *
 * ibwa_pac2cspac: bwa_pac2cspac_core (bwtmisc.c:202-219).  nt_pac: (l_pac + 3) / 4 bytes of a
 * nucleotide .pac; cs_pac_out: l_pac / 4 + 1 bytes, what bwa_pac2cspac writes before the count byte
 * (bwtmisc.c:239).  Symbol 0 is base 0, colour i is nst_color_space_table of bases i - 1 and i; every
 * bit past l_pac is 0.  Needs no index.
 *
 * ibwa_ctx_load_ntpac: the second sequence set of a colour-space dbset (dbs->ntbns, <prefix>.nt.pac of
 * every reference; dbset.c:144), resident beside ibwa_ctx_load_pac's in the same layout.  Lent by
 * ibwa_ctx_share_index; refused (IBWA_EINVAL) by a context that borrows or lends its index.
 *
 * ibwa_cs2nt_rows: cs2nt_DP (cs2nt.c:37-78) then cs2nt_nt_qual (:84-110) on n caller-built row pairs.
 * Job i: nt_ref[off[i] .. off[i] + size[i]] (size + 1 codes 0-4) and cs_read[off[i] .. off[i] +
 * size[i]) (colour << 6 | qual, qual == 63 for an N colour); out[out_off[i] .. + size[i] - 1) gets
 * cs2nt_nt_qual's result, base << 6 | qual.  size[i] == 0 is IBWA_EINVAL (the reference's loop does
 * not end there).  Needs no index.
 *
 * ibwa_cs2nt_batch: the row construction of bwa_cs2nt_core (cs2nt.c:136-171) from the resident
 * nucleotide sequence, then the same two functions, for n mapped reads.  Read i: the hit position
 * pos[i], strand[i], its colour codes seq[off[i] .. + len[i]) in the hit's orientation (p->strand ?
 * p->rseq : p->seq), its quality string qual[off[i] .. + len[i]) as read (ASCII, + 33; indexed
 * len - 1 - j on strand 1 as __gen_csbase does), and n_cigar[i] bwa_cigar_t's taken in read order from
 * `cigar` (<= 0: none; n_cigar == NULL: no read has one).  out[off[i] .. + new_len[i]) gets the
 * decoded base << 6 | qual bytes and new_len[i] = rows - 1, the read's new length (cs2nt.c:177); the
 * host updates of cs2nt.c:178-194 are the caller's.  A reference base at or past l_pac is not
 * defined by the reference (its buffer is uninitialised there): it counts as 4, no base known.
 * IBWA_ENOINDEX while no nucleotide sequence is loaded; IBWA_EINVAL for a CIGAR that consumes more
 * colours than the read has or no colour at all.
 */
int ibwa_pac2cspac(ibwa_ctx_t *ctx, const uint8_t *nt_pac, uint64_t l_pac, uint8_t *cs_pac_out);
int ibwa_ctx_load_ntpac(ibwa_ctx_t *ctx, int n_db, const uint8_t *const *pac, const uint64_t *l_pac);
int ibwa_cs2nt_rows(ibwa_ctx_t *ctx, int64_t n, const uint8_t *nt_ref, const uint8_t *cs_read, const uint64_t *off,
                    const uint32_t *size, uint8_t *out, const uint64_t *out_off);
int ibwa_cs2nt_batch(ibwa_ctx_t *ctx, int64_t n, const uint64_t *pos, const uint8_t *strand, const uint8_t *seq,
                     const uint8_t *qual, const uint64_t *off, const uint32_t *len, const int32_t *n_cigar,
                     const uint32_t *cigar, uint8_t *out, uint32_t *new_len);

/*
 * Batched pairwise alignment with any scoring scheme: aln_local_core (stdaln.c:529-760, with its
 * suboptimal score) or aln_global_core (stdaln.c:345-525) for a run-time AlnParam, plus
 * aln_path2cigar32.  What `stdsw` (simple_dp.c) runs per short sequence and strand.
 *
 * ibwa_aln_param_t is the reference's AlnParam: gap_open, gap_ext, gap_end, a row x row score matrix
 * (2 <= row <= 32; the score of codes x of seq2 and y of seq1 is matrix[x * row + y]) and band_width
 * (<= 0: len1 + len2 of each pair, a full matrix, as stdsw sets it).  ibwa_aln_param_preset fills
 * one of the presets: "blast" (5 / 2 / 2, +1 / -3, -2 with N, 5 x 5, band 50), "aa2aa" (10 / 2 / 2,
 * BLOSUM62 over ARNDCQEGHILKMFPSTWYV*X, 22 x 22, band 50) or "bwa" (26 / 9 / 5, 11 / -19 / -13,
 * 5 x 5, band 50); the matrix points at static storage.
 *
 * Pair p aligns seq1[off1[p] .. +len1[p]) (the inner dimension i) with seq2[off2[p] .. +len2[p]) (the
 * outer loop j, which the suboptimal score is taken over); the codes arrive encoded, each < row.
 * type 0 (local, _thres = thres >= 1): score (-1 for an empty sequence), subo, path_len (0 when
 * score < thres: no path, ends and CIGAR then), ends[4p..4p+3] = start i, start j, end i, end j
 * (1-based: path[path_len-1] and path[0]), n_cigar.  type 1 (global): score, path_len, ends, n_cigar;
 * subo is 0; an empty sequence gives score 0 and path_len 0.  type 2 (extend): see ibwa_extend_batch
 * below.  *cigar = malloc'd concatenation of the
 * CIGARs (len << 4 | op, op 0 M, 1 I, 2 D; ibwa_free).
 *
 * IBWA_EINVAL, with a message that names the offender, for: gap_open or gap_ext < 1, gap_end > 700 or
 * gap_open + gap_ext > 700; row outside 2..32; a matrix whose maximum is <= 0; a code >= row;
 * thres < 1 in local mode; local mode with max_score * min(len1, len2) > 32000 (the reference's
 * rebasing is then unreachable); a length above IBWA_STDALN_MAX_LEN; global mode with more than
 * IBWA_STDALN_MAX_CELLS cells, (len1 + 1) * (len2 + 1), or in which (len1 + len2) times the largest
 * score or gap cost reaches 2^30 (the global core's scores are ints beside -2^30); a pair whose
 * scratch alone is past the per-launch scratch (option "stdaln_scratch_mb", MiB).  The local path
 * fill's scratch is sized for the longest region a hit can cover, S + (S * max_score + gap_open +
 * gap_ext) / gap_ext + 1 symbols of a sequence with S = min(len1, len2), so cheap gaps beside large
 * scores make a pair's scratch large.  A batch larger than the scratch runs in several launches; ibwa_stdaln_chunks tells how many the last call took (and their kernel time).
 */
typedef struct {
	int gap_open, gap_ext, gap_end;
	const int32_t *matrix;
	int row, band_width;
} ibwa_aln_param_t;
#define IBWA_STDALN_MAX_LEN (4 << 20)
#define IBWA_STDALN_MAX_CELLS (32ll << 20)
int ibwa_aln_param_preset(const char *name, ibwa_aln_param_t *ap);
int ibwa_stdaln_batch(ibwa_ctx_t *ctx, const ibwa_aln_param_t *ap, int type, int thres, int64_t n, const uint8_t *seq1,
                      const uint64_t *off1, const uint32_t *len1, const uint8_t *seq2, const uint64_t *off2,
                      const uint32_t *len2, int32_t *score, int32_t *subo, int32_t *path_len, int32_t *ends,
                      int32_t *n_cigar, uint32_t **cigar, int64_t *n_cigar_total);
int ibwa_stdaln_chunks(const ibwa_ctx_t *ctx, int64_t *launches, double *kernel_ms);
/* The parameter and size checks of ibwa_stdaln_batch alone (no device is touched). */
int ibwa_stdaln_check(const ibwa_aln_param_t *ap, int type, int thres, int64_t n, const uint8_t *seq1,
                      const uint64_t *off1, const uint32_t *len1, const uint8_t *seq2, const uint64_t *off2,
                      const uint32_t *len2);

/*
 * Seed extension: aln_extend_core (stdaln.c:862-1008) for a run-time AlnParam, batched.  Pair p extends
 * from the corner cell with the score g0[p] (NULL: 1 for every pair) into seq1[off1[p] .. +len1[p]) (the
 * inner dimension i) and seq2[off2[p] .. +len2[p]) (the rows j) inside the reference's adaptive band;
 * a zero cell never restarts.  The score is what aln_extend_core returns: best cell + rebasing - 1, -1
 * for an empty sequence; past 32000 the rows are rebased by 16000 as at stdaln.c:917-930.
 * band_width <= 0 is len1 + len2 of each pair, this library's convention (the reference takes the
 * number as it is: its first row is then empty, or its row bounds leave the array).
 *   mode 0  the score alone.
 *   mode 1  the end cell: ends[2p], ends[2p + 1] = end_i, end_j of the first best cell in row-major order
 *           (0, 0 when score <= 0).  What bsw2_extend_left / _rght use (bwtsw2_aux.c:80-164).
 *   mode 2  the path: aln_global_core over seq1[0, end_i) x seq2[0, end_j) with gap_end -1, the band
 *           doubling from band_width until the global score equals the extension score or the band
 *           passes max(end_i, end_j); score = that global score, which leaves g0 out (so for g0 > 1
 *           the band always runs to the end); path_len, n_cigar, *cigar as ibwa_stdaln_batch gives them.
 *           Where the reference prints "no suitable bandwidth" the pair is counted: ibwa_extend_stats.
 * path_len / n_cigar / cigar may be NULL in modes 0 and 1.  ibwa_stdaln_batch with type 2 is
 * aln_stdaln_aux's ALN_TYPE_EXTEND: g0 = 1, mode 2, subo = 0, ends[4p..] = the path's first and last cell.
 *
 * IBWA_EINVAL, with a message that names the pair, for ibwa_stdaln_batch's parameter checks, g0 outside
 * 1..32000, a code >= row, a length above IBWA_STDALN_MAX_LEN, and in mode 2 a pair whose path fill can
 * pass IBWA_STDALN_MAX_CELLS or the per-launch scratch; end_i <= len2 + band - 1 and end_j <= len1 + band
 * bound the fill.  A batch larger than the scratch runs in several launches (ibwa_stdaln_chunks).
 *
 * ibwa_extend_seeds: mode 1 with the targets read on the device from ibwa_ctx_load_pac's sequence (no
 * target byte crosses the bus).  Seed p, dir[p] == 0 (right): the bases pos[p], pos[p] + 1, ..., at most
 * lt[p] of them, clipped at the set's total length l.  dir[p] == 1 (left): pos[p] - 1, pos[p] - 2, ...,
 * at most lt[p], ending with base 0 at the latest; bsw2_extend_left's loop never takes base 0, so to
 * match it pass lt = min(lt, pos - 1).  rev != 0 reads base x as __rpac does (bwtsw2_aux.c:78): base
 * l - x - 1 of the stored sequence, reversed and not complemented.  qry[off[p] .. +len[p]) is the
 * query slice in the orientation the DP consumes it (for a left extension the reversed prefix, as
 * bsw2_extend_left builds it).  The windows may run from one reference of the set into the next.
 * IBWA_ENOINDEX while no sequence is loaded; an empty window gives score -1; a left seed with
 * pos > l, a dir above 1 or row < 4 is IBWA_EINVAL.  Sorting hits and the containment test of
 * bsw2_extend_left are the caller's.
 */
int ibwa_extend_batch(ibwa_ctx_t *ctx, const ibwa_aln_param_t *ap, int mode, int64_t n, const uint8_t *seq1,
                      const uint64_t *off1, const uint32_t *len1, const uint8_t *seq2, const uint64_t *off2,
                      const uint32_t *len2, const int32_t *g0, int32_t *score, int32_t *ends, int32_t *path_len,
                      int32_t *n_cigar, uint32_t **cigar, int64_t *n_cigar_total);
/* The parameter and size checks of ibwa_extend_batch alone (no device is touched). */
int ibwa_extend_check(const ibwa_aln_param_t *ap, int mode, int64_t n, const uint8_t *seq1, const uint64_t *off1,
                      const uint32_t *len1, const uint8_t *seq2, const uint64_t *off2, const uint32_t *len2,
                      const int32_t *g0);
int ibwa_extend_seeds(ibwa_ctx_t *ctx, const ibwa_aln_param_t *ap, int64_t n, const uint64_t *pos, const uint8_t *dir,
                      const uint32_t *lt, int rev, const uint8_t *qry, const uint64_t *off, const uint32_t *len,
                      const int32_t *g0, int32_t *score, int32_t *ends);
/* path-mode pairs of the last extension call whose global fill stayed below the extension score */
int ibwa_extend_stats(const ibwa_ctx_t *ctx, int64_t *no_band);

/*
 * bwasw's seeding: bsw2_core (bwtsw2_core.c:429-594) on the read's bwtl (bwt_lite.c:9-54), batched.
 *
 * Task i is seq[off[i] .. off[i] + len[i]), codes 0-3, searched against .bwt / .sa when strand[i] == 0 and
 * against .rbwt / .rsa when it is 1 (bsw2_aln_core's second pass takes the reversed read there).  opt is what
 * bsw2_aln receives, t and coef already scaled by a (bwtsw2_main.c:82-83).  With adjust != 0 each task's t
 * and bw are derived from its length as bsw2_aln_core does (bwtsw2_aux.c:483-497; ibwa_bsw2_opt_for_len);
 * with adjust == 0 they are used as given.
 *
 * *hits = malloc'd (ibwa_free): per task the n_all[i] hits of b_ret[0], then the n_narrow[i] hits of
 * b_ret[1], each list in the reference's final order after bsw2_resolve_duphits, so l == 0, k is a
 * coordinate (bwt_sa) and flag & 1 marks a repetitive hit.  bsw2hit_t's n_seeds is not part of the
 * contract (the reference leaves it unset for narrow hits).  With is == 0 and no hit the reference reads
 * a hit it never allocated; here such a list is empty.
 *
 * The traversal, the read's BWT and the bwt_sa lookups run on the device (k_bsw2_seed, one task per
 * wavefront, each in an arena of HBM); the unstable sort and the containment pass of
 * bsw2_resolve_duphits run on the host.  A task that outgrows its arena runs once more in a larger one;
 * IBWA_EOVERFLOW, naming the first such task, if it still does not fit.  A task whose hits do not fit
 * the launch's output buffer has counted them, and runs once more with room for exactly that count:
 * a batch in which no task outgrows its arena never ends in IBWA_EOVERFLOW.  (A task that did outgrow
 * it has no count; it gets 16 times its planned room, and if it needs more, it or a task that claims
 * room after it is the one named.)
 *
 * IBWA_ENOINDEX without the index or the suffix array of a strand a task names.  IBWA_EINVAL, with a
 * message that names the task, for a code >= 4, a strand above 1, a length of 0 or above
 * IBWA_BSW2_MAX_LEN; and for a, b, q, r or z < 1, is < 0, and t < 1 or bw < 1 with adjust == 0.
 * n == 0 returns 0 with no hits.  Options: "seed_arena_cells" (0: by read length) the first launch's
 * cells per task arena, "seed_waves_per_cu" (8).
 */
#define IBWA_BSW2_MAX_LEN 8192
typedef struct { int32_t a, b, q, r, t, bw, z, is; float coef; int32_t adjust; } ibwa_bsw2_opt_t;
typedef struct { uint32_t k, l, flag; int32_t len, G, G2, beg, end; } ibwa_bsw2_hit_t;   /* bsw2hit_t without n_seeds */
/* bsw2_init_opt's values for "bwasw" (adjust = 1); IBWA_EINVAL for another name */
int ibwa_bsw2_opt_preset(const char *name, ibwa_bsw2_opt_t *opt);
int ibwa_bsw2_seed_batch(ibwa_ctx_t *ctx, const ibwa_bsw2_opt_t *opt, int64_t n, const uint8_t *seq,
                         const uint64_t *off, const uint32_t *len, const uint8_t *strand,
                         int32_t *n_all, int32_t *n_narrow, ibwa_bsw2_hit_t **hits, int64_t *n_hits_total);
/* The checks of ibwa_bsw2_seed_batch alone (no device is touched). */
int ibwa_bsw2_seed_check(const ibwa_bsw2_opt_t *opt, int64_t n, const uint8_t *seq, const uint64_t *off,
                         const uint32_t *len, const uint8_t *strand);
/* t and bw of a read of length len (bwtsw2_aux.c:483-497) */
void ibwa_bsw2_opt_for_len(const ibwa_bsw2_opt_t *opt, uint32_t len, int32_t *t, int32_t *bw);
/* The last ibwa_bsw2_seed_batch: out[0..2] wall-clock ticks its waves spent building bwtls, traversing and
 * resolving, out[3] cells visited, out[4] tasks run again, out[5] the largest arena a task used (bytes),
 * out[6] the first launch's arena per task (bytes), out[7] its workgroups. */
int ibwa_bsw2_seed_stats(const ibwa_ctx_t *ctx, int64_t out[8]);

/*
 * bwasw from a read to its hits on one index strand: bsw2_aln1_core (bwtsw2_aux.c:252-276), batched.
 *
 * Read i is seq[off[i] .. off[i] + len[i]), codes 0-3; the library builds its reverse complement.  With
 * is_rev[i] == 0 it is searched against .bwt / .sa and the target bases are read forwards; with 1 against
 * .rbwt / .rsa and through __rpac, and the caller passes what bsw2_aln_core calls rseq[0], the reversed read.
 * opt->seed is what ibwa_bsw2_seed_batch takes (t and bw per read when adjust != 0); t_seeds and mask_level
 * are bsw2opt_t's.  u[i] in [0, 1) stands for the drand48() of bsw2_resolve_query_overlaps (NULL: 0.0).
 *
 * Stages, each one launch over the whole batch: the seeds of 2n tasks (ibwa_bsw2_seed_batch); on the host,
 * bsw2_chain_filter and the sort by end; bsw2_extend_left in dependency order on the device
 * (k_bsw2_extend, one list per wave); on the host, merge_hits and bsw2_resolve_duphits; bsw2_extend_rght
 * on the device (the same kernel, unordered); on the host, the strand merge and
 * bsw2_resolve_query_overlaps.  The host stages are bsw2_aln1.h's functions, run per read on up to 16
 * threads.  Every field of every hit equals the reference's; *hits = malloc'd (ibwa_free), read i's
 * n_hits[i] hits in the reference's order, l == 0, flag & 0x10 for a hit of the reverse complement.
 *
 * Not part of this call: bsw2_aln_core's second pass and flag_fr, its drand48 fill of ambiguous bases,
 * CIGARs and SAM.
 *
 * IBWA_ENOINDEX without the strand's index and suffix array or without the resident sequence
 * (ibwa_ctx_load_pac).  IBWA_EINVAL, naming the read, for what ibwa_bsw2_seed_check refuses, for
 * t_seeds < 0, mask_level outside [0, 1], u outside [0, 1), is_rev > 1, and for a narrow hit whose score
 * is past 32000, the extension's 16-bit cells.  IBWA_EOVERFLOW, naming the task, when a window or a ring
 * did not fit what the launch was sized for.  n == 0 returns 0.
 *
 * ibwa_bsw2_extend_left_batch is the left stage alone: per task a query qry[off[t] .. +len[t]) (the strand's
 * sequence as bsw2_extend_left receives it), a band bw[t], is_rev[t] and n_hits[t] hits in the caller's
 * order, concatenated in hits; the sort by end is inside, and the same list comes back in sorted order
 * with G, len, beg, k and n_seeds updated.  Of opt only a, b, q, r are read.  IBWA_EINVAL for a hit with
 * beg outside [0, len], and, where l == 0 and k != 0, k > l_pac or G outside 1..32000.
 */
typedef struct { ibwa_bsw2_opt_t seed; int32_t t_seeds; float mask_level; } ibwa_bsw2_aln_opt_t;
typedef struct { uint32_t k, l, flag, n_seeds; int32_t len, G, G2, beg, end; } ibwa_bsw2_aln_hit_t;
/* "bwasw": ibwa_bsw2_opt_preset's values, t_seeds 5, mask_level 0.50 */
int ibwa_bsw2_aln_opt_preset(const char *name, ibwa_bsw2_aln_opt_t *opt);
int ibwa_bsw2_aln1_batch(ibwa_ctx_t *ctx, const ibwa_bsw2_aln_opt_t *opt, int64_t n, const uint8_t *seq,
                         const uint64_t *off, const uint32_t *len, const uint8_t *is_rev, const double *u,
                         int32_t *n_hits, ibwa_bsw2_aln_hit_t **hits, int64_t *n_hits_total);
int ibwa_bsw2_extend_left_batch(ibwa_ctx_t *ctx, const ibwa_bsw2_opt_t *opt, int64_t n, const uint8_t *qry,
                                const uint64_t *off, const uint32_t *len, const int32_t *bw, const uint8_t *is_rev,
                                const int32_t *n_hits, ibwa_bsw2_aln_hit_t *hits);
/* The argument checks of ibwa_bsw2_aln1_batch alone (no device is touched). */
int ibwa_bsw2_aln1_check(const ibwa_bsw2_aln_opt_t *opt, int64_t n, const uint8_t *seq, const uint64_t *off,
                         const uint32_t *len, const uint8_t *is_rev, const double *u);
/* The last ibwa_bsw2_aln1_batch or ibwa_bsw2_extend_left_batch: out[0], out[1] microseconds of the left and
 * the right launch; of the left launch out[2] hits extended (DP runs whose result counted), out[3] hits
 * skipped as contained before any DP, out[4] speculative DP runs discarded, out[5] hits skipped for
 * l != 0 or k == 0 (out[2..5] add up to its hits), out[6] its tasks, out[7] its windows of 64. */
int ibwa_bsw2_aln1_stats(const ibwa_ctx_t *ctx, int64_t out[8]);

/* Device Occ KAT: bwt_occ4 (bwt.c:157) for n positions k[] on strand s -> cnt[4*n] */
int ibwa_occ4(ibwa_ctx_t *ctx, int strand, int64_t n, const uint32_t *k, uint32_t *cnt);

#ifdef __cplusplus
}
#endif
#endif
