// engine_context.hip -- host side of the C ABI in include/ibwa_aln.h: errors, the device arena and
// the buffers carved from it, a context's life, its options, device queries.
//
// The engine replaces, per batch, the pthread fan-out of bwa_aln_core (bwtaln.c:199-218)
// and the per-thread scratch of bwa_cal_sa_reg_gap (bwtaln.c:88-97, 139) with
// one HIP launch grid over the batch and HBM-resident per-lane scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>

#include "arena.h"
#include "engine_ctx.h"

using namespace ibwa;

namespace ibwa {

thread_local std::string g_err;
thread_local double g_alloc_ms = 0;
thread_local hipStream_t g_stream = nullptr;

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

namespace {
// Device bytes the library's buffers hold (all contexts of the process) and their high-water mark.
std::atomic<int64_t> g_dev_bytes{0}, g_dev_peak{0};
void dev_bytes_add(int64_t d) {
  const int64_t now = g_dev_bytes.fetch_add(d) + d;
  int64_t pk = g_dev_peak.load();
  while (now > pk && !g_dev_peak.compare_exchange_weak(pk, now)) {
  }
}

constexpr int MAX_DEV = 64;
Arena g_arena[MAX_DEV];
Arena *arena_here() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= MAX_DEV) return nullptr;
  return g_arena[d].base ? &g_arena[d] : nullptr;
}
}  // namespace

hipError_t zero_async(void *p, size_t bytes, hipStream_t st) {
  constexpr size_t kZ = 64u << 20;
  static std::once_flag once;
  static void *zeros = nullptr;
  std::call_once(once, []() {
    if (hipHostMalloc(&zeros, kZ, hipHostMallocDefault) != hipSuccess) zeros = nullptr;
    else memset(zeros, 0, kZ);
  });
  if (!zeros) return hipMemsetAsync(p, 0, bytes, st);
  for (size_t o = 0; o < bytes; o += kZ) {
    hipError_t e = hipMemcpyAsync(static_cast<char *>(p) + o, zeros, std::min(kZ, bytes - o), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int DBuf::ensure(size_t bytes) {
  if (bytes <= cap) return 0;
  if (borrowed) return fail(IBWA_EINVAL, "a shared index buffer cannot grow (%zu > %zu bytes)", bytes, cap);
  release();
  size_t want = std::max<size_t>(bytes, 256);
  static const bool verbose = getenv("IBWA_VERBOSE") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  if (Arena *a = arena_here()) p = a->alloc(want);
  if (!p) {
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) return fail(IBWA_EHIP, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  g_alloc_ms += ms;
  if (verbose && ms > 20.0) fprintf(stderr, "[ibwa_amd] hipMalloc(%.2f GB) took %.0f ms\n", want / 1e9, ms);
  cap = want;
  dev_bytes_add((int64_t)want);
  return 0;
}

void DBuf::free_dev(void *q, size_t n) {
  for (Arena &a : g_arena)
    if (a.owns(q)) {
      // the range may still be used by work queued on the owning context's stream (the API call
      // in progress on this thread: g_stream); other contexts never touch it (an index a context
      // lends is never freed while borrowed, and an ingest slot is not parsed over while a lane
      // still reads it)
      if (g_stream) (void)hipStreamSynchronize(g_stream);
      else (void)hipDeviceSynchronize();
      a.release(q, n);
      dev_bytes_add(-(int64_t)n);
      return;
    }
  (void)hipFree(q);
  dev_bytes_add(-(int64_t)n);
}

// An operation that would rebuild or replace index structures shared by ibwa_ctx_share_index
// (borrowed buffers are written in place or cannot grow, and the other context may be aligning).
int refuse_shared(const ibwa_ctx *c, const char *what) {
  if (c->share_src) return fail(IBWA_EINVAL, "%s: this context shares another context's index", what);
  if (c->n_borrowers) return fail(IBWA_EINVAL, "%s: %d other context(s) share this context's index", what, c->n_borrowers);
  return 0;
}

}  // namespace ibwa

extern "C" {

const char *ibwa_last_error(void) { return g_err.c_str(); }
void ibwa_free(void *p) { free(p); }

void ibwa_gap_init_opt(ibwa_gap_opt_t *o) {  // bwtaln.c:21-37
  memset(o, 0, sizeof(*o));
  o->s_mm = 3; o->s_gapo = 11; o->s_gape = 4;
  o->max_diff = -1; o->max_gapo = 1; o->max_gape = 6;
  o->indel_end_skip = 5; o->max_del_occ = 10; o->max_entries = 2000000;
  o->mode = IBWA_MODE_GAPE | IBWA_MODE_COMPREAD;
  o->seed_len = 32; o->max_seed_diff = 2;
  o->fnr = 0.04f;
  o->n_threads = 1;
  o->max_top2 = 30;
  o->trim_qual = 0;
}

int ibwa_cal_maxdiff(int l, double err, double thres) {  // bwtaln.c:39-51
  double elambda = exp(-l * err);
  double sum, y = 1.0;
  int k, x = 1;
  for (k = 1, sum = elambda; k < 1000; ++k) {
    y *= l * err;
    x *= k;
    sum += elambda * y / x;
    if (1.0 - sum < thres) return k;
  }
  return 2;
}

int ibwa_device_count(int *n) {
  int d = 0;
  hipError_t e = hipGetDeviceCount(&d);
  if (e != hipSuccess) return fail(IBWA_EHIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
  if (n) *n = d;
  return 0;
}

int ibwa_device_memory(int device, uint64_t *free_b, uint64_t *total_b) {
  HIPCHK(hipSetDevice(device));
  size_t f = 0, t = 0;
  HIPCHK(hipMemGetInfo(&f, &t));
  if (free_b) *free_b = f;
  if (total_b) *total_b = t;
  return 0;
}

int ibwa_reserve(int device, uint64_t bytes) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail(IBWA_EHIP, "no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= n || device >= MAX_DEV) return fail(IBWA_EINVAL, "device %d out of range (%d devices)", device, n);
  Arena &a = g_arena[device];
  std::lock_guard<std::mutex> lk(a.mu);
  if (a.base) return fail(IBWA_EINVAL, "device %d already has an arena of %zu bytes", device, a.size);
  if (bytes == 0) return 0;
  HIPCHK(hipSetDevice(device));
  const size_t want = ((size_t)bytes + 4095) & ~(size_t)4095;
  void *p = nullptr;
  e = hipMalloc(&p, want);
  if (e != hipSuccess) return fail(IBWA_EHIP, "hipMalloc(%zu) for the arena: %s", want, hipGetErrorString(e));
  a.base = static_cast<char *>(p);
  a.size = want;
  a.free_[0] = want;
  return 0;
}

int ibwa_release(int device) {
  if (device < 0 || device >= MAX_DEV) return fail(IBWA_EINVAL, "device %d out of range", device);
  Arena &a = g_arena[device];
  std::lock_guard<std::mutex> lk(a.mu);
  if (!a.base) return 0;
  // a buffer still carved from it belongs to a context that may use it again: the contexts go first
  if (a.used > 0)
    return fail(IBWA_EINVAL, "device %d's arena still holds %zu bytes of context buffers (destroy the contexts first)",
                device, a.used);
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipFree(a.base));
  a.base = nullptr;
  a.size = a.used = 0;
  a.free_.clear();
  return 0;
}

int ibwa_arena_stats(int device, uint64_t *size, uint64_t *used, uint64_t *peak) {
  if (device < 0 || device >= MAX_DEV) return fail(IBWA_EINVAL, "device %d out of range", device);
  Arena &a = g_arena[device];
  std::lock_guard<std::mutex> lk(a.mu);
  if (size) *size = a.size;
  if (used) *used = a.used;
  if (peak) *peak = a.peak;
  return 0;
}

int ibwa_device_bytes(int64_t *now, int64_t *peak) {
  if (now) *now = g_dev_bytes.load();
  if (peak) *peak = g_dev_peak.load();
  return 0;
}

int ibwa_ctx_create(int device, ibwa_ctx_t **out) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail(IBWA_EHIP, "no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= n) return fail(IBWA_EINVAL, "device %d out of range (%d devices)", device, n);
  HIPCHK(hipSetDevice(device));
  ibwa_ctx *c = new ibwa_ctx();
  c->device = device;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
  {
    c->exact_blocks = cus * 8;  // 8 x 256-thread blocks per CU: 32 waves/CU when registers allow
    c->n_cus = cus;
  }
  e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  for (auto &x : c->ev)
    if (e == hipSuccess) e = hipEventCreate(&x);
  if (e != hipSuccess) {
    delete c;
    return fail(IBWA_EHIP, "ibwa_ctx_create: %s", hipGetErrorString(e));
  }
  *out = c;
  return 0;
}

void ibwa_ctx_destroy(ibwa_ctx_t *c) {
  if (!c) return;
  (void)enter(c);
  (void)hipStreamSynchronize(c->stream);
  // a context whose index other contexts still borrow (ibwa_ctx_share_index) stays alive until the
  // last of them is destroyed: its index buffers are theirs too
  if (c->n_borrowers > 0) {
    c->destroy_pending = true;
    g_stream = nullptr;
    return;
  }
  // the context whose index this one borrowed is destroyed after this one's own buffers are released
  // (their arena release synchronises this context's stream, g_stream)
  ibwa_ctx *src = c->share_src;
  c->share_src = nullptr;
  // every buffer the context owns is released here, while its stream is alive and g_stream names it;
  // the stream and the events go last (CtxQueue)
  delete c;
  g_stream = nullptr;  // not left naming a destroyed stream
  if (src && --src->n_borrowers == 0 && src->destroy_pending) ibwa_ctx_destroy(src);
}

int ibwa_ctx_set_option(ibwa_ctx_t *c, const char *key, long value) {
  std::string k = key ? key : "";
  if (k == "exact_path") c->exact_path = value != 0;
  else if (k == "kmer_k" && value >= -1 && value <= 16) {
    if (value != c->kmer_k)
      if (int rc = refuse_shared(c, "option kmer_k")) return rc;
    c->kmer_k = (int)value;
    c->index.kmer_valid = false;
  }
  else if (k == "gap_tab_k" && value >= -1 && value <= 14) {
    if (value != c->gap_tab_k) {
      if (int rc = refuse_shared(c, "option gap_tab_k")) return rc;
      c->index.kmer_valid = false;  // built with the K-mer tables
    }
    c->gap_tab_k = (int)value;
  }
  else if (k == "exact_blocks" && value > 0) c->exact_blocks = (int)value;
  else if (k == "lanes_per_chunk" && value > 0) c->lanes_per_chunk = value;
  else if (k == "gapped_v2") c->gapped_v2 = value != 0;
  else if (k == "gap_blocks_per_cu" && value > 0 && value <= 8) c->gap_blocks_per_cu = (int)value;
  else if (k == "gap_cap1" && value >= 16 && value <= 65536) c->gap_cap1 = (uint32_t)value;
  else if (k == "gap_pages_per_block" && value >= 1 && value <= 65536) c->gap_pages_per_block = (int)value;
  else if (k == "gap_hit_slots" && value >= 1 && value <= 4096) c->gap_hit_slots = (uint32_t)value;
  else if (k == "gap_reads_per_chunk" && value > 0) c->gap_reads_per_chunk = value;
  else if (k == "gap_iter_budget" && value >= 0) c->gap_iter_budget = (uint32_t)value;
  else if (k == "gap_early_iters" && value >= 0) c->gap_early_iters = (uint32_t)value;
  else if (k == "gap_early_entries" && value >= 0) c->gap_early_entries = (uint32_t)value;
  else if (k == "gap_lw" && (value == 0 || value == 1)) c->gap_lw = (int)value;
  else if (k == "gap_lw_min_waves" && value >= 1 && value <= 32) c->gap_lw_min_waves = (int)value;
  else if (k == "gap_resume" && (value == 0 || value == 1)) c->gap_resume = (int)value;
  else if (k == "gap_resume_gb" && value >= 1 && value <= 256) c->gap_resume_gb = (int)value;
  else if (k == "gap_resume_records" && value >= 0) c->gap_resume_records = (int64_t)value;
  else if (k == "gap_resume_iters" && value >= 0) c->gap_resume_iters = (uint32_t)value;
  else if (k == "gap_resume_entries" && value >= 0) c->gap_resume_entries = (uint32_t)value;
  else if (k == "gap_tail_lanes" && value >= 0 && value <= 64) c->gap_tail_lanes = (uint32_t)value;
  else if (k == "gap_tail_iters" && value >= 0) c->gap_tail_iters = (uint32_t)value;
  else if (k == "gap_resume_ppb" && value >= 1 && value <= 65536) c->gap_resume_ppb = (int)value;
  else if (k == "gap_resume_cap1" && value >= 16 && value <= 65536) c->gap_resume_cap1 = (uint32_t)value;
  else if (k == "coop_roots" && (value == 0 || value == 1)) c->coop_roots = (int)value;
  else if (k == "gap_stream_per_read" && value >= 0 && value <= 4096) c->gap_stream_per_read = (uint32_t)value;
  else if (k == "gap_stream_min" && value >= 1) c->gap_stream_min = (uint64_t)value;
  else if (k == "exact_jump") c->exact_jump = value != 0;
  else if (k == "jump_derive") c->jump_derive = value != 0;
  else if (k == "width_jump" && value >= 0 && value <= 2) c->width_jump = (int)value;
  else if (k == "width_tab" && value >= 0 && value <= 2) c->width_tab = (int)value;
  else if (k == "width_rec_stage" && (value == 0 || value == 1)) c->width_rec_stage = (int)value;
  else if (k == "diag_width") c->diag_width = value != 0;
  else if (k == "gap_tail_tab" && (value == 0 || value == 1)) c->gap_tail_tab = (int)value;
  else if (k == "diag") c->diag = value != 0;
  else if (k == "sa_walk") c->sa_walk = value != 0;
  else if (k == "gap_coop") c->gap_coop = value != 0;
  else if (k == "coop_early" && (value == 0 || value == 1)) c->coop_early = (int)value;
  else if (k == "coop_waves_per_cu" && value > 0 && value <= 16) c->coop_waves_per_cu = (int)value;
  else if (k == "coop_pool_gb" && value >= 0 && value <= 256) c->coop_pool_gb = (int)value;
  else if (k == "coop_stg_room" && value >= 1 && value <= 4) c->coop_stg_room = (int)value;
  else if (k == "coop_pool_pages" && value >= 0 && value <= (1l << 24)) c->coop_pool_pages = (uint32_t)value;
  else if (k == "gap_resume_recs" && value >= 1 && value <= 65536) c->gap_resume_recs = (uint32_t)value;
  else if (k == "sw_stop" && value >= 0 && value <= 2) c->sw_stop_after = (int)value;  // SW phase timing
  else if (k == "stdaln_suba_rows" && value >= 0) c->stdaln_suba_rows = value;
  else if (k == "stdaln_scratch_mb" && value >= 1 && value <= (1l << 18)) c->stdaln_scratch_mb = value;
  else if (k == "seed_arena_cells" && value >= 0 && value <= (1l << 26)) c->seed_arena_cells = value;
  else if (k == "seed_waves_per_cu" && value >= 1 && value <= 8) c->seed_waves_per_cu = (int)value;
  else if (k == "bsw2_ext_waves_per_cu" && value >= 0 && value <= 8) c->bsw2_ext_waves_per_cu = (int)value;
  else return fail(IBWA_EINVAL, "unknown option %s", k.c_str());
  return 0;
}

int ibwa_ctx_set_tuning(ibwa_ctx_t *c, int stack_cap, int aln_cap, int block) {
  if (stack_cap > 0) c->stack_cap = stack_cap;
  if (aln_cap > 0) c->aln_cap = aln_cap;
  if (block > 0) {
    if (block % 64 || block > 256) return fail(IBWA_EINVAL, "block must be a multiple of 64 and <= 256");
    c->block = block;
  }
  return 0;
}

}  // extern "C"
