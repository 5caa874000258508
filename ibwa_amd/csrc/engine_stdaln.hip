// engine_stdaln.hip -- ibwa_stdaln_batch, ibwa_extend_batch and ibwa_extend_seeds: the parameter presets,
// the checks, and the launches of k_stdaln (stdaln.hip) and k_extend (extend.hip) over a batch cut into
// chunks that fit the per-launch scratch.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <utility>
#include <vector>

#include "engine_ctx.h"
#include "stdaln_core.h"

using namespace ibwa;

namespace {

// BLOSUM62 (Henikoff & Henikoff 1992) as published, lower triangle, residues in the order
// A R N D C Q E G H I L K M F P S T W Y V * X
const int8_t kBlosum62Lower[] = {
    4,
    -1, 5,
    -2, 0, 6,
    -2, -2, 1, 6,
    0, -3, -3, -3, 9,
    -1, 1, 0, 0, -3, 5,
    -1, 0, 0, 2, -4, 2, 5,
    0, -2, 0, -1, -3, -2, -2, 6,
    -2, 0, 1, -1, -3, 0, 0, -2, 8,
    -1, -3, -3, -3, -1, -3, -3, -4, -3, 4,
    -1, -2, -3, -4, -1, -2, -3, -4, -3, 2, 4,
    -1, 2, 0, -1, -3, 1, 1, -2, -1, -3, -2, 5,
    -1, -1, -2, -3, -1, 0, -2, -3, -2, 1, 2, -1, 5,
    -2, -3, -3, -3, -2, -3, -3, -3, -1, 0, 0, -3, 0, 6,
    -1, -2, -2, -1, -3, -1, -1, -2, -2, -3, -3, -1, -2, -4, 7,
    1, -1, 1, 0, -1, 0, 0, 0, -1, -2, -2, 0, -1, -2, -1, 4,
    0, -1, 0, -1, -1, -1, -1, -2, -2, -1, -1, -1, -1, -2, -1, 1, 5,
    -3, -3, -4, -4, -2, -2, -3, -2, -2, -3, -2, -3, -1, 1, -4, -3, -2, 11,
    -2, -2, -2, -3, -2, -1, -2, -3, 2, -1, -1, -2, -1, 3, -3, -2, -2, 2, 7,
    0, -3, -3, -3, -1, -2, -2, -3, -3, 3, 1, -2, 1, -1, -2, -2, 0, -3, -1, 4,
    -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, 1,
    0, -1, -1, -1, -2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -2, 0, 0, -2, -1, -1, -4, -1};

struct Presets {
  int32_t blast[25], bwa[25], aa[22 * 22];
  Presets() {
    for (int x = 0; x < 5; ++x)
      for (int y = 0; y < 5; ++y) {
        const bool n = x == 4 || y == 4;
        blast[x * 5 + y] = n ? -2 : x == y ? 1 : -3;
        bwa[x * 5 + y] = n ? -13 : x == y ? 11 : -19;
      }
    int k = 0;
    for (int x = 0; x < 22; ++x)
      for (int y = 0; y <= x; ++y) aa[x * 22 + y] = aa[y * 22 + x] = kBlosum62Lower[k++];
  }
};
const Presets &presets() {
  static const Presets P;
  return P;
}

struct Checked {
  int max_score = 0;
  int64_t max_step = 0;  // the most one cell can add to or take from a global score
};

int check_param(const ibwa_aln_param_t *ap, int type, int thres, Checked &C) {
  if (!ap || !ap->matrix) return fail(IBWA_EINVAL, "stdaln: no parameters / no score matrix");
  if (type < 0 || type > 2) return fail(IBWA_EINVAL, "stdaln: type %d is none of 0 (local), 1 (global), 2 (extend)", type);
  if (ap->gap_open < 1) return fail(IBWA_EINVAL, "stdaln: gap_open %d < 1", ap->gap_open);
  if (ap->gap_ext < 1) return fail(IBWA_EINVAL, "stdaln: gap_ext %d < 1 (the reverse pass divides by it)", ap->gap_ext);
  if (ap->gap_open + ap->gap_ext > 700) return fail(IBWA_EINVAL, "stdaln: gap_open + gap_ext %d > 700", ap->gap_open + ap->gap_ext);
  if (ap->gap_end > 700) return fail(IBWA_EINVAL, "stdaln: gap_end %d > 700", ap->gap_end);
  if (ap->row < 2 || ap->row > 32) return fail(IBWA_EINVAL, "stdaln: row %d outside 2..32", ap->row);
  int mx = ap->matrix[0], mn = ap->matrix[0];
  for (int i = 0; i < ap->row * ap->row; ++i) {
    mx = std::max<int>(mx, ap->matrix[i]);
    mn = std::min<int>(mn, ap->matrix[i]);
  }
  if (mx <= 0) return fail(IBWA_EINVAL, "stdaln: the score matrix's maximum %d is <= 0", mx);
  if (mx > 32000 || mn < -32000) return fail(IBWA_EINVAL, "stdaln: a matrix score outside -32000..32000");
  if (type == 0 && thres < 1) return fail(IBWA_EINVAL, "stdaln: thres %d < 1 in local mode (the reference then fills no path)", thres);
  C.max_score = mx;
  C.max_step = std::max<int64_t>({mx, -(int64_t)mn, (int64_t)ap->gap_open + std::max(ap->gap_ext, ap->gap_end)});
  return 0;
}

// every code of [seq + off, +len) below row; a range checked before is skipped (stdsw: the pairs
// name the same few long sequences over and over)
struct CodeCheck {
  uint64_t last_off = 0, last_len = UINT64_MAX;
  std::set<std::pair<uint64_t, uint32_t>> done;
  int bad(const uint8_t *seq, uint64_t off, uint32_t len, int row, int64_t &at) {
    if (off == last_off && len == last_len) return -1;
    last_off = off; last_len = len;
    if (len >= 256 && !done.insert({off, len}).second) return -1;  // short ranges: the scan is cheaper
    for (uint32_t k = 0; k < len; ++k)
      if (seq[off + k] >= row) { at = k; return seq[off + k]; }
    return -1;
  }
};

int check_extend_pairs(const ibwa_aln_param_t *ap, int mode, const Checked &C, int64_t n, const uint8_t *seq1, const uint64_t *off1,
                       const uint32_t *len1, const uint8_t *seq2, const uint64_t *off2, const uint32_t *len2, const int32_t *g0);

int check_pairs(const ibwa_aln_param_t *ap, int type, const Checked &C, int64_t n, const uint8_t *seq1, const uint64_t *off1,
                const uint32_t *len1, const uint8_t *seq2, const uint64_t *off2, const uint32_t *len2) {
  if (n < 0) return fail(IBWA_EINVAL, "negative pair count");
  if (type == 2) return check_extend_pairs(ap, 2, C, n, seq1, off1, len1, seq2, off2, len2, nullptr);  // aln_stdaln_aux: G0 = 1, path
  CodeCheck c1, c2;
  for (int64_t p = 0; p < n; ++p) {
    if (len1[p] > (uint32_t)IBWA_STDALN_MAX_LEN || len2[p] > (uint32_t)IBWA_STDALN_MAX_LEN)
      return fail(IBWA_EINVAL, "stdaln: pair %lld: length %u / %u is past %d", (long long)p, len1[p], len2[p], IBWA_STDALN_MAX_LEN);
    if (type == 0 && (uint64_t)C.max_score * std::min(len1[p], len2[p]) > 32000)
      return fail(IBWA_EINVAL, "stdaln: pair %lld: max_score %d * min(len1, len2) %u > 32000", (long long)p, C.max_score,
                  std::min(len1[p], len2[p]));
    if (type == 1 && ((uint64_t)len1[p] + 1) * ((uint64_t)len2[p] + 1) > (uint64_t)IBWA_STDALN_MAX_CELLS)
      return fail(IBWA_EINVAL, "stdaln: pair %lld: (%u + 1) x (%u + 1) cells is past the traceback bound %lld", (long long)p,
                  len1[p], len2[p], (long long)IBWA_STDALN_MAX_CELLS);
    // the global scores are plain ints beside MINOR_INF = -2^30 + 1: no path may move one by 2^30
    if (type == 1 && ((int64_t)len1[p] + len2[p] + 2) * C.max_step >= (1ll << 30))
      return fail(IBWA_EINVAL, "stdaln: pair %lld: (%u + %u) symbols x %lld per cell can pass 2^30, the global core's infinity",
                  (long long)p, len1[p], len2[p], (long long)C.max_step);
    int64_t at = 0;
    int v = c1.bad(seq1, off1[p], len1[p], ap->row, at);
    if (v >= 0) return fail(IBWA_EINVAL, "stdaln: pair %lld: seq1[%lld] = %d is not below row %d", (long long)p, (long long)at, v, ap->row);
    v = c2.bad(seq2, off2[p], len2[p], ap->row, at);
    if (v >= 0) return fail(IBWA_EINVAL, "stdaln: pair %lld: seq2[%lld] = %d is not below row %d", (long long)p, (long long)at, v, ap->row);
  }
  return 0;
}

// a chunk's scratch layout for the maxima max1 / max2 (and, global mode, its most cells)
struct Plan {
  uint32_t e_eh = 0, e_mid = 0, e_suba = 0, mid_w = 1;
  uint64_t wpl = 0, tpl = 0;
  int cap = 1, eh_lds = 0, keep_suba = 0;
  uint64_t per_wave() const { return (wpl * 4 + tpl) * 64; }
};

constexpr uint32_t kEhLdsBytes = 40u << 10;  // eh rows in LDS up to this much per wave (len1 <= 158)

Plan make_plan(int type, const stdaln::Param &sp, int max1, int max2, uint64_t max_cells, int64_t suba_rows) {
  Plan P;
  // local mode: the path fill covers the hit's region only (stdaln::local_span)
  const uint64_t S = std::min(max1, max2);
  const uint64_t w1 = type == 0 ? stdaln::local_span(max1, S, sp) : max1, w2 = type == 0 ? stdaln::local_span(max2, S, sp) : max2;
  P.eh_lds = type == 0 && (uint64_t)(max1 + 2) * 256 <= kEhLdsBytes;
  P.mid_w = (uint32_t)w1 + 1;
  P.e_eh = 0;
  P.e_mid = (type == 0 && !P.eh_lds) ? (uint32_t)max1 + 2 : 0;
  P.e_suba = P.e_mid + 6 * P.mid_w;
  P.keep_suba = type == 0 && max2 <= suba_rows;
  P.wpl = (uint64_t)P.e_suba + (P.keep_suba ? ((uint64_t)max2 + 2) / 2 : 0);
  P.tpl = ((type == 0 ? (w1 + 1) * (w2 + 1) : max_cells) + 7) / 4 * 4;
  P.cap = (int)std::max<uint64_t>(1, w1 + w2);
  return P;
}

// ---- seed extension (extend.hip)

// the checks of the extension's pairs; seq1 == nullptr: the targets are windows of the resident
// sequence (2-bit codes), nothing to scan
int check_extend_pairs(const ibwa_aln_param_t *ap, int mode, const Checked &C, int64_t n, const uint8_t *seq1, const uint64_t *off1,
                       const uint32_t *len1, const uint8_t *seq2, const uint64_t *off2, const uint32_t *len2, const int32_t *g0) {
  if (n < 0) return fail(IBWA_EINVAL, "negative pair count");
  if (mode < 0 || mode > 2) return fail(IBWA_EINVAL, "extend: mode %d is none of 0 (score), 1 (end cell), 2 (path)", mode);
  CodeCheck c1, c2;
  for (int64_t p = 0; p < n; ++p) {
    if (len1[p] > (uint32_t)IBWA_STDALN_MAX_LEN || len2[p] > (uint32_t)IBWA_STDALN_MAX_LEN)
      return fail(IBWA_EINVAL, "extend: pair %lld: length %u / %u is past %d", (long long)p, len1[p], len2[p], IBWA_STDALN_MAX_LEN);
    if (g0 && (g0[p] < 1 || g0[p] > 32000))
      return fail(IBWA_EINVAL, "extend: pair %lld: G0 %d outside 1..32000", (long long)p, g0[p]);
    if (mode == 2 && len1[p] && len2[p]) {
      // the path fill covers seq1[0, end_i) x seq2[0, end_j), and the band bounds the end cell
      const int band = stdaln::extend_band(ap->band_width, (int)len1[p], (int)len2[p]);
      const uint64_t w1 = stdaln::extend_span1(band, (int)len1[p], (int)len2[p]), w2 = stdaln::extend_span2(band, (int)len1[p], (int)len2[p]);
      if ((w1 + 1) * (w2 + 1) > (uint64_t)IBWA_STDALN_MAX_CELLS)
        return fail(IBWA_EINVAL, "extend: pair %lld: the path fill of %u x %u in band %d can take (%llu + 1) x (%llu + 1) cells, past "
                    "the traceback bound %lld", (long long)p, len1[p], len2[p], band, (unsigned long long)w1, (unsigned long long)w2,
                    (long long)IBWA_STDALN_MAX_CELLS);
      if ((int64_t)(w1 + w2 + 2) * C.max_step >= (1ll << 30))
        return fail(IBWA_EINVAL, "extend: pair %lld: (%llu + %llu) symbols x %lld per cell can pass 2^30, the global core's infinity",
                    (long long)p, (unsigned long long)w1, (unsigned long long)w2, (long long)C.max_step);
    }
    int64_t at = 0;
    int v = seq1 ? c1.bad(seq1, off1[p], len1[p], ap->row, at) : -1;
    if (v >= 0) return fail(IBWA_EINVAL, "extend: pair %lld: seq1[%lld] = %d is not below row %d", (long long)p, (long long)at, v, ap->row);
    v = c2.bad(seq2, off2[p], len2[p], ap->row, at);
    if (v >= 0) return fail(IBWA_EINVAL, "extend: pair %lld: seq2[%lld] = %d is not below row %d", (long long)p, (long long)at, v, ap->row);
  }
  return 0;
}

// a chunk's scratch layout for the extension
struct ExtPlan {
  uint32_t ring = 3, lds_ring = 3, eh_words = 0, mid_w = 1;
  uint64_t wpl = 0, tpl = 0;
  int cap = 0, all_lds = 1;
  uint64_t per_wave() const { return (wpl * 4 + tpl) * 64; }
};

struct ExtMax {  // a run's maxima: the widest ring, and for the path fill the widest row, most cells, longest path
  uint32_t ring = 3;
  uint64_t w1 = 0, cells = 0, cap = 0;
  void add(int band_width, uint32_t l1, uint32_t l2, int mode) {
    const int band = stdaln::extend_band(band_width, (int)l1, (int)l2);
    ring = std::max(ring, stdaln::extend_ring(band, (int)l1));
    if (mode == 2) {
      const uint64_t a = stdaln::extend_span1(band, (int)l1, (int)l2), b = stdaln::extend_span2(band, (int)l1, (int)l2);
      w1 = std::max(w1, a);
      cells = std::max(cells, (a + 1) * (b + 1));
      cap = std::max(cap, a + b);
    }
  }
};

ExtPlan make_ext_plan(int mode, const ExtMax &M) {
  ExtPlan P;
  const uint32_t lds_words = kEhLdsBytes / 256;
  P.ring = M.ring;
  P.all_lds = M.ring <= lds_words;
  P.lds_ring = P.all_lds ? M.ring : lds_words;
  P.eh_words = P.all_lds ? 0 : M.ring;
  if (mode == 2) {
    P.mid_w = (uint32_t)M.w1 + 1;
    P.wpl = (uint64_t)P.eh_words + 6ull * P.mid_w;
    P.tpl = (M.cells + 7) / 4 * 4;
    P.cap = (int)std::max<uint64_t>(1, M.cap);
  } else {
    P.wpl = P.eh_words;
  }
  return P;
}

struct ExtJob {
  int mode;
  int64_t n;
  const uint8_t *seq1;  // nullptr: the targets are on the device already (StdBufs::s1, off1 / len1 as given)
  const uint64_t *off1;
  const uint32_t *len1;
  const uint8_t *seq2;
  const uint64_t *off2;
  const uint32_t *len2;
  const int32_t *g0;
  int32_t *score, *ends4, *path_len, *n_cigar;  // ends4: start i, start j, end i, end j
  uint32_t **cigar;                             // mode 2
  int64_t *n_cigar_total;
};

// the launches of k_extend over the job cut into runs that fit the per-launch scratch.  The caller has
// checked the pairs; the context is entered.
int extend_run(ibwa_ctx_t *c, const ibwa_aln_param_t *ap, const Checked &C, const ExtJob &J) {
  const int64_t n = J.n;
  if (J.cigar) *J.cigar = nullptr;
  if (J.n_cigar_total) *J.n_cigar_total = 0;
  c->stdaln_chunks = 0;
  c->stdaln_ms = 0;
  c->extend_no_band = 0;
  if (n == 0) {
    if (J.cigar) *J.cigar = (uint32_t *)malloc(4);
    return 0;
  }
  uint64_t end1 = 0, end2 = 0;
  for (int64_t p = 0; p < n; ++p) {
    end1 = std::max<uint64_t>(end1, J.off1[p] + J.len1[p]);
    end2 = std::max<uint64_t>(end2, J.off2[p] + J.len2[p]);
  }
  StdBufs &W = c->sd;
  int rc = 0;
  if ((J.seq1 && (rc = W.s1.ensure(end1 + 16))) || (rc = W.s2.ensure(end2 + 16)) || (rc = W.o1.ensure(n * 8)) ||
      (rc = W.o2.ensure(n * 8)) || (rc = W.l1.ensure(n * 4)) || (rc = W.l2.ensure(n * 4)) || (rc = W.g0.ensure(n * 4)) ||
      (rc = W.sc.ensure(n * 4)) || (rc = W.su.ensure(n * 4)) || (rc = W.pl.ensure(n * 4)) || (rc = W.nc.ensure(n * 4)) ||
      (rc = W.en.ensure(n * 16)) || (rc = W.cf.ensure(n * 8)) || (rc = W.mat.ensure(32 * 32 * 4)) || (rc = c->d_counter.ensure(64)))
    return rc;
  auto chk = [&](hipError_t e, const char *what) {
    if (e != hipSuccess && !rc) rc = fail(IBWA_EHIP, "%s: %s", what, hipGetErrorString(e));
  };
  if (J.seq1) chk(hipMemcpyAsync(W.s1.p, J.seq1, end1, hipMemcpyHostToDevice, c->stream), "H2D seq1");
  chk(hipMemcpyAsync(W.s2.p, J.seq2, end2, hipMemcpyHostToDevice, c->stream), "H2D seq2");
  chk(hipMemcpyAsync(W.o1.p, J.off1, n * 8, hipMemcpyHostToDevice, c->stream), "H2D off1");
  chk(hipMemcpyAsync(W.o2.p, J.off2, n * 8, hipMemcpyHostToDevice, c->stream), "H2D off2");
  chk(hipMemcpyAsync(W.l1.p, J.len1, n * 4, hipMemcpyHostToDevice, c->stream), "H2D len1");
  chk(hipMemcpyAsync(W.l2.p, J.len2, n * 4, hipMemcpyHostToDevice, c->stream), "H2D len2");
  if (J.g0) chk(hipMemcpyAsync(W.g0.p, J.g0, n * 4, hipMemcpyHostToDevice, c->stream), "H2D g0");
  chk(hipMemcpyAsync(W.mat.p, ap->matrix, (size_t)ap->row * ap->row * 4, hipMemcpyHostToDevice, c->stream), "H2D matrix");
  if (rc) return rc;

  const uint64_t budget = (uint64_t)c->stdaln_scratch_mb << 20;
  const uint64_t cig_budget = budget / 16, dp_budget = budget - cig_budget;
  std::vector<uint32_t> all_cig;
  std::vector<uint64_t> first;
  std::vector<int32_t> flags;
  for (int64_t p0 = 0; p0 < n && !rc;) {
    ExtMax M;
    ExtPlan P;
    int64_t p1 = p0;
    for (; p1 < n; ++p1) {
      ExtMax N = M;
      N.add(ap->band_width, J.len1[p1], J.len2[p1], J.mode);
      const ExtPlan Q = make_ext_plan(J.mode, N);
      // the run ends before a pair that takes its CIGAR rows or one wave's scratch past the budget
      if (p1 > p0 && ((uint64_t)(p1 - p0 + 1) * Q.cap * 4 > cig_budget || Q.per_wave() > dp_budget)) break;
      M = N; P = Q;
    }
    const int64_t m = p1 - p0;
    const uint64_t pw = P.per_wave();
    if (pw > dp_budget || (uint64_t)m * P.cap * 4 > cig_budget)
      return fail(IBWA_EINVAL, "extend: pair %lld (%u x %u) needs %llu MiB of scratch, past the %lld MiB of one launch "
                  "(option stdaln_scratch_mb)", (long long)p0, J.len1[p0], J.len2[p0],
                  (unsigned long long)((pw + (uint64_t)m * P.cap * 4) >> 20) + 1, (long long)c->stdaln_scratch_mb);
    ExtArgs A = {};
    A.seq1 = W.s1.as<uint8_t>(); A.seq2 = W.s2.as<uint8_t>();
    A.off1 = W.o1.as<uint64_t>() + p0; A.off2 = W.o2.as<uint64_t>() + p0;
    A.len1 = W.l1.as<uint32_t>() + p0; A.len2 = W.l2.as<uint32_t>() + p0;
    A.g0 = J.g0 ? W.g0.as<int32_t>() + p0 : nullptr;
    A.n = m;
    A.gap_open = ap->gap_open; A.gap_ext = ap->gap_ext; A.band = ap->band_width; A.row = ap->row; A.max_score = C.max_score;
    A.matrix = W.mat.as<int32_t>();
    A.mode = J.mode;
    A.lds_ring = P.lds_ring;
    // as many single-wave workgroups as a CU's 160 KiB of LDS holds, eight at the most
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(8, (160 << 10) / extend_lds_bytes(A)));
    const int64_t waves = std::max<int64_t>(1, std::min<int64_t>({(m + 63) / 64, pw ? (int64_t)(dp_budget / pw) : INT64_MAX,
                                                                  (int64_t)c->n_cus * per_cu}));
    if ((rc = W.scr.ensure((uint64_t)waves * P.wpl * 4 * 64 + 256)) || (rc = W.tbb.ensure((uint64_t)waves * P.tpl * 64 + 256)) ||
        (rc = W.cg.ensure((uint64_t)m * P.cap * 4 + 4)))
      return rc;
    A.scratch = W.scr.as<uint32_t>(); A.words_per_lane = P.wpl;
    A.e_mid = P.eh_words; A.mid_w = P.mid_w;
    A.tb = W.tbb.as<uint8_t>(); A.tb_per_lane = P.tpl;
    A.score = W.sc.as<int32_t>() + p0; A.no_band = W.su.as<int32_t>() + p0; A.path_len = W.pl.as<int32_t>() + p0;
    A.n_cigar = W.nc.as<int32_t>() + p0; A.ends = W.en.as<int4>() + p0;
    A.cigar = W.cg.as<uint32_t>(); A.cigar_cap = P.cap;
    chk(hipEventRecord(c->ev[0], c->stream), "event");
    chk(launch_extend(A, P.all_lds != 0, counter(c, CTR_CLAIM), (int)waves, c->stream), "k_extend");
    chk(hipEventRecord(c->ev[1], c->stream), "event");
    chk(hipMemcpyAsync(J.score + p0, A.score, m * 4, hipMemcpyDeviceToHost, c->stream), "D2H score");
    chk(hipMemcpyAsync(J.ends4 + 4 * p0, A.ends, m * 16, hipMemcpyDeviceToHost, c->stream), "D2H ends");
    if (J.mode == 2) {
      flags.resize(m);
      chk(hipMemcpyAsync(flags.data(), A.no_band, m * 4, hipMemcpyDeviceToHost, c->stream), "D2H no_band");
      chk(hipMemcpyAsync(J.path_len + p0, A.path_len, m * 4, hipMemcpyDeviceToHost, c->stream), "D2H path_len");
      chk(hipMemcpyAsync(J.n_cigar + p0, A.n_cigar, m * 4, hipMemcpyDeviceToHost, c->stream), "D2H n_cigar");
    }
    chk(hipStreamSynchronize(c->stream), "sync");
    if (rc) return rc;
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->stdaln_ms += ms;
    ++c->stdaln_chunks;
    if (J.mode == 2) {
      for (int64_t p = 0; p < m; ++p) {
        if (J.score[p0 + p] == INT32_MIN)
          return fail(IBWA_EINVAL, "extend: pair %lld: the end cell lies outside the band's reach, past the path fill's scratch",
                      (long long)(p0 + p));
        c->extend_no_band += flags[p];
      }
      // the chunk's CIGARs packed on the device, appended on the host
      first.resize(m);
      uint64_t tot = 0;
      for (int64_t p = 0; p < m; ++p) {
        first[p] = tot;
        tot += (uint64_t)J.n_cigar[p0 + p];
      }
      if (tot) {
        if ((rc = W.cc.ensure(tot * 4))) return rc;
        const size_t at = all_cig.size();
        all_cig.resize(at + tot);
        chk(hipMemcpyAsync(W.cf.p, first.data(), m * 8, hipMemcpyHostToDevice, c->stream), "H2D cigar offsets");
        chk(launch_pack_cigar(A.cigar, P.cap, A.n_cigar, W.cf.as<uint64_t>(), m, W.cc.as<uint32_t>(), c->stream), "k_pack_cigar");
        chk(hipMemcpyAsync(all_cig.data() + at, W.cc.p, tot * 4, hipMemcpyDeviceToHost, c->stream), "D2H cigar");
        chk(hipStreamSynchronize(c->stream), "sync");
        if (rc) return rc;
      }
    }
    p0 = p1;
  }
  if (rc) return rc;
  if (J.cigar) {
    uint32_t *o = (uint32_t *)malloc(std::max<size_t>(all_cig.size(), 1) * 4);
    if (!o) return fail(IBWA_EINVAL, "out of host memory");
    if (!all_cig.empty()) memcpy(o, all_cig.data(), all_cig.size() * 4);
    *J.cigar = o;
    if (J.n_cigar_total) *J.n_cigar_total = (int64_t)all_cig.size();
  }
  return 0;
}

}  // namespace

extern "C" {

int ibwa_aln_param_preset(const char *name, ibwa_aln_param_t *ap) {
  const std::string k = name ? name : "";
  if (!ap) return fail(IBWA_EINVAL, "no parameter struct");
  const Presets &P = presets();
  if (k == "blast") *ap = {5, 2, 2, P.blast, 5, 50};
  else if (k == "bwa") *ap = {26, 9, 5, P.bwa, 5, 50};
  else if (k == "aa2aa") *ap = {10, 2, 2, P.aa, 22, 50};
  else return fail(IBWA_EINVAL, "unknown alignment preset %s (blast, aa2aa, bwa)", k.c_str());
  return 0;
}

int ibwa_stdaln_check(const ibwa_aln_param_t *ap, int type, int thres, int64_t n, const uint8_t *seq1, const uint64_t *off1,
                      const uint32_t *len1, const uint8_t *seq2, const uint64_t *off2, const uint32_t *len2) {
  Checked C;
  if (int rc = check_param(ap, type, thres, C)) return rc;
  return check_pairs(ap, type, C, n, seq1, off1, len1, seq2, off2, len2);
}

int ibwa_stdaln_chunks(const ibwa_ctx_t *c, int64_t *launches, double *kernel_ms) {
  if (launches) *launches = c->stdaln_chunks;
  if (kernel_ms) *kernel_ms = c->stdaln_ms;
  return 0;
}

int ibwa_extend_check(const ibwa_aln_param_t *ap, int mode, int64_t n, const uint8_t *seq1, const uint64_t *off1, const uint32_t *len1,
                      const uint8_t *seq2, const uint64_t *off2, const uint32_t *len2, const int32_t *g0) {
  Checked C;
  if (int rc = check_param(ap, 2, 1, C)) return rc;
  return check_extend_pairs(ap, mode, C, n, seq1, off1, len1, seq2, off2, len2, g0);
}

int ibwa_extend_stats(const ibwa_ctx_t *c, int64_t *no_band) {
  if (no_band) *no_band = c->extend_no_band;
  return 0;
}

int ibwa_extend_batch(ibwa_ctx_t *c, const ibwa_aln_param_t *ap, int mode, int64_t n, const uint8_t *seq1, const uint64_t *off1,
                      const uint32_t *len1, const uint8_t *seq2, const uint64_t *off2, const uint32_t *len2, const int32_t *g0,
                      int32_t *score, int32_t *ends, int32_t *path_len, int32_t *n_cigar, uint32_t **cigar, int64_t *n_cigar_total) {
  Checked C;
  if (int rc = check_param(ap, 2, 1, C)) return rc;
  if (int rc = check_extend_pairs(ap, mode, C, n, seq1, off1, len1, seq2, off2, len2, g0)) return rc;
  if (mode == 2 && (!path_len || !n_cigar || !cigar)) return fail(IBWA_EINVAL, "extend: path mode needs path_len, n_cigar and cigar");
  if (n > 0) HIPCHK(enter(c));
  std::vector<int32_t> e4((size_t)n * 4);
  const ExtJob J = {mode, n, seq1, off1, len1, seq2, off2, len2, g0, score, e4.data(), path_len, n_cigar, mode == 2 ? cigar : nullptr,
                    n_cigar_total};
  if (mode != 2) {
    if (cigar) *cigar = nullptr;
    if (n_cigar_total) *n_cigar_total = 0;
  }
  if (int rc = extend_run(c, ap, C, J)) return rc;
  for (int64_t p = 0; p < n; ++p) {
    ends[2 * p] = e4[4 * p + 2];
    ends[2 * p + 1] = e4[4 * p + 3];
    if (mode != 2) {
      if (path_len) path_len[p] = 0;
      if (n_cigar) n_cigar[p] = 0;
    }
  }
  return 0;
}

int ibwa_extend_seeds(ibwa_ctx_t *c, const ibwa_aln_param_t *ap, int64_t n, const uint64_t *pos, const uint8_t *dir, const uint32_t *lt,
                      int rev, const uint8_t *qry, const uint64_t *off, const uint32_t *len, const int32_t *g0, int32_t *score,
                      int32_t *ends) {
  Checked C;
  if (int rc = check_param(ap, 2, 1, C)) return rc;
  if (ap->row < 4) return fail(IBWA_EINVAL, "extend_seeds: row %d < 4, the targets are nucleotide codes 0..3", ap->row);
  if (!c->index.pac_loaded) return fail(IBWA_ENOINDEX, "no reference sequence loaded (ibwa_ctx_load_pac)");
  if (n < 0) return fail(IBWA_EINVAL, "negative pair count");
  const uint64_t l = c->index.pac_len;
  // the windows: right, the bases pos .. clipped at l; left, pos - 1 down to base 0
  std::vector<uint64_t> off1((size_t)n);
  std::vector<uint32_t> len1((size_t)n);
  uint64_t tot = 0;
  for (int64_t p = 0; p < n; ++p) {
    if (dir[p] > 1) return fail(IBWA_EINVAL, "extend_seeds: seed %lld: dir %d is neither 0 (right) nor 1 (left)", (long long)p, dir[p]);
    if (dir[p] && pos[p] > l)
      return fail(IBWA_EINVAL, "extend_seeds: seed %lld: position %llu > l_pac %llu", (long long)p, (unsigned long long)pos[p],
                  (unsigned long long)l);
    const uint64_t room = dir[p] ? pos[p] : (pos[p] < l ? l - pos[p] : 0);
    len1[p] = (uint32_t)std::min<uint64_t>(lt[p], room);
    off1[p] = tot;
    tot += len1[p];
  }
  if (int rc = check_extend_pairs(ap, 1, C, n, nullptr, off1.data(), len1.data(), qry, off, len, g0)) return rc;
  std::vector<int32_t> e4((size_t)n * 4);
  if (n > 0) {
    HIPCHK(enter(c));
    StdBufs &W = c->sd;
    int rc = 0;
    if ((rc = W.s1.ensure(tot + 16)) || (rc = W.o1.ensure(n * 8)) || (rc = W.l1.ensure(n * 4)) || (rc = W.pos.ensure(n * 8)) ||
        (rc = W.dir.ensure(n + 16)))
      return rc;
    HIPCHK(hipMemcpyAsync(W.o1.p, off1.data(), n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(W.l1.p, len1.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(W.pos.p, pos, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(W.dir.p, dir, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_extend_gather(c->index.pac.as<uint32_t>(), l, rev != 0, n, W.pos.as<uint64_t>(), W.dir.as<uint8_t>(),
                                W.o1.as<uint64_t>(), W.l1.as<uint32_t>(), W.s1.as<uint8_t>(), c->stream));
  }
  const ExtJob J = {1, n, nullptr, off1.data(), len1.data(), qry, off, len, g0, score, e4.data(), nullptr, nullptr, nullptr, nullptr};
  if (int rc = extend_run(c, ap, C, J)) return rc;
  for (int64_t p = 0; p < n; ++p) {
    ends[2 * p] = e4[4 * p + 2];
    ends[2 * p + 1] = e4[4 * p + 3];
  }
  return 0;
}

int ibwa_stdaln_batch(ibwa_ctx_t *c, const ibwa_aln_param_t *ap, int type, int thres, int64_t n, const uint8_t *seq1,
                      const uint64_t *off1, const uint32_t *len1, const uint8_t *seq2, const uint64_t *off2,
                      const uint32_t *len2, int32_t *score, int32_t *subo, int32_t *path_len, int32_t *ends,
                      int32_t *n_cigar, uint32_t **cigar, int64_t *n_cigar_total) {
  Checked C;
  if (int rc = check_param(ap, type, thres, C)) return rc;
  if (int rc = check_pairs(ap, type, C, n, seq1, off1, len1, seq2, off2, len2)) return rc;
  if (type == 2) {  // aln_stdaln_aux's extend: G0 = 1, the path; ends = its first and last entry
    if (n > 0) HIPCHK(enter(c));
    const ExtJob J = {2, n, seq1, off1, len1, seq2, off2, len2, nullptr, score, ends, path_len, n_cigar, cigar, n_cigar_total};
    if (n > 0) memset(subo, 0, (size_t)n * 4);
    return extend_run(c, ap, C, J);
  }
  *cigar = nullptr;
  if (n_cigar_total) *n_cigar_total = 0;
  c->stdaln_chunks = 0;
  c->stdaln_ms = 0;
  if (n == 0) {
    *cigar = (uint32_t *)malloc(4);
    return 0;
  }
  HIPCHK(enter(c));
  uint64_t end1 = 0, end2 = 0;
  for (int64_t p = 0; p < n; ++p) {
    end1 = std::max<uint64_t>(end1, off1[p] + len1[p]);
    end2 = std::max<uint64_t>(end2, off2[p] + len2[p]);
  }
  StdBufs &W = c->sd;
  int rc = 0;
  if ((rc = W.s1.ensure(end1 + 16)) || (rc = W.s2.ensure(end2 + 16)) || (rc = W.o1.ensure(n * 8)) || (rc = W.o2.ensure(n * 8)) ||
      (rc = W.l1.ensure(n * 4)) || (rc = W.l2.ensure(n * 4)) || (rc = W.sc.ensure(n * 4)) || (rc = W.su.ensure(n * 4)) ||
      (rc = W.pl.ensure(n * 4)) || (rc = W.nc.ensure(n * 4)) || (rc = W.en.ensure(n * 16)) || (rc = W.cf.ensure(n * 8)) ||
      (rc = W.mat.ensure(32 * 32 * 4)) || (rc = c->d_counter.ensure(64)))
    return rc;
  auto chk = [&](hipError_t e, const char *what) {
    if (e != hipSuccess && !rc) rc = fail(IBWA_EHIP, "%s: %s", what, hipGetErrorString(e));
  };
  chk(hipMemcpyAsync(W.s1.p, seq1, end1, hipMemcpyHostToDevice, c->stream), "H2D seq1");
  chk(hipMemcpyAsync(W.s2.p, seq2, end2, hipMemcpyHostToDevice, c->stream), "H2D seq2");
  chk(hipMemcpyAsync(W.o1.p, off1, n * 8, hipMemcpyHostToDevice, c->stream), "H2D off1");
  chk(hipMemcpyAsync(W.o2.p, off2, n * 8, hipMemcpyHostToDevice, c->stream), "H2D off2");
  chk(hipMemcpyAsync(W.l1.p, len1, n * 4, hipMemcpyHostToDevice, c->stream), "H2D len1");
  chk(hipMemcpyAsync(W.l2.p, len2, n * 4, hipMemcpyHostToDevice, c->stream), "H2D len2");
  chk(hipMemcpyAsync(W.mat.p, ap->matrix, (size_t)ap->row * ap->row * 4, hipMemcpyHostToDevice, c->stream), "H2D matrix");
  if (rc) return rc;

  // the per-launch scratch: a sixteenth for a chunk's CIGAR rows, the rest for the waves' DP scratch
  const uint64_t budget = (uint64_t)c->stdaln_scratch_mb << 20;
  const uint64_t cig_budget = budget / 16, dp_budget = budget - cig_budget;
  const stdaln::Param sp = {ap->gap_open, ap->gap_ext, ap->gap_end, ap->band_width, ap->row, C.max_score, nullptr};
  std::vector<uint32_t> all_cig;
  std::vector<uint64_t> first;
  for (int64_t p0 = 0; p0 < n && !rc;) {
    // the longest run of pairs whose CIGAR rows fit
    int max1 = 0, max2 = 0;
    uint64_t cells = 0;
    int64_t p1 = p0;
    Plan P;
    for (; p1 < n; ++p1) {
      const int m1 = std::max<int>(max1, (int)len1[p1]), m2 = std::max<int>(max2, (int)len2[p1]);
      const uint64_t cl = std::max<uint64_t>(cells, ((uint64_t)len1[p1] + 1) * ((uint64_t)len2[p1] + 1));
      const Plan Q = make_plan(type, sp, m1, m2, cl, c->stdaln_suba_rows);
      // the run ends before a pair that takes its CIGAR rows or one wave's scratch past the budget
      if (p1 > p0 && ((uint64_t)(p1 - p0 + 1) * Q.cap * 4 > cig_budget || Q.per_wave() > dp_budget)) break;
      max1 = m1; max2 = m2; cells = cl; P = Q;
    }
    const int64_t m = p1 - p0;
    const uint64_t pw = P.per_wave();
    if (pw > dp_budget || (uint64_t)m * P.cap * 4 > cig_budget)
      return fail(IBWA_EINVAL, "stdaln: pair %lld (%u x %u) needs %llu MiB of scratch, past the %lld MiB of one launch "
                  "(option stdaln_scratch_mb)", (long long)p0, len1[p0], len2[p0],
                  (unsigned long long)((pw + (uint64_t)m * P.cap * 4) >> 20) + 1, (long long)c->stdaln_scratch_mb);
    const int64_t waves = std::max<int64_t>(1, std::min<int64_t>({(m + 63) / 64, (int64_t)(dp_budget / pw), (int64_t)c->n_cus * 8}));
    if ((rc = W.scr.ensure((uint64_t)waves * P.wpl * 4 * 64 + 256)) || (rc = W.tbb.ensure((uint64_t)waves * P.tpl * 64 + 256)) ||
        (rc = W.cg.ensure((uint64_t)m * P.cap * 4)))
      return rc;
    StdArgs A = {};
    A.seq1 = W.s1.as<uint8_t>(); A.seq2 = W.s2.as<uint8_t>();
    A.off1 = W.o1.as<uint64_t>() + p0; A.off2 = W.o2.as<uint64_t>() + p0;
    A.len1 = W.l1.as<uint32_t>() + p0; A.len2 = W.l2.as<uint32_t>() + p0;
    A.n = m;
    A.gap_open = ap->gap_open; A.gap_ext = ap->gap_ext; A.gap_end = ap->gap_end; A.band = ap->band_width;
    A.row = ap->row; A.max_score = C.max_score;
    A.matrix = W.mat.as<int32_t>();
    A.type = type; A.thres = thres;
    A.max_len1 = max1; A.eh_lds = P.eh_lds; A.keep_suba = P.keep_suba;
    A.scratch = W.scr.as<uint32_t>(); A.words_per_lane = P.wpl;
    A.e_eh = P.e_eh; A.e_mid = P.e_mid; A.e_suba = P.e_suba; A.mid_w = P.mid_w;
    A.tb = W.tbb.as<uint8_t>(); A.tb_per_lane = P.tpl;
    A.score = W.sc.as<int32_t>() + p0; A.subo = W.su.as<int32_t>() + p0; A.path_len = W.pl.as<int32_t>() + p0;
    A.n_cigar = W.nc.as<int32_t>() + p0; A.ends = W.en.as<int4>() + p0;
    A.cigar = W.cg.as<uint32_t>(); A.cigar_cap = P.cap;
    chk(hipEventRecord(c->ev[0], c->stream), "event");
    chk(launch_stdaln(A, counter(c, CTR_CLAIM), (int)waves, c->stream), "k_stdaln");
    chk(hipEventRecord(c->ev[1], c->stream), "event");
    chk(hipMemcpyAsync(score + p0, A.score, m * 4, hipMemcpyDeviceToHost, c->stream), "D2H score");
    chk(hipMemcpyAsync(subo + p0, A.subo, m * 4, hipMemcpyDeviceToHost, c->stream), "D2H subo");
    chk(hipMemcpyAsync(path_len + p0, A.path_len, m * 4, hipMemcpyDeviceToHost, c->stream), "D2H path_len");
    chk(hipMemcpyAsync(n_cigar + p0, A.n_cigar, m * 4, hipMemcpyDeviceToHost, c->stream), "D2H n_cigar");
    chk(hipMemcpyAsync(ends + 4 * p0, A.ends, m * 16, hipMemcpyDeviceToHost, c->stream), "D2H ends");
    chk(hipStreamSynchronize(c->stream), "sync");
    if (rc) return rc;
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->stdaln_ms += ms;
    ++c->stdaln_chunks;
    for (int64_t p = p0; p < p1; ++p)
      if (score[p] == INT32_MIN)
        return fail(IBWA_EINVAL, "stdaln: pair %lld: the reverse pass left the forward pass's hit (the reference's 'unknown "
                    "flaw', score_f != score_r) for a region past the path fill's scratch", (long long)p);
    // the chunk's CIGARs packed on the device, appended on the host
    first.resize(m);
    uint64_t tot = 0;
    for (int64_t p = 0; p < m; ++p) {
      first[p] = tot;
      tot += (uint64_t)n_cigar[p0 + p];
    }
    if (tot) {
      if ((rc = W.cc.ensure(tot * 4))) return rc;
      const size_t at = all_cig.size();
      all_cig.resize(at + tot);
      chk(hipMemcpyAsync(W.cf.p, first.data(), m * 8, hipMemcpyHostToDevice, c->stream), "H2D cigar offsets");
      chk(launch_pack_cigar(A.cigar, P.cap, A.n_cigar, W.cf.as<uint64_t>(), m, W.cc.as<uint32_t>(), c->stream), "k_pack_cigar");
      chk(hipMemcpyAsync(all_cig.data() + at, W.cc.p, tot * 4, hipMemcpyDeviceToHost, c->stream), "D2H cigar");
      chk(hipStreamSynchronize(c->stream), "sync");
      if (rc) return rc;
    }
    p0 = p1;
  }
  if (rc) return rc;
  uint32_t *o = (uint32_t *)malloc(std::max<size_t>(all_cig.size(), 1) * 4);
  if (!o) return fail(IBWA_EINVAL, "out of host memory");
  if (!all_cig.empty()) memcpy(o, all_cig.data(), all_cig.size() * 4);
  *cigar = o;
  if (n_cigar_total) *n_cigar_total = (int64_t)all_cig.size();
  return 0;
}

}  // extern "C"
