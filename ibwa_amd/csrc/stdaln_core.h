// stdaln_core.h -- aln_local_core (stdaln.c:529-760), aln_global_core (stdaln.c:345-525) and
// aln_extend_core (stdaln.c:862-1008) for a run-time AlnParam, one alignment per caller.  The passes are
// written over strided views of the caller's storage, so that the kernels (stdaln.hip, extend.hip: a
// lane's elements 64 apart, the eh row in LDS or in HBM) and a host build (stride 1) run the same
// statements.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define STD_HD __host__ __device__ __forceinline__
#else
#define STD_HD inline
#endif

namespace ibwa {
namespace stdaln {

constexpr int NEG_INF = -1073741823;   // MINOR_INF (stdaln.h:84)
constexpr int FM = 0, FI = 1, FD = 2;  // FROM_M / FROM_I / FROM_D
constexpr int REFUSED = INT32_MIN;     // score of a pair whose path fill is past the traceback area

// element e of a view lies at p[e * s]
template <class T>
struct View {
  T *p;
  uint32_t s;
  STD_HD T &operator[](uint64_t e) const { return p[e * s]; }
};

// traceback bytes: the dword of bytes 4q .. 4q+3 of a lane at (q * s + lane) * 4
struct TbView {
  uint8_t *p;
  uint32_t s, lane;
  STD_HD uint8_t &operator[](uint64_t e) const { return p[((e >> 2) * s + lane) * 4 + (e & 3)]; }
};

struct Param {
  int q, r, gap_end, band, row, max_score;
  const int *mat;  // row x row
};

// a + .33 * span + .499 and a - .33 * span + .499 in double, one rounding per operation as the
// reference's host code does them (no fused multiply-add), truncated toward zero
STD_HD int subo_bound(int a, int span, bool minus) {
#if defined(__HIP_DEVICE_COMPILE__)
  const double pr = __dmul_rn(.33, (double)span);
  const double x = minus ? __dsub_rn((double)a, pr) : __dadd_rn((double)a, pr);
  return (int)__dadd_rn(x, .499);
#else
  volatile double pr = .33 * (double)span;
  volatile double x = minus ? (double)a - pr : (double)a + pr;
  volatile double y = x + .499;
  return (int)y;
#endif
}

// banded global alignment.  seq1 = a[0..n1) along i (FROM_D steps i), seq2 = b[0..n2) along j
// (FROM_I steps j).  Row j covers lo(j)..hi(j): lo = 0 while j <= b2 (cell 0 takes an I from above by
// set_end_I) and j - b2 after (the -inf cell of SET_INF(curr[j - b2])); hi = min(j + b1 - 1, n1), and
// the last cell takes an I from above only when the band was clipped at len1 (set_end_I) -- the
// union of the reference's part 1-3 rows.  The last row's deletions are set_end_D, except where the
// reference reaches the last row inside its part 2 loop (b2 == 1 and len2 >= 2), which uses set_D.
// mid: (M, I, D) of two rows, element ((sel * W + i) * 3 + k); T: one byte per cell, row j at
// j * (n1 + 1).  The path is traced into cig (end -> start, run-length encoded; the caller reverses
// it); si / sj are the cell of the last counted path entry.
template <class MID, class TB>
STD_HD int global_core(const MID &mid, uint32_t W, const TB &T, const Param &P, const uint8_t *a, int n1,
                       const uint8_t *b, int n2, int band, int gap_end, uint32_t *cig, int cap, int &n_cig,
                       int &path_len, int &si, int &sj) {
  const int Q = P.q, R = P.r;
  const int RE = gap_end >= 0 ? gap_end : R;
  int b1, b2;
  if (n1 > n2) { b1 = n1 - n2 + band; b2 = band; } else { b1 = band; b2 = n2 - n1 + band; }
  if (b1 > n1 || b1 < 0) b1 = n1;  // < 0: the doubled band wrapped
  if (b2 > n2 || b2 < 0) b2 = n2;
  const uint32_t tw = (uint32_t)n1 + 1;
  uint32_t cur = 0, last = 1;
  auto E = [&](uint32_t sel, int i, int k) -> int & { return (int &)mid[((uint64_t)sel * W + (uint32_t)i) * 3 + k]; };
  E(cur, 0, 0) = 0; E(cur, 0, 1) = NEG_INF; E(cur, 0, 2) = NEG_INF;
  for (int i = 1; i < b1; ++i) {
    E(cur, i, 0) = NEG_INF; E(cur, i, 1) = NEG_INF; E(cur, i, 2) = -Q - i * RE;
    T[i] = (uint8_t)((i == 1 ? FM : FD) << 4);
  }
  { const uint32_t t = cur; cur = last; last = t; }
  const bool part2_last = b2 == 1 && n2 >= 2;
  for (int j = 1; j <= n2; ++j) {
    const int lo = j <= b2 ? 0 : j - b2;
    const int hi = j + b1 - 1 < n1 ? j + b1 - 1 : n1;
    const bool clipped = j + b1 - 1 > n1;
    const int rd = (j == n2 && !part2_last) ? RE : R;
    const int *srow = P.mat + (int)b[j - 1] * P.row;
    const uint64_t trow = (uint64_t)j * tw;
    int dm = E(last, lo, 0), di = E(last, lo, 1), dd = E(last, lo, 2);  // (j-1, i-1)
    int lm, ld;                                                          // (j, i-1)
    if (lo == 0) {
      const int x = dm - Q;
      const bool c = x > di;
      E(cur, 0, 0) = NEG_INF; E(cur, 0, 1) = (c ? x : di) - RE; E(cur, 0, 2) = NEG_INF;
      T[trow] = (uint8_t)((c ? FM : FI) << 2);
    } else {
      E(cur, lo, 0) = NEG_INF; E(cur, lo, 1) = NEG_INF; E(cur, lo, 2) = NEG_INF;
    }
    lm = ld = NEG_INF;
    for (int i = lo + 1; i <= hi; ++i) {
      const int sc = srow[a[i - 1]];
      int m, iv, dv, tm, ti, td;
      if (dm >= di) {
        if (dm >= dd) { m = dm + sc; tm = FM; } else { m = dd + sc; tm = FD; }
      } else {
        if (di > dd) { m = di + sc; tm = FI; } else { m = dd + sc; tm = FD; }
      }
      const bool inner = i < hi;
      if (inner || clipped) {
        const int um = E(last, i, 0), ui = E(last, i, 1), ud = E(last, i, 2);
        const int x = um - Q;
        const bool c = x > ui;
        iv = (c ? x : ui) - (inner ? R : RE);
        ti = c ? FM : FI;
        dm = um; di = ui; dd = ud;
      } else {
        iv = NEG_INF;
        ti = FM;
      }
      const int y = lm - Q;
      const bool cd = y > ld;
      dv = (cd ? y : ld) - rd;
      td = cd ? FM : FD;
      E(cur, i, 0) = m; E(cur, i, 1) = iv; E(cur, i, 2) = dv;
      T[trow + (uint32_t)i] = (uint8_t)(tm | ti << 2 | td << 4);
      lm = m; ld = dv;
    }
    { const uint32_t t = cur; cur = last; last = t; }
  }
  // backtrace from (n1, n2) (stdaln.c:487-514)
  const int fm = E(last, n1, 0), fi = E(last, n1, 1), fd = E(last, n1, 2);
  int best = fm, ctype = FM;
  uint8_t cell = T[(uint64_t)n2 * tw + (uint32_t)n1];
  int type = cell & 3;
  if (fi > best) { best = fi; type = (cell >> 2) & 3; ctype = FI; }
  if (fd > best) { best = fd; type = (cell >> 4) & 3; ctype = FD; }
  int i = n1, j = n2, n = 1;
  n_cig = 0;
  auto emit = [&](int op) {
    if (n_cig > 0 && (int)(cig[n_cig - 1] & 0xf) == op) cig[n_cig - 1] += 1u << 4;
    else if (n_cig < cap) cig[n_cig++] = 1u << 4 | (uint32_t)op;
  };
  int pi = i, pj = j;
  emit(ctype);
  for (;;) {
    if (ctype == FM) { --i; --j; } else if (ctype == FI) --j; else --i;
    ctype = type;
    if (i == 0 && j == 0) break;  // the (0,0) entry is not part of path_len
    if (i < 0 || j < 0) break;    // memory guard: a valid traceback never leaves the matrix
    cell = T[(uint64_t)j * tw + (uint32_t)i];
    type = ctype == FM ? (cell & 3) : ctype == FI ? ((cell >> 2) & 3) : ((cell >> 4) & 3);
    emit(ctype);
    ++n;
    pi = i;
    pj = j;
  }
  path_len = n;
  si = pi;
  sj = pj;
  return best;
}

// The most symbols of a sequence of length `len` that a local hit's region can cover.  The region is
// a path from the reverse pass's start cell to the forward pass's end cell whose score, plus the
// q + r the reverse pass seeds its first cell with, is positive: its m <= S = min(len1, len2) aligned
// pairs earn at most m * max_score and each of its g gap symbols costs at least r, so
// g * r < S * max_score + q + r and the region covers at most S + g symbols.
STD_HD uint64_t local_span(uint64_t len, uint64_t S, const Param &P) {
  const uint64_t w = S + (S * (uint64_t)P.max_score + (uint64_t)(P.q + P.r)) / (uint64_t)P.r + 1;
  return len < w ? len : w;
}

struct LocalOut {
  int score, subo, path_len, n_cig, s_i, s_j, e_i, e_j;
};

// The forward pass (stdaln.c:579-631): row j over seq2, cell i over seq1, the first maximum in
// row-major order.  KEEP: suba[j] = the row's largest h.  Otherwise (the second run of a pair whose
// suba row is not kept) the largest h of the rows j <= t1 and j >= t2 is returned in `best`.
template <bool KEEP, class EH, class SUBA>
STD_HD void forward_pass(const EH &eh, const SUBA &suba, const Param &P, const uint8_t *a, int n1, const uint8_t *b, int n2,
                         int t1, int t2, int &score_f, int &end_i, int &end_j, int &best) {
  const int q = P.q, r = P.r, qr = q + r, qr_shift = (qr + 1) << 16;
  for (int i = 0; i <= n1; ++i) eh[i] = 0;
  score_f = end_i = end_j = best = 0;
  if (KEEP) suba[0] = 0;
  for (int j = 1; j <= n2; ++j) {
    int subo = 0, last_h = 0, f = 0;
    const int *srow = P.mat + (int)b[j - 1] * P.row;
    int s_cur = (int)eh[0];
    for (int i = 1; i <= n1; ++i) {
      const int s_nxt = (int)eh[i];
      int curr_h = (s_cur >> 16) + srow[a[i - 1]];
      if (curr_h < 0) curr_h = 0;
      if (last_h > 0) {
        f = (f > last_h - q) ? f - r : last_h - qr;
        if (curr_h < f) curr_h = f;
      }
      if (s_nxt >= qr_shift) {
        const int curr_last_h = s_nxt >> 16, e_old = s_cur & 0xffff;
        const int e = (e_old > curr_last_h - q) ? e_old - r : curr_last_h - qr;
        if (curr_h < e) curr_h = e;
        eh[i - 1] = (uint32_t)(last_h << 16 | e);
      } else {
        eh[i - 1] = (uint32_t)(last_h << 16);
      }
      last_h = curr_h;
      if (subo < curr_h) subo = curr_h;
      if (score_f < curr_h) { score_f = curr_h; end_i = i; end_j = j; }
      s_cur = s_nxt;
    }
    eh[n1] = (uint32_t)(last_h << 16);
    if (KEEP) suba[j] = (uint16_t)subo;
    else if ((j <= t1 || j >= t2) && best < subo) best = subo;
  }
}

// aln_local_core with _thres = thres > 0 and _subo.  eh: n1 + 2 words (h << 16 | e, as the
// reference packs them).  keep_suba: suba holds n2 + 1 entries of 16 bits (the host refuses max_score
// * min(len1, len2) > 32000, so every h fits and the reference's rebasing is unreachable), one per
// row of seq2; otherwise nothing is kept per row and the forward pass runs a second time, once the
// reverse pass has fixed the two bounds, for the rows outside them.  W / fill_cells: the widest row
// and the cells the path fill may use.
template <class EH, class SUBA, class MID, class TB>
STD_HD void local_core(const EH &eh, const SUBA &suba, bool keep_suba, const MID &mid, uint32_t W, const TB &T,
                       uint64_t fill_cells, const Param &P, int thres, const uint8_t *a, int n1, const uint8_t *b, int n2,
                       uint32_t *cig, int cap, LocalOut &o) {
  o.score = -1;
  o.subo = o.path_len = o.n_cig = o.s_i = o.s_j = o.e_i = o.e_j = 0;
  if (n1 == 0 || n2 == 0) return;
  const int q = P.q, r = P.r, qr = q + r;
  int score_f = 0, end_i = 0, end_j = 0, unused = 0;
  if (keep_suba) forward_pass<true>(eh, suba, P, a, n1, b, n2, 0, 0, score_f, end_i, end_j, unused);
  else forward_pass<false>(eh, suba, P, a, n1, b, n2, 0, n2 + 1, score_f, end_i, end_j, unused);
  o.score = score_f;
  if (score_f < thres || end_i == 0 || end_j == 0) return;
  // ---- reverse pass in the adaptive band (stdaln.c:639-696)
  for (int i = end_i; i >= 0; --i) eh[i] = 0;
  int score_r = P.mat[(int)a[end_i - 1] * P.row + (int)b[end_j - 1]];
  int start_i = end_i, start_j = end_j;
  eh[end_i] = (uint32_t)((qr + score_r) * 65536);
  int start = end_i - 1, end = end_i - 3;
  if (end <= 0) end = 0;
  for (int j = end_j - 1; j != 0; --j) {
    int last_h = 0, f = 0;
    const int *srow = P.mat + (int)b[j - 1] * P.row;
    int i = start;
    bool found = false;
    // the reference's loop runs while i != end; start > end holds wherever it stays inside eh
    for (; i > end; --i) {
      const int sv = (int)eh[i + 1];
      int curr_h = (sv >> 16) + srow[a[i - 1]];
      if (curr_h < 0) curr_h = 0;
      if (last_h > 0) {
        f = (f > last_h - q) ? f - r : last_h - qr;
        if (curr_h < f) curr_h = f;
      }
      const int curr_last_h = (int)eh[i] >> 16, e_old = sv & 0xffff;
      int e = (e_old > curr_last_h - q) ? e_old - r : curr_last_h - qr;
      if (e < 0) e = 0;
      if (curr_h < e) curr_h = e;
      eh[i + 1] = (uint32_t)(last_h << 16 | e);
      last_h = curr_h;
      if (score_r < curr_h) {
        score_r = curr_h; start_i = i; start_j = j;
        if (score_r - qr == score_f) { found = true; break; }
      }
    }
    eh[i + 1] = (uint32_t)(last_h << 16);
    if (found) break;
    if (((int)eh[start] >> 16) <= qr) --start;
    if (start <= 0) start = 0;
    end = start_i - (start_j - j) - (score_r + (start_j - j) * P.max_score) / r - 1;
    if (end <= 0) end = 0;
  }
  // ---- the suboptimal score (stdaln.c:698-706)
  {
    const int t1 = subo_bound(start_j, end_j - start_j, true), t2 = subo_bound(end_j, end_j - start_j, false);
    int best = 0;
    if (keep_suba) {
      for (int j = 1; j <= t1; ++j) { const int v = suba[j]; if (best < v) best = v; }
      for (int j = t2; j <= n2; ++j) { const int v = suba[j]; if (best < v) best = v; }
    } else {
      int sf, ei, ej;
      forward_pass<false>(eh, suba, P, a, n1, b, n2, t1, t2, sf, ei, ej, best);
    }
    o.subo = best;
  }
  score_r -= qr;
  // ---- path by banded global alignment, the band doubling from band_width (stdaln.c:723-745)
  const int n1s = end_i - start_i + 1, n2s = end_j - start_j + 1;
  // memory guard: the host sizes W, fill_cells and cap for local_span(), the longest region a path
  // from the start to the end cell can cover
  if (n1s < 1 || n2s < 1 || (uint32_t)n1s + 1 > W || (uint64_t)(n1s + 1) * (uint64_t)(n2s + 1) > fill_cells || n1s + n2s > cap) {
    o.score = REFUSED;
    return;
  }
  const int span = (n1s > n2s ? n1s : n2s);  // max(end - start) + 1
  int score_g = 0, si = 0, sj = 0;
  for (int bw = P.band;; bw <<= 1) {
    score_g = global_core(mid, W, T, P, a + start_i - 1, n1s, b + start_j - 1, n2s, bw, -1, cig, cap, o.n_cig,
                          o.path_len, si, sj);
    if (score_g == score_r || score_f == score_g) break;
    if (bw > span || bw <= 0) break;
  }
  o.score = (score_r > score_g && score_f > score_g) ? -1 : score_g;
  for (int k = 0; k < o.n_cig / 2; ++k) {
    const uint32_t t = cig[k];
    cig[k] = cig[o.n_cig - 1 - k];
    cig[o.n_cig - 1 - k] = t;
  }
  o.s_i = si + start_i - 1; o.s_j = sj + start_j - 1;
  o.e_i = n1s + start_i - 1; o.e_j = n2s + start_j - 1;
}

// ---- aln_extend_core (stdaln.c:862-1008)
constexpr int EXT_OVERFLOW = 32000, EXT_REDUCE = 16000;  // LOCAL_OVERFLOW_THRESHOLD / _REDUCE

// the band a pair runs with: band_width <= 0 is len1 + len2, and nothing wider than that changes a
// row (start stays 1, end is clipped at len1 + 1), so j + band cannot wrap
STD_HD int extend_band(int band_width, int n1, int n2) {
  return (band_width <= 0 || band_width > n1 + n2) ? n1 + n2 : band_width;
}

// words of the eh ring.  A row reads the cells start .. end, start >= j - band and end <= j + band,
// and start never decreases: a ring of 2 * band + 2 words holds every cell that is read again
// (cell i shares its word with i - R < start and i + R > the highest cell touched so far); len1 + 2
// words is the reference's whole array and never wraps.
STD_HD uint32_t extend_ring(int band, int n1) {
  const uint64_t w = 2ull * (uint32_t)band + 2;
  return (uint32_t)(w < (uint64_t)n1 + 2 ? w : (uint64_t)n1 + 2);
}

// the rows of seq1 / seq2 the best cell can lie in: a cell (j, i) of the band has i <= j + band - 1
// and j <= i + band
STD_HD uint64_t extend_span1(int band, int n1, int n2) {
  const uint64_t w = (uint64_t)n2 + (uint32_t)band - 1;
  return w < (uint64_t)n1 ? w : (uint64_t)n1;
}
STD_HD uint64_t extend_span2(int band, int n1, int n2) {
  const uint64_t w = (uint64_t)n1 + (uint32_t)band;
  return w < (uint64_t)n2 ? w : (uint64_t)n2;
}

// The extension pass (stdaln.c:901-973): row j over seq2, cell i over seq1, eh[i] = h[j-1,i-1] << 16 |
// e[j,i] in a ring of R words (extend_ring, or len1 + 2 for the whole array), eh[1] = G0 << 16.  A
// cell that enters the window for the first time is zeroed there (the reference's memset), so the
// ring needs no clearing.  band: extend_band().  Returns score + of_base - 1.
template <class EH>
STD_HD int extend_fill(const EH &eh, uint32_t R, const Param &P, int band, const uint8_t *a, int n1, const uint8_t *b, int n2,
                       int G0, int &end_i, int &end_j) {
  const int r = P.r, qr = P.q + P.r;
  int start = 1, end = 2, score = 0, of_base = 0;
  bool is_overflow = false;
  end_i = end_j = 0;
  eh[1] = (uint32_t)G0 << 16;  // R >= 3
  eh[2] = 0;
  int hw = 2;        // the highest cell initialised
  uint32_t hwk = 2;  // ... and its word
  for (int j = 1; j <= n2; ++j) {
    int h1 = 0, f = 0;
    const int *srow = P.mat + (int)b[j - 1] * P.row;
    int s0 = j - band, e0 = j + band;
    if (s0 < 1) s0 = 1;
    if (s0 > start) start = s0;
    if (e0 > n1 + 1) e0 = n1 + 1;
    if (e0 < end) end = e0;
    if (start >= end) break;  // ==: the reference's break; >: its row is empty, which ends it as well
    while (hw < end) {
      ++hw;
      if (++hwk == R) hwk = 0;
      eh[hwk] = 0;
    }
    const uint32_t k0 = (uint32_t)start % R;
    if (is_overflow) {  // stdaln.c:917-930, cells below the reduction clamp to zero
      score -= EXT_REDUCE;
      of_base += EXT_REDUCE;
      is_overflow = false;
      uint32_t k = k0;
      for (int i = start; i <= end; ++i) {
        const uint32_t sv = eh[k];
        int hh = (int)(sv >> 16), ee = (int)(sv & 0xffff);
        ee = ee < EXT_REDUCE ? 0 : ee - EXT_REDUCE;
        hh = hh < EXT_REDUCE ? 0 : hh - EXT_REDUCE;
        eh[k] = (uint32_t)hh << 16 | (uint32_t)ee;
        if (++k == R) k = 0;
      }
    }
    int first = 0, lastp = 0;
    uint32_t k = k0;
    for (int i = start; i < end; ++i) {
      const uint32_t sv = eh[k];
      int h = (int)(sv >> 16), e = (int)(sv & 0xffff);
      const uint32_t nv = (uint32_t)h1 << 16;
      h += h ? srow[a[i - 1]] : 0;  // a zero diagonal never restarts
      h = h > e ? h : e;
      h = h > f ? h : f;
      h1 = h;
      if (h > 0) {
        if (first == 0) first = i;
        lastp = i;
        if (score < h) {
          score = h; end_i = i; end_j = j;
          if (score > EXT_OVERFLOW) is_overflow = true;
        }
      }
      h -= qr;
      h = h > 0 ? h : 0;
      e -= r;
      e = e > h ? e : h;
      f -= r;
      f = f > h ? f : h;
      eh[k] = nv | (uint32_t)e;
      if (++k == R) k = 0;
    }
    eh[k] = (uint32_t)h1 << 16;  // cell `end`
    if (lastp <= 0) break;       // no positive cell in this row
    start = first;
    end = lastp + 3;
  }
  return score + of_base - 1;
}

struct ExtOut {
  int score, end_i, end_j, path_len, n_cig, s_i, s_j, no_band;
};

// aln_extend_core.  mode 0: the score alone; 1: the end cell (path != 0, path_len == 0); 2: the path, by
// global alignment of seq1[0, end_i) with seq2[0, end_j), gap_end -1, the band doubling from band_width
// until the global score equals the extension score or the band passes max(end_i, end_j).  The score
// returned is then the global one, which leaves G0 out: for G0 > 1 the two never meet, the band runs
// to the end and no_band is set where the reference prints "no suitable bandwidth".  P.band:
// extend_band().  W / fill_cells / cap: the widest (M, I, D) row, the traceback cells and the CIGAR
// words the caller has, sized by extend_span1 / extend_span2.
template <class EH, class MID, class TB>
STD_HD void extend_core(const EH &eh, uint32_t R, const MID &mid, uint32_t W, const TB &T, uint64_t fill_cells, const Param &P,
                        int mode, int G0, const uint8_t *a, int n1, const uint8_t *b, int n2, uint32_t *cig, int cap,
                        ExtOut &o) {
  o.score = -1;
  o.end_i = o.end_j = o.path_len = o.n_cig = o.s_i = o.s_j = o.no_band = 0;
  if (n1 == 0 || n2 == 0) return;
  int end_i = 0, end_j = 0;
  const int score = extend_fill(eh, R, P, P.band, a, n1, b, n2, G0, end_i, end_j);
  o.score = score;
  if (score <= 0 || mode == 0) return;
  o.end_i = end_i; o.end_j = end_j;
  if (mode == 1) return;
  // memory guard: the host sizes W, fill_cells and cap for the band's reach
  if ((uint32_t)end_i + 1 > W || (uint64_t)(end_i + 1) * (uint64_t)(end_j + 1) > fill_cells || end_i + end_j > cap) {
    o.score = REFUSED;
    return;
  }
  const int jmax = end_i > end_j ? end_i : end_j;
  int score_g = 0;
  for (int bw = P.band;; bw <<= 1) {
    score_g = global_core(mid, W, T, P, a, end_i, b, end_j, bw, -1, cig, cap, o.n_cig, o.path_len, o.s_i, o.s_j);
    if (score == score_g) break;
    if (bw > jmax) break;
  }
  if (score > score_g) o.no_band = 1;
  o.score = score_g;
  for (int k = 0; k < o.n_cig / 2; ++k) {
    const uint32_t t = cig[k];
    cig[k] = cig[o.n_cig - 1 - k];
    cig[o.n_cig - 1 - k] = t;
  }
}

}  // namespace stdaln
}  // namespace ibwa
