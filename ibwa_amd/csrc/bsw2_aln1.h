// bsw2_aln1.h -- bwasw from seeds to hits on the host: a sequential restatement of bsw2_aln1_core
// (bwtsw2_aux.c:252-276) and what it calls: bsw2_chain_filter (bwtsw2_chain.c), bsw2_extend_left and
// bsw2_extend_rght (bwtsw2_aux.c:80-164), merge_hits (:230-250), bsw2_resolve_duphits without an index
// (finish_duphits of bsw2_core.h) and bsw2_resolve_query_overlaps (bwtsw2_core.c:329-378).  Plain
// C++17, no HIP: it is the executable specification of k_bsw2_extend (bsw2_extend.hip) and of the host
// stages of ibwa_bsw2_aln1_batch, which calls these very functions.  tests/host/bsw2_aln1_check.cpp
// runs it over the golden vectors and classifies them.
//
// The target bases come through a two-function interface (template parameter Ref):
//   uint32_t l_pac() const;
//   uint32_t base(uint32_t i) const;   // base i of the forward sequence, i < l_pac()
// With is_rev the reference reads base i of the reversed sequence, __rpac: base(l_pac - i - 1).
//
// Kept as the reference has them: klib's unstable introsort wherever it sorts (by qbeg twice in the
// chain filter, by end in the left extension, by G in both resolve passes), the greedy chaining and its
// flag array indexed by chain number, the containment test on the earlier hits' current coordinates
// with uint32_t sums, the int / uint32_t comparison lt > k, base 0 never taken on the left (the
// reference's FIXME), > on the left and >= on the right, float for fol and mask_level, double for the
// tol ratios.  The draw of bsw2_resolve_query_overlaps is an argument u in [0, 1): the restatement owns
// no random stream.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "bsw2_core.h"
#include "stdaln_core.h"

namespace ibwa_bsw2 {

struct AlnHit {  // bsw2hit_t with flag and n_seeds as words (== ibwa_bsw2_aln_hit_t)
  uint32_t k, l, flag, n_seeds;
  int32_t len, G, G2, beg, end;
};

struct AlnOpt {  // one read's options: seed.t and seed.bw already derived from its length
  Opt seed;
  int t_seeds;
  float mask_level;
};

constexpr uint32_t kMaxSeeds = (1u << 14) - 2;  // where ++n_seeds stops (bwtsw2_aux.c:106)
constexpr int kWindow = 64;                     // hits per window of k_bsw2_extend (classification only)

inline AlnHit to_aln_hit(const Hit &h) { return AlnHit{h.k, h.l, h.flag, 0, h.len, h.G, h.G2, h.beg, h.end}; }

// what the golden vectors are classified by (see tools/make_bwasw_hits_golden.py)
struct AlnCounters {
  // left, per hit
  int64_t extended = 0, not_extensible = 0, contained_orig = 0, contained_ext_only = 0, contained_same_window = 0,
          contained_earlier_window = 0, k_zero = 0, lt_clipped = 0, beg_zero = 0, equal_end = 0;
  int64_t max_n_seeds = 0, dp_runs = 0;
  // chain filter
  int64_t chain_lost = 0, chain_other_strand = 0;
  // right
  int64_t right_clipped = 0, right_equal = 0, right_kept = 0, right_raised = 0;
  // query overlaps
  int64_t tie_j = 0, zeroed = 0, g2_raised = 0;
};

// ---- bsw2_chain_filter (bwtsw2_chain.c) ----
namespace detail {

struct Hsaip {  // hsaip_t
  uint32_t tbeg, tend;
  int qbeg, qend;
  uint32_t flag, idx;
  int chain;
};

inline int chaining(int bw, int shift, int n, Hsaip *z, Hsaip *chain) {
  int m = 0;
  ibwa_sam::ks_introsort((size_t)n, z, [](const Hsaip &a, const Hsaip &b) { return a.qbeg < b.qbeg; });
  for (int j = 0; j < n; ++j) {
    Hsaip *p = z + j;
    int k;
    for (k = m - 1; k >= 0; --k) {
      Hsaip *q = chain + k;
      const int x = p->qbeg - q->qbeg;
      const int y = (int)(p->tbeg - q->tbeg);
      if (y > 0 && x - y <= bw && y - x <= bw) {
        if (p->qend > q->qend) q->qend = p->qend;
        if (p->tend > q->tend) q->tend = p->tend;
        ++q->chain;
        p->chain = shift + k;
        break;
      }
    }
    if (k < 0) {
      chain[m] = *p;
      chain[m].chain = 1;
      chain[m].idx = (uint32_t)(p->chain = shift + m);
      ++m;
    }
  }
  return m;
}

}  // namespace detail

// b[0], b[1]: the narrow lists of the read and of its reverse complement, len the read's length
inline void chain_filter(const AlnOpt &opt, int len, std::vector<AlnHit> b[2], AlnCounters *ct = nullptr) {
  using detail::Hsaip;
  const int n[2] = {(int)b[0].size(), (int)b[1].size()};
  if (n[0] + n[1] == 0) return;
  std::vector<Hsaip> zbuf((size_t)n[0] + n[1]), cbuf((size_t)n[0] + n[1]);
  Hsaip *z[2] = {zbuf.data(), zbuf.data() + n[0]}, *chain[2] = {cbuf.data(), nullptr};
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < n[k]; ++i) {
      const AlnHit &p = b[k][i];
      Hsaip *q = z[k] + i;
      q->flag = (uint32_t)k;
      q->idx = (uint32_t)i;
      q->tbeg = p.k;
      q->tend = p.k + (uint32_t)p.len;
      q->chain = -1;
      q->qbeg = p.beg;
      q->qend = p.end;
    }
  int m[2];
  m[0] = detail::chaining(opt.seed.bw, 0, n[0], z[0], chain[0]);
  chain[1] = chain[0] + m[0];
  m[1] = detail::chaining(opt.seed.bw, m[0], n[1], z[1], chain[1]);
  for (int k = 0; k < m[1]; ++k) {  // the reverse strand's chains in forward query coordinates
    Hsaip *p = chain[1] + k;
    const int tmp = p->qbeg;
    p->qbeg = len - p->qend;
    p->qend = len - tmp;
  }
  std::vector<char> flag((size_t)m[0] + m[1], 0);
  ibwa_sam::ks_introsort((size_t)(m[0] + m[1]), chain[0], [](const Hsaip &a, const Hsaip &b) { return a.qbeg < b.qbeg; });
  bool other = false;
  for (int k = 1; k < m[0] + m[1]; ++k) {
    const Hsaip *p = chain[0] + k;
    for (int j = 0; j < k; ++j) {
      const Hsaip *q = chain[0] + j;
      if (flag[q->idx]) continue;
      if (q->qend >= p->qend && q->chain > p->chain * opt.t_seeds * 2) {
        flag[p->idx] = 1;
        if (q->flag != p->flag) other = true;
        break;
      }
    }
  }
  for (int k = 0; k < n[0] + n[1]; ++k) {
    const Hsaip *p = z[0] + k;
    if (flag[p->chain]) b[p->flag][p->idx].G = 0;
  }
  int lost = 0;
  for (int k = 0; k < 2; ++k) {
    size_t i = 0;
    for (size_t j = 0; j < b[k].size(); ++j)
      if (b[k][j].G) b[k][i++] = b[k][j];
    lost += (int)(b[k].size() - i);
    b[k].resize(i);
  }
  if (ct) {
    ct->chain_lost += lost;
    ct->chain_other_strand += other;
  }
}

// ---- the extensions ----

// the 5 x 5 matrix of __gen_ap (bwtsw2_aux.c:69-76)
inline void gen_matrix(const Opt &o, int mat[25]) {
  for (int i = 0; i < 25; ++i) mat[i] = -o.b;
  for (int i = 0; i < 4; ++i) mat[i * 5 + i] = o.a;
}

// the sort bsw2_extend_left starts with (:91): by end, descending, unstable
inline void sort_for_left(std::vector<AlnHit> &b) {
  ibwa_sam::ks_introsort(b.size(), b.data(), [](const AlnHit &x, const AlnHit &y) { return x.end > y.end; });
}

// aln_extend_core in end-cell mode (path != 0, path_len == 0): the score; end_i / end_j where it is > 0
inline int extend_end(const Opt &o, const int *mat, const uint8_t *target, int lt, const uint8_t *query, int lq, int G0,
                      std::vector<uint32_t> &eh, int &end_i, int &end_j) {
  using namespace ibwa::stdaln;
  Param P = {o.q, o.r, o.r, extend_band(o.bw, lt, lq), 5, o.a, mat};
  const uint32_t R = extend_ring(P.band, lt);
  if (eh.size() < R) eh.resize(R);
  ExtOut x;
  extend_core(View<uint32_t>{eh.data(), 1}, R, View<uint32_t>{nullptr, 1}, 0, TbView{nullptr, 1, 0}, 0, P, 1, G0, target, lt, query, lq,
              nullptr, 0, x);
  end_i = x.end_i;
  end_j = x.end_j;
  return x.score;
}

// bsw2_extend_left (bwtsw2_aux.c:80-129).  query: the strand's sequence as given, lq bases.
template <class Ref>
inline void extend_left(const Opt &o, std::vector<AlnHit> &b, const uint8_t *query_, int lq, const Ref &ref, int is_rev,
                        AlnCounters *ct = nullptr) {
  int mat[25];
  gen_matrix(o, mat);
  sort_for_left(b);
  if (b.empty()) return;
  std::vector<uint8_t> query((size_t)lq), target((size_t)(((lq + 1) / 2 * o.a + o.r) / o.r + lq));
  for (int i = 0; i < lq; ++i) query[lq - i - 1] = query_[i];
  std::vector<uint32_t> eh;
  std::vector<AlnHit> orig;
  if (ct) orig = b;
  const uint32_t l_pac = ref.l_pac();
  const int bn = (int)b.size();
  for (int i = 0; i < bn; ++i) {
    AlnHit *p = &b[i];
    int lt = ((p->beg + 1) / 2 * o.a + o.r) / o.r + lq;
    int score = 0, j;
    p->n_seeds = 1;
    if (ct && i > 0 && b[i - 1].end == p->end) ++ct->equal_end;
    if (ct && p->l == 0 && p->k == 0) ++ct->k_zero;
    if (p->l || p->k == 0) continue;
    bool by_orig = false, same_w = false, earlier_w = false;
    for (j = 0; j < i; ++j) {
      AlnHit *q = &b[j];
      if (q->beg <= p->beg && q->k <= p->k && q->k + (uint32_t)q->len >= p->k + (uint32_t)p->len) {
        if (q->n_seeds < kMaxSeeds) ++q->n_seeds;
        ++score;
        if (ct) {
          const AlnHit &q0 = orig[j];
          if (q0.beg <= p->beg && q0.k <= p->k && q0.k + (uint32_t)q0.len >= p->k + (uint32_t)p->len) by_orig = true;
          if (j / kWindow == i / kWindow) same_w = true;
          else earlier_w = true;
        }
      }
    }
    if (score) {
      if (ct) {
        ++(by_orig ? ct->contained_orig : ct->contained_ext_only);
        ct->contained_same_window += same_w;
        ct->contained_earlier_window += earlier_w;
      }
      continue;
    }
    if ((uint32_t)lt > p->k) {  // int against uint32_t, as in the reference
      lt = (int)p->k;
      if (ct) ++ct->lt_clipped;
    }
    uint32_t k;
    for (k = p->k - 1, j = 0; k > 0 && j < lt; --k)  // base 0 is never taken
      target[j++] = (uint8_t)(is_rev ? ref.base(l_pac - k - 1) : ref.base(k));
    lt = j;
    if (ct) {
      ++ct->dp_runs;
      if (p->beg == 0) ++ct->beg_zero;
    }
    int ei = 0, ej = 0;
    score = extend_end(o, mat, target.data(), lt, query.data() + lq - p->beg, p->beg, p->G, eh, ei, ej);
    if (score > p->G) {
      p->G = score;
      p->len += ei;
      p->beg -= ej;
      p->k -= (uint32_t)ei;
      if (ct) ++ct->extended;
    } else if (ct) ++ct->not_extensible;
  }
  if (ct)
    for (const AlnHit &h : b)
      if ((int64_t)h.n_seeds > ct->max_n_seeds) ct->max_n_seeds = h.n_seeds;
}

// merge_hits (bwtsw2_aux.c:230-250): b1 behind b0; is_reverse flips b1's query coordinates
inline void merge(std::vector<AlnHit> &b0, const std::vector<AlnHit> &b1, int l, int is_reverse) {
  for (AlnHit p : b1) {
    if (is_reverse) {
      const int x = p.beg;
      p.beg = l - p.end;
      p.end = l - x;
      p.flag |= 0x10;
    }
    b0.push_back(p);
  }
}

// bsw2_resolve_duphits(0, b, 0)
inline void resolve_duphits_noindex(std::vector<AlnHit> &b) {
  if (b.empty()) return;
  std::vector<AlnHit> out;
  finish_duphits(b, out);
  b.swap(out);
}

// bsw2_extend_rght (bwtsw2_aux.c:131-164).  query: the strand's sequence, lq bases.
template <class Ref>
inline void extend_right(const Opt &o, std::vector<AlnHit> &b, const uint8_t *query, int lq, const Ref &ref, int is_rev,
                         AlnCounters *ct = nullptr) {
  int mat[25];
  gen_matrix(o, mat);
  if (b.empty()) return;
  std::vector<uint8_t> target((size_t)(((lq + 1) / 2 * o.a + o.r) / o.r + lq));
  std::vector<uint32_t> eh;
  const uint32_t l_pac = ref.l_pac();
  for (AlnHit &h : b) {
    AlnHit *p = &h;
    int lt = ((lq - p->beg + 1) / 2 * o.a + o.r) / o.r + lq;
    if (p->l) continue;
    int j = 0;
    uint32_t k;
    for (k = p->k; k < p->k + (uint32_t)lt && k < l_pac; ++k) target[j++] = (uint8_t)(is_rev ? ref.base(l_pac - k - 1) : ref.base(k));
    if (ct && j < lt) ++ct->right_clipped;
    lt = j;
    int ei = 0, ej = 0;
    const int score = extend_end(o, mat, target.data(), lt, query + p->beg, lq - p->beg, 1, eh, ei, ej);
    if (ct) ++(score == p->G ? ct->right_equal : score < p->G ? ct->right_kept : ct->right_raised);
    if (score >= p->G) {
      p->G = score;
      p->len = ei;
      p->end = ej + p->beg;
    }
  }
}

// bsw2_resolve_query_overlaps (bwtsw2_core.c:329-378); u stands for its drand48()
inline void resolve_query_overlaps(std::vector<AlnHit> &b, float mask_level, double u, AlnCounters *ct = nullptr) {
  const int bn = (int)b.size();
  if (bn == 0) return;
  ibwa_sam::ks_introsort(b.size(), b.data(), [](const AlnHit &x, const AlnHit &y) { return x.G > y.G; });
  int i, j;
  {
    const int G0 = b[0].G;
    for (i = 1; i < bn; ++i)
      if (b[i].G != G0) break;
    j = (int)(i * u);
    if (j) std::swap(b[0], b[j]);
    if (ct && i > 1 && j) ++ct->tie_j;
  }
  for (i = 1; i < bn; ++i) {
    AlnHit *p = &b[i];
    bool all_compatible = true;
    if (p->G == 0) break;
    for (j = 0; j < i; ++j) {
      AlnHit *q = &b[j];
      int64_t tol = 0;
      if (q->G == 0) continue;
      int qol = (p->end < q->end ? p->end : q->end) - (p->beg > q->beg ? p->beg : q->beg);
      if (qol < 0) qol = 0;
      if (p->l == 0 && q->l == 0) {
        const uint32_t pe = p->k + (uint32_t)p->len, qe = q->k + (uint32_t)q->len;
        tol = (int64_t)(pe < qe ? pe : qe) - (p->k > q->k ? p->k : q->k);
        if (tol < 0) tol = 0;
      }
      const float fol = (float)qol / (p->end - p->beg < q->end - q->beg ? p->end - p->beg : q->end - q->beg);
      const bool compatible = fol < mask_level || (tol > 0 && qol < p->end - p->beg && qol < q->end - q->beg);
      if (!compatible) {
        if (q->G2 < p->G) {
          q->G2 = p->G;
          if (ct) ++ct->g2_raised;
        }
        all_compatible = false;
      }
    }
    if (!all_compatible) {
      p->G = 0;
      if (ct) ++ct->zeroed;
    }
  }
  const int n = i;
  size_t w = 0;
  for (i = 0; i < n; ++i)
    if (b[i].G != 0) b[w++] = b[i];
  b.resize(w);
}

// ---- bsw2_aln1_core ----

// the reverse complement of codes 0-3
inline void revcomp(const uint8_t *s, int l, std::vector<uint8_t> &out) {
  out.resize((size_t)l);
  for (int i = 0; i < l; ++i) out[l - 1 - i] = (uint8_t)(3 - s[i]);
}

// From the four seed lists on: all[k] / narrow[k] of seq[k] as bsw2_core left them.  narrow_after_left
// (optional) receives the two narrow lists as they stand right after bsw2_extend_left.
template <class Ref>
inline void aln1_from_seeds(const AlnOpt &opt, int l, const uint8_t *const seq[2], std::vector<AlnHit> all[2],
                            std::vector<AlnHit> narrow[2], const Ref &ref, int is_rev, double u, std::vector<AlnHit> &out,
                            AlnCounters *ct = nullptr, std::vector<AlnHit> *narrow_after_left = nullptr) {
  chain_filter(opt, l, narrow, ct);
  for (int k = 0; k < 2; ++k) {
    extend_left(opt.seed, narrow[k], seq[k], l, ref, is_rev, ct);
    if (narrow_after_left) narrow_after_left[k] = narrow[k];
    merge(all[k], narrow[k], l, 0);
    resolve_duphits_noindex(all[k]);
    extend_right(opt.seed, all[k], seq[k], l, ref, is_rev, ct);
  }
  merge(all[0], all[1], l, 1);
  resolve_query_overlaps(all[0], opt.mask_level, u, ct);
  out.swap(all[0]);
}

// seq0: the read (for is_rev, reversed: bsw2_aln_core's rseq[0]); idx: the strand's index (bsw2_core.h)
template <class Idx, class Ref>
inline void aln1(const AlnOpt &opt, const uint8_t *seq0, int l, const Idx &idx, const Ref &ref, int is_rev, double u,
                 std::vector<AlnHit> &out, AlnCounters *ct = nullptr, std::vector<AlnHit> *narrow_after_left = nullptr) {
  std::vector<uint8_t> rc;
  revcomp(seq0, l, rc);
  const uint8_t *seq[2] = {seq0, rc.data()};
  std::vector<AlnHit> all[2], narrow[2];
  for (int k = 0; k < 2; ++k) {
    std::vector<Hit> a, n;
    seed_task(opt.seed, seq[k], l, idx, a, n);
    for (const Hit &h : a) all[k].push_back(to_aln_hit(h));
    for (const Hit &h : n) narrow[k].push_back(to_aln_hit(h));
  }
  aln1_from_seeds(opt, l, seq, all, narrow, ref, is_rev, u, out, ct, narrow_after_left);
}

}  // namespace ibwa_bsw2
