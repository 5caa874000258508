// bsw2_core.h -- bwasw's seeding on the host: a sequential restatement of bwtl_seq2bwtl
// (bwt_lite.c:9-54), bsw2_core (bwtsw2_core.c:429-594), bsw2_resolve_duphits (:261-327) and the
// per-length options of bsw2_aln_core (bwtsw2_aux.c:483-497).  Plain C++17, no HIP: it is the
// executable specification of k_bsw2_seed (seed.hip).  tests/host/bsw2_seed_check.cpp runs it over
// the golden vectors, tools/make_bwasw_golden.py classifies vectors with it, and it counts what
// sizes the kernel's per-task arena.
//
// The genome index comes through a small interface (template parameter Idx):
//   uint32_t seq_len, L2[5];
//   void occ4(uint32_t k, uint32_t cnt[4]) const;   // bwt_occ4 (bwt.c:157-174), k == (u32)-1 -> zeros
//   uint32_t sa(uint32_t k) const;                  // bwt_sa (bwt.c:69-79)
//
// Everything that makes the result depend on order is kept as the reference has it: the cell loop
// that visits the cells it appends, positions in u handed out in visit order, the z-best threshold
// including the current cell, cut_tail's tie rule, remove_duplicate's "first wins unless a later
// one is strictly better", the smaller array appended to the larger on a pending merge, the
// -1 / -3 / -5 marks of which only -1 lets a child be made again, save_hits' strict >, and klib's
// unstable introsort (ksort.h) in resolve_duphits.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "ksort.h"

namespace ibwa_bsw2 {

constexpr int kMinusInf = -0x3fffffff;
constexpr float kMaskLevel = 0.90f;

struct Opt {  // one task's options, t and bw already derived
  int a, b, q, r, t, bw, z, is;
};

struct Hit {  // bsw2hit_t without n_seeds (== ibwa_bsw2_hit_t)
  uint32_t k, l, flag;
  int32_t len, G, G2, beg, end;
};

// bwtsw2_aux.c:483-497: t from log(l) * coef, then the band width
inline void opt_for_len(int a, int q, int r, int t0, int bw0, float coef, uint32_t len, int *t, int *bw) {
  const int l = (int)len;
  int tt = t0;
  if (tt < log((double)l) * coef) tt = (int)(log((double)l) * coef + .499);
  int k = (l * a - 2 * q) / (2 * r + a);
  const int i = (l * a - a - tt) / r;
  if (k > i) k = i;
  if (k < 1) k = 1;
  *t = tt;
  *bw = bw0 < k ? bw0 : k;
}

// what sizes the device arena, and the events the golden vectors are classified by
struct Counters {
  int64_t peak_cells = 0, peak_pending = 0, max_array = 0, max_stack = 0, iters = 0, cells_visited = 0;
  int64_t narrow_raw = 0, dag_nodes = 0;
  int64_t n_swap = 0, n_dup = 0, n_tie_cut = 0, n_band_del = 0, n_recreate = 0, n_flag1 = 0, n_displaced = 0,
          n_narrow_tie = 0;
};

// ---- the read's BWT (bwt_lite.c) ----
struct Bwtl {
  uint32_t seq_len = 0, primary = 0, L2[5] = {0, 0, 0, 0, 0};
  std::vector<uint32_t> sa, bwt, occ;

  // suffix array of seq with the empty suffix first (what is_sa leaves): prefix doubling
  static void suffix_sort(int len, const uint8_t *seq, std::vector<uint32_t> &sa) {
    const int n = len + 1;
    std::vector<int> rk(n), tmp(n);
    sa.resize(n);
    for (int i = 0; i < n; ++i) {
      sa[i] = i;
      rk[i] = i < len ? seq[i] + 1 : 0;
    }
    for (int h = 1;; h <<= 1) {
      auto key2 = [&](int i) { return i + h < n ? rk[i + h] : -1; };
      std::sort(sa.begin(), sa.end(), [&](uint32_t x, uint32_t y) {
        return rk[x] != rk[y] ? rk[x] < rk[y] : key2(x) < key2(y);
      });
      tmp[sa[0]] = 0;
      for (int i = 1; i < n; ++i)
        tmp[sa[i]] = tmp[sa[i - 1]] + (rk[sa[i]] != rk[sa[i - 1]] || key2(sa[i]) != key2(sa[i - 1]));
      rk = tmp;
      if (rk[sa[n - 1]] == n - 1) break;
    }
  }

  void build(int len, const uint8_t *seq) {
    seq_len = len;
    suffix_sort(len, seq, sa);
    std::vector<uint8_t> s(len + 1, 0);
    for (int i = 0; i <= len; ++i) {
      if (sa[i] == 0) primary = i;
      else s[i] = seq[sa[i] - 1];
    }
    for (int i = primary; i < len; ++i) s[i] = s[i + 1];
    bwt.assign((len + 15) / 16, 0);
    for (int i = 0; i < len; ++i) bwt[i >> 4] |= (uint32_t)s[i] << ((15 - (i & 15)) << 1);
    occ.assign((len + 15) / 16 * 4, 0);
    uint32_t c[4] = {0, 0, 0, 0};
    for (int i = 0; i < len; ++i) {
      if (i % 16 == 0) memcpy(&occ[(i / 16) * 4], c, 16);
      ++c[bwt[i >> 4] >> ((~i & 15) << 1) & 3];
    }
    L2[0] = 0;
    for (int i = 0; i < 4; ++i) L2[i + 1] = L2[i] + c[i];
  }

  // bwtl_occ4 (bwt_lite.c:68-82): the counts over BWT[0..k], $ skipped
  void occ4(uint32_t k, uint32_t cnt[4]) const {
    if (k == (uint32_t)-1) {
      cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
      return;
    }
    if (k >= primary) --k;
    memcpy(cnt, &occ[k >> 4 << 2], 16);
    const uint32_t w = bwt[k >> 4];
    for (uint32_t j = 0; j <= (k & 15); ++j) ++cnt[w >> ((15 - j) << 1) & 3];
  }
};

// ---- bsw2_resolve_duphits with an index (bwtsw2_core.c:261-327) ----
// The second half (:295-326): the unstable sort by G, then every hit contained in a better one goes.
// b is the expanded array, one element per SA row, G == 0 for the rows of empty slots.
// H: Hit, or bsw2_aln1.h's AlnHit, which carries n_seeds.
template <class H>
inline void finish_duphits(std::vector<H> &b, std::vector<H> &out) {
  ibwa_sam::ks_introsort(b.size(), b.data(), [](const H &x, const H &y) { return x.G > y.G; });
  const int bn = (int)b.size();
  int i;
  for (i = 1; i < bn; ++i) {
    H *p = &b[i];
    if (p->G == 0) break;
    for (int j = 0; j < i; ++j) {
      const H *q = &b[j];
      bool compatible = true;
      if (q->G == 0) continue;
      if (p->l == 0 && q->l == 0) {
        int qol = (p->end < q->end ? p->end : q->end) - (p->beg > q->beg ? p->beg : q->beg);
        if (qol < 0) qol = 0;
        if ((float)qol / (p->end - p->beg) > kMaskLevel || (float)qol / (q->end - q->beg) > kMaskLevel) {
          const uint32_t pe = p->k + (uint32_t)p->len, qe = q->k + (uint32_t)q->len;
          const int64_t tol = (int64_t)(pe < qe ? pe : qe) - (int64_t)(p->k > q->k ? p->k : q->k);
          if ((double)tol / p->len > kMaskLevel || (double)tol / q->len > kMaskLevel) compatible = false;
        }
      }
      if (!compatible) {
        p->G = 0;
        break;
      }
    }
  }
  // with nothing to sort the reference reads the score of a hit it never allocated (:273-274,
  // :319-321); here an empty array gives an empty list
  const int n = bn < 1 ? 0 : (i < bn ? i : bn);
  out.clear();
  for (int x = 0; x < n; ++x)
    if (b[x].G != 0) out.push_back(b[x]);
}

template <class Idx>
inline void resolve_duphits(const Idx &idx, std::vector<Hit> &hits, int IS, Counters *ct = nullptr, bool narrow = false) {
  if (hits.empty()) return;
  std::vector<Hit> b;
  for (const Hit &p : hits) {  // :268-292
    if (p.l - p.k + 1 <= (uint32_t)IS) {  // int converted to unsigned, as in the reference's comparison
      for (uint32_t k = p.k; k <= p.l; ++k) {
        Hit h = p;
        h.k = idx.sa(k);
        h.l = 0;
        b.push_back(h);
        if (k == 0xffffffffu) break;
      }
    } else if (p.G > 0) {
      Hit h = p;
      h.k = idx.sa(p.k);
      h.l = 0;
      h.flag |= 1;
      b.push_back(h);
    }
  }
  if (ct && narrow) {
    std::vector<int> g;
    for (const Hit &h : b) g.push_back(h.G);
    std::sort(g.begin(), g.end());
    if (std::adjacent_find(g.begin(), g.end()) != g.end()) ++ct->n_narrow_tie;
  }
  finish_duphits(b, hits);
  if (ct)
    for (const Hit &h : hits) ct->n_flag1 += h.flag & 1;
}

// ---- bsw2_core ----
struct Cell {  // bsw2cell_t
  uint32_t qk, ql;
  int I, D, G;
  uint32_t pj, qlen;
  int tlen, ppos, upos;
  int cpos[4];
  uint8_t cut;  // restatement only: bit j set when cut_tail wrote -1 into cpos[j] (classifies vectors)
};

struct Entry {  // bsw2entry_t
  uint32_t tk = 0, tl = 0;
  std::vector<Cell> a;
};

namespace detail {

inline void heapadjust(size_t i, size_t n, int *l) {  // ks_heapadjust(int): a max-heap
  size_t k = i;
  const int tmp = l[i];
  while ((k = (k << 1) + 1) < n) {
    if (k != n - 1 && l[k] < l[k + 1]) ++k;
    if (l[k] < tmp) break;
    l[i] = l[k];
    i = k;
  }
  l[i] = tmp;
}

// bwtsw2_core.c:122-145.  ks_ksmall(n, a, T) is the element of rank T (0-based) of a = -G in
// ascending order, so x is the (T+1)-th largest G.
inline void cut_tail(Entry *u, int T, Counters *ct) {
  const int un = (int)u->a.size();
  if (un <= T) return;
  std::vector<int> a;
  for (const Cell &c : u->a)
    if (c.ql && c.G > 0) a.push_back(-c.G);
  if ((int)a.size() <= T) return;
  std::nth_element(a.begin(), a.begin() + T, a.end());
  const int x = -a[T];
  int n = 0;
  for (int i = 0; i < un; ++i) {
    Cell *p = &u->a[i];
    if (p->G == x) ++n;
    if (p->G < x || (p->G == x && n >= T)) {
      if (ct && p->ql && p->G == x) ++ct->n_tie_cut;
      p->qk = p->ql = 0;
      p->G = 0;
      if (p->ppos >= 0) {
        u->a[p->ppos].cpos[p->pj] = -1;
        u->a[p->ppos].cut |= 1u << p->pj;
      }
    }
  }
}

// :147-172
inline void remove_duplicate(Entry *u, std::unordered_map<uint64_t, uint64_t> &hash, Counters *ct) {
  hash.clear();
  const int un = (int)u->a.size();
  for (int i = 0; i != un; ++i) {
    Cell *p = &u->a[i];
    if (p->ql == 0) continue;
    const uint64_t key = (uint64_t)p->qk << 32 | p->ql;
    auto ins = hash.emplace(key, 0);
    int j = -1;
    if (!ins.second) {
      if ((uint32_t)ins.first->second >= (uint32_t)p->G) j = i;
      else {
        j = (int)(ins.first->second >> 32);
        ins.first->second = (uint64_t)i << 32 | (uint32_t)p->G;
      }
    } else ins.first->second = (uint64_t)i << 32 | (uint32_t)p->G;
    if (j >= 0) {
      p = &u->a[j];
      p->qk = p->ql = 0;
      p->G = 0;
      if (p->ppos >= 0) u->a[p->ppos].cpos[p->pj] = -3;
      if (ct) ++ct->n_dup;
    }
  }
}

// :174-191: v appended to u
inline void merge_entry(Entry *u, Entry *v) {
  const int un = (int)u->a.size();
  for (Cell &p : v->a) {
    if (p.ppos >= 0) p.ppos += un;
    for (int j = 0; j < 4; ++j)
      if (p.cpos[j] >= 0) p.cpos[j] += un;
  }
  u->a.insert(u->a.end(), v->a.begin(), v->a.end());
}

// :211-233
inline void save_hits(const Bwtl &bwt, int thres, std::vector<Hit> &hits, const Entry *u, Counters *ct) {
  for (const Cell &p : u->a) {
    if (p.G < thres) continue;
    for (uint32_t k = u->tk; k <= u->tl; ++k) {
      const int beg = bwt.sa[k], end = beg + p.tlen;
      Hit *q = nullptr;
      if (p.G > hits[beg * 2].G) {
        if (ct && hits[beg * 2].G > 0) ++ct->n_displaced;
        hits[beg * 2 + 1] = hits[beg * 2];
        q = &hits[beg * 2];
      } else if (p.G > hits[beg * 2 + 1].G) q = &hits[beg * 2 + 1];
      if (q) {
        q->k = p.qk;
        q->l = p.ql;
        q->len = p.qlen;
        q->G = p.G;
        q->beg = beg;
        q->end = end;
        q->G2 = q->k == q->l ? 0 : q->G;
        q->flag = 0;
      }
    }
  }
}

// :236-258
inline void save_narrow_hits(const Bwtl &bwtl, Entry *u, std::vector<Hit> &b1, int t, int IS) {
  for (Cell &p : u->a) {
    if (p.G >= t && p.ql - p.qk + 1 <= (uint32_t)IS) {
      Hit q;
      q.k = p.qk;
      q.l = p.ql;
      q.len = p.qlen;
      q.G = p.G;
      q.G2 = 0;
      q.beg = bwtl.sa[u->tk];
      q.end = q.beg + p.tlen;
      q.flag = 0;
      b1.push_back(q);
      p.qk = p.ql = 0;
      p.G = 0;
      if (p.ppos >= 0) u->a[p.ppos].cpos[p.pj] = -3;
    }
  }
}

}  // namespace detail

// One task: all = b_ret[0], narrow = b_ret[1], both after bsw2_resolve_duphits.
template <class Idx>
inline void seed_task(const Opt &opt, const uint8_t *seq, int len, const Idx &query, std::vector<Hit> &all,
                      std::vector<Hit> &narrow, Counters *ct = nullptr) {
  using namespace detail;
  Bwtl target;
  target.build(len, seq);
  const int qr = opt.q + opt.r;
  Counters local;
  Counters &C = ct ? *ct : local;

  // bsw2_connectivity (:87-120): how many parents every DAWG node has
  std::unordered_map<uint64_t, uint64_t> chash, rhash;
  {
    std::vector<uint64_t> st;
    st.push_back((uint64_t)target.seq_len);
    while (!st.empty()) {
      const uint64_t x = st.back();
      st.pop_back();
      uint32_t ck[4], cl[4];
      target.occ4((uint32_t)(x >> 32) - 1, ck);
      target.occ4((uint32_t)x, cl);
      for (int j = 0; j != 4; ++j) {
        const uint32_t k = target.L2[j] + ck[j] + 1, l = target.L2[j] + cl[j];
        if (k > l) continue;
        const uint64_t y = (uint64_t)k << 32 | l;
        auto ins = chash.emplace(y, 1);
        if (ins.second) st.push_back(y);
        else ++ins.first->second;
      }
    }
    C.dag_nodes = (int64_t)chash.size();
  }
  int score_mat[16];
  for (int i = 0; i != 4; ++i)
    for (int j = 0; j != 4; ++j) score_mat[i << 2 | j] = i == j ? opt.a : -opt.b;

  std::vector<Entry *> stack0, pending;
  int n_pending = 0;
  int64_t live = 0;  // cells held by stack0, pending, v and u
  auto note = [&](const Entry *e) {
    if ((int64_t)e->a.size() > C.max_array) C.max_array = (int64_t)e->a.size();
    if (live > C.peak_cells) C.peak_cells = live;
  };
  auto release = [&](Entry *e) {
    live -= (int64_t)e->a.size();
    delete e;
  };
  {  // init_bwtsw2 (:415-427)
    Entry *u = new Entry;
    u->tk = 0;
    u->tl = target.seq_len;
    Cell x = {0, 0, kMinusInf, kMinusInf, 0, 0, 0, 0, -1, -1, {-1, -1, -1, -1}, 0};
    x.ql = query.seq_len;
    u->a.push_back(x);
    ++live;
    stack0.push_back(u);
  }
  std::vector<int> heap(opt.z, 0);
  all.assign((size_t)len * 2, Hit{0, 0, 0, 0, 0, 0, 0, 0});
  narrow.clear();

  while (!(stack0.empty() && n_pending == 0)) {
    Entry *v = stack0.back();
    stack0.pop_back();
    const int old_n = (int)v->a.size();
    ++C.iters;
    for (Cell &p : v->a) {  // max depth and band width (:466-473)
      if (p.ql == 0) continue;
      if (p.tlen - (int)p.qlen > opt.bw || (int)p.qlen - p.tlen > opt.bw) {
        p.qk = p.ql = 0;
        if (p.ppos >= 0) {
          v->a[p.ppos].cpos[p.pj] = -5;
          ++C.n_band_del;
        }
      }
    }
    uint32_t tcntk[4], tcntl[4];
    target.occ4(v->tk - 1, tcntk);
    target.occ4(v->tl, tcntl);
    for (int tj = 0; tj != 4; ++tj) {
      const int *curr_score_mat = score_mat + tj * 4;
      uint32_t k = target.L2[tj] + tcntk[tj] + 1, l = target.L2[tj] + tcntl[tj];
      if (k > l) continue;
      auto iter = chash.find((uint64_t)k << 32 | l);
      --iter->second;
      Entry *u = new Entry;
      u->tk = k;
      u->tl = l;
      std::fill(heap.begin(), heap.end(), 0);
      for (int i = 0; i < (int)v->a.size(); ++i) {  // visits the cells it appends (:494-544)
        Cell *p = &v->a[i];
        bool is_added = false;
        if (p->ql == 0) continue;
        ++C.cells_visited;
        Cell x;
        memset(&x, 0, sizeof x);
        x.G = kMinusInf;
        p->upos = x.upos = -1;
        if (p->ppos >= 0) {
          const Cell &par = v->a[p->ppos];
          const Cell *c1 = par.upos >= 0 ? &u->a[par.upos] : nullptr;
          // fill_cell (:401-413): c[1] = c1, c[2] = p, c[3] = par
          int G = par.G + curr_score_mat[p->pj];
          if (c1) {
            x.I = c1->I > c1->G - opt.q ? c1->I - opt.r : c1->G - qr;
            if (x.I > G) G = x.I;
          } else x.I = kMinusInf;
          x.D = p->D > p->G - opt.q ? p->D - opt.r : p->G - qr;
          if (x.D > G) G = x.D;
          x.G = G;
          if (G > 0) {
            x.ppos = par.upos;
            p->upos = (int)u->a.size();
            if (x.ppos >= 0) u->a[x.ppos].cpos[p->pj] = p->upos;
            is_added = true;
          }
        } else {
          x.D = p->D > p->G - opt.q ? p->D - opt.r : p->G - qr;
          if (x.D > 0) {
            x.G = x.D;
            x.I = kMinusInf;
            x.ppos = -1;
            p->upos = (int)u->a.size();
            is_added = true;
          }
        }
        if (is_added) {
          x.cpos[0] = x.cpos[1] = x.cpos[2] = x.cpos[3] = -1;
          x.pj = p->pj;
          x.qk = p->qk;
          x.ql = p->ql;
          x.qlen = p->qlen;
          x.tlen = p->tlen + 1;
          x.cut = 0;
          u->a.push_back(x);
          ++live;
          if (x.G > -heap[0]) {
            heap[0] = -x.G;
            heapadjust(0, heap.size(), heap.data());
          }
        }
        if ((x.G > qr && x.G >= -heap[0]) || i < old_n) {  // good node in u, or in v
          if (p->cpos[0] == -1 || p->cpos[1] == -1 || p->cpos[2] == -1 || p->cpos[3] == -1) {
            uint32_t qcntk[4], qcntl[4];
            query.occ4(p->qk - 1, qcntk);
            query.occ4(p->ql, qcntl);
            for (int qj = 0; qj != 4; ++qj) {
              p = &v->a[i];
              if (p->cpos[qj] != -1) continue;
              k = query.L2[qj] + qcntk[qj] + 1;
              l = query.L2[qj] + qcntl[qj];
              if (k > l) {
                p->cpos[qj] = -2;
                continue;
              }
              if (p->cut >> qj & 1) {
                ++C.n_recreate;
                p->cut &= ~(1u << qj);
              }
              Cell y;
              memset(&y, 0, sizeof y);
              y.G = y.I = y.D = kMinusInf;
              y.qk = k;
              y.ql = l;
              y.pj = qj;
              y.qlen = p->qlen + 1;
              y.ppos = i;
              y.tlen = p->tlen;
              y.upos = -1;
              y.cpos[0] = y.cpos[1] = y.cpos[2] = y.cpos[3] = -1;
              p->cpos[qj] = (int)v->a.size();
              v->a.push_back(y);
              ++live;
            }
          }
        }
      }
      note(v);
      note(u);
      if (!u->a.empty()) save_hits(target, opt.t, all, u, &C);
      {  // push u to the stack, or to the pending array (:546-580)
        const uint32_t cnt = (uint32_t)iter->second, pos = (uint32_t)(iter->second >> 32);
        if (pos) {
          Entry *w = pending[pos - 1];
          if (!u->a.empty()) {
            if (w->a.size() < u->a.size()) {
              w = u;
              u = pending[pos - 1];
              pending[pos - 1] = w;
              ++C.n_swap;
            }
            merge_entry(w, u);
            live += (int64_t)u->a.size();
            note(w);
          }
          if (cnt == 0) {
            remove_duplicate(w, rhash, &C);
            save_narrow_hits(target, w, narrow, opt.t, opt.is);
            cut_tail(w, opt.z, &C);
            stack0.push_back(w);
            pending[pos - 1] = nullptr;
            --n_pending;
          }
          release(u);
        } else if (cnt) {
          if (!u->a.empty()) {
            ++n_pending;
            pending.push_back(u);
            iter->second = (uint64_t)pending.size() << 32 | cnt;
          } else release(u);
        } else {
          save_narrow_hits(target, u, narrow, opt.t, opt.is);
          cut_tail(u, opt.z, &C);
          stack0.push_back(u);
        }
        if (n_pending > C.peak_pending) C.peak_pending = n_pending;
        if ((int64_t)stack0.size() > C.max_stack) C.max_stack = (int64_t)stack0.size();
      }
    }
    release(v);
  }
  C.narrow_raw = (int64_t)narrow.size();
  resolve_duphits(query, all, opt.is, &C, false);
  resolve_duphits(query, narrow, opt.is, &C, true);
}

}  // namespace ibwa_bsw2
