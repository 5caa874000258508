// seed.hip -- k_bsw2_seed: bwasw's seeding, bsw2_core (bwtsw2_core.c:429-594) with the read's
// bwtl (bwt_lite.c:9-54), one task per wavefront.  bsw2_core.h is the host statement of the same
// algorithm; DESIGN §4.13 has the arena layout and the order rules.
//
// A workgroup is one wave.  Waves are persistent and claim tasks from an atomic counter.  Per task:
//   prologue   suffix array of the read by prefix doubling (bitonic sort of 64-bit keys, in LDS up
//              to 2 047 bases), BWT / Occ / L2, and the DAWG's connectivity counts (wave-parallel
//              DFS, the node table filled by atomics);
//   traversal  the DAWG walk.  Per popped node: the band test, then per child node the cell loop in
//              chunks of 64 cells -- the wave first issues the rank loads (occ4x2) of the chunk's
//              cells together, then lane 0 walks the chunk in the reference's order (positions in
//              u, the z-best threshold, the appended cells) -- then save_hits, the merge into the
//              pending entry, remove_duplicate, save_narrow_hits and cut_tail, all lane-parallel;
//   resolve    the two lists expanded to the array bsw2_resolve_duphits sorts: one record per SA
//              row, k through bwt_sa (sampled walk or full SA).  The unstable sort and the
//              containment pass over that array are the host's (engine_seed.hip).
// Everything a task needs lives in its wave's arena in HBM, carved here; a task that outgrows it,
// or the launch's output buffer, ends with a status and is run again by the engine.  Every store
// is bounds-checked against the arena: nothing is written outside it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"
#include "occ.h"

namespace ibwa {

namespace {

constexpr int MINF = -0x3fffffff;
constexpr uint32_t CW = 16;  // words per cell: one 64 B line
enum { C_QK, C_QL, C_I, C_D, C_G, C_PJ /* pj | qlen << 2 */, C_TLEN, C_PPOS, C_UPOS, C_CP0 };
constexpr int NCLS = 22;     // cell blocks come in classes of 8 << c cells
constexpr uint32_t EW = 6;   // words per entry
enum { E_N, E_CLS, E_TK, E_TL, E_OFF };
constexpr uint32_t RW = 6;   // words per top-2 slot and per raw narrow hit
enum { R_K, R_L, R_LEN, R_G, R_BEG, R_END };
constexpr uint32_t HW = 4;   // words per node-table slot: k, l, count, pending entry + 1
constexpr int SORT_LDS = 2048;

struct Sh {
  uint32_t o_sa, o_bw, o_occ, o_top, o_hash, o_stk, o_ent, o_heap, o_cells;  // word offsets in the arena
  uint32_t hmask, ent_cap, stk_cap, cell_words;
  uint32_t L2[5], primary;
  uint32_t heap_top, peak_words, narrow_n;
  int free_head[NCLS];
  int ent_free, ent_next, stack_n, n_pending, overflow;
  int v, u, hslot, tmp, tmp2;
  unsigned long long obase;
  uint32_t dfs_top;
  long long task;
  unsigned long long cells_visited;
  uint32_t rk[64][8];
  unsigned long long sortbuf[SORT_LDS];
};

__device__ __forceinline__ int wave_max(int v) {
  for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ uint32_t round4(uint32_t x) { return (x + 3u) & ~3u; }

__device__ __forceinline__ uint32_t *cellp(const Sh &S, uint32_t *A, int off, int i) {
  return A + S.o_cells + (size_t)(uint32_t)(off + i) * CW;
}
__device__ __forceinline__ uint32_t *entp(const Sh &S, uint32_t *A, int e) { return A + S.o_ent + (uint32_t)e * EW; }

// ---- the arena's allocators (lane 0) ----
__device__ int cls_for(uint32_t cells) {
  int c = 0;
  while (c < NCLS && (8u << c) < cells) ++c;
  return c;
}
__device__ void note_peak(Sh &S) {
  const uint32_t w = S.heap_top * CW + S.narrow_n * RW;
  if (w > S.peak_words) S.peak_words = w;
}
__device__ int alloc_block(Sh &S, uint32_t *A, int cls) {
  if (cls >= NCLS) {
    S.overflow = 1;
    return -1;
  }
  int h = S.free_head[cls];
  if (h >= 0) {
    S.free_head[cls] = (int)A[S.o_cells + (size_t)(uint32_t)h * CW];
    return h;
  }
  const uint64_t top = (uint64_t)S.heap_top + (8u << cls);
  if (top * CW + (uint64_t)S.narrow_n * RW > S.cell_words) {
    S.overflow = 1;
    return -1;
  }
  h = (int)S.heap_top;
  S.heap_top = (uint32_t)top;
  note_peak(S);
  return h;
}
__device__ void free_block(Sh &S, uint32_t *A, int off, int cls) {
  if (off < 0 || cls < 0) return;
  A[S.o_cells + (size_t)(uint32_t)off * CW] = (uint32_t)S.free_head[cls];
  S.free_head[cls] = off;
}
__device__ int ent_alloc(Sh &S, uint32_t *A, uint32_t tk, uint32_t tl) {
  int e;
  if (S.ent_free >= 0) {
    e = S.ent_free;
    S.ent_free = (int)entp(S, A, e)[E_N];
  } else {
    if ((uint32_t)S.ent_next >= S.ent_cap) {
      S.overflow = 1;
      return -1;
    }
    e = S.ent_next++;
  }
  uint32_t *E = entp(S, A, e);
  E[E_N] = 0;
  E[E_CLS] = (uint32_t)-1;
  E[E_TK] = tk;
  E[E_TL] = tl;
  E[E_OFF] = (uint32_t)-1;
  return e;
}
__device__ void ent_release(Sh &S, uint32_t *A, int e) {
  uint32_t *E = entp(S, A, e);
  free_block(S, A, (int)E[E_OFF], (int)E[E_CLS]);
  E[E_N] = (uint32_t)S.ent_free;
  S.ent_free = e;
}

// Room for `need` cells in entry e (wave): a larger block, the cells copied by the wave.
__device__ bool ensure_cap(Sh &S, uint32_t *A, int e, uint32_t need, int lane) {
  uint32_t *E = entp(S, A, e);
  const int cls = (int)E[E_CLS], off = (int)E[E_OFF];
  const uint32_t n = E[E_N];
  if (cls >= 0 && (8u << cls) >= need) return true;
  __syncthreads();
  if (lane == 0) {
    S.tmp2 = cls_for(need);
    S.tmp = alloc_block(S, A, S.tmp2);
  }
  __syncthreads();
  const int noff = S.tmp, ncls = S.tmp2;
  if (noff < 0) return false;
  if (cls >= 0) {
    const uint4 *src = reinterpret_cast<const uint4 *>(cellp(S, A, off, 0));
    uint4 *dst = reinterpret_cast<uint4 *>(cellp(S, A, noff, 0));
    for (uint32_t i = lane; i < n * 4; i += 64) dst[i] = src[i];
  }
  __syncthreads();
  if (lane == 0) {
    free_block(S, A, off, cls);
    E[E_CLS] = (uint32_t)ncls;
    E[E_OFF] = (uint32_t)noff;
  }
  __syncthreads();
  return true;
}

// ---- the read's BWT ----
// bwtl_occ4 (bwt_lite.c:68-82)
__device__ void bwtl_occ4(const Sh &S, const uint32_t *A, uint32_t k, uint32_t cnt[4]) {
  if (k == 0xFFFFFFFFu) {
    cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
    return;
  }
  if (k >= S.primary) --k;
  const uint32_t *o = A + S.o_occ + (k >> 4) * 4;
  const uint32_t n = (k & 15) + 1, w = A[S.o_bw + (k >> 4)] >> (2 * (16 - n));  // the first n symbols, low bits
  const uint32_t m = n == 16 ? 0x55555555u : ((1u << (2 * n)) - 1u) & 0x55555555u;
  for (uint32_t c = 0; c < 4; ++c) {
    const uint32_t x = w ^ (c * 0x55555555u);
    cnt[c] = o[c] + (uint32_t)__builtin_popcount(~(x | (x >> 1)) & m);
  }
}

__device__ void bitonic_sort(unsigned long long *a, uint32_t P, int lane) {
  for (uint32_t k = 2; k <= P; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = lane; t < P / 2; t += 64) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), x = i | j;
        const unsigned long long p = a[i], q = a[x];
        const bool asc = (i & k) == 0;
        if ((p > q) == asc) {
          a[i] = q;
          a[x] = p;
        }
      }
      __syncthreads();
    }
}

// Suffix array, BWT, Occ, L2 and primary of seq[0, L) into the arena.  rk: L + 1 scratch words (the
// node table's area, cleared afterwards); keys: the sort buffer (LDS, or the empty cell area).
__device__ void build_bwtl(Sh &S, uint32_t *A, const uint8_t *seq, uint32_t L, int lane) {
  const uint32_t N = L + 1;
  uint32_t P = 64;
  while (P < N) P <<= 1;
  unsigned long long *keys = P <= SORT_LDS ? S.sortbuf : reinterpret_cast<unsigned long long *>(A + S.o_cells);
  uint32_t *rk = A + S.o_hash, *sa = A + S.o_sa;
  // first ranks: six symbols as base-5 digits, the end of the read below every symbol
  for (uint32_t i = lane; i < N; i += 64) {
    uint32_t r = 0;
    for (uint32_t d = 0; d < 6; ++d) r = r * 5 + (i + d < L ? seq[i + d] + 1u : 0u);
    rk[i] = r;
  }
  __syncthreads();
  for (uint32_t h = 6;; h <<= 1) {
    for (uint32_t i = lane; i < P; i += 64) {
      unsigned long long key = ~0ull;
      if (i < N) key = (unsigned long long)rk[i] << 28 | (unsigned long long)(i + h < N ? rk[i + h] + 1u : 0u) << 14 | i;
      keys[i] = key;
    }
    __syncthreads();
    bitonic_sort(keys, P, lane);
    // new ranks: the number of key changes before each sorted position
    uint32_t base = 0;
    for (uint32_t p0 = 0; p0 < N; p0 += 64) {
      const uint32_t p = p0 + lane;
      bool flag = false;
      unsigned long long key = 0;
      if (p < N) {
        key = keys[p];
        flag = p > 0 && (keys[p - 1] >> 14) != (key >> 14);
      }
      const unsigned long long m = __ballot(flag);
      const uint32_t r = base + (uint32_t)__popcll(m & ((2ull << lane) - 1ull));
      if (p < N) {
        const uint32_t i = (uint32_t)key & 0x3FFFu;  // < N: the padding keys sort behind the N suffixes
        if (i < N) rk[i] = r;
        sa[p] = i < N ? i : 0;
      }
      base += (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (base == N - 1 || h >= N) break;
  }
  // BWT words, their symbol counts, primary
  const uint32_t W = (L + 15) / 16;
  for (uint32_t p = lane; p < N; p += 64)
    if (sa[p] == 0) S.primary = p;
  __syncthreads();
  const uint32_t primary = S.primary;
  uint32_t run[4] = {0, 0, 0, 0};
  for (uint32_t w0 = 0; w0 < W; w0 += 64) {
    const uint32_t w = w0 + lane;
    uint32_t word = 0, c01 = 0, c23 = 0;
    if (w < W) {
      for (uint32_t j = 0; j < 16; ++j) {
        const uint32_t i = w * 16 + j;
        if (i >= L) break;
        const uint32_t at = sa[i < primary ? i : i + 1];
        const uint32_t c = at - 1 < L ? seq[at - 1] : 0;
        word |= c << ((15 - j) << 1);
        if (c < 2) c01 += c == 0 ? 1u : 0x10000u;
        else c23 += c == 2 ? 1u : 0x10000u;
      }
      A[S.o_bw + w] = word;
    }
    const uint32_t s01 = wave_scan_incl(c01, lane), s23 = wave_scan_incl(c23, lane);
    if (w < W) {
      uint32_t *o = A + S.o_occ + w * 4;
      o[0] = run[0] + ((s01 - c01) & 0xFFFF);
      o[1] = run[1] + ((s01 - c01) >> 16);
      o[2] = run[2] + ((s23 - c23) & 0xFFFF);
      o[3] = run[3] + ((s23 - c23) >> 16);
    }
    const uint32_t t01 = __shfl(s01, 63), t23 = __shfl(s23, 63);
    run[0] += t01 & 0xFFFF;
    run[1] += t01 >> 16;
    run[2] += t23 & 0xFFFF;
    run[3] += t23 >> 16;
  }
  if (lane == 0) {
    S.L2[0] = 0;
    for (int c = 0; c < 4; ++c) S.L2[c + 1] = S.L2[c] + run[c];
  }
  __syncthreads();
}

__device__ __forceinline__ uint32_t node_hash(uint32_t k, uint32_t l) {
  uint32_t h = k * 0x9E3779B1u ^ l * 0x85EBCA77u;
  return h ^ (h >> 15);
}
// slot of node (k, l) in the node table (present by construction); -1 if the table is corrupt
__device__ int node_find(const Sh &S, const uint32_t *A, uint32_t k, uint32_t l) {
  uint32_t h = node_hash(k, l) & S.hmask;
  for (uint32_t probe = 0; probe <= S.hmask; ++probe, h = (h + 1) & S.hmask) {
    const uint32_t *s = A + S.o_hash + h * HW;
    if (s[0] == k && s[1] == l) return (int)h;
    if (s[0] == 0) return -1;
  }
  return -1;
}

// bsw2_connectivity (:87-120): every DAWG node's number of parents.  The DFS stack (k, l pairs) borrows
// the top-2 table's area, which is cleared afterwards.
__device__ void connectivity(Sh &S, uint32_t *A, uint32_t L, int lane) {
  uint32_t *st = A + S.o_top;
  const uint32_t st_cap = RW * 2 * L / 2;  // pairs
  for (uint32_t i = lane; i < (S.hmask + 1) * HW; i += 64) A[S.o_hash + i] = 0;
  if (lane == 0) {
    st[0] = 0;
    st[1] = L;
    S.dfs_top = 1;
  }
  for (;;) {
    __syncthreads();
    const uint32_t top = S.dfs_top;
    if (top == 0 || S.overflow) break;
    const uint32_t m = top < 64 ? top : 64;
    uint32_t k = 0, l = 0;
    if ((uint32_t)lane < m) {
      k = st[2 * (top - 1 - lane)];
      l = st[2 * (top - 1 - lane) + 1];
    }
    __syncthreads();
    if (lane == 0) S.dfs_top = top - m;
    __syncthreads();
    if ((uint32_t)lane < m) {
      uint32_t ck[4], cl[4];
      bwtl_occ4(S, A, k - 1, ck);
      bwtl_occ4(S, A, l, cl);
      for (int j = 0; j < 4; ++j) {
        const uint32_t kk = S.L2[j] + ck[j] + 1, ll = S.L2[j] + cl[j];
        if (kk > ll) continue;
        const unsigned long long key = (unsigned long long)ll << 32 | kk;
        uint32_t h = node_hash(kk, ll) & S.hmask;
        for (uint32_t probe = 0; probe <= S.hmask; ++probe, h = (h + 1) & S.hmask) {
          uint32_t *s = A + S.o_hash + h * HW;
          const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long *>(s), 0ull, key);
          if (old == 0ull || old == key) {
            atomicAdd(s + 2, 1u);
            if (old == 0ull) {
              const uint32_t pos = atomicAdd(&S.dfs_top, 1u);
              if (pos < st_cap) {
                st[2 * pos] = kk;
                st[2 * pos + 1] = ll;
              } else S.overflow = 1;
            }
            break;
          }
        }
      }
    }
  }
  __syncthreads();
}

// ---- the stages of the traversal ----
// :466-473, the band test over the popped node's cells
__device__ void band_test(const Sh &S, uint32_t *A, int v, int bw, int lane) {
  const uint32_t *E = entp(S, A, v);
  const int n = (int)E[E_N], off = (int)E[E_OFF];
  for (int i = lane; i < n; i += 64) {
    uint32_t *p = cellp(S, A, off, i);
    if (p[C_QL] == 0) continue;
    const int tlen = (int)p[C_TLEN], qlen = (int)(p[C_PJ] >> 2);
    if (tlen - qlen > bw || qlen - tlen > bw) {
      p[C_QK] = p[C_QL] = 0;
      if ((int)p[C_PPOS] >= 0) cellp(S, A, off, (int)p[C_PPOS])[C_CP0 + (p[C_PJ] & 3)] = (uint32_t)-5;
    }
  }
}

struct SeedOpt {
  int a, b, q, r, qr, t, bw, z, is;
};

// :494-544 for cells [base, base + cnt) of v, lane 0 alone, in the reference's order.  The ranks of
// the chunk's cells are in S.rk; v has room for 4 * cnt more cells and u for cnt more.
__device__ void walk_chunk(Sh &S, uint32_t *A, const IndexView &ix, const SeedOpt &o, int v, int u, int tj, int old_n,
                           int base, int cnt) {
  uint32_t *EV = entp(S, A, v), *EU = entp(S, A, u);
  const int voff = (int)EV[E_OFF], uoff = (int)EU[E_OFF];
  int vn = (int)EV[E_N], un = (int)EU[E_N];
  int *heap = reinterpret_cast<int *>(A + S.o_heap);
  unsigned long long visited = 0;
  for (int i = base; i < base + cnt; ++i) {
    uint32_t *p = cellp(S, A, voff, i);
    if (p[C_QL] == 0) continue;
    ++visited;
    const uint32_t pj = p[C_PJ] & 3;
    const int ppos = (int)p[C_PPOS];
    uint32_t *x = cellp(S, A, uoff, un);
    int xI = MINF, xD, xG = MINF, xppos = -1;
    bool is_added = false;
    p[C_UPOS] = (uint32_t)-1;
    if (ppos >= 0) {
      const uint32_t *par = cellp(S, A, voff, ppos);
      const int pupos = (int)par[C_UPOS];
      int G = (int)par[C_G] + (pj == (uint32_t)tj ? o.a : -o.b);
      if (pupos >= 0) {
        const uint32_t *c1 = cellp(S, A, uoff, pupos);
        xI = (int)c1[C_I] > (int)c1[C_G] - o.q ? (int)c1[C_I] - o.r : (int)c1[C_G] - o.qr;
        if (xI > G) G = xI;
      }
      xD = (int)p[C_D] > (int)p[C_G] - o.q ? (int)p[C_D] - o.r : (int)p[C_G] - o.qr;
      if (xD > G) G = xD;
      xG = G;
      if (G > 0) {
        xppos = pupos;
        p[C_UPOS] = (uint32_t)un;
        if (xppos >= 0) cellp(S, A, uoff, xppos)[C_CP0 + pj] = (uint32_t)un;
        is_added = true;
      }
    } else {
      xD = (int)p[C_D] > (int)p[C_G] - o.q ? (int)p[C_D] - o.r : (int)p[C_G] - o.qr;
      if (xD > 0) {
        xG = xD;
        xI = MINF;
        xppos = -1;
        p[C_UPOS] = (uint32_t)un;
        is_added = true;
      }
    }
    if (is_added) {
      x[C_QK] = p[C_QK];
      x[C_QL] = p[C_QL];
      x[C_I] = (uint32_t)xI;
      x[C_D] = (uint32_t)xD;
      x[C_G] = (uint32_t)xG;
      x[C_PJ] = p[C_PJ];
      x[C_TLEN] = p[C_TLEN] + 1;
      x[C_PPOS] = (uint32_t)xppos;
      x[C_UPOS] = (uint32_t)-1;
      x[C_CP0] = x[C_CP0 + 1] = x[C_CP0 + 2] = x[C_CP0 + 3] = (uint32_t)-1;
      ++un;
      if (xG > -heap[0]) {  // ks_heapadjust(int) on the z-best heap
        heap[0] = -xG;
        size_t hi = 0, k = 0;
        const size_t n = (size_t)o.z;
        const int tmp = heap[0];
        while ((k = (k << 1) + 1) < n) {
          if (k != n - 1 && heap[k] < heap[k + 1]) ++k;
          if (heap[k] < tmp) break;
          heap[hi] = heap[k];
          hi = k;
        }
        heap[hi] = tmp;
      }
    }
    if ((xG > o.qr && xG >= -heap[0]) || i < old_n) {
      if ((int)p[C_CP0] == -1 || (int)p[C_CP0 + 1] == -1 || (int)p[C_CP0 + 2] == -1 || (int)p[C_CP0 + 3] == -1) {
        const uint32_t *r = S.rk[i - base];
        for (uint32_t qj = 0; qj < 4; ++qj) {
          if ((int)p[C_CP0 + qj] != -1) continue;
          const uint32_t k = l2of(ix, qj) + r[qj] + 1, l = l2of(ix, qj) + r[4 + qj];
          if (k > l) {
            p[C_CP0 + qj] = (uint32_t)-2;
            continue;
          }
          uint32_t *y = cellp(S, A, voff, vn);
          y[C_QK] = k;
          y[C_QL] = l;
          y[C_I] = y[C_D] = y[C_G] = (uint32_t)MINF;
          y[C_PJ] = qj | ((p[C_PJ] >> 2) + 1) << 2;
          y[C_TLEN] = p[C_TLEN];
          y[C_PPOS] = (uint32_t)i;
          y[C_UPOS] = (uint32_t)-1;
          y[C_CP0] = y[C_CP0 + 1] = y[C_CP0 + 2] = y[C_CP0 + 3] = (uint32_t)-1;
          p[C_CP0 + qj] = (uint32_t)vn++;
        }
      }
    }
  }
  EV[E_N] = (uint32_t)vn;
  EU[E_N] = (uint32_t)un;
  S.cells_visited += visited;
}

// save_hits (:211-233): cells in order, the rows tk..tl of one cell across the lanes (their read
// positions differ, so their slots do)
__device__ void save_hits(const Sh &S, uint32_t *A, int u, int thres, int lane) {
  const uint32_t *E = entp(S, A, u);
  const int n = (int)E[E_N], off = (int)E[E_OFF];
  const uint32_t tk = E[E_TK], tl = E[E_TL];
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    int G = MINF;
    uint32_t qk = 0, ql = 0, qlen = 0, tlen = 0;
    if (i < n) {
      const uint32_t *p = cellp(S, A, off, i);
      G = (int)p[C_G];
      qk = p[C_QK];
      ql = p[C_QL];
      qlen = p[C_PJ] >> 2;
      tlen = p[C_TLEN];
    }
    unsigned long long m = __ballot(i < n && G >= thres);
    while (m) {
      const int j = __builtin_ctzll(m);
      m &= m - 1;
      const int g = __shfl(G, j);
      const uint32_t k0 = __shfl(qk, j), l0 = __shfl(ql, j), len0 = __shfl(qlen, j), tlen0 = __shfl(tlen, j);
      for (uint32_t k = tk + lane; k <= tl; k += 64) {
        const uint32_t beg = A[S.o_sa + k];
        uint32_t *h0 = A + S.o_top + (size_t)beg * 2 * RW, *h1 = h0 + RW, *q = nullptr;
        if (g > (int)h0[R_G]) {
          for (uint32_t w = 0; w < RW; ++w) h1[w] = h0[w];
          q = h0;
        } else if (g > (int)h1[R_G]) q = h1;
        if (q) {
          q[R_K] = k0;
          q[R_L] = l0;
          q[R_LEN] = len0;
          q[R_G] = (uint32_t)g;
          q[R_BEG] = beg;
          q[R_END] = beg + tlen0;
        }
      }
    }
  }
}

// merge_entry (:174-191): u's cells appended to w's (w has room)
__device__ void merge_cells(const Sh &S, uint32_t *A, int w, int u, int lane) {
  const uint32_t *EWp = entp(S, A, w), *EU = entp(S, A, u);
  const int wn = (int)EWp[E_N], woff = (int)EWp[E_OFF], un = (int)EU[E_N], uoff = (int)EU[E_OFF];
  for (int i = lane; i < un; i += 64) {
    const uint4 *src = reinterpret_cast<const uint4 *>(cellp(S, A, uoff, i));
    uint4 c0 = src[0], c1 = src[1], c2 = src[2], c3 = src[3];
    if ((int)c1.w >= 0) c1.w += wn;  // ppos
    if ((int)c2.y >= 0) c2.y += wn;  // cpos[0..3]
    if ((int)c2.z >= 0) c2.z += wn;
    if ((int)c2.w >= 0) c2.w += wn;
    if ((int)c3.x >= 0) c3.x += wn;
    uint4 *dst = reinterpret_cast<uint4 *>(cellp(S, A, woff, wn + i));
    dst[0] = c0;
    dst[1] = c1;
    dst[2] = c2;
    dst[3] = c3;
  }
}

__device__ __forceinline__ void delete_cell(const Sh &S, uint32_t *A, int off, uint32_t *p, int mark) {
  p[C_QK] = p[C_QL] = 0;
  p[C_G] = 0;
  if ((int)p[C_PPOS] >= 0) cellp(S, A, off, (int)p[C_PPOS])[C_CP0 + (p[C_PJ] & 3)] = (uint32_t)mark;
}

// remove_duplicate (:147-172): among equal (qk, ql) the first cell with the largest G stays.  The
// table (key, G << 32 | ~i by atomicMax) lives in a block of the cell area.
__device__ bool remove_duplicate(Sh &S, uint32_t *A, int w, int lane) {
  const uint32_t *E = entp(S, A, w);
  const int n = (int)E[E_N], off = (int)E[E_OFF];
  if (n < 2) return true;
  uint32_t slots = 64;
  while (slots < 2u * (uint32_t)n) slots <<= 1;
  __syncthreads();
  if (lane == 0) {
    S.tmp2 = cls_for(slots * 4 / CW);
    S.tmp = alloc_block(S, A, S.tmp2);
  }
  __syncthreads();
  const int toff = S.tmp, tcls = S.tmp2;
  if (toff < 0) return false;
  unsigned long long *tab = reinterpret_cast<unsigned long long *>(cellp(S, A, toff, 0));
  for (uint32_t i = lane; i < slots * 2; i += 64) tab[i] = 0;
  __syncthreads();
  const uint32_t mask = slots - 1;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = lane; i < n; i += 64) {
      uint32_t *p = cellp(S, A, off, i);
      if (p[C_QL] == 0) continue;
      const unsigned long long key = (unsigned long long)p[C_QK] << 32 | p[C_QL];
      const unsigned long long val = (unsigned long long)p[C_G] << 32 | (0xFFFFFFFFu - (uint32_t)i);
      uint32_t h = node_hash(p[C_QK], p[C_QL]) & mask;
      for (uint32_t probe = 0; probe < slots; ++probe, h = (h + 1) & mask) {
        if (pass == 0) {
          const unsigned long long old = atomicCAS(&tab[2 * h], 0ull, key);
          if (old == 0ull || old == key) {
            atomicMax(&tab[2 * h + 1], val);
            break;
          }
        } else if (tab[2 * h] == key) {
          if (tab[2 * h + 1] != val) delete_cell(S, A, off, p, -3);
          break;
        }
      }
    }
    __syncthreads();
  }
  if (lane == 0) free_block(S, A, toff, tcls);
  __syncthreads();
  return true;
}

// save_narrow_hits (:236-258): appended in cell order, from the arena's end downwards
__device__ bool save_narrow(Sh &S, uint32_t *A, int u, int t, int IS, int lane) {
  const uint32_t *E = entp(S, A, u);
  const int n = (int)E[E_N], off = (int)E[E_OFF];
  const uint32_t beg = A[S.o_sa + E[E_TK]];
  uint32_t nn = S.narrow_n;
  const uint32_t heap_words = S.heap_top * CW;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    uint32_t *p = nullptr;
    bool hit = false;
    if (i < n) {
      p = cellp(S, A, off, i);
      hit = (int)p[C_G] >= t && p[C_QL] - p[C_QK] + 1 <= (uint32_t)IS;
    }
    const unsigned long long m = __ballot(hit);
    if (!m) continue;
    const uint32_t add = (uint32_t)__popcll(m);
    if ((uint64_t)heap_words + (uint64_t)(nn + add) * RW > S.cell_words) {
      __syncthreads();
      if (lane == 0) S.overflow = 1;
      __syncthreads();
      return false;
    }
    if (hit) {
      const uint32_t j = nn + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      uint32_t *q = A + S.o_cells + S.cell_words - (size_t)(j + 1) * RW;
      q[R_K] = p[C_QK];
      q[R_L] = p[C_QL];
      q[R_LEN] = p[C_PJ] >> 2;
      q[R_G] = p[C_G];
      q[R_BEG] = beg;
      q[R_END] = beg + p[C_TLEN];
      delete_cell(S, A, off, p, -3);
    }
    nn += add;
  }
  __syncthreads();
  if (lane == 0) {
    S.narrow_n = nn;
    note_peak(S);
  }
  __syncthreads();
  return true;
}

// cut_tail (:122-145): x is the (T+1)-th largest positive G of the live cells; every cell below it goes,
// and of those equal to it all from the T-th on, in array order
__device__ void cut_tail(const Sh &S, uint32_t *A, int u, int T, int lane) {
  const uint32_t *E = entp(S, A, u);
  const int n = (int)E[E_N], off = (int)E[E_OFF];
  if (n <= T) return;
  uint32_t live = 0;
  for (int i = lane; i < n; i += 64) {
    const uint32_t *p = cellp(S, A, off, i);
    live += p[C_QL] != 0 && (int)p[C_G] > 0;
  }
  if ((int)wave_sum(live) <= T) return;
  int cur = 0x7fffffff, rem = T + 1, x = 0;
  for (;;) {
    int mx = 0;
    for (int i = lane; i < n; i += 64) {
      const uint32_t *p = cellp(S, A, off, i);
      const int G = (int)p[C_G];
      if (p[C_QL] != 0 && G > 0 && G < cur && G > mx) mx = G;
    }
    mx = wave_max(mx);
    uint32_t c = 0;
    for (int i = lane; i < n; i += 64) {
      const uint32_t *p = cellp(S, A, off, i);
      c += p[C_QL] != 0 && (int)p[C_G] == mx;
    }
    c = wave_sum(c);
    if ((int)c >= rem || mx == 0) {
      x = mx;
      break;
    }
    rem -= (int)c;
    cur = mx;
  }
  int seen = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    uint32_t *p = nullptr;
    int G = 0;
    if (i < n) {
      p = cellp(S, A, off, i);
      G = (int)p[C_G];
    }
    const unsigned long long m = __ballot(i < n && G == x);
    const int cntx = seen + __popcll(m & ((2ull << lane) - 1ull));
    if (i < n && (G < x || (G == x && cntx >= T))) delete_cell(S, A, off, p, -1);
    seen += __popcll(m);
  }
}

// symbol stored at row k of the $-removed BWT and the LF step (bwt_invPsi, bwt.h:66-70)
__device__ __forceinline__ uint32_t seed_inv_psi(const IndexView &ix, uint32_t k) {
  if (k == ix.primary) return 0;
  const uint32_t p = k < ix.primary ? k : k - 1;
  const uint4 *b = ix.blk + (size_t)(p >> 7) * 4;
  const uint32_t off = p & 127, q = off >> 5;
  const uint4 cnt = b[0], bs = b[1 + (q >> 1)], sb = b[3];
  uint32_t w0, w1, m0, m1;
  chunk_words(bs, q, w0, w1);
  const uint32_t r = off & 31;
  const uint32_t c = ((r < 16 ? w0 : w1) >> (2 * (15 - (r & 15)))) & 3u;
  chunk_masks(r, m0, m1);
  return l2of(ix, c) + sel4(cnt, c) + sub_byte(sb, q, c) + count1(w0, w1, m0, m1, c);
}
// bwt_sa (bwt.c:69-79)
__device__ uint32_t seed_sa(const IndexView &ix, const uint32_t *sa, uint32_t intv, uint32_t k) {
  uint32_t s = 0;
  while (k % intv != 0) {
    ++s;
    k = seed_inv_psi(ix, k);
  }
  return s + (k == 0 ? 0xFFFFFFFFu : sa[k / intv]);
}

// rows a raw hit becomes in the array bsw2_resolve_duphits sorts (:268-272)
__device__ __forceinline__ uint32_t rows_of(uint32_t k, uint32_t l, int G, int IS) {
  const uint32_t d = l - k + 1;
  return d <= (uint32_t)IS ? d : (G > 0 ? 1u : 0u);
}

// One of the two lists on its way to bsw2_resolve_duphits' array (:268-292): counts the rows it becomes
// (pre) and those with G > 0 (real); with out, writes the latter as ibwa_bsw2_hit_t records whose l is
// the row's place in the array to sort (the rows with G == 0 are the empty slots: only their number
// matters to the sort).
__device__ void resolve_list(const Sh &S, const uint32_t *A, const SeedArgs &a, const IndexView &ix, int sx, int IS,
                             bool narrow, uint32_t cnt, uint32_t *out, uint32_t &n_pre, uint32_t &n_real, int lane) {
  uint32_t pre = 0, real = 0;
  for (uint32_t s0 = 0; s0 < cnt; s0 += 64) {
    const uint32_t s = s0 + lane;
    uint32_t rows = 0, rrows = 0;
    const uint32_t *h = nullptr;
    if (s < cnt) {
      h = narrow ? A + S.o_cells + S.cell_words - (size_t)(s + 1) * RW : A + S.o_top + (size_t)s * RW;
      rows = rows_of(h[R_K], h[R_L], (int)h[R_G], IS);
      rrows = (int)h[R_G] > 0 ? rows : 0;
    }
    const uint32_t sp = wave_scan_incl(rows, lane), sr = wave_scan_incl(rrows, lane);
    if (out && rrows) {
      const uint32_t first_pre = pre + sp - rows, first_out = real + sr - rrows;
      const bool rep = h[R_L] - h[R_K] + 1 > (uint32_t)IS;
      for (uint32_t e = 0; e < rrows; ++e) {
        uint32_t *q = out + (size_t)(first_out + e) * 8;
        q[0] = seed_sa(ix, a.sa[sx], a.intv[sx], h[R_K] + e);
        q[1] = first_pre + e;
        q[2] = rep ? 1u : 0u;
        q[3] = h[R_LEN];
        q[4] = h[R_G];
        q[5] = narrow ? 0u : (h[R_K] == h[R_L] ? 0u : h[R_G]);
        q[6] = h[R_BEG];
        q[7] = h[R_END];
      }
    }
    pre += __shfl(sp, 63);
    real += __shfl(sr, 63);
  }
  n_pre = pre;
  n_real = real;
}

}  // namespace

__global__ void __launch_bounds__(64) k_bsw2_seed(SeedArgs a) {
  __shared__ Sh S;
  const int lane = threadIdx.x;
  uint32_t *A = a.arena + (size_t)blockIdx.x * a.arena_words;
  unsigned long long t_build = 0, t_walk = 0, t_resolve = 0;
  for (;;) {
    __syncthreads();
    if (lane == 0) S.task = (long long)atomicAdd(a.claim, 1ull);
    __syncthreads();
    const long long slot = S.task;
    if (slot >= a.n) break;
    const long long task = a.ids ? a.ids[slot] : slot;
    const uint32_t L = a.len[task], N = L + 1;
    const uint8_t *seq = a.seq + a.off[task];
    const int sx = a.strand[task] ? 1 : 0;
    const IndexView ix = sx ? a.ix[1] : a.ix[0];
    SeedOpt o = {a.a, a.b, a.q, a.r, a.q + a.r, a.t[task], a.bw[task], a.z, a.is};
    uint32_t *res = a.res + task * 8;
    unsigned long long c0 = wall_clock64();
    if (lane == 0) {  // carve the arena
      uint32_t hcap = 64;
      while (hcap < 4 * N) hcap <<= 1;
      const uint32_t W = (L + 15) / 16;
      uint64_t p = 0;
      S.o_sa = (uint32_t)p;   p += round4(N);
      S.o_bw = (uint32_t)p;   p += round4(W);
      S.o_occ = (uint32_t)p;  p += 4 * W;
      S.o_top = (uint32_t)p;  p += round4(2 * L * RW);
      S.o_hash = (uint32_t)p; p += (uint64_t)hcap * HW;
      S.o_stk = (uint32_t)p;  p += round4(2 * N + 2);
      S.o_ent = (uint32_t)p;  p += round4((2 * N + 8) * EW);
      S.o_heap = (uint32_t)p; p += round4((uint32_t)o.z);
      S.o_cells = (uint32_t)p;
      S.hmask = hcap - 1;
      S.stk_cap = 2 * N + 2;
      S.ent_cap = 2 * N + 8;
      uint32_t P = 64;
      while (P < N) P <<= 1;
      // the cell area also lends the suffix sort its keys when they do not fit LDS
      const uint64_t need = p + (P > SORT_LDS ? 2ull * P : 0ull) + 16 * CW;
      S.overflow = need > a.arena_words;
      S.cell_words = S.overflow ? 0 : (uint32_t)((a.arena_words - p) / CW * CW);
      S.heap_top = 0;
      S.narrow_n = 0;
      S.peak_words = 0;
      for (int c = 0; c < NCLS; ++c) S.free_head[c] = -1;
      S.ent_free = -1;
      S.ent_next = 0;
      S.stack_n = 0;
      S.n_pending = 0;
      S.cells_visited = 0;
      S.primary = 0;
    }
    __syncthreads();
    bool ok = !S.overflow;
    if (ok) {
      build_bwtl(S, A, seq, L, lane);
      connectivity(S, A, L, lane);
      ok = !S.overflow;
    }
    if (ok) {
      for (uint32_t i = lane; i < 2 * L * RW; i += 64) A[S.o_top + i] = 0;
      __syncthreads();
      if (lane == 0) {  // init_bwtsw2 (:415-427)
        const int e = ent_alloc(S, A, 0, L);
        const int off = alloc_block(S, A, 0);
        if (e >= 0 && off >= 0) {
          uint32_t *E = entp(S, A, e), *x = cellp(S, A, off, 0);
          E[E_CLS] = 0;
          E[E_OFF] = (uint32_t)off;
          E[E_N] = 1;
          x[C_QK] = 0;
          x[C_QL] = ix.seq_len;
          x[C_I] = x[C_D] = (uint32_t)MINF;
          x[C_G] = 0;
          x[C_PJ] = 0;
          x[C_TLEN] = 0;
          x[C_PPOS] = x[C_UPOS] = (uint32_t)-1;
          x[C_CP0] = x[C_CP0 + 1] = x[C_CP0 + 2] = x[C_CP0 + 3] = (uint32_t)-1;
          A[S.o_stk] = (uint32_t)e;
          S.stack_n = 1;
        }
      }
      __syncthreads();
      ok = !S.overflow;
    }
    unsigned long long c1 = wall_clock64();
    t_build += c1 - c0;

    // the main loop: traversal of the DAG (:458-583)
    while (ok) {
      __syncthreads();
      if (S.stack_n == 0 && S.n_pending == 0) break;
      if (S.stack_n == 0) {  // the reference asserts this cannot happen
        ok = false;
        break;
      }
      __syncthreads();
      if (lane == 0) S.v = (int)A[S.o_stk + (uint32_t)--S.stack_n];
      __syncthreads();
      const int v = S.v;
      const int old_n = (int)entp(S, A, v)[E_N];
      band_test(S, A, v, o.bw, lane);
      __syncthreads();
      uint32_t tck[4], tcl[4];
      bwtl_occ4(S, A, entp(S, A, v)[E_TK] - 1, tck);
      bwtl_occ4(S, A, entp(S, A, v)[E_TL], tcl);
      for (int tj = 0; tj < 4 && ok; ++tj) {
        const uint32_t k = S.L2[tj] + tck[tj] + 1, l = S.L2[tj] + tcl[tj];
        if (k > l) continue;
        __syncthreads();
        if (lane == 0) {
          S.hslot = node_find(S, A, k, l);
          if (S.hslot < 0) S.overflow = 1;
          else --A[S.o_hash + (uint32_t)S.hslot * HW + 2];
          S.u = ent_alloc(S, A, k, l);
          int *heap = reinterpret_cast<int *>(A + S.o_heap);
          for (int i = 0; i < o.z; ++i) heap[i] = 0;
        }
        __syncthreads();
        if (S.overflow) {
          ok = false;
          break;
        }
        int u = S.u;
        uint32_t *hs = A + S.o_hash + (uint32_t)S.hslot * HW;
        // the cell loop, a chunk of 64 cells at a time; it visits the cells it appends
        for (int base = 0, cnt = 0; ok; base += cnt) {
          __syncthreads();
          const int vn = (int)entp(S, A, v)[E_N];
          if (base >= vn) break;
          cnt = vn - base < 64 ? vn - base : 64;
          // a visited cell appends at most four cells to v and one to u
          if (!ensure_cap(S, A, v, (uint32_t)(vn + 4 * cnt), lane) ||
              !ensure_cap(S, A, u, entp(S, A, u)[E_N] + (uint32_t)cnt, lane)) {
            ok = false;
            break;
          }
          if (lane < cnt) {  // the chunk's rank loads, issued together
            const uint32_t *p = cellp(S, A, (int)entp(S, A, v)[E_OFF], base + lane);
            if (p[C_QL] != 0 && ((int)p[C_CP0] == -1 || (int)p[C_CP0 + 1] == -1 || (int)p[C_CP0 + 2] == -1 ||
                                 (int)p[C_CP0 + 3] == -1)) {
              uint32_t ck[4], cl[4];
              occ4x2(ix, p[C_QK] - 1, p[C_QL], ck, cl);
              for (int j = 0; j < 4; ++j) {
                S.rk[lane][j] = ck[j];
                S.rk[lane][4 + j] = cl[j];
              }
            }
          }
          __syncthreads();
          if (lane == 0) walk_chunk(S, A, ix, o, v, u, tj, old_n, base, cnt);
        }
        if (!ok) break;
        __syncthreads();
        const int un = (int)entp(S, A, u)[E_N];
        if (un) save_hits(S, A, u, o.t, lane);
        __syncthreads();
        // push u to the stack, or to the pending array (:546-580)
        const uint32_t pcnt = hs[2], pent = hs[3];
        int push = -1;
        if (pent) {
          int w = (int)pent - 1;
          if (un) {
            if ((int)entp(S, A, w)[E_N] < un) {  // the smaller array is appended to the larger
              const int tmp = w;
              w = u;
              u = tmp;
              __syncthreads();
              if (lane == 0) hs[3] = (uint32_t)w + 1;
              __syncthreads();
            }
            const uint32_t wn = entp(S, A, w)[E_N], un2 = entp(S, A, u)[E_N];
            if (!ensure_cap(S, A, w, wn + un2, lane)) {
              ok = false;
              break;
            }
            merge_cells(S, A, w, u, lane);
            __syncthreads();
            if (lane == 0) entp(S, A, w)[E_N] = wn + un2;
            __syncthreads();
          }
          if (pcnt == 0) {
            if (!remove_duplicate(S, A, w, lane) || !save_narrow(S, A, w, o.t, o.is, lane)) {
              ok = false;
              break;
            }
            cut_tail(S, A, w, o.z, lane);
            push = w;
          }
          __syncthreads();
          if (lane == 0) {
            if (pcnt == 0) {
              hs[3] = 0;
              --S.n_pending;
            }
            ent_release(S, A, u);
          }
        } else if (pcnt) {
          __syncthreads();
          if (lane == 0) {
            if (un) {
              ++S.n_pending;
              hs[3] = (uint32_t)u + 1;
            } else ent_release(S, A, u);
          }
        } else {
          if (!save_narrow(S, A, u, o.t, o.is, lane)) {
            ok = false;
            break;
          }
          cut_tail(S, A, u, o.z, lane);
          push = u;
        }
        __syncthreads();
        if (lane == 0 && push >= 0) {
          if ((uint32_t)S.stack_n < S.stk_cap) A[S.o_stk + (uint32_t)S.stack_n++] = (uint32_t)push;
          else S.overflow = 1;
        }
        __syncthreads();
        if (S.overflow) ok = false;
      }
      if (!ok) break;
      __syncthreads();
      if (lane == 0) ent_release(S, A, v);
    }
    __syncthreads();
    unsigned long long c2 = wall_clock64();
    t_walk += c2 - c1;

    // resolve: the arrays bsw2_resolve_duphits sorts, k through bwt_sa
    uint32_t pre_a = 0, real_a = 0, pre_n = 0, real_n = 0;
    int status = ok && !S.overflow ? 0 : 1;
    unsigned long long obase = 0;
    if (status == 0) {
      const uint32_t nn = S.narrow_n;
      resolve_list(S, A, a, ix, sx, o.is, false, 2 * L, nullptr, pre_a, real_a, lane);
      resolve_list(S, A, a, ix, sx, o.is, true, nn, nullptr, pre_n, real_n, lane);
      __syncthreads();
      if (lane == 0) {
        const unsigned long long need = (unsigned long long)real_a + real_n;
        S.obase = atomicAdd(a.out_next, need);
        S.tmp = S.obase + need <= a.out_cap ? 0 : 2;
      }
      __syncthreads();
      status = S.tmp;
      obase = S.obase;
      if (status == 0) {
        resolve_list(S, A, a, ix, sx, o.is, false, 2 * L, a.out + obase * 8, pre_a, real_a, lane);
        resolve_list(S, A, a, ix, sx, o.is, true, nn, a.out + (obase + real_a) * 8, pre_n, real_n, lane);
      }
    }
    __syncthreads();
    if (lane == 0) {
      res[0] = (uint32_t)status;
      res[1] = pre_a;
      res[2] = real_a;
      res[3] = pre_n;
      res[4] = real_n;
      res[5] = (uint32_t)obase;
      res[6] = (uint32_t)(obase >> 32);
      res[7] = S.o_cells + S.peak_words;
      if (a.prof) atomicAdd(a.prof + 3, S.cells_visited);
    }
    t_resolve += wall_clock64() - c2;
  }
  if (lane == 0 && a.prof) {  // wall-clock ticks per phase, summed over the waves
    atomicAdd(a.prof + 0, t_build);
    atomicAdd(a.prof + 1, t_walk);
    atomicAdd(a.prof + 2, t_resolve);
  }
}

hipError_t launch_seed(const SeedArgs &a, int blocks, hipStream_t st) {
  hipError_t e = zero_async(a.claim, 8, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_bsw2_seed, dim3((unsigned)blocks), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace ibwa
