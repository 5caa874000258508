// bsw2_extend.hip -- bwasw's extensions over hit lists: bsw2_extend_left (bwtsw2_aux.c:80-129) in
// dependency order and bsw2_extend_rght (:131-164), as bsw2_aln1.h states them.
//
// Ordered mode (left).  One wave per task, a task being one strand's narrow list of one read, sorted
// by end on the host; the grid is persistent and claims tasks from a counter.  The reference walks
// the list in order: hit i is left alone when an earlier hit, with the coordinates that hit has by
// then, contains it, and is extended otherwise.  The wave takes the list in windows of 64
// consecutive hits, one hit per lane:
//   A  every lane tests its hit against the hits before the window, which are final, 64 of them at a
//      time (each lane loads one, the wave passes them round by shuffles);
//   B  lanes whose hit is neither skipped (l != 0 or k == 0) nor contained yet gather their target
//      window from the resident sequence into the wave's scratch and run extend_core in end-cell mode,
//      lane-serial as k_extend does, the eh ring in LDS when it fits lds_ring words and in the wave's
//      HBM scratch otherwise;
//   C  in window order, hit i is tested against the earlier hits of the window in their final state: a
//      hit found contained drops its speculative result, another applies it when score > G.
// This is the sequential rule: a hit's extension is a function of its own beg, k, G and the read
// alone, and the containment test reads only beg, k, len of earlier hits, which are final after
// their own turn.  The cost is the DP runs that C discards.  Every earlier hit that contains p gets
// its ++n_seeds, saturating at (1 << 14) - 2, whether or not p was known to be contained already.
// Hit j of a list is only ever loaded and stored by lane j % 64, so no store has to become visible
// to another lane.
//
// Unordered mode (right).  The hits are independent, so a claim is 64 consecutive hits of any tasks
// and only step B runs, with the right extension's window, query, G0 = 1 and >=.
//
// A window longer than tgt_bytes or a ring longer than both lds_ring and eh_words is not run: the
// task's status becomes 1 and the host reports the task.  Nothing is stored outside what the launcher sized.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"
#include "stdaln_core.h"

namespace ibwa {

namespace {

using namespace stdaln;

constexpr uint32_t kMaxSeeds = (1u << 14) - 2;

// base g of the resident sequence from word g / 16 (the layout of refine.hip)
__device__ __forceinline__ uint32_t pac_code(uint32_t word, uint64_t g) {
  return (word >> (8u * ((uint32_t)(g >> 2) & 3u) + 6u - 2u * ((uint32_t)g & 3u))) & 3u;
}

struct LaneHit {
  uint32_t k, l, flag, ns;
  int len, G, G2, beg, end;
};

__device__ __forceinline__ void load_hit(const uint32_t *h, LaneHit &x) {
  x.k = h[0]; x.l = h[1]; x.flag = h[2]; x.ns = h[3];
  x.len = (int)h[4]; x.G = (int)h[5]; x.G2 = (int)h[6]; x.beg = (int)h[7]; x.end = (int)h[8];
}

// q contains p (bwtsw2_aux.c:105), the sums in uint32_t
__device__ __forceinline__ bool contains(int qbeg, uint32_t qk, int qlen, int pbeg, uint32_t pk, int plen) {
  return qbeg <= pbeg && qk <= pk && qk + (uint32_t)qlen >= pk + (uint32_t)plen;
}

// One lane's extension: the target window gathered into tg, then extend_core in end-cell mode.
// left: bases k - 1, k - 2, ... down to base 1, at most min(lt, k) of them, against the query
// qry[lq - beg, lq) (the reversed sequence's tail), G0 = G.  right: bases k, k + 1, ... below l_pac, at
// most lt, against qry[beg, lq), G0 = 1.  Returns false when the window or the ring does not fit.
template <bool ALL_LDS>
__device__ __forceinline__ bool lane_extend(const Bsw2ExtArgs &A, bool left, const LaneHit &h, const uint8_t *qry, int lq, int bw,
                                            bool rev, Param P, uint8_t *tg, const View<uint32_t> &eh_lds, const View<uint32_t> &eh_hbm,
                                            int &score, int &end_i, int &end_j) {
  const uint32_t l_pac = (uint32_t)A.l_pac;
  const int n2 = left ? h.beg : lq - h.beg;
  int lt = ((n2 + 1) / 2 * A.a + A.r) / A.r + lq;
  uint32_t n1 = 0;
  if (left) {
    if ((uint32_t)lt > h.k) lt = (int)h.k;
    n1 = (uint32_t)lt < h.k - 1 ? (uint32_t)lt : h.k - 1;  // base 0 is never taken; k >= 1 here
    if (h.k > l_pac) n1 = 0;                                // the host refuses such a hit
  } else {
    const uint32_t e = h.k + (uint32_t)lt;  // uint32_t, as the reference's loop bound
    const uint32_t stop = e < l_pac ? e : l_pac;
    n1 = (e > h.k && stop > h.k) ? stop - h.k : 0;
  }
  score = -1;
  end_i = end_j = 0;
  if (n1 == 0 || n2 <= 0) return true;  // aln_extend_core returns -1
  if (n1 > A.tgt_bytes) return false;
  for (uint32_t j = 0; j < n1; ++j) {
    const uint32_t x = left ? h.k - 1 - j : h.k + j;  // < l_pac
    const uint64_t g = rev ? (uint64_t)l_pac - x - 1 : x;
    tg[j] = (uint8_t)pac_code(A.pac[g >> 4], g);
  }
  P.band = extend_band(bw, (int)n1, n2);
  const uint32_t R = extend_ring(P.band, (int)n1);
  const uint8_t *b = qry + (left ? lq - h.beg : h.beg);
  const int G0 = left ? h.G : 1;
  ExtOut o;
  const View<uint32_t> none{nullptr, 64};
  const TbView T{nullptr, 64u, 0u};
  if (ALL_LDS) {
    if (R > A.lds_ring) return false;
    extend_core(eh_lds, R, none, 0u, T, 0ull, P, 1, G0, tg, (int)n1, b, n2, nullptr, 0, o);
  } else {
    if (R > A.lds_ring && R > A.eh_words) return false;
    const View<uint32_t> eh = R <= A.lds_ring ? eh_lds : eh_hbm;
    extend_core(eh, R, none, 0u, T, 0ull, P, 1, G0, tg, (int)n1, b, n2, nullptr, 0, o);
  }
  score = o.score;
  end_i = o.end_i;
  end_j = o.end_j;
  return true;
}

template <bool ALL_LDS>
__global__ void __launch_bounds__(64) k_bsw2_extend(Bsw2ExtArgs A) {
  extern __shared__ uint32_t smem[];  // matrix (25), then lds_ring ring words per lane
  const int lane = threadIdx.x;
  int *mat = reinterpret_cast<int *>(smem);
  if (lane < 25) mat[lane] = (lane % 6 == 0 && lane < 24) ? A.a : -A.b;  // a on the diagonal of codes 0-3
  __syncthreads();
  Param P;
  P.q = A.q; P.r = A.r; P.gap_end = -1; P.band = 0; P.row = 5; P.max_score = A.a; P.mat = mat;
  const View<uint32_t> eh_lds{smem + 25 + lane, 64};
  const View<uint32_t> eh_hbm{A.eh + (uint64_t)blockIdx.x * A.eh_words * 64 + lane, 64};
  uint8_t *tg = A.tgt + ((uint64_t)blockIdx.x * 64 + lane) * A.tgt_bytes;
  unsigned long long n_run = 0, n_cont = 0, n_disc = 0, n_skip = 0, n_task = 0, n_win = 0;

  if (!A.ordered) {
    for (;;) {
      int64_t base = 0;
      if (lane == 0) base = (int64_t)atomicAdd(A.ctr, 64ull);
      base = __shfl(base, 0);
      if (base >= A.n_hits) break;
      if (lane == 0) ++n_win;
      const int64_t i = base + lane;
      if (i < A.n_hits) {  // the tail lanes idle; every lane comes back to the claim together
        uint32_t *H = A.hits + (uint64_t)i * 9;
        LaneHit h;
        load_hit(H, h);
        if (h.l) {
          ++n_skip;
        } else {
          const uint32_t t = A.htask[i];
          int score, ei, ej;
          if (!lane_extend<ALL_LDS>(A, false, h, A.qry + A.qoff[t], (int)A.qlen[t], A.bw[t], A.is_rev[t] != 0, P, tg, eh_lds, eh_hbm,
                                    score, ei, ej)) {
            A.status[t] = 1;
          } else {
            ++n_run;
            if (score >= h.G) {  // bwtsw2_aux.c:157-161
              H[5] = (uint32_t)score;
              H[4] = (uint32_t)ei;
              H[8] = (uint32_t)(ej + h.beg);
            }
          }
        }
      }
    }
  } else {
    for (;;) {
      int64_t t = 0;
      if (lane == 0) t = (int64_t)atomicAdd(A.ctr, 1ull);
      t = __shfl(t, 0);
      if (t >= A.n_tasks) break;
      if (lane == 0) ++n_task;
      uint32_t *H = A.hits + A.hoff[t] * 9;
      const int64_t n = (int64_t)(A.hoff[t + 1] - A.hoff[t]);
      const uint8_t *qry = A.qry + A.qoff[t];
      const int lq = (int)A.qlen[t], bw = A.bw[t];
      const bool rev = A.is_rev[t] != 0;
      bool overflow = false;
      for (int64_t w0 = 0; w0 < n; w0 += 64) {
        if (lane == 0) ++n_win;
        const bool have = w0 + lane < n;
        LaneHit h = {0, 1, 0, 0, 0, 0, 0, 0, 0};
        if (have) load_hit(H + (uint64_t)(w0 + lane) * 9, h);
        const bool skip = !have || h.l != 0 || h.k == 0;
        // A: the hits before the window, final; chunk c0 .. c0 + 63 is complete, w0 being a multiple of 64
        int before = 0;
        for (int64_t c0 = 0; c0 < w0; c0 += 64) {
          uint32_t *Q = H + (uint64_t)(c0 + lane) * 9;
          const uint32_t qk = Q[0];
          const int qlen = (int)Q[4], qbeg = (int)Q[7];
          uint32_t inc = 0;
          for (int s = 0; s < 64; ++s) {
            // the shuffles first, by every lane: behind a lane's own condition the source lane may be idle
            const int sb = __shfl(qbeg, s), sl = __shfl(qlen, s);
            const uint32_t sk = __shfl(qk, s);
            const bool c = !skip && contains(sb, sk, sl, h.beg, h.k, h.len);
            const unsigned long long m = __ballot(c);
            before += c;
            if (lane == s) inc = (uint32_t)__popcll(m);
          }
          if (inc) {
            const uint32_t v = Q[3] + inc;
            Q[3] = v < kMaxSeeds ? v : kMaxSeeds;
          }
        }
        // B: the speculative extensions
        const bool run = !skip && before == 0;
        int score = -1, ei = 0, ej = 0;
        if (run && !lane_extend<ALL_LDS>(A, true, h, qry, lq, bw, rev, P, tg, eh_lds, eh_hbm, score, ei, ej)) overflow = true;
        // C: the window in order
        uint32_t inc = 0;
        bool discarded = false;
        const int cnt = n - w0 < 64 ? (int)(n - w0) : 64;
        for (int i = 0; i < cnt; ++i) {
          if (__shfl((int)skip, i)) continue;
          const int pb = __shfl(h.beg, i), pl = __shfl(h.len, i);  // by every lane, as in A
          const uint32_t pk = __shfl(h.k, i);
          const bool c = lane < i && contains(h.beg, h.k, h.len, pb, pk, pl);
          const unsigned long long m = __ballot(c);
          inc += c;
          if (lane == i) {
            if (m) discarded = run;
            else if (run && score > h.G) {  // bwtsw2_aux.c:121-126
              h.G = score;
              h.len += ei;
              h.beg -= ej;
              h.k -= (uint32_t)ei;
            }
          }
        }
        if (have) {
          uint32_t *W = H + (uint64_t)(w0 + lane) * 9;
          const uint32_t ns = 1 + inc;
          W[0] = h.k;
          W[3] = ns < kMaxSeeds ? ns : kMaxSeeds;
          W[4] = (uint32_t)h.len;
          W[5] = (uint32_t)h.G;
          W[7] = (uint32_t)h.beg;
          n_skip += skip;
          n_cont += !skip && !run;
          n_disc += discarded;
          n_run += run && !discarded;
        }
      }
      if (__ballot(overflow) && lane == 0) A.status[t] = 1;
    }
  }
  // the wave's counts
  unsigned long long v[6] = {n_run, n_cont, n_disc, n_skip, n_task, n_win};
  for (int k = 0; k < 6; ++k) {
    unsigned long long x = v[k];
    for (int d = 32; d; d >>= 1) x += __shfl_down(x, d);
    if (lane == 0 && x) atomicAdd(A.ctr + 1 + k, x);
  }
}

}  // namespace

uint32_t bsw2_extend_lds_bytes(const Bsw2ExtArgs &a) { return (25u + a.lds_ring * 64u) * 4u; }

hipError_t launch_bsw2_extend(const Bsw2ExtArgs &a, bool all_lds, int waves, hipStream_t st) {
  if (a.n_tasks <= 0 || a.n_hits <= 0) return hipSuccess;
  if (all_lds) hipLaunchKernelGGL(k_bsw2_extend<true>, dim3(waves), dim3(64), bsw2_extend_lds_bytes(a), st, a);
  else hipLaunchKernelGGL(k_bsw2_extend<false>, dim3(waves), dim3(64), bsw2_extend_lds_bytes(a), st, a);
  return hipGetLastError();
}

}  // namespace ibwa
