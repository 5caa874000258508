// extend.hip -- batched seed extension: aln_extend_core (stdaln.c:862-1008) for a run-time AlnParam, as
// stdaln_core.h states it, and the gather of the seeds' target windows from the resident reference.
//
// k_extend maps as k_stdaln does: one alignment per lane, one wave per workgroup, persistent grid with
// per-wave claiming, the score matrix staged once per workgroup in LDS.  The eh row is a ring of
// 2 * band + 2 words (stdaln_core.h: extend_ring), lane-minor (word e of lane l at e * 64 + l), in LDS
// for every pair whose ring is at most ExtArgs::lds_ring words and in the wave's HBM scratch for the
// others -- with the bwa band of 50 that is 102 words, 26 KiB per wave, at any length.  A launch in
// which every ring fits (ALL_LDS) addresses the ring as LDS; a mixed launch chooses per lane, through
// a generic pointer.  Score-only and end-cell mode touch no other scratch; path mode runs the global
// fill over the (M, I, D) rows and the traceback bytes of the wave's HBM scratch, as k_stdaln does.
// Integer VALU work with one LDS lookup and one ring word read and written per cell.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "engine.h"
#include "stdaln_core.h"

namespace ibwa {

namespace {

using namespace stdaln;

template <bool ALL_LDS>
__global__ void __launch_bounds__(64) k_extend(ExtArgs A, unsigned long long *counter) {
  extern __shared__ uint32_t smem[];  // matrix (row * row), then lds_ring ring words per lane
  const int lane = threadIdx.x;
  int *mat = reinterpret_cast<int *>(smem);
  for (int k = lane; k < A.row * A.row; k += 64) mat[k] = A.matrix[k];
  __syncthreads();
  Param P;
  P.q = A.gap_open; P.r = A.gap_ext; P.gap_end = -1; P.band = A.band; P.row = A.row;
  P.max_score = A.max_score; P.mat = mat;
  // this wave's scratch: words [eh | mid], lane-minor
  uint32_t *w = A.scratch + (uint64_t)blockIdx.x * A.words_per_lane * 64 + lane;
  const View<uint32_t> eh_lds{smem + A.row * A.row + lane, 64};
  View<uint32_t> mid{w + (uint64_t)A.e_mid * 64, 64};
  TbView T{A.tb + (uint64_t)blockIdx.x * A.tb_per_lane * 64, 64u, (uint32_t)lane};
  int64_t cur = 0, cend = 0;
  for (;;) {
    if (cur >= cend) {
      int64_t base = 0;
      if (lane == 0) base = (int64_t)atomicAdd(counter, 64ull);
      base = __shfl(base, 0);
      if (base >= A.n) break;
      cur = base;
      cend = base + 64 < A.n ? base + 64 : A.n;
    }
    const int64_t p = cur + lane;
    cur = cend;
    if (p < cend) {  // the group's tail lanes idle; every lane comes back to the claim together
      const int n1 = (int)A.len1[p], n2 = (int)A.len2[p];
      const uint8_t *a = A.seq1 + A.off1[p];
      const uint8_t *b = A.seq2 + A.off2[p];
      uint32_t *cig = A.cigar + (uint64_t)p * A.cigar_cap;
      P.band = extend_band(A.band, n1, n2);
      const uint32_t R = extend_ring(P.band, n1);
      const int G0 = A.g0 ? A.g0[p] : 1;
      ExtOut o;
      if (ALL_LDS) {
        extend_core(eh_lds, R, mid, A.mid_w, T, A.tb_per_lane, P, A.mode, G0, a, n1, b, n2, cig, A.cigar_cap, o);
      } else {
        const View<uint32_t> eh = R <= A.lds_ring ? eh_lds : View<uint32_t>{w, 64};
        extend_core(eh, R, mid, A.mid_w, T, A.tb_per_lane, P, A.mode, G0, a, n1, b, n2, cig, A.cigar_cap, o);
      }
      A.score[p] = o.score;
      A.no_band[p] = o.no_band;
      A.path_len[p] = o.path_len;
      A.n_cigar[p] = o.n_cig;
      A.ends[p] = make_int4(o.s_i, o.s_j, o.end_i, o.end_j);
    }
  }
}

// base g of the resident sequence from word g / 16 (the layout of refine.hip)
__device__ __forceinline__ uint32_t pac_code(uint32_t word, uint64_t g) {
  return (word >> (8u * ((uint32_t)(g >> 2) & 3u) + 6u - 2u * ((uint32_t)g & 3u))) & 3u;
}

// one window per wave, a base per lane and step
__global__ void __launch_bounds__(256) k_extend_gather(const uint32_t *pac, uint64_t l_pac, int rev, int64_t n,
                                                       const uint64_t *pos, const uint8_t *dir, const uint64_t *off1,
                                                       const uint32_t *len1, uint8_t *seq1) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < n; p += stride) {
    const uint64_t ps = pos[p];
    const uint32_t len = len1[p];
    const bool left = dir[p] != 0;
    uint8_t *out = seq1 + off1[p];
    for (uint32_t k = lane; k < len; k += 64) {
      const uint64_t x = left ? ps - 1 - k : ps + k;  // the host clipped len: 0 <= x < l_pac
      const uint64_t g = rev ? l_pac - x - 1 : x;
      out[k] = (uint8_t)pac_code(pac[g >> 4], g);
    }
  }
}

}  // namespace

uint32_t extend_lds_bytes(const ExtArgs &a) { return ((uint32_t)(a.row * a.row) + a.lds_ring * 64u) * 4u; }

hipError_t launch_extend(const ExtArgs &a, bool all_lds, unsigned long long *d_counter, int waves, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipError_t e = zero_async(d_counter, sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  if (all_lds) hipLaunchKernelGGL(k_extend<true>, dim3(waves), dim3(64), extend_lds_bytes(a), st, a, d_counter);
  else hipLaunchKernelGGL(k_extend<false>, dim3(waves), dim3(64), extend_lds_bytes(a), st, a, d_counter);
  return hipGetLastError();
}

hipError_t launch_extend_gather(const uint32_t *pac, uint64_t l_pac, int rev, int64_t n, const uint64_t *pos, const uint8_t *dir,
                                const uint64_t *off1, const uint32_t *len1, uint8_t *seq1, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>((n + 3) / 4, 1 << 16);
  hipLaunchKernelGGL(k_extend_gather, dim3((unsigned)blocks), dim3(256), 0, st, pac, l_pac, rev, n, pos, dir, off1, len1, seq1);
  return hipGetLastError();
}

}  // namespace ibwa
