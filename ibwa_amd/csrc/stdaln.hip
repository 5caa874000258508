// stdaln.hip -- batched pairwise alignment for a run-time AlnParam: aln_local_core (stdaln.c:529-760,
// with the suboptimal score) and aln_global_core (stdaln.c:345-525), as stdaln_core.h states them.
//
// One alignment per lane, one wave per workgroup, persistent grid with per-wave claiming (as k_sw).
// The score matrix is staged once per workgroup in LDS.  The local passes' eh row (len1 + 2 words per
// lane) lives in LDS too while 64 lanes' rows fit 40 KiB (StdArgs::eh_lds, engine_stdaln.hip), and in
// HBM scratch otherwise; in both it is lane-minor (element e of lane l at e * 64 + l), so a wave's
// step touches one contiguous segment / 64 different banks.  The rest of a lane's scratch is
// lane-minor HBM: suba (16 bits per row of seq2: every h is below 32768) while seq2 is short enough
// to keep it (StdArgs::keep_suba; past that the forward pass runs twice instead, stdaln_core.h),
// the global fill's two (M, I, D) rows, and one traceback byte per cell.  Integer VALU work with an
// LDS lookup per cell; unlike k_sw nothing is strip-mined into registers, because the strip
// boundaries cost 8 B per row of seq2, which here is the long sequence.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"
#include "stdaln_core.h"

namespace ibwa {

namespace {

using namespace stdaln;

template <bool EH_LDS>
__global__ void __launch_bounds__(64) k_stdaln(StdArgs A, unsigned long long *counter) {
  extern __shared__ uint32_t smem[];  // matrix (row * row), then the eh rows (EH_LDS)
  const int lane = threadIdx.x;
  int *mat = reinterpret_cast<int *>(smem);
  for (int k = lane; k < A.row * A.row; k += 64) mat[k] = A.matrix[k];
  __syncthreads();
  Param P;
  P.q = A.gap_open; P.r = A.gap_ext; P.gap_end = A.gap_end; P.band = A.band; P.row = A.row;
  P.max_score = A.max_score; P.mat = mat;
  // this wave's scratch: words [eh | mid | suba], lane-minor
  uint32_t *w = A.scratch + (uint64_t)blockIdx.x * A.words_per_lane * 64 + lane;
  View<uint32_t> eh;
  if (EH_LDS) { eh.p = smem + A.row * A.row + lane; eh.s = 64; } else { eh.p = w + (uint64_t)A.e_eh * 64; eh.s = 64; }
  View<uint32_t> mid{w + (uint64_t)A.e_mid * 64, 64};
  View<uint16_t> suba{reinterpret_cast<uint16_t *>(A.scratch + ((uint64_t)blockIdx.x * A.words_per_lane + A.e_suba) * 64) + lane, 64};
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
      if (A.band <= 0) P.band = n1 + n2;
      LocalOut o;
      if (A.type == 0) {
        local_core(eh, suba, A.keep_suba != 0, mid, A.mid_w, T, A.tb_per_lane, P, A.thres, a, n1, b, n2, cig, A.cigar_cap, o);
      } else {
        o.score = 0;
        o.subo = o.path_len = o.n_cig = o.s_i = o.s_j = o.e_i = o.e_j = 0;
        if (n1 > 0 && n2 > 0) {
          int si = 0, sj = 0;
          o.score = global_core(mid, A.mid_w, T, P, a, n1, b, n2, P.band, P.gap_end, cig, A.cigar_cap, o.n_cig,
                                o.path_len, si, sj);
          for (int k = 0; k < o.n_cig / 2; ++k) {
            const uint32_t t = cig[k];
            cig[k] = cig[o.n_cig - 1 - k];
            cig[o.n_cig - 1 - k] = t;
          }
          o.s_i = si; o.s_j = sj; o.e_i = n1; o.e_j = n2;
        }
      }
      A.score[p] = o.score;
      A.subo[p] = o.subo;
      A.path_len[p] = o.path_len;
      A.n_cigar[p] = o.n_cig;
      A.ends[p] = make_int4(o.s_i, o.s_j, o.e_i, o.e_j);
    }
  }
}

}  // namespace

uint32_t stdaln_lds_bytes(const StdArgs &a, bool eh_lds) {
  return (uint32_t)(a.row * a.row) * 4u + (eh_lds ? (uint32_t)(a.max_len1 + 2) * 64u * 4u : 0u);
}

hipError_t launch_stdaln(const StdArgs &a, unsigned long long *d_counter, int waves, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipError_t e = zero_async(d_counter, sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  if (a.eh_lds)
    hipLaunchKernelGGL(k_stdaln<true>, dim3(waves), dim3(64), stdaln_lds_bytes(a, true), st, a, d_counter);
  else
    hipLaunchKernelGGL(k_stdaln<false>, dim3(waves), dim3(64), stdaln_lds_bytes(a, false), st, a, d_counter);
  return hipGetLastError();
}

}  // namespace ibwa
