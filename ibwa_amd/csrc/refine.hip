// refine.hip -- the packed reference in HBM and the two halves of bwa_refine_gapped (bwase.c:333-416)
// that read it: the windows and CIGAR fix-ups of refine_gapped_core (bwase.c:167-221) around the
// global fill of sw.hip, and bwa_cal_md1 (bwase.c:243-295).
//
// The resident sequence is the set's references 2-bit packed back to back (base g of the set at bits
// 7-6 .. 1-0 of byte g / 4, the .pac layout of bntseq.c continued across the references), read as
// 32-bit words of 16 bases.  A reference after the first starts at a base offset that is in general
// no multiple of 4, so the concatenation shifts (k_pac_concat).
//
// Kernels: k_pac_concat (one output word per lane), k_pac_gather / k_refine_gather (one window per
// wave, a base per lane and step: the window's bytes are one contiguous segment), k_refine_fixup (one
// job per lane, a few CIGAR words), k_md<false / true> (one read per lane: a sizing pass and a
// writing pass around an exclusive scan of the text sizes).  All are memory / latency bound and small
// next to k_sw; none uses LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include <rocprim/rocprim.hpp>

#include "engine.h"

namespace ibwa {

namespace {

// base g of the resident sequence from word g / 16
__device__ __forceinline__ uint32_t pac_code(uint32_t word, uint64_t g) {
  return (word >> (8u * ((uint32_t)(g >> 2) & 3u) + 6u - 2u * ((uint32_t)g & 3u))) & 3u;
}

// consecutive bases: one load per 16
struct PacReader {
  const uint32_t *p;
  uint64_t w = ~0ull;
  uint32_t v = 0;
  __device__ __forceinline__ uint32_t at(uint64_t g) {
    const uint64_t i = g >> 4;
    if (i != w) {
      w = i;
      v = p[i];
    }
    return pac_code(v, g);
  }
};

__global__ void __launch_bounds__(256) k_pac_concat(const uint8_t *src, const uint64_t *byte_off, const uint64_t *base_off,
                                                    int n_db, uint32_t *out, uint64_t out_words) {
  const uint64_t total = base_off[n_db];
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < out_words; w += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t v = 0;
    int d = 0;
    for (int k = 0; k < 16; ++k) {
      const uint64_t g = w * 16 + k;
      if (g >= total) break;
      while (d + 1 < n_db && g >= base_off[d + 1]) ++d;  // an empty reference is skipped
      const uint64_t x = g - base_off[d];
      const uint32_t code = (src[byte_off[d] + (x >> 2)] >> (6u - 2u * ((uint32_t)x & 3u))) & 3u;
      v |= code << (8u * ((uint32_t)(k >> 2)) + 6u - 2u * ((uint32_t)k & 3u));
    }
    out[w] = v;
  }
}

// bases [beg, beg + len) before l_pac, 1 B each, by the lanes of one wave; returns the count
__device__ __forceinline__ uint32_t gather_wave(const uint32_t *pac, uint64_t l_pac, uint64_t beg, uint32_t len, uint8_t *out,
                                                int lane) {
  if (beg >= l_pac) return 0;
  const uint32_t got = (uint32_t)(l_pac - beg < (uint64_t)len ? l_pac - beg : (uint64_t)len);
  for (uint32_t k = (uint32_t)lane; k < got; k += 64) {
    const uint64_t g = beg + k;
    out[k] = (uint8_t)pac_code(pac[g >> 4], g);
  }
  return got;
}

__global__ void __launch_bounds__(256) k_pac_gather(const uint32_t *pac, uint64_t l_pac, int64_t n, const uint64_t *beg,
                                                    const uint32_t *len, const uint64_t *out_off, uint8_t *out, uint32_t *got) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < n; p += stride) {
    const uint32_t g = gather_wave(pac, l_pac, beg[p], len[p], out + out_off[p], lane);
    if (lane == 0) got[p] = g;
  }
}

// the window rule of refine_gapped_core (bwase.c:185-192, is_end_correct = 1) and the window's bases
// (dbset_extract_sequence, clipped at l_pac) into the buffer the global fill reads
__global__ void __launch_bounds__(256) k_refine_gather(const uint32_t *pac, uint64_t l_pac, int64_t n, const uint64_t *pos,
                                                       const int32_t *ext, const uint32_t *len, const uint64_t *off1,
                                                       uint8_t *seq1, uint32_t *len1) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < n; p += stride) {
    const int64_t ps = (int64_t)pos[p], l = (int64_t)len[p];
    const int e = ext[p];
    int64_t ref_len = l + (e < 0 ? -(int64_t)e : (int64_t)e), ref_start;
    if (e > 0) {
      ref_start = ps;
    } else {
      const int64_t x = ps + l;
      ref_start = x - ref_len > 0 ? x - ref_len : 0;
      ref_len = x - ref_start;
    }
    const uint32_t g = gather_wave(pac, l_pac, (uint64_t)ref_start, (uint32_t)ref_len, seq1 + off1[p], lane);
    if (lane == 0) len1[p] = g;
  }
}

constexpr uint32_t OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 3;
__device__ __forceinline__ uint32_t c_op(uint32_t c) { return c >> 29; }  // bwa_cigar_t (bwtaln.h:44-49)
__device__ __forceinline__ uint32_t c_len(uint32_t c) { return c & 0x1fffffffu; }

// bwa_aln_path2cigar's encoding of row p's CIGAR, then the fix-ups of bwase.c:201-218; the row is
// rewritten from its first word, n_cigar and pos_out get the results
__global__ void __launch_bounds__(256) k_refine_fixup(int64_t n, const uint64_t *pos, const int32_t *ext, uint32_t *cig, int cap,
                                                      int32_t *n_cigar, uint64_t *pos_out) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    uint32_t *c = cig + (uint64_t)p * cap;
    const int m = n_cigar[p];
    int64_t ps = (int64_t)pos[p], shift = 0;
    for (int k = 0; k < m; ++k) {
      const uint32_t w = c[k], op = w & 0xfu, l = w >> 4;
      c[k] = op << 29 | l;
      if (op == OP_D) shift -= l;
      else if (op == OP_I) shift += l;
    }
    if (ext[p] < 0) ps += shift;  // the coordinate of a forward-strand read
    int b = 0, e = m;
    if (e > b && c_op(c[b]) == OP_D) {  // deletion at the 5'-end
      ps += c_len(c[b]);
      ++b;
    }
    if (e > b && c_op(c[e - 1]) == OP_D) --e;  // at the 3'-end
    if (e > b && c_op(c[e - 1]) == OP_I) c[e - 1] = OP_S << 29 | c_len(c[e - 1]);
    if (e > b && c_op(c[b]) == OP_I) c[b] = OP_S << 29 | c_len(c[b]);
    if (b > 0)
      for (int k = b; k < e; ++k) c[k - b] = c[k];
    n_cigar[p] = e - b;
    pos_out[p] = (uint64_t)ps;
  }
}

// the MD text of one read: counted (W = false) or written (W = true)
template <bool W>
struct MdText {
  char *t;
  uint64_t n = 0;
  __device__ __forceinline__ void ch(char c) {
    if (W) t[n] = c;
    ++n;
  }
  __device__ __forceinline__ void num(uint32_t u) {  // "%d" of a count
    int d = 1;
    for (uint32_t v = u; v >= 10; v /= 10) ++d;
    if (W)
      for (int k = d - 1; k >= 0; --k) {
        t[n + k] = (char)('0' + u % 10);
        u /= 10;
      }
    n += d;
  }
};

// bwa_cal_md1 (bwase.c:243-295) of read p
template <bool W>
__global__ void __launch_bounds__(256) k_md(MdArgs A) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < A.n; p += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t *seq = A.seq + A.off[p];
    const uint64_t l_pac = A.l_pac;
    PacReader R{A.pac};
    MdText<W> T{W ? A.text + A.text_off[p] : nullptr};
    uint64_t x = A.pos[p], y = 0;
    uint32_t u = 0, c = 0;
    int nm = 0;
    // bases [at, at + l) before l_pac
    auto run = [&](uint64_t at, uint32_t l) -> uint32_t {
      if (at >= l_pac) return 0u;
      return (uint32_t)(l_pac - at < (uint64_t)l ? l_pac - at : (uint64_t)l);
    };
    auto cmp = [&](uint32_t s) {  // the reference base c against read code s
      if (s > 3 || c != s) {
        T.num(u);
        T.ch("ACGT"[c]);
        ++nm;
        u = 0;
      } else {
        ++u;
      }
    };
    const int nc = A.n_cigar ? A.n_cigar[p] : -1;
    if (nc >= 0) {
      const uint32_t *cg = A.cigar + A.cig_off[p];
      for (int k = 0; k < nc; ++k) {
        const uint32_t l = c_len(cg[k]), op = c_op(cg[k]);
        if (op == OP_M) {
          const uint32_t m = run(x, l);
          for (uint32_t z = 0; z < m; ++z) {
            c = R.at(x + z);
            cmp(seq[y + z]);
          }
          x += l;
          y += l;
        } else if (op == OP_I || op == OP_S) {
          y += l;
          if (op == OP_I) nm += (int)l;
        } else if (op == OP_D) {
          T.num(u);
          T.ch('^');
          const uint32_t m = run(x, l);
          for (uint32_t z = 0; z < m; ++z) T.ch("ACGT"[R.at(x + z)]);
          u = 0;
          x += l;
          nm += (int)l;
        }
      }
    } else {
      // past l_pac nothing is extracted: c keeps the last base's value (0 when there was none)
      const uint32_t len = A.len[p], m = run(x, len);
      for (uint32_t z = 0; z < len; ++z) {
        if (z < m) c = R.at(x + z);
        cmp(seq[z]);
      }
    }
    T.num(u);
    T.ch('\0');
    if (W) {
      A.nm[p] = nm;
    } else {
      A.text_off[p] = T.n;  // sizes; the scan turns them into offsets
      if (p == 0) A.text_off[A.n] = 0;
    }
  }
}

int grid_for(int64_t items) { return (int)std::min<int64_t>(std::max<int64_t>((items + 255) / 256, 1), 16384); }

}  // namespace

hipError_t launch_pac_concat(const uint8_t *src, const uint64_t *byte_off, const uint64_t *base_off, int n_db, uint32_t *out,
                             uint64_t out_words, hipStream_t st) {
  if (out_words == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pac_concat, dim3(grid_for((int64_t)out_words)), dim3(256), 0, st, src, byte_off, base_off, n_db, out,
                     out_words);
  return hipGetLastError();
}

hipError_t launch_pac_gather(const uint32_t *pac, uint64_t l_pac, int64_t n, const uint64_t *beg, const uint32_t *len,
                             const uint64_t *out_off, uint8_t *out, uint32_t *got, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pac_gather, dim3(grid_for(n * 64)), dim3(256), 0, st, pac, l_pac, n, beg, len, out_off, out, got);
  return hipGetLastError();
}

hipError_t launch_refine_gather(const uint32_t *pac, uint64_t l_pac, int64_t n, const uint64_t *pos, const int32_t *ext,
                                const uint32_t *len, const uint64_t *off1, uint8_t *seq1, uint32_t *len1, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_refine_gather, dim3(grid_for(n * 64)), dim3(256), 0, st, pac, l_pac, n, pos, ext, len, off1, seq1, len1);
  return hipGetLastError();
}

hipError_t launch_refine_fixup(int64_t n, const uint64_t *pos, const int32_t *ext, uint32_t *cig, int cap, int32_t *n_cigar,
                               uint64_t *pos_out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_refine_fixup, dim3(grid_for(n)), dim3(256), 0, st, n, pos, ext, cig, cap, n_cigar, pos_out);
  return hipGetLastError();
}

hipError_t launch_md(const MdArgs &a, bool write, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  if (write) hipLaunchKernelGGL(k_md<true>, dim3(grid_for(a.n)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_md<false>, dim3(grid_for(a.n)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t md_scan_sizes(uint64_t *text_off, int64_t n, void *tmp, size_t *tmp_bytes, hipStream_t st) {
  return rocprim::exclusive_scan(tmp, *tmp_bytes, text_off, text_off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st);
}

}  // namespace ibwa
