// cs2nt.hip -- colour space to nucleotides on the device: bwa_pac2cspac_core (bwtmisc.c:202-219) and
// bwa_cs2nt_core's row construction (cs2nt.c:136-171), cs2nt_DP (:37-78) and cs2nt_nt_qual (:84-110).
//
// k_pac2cs: one lane per word of 16 bases of the packed sequence (refine.hip's layout: base g at bits
// 7-6 .. 1-0 of byte g / 4).  Colour i >= 1 is nst_color_space_table[1 << c1 | 1 << c2], which on two
// 2-bit codes is c1 ^ c2; symbol 0 is base 0 itself.  A word's colours are the word xor the word moved
// one base on, with the previous word's last base carried in; every bit past l_pac is cleared.
//
// k_cs2nt<Rows>: one read per lane.  Rows hands out the row pair position by position: nt_ref[k]
// (codes 0-4) and cs_read[k - 1] (colour << 6 | qual, qual == 63 for an N colour), either from the
// caller's arrays (HostRows) or built from the resident nucleotide sequence and the hit's CIGAR
// (PacRows, cs2nt.c:136-171), so the DP and the row construction are one kernel.  The two score rows
// h[0..3] stay in registers.  Each step's four back-pointers (2 bits each) are one byte and the step's
// colour byte another, in position-major scratch (bt[k * lanes + lane], cs[k * lanes + lane]): a
// wave's store and its later load are one contiguous 64 B segment.  The traceback walks backwards with
// a window of three decoded bases and emits cs2nt_nt_qual's t2array[k] in the same pass.
//
// A base at or past l_pac is not defined by the reference (dbset_extract_sequence stops at l_pac and
// bwa_cs2nt_core's buffer is uninitialised there): PacRows returns 4 for it, "no base known".
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "engine.h"

namespace ibwa {

namespace {

__global__ void __launch_bounds__(256) k_pac2cs(const uint32_t *nt, uint64_t l_pac, uint32_t *cs, uint64_t words) {
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = nt[w];
    const uint32_t carry = w ? (nt[w - 1] >> 24) & 3u : 0u;  // the last base of the previous word
    // base i - 1 at base i's place: inside a byte two bits down, across bytes from the byte before
    const uint32_t prev = ((v >> 2) & 0x3f3f3f3fu) | ((v & 0x00030303u) << 14) | (carry << 6);
    uint32_t c = v ^ prev;
    const uint64_t first = w * 16;
    if (l_pac < first + 16) {  // the last word: nothing past l_pac
      const uint32_t nb = l_pac > first ? (uint32_t)(l_pac - first) : 0u;
      uint32_t mask = 0;
      for (uint32_t k = 0; k < nb; ++k) mask |= 3u << (8u * (k >> 2) + 6u - 2u * (k & 3u));
      c &= mask;
    }
    cs[w] = c;
  }
}

constexpr int COLOR_MM = 19, NUCL_MM = 25;  // cs2nt.c:25-26

// the caller's row pair of job p: nt_ref[0 .. size], cs_read[0 .. size - 1]
struct HostRows {
  const uint8_t *ref, *cs;
  __device__ __forceinline__ HostRows(const Cs2ntArgs &A, int64_t p) : ref(A.nt_ref + A.off[p]), cs(A.cs_read + A.off[p]) {}
  __device__ __forceinline__ uint32_t first() { return *ref++; }
  __device__ __forceinline__ void next(uint32_t &r, uint32_t &c) {
    r = *ref++;
    c = *cs++;
  }
};

constexpr uint32_t OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 3;  // bwa_cigar_t (bwtaln.h:44-49)

// the row pair bwa_cs2nt_core builds for read p (cs2nt.c:136-171)
struct PacRows {
  const uint32_t *pac;
  uint64_t l_pac, x;      // x: the reference cursor
  uint64_t pw = ~0ull;    // the loaded word of the sequence
  uint32_t pv = 0;
  const uint8_t *seq, *qual;
  const uint32_t *cg;
  uint32_t len, y = 0;    // y: the read cursor
  int nc, k = 0;          // CIGAR words, the next one
  uint32_t run = 0, op = OP_M;  // what is left of the current M / I run
  bool strand;
  __device__ __forceinline__ PacRows(const Cs2ntArgs &A, int64_t p)
      : pac(A.pac), l_pac(A.l_pac), x(A.pos[p]), seq(A.seq + A.off[p]), qual(A.qual + A.off[p]),
        cg(A.cigar + A.cig_off[p]), len(A.len[p]), nc(A.n_cigar[p]), strand(A.strand[p] != 0) {
    if (nc <= 0) run = len;  // no gap or clipping: one M run of the whole read
  }
  __device__ __forceinline__ uint32_t base(uint64_t g) {
    if (g >= l_pac) return 4u;
    if ((g >> 4) != pw) {
      pw = g >> 4;
      pv = pac[pw];
    }
    return (pv >> (8u * ((uint32_t)(g >> 2) & 3u) + 6u - 2u * ((uint32_t)g & 3u))) & 3u;
  }
  __device__ __forceinline__ uint32_t first() { return x ? base(x - 1) : 4u; }
  __device__ __forceinline__ void next(uint32_t &r, uint32_t &c) {
    while (run == 0 && k < nc) {  // S skips read colours, D skips reference bases
      const uint32_t w = cg[k++], l = w & 0x1fffffffu;
      op = w >> 29;
      if (op == OP_M || op == OP_I) run = l;
      else if (op == OP_S) y += l;
      else if (op == OP_D) x += l;
    }
    --run;
    if (op == OP_M) r = base(x++);
    else r = 4u;
    // __gen_csbase (cs2nt.c:129-134)
    const uint32_t s = seq[y];
    int q = (int)qual[strand ? len - 1 - y : y] - 33;
    if (q > 60) q = 60;
    if (s > 3) q = 63;
    c = (uint8_t)(s << 6 | (uint32_t)q);
    ++y;
  }
};

template <class Rows>
__global__ void __launch_bounds__(256) k_cs2nt(Cs2ntArgs A) {
  const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // < A.lanes by the launch
  const int64_t p = A.first + lane;
  if (p >= A.n) return;
  const int size = (int)A.size[p];
  uint8_t *bt = A.bt + lane, *cs = A.cs + lane;
  const uint64_t L = (uint64_t)A.lanes;
  Rows R(A, p);
  // recursion: initial value (cs2nt.c:45-49)
  int h0, h1, h2, h3;
  {
    const uint32_t r = R.first();
    h0 = r >= 4 || r == 0 ? 0 : NUCL_MM;
    h1 = r >= 4 || r == 1 ? 0 : NUCL_MM;
    h2 = r >= 4 || r == 2 ? 0 : NUCL_MM;
    h3 = r >= 4 || r == 3 ? 0 : NUCL_MM;
  }
  for (int k = 1; k <= size; ++k) {
    uint32_t r, c;
    R.next(r, c);
    const uint32_t col = c >> 6, q = c & 0x3fu;
    const int pen = q == 63 ? 0 : (q < (uint32_t)COLOR_MM ? COLOR_MM : (int)q);  // colour mismatch (:57-58)
    const int h[4] = {h0, h1, h2, h3};
    int g[4];
    uint32_t b = 0;
#pragma unroll
    for (uint32_t x = 0; x < 4; ++x) {
      int mn = 0x7fffffff;
      uint32_t ymin = 0;
#pragma unroll
      for (uint32_t y = 0; y < 4; ++y) {  // s < min with y ascending (:60)
        const int s = h[y] + (col != (x ^ y) ? pen : 0);
        if (s < mn) {
          mn = s;
          ymin = y;
        }
      }
      // the nucleotide penalty (:59) is the same for every y: it moves no minimum
      g[x] = mn + (r < 4 && r != x ? NUCL_MM : 0);
      b |= ymin << (2 * x);
    }
    h0 = g[0], h1 = g[1], h2 = g[2], h3 = g[3];
    bt[(uint64_t)k * L] = (uint8_t)b;
    cs[(uint64_t)(k - 1) * L] = (uint8_t)c;
  }
  // back trace: the first minimal x (:69-74)
  uint32_t n2 = 0;
  {
    int hmin = h0;
    if (h1 < hmin) hmin = h1, n2 = 1;
    if (h2 < hmin) hmin = h2, n2 = 2;
    if (h3 < hmin) hmin = h3, n2 = 3;
  }
  // n0, n1, n2 = nt_read[k - 1], [k], [k + 1]; c1 = cs_read[k]; cs2nt_nt_qual's t2array[k] (:95-108)
  uint8_t *out = A.out + A.out_off[p];
  uint32_t n1 = (bt[(uint64_t)size * L] >> (2 * n2)) & 3u;
  uint32_t c1 = cs[(uint64_t)(size - 1) * L];
  for (int k = size - 1; k >= 1; --k) {
    const uint32_t n0 = (bt[(uint64_t)k * L] >> (2 * n1)) & 3u;
    const uint32_t c0 = cs[(uint64_t)(k - 1) * L];
    const int q0 = (int)(c0 & 0x3fu), q1 = (int)(c1 & 0x3fu);
    const bool m0 = (n0 ^ n1) == (c0 >> 6), m1 = (n1 ^ n2) == (c1 >> 6);
    int q = m0 && m1 ? q0 + q1 + 10 : m0 ? q0 - q1 : m1 ? q1 - q0 : 0;
    q = q < 0 ? 0 : q > 60 ? 60 : q;
    out[k - 1] = q0 == 63 || q1 == 63 ? (uint8_t)0 : (uint8_t)(n1 << 6 | (uint32_t)q);
    n2 = n1;
    n1 = n0;
    c1 = c0;
  }
}

int grid_for(int64_t items) { return (int)std::min<int64_t>(std::max<int64_t>((items + 255) / 256, 1), 16384); }

}  // namespace

hipError_t launch_pac2cs(const uint32_t *nt, uint64_t l_pac, uint32_t *cs, uint64_t words, hipStream_t st) {
  if (words == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pac2cs, dim3(grid_for((int64_t)words)), dim3(256), 0, st, nt, l_pac, cs, words);
  return hipGetLastError();
}

hipError_t launch_cs2nt(const Cs2ntArgs &a, bool from_pac, hipStream_t st) {
  if (a.lanes <= 0 || a.first >= a.n) return hipSuccess;
  const dim3 grid((unsigned)(a.lanes / 256)), block(256);  // lanes is a multiple of 256
  if (from_pac) hipLaunchKernelGGL(k_cs2nt<PacRows>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(k_cs2nt<HostRows>, grid, block, 0, st, a);
  return hipGetLastError();
}

}  // namespace ibwa
