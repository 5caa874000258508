// extend_core_check.cpp -- TEST INFRASTRUCTURE: stdaln_core.h's extend_core instantiated on the host
// (stride 1) against the compiled reference's aln_extend_core / aln_path2cigar32, loaded from the shared
// library named on the command line.  Every pair runs in all three modes (score only, end cell,
// path), once with the eh ring of extend_ring() words and once with the whole len1 + 2 array; the two
// must agree with each other and with the reference.  Random pairs over five schemes, bands 1, 2, 3,
// random, 50 and the full matrix, G0 of 1, mid-size and beyond any gain; then the fixed classes: 1 x 1,
// 1 x n, n x 1, len1 >> len2 and the reverse, N codes, long gaps under a cheap scheme, and pairs of
// about 3 000 near-identical bases whose score passes 32000 (the rebasing of stdaln.c:917-930).
//   usage: extend_core_check <libibwa_ref.so> <pairs>      exit status 0: all equal
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "stdaln_core.h"

using namespace ibwa::stdaln;

// the reference's interface (stdaln.h)
struct RefParam { int gap_open, gap_ext, gap_end; int *matrix; int row, band_width; };
struct RefPath { int i, j; unsigned char ctype; };
typedef int (*extend_fn)(unsigned char *, int, unsigned char *, int, const RefParam *, RefPath *, int *, int, uint8_t *);
typedef uint32_t *(*cigar_fn)(const RefPath *, int, int *);

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 11); }

static extend_fn ref_extend;
static cigar_fn ref_cigar;
static long n_rebased, n_no_band, n_ring;

struct Res {
  int score[3], end_i, end_j, path_len, n_cig, s_i, s_j, no_band;
  std::vector<uint32_t> cig;
  bool operator==(const Res &o) const {
    return !memcmp(score, o.score, sizeof score) && end_i == o.end_i && end_j == o.end_j && path_len == o.path_len &&
           n_cig == o.n_cig && s_i == o.s_i && s_j == o.s_j && no_band == o.no_band && cig == o.cig;
  }
};

static Res run_mine(const RefParam &ap, int G0, const std::vector<uint8_t> &a, const std::vector<uint8_t> &b, bool ring) {
  const int n1 = (int)a.size(), n2 = (int)b.size();
  Param P = {ap.gap_open, ap.gap_ext, ap.gap_end, extend_band(ap.band_width, n1, n2), ap.row, 0, ap.matrix};
  const uint32_t R = ring ? extend_ring(P.band, n1) : (uint32_t)n1 + 2;
  const uint64_t w1 = extend_span1(P.band, n1, n2), w2 = extend_span2(P.band, n1, n2);
  const uint32_t W = (uint32_t)w1 + 1;
  // the ring is filled with garbage first: nothing may depend on what it held
  std::vector<uint32_t> eh(R, 0xDEADBEEFu), mid(6 * (size_t)W), cig(w1 + w2 + 2);
  std::vector<uint8_t> tb((w1 + 1) * (w2 + 1) + 8);
  View<uint32_t> EH{eh.data(), 1}, MID{mid.data(), 1};
  TbView T{tb.data(), 1, 0};
  Res r = {};
  for (int mode = 0; mode < 3; ++mode) {
    ExtOut o;
    std::fill(eh.begin(), eh.end(), 0xDEADBEEFu);
    extend_core(EH, R, MID, W, T, (w1 + 1) * (w2 + 1), P, mode, G0, a.data(), n1, b.data(), n2, cig.data(), (int)(w1 + w2), o);
    r.score[mode] = o.score;
    if (mode == 1) { r.end_i = o.end_i; r.end_j = o.end_j; }
    if (mode == 2) {
      r.path_len = o.path_len; r.n_cig = o.n_cig; r.s_i = o.s_i; r.s_j = o.s_j; r.no_band = o.no_band;
      r.cig.assign(cig.begin(), cig.begin() + o.n_cig);
    }
  }
  return r;
}

static bool check(RefParam ap, int G0, std::vector<uint8_t> &a, std::vector<uint8_t> &b, const char *what) {
  const int n1 = (int)a.size(), n2 = (int)b.size();
  const int given = ap.band_width;
  if (ap.band_width <= 0) ap.band_width = n1 + n2;  // the library's convention; the reference takes the number as it is
  Res want = {};
  std::vector<RefPath> path(n1 + n2 + 2);
  want.score[0] = ref_extend(a.data(), n1, b.data(), n2, &ap, nullptr, nullptr, G0, nullptr);
  path[0].i = path[0].j = 0;
  want.score[1] = ref_extend(a.data(), n1, b.data(), n2, &ap, path.data(), nullptr, G0, nullptr);
  if (want.score[1] > 0) { want.end_i = path[0].i; want.end_j = path[0].j; }
  int rpl = 0, rnc = 0;
  want.score[2] = ref_extend(a.data(), n1, b.data(), n2, &ap, path.data(), &rpl, G0, nullptr);
  if (n1 && n2 && want.score[0] > 0) {
    uint32_t *rc = ref_cigar(path.data(), rpl, &rnc);
    want.path_len = rpl; want.n_cig = rnc;
    want.cig.assign(rc, rc + rnc);
    want.s_i = path[rpl - 1].i; want.s_j = path[rpl - 1].j;
    want.no_band = want.score[0] > want.score[2];
    free(rc);
  }
  ap.band_width = given;
  const Res ring = run_mine(ap, G0, a, b, true), full = run_mine(ap, G0, a, b, false);
  const int band = extend_band(given, n1, n2);
  if (extend_ring(band, n1) < (uint32_t)n1 + 2) ++n_ring;
  if (want.score[0] > 32000 - 1) ++n_rebased;
  if (want.no_band) ++n_no_band;
  const bool ok = ring == want && full == want;
  if (!ok)
    printf("BAD %s %d x %d band %d G0 %d q %d r %d: score %d/%d/%d ring %d/%d/%d full %d/%d/%d end %d,%d ring %d,%d path_len %d ring %d\n",
           what, n1, n2, given, G0, ap.gap_open, ap.gap_ext, want.score[0], want.score[1], want.score[2], ring.score[0],
           ring.score[1], ring.score[2], full.score[0], full.score[1], full.score[2], want.end_i, want.end_j, ring.end_i,
           ring.end_j, want.path_len, ring.path_len);
  return ok;
}

// b = a noisy copy of a: substitutions, and indels of up to `gap` symbols
static std::vector<uint8_t> noisy(const std::vector<uint8_t> &a, int alpha, int sub_in, int indel_in, int gap) {
  std::vector<uint8_t> b;
  for (size_t i = 0; i < a.size(); ++i) {
    if (indel_in && rnd() % indel_in == 0) {
      const int g = 1 + rnd() % gap;
      if (rnd() & 1) { i += g - 1; continue; }
      for (int k = 0; k < g; ++k) b.push_back(rnd() % alpha);
    }
    b.push_back(sub_in && rnd() % sub_in == 0 ? rnd() % alpha : a[i]);
  }
  return b;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  void *h = dlopen(argv[1], RTLD_LAZY);
  if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
  ref_extend = (extend_fn)dlsym(h, "aln_extend_core");
  ref_cigar = (cigar_fn)dlsym(h, "aln_path2cigar32");
  const RefParam *presets[3] = {(RefParam *)dlsym(h, "aln_param_blast"), (RefParam *)dlsym(h, "aln_param_aa2aa"),
                                (RefParam *)dlsym(h, "aln_param_bwa")};
  if (!ref_extend || !ref_cigar || !presets[0] || !presets[1] || !presets[2]) return 2;
  static int m5[25], msw[25];
  for (int x = 0; x < 5; ++x)
    for (int y = 0; y < 5; ++y) {
      m5[x * 5 + y] = x == y ? 5 : -2;
      msw[x * 5 + y] = (x == y && x < 4) ? 1 : -3;
    }
  const RefParam cheap = {10, 2, 2, m5, 5, 50}, sw2 = {5, 2, 2, msw, 5, 50};
  const int pairs = atoi(argv[2]);
  long nbad = 0, total = 0;
  for (int it = 0; it < pairs; ++it) {
    RefParam ap = it % 5 == 3 ? cheap : it % 5 == 4 ? sw2 : *presets[it % 5];
    const int alpha = ap.row == 22 ? 20 : 4;
    const int n1 = 1 + rnd() % (it % 7 == 0 ? 400 : 80);
    std::vector<uint8_t> a(n1), b;
    const int eff = (it % 11 == 0) ? 2 : alpha;  // low complexity: ties between cells
    for (auto &x : a) x = rnd() % eff;
    if (it % 6 == 5) {  // unrelated
      b.resize(1 + rnd() % 80);
      for (auto &x : b) x = rnd() % eff;
    } else {
      b = noisy(a, eff, 4 + rnd() % 30, it % 3 ? 10 + rnd() % 40 : 0, 1 + rnd() % 12);
      if (b.empty()) b.push_back(a[0]);
      const int cut = rnd() % 4;  // len1 >> len2 and the reverse
      if (cut == 0 && b.size() > 8) b.resize(1 + rnd() % (b.size() / 4));
      if (cut == 1 && a.size() > 8) a.resize(1 + rnd() % (a.size() / 4));
    }
    if (ap.row == 5 && it % 13 == 0) a[rnd() % a.size()] = 4;  // N
    if (ap.row == 5 && it % 17 == 0) b[rnd() % b.size()] = 4;
    const int bs = rnd() % 7;
    ap.band_width = bs == 0 ? 0 : bs == 1 ? 1 : bs == 2 ? 2 : bs == 3 ? 3 : bs == 4 ? 50 : bs == 5 ? 1 + rnd() % 50 : -1;
    const int gs = rnd() % 4;
    const int G0 = gs < 2 ? 1 : gs == 2 ? 2 + rnd() % 60 : 20000 + rnd() % 12001;
    ++total;
    if (!check(ap, G0, a, b, "random")) ++nbad;
  }
  // the fixed classes
  {
    std::vector<uint8_t> x1 = {2}, y1 = {2}, z1 = {1}, e;
    for (int band : {1, 2, 3, 50, 0}) {
      RefParam ap = *presets[0];
      ap.band_width = band;
      total += 5;
      nbad += !check(ap, 1, x1, y1, "1x1 match") + !check(ap, 1, x1, z1, "1x1 mismatch") + !check(ap, 7, x1, z1, "1x1 G0") +
              !check(ap, 1, e, x1, "empty seq1") + !check(ap, 1, x1, e, "empty seq2");
      std::vector<uint8_t> l(200), one = {3};
      for (auto &v : l) v = rnd() % 4;
      one[0] = l[0];
      total += 2;
      nbad += !check(ap, 1, one, l, "1xn") + !check(ap, 1, l, one, "nx1");
    }
  }
  for (int it = 0; it < 24; ++it) {  // long gaps with cheap gap costs, every band kind
    RefParam ap = cheap;
    ap.band_width = it % 3 == 0 ? 0 : it % 3 == 1 ? 50 : 20;
    std::vector<uint8_t> a, b;
    for (int k = 0; k < 3; ++k) {
      for (int i = 0, blk = 40 + rnd() % 60; i < blk; ++i) { const uint8_t c = rnd() % 4; a.push_back(c); b.push_back(c); }
      if (k < 2) for (int i = 0, g = 5 + rnd() % 45; i < g; ++i) b.push_back(rnd() % 4);
    }
    if (it & 1) a.swap(b);
    ++total;
    if (!check(ap, it & 2 ? 1 : 30, a, b, "long gap")) ++nbad;
  }
  for (int it = 0; it < 8; ++it) {  // past 32000: the bwa preset, about 3 000 near-identical bases and more
    RefParam ap = *presets[2];
    ap.band_width = it & 1 ? 50 : 0;
    std::vector<uint8_t> a(it < 4 ? 3100 : 4000 + rnd() % 500);
    for (auto &x : a) x = rnd() % 4;
    std::vector<uint8_t> b = noisy(a, 4, 300, it & 2 ? 500 : 0, 3);
    ++total;
    if (!check(ap, it == 7 ? 31000 : 1, a, b, "rebasing")) ++nbad;
  }
  printf("rebased %ld no_band %ld ring %ld\n", n_rebased, n_no_band, n_ring);
  if (!n_rebased || !n_no_band || !n_ring) { printf("a class is empty\n"); return 1; }
  printf("%ld pairs, %ld differ\n", total, nbad);
  return nbad != 0;
}
