// stdaln_core_check.cpp -- TEST INFRASTRUCTURE: stdaln_core.h instantiated on the host (stride 1) against
// the compiled reference's aln_local_core / aln_global_core / aln_path2cigar32, loaded from the shared
// library named on the command line.  Random pairs over three schemes, bands from 1 to the full
// matrix, both gap_end kinds, thresholds, and both ways of taking the suboptimal score; then pairs
// with long internal gaps, whose hit spans several times the shorter sequence.
//   usage: stdaln_core_check <libibwa_ref.so> <pairs>      exit status 0: all equal
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "stdaln_core.h"

using namespace ibwa::stdaln;

// the reference's interface (stdaln.h)
struct RefParam { int gap_open, gap_ext, gap_end; int *matrix; int row, band_width; };
struct RefPath { int i, j; unsigned char ctype; };
typedef int (*local_fn)(unsigned char *, int, unsigned char *, int, const RefParam *, RefPath *, int *, int, int *);
typedef int (*global_fn)(unsigned char *, int, unsigned char *, int, const RefParam *, RefPath *, int *);
typedef uint32_t *(*cigar_fn)(const RefPath *, int, int *);

static uint64_t rs = 88172645463325252ull;
static uint32_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 11); }

static local_fn ref_local;
static global_fn ref_global;
static cigar_fn ref_cigar;

// one pair through both; the scratch is sized as the engine sizes it (local_span)
static bool check(const RefParam &ap, int type, int thres, bool keep, std::vector<uint8_t> &a, std::vector<uint8_t> &b,
                  const char *what) {
  const int n1 = (int)a.size(), n2 = (int)b.size();
  std::vector<RefPath> path(n1 + n2 + 2);
  int rpl = 0, rsubo = 0, rnc = 0;
  const int rscore = type == 0 ? ref_local(a.data(), n1, b.data(), n2, &ap, path.data(), &rpl, thres, &rsubo)
                               : ref_global(a.data(), n1, b.data(), n2, &ap, path.data(), &rpl);
  uint32_t *rc = rpl > 0 ? ref_cigar(path.data(), rpl, &rnc) : nullptr;
  Param P = {ap.gap_open, ap.gap_ext, ap.gap_end, ap.band_width, ap.row, 0, ap.matrix};
  for (int i = 0; i < ap.row * ap.row; ++i)
    if (ap.matrix[i] > P.max_score) P.max_score = ap.matrix[i];
  const uint64_t S = n1 < n2 ? n1 : n2;
  const uint64_t w1 = type == 0 ? local_span(n1, S, P) : n1, w2 = type == 0 ? local_span(n2, S, P) : n2;
  const uint32_t W = (uint32_t)w1 + 1;
  std::vector<uint32_t> eh(n1 + 2), mid(6 * W), cig(w1 + w2 + 2);
  std::vector<uint16_t> suba(n2 + 1);
  std::vector<uint8_t> tb((w1 + 1) * (w2 + 1) + 8);
  View<uint32_t> EH{eh.data(), 1}, MID{mid.data(), 1};
  View<uint16_t> SU{suba.data(), 1};
  TbView T{tb.data(), 1, 0};
  LocalOut o;
  if (type == 0) {
    local_core(EH, SU, keep, MID, W, T, (w1 + 1) * (w2 + 1), P, thres, a.data(), n1, b.data(), n2, cig.data(), (int)(w1 + w2), o);
  } else {
    int si = 0, sj = 0;
    o.subo = 0;
    o.score = global_core(MID, W, T, P, a.data(), n1, b.data(), n2, ap.band_width, ap.gap_end, cig.data(), n1 + n2, o.n_cig,
                          o.path_len, si, sj);
    for (int k = 0; k < o.n_cig / 2; ++k) { const uint32_t t = cig[k]; cig[k] = cig[o.n_cig - 1 - k]; cig[o.n_cig - 1 - k] = t; }
    o.s_i = si; o.s_j = sj; o.e_i = n1; o.e_j = n2;
  }
  bool bad = o.score != rscore || o.path_len != rpl;
  if (!bad && rpl > 0)
    bad = o.n_cig != rnc || memcmp(cig.data(), rc, rnc * 4) || o.s_i != path[rpl - 1].i || o.s_j != path[rpl - 1].j ||
          o.e_i != path[0].i || o.e_j != path[0].j || (type == 0 && o.subo != rsubo);
  if (bad)
    printf("BAD %s type %d %d x %d band %d gap_end %d thres %d keep %d: score %d / %d path_len %d / %d subo %d / %d\n", what, type,
           n1, n2, ap.band_width, ap.gap_end, thres, (int)keep, o.score, rscore, o.path_len, rpl, o.subo, rsubo);
  free(rc);
  return !bad;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  void *h = dlopen(argv[1], RTLD_LAZY);
  if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
  ref_local = (local_fn)dlsym(h, "aln_local_core");
  ref_global = (global_fn)dlsym(h, "aln_global_core");
  ref_cigar = (cigar_fn)dlsym(h, "aln_path2cigar32");
  const RefParam *presets[3] = {(RefParam *)dlsym(h, "aln_param_blast"), (RefParam *)dlsym(h, "aln_param_aa2aa"),
                                (RefParam *)dlsym(h, "aln_param_bwa")};
  if (!ref_local || !ref_global || !ref_cigar || !presets[0] || !presets[1] || !presets[2]) return 2;
  const int pairs = atoi(argv[2]);
  long nbad = 0;
  for (int it = 0; it < pairs; ++it) {
    RefParam ap = *presets[it % 3];
    const int type = (it / 3) % 2, alpha = ap.row;
    const int n1 = 1 + rnd() % (it % 7 == 0 ? 300 : 40), n2 = 1 + rnd() % (it % 5 == 0 ? 600 : 60);
    std::vector<uint8_t> a(n1), b(n2);
    const int eff = (it % 11 == 0) ? 2 : alpha;  // low complexity: ties
    for (auto &x : b) x = rnd() % eff;
    for (auto &x : a) x = rnd() % eff;
    if (it % 2 == 0 && n2 > 4) {  // a noisy copy of seq2 inside seq1, sometimes with an indel
      const int st = rnd() % n2;
      for (int i = 0; i < n1 && st + i < n2; ++i) a[i] = (rnd() % 10 == 0) ? rnd() % alpha : b[st + i];
      if (it % 4 == 0 && n1 > 6) { a.erase(a.begin() + n1 / 2); a.push_back(rnd() % alpha); }
    }
    const int bs = rnd() % 4;
    if (bs == 0) ap.band_width = n1 + n2; else if (bs == 1) ap.band_width = 1 + rnd() % 5; else if (bs == 2) ap.band_width = 1;
    if (type == 1) ap.gap_end = (rnd() % 3 == 0) ? 0 : (rnd() % 3 == 0 ? -1 : ap.gap_end);
    const int thres = 1 + (rnd() % 4 == 0 ? rnd() % 30 : 0);
    if (!check(ap, type, thres, (it / 6) % 2 == 0, a, b, "random")) ++nbad;
  }
  // long internal gaps: match 5, anything else -2, open 10, extend 2; and BLOSUM62
  static int m5[25];
  for (int x = 0; x < 5; ++x) for (int y = 0; y < 5; ++y) m5[x * 5 + y] = x == y ? 5 : -2;
  const RefParam cheap = {10, 2, 2, m5, 5, 0};
  for (int it = 0; it < 40; ++it) {
    RefParam ap = it & 1 ? *presets[1] : cheap;
    const int alpha = it & 1 ? 20 : 4, blk = 20 + rnd() % 90, nb = 2 + rnd() % 3;
    std::vector<uint8_t> a, b;
    for (int k = 0; k < nb; ++k) {
      for (int i = 0; i < blk; ++i) { const uint8_t c = rnd() % alpha; a.push_back(c); b.push_back(c); }
      if (k + 1 < nb) for (int i = 0, g = blk + rnd() % (2 * blk); i < g; ++i) b.push_back(rnd() % alpha);
    }
    ap.band_width = (it & 2) ? 50 : (int)(a.size() + b.size());
    if (it & 4) a.swap(b);
    if (!check(ap, 0, 1, (it & 8) != 0, a, b, "long gap")) ++nbad;
  }
  printf("%d + 40 pairs, %ld differ\n", pairs, nbad);
  return nbad != 0;
}
