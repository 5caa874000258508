// stdsw_main.cpp -- `ibwa-amd stdsw`: bwa_stdsw (simple_dp.c:129-162) over ibwa_stdaln_batch.
// Every short sequence (and strand) is aligned against every long one: seq1 = the short, seq2 = the
// long, band_width = both lengths, gap_end 0, aln_param_blast or (-p) aln_param_aa2aa; the records
// and the messages on stderr are the reference's, byte for byte, for one long sequence.  With
// several long sequences the reference's loop goes astray (its index is reused by the CIGAR print
// loop, simple_dp.c:91 / :102); here every short and strand meets every long, in file order.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "ibwa_aln.h"
#include "readers.h"

namespace {

struct Seq {
  std::string name, s;
};

// stdaln's own alphabets (aln_nt4_table / aln_aa_table): A G C T, anything else 4, '-' 5; the 20
// residues in the order of the score matrix, '*' 20, anything else 21, '-' 22
struct Tables {
  uint8_t nt[256], aa[256], rev[256];
  Tables() {
    memset(nt, 4, sizeof nt);
    memset(aa, 21, sizeof aa);
    memset(rev, 'N', sizeof rev);
    const char *n4 = "AGCT", *res = "ARNDCQEGHILKMFPSTWYV", *pairs = "ATCGBVDHKMRYSSWWXX";
    for (int k = 0; n4[k]; ++k) nt[(int)n4[k]] = nt[n4[k] + 32] = (uint8_t)k;
    for (int k = 0; res[k]; ++k) aa[(int)res[k]] = aa[res[k] + 32] = (uint8_t)k;
    nt['-'] = 5;
    aa['*'] = 20;
    aa['-'] = 22;
    // the complement of an IUPAC letter keeps its case; anything unknown becomes N (simple_dp.c:24-41)
    for (int k = 0; pairs[k]; k += 2) {
      const int x = pairs[k], y = pairs[k + 1];
      rev[x] = (uint8_t)y; rev[y] = (uint8_t)x;
      rev[x + 32] = (uint8_t)(y + 32); rev[y + 32] = (uint8_t)(x + 32);
    }
  }
};

void usage(int thres) {
  fprintf(stderr, "\nUsage:   bwa stdsw [options] <seq1.long.fa> <seq2.short.fa>\n\n");
  fprintf(stderr, "Options: -T INT    minimum score [%d]\n", thres);
  fprintf(stderr, "         -p        protein alignment (suppressing -r)\n");
  fprintf(stderr, "         -f        forward strand only\n");
  fprintf(stderr, "         -r        reverse strand only\n");
  fprintf(stderr, "         -g        global alignment\n\n");
  fprintf(stderr, "Note: This program is specifically designed for alignment between multiple short\n");
  fprintf(stderr, "      sequences and ONE long sequence. It outputs the suboptimal score on the long\n");
  fprintf(stderr, "      sequence.\n\n");
}

bool load(const char *fn, std::vector<Seq> &out, size_t limit, ibwa_cli::SeqReader &rd) {
  out.clear();
  while (out.size() < limit && rd.read() >= 0) out.push_back({rd.name, rd.seq});
  return !out.empty();
}

// the codes of s; a character that encodes to >= row ('-') indexes past the matrix in the reference
bool encode(const Seq &q, const uint8_t *tab, int row, std::vector<uint8_t> &codes) {
  for (char ch : q.s) {
    const uint8_t v = tab[(unsigned char)ch];
    if (v >= row) {
      fprintf(stderr, "[stdsw] sequence '%s' holds '%c', which has no row in the score matrix\n", q.name.c_str(), ch);
      return false;
    }
    codes.push_back(v);
  }
  return true;
}

}  // namespace

int stdsw_main(int argc, char *argv[]) {
  int is_global = 0, thres = 1, strand = 0, aa = 0, c;
  optind = 1;
  while ((c = getopt(argc, argv, "gT:frp")) >= 0) {
    switch (c) {
      case 'g': is_global = 1; break;
      case 'T': thres = atoi(optarg); break;
      case 'f': strand |= 1; break;
      case 'r': strand |= 2; break;
      case 'p': aa = 1; break;
    }
  }
  if (strand == 0) strand = 3;
  if (aa) strand = 1;
  if (optind + 1 >= argc) {
    usage(thres);
    return 1;
  }
  if (thres <= 0) {
    // the reference then skips the path fill and prints unallocated strings
    fprintf(stderr, "[stdsw] -T %d: the minimum score must be at least 1\n", thres);
    return 1;
  }
  static const Tables tabs;
  ibwa_aln_param_t ap;
  if (ibwa_aln_param_preset(aa ? "aa2aa" : "blast", &ap)) {
    fprintf(stderr, "[stdsw] %s\n", ibwa_last_error());
    return 1;
  }
  ap.gap_end = 0;
  ap.band_width = 0;  // len1 + len2 of each pair
  const uint8_t *tab = aa ? tabs.aa : tabs.nt;

  ibwa_cli::SeqReader lrd, srd;
  if (!lrd.open(argv[optind])) {
    fprintf(stderr, "[stdsw] fail to open file '%s'\n", argv[optind]);
    return 1;
  }
  std::vector<Seq> longs, shorts;
  load(argv[optind], longs, SIZE_MAX, lrd);
  fprintf(stderr, "[load_seqs] %d sequences are loaded.\n", (int)longs.size());
  if (!srd.open(argv[optind + 1])) {
    fprintf(stderr, "[stdsw] fail to open file '%s'\n", argv[optind + 1]);
    return 1;
  }
  std::vector<uint8_t> lcodes;
  std::vector<uint64_t> loff;
  for (const Seq &q : longs) {
    if (is_global && q.s.empty()) {
      fprintf(stderr, "[stdsw] sequence '%s' is empty: no global alignment\n", q.name.c_str());
      return 1;
    }
    loff.push_back(lcodes.size());
    if (!encode(q, tab, ap.row, lcodes)) return 1;
  }
  lcodes.push_back(0);

  ibwa_ctx_t *ctx = nullptr;
  int rc = 0;
  const int n_strand = (strand & 1) + (strand >> 1);
  while (!rc && load(argv[optind + 1], shorts, 1 << 16, srd)) {
    // the batch: per short its strands ('-': the complemented text reversed, simple_dp.c:46-55)
    std::vector<std::string> text;
    std::vector<char> sch;
    std::vector<uint8_t> scodes;
    std::vector<uint64_t> soff;
    for (const Seq &q : shorts) {
      if (is_global && q.s.empty()) {
        fprintf(stderr, "[stdsw] sequence '%s' is empty: no global alignment\n", q.name.c_str());
        rc = 1;
        break;
      }
      for (int s = 0; s < 2; ++s) {
        if (!(strand >> s & 1)) continue;
        Seq t = q;
        if (s == 1) {
          const size_t l = q.s.size();
          for (size_t k = 0; k < l; ++k) t.s[k] = (char)tabs.rev[(unsigned char)q.s[l - 1 - k]];
        }
        soff.push_back(scodes.size());
        if (!encode(t, tab, ap.row, scodes)) { rc = 1; break; }
        text.push_back(t.s);
        sch.push_back(s ? '-' : '+');
      }
      if (rc) break;
    }
    if (rc) break;
    scodes.push_back(0);
    const int64_t n = (int64_t)text.size() * (int64_t)longs.size();
    if (n == 0) continue;
    std::vector<uint64_t> off1(n), off2(n);
    std::vector<uint32_t> len1(n), len2(n);
    int64_t p = 0;
    for (size_t k = 0; k < text.size(); ++k)
      for (size_t g = 0; g < longs.size(); ++g, ++p) {
        off1[p] = soff[k]; len1[p] = (uint32_t)text[k].size();
        off2[p] = loff[g]; len2[p] = (uint32_t)longs[g].s.size();
      }
    std::vector<int32_t> score(n), subo(n), plen(n), ends(4 * n), ncig(n);
    uint32_t *cigar = nullptr;
    int64_t tot = 0;
    // the checks first: a refusal needs no device
    if (ibwa_stdaln_check(&ap, is_global, thres, n, scodes.data(), off1.data(), len1.data(), lcodes.data(), off2.data(),
                          len2.data()) ||
        (!ctx && ibwa_ctx_create(0, &ctx)) ||
        ibwa_stdaln_batch(ctx, &ap, is_global, thres, n, scodes.data(), off1.data(), len1.data(), lcodes.data(), off2.data(),
                          len2.data(), score.data(), subo.data(), plen.data(), ends.data(), ncig.data(), &cigar, &tot)) {
      fprintf(stderr, "[stdsw] %s\n", ibwa_last_error());
      rc = 1;
      break;
    }
    std::string o1, o2, om;
    int64_t cq = 0;
    p = 0;
    for (size_t k = 0; k < text.size(); ++k)
      for (size_t g = 0; g < longs.size(); ++g, ++p) {
        const uint32_t *cg = cigar + cq;
        cq += ncig[p];
        if (score[p] == -1 && plen[p] > 0)
          fprintf(stderr, "[aln_local_core] Potential bug: the path's score is below the local score\n");
        if (!(score[p] >= thres || is_global)) continue;
        const std::string &s1 = text[k], &s2 = longs[g].s;
        const uint8_t *c1 = scodes.data() + soff[k], *c2 = lcodes.data() + loff[g];
        const int *e = ends.data() + 4 * p;
        printf(">%s\t%d\t%d\t%s\t%c\t%d\t%d\t%d\t%d\t", longs[g].name.c_str(), e[0] ? e[0] : 1, e[2], shorts[k / n_strand].name.c_str(),
               sch[k], e[1] ? e[1] : 1, e[3], score[p], subo[p]);
        o1.clear(); o2.clear(); om.clear();
        // the next unconsumed symbol of each sequence (1-based): the first path entry is (e[0], e[1])
        int i = e[0], j = e[1];
        if (ncig[p] > 0) {
          const int op0 = (int)(cg[0] & 0xf);
          if (op0 == 1) ++i; else if (op0 == 2) ++j;
        }
        for (int x = 0; x < ncig[p]; ++x) {
          const int len = (int)(cg[x] >> 4), op = (int)(cg[x] & 0xf);
          printf("%d%c", len, "MDI"[op]);
          for (int t = 0; t < len; ++t) {
            if (op == 0) {
              o1 += s1[i - 1]; o2 += s2[j - 1];
              om += (c1[i - 1] == c2[j - 1] && c1[i - 1] != ap.row) ? '|' : ' ';
              ++i; ++j;
            } else if (op == 1) {
              o1 += '-'; o2 += s2[j - 1]; om += ' ';
              ++j;
            } else {
              o1 += s1[i - 1]; o2 += '-'; om += ' ';
              ++i;
            }
          }
        }
        printf("\n%s\n%s\n%s\n", o2.c_str(), om.c_str(), o1.c_str());
      }
    ibwa_free(cigar);
  }
  if (ctx) ibwa_ctx_destroy(ctx);
  return rc;
}
