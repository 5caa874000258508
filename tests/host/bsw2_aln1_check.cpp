// bsw2_aln1_check.cpp -- bsw2_aln1.h on the host over an index and a sequence read from the .bwt / .sa /
// .pac files.  TEST INFRASTRUCTURE, built with g++ (no HIP), stand-alone.
//
//   bsw2_aln1_check stages PREFIX TASKS [time]
//       TASKS: one read per line, "a b q r t bw z is coef adjust t_seeds mask_level is_rev s seq" (t, bw as
//       bsw2_aln receives them; adjust: derive them from the length; s: the seed of srand48, from which
//       the draw u comes; seq: digits 0-3, for is_rev the reversed read).  Prints per task "t bw" and seven
//       hit lists, tab separated: the two narrow lists after the chain filter, the two after the left
//       extension, the two strand lists after the right extension, the final list.  A list is "n hit..."
//       with hit = k,l,flag,n_seeds,len,G,G2,beg,end.  With "time" only the wall time is printed.
//   bsw2_aln1_check left PREFIX TASKS
//       TASKS: "a b q r bw is_rev seq hits", tab separated -> the list after extend_left.
//   bsw2_aln1_check vectors PREFIX aln1_vectors.tsv      bsw2_aln1_check leftvectors PREFIX left_vectors.tsv
//       every line of a golden file (tools/make_bwasw_hits_golden.py) recomputed and compared; prints
//       the class counts and "N vectors, D differ".
#include <chrono>

#define main bsw2_seed_check_main  // FileIdx and codes() of the seeding checker, without its main
#include "bsw2_seed_check.cpp"
#undef main

#include "bsw2_aln1.h"

struct PacRef {
  std::vector<uint8_t> pac;
  uint32_t n = 0;
  bool load(const std::string &fn, uint32_t l_pac) {
    FILE *f = fopen(fn.c_str(), "rb");
    if (!f) return false;
    pac.resize((size_t)l_pac / 4 + 1);
    const bool ok = fread(pac.data(), 1, pac.size(), f) == pac.size();
    fclose(f);
    n = l_pac;
    return ok;
  }
  uint32_t l_pac() const { return n; }
  uint32_t base(uint32_t i) const { return pac[i >> 2] >> ((~i & 3) << 1) & 3; }
};

static std::string list_text(const std::vector<AlnHit> &v) {
  std::string s = std::to_string(v.size());
  char buf[200];
  for (const AlnHit &h : v) {
    snprintf(buf, sizeof buf, " %u,%u,%u,%u,%d,%d,%d,%d,%d", h.k, h.l, h.flag, h.n_seeds, h.len, h.G, h.G2, h.beg, h.end);
    s += buf;
  }
  return s;
}

static std::vector<AlnHit> parse_list(const std::string &s) {
  std::vector<AlnHit> v;
  const char *p = s.c_str();
  char *e;
  const long n = strtol(p, &e, 10);
  p = e;
  for (long i = 0; i < n; ++i) {
    long long x[9];
    for (int k = 0; k < 9; ++k) {
      x[k] = strtoll(p, &e, 10);
      p = e + (*e == ',');
    }
    v.push_back(AlnHit{(uint32_t)x[0], (uint32_t)x[1], (uint32_t)x[2], (uint32_t)x[3], (int)x[4], (int)x[5], (int)x[6], (int)x[7],
                       (int)x[8]});
  }
  return v;
}

static double draw(long s) {  // the first drand48() after srand48(s)
  const uint64_t X = ((uint64_t)(uint32_t)s << 16 | 0x330E), Y = (0x5DEECE66Dull * X + 0xB) & ((1ull << 48) - 1);
  return (double)Y / 281474976710656.0;
}

static std::vector<std::string> split(const std::string &line, char sep) {
  std::vector<std::string> f;
  size_t a = 0;
  for (size_t b; (b = line.find(sep, a)) != std::string::npos; a = b + 1) f.push_back(line.substr(a, b - a));
  f.push_back(line.substr(a));
  return f;
}

struct Stages {
  int t, bw;
  std::vector<AlnHit> cf[2], left[2], right[2], fin;
};

// the read's run, stage by stage: the same calls as aln1_from_seeds, with the lists kept in between
static void run_stages(AlnOpt o, float coef, int adjust, const std::vector<uint8_t> &s0, const FileIdx *idx, const PacRef &ref, int is_rev,
                       double u, Stages &S, AlnCounters *ct) {
  const int l = (int)s0.size();
  if (adjust) opt_for_len(o.seed.a, o.seed.q, o.seed.r, o.seed.t, o.seed.bw, coef, (uint32_t)l, &o.seed.t, &o.seed.bw);
  S.t = o.seed.t;
  S.bw = o.seed.bw;
  std::vector<uint8_t> rc;
  revcomp(s0.data(), l, rc);
  const uint8_t *seq[2] = {s0.data(), rc.data()};
  std::vector<AlnHit> all[2], narrow[2];
  for (int k = 0; k < 2; ++k) {
    std::vector<Hit> a, n;
    seed_task(o.seed, seq[k], l, idx[is_rev], a, n);
    for (const Hit &h : a) all[k].push_back(to_aln_hit(h));
    for (const Hit &h : n) narrow[k].push_back(to_aln_hit(h));
  }
  chain_filter(o, l, narrow, ct);
  for (int k = 0; k < 2; ++k) {
    S.cf[k] = narrow[k];
    for (AlnHit &h : S.cf[k]) h.n_seeds = 0;  // unset in the reference at this point
    extend_left(o.seed, narrow[k], seq[k], l, ref, is_rev, ct);
    S.left[k] = narrow[k];
    merge(all[k], narrow[k], l, 0);
    resolve_duphits_noindex(all[k]);
    extend_right(o.seed, all[k], seq[k], l, ref, is_rev, ct);
    S.right[k] = all[k];
  }
  merge(all[0], all[1], l, 1);
  resolve_query_overlaps(all[0], o.mask_level, u, ct);
  S.fin = all[0];
}

struct LeftClasses {
  std::map<std::string, long> cls;
  void add_list(size_t n_in, const AlnCounters &c, const AlnCounters &before) {
    cls["left:extended"] += c.extended - before.extended;
    cls["left:not_extensible"] += c.not_extensible - before.not_extensible;
    cls["left:contained_orig"] += c.contained_orig - before.contained_orig;
    cls["left:contained_ext_only"] += c.contained_ext_only - before.contained_ext_only;
    cls["left:same_window"] += c.contained_same_window - before.contained_same_window;
    cls["left:earlier_window"] += c.contained_earlier_window - before.contained_earlier_window;
    cls["left:k_zero"] += c.k_zero - before.k_zero;
    cls["left:lt_clipped"] += c.lt_clipped - before.lt_clipped;
    cls["left:beg_zero"] += c.beg_zero - before.beg_zero;
    cls["left:equal_end"] += c.equal_end - before.equal_end;
    cls["task:n0"] += n_in == 0;
    cls["task:n1"] += n_in == 1;
    cls["task:n64"] += n_in == 64;
    cls["task:n65"] += n_in == 65;
    cls["task:n129"] += n_in > 128;
  }
};

int main(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: bsw2_aln1_check stages|left|vectors|leftvectors PREFIX FILE [time]\n");
    return 2;
  }
  const std::string mode = argv[1], prefix = argv[2];
  FileIdx idx[2];
  if (!idx[0].load(prefix + ".bwt", prefix + ".sa") || !idx[1].load(prefix + ".rbwt", prefix + ".rsa")) {
    fprintf(stderr, "cannot load %s.{bwt,sa,rbwt,rsa}\n", prefix.c_str());
    return 2;
  }
  PacRef ref;
  if (!ref.load(prefix + ".pac", idx[0].seq_len)) {
    fprintf(stderr, "cannot load %s.pac\n", prefix.c_str());
    return 2;
  }
  std::ifstream in(argv[3]);
  if (!in) {
    fprintf(stderr, "cannot open %s\n", argv[3]);
    return 2;
  }
  std::string line;
  if (mode == "stages") {
    const bool timed = argc > 4;
    const auto t0 = std::chrono::steady_clock::now();
    long n = 0;
    AlnCounters ct;
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      std::istringstream ss(line);
      AlnOpt o;
      float coef;
      int adjust, is_rev;
      long s;
      std::string seq;
      ss >> o.seed.a >> o.seed.b >> o.seed.q >> o.seed.r >> o.seed.t >> o.seed.bw >> o.seed.z >> o.seed.is >> coef >> adjust >>
          o.t_seeds >> o.mask_level >> is_rev >> s >> seq;
      Stages S;
      run_stages(o, coef, adjust, codes(seq), idx, ref, is_rev, draw(s), S, &ct);
      ++n;
      if (!timed)
        printf("%d %d\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n", S.t, S.bw, list_text(S.cf[0]).c_str(), list_text(S.cf[1]).c_str(),
               list_text(S.left[0]).c_str(), list_text(S.left[1]).c_str(), list_text(S.right[0]).c_str(),
               list_text(S.right[1]).c_str(), list_text(S.fin).c_str());
    }
    if (timed)
      printf("{\"reads\": %ld, \"seconds\": %.6f, \"dp_runs\": %lld}\n", n,
             std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), (long long)ct.dp_runs);
    return 0;
  }
  if (mode == "left") {
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      const std::vector<std::string> f = split(line, '\t');
      if (f.size() != 8) return 2;
      Opt o = {atoi(f[0].c_str()), atoi(f[1].c_str()), atoi(f[2].c_str()), atoi(f[3].c_str()), 0, atoi(f[4].c_str()), 1, 3};
      const std::vector<uint8_t> q = codes(f[6]);
      std::vector<AlnHit> b = parse_list(f[7]);
      extend_left(o, b, q.data(), (int)q.size(), ref, atoi(f[5].c_str()));
      printf("%s\n", list_text(b).c_str());
    }
    return 0;
  }
  long n = 0, differ = 0;
  LeftClasses L;
  std::map<std::string, long> &cls = L.cls;
  if (mode == "vectors") {
    // optset a b q r t0 bw0 z is coef adjust t_seeds mask_level t bw is_rev kind s seq final left0 left1
    while (std::getline(in, line)) {
      if (line.empty() || line[0] == '#') continue;
      const std::vector<std::string> f = split(line, '\t');
      if (f.size() != 22) {
        fprintf(stderr, "vector %ld: %zu fields\n", n, f.size());
        return 2;
      }
      AlnOpt o = {{atoi(f[1].c_str()), atoi(f[2].c_str()), atoi(f[3].c_str()), atoi(f[4].c_str()), atoi(f[5].c_str()),
                   atoi(f[6].c_str()), atoi(f[7].c_str()), atoi(f[8].c_str())},
                  atoi(f[11].c_str()),
                  strtof(f[12].c_str(), nullptr)};
      const int is_rev = atoi(f[15].c_str());
      const std::vector<uint8_t> seq = codes(f[18]);
      Stages S;
      AlnCounters c;
      const double u = draw(atol(f[17].c_str()));
      run_stages(o, strtof(f[9].c_str(), nullptr), atoi(f[10].c_str()), seq, idx, ref, is_rev, u, S, &c);
      bool bad = S.t != atoi(f[13].c_str()) || S.bw != atoi(f[14].c_str()) || list_text(S.fin) != f[19] ||
                 list_text(S.left[0]) != f[20] || list_text(S.left[1]) != f[21];
      if (seq.size() <= 1000) {  // aln1(), the calls strung together, gives the same lists
        AlnOpt o1 = o;
        o1.seed.t = S.t;
        o1.seed.bw = S.bw;
        std::vector<AlnHit> fin, left[2];
        aln1(o1, seq.data(), (int)seq.size(), idx[is_rev], ref, is_rev, u, fin, nullptr, left);
        bad = bad || list_text(fin) != f[19] || list_text(left[0]) != f[20] || list_text(left[1]) != f[21];
      }
      if (bad && ++differ <= 5)
        fprintf(stderr, "vector %ld (%s, %s, len %zu) differs:\n got  %s | %s | %s\n want %s | %s | %s\n", n, f[0].c_str(),
                f[16].c_str(), seq.size(), list_text(S.fin).c_str(), list_text(S.left[0]).c_str(), list_text(S.left[1]).c_str(),
                f[19].c_str(), f[20].c_str(), f[21].c_str());
      ++n;
      ++cls["optset:" + f[0]];
      ++cls["kind:" + f[16]];
      ++cls["len:" + std::to_string(seq.size())];
      ++cls[is_rev ? "is_rev:1" : "is_rev:0"];
      {  // the per-list counters: both lists share c, so the list sizes are classified here
        AlnCounters zero;
        L.add_list(S.cf[0].size(), c, zero);
        L.add_list(S.cf[1].size(), zero, zero);
      }
      cls["task:n_seeds64"] += c.max_n_seeds > 64;
      cls["chain:lost"] += c.chain_lost > 0;
      cls["chain:other_strand"] += c.chain_other_strand > 0;
      cls["right:clipped"] += c.right_clipped > 0;
      cls["right:equal"] += c.right_equal > 0;
      cls["right:kept"] += c.right_kept > 0;
      cls[is_rev ? "right:is_rev1" : "right:is_rev0"] += !S.right[0].empty() || !S.right[1].empty();
      cls["overlap:tie_j"] += c.tie_j > 0;
      cls["overlap:zeroed"] += c.zeroed > 0;
      cls["overlap:g2_raised"] += c.g2_raised > 0;
      cls["event:empty"] += S.fin.empty();
    }
  } else if (mode == "leftvectors") {
    // a b q r bw is_rev kind seq hits_in hits_out
    while (std::getline(in, line)) {
      if (line.empty() || line[0] == '#') continue;
      const std::vector<std::string> f = split(line, '\t');
      if (f.size() != 10) {
        fprintf(stderr, "vector %ld: %zu fields\n", n, f.size());
        return 2;
      }
      Opt o = {atoi(f[0].c_str()), atoi(f[1].c_str()), atoi(f[2].c_str()), atoi(f[3].c_str()), 0, atoi(f[4].c_str()), 1, 3};
      const std::vector<uint8_t> q = codes(f[7]);
      std::vector<AlnHit> b = parse_list(f[8]);
      const size_t n_in = b.size();
      AlnCounters c, zero;
      extend_left(o, b, q.data(), (int)q.size(), ref, atoi(f[5].c_str()), &c);
      if (list_text(b) != f[9] && ++differ <= 5)
        fprintf(stderr, "left vector %ld (%s, %zu hits) differs:\n got  %.600s\n want %.600s\n", n, f[6].c_str(), n_in,
                list_text(b).c_str(), f[9].c_str());
      ++n;
      ++cls["kind:" + f[6]];
      L.add_list(n_in, c, zero);
      cls["task:n_seeds64"] += c.max_n_seeds > 64;
    }
  } else {
    return 2;
  }
  for (const auto &kv : cls) printf("%s\t%ld\n", kv.first.c_str(), kv.second);
  printf("%ld vectors, %ld differ\n", n, differ);
  return differ ? 1 : 0;
}
