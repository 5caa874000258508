// bsw2_seed_check.cpp -- bsw2_core.h on the host over an index read from .bwt / .sa files.
// TEST INFRASTRUCTURE, built with g++ (no HIP).
//
//   bsw2_seed_check run PREFIX TASKS [threads]
//       TASKS: one task per line, "a b q r t bw z is strand seq" (t and bw as the core gets them,
//       strand 0: PREFIX.bwt / .sa, 1: PREFIX.rbwt / .rsa, seq: digits 0-3).  Prints per task
//       "n_all n_narrow hit..." (hit = k,l,flag,len,G,G2,beg,end), a tab, and the counters.
//       With threads > 0 nothing is printed but the wall time (the bench's host baseline).
//   bsw2_seed_check vectors PREFIX VECTORS.tsv
//       every line of a golden file (see tools/make_bwasw_golden.py) recomputed and compared;
//       prints the class counts and "N vectors, D differ".  A vector whose option-set name is
//       "INDEX/name" runs on the index INDEX that lies next to PREFIX, every other one on PREFIX.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <thread>

#include "bsw2_core.h"

using namespace ibwa_bsw2;

struct FileIdx {
  uint32_t seq_len = 0, primary = 0, L2[5] = {0, 0, 0, 0, 0}, sa_intv = 0;
  std::vector<uint32_t> bwt, cp, sav;  // 2-bit words, counts before every 64 symbols, sampled SA

  bool load(const std::string &bwt_fn, const std::string &sa_fn) {
    FILE *f = fopen(bwt_fn.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    bwt.resize((sz - 20) / 4);
    bool ok = fread(&primary, 4, 1, f) == 1 && fread(L2 + 1, 4, 4, f) == 4 && fread(bwt.data(), 4, bwt.size(), f) == bwt.size();
    fclose(f);
    if (!ok) return false;
    seq_len = L2[4];
    {  // the file interleaves 4 counts before every 8 words of symbols (bwtmisc.c:122-144): drop them
      std::vector<uint32_t> raw;
      for (size_t k = 0; k < bwt.size(); k += 12)
        for (size_t j = k + 4; j < k + 12 && j < bwt.size(); ++j) raw.push_back(bwt[j]);
      bwt.swap(raw);
      if (bwt.size() < ((size_t)seq_len + 15) / 16) return false;
    }
    cp.assign(((size_t)seq_len / 64 + 1) * 4, 0);
    uint32_t c[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < seq_len; ++i) {
      if (i % 64 == 0) memcpy(&cp[i / 64 * 4], c, 16);
      ++c[sym(i)];
    }
    if (seq_len % 64 == 0) memcpy(&cp[seq_len / 64 * 4], c, 16);
    f = fopen(sa_fn.c_str(), "rb");
    if (!f) return false;
    uint32_t hdr[7];
    ok = fread(hdr, 4, 7, f) == 7;  // primary, L2[1..4], sa_intv, seq_len
    sa_intv = hdr[5];
    ok = ok && hdr[0] == primary && hdr[6] == seq_len && sa_intv > 0;
    if (ok) {
      sav.assign(((size_t)seq_len + sa_intv) / sa_intv, 0xffffffffu);
      ok = fread(sav.data() + 1, 4, sav.size() - 1, f) == sav.size() - 1;
    }
    fclose(f);
    return ok;
  }
  uint32_t sym(uint32_t i) const { return bwt[i >> 4] >> ((~i & 15) << 1) & 3; }
  void occ4(uint32_t k, uint32_t cnt[4]) const {  // bwt_occ4
    if (k == (uint32_t)-1) {
      cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
      return;
    }
    if (k >= primary) --k;
    memcpy(cnt, &cp[k / 64 * 4], 16);
    for (uint32_t i = k / 64 * 64; i <= k; i += 16) {  // 16 symbols a word, the first n of this one
      const uint32_t n = std::min<uint32_t>(16, k - i + 1), w = bwt[i >> 4] >> (2 * (16 - n));
      const uint32_t m = n == 16 ? 0x55555555u : ((1u << (2 * n)) - 1u) & 0x55555555u;
      for (uint32_t c = 0; c < 4; ++c) {
        const uint32_t x = w ^ (c * 0x55555555u);
        cnt[c] += (uint32_t)__builtin_popcount(~(x | (x >> 1)) & m);
      }
    }
  }
  uint32_t inv_psi(uint32_t k) const {  // bwt_invPsi (bwt.h:66-70)
    if (k == primary) return 0;
    const uint32_t c = sym(k > primary ? k - 1 : k);
    uint32_t cnt[4];
    occ4(k, cnt);
    return L2[c] + cnt[c];
  }
  uint32_t sa(uint32_t k) const {  // bwt_sa
    uint32_t s = 0;
    while (k % sa_intv != 0) {
      ++s;
      k = inv_psi(k);
    }
    return s + sav[k / sa_intv];
  }
};

static std::string hits_text(const std::vector<Hit> &all, const std::vector<Hit> &narrow) {
  std::string s = std::to_string(all.size()) + " " + std::to_string(narrow.size());
  char buf[160];
  for (const std::vector<Hit> *v : {&all, &narrow})
    for (const Hit &h : *v) {
      snprintf(buf, sizeof buf, " %u,%u,%u,%d,%d,%d,%d,%d", h.k, h.l, h.flag, h.len, h.G, h.G2, h.beg, h.end);
      s += buf;
    }
  return s;
}

static std::vector<uint8_t> codes(const std::string &s) {
  std::vector<uint8_t> v(s.size());
  for (size_t i = 0; i < s.size(); ++i) v[i] = (uint8_t)(s[i] - '0');
  return v;
}

struct Task {
  Opt o;
  int strand;
  std::vector<uint8_t> seq;
};

int main(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: bsw2_seed_check run|vectors PREFIX FILE [threads]\n");
    return 2;
  }
  const std::string mode = argv[1], prefix = argv[2];
  std::map<std::string, FileIdx[2]> loaded;
  auto index_at = [&](const std::string &p) -> FileIdx * {
    auto it = loaded.find(p);
    if (it != loaded.end()) return it->second;
    FileIdx *x = loaded[p];
    if (!x[0].load(p + ".bwt", p + ".sa") || !x[1].load(p + ".rbwt", p + ".rsa")) {
      fprintf(stderr, "cannot load %s.{bwt,sa,rbwt,rsa}\n", p.c_str());
      exit(2);
    }
    return x;
  };
  const FileIdx *idx = index_at(prefix);
  std::ifstream in(argv[3]);
  if (!in) {
    fprintf(stderr, "cannot open %s\n", argv[3]);
    return 2;
  }
  std::string line;
  if (mode == "run") {
    std::vector<Task> tasks;
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      std::istringstream ss(line);
      Task t;
      std::string seq;
      ss >> t.o.a >> t.o.b >> t.o.q >> t.o.r >> t.o.t >> t.o.bw >> t.o.z >> t.o.is >> t.strand >> seq;
      t.seq = codes(seq);
      tasks.push_back(std::move(t));
    }
    const int threads = argc > 4 ? atoi(argv[4]) : 0;
    if (threads > 0) {
      std::atomic<size_t> next{0};
      std::atomic<long long> cells{0};
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<std::thread> th;
      for (int w = 0; w < threads; ++w)
        th.emplace_back([&] {
          std::vector<Hit> all, narrow;
          for (size_t i; (i = next++) < tasks.size();) {
            Counters ct;
            seed_task(tasks[i].o, tasks[i].seq.data(), (int)tasks[i].seq.size(), idx[tasks[i].strand], all, narrow, &ct);
            cells += ct.cells_visited;
          }
        });
      for (auto &t : th) t.join();
      const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      printf("{\"tasks\": %zu, \"threads\": %d, \"seconds\": %.6f, \"cells\": %lld}\n", tasks.size(), threads, s,
             (long long)cells);
      return 0;
    }
    for (const Task &t : tasks) {
      std::vector<Hit> all, narrow;
      Counters c;
      seed_task(t.o, t.seq.data(), (int)t.seq.size(), idx[t.strand], all, narrow, &c);
      printf("%s\tpeak_cells=%lld peak_pending=%lld max_array=%lld max_stack=%lld iters=%lld cells=%lld narrow_raw=%lld "
             "dag_nodes=%lld swap=%lld dup=%lld tie_cut=%lld band_del=%lld recreate=%lld flag1=%lld displaced=%lld "
             "narrow_tie=%lld\n",
             hits_text(all, narrow).c_str(), (long long)c.peak_cells, (long long)c.peak_pending, (long long)c.max_array,
             (long long)c.max_stack, (long long)c.iters, (long long)c.cells_visited, (long long)c.narrow_raw,
             (long long)c.dag_nodes, (long long)c.n_swap, (long long)c.n_dup, (long long)c.n_tie_cut,
             (long long)c.n_band_del, (long long)c.n_recreate, (long long)c.n_flag1, (long long)c.n_displaced,
             (long long)c.n_narrow_tie);
    }
    return 0;
  }
  if (mode != "vectors") return 2;
  // optset a b q r t0 bw0 z is coef adjust t bw strand kind seq hits
  long n = 0, differ = 0;
  std::map<std::string, long> cls;
  Counters peak;
  while (std::getline(in, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::vector<std::string> f;
    size_t a = 0;
    for (size_t b; (b = line.find('\t', a)) != std::string::npos; a = b + 1) f.push_back(line.substr(a, b - a));
    f.push_back(line.substr(a));
    if (f.size() != 17) {
      fprintf(stderr, "vector %ld: %zu fields\n", n, f.size());
      return 2;
    }
    Opt o = {atoi(f[1].c_str()), atoi(f[2].c_str()), atoi(f[3].c_str()), atoi(f[4].c_str()), atoi(f[5].c_str()),
             atoi(f[6].c_str()), atoi(f[7].c_str()), atoi(f[8].c_str())};
    const float coef = strtof(f[9].c_str(), nullptr);
    const int adjust = atoi(f[10].c_str()), strand = atoi(f[13].c_str());
    const std::vector<uint8_t> seq = codes(f[15]);
    const FileIdx *idx = index_at(prefix);
    const size_t slash = f[0].find('/');
    if (slash != std::string::npos) {  // "INDEX/name": the index of that name next to PREFIX
      const size_t dir = prefix.rfind('/');
      idx = index_at((dir == std::string::npos ? std::string() : prefix.substr(0, dir + 1)) + f[0].substr(0, slash));
      ++cls["index:" + f[0].substr(0, slash)];
    }
    if (adjust) opt_for_len(o.a, o.q, o.r, o.t, o.bw, coef, (uint32_t)seq.size(), &o.t, &o.bw);
    bool bad = o.t != atoi(f[11].c_str()) || o.bw != atoi(f[12].c_str());
    std::vector<Hit> all, narrow;
    Counters c;
    seed_task(o, seq.data(), (int)seq.size(), idx[strand], all, narrow, &c);
    bad = bad || hits_text(all, narrow) != f[16];
    if (bad) {
      if (++differ <= 5) fprintf(stderr, "vector %ld (%s, %s, len %zu) differs:\n got  %s\n want %s\n", n, f[0].c_str(), f[14].c_str(), seq.size(), hits_text(all, narrow).c_str(), f[16].c_str());
    }
    ++n;
    ++cls["optset:" + f[0]];
    ++cls["kind:" + f[14]];
    ++cls["len:" + std::to_string(seq.size()) + (strand ? ":r" : ":f")];
    if (seq.size() >= 2048) ++cls["long:" + f[14]];
    if (seq.size() > 1000) ++cls["at:" + std::to_string(seq.size()) + ":" + f[14]];
    if (seq.size() > 1000) cls["hits:" + std::to_string(seq.size())] += !all.empty() || !narrow.empty();
    cls["event:swap"] += c.n_swap > 0;
    cls["event:dup"] += c.n_dup > 0;
    cls["event:tie_cut"] += c.n_tie_cut > 0;
    cls["event:band_del"] += c.n_band_del > 0;
    cls["event:recreate"] += c.n_recreate > 0;
    cls["event:array256"] += c.max_array > 256;
    cls["event:flag1"] += c.n_flag1 > 0;
    cls["event:displaced"] += c.n_displaced > 0;
    cls["event:narrow_tie"] += c.n_narrow_tie > 0 && !narrow.empty();
    cls["event:empty"] += all.empty() && narrow.empty();
    peak.peak_cells = std::max(peak.peak_cells, c.peak_cells);
    peak.peak_pending = std::max(peak.peak_pending, c.peak_pending);
    peak.max_array = std::max(peak.max_array, c.max_array);
    peak.max_stack = std::max(peak.max_stack, c.max_stack);
    peak.narrow_raw = std::max(peak.narrow_raw, c.narrow_raw);
    const long per_base = (long)((c.peak_cells + (long)seq.size() - 1) / (long)seq.size());
    cls["peak:cells_per_base"] = std::max(cls["peak:cells_per_base"], per_base);
  }
  for (const auto &kv : cls) printf("%s\t%ld\n", kv.first.c_str(), kv.second);
  printf("peak:cells\t%lld\npeak:pending\t%lld\npeak:array\t%lld\npeak:stack\t%lld\npeak:narrow_raw\t%lld\n",
         (long long)peak.peak_cells, (long long)peak.peak_pending, (long long)peak.max_array, (long long)peak.max_stack,
         (long long)peak.narrow_raw);
  printf("%ld vectors, %ld differ\n", n, differ);
  return differ ? 1 : 0;
}
