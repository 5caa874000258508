// engine_bsw2_aln.hip -- ibwa_bsw2_aln1_batch and ibwa_bsw2_extend_left_batch: bwasw from a read to its
// hits on one index strand (bsw2_aln1_core).  The seeds come from ibwa_bsw2_seed_batch, the two
// extensions run on the device (bsw2_extend.hip), and what lies between them -- the chain filter, the
// unstable sorts, the merges and the two resolve passes, a handful of hits per read -- is bsw2_aln1.h on
// the host, per read on a few threads.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "bsw2_aln1.h"
#include "engine_ctx.h"

using namespace ibwa;
using ibwa_bsw2::AlnHit;

namespace {

static_assert(sizeof(ibwa_bsw2_aln_hit_t) == 36 && sizeof(AlnHit) == 36, "hit records are 9 words");

constexpr uint32_t kLdsRingMax = (40u << 10) / 256;  // ring words per lane kept in LDS, as k_extend
constexpr uint64_t kScratchBudget = 4ull << 30;      // target windows and HBM rings of all waves

// fn(i) for i in [0, n) on up to 16 host threads
template <class F>
void for_reads(int64_t n, F &&fn) {
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(16, n / 64));
  std::atomic<int64_t> next{0};
  auto work = [&] {
    for (int64_t i; (i = next++) < n;) fn(i);
  };
  if (T == 1) work();
  else {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back(work);
    for (auto &x : th) x.join();
  }
}

// one launch of k_bsw2_extend over lists of hits
struct ExtJob {
  bool ordered = true;
  std::vector<uint8_t> qry;    // per task the sequence the DP reads, concatenated
  std::vector<uint64_t> qoff;
  std::vector<uint32_t> qlen;
  std::vector<int32_t> bw;
  std::vector<uint8_t> rev;
  std::vector<uint64_t> hoff;  // n_tasks + 1
  std::vector<AlnHit> hits;    // in and out
};

int run_ext(ibwa_ctx_t *c, const ibwa_bsw2_opt_t &o, ExtJob &J, int64_t *us, int64_t counts[6], const char *what) {
  const int64_t nt = (int64_t)J.qlen.size(), nh = (int64_t)J.hits.size();
  *us = 0;
  for (int k = 0; k < 6; ++k) counts[k] = 0;
  if (nt == 0 || nh == 0) return 0;
  // the longest window a lane gathers and the widest ring (stdaln_core.h: extend_ring)
  uint64_t tgt = 16, ring = 3;
  for (int64_t t = 0; t < nt; ++t) {
    const uint64_t lq = J.qlen[t], w = ((lq + 1) / 2 * (uint64_t)o.a + (uint64_t)o.r) / (uint64_t)o.r + lq;
    tgt = std::max(tgt, w);
    ring = std::max(ring, std::min<uint64_t>(2ull * (uint32_t)J.bw[t] + 2, w + 2));
  }
  tgt = (tgt + 15) & ~15ull;
  Bsw2ExtArgs A = {};
  const bool all_lds = ring <= kLdsRingMax;
  A.lds_ring = all_lds ? (uint32_t)ring : kLdsRingMax;
  A.eh_words = all_lds ? 0 : (uint32_t)ring;
  A.tgt_bytes = (uint32_t)tgt;
  const uint64_t per_wave = 64 * (tgt + 4ull * A.eh_words);
  if (tgt > UINT32_MAX || per_wave > kScratchBudget)
    return fail(IBWA_EINVAL, "%s: one wave's target windows and rings take %llu MiB, past %llu MiB", what,
                (unsigned long long)(per_wave >> 20), (unsigned long long)(kScratchBudget >> 20));
  // as many single-wave workgroups as a CU's 160 KiB of LDS holds, eight at the most
  const int64_t per_cu = c->bsw2_ext_waves_per_cu ? c->bsw2_ext_waves_per_cu
                                                  : std::max<int64_t>(1, std::min<int64_t>(8, (160 << 10) / bsw2_extend_lds_bytes(A)));
  const int64_t waves = std::max<int64_t>(1, std::min<int64_t>({J.ordered ? nt : (nh + 63) / 64, (int64_t)c->n_cus * per_cu,
                                                                (int64_t)(kScratchBudget / per_wave)}));
  std::vector<uint32_t> htask;
  if (!J.ordered) {
    htask.resize(nh);
    for (int64_t t = 0; t < nt; ++t)
      for (uint64_t h = J.hoff[t]; h < J.hoff[t + 1]; ++h) htask[h] = (uint32_t)t;
  }
  auto &B = c->bext;
  int rc;
  if ((rc = B.qry.ensure(J.qry.size() + 16)) || (rc = B.qoff.ensure(nt * 8)) || (rc = B.qlen.ensure(nt * 4)) ||
      (rc = B.bw.ensure(nt * 4)) || (rc = B.rev.ensure(nt + 16)) || (rc = B.hoff.ensure((nt + 1) * 8)) || (rc = B.hits.ensure(nh * 36)) ||
      (rc = B.htask.ensure(nh * 4 + 16)) || (rc = B.tgt.ensure((uint64_t)waves * 64 * tgt)) ||
      (rc = B.eh.ensure((uint64_t)waves * 64 * 4 * A.eh_words + 256)) || (rc = B.status.ensure(nt * 4)) || (rc = B.ctr.ensure(64)))
    return rc;
  HIPCHK(hipMemcpyAsync(B.qry.p, J.qry.data(), J.qry.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(B.qoff.p, J.qoff.data(), nt * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(B.qlen.p, J.qlen.data(), nt * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(B.bw.p, J.bw.data(), nt * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(B.rev.p, J.rev.data(), nt, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(B.hoff.p, J.hoff.data(), (nt + 1) * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(B.hits.p, J.hits.data(), nh * 36, hipMemcpyHostToDevice, c->stream));
  if (!J.ordered) HIPCHK(hipMemcpyAsync(B.htask.p, htask.data(), nh * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(zero_async(B.status.p, nt * 4, c->stream));
  HIPCHK(zero_async(B.ctr.p, 64, c->stream));
  A.pac = c->index.pac.as<uint32_t>();
  A.l_pac = c->index.pac_len;
  A.n_tasks = nt;
  A.qry = B.qry.as<uint8_t>();
  A.qoff = B.qoff.as<uint64_t>();
  A.qlen = B.qlen.as<uint32_t>();
  A.bw = B.bw.as<int32_t>();
  A.is_rev = B.rev.as<uint8_t>();
  A.hoff = B.hoff.as<uint64_t>();
  A.hits = B.hits.as<uint32_t>();
  A.htask = B.htask.as<uint32_t>();
  A.n_hits = nh;
  A.ordered = J.ordered;
  A.a = o.a; A.b = o.b; A.q = o.q; A.r = o.r;
  A.tgt = B.tgt.as<uint8_t>();
  A.eh = B.eh.as<uint32_t>();
  A.status = B.status.as<uint32_t>();
  A.ctr = B.ctr.as<unsigned long long>();
  HIPCHK(hipEventRecord(c->ev[0], c->stream));
  HIPCHK(launch_bsw2_extend(A, all_lds, (int)waves, c->stream));
  HIPCHK(hipEventRecord(c->ev[1], c->stream));
  std::vector<uint32_t> status(nt);
  unsigned long long hctr[8];
  HIPCHK(hipMemcpyAsync(J.hits.data(), B.hits.p, nh * 36, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(status.data(), B.status.p, nt * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hctr, B.ctr.p, 64, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) *us = (int64_t)(ms * 1000.0f);
  for (int k = 0; k < 6; ++k) counts[k] = (int64_t)hctr[1 + k];
  for (int64_t t = 0; t < nt; ++t)
    if (status[t])
      return fail(IBWA_EOVERFLOW, "%s: task %lld (length %u, band %d): a target window or an eh ring does not fit the launch's scratch "
                  "(%u bytes, %u words)", what, (long long)t, J.qlen[t], J.bw[t], A.tgt_bytes, std::max(A.lds_ring, A.eh_words));
  return 0;
}

int check_aln1(const ibwa_bsw2_aln_opt_t *o, int64_t n, const uint8_t *seq, const uint64_t *off, const uint32_t *len,
               const uint8_t *is_rev, const double *u) {
  if (!o) return fail(IBWA_EINVAL, "bsw2 aln1: no options");
  if (n && !is_rev) return fail(IBWA_EINVAL, "bsw2 aln1: null input");
  for (int64_t i = 0; i < n; ++i)
    if (is_rev[i] > 1) return fail(IBWA_EINVAL, "task %lld: is_rev %d is above 1", (long long)i, is_rev[i]);
  if (int rc = ibwa_bsw2_seed_check(&o->seed, n, seq, off, len, is_rev)) return rc;
  if (o->t_seeds < 0) return fail(IBWA_EINVAL, "bsw2 aln1: t_seeds %d < 0", o->t_seeds);
  if (!(o->mask_level >= 0.0f && o->mask_level <= 1.0f)) return fail(IBWA_EINVAL, "bsw2 aln1: mask_level %g outside [0, 1]", o->mask_level);
  if (u)
    for (int64_t i = 0; i < n; ++i)
      if (!(u[i] >= 0.0 && u[i] < 1.0)) return fail(IBWA_EINVAL, "task %lld: u %g outside [0, 1)", (long long)i, u[i]);
  return 0;
}

}  // namespace

extern "C" {

int ibwa_bsw2_aln_opt_preset(const char *name, ibwa_bsw2_aln_opt_t *opt) {
  if (!opt) return fail(IBWA_EINVAL, "no option struct");
  if (int rc = ibwa_bsw2_opt_preset(name, &opt->seed)) return rc;
  opt->t_seeds = 5;  // bsw2_init_opt (bwtsw2_aux.c:48-57)
  opt->mask_level = 0.50f;
  return 0;
}

int ibwa_bsw2_aln1_check(const ibwa_bsw2_aln_opt_t *opt, int64_t n, const uint8_t *seq, const uint64_t *off, const uint32_t *len,
                         const uint8_t *is_rev, const double *u) {
  return check_aln1(opt, n, seq, off, len, is_rev, u);
}

int ibwa_bsw2_aln1_stats(const ibwa_ctx_t *c, int64_t out[8]) {
  memcpy(out, c->aln1_stats, sizeof c->aln1_stats);
  return 0;
}

int ibwa_bsw2_extend_left_batch(ibwa_ctx_t *c, const ibwa_bsw2_opt_t *opt, int64_t n, const uint8_t *qry, const uint64_t *off,
                                const uint32_t *len, const int32_t *bw, const uint8_t *is_rev, const int32_t *n_hits,
                                ibwa_bsw2_aln_hit_t *hits) {
  if (!opt) return fail(IBWA_EINVAL, "bsw2 extend_left: no options");
  if (n < 0) return fail(IBWA_EINVAL, "bsw2 extend_left: n < 0");
  if (opt->a < 1 || opt->b < 1 || opt->q < 1 || opt->r < 1 || opt->a > 1000 || opt->b > 1000 || opt->q > 1000 || opt->r > 1000)
    return fail(IBWA_EINVAL, "bsw2 extend_left: a, b, q, r outside 1..1000");
  if (n && (!qry || !off || !len || !bw || !is_rev || !n_hits)) return fail(IBWA_EINVAL, "bsw2 extend_left: null input");
  if (!c->index.pac_loaded) return fail(IBWA_ENOINDEX, "no reference sequence loaded (ibwa_ctx_load_pac)");
  if (c->index.pac_len > UINT32_MAX) return fail(IBWA_EINVAL, "bsw2 extend_left: the sequence is past 2^32 bases");
  memset(c->aln1_stats, 0, sizeof c->aln1_stats);
  ExtJob J;
  J.hoff.push_back(0);
  for (int64_t t = 0; t < n; ++t) {
    if (is_rev[t] > 1) return fail(IBWA_EINVAL, "task %lld: is_rev %d is above 1", (long long)t, is_rev[t]);
    if (len[t] > IBWA_BSW2_MAX_LEN) return fail(IBWA_EINVAL, "task %lld: length %u is above %d", (long long)t, len[t], IBWA_BSW2_MAX_LEN);
    if (bw[t] < 1) return fail(IBWA_EINVAL, "task %lld: bw %d < 1", (long long)t, bw[t]);
    if (n_hits[t] < 0) return fail(IBWA_EINVAL, "task %lld: %d hits", (long long)t, n_hits[t]);
    if (n_hits[t] && !hits) return fail(IBWA_EINVAL, "bsw2 extend_left: null hits");
    const uint8_t *s = qry + off[t];
    J.qoff.push_back(J.qry.size());
    for (uint32_t j = 0; j < len[t]; ++j) {
      if (s[len[t] - 1 - j] >= 4)
        return fail(IBWA_EINVAL, "task %lld: seq[%u] = %d is not below 4", (long long)t, len[t] - 1 - j, s[len[t] - 1 - j]);
      J.qry.push_back(s[len[t] - 1 - j]);  // reversed: a hit's query is the tail [len - beg, len)
    }
    J.qlen.push_back(len[t]);
    J.bw.push_back(bw[t]);
    J.rev.push_back(is_rev[t]);
    const AlnHit *h = reinterpret_cast<const AlnHit *>(hits) + J.hits.size();
    for (int32_t j = 0; j < n_hits[t]; ++j) {
      if (h[j].beg < 0 || (uint32_t)h[j].beg > len[t])
        return fail(IBWA_EINVAL, "task %lld: hit %d: beg %d outside [0, %u]", (long long)t, j, h[j].beg, len[t]);
      if (h[j].l == 0 && h[j].k != 0 && (h[j].k > c->index.pac_len || h[j].G < 1 || h[j].G > 32000))
        return fail(IBWA_EINVAL, "task %lld: hit %d: k %u past l_pac or G %d outside 1..32000", (long long)t, j, h[j].k, h[j].G);
    }
    std::vector<AlnHit> b(h, h + n_hits[t]);
    ibwa_bsw2::sort_for_left(b);
    J.hits.insert(J.hits.end(), b.begin(), b.end());
    J.hoff.push_back(J.hits.size());
  }
  if (J.hits.empty()) return 0;
  HIPCHK(enter(c));
  if (int rc = run_ext(c, *opt, J, &c->aln1_stats[0], &c->aln1_stats[2], "bsw2 extend_left")) return rc;
  memcpy(hits, J.hits.data(), J.hits.size() * sizeof(AlnHit));
  return 0;
}

int ibwa_bsw2_aln1_batch(ibwa_ctx_t *c, const ibwa_bsw2_aln_opt_t *opt, int64_t n, const uint8_t *seq, const uint64_t *off,
                         const uint32_t *len, const uint8_t *is_rev, const double *u, int32_t *n_hits, ibwa_bsw2_aln_hit_t **hits,
                         int64_t *n_hits_total) {
  if (int rc = check_aln1(opt, n, seq, off, len, is_rev, u)) return rc;
  if (!hits || !n_hits_total || (n && !n_hits)) return fail(IBWA_EINVAL, "bsw2 aln1: null output");
  *hits = nullptr;
  *n_hits_total = 0;
  memset(c->aln1_stats, 0, sizeof c->aln1_stats);
  if (n == 0) {
    *hits = (ibwa_bsw2_aln_hit_t *)malloc(sizeof(ibwa_bsw2_aln_hit_t));
    return 0;
  }
  if (!c->index.pac_loaded) return fail(IBWA_ENOINDEX, "no reference sequence loaded (ibwa_ctx_load_pac)");
  if (c->index.pac_len > UINT32_MAX) return fail(IBWA_EINVAL, "bsw2 aln1: the sequence is past 2^32 bases");
  const ibwa_bsw2_opt_t &so = opt->seed;

  // 1. the seeds: task 2i is read i, task 2i + 1 its reverse complement, both on the strand is_rev[i] names
  std::vector<uint64_t> soff(2 * n);
  std::vector<uint32_t> slen(2 * n);
  std::vector<uint8_t> sstrand(2 * n);
  uint64_t tot = 0;
  for (int64_t i = 0; i < n; ++i) {
    for (int k = 0; k < 2; ++k) {
      soff[2 * i + k] = tot;
      slen[2 * i + k] = len[i];
      sstrand[2 * i + k] = is_rev[i];
      tot += len[i];
    }
  }
  std::vector<uint8_t> fwd(tot), bwd(tot);  // per task the sequence, and the sequence reversed
  for_reads(n, [&](int64_t i) {
    const uint8_t *s = seq + off[i];
    const uint32_t l = len[i];
    uint8_t *f0 = &fwd[soff[2 * i]], *f1 = &fwd[soff[2 * i + 1]], *b0 = &bwd[soff[2 * i]], *b1 = &bwd[soff[2 * i + 1]];
    for (uint32_t j = 0; j < l; ++j) {
      f0[j] = s[j];
      f1[l - 1 - j] = (uint8_t)(3 - s[j]);
      b0[l - 1 - j] = s[j];
      b1[j] = (uint8_t)(3 - s[j]);
    }
  });
  std::vector<int32_t> n_all(2 * n), n_narrow(2 * n);
  ibwa_bsw2_hit_t *seeds = nullptr;
  int64_t n_seeds = 0;
  if (int rc = ibwa_bsw2_seed_batch(c, &so, 2 * n, fwd.data(), soff.data(), slen.data(), sstrand.data(), n_all.data(), n_narrow.data(),
                                    &seeds, &n_seeds))
    return rc;
  std::vector<uint64_t> first(2 * n + 1, 0);
  for (int64_t t = 0; t < 2 * n; ++t) first[t + 1] = first[t] + (uint64_t)n_all[t] + (uint64_t)n_narrow[t];

  for (int64_t t = 0; t < 2 * n; ++t)  // here, not on a worker thread: the message is the calling thread's
    for (uint64_t j = first[t] + (uint64_t)n_all[t]; j < first[t + 1]; ++j)
      if (seeds[j].G > 32000) {
        const int G = seeds[j].G;
        ibwa_free(seeds);
        return fail(IBWA_EINVAL, "task %lld: a narrow hit's score %d is past 32000, the extension's 16-bit cells", (long long)(t / 2), G);
      }
  // 2. per read: the chain filter over the two narrow lists, then the sort the left extension starts with
  struct Read {
    ibwa_bsw2::AlnOpt o;
    std::vector<AlnHit> all[2], narrow[2];
  };
  std::vector<Read> R(n);
  for_reads(n, [&](int64_t i) {
    Read &r = R[i];
    int32_t t = so.t, bw = so.bw;
    if (so.adjust) ibwa_bsw2_opt_for_len(&so, len[i], &t, &bw);
    r.o = {{so.a, so.b, so.q, so.r, t, bw, so.z, so.is}, opt->t_seeds, opt->mask_level};
    for (int k = 0; k < 2; ++k) {
      const ibwa_bsw2::Hit *h = reinterpret_cast<const ibwa_bsw2::Hit *>(seeds) + first[2 * i + k];
      for (int32_t j = 0; j < n_all[2 * i + k]; ++j) r.all[k].push_back(ibwa_bsw2::to_aln_hit(h[j]));
      h += n_all[2 * i + k];
      for (int32_t j = 0; j < n_narrow[2 * i + k]; ++j) r.narrow[k].push_back(ibwa_bsw2::to_aln_hit(h[j]));
    }
    ibwa_bsw2::chain_filter(r.o, (int)len[i], r.narrow);
    for (int k = 0; k < 2; ++k) ibwa_bsw2::sort_for_left(r.narrow[k]);
  });
  ibwa_free(seeds);
  int rc;

  // 3. the left extension, one task per strand list
  ExtJob J;
  J.qoff = soff;
  J.qlen = slen;
  J.rev = sstrand;
  J.bw.resize(2 * n);
  J.hoff.push_back(0);
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < 2; ++k) {
      J.bw[2 * i + k] = R[i].o.seed.bw;
      J.hits.insert(J.hits.end(), R[i].narrow[k].begin(), R[i].narrow[k].end());
      J.hoff.push_back(J.hits.size());
    }
  J.qry.swap(bwd);
  if ((rc = run_ext(c, so, J, &c->aln1_stats[0], &c->aln1_stats[2], "bsw2 aln1, left extension"))) return rc;

  // 4. per read and strand: the narrow list behind the all-list, then bsw2_resolve_duphits(0, ., 0)
  for_reads(n, [&](int64_t i) {
    for (int k = 0; k < 2; ++k) {
      const AlnHit *h = J.hits.data() + J.hoff[2 * i + k];
      R[i].narrow[k].assign(h, h + (J.hoff[2 * i + k + 1] - J.hoff[2 * i + k]));
      ibwa_bsw2::merge(R[i].all[k], R[i].narrow[k], (int)len[i], 0);
      ibwa_bsw2::resolve_duphits_noindex(R[i].all[k]);
    }
  });

  // 5. the right extension: the hits are independent, so the same kernel runs them unordered, 64 hits
  // of any reads per wave, each with its read's band
  J.ordered = false;
  J.qry.swap(fwd);
  J.hits.clear();
  J.hoff.assign(1, 0);
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < 2; ++k) {
      J.hits.insert(J.hits.end(), R[i].all[k].begin(), R[i].all[k].end());
      J.hoff.push_back(J.hits.size());
    }
  int64_t right_counts[6];
  if ((rc = run_ext(c, so, J, &c->aln1_stats[1], right_counts, "bsw2 aln1, right extension"))) return rc;

  // 6. per read: the strand merge and bsw2_resolve_query_overlaps
  for_reads(n, [&](int64_t i) {
    for (int k = 0; k < 2; ++k) {
      const AlnHit *h = J.hits.data() + J.hoff[2 * i + k];
      R[i].all[k].assign(h, h + (J.hoff[2 * i + k + 1] - J.hoff[2 * i + k]));
    }
    ibwa_bsw2::merge(R[i].all[0], R[i].all[1], (int)len[i], 1);
    ibwa_bsw2::resolve_query_overlaps(R[i].all[0], opt->mask_level, u ? u[i] : 0.0);
  });
  uint64_t total = 0;
  for (int64_t i = 0; i < n; ++i) {
    n_hits[i] = (int32_t)R[i].all[0].size();
    total += R[i].all[0].size();
  }
  ibwa_bsw2_aln_hit_t *o = (ibwa_bsw2_aln_hit_t *)malloc(std::max<size_t>(1, total) * sizeof(ibwa_bsw2_aln_hit_t));
  if (!o) return fail(IBWA_EHIP, "out of host memory");
  uint64_t at = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!R[i].all[0].empty()) memcpy(o + at, R[i].all[0].data(), R[i].all[0].size() * sizeof(AlnHit));
    at += R[i].all[0].size();
  }
  *hits = o;
  *n_hits_total = (int64_t)total;
  return 0;
}

}  // extern "C"
