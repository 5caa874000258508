// engine_seed.hip -- ibwa_bsw2_seed_batch: bwasw's seeding over a batch of (sequence, index) tasks.
// The device runs bsw2_core per task (seed.hip) and expands the two hit lists to the arrays
// bsw2_resolve_duphits sorts; the unstable sort and the containment pass over those arrays are
// finish_duphits of bsw2_core.h, here on the host.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bsw2_core.h"
#include "engine_ctx.h"

using namespace ibwa;

namespace {

static_assert(sizeof(ibwa_bsw2_hit_t) == 32 && sizeof(ibwa_bsw2::Hit) == 32, "hit records are 8 words");

// words of a task's arena before its cell area (seed.hip carves the same layout)
uint64_t fixed_words(uint32_t L, int z) {
  auto r4 = [](uint64_t x) { return (x + 3) & ~3ull; };
  const uint64_t N = (uint64_t)L + 1, W = ((uint64_t)L + 15) / 16;
  uint64_t hcap = 64;
  while (hcap < 4 * N) hcap <<= 1;
  return r4(N) + r4(W) + 4 * W + r4(2ull * L * 6) + hcap * 4 + r4(2 * N + 2) + r4((2 * N + 8) * 6) + r4((uint64_t)z);
}

// The default cell area.  Over the golden vectors the host restatement's peak of live cells is 23 per
// base of read; twice that, and twice again for the power-of-two blocks the cells come
// in, with a floor that also lends the suffix sort of a read above 2 047 bases its keys.
uint64_t default_cells(uint32_t max_len) { return std::max<uint64_t>(4096, 96ull * max_len); }

int check(const ibwa_bsw2_opt_t *o, int64_t n, const uint8_t *seq, const uint64_t *off, const uint32_t *len,
          const uint8_t *strand) {
  if (!o) return fail(IBWA_EINVAL, "bsw2 seed: no options");
  if (n < 0) return fail(IBWA_EINVAL, "bsw2 seed: n < 0");
  if (o->a < 1) return fail(IBWA_EINVAL, "bsw2 seed: a %d < 1", o->a);
  if (o->b < 1) return fail(IBWA_EINVAL, "bsw2 seed: b %d < 1", o->b);
  if (o->q < 1) return fail(IBWA_EINVAL, "bsw2 seed: q %d < 1", o->q);
  if (o->r < 1) return fail(IBWA_EINVAL, "bsw2 seed: r %d < 1", o->r);
  if (o->z < 1) return fail(IBWA_EINVAL, "bsw2 seed: z %d < 1", o->z);
  if (o->is < 0) return fail(IBWA_EINVAL, "bsw2 seed: is %d < 0", o->is);
  if (!o->adjust && o->t < 1) return fail(IBWA_EINVAL, "bsw2 seed: t %d < 1 with adjust == 0", o->t);
  if (!o->adjust && o->bw < 1) return fail(IBWA_EINVAL, "bsw2 seed: bw %d < 1 with adjust == 0", o->bw);
  if (o->a > 1000 || o->b > 1000 || o->q > 1000 || o->r > 1000 || o->z > 65536)
    return fail(IBWA_EINVAL, "bsw2 seed: a, b, q, r above 1000 or z above 65536");
  if (n && (!seq || !off || !len || !strand)) return fail(IBWA_EINVAL, "bsw2 seed: null input");
  for (int64_t i = 0; i < n; ++i) {
    if (strand[i] > 1) return fail(IBWA_EINVAL, "task %lld: strand %d is above 1", (long long)i, strand[i]);
    if (len[i] == 0) return fail(IBWA_EINVAL, "task %lld: length 0", (long long)i);
    if (len[i] > IBWA_BSW2_MAX_LEN)
      return fail(IBWA_EINVAL, "task %lld: length %u is above %d", (long long)i, len[i], IBWA_BSW2_MAX_LEN);
    const uint8_t *s = seq + off[i];
    for (uint32_t j = 0; j < len[i]; ++j)
      if (s[j] >= 4) return fail(IBWA_EINVAL, "task %lld: seq[%u] = %d is not below 4", (long long)i, j, s[j]);
  }
  return 0;
}

}  // namespace

extern "C" {

int ibwa_bsw2_opt_preset(const char *name, ibwa_bsw2_opt_t *opt) {
  if (!name || strcmp(name, "bwasw") != 0) return fail(IBWA_EINVAL, "no bsw2 option preset %s", name ? name : "(null)");
  *opt = {1, 3, 5, 2, 30, 50, 1, 3, 5.5f, 1};  // bsw2_init_opt (bwtsw2_aux.c:48-57)
  return 0;
}

void ibwa_bsw2_opt_for_len(const ibwa_bsw2_opt_t *o, uint32_t len, int32_t *t, int32_t *bw) {
  int tt, b;
  ibwa_bsw2::opt_for_len(o->a, o->q, o->r, o->t, o->bw, o->coef, len, &tt, &b);
  if (t) *t = tt;
  if (bw) *bw = b;
}

int ibwa_bsw2_seed_check(const ibwa_bsw2_opt_t *opt, int64_t n, const uint8_t *seq, const uint64_t *off,
                         const uint32_t *len, const uint8_t *strand) {
  return check(opt, n, seq, off, len, strand);
}

int ibwa_bsw2_seed_stats(const ibwa_ctx_t *c, int64_t out[8]) {
  memcpy(out, c->seed_stats, sizeof c->seed_stats);
  return 0;
}

int ibwa_bsw2_seed_batch(ibwa_ctx_t *c, const ibwa_bsw2_opt_t *opt, int64_t n, const uint8_t *seq, const uint64_t *off,
                         const uint32_t *len, const uint8_t *strand, int32_t *n_all, int32_t *n_narrow,
                         ibwa_bsw2_hit_t **hits, int64_t *n_hits_total) {
  if (int rc = check(opt, n, seq, off, len, strand)) return rc;
  if (!hits || !n_hits_total || (n && (!n_all || !n_narrow))) return fail(IBWA_EINVAL, "bsw2 seed: null output");
  const bool full = (c->index.jump_ready || c->index.sa_expanded) && !c->sa_walk;
  for (int64_t i = 0; i < n; ++i) {
    const int s = strand[i];
    if (!c->index.loaded[s]) return fail(IBWA_ENOINDEX, "task %lld: the index of strand %d is not loaded", (long long)i, s);
    if (!full && !c->index.sa_loaded[s])
      return fail(IBWA_ENOINDEX, "task %lld: no suffix array of strand %d is loaded", (long long)i, s);
  }
  c->stats.ms_bsw2_seed = 0;
  c->stats.n_bsw2_retry = 0;
  c->stats.bsw2_arena_peak = 0;
  memset(c->seed_stats, 0, sizeof c->seed_stats);
  *hits = nullptr;
  *n_hits_total = 0;
  if (n == 0) {
    *hits = (ibwa_bsw2_hit_t *)malloc(sizeof(ibwa_bsw2_hit_t));
    return 0;
  }
  HIPCHK(enter(c));
  uint64_t seq_end = 0, len_sum = 0;
  uint32_t max_len = 0;
  std::vector<int32_t> ht(n), hbw(n);
  for (int64_t i = 0; i < n; ++i) {
    seq_end = std::max<uint64_t>(seq_end, off[i] + len[i]);
    len_sum += len[i];
    max_len = std::max(max_len, len[i]);
    ht[i] = opt->t;
    hbw[i] = opt->bw;
    if (opt->adjust) ibwa_bsw2_opt_for_len(opt, len[i], &ht[i], &hbw[i]);
  }
  auto &B = c->seed;
  int rc;
  if ((rc = B.seq.ensure(seq_end)) || (rc = B.off.ensure(n * 8)) || (rc = B.len.ensure(n * 4)) ||
      (rc = B.strand.ensure(n)) || (rc = B.t.ensure(n * 4)) || (rc = B.bw.ensure(n * 4)) || (rc = B.ids.ensure(n * 8)) ||
      (rc = B.res.ensure(n * 32)) || (rc = B.ctr.ensure(64)))
    return rc;
  HIPCHK(hipMemcpyAsync(B.seq.p, seq, seq_end, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(B.off.p, off, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(B.len.p, len, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(B.strand.p, strand, n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(B.t.p, ht.data(), n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(B.bw.p, hbw.data(), n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(zero_async(B.ctr.p, 64, c->stream));

  SeedArgs a = {};
  for (int s = 0; s < 2; ++s) {
    a.ix[s] = c->index.ix[s];
    a.sa[s] = full ? c->index.sa_full[s].as<uint32_t>() : c->index.sa_s[s].as<uint32_t>();
    a.intv[s] = full ? 1 : c->index.sa_intv;
  }
  a.seq = B.seq.as<uint8_t>();
  a.off = B.off.as<uint64_t>();
  a.len = B.len.as<uint32_t>();
  a.strand = B.strand.as<uint8_t>();
  a.t = B.t.as<int32_t>();
  a.bw = B.bw.as<int32_t>();
  a.a = opt->a;
  a.b = opt->b;
  a.q = opt->q;
  a.r = opt->r;
  a.z = opt->z;
  a.is = opt->is;
  a.res = B.res.as<uint32_t>();
  unsigned long long *ctr = B.ctr.as<unsigned long long>();
  a.claim = ctr;
  a.out_next = ctr + 1;
  a.prof = ctr + 2;

  std::vector<uint32_t> res(n * 8);
  std::vector<std::vector<uint32_t>> outs;  // a launch's records; res[5..6] index the launch's own buffer
  std::vector<int8_t> launch_of(n, 0);
  std::vector<int64_t> todo;
  const uint64_t fixed = fixed_words(max_len, opt->z);
  for (int pass = 0; pass < 2; ++pass) {
    const int64_t m = pass == 0 ? n : (int64_t)todo.size();
    if (m == 0) break;
    uint64_t cells = c->seed_arena_cells ? (uint64_t)c->seed_arena_cells : default_cells(max_len);
    if (pass == 1) cells = 8 * std::max<uint64_t>(cells, default_cells(max_len));
    const uint64_t arena_words = std::min<uint64_t>(fixed + cells * 16, 1ull << 30);
    // arenas of all workgroups within 32 GiB
    const int64_t blocks = std::max<int64_t>(
        1, std::min<int64_t>({m, (int64_t)c->n_cus * c->seed_waves_per_cu, (int64_t)((32ull << 30) / (arena_words * 4))}));
    // output records (32 B): the narrow hits dominate, about one per base at z = 1 and ten at z = 10 on the
    // golden vectors; the launch shares one buffer.  In the retry launch a task that ended
    // with status 2 gets the rows it counted itself (res[2] + res[4], exact: it resolved both lists
    // before it asked for room), a task that outgrew its arena 16 times the first launch's share
    const uint64_t per_base = 2 + 2 * (uint64_t)std::min(opt->z, 8);
    uint64_t out_cap = 4096;
    if (pass == 0) out_cap += (uint64_t)n * 64 + len_sum * per_base;
    else
      for (int64_t i : todo)
        out_cap += res[i * 8] == 2 ? (uint64_t)res[i * 8 + 2] + res[i * 8 + 4] : 16 * (64 + len[i] * per_base);
    if ((rc = B.arena.ensure((uint64_t)blocks * arena_words * 4)) || (rc = B.out.ensure(out_cap * 32))) return rc;
    a.arena = B.arena.as<uint32_t>();
    a.arena_words = arena_words;
    a.out = B.out.as<uint32_t>();
    a.out_cap = out_cap;
    a.n = m;
    a.ids = nullptr;
    if (pass == 1) {
      HIPCHK(hipMemcpyAsync(B.ids.p, todo.data(), m * 8, hipMemcpyHostToDevice, c->stream));
      HIPCHK(zero_async(ctr, 16, c->stream));  // the claim and output counters; the profile goes on
      a.ids = B.ids.as<int64_t>();
    }
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    HIPCHK(launch_seed(a, (int)blocks, c->stream));
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    unsigned long long hctr[8];
    HIPCHK(hipMemcpyAsync(res.data(), a.res, n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hctr, ctr, 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->stats.ms_bsw2_seed += ms;
    const uint64_t used = std::min<uint64_t>(hctr[1], out_cap);
    outs.emplace_back(used * 8);
    if (used) HIPCHK(hipMemcpy(outs.back().data(), a.out, used * 32, hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; ++k) c->seed_stats[k] = (int64_t)hctr[2 + k];
    if (pass == 0) {
      c->seed_stats[6] = (int64_t)(arena_words * 4);
      c->seed_stats[7] = blocks;
      for (int64_t i = 0; i < n; ++i)
        if (res[i * 8] != 0) todo.push_back(i);
      c->stats.n_bsw2_retry = c->seed_stats[4] = (int64_t)todo.size();
    } else {
      for (int64_t i : todo) {
        launch_of[i] = 1;
        if (res[i * 8] != 0)
          return fail(IBWA_EOVERFLOW, "task %lld (length %u): %s even in the retry launch (arena of %llu MiB)",
                      (long long)i, len[i], res[i * 8] == 2 ? "its hits do not fit the output buffer" : "it outgrows its arena",
                      (unsigned long long)(arena_words * 4 >> 20));
      }
    }
  }
  // the host's half of bsw2_resolve_duphits
  std::vector<ibwa_bsw2::Hit> b, fin, all_hits;
  int64_t peak = 0;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t *r = &res[i * 8];
    peak = std::max<int64_t>(peak, (int64_t)r[7] * 4);
    const ibwa_bsw2::Hit *rec =
        reinterpret_cast<const ibwa_bsw2::Hit *>(outs[launch_of[i]].data()) + ((uint64_t)r[6] << 32 | r[5]);
    const uint32_t pre[2] = {r[1], r[3]}, real[2] = {r[2], r[4]};
    int32_t *cnt[2] = {&n_all[i], &n_narrow[i]};
    for (int x = 0; x < 2; ++x) {
      b.assign(pre[x], ibwa_bsw2::Hit{0, 0, 0, 0, 0, 0, 0, 0});
      for (uint32_t j = 0; j < real[x]; ++j) {
        ibwa_bsw2::Hit h = rec[j];
        const uint32_t at = h.l;
        if (at >= pre[x]) return fail(IBWA_EHIP, "task %lld: a seed record outside its array", (long long)i);
        h.l = 0;
        b[at] = h;
      }
      rec += real[x];
      ibwa_bsw2::finish_duphits(b, fin);
      *cnt[x] = (int32_t)fin.size();
      all_hits.insert(all_hits.end(), fin.begin(), fin.end());
    }
  }
  c->stats.bsw2_arena_peak = c->seed_stats[5] = peak;
  *hits = (ibwa_bsw2_hit_t *)malloc(std::max<size_t>(1, all_hits.size()) * sizeof(ibwa_bsw2_hit_t));
  if (!*hits) return fail(IBWA_EHIP, "out of host memory");
  memcpy(*hits, all_hits.data(), all_hits.size() * sizeof(ibwa_bsw2_hit_t));
  *n_hits_total = (int64_t)all_hits.size();
  return 0;
}

}  // extern "C"
