// engine_post.hip -- post-alignment services: local / global alignment, the packed reference, refinement,
// MD / NM, colour space.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "engine_ctx.h"

using namespace ibwa;

namespace {
// A k_sw launch in three steps, so that its inputs may come from the host (sw_batch) or be written on
// the device (ibwa_refine_batch): sw_plan sizes the context's SW buffers (SwBufs s1 .. l2: seq1, seq2, off1,
// off2, len1, len2 -- the caller fills them on the stream), sw_launch runs the kernel, and
// sw_fetch_cigars packs and returns the CIGAR rows once the host knows their lengths.
struct SwPlan {
  int max1 = 0, max2 = 0, cap = 1, blocks = 1;
  uint64_t wpl = 0, tpl = 0;
};

int sw_plan(ibwa_ctx_t *c, int64_t n, int max1, int max2, uint64_t end1, uint64_t end2, SwPlan &P) {
  P.max1 = max1;
  P.max2 = max2;
  P.cap = std::max(1, max1 + max2);
  // the context's SW buffers, grown as needed and kept (a per-call hipMalloc / hipFree of the DP
  // scratch cost more than the kernel on a sampe batch)
  SwBufs &W = c->sw;
  P.wpl = sw_words_per_lane(max1, max2);
  P.tpl = sw_tb_per_lane(max1, max2);
  const uint64_t per_wave = (P.wpl * 4 + P.tpl) * 64;
  // a persistent grid within ~32 GiB of DP scratch (5 waves per SIMD at most: 94 VGPRs)
  const int64_t waves = std::max<int64_t>(
      1, std::min<int64_t>({(n + 63) / 64, (int64_t)((32ull << 30) / per_wave), (int64_t)c->n_cus * 20}));
  P.blocks = (int)((waves + 3) / 4);
  int rc = 0;
  if ((rc = W.s1.ensure(end1 + 16)) || (rc = W.s2.ensure(end2 + 16)) || (rc = W.o1.ensure(n * 8)) || (rc = W.o2.ensure(n * 8)) ||
      (rc = W.l1.ensure(n * 4)) || (rc = W.l2.ensure(n * 4)) || (rc = W.sc.ensure(n * 4)) || (rc = W.pl.ensure(n * 4)) ||
      (rc = W.nc.ensure(n * 4)) || (rc = W.en.ensure(n * 16)) || (rc = W.cg.ensure((uint64_t)n * P.cap * 4)) ||
      (rc = W.scr.ensure((uint64_t)P.blocks * 4 * P.wpl * 4 * 64)) || (rc = W.tbb.ensure((uint64_t)P.blocks * 4 * P.tpl * 64)) ||
      (rc = c->d_counter.ensure(64)) || (rc = W.cf.ensure(n * 8)))
    return rc;
  return 0;
}

// the kernel between the events ev[0] / ev[1], on the context's stream; no synchronisation
int sw_launch(ibwa_ctx_t *c, int64_t n, const SwPlan &P, int global_band, int gap_end) {
  SwArgs A = {};
  A.seq1 = c->sw.s1.as<uint8_t>(); A.seq2 = c->sw.s2.as<uint8_t>();
  A.off1 = c->sw.o1.as<uint64_t>(); A.off2 = c->sw.o2.as<uint64_t>();
  A.len1 = c->sw.l1.as<uint32_t>(); A.len2 = c->sw.l2.as<uint32_t>();
  A.n = n;
  A.max_len1 = P.max1;
  A.max_len2 = P.max2;
  A.scratch = c->sw.scr.as<uint32_t>(); A.words_per_lane = P.wpl;
  A.tb = c->sw.tbb.as<uint8_t>(); A.tb_per_lane = P.tpl;
  A.score = c->sw.sc.as<int32_t>(); A.path_len = c->sw.pl.as<int32_t>(); A.n_cigar = c->sw.nc.as<int32_t>();
  A.ends = c->sw.en.as<int4>();
  A.cigar = c->sw.cg.as<uint32_t>(); A.cigar_cap = P.cap;
  A.stop_after = c->sw_stop_after;
  A.global_band = global_band;
  A.gap_end = gap_end;
  HIPCHK(hipEventRecord(c->ev[0], c->stream));
  HIPCHK(launch_sw(A, counter(c, CTR_CLAIM), P.blocks, c->stream));
  HIPCHK(hipEventRecord(c->ev[1], c->stream));
  return 0;
}

// the CIGARs packed on the device (row p's n_cigar[p] words at its prefix offset), one copy back
int sw_fetch_cigars(ibwa_ctx_t *c, int64_t n, const SwPlan &P, const int32_t *n_cigar, uint32_t **cigar,
                    int64_t *n_cigar_total) {
  SwBufs &W = c->sw;
  int rc = 0;
  auto chk = [&](hipError_t e, const char *what) {
    if (e != hipSuccess && !rc) rc = fail(IBWA_EHIP, "%s: %s", what, hipGetErrorString(e));
  };
  std::vector<uint64_t> first(n);
  int64_t tot = 0;
  for (int64_t p = 0; p < n; ++p) {
    first[p] = (uint64_t)tot;
    tot += n_cigar[p];
  }
  uint32_t *o = (uint32_t *)malloc(std::max<int64_t>(tot, 1) * 4);
  if (!o) return fail(IBWA_EINVAL, "out of host memory");
  if (tot) {
    if ((rc = W.cc.ensure((uint64_t)tot * 4))) { free(o); return rc; }
    chk(hipMemcpyAsync(W.cf.p, first.data(), n * 8, hipMemcpyHostToDevice, c->stream), "H2D cigar offsets");
    chk(launch_pack_cigar(W.cg.as<uint32_t>(), P.cap, W.nc.as<int32_t>(), W.cf.as<uint64_t>(), n, W.cc.as<uint32_t>(), c->stream),
        "k_pack_cigar");
    chk(hipMemcpyAsync(o, W.cc.p, (uint64_t)tot * 4, hipMemcpyDeviceToHost, c->stream), "D2H cigar");
    chk(hipStreamSynchronize(c->stream), "sync");
    if (rc) { free(o); return rc; }
  }
  *cigar = o;
  if (n_cigar_total) *n_cigar_total = tot;
  return 0;
}

// k_sw launch over host arrays: the local core (global_band == 0) or aln_global_core alone
int sw_batch(ibwa_ctx_t *c, int64_t n, const uint8_t *ref, const uint64_t *off1, const uint32_t *len1,
             const uint8_t *qry, const uint64_t *off2, const uint32_t *len2, int global_band, int gap_end,
             int32_t *score, int32_t *path_len, int32_t *ends, int32_t *n_cigar, uint32_t **cigar,
             int64_t *n_cigar_total) {
  if (n < 0) return fail(IBWA_EINVAL, "negative pair count");
  *cigar = nullptr;
  if (n_cigar_total) *n_cigar_total = 0;
  if (n == 0) {
    *cigar = (uint32_t *)malloc(4);
    return 0;
  }
  HIPCHK(enter(c));
  int max1 = 0, max2 = 0;
  uint64_t end1 = 0, end2 = 0;
  for (int64_t p = 0; p < n; ++p) {
    if (!global_band && std::min(len1[p], len2[p]) * 11ull > 32000)
      return fail(IBWA_EINVAL, "pair %lld: min(len1, len2) * 11 > 32000", (long long)p);
    if (global_band && (uint64_t)len1[p] * len2[p] > (64ull << 20))
      return fail(IBWA_EINVAL, "pair %lld: %u x %u cells is past the traceback bound", (long long)p, len1[p], len2[p]);
    max1 = std::max<int>(max1, (int)len1[p]);
    max2 = std::max<int>(max2, (int)len2[p]);
    end1 = std::max<uint64_t>(end1, off1[p] + len1[p]);
    end2 = std::max<uint64_t>(end2, off2[p] + len2[p]);
  }
  SwPlan P;
  if (int rc = sw_plan(c, n, max1, max2, end1, end2, P)) return rc;
  SwBufs &W = c->sw;
  int rc = 0;
  auto chk = [&](hipError_t e, const char *what) {
    if (e != hipSuccess && !rc) rc = fail(IBWA_EHIP, "%s: %s", what, hipGetErrorString(e));
  };
  chk(hipMemcpyAsync(W.s1.p, ref, end1, hipMemcpyHostToDevice, c->stream), "H2D ref");
  chk(hipMemcpyAsync(W.s2.p, qry, end2, hipMemcpyHostToDevice, c->stream), "H2D qry");
  chk(hipMemcpyAsync(W.o1.p, off1, n * 8, hipMemcpyHostToDevice, c->stream), "H2D off1");
  chk(hipMemcpyAsync(W.o2.p, off2, n * 8, hipMemcpyHostToDevice, c->stream), "H2D off2");
  chk(hipMemcpyAsync(W.l1.p, len1, n * 4, hipMemcpyHostToDevice, c->stream), "H2D len1");
  chk(hipMemcpyAsync(W.l2.p, len2, n * 4, hipMemcpyHostToDevice, c->stream), "H2D len2");
  if (!rc) rc = sw_launch(c, n, P, global_band, gap_end);
  if (!rc) {
    chk(hipMemcpyAsync(score, W.sc.p, n * 4, hipMemcpyDeviceToHost, c->stream), "D2H score");
    chk(hipMemcpyAsync(path_len, W.pl.p, n * 4, hipMemcpyDeviceToHost, c->stream), "D2H path_len");
    chk(hipMemcpyAsync(n_cigar, W.nc.p, n * 4, hipMemcpyDeviceToHost, c->stream), "D2H n_cigar");
    chk(hipMemcpyAsync(ends, W.en.p, n * 16, hipMemcpyDeviceToHost, c->stream), "D2H ends");
    chk(hipStreamSynchronize(c->stream), "sync");
    float ms = 0;
    if (!rc && hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->stats.ms_sw = ms;
  }
  if (rc) return rc;
  return sw_fetch_cigars(c, n, P, n_cigar, cigar, n_cigar_total);
}
}  // namespace

extern "C" {

int ibwa_sw_batch(ibwa_ctx_t *c, int64_t n, const uint8_t *ref, const uint64_t *off1, const uint32_t *len1,
                  const uint8_t *qry, const uint64_t *off2, const uint32_t *len2, int32_t *score,
                  int32_t *path_len, int32_t *ends, int32_t *n_cigar, uint32_t **cigar, int64_t *n_cigar_total) {
  return sw_batch(c, n, ref, off1, len1, qry, off2, len2, 0, -1, score, path_len, ends, n_cigar, cigar, n_cigar_total);
}

int ibwa_global_batch(ibwa_ctx_t *c, int64_t n, const uint8_t *ref, const uint64_t *off1, const uint32_t *len1,
                      const uint8_t *qry, const uint64_t *off2, const uint32_t *len2, int band, int gap_end,
                      int32_t *score, int32_t *path_len, int32_t *n_cigar, uint32_t **cigar, int64_t *n_cigar_total) {
  if (band <= 0) return fail(IBWA_EINVAL, "band must be > 0");
  std::vector<int32_t> ends(4 * std::max<int64_t>(n, 1));
  return sw_batch(c, n, ref, off1, len1, qry, off2, len2, band, gap_end, score, path_len, ends.data(), n_cigar, cigar,
                  n_cigar_total);
}

// the n_db references' .pac bytes back to back into `dst` (ibwa_ctx_load_pac / ibwa_ctx_load_ntpac)
static int load_pac_set(ibwa_ctx_t *c, int n_db, const uint8_t *const *pac, const uint64_t *l_pac, DBuf &dst, uint64_t &dst_len,
                        bool &dst_loaded) {
  HIPCHK(enter(c));
  // the references' own bytes side by side (8 B-aligned starts), then the shifting concatenation
  std::vector<uint64_t> tab(2 * (size_t)n_db + 1);
  uint64_t *byte_off = tab.data(), *base_off = tab.data() + n_db;
  uint64_t bytes = 0, total = 0;
  for (int d = 0; d < n_db; ++d) {
    if (l_pac[d] && !pac[d]) return fail(IBWA_EINVAL, "load_pac: reference %d has no bytes", d);
    byte_off[d] = bytes;
    base_off[d] = total;
    bytes += ((l_pac[d] + 3) / 4 + 7) & ~7ull;
    total += l_pac[d];
  }
  base_off[n_db] = total;
  const uint64_t words = (total + 15) / 16;
  DBuf src, dtab;
  int rc = 0;
  if ((rc = dst.ensure((words + 1) * 4)) || (rc = src.ensure(bytes + 8)) || (rc = dtab.ensure(tab.size() * 8))) return rc;
  auto chk = [&](hipError_t e, const char *what) {
    if (e != hipSuccess && !rc) rc = fail(IBWA_EHIP, "load_pac %s: %s", what, hipGetErrorString(e));
  };
  dst_loaded = false;
  for (int d = 0; d < n_db; ++d)
    if (l_pac[d])
      chk(hipMemcpyAsync(src.as<uint8_t>() + byte_off[d], pac[d], (l_pac[d] + 3) / 4, hipMemcpyHostToDevice, c->stream), "H2D");
  chk(hipMemcpyAsync(dtab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream), "H2D offsets");
  // one word more than the sequence needs stays zero
  chk(launch_pac_concat(src.as<uint8_t>(), dtab.as<uint64_t>(), dtab.as<uint64_t>() + n_db, n_db, dst.as<uint32_t>(),
                        words + 1, c->stream), "k_pac_concat");
  chk(hipStreamSynchronize(c->stream), "sync");
  if (rc) return rc;
  dst_len = total;
  dst_loaded = true;
  return 0;
}

int ibwa_ctx_load_pac(ibwa_ctx_t *c, int n_db, const uint8_t *const *pac, const uint64_t *l_pac) {
  if (!c || n_db <= 0 || !pac || !l_pac) return fail(IBWA_EINVAL, "load_pac: bad arguments");
  if (int rc = refuse_shared(c, "load_pac")) return rc;
  return load_pac_set(c, n_db, pac, l_pac, c->index.pac, c->index.pac_len, c->index.pac_loaded);
}

int ibwa_ctx_load_ntpac(ibwa_ctx_t *c, int n_db, const uint8_t *const *pac, const uint64_t *l_pac) {
  if (!c || n_db <= 0 || !pac || !l_pac) return fail(IBWA_EINVAL, "load_ntpac: bad arguments");
  if (int rc = refuse_shared(c, "load_ntpac")) return rc;
  return load_pac_set(c, n_db, pac, l_pac, c->index.ntpac, c->index.ntpac_len, c->index.ntpac_loaded);
}

int ibwa_pac_extract(ibwa_ctx_t *c, int64_t n, const uint64_t *beg, const uint32_t *len, const uint64_t *out_off,
                     uint8_t *out, uint32_t *got) {
  if (!c || n < 0) return fail(IBWA_EINVAL, "pac_extract: bad arguments");
  if (!c->index.pac_loaded) return fail(IBWA_ENOINDEX, "no reference sequence loaded (ibwa_ctx_load_pac)");
  if (n == 0) return 0;
  HIPCHK(enter(c));
  uint64_t end = 0;
  for (int64_t p = 0; p < n; ++p) end = std::max<uint64_t>(end, out_off[p] + len[p]);
  DBuf &db = c->rf.dpos, &dl = c->rf.dext, &dg = c->rf.dout, &dof = c->sw.o1, &dout = c->sw.s1;
  int rc = 0;
  if ((rc = db.ensure(n * 8)) || (rc = dl.ensure(n * 4)) || (rc = dg.ensure(n * 8)) || (rc = dof.ensure(n * 8)) ||
      (rc = dout.ensure(end + 16)))
    return rc;
  HIPCHK(hipMemcpyAsync(db.p, beg, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dl.p, len, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dof.p, out_off, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(zero_async(dout.p, end, c->stream));
  HIPCHK(launch_pac_gather(c->index.pac.as<uint32_t>(), c->index.pac_len, n, db.as<uint64_t>(), dl.as<uint32_t>(), dof.as<uint64_t>(),
                           dout.as<uint8_t>(), dg.as<uint32_t>(), c->stream));
  if (end) HIPCHK(hipMemcpyAsync(out, dout.p, end, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(got, dg.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ibwa_refine_batch(ibwa_ctx_t *c, int64_t n, const uint64_t *pos, const int32_t *ext, const uint8_t *seq,
                      const uint64_t *off, const uint32_t *len, uint64_t *pos_out, int32_t *n_cigar, uint32_t **cigar,
                      int64_t *n_cigar_total) {
  if (!c || n < 0 || !cigar) return fail(IBWA_EINVAL, "refine_batch: bad arguments");
  if (!c->index.pac_loaded) return fail(IBWA_ENOINDEX, "no reference sequence loaded (ibwa_ctx_load_pac)");
  // the windows' sizes before clipping: where each window goes and how large the fill can get
  std::vector<uint64_t> off1((size_t)std::max<int64_t>(n, 1));
  int max1 = 0, max2 = 0;
  uint64_t end1 = 0, end2 = 0;
  for (int64_t p = 0; p < n; ++p) {
    if (pos[p] > c->index.pac_len)  // bwase.c:179-181
      return fail(IBWA_EINVAL, "[refine_gapped_core] job %lld: position=%llu > l_pac=%llu", (long long)p,
                  (unsigned long long)pos[p], (unsigned long long)c->index.pac_len);
    const uint64_t w = (uint64_t)len[p] + (uint64_t)std::abs((int64_t)ext[p]);
    if (w > 0x7fffffffull || w * len[p] > (64ull << 20))
      return fail(IBWA_EINVAL, "job %lld: %llu x %u cells is past the traceback bound", (long long)p, (unsigned long long)w,
                  len[p]);
    off1[p] = end1;
    end1 += w;
    max1 = std::max<int>(max1, (int)w);
    max2 = std::max<int>(max2, (int)len[p]);
    end2 = std::max<uint64_t>(end2, off[p] + len[p]);
  }
  *cigar = nullptr;
  if (n_cigar_total) *n_cigar_total = 0;
  if (n == 0) {
    *cigar = (uint32_t *)malloc(4);
    return 0;
  }
  HIPCHK(enter(c));
  SwPlan P;
  if (int rc = sw_plan(c, n, max1, max2, end1, end2, P)) return rc;
  SwBufs &W = c->sw;
  RefineBufs &F = c->rf;
  int rc = 0;
  if ((rc = F.dpos.ensure(n * 8)) || (rc = F.dext.ensure(n * 4)) || (rc = F.dout.ensure(n * 8))) return rc;
  auto chk = [&](hipError_t e, const char *what) {
    if (e != hipSuccess && !rc) rc = fail(IBWA_EHIP, "%s: %s", what, hipGetErrorString(e));
  };
  chk(hipMemcpyAsync(F.dpos.p, pos, n * 8, hipMemcpyHostToDevice, c->stream), "H2D pos");
  chk(hipMemcpyAsync(F.dext.p, ext, n * 4, hipMemcpyHostToDevice, c->stream), "H2D ext");
  chk(hipMemcpyAsync(W.s2.p, seq, end2, hipMemcpyHostToDevice, c->stream), "H2D reads");
  chk(hipMemcpyAsync(W.o1.p, off1.data(), n * 8, hipMemcpyHostToDevice, c->stream), "H2D window offsets");
  chk(hipMemcpyAsync(W.o2.p, off, n * 8, hipMemcpyHostToDevice, c->stream), "H2D read offsets");
  chk(hipMemcpyAsync(W.l2.p, len, n * 4, hipMemcpyHostToDevice, c->stream), "H2D read lengths");
  chk(launch_refine_gather(c->index.pac.as<uint32_t>(), c->index.pac_len, n, F.dpos.as<uint64_t>(), F.dext.as<int32_t>(), W.l2.as<uint32_t>(),
                           W.o1.as<uint64_t>(), W.s1.as<uint8_t>(), W.l1.as<uint32_t>(), c->stream), "k_refine_gather");
  if (!rc) rc = sw_launch(c, n, P, 50, 5);  // aln_param_bwa: band 50, gap_end 5 (stdaln.c:227)
  if (!rc)
    chk(launch_refine_fixup(n, F.dpos.as<uint64_t>(), F.dext.as<int32_t>(), W.cg.as<uint32_t>(), P.cap, W.nc.as<int32_t>(),
                            F.dout.as<uint64_t>(), c->stream), "k_refine_fixup");
  // the results land in the caller's arrays only once every step succeeded
  std::vector<uint64_t> h_pos((size_t)n);
  std::vector<int32_t> h_nc((size_t)n);
  chk(hipMemcpyAsync(h_pos.data(), F.dout.p, n * 8, hipMemcpyDeviceToHost, c->stream), "D2H pos");
  chk(hipMemcpyAsync(h_nc.data(), W.nc.p, n * 4, hipMemcpyDeviceToHost, c->stream), "D2H n_cigar");
  chk(hipStreamSynchronize(c->stream), "sync");
  if (rc) return rc;
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->stats.ms_sw = ms;
  if ((rc = sw_fetch_cigars(c, n, P, h_nc.data(), cigar, n_cigar_total))) return rc;
  memcpy(pos_out, h_pos.data(), (size_t)n * 8);
  memcpy(n_cigar, h_nc.data(), (size_t)n * 4);
  return 0;
}

int ibwa_md_batch(ibwa_ctx_t *c, int64_t n, const uint64_t *pos, const uint8_t *seq, const uint64_t *off,
                  const uint32_t *len, const int32_t *n_cigar, const uint32_t *cigar, int32_t *nm, uint64_t **md_off,
                  const char **md) {
  if (!c || n < 0 || !md_off || !md) return fail(IBWA_EINVAL, "md_batch: bad arguments");
  if (!c->index.pac_loaded) return fail(IBWA_ENOINDEX, "no reference sequence loaded (ibwa_ctx_load_pac)");
  *md_off = nullptr;
  *md = nullptr;
  std::vector<uint64_t> cig_off((size_t)n + 1, 0);
  uint64_t end = 0;
  for (int64_t p = 0; p < n; ++p) {
    cig_off[p + 1] = cig_off[p] + (uint64_t)(n_cigar && n_cigar[p] > 0 ? n_cigar[p] : 0);
    end = std::max<uint64_t>(end, off[p] + len[p]);
  }
  const uint64_t n_cig = cig_off[n];
  if (n == 0) {
    uint64_t *o = (uint64_t *)calloc(2, 8);
    if (!o) return fail(IBWA_EINVAL, "out of host memory");
    *md_off = o;
    *md = (const char *)(o + 1);
    return 0;
  }
  HIPCHK(enter(c));
  MdBufs &M = c->md;
  size_t tmp_bytes = 0;
  HIPCHK(md_scan_sizes(nullptr, n, nullptr, &tmp_bytes, c->stream));
  int rc = 0;
  if ((rc = M.dpos.ensure(n * 8)) || (rc = M.dseq.ensure(end + 16)) || (rc = M.doff.ensure(n * 8)) || (rc = M.dlen.ensure(n * 4)) ||
      (rc = M.dnc.ensure(n * 4)) || (rc = M.dco.ensure((n + 1) * 8)) || (rc = M.dcg.ensure((n_cig + 1) * 4)) ||
      (rc = M.dto.ensure((n + 1) * 8)) || (rc = M.dnm.ensure(n * 4)) || (rc = M.dtmp.ensure(std::max<size_t>(tmp_bytes, 256))))
    return rc;
  HIPCHK(hipMemcpyAsync(M.dpos.p, pos, n * 8, hipMemcpyHostToDevice, c->stream));
  if (end) HIPCHK(hipMemcpyAsync(M.dseq.p, seq, end, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(M.doff.p, off, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(M.dlen.p, len, n * 4, hipMemcpyHostToDevice, c->stream));
  if (n_cigar) {
    HIPCHK(hipMemcpyAsync(M.dnc.p, n_cigar, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(M.dco.p, cig_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n_cig) HIPCHK(hipMemcpyAsync(M.dcg.p, cigar, n_cig * 4, hipMemcpyHostToDevice, c->stream));
  }
  MdArgs A = {};
  A.pac = c->index.pac.as<uint32_t>();
  A.l_pac = c->index.pac_len;
  A.n = n;
  A.pos = M.dpos.as<uint64_t>();
  A.seq = M.dseq.as<uint8_t>();
  A.off = M.doff.as<uint64_t>();
  A.len = M.dlen.as<uint32_t>();
  A.n_cigar = n_cigar ? M.dnc.as<int32_t>() : nullptr;
  A.cig_off = M.dco.as<uint64_t>();
  A.cigar = M.dcg.as<uint32_t>();
  A.text_off = M.dto.as<uint64_t>();
  A.nm = M.dnm.as<int32_t>();
  // sizing pass, exclusive scan, writing pass
  HIPCHK(launch_md(A, false, c->stream));
  HIPCHK(md_scan_sizes(A.text_off, n, M.dtmp.p, &tmp_bytes, c->stream));
  uint64_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, A.text_off + n, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if ((rc = M.dtx.ensure(total + 16))) return rc;
  A.text = M.dtx.as<char>();
  HIPCHK(launch_md(A, true, c->stream));
  // one allocation: the n + 1 offsets, then the texts
  uint64_t *o = (uint64_t *)malloc((size_t)(n + 1) * 8 + total + 1);
  if (!o) return fail(IBWA_EINVAL, "out of host memory");
  hipError_t e = hipMemcpyAsync(o, M.dto.p, (n + 1) * 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(o + n + 1, M.dtx.p, total, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(nm, M.dnm.p, n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    free(o);
    return fail(IBWA_EHIP, "md_batch: %s", hipGetErrorString(e));
  }
  *md_off = o;
  *md = (const char *)(o + n + 1);
  return 0;
}

int ibwa_pac2cspac(ibwa_ctx_t *c, const uint8_t *nt_pac, uint64_t l_pac, uint8_t *cs_pac_out) {
  if (!c || !nt_pac || !cs_pac_out || l_pac == 0) return fail(IBWA_EINVAL, "pac2cspac: bad arguments");
  HIPCHK(enter(c));
  const uint64_t in_bytes = (l_pac + 3) / 4, out_bytes = l_pac / 4 + 1, words = (l_pac + 15) / 16;
  DBuf &din = c->cs.din, &dout = c->cs.dout_cs;
  int rc = 0;
  // one word more than the sequence needs: l_pac / 4 + 1 bytes can end in the word after the last base
  if ((rc = din.ensure((words + 1) * 4)) || (rc = dout.ensure((words + 1) * 4))) return rc;
  HIPCHK(zero_async(din.as<uint8_t>() + (words - 1) * 4, 8, c->stream));
  HIPCHK(hipMemcpyAsync(din.p, nt_pac, in_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(launch_pac2cs(din.as<uint32_t>(), l_pac, dout.as<uint32_t>(), words + 1, c->stream));
  HIPCHK(hipMemcpyAsync(cs_pac_out, dout.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

namespace {
// the launches of k_cs2nt over n jobs whose per-job arrays are on the device: the position-major
// scratch holds `lanes` jobs at a time (at most CS_SCRATCH bytes), so a large batch takes several
constexpr uint64_t CS_SCRATCH = 512ull << 20;
int cs2nt_run(ibwa_ctx *c, Cs2ntArgs &A, uint32_t max_size, bool from_pac) {
  const uint64_t per_lane = 2 * ((uint64_t)max_size + 1);
  int64_t lanes = (A.n + 255) & ~255ll;
  lanes = std::min<int64_t>(lanes, std::max<int64_t>(256, (int64_t)(CS_SCRATCH / per_lane) & ~255ll));
  DBuf &dbt = c->cs.dbt;
  if (int rc = dbt.ensure(per_lane * (uint64_t)lanes)) return rc;
  A.lanes = lanes;
  A.bt = dbt.as<uint8_t>();
  A.cs = A.bt + ((uint64_t)max_size + 1) * (uint64_t)lanes;
  for (A.first = 0; A.first < A.n; A.first += lanes) HIPCHK(launch_cs2nt(A, from_pac, c->stream));
  return 0;
}
}  // namespace

int ibwa_cs2nt_rows(ibwa_ctx_t *c, int64_t n, const uint8_t *nt_ref, const uint8_t *cs_read, const uint64_t *off,
                    const uint32_t *size, uint8_t *out, const uint64_t *out_off) {
  if (!c || n < 0 || (n && (!nt_ref || !cs_read || !off || !size || !out || !out_off)))
    return fail(IBWA_EINVAL, "cs2nt_rows: bad arguments");
  uint64_t end = 0, out_end = 0;
  uint32_t max_size = 0;
  for (int64_t p = 0; p < n; ++p) {
    if (size[p] == 0 || size[p] > 0x7ffffffeu)  // cs2nt_nt_qual's loop (cs2nt.c:95) does not end at size 0
      return fail(IBWA_EINVAL, "cs2nt_rows: job %lld has size %u", (long long)p, size[p]);
    end = std::max<uint64_t>(end, off[p] + size[p] + 1);
    out_end = std::max<uint64_t>(out_end, out_off[p] + size[p] - 1);
    max_size = std::max(max_size, size[p]);
  }
  if (n == 0) return 0;
  HIPCHK(enter(c));
  DBuf &dref = c->cs.dseq, &dcs = c->cs.dq, &doff = c->cs.doff, &dsz = c->cs.dsz, &dout = c->cs.dout, &doo = c->cs.dpos;
  int rc = 0;
  if ((rc = dref.ensure(end)) || (rc = dcs.ensure(end)) || (rc = doff.ensure(n * 8)) || (rc = dsz.ensure(n * 4)) ||
      (rc = dout.ensure(out_end + 16)) || (rc = doo.ensure(n * 8)))
    return rc;
  HIPCHK(hipMemcpyAsync(dref.p, nt_ref, end, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dcs.p, cs_read, end - 1, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(doff.p, off, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dsz.p, size, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(doo.p, out_off, n * 8, hipMemcpyHostToDevice, c->stream));
  Cs2ntArgs A = {};
  A.n = n;
  A.size = dsz.as<uint32_t>();
  A.off = doff.as<uint64_t>();
  A.out = dout.as<uint8_t>();
  A.out_off = doo.as<uint64_t>();
  A.nt_ref = dref.as<uint8_t>();
  A.cs_read = dcs.as<uint8_t>();
  if ((rc = cs2nt_run(c, A, max_size, false))) return rc;
  // only the jobs' own size - 1 bytes are the caller's to overwrite
  std::vector<uint8_t> h(out_end);
  if (out_end) HIPCHK(hipMemcpyAsync(h.data(), dout.p, out_end, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int64_t p = 0; p < n; ++p) memcpy(out + out_off[p], h.data() + out_off[p], size[p] - 1);
  return 0;
}

int ibwa_cs2nt_batch(ibwa_ctx_t *c, int64_t n, const uint64_t *pos, const uint8_t *strand, const uint8_t *seq,
                     const uint8_t *qual, const uint64_t *off, const uint32_t *len, const int32_t *n_cigar,
                     const uint32_t *cigar, uint8_t *out, uint32_t *new_len) {
  if (!c || n < 0 || (n && (!pos || !strand || !seq || !qual || !off || !len || !out || !new_len)))
    return fail(IBWA_EINVAL, "cs2nt_batch: bad arguments");
  if (!c->index.ntpac_loaded) return fail(IBWA_ENOINDEX, "no nucleotide sequence loaded (ibwa_ctx_load_ntpac)");
  if (n == 0) return 0;
  // the rows' sizes (cs2nt.c:143-171: every M and I colour), checked against the read
  std::vector<uint32_t> size((size_t)n);
  std::vector<uint64_t> cig_off((size_t)n + 1, 0);
  std::vector<int32_t> nc((size_t)n, 0);
  uint64_t end = 0;
  uint32_t max_size = 0;
  for (int64_t p = 0; p < n; ++p) {
    nc[p] = n_cigar && n_cigar[p] > 0 ? n_cigar[p] : 0;
    cig_off[p + 1] = cig_off[p] + (uint64_t)nc[p];
    uint64_t rows = len[p], used = len[p];
    if (nc[p]) {
      if (!cigar) return fail(IBWA_EINVAL, "cs2nt_batch: read %lld has a CIGAR count and no CIGAR", (long long)p);
      rows = used = 0;
      for (int k = 0; k < nc[p]; ++k) {
        const uint32_t w = cigar[cig_off[p] + k], op = w >> 29, l = w & 0x1fffffffu;
        if (op > 3) return fail(IBWA_EINVAL, "cs2nt_batch: read %lld: CIGAR operation %u", (long long)p, op);
        if (op == 0 || op == 1) rows += l;
        if (op != 2) used += l;
      }
    }
    if (rows == 0 || used > len[p])
      return fail(IBWA_EINVAL, "cs2nt_batch: read %lld: %llu row colours, %llu of %u read colours used", (long long)p,
                  (unsigned long long)rows, (unsigned long long)used, len[p]);
    size[p] = (uint32_t)rows;
    max_size = std::max(max_size, size[p]);
    end = std::max<uint64_t>(end, off[p] + len[p]);
  }
  const uint64_t n_cig = cig_off[n];
  HIPCHK(enter(c));
  CsBufs &S = c->cs;
  int rc = 0;
  if ((rc = S.dseq.ensure(end)) || (rc = S.dq.ensure(end)) || (rc = S.doff.ensure(n * 8)) || (rc = S.dsz.ensure(n * 4)) ||
      (rc = S.dout.ensure(end + 16)) || (rc = S.dpos.ensure(n * 8)) || (rc = S.dst.ensure(n)) || (rc = S.dlen.ensure(n * 4)) ||
      (rc = S.dnc.ensure(n * 4)) || (rc = S.dco.ensure((n + 1) * 8)) || (rc = S.dcg.ensure((n_cig + 1) * 4)))
    return rc;
  HIPCHK(hipMemcpyAsync(S.dseq.p, seq, end, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(S.dq.p, qual, end, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(S.doff.p, off, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(S.dsz.p, size.data(), n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(S.dpos.p, pos, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(S.dst.p, strand, n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(S.dlen.p, len, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(S.dnc.p, nc.data(), n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(S.dco.p, cig_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
  if (n_cig) HIPCHK(hipMemcpyAsync(S.dcg.p, cigar, n_cig * 4, hipMemcpyHostToDevice, c->stream));
  Cs2ntArgs A = {};
  A.n = n;
  A.size = S.dsz.as<uint32_t>();
  A.off = S.doff.as<uint64_t>();
  A.out = S.dout.as<uint8_t>();
  A.out_off = S.doff.as<uint64_t>();  // a read's bases go where its colours were: size - 1 < len
  A.pac = c->index.ntpac.as<uint32_t>();
  A.l_pac = c->index.ntpac_len;
  A.pos = S.dpos.as<uint64_t>();
  A.strand = S.dst.as<uint8_t>();
  A.seq = S.dseq.as<uint8_t>();
  A.qual = S.dq.as<uint8_t>();
  A.len = S.dlen.as<uint32_t>();
  A.n_cigar = S.dnc.as<int32_t>();
  A.cig_off = S.dco.as<uint64_t>();
  A.cigar = S.dcg.as<uint32_t>();
  if ((rc = cs2nt_run(c, A, max_size, true))) return rc;
  std::vector<uint8_t> h(end);
  HIPCHK(hipMemcpyAsync(h.data(), S.dout.p, end, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int64_t p = 0; p < n; ++p) {
    memcpy(out + off[p], h.data() + off[p], size[p] - 1);
    new_len[p] = size[p] - 1;
  }
  return 0;
}

}  // extern "C"
