// engine_index.hip -- the index set of a context: load, export, clone, share and build; the tables and
// jump arrays derived from it; SA row -> coordinate.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "engine_ctx.h"

using namespace ibwa;

namespace ibwa {

// (Re)build the K-mer tables for the resident index if needed.
int ensure_kmer(ibwa_ctx *c) {
  if (c->index.kmer_valid) return 0;
  if (int rc = refuse_shared(c, "K-mer tables")) return rc;
  int K = c->kmer_k;
  if (K < 0) {
    // auto: K ~ log4(2n) (past that most K-mers are absent), up to 15 (2 x 8.6 GB for a
    // human genome; K = 16 measured slower: 2 x 34 GB of randomly probed tables),
    // and both tables within 40 % of the free HBM
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    K = 1;
    // at most 14: K = 15 tables (2 x 8.6 GB at GRCh37 size) bought nothing over 14 (2 x 2.1 GB):
    // 5 311 vs 5 316 ms per 50 M-read step, profiles/r05_sweep_mem.jsonl
    while (K < 14 && (1ull << (2 * (K + 1))) <= 2ull * c->index.ix[0].seq_len &&
           2ull * 8ull * (1ull << (2 * (K + 1))) <= (uint64_t)(0.4 * (double)free_b))
      ++K;
  }
  if (K > 16) K = 16;
  c->index.kmer_K = 0;
  // bit-plane Occ layouts (occ64.hip), 1 byte per BWT row and strand
  for (int s = 0; s < 2; ++s) {
    if (int rc = c->index.o64[s].ensure(occ64_blocks(c->index.ix[s].seq_len) * 64)) return rc;
    HIPCHK(build_occ64(c->index.ix[s], c->index.o64[s].as<uint4>(), c->stream));
  }
  if (K > 0) {
    DBuf tmp;
    if (int rc = tmp.ensure((1ull << (2 * (K - 1))) * 8)) return rc;
    for (int s = 0; s < 2; ++s) {
      if (int rc = c->index.kt[s].ensure((1ull << (2 * K)) * 8)) return rc;
      hipError_t e = build_kmer_table(c->index.ix[s], K, c->index.kt[s].as<uint2>(), tmp.as<uint2>(), c->stream);
      if (e != hipSuccess) return fail(IBWA_EHIP, "K-mer table: %s", hipGetErrorString(e));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->index.kmer_K = K;
  }
  c->index.ltab_K = 0;
  int TK = c->gap_tab_k;
  if (TK < 0) {
    // auto: as deep as strings of that length still mostly occur, at most 13 (2 x 2.9 GB at GRCh37
    // size); 14 (2 x 11.5 GB) when both tables take at most 15 % of the free HBM: k_gapped 1 935 ->
    // 1 844 ms per 50 M-read step (profiles/r06_sweep_tab2.jsonl).  The CLI pins its K (aln_main.cpp).
    TK = 0;
    while (TK < 13 && (1ull << (2 * (TK + 1))) <= (uint64_t)c->index.ix[0].seq_len) ++TK;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    if (TK == 13 && (1ull << 30) <= (uint64_t)c->index.ix[0].seq_len &&
        2.0 * 8.0 * (double)ltab_off(16) <= 0.15 * (double)free_b)
      TK = 14;
  }
  if (TK > 0 && c->index.ix[0].seq_len < LTAB_MARK) {
    for (int s = 0; s < 2; ++s) {
      if (int rc = c->index.ltab[s].ensure(ltab_off((uint32_t)TK + 2) * 8)) return rc;
      hipError_t e = build_level_tables(c->index.ix[s], TK + 1, c->index.ltab[s].as<uint2>(), c->stream);
      if (e != hipSuccess) return fail(IBWA_EHIP, "level tables: %s", hipGetErrorString(e));
    }
    c->index.ltab_K = TK;
  }
  c->index.kmer_valid = true;
  return 0;
}
// The exact path's unique-interval jump needs the full SA, the ISA and the 2-bit text of both
// strands.  An index built here keeps them (ibwa_ctx_build_index); for an index loaded from .bwt
// files (the drop-in, the CLI) they are derived on the device from the BWT alone: the sampled SA
// by an LF walk between marked rows plus list ranking, then the full SA (k_expand_sa), the ISA
// (a scatter) and the text (a gather through the ISA).  Skipped when HBM is short: the exact path
// then runs without the jump (same results).
int derive_sa_locked(ibwa_ctx *c, uint32_t intv) {
  if (c->share_src) return fail(IBWA_EINVAL, "sampled SA: this context shares another context's index");
  HIPCHK(enter(c));
  for (int s = 0; s < 2; ++s) {
    const uint64_t n_nodes = ((uint64_t)c->index.ix[s].seq_len + intv) / intv;
    DBuf tmp;
    if (int rc = tmp.ensure((4 * n_nodes + 1) * 4)) return rc;
    if (int rc = c->index.sa_s[s].ensure(n_nodes * 4)) return rc;
    hipError_t e = derive_sampled_sa(c->index.ix[s], intv, c->index.sa_s[s].as<uint32_t>(), tmp.as<uint32_t>(), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(IBWA_EHIP, "sampled SA from the BWT (strand %d): %s", s, hipGetErrorString(e));
    c->index.sa_loaded[s] = true;
  }
  c->index.sa_intv = intv;
  c->index.sa_expanded = false;
  return 0;
}

int ensure_jump(ibwa_ctx *c) {
  if (c->index.jump_ready || !c->exact_jump || !c->jump_derive) return 0;
  // a context sharing another's index runs without the jump unless the source had it when shared
  // (the same results; the jump only saves rank queries)
  if (c->share_src) return 0;
  const uint64_t n = c->index.ix[0].seq_len;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
  // full SA + ISA + text of both strands (~16.6 B per base) and the derivation's temporaries
  if ((double)free_b < (double)n * 18.0 + 4e9 || (double)n * 16.6 > 0.3 * (double)total_b) return 0;
  if (!c->index.sa_loaded[0] || !c->index.sa_loaded[1])
    if (int rc = derive_sa_locked(c, 32)) return rc;
  if (int rc = ibwa_ctx_expand_sa(c)) return rc;
  for (int s = 0; s < 2; ++s) {
    const uint64_t words = n / 16 + 4;
    if (int rc = c->index.isa_full[s].ensure((n + 1) * 4)) return rc;
    if (int rc = c->index.txt2[s].ensure(words * 4)) return rc;
    HIPCHK(hipMemsetAsync(c->index.txt2[s].p, 0, words * 4, c->stream));
    HIPCHK(derive_isa_text(c->index.ix[s], c->index.sa_full[s].as<uint32_t>(), c->index.isa_full[s].as<uint32_t>(),
                           c->index.txt2[s].as<uint32_t>(), words, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  c->index.jump_ready = true;
  c->index.jump_derived = true;
  return 0;
}

}  // namespace ibwa

extern "C" {

int ibwa_ctx_load_bwt(ibwa_ctx_t *c, int strand, uint32_t primary, const uint32_t L2[4], const uint32_t *bwt,
                      uint64_t bwt_size) {
  if (strand < 0 || strand > 1) return fail(IBWA_EINVAL, "strand must be 0 (.bwt) or 1 (.rbwt)");
  if (int rc = refuse_shared(c, "load_bwt")) return rc;
  HIPCHK(enter(c));
  const uint32_t seq_len = L2[3];
  const uint64_t n_blocks = ((uint64_t)seq_len + 127) / 128 + 1;
  // expected reference size: 4 words per 128 symbols (+1 final count block) + ceil(n/16) words
  const uint64_t expect = ((uint64_t)seq_len + 127) / 128 * 4 + 4 + ((uint64_t)seq_len + 15) / 16;
  if (bwt_size != expect)
    return fail(IBWA_EINVAL, "bwt_size %llu does not match seq_len %u (expected %llu)", (unsigned long long)bwt_size,
                seq_len, (unsigned long long)expect);
  DBuf tmp;
  if (int rc = tmp.ensure(bwt_size * 4)) return rc;
  if (int rc = c->index.idx[strand].ensure(n_blocks * 64)) return rc;
  HIPCHK(hipMemcpyAsync(tmp.p, bwt, bwt_size * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(relayout_reference_bwt(tmp.as<uint32_t>(), bwt_size, n_blocks, c->index.idx[strand].as<uint4>(), c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  IndexView &ix = c->index.ix[strand];
  ix.blk = c->index.idx[strand].as<uint4>();
  ix.primary = primary;
  ix.seq_len = seq_len;
  ix.L2[0] = 0;
  for (int j = 0; j < 4; ++j) ix.L2[j + 1] = L2[j];
  c->index.loaded[strand] = true;
  c->index.build_rounds[strand] = 0;
  c->index.kmer_valid = false;
  c->index.jump_ready = false;  // SA / ISA / text belong to an index built here (or are derived again)
  c->index.jump_derived = false;
  c->index.sa_loaded[strand] = false;
  c->index.sa_expanded = false;
  return 0;
}

int ibwa_ctx_load_bwt_file(ibwa_ctx_t *c, int strand, const char *path) {  // bwtio.c:51-70
  FILE *fp = fopen(path, "rb");
  if (!fp) return fail(IBWA_EIO, "cannot open %s", path);
  fseek(fp, 0, SEEK_END);
  long sz = ftell(fp);
  fseek(fp, 0, SEEK_SET);
  if (sz < 20) { fclose(fp); return fail(IBWA_EIO, "%s: too short", path); }
  uint64_t n_words = (uint64_t)(sz - 20) >> 2;
  uint32_t primary, L2[4];
  std::vector<uint32_t> buf(n_words);
  bool ok = fread(&primary, 4, 1, fp) == 1 && fread(L2, 4, 4, fp) == 4 && fread(buf.data(), 4, n_words, fp) == n_words;
  fclose(fp);
  if (!ok) return fail(IBWA_EIO, "%s: short read", path);
  return ibwa_ctx_load_bwt(c, strand, primary, L2, buf.data(), n_words);
}

int ibwa_ctx_clone_index(ibwa_ctx_t *dst, const ibwa_ctx_t *src) {
  if (int rc = refuse_shared(dst, "clone_index")) return rc;
  for (int s = 0; s < 2; ++s) {
    if (!src->index.loaded[s]) return fail(IBWA_ENOINDEX, "source index not loaded");
    HIPCHK(enter(dst));
    uint64_t bytes = ((uint64_t)src->index.ix[s].seq_len + 127) / 128 * 64 + 64;
    if (int rc = dst->index.idx[s].ensure(bytes)) return rc;
    if (src->device == dst->device) {
      HIPCHK(hipMemcpyAsync(dst->index.idx[s].p, src->index.idx[s].p, bytes, hipMemcpyDeviceToDevice, dst->stream));
    } else {
      HIPCHK(hipMemcpyPeerAsync(dst->index.idx[s].p, dst->device, src->index.idx[s].p, src->device, bytes, dst->stream));
    }
    HIPCHK(hipStreamSynchronize(dst->stream));
    dst->index.ix[s] = src->index.ix[s];
    dst->index.ix[s].blk = dst->index.idx[s].as<uint4>();
    dst->index.loaded[s] = true;
    dst->index.build_rounds[s] = src->index.build_rounds[s];
    dst->index.kmer_valid = false;
    dst->index.sa_loaded[s] = false;
  }
  dst->index.jump_ready = false;
  dst->index.sa_expanded = false;
  return 0;
}

int ibwa_ctx_share_index(ibwa_ctx_t *dst, const ibwa_ctx_t *src) {
  if (!dst || !src || dst == src) return fail(IBWA_EINVAL, "share_index: two distinct contexts");
  if (dst->device != src->device) return fail(IBWA_EINVAL, "share_index: contexts on devices %d and %d", dst->device, src->device);
  for (int s = 0; s < 2; ++s)
    if (!src->index.loaded[s]) return fail(IBWA_ENOINDEX, "source index not loaded");
  if (int rc = refuse_shared(dst, "share_index (destination)")) return rc;
  if (src->share_src) return fail(IBWA_EINVAL, "share_index: the source shares another context's index; share that one");
  HIPCHK(enter(dst));
  HIPCHK(hipStreamSynchronize(src->stream));  // src's structures are complete
  borrow_index(dst, src);
  dst->share_src = const_cast<ibwa_ctx *>(src);
  ++dst->share_src->n_borrowers;
  return 0;
}

int ibwa_ctx_build_index(ibwa_ctx_t *c, const uint8_t *codes, uint64_t n, int sa_intv) {
  if (n == 0 || n >= 0xFFFFFFFEull) return fail(IBWA_EINVAL, "text length %llu outside [1, 2^32-2)", (unsigned long long)n);
  if (sa_intv < 0) return fail(IBWA_EINVAL, "sa_intv < 0");
  if (int rc = refuse_shared(c, "build_index")) return rc;
  HIPCHK(enter(c));
  DBuf T;
  if (int rc = T.ensure(n)) return rc;
  HIPCHK(hipMemcpyAsync(T.p, codes, n, hipMemcpyHostToDevice, c->stream));
  // keep SA / ISA / text for the exact path's jump when HBM allows (2 x 8.25 B per base)
  c->index.jump_ready = false;
  bool keep_full = c->exact_jump != 0;
  if (keep_full) {
    size_t free_b = 0, total_b = 0;
    // the kept arrays (16.5 B per base) plus the builder's sort temporaries (~45 B per base)
    // and headroom must fit in what is free now
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || (double)free_b < (double)n * 61.5 + 4e9) keep_full = false;
    if ((double)n * 16.5 > 0.3 * (double)total_b) keep_full = false;
  }
  if (!keep_full)
    for (int s = 0; s < 2; ++s) { c->index.sa_full[s].release(); c->index.isa_full[s].release(); c->index.txt2[s].release(); }
  for (int s = 0; s < 2; ++s) {
    c->index.loaded[s] = false;
    if (s == 1) HIPCHK(reverse_text(T.as<uint8_t>(), n, c->stream));  // .rpac (bwtmisc.c:160-185)
    const uint64_t n_blocks = (n + 127) / 128 + 1;
    if (int rc = c->index.idx[s].ensure(n_blocks * 64)) return rc;
    uint32_t *sa_full = nullptr, *isa_full = nullptr;
    if (keep_full) {
      if (int rc = c->index.sa_full[s].ensure((n + 1) * 4)) return rc;
      if (int rc = c->index.isa_full[s].ensure((n + 1) * 4)) return rc;
      if (int rc = c->index.txt2[s].ensure((n / 16 + 4) * 4)) return rc;
      HIPCHK(pack_text2(T.as<uint8_t>(), n, c->index.txt2[s].as<uint32_t>(), n / 16 + 4, c->stream));
      sa_full = c->index.sa_full[s].as<uint32_t>();
      isa_full = c->index.isa_full[s].as<uint32_t>();
    }
    uint32_t *sa_out = nullptr;
    if (sa_intv > 0) {
      if (int rc = c->index.sa_s[s].ensure(((n + sa_intv) / sa_intv) * 4)) return rc;
      sa_out = c->index.sa_s[s].as<uint32_t>();
    }
    uint32_t primary = 0, tot[4] = {0, 0, 0, 0};
    hipError_t e = build_strand(T.as<uint8_t>(), n, c->index.idx[s].as<uint4>(), &primary, tot, sa_out, (uint32_t)sa_intv,
                                &c->index.build_rounds[s], sa_full, isa_full, c->stream);
    if (e != hipSuccess) return fail(IBWA_EHIP, "suffix sort (strand %d): %s", s, hipGetErrorString(e));
    IndexView &ix = c->index.ix[s];
    ix.blk = c->index.idx[s].as<uint4>();
    ix.primary = primary;
    ix.seq_len = (uint32_t)n;
    ix.L2[0] = 0;
    ix.L2[1] = tot[0];
    ix.L2[2] = tot[0] + tot[1];
    ix.L2[3] = tot[0] + tot[1] + tot[2];
    ix.L2[4] = tot[0] + tot[1] + tot[2] + tot[3];
    if (ix.L2[4] != n) return fail(IBWA_EHIP, "index build: symbol total %u != n", ix.L2[4]);
    c->index.loaded[s] = true;
  }
  c->index.kmer_valid = false;
  c->index.sa_intv = (uint32_t)sa_intv;
  c->index.sa_loaded[0] = c->index.sa_loaded[1] = sa_intv > 0;
  c->index.sa_expanded = false;
  c->index.jump_ready = keep_full;
  return 0;
}

int ibwa_ctx_bwt_info(const ibwa_ctx_t *c, int strand, uint32_t *primary, uint32_t L2[4], uint64_t *bwt_size) {
  if (strand < 0 || strand > 1 || !c->index.loaded[strand]) return fail(IBWA_ENOINDEX, "index not loaded");
  const IndexView &ix = c->index.ix[strand];
  if (primary) *primary = ix.primary;
  if (L2) for (int j = 0; j < 4; ++j) L2[j] = ix.L2[j + 1];
  const uint64_t n = ix.seq_len;
  if (bwt_size) *bwt_size = (n + 127) / 128 * 4 + 4 + (n + 15) / 16;
  return 0;
}

int ibwa_ctx_export_bwt(const ibwa_ctx_t *c, int strand, uint32_t *words, uint64_t cap) {
  uint64_t need = 0;
  if (int rc = ibwa_ctx_bwt_info(c, strand, nullptr, nullptr, &need)) return rc;
  if (cap < need) return fail(IBWA_EINVAL, "export buffer too small (%llu < %llu)", (unsigned long long)cap,
                              (unsigned long long)need);
  HIPCHK(enter(c));
  const uint64_t n = c->index.ix[strand].seq_len, nb = (n + 127) / 128;
  std::vector<uint4> blk((nb + 1) * 4);
  HIPCHK(hipMemcpy(blk.data(), c->index.idx[strand].p, blk.size() * 16, hipMemcpyDeviceToHost));
  // bwt_bwtupdate_core (bwtmisc.c:122-144): [4 counts][<=8 words] per 128 symbols, then final counts
  uint64_t k = 0;
  for (uint64_t b = 0; b < nb; ++b) {
    const uint4 *p = &blk[b * 4];
    words[k++] = p[0].x; words[k++] = p[0].y; words[k++] = p[0].z; words[k++] = p[0].w;
    const uint32_t w8[8] = {p[1].x, p[1].y, p[1].z, p[1].w, p[2].x, p[2].y, p[2].z, p[2].w};
    const uint64_t nw = std::min<uint64_t>(8, (n - b * 128 + 15) / 16);
    for (uint64_t q = 0; q < nw; ++q) words[k++] = w8[q];
  }
  const IndexView &ix = c->index.ix[strand];
  for (int j = 0; j < 4; ++j) words[k++] = ix.L2[j + 1] - ix.L2[j];
  return k == need ? 0 : fail(IBWA_EINVAL, "internal: exported %llu words, expected %llu", (unsigned long long)k,
                              (unsigned long long)need);
}

int ibwa_ctx_export_sa(const ibwa_ctx_t *c, int strand, uint32_t *out, uint64_t cap) {
  if (strand < 0 || strand > 1 || !c->index.loaded[strand] || !c->index.sa_intv) return fail(IBWA_ENOINDEX, "no sampled SA");
  const uint64_t n = c->index.ix[strand].seq_len, n_sa = (n + c->index.sa_intv) / c->index.sa_intv;
  if (cap < n_sa) return fail(IBWA_EINVAL, "export buffer too small");
  HIPCHK(enter(c));
  HIPCHK(hipMemcpy(out, c->index.sa_s[strand].p, n_sa * 4, hipMemcpyDeviceToHost));
  out[0] = 0xFFFFFFFFu;  // bwt.c:66
  return 0;
}

int ibwa_ctx_build_rounds(const ibwa_ctx_t *c, int strand, int *rounds) {
  if (strand < 0 || strand > 1 || !c->index.loaded[strand] || !c->index.build_rounds[strand])
    return fail(IBWA_ENOINDEX, "no index built here");
  if (rounds) *rounds = c->index.build_rounds[strand];
  return 0;
}

int ibwa_ctx_load_sa(ibwa_ctx_t *c, int strand, uint32_t sa_intv, const uint32_t *sa, uint64_t n_sa) {
  if (strand < 0 || strand > 1 || !c->index.loaded[strand]) return fail(IBWA_ENOINDEX, "index not loaded");
  if (sa_intv == 0) return fail(IBWA_EINVAL, "sa_intv == 0");
  if (int rc = refuse_shared(c, "load_sa")) return rc;
  const uint64_t n = c->index.ix[strand].seq_len;
  if (n_sa != (n + sa_intv) / sa_intv)
    return fail(IBWA_EINVAL, "n_sa %llu != (seq_len + intv) / intv", (unsigned long long)n_sa);
  if (c->index.sa_loaded[1 - strand] && c->index.sa_intv != sa_intv)
    return fail(IBWA_EINVAL, "sa_intv %u differs from the other strand's %u", sa_intv, c->index.sa_intv);
  HIPCHK(enter(c));
  if (int rc = c->index.sa_s[strand].ensure(n_sa * 4)) return rc;
  HIPCHK(hipMemcpy(c->index.sa_s[strand].p, sa, n_sa * 4, hipMemcpyHostToDevice));
  c->index.sa_intv = sa_intv;
  c->index.sa_loaded[strand] = true;
  c->index.sa_expanded = false;
  if (c->index.jump_ready) c->index.sa_full[strand].release(), c->index.isa_full[strand].release(), c->index.jump_ready = false;
  return 0;
}

int ibwa_ctx_load_sa_file(ibwa_ctx_t *c, int strand, const char *path) {  // bwt_restore_sa, bwtio.c:29-49
  if (strand < 0 || strand > 1 || !c->index.loaded[strand]) return fail(IBWA_ENOINDEX, "index not loaded");
  FILE *fp = fopen(path, "rb");
  if (!fp) return fail(IBWA_EIO, "cannot open %s", path);
  uint32_t hdr[7];
  if (fread(hdr, 4, 7, fp) != 7) { fclose(fp); return fail(IBWA_EIO, "%s: short header", path); }
  const IndexView &ix = c->index.ix[strand];
  if (hdr[0] != ix.primary) { fclose(fp); return fail(IBWA_EINVAL, "SA-BWT inconsistency: primary is not the same."); }
  if (hdr[6] != ix.seq_len) { fclose(fp); return fail(IBWA_EINVAL, "SA-BWT inconsistency: seq_len is not the same."); }
  if (hdr[5] == 0) { fclose(fp); return fail(IBWA_EINVAL, "%s: sa_intv 0", path); }
  const uint64_t n_sa = ((uint64_t)ix.seq_len + hdr[5]) / hdr[5];
  std::vector<uint32_t> sa(n_sa);
  sa[0] = 0xFFFFFFFFu;  // bwtio.c:45
  const bool ok = fread(sa.data() + 1, 4, n_sa - 1, fp) == n_sa - 1;
  fclose(fp);
  if (!ok) return fail(IBWA_EIO, "%s: short read", path);
  return ibwa_ctx_load_sa(c, strand, hdr[5], sa.data(), n_sa);
}

int ibwa_ctx_derive_sa(ibwa_ctx_t *c, uint32_t sa_intv) {
  if (!c->index.loaded[0] || !c->index.loaded[1]) return fail(IBWA_ENOINDEX, "load both .bwt and .rbwt first");
  if (sa_intv == 0) return fail(IBWA_EINVAL, "sa_intv == 0");
  return derive_sa_locked(c, sa_intv);
}

int ibwa_ctx_expand_sa(ibwa_ctx_t *c) {
  if (!c->index.sa_loaded[0] || !c->index.sa_loaded[1]) return fail(IBWA_ENOINDEX, "sampled SA of both strands needed");
  if (c->index.jump_ready || c->index.sa_expanded) return 0;  // full SA already resident
  if (c->share_src) return fail(IBWA_EINVAL, "expand_sa: this context shares another context's index");
  HIPCHK(enter(c));
  for (int s = 0; s < 2; ++s) {
    if (int rc = c->index.sa_full[s].ensure(((uint64_t)c->index.ix[s].seq_len + 1) * 4)) return rc;
    HIPCHK(expand_sa(c->index.ix[s], c->index.sa_s[s].as<uint32_t>(), c->index.sa_intv, c->index.sa_full[s].as<uint32_t>(), c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  c->index.sa_expanded = true;
  return 0;
}

int ibwa_sa2pos(ibwa_ctx_t *c, int64_t n, const uint8_t *strand, const uint32_t *k, const uint32_t *len,
                uint64_t offset, uint64_t *pos) {
  if (n < 0) return fail(IBWA_EINVAL, "n < 0");
  if (!c->index.loaded[0] || !c->index.loaded[1]) return fail(IBWA_ENOINDEX, "index not loaded");
  const bool full = (c->index.jump_ready || c->index.sa_expanded) && !c->sa_walk;
  if (!full && (!c->index.sa_loaded[0] || !c->index.sa_loaded[1])) return fail(IBWA_ENOINDEX, "no suffix array loaded");
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t sl = c->index.ix[strand[i] ? 0 : 1].seq_len;
    if (k[i] > sl) return fail(IBWA_EINVAL, "hit %lld: row %u > seq_len %u", (long long)i, k[i], sl);
  }
  c->stats.ms_sa2pos = 0;
  if (n == 0) return 0;
  HIPCHK(enter(c));
  // one staging buffer: strand bytes, rows, lengths in; positions + walk lengths out
  const uint64_t o_k = (n + 15) / 16 * 16, o_len = o_k + n * 4, in_bytes = o_len + n * 4;
  if (int rc = c->h2p_in.ensure(in_bytes)) return rc;
  if (int rc = c->h2p_out.ensure(n * 12)) return rc;
  uint8_t *din = c->h2p_in.as<uint8_t>();
  HIPCHK(hipMemcpyAsync(din, strand, n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(din + o_k, k, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(din + o_len, len, n * 4, hipMemcpyHostToDevice, c->stream));
  SaArgs a = {};
  for (int s = 0; s < 2; ++s) {
    a.ix[s] = c->index.ix[s];
    a.sa[s] = full ? c->index.sa_full[s].as<uint32_t>() : c->index.sa_s[s].as<uint32_t>();
    a.intv[s] = full ? 1 : c->index.sa_intv;
  }
  a.strand = din;
  a.k = reinterpret_cast<const uint32_t *>(din + o_k);
  a.len = reinterpret_cast<const uint32_t *>(din + o_len);
  a.n = n;
  a.offset = offset;
  a.pos = c->h2p_out.as<uint64_t>();
  a.steps = reinterpret_cast<uint32_t *>(c->h2p_out.as<uint8_t>() + n * 8);
  HIPCHK(hipEventRecord(c->ev[0], c->stream));
  HIPCHK(launch_sa2pos(a, full, c->stream));
  HIPCHK(hipEventRecord(c->ev[1], c->stream));
  HIPCHK(hipMemcpyAsync(pos, a.pos, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->stats.ms_sa2pos = ms;
  c->stats.sa2pos_full = full;
  return 0;
}

int ibwa_occ4(ibwa_ctx_t *c, int strand, int64_t n, const uint32_t *k, uint32_t *cnt) {
  if (!c->index.loaded[strand]) return fail(IBWA_ENOINDEX, "index not loaded");
  HIPCHK(enter(c));
  DBuf dk, dc;
  if (int rc = dk.ensure(n * 4 + 4)) return rc;
  if (int rc = dc.ensure(n * 16 + 16)) return rc;
  HIPCHK(hipMemcpyAsync(dk.p, k, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(launch_occ4(c->index.ix[strand], n, dk.as<uint32_t>(), dc.as<uint32_t>(), c->stream));
  HIPCHK(hipMemcpyAsync(cnt, dc.p, n * 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
