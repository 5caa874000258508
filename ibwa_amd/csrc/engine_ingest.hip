// engine_ingest.hip -- reads into a context: pinned host memory, FASTQ parsing on the device, staging a batch.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <thread>

#include "engine_ctx.h"

using namespace ibwa;

// src[0, n) to device dst on stream st
hipError_t FqScratch::h2d(void *dst, const void *src, size_t n, hipStream_t st) {
  hipPointerAttribute_t at;
  const bool pinned = hipPointerGetAttributes(&at, src) == hipSuccess;
  (void)hipGetLastError();  // an unregistered pointer is not an error here
  if (pinned || n < (8u << 20)) return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st);
  for (int i = 0; i < 2; ++i) {
    if (!stage[i]) {
      void *p = nullptr;
      if (hipError_t e = hipHostMalloc(&p, kStage, hipHostMallocDefault)) return e;
      stage[i] = static_cast<char *>(p);
    }
    if (!sev[i])
      if (hipError_t e = hipEventCreateWithFlags(&sev[i], hipEventDisableTiming)) return e;
  }
  const char *s = static_cast<const char *>(src);
  for (size_t o = 0, k = 0; o < n; o += kStage, ++k) {
    const int b = (int)(k & 1);
    const size_t len = std::min(kStage, n - o);
    if (k >= 2)
      if (hipError_t e = hipEventSynchronize(sev[b])) return e;  // its previous chunk has left
    const int T = 8;
    std::thread th[T];
    for (int t = 0; t < T; ++t)
      th[t] = std::thread([&, t]() {
        const size_t a = len * t / T, z = len * (t + 1) / T;
        memcpy(stage[b] + a, s + o + a, z - a);
      });
    for (auto &x : th) x.join();
    if (hipError_t e = hipMemcpyAsync(static_cast<char *>(dst) + o, stage[b], len, hipMemcpyHostToDevice, st)) return e;
    if (hipError_t e = hipEventRecord(sev[b], st)) return e;
  }
  return hipSuccess;
}

extern "C" {

int ibwa_host_alloc(uint64_t bytes, void **p) {
  if (!p) return fail(IBWA_EINVAL, "null pointer");
  hipError_t e = hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault);
  if (e != hipSuccess) return fail(IBWA_EHIP, "hipHostMalloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(e));
  return 0;
}

int ibwa_host_free(void *p) {
  if (p) HIPCHK(hipHostFree(p));
  return 0;
}

int ibwa_fq_parse(ibwa_ctx_t *c, const void *raw, uint64_t nbytes, int mode, int trim_qual, int64_t *n_rec,
                  uint64_t *consumed, int *not_strict, int32_t *rec_len, uint32_t *rec_L, int64_t cap) {
  if (!c || !raw || !n_rec || !consumed || !not_strict || cap < 0) return fail(IBWA_EINVAL, "fq_parse: bad arguments");
  if (nbytes >= 0xFFFF0000ull) return fail(IBWA_EINVAL, "fq_parse: a block of %llu bytes (< 4 GiB)", (unsigned long long)nbytes);
  if (((unsigned)mode >> 24) > 15) return fail(IBWA_EINVAL, "the maximum barcode length is 15");
  *n_rec = 0;
  *consumed = 0;
  *not_strict = 0;
  c->fq_kept = 0;
  c->fq_ms = 0;
  if (nbytes == 0) return 0;
  HIPCHK(enter(c));
  const uint64_t padded = fq_padded_bytes(nbytes);
  // a strict line holds >= 2 bytes, and records of real reads far more: past cap_lines the block
  // simply ends earlier (the caller parses on from *consumed)
  const uint64_t cap_lines = std::min<uint64_t>(nbytes / 12 + 64, 0xFFFFFF00ull);
  const uint64_t max_rec = cap_lines / 4 + 1, n_tiles = padded / 16384;
  if (!c->fqs) c->fqs = new FqScratch();
  FqScratch &S = *c->fqs;
  S.last = nullptr;
  if (int rc = S.raw.ensure(padded)) return rc;
  if (int rc = S.tile.ensure(n_tiles * 8 + 8)) return rc;
  if (int rc = S.nl.ensure(cap_lines * 4)) return rc;
  if (int rc = S.cnt.ensure(16)) return rc;
  if (int rc = S.len.ensure(max_rec * 4)) return rc;
  if (int rc = S.L.ensure(max_rec * 4)) return rc;
  if (int rc = S.key.ensure(max_rec * 8)) return rc;
  // the kept reads' codes: at most half the block (a strict record of L bases takes 2 L + 4 bytes)
  if (int rc = c->fq_codes.ensure(nbytes / 2 + 16)) return rc;
  if (int rc = c->fq_offk.ensure(max_rec * 8)) return rc;
  if (int rc = c->fq_lenk.ensure(max_rec * 4)) return rc;
  FqBufs B;
  B.raw = S.raw.as<uint8_t>();
  B.tile_cnt = S.tile.as<uint32_t>();
  B.tile_base = B.tile_cnt + n_tiles;
  B.nl = S.nl.as<uint32_t>();
  B.cap_lines = (uint32_t)cap_lines;
  B.n_lines = S.cnt.as<uint32_t>();
  B.bad = B.n_lines + 1;
  B.rec_len = S.len.as<int32_t>();
  B.rec_L = S.L.as<uint32_t>();
  B.rec_key = S.key.as<uint64_t>();
  B.codes = c->fq_codes.as<uint8_t>();
  B.offk = c->fq_offk.as<uint64_t>();
  B.lenk = c->fq_lenk.as<uint32_t>();
  const FqOpt o{(int)((unsigned)mode >> 24), trim_qual, (mode & IBWA_MODE_IL13) ? 1 : 0};
  size_t tb = 0;
  HIPCHK(fq_parse_launch(B, nbytes, o, nullptr, &tb, c->stream));
  if (int rc = S.tmp.ensure(tb + 256)) return rc;
  HIPCHK(hipEventRecord(c->ev[6], c->stream));
  // the padding and the counters' initial values come from pinned host memory (copy engine), not
  // from memsets (kernels)
  if (!S.hinit) {
    void *h = nullptr;
    HIPCHK(hipHostMalloc(&h, 8 + 2 * FQ_PAD_MAX, 0));
    memset(h, 0, 8 + 2 * FQ_PAD_MAX);
    static_cast<uint32_t *>(h)[1] = 0xFFFFFFFFu;
    S.hinit = static_cast<uint32_t *>(h);
  }
  HIPCHK(S.h2d(S.raw.p, raw, nbytes, c->stream));
  if (padded - nbytes <= 2 * FQ_PAD_MAX)
    HIPCHK(hipMemcpyAsync(S.raw.as<uint8_t>() + nbytes, S.hinit + 2, padded - nbytes, hipMemcpyHostToDevice, c->stream));
  else
    HIPCHK(hipMemsetAsync(S.raw.as<uint8_t>() + nbytes, 0, padded - nbytes, c->stream));
  HIPCHK(fq_parse_launch(B, nbytes, o, S.tmp.p, &tb, c->stream, S.hinit));
  HIPCHK(hipEventRecord(c->ev[7], c->stream));
  uint32_t cnt[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(cnt, S.cnt.p, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
  c->fq_ms = ms;
  const uint64_t complete = cnt[0] / 4;
  uint64_t n = std::min<uint64_t>(complete, cnt[1]);
  *not_strict = cnt[1] < complete && n == cnt[1];
  // the caller takes at most cap records: the block ends at the last of them, and a record past
  // them is not reported on (cap records that end right before a bad one included)
  if (n >= (uint64_t)cap) {
    n = (uint64_t)cap;
    *not_strict = 0;
  }
  if (n == 0) return 0;
  uint32_t last_nl = 0;
  HIPCHK(hipMemcpy(&last_nl, S.nl.as<uint32_t>() + 4 * n - 1, 4, hipMemcpyDeviceToHost));
  if (rec_len) HIPCHK(hipMemcpy(rec_len, S.len.p, n * 4, hipMemcpyDeviceToHost));
  if (rec_L) HIPCHK(hipMemcpy(rec_L, S.L.p, n * 4, hipMemcpyDeviceToHost));
  uint64_t key = 0;
  int32_t ll = 0;
  HIPCHK(hipMemcpy(&key, S.key.as<uint64_t>() + n - 1, 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&ll, S.len.as<int32_t>() + n - 1, 4, hipMemcpyDeviceToHost));
  c->fq_kept = (int64_t)(key >> 32) + (ll >= 0 ? 1 : 0);
  S.last = c;
  *n_rec = (int64_t)n;
  *consumed = (uint64_t)last_nl + 1;
  return 0;
}

int ibwa_fq_share_scratch(ibwa_ctx_t *dst, const ibwa_ctx_t *src) {
  if (!dst || !src || dst == src) return fail(IBWA_EINVAL, "fq_share_scratch: bad arguments");
  if (dst->device != src->device)
    return fail(IBWA_EINVAL, "fq_share_scratch: contexts on devices %d and %d", dst->device, src->device);
  ibwa_ctx *s = const_cast<ibwa_ctx *>(src);
  HIPCHK(enter(s));
  if (!s->fqs) s->fqs = new FqScratch();
  if (dst->fqs == s->fqs) return 0;
  if (dst->fqs) {
    HIPCHK(enter(dst));
    dst->fqs->unref();
  }
  dst->fqs = s->fqs;
  ++dst->fqs->refs;
  return 0;
}

int ibwa_fq_offset(const ibwa_ctx_t *c, int64_t r, uint64_t *off) {
  if (!c || !off || r < 0) return fail(IBWA_EINVAL, "fq_offset: bad arguments");
  *off = 0;
  if (r == 0) return 0;
  HIPCHK(enter(c));
  if (!c->fqs || !c->fqs->nl.p || c->fqs->last != c)
    return fail(IBWA_EINVAL, "fq_offset: this context's block is not the last one parsed in its scratch");
  uint32_t x = 0;
  HIPCHK(hipMemcpy(&x, c->fqs->nl.as<uint32_t>() + 4 * r - 1, 4, hipMemcpyDeviceToHost));
  *off = (uint64_t)x + 1;
  return 0;
}

int ibwa_fq_stats(const ibwa_ctx_t *c, int64_t *kept, double *ms) {
  if (kept) *kept = c->fq_kept;
  if (ms) *ms = c->fq_ms;
  return 0;
}

int ibwa_fq_fetch(const ibwa_ctx_t *c, int64_t first, int64_t n, uint32_t *len, uint64_t *off, uint8_t *codes,
                  uint64_t codes_cap) {
  if (!c || !len || !off || !codes) return fail(IBWA_EINVAL, "fq_fetch: null pointer");
  if (first < 0 || n < 0 || first > c->fq_kept || n > c->fq_kept - first)
    return fail(IBWA_EINVAL, "fq_fetch: reads [%lld, %lld) outside the %lld kept reads of the parsed block",
                (long long)first, (long long)(first + n), (long long)c->fq_kept);
  if (n == 0) return 0;
  HIPCHK(enter(c));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(len, c->fq_lenk.as<uint32_t>() + first, n * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(off, c->fq_offk.as<uint64_t>() + first, n * 8, hipMemcpyDeviceToHost));
  // the kept reads lie in the code array in order, one behind the other
  const uint64_t lo = off[0], hi = off[n - 1] + len[n - 1];
  if (hi < lo || hi > c->fq_codes.cap)
    return fail(IBWA_EINVAL, "fq_fetch: offsets [%llu, %llu) outside the block's %llu code bytes", (unsigned long long)lo,
                (unsigned long long)hi, (unsigned long long)c->fq_codes.cap);
  if (hi - lo > codes_cap)
    return fail(IBWA_EINVAL, "fq_fetch: %llu code bytes, room for %llu", (unsigned long long)(hi - lo),
                (unsigned long long)codes_cap);
  if (hi > lo) HIPCHK(hipMemcpy(codes, c->fq_codes.as<uint8_t>() + lo, hi - lo, hipMemcpyDeviceToHost));
  return 0;
}

int ibwa_batch_stage_fq(ibwa_ctx_t *c, const ibwa_ctx_t *src, int64_t first, int64_t n, int max_len) {
  if (!c || !src || first < 0 || n < 0 || first + n > src->fq_kept)
    return fail(IBWA_EINVAL, "stage_fq: reads [%lld, %lld) outside the %lld kept reads of the parsed block",
                (long long)first, (long long)(first + n), (long long)(src ? src->fq_kept : 0));
  if (c->device != src->device) return fail(IBWA_EINVAL, "stage_fq: contexts on devices %d and %d", c->device, src->device);
  if (max_len > 65535) return fail(IBWA_EINVAL, "read length %d > 65535 is not supported", max_len);
  HIPCHK(enter(c));
  HIPCHK(hipStreamSynchronize(src->stream));  // the block is parsed
  // no copy: the batch is a view of the parsed block's kept reads (their codes, offsets into them
  // and lengths), which must stay as they are until this context's runs over it are over -- a
  // copy would be a kernel waiting for CUs that the other contexts' persistent searches hold
  c->batch.v_seq = src->fq_codes.as<uint8_t>();
  c->batch.v_off = src->fq_offk.as<uint64_t>() + first;
  c->batch.v_len = src->fq_lenk.as<uint32_t>() + first;
  c->batch.n = n;
  c->batch.seq_bytes = 0;
  c->batch.max_len = max_len;
  return 0;
}

int ibwa_batch_stage(ibwa_ctx_t *c, int64_t n, const uint8_t *seq, const uint64_t *off, const uint32_t *len) {
  if (n < 0) return fail(IBWA_EINVAL, "n < 0");
  HIPCHK(enter(c));
  uint64_t bytes = 0;
  int max_len = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (len[i] > 65535) return fail(IBWA_EINVAL, "read length %u > 65535 is not supported (read %lld)", len[i], (long long)i);
    bytes = std::max<uint64_t>(bytes, off[i] + len[i]);
    max_len = std::max<int>(max_len, (int)len[i]);
  }
  if (int rc = c->batch.d_seq.ensure(bytes + 16)) return rc;
  if (int rc = c->batch.d_off.ensure(n * 8 + 8)) return rc;
  if (int rc = c->batch.d_len.ensure(n * 4 + 4)) return rc;
  if (bytes) HIPCHK(hipMemcpyAsync(c->batch.d_seq.p, seq, bytes, hipMemcpyHostToDevice, c->stream));
  if (n) {
    HIPCHK(hipMemcpyAsync(c->batch.d_off.p, off, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->batch.d_len.p, len, n * 4, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  c->batch.n = n;
  c->batch.seq_bytes = bytes;
  c->batch.max_len = max_len;
  c->batch.v_seq = c->batch.d_seq.as<uint8_t>();
  c->batch.v_off = c->batch.d_off.as<uint64_t>();
  c->batch.v_len = c->batch.d_len.as<uint32_t>();
  return 0;
}

}  // extern "C"
