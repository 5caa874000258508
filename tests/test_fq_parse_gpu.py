"""The FASTQ ingest on the device (fastq.hip k_fq_count / k_fq_lines / k_fq_rec / k_fq_encode and the
scans; engine_ingest.hip ibwa_fq_parse, ibwa_fq_offset, ibwa_fq_share_scratch, ibwa_batch_stage_fq,
FqScratch::h2d) record by record against tests/fq_ref.py: the records, the bytes consumed, where and
why the block ends, the per-record lengths, and -- read back with ibwa_fq_fetch -- every kept read's
length, offset and code bytes, bit for bit.  tests/test_fq_ref.py pins the expectation on the CPU."""
import ctypes as c

import numpy as np
import pytest

import oracle
from ibwa_amd import engine as E
from tests import fq_ref, synth_util

pytestmark = pytest.mark.gpu

# fastq.hip: FQ_TILE bytes per workgroup, 64 B per thread, SWAR on 4 B words, 16 B loads
TILE, SPAN, WORD, LOAD = 16384, 64, 4, 16
assert (TILE, SPAN, WORD, LOAD) == (fq_ref.TILE, fq_ref.SPAN, fq_ref.WORD, fq_ref.LOAD)
N_WAVES = 16384  # of k_fq_rec / k_fq_encode: more records than this take the grid-stride loop

FAMILIES = fq_ref.small_families()


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def compare(eng, got, exp, name, offsets=True):
    n_rec, consumed, not_strict, rec_len, rec_L = got
    assert (n_rec, consumed, not_strict) == (exp.n_rec, exp.consumed, exp.not_strict), name
    assert rec_len.dtype == np.int32 and np.array_equal(rec_len, exp.rec_len), name
    assert rec_L.dtype == np.uint32 and np.array_equal(rec_L, exp.rec_L), name
    assert eng.fq_stats()[0] == len(exp.lens), name
    codes, off, lens = eng.fq_kept()
    assert np.array_equal(lens, exp.lens), name
    assert np.array_equal(off, exp.off), name
    assert codes.size == exp.codes.size and np.array_equal(codes, exp.codes), name
    if offsets and n_rec:
        for r in sorted({0, min(1, n_rec), n_rec // 2, n_rec}):
            assert eng.fq_offset(r) == exp.starts[r], (name, r)


def check(eng, raw, name="", **kw):
    exp = fq_ref.expected(raw, **kw)
    compare(eng, eng.fq_parse(raw, **kw), exp, name)
    return exp


@pytest.mark.parametrize("family", ["geometry", "strictness", "cap", "barcode", "trim", "bytes"])
def test_family(eng, family):
    """Every block of the family (fq_ref: newlines on tile / span / word / load edges, block lengths,
    sequence lines across tile edges; every offending record at index 0, 1, behind a tile edge and
    last, truncated blocks; cap; barcodes; bwa_trim_read's branches; every sequence byte)."""
    for cs in FAMILIES[family]:
        check(eng, cs.raw, cs.name, **cs.kw)


def test_every_sequence_byte_has_its_code(eng):
    """Codes 0-3 for ACGTacgt, 5 for '-', 4 for the other 82 values, at the first, a middle and the last
    base of a read that comes back reversed."""
    (cs,) = FAMILIES["bytes"]
    exp = check(eng, cs.raw, cs.name)
    codes = eng.fq_kept()[0].reshape(-1, len(fq_ref.BYTES_BASE))
    want = {v: 4 for v in fq_ref.SEQ_BYTES}
    want.update({ord(a): k for a, k in zip("ACGTacgt", [0, 1, 2, 3] * 2)})
    want[ord("-")] = 5
    base = [want[v] for v in fq_ref.BYTES_BASE]
    for i, v in enumerate(fq_ref.SEQ_BYTES):
        for j, pos in enumerate(fq_ref.BYTES_POS):
            row = list(base)
            row[pos] = want[v]
            assert list(codes[3 * i + j]) == row[::-1], (v, pos)
    assert exp.n_rec == 273


def test_barcode_16_is_refused(eng):
    with pytest.raises(E.IbwaError):
        eng.fq_parse(b"@r\nACGT\n+\nIIII\n", barcode=16)
    check(eng, b"@r\nACGT\n+\nIIII\n", barcode=15)


def test_two_bad_records_the_earlier_wins(eng):
    """Records 5 and 30 000 of 40 000 are not strict (the atomicMin; more records than wavefronts):
    the block ends at 5 and nothing from there on counts as kept; without them all 40 000 come back."""
    bad, clean = FAMILIES["two_bad"]
    exp = check(eng, bad.raw, bad.name)
    assert (exp.n_rec, exp.not_strict, len(exp.lens)) == (5, 1, 5)
    exp = check(eng, clean.raw, clean.name)
    assert exp.n_rec == 40000 > N_WAVES


def test_line_table_overflow_and_parsing_on(eng):
    """3 000 records of 8 bytes: more lines than the line table holds.  One call returns
    (nbytes // 12 + 64) // 4 records and not_strict = 0; calls from *consumed on yield them all."""
    raw = FAMILIES["line_table"][0].raw
    seqs, pos, calls = [], 0, 0
    while pos < len(raw):
        blk = raw[pos:]
        exp = check(eng, blk, f"line_table@{pos}")
        assert exp.n_rec == min((len(blk) // 12 + 64) // 4, len(blk) // 8) and exp.not_strict == 0
        seqs.append(eng.fq_kept()[0])
        pos += exp.consumed
        calls += 1
    assert calls > 3 and pos == len(raw)
    recs = fq_ref.strict_prefix(raw)[0]
    assert len(recs) == fq_ref.LINE_TABLE_N
    assert np.array_equal(np.concatenate(seqs), oracle.encode_reads(recs, 0, 0)[0])


def _block(seed, n, lo, hi):
    rng = np.random.default_rng(seed)
    return b"".join(fq_ref.rec(i, int(rng.integers(lo, hi)), rng) for i in range(n))


def test_stale_scratch(eng):
    """A small block parsed through a scratch that holds a larger block's bytes, line table and
    per-record arrays, then the larger one again: each exact."""
    big = _block(21, 1500, 40, 80)[:200000]
    small = _block(22, 200, 30, 50)[:9000]  # ends inside a record; the first block's bytes behind it hold newlines
    assert big[:199000].count(b"\n") > 4000 and small[-1:] != b"\n"
    e = E.Engine(0)
    try:
        check(e, big, "big")
        check(e, small, "small over big")
        check(e, big, "big again")
    finally:
        e.close()


def test_two_contexts_on_a_shared_scratch(eng):
    a_raw, b_raw = _block(23, 300, 36, 60), _block(24, 500, 20, 45)
    a, b = E.Engine(0), E.Engine(0)
    try:
        E._chk(E.lib().ibwa_fq_share_scratch(b.h, a.h))
        ea = check(a, a_raw, "a")
        eb = check(b, b_raw, "b")
        # a's kept reads are still a's, byte for byte, though its line table is gone
        compare(a, (ea.n_rec, ea.consumed, ea.not_strict, ea.rec_len, ea.rec_L), ea, "a after b", offsets=False)
        with pytest.raises(E.IbwaError):
            a.fq_offset(10)
        assert b.fq_offset(7) == eb.starts[7]
        # a part of the range, and what ibwa_fq_fetch refuses
        codes, off, lens = a.fq_kept(17, 100)
        assert np.array_equal(off, ea.off[17:117]) and np.array_equal(lens, ea.lens[17:117])
        assert np.array_equal(codes, ea.codes[int(ea.off[17]):int(ea.off[116] + ea.lens[116])])
        assert a.fq_kept(300, 0)[2].size == 0
        L = E.lib()
        ln, of, cd = np.zeros(400, np.uint32), np.zeros(400, np.uint64), np.zeros(len(a_raw), np.uint8)
        args = (ln.ctypes.data, of.ctypes.data, cd.ctypes.data, cd.size)
        assert L.ibwa_fq_fetch(a.h, 0, 300, *args) == 0
        for first, n in ((0, 301), (1, 300), (-1, 2), (301, 0), (0, -1)):
            assert L.ibwa_fq_fetch(a.h, first, n, *args) != 0, (first, n)
        assert L.ibwa_fq_fetch(a.h, 0, 300, None, args[1], args[2], cd.size) != 0
        assert L.ibwa_fq_fetch(a.h, 0, 300, args[0], None, args[2], cd.size) != 0
        assert L.ibwa_fq_fetch(a.h, 0, 300, args[0], args[1], None, cd.size) != 0
        assert L.ibwa_fq_fetch(None, 0, 300, *args) != 0
        need = int(ea.codes.size)
        assert L.ibwa_fq_fetch(a.h, 0, 300, args[0], args[1], args[2], need - 1) != 0
        assert L.ibwa_fq_fetch(a.h, 0, 300, args[0], args[1], args[2], need) == 0
        assert np.array_equal(cd[:need], ea.codes)
    finally:
        b.close()
        a.close()


@pytest.mark.parametrize("nzero", [False, True])
def test_stage_fq_views(gpu_engine, nzero):
    """ibwa_batch_stage_fq: the view [first, first + n) of a parsed block's kept reads aligns as the
    same reads staged from the expectation's codes with ibwa_batch_stage."""
    genome = synth_util.golden_genome_ascii()[0]
    rng = np.random.default_rng(31)
    bc, recs = 5, []
    while len(recs) < 640:
        if len(recs) % 16 == 7:  # not kept: no longer than the barcode
            recs.append(fq_ref.rec(len(recs), int(rng.integers(1, bc + 1)), rng))
            continue
        ln, p = int(rng.integers(36, 101)), int(rng.integers(0, len(genome) - 200))
        s = bytearray(("ACGTA"[:bc] + genome[p:p + ln]).encode())
        if len(recs) % 5 == 0:
            s[bc + ln // 2] = ord("ACGT"[int(rng.integers(0, 4))])  # some reads with a mismatch
        recs.append(fq_ref.rec(len(recs), bc + ln, rng, seq=bytes(s)))
    raw = b"".join(recs)
    ing = E.Engine(0)
    try:
        exp = fq_ref.expected(raw, barcode=bc)
        compare(ing, ing.fq_parse(raw, barcode=bc), exp, "reads")
        assert len(exp.lens) == 600 and (exp.rec_len < 0).sum() == 40
        opt = E.parse_aln_args(["-n", "0"]) if nzero else E.default_opt()
        for first in (0, 1, 257):
            n = 300
            ln = exp.lens[first:first + n]
            gpu_engine.stage_fq(ing, first, n, int(ln.max()))
            gpu_engine.run(opt)
            got_n, got_a = gpu_engine.fetch()
            lo = int(exp.off[first])
            want_n, want_a = gpu_engine.aln(exp.codes[lo:int(exp.off[first + n - 1]) + int(ln[-1])], exp.off[first:first + n] - np.uint64(lo),
                                            ln, opt)
            assert np.array_equal(got_n, want_n) and got_a.tobytes() == want_a.tobytes(), first
            assert got_n.sum() > 200
    finally:
        ing.close()


def _check_large(eng, raw, seq):
    exp = fq_ref.expected_fixed(raw, seq, 11)
    n_rec, consumed, not_strict, rec_len, rec_L = eng.fq_parse(raw)
    assert (n_rec, consumed, not_strict) == (exp.n_rec, exp.consumed, 0)
    assert np.array_equal(rec_len, exp.rec_len) and np.array_equal(rec_L, exp.rec_L)
    codes, off, lens = eng.fq_kept()
    assert np.array_equal(lens, exp.lens) and np.array_equal(off, exp.off) and np.array_equal(codes, exp.codes)
    assert eng.fq_offset(n_rec) == consumed and eng.fq_offset(n_rec // 2) == consumed // n_rec * (n_rec // 2)


STAGE_MIN, STAGE_CHUNK = 8 << 20, 64 << 20  # FqScratch::h2d: pageable blocks from 8 MiB on go through two 64 MiB chunks


def test_large_pageable_8mib(eng):
    """The first size that goes through the pinned staging chunks."""
    raw, seq = fq_ref.fixed_block(STAGE_MIN + 211, 100, 41)
    _check_large(eng, raw, seq)


def test_large_pageable_128mib_and_a_tile(eng):
    """The smallest size that uses a staging chunk a second time, and so waits on its event."""
    raw, seq = fq_ref.fixed_block(2 * STAGE_CHUNK + TILE, 100, 42)
    e = E.Engine(0)
    try:
        _check_large(e, raw, seq)
    finally:
        e.close()


def test_large_pinned_8mib(eng):
    """The same 8 MiB block from ibwa_host_alloc memory: one copy, no staging."""
    raw, seq = fq_ref.fixed_block(STAGE_MIN + 211, 100, 41)
    p = c.c_void_p()
    E._chk(E.lib().ibwa_host_alloc(raw.size, c.byref(p)))
    try:
        pinned = np.ctypeslib.as_array(c.cast(p, c.POINTER(c.c_uint8)), shape=(raw.size,))
        pinned[:] = raw
        _check_large(eng, pinned, seq)
        del pinned
    finally:
        E.lib().ibwa_host_free(p)
