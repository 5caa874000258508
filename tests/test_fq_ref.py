"""tests/fq_ref.py, the expectation of the device FASTQ parse tests, pinned on the CPU: on the
blocks tests/test_fq_parse_gpu.py feeds the device (and on test_fastq_bulk's inputs) its strict
records are the records the serial kseq-semantics reader (tools/parse_check.cpp serial) reads, and
the geometry blocks put their newlines where they claim to.  Builds parse_check with g++."""
import os
import subprocess

import numpy as np
import pytest

import oracle

from tests import fq_ref, test_fastq_bulk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pc") / "parse_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "tools", "parse_check.cpp"),
                    "-lz"], check=True)
    return exe


FAMILIES = fq_ref.small_families()


def _serial(checker, path, raw):
    with open(path, "wb") as f:
        f.write(raw)
    out = subprocess.run([checker, "serial", path], capture_output=True, check=True).stdout
    lines = out.split(b"\n")
    assert lines[-1] == b"" and lines[-2].startswith(b"#end "), lines[-3:]
    return lines[:-2]


def _check_against_serial(checker, path, name, raw):
    recs, consumed, not_strict = fq_ref.strict_prefix(raw)
    mine = [s + b"\t" + q for _, s, q in recs]
    ser = _serial(checker, path, raw)
    assert ser[:len(mine)] == mine, name
    if not_strict == 0 and consumed == len(raw):
        assert len(ser) == len(mine), name
    # the walk itself: whole records, four lines each
    assert raw[:consumed].count(b"\n") == 4 * len(recs) and (consumed == 0 or raw[consumed - 1:consumed] == b"\n"), name
    return len(mine)


@pytest.mark.parametrize("name", sorted(test_fastq_bulk.CASES))
def test_strict_prefix_on_the_bulk_cases(checker, tmp_path, name):
    raw = test_fastq_bulk.CASES[name]().encode()
    _check_against_serial(checker, str(tmp_path / "x.fq"), name, raw)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_strict_prefix_on_the_device_cases(checker, tmp_path, family):
    seen, total = set(), 0
    for cs in FAMILIES[family]:
        if cs.raw in seen:
            continue
        seen.add(cs.raw)
        n = _check_against_serial(checker, str(tmp_path / "x.fq"), cs.name, cs.raw)
        if family not in ("line_table", "cap"):  # nowhere else does the line table or cap end a block
            assert fq_ref.expected(cs.raw, **cs.kw).n_rec == n, cs.name
        total += n
    assert total > 0


def _newlines(raw):
    return np.flatnonzero(np.frombuffer(raw, np.uint8) == 10)


def test_geometry_covers_the_positions():
    """The geometry blocks are what they claim: for every p and every newline kind a strict record's
    newline of that kind lies on byte p -- in the block's first record, in one with records on both
    sides, and in the last -- except where no FASTQ block can have it; the block lengths, the tile
    edges the long sequence lines cross, and every byte value are there."""
    cases = {c.name: c for c in FAMILIES["geometry"]}
    got = set()
    for c in cases.values():
        m = c.meta
        if "p" not in m:
            continue
        recs, consumed, ns = fq_ref.strict_prefix(c.raw)
        assert ns == 0 and consumed == len(c.raw), c.name  # all of it strict records
        nl = _newlines(c.raw)
        at = int(np.searchsorted(nl, m["p"]))
        assert nl[at] == m["p"] and at % 4 == m["kind"], c.name
        r, n = at // 4, len(recs)
        assert {"first": r == 0 and n > 1, "middle": 0 < r < n - 1, "last": r == n - 1}[m["place"]], c.name
        got.add((m["p"], m["kind"], m["place"]))
    for p in fq_ref.P_VALUES:
        for k in range(4):
            # a record's k-th newline lies at least _KIND_MIN[k] bytes behind the record's start, and a
            # record that is not the block's first starts at byte 8 or later (the shortest record)
            assert ((p, k, "first") in got) == (p >= fq_ref._KIND_MIN[k]), (p, k)
            assert ((p, k, "last") in got) == (p >= fq_ref._KIND_MIN[k]), (p, k)
            assert ((p, k, "middle") in got) == (p >= 8 + fq_ref._KIND_MIN[k]), (p, k)
    # every p is a tile, span, word or load edge (first or last byte of one)
    T, S, W, Q = fq_ref.TILE, fq_ref.SPAN, fq_ref.WORD, fq_ref.LOAD
    assert (T, S, W, Q) == (16384, 64, 4, 16)
    assert set(fq_ref.P_VALUES) == {W - 1, W, Q - 1, Q, S - 1, S, T - 1, T, T + 1, 2 * T - 1, 2 * T}
    for n in (T - 1, T, T + 1, 2 * T, 8):
        raw = cases[f"block_of_{n}"].raw
        assert len(raw) == n and raw[-1:] == b"\n" and fq_ref.strict_prefix(raw)[1:] == (n, 0)
    assert b"\n" not in cases["no_newline"].raw and b"\n" not in cases["no_newline_two_tiles"].raw
    assert len(cases["no_newline_two_tiles"].raw) > T and cases["empty"].raw == b""
    for L in (1, 63, 64, 65, 129, 20000):
        c = cases[f"seq_of_{L}_over_tile_edge"]
        s0 = c.meta["seq_start"]
        assert c.raw[s0 - 1:s0] == b"\n" and c.raw[s0 + L:s0 + L + 1] == b"\n" and b"\n" not in c.raw[s0:s0 + L]
        assert s0 < T <= s0 + L  # the line's newline is in the next tile
        assert fq_ref.strict_prefix(c.raw)[1:] == (len(c.raw), 0)
    assert s0 + L > 2 * T  # the longest lies across two edges
    (bv,) = FAMILIES["bytes"]
    recs = fq_ref.strict_prefix(bv.raw)[0]
    assert len(recs) == 3 * 91 == bv.meta["n"] and len(fq_ref.SEQ_BYTES) == 91
    for pos in fq_ref.BYTES_POS:
        assert {s[pos] for _, s, _ in recs} >= set(fq_ref.SEQ_BYTES)


def test_strictness_blocks_stop_where_they_claim():
    """Every offending record ends the strict prefix at its own index (in the first tile, just
    behind the tile edge, last), the strict look-alikes end nothing, and a truncated block ends at its
    last complete record with not_strict = 0."""
    for c in FAMILIES["strictness"]:
        recs, consumed, ns = fq_ref.strict_prefix(c.raw)
        m = c.meta
        if "consumed" in m:
            assert (consumed, ns) == (m["consumed"], 0), c.name
        elif "blank" in m:
            assert len(recs) == m["blank"] and ns == (1 if m["bad"] is not None else 0), c.name
        elif m["bad"] is None:
            assert ns == 0 and consumed == len(c.raw), c.name
        else:
            assert (len(recs), ns) == (m["bad"], 1), c.name
    idx = {c.meta["bad"] for c in FAMILIES["strictness"] if c.meta.get("bad") is not None}
    first_behind = min(i for i in idx if i > 1)
    raw = [c for c in FAMILIES["strictness"] if c.name == "qual_32_at_behind_tile_edge"][0].raw
    start = fq_ref.expected(raw).starts[first_behind]
    assert fq_ref.TILE <= start < fq_ref.TILE + 64 and {0, 1} <= idx


def test_two_bad_block_and_line_table_block():
    raw = FAMILIES["two_bad"][0].raw
    recs, consumed, ns = fq_ref.strict_prefix(raw)
    assert (len(recs), ns) == (5, 1)
    e = fq_ref.expected(FAMILIES["two_bad"][1].raw)
    assert e.n_rec == 40000 > 16384 and e.not_strict == 0 and len(e.lens) == 40000
    # with record 5 alone repaired, the block stops at record 30 000
    fixed = raw.split(b"\n")
    fixed[4 * 5 + 1] = fixed[4 * 5 + 1].replace(b" ", b"A")
    assert len(fq_ref.strict_prefix(b"\n".join(fixed))[0]) == 30000
    lt = FAMILIES["line_table"][0].raw
    e = fq_ref.expected(lt)
    assert len(lt) == 8 * fq_ref.LINE_TABLE_N and e.n_rec == (len(lt) // 12 + 64) // 4 == 516 and e.not_strict == 0
    assert len(fq_ref.strict_prefix(lt)[0]) == fq_ref.LINE_TABLE_N


def test_expected_models_cap():
    for c in FAMILIES["cap"]:
        e = fq_ref.expected(c.raw, **c.kw)
        n_strict = len(fq_ref.strict_prefix(c.raw)[0])
        if "cap" in c.kw:
            assert e.n_rec == min(c.kw["cap"], n_strict), c.name
            if c.kw["cap"] <= n_strict:
                assert e.not_strict == 0, c.name
        else:
            assert e.n_rec == n_strict and e.not_strict == 1, c.name
        assert e.consumed == e.starts[e.n_rec] and len(e.rec_len) == e.n_rec


def test_trim_tails_drive_each_branch():
    """The quality tails make bwa_trim_read stop at BWA_MIN_RDLEN, stop where the qualities rise, break
    on a negative sum, and meet its maximum twice: the kept lengths differ as those branches say."""
    for t in (1, 15, 20, 40):
        for L in (64, 100, 150):
            kept = {}
            for nm, ql in fq_ref.trim_tails(L, t).items():
                r = [(b"x", b"A" * L, bytes(33 + v for v in ql))]
                kept[nm] = int(oracle.encode_reads(r, 0, t)[2][0])
            assert kept["low_throughout"] == fq_ref.MIN_RDLEN
            assert kept["low_then_high"] == L - 9
            assert kept["negative_then_low"] == L - 2
            assert kept["maximum_twice"] == L  # the later maximum stays (>, not >=)
            assert kept["maximum_twice_then_low"] == fq_ref.MIN_RDLEN


def test_fixed_layout_expectation_equals_the_walk():
    for nbytes, L in ((5000, 36), (16384 + 17, 100), (40000, 20)):
        raw, seq = fq_ref.fixed_block(nbytes, L, 5)
        assert raw.size == nbytes
        a, b = fq_ref.expected_fixed(raw, seq, 11), fq_ref.expected(raw.tobytes(), cap=1 << 30)
        assert fq_ref.line_table_records(nbytes) > a.n_rec > 0
        assert (a.n_rec, a.consumed, a.not_strict) == (b.n_rec, b.consumed, b.not_strict)
        for x, y in zip(a[3:8], b[3:8]):
            assert x.dtype == y.dtype and np.array_equal(x, y)
