"""What ibwa_fq_parse must return for a raw block, stated in plain Python, and the blocks the parse
tests feed it.  Shares no code with the product: the record rule is the one include/ibwa_aln.h
states for ibwa_fq_parse, walked byte-wise here; the kept reads' codes, offsets and lengths come
from oracle.encode_reads (the restatement of bwa_read_seq).  tests/test_fq_ref.py pins this file
against the serial kseq-semantics reader on the very blocks tests/test_fq_parse_gpu.py uses."""
import collections

import numpy as np

import oracle

# the parse kernels' geometry (fastq.hip): bytes per workgroup, per thread, per SWAR word, per load
TILE, SPAN, WORD, LOAD = 16384, 64, 4, 16
MIN_RDLEN = 35  # BWA_MIN_RDLEN: bwa_trim_read keeps at least this

_SEQ_OK = bytes(b for b in range(33, 127) if b not in b">+@")
_QUAL_OK = bytes(range(33, 128))
SEQ_BYTES = _SEQ_OK  # the 91 values a strict sequence line may hold

Expected = collections.namedtuple("Expected", "n_rec consumed not_strict rec_len rec_L codes off lens starts")


def _walk(raw):
    """(records, ends, not_strict): the strict records from the block's start, the byte offset
    behind each, and 1 when four complete lines followed them that are no strict record."""
    recs, ends, pos = [], [], 0
    while True:
        nl, p = [], pos
        for _ in range(4):
            q = raw.find(b"\n", p)
            if q < 0:
                break
            nl.append(q)
            p = q + 1
        if len(nl) < 4:
            return recs, ends, 0
        head, seq, plus, qual = raw[pos:nl[0]], raw[nl[0] + 1:nl[1]], raw[nl[1] + 1:nl[2]], raw[nl[2] + 1:nl[3]]
        ok = (head[:1] == b"@" and 1 <= len(seq) <= 1 << 24 and plus[:1] == b"+" and len(qual) == len(seq)
              and not seq.translate(None, _SEQ_OK) and not qual.translate(None, _QUAL_OK))
        if not ok:
            return recs, ends, 1
        recs.append((head[1:], seq, qual))
        pos = nl[3] + 1
        ends.append(pos)


def strict_prefix(raw):
    """(records [(name, seq, qual)], consumed, not_strict) of a block, by the rule of ibwa_fq_parse."""
    recs, ends, ns = _walk(bytes(raw))
    return recs, (ends[-1] if ends else 0), ns


def line_table_records(nbytes):
    """Records one call returns at most: the line table holds nbytes // 12 + 64 lines."""
    return (nbytes // 12 + 64) // 4


def expected(raw, barcode=0, trim_qual=0, il13=False, cap=None):
    """The whole tuple ibwa_fq_parse + ibwa_fq_fetch must give for raw (Expected); starts[r] is the
    byte offset of record r (r <= n_rec)."""
    raw = bytes(raw)
    if cap is None:
        cap = len(raw) // 48 + 17
    recs, ends, ns = _walk(raw)
    n = len(recs)
    lim = line_table_records(len(raw))
    if n >= lim:  # the line table ended the block: the record behind it was never looked at
        n, ns = lim, 0
    if n >= cap:  # the caller's room ended it
        n, ns = cap, 0
    recs, ends = recs[:n], ends[:n]
    mode = (barcode << 24) | (oracle.MODE_IL13 if il13 else 0)
    codes, off, lens = oracle.encode_reads(recs, mode, trim_qual)
    rec_len, k = np.full(n, -1, np.int32), 0
    for r, (_, seq, _) in enumerate(recs):
        if len(seq) > barcode:
            rec_len[r] = lens[k]
            k += 1
    assert k == len(lens)
    rec_L = np.array([len(s) for _, s, _ in recs], np.uint32)
    return Expected(n, ends[-1] if ends else 0, ns, rec_len, rec_L, codes, off.astype(np.uint64), lens.astype(np.uint32),
                    [0] + ends)


# ---- fixed-layout records: the large blocks, numpy only ----

def fixed_block(nbytes, L, seed, hdr=b"@fixed:0001"):
    """A block of nbytes: records hdr \\n seq[L] \\n + \\n qual[L] \\n, as many as fit whole, then the start
    of one more.  -> (raw uint8[nbytes], seq uint8[n, L])"""
    rs = len(hdr) + 2 * L + 5
    n = nbytes // rs
    rng = np.random.default_rng(seed)
    rec = np.empty((n + 1, rs), np.uint8)
    h = len(hdr)
    rec[:, :h] = np.frombuffer(hdr, np.uint8)
    rec[:, h] = 10
    rec[:, h + 1:h + 1 + L] = np.frombuffer(b"ACGTNacgtn-RYK.", np.uint8)[rng.integers(0, 15, (n + 1, L), dtype=np.uint8)]
    rec[:, h + 1 + L] = 10
    rec[:, h + 2 + L] = ord("+")
    rec[:, h + 3 + L] = 10
    rec[:, h + 4 + L:h + 4 + 2 * L] = rng.integers(33, 127, (n + 1, L), dtype=np.uint8)
    rec[:, h + 4 + 2 * L] = 10
    raw = rec.reshape(-1)[:nbytes]
    return raw, rec[:n, h + 1:h + 1 + L]


def expected_fixed(raw, seq, hdr_len):
    """Expected for fixed_block's block with no barcode and no trimming (starts is left empty)."""
    n, L = seq.shape
    rs = hdr_len + 2 * L + 5
    codes = oracle._NT4[seq[:, ::-1]].reshape(-1)
    return Expected(n, n * rs, 0, np.full(n, L, np.int32), np.full(n, L, np.uint32), codes,
                    np.arange(n, dtype=np.uint64) * np.uint64(L), np.full(n, L, np.uint32), [])


# ---- the blocks ----

Case = collections.namedtuple("Case", "name raw kw meta")


def case(name, raw, meta=None, **kw):
    return Case(name, bytes(raw), kw, meta or {})


def rec(i, L, rng, name=None, seq=None, qual=None, plus=b"+"):
    name = (b"r%d" % i) if name is None else name
    if seq is None:
        seq = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), L))
    if qual is None:
        qual = bytes(rng.integers(33, 127, len(seq), dtype=np.uint8))
    return b"@" + name + b"\n" + seq + b"\n" + plus + b"\n" + qual + b"\n"


def sized_record(size, rng):
    """One strict record of exactly size >= 8 bytes."""
    assert size >= 8
    L = min((size - 6) // 2, 30)
    r = rec(0, L, rng, name=b"x" * (size - 6 - 2 * L))  # '@' name \n seq \n '+' \n qual \n
    assert len(r) == size
    return r


def filler(size, rng):
    """Strict records that fill exactly size bytes (0, or >= 8)."""
    assert size == 0 or size >= 8, size
    out, left, i = [], size, 0
    while left >= 200:
        r = rec(i, 20 + i % 17, rng)
        out.append(r)
        left -= len(r)
        i += 1
    if left:
        if left >= 16:
            a = left // 2
            out += [sized_record(a, rng), sized_record(left - a, rng)]
        else:
            out.append(sized_record(left, rng))
    b = b"".join(out)
    assert len(b) == size
    return b


P_VALUES = (3, 4, 15, 16, 63, 64, 16383, 16384, 16385, 32767, 32768)
KINDS = ("header", "sequence", "plus", "quality")
PLACES = ("first", "middle", "last")
_KIND_MIN = (1, 3, 5, 7)  # the earliest byte a record's k-th newline can lie on: "@\nA\n+\nI\n"


def newline_at(p, kind, place, rng):
    """A block in which newline `kind` (0..3) of one record lies on byte p; the record is the block's
    first, one with records before and after, or the last.  None where no such block exists: the
    record's k-th newline lies at least _KIND_MIN[k] bytes behind its start, and a record that is
    not the first starts at byte 8 or later."""
    Lt = 1 if p < 64 else 7
    d = (1, 2 + Lt, 4 + Lt, 5 + 2 * Lt)[kind]  # offset of the newline in a record with an empty name
    if p < d:
        return None
    if place == "first" or (place == "last" and p - d < 8):
        start = 0
    elif p - d < 8:
        return None
    else:
        start = max(8, p - d - 2)
    h = p - d - start  # the name's length
    tgt = rec(0, Lt, rng, name=b"t" * h)
    after = b"" if place == "last" else filler(300, rng)
    return filler(start, rng) + tgt + after, start


def geometry_cases():
    out = []
    rng = np.random.default_rng(11)
    for p in P_VALUES:
        for k in range(4):
            for place in PLACES:
                g = newline_at(p, k, place, rng)
                if g is not None:
                    out.append(case(f"nl_{KINDS[k]}_at_{p}_{place}", g[0], meta=dict(p=p, kind=k, place=place, start=g[1])))
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE):  # the last newline on byte n - 1
        out.append(case(f"block_of_{n}", filler(n, rng), meta=dict(nbytes=n)))
    out.append(case("block_of_8", b"@\nA\n+\nI\n", meta=dict(nbytes=8)))
    out.append(case("no_newline", b"@abc" * 25, meta=dict(nbytes=100)))
    out.append(case("no_newline_two_tiles", b"@abc" * (TILE // 4 + 1), meta=dict(nbytes=TILE + 4)))
    out.append(case("empty", b"", meta=dict(nbytes=0)))
    for L in (1, 63, 64, 65, 129, 20000):  # a sequence line across a tile edge (20 000: across two)
        s0 = TILE - min((L + 1) // 2, 1000)  # where the sequence line starts
        front = filler(s0 - 10, rng)
        out.append(case(f"seq_of_{L}_over_tile_edge", front + rec(0, L, rng, name=b"spanning") + filler(120, rng),
                        meta=dict(seq_start=s0, L=L)))
    return out


def _std_block(rng, n=330, L=24):
    """n records of 2 L + 12 bytes each (n = 330, L = 24: 19.8 KB, two tiles)."""
    return [rec(i, L, rng, name=b"s%05d" % i) for i in range(n)]


def offenders(rng):
    """name -> (record bytes, strict?)"""
    L = 24
    s = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L))
    q = bytes(rng.integers(33, 127, L, dtype=np.uint8))
    o = collections.OrderedDict()
    o["fasta_header"] = (b">bad001\n" + s + b"\n+\n" + q + b"\n", False)
    for nm, b in (("gt", b">"), ("plus", b"+"), ("at", b"@"), ("space", b" "), ("tab", b"\t"), ("nul", b"\0"),
                  ("del", b"\x7f"), ("x80", b"\x80"), ("xff", b"\xff")):
        o["seq_has_" + nm] = (b"@bad001\n" + s[:9] + b + s[10:] + b"\n+\n" + q + b"\n", False)
    o["crlf"] = (b"@bad001\r\n" + s + b"\r\n+\r\n" + q + b"\r\n", False)
    o["empty_seq"] = (b"@bad001\n\n+\n\n", False)
    o["third_line_no_plus"] = (b"@bad001\n" + s + b"\n-\n" + q + b"\n", False)
    o["plus_with_name"] = (b"@bad001\n" + s + b"\n+bad001\n" + q + b"\n", True)
    o["qual_one_short"] = (b"@bad001\n" + s + b"\n+\n" + q[:-1] + b"\n", False)
    o["qual_one_long"] = (b"@bad001\n" + s + b"\n+\n" + q + b"I\n", False)
    o["qual_32"] = (b"@bad001\n" + s + b"\n+\n" + q[:5] + b" " + q[6:] + b"\n", False)
    o["qual_x80"] = (b"@bad001\n" + s + b"\n+\n" + q[:5] + b"\x80" + q[6:] + b"\n", False)
    o["qual_starts_with_at"] = (b"@bad001\n" + s + b"\n+\n@" + q[1:] + b"\n", True)
    return o


def strictness_cases():
    out = []
    rng = np.random.default_rng(12)
    recs = _std_block(rng)
    rs = len(recs[0])
    behind_edge = -(-TILE // rs)  # the first record that starts at or behind the tile edge
    places = (("0", 0), ("1", 1), ("behind_tile_edge", behind_edge), ("last", len(recs) - 1))
    for nm, (bad, strict) in offenders(rng).items():
        for pn, idx in places:
            rr = list(recs)
            rr[idx] = bad
            out.append(case(f"{nm}_at_{pn}", b"".join(rr), meta=dict(bad=None if strict else idx)))
    # a blank line in front of record idx, then `after` complete lines (None: the rest of the block)
    for pn, idx in places:
        for after in (2, 3, 4, None):
            rest = b"".join(recs[idx:])
            if after is not None:  # `after` lines and the start of one more
                rest = b"".join(x + b"\n" for x in rest.split(b"\n")[:after]) + b"@cut"
            out.append(case(f"blank_line_at_{pn}_then_{after}", b"".join(recs[:idx]) + b"\n" + rest,
                            meta=dict(bad=idx if after is None or after >= 3 else None, blank=idx, after=after)))
    # where the block ends
    body, last = b"".join(recs[:-1]), recs[-1]
    nl = [i for i, b in enumerate(last) if b == 10]
    for nm, cut in (("header", 3), ("sequence", nl[0] + 5), ("plus_line", nl[1] + 2), ("quality", nl[2] + 7),
                    ("quality_without_newline", nl[3])):
        out.append(case(f"ends_inside_{nm}", body + last[:cut], meta=dict(consumed=len(body))))
        out.append(case(f"short_ends_inside_{nm}", recs[0] + last[:cut], meta=dict(consumed=len(recs[0]))))
    return out


def two_bad_block(bad=(5, 30000), n=40000, L=20):
    """n records of L bp, more than the 16 384 wavefronts of the per-record kernels; the records in
    `bad` hold a space in the sequence."""
    rng = np.random.default_rng(13)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, L))]
    qual = rng.integers(33, 127, (n, L), dtype=np.uint8)
    for b in bad:
        seq[b, L // 2] = 32
    return b"".join(b"@p%05d\n%s\n+\n%s\n" % (i, seq[i].tobytes(), qual[i].tobytes()) for i in range(n))


def cap_cases():
    out = []
    rng = np.random.default_rng(14)
    n = 50
    recs = [rec(i, 30 + i % 9, rng) for i in range(n + 3)]
    clean = b"".join(recs[:n])
    for cap in (0, 1, n - 1, n, n + 1):
        out.append(case(f"clean_cap_{cap}", clean, cap=cap))
        rr = list(recs)
        rr[cap] = rr[cap].replace(b"\n+\n", b"\n-\n")
        out.append(case(f"record_cap_{cap}_not_strict", b"".join(rr), cap=cap))
        out.append(case(f"record_cap_{cap}_not_strict_uncapped", b"".join(rr)))
    return out


LINE_TABLE_N = 3000


def line_table_block():
    return b"".join(b"@\n%c\n+\nI\n" % b"ACGTN"[i % 5] for i in range(LINE_TABLE_N))


def barcode_cases():
    out = []
    rng = np.random.default_rng(15)
    for b in (0, 1, 5, 15):
        Ls = [L for L in (b - 1, b, b + 1, b + 40) if L >= 1]
        recs = [rec(i, L, rng) for i, L in enumerate(Ls * 3)]
        out.append(case(f"barcode_{b}", b"".join(recs), barcode=b))
    return out


TRIM_QUALS = (0, 1, 15, 20, 40)
KEPT_L = (34, 35, 36, 37, 64, 65, 100, 150)


def trim_tails(L, t):
    """name -> qualities (phred values, read order) that drive bwa_trim_read's branches at threshold t."""
    a = min(max(t, 1), 2)
    lo, hi, hi2 = max(t - a, 0), 45, t + a
    tails = collections.OrderedDict()
    tails["low_throughout"] = [0] * L  # the sum only grows: stops at MIN_RDLEN
    tails["low_then_high"] = [hi] * (L - min(10, L)) + [lo] * min(10, L)
    # read from the end: three steps of +1, one of -10 that takes the sum below zero (break), low again before it
    tails["negative_then_low"] = [0] * max(L - 4, 0) + [t + 10] + [max(t - 1, 0)] * min(3, L)
    # from the end: +a, -a, +a: the maximum comes back once and the later (longer) length stays
    tails["maximum_twice"] = [hi] * max(L - 3, 0) + [lo, hi2, lo][-min(3, L):]
    tails["maximum_twice_then_low"] = [0] * max(L - 3, 0) + [lo, hi2, lo][-min(3, L):]
    return tails


def trim_cases():
    out = []
    for t in TRIM_QUALS:
        for il13 in (False, True):
            for b in (0, 5):
                rng = np.random.default_rng(16)
                recs, base = [], 64 if il13 else 33
                for L in KEPT_L:
                    for nm, ql in trim_tails(L, t).items():
                        qual = bytes([base] * b + [base + v for v in ql])
                        recs.append(rec(len(recs), L + b, rng, qual=qual))
                    recs.append(rec(len(recs), L + b, rng, qual=bytes(rng.integers(base, base + 50, L + b, dtype=np.uint8))))
                out.append(case(f"trim_{t}_il13_{int(il13)}_barcode_{b}", b"".join(recs), barcode=b, trim_qual=t, il13=il13))
    return out


BYTES_BASE = b"ACGTTGCAAGGCTTACCGATA"  # 21 bases: records of 52 bytes, which the line table holds
BYTES_POS = (0, 10, 20)


def byte_value_cases():
    rng = np.random.default_rng(17)
    L, recs = len(BYTES_BASE), []
    for v in SEQ_BYTES:
        for pos in BYTES_POS:
            s = bytearray(BYTES_BASE)
            s[pos] = v
            recs.append(rec(len(recs), L, rng, seq=bytes(s)))
    return [case("every_sequence_byte", b"".join(recs), meta=dict(n=len(recs)))]


def small_families():
    """Every block small enough to go through the serial reader in the CPU test, by family."""
    return collections.OrderedDict((
        ("geometry", geometry_cases()), ("strictness", strictness_cases()), ("cap", cap_cases()),
        ("line_table", [case("line_table", line_table_block())]), ("barcode", barcode_cases()),
        ("trim", trim_cases()), ("bytes", byte_value_cases()),
        ("two_bad", [case("two_bad", two_bad_block()), case("two_bad_removed", two_bad_block(bad=()))]),
    ))
