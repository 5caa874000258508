"""Colour space on the device (cs2nt.hip): k_cs2nt against the reference's cs2nt_DP / cs2nt_nt_qual
vectors (tests/golden/cs2nt_vectors.tsv.gz), the device row construction of bwa_cs2nt_core
(cs2nt.c:136-171) against rows built here from an unpack of csg.nt.pac, and k_pac2cs against the xor
rule and the reference's colour .pac."""
import os
import random

import numpy as np
import pytest

from tests.test_cs2nt_vectors import cs2nt as cs2nt_py
from tests.test_cs2nt_vectors import load_vectors

pytestmark = pytest.mark.gpu

M, I, D, S = 0, 1, 2, 3  # bwa_cigar_t operations (bwtaln.h:44-49)


@pytest.fixture(scope="module")
def eng():
    from ibwa_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def vectors():
    return load_vectors()


def _read_pac(path):
    raw = np.frombuffer(open(path, "rb").read(), np.uint8)
    l_pac = (raw.size - 2) * 4 + int(raw[-1])
    codes = ((raw[:-1, None] >> np.array([6, 4, 2, 0], np.uint8)) & 3).reshape(-1)[:l_pac]
    return raw, codes.astype(np.uint8), l_pac


def _pack(codes):
    c = np.zeros((len(codes) + 3) // 4 * 4, np.uint8)
    c[:len(codes)] = codes
    c = c.reshape(-1, 4)
    return (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)


def _check(got, vectors):
    assert len(got) == len(vectors)
    for i, (g, (_, cs, want)) in enumerate(zip(got, vectors)):
        assert g.tobytes() == want.tobytes(), f"vector {i} (size {len(cs)})"


def test_rows_equal_every_vector_in_one_batch(eng, vectors):
    assert len(vectors) == 1501 and len(vectors) % 64
    _check(eng.cs2nt_rows([v[0] for v in vectors], [v[1] for v in vectors]), vectors)


def test_rows_batch_of_one(eng, vectors):
    for v in (next(v for v in vectors if len(v[1]) == 1), next(v for v in vectors if len(v[1]) == 50)):
        _check(eng.cs2nt_rows([v[0]], [v[1]]), [v])


def test_rows_thousand_long_alone(eng, vectors):
    long = [v for v in vectors if len(v[1]) == 1000]
    assert len(long) == 20
    _check(eng.cs2nt_rows([v[0] for v in long], [v[1] for v in long]), long)


def _rows(nt, l_pac, pos, strand, seq, qual, cigar):
    """bwa_cs2nt_core's nt_ref / cs_read (cs2nt.c:136-171); a base at or past l_pac counts as 4."""
    n = len(seq)

    def base(g):
        return int(nt[g]) if g < l_pac else 4

    def csbase(i):
        q = min(qual[n - 1 - i if strand else i] - 33, 60)
        if seq[i] > 3:
            q = 63
        return (int(seq[i]) << 6 | q) & 0xff

    ref, cs = [base(pos - 1) if pos else 4], []
    x, y = pos, 0
    for w in (cigar if cigar is not None else [M << 29 | n]):
        op, ln = w >> 29, w & 0x1fffffff
        for _ in range(ln if op in (M, I) else 0):
            ref.append(base(x) if op == M else 4)
            cs.append(csbase(y))
            x += op == M
            y += 1
        if op == S:
            y += ln
        elif op == D:
            x += ln
    return np.array(ref, np.uint8), np.array(cs, np.uint8)


def test_device_rows_equal_host_rows(eng, golden_dir):
    raw, nt, l_pac = _read_pac(os.path.join(golden_dir, "csg.nt.pac"))
    rnd = random.Random(7)
    jobs = []
    for j in range(200):
        n = rnd.choice((35, 50, 50, 51, 76))
        shape = j % 8
        if shape < 3:
            cigar, span = None, n
        else:
            a = rnd.randrange(5, n - 12)
            g = rnd.randrange(1, 4)
            if shape == 3:
                ops = [(M, a), (I, g), (M, n - a - g)]
            elif shape == 4:
                ops = [(M, a), (D, g), (M, n - a)]
            elif shape == 5:
                ops = [(S, g), (M, n - g - 2), (S, 2)]
            elif shape == 6:
                ops = [(S, 1), (M, a), (I, 1), (M, 3), (D, 2), (M, n - a - 5 - g), (S, g)]
            else:
                ops = [(I, g), (M, a), (D, 1), (M, n - a - g)]  # refine leaves no leading I; the kernel takes it
            cigar = [op << 29 | ln for op, ln in ops]
            span = sum(ln for op, ln in ops if op in (M, D))
        if j in (0, 1, 3):
            pos = 0
        elif j in (2, 4, 5):
            pos = l_pac - span  # the last base
        elif j == 6:
            pos = l_pac - span + 7  # runs past l_pac: those bases count as 4
        else:
            pos = rnd.randrange(1, l_pac - span)
        seq = np.array([rnd.choice((0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 4)) for _ in range(n)], np.uint8)
        # near the reference, so that the decode is not all ties: colours of the bases at pos
        if j % 3 and pos and pos + n < l_pac:
            seq = (nt[pos - 1:pos + n - 1] ^ nt[pos:pos + n]).astype(np.uint8)
            if j % 2:
                seq[rnd.randrange(n)] ^= 1
        qual = bytes(33 + rnd.choice((0, 5, 19, 25, 30, 40, 60, 70, 93)) for _ in range(n))
        jobs.append((pos, j & 1 if j > 6 else j % 2, seq, qual, cigar))
    eng.load_ntpac([raw], [l_pac])
    got = eng.cs2nt([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs],
                    [j[4] for j in jobs])
    rows = [_rows(nt, l_pac, *j) for j in jobs]
    want = eng.cs2nt_rows([r[0] for r in rows], [r[1] for r in rows])
    assert sum(1 for j in jobs if j[1]) > 50 and sum(1 for j in jobs if j[4]) > 100
    for k, (g, w, (ref, cs)) in enumerate(zip(got, want, rows)):
        assert len(g) == len(cs) - 1, f"job {k}"
        assert g.tobytes() == w.tobytes(), f"job {k}"
        assert g.tobytes() == cs2nt_py(ref.tolist(), cs.tolist()).tobytes(), f"job {k}"
    # without CIGARs at all (n_cigar == NULL)
    plain = [j for j in jobs if j[4] is None]
    got = eng.cs2nt([j[0] for j in plain], [j[1] for j in plain], [j[2] for j in plain], [j[3] for j in plain])
    for g, j in zip(got, plain):
        ref, cs = _rows(nt, l_pac, *j)
        assert g.tobytes() == cs2nt_py(ref.tolist(), cs.tolist()).tobytes()


def test_pac2cspac(eng, golden_dir):
    _, nt, l_pac = _read_pac(os.path.join(golden_dir, "csg.nt.pac"))
    cs_raw, cs_codes, l_cs = _read_pac(os.path.join(golden_dir, "csg.pac"))
    assert l_cs == l_pac and l_pac % 16 and l_pac % 4
    for n in (1, 3, 4, 5, 15, 16, 17, 1023, 1025, l_pac):
        got = eng.pac2cspac(_pack(nt[:n]), n)
        want = nt[:n].copy()
        want[1:] ^= nt[:n - 1]  # colour i = base i - 1 xor base i; symbol 0 is base 0
        packed = np.zeros(n // 4 + 1, np.uint8)  # what bwa_pac2cspac writes before the count byte
        p = _pack(want)
        packed[:p.size] = p
        assert got.tobytes() == packed.tobytes(), f"l_pac {n}"
        assert (want == cs_codes[:n]).all()
    assert got.tobytes() == cs_raw[:l_pac // 4 + 1].tobytes()  # the fixture's own length: the reference's file


def test_errors(eng, vectors):
    from ibwa_amd.engine import Engine, IbwaError
    fresh = Engine(0)
    try:
        with pytest.raises(IbwaError, match="ibwa_ctx_load_ntpac"):
            fresh.cs2nt([0], [0], [np.zeros(50, np.uint8)], [b"I" * 50])
    finally:
        fresh.close()
    v = vectors[0]
    with pytest.raises(IbwaError, match="size 0"):
        eng.cs2nt_rows([v[0], np.zeros(1, np.uint8)], [v[1], np.zeros(0, np.uint8)])
