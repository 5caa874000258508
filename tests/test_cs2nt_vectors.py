"""The colour-space decode vectors (tests/golden/cs2nt_vectors.tsv.gz, tools/make_cs_golden.py): row
pairs the reference's cs2nt_DP and cs2nt_nt_qual (cs2nt.c:37-110) were run on.  A restatement of the
two loops reproduces every vector, so the file says what the device kernel must compute, and the
colour goldens' manifest keeps the branch counts their generator asserted."""
import gzip
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
COLOR_MM, NUCL_MM = 19, 25  # cs2nt.c:25-26


def load_vectors():
    """-> list of (nt_ref uint8[size + 1], cs_read uint8[size], result uint8[size - 1])"""
    out = []
    with gzip.open(os.path.join(GOLD, "cs2nt_vectors.tsv.gz"), "rt") as f:
        for line in f:
            ref, cs, res = line.rstrip("\n").split("\t")
            out.append((np.frombuffer(ref.encode(), np.uint8) - ord("0"), np.frombuffer(bytes.fromhex(cs), np.uint8),
                        np.frombuffer(bytes.fromhex(res), np.uint8)))
    return out


def cs2nt(nt_ref, cs_read):
    """cs2nt_DP (cs2nt.c:37-78) then cs2nt_nt_qual (:84-110): -> size - 1 bytes, base << 6 | qual."""
    size = len(cs_read)
    h = [0] * 4 if nt_ref[0] >= 4 else [0 if x == nt_ref[0] else NUCL_MM for x in range(4)]
    bt = [None] * (size + 1)
    for k in range(1, size + 1):
        col, q = int(cs_read[k - 1]) >> 6, int(cs_read[k - 1]) & 0x3f
        g, b = [0] * 4, [0] * 4
        for x in range(4):
            best, ymin = 0x7fffffff, 0
            for y in range(4):
                s = h[y]
                if q != 63 and col != x ^ y:
                    s += max(q, COLOR_MM)
                if nt_ref[k] < 4 and nt_ref[k] != x:
                    s += NUCL_MM
                if s < best:
                    best, ymin = s, y
            g[x], b[x] = best, ymin
        h, bt[k] = g, b
    nt = [0] * (size + 1)
    nt[size] = min(range(4), key=lambda x: (h[x], x))
    for k in range(size - 1, -1, -1):
        nt[k] = bt[k + 1][nt[k + 1]]
    t = [nt[k - 1] ^ nt[k] for k in range(1, size + 1)]
    out = np.zeros(max(size - 1, 0), np.uint8)
    for k in range(1, size):
        c0, c1 = int(cs_read[k - 1]), int(cs_read[k])
        q0, q1 = c0 & 0x3f, c1 & 0x3f
        m0, m1 = t[k - 1] == c0 >> 6, t[k] == c1 >> 6
        q = q0 + q1 + 10 if m0 and m1 else q0 - q1 if m0 else q1 - q0 if m1 else 0
        out[k - 1] = 0 if q0 == 63 or q1 == 63 else nt[k] << 6 | min(max(q, 0), 60)
    return out


@pytest.fixture(scope="module")
def vectors():
    return load_vectors()


def test_vector_file_shape(vectors):
    man = json.load(open(os.path.join(GOLD, "cs_manifest.json")))["vectors"]
    assert len(vectors) == man["n"] == 1501
    sizes = {}
    for ref, cs, res in vectors:
        assert len(ref) == len(cs) + 1 and len(res) == len(cs) - 1 and ref.max() <= 4
        sizes[len(cs)] = sizes.get(len(cs), 0) + 1
    assert {str(k): v for k, v in sizes.items()} == man["sizes"]
    assert set(sizes) == {1, 2, 3, 35, 50, 100, 151, 1000}
    assert sum(1 for ref, _, _ in vectors if ref[0] == 4) > 100
    assert sum(1 for _, cs, _ in vectors if ((cs & 0x3f) == 63).any()) > 100
    # a third are adversarial ties: every quality 6, 19 or 25
    assert sum(1 for _, cs, _ in vectors if set((cs & 0x3f).tolist()) <= {6, 19, 25}) >= len(vectors) // 3


def test_restatement_reproduces_every_vector(vectors):
    for i, (ref, cs, res) in enumerate(vectors):
        got = cs2nt(ref.tolist(), cs.tolist())
        assert got.tobytes() == res.tobytes(), f"vector {i} (size {len(cs)})"


def test_manifest_branch_counts():
    """What tools/make_cs_golden.py asserted of the SAM goldens, from the counts it recorded."""
    man = json.load(open(os.path.join(GOLD, "cs_manifest.json")))
    assert man["dropped"] == []
    assert man["l_pac"] % 16 and man["l_pac"] % 4
    assert len(man["index"]) == 11 and all(os.path.exists(os.path.join(GOLD, f)) for f in man["index"])
    se, pe = man["samse"], man["sampe"]
    assert se["cs_r1.default"]["counts"]["own_indel"] >= 50
    assert pe["cs.R"]["counts"]["XT_M"] >= 50
    assert se["cs_r1.n5"]["counts"]["XA_indel"] >= 10
    assert se["cs_r1.default"]["counts"]["strand1_cigar"] >= 1
    assert se["cs_edge.default"]["counts"]["pos0"] >= 1
    for grp in (se, pe):
        for m in grp.values():
            assert os.path.getsize(os.path.join(GOLD, m["sam"])) < 400 * 1000
