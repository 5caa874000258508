"""tests/golden/refine_vectors.tsv.gz (tools/make_refine_golden.py: the reference's bwa_refine_gapped over
hand-made hits) parses, keeps every category of edge case, and its MD / NM columns follow from its
own pos / CIGAR / read columns by a plain restatement of bwa_cal_md1 (bwase.c:243-295) over the .pac
files -- so the GPU tests that replay the vectors (test_refine_gpu.py) compare against consistent data."""
import gzip
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LENGTHS = [1, 2, 17, 36, 100, 150, 250]
# every category the fixture must keep at least 20 vectors of
CATEGORIES = ([f"len{x}" for x in LENGTHS] + ["ins", "del", "lead_indel", "trail_indel", "D_lead", "S_lead", "S_trail",
                                              "sub", "readN", "strand0", "strand1", "pos0", "pos1_5"] +
              [f"res{r}" for r in range(16)] +
              ["clamp0", "clip_lpac", "pos_eq_lpac", "boundary", "multi", "own", "ungapped", "ungapped_hang",
               "md_refined", "md_pre", "md_zero", "run10", "run100"])


def parse_cigar(s):
    """'15M2S' -> [bwa_cigar_t]; '*' -> None"""
    if s == "*":
        return None
    return [("MIDS".index(op) << 29) | int(n) for n, op in re.findall(r"(\d+)([MIDS])", s)]


def load_vectors():
    out = []
    with gzip.open(os.path.join(GOLD, "refine_vectors.tsv.gz"), "rt") as f:
        for ln in f:
            c = ln.rstrip("\n").split("\t")
            assert len(c) == 12, ln
            out.append(dict(set=c[0], pos=int(c[1]), ext=int(c[2]), len=int(c[3]), type=c[4],
                            codes=np.frombuffer(c[5].encode(), np.uint8) - ord("0"),
                            md_pos=None if c[6] == "*" else int(c[6]), pos1=int(c[7]), cigar=parse_cigar(c[8]),
                            cigar_text=c[8], md=None if c[9] == "*" else c[9], nm=None if c[10] == "*" else int(c[10]),
                            tags=set(c[11].split(","))))
    return out


def load_sets():
    """set name -> (codes of the references back to back, [(pac bytes, l_pac)])"""
    man = json.load(open(os.path.join(GOLD, "refine_vectors.json")))
    sets = {}
    for name, s in man["sets"].items():
        parts, codes = [], []
        for ref, l_pac in zip(s["references"], s["l_pac"]):
            b = np.fromfile(os.path.join(GOLD, ref + ".pac"), dtype=np.uint8)
            assert int(open(os.path.join(GOLD, ref + ".ann")).readline().split()[0]) == l_pac
            codes.append(np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=1).reshape(-1)[:l_pac])
            parts.append((b, l_pac))
        sets[name] = (np.concatenate(codes), parts)
    return sets


def cal_md1(text, pos, codes, cigar):
    """bwa_cal_md1 (bwase.c:243-295) -> (MD, NM)"""
    l_pac, x, y, u, nm, out, c = len(text), pos, 0, 0, 0, [], 0

    def cmp(c, s):
        nonlocal u, nm
        if c > 3 or s > 3 or c != s:
            out.append(f"{u}{'ACGTN'[c]}")
            nm += 1
            u = 0
        else:
            u += 1

    if cigar is not None:
        for cg in cigar:
            ln, op = cg & 0x1FFFFFFF, cg >> 29
            if op == 0:
                for z in range(ln):
                    if x + z >= l_pac:
                        break
                    cmp(int(text[x + z]), int(codes[y + z]))
                x += ln
                y += ln
            elif op in (1, 3):
                y += ln
                nm += ln if op == 1 else 0
            elif op == 2:
                out.append(f"{u}^" + "".join("ACGT"[int(text[x + z])] for z in range(ln) if x + z < l_pac))
                u = 0
                x += ln
                nm += ln
    else:
        for z in range(len(codes)):
            if x + z < l_pac:
                c = int(text[x + z])  # past l_pac nothing is extracted: c keeps its value
            cmp(c, int(codes[z]))
    out.append(str(u))
    return "".join(out), nm


@pytest.fixture(scope="module")
def vectors():
    return load_vectors()


def test_fixture_parses(vectors):
    path = os.path.join(GOLD, "refine_vectors.tsv.gz")
    assert os.path.getsize(path) < 1_000_000 and len(gzip.open(path).read()) < 1_000_000  # packed and unpacked
    for v in vectors:
        assert v["set"] in "AB" and v["type"] in ("own", "multi", "ungapped")
        assert len(v["codes"]) == v["len"] and v["codes"].max() <= 4
        assert (v["ext"] == 0) == (v["type"] == "ungapped") == (v["cigar"] is None)
        assert (v["md"] is None) == (v["type"] == "multi") == (v["md_pos"] is None) == (v["nm"] is None)
        if v["cigar"] is not None:
            # the CIGAR covers the read: M, I and S consume it
            assert sum(c & 0x1FFFFFFF for c in v["cigar"] if c >> 29 != 2) == v["len"], v


def test_manifest_counts_and_categories(vectors):
    man = json.load(open(os.path.join(GOLD, "refine_vectors.json")))
    assert man["vectors"] == len(vectors) and 1500 <= len(vectors) <= 2500
    counts = {}
    for v in vectors:
        for t in v["tags"]:
            counts[t] = counts.get(t, 0) + 1
    assert counts == man["tags"]
    few = {t: counts.get(t, 0) for t in CATEGORIES if counts.get(t, 0) < 20}
    assert not few, f"categories with fewer than 20 vectors: {few}"
    # the tags say what the columns show
    sets = man["sets"]
    for v in vectors:
        l_pac = sum(sets[v["set"]]["l_pac"])
        t = v["tags"]
        assert v["pos"] <= l_pac and f"res{v['pos'] % 16}" in t and f"len{v['len']}" in t
        if "clamp0" in t:
            assert v["ext"] < 0 and v["pos"] < -v["ext"]
        if "clip_lpac" in t:
            assert v["ext"] > 0 and v["pos"] + v["len"] + v["ext"] > l_pac
        if "pos_eq_lpac" in t:
            assert v["pos"] == l_pac
        if "ungapped_hang" in t:
            assert v["pos"] < l_pac < v["pos"] + v["len"]
        if "boundary" in t:
            b = sets["B"]["l_pac"][0]
            assert v["set"] == "B" and v["pos"] < b < v["pos"] + v["len"] + abs(v["ext"])
        if v["type"] == "ungapped":
            assert v["pos"] < l_pac
        if "md_refined" in t:
            assert v["md_pos"] == v["pos1"]
        if "md_pre" in t:
            assert v["md_pos"] == v["pos"]
        if "md_zero" in t:
            assert v["md_pos"] == 0
    assert sets["A"]["l_pac"][0] % 4 != 0, "the second reference of set B must start inside a byte"


def test_md_restatement_reproduces_every_vector(vectors):
    sets = load_sets()
    n = 0
    for v in vectors:
        if v["md"] is None:
            continue
        md, nm = cal_md1(sets[v["set"]][0], v["md_pos"], v["codes"], v["cigar"])
        assert (md, nm & 0xfff) == (v["md"], v["nm"]), v
        n += 1
    assert n > 1000
