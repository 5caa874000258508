#!/usr/bin/env python3
"""Generate tests/golden/extend/ (build container only): known answers of the reference's aln_extend_core
and of aln_stdaln_aux(type 2), read through ctypes from oracle/_ref/libibwa_ref.so.

TEST INFRASTRUCTURE.  Two files, data only:

* extend_vectors.tsv.gz: pairs with their parameter set, band, G0 and mode (score / end / path through
  aln_extend_core, std2 through aln_stdaln_aux) and the reference's score, end cell, path length, path
  start and CIGAR.  A band of 0 stands for len1 + len2, which is what the reference is called with.
* seed_vectors.tsv.gz: seeds on the two sets of tests/golden/refine_vectors.json (position, direction,
  lt, rev, query, G0) answered by aln_extend_core in end-cell mode over the window this tool cuts from
  the sets' .pac files by the rule of ibwa_extend_seeds.

Inputs come from random.Random with fixed seeds and from slices of the seeded synthetic genome.  A
restatement of the reference's loop classifies each pair (how the loop ended, ties, rebasing); it must
agree with the reference's score on every pair it is run on.  The tool prints how many vectors fall
into each class and fails if one is empty.
"""
import collections
import ctypes
import gzip
import io
import os
import random
import re
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REFLIB = os.path.join(ROOT, "oracle", "_ref", "libibwa_ref.so")
OUT = os.path.join(ROOT, "tests", "golden", "extend")
AA = "ARNDCQEGHILKMFPSTWYV"
NT = {ch: k for k, ch in enumerate("AGCT")}  # aln_nt4_table's codes; anything else is 4
AAC = dict({ch: k for k, ch in enumerate(AA)}, **{"*": 20})


class AlnParam(ctypes.Structure):
    _fields_ = [("gap_open", ctypes.c_int), ("gap_ext", ctypes.c_int), ("gap_end", ctypes.c_int),
                ("matrix", ctypes.POINTER(ctypes.c_int)), ("row", ctypes.c_int), ("band_width", ctypes.c_int)]


class AlnAln(ctypes.Structure):
    _fields_ = [("path", ctypes.c_void_p), ("path_len", ctypes.c_int), ("start1", ctypes.c_int), ("end1", ctypes.c_int),
                ("start2", ctypes.c_int), ("end2", ctypes.c_int), ("score", ctypes.c_int), ("subo", ctypes.c_int),
                ("out1", ctypes.c_void_p), ("out2", ctypes.c_void_p), ("outm", ctypes.c_void_p),
                ("n_cigar", ctypes.c_int), ("cigar32", ctypes.POINTER(ctypes.c_uint32))]


class Path(ctypes.Structure):
    _fields_ = [("i", ctypes.c_int), ("j", ctypes.c_int), ("ctype", ctypes.c_ubyte)]


def encode(pname, s):
    tab = AAC if pname == "aa2aa" else NT
    return bytes(tab.get(ch.upper(), 21 if pname == "aa2aa" else 4) for ch in s)


def restate(mat, row, q, r, band, a, b, g0):
    """The reference's loop (stdaln.c:901-973) -> (score, end_i, end_j, how it ended, ties, rebased)."""
    n1, n2, qr = len(a), len(b), q + r
    eh = [0] * (n1 + 2)
    eh[1] = g0 << 16
    start, end, score, of_base, over, end_i, end_j, ties, rebased, how = 1, 2, 0, 0, False, 0, 0, 0, False, "rows"
    for j in range(1, n2 + 1):
        h1 = f = 0
        srow = mat[b[j - 1] * row:(b[j - 1] + 1) * row]
        start = max(start, j - band, 1)
        end = min(end, j + band, n1 + 1)
        if start == end:
            how = "start==end"
            break
        if over:
            score -= 16000
            of_base += 16000
            over, rebased, ties = False, True, 0
            for i in range(start, end + 1):
                h, e = eh[i] >> 16, eh[i] & 0xffff
                eh[i] = max(h - 16000, 0) << 16 | max(e - 16000, 0)
        first = last = 0
        for i in range(start, end):
            h, e = eh[i] >> 16, eh[i] & 0xffff
            nv = h1 << 16
            if h:
                h += srow[a[i - 1]]
            h = max(h, e, f)
            h1 = h
            if h > 0:
                if not first:
                    first = i
                last = i
                if score < h:
                    score, end_i, end_j, ties = h, i, j, 0
                    over = over or score > 32000
                elif score == h:
                    ties += 1
            h = max(h - qr, 0)
            e = max(e - r, h)
            f = max(f - r, h)
            eh[i] = nv | e
        if end >= 0:
            eh[end] = (h1 << 16) & 0xffffffff
        if last <= 0:
            how = "no positive"
            break
        start, end = first, last + 3
    return score + of_base - 1, end_i, end_j, how, ties, rebased


def mutate(rng, s, alphabet, sub=0.04, indel=0.01, gap=1):
    out = []
    for ch in s:
        x = rng.random()
        if x < sub:
            out.append(rng.choice(alphabet))
        elif x < sub + indel:
            continue
        elif x < sub + 2 * indel:
            out.append(ch + "".join(rng.choice(alphabet) for _ in range(rng.randint(1, gap))))
        else:
            out.append(ch)
    return "".join(out)


class Gen:
    def __init__(self):
        L = self.L = ctypes.CDLL(REFLIB, mode=os.RTLD_LAZY)  # its @PG printer lives in the harness executable, not needed here
        L.aln_extend_core.restype = ctypes.c_int
        L.aln_extend_core.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(AlnParam),
                                      ctypes.POINTER(Path), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_void_p]
        L.aln_global_core.restype = ctypes.c_int
        L.aln_global_core.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(AlnParam),
                                      ctypes.POINTER(Path), ctypes.POINTER(ctypes.c_int)]
        L.aln_path2cigar32.restype = ctypes.POINTER(ctypes.c_uint32)
        L.aln_path2cigar32.argtypes = [ctypes.POINTER(Path), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.aln_stdaln_aux.restype = ctypes.POINTER(AlnAln)
        L.aln_stdaln_aux.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(AlnParam), ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int]
        L.aln_free_AlnAln.argtypes = [ctypes.POINTER(AlnAln)]
        L.aln_free_AlnAln.restype = None
        L.free.argtypes = [ctypes.c_void_p]
        self.presets = {k: AlnParam.in_dll(L, "aln_param_" + k) for k in ("blast", "bwa", "aa2aa")}
        # the custom scheme of make_stdsw_golden.py (match 5, anything else -2, open 10, extend 2), and bwasw's defaults
        self.keep = [(ctypes.c_int * 25)(*[5 if x == y else -2 for x in range(5) for y in range(5)]),
                     (ctypes.c_int * 25)(*[1 if x == y and x < 4 else -3 for x in range(5) for y in range(5)])]
        self.presets["match5"] = AlnParam(10, 2, 2, self.keep[0], 5, 50)
        self.presets["bwasw"] = AlnParam(5, 2, 2, self.keep[1], 5, 50)
        self.rows = []
        self.classes = collections.Counter()

    def param(self, pname, band, n1, n2):
        src = self.presets[pname]
        return AlnParam(src.gap_open, src.gap_ext, src.gap_end, src.matrix, src.row, band if band > 0 else n1 + n2)

    def core(self, pname, band, g0, a, b, mode):
        """aln_extend_core on code strings -> (score, end_i, end_j, path_len, start_i, start_j, cigar)"""
        ap = self.param(pname, band, len(a), len(b))
        path = (Path * (len(a) + len(b) + 2))()
        if mode == "score":
            return (self.L.aln_extend_core(a, len(a), b, len(b), ctypes.byref(ap), None, None, g0, None), "", "", "", "", "", "")
        if mode == "end":
            sc = self.L.aln_extend_core(a, len(a), b, len(b), ctypes.byref(ap), path, None, g0, None)
            return (sc, path[0].i, path[0].j, "", "", "", "") if sc > 0 else (sc, 0, 0, "", "", "", "")
        pl, nc = ctypes.c_int(0), ctypes.c_int(0)
        sc = self.L.aln_extend_core(a, len(a), b, len(b), ctypes.byref(ap), path, ctypes.byref(pl), g0, None)
        if pl.value <= 0 or not a or not b:
            return (sc, 0, 0, 0, "", "", "")
        cg = self.L.aln_path2cigar32(path, pl.value, ctypes.byref(nc))
        cig = "".join(f"{cg[k] >> 4}{'MID'[cg[k] & 0xf]}" for k in range(nc.value))
        self.L.free(cg)
        return (sc, path[0].i, path[0].j, pl.value, path[pl.value - 1].i, path[pl.value - 1].j, cig)

    def add(self, tag, pname, band, g0, s1, s2, modes=("score", "end", "path")):
        a, b = encode(pname, s1), encode(pname, s2)
        src = self.presets[pname]
        bw = band if band > 0 else len(a) + len(b)
        C = self.classes
        ext = self.core(pname, band, g0, a, b, "score")[0]
        end = self.core(pname, band, g0, a, b, "end")
        if a and b and len(a) * min(len(b), 2 * bw + 1) <= 400000:
            mat = [src.matrix[k] for k in range(src.row * src.row)]
            sc, ei, ej, how, ties, rebased = restate(mat, src.row, src.gap_open, src.gap_ext, bw, a, b, g0)
            assert (sc, ei, ej) == (ext, end[1], end[2]) or (sc <= 0 and sc == ext), (tag, sc, ei, ej, ext, end)
            C["ends by " + how] += 1
            C["ties"] += ties > 0
            C["rebased"] += rebased
        if not a or not b:
            C["empty"] += 1
        C[f"band {band if band in (1, 2, 3, 50) else ('<=0' if band <= 0 else 'other')}"] += 1
        C["preset " + pname] += 1
        C["G0 1" if g0 == 1 else "G0 mid" if g0 <= 100 else "G0 large"] += 1
        C["N codes"] += pname != "aa2aa" and (4 in a or 4 in b)
        C["G0 unbeaten"] += g0 > 1 and 0 < ext <= g0
        C["score <= 0"] += ext <= 0 and bool(a) and bool(b)
        C["1x1"] += len(a) == 1 and len(b) == 1
        C["1xn"] += len(a) == 1 and len(b) > 1
        C["nx1"] += len(a) > 1 and len(b) == 1
        C["len1 >> len2"] += len(a) >= 4 * len(b) > 0
        C["len2 >> len1"] += len(b) >= 4 * len(a) > 0
        for mode in modes:
            if mode == "std2":
                ap = self.param(pname, band, len(a), len(b))
                aa = self.L.aln_stdaln_aux(s1.encode(), s2.encode(), ctypes.byref(ap), 2, 1, len(s1), len(s2))
                r = aa.contents
                if r.path_len > 0:
                    cig = "".join(f"{r.cigar32[k] >> 4}{'MID'[r.cigar32[k] & 0xf]}" for k in range(r.n_cigar))
                    rec = (r.score, r.end1, r.end2, r.path_len, r.start1, r.start2, cig)
                else:  # no path: the other fields are not set by the reference
                    rec = (r.score, 0, 0, 0, "", "", "")
                self.L.aln_free_AlnAln(aa)
                if g0 == 1:  # the tables above are the reference's: the codes give what the letters give
                    assert rec[0] == self.core(pname, band, 1, a, b, "path")[0], (tag, rec)
                C["std2"] += 1
            else:
                rec = end if mode == "end" else self.core(pname, band, g0, a, b, mode)
            if mode == "path" and rec[3]:
                C["path G0 1" if g0 == 1 else "path G0 > 1"] += 1
                C["no suitable bandwidth"] += ext > rec[0]
                if g0 == 1:  # does the first band already give the extension score?
                    ap = self.param(pname, band, len(a), len(b))
                    ap.gap_end = -1
                    path, pl = (Path * (len(a) + len(b) + 2))(), ctypes.c_int(0)
                    g = self.L.aln_global_core(a, rec[1], b, rec[2], ctypes.byref(ap), path, ctypes.byref(pl))
                    C["band doubled"] += g != ext
                C["path past 32000"] += ext > 32000
                C["long gap in path"] += any(int(x[:-1]) >= 20 for x in re.findall(r"\d+[ID]", rec[6]))
            if mode == "end":
                C["end past 32000"] += ext > 32000
            self.rows.append((tag, pname, mode, band if band > 0 else 0, g0, s1, s2) + tuple(rec))
        return ext


def library_part(genome, G):
    rng = random.Random(20263)
    g = genome.replace("N", "")
    rs = lambda n, al="ACGT": "".join(rng.choice(al) for _ in range(n))  # noqa: E731
    piece = lambda n: (lambda a: g[a:a + n])(rng.randrange(0, len(g) - n))  # noqa: E731
    # 1 x 1, 1 x n, n x 1 and empty, every band kind
    for band in (1, 2, 3, 50, 0):
        for pname in ("blast", "bwa"):
            G.add("1x1_match", pname, band, 1, "A", "A")
            G.add("1x1_mismatch", pname, band, 1, "A", "C")
            G.add("1x1_g0", pname, band, 9, "A", "C")
        s = piece(120)
        G.add("1xn", "blast", band, 1, s[0], s)
        G.add("nx1", "blast", band, 1, s, s[0])
        G.add("empty1", "blast", band, 1, "", s[:9], modes=("score", "end", "path"))
        G.add("empty2", "blast", band, 1, s[:9], "")
    # the grid: related pairs over the presets, bands, G0 kinds and both length skews
    for pname in ("blast", "bwa", "aa2aa", "match5", "bwasw"):
        al = AA if pname == "aa2aa" else "ACGT"
        for band in (1, 2, 3, 50, 0, 17):
            for n1 in (5, 31, 64, 65, 150, 400):
                a = rs(n1, AA) if pname == "aa2aa" else piece(n1)
                b = mutate(rng, a, al, 0.05, 0.015, 6) + rs(rng.randrange(0, 30), al)
                k = rng.random()
                if k < 0.2 and len(b) > 8:
                    b = b[:max(1, len(b) // 5)]    # len1 >> len2
                elif k < 0.4 and len(a) > 8:
                    a = a[:max(1, len(a) // 5)]    # len2 >> len1
                if pname != "aa2aa" and rng.random() < 0.25:
                    t = list(b)
                    t[rng.randrange(len(t))] = "N"
                    b = "".join(t)
                g0 = rng.choice([1, 1, rng.randint(2, 60), 30000])
                G.add("grid", pname, band, g0, a, b, modes=("score", "end", "path") + (("std2",) if g0 == 1 else ()))
    # unrelated pairs: the extension dies in the first rows; a G0 that nothing improves on
    for _ in range(30):
        a, b = rs(rng.randint(2, 90)), rs(rng.randint(2, 90))
        G.add("unrelated", rng.choice(["blast", "bwa", "bwasw"]), rng.choice([1, 3, 50, 0]), rng.choice([1, 40, 25000]), a, b)
    # ties: low complexity
    for unit in ("A", "AC", "ACG", "AACGT"):
        for reps in (3, 12):
            G.add("tie", "blast", rng.choice([3, 50, 0]), 1, unit * reps, unit * (reps + 2), modes=("score", "end", "path", "std2"))
            G.add("tie", "match5", 50, 7, unit * reps + "T" + unit * reps, unit * reps + unit * reps)
    # long gaps under the cheap scheme, in either sequence
    for k in range(12):
        blocks = [piece(rng.randint(50, 110)) for _ in range(3)]
        a = "".join(blocks)
        b = blocks[0] + rs(rng.randint(20, 45)) + blocks[1] + rs(rng.randint(20, 45)) + blocks[2]
        if k & 1:
            a, b = b, a
        G.add("long_gap", "match5", (50, 0, 30)[k % 3], 1 if k & 2 else 20, a, b, modes=("end", "path", "std2") if k & 2 else ("end", "path"))
    # band doubling: a narrow first band beside gaps it cannot hold
    for k in range(12):
        a = piece(rng.randint(80, 200))
        cut = rng.randrange(20, len(a) - 30)
        b = a[:cut] + a[cut + rng.randint(4, 9):]
        G.add("doubling", "match5", rng.choice([10, 12, 16]), 1, a, b, modes=("end", "path", "std2"))
    # the whole eh row (band len1 + len2) on both sides of the 160 words a lane has in LDS
    for n1 in (40, 100, 157, 158, 159, 160, 200, 300, 600, 1000) * 2:
        a = piece(n1)
        G.add("eh_row", "blast", 0, rng.choice([1, 1, 30]), a, mutate(rng, a, "ACGT", 0.04, 0.01, 4), modes=("score", "end"))
    # rebasing: the bwa preset, about 3 000 near-identical bases, score past 32000
    for k in range(3):
        a = piece(3100 + 40 * k)
        b = mutate(rng, a, "ACGT", 0.003, 0.001 if k else 0, 2)
        modes = ("score", "end", "path", "std2") if k == 0 else ("score", "end", "path") if k == 1 else ("score", "end")
        sc = G.add("rebasing", "bwa", 50, 1 if k < 2 else 500, a, b, modes=modes)
        assert sc > 32000, sc


def seed_part(G):
    from tests.test_refine_vectors import load_sets
    rng = random.Random(20264)
    sets = load_sets()
    rows = []
    n = collections.Counter()
    for name in sorted(sets):
        text, parts = sets[name]
        T, first = len(text), parts[0][1]
        spots = [rng.randrange(300, T - 300) for _ in range(40)] + [1, 2, T - 1, T, 0, 150, T - 150]
        if len(parts) > 1:
            spots += [first - 20, first + 20, first, first - 60, first + 60]  # windows across the boundary inside the set
        for pos in spots:
            for direction in (0, 1):
                for rev in (0, 1):
                    if direction and pos > T:
                        continue
                    lq = 150 if abs(pos - first) <= 60 else rng.choice([20, 60, 150])  # long enough to cross the boundary
                    lt = lq + lq // 2
                    if direction and rng.random() < 0.7:
                        lt = min(lt, max(pos - 1, 0))  # the caller's clip for bsw2_extend_left
                    rd = (lambda x: text[T - x - 1]) if rev else (lambda x: text[x])
                    xs = range(pos - 1, max(pos - 1 - lt, -1), -1) if direction else range(pos, min(pos + lt, T))
                    win = bytes(int(rd(x)) for x in xs)
                    q = "".join("ACGT"[c] for c in win[:lq]) or "ACGT"[rng.randrange(4)]
                    q = mutate(rng, q, "ACGT", 0.05, 0.01, 3) or "A"
                    qc = bytes("ACGT".index(ch) for ch in q)
                    g0 = rng.choice([1, 1, 25, 300])
                    pname = rng.choice(["bwasw", "bwa"])
                    sc, ei, ej = G.core(pname, 50, g0, win, qc, "end")[:3] if win else (-1, 0, 0)
                    rows.append((name, pname, pos, direction, lt, rev, g0, "".join(str(c) for c in qc), sc, ei, ej))
                    n["left" if direction else "right"] += 1
                    n["rev" if rev else "fwd"] += 1
                    n["empty window"] += not win
                    n["extended"] += sc > g0
                    n["base 1 / last base"] += pos in (1, T - 1, T)
                    if len(parts) > 1 and win:
                        lo, hi = min(xs), max(xs)
                        n["across references"] += (T - hi - 1 if rev else lo) < first <= (T - lo - 1 if rev else hi)
    for k in ("left", "right", "rev", "fwd", "empty window", "extended", "base 1 / last base", "across references"):
        print(f"  seeds: {k}: {n[k]}")
        assert n[k] > 0, f"no seed vector of class '{k}'"
    path = os.path.join(OUT, "seed_vectors.tsv.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as gz, io.TextIOWrapper(gz) as f:
        f.write("#set\tparam\tpos\tdir\tlt\trev\tg0\tquery codes\tscore\tend_i\tend_j\n")
        for r in rows:
            f.write("\t".join(str(x) for x in r) + "\n")
    print(f"{len(rows)} seed vectors -> {path} ({os.path.getsize(path)} B)")


NEEDED = ["1x1", "1xn", "nx1", "len1 >> len2", "len2 >> len1", "band 1", "band 2", "band 3", "band 50", "band <=0",
          "ends by start==end", "ends by no positive", "ends by rows", "G0 1", "G0 mid", "G0 large", "G0 unbeaten", "score <= 0", "ties",
          "long gap in path", "preset blast", "preset bwa", "preset aa2aa", "preset match5", "preset bwasw", "N codes", "path G0 1",
          "path G0 > 1", "no suitable bandwidth", "band doubled", "rebased", "end past 32000", "path past 32000", "empty", "std2"]


def main():
    if not os.path.exists(REFLIB):
        sys.exit("needs oracle/_ref/libibwa_ref.so (make -C oracle ref)")
    from tests.synth_util import golden_genome_ascii
    genome, _, _ = golden_genome_ascii()
    os.makedirs(OUT, exist_ok=True)
    G = Gen()
    library_part(genome, G)
    for k in NEEDED:
        print(f"  {k}: {G.classes[k]}")
    empty = [k for k in NEEDED if not G.classes[k]]
    if empty:
        sys.exit(f"empty classes: {empty}")
    path = os.path.join(OUT, "extend_vectors.tsv.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as gz, io.TextIOWrapper(gz) as f:
        f.write("#tag\tparam\tmode\tband(0: len1+len2)\tg0\tseq1\tseq2\tscore\tend_i\tend_j\tpath_len\tstart_i\tstart_j\tcigar\n")
        for r in G.rows:
            f.write("\t".join(str(x) for x in r) + "\n")
    print(f"{len(G.rows)} library vectors -> {path} ({os.path.getsize(path)} B)")
    seed_part(G)


if __name__ == "__main__":
    main()
