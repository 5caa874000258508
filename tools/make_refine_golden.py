#!/usr/bin/env python3
"""Known answers for ibwa_refine_batch / ibwa_md_batch, from the reference's own bwa_refine_gapped
(run in the build container).

TEST INFRASTRUCTURE.  oracle/_ref/libibwa_ref.so (the reference compiled from its sources by
oracle/Makefile) is called through ctypes: dbset_restore (dbset.c:135) over two sets and
bwa_refine_gapped (bwase.c:333) over hand-made bwa_seq_t records, one per vector.

  set A  tests/golden/g1m                      l_pac 998 593 (998593 % 4 == 1: no multiple of 4)
  set B  g1m + idx_quirks, remap = 0           l_pac 998 593 + 52 000; idx_quirks starts at a bit
                                               offset of 2 inside a byte of the packed set

A read is cut from the set's text at a chosen place, then edited (insertions, deletions,
substitutions, N).  Its codes are kept in the orientation bwa_refine_gapped passes them to
refine_gapped_core (strand 0: bwa_seq_t.seq holds them reversed, as bwa_read_seq leaves it; strand 1:
bwa_seq_t.rseq).  Kinds of vectors:

  own       the read's own gapped hit: pos', CIGAR, and MD/NM at md_pos (bwa_seq_t.remapped_pos)
  multi     a bwt_multi1_t hit with gap > 0 of an unmapped read: pos' and CIGAR only
  ungapped  no CIGAR: MD/NM only

md_pos is the refined position, the position before refinement (sampe's quirk) or 0 (samse's).
Left out because the reference reads uninitialised or unallocated memory there: an ungapped read at
pos >= l_pac, and a window without a base (ext > 0 at pos == l_pac).

tests/golden/refine_vectors.tsv.gz (gzip without a time stamp, like the golden .sam.gz files: the same
run writes the same bytes), one line per vector (tab separated):
  set  pos  ext  len  type  read codes (digits 0-4)  md_pos  pos'  CIGAR  MD  NM  tags
('*' where a field does not apply); tests/golden/refine_vectors.json: the seed and the counts.
"""
import ctypes as C
import gzip
import json
import os
import random
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ibwa_amd.engine import RefSeq  # noqa: E402  bwa_seq_t

REF = os.path.join(ROOT, "oracle", "_ref", "libibwa_ref.so")
GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "refine_vectors.tsv.gz")
MANIFEST = os.path.join(GOLD, "refine_vectors.json")
SEED = 20261019
LENGTHS = [1, 2, 17, 36, 100, 150, 250]
SETS = {"A": ["g1m"], "B": ["g1m", "idx_quirks"]}


class Multi(C.Structure):  # bwt_multi1_t (bwtaln.h:50-59)
    _fields_ = [("pos", C.c_uint64), ("remapped_pos", C.c_uint64), ("dbidx", C.c_uint32),
                ("remapped_dbidx", C.c_uint32), ("remapped_seqid", C.c_int32), ("remap_identical", C.c_int),
                ("n_cigar", C.c_uint32, 15), ("gap", C.c_uint32, 8), ("mm", C.c_uint32, 8), ("strand", C.c_uint32, 1),
                ("cigar", C.c_void_p)]


def unpack_pac(name):
    with open(os.path.join(GOLD, name + ".ann")) as f:
        l_pac = int(f.readline().split()[0])
    b = np.fromfile(os.path.join(GOLD, name + ".pac"), dtype=np.uint8)
    codes = np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=1).reshape(-1)[:l_pac]
    return codes, l_pac


def make_read(rng, text, start, L, events, n_sub, n_N):
    """-> (codes, reference span, gap bases); events: read position -> ('I' | 'D', k); position L: a
    deletion after the last base."""
    T = len(text)
    R, x, gaps = [], start, 0
    while len(R) < L:
        ev = events.pop(len(R), None)
        if ev and ev[0] == "I":
            k = min(ev[1], L - len(R))
            R += [rng.randrange(4) for _ in range(k)]
            gaps += k
        elif ev:
            x += ev[1]
            gaps += ev[1]
        if len(R) < L:
            R.append(int(text[x]) if 0 <= x < T else rng.randrange(4))
            x += 1
    ev = events.pop(L, None)
    if ev and ev[0] == "D":
        x += ev[1]
        gaps += ev[1]
    for _ in range(n_sub):
        y = rng.randrange(L)
        R[y] = (R[y] + rng.randrange(1, 4)) % 4 if R[y] < 4 else R[y]
    for _ in range(n_N):
        R[rng.randrange(L)] = 4
    return R, x - start, gaps


def plan(rng, sets):
    """The vectors before the reference sees them: dicts with set, pos, ext, len, type, codes, md, tags."""
    V = []

    def events_for(L, where):
        ev = {}
        n = rng.randrange(1, 4)
        for _ in range(n):
            kind = rng.choice("ID")
            k = rng.randrange(1, 7)
            if where == "lead":
                y = rng.choice([0, 1])
            elif where == "trail":
                y = rng.choice([L - 2, L - 1, L]) if kind == "D" else rng.choice([L - 2, L - 1])
            else:
                y = rng.randrange(0, L + 1)
            y = max(0, min(L, y))
            if kind == "I" and y >= L:
                y = L - 1
            ev[y] = (kind, k)
        return ev

    def add(sname, L, strand, where="any", pos_rule=None, kind="own", md="refined", tags=()):
        text = sets[sname][0]
        T = len(text)
        for _ in range(200):
            ev = events_for(L, where) if kind != "ungapped" else {}
            tg = set(tags)
            for y, (k, _) in ev.items():
                tg.add("ins" if k == "I" else "del")
            if where in ("lead", "trail") and ev:
                tg.add(where + "_indel")
            n_sub = rng.choice([0, 0, 1, 2, 5])
            n_N = rng.choice([0, 0, 0, 1, 3])
            start = rng.randrange(300, T - 600)
            R, span, gaps = make_read(rng, text, start, L, dict(ev), n_sub, n_N)
            if kind != "ungapped" and gaps == 0:
                continue
            # the hit position bwa_cal_pac_pos would give: the window's start (strand 1) or the end
            # coordinate minus the read length (strand 0)
            shift = 0 if (strand or kind == "ungapped") else span - L
            if pos_rule is not None:
                want = pos_rule(L, gaps, T)
                start = want - shift
                R, span2, gaps2 = make_read(rng, text, start, L, dict(ev), n_sub, n_N)
                if span2 != span or gaps2 != gaps:
                    continue
            pos = start + shift
            if pos < 0 or pos > T:
                continue
            if kind == "ungapped":
                if pos >= T:
                    continue
                ext = 0
            else:
                ext = gaps if strand else -gaps
                if ext > 0 and pos >= T:
                    continue
            if n_sub:
                tg.add("sub")
            if 4 in R:
                tg.add("readN")
            tg.add(f"len{L}")
            tg.add(f"strand{strand}")
            tg.add(f"res{pos % 16}")
            tg.add(kind)
            if kind != "multi":
                tg.add("md_" + md)
            V.append(dict(set=sname, pos=pos, ext=ext, len=L, type=kind, codes=R, strand=strand, md=md, tags=tg))
            return
        raise SystemExit(f"no vector for {sname} {L} {where} {kind} {tags}")

    mds = ["refined", "pre", "zero"]
    big = [17, 36, 100, 150, 250]
    # the bulk: every length, both strands and sets, every place of the indels
    for i in range(900):
        L = LENGTHS[i % 7] if i % 3 else rng.choice([1, 2, 17, 36])
        add("AB"[i % 2], L, (i // 2) % 2, where=["any", "lead", "trail"][i % 3] if L > 2 else "any", md=mds[i % 3])
    # hit positions: 0, 1..5, and every residue mod 16
    for i in range(24):
        add("AB"[i % 2], rng.choice(big), 1, pos_rule=lambda L, g, T: 0, md=mds[i % 3], tags=["pos0"])
    for i in range(30):
        add("AB"[i % 2], rng.choice(big), i % 2, pos_rule=lambda L, g, T, i=i: 1 + i % 5, md=mds[i % 3], tags=["pos1_5"])
    for i in range(16 * 8):
        add("AB"[i % 2], rng.choice(LENGTHS), (i // 16) % 2, pos_rule=lambda L, g, T, i=i: 4096 + 16 * rng.randrange(1000) + i % 16,
            md=mds[i % 3])
    # windows clamped at 0 (ext < 0 and pos < |ext|), clipped at l_pac, and pos == l_pac
    for i in range(30):
        add("AB"[i % 2], rng.choice(big), 0, pos_rule=lambda L, g, T: rng.randrange(0, g), md=mds[i % 3], tags=["clamp0"])
    for i in range(40):
        add("AB"[i % 2], rng.choice(big), 1, pos_rule=lambda L, g, T: T - rng.randrange(1, L + g), md=mds[i % 3],
            tags=["clip_lpac"])
    for i in range(30):
        add("AB"[i % 2], rng.choice([17, 36]), 0, pos_rule=lambda L, g, T: T, md=mds[i % 3], tags=["pos_eq_lpac"])
    # hits straddling the boundary of the two references of set B
    tA = len(sets["A"][0])
    for i in range(60):
        add("B", rng.choice(big), i % 2, pos_rule=lambda L, g, T: tA - rng.randrange(1, L), md=mds[i % 3], tags=["boundary"])
    # multi hits with gap > 0
    for i in range(200):
        add("AB"[i % 2], LENGTHS[i % 7], (i // 2) % 2, where=["any", "lead", "trail"][i % 3] if LENGTHS[i % 7] > 2 else "any",
            kind="multi")
    # ungapped reads, some hanging off the end (pos < l_pac < pos + len)
    for i in range(260):
        add("AB"[i % 2], LENGTHS[i % 7], (i // 2) % 2, kind="ungapped", md=["pre", "zero"][i % 2])
    for i in range(40):
        add("AB"[i % 2], rng.choice([2] + big), i % 2, kind="ungapped", pos_rule=lambda L, g, T: T - rng.randrange(1, L),
            md="pre", tags=["ungapped_hang"])
    for i in range(30):
        add("B", rng.choice(big), i % 2, kind="ungapped", pos_rule=lambda L, g, T: tA - rng.randrange(1, L), md="pre",
            tags=["boundary"])
    return V


def run_reference(L, dbs, vs, md_pos):
    """bwa_refine_gapped over one bwa_seq_t per vector -> [(pos', cigar | None, md | None, nm | None)]."""
    n = len(vs)
    seqs = (RefSeq * n)()
    keep = []
    for i, v in enumerate(vs):
        s = seqs[i]
        Lr = v["len"]
        fwd = (C.c_ubyte * Lr)(*v["codes"])
        rev = (C.c_ubyte * Lr)(*v["codes"][::-1])  # seq_reverse turns it into the codes
        keep += [fwd, rev]
        s.seq = C.cast(rev, C.c_void_p)
        s.rseq = C.cast(fwd, C.c_void_p)
        s.len = s.full_len = Lr
        s.strand = v["strand"]
        s.pos = v["pos"]
        s.remapped_pos = md_pos[i]
        if v["type"] == "multi":
            m = (Multi * 1)()
            m[0].pos = v["pos"]
            m[0].gap = abs(v["ext"])
            m[0].strand = v["strand"]
            keep.append(m)
            s.type = 0  # BWA_TYPE_NO_MATCH: only the multi hit is refined, no MD
            s.n_multi = 1
            s.multi = C.cast(m, C.c_void_p)
        else:
            s.type = 1  # BWA_TYPE_UNIQUE
            s.n_gapo = abs(v["ext"])
    L.bwa_refine_gapped(dbs, n, seqs)
    out = []
    for i, v in enumerate(vs):
        s = seqs[i]
        if v["type"] == "multi":
            m = C.cast(s.multi, C.POINTER(Multi))[0]
            cg = C.cast(m.cigar, C.POINTER(C.c_uint32))
            out.append((int(m.pos), [int(cg[k]) for k in range(m.n_cigar)], None, None))
        else:
            cig = None
            if s.cigar:
                cg = C.cast(s.cigar, C.POINTER(C.c_uint32))
                cig = [int(cg[k]) for k in range(s.n_cigar)]
            out.append((int(s.pos), cig, C.string_at(s.md).decode(), int(s.nm)))
    return out


def main():
    rng = random.Random(SEED)
    Lref = C.CDLL(REF, mode=os.RTLD_LAZY)  # its @PG printer lives in the harness executable, not needed here
    Lref.dbset_restore.restype = C.c_void_p
    Lref.dbset_restore.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int]
    Lref.bwa_refine_gapped.restype = None
    Lref.bwa_refine_gapped.argtypes = [C.c_void_p, C.c_int, C.POINTER(RefSeq)]
    sets = {}
    for name, members in SETS.items():
        parts = [unpack_pac(m) for m in members]
        assert parts[0][1] % 4 != 0, "the first reference must end inside a byte"
        sets[name] = (np.concatenate([p[0] for p in parts]), [p[1] for p in parts])
    V = plan(rng, sets)
    rows = []
    for name, members in SETS.items():
        vs = [v for v in V if v["set"] == name]
        pre = (C.c_char_p * len(members))(*[os.path.join(GOLD, m).encode() for m in members])
        dbs = Lref.dbset_restore(len(members), pre, 0x02, 0, 0)  # BWA_MODE_COMPREAD, no remap
        first = run_reference(Lref, dbs, vs, [v["pos"] for v in vs])  # pass 1: the refined positions
        md_pos = [{"refined": r[0], "pre": v["pos"], "zero": 0}[v["md"]] for v, r in zip(vs, first)]
        res = run_reference(Lref, dbs, vs, md_pos)
        for v, mp, (p1, cig, md, nm) in zip(vs, md_pos, res):
            cs = "*" if cig is None else "".join(f"{c & 0x1FFFFFFF}{'MIDS'[c >> 29]}" for c in cig)
            tg = set(v["tags"])
            if cig is not None:
                if cig[0] >> 29 == 3:
                    tg.add("S_lead")
                if cig[-1] >> 29 == 3:
                    tg.add("S_trail")
                if v["ext"] > 0 and p1 != v["pos"]:
                    tg.add("D_lead")
            if md is not None:
                runs = [int(x) for x in re.findall(r"\d+", md)]
                if max(runs) >= 10:
                    tg.add("run10")
                if max(runs) >= 100:
                    tg.add("run100")
            rows.append((name, v["pos"], v["ext"], v["len"], v["type"], "".join(map(str, v["codes"])),
                         "*" if md is None else mp, p1, cs, "*" if md is None else md, "*" if nm is None else nm,
                         ",".join(sorted(tg))))
    text = "".join("\t".join(str(x) for x in r) + "\n" for r in rows).encode()
    with open(OUT, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(text)
    counts = {}
    for r in rows:
        for t in r[-1].split(","):
            counts[t] = counts.get(t, 0) + 1
    with open(MANIFEST, "w") as f:
        json.dump({"seed": SEED, "vectors": len(rows), "sets": {k: {"references": m, "l_pac": sets[k][1]} for k, m in SETS.items()},
                   "tags": dict(sorted(counts.items()))}, f, indent=1)
        f.write("\n")
    print(len(rows), "vectors ->", OUT, os.path.getsize(OUT), "bytes,", len(text), "uncompressed")


if __name__ == "__main__":
    main()
