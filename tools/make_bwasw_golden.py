#!/usr/bin/env python3
"""Generate tests/golden/bwasw/seed_vectors.tsv.gz (build container only): known answers of the
reference's bwtl_seq2bwtl + bsw2_core on tests/golden/g1m.

TEST INFRASTRUCTURE.  The reference's sources are compiled where they lie into a temporary
directory, with a main written there by this tool: it restores the index, and per task derives t
and bw as bsw2_aln_core does, builds the read's bwtl, runs bsw2_core and prints the two hit lists
without n_seeds.  Only the tasks and the recorded results are kept.

One line per vector, tab separated:
  optset a b q r t0 bw0 z is coef adjust t bw strand kind seq hits
(t0, bw0, coef: what bsw2_aln receives; t, bw: what the core ran with; seq: digits 0-3;
hits: "n_all n_narrow" then every hit as k,l,flag,len,G,G2,beg,end).

The host restatement (ibwa_amd/csrc/bsw2_core.h through tests/host/bsw2_seed_check.cpp) classifies
every vector; the file is written only if it reproduces every vector and every class of
tests/test_bsw2_vectors.py has its count.

Two more files in the same line format, by the same harness, under the same rule:
  --long   seed_long_vectors.tsv.gz: reads of 1 023 to 8 192 bases on g1m, option sets defaults and
           z3 (conditions: check_long_classes);
  --small  seed_small_index_vectors.tsv.gz: the tasks of tests/test_bsw2_core_host.small_index_tasks
           on the small indexes idx_quirks and csg with at most 1 500 final hits, and with is == 0
           only those whose all-list the reference returned empty.  Their option-set name is
           "INDEX/is<is>t<t>z<z>": the part before the slash names the index under tests/golden.
  --all    all three.
"""
import gzip
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REFSRC = os.environ.get("IBWA_REFERENCE", "/root/reference")
GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "bwasw", "seed_vectors.tsv.gz")
REF_FILES = ("bwtsw2_core.c", "bwtsw2_aux.c", "bwtsw2_chain.c", "bwt_lite.c", "bwt.c", "bwtio.c", "is.c", "utils.c",
             "stdaln.c", "bntseq.c", "kstring.c")

HARNESS = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bwt.h"
#include "bwt_lite.h"
#include "bwtsw2.h"
static char line[1 << 16], seq[1 << 16];
int main(int argc, char **argv)
{
	char fn[4096];
	bwt_t *idx[2];
	bsw2global_t *pool = bsw2_global_init();
	FILE *in = fopen(argv[2], "r");
	sprintf(fn, "%s.bwt", argv[1]); idx[0] = bwt_restore_bwt(fn);
	sprintf(fn, "%s.sa", argv[1]); bwt_restore_sa(fn, idx[0]);
	sprintf(fn, "%s.rbwt", argv[1]); idx[1] = bwt_restore_bwt(fn);
	sprintf(fn, "%s.rsa", argv[1]); bwt_restore_sa(fn, idx[1]);
	while (fgets(line, sizeof line, in)) {
		bsw2opt_t *o = bsw2_init_opt();
		int adjust, strand, l, i, k, x;
		bwtl_t *q;
		bwtsw2_t **bb;
		if (sscanf(line, "%d %d %d %d %d %d %d %d %f %d %d %s", &o->a, &o->b, &o->q, &o->r, &o->t, &o->bw, &o->z,
				&o->is, &o->coef, &adjust, &strand, seq) != 12) return 3;
		o->qr = o->q + o->r;
		l = strlen(seq);
		for (i = 0; i < l; ++i) seq[i] -= '0';
		if (adjust) { /* what bsw2_aln_core does with the read's length */
			int bw0 = o->bw;
			if (o->t < log(l) * o->coef) o->t = (int)(log(l) * o->coef + .499);
			k = (l * o->a - 2 * o->q) / (2 * o->r + o->a);
			i = (l * o->a - o->a - o->t) / o->r;
			if (k > i) k = i;
			if (k < 1) k = 1;
			o->bw = bw0 < k? bw0 : k;
		}
		q = bwtl_seq2bwtl(l, (uint8_t*)seq);
		bb = bsw2_core(o, q, idx[strand], pool);
		printf("%d %d\t%d %d", o->t, o->bw, bb[0]->n, bb[1]->n);
		for (x = 0; x < 2; ++x)
			for (i = 0; i < bb[x]->n; ++i) {
				bsw2hit_t *p = bb[x]->hits + i;
				printf(" %u,%u,%u,%d,%d,%d,%d,%d", p->k, p->l, (unsigned)p->flag, p->len, p->G, p->G2, p->beg, p->end);
			}
		printf("\n");
		bwtl_destroy(q); bsw2_destroy(bb[0]); bsw2_destroy(bb[1]); free(bb); free(o);
	}
	return 0;
}
"""

# name -> a b q r t bw z is coef adjust, as bsw2_aln receives them (t and coef scaled by a)
OPTSETS = {
    "defaults": (1, 3, 5, 2, 30, 50, 1, 3, 5.5, 1),
    "z3": (1, 3, 5, 2, 30, 50, 3, 3, 5.5, 1),
    "b5q2r1z10": (1, 5, 2, 1, 30, 50, 10, 3, 5.5, 1),
    "s1": (1, 3, 5, 2, 30, 50, 1, 1, 5.5, 1),
    "s10": (1, 3, 5, 2, 30, 50, 1, 10, 5.5, 1),
    "a2": (2, 3, 5, 2, 60, 50, 1, 3, 11.0, 1),
    "w5": (1, 3, 5, 2, 30, 5, 1, 3, 5.5, 1),
    "T10": (1, 3, 5, 2, 10, 50, 1, 3, 5.5, 1),
    "fixed": (1, 3, 5, 2, 12, 3, 1, 3, 5.5, 0),
}
KINDS = ("exact", "sub2", "sub5", "sub10", "sub2indel", "sub5indel", "sub10indel", "longdel", "chimera", "random",
         "polyA", "ACAC", "period3")


def load_genome(name="g1m"):
    with open(os.path.join(GOLD, name + ".pac"), "rb") as f:
        pac = f.read()
    with open(os.path.join(GOLD, name + ".ann")) as f:
        n = int(f.readline().split()[0])  # l_pac
    return [pac[i >> 2] >> ((~i & 3) << 1) & 3 for i in range(n)]


def make_read(rng, g, kind, ln):
    def locus(n):
        a = rng.randrange(0, len(g) - n - 200)
        return g[a:a + n]

    def mutate(s, sub, indel):
        out = []
        for c in s:
            r = rng.random()
            if r < sub:
                out.append((c + rng.randrange(1, 4)) & 3)
            elif indel and r < sub + 0.004:
                continue
            elif indel and r < sub + 0.008:
                out.append(c)
                out.extend(rng.randrange(4) for _ in range(rng.randrange(1, 6)))
            else:
                out.append(c)
        if indel and len(s) > 40:  # at least one 1-5 bp deletion
            p = rng.randrange(10, len(out) - 10)
            del out[p:p + rng.randrange(1, 6)]
        return out

    if kind == "exact":
        s = locus(ln)
    elif kind.startswith("sub"):
        rate = int(kind[3:].replace("indel", "")) / 100.0
        s = mutate(locus(ln + 12), rate, kind.endswith("indel"))
    elif kind == "longdel":
        w = locus(ln + 80)
        s = w[:ln // 2] + w[ln // 2 + 70:]
    elif kind == "chimera":
        s = locus(ln // 2) + locus(ln - ln // 2)
    elif kind == "random":
        s = [rng.randrange(4) for _ in range(ln)]
    elif kind == "polyA":
        s = [0] * ln
    elif kind == "ACAC":
        s = [i & 1 for i in range(ln)]
    elif kind == "period3":
        s = [(i % 3 + (rng.randrange(1, 4) if rng.random() < 0.03 else 0)) & 3 for i in range(ln)]
    else:
        raise ValueError(kind)
    s = (s + locus(ln))[:ln] if len(s) < ln else s[:ln]
    return s


def make_tasks(g):
    rng = random.Random(20261020)
    tasks = []  # (optset, strand, kind, seq)

    def add(optset, strand, kind, ln):
        s = make_read(rng, g, kind, ln)
        tasks.append((optset, strand, kind, s[::-1] if strand else s))

    for ln in (1, 2, 8, 16, 17, 30, 32, 33, 64, 100, 150, 400, 1000):
        for kind in ("exact", "sub2", "sub5indel"):
            add("defaults", 0, kind, ln)
    for ln in (150, 400):
        for kind in ("exact", "sub2", "sub5indel", "chimera"):
            add("defaults", 1, kind, ln)
    for optset in OPTSETS:
        for kind in KINDS:
            add(optset, 0, kind, 150)
            add(optset, 0, kind, 100)
        for kind in ("sub5", "sub10indel", "longdel", "chimera", "period3"):
            add(optset, 0, kind, 400)
        for kind in ("sub2", "sub10indel"):
            add(optset, 1, kind, 150)
    for optset in ("defaults", "z3", "b5q2r1z10"):
        for kind in ("sub5", "sub10indel", "chimera"):
            add(optset, 0, kind, 1000)
    # long low-complexity reads and z = 10: the cell arrays that pass 256
    for optset in ("defaults", "z3", "b5q2r1z10", "s10", "T10"):
        for kind in ("polyA", "ACAC", "period3"):
            add(optset, 0, kind, 400)
    for kind in ("sub2", "sub5indel", "sub10", "longdel", "period3"):
        add("b5q2r1z10", 0, kind, 1000)
    for ln in (100, 150, 150, 400, 400, 400):
        add("b5q2r1z10", 0, "period3", ln)
        add("b5q2r1z10", 1, "period3", ln)
    add("b5q2r1z10", 1, "sub5indel", 400)
    for optset in OPTSETS:
        for kind in ("sub2indel", "sub10", "longdel", "chimera", "random"):
            add(optset, 0, kind, 64)
    # short reads under the low thresholds, where ties and displaced slots are common
    for optset in ("T10", "fixed", "b5q2r1z10", "z3"):
        for ln in (17, 30, 33, 64):
            for kind in ("exact", "sub5", "sub10indel", "period3", "ACAC"):
                add(optset, 0, kind, ln)
    return tasks


def build(tmp):
    with open(os.path.join(tmp, "main.c"), "w") as f:
        f.write(HARNESS)
    ref = os.path.join(tmp, "ref_seed")
    subprocess.run(["gcc", "-O2", "-fgnu89-inline", "-w", "-I", REFSRC, "-o", ref, os.path.join(tmp, "main.c")] +
                   [os.path.join(REFSRC, x) for x in REF_FILES] + ["-lz", "-lm"], check=True)
    chk = os.path.join(tmp, "bsw2_seed_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "ibwa_amd", "csrc"), "-o", chk,
                    os.path.join(ROOT, "tests", "host", "bsw2_seed_check.cpp")], check=True)
    return ref, chk


LONG_LENGTHS = (1023, 1024, 2047, 2048, 2049, 4095, 4096, 8191, 8192)
LONG_KINDS = ("sub2", "sub10", "chimera", "random", "period3", "polyA", "ACAC", "period3exact")


def make_long_tasks(g):
    """Every length x kind x option set on .bwt and one row per length on .rbwt: the size limit does
    not bind (about 175 KB), so nothing is thinned."""
    rng = random.Random(20261021)
    tasks = []
    for ln in LONG_LENGTHS:
        for kind in LONG_KINDS:
            for optset in ("defaults", "z3"):
                s = [i % 3 for i in range(ln)] if kind == "period3exact" else make_read(rng, g, kind, ln)
                tasks.append((optset, 0, kind, s))
        k = LONG_LENGTHS.index(ln)
        kind = ("sub2", "chimera", "period3")[k % 3]
        tasks.append((("defaults", "z3")[k & 1], 1, kind, make_read(rng, g, kind, ln)[::-1]))
    return tasks


def reference_lines(ref, tmp, index, tasks, optsets):
    """The vector lines of tasks [(optset, strand, kind, codes)] on tests/golden/<index>."""
    tf = os.path.join(tmp, "tasks.txt")
    with open(tf, "w") as f:
        for optset, strand, _kind, s in tasks:
            a, b, q, r, t, bw, z, is_, coef, adjust = optsets[optset]
            f.write(f"{a} {b} {q} {r} {t} {bw} {z} {is_} {coef} {adjust} {strand} {''.join(map(str, s))}\n")
    out = subprocess.run([ref, os.path.join(GOLD, index), tf], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    assert len(out) == len(tasks), (len(out), len(tasks))
    lines = []
    for (optset, strand, kind, s), o in zip(tasks, out):
        tbw, hits = o.split("\t")
        t, bw = tbw.split()
        a, b, q, r, t0, bw0, z, is_, coef, adjust = optsets[optset]
        lines.append("\t".join(map(str, (optset, a, b, q, r, t0, bw0, z, is_, coef, adjust, t, bw, strand, kind,
                                         "".join(map(str, s)), hits))))
    return lines


SMALL_PER_INDEX = 150  # the first so many tasks that qualify: the size limit of the file


def small_index_lines(ref, tmp):
    from tests.test_bsw2_core_host import SMALL_INDEXES, small_index_tasks
    lines = []
    for index in SMALL_INDEXES:
        optsets, tasks = {}, []
        for a, b, q, r, t, bw, z, is_, strand, s in small_index_tasks(index):
            name = f"{index}/is{is_}t{t}z{z}"
            optsets[name] = (a, b, q, r, t, bw, z, is_, 5.5, 0)
            kind = "homopolymer" if len(set(s)) == 1 else "other"
            tasks.append((name, strand, kind, s))
        kept = 0
        for line in reference_lines(ref, tmp, index, tasks, optsets):
            c = line.split("\t")
            n_all, n_narrow = map(int, c[16].split()[:2])
            if n_all + n_narrow <= 1500 and (int(c[8]) != 0 or n_all == 0) and kept < SMALL_PER_INDEX:
                lines.append(line)
                kept += 1
    return lines


def write_vectors(chk, tmp, out, lines, check):
    """Write out only if the host restatement reproduces every line and check finds no class short."""
    from tests.test_bsw2_vectors import parse_classes
    text = "\n".join(lines) + "\n"
    plain = os.path.join(tmp, "vectors.tsv")
    with open(plain, "w") as f:
        f.write(text)
    r = subprocess.run([chk, "vectors", os.path.join(GOLD, "g1m"), plain], stdout=subprocess.PIPE, text=True)
    print(r.stdout)
    if r.returncode != 0:
        sys.exit("the host restatement does not reproduce the vectors: nothing written")
    problems = check(parse_classes(r.stdout))
    if problems:
        sys.exit("classes short of their counts, nothing written:\n  " + "\n  ".join(problems))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", filename="", mtime=0, compresslevel=9) as z:
        z.write(text.encode())
    size = os.path.getsize(out)
    print(f"{out}: {len(lines)} vectors, {size} bytes")
    if size > 256 * 1024:
        os.remove(out)
        sys.exit("the file is above 256 KB: removed")


def main():
    from tests.test_bsw2_vectors import LONG_VECTORS, SMALL_VECTORS, check_classes, check_long_classes, check_small_classes
    flags = set(sys.argv[1:])
    if flags - {"--long", "--small", "--all"}:
        sys.exit("usage: make_bwasw_golden.py [--long] [--small] [--all]")
    with tempfile.TemporaryDirectory() as tmp:
        ref, chk = build(tmp)
        if not flags or "--all" in flags:
            write_vectors(chk, tmp, OUT, reference_lines(ref, tmp, "g1m", make_tasks(load_genome()), OPTSETS), check_classes)
        if flags & {"--long", "--all"}:
            write_vectors(chk, tmp, LONG_VECTORS, reference_lines(ref, tmp, "g1m", make_long_tasks(load_genome()), OPTSETS),
                          check_long_classes)
        if flags & {"--small", "--all"}:
            write_vectors(chk, tmp, SMALL_VECTORS, small_index_lines(ref, tmp), check_small_classes)


if __name__ == "__main__":
    main()
