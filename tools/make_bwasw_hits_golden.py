#!/usr/bin/env python3
"""Generate tests/golden/bwasw/aln1_vectors.tsv.gz and left_vectors.tsv.gz (build container only): known
answers of the reference's bsw2_aln1_core and bsw2_extend_left on tests/golden/g1m.

TEST INFRASTRUCTURE.  The reference's sources are compiled where they lie into a temporary directory,
with a main written there by this tool, which includes bwtsw2_aux.c to reach its static functions.
Per read it derives t and bw as bsw2_aln_core does, calls bsw2_aln1_core after srand48(s), then makes
the same calls itself to print the lists in between, and stops unless its own final list equals
bsw2_aln1_core's.  Only the tasks and the recorded results are kept.

aln1_vectors.tsv.gz, one line per read, tab separated:
  optset a b q r t0 bw0 z is coef adjust t_seeds mask_level t bw is_rev kind s seq final left0 left1
(t0, bw0: what bsw2_aln receives; t, bw: what the core ran with; s: the seed of srand48, the draw of a
test is the first drand48() after it; seq: digits 0-3, reversed for is_rev; final: the list
bsw2_aln1_core returned; left0 / left1: the narrow lists right after bsw2_extend_left.  A list is
"n hit..." with hit = k,l,flag,n_seeds,len,G,G2,beg,end.)

left_vectors.tsv.gz, one line per list:
  a b q r bw is_rev kind seq hits_in hits_out
(the reference's bsw2_extend_left on hits_in with the query seq: lists taken after the chain filter of
real reads, and synthetic ones for the classes whole reads do not reach on g1m.)

The host restatement (ibwa_amd/csrc/bsw2_aln1.h through tests/host/bsw2_aln1_check.cpp) classifies
every line; a file is written only if it reproduces every line and every class of
tests/test_bsw2_aln1_vectors.py has its count over the two files.
"""
import gzip
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.make_bwasw_golden import GOLD, KINDS, OPTSETS, REFSRC, load_genome, make_read  # noqa: E402

OUT_ALN1 = os.path.join(GOLD, "bwasw", "aln1_vectors.tsv.gz")
OUT_LEFT = os.path.join(GOLD, "bwasw", "left_vectors.tsv.gz")
REF_FILES = ("bwtsw2_core.c", "bwtsw2_chain.c", "bwt_lite.c", "bwt.c", "bwtio.c", "is.c", "utils.c", "stdaln.c", "bntseq.c",
             "kstring.c")

HARNESS = r"""
#include <math.h>
#include "bwtsw2_aux.c"
#include "bwt_lite.h"

static void put(const bwtsw2_t *b, int unset)
{
	int i;
	printf("\t%d", b->n);
	for (i = 0; i < b->n; ++i) {
		const bsw2hit_t *p = b->hits + i;
		printf(" %u,%u,%u,%u,%d,%d,%d,%d,%d", p->k, p->l, (unsigned)p->flag, unset? 0 : (unsigned)p->n_seeds, p->len, p->G,
			p->G2, p->beg, p->end);
	}
}
static int same(const bwtsw2_t *x, const bwtsw2_t *y)
{
	int i;
	if (x->n != y->n) return 0;
	for (i = 0; i < x->n; ++i) {
		const bsw2hit_t *p = x->hits + i, *q = y->hits + i;
		if (p->k != q->k || p->l != q->l || p->flag != q->flag || p->n_seeds != q->n_seeds || p->len != q->len || p->G != q->G
			|| p->G2 != q->G2 || p->beg != q->beg || p->end != q->end) return 0;
	}
	return 1;
}
static bwtsw2_t *get(char *s)
{
	bwtsw2_t *b = calloc(1, sizeof(bwtsw2_t));
	int i;
	b->n = b->max = strtol(s, &s, 10);
	b->hits = calloc(b->n + 1, sizeof(bsw2hit_t));
	for (i = 0; i < b->n; ++i) {
		bsw2hit_t *p = b->hits + i;
		unsigned flag, ns;
		int used;
		if (sscanf(s, " %u,%u,%u,%u,%d,%d,%d,%d,%d%n", &p->k, &p->l, &flag, &ns, &p->len, &p->G, &p->G2, &p->beg, &p->end, &used) != 9) exit(4);
		p->flag = flag; p->n_seeds = ns;
		s += used;
	}
	return b;
}
int main(int argc, char **argv)
{
	extern void bsw2_chain_filter(const bsw2opt_t *opt, int len, bwtsw2_t *b[2]);
	char fn[4096], *line = 0;
	size_t cap = 0;
	bwt_t *idx[2];
	bsw2global_t *pool = bsw2_global_init();
	bntseq_t *bns = bns_restore(argv[2]);
	uint8_t *pac = calloc(bns->l_pac / 4 + 1, 1);
	FILE *in = fopen(argv[3], "r");
	fread(pac, 1, bns->l_pac / 4 + 1, bns->fp_pac);
	pool->aln_mem = calloc(1 << 20, 24);
	pool->max_l = 1 << 19;
	if (strcmp(argv[1], "left") == 0) {
		while (getline(&line, &cap, in) > 0) {
			bsw2opt_t *o = bsw2_init_opt();
			int is_rev, l, i, n = 0;
			char *seq = malloc(strlen(line) + 1), *h;
			bwtsw2_t *b;
			if (sscanf(line, "%d %d %d %d %d %d %s%n", &o->a, &o->b, &o->q, &o->r, &o->bw, &is_rev, seq, &n) != 7) return 3;
			h = line + n;
			l = strlen(seq);
			for (i = 0; i < l; ++i) seq[i] -= '0';
			b = get(h);
			bsw2_extend_left(o, b, (uint8_t*)seq, l, pac, bns->l_pac, is_rev, calloc((size_t)l * 3 + 64, 24));
			printf("-"); put(b, 0); printf("\n");
		}
		return 0;
	}
	sprintf(fn, "%s.bwt", argv[2]); idx[0] = bwt_restore_bwt(fn);
	sprintf(fn, "%s.sa", argv[2]); bwt_restore_sa(fn, idx[0]);
	sprintf(fn, "%s.rbwt", argv[2]); idx[1] = bwt_restore_bwt(fn);
	sprintf(fn, "%s.rsa", argv[2]); bwt_restore_sa(fn, idx[1]);
	while (getline(&line, &cap, in) > 0) {
		bsw2opt_t *o = bsw2_init_opt();
		int adjust, is_rev, l, i, k;
		long s;
		char *str = malloc(strlen(line) + 1);
		uint8_t *seq[2];
		bwtsw2_t *want, *b[2], **bb[2];
		if (sscanf(line, "%d %d %d %d %d %d %d %d %f %d %d %f %d %ld %s", &o->a, &o->b, &o->q, &o->r, &o->t, &o->bw, &o->z,
				&o->is, &o->coef, &adjust, &o->t_seeds, &o->mask_level, &is_rev, &s, str) != 15) return 3;
		o->qr = o->q + o->r;
		l = strlen(str);
		seq[0] = calloc(2 * l, 1); seq[1] = seq[0] + l;
		for (i = 0; i < l; ++i) { seq[0][i] = str[i] - '0'; seq[1][l-1-i] = 3 - seq[0][i]; }
		if (adjust) { /* what bsw2_aln_core does with the read's length */
			int bw0 = o->bw;
			if (o->t < log(l) * o->coef) o->t = (int)(log(l) * o->coef + .499);
			k = (l * o->a - 2 * o->q) / (2 * o->r + o->a);
			i = (l * o->a - o->a - o->t) / o->r;
			if (k > i) k = i;
			if (k < 1) k = 1;
			o->bw = bw0 < k? bw0 : k;
		}
		srand48(s);
		want = bsw2_aln1_core(o, bns, pac, idx[is_rev], l, seq, is_rev, pool);
		printf("%d %d", o->t, o->bw);
		/* the same calls, with the lists printed in between */
		for (k = 0; k < 2; ++k) {
			bwtl_t *query = bwtl_seq2bwtl(l, seq[k]);
			bb[k] = bsw2_core(o, query, idx[is_rev], pool);
			bwtl_destroy(query);
		}
		b[0] = bb[0][1]; b[1] = bb[1][1];
		bsw2_chain_filter(o, l, b);
		put(b[0], 1); put(b[1], 1);
		for (k = 0; k < 2; ++k) bsw2_extend_left(o, bb[k][1], seq[k], l, pac, bns->l_pac, is_rev, pool->aln_mem);
		put(b[0], 0); put(b[1], 0);
		for (k = 0; k < 2; ++k) {
			merge_hits(bb[k], l, 0);
			bsw2_resolve_duphits(0, bb[k][0], 0);
			bsw2_extend_rght(o, bb[k][0], seq[k], l, pac, bns->l_pac, is_rev, pool->aln_mem);
			b[k] = bb[k][0];
		}
		put(b[0], 0); put(b[1], 0);
		merge_hits(b, l, 1);
		srand48(s);
		bsw2_resolve_query_overlaps(b[0], o->mask_level);
		put(b[0], 0);
		printf("\n");
		if (!same(want, b[0])) { fprintf(stderr, "the harness's own calls differ from bsw2_aln1_core\n"); return 5; }
		fflush(stdout);
	}
	return 0;
}
"""

# the option sets of make_bwasw_golden.py with bwasw's t_seeds and mask_level, and two that move those
ALN_OPTSETS = {k: v + (5, 0.5) for k, v in OPTSETS.items()}
ALN_OPTSETS["ts1"] = OPTSETS["defaults"] + (1, 0.5)
ALN_OPTSETS["m90"] = OPTSETS["defaults"] + (5, 0.9)


def build(tmp):
    with open(os.path.join(tmp, "main.c"), "w") as f:
        f.write(HARNESS)
    ref = os.path.join(tmp, "ref_aln1")
    subprocess.run(["gcc", "-O2", "-fgnu89-inline", "-w", "-I", REFSRC, "-o", ref, os.path.join(tmp, "main.c")] +
                   [os.path.join(REFSRC, x) for x in REF_FILES] + ["-lz", "-lm"], check=True)
    chk = os.path.join(tmp, "bsw2_aln1_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "ibwa_amd", "csrc"), "-o", chk,
                    os.path.join(ROOT, "tests", "host", "bsw2_aln1_check.cpp")], check=True)
    return ref, chk


def task_line(optset, is_rev, s, seq):
    a, b, q, r, t, bw, z, is_, coef, adjust, t_seeds, mask = ALN_OPTSETS[optset]
    return f"{a} {b} {q} {r} {t} {bw} {z} {is_} {coef} {adjust} {t_seeds} {mask} {is_rev} {s} {''.join(map(str, seq))}"


def make_tasks(g):
    """[(optset, is_rev, kind, s, codes)]"""
    rng = random.Random(20261021)
    tasks = []

    def add(optset, is_rev, kind, seq):
        tasks.append((optset, is_rev, kind, rng.randrange(1, 1 << 20), seq[::-1] if is_rev else seq))

    for ln in (17, 30, 33, 64, 100, 150, 400):
        for kind in ("exact", "sub2", "sub5indel", "chimera", "random"):
            add("defaults", 0, kind, make_read(rng, g, kind, ln))
            add("defaults", 1, kind, make_read(rng, g, kind, ln))
    for optset in ALN_OPTSETS:
        for kind in KINDS:
            add(optset, 0, kind, make_read(rng, g, kind, 150))
        for kind in ("sub5", "sub10indel", "longdel", "chimera"):
            add(optset, 1, kind, make_read(rng, g, kind, 100))
    for optset in ("defaults", "z3", "ts1"):
        for kind in ("sub5", "sub10indel", "chimera", "longdel"):
            add(optset, 0, kind, make_read(rng, g, kind, 1000))
            add(optset, 1, kind, make_read(rng, g, kind, 400))
    add("defaults", 0, "sub5indel", make_read(rng, g, "sub5indel", 2049))
    add("defaults", 1, "sub2", make_read(rng, g, "sub2", 8192))
    # a locus twice in one read: ties at the top G
    for k in range(24):
        ln = rng.choice((40, 60, 100))
        a0 = rng.randrange(1000, len(g) - 1000)
        unit = g[a0:a0 + ln]
        gap = [rng.randrange(4) for _ in range(rng.choice((0, 5, 30)))]
        add(("defaults", "m90", "ts1", "z3")[k & 3], k & 1, "twice", unit + gap + unit)
    # reads cut at bases 0, 1, 2 of the genome and ending at its last base
    n = len(g)
    for k in range(8):
        ln = (40, 100, 150, 400)[k & 3]
        for a0 in (0, 1, 2):
            add("defaults", k & 1, f"cut{a0}", g[a0:a0 + ln])
        add("defaults", k & 1, "cutend", g[n - ln:])
        w = g[n - ln - 20:]  # a deletion near the end: the right window runs into l_pac
        add("defaults", k & 1, "cutend", w[:ln // 2] + w[ln // 2 + 3:])
    # period-3 and low-complexity reads under low thresholds: many narrow hits, chains that flag others
    for optset in ("T10", "b5q2r1z10", "s10", "z3"):
        for ln in (100, 150, 400):
            for kind in ("period3", "ACAC", "sub10indel"):
                add(optset, 0, kind, make_read(rng, g, kind, ln))
                add(optset, 1, kind, make_read(rng, g, kind, ln))
    return tasks


def run_ref(ref, tmp, mode, lines):
    tf = os.path.join(tmp, "tasks.txt")
    with open(tf, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([ref, mode, os.path.join(GOLD, "g1m"), tf], check=True, stdout=subprocess.PIPE, text=True).stdout
    out = out.splitlines()
    assert len(out) == len(lines), (len(out), len(lines))
    return out


def aln1_lines(ref, tmp, tasks):
    """-> (the vector lines, the left tasks (a, b, q, r, bw, is_rev, kind, strand's query, list after the chain filter))"""
    out = run_ref(ref, tmp, "stages", [task_line(o, r, s, seq) for o, r, _k, s, seq in tasks])
    lines, lefts = [], []
    for (optset, is_rev, kind, s, seq), o in zip(tasks, out):
        f = o.split("\t")
        t, bw = f[0].split()
        a, b, q, r, t0, bw0, z, is_, coef, adjust, t_seeds, mask = ALN_OPTSETS[optset]
        text = "".join(map(str, seq))
        lines.append("\t".join(map(str, (optset, a, b, q, r, t0, bw0, z, is_, coef, adjust, t_seeds, mask, t, bw, is_rev, kind, s,
                                         text, f[7], f[3], f[4]))))
        rc = "".join(str(3 - c) for c in reversed(seq))
        for k, query in ((0, text), (1, rc)):
            lefts.append((a, b, q, r, int(bw), is_rev, kind, query, f[1 + k]))
    return lines, lefts


def hit(k, ln, G, beg, end, l=0):
    return f"{k},{l},0,0,{ln},{G},0,{beg},{end}"


def synthetic_lefts(g):
    """Lists that whole reads do not produce on g1m: exact sizes around the window of 64, containers in
    the same and in an earlier window, containment that holds only after the container was extended,
    k == 0, windows clipped by k, empty queries, equal ends, n_seeds above 64."""
    rng = random.Random(20261022)
    out = []
    n = len(g)

    def read_at(a0, ln):
        return g[a0:a0 + ln]

    def add(kind, is_rev, query, hits, bw=50):
        out.append((1, 3, 5, 2, bw, is_rev, kind, "".join(map(str, query)), f"{len(hits)} " + " ".join(hits)))

    def coords(a0, is_rev, ln):
        # a read that matches g[a0, a0 + ln) forwards; on the reversed sequence it is the reversed read at n - a0 - ln
        return (read_at(a0, ln)[::-1], n - a0 - ln) if is_rev else (read_at(a0, ln), a0)

    for size in (0, 1, 64, 65, 129, 200):
        for rep in range(5):
            is_rev = rep & 1
            ln = 400
            a0 = rng.randrange(5000, n - 5000)
            q, t0 = coords(a0, is_rev, ln)
            hits = []
            for i in range(size):
                # seeds of 20 to 40 bases on the diagonal; every third one a sub-seed of its predecessor
                b0 = rng.randrange(0, ln - 45)
                sl = rng.randrange(20, 41)
                if i % 3 == 2 and hits:
                    pk, _, _, _, pl, pG, _, pb, pe = map(int, hits[-1].split(","))
                    hits.append(hit(pk + 2, pl - 4, pG - 4, pb + 2, pe - 2))
                else:
                    hits.append(hit(t0 + b0, sl, sl, b0, b0 + sl))
            add(f"size{size}", is_rev, q, hits)
    for rep in range(6):  # one long seed at the read's end, then many inside it: n_seeds above 64, containers far back
        is_rev = rep & 1
        ln = 300
        a0 = rng.randrange(5000, n - 5000)
        q, t0 = coords(a0, is_rev, ln)
        hits = [hit(t0 + 100, 200, 200, 100, 300)]
        for i in range(70 + 30 * rep):
            b0 = rng.randrange(100, 260)
            sl = rng.randrange(20, 300 - b0 - 1)
            hits.append(hit(t0 + b0, sl, sl, b0, b0 + sl))
        add("nested", is_rev, q, hits)
    for rep in range(6):  # contained only once the container has been extended to the left
        is_rev = rep & 1
        ln = 200
        a0 = rng.randrange(5000, n - 5000)
        q, t0 = coords(a0, is_rev, ln)
        hits = [hit(t0 + 120, 60, 60, 120, 180), hit(t0 + 40, 30, 30, 40, 70), hit(t0 + 90, 25, 25, 90, 115)]
        add("ext_only", is_rev, q, hits)
    for rep in range(6):  # seeds at the very start of the sequence: k == 0, k == 1, windows clipped by k
        is_rev = rep & 1
        ln = 120
        if is_rev:
            q, t0 = read_at(n - ln, ln)[::-1], 0
        else:
            q, t0 = read_at(0, ln), 0
        hits = [hit(t0 + 60, 40, 40, 60, 100), hit(t0, 30, 30, 0, 30), hit(t0 + 1, 20, 20, 1, 21), hit(t0 + 5, 20, 20, 5 + rep, 25 + rep),
                hit(t0 + 30, 20, 20, 30, 50), hit(t0 + 31, 20, 20, 31, 50)]
        add("start", is_rev, q, hits)
    for rep in range(6):  # beg == 0: an empty query, nothing to extend; equal ends
        is_rev = rep & 1
        ln = 150
        a0 = rng.randrange(5000, n - 5000)
        q, t0 = coords(a0, is_rev, ln)
        hits = [hit(t0, 50, 50, 0, 50), hit(rng.randrange(1000, n - 1000), 50, 45, 0, 50), hit(t0 + 70, 30, 30, 70, 100),
                hit(t0 + 75, 25, 25, 75, 100), hit(rng.randrange(1000, n - 1000), 30, 28, 70, 100)]
        add("beg0", is_rev, q, hits)
    return out


def left_lines(ref, tmp, lefts):
    out = run_ref(ref, tmp, "left", [f"{a} {b} {q} {r} {bw} {is_rev} {query} {hits}" for a, b, q, r, bw, is_rev, _k, query, hits in lefts])
    lines = []
    for (a, b, q, r, bw, is_rev, kind, query, hits), o in zip(lefts, out):
        lines.append("\t".join(map(str, (a, b, q, r, bw, is_rev, kind, query, hits, o.split("\t")[1]))))
    return lines


def check_file(chk, tmp, mode, lines):
    from tests.test_bsw2_aln1_vectors import parse_classes
    plain = os.path.join(tmp, mode + ".tsv")
    with open(plain, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([chk, mode, os.path.join(GOLD, "g1m"), plain], stdout=subprocess.PIPE, text=True)
    print(r.stdout)
    if r.returncode != 0:
        sys.exit(f"the host restatement does not reproduce the {mode}: nothing written")
    return parse_classes(r.stdout)


def write(out, lines):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", filename="", mtime=0, compresslevel=9) as z:
        z.write(("\n".join(lines) + "\n").encode())
    size = os.path.getsize(out)
    print(f"{out}: {len(lines)} vectors, {size} bytes")
    if size > 256 * 1024:
        os.remove(out)
        sys.exit("the file is above 256 KB: removed")


def main():
    from tests.test_bsw2_aln1_vectors import check_classes
    g = load_genome()
    with tempfile.TemporaryDirectory() as tmp:
        ref, chk = build(tmp)
        aln1, real_lefts = aln1_lines(ref, tmp, make_tasks(g))
        # of the real lists keep those of the shorter reads with at least two hits: the size limit
        real_lefts = [x for x in real_lefts if len(x[7]) <= 400 and int(x[8].split()[0]) >= 2][:150]
        left = left_lines(ref, tmp, real_lefts + synthetic_lefts(g))
        problems = check_classes(check_file(chk, tmp, "vectors", aln1), check_file(chk, tmp, "leftvectors", left))
        if problems:
            sys.exit("classes short of their counts, nothing written:\n  " + "\n  ".join(problems))
        write(OUT_ALN1, aln1)
        write(OUT_LEFT, left)


if __name__ == "__main__":
    main()
