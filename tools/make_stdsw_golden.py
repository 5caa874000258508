#!/usr/bin/env python3
"""Generate tests/golden/stdsw/ (build container only): known answers of the reference's `stdsw`
command and of its aln_stdaln_aux.

TEST INFRASTRUCTURE.  Two parts:

* CLI cases.  The reference's simple_dp.c, stdaln.c and utils.c are compiled where they lie into a
  temporary directory, with a two-line main written there, and the binary is run on inputs this
  tool generates.  Only the inputs and the recorded stdout / stderr / exit status are kept
  (tests/golden/stdsw/*.fa, *.gz, NAME.out, NAME.err; cases.json: per case its arguments, files and
  exit status).
* Library vectors (stdaln_vectors.tsv.gz): score, subo, path length, ends and CIGAR of aln_stdaln_aux in
  oracle/_ref/libibwa_ref.so (through ctypes) for the blast and aa2aa presets, local and global, over
  a grid of lengths, plus the suboptimal-score, tie and threshold cases.

Nucleotide long sequences are slices of the project's seeded synthetic genome; everything else comes
from random.Random with fixed seeds.
"""
import ctypes
import gzip
import io
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REFSRC = os.environ.get("IBWA_REFERENCE", "/root/reference")
REFLIB = os.path.join(ROOT, "oracle", "_ref", "libibwa_ref.so")
OUT = os.path.join(ROOT, "tests", "golden", "stdsw")
AA = "ARNDCQEGHILKMFPSTWYV"
COMP = str.maketrans("ACGTacgt", "TGCAtgca")


class AlnParam(ctypes.Structure):
    _fields_ = [("gap_open", ctypes.c_int), ("gap_ext", ctypes.c_int), ("gap_end", ctypes.c_int),
                ("matrix", ctypes.POINTER(ctypes.c_int)), ("row", ctypes.c_int), ("band_width", ctypes.c_int)]


class AlnAln(ctypes.Structure):
    _fields_ = [("path", ctypes.c_void_p), ("path_len", ctypes.c_int), ("start1", ctypes.c_int), ("end1", ctypes.c_int),
                ("start2", ctypes.c_int), ("end2", ctypes.c_int), ("score", ctypes.c_int), ("subo", ctypes.c_int),
                ("out1", ctypes.c_void_p), ("out2", ctypes.c_void_p), ("outm", ctypes.c_void_p),
                ("n_cigar", ctypes.c_int), ("cigar32", ctypes.POINTER(ctypes.c_uint32))]


def mutate(rng, s, alphabet, sub=0.04, indel=0.01):
    out = []
    for ch in s:
        r = rng.random()
        if r < sub:
            out.append(rng.choice(alphabet))
        elif r < sub + indel:
            continue
        elif r < sub + 2 * indel:
            out.append(ch + rng.choice(alphabet))
        else:
            out.append(ch)
    return "".join(out)


def fasta(path, recs, width=0):
    with open(path, "w") as f:
        for name, s in recs:
            f.write(f">{name}\n")
            if width:
                for k in range(0, len(s), width):
                    f.write(s[k:k + width] + "\n")
            else:
                f.write(s + "\n")


def build_ref_cli(tmp):
    with open(os.path.join(tmp, "main.c"), "w") as f:
        f.write("int bwa_stdsw(int argc, char *argv[]);\nint main(int argc, char *argv[]) { return bwa_stdsw(argc, argv); }\n")
    exe = os.path.join(tmp, "ref_stdsw")
    subprocess.run(["cc", "-O2", "-w", "-I", REFSRC, "-o", exe, os.path.join(tmp, "main.c")] +
                   [os.path.join(REFSRC, x) for x in ("simple_dp.c", "stdaln.c", "utils.c")] + ["-lz", "-lm"], check=True)
    return exe


def cli_part(genome):
    rng = random.Random(20261)
    os.makedirs(OUT, exist_ok=True)
    g = genome.replace("N", "")
    long_nt = g[50000:50000 + 4096]
    fasta(os.path.join(OUT, "long_nt.fa"), [("L1 the long sequence", long_nt)], width=60)
    # mixed shorts: both strands of the long, mutations, lower case, N, IUPAC letters, odd lengths
    shorts = []
    for k, ln in enumerate([1, 2, 5, 17, 31, 32, 33, 36, 50, 64, 65, 100, 150, 200] * 3):
        a = rng.randrange(0, len(long_nt) - ln)
        s = long_nt[a:a + ln]
        if k % 3 == 1:
            s = s.translate(COMP)[::-1]
        if ln > 4:
            s = mutate(rng, s, "ACGT")
        if k % 4 == 0:
            s = s.lower()
        elif k % 4 == 1:
            s = "".join(ch.lower() if rng.random() < 0.3 else ch for ch in s)
        if k % 5 == 2 and s:
            t = list(s)
            for _ in range(1 + len(t) // 20):
                t[rng.randrange(len(t))] = rng.choice("NnRYKMSWBDHVXx.")
            s = "".join(t)
        shorts.append((f"s{k} mixed short {k}", s))
    shorts.append(("first", long_nt[:40]))
    shorts.append(("last", long_nt[-40:]))
    shorts.append(("random", "".join(rng.choice("ACGT") for _ in range(70))))
    shorts.append(("empty", ""))  # no record in local mode
    fasta(os.path.join(OUT, "short_mixed.fa"), shorts, width=70)
    with gzip.GzipFile(os.path.join(OUT, "short_mixed.fq.gz"), "wb", mtime=0) as f:
        for name, s in shorts[:20]:
            f.write(f"@{name}\n{s}\n+\n{'I' * len(s)}\n".encode())
    s300 = []
    for k in range(300):
        a = rng.randrange(0, len(long_nt) - 36)
        s = mutate(rng, long_nt[a:a + 36], "ACGT", 0.05, 0.01)
        s300.append((f"r{k}", s.translate(COMP)[::-1] if k & 1 else s))
    with gzip.GzipFile(os.path.join(OUT, "short300.fa.gz"), "wb", mtime=0) as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in s300).encode())
    # three long sequences, alone and together, and a few shorts that hit them
    longs3 = [("La", g[200000:200000 + 700]), ("Lb", g[300000:300000 + 333]), ("Lc", g[400000:400000 + 1025])]
    for name, s in longs3:
        fasta(os.path.join(OUT, f"long_{name}.fa"), [(name, s)], width=80)
    few = []
    for k in range(12):
        name, s = longs3[k % 3]
        ln = rng.choice([20, 33, 64, 90])
        a = rng.randrange(0, len(s) - ln)
        few.append((f"f{k}", mutate(rng, s[a:a + ln], "ACGT")))
    fasta(os.path.join(OUT, "short_few.fa"), few)
    # protein: all 20 residues, '*', 'X', and letters without a residue
    long_aa = "".join(rng.choice(AA) for _ in range(600))
    long_aa = long_aa[:300] + "*" + long_aa[300:450] + "XBZ" + long_aa[450:]
    fasta(os.path.join(OUT, "long_aa.fa"), [("P1 protein", long_aa)], width=60)
    paa = [("all20", AA + "*XJ")]
    for k in range(16):
        ln = rng.choice([8, 31, 33, 64, 120])
        a = rng.randrange(0, len(long_aa) - ln)
        s = mutate(rng, long_aa[a:a + ln], AA, 0.08, 0.02)
        paa.append((f"p{k}", s.lower() if k % 4 == 0 else s))
    fasta(os.path.join(OUT, "short_aa.fa"), paa)

    cases = [
        ("default", [], "long_nt.fa", "short_mixed.fa"),
        ("forward", ["-f"], "long_nt.fa", "short_mixed.fa"),
        ("reverse", ["-r"], "long_nt.fa", "short_mixed.fa"),
        ("thres30", ["-T", "30"], "long_nt.fa", "short_mixed.fa"),
        ("global_f", ["-g", "-f"], "long_La.fa", "short_few.fa"),
        ("protein", ["-p"], "long_aa.fa", "short_aa.fa"),
        ("gzip", [], "long_nt.fa", "short_mixed.fq.gz"),
        ("s300", ["-f"], "long_nt.fa", "short300.fa.gz"),
        ("few_La", [], "long_La.fa", "short_few.fa"),
        ("few_Lb", [], "long_Lb.fa", "short_few.fa"),
        ("few_Lc", [], "long_Lc.fa", "short_few.fa"),
        ("usage", [], None, None),
    ]
    listing = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_ref_cli(tmp)
        for name, args, lf, sf in cases:
            files = [os.path.join(OUT, x) for x in (lf, sf) if x]
            r = subprocess.run([exe] + args + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            with open(os.path.join(OUT, name + ".out"), "wb") as f:
                f.write(r.stdout)
            with open(os.path.join(OUT, name + ".err"), "wb") as f:
                f.write(r.stderr)
            listing.append({"name": name, "args": args, "long": lf, "short": sf, "status": r.returncode})
            print(f"{name}: exit {r.returncode}, {len(r.stdout)} B out, {len(r.stderr)} B err")
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in listing) + "\n]\n")


def lib_part(genome):
    L = ctypes.CDLL(REFLIB, mode=os.RTLD_LAZY)  # its @PG printer lives in the harness executable, not needed here
    L.aln_stdaln_aux.restype = ctypes.POINTER(AlnAln)
    L.aln_stdaln_aux.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(AlnParam), ctypes.c_int, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_int]
    L.aln_free_AlnAln.argtypes = [ctypes.POINTER(AlnAln)]
    L.aln_free_AlnAln.restype = None
    presets = {"blast": AlnParam.in_dll(L, "aln_param_blast"), "aa2aa": AlnParam.in_dll(L, "aln_param_aa2aa")}
    # a custom scheme: match 5, anything else -2, gap open 10, extend 2 (gaps cheap beside matches)
    m52 = (ctypes.c_int * 25)(*[5 if x == y else -2 for x in range(5) for y in range(5)])
    presets["match5"] = AlnParam(10, 2, 2, m52, 5, 50)
    rows = []

    def run(pname, mode, thres, band, gap_end, s1, s2, tag):
        src = presets[pname]
        ap = AlnParam(src.gap_open, src.gap_ext, src.gap_end if gap_end is None else gap_end, src.matrix, src.row,
                      src.band_width if band is None else (band if band > 0 else len(s1) + len(s2)))
        aa = L.aln_stdaln_aux(s1.encode(), s2.encode(), ctypes.byref(ap), 0 if mode == "local" else 1, thres, len(s1), len(s2))
        a = aa.contents
        if a.path_len > 0:
            cig = "".join(f"{a.cigar32[k] >> 4}{'MID'[a.cigar32[k] & 0xf]}" for k in range(a.n_cigar))
            rec = (a.score, a.subo if mode == "local" else 0, a.path_len, a.start1, a.end1, a.start2, a.end2, cig)
        else:  # no path: the other fields are not set by the reference
            rec = (a.score, "", 0, "", "", "", "", "")
        L.aln_free_AlnAln(aa)
        rows.append((tag, pname, mode, thres, 0 if band == 0 else ap.band_width, ap.gap_end, s1, s2) + rec)
        return rec

    rng = random.Random(20262)
    g = genome.replace("N", "")
    slens = [1, 2, 31, 32, 33, 64, 65, 200]
    llens = [1, 63, 64, 65, 257, 1000, 4096]
    for pname in ("blast", "aa2aa"):
        alpha = "ACGT" if pname == "blast" else AA
        for ll in llens:
            if pname == "blast":
                a = rng.randrange(0, len(g) - ll)
                lng = g[a:a + ll]
            else:
                lng = "".join(rng.choice(AA) for _ in range(ll))
            for sl in slens:
                if sl <= ll:
                    a = rng.randrange(0, ll - sl + 1)
                    sh = lng[a:a + sl]
                    sh = mutate(rng, sh, alpha, 0.06, 0.02) if sl > 2 else sh
                    sh = (sh + "".join(rng.choice(alpha) for _ in range(sl)))[:sl]
                else:  # a short longer than the long: the long inside it
                    a = rng.randrange(0, sl - ll + 1)
                    sh = "".join(rng.choice(alpha) for _ in range(a)) + lng + "".join(rng.choice(alpha) for _ in range(sl - ll - a))
                if pname == "blast" and rng.random() < 0.2:
                    t = list(sh)
                    t[rng.randrange(len(t))] = "N"
                    sh = "".join(t)
                run(pname, "local", 1, rng.choice([None, 0]), None, sh, lng, "grid")
                run(pname, "global", 1, rng.choice([None, 0]), rng.choice([None, 0]), sh, lng, "grid")
    # ---- suboptimal score (stdsw's own settings: full band, gap_end 0)
    rs = lambda n: "".join(rng.choice("ACGT") for _ in range(n))  # noqa: E731
    for ln in (20, 60, 101):
        s = rs(ln)
        run("blast", "local", 1, 0, 0, s, rs(300) + s + rs(500) + s + rs(200), "subo_far_copy")
        run("blast", "local", 1, 0, 0, s, rs(200) + s + s[-(ln // 4):] + rs(300), "subo_window_tail")
        run("blast", "local", 1, 0, 0, s, rs(200) + s[:ln // 4] + s + rs(300), "subo_window_head")
        run("blast", "local", 1, 0, 0, s, rs(200) + s + rs(ln // 5) + s + rs(100), "subo_near_copy")
        run("blast", "local", 1, 0, 0, s, s + rs(400), "subo_hit_first")
        run("blast", "local", 1, 0, 0, s, rs(400) + s, "subo_hit_last")
        run("blast", "local", 1, 0, 0, s, s, "subo_whole")
        run("blast", "local", 1, 0, 0, "ACGT" * (ln // 4), "A" * 150 + "ACGT" * (ln // 4) + "C" * 150, "subo_no_other")
    # ---- long internal gaps: blocks of seq1 separated in seq2 by linkers twice their length, which
    # the optimal local path bridges (the hit spans far more of seq2 than seq1 is long)
    for pname, alpha, blk in (("match5", "ACGT", 100), ("aa2aa", AA, 60), ("match5", "ACGT", 33)):
        blocks = ["".join(rng.choice(alpha) for _ in range(blk)) for _ in range(3)]
        link = lambda: "".join(rng.choice(alpha) for _ in range(2 * blk))  # noqa: E731
        for band in (0, None):
            run(pname, "local", 1, band, None, "".join(blocks), link()[:50] + blocks[0] + link() + blocks[1] + link() + blocks[2] + link()[:70], "long_gap")
            run(pname, "local", 1, band, None, link()[:9] + blocks[0] + link() + blocks[1] + link() + blocks[2], "".join(blocks), "long_gap_seq1")
    # ---- ties: a tandem repeat unit against a run of repeats
    for unit in ("A", "AC", "ACG", "ACGT", "AACGT", rs(31), rs(32), rs(33)):
        for reps in (3, 10):
            run("blast", "local", 1, 0, 0, unit, unit * reps, "tie_unit")
            run("blast", "local", 1, None, None, unit * 2, rs(7) + unit * reps + rs(9), "tie_unit2")
            run("aa2aa", "local", 1, 0, 0, "WKV", "WKV" * reps, "tie_aa")
    # ---- thresholds: thres equal to the score and one above it
    for ln in (12, 40, 90):
        s = rs(ln)
        lng = rs(100) + mutate(rng, s, "ACGT") + rs(100)
        sc = run("blast", "local", 1, 0, 0, s, lng, "thres_base")[0]
        run("blast", "local", sc, 0, 0, s, lng, "thres_equal")
        run("blast", "local", sc + 1, 0, 0, s, lng, "thres_above")
    path = os.path.join(OUT, "stdaln_vectors.tsv.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as gz, io.TextIOWrapper(gz) as f:
        f.write("#tag\tparam\tmode\tthres\tband(0: len1+len2)\tgap_end\tseq1\tseq2\tscore\tsubo\tpath_len\tstart1\tend1\tstart2\tend2\tcigar\n")
        for r in rows:
            f.write("\t".join(str(x) for x in r) + "\n")
    print(f"{len(rows)} library vectors -> {path} ({os.path.getsize(path)} B)")


def main():
    if not os.path.isdir(REFSRC) or not os.path.exists(REFLIB):
        sys.exit("needs the reference's sources and oracle/_ref/libibwa_ref.so (make -C oracle ref)")
    from tests.synth_util import golden_genome_ascii
    genome, _, _ = golden_genome_ascii()
    cli_part(genome)
    lib_part(genome)


if __name__ == "__main__":
    main()
