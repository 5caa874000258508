#!/usr/bin/env python3
"""Generate tests/golden/aln_edges/: `aln` at the option values and read lengths where the engine
chooses another kernel (engine_aln.hip run_setup / plan_first_pass).

TEST INFRASTRUCTURE.  Run where `make -C oracle ref` has built oracle/_ref/ibwa_ref.  The reads are
cut from the committed .pac files (fixed positions, a seeded generator for the edits).  Those on the
300 bp text are committed as FASTQ; those on g1m as recipes (reads.json: positions, lengths, strands
and the substituted bases, or a range of reads_r100.fq's records) from which tests/aln_edges_util.py
rebuilds them, here for the reference and in the tests.  The reference's `aln` writes one .sai per (reads, argv); manifest.json holds, per case, the
index prefix, the reads file, the argv, the .sai's sha1 and -- for the cases that fill an entry bit
field of k_gapped (gapped.hip: n_mm 5 bits, n_gapo 3, n_gape 4) -- the largest n_mm / n_gapo /
n_gape among the reference's hits.  Only program output and generated inputs are stored.

  stale_alt (300 bp; the tiny text bounds every search):
    bf_mm.fq    50 bp reads at 50 % substitutions            -n 30 / -n 31: hits of 30 mismatches
    bf_gapo.fq  reads lacking 7 single bases, 9 apart        -o 7 / -o 8:   hits of 7 gap opens
    bf_gape.fq  reads with one 16-base deletion / insertion  -e 15 / -e 16: hits of 15 extensions
                (the two gap sets also hold reads without a hit whose search runs into -m 20000)
  g1m (recipes in reads.json under these names):
    r100_200.fq / r100_40.fq  the first reads of reads_r100.fq
    r100_plus300.fq           r100_200.fq with one 300-base read inserted
    long.fq                   256 ... 5 000 bases, 0-2 substitutions, both strands
    len257.fq len300.fq len1000.fq   0-3 substitutions, for the default -n 0.04
    len65535.fq               two reads of 65 535 bases
"""
import hashlib
import json
import os
import random
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "aln_edges")
REF = os.path.join(ROOT, "oracle", "_ref", "ibwa_ref")
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from tests import aln_edges_util as U  # noqa: E402

TMP = tempfile.mkdtemp(prefix="aln_edges_")

ACGT = "ACGT"
TAIL = ["-l", "1000"]
GAP_TAIL = ["-i", "0", "-d", "100", "-l", "1000"]
GAPE_SCORES = ["-M", "11", "-O", "3", "-E", "1"]

# name -> (index prefix, reads file, argv, records the bit-field maxima)
CASES = {}


def case(prefix, reads, argv, fields=False):
    key = reads[:-3] + "." + ("".join(argv).replace("-", "") or "default")
    assert key not in CASES, key
    CASES[key] = (prefix, reads, argv, fields)


# entry bit fields, at the last value each holds and one past it
case("stale_alt", "bf_mm.fq", ["-n", "30", "-o", "0"] + TAIL, True)
case("stale_alt", "bf_mm.fq", ["-n", "31", "-o", "0"] + TAIL, True)
case("stale_alt", "bf_gapo.fq", ["-n", "7", "-o", "7"] + GAP_TAIL + ["-m", "20000"], True)
case("stale_alt", "bf_gapo.fq", ["-n", "8", "-o", "8"] + GAP_TAIL + ["-m", "20000"], True)
case("stale_alt", "bf_gape.fq", ["-n", "16", "-o", "1", "-e", "15"] + GAP_TAIL + GAPE_SCORES + ["-m", "20000"], True)
case("stale_alt", "bf_gape.fq", ["-n", "17", "-o", "1", "-e", "16"] + GAP_TAIL + GAPE_SCORES + ["-m", "20000"], True)
# LDS-width selection (plan_first_pass): batch max_diff, seed differences, the largest penalty
for argv in ([], ["-n", "6"], ["-n", "7"], ["-k", "2"], ["-k", "3"], ["-M", "15"], ["-M", "16"], ["-O", "15"],
             ["-O", "16"], ["-E", "15"], ["-E", "16"], ["-e", "16"]):
    case("g1m", "r100_200.fq", argv)
# workgroup size by n_stacks with the LDS widths off (-k 3: n_stacks 46 + 2 O; -M 16: 124 + 2 O)
for argv in (["-k", "3", "-O", "25"], ["-k", "3", "-O", "26"], ["-k", "3", "-O", "89"], ["-k", "3", "-O", "90"],
             ["-M", "16", "-O", "50"], ["-M", "16", "-O", "51"]):
    case("g1m", "r100_200.fq", argv)
# k_coop's bucket limit (n_stacks 128 / 130) and scores past the 128th bucket
for argv in (["-O", "41"], ["-O", "42"], ["-O", "43"], ["-O", "50"], ["-O", "130"], ["-M", "16", "-O", "120"]):
    case("g1m", "r100_200.fq", argv)
# n_stacks at the first pass's LDS limit (480 / 482), beyond it, and beyond the wide kernel's
for argv in (["-O", "217"], ["-O", "218"], ["-O", "250"], ["-O", "700"], ["-O", "6200"]):
    case("g1m", "r100_40.fq", argv)
# read length
case("g1m", "long.fq", ["-n", "2"])
case("g1m", "long.fq", ["-n", "0"])
for f in ("len257.fq", "len300.fq", "len1000.fq", "r100_plus300.fq"):
    case("g1m", f, [])
case("g1m", "len65535.fq", ["-n", "1"])
case("g1m", "len65535.fq", ["-n", "0"])


def text_of(prefix):
    codes, _ = oracle.read_pac(os.path.join(GOLD, prefix))
    return "".join(ACGT[c] for c in codes)


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def substitute(s, positions, rng):
    s = list(s)
    for j in positions:
        s[j] = rng.choice([c for c in ACGT if c != s[j]])
    return "".join(s)


def fq(name, recs):
    with open(os.path.join(OUT, name), "w") as f:
        for nm, s in recs:
            f.write(f"@{nm}\n{s}\n+\n{'I' * len(s)}\n")


def run_ref(prefix, reads, argv, out):
    path = os.path.join(OUT, reads)
    if not os.path.exists(path):  # a set kept as a recipe: its FASTQ only for this run
        path = U.write_fastq(os.path.join(TMP, reads), U.records(GOLD, reads))
    subprocess.run([REF, "aln", *argv, "-f", out, os.path.join(GOLD, prefix), path], check=True,
                   stderr=subprocess.DEVNULL)


def sai_fields(path):
    """Per read the largest (n_mm, n_gapo, n_gape) of its hits (bwt_aln1_t, bwtaln.h:34-38); -1 without hits."""
    b = open(path, "rb").read()
    p, out = 64, []
    while p < len(b):
        n, = struct.unpack_from("<i", b, p)
        info = np.frombuffer(b, dtype="<u4", count=n * 4, offset=p + 4)[0::4]
        out.append(tuple(int(((info >> sh) & 0xff).max()) if n else -1 for sh in (0, 8, 16)))
        p += 4 + 16 * n
    return out


def stale_sets():
    g = text_of("stale_alt")
    rng = random.Random(20261021)
    # 50 % substitutions; on the 300 bp text the best placements have 24 to 30 mismatches.  The set keeps
    # the first 32 candidates none of whose hits under -n 31 has more than 30, so that the field's last
    # value is the largest on both sides of the boundary.
    tmp_fq, tmp_sai = "bf_mm.cand.fq", os.path.join(OUT, "bf_mm.cand.sai")
    cand = []
    for k in range(96):
        p = rng.randrange(0, len(g) - 50)
        s = g[p:p + 50] if k & 1 else rc(g[p:p + 50])
        cand.append((f"mm{k}", substitute(s, [j for j in range(50) if rng.random() < 0.5], rng)))
    fq(tmp_fq, cand)
    run_ref("stale_alt", tmp_fq, ["-n", "31", "-o", "0"] + TAIL, tmp_sai)
    keep = [r for r, f in zip(cand, sai_fields(tmp_sai)) if f[0] <= 30][:32]
    os.remove(os.path.join(OUT, tmp_fq))
    os.remove(tmp_sai)
    assert len(keep) == 32
    fq("bf_mm.fq", keep)

    recs = []
    for k in range(12):  # 8 runs of 9 bases, the base between two runs left out
        p = rng.randrange(0, len(g) - 80)
        s = "".join(g[p + 10 * j:p + 10 * j + 9] for j in range(8))
        recs.append((f"go{k}", s if k & 1 else rc(s)))
    # No hit, and a lower bound of one difference: two 36-base pieces of the text from different places.
    # The search widens until its stack passes -m 20000.
    for k in range(6):
        p, q = rng.randrange(0, len(g) - 36), rng.randrange(0, len(g) - 36)
        recs.append((f"go_none{k}", g[p:p + 36] + (rc(g[q:q + 36]) if k & 1 else g[q:q + 36])))
    fq("bf_gapo.fq", recs)

    recs = []
    for k in range(16):
        p = rng.randrange(0, len(g) - 80)
        if k & 2:  # 16 bases of the text left out
            s = g[p:p + 30] + g[p + 46:p + 76]
        else:      # 16 bases put in
            s = g[p:p + 30] + "".join(rng.choice(ACGT) for _ in range(16)) + g[p + 30:p + 60]
        recs.append((f"ge{k}", s if k & 1 else rc(s)))
    for k in range(4):  # a gap of 18 bases: two more extensions than either case allows, stopped by -m 20000
        p = rng.randrange(0, len(g) - 80)
        if k & 2:
            s = g[p:p + 30] + g[p + 48:p + 78]
        else:
            s = g[p:p + 30] + "".join(rng.choice(ACGT) for _ in range(18)) + g[p + 30:p + 60]
        recs.append((f"ge_none{k}", s if k & 1 else rc(s)))
    fq("bf_gape.fq", recs)


def g1m_sets():
    """The g1m sets as recipes (tests/aln_edges_util.py builds the reads): reads.json."""
    g = text_of("g1m")
    rng = random.Random(20261022)
    r100 = "reads_r100.fq"
    sets = {"r100_200.fq": [["fastq", r100, 0, 200]], "r100_40.fq": [["fastq", r100, 0, 40]]}

    def cut(name, n, nsub, k, p=None, at=None):
        p = rng.randrange(0, len(g) - n) if p is None else p
        at = rng.sample(range(n), nsub) if at is None else at
        s = substitute(g[p:p + n], at, rng)
        return ["cut", name, p, n, k & 1, [[j, s[j]] for j in at]]

    recs, k = [], 0
    for n in (256, 257, 300, 1000, 4095, 4096, 5000):
        for nsub in (0, 1, 2):
            for _ in range(2):
                recs.append(cut(f"L{n}_s{nsub}_{k & 1}", n, nsub, k))
                k += 1
    sets["long.fq"] = recs
    for n in (257, 300, 1000):
        sets[f"len{n}.fq"] = [cut(f"F{n}_s{j >> 1}_{j & 1}", n, j >> 1, j) for j in range(8)]
    sets["r100_plus300.fq"] = [["fastq", r100, 0, 77], cut("ins300", 300, 1, 0), ["fastq", r100, 77, 200]]
    sets["len65535.fq"] = [cut("M65535_0", 65535, 0, 0, p=100000, at=[]), cut("M65535_1", 65535, 1, 1, p=600000, at=[40000])]
    with open(os.path.join(OUT, "reads.json"), "w") as f:
        f.write("{\n" + ",\n".join(f' {json.dumps(k)}: [\n  ' + ",\n  ".join(json.dumps(i) for i in v) + "\n ]"
                                     for k, v in sorted(sets.items())) + "\n}\n")


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    os.makedirs(OUT, exist_ok=True)
    stale_sets()
    g1m_sets()
    manifest = {}
    for key, (prefix, reads, argv, fields) in CASES.items():
        out = os.path.join(OUT, key + ".sai")
        run_ref(prefix, reads, argv, out)
        m = {"index": prefix, "reads": reads, "argv": argv, "sha1": hashlib.sha1(open(out, "rb").read()).hexdigest()}
        if fields:
            f = sai_fields(out)
            m["max_fields"] = {nm: max(x[j] for x in f) for j, nm in enumerate(("n_mm", "n_gapo", "n_gape"))}
        manifest[key] = m
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(manifest.items())) + "\n}\n")
    shutil.rmtree(TMP)
    print("aln edge fixtures written to", OUT)


if __name__ == "__main__":
    main()
