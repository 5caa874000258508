"""bsw2_aln1.h, the host restatement of bwasw from seeds to hits, against the golden vectors.

tests/golden/bwasw/aln1_vectors.tsv.gz holds what the reference's bsw2_aln1_core gave on tests/golden/g1m,
left_vectors.tsv.gz what its bsw2_extend_left gave on hit lists (tools/make_bwasw_hits_golden.py).
tests/host/bsw2_aln1_check.cpp, a stand-alone program built here with g++ and no HIP, once plain and
once with -fsanitize=address,undefined, must reproduce every line and counts the classes the lines
have to cover; check_classes repeats the conditions the tool wrote the files under, so a thinned
file cannot pass.  Needs no reference and no device.
"""
import gzip
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ALN1_VECTORS = os.path.join(GOLD, "bwasw", "aln1_vectors.tsv.gz")
LEFT_VECTORS = os.path.join(GOLD, "bwasw", "left_vectors.tsv.gz")

MIN = 5  # members of every class
# per hit and per list of the left extension, counted over both files
LEFT_CLASSES = ("left:extended", "left:not_extensible", "left:contained_orig", "left:contained_ext_only", "left:same_window",
                "left:earlier_window", "left:k_zero", "left:lt_clipped", "left:beg_zero", "left:equal_end", "task:n0", "task:n1",
                "task:n64", "task:n65", "task:n129", "task:n_seeds64")
# per read, in the file of whole reads
ALN1_CLASSES = ("chain:lost", "chain:other_strand", "right:clipped", "right:equal", "right:kept", "right:is_rev0", "right:is_rev1",
                "overlap:tie_j", "overlap:zeroed", "overlap:g2_raised")
KINDS = ("twice", "cut0", "cut1", "cut2", "cutend")


def parse_classes(stdout):
    out = {}
    for line in stdout.splitlines():
        if "\t" in line:
            k, v = line.split("\t")
            out[k] = int(v)
    return out


def check_classes(aln1, left):
    """The conditions on the two vector files; returns the list of those they miss."""
    bad = []
    for k in LEFT_CLASSES:
        n = aln1.get(k, 0) + left.get(k, 0)
        if n < MIN:
            bad.append(f"{k}: {n} < {MIN}")
    for k in ALN1_CLASSES:
        if aln1.get(k, 0) < MIN:
            bad.append(f"{k}: {aln1.get(k, 0)} < {MIN}")
    for k in KINDS:
        if aln1.get("kind:" + k, 0) < 1:
            bad.append(f"read kind {k}: none")
    for ln in (17, 1000, 2049, 8192):
        if aln1.get(f"len:{ln}", 0) < 1:
            bad.append(f"length {ln}: none")
    return bad


def read_aln1_vectors(path=ALN1_VECTORS):
    """[(optset, opt dict, is_rev, kind, s, codes, final, (left0, left1))]; a hit is a 9-tuple
    (k, l, flag, n_seeds, len, G, G2, beg, end)."""
    out = []
    with gzip.open(path, "rt") as f:
        for line in f:
            c = line.rstrip("\n").split("\t")
            opt = dict(zip(("a", "b", "q", "r", "t", "bw", "z", "is"), map(int, c[1:9])), coef=float(c[9]), adjust=int(c[10]),
                       t_seeds=int(c[11]), mask_level=float(c[12]))
            out.append((c[0], opt, int(c[15]), c[16], int(c[17]), [int(x) for x in c[18]], parse_list(c[19]),
                        (parse_list(c[20]), parse_list(c[21]))))
    return out


def read_left_vectors(path=LEFT_VECTORS):
    """[(a, b, q, r, bw, is_rev, kind, codes, hits_in, hits_out)]"""
    out = []
    with gzip.open(path, "rt") as f:
        for line in f:
            c = line.rstrip("\n").split("\t")
            out.append(tuple(map(int, c[:6])) + (c[6], [int(x) for x in c[7]], parse_list(c[8]), parse_list(c[9])))
    return out


def parse_list(text):
    w = text.split()
    hits = [tuple(int(x) for x in h.split(",")) for h in w[1:]]
    assert len(hits) == int(w[0])
    return hits


def draw(s):
    """The first drand48() after srand48(s)."""
    x = (s & 0xffffffff) << 16 | 0x330E
    return ((0x5DEECE66D * x + 0xB) & ((1 << 48) - 1)) / float(1 << 48)


def build_checker(tmp_path, sanitize=False):
    exe = str(tmp_path / ("bsw2_aln1_check_san" if sanitize else "bsw2_aln1_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-pthread"] + flags + ["-I", os.path.join(ROOT, "ibwa_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "bsw2_aln1_check.cpp")], check=True)
    return exe


def run_vectors(exe, tmp_path, mode, path):
    plain = tmp_path / (mode + ".tsv")
    with gzip.open(path, "rb") as f:
        plain.write_bytes(f.read())
    r = subprocess.run([exe, mode, os.path.join(GOLD, "g1m"), str(plain)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith(" 0 differ")
    return parse_classes(r.stdout), int(r.stdout.strip().splitlines()[-1].split()[0])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", (False, True), ids=("plain", "asan_ubsan"))
def test_restatement_reproduces_every_vector(tmp_path, sanitize):
    exe = build_checker(tmp_path, sanitize)
    aln1, n_aln1 = run_vectors(exe, tmp_path, "vectors", ALN1_VECTORS)
    left, n_left = run_vectors(exe, tmp_path, "leftvectors", LEFT_VECTORS)
    assert check_classes(aln1, left) == []
    assert n_aln1 == len(read_aln1_vectors()) and n_left == len(read_left_vectors())


def test_draw_is_drand48():
    # srand48(1); drand48() of the C library (POSIX fixes the generator)
    assert abs(draw(1) - 0.041630344771475) < 1e-12
    assert all(0.0 <= draw(s) < 1.0 for s in range(1, 2000))


def test_vector_files_are_small():
    assert os.path.getsize(ALN1_VECTORS) <= 256 * 1024
    assert os.path.getsize(LEFT_VECTORS) <= 256 * 1024
