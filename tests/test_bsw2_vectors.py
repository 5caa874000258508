"""bsw2_core.h, the host restatement of bwasw's seeding, against the golden vectors.

tests/golden/bwasw/seed_vectors.tsv.gz holds what the reference's bwtl_seq2bwtl + bsw2_core gave on
tests/golden/g1m (tools/make_bwasw_golden.py).  tests/host/bsw2_seed_check.cpp, built here with g++
and no HIP, instantiates the restatement over the .bwt / .sa files, must reproduce every vector,
and counts the classes the vectors have to cover; check_classes repeats the conditions the tool
wrote the file under, so a thinned file cannot pass.  Needs no reference and no device.

Two more files of the same format and origin: seed_long_vectors.tsv.gz, reads of 1 023 to 8 192 bases
(check_long_classes), and seed_small_index_vectors.tsv.gz, tasks on the small indexes idx_quirks and
csg with their N-runs and repeats (check_small_classes).
"""
import gzip
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
VECTORS = os.path.join(GOLD, "bwasw", "seed_vectors.tsv.gz")
LONG_VECTORS = os.path.join(GOLD, "bwasw", "seed_long_vectors.tsv.gz")  # g1m, 1 023 to 8 192 bases
SMALL_VECTORS = os.path.join(GOLD, "bwasw", "seed_small_index_vectors.tsv.gz")  # idx_quirks and csg

LENGTHS = (1, 2, 8, 17, 30, 64, 100, 150, 400, 1000)
KINDS = ("exact", "sub2", "sub5", "sub10", "sub2indel", "sub5indel", "sub10indel", "longdel", "chimera", "random",
         "polyA", "ACAC", "period3")
OPTSETS = ("defaults", "z3", "b5q2r1z10", "s1", "s10", "a2", "w5", "T10", "fixed")
EVENTS = ("swap", "dup", "tie_cut", "band_del", "recreate", "array256", "flag1", "displaced", "narrow_tie", "empty")


def parse_classes(stdout):
    out = {}
    for line in stdout.splitlines():
        if "\t" in line:
            k, v = line.split("\t")
            out[k] = int(v)
    return out


def check_classes(cls):
    """The conditions on the vector file; returns the list of those it misses."""
    bad = []
    for ln in LENGTHS:
        if cls.get(f"len:{ln}:f", 0) < 3:
            bad.append(f"length {ln} on the forward index: {cls.get(f'len:{ln}:f', 0)} < 3")
    for ln in (150, 400):
        if cls.get(f"len:{ln}:r", 0) < 1:
            bad.append(f"length {ln} on .rbwt: none")
    for k in KINDS:
        if cls.get("kind:" + k, 0) < 1:
            bad.append(f"read kind {k}: none")
    for k in OPTSETS:
        if cls.get("optset:" + k, 0) < 1:
            bad.append(f"option set {k}: none")
    for k in EVENTS:
        if cls.get("event:" + k, 0) < 10:
            bad.append(f"event {k}: {cls.get('event:' + k, 0)} < 10")
    return bad


LONG_LENGTHS = (1023, 1024, 2047, 2048, 2049, 4095, 4096, 8191, 8192)
LONG_KINDS = ("sub2", "sub10", "chimera", "random", "period3", "polyA", "ACAC", "period3exact")
SMALL_INDEXES = ("idx_quirks", "csg")


def check_long_classes(cls):
    """The conditions on the file of long reads: the lengths around the 2 048 keys the suffix sort
    holds in LDS and around the longest read, every kind beyond the LDS sort, the periodic reads of
    many doubling rounds at full length, and hits -- not only empty lists -- on both sides of 2 048."""
    bad = []
    for ln in LONG_LENGTHS:
        if cls.get(f"len:{ln}:f", 0) < 4:
            bad.append(f"length {ln} on the forward index: {cls.get(f'len:{ln}:f', 0)} < 4")
        if cls.get(f"len:{ln}:r", 0) < 1:
            bad.append(f"length {ln} on .rbwt: none")
    for ln in LONG_LENGTHS:  # the size limit does not bind: nothing is thinned
        for k in LONG_KINDS:
            if cls.get(f"at:{ln}:{k}", 0) < 2:
                bad.append(f"read kind {k} at length {ln}: {cls.get(f'at:{ln}:{k}', 0)} < 2")
    for k in LONG_KINDS:
        if cls.get("long:" + k, 0) < 1:
            bad.append(f"read kind {k} at 2 048 bases or more: none")
    for k in ("polyA", "period3exact"):
        if cls.get(f"at:8192:{k}", 0) < 1:
            bad.append(f"read kind {k} at 8 192 bases: none")
    for ln in (2047, 2049):
        if cls.get(f"hits:{ln}", 0) < 1:
            bad.append(f"length {ln}: no vector with a hit")
    for k in ("defaults", "z3"):
        if cls.get("optset:" + k, 0) < 1:
            bad.append(f"option set {k}: none")
    return bad


def check_small_classes(cls):
    """The conditions on the file of the small indexes."""
    return [f"index {k}: {cls.get('index:' + k, 0)} < 40" for k in SMALL_INDEXES if cls.get("index:" + k, 0) < 40]


def build_checker(tmp_path):
    exe = str(tmp_path / "bsw2_seed_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "ibwa_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "bsw2_seed_check.cpp")], check=True)
    return exe


def read_vectors(path=VECTORS):
    """[(optset, opt dict, strand, kind, codes, (all, narrow), (t, bw))] of a golden file.  In the file
    of the small indexes optset is "INDEX/name": the vector was made on tests/golden/INDEX (index_of)."""
    out = []
    with gzip.open(path, "rt") as f:
        for line in f:
            c = line.rstrip("\n").split("\t")
            opt = dict(zip(("a", "b", "q", "r", "t", "bw", "z", "is"), map(int, c[1:9])), coef=float(c[9]), adjust=int(c[10]))
            w = c[16].split()
            na, nn = int(w[0]), int(w[1])
            hits = [tuple(int(x) for x in h.split(",")) for h in w[2:]]
            assert len(hits) == na + nn
            out.append((c[0], opt, int(c[13]), c[14], [int(x) for x in c[15]], (hits[:na], hits[na:]), (int(c[11]), int(c[12]))))
    return out


def index_of(optset):
    """The index under tests/golden a vector's option set names: "INDEX/name", else g1m."""
    return optset.split("/")[0] if "/" in optset else "g1m"


def run_vectors(tmp_path, path):
    """bsw2_seed_check vectors over a golden file -> (classes, number of vectors); every one reproduced."""
    exe = build_checker(tmp_path)
    plain = tmp_path / "vectors.tsv"
    with gzip.open(path, "rb") as f:
        plain.write_bytes(f.read())
    r = subprocess.run([exe, "vectors", os.path.join(GOLD, "g1m"), str(plain)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith(" 0 differ")
    return parse_classes(r.stdout), int(r.stdout.strip().splitlines()[-1].split()[0])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_restatement_reproduces_every_vector(tmp_path):
    cls, n = run_vectors(tmp_path, VECTORS)
    assert check_classes(cls) == []
    assert 400 <= n <= 800


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_restatement_reproduces_every_long_vector(tmp_path):
    cls, n = run_vectors(tmp_path, LONG_VECTORS)
    assert check_long_classes(cls) == []
    assert n >= 9 * (8 * 2 + 1)  # every length x kind x option set on .bwt, one per length on .rbwt
    # the same conditions read from the file itself
    vs = read_vectors(LONG_VECTORS)
    assert len(vs) == n and {v[0] for v in vs} == {"defaults", "z3"} and {len(v[4]) for v in vs} == set(LONG_LENGTHS)
    assert {v[3] for v in vs if len(v[4]) >= 2048} == set(LONG_KINDS)
    assert all(v[4] == [0] * 8192 for v in vs if v[3] == "polyA" and len(v[4]) == 8192)
    for ln in (2047, 2049):
        assert any(v[5][0] or v[5][1] for v in vs if len(v[4]) == ln)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_restatement_reproduces_every_small_index_vector(tmp_path):
    cls, n = run_vectors(tmp_path, SMALL_VECTORS)
    assert check_small_classes(cls) == []
    vs = read_vectors(SMALL_VECTORS)
    assert len(vs) == n
    for name in SMALL_INDEXES:
        mine = [v for v in vs if index_of(v[0]) == name]
        assert len(mine) >= 40 and {v[1]["is"] for v in mine} == {0, 1, 3, 6, 50}
        assert all(1 <= len(v[4]) <= 300 and len(v[5][0]) + len(v[5][1]) <= 1500 for v in mine)
        assert all(v[5][0] == [] for v in mine if v[1]["is"] == 0)  # the undefined read is not recorded


def test_vector_file_is_small():
    assert os.path.getsize(VECTORS) <= 256 * 1024


def test_long_and_small_index_vector_files_are_small():
    assert os.path.getsize(LONG_VECTORS) <= 256 * 1024
    assert os.path.getsize(SMALL_VECTORS) <= 256 * 1024
