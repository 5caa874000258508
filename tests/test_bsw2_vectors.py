"""bsw2_core.h, the host restatement of bwasw's seeding, against the golden vectors.

tests/golden/bwasw/seed_vectors.tsv.gz holds what the reference's bwtl_seq2bwtl + bsw2_core gave on
tests/golden/g1m (tools/make_bwasw_golden.py).  tests/host/bsw2_seed_check.cpp, built here with g++
and no HIP, instantiates the restatement over the .bwt / .sa files, must reproduce every vector,
and counts the classes the vectors have to cover; check_classes repeats the conditions the tool
wrote the file under, so a thinned file cannot pass.  Needs no reference and no device.
"""
import gzip
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
VECTORS = os.path.join(GOLD, "bwasw", "seed_vectors.tsv.gz")

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


def build_checker(tmp_path):
    exe = str(tmp_path / "bsw2_seed_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "ibwa_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "bsw2_seed_check.cpp")], check=True)
    return exe


def read_vectors():
    """[(optset, opt dict, strand, kind, codes, (all, narrow))] of the golden file."""
    out = []
    with gzip.open(VECTORS, "rt") as f:
        for line in f:
            c = line.rstrip("\n").split("\t")
            opt = dict(zip(("a", "b", "q", "r", "t", "bw", "z", "is"), map(int, c[1:9])), coef=float(c[9]), adjust=int(c[10]))
            w = c[16].split()
            na, nn = int(w[0]), int(w[1])
            hits = [tuple(int(x) for x in h.split(",")) for h in w[2:]]
            assert len(hits) == na + nn
            out.append((c[0], opt, int(c[13]), c[14], [int(x) for x in c[15]], (hits[:na], hits[na:]), (int(c[11]), int(c[12]))))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_restatement_reproduces_every_vector(tmp_path):
    exe = build_checker(tmp_path)
    plain = tmp_path / "vectors.tsv"
    with gzip.open(VECTORS, "rb") as f:
        plain.write_bytes(f.read())
    r = subprocess.run([exe, "vectors", os.path.join(GOLD, "g1m"), str(plain)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith(" 0 differ")
    cls = parse_classes(r.stdout)
    assert check_classes(cls) == []
    n = int(r.stdout.strip().splitlines()[-1].split()[0])
    assert 400 <= n <= 800


def test_vector_file_is_small():
    assert os.path.getsize(VECTORS) <= 256 * 1024
