"""bsw2_aln1.h against the reference's own bsw2_aln1_core on seeded random reads (build container only).

The reference's sources are compiled where they lie into tmp_path with the harness main of
tools/make_bwasw_hits_golden.py, next to tests/host/bsw2_aln1_check.cpp; both run the same 500 reads on
tests/golden/g1m -- 20 to 500 bases, both strands of the index, a 1 to 2, z 1 to 3, is 1 to 6, t 8 to 40, bw 1 to
50, t_seeds 1 to 6, three mask levels -- and every stage is compared field for field: the narrow lists
after the chain filter and after the left extension, the strand lists after the right extension, and
the final list.  The harness stops unless its own final list equals bsw2_aln1_core's.  The device tests
draw from the same generators.
"""
import os
import random
import shutil
import subprocess

import pytest

from tests.test_bsw2_core_host import GOLD, REFSRC, genome

needs_reference = pytest.mark.skipif(
    not os.path.isdir(REFSRC) or shutil.which("gcc") is None or shutil.which("g++") is None,
    reason="needs the reference tree, gcc and g++")

MASKS = (0.5, 0.9, 0.1)


def random_reads(n, seed, min_len=20, max_len=500):
    """[(a, b, q, r, t, bw, z, is, t_seeds, mask_level, is_rev, s, codes)]: two thirds of the reads come from
    the genome, mutated, a sixth of those with the locus twice; the rest are periodic or random."""
    g = genome()
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        ln = rng.randrange(min_len, max_len + 1)
        x = rng.random()
        if x < 0.66:
            a0 = rng.randrange(0, len(g) - ln)
            rate = rng.choice((0.0, 0.02, 0.05, 0.1))
            s = [(c + rng.randrange(1, 4)) & 3 if rng.random() < rate else c for c in g[a0:a0 + ln]]
            if ln > 40 and rng.random() < 0.4:
                p = rng.randrange(10, ln - 10)
                s = s[:p] + s[p + rng.randrange(1, 8):]
            if rng.random() < 0.16:
                s = s[:ln // 2] + s[:ln // 2]
        elif x < 0.8:
            per = rng.randrange(1, 5)
            s = [(j % per + (rng.random() < 0.03)) & 3 for j in range(ln)]
        else:
            s = [rng.randrange(4) for _ in range(ln)]
        is_rev = rng.randrange(2)
        out.append((rng.randrange(1, 3), rng.randrange(1, 6), rng.randrange(1, 7), rng.randrange(1, 4), rng.randrange(8, 41),
                    rng.randrange(1, 51), rng.randrange(1, 4), rng.randrange(1, 7), rng.randrange(1, 7), rng.choice(MASKS), is_rev,
                    rng.randrange(1, 1 << 20), s[::-1] if is_rev else s))
    return out


def write_reads(path, reads):
    """The task file of both programs' "stages" mode; t and bw are used as given (adjust 0)."""
    with open(path, "w") as f:
        for a, b, q, r, t, bw, z, is_, t_seeds, mask, is_rev, s, seq in reads:
            f.write(f"{a} {b} {q} {r} {t} {bw} {z} {is_} 5.5 0 {t_seeds} {mask} {is_rev} {s} {''.join(map(str, seq))}\n")


def nested_list(n=16400, lq=400, a0=500000):
    """(query codes, hits): hit 0 spans bases 100 to 300 of the read and ends last; the other n - 1 lie
    inside it, many inside one another, so hit 0's n_seeds would pass (1 << 14) - 2."""
    g = genome()
    hits = [(a0 + 100, 0, 0, 0, 200, 200, 0, 100, 300)]
    for i in range(1, n):
        beg = 100 + i % 150
        ln = 20 + i * 7 % 30
        hits.append((a0 + beg, 0, 0, 0, ln, ln, 0, beg, beg + ln))
    return g[a0:a0 + lq], hits


def list_text(hits):
    return f"{len(hits)} " + " ".join(",".join(map(str, h)) for h in hits)


def parse_list(text):
    w = text.split()
    return [tuple(int(x) for x in h.split(",")) for h in w[1:]]


def run_left(chk, tmp_path, tasks):
    """bsw2_aln1_check left over [(a, b, q, r, bw, is_rev, codes, hits)] -> the lists after extend_left."""
    path = tmp_path / "left_own.txt"
    with open(path, "w") as f:
        for a, b, q, r, bw, is_rev, seq, hits in tasks:
            f.write("\t".join(map(str, (a, b, q, r, bw, is_rev, "".join(map(str, seq)), list_text(hits)))) + "\n")
    out = subprocess.run([chk, "left", os.path.join(GOLD, "g1m"), str(path)], check=True, stdout=subprocess.PIPE, text=True).stdout
    out = out.splitlines()
    assert len(out) == len(tasks)
    return [parse_list(o) for o in out]


def run_stages(chk, tmp_path, reads):
    """bsw2_aln1_check stages over reads -> per read the seven lists."""
    path = tmp_path / "reads_own.txt"
    write_reads(path, reads)
    out = subprocess.run([chk, "stages", os.path.join(GOLD, "g1m"), str(path)], check=True, stdout=subprocess.PIPE, text=True).stdout
    out = out.splitlines()
    assert len(out) == len(reads)
    return [[parse_list(x) for x in o.split("\t")[1:]] for o in out]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    from tools.make_bwasw_hits_golden import build
    return build(str(tmp_path_factory.mktemp("bsw2_aln1_programs")))


@needs_reference
def test_every_stage_equals_the_reference(programs, tmp_path):
    ref, chk = programs
    reads = random_reads(500, 91)
    write_reads(tmp_path / "reads.txt", reads)
    prefix = os.path.join(GOLD, "g1m")
    want = subprocess.run([ref, "stages", prefix, str(tmp_path / "reads.txt")], check=True, stdout=subprocess.PIPE, text=True).stdout
    got = subprocess.run([chk, "stages", prefix, str(tmp_path / "reads.txt")], check=True, stdout=subprocess.PIPE, text=True).stdout
    want, got = want.splitlines(), got.splitlines()
    assert len(want) == len(got) == len(reads)
    stages = ("t bw", "filter 0", "filter 1", "left 0", "left 1", "right 0", "right 1", "final")
    with_hits = 0
    for i, (w, g) in enumerate(zip(want, got)):
        for name, ws, gs in zip(stages, w.split("\t"), g.split("\t")):
            assert ws == gs, (i, name, reads[i][:12], len(reads[i][12]), ws[:300], gs[:300])
        with_hits += not w.endswith("\t0")
    assert with_hits > 250


@needs_reference
def test_n_seeds_ceiling_equals_the_reference(programs, tmp_path):
    ref, chk = programs
    seq, hits = nested_list()
    assert len(hits) == 16400
    with open(tmp_path / "left_ref.txt", "w") as f:
        f.write(f"1 3 5 2 50 0 {''.join(map(str, seq))} {list_text(hits)}\n")
    want = subprocess.run([ref, "left", os.path.join(GOLD, "g1m"), str(tmp_path / "left_ref.txt")], check=True, stdout=subprocess.PIPE,
                          text=True).stdout.splitlines()
    got = run_left(chk, tmp_path, [(1, 3, 5, 2, 50, 0, seq, hits)])[0]
    assert got == parse_list(want[0].split("\t")[1])
    assert max(h[3] for h in got) == 16382 and got[0][3] == 16382
