"""bsw2_core.h against the reference's own bsw2_core on seeded random tasks (build container only).

The reference's sources are compiled where they lie into tmp_path with the harness main of
tools/make_bwasw_golden.py, next to tests/host/bsw2_seed_check.cpp; both run the same 2 000 tasks on
tests/golden/g1m -- lengths 1 to 600, z 1 to 4, is 0 to 6, t 8 to 40, bw 1 to 50, a 1 to 2, both
indexes -- and every hit is compared field for field (n_seeds is not part of the contract).  So are
150 tasks of 1 001 to 8 192 bases, 400 tasks on each of the small indexes idx_quirks and csg, and the
32 tasks whose lists run to thousands of hits; the device tests draw from the same generators.

With is == 0 and no hit above 0 the reference's bsw2_resolve_duphits allocates no hits and then reads
the score of the first (bwtsw2_core.c:273-274, :319-321): what it returns there is not defined, the
restatement returns nothing, and such a list is compared only when the reference returned nothing too.
"""
import os
import random
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFSRC = os.environ.get("IBWA_REFERENCE", "/root/reference")


_GENOMES = {}


def genome(name="g1m"):
    if name not in _GENOMES:
        sys.path.insert(0, ROOT)
        from tools.make_bwasw_golden import load_genome
        _GENOMES[name] = load_genome(name)
    return _GENOMES[name]


def random_tasks(n, seed, max_len=600, min_len=1):
    """[(a, b, q, r, t, bw, z, is, strand, codes)]: half the reads come from the genome, mutated.
    With min_len above 1 every read has min_len to max_len bases; else every fourth is below 40."""
    g = genome()
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ln = rng.randrange(min_len, max_len + 1) if i % 4 or min_len > 1 else rng.randrange(1, 40)
        if rng.random() < 0.5:
            a0 = rng.randrange(0, len(g) - ln)
            rate = rng.choice((0.0, 0.02, 0.05, 0.1))
            s = [(c + rng.randrange(1, 4)) & 3 if rng.random() < rate else c for c in g[a0:a0 + ln]]
            if ln > 20 and rng.random() < 0.3:
                p = rng.randrange(5, ln - 5)
                s = s[:p] + s[p + rng.randrange(1, 6):]
        elif rng.random() < 0.3:
            per = rng.randrange(1, 5)
            s = [(j % per + (rng.random() < 0.03)) & 3 for j in range(ln)]
        else:
            s = [rng.randrange(4) for _ in range(ln)]
        strand = rng.randrange(2)
        a = rng.randrange(1, 3)
        out.append((a, rng.randrange(1, 6), rng.randrange(1, 7), rng.randrange(1, 4), rng.randrange(8, 41),
                    rng.randrange(1, 51), rng.randrange(1, 5), rng.randrange(0, 7), strand, s[::-1] if strand else s))
    return out


def write_tasks(path, tasks, for_reference=False):
    with open(path, "w") as f:
        for a, b, q, r, t, bw, z, is_, strand, s in tasks:
            seq = "".join(map(str, s))
            if for_reference:
                f.write(f"{a} {b} {q} {r} {t} {bw} {z} {is_} 5.5 0 {strand} {seq}\n")
            else:
                f.write(f"{a} {b} {q} {r} {t} {bw} {z} {is_} {strand} {seq}\n")


SMALL_INDEXES = ("idx_quirks", "csg")
SMALL_IS = (0, 1, 3, 6, 50)
SMALL_T = (5, 10, 30)


def small_index_tasks(name, n=400, seed=31):
    """n tasks on a small committed index with N-runs and repeats (idx_quirks, csg): 1 to 300 bases;
    homopolymers, period 2 to 4, random and genome-derived reads; is from SMALL_IS, t from SMALL_T, z 1
    or 3, the other options bwasw's defaults with bw 50.  The first four are the 300-base homopolymers at
    z 3, is 50, t 5, whose hit lists pass the first launch's output room."""
    g = genome(name)
    rng = random.Random(f"{name}:{seed}")
    out = [(1, 3, 5, 2, 5, 50, 3, 50, 0, [c] * 300) for c in range(4)]
    while len(out) < n:
        ln = rng.choice((1, 2, 3, 17, 33, 64, 100, 150, 299, 300)) if rng.random() < 0.3 else rng.randrange(1, 301)
        kind = rng.randrange(4)
        if kind == 0:
            s = [rng.randrange(4)] * ln
        elif kind == 1:
            per = rng.randrange(2, 5)
            unit = [rng.randrange(4) for _ in range(per)]
            s = [(unit[j % per] + (rng.random() < 0.02)) & 3 for j in range(ln)]
        elif kind == 2:
            s = [rng.randrange(4) for _ in range(ln)]
        else:
            a0 = rng.randrange(0, len(g) - ln)
            rate = rng.choice((0.0, 0.02, 0.1))
            s = [(c + rng.randrange(1, 4)) & 3 if rng.random() < rate else c for c in g[a0:a0 + ln]]
        strand = rng.randrange(2)
        out.append((1, 3, 5, 2, rng.choice(SMALL_T), 50, rng.choice((1, 3)), rng.choice(SMALL_IS), strand,
                    s[::-1] if strand else s))
    return out


def big_output_tasks():
    """32 tasks on g1m whose intervals are expanded far beyond the output room a launch plans for:
    single-symbol and period-2 reads of 8, 17, 33 and 64 bases, t 5, is 1000 or 100000, z 1 or 3."""
    out = []
    for unit in ([0], [0, 1]):
        for ln in (8, 17, 33, 64):
            for is_ in (1000, 100000):
                for z in (1, 3):
                    out.append((1, 3, 5, 2, 5, 50, z, is_, 0, [unit[j % len(unit)] for j in range(ln)]))
    return out


def long_tasks(n=150, seed=78):
    """Random tasks of 1 001 to 8 192 bases on g1m: the reads whose suffix sort leaves the LDS."""
    return random_tasks(n, seed, max_len=8192, min_len=1001)


def parse_hits(text):
    """"n_all n_narrow hit..." of either program -> (all, narrow), lists of 8-tuples."""
    w = text.split()
    hits = [tuple(int(x) for x in h.split(",")) for h in w[2:]]
    assert len(hits) == int(w[0]) + int(w[1])
    return hits[:int(w[0])], hits[int(w[0]):]


def run_sliced(argv, tasks, path, for_reference=False, procs=8):
    """argv + [task file] over every procs-th task in a process of its own -> the output lines in task order."""
    running = []
    for k in range(min(procs, max(1, len(tasks)))):
        part = f"{path}.{k}"
        write_tasks(part, tasks[k::procs], for_reference)
        running.append(subprocess.Popen(argv + [part], stdout=subprocess.PIPE, text=True))
    out = [None] * len(tasks)
    for k, p in enumerate(running):
        lines = p.communicate()[0].splitlines()
        assert p.returncode == 0 and len(lines) == len(tasks[k::procs]), (argv[0], k, p.returncode)
        out[k::procs] = lines
    return out


def run_checker(exe, prefix, tasks, path):
    """bsw2_seed_check run over tasks -> [(all, narrow)]."""
    return [parse_hits(o.split("\t")[0]) for o in run_sliced([exe, "run", prefix], tasks, path)]


needs_reference = pytest.mark.skipif(
    not os.path.isdir(REFSRC) or shutil.which("gcc") is None or shutil.which("g++") is None,
    reason="needs the reference tree, gcc and g++")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    from tools.make_bwasw_golden import build
    return build(str(tmp_path_factory.mktemp("bsw2_programs")))


def compare(programs, tmp_path, index, tasks):
    """Both programs over tasks on tests/golden/<index>, field for field; returns the number of
    undefined all-lists (see the module's docstring) and the largest hit count of a task."""
    ref, chk = programs
    prefix = os.path.join(GOLD, index)
    with ThreadPoolExecutor(2) as pool:  # both programs at once, each over its slices
        want = pool.submit(run_sliced, [ref, prefix], tasks, str(tmp_path / "ref.txt"), True)
        got = pool.submit(run_sliced, [chk, "run", prefix], tasks, str(tmp_path / "own.txt"))
        want, got = want.result(), got.result()
    assert len(want) == len(got) == len(tasks)
    undefined = most = 0
    for i, (w, g, task) in enumerate(zip(want, got, tasks)):
        w, g = w.split("\t")[1], g.split("\t")[0]
        if w != g and task[7] == 0 and g.split()[0] == "0":
            # the undefined read described above: drop the reference's all-list, compare the rest
            wn = w.split()
            w = " ".join(["0", wn[1]] + wn[2 + int(wn[0]):])
            undefined += 1
        assert w == g, (i, task[:9], len(task[9]), w[:300], g[:300])
        most = max(most, int(g.split()[0]) + int(g.split()[1]))
    return undefined, most


@needs_reference
def test_restatement_equals_reference(programs, tmp_path):
    tasks = random_tasks(2000, 77)
    undefined, _ = compare(programs, tmp_path, "g1m", tasks)
    assert undefined < len(tasks) // 10


@needs_reference
def test_long_reads_equal_reference(programs, tmp_path):
    tasks = long_tasks()
    assert len(tasks) == 150 and all(1001 <= len(x[9]) <= 8192 for x in tasks)
    assert sum(len(x[9]) > 2047 for x in tasks) > 100  # most sort their suffixes outside the LDS
    undefined, _ = compare(programs, tmp_path, "g1m", tasks)
    assert undefined < len(tasks) // 10


@needs_reference
@pytest.mark.parametrize("index", SMALL_INDEXES)
def test_small_indexes_equal_reference(programs, tmp_path, index):
    tasks = small_index_tasks(index)
    assert len(tasks) == 400
    undefined, most = compare(programs, tmp_path, index, tasks)
    assert undefined < len(tasks) // 5  # is == 0 is a fifth of the tasks
    assert most > 4096  # some lists pass the output room of a single-task launch


@needs_reference
def test_big_outputs_equal_reference(programs, tmp_path):
    tasks = big_output_tasks()
    assert len(tasks) == 32
    _, most = compare(programs, tmp_path, "g1m", tasks)
    assert most > 5632  # beyond 16 times the planned room of an 8-base task: what the retry launch had
    # the case the engine refused before the retry launch took the task's own count
    ref, chk = programs
    polya8 = [x for x in tasks if x[9] == [0] * 8 and x[6] == 1 and x[7] == 100000]
    got = run_checker(chk, os.path.join(GOLD, "g1m"), polya8, tmp_path / "one.txt")
    assert len(got[0][0]) + len(got[0][1]) == 12845
