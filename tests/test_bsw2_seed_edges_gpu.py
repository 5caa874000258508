"""k_bsw2_seed where the first device test does not reach: reads whose suffix sort leaves the LDS
(above 2 047 bases) up to the longest the ABI takes, waves that run many tasks in one arena, lengths
mixed under one arena size, the four ways bwt_sa is served, small indexes with N-runs and repeats,
and hit lists beyond the output room of a launch.

Expected values are the reference's own where a golden file has them (tests/golden/bwasw), else
those of the host restatement (bsw2_seed_check run) on the same index files, which
tests/test_bsw2_core_host.py ties to the reference on the same generators.  Whole (all, narrow)
tuples are compared for equality.  A batch with a read above 2 049 bases has at most 48 tasks: the
arena follows the batch's longest read and every workgroup has one.
"""
import os
import random
import shutil

import pytest

from ibwa_amd import engine as E
from tests.test_bsw2_core_host import (SMALL_INDEXES, big_output_tasks, genome, random_tasks, run_checker,
                                       small_index_tasks)
from tests.test_bsw2_vectors import (GOLD, LONG_VECTORS, SMALL_VECTORS, build_checker, index_of, read_vectors)

pytestmark = pytest.mark.gpu
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
BATCH = 48


@pytest.fixture(scope="module")
def seed_engine(gpu_engine):
    gpu_engine.load_sa_files(os.path.join(GOLD, "g1m"))
    return gpu_engine


@pytest.fixture(scope="module")
def vectors():
    return read_vectors()


@pytest.fixture(scope="module")
def long_vectors():
    return read_vectors(LONG_VECTORS)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("bsw2_checker"))


@pytest.fixture(scope="module")
def small_engines():
    """One engine per small index, .bwt / .rbwt and .sa / .rsa from the files."""
    engines = {}
    try:
        for name in SMALL_INDEXES:
            engines[name] = E.Engine(0)
            engines[name].load_index_files(os.path.join(GOLD, name))
            engines[name].load_sa_files(os.path.join(GOLD, name))
        yield engines
    finally:
        for e in engines.values():
            e.close()


@pytest.fixture(scope="module")
def small_expected(checker, tmp_path_factory):
    """The host restatement's answers to the 400 tasks of each small index."""
    tmp = tmp_path_factory.mktemp("bsw2_small")
    out = {}
    for name in SMALL_INDEXES:
        tasks = small_index_tasks(name)
        out[name] = (tasks, run_checker(checker, os.path.join(GOLD, name), tasks, tmp / (name + ".txt")))
    return out


def _opt(opt):
    return {k: v for k, v in opt.items() if k != "adjust"}


def _task_opt(task):
    a, b, q, r, t, bw, z, is_ = task[:8]
    return dict(a=a, b=b, q=q, r=r, t=t, bw=bw, z=z, is_=is_)


def _by_optset(vectors):
    groups = {}
    for v in vectors:
        groups.setdefault(v[0], []).append(v)
    return groups


def _run_vectors(eng, vs):
    opt = vs[0][1]
    return eng.bwasw_seeds([v[4] for v in vs], [v[2] for v in vs], _opt(opt), adjust=bool(opt["adjust"]))


def _room(task):
    """The output records a single-task first launch plans for (engine_seed.hip)."""
    return 4096 + 64 + len(task[9]) * (2 + 2 * min(task[6], 8))


def test_long_vectors(seed_engine, long_vectors):
    """1 023 to 8 192 bases: the sort in LDS up to its 2 048 keys, the sort in the arena's cell area
    above, the 14-bit fields of its keys at 8 193 suffixes, the many rounds of a periodic read.  The
    default arena holds every one: the host's peak of live cells is below 9 per base here, the arena
    has 96, so a retry would mean the device needs far more than the host."""
    n, peak = 0, 0
    for name, vs in _by_optset(long_vectors).items():
        for at in range(0, len(vs), BATCH):
            part = vs[at:at + BATCH]
            got = _run_vectors(seed_engine, part)
            st = seed_engine.stats()
            longest = max(len(v[4]) for v in part)
            peak = max(peak, st.bsw2_arena_peak / longest)
            print(f"{name}[{at}:{at + len(part)}]: {st.ms_bsw2_seed:.1f} ms, arena peak {st.bsw2_arena_peak} bytes, "
                  f"{st.n_bsw2_retry} retried")
            for v, g in zip(part, got):
                assert g == v[5], (name, v[3], len(v[4]), v[2], g[0][:3], v[5][0][:3])
                n += 1
            assert st.n_bsw2_retry == 0
    assert n == len(long_vectors)


def test_sort_keys_must_fit_the_cell_area(seed_engine, long_vectors):
    """A read above 2 047 bases borrows the empty cell area for 2 P = 8 192 words of sort keys.  With 256
    cells that area has 4 096 words: the carve has to refuse, and the task comes back through the retry
    launch with the file's answer.  The count of retried tasks alone does not tell the guard from a
    later overflow of the cells, which 256 cells would also bring; what a missing guard would show is
    keys written into the next workgroup's arena, so every answer of the batch is compared."""
    for name, vs in _by_optset(long_vectors).items():
        part = [v for v in vs if len(v[4]) in (2047, 2049)]
        beyond_lds = sum(len(v[4]) >= 2048 for v in part)
        assert beyond_lds >= 8 and len(part) > beyond_lds
        seed_engine.set_option("seed_arena_cells", 256)
        try:
            got = _run_vectors(seed_engine, part)
            ss = seed_engine.seed_stats()
        finally:
            seed_engine.set_option("seed_arena_cells", 0)
        assert got == [v[5] for v in part], name
        assert ss["retried"] >= beyond_lds


@needs_gxx
def test_waves_run_many_tasks(seed_engine, checker, tmp_path):
    """One wave per CU and about five tasks per wave: short tasks follow 2 049-base ones in the same
    arena -- the node table the suffix sort borrowed for its ranks, sort keys left in the cell area,
    the free lists, the narrow hits and the top-2 table of the task before must not show."""
    opt = (1, 3, 5, 2, 20, 50, 2, 3)
    g = genome()
    rng = random.Random(41)
    tasks = [opt + x[8:] for x in random_tasks(1160, 40, max_len=150)]
    ln = 2049
    for i in range(40):
        if i % 2:
            a0 = rng.randrange(0, len(g) - ln)
            rate = (0.0, 0.02, 0.1)[i // 2 % 3]
            s = [(c + rng.randrange(1, 4)) & 3 if rng.random() < rate else c for c in g[a0:a0 + ln]]
        else:
            per = 1 + i // 2 % 4
            unit = [rng.randrange(4) for _ in range(per)]
            s = [unit[j % per] for j in range(ln)]
        strand = i // 4 % 2
        tasks.append(opt + (strand, s[::-1] if strand else s))
    random.Random(42).shuffle(tasks)
    n = len(tasks)
    want = run_checker(checker, os.path.join(GOLD, "g1m"), tasks, tmp_path / "tasks.txt")
    seqs, strands = [x[9] for x in tasks], [x[8] for x in tasks]
    seed_engine.set_option("seed_waves_per_cu", 1)
    try:
        got = seed_engine.bwasw_seeds(seqs, strands, _task_opt(tasks[0]), adjust=False)
        ss = seed_engine.seed_stats()
        back = seed_engine.bwasw_seeds(seqs[::-1], strands[::-1], _task_opt(tasks[0]), adjust=False)
    finally:
        seed_engine.set_option("seed_waves_per_cu", 8)
    assert 0 < ss["workgroups"] and ss["workgroups"] * 4 <= n  # every wave ran four tasks on average
    for i, (gi, w) in enumerate(zip(got, want)):
        assert gi == w, (i, len(seqs[i]), strands[i], gi[0][:3], w[0][:3])
    assert back == got[::-1]
    assert sum(bool(w[0]) for w in want) > n // 4


def test_mixed_lengths_under_one_arena_size(seed_engine, vectors, long_vectors):
    """The batch's longest read fixes the arena, every task carves its own layout under it: 1, 2, 17
    and 150 bases next to 2 049 and 8 192 give what each gives alone, and what the files hold."""
    short = [v for v in _by_optset(vectors)["defaults"] if len(v[4]) in (1, 2, 17, 150)][:32]
    assert {len(v[4]) for v in short} == {1, 2, 17, 150}  # of the tasks that are sent
    kinds = ("sub2", "chimera", "polyA", "period3exact")
    long_ = [v for v in _by_optset(long_vectors)["defaults"] if len(v[4]) in (2049, 8192) and v[3] in kinds and v[2] == 0]
    assert len(long_) == 8
    vs = short + long_
    random.Random(7).shuffle(vs)
    assert len(vs) <= BATCH
    got = _run_vectors(seed_engine, vs)
    assert got == [v[5] for v in vs]
    for v, g in zip(vs, got):
        assert _run_vectors(seed_engine, [v]) == [g], (v[3], len(v[4]))


def test_every_way_to_the_suffix_array(vectors):
    """bwt_sa through the .sa files' samples, through the full array after expand_sa (interval 1, row 0
    its own case), through the samples again under sa_walk, and through samples of another interval
    derived on the device: the same hits."""
    vs = _by_optset(vectors)["defaults"]
    assert len(vs) >= 50 and {len(v[4]) for v in vs} >= {1, 2, 8, 17, 30, 64, 100, 150, 400, 1000}
    want = [v[5] for v in vs]
    prefix = os.path.join(GOLD, "g1m")
    eng = E.Engine(0)
    try:
        eng.load_index_files(prefix)
        eng.load_sa_files(prefix)
        assert _run_vectors(eng, vs) == want
        eng.expand_sa()
        assert _run_vectors(eng, vs) == want
        eng.set_option("sa_walk", 1)
        assert _run_vectors(eng, vs) == want
    finally:
        eng.close()
    eng = E.Engine(0)
    try:
        eng.load_index_files(prefix)
        eng.derive_sa(8)
        assert _run_vectors(eng, vs) == want
    finally:
        eng.close()


def test_small_index_vectors(small_engines):
    """idx_quirks and csg: wide trie intervals, large expansions of rows, many narrow hits per cell."""
    vs = read_vectors(SMALL_VECTORS)
    n = 0
    for name, part in _by_optset(vs).items():
        got = _run_vectors(small_engines[index_of(name)], part)
        for v, g in zip(part, got):
            assert g == v[5], (name, len(v[4]), v[2], g[0][:3], v[5][0][:3])
            n += 1
    assert n == len(vs) >= 80


@needs_gxx
@pytest.mark.parametrize("name", SMALL_INDEXES)
def test_small_index_tasks_equal_the_host_restatement(small_engines, small_expected, name):
    """All 400 tasks of the generator, those with thousands of hits included, one option set a batch."""
    tasks, want = small_expected[name]
    groups = {}
    for i, x in enumerate(tasks):
        groups.setdefault(x[:8], []).append(i)
    assert len(groups) >= 25
    most = 0
    for ids in groups.values():
        got = small_engines[name].bwasw_seeds([tasks[i][9] for i in ids], [tasks[i][8] for i in ids],
                                              _task_opt(tasks[ids[0]]), adjust=False)
        for i, g in zip(ids, got):
            assert g == want[i], (name, i, tasks[i][:9], len(tasks[i][9]), g[0][:3], want[i][0][:3])
            most = max(most, len(g[0]) + len(g[1]))
    assert most > 4096


@needs_gxx
def test_output_room_alone(small_engines, small_expected):
    """A task whose hits pass the launch's output buffer ends with status 2 and its own count of rows;
    the retry launch makes that room."""
    eng = small_engines["idx_quirks"]
    tasks, want = small_expected["idx_quirks"]
    over = [i for i, x in enumerate(tasks) if len(want[i][0]) + len(want[i][1]) > _room(x)]
    assert len(over) >= 4 and 3 in over  # 3: 300 bases of T, z 3, is 50, t 5
    for i in over:
        x = tasks[i]
        assert eng.bwasw_seeds([x[9]], [x[8]], _task_opt(x), adjust=False) == [want[i]], (i, x[:9], len(x[9]))
        assert eng.stats().n_bsw2_retry == 1


@needs_gxx
def test_output_room_among_others(small_engines, checker, tmp_path):
    """Thirty such tasks among thirty ordinary reads: which of them run again follows the order the
    waves claim in, the answers do not."""
    eng = small_engines["idx_quirks"]
    prefix = os.path.join(GOLD, "idx_quirks")
    opt = (1, 3, 5, 2, 5, 50, 3, 50)
    rng = random.Random(43)
    cand = [opt + (0, [c] * ln) for ln in range(200, 185, -1) for c in (0, 3)]  # runs of A and of T
    plain = [opt + (k & 1, [rng.randrange(4) for _ in range(rng.randrange(5, 61))]) for k in range(30)]
    want = run_checker(checker, prefix, cand + plain, tmp_path / "tasks.txt")
    assert all(len(w[0]) + len(w[1]) > _room(x) for x, w in zip(cand, want[:30]))
    assert all(0 < len(w[0]) + len(w[1]) <= _room(x) for x, w in zip(plain, want[30:]))
    mixed = list(zip(cand + plain, want))
    random.Random(44).shuffle(mixed)
    got = eng.bwasw_seeds([x[9] for x, _ in mixed], [x[8] for x, _ in mixed], _task_opt(opt), adjust=False)
    assert eng.stats().n_bsw2_retry >= 1
    for k, ((x, w), g) in enumerate(zip(mixed, got)):
        assert g == w, (k, len(x[9]), x[8], len(g[0]), len(w[0]))


@needs_gxx
def test_output_far_beyond_the_planned_room(seed_engine, vectors, checker, tmp_path):
    """8 bases of A on g1m with t = 5 and is = 100000: 12 845 hits in the reference, where 16 times the
    planned room -- what the retry launch had before it took the task's own count -- is 5 632."""
    polya = [x for x in big_output_tasks() if x[9] == [0] * 8 and x[6] == 1 and x[7] == 100000]
    assert len(polya) == 1
    want = run_checker(checker, os.path.join(GOLD, "g1m"), polya, tmp_path / "polya.txt")
    assert len(want[0][0]) + len(want[0][1]) == 12845
    got = seed_engine.bwasw_seeds([polya[0][9]], [0], _task_opt(polya[0]), adjust=False)
    assert len(got[0][0]) + len(got[0][1]) == 12845
    assert got == want
    assert seed_engine.stats().n_bsw2_retry == 1
    # and the engine goes on as before
    vs = _by_optset(vectors)["defaults"]
    assert _run_vectors(seed_engine, vs) == [v[5] for v in vs]
    assert seed_engine.stats().n_bsw2_retry == 0
