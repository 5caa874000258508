"""k_bsw2_seed through Engine.bwasw_seeds on the device: the golden vectors, independence of batch
order, the arena retry, random tasks against the host restatement, and the error and empty cases."""
import os
import random
import shutil
import subprocess

import pytest

from ibwa_amd import engine as E
from tests.test_bsw2_core_host import random_tasks, write_tasks
from tests.test_bsw2_vectors import GOLD, build_checker, read_vectors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seed_engine(gpu_engine):
    gpu_engine.load_sa_files(os.path.join(GOLD, "g1m"))
    return gpu_engine


@pytest.fixture(scope="module")
def vectors():
    return read_vectors()


def _opt(opt):
    return {k: v for k, v in opt.items() if k != "adjust"}


def _by_optset(vectors):
    groups = {}
    for v in vectors:
        groups.setdefault(v[0], []).append(v)
    return groups


def test_every_vector(seed_engine, vectors):
    n = 0
    for name, vs in _by_optset(vectors).items():
        opt = vs[0][1]
        got = seed_engine.bwasw_seeds([v[4] for v in vs], [v[2] for v in vs], _opt(opt), adjust=bool(opt["adjust"]))
        for v, g in zip(vs, got):
            assert g == v[5], (name, v[3], len(v[4]), v[2], g[0][:3], v[5][0][:3])
            n += 1
    assert n == len(vectors)
    assert seed_engine.stats().ms_bsw2_seed > 0


def test_batch_order_does_not_matter(seed_engine, vectors):
    """One wave runs many tasks one after another in one arena: nothing may carry over."""
    vs = _by_optset(vectors)["defaults"]
    opt = _opt(vs[0][1])
    order = list(range(len(vs)))
    random.Random(5).shuffle(order)
    seqs, strands = [v[4] for v in vs], [v[2] for v in vs]
    a = seed_engine.bwasw_seeds(seqs, strands, opt)
    b = seed_engine.bwasw_seeds([seqs[i] for i in order], [strands[i] for i in order], opt)
    assert [a[i] for i in order] == b
    assert a == [v[5] for v in vs]
    # one wave per CU: still more waves than this batch has tasks, so each claims one task at most;
    # waves that run many tasks are the matter of tests/test_bsw2_seed_edges_gpu.py
    seed_engine.set_option("seed_waves_per_cu", 1)
    try:
        assert seed_engine.bwasw_seeds(seqs[::-1], strands[::-1], opt) == a[::-1]
    finally:
        seed_engine.set_option("seed_waves_per_cu", 8)


def test_small_arena_retries(seed_engine, vectors):
    """An arena of 256 cells overflows for the larger tasks -- an ordinary status, every store is checked
    against the arena -- and the engine runs them again in a larger one: same answers."""
    vs = _by_optset(vectors)["b5q2r1z10"]
    opt = _opt(vs[0][1])
    seed_engine.set_option("seed_arena_cells", 256)
    try:
        got = seed_engine.bwasw_seeds([v[4] for v in vs], [v[2] for v in vs], opt)
        st, ss = seed_engine.stats(), seed_engine.seed_stats()
    finally:
        seed_engine.set_option("seed_arena_cells", 0)
    assert got == [v[5] for v in vs]
    assert 0 < st.n_bsw2_retry < len(vs) and ss["retried"] == st.n_bsw2_retry
    assert st.bsw2_arena_peak > 256 * 64
    seed_engine.bwasw_seeds([v[4] for v in vs], [v[2] for v in vs], opt)
    assert seed_engine.stats().n_bsw2_retry == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_random_tasks_equal_the_host_restatement(seed_engine, tmp_path):
    exe = build_checker(tmp_path)
    rng = random.Random(11)
    tasks = []
    for g in range(6):  # one option set per batch
        a, b, q, r = rng.randrange(1, 3), rng.randrange(1, 6), rng.randrange(1, 7), rng.randrange(1, 4)
        t, bw, z, is_ = rng.randrange(8, 41), rng.randrange(1, 51), rng.randrange(1, 5), rng.randrange(0, 7)
        tasks += [(a, b, q, r, t, bw, z, is_) + x[8:] for x in random_tasks(50, 100 + g, max_len=300)]
    write_tasks(tmp_path / "tasks.txt", tasks)
    out = subprocess.run([exe, "run", os.path.join(GOLD, "g1m"), str(tmp_path / "tasks.txt")], check=True,
                         stdout=subprocess.PIPE, text=True).stdout.splitlines()
    assert len(out) == len(tasks) == 300
    for g in range(6):
        part = tasks[g * 50:(g + 1) * 50]
        a, b, q, r, t, bw, z, is_ = part[0][:8]
        got = seed_engine.bwasw_seeds([x[9] for x in part], [x[8] for x in part],
                                      dict(a=a, b=b, q=q, r=r, t=t, bw=bw, z=z, is_=is_), adjust=False)
        for i, gi in enumerate(got):
            w = out[g * 50 + i].split("\t")[0].split()
            hits = [tuple(int(x) for x in h.split(",")) for h in w[2:]]
            assert gi == (hits[:int(w[0])], hits[int(w[0]):]), (g, i, part[i][:9], len(part[i][9]))


def test_errors_and_empty(seed_engine):
    assert seed_engine.bwasw_seeds([], []) == []
    with pytest.raises(E.IbwaError, match=r"task 1: seq\[0\] = 7"):
        seed_engine.bwasw_seeds([[0, 1], [7]], [0, 1])
    with pytest.raises(E.IbwaError, match="task 0: strand 3"):
        seed_engine.bwasw_seeds([[0, 1]], [3])
    with pytest.raises(E.IbwaError, match="z 0 < 1"):
        seed_engine.bwasw_seeds([[0, 1]], [0], {"z": 0})
    bare = E.Engine(0)
    try:
        with pytest.raises(E.IbwaError, match="ibwa error -3"):
            bare.bwasw_seeds([[0, 1, 2]], [0])
        bare.load_index_files(os.path.join(GOLD, "g1m"))
        with pytest.raises(E.IbwaError, match="ibwa error -3.*suffix array"):
            bare.bwasw_seeds([[0, 1, 2]], [1])
    finally:
        bare.close()
