"""k_bsw2_extend through Engine.bwasw_hits and Engine.bwasw_extend_left on the device: the golden vectors
of tests/golden/bwasw/aln1_vectors.tsv.gz and left_vectors.tsv.gz, independence of batch order and of the
number of waves, random reads and the 16 400-hit list against the host restatement, a band wide enough
to put the eh ring into HBM, a batch that mixes 17 and 8 192 bases, the error cases, and the stats.
Every field of every hit is compared as an integer."""
import os
import random
import shutil

import pytest

from ibwa_amd import engine as E
from tests.test_bsw2_aln1_host import nested_list, random_reads, run_left, run_stages
from tests.test_bsw2_aln1_vectors import GOLD, build_checker, draw, read_aln1_vectors, read_left_vectors
from tests.test_bsw2_vectors import read_vectors

pytestmark = pytest.mark.gpu

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def load_g1m(eng):
    prefix = os.path.join(GOLD, "g1m")
    eng.load_index_files(prefix)
    eng.load_sa_files(prefix)
    with open(prefix + ".ann") as f:
        l_pac = int(f.readline().split()[0])
    with open(prefix + ".pac", "rb") as f:
        pac = f.read()[:(l_pac + 3) // 4]
    eng.load_pac([pac], [l_pac])
    return l_pac


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    load_g1m(e)
    yield e
    e.close()


@pytest.fixture(scope="module")
def vectors():
    return read_aln1_vectors()


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("bsw2_aln1_checker"))


def _opt(opt):
    return {k: v for k, v in opt.items() if k != "adjust"}


def _by_optset(vectors):
    groups = {}
    for v in vectors:
        groups.setdefault(v[0], []).append(v)
    return groups


def _hits(eng, vs):
    opt = vs[0][1]
    return eng.bwasw_hits([v[5] for v in vs], [v[2] for v in vs], _opt(opt), adjust=bool(opt["adjust"]), u=[draw(v[4]) for v in vs])


def _stats_add_up(eng, n_hits):
    st = eng.bwasw_hits_stats()
    assert st["extended"] + st["contained"] + st["discarded"] + st["skipped"] == n_hits, st
    return st


def test_every_aln1_vector(eng, vectors):
    n = 0
    for name, vs in _by_optset(vectors).items():
        got = _hits(eng, vs)
        for v, g in zip(vs, got):
            assert g == v[6], (name, v[3], len(v[5]), v[2], g[:3], v[6][:3])
            n += 1
        # the left launch saw the narrow lists that came through the chain filter
        st = _stats_add_up(eng, sum(len(v[7][0]) + len(v[7][1]) for v in vs))
        assert st["tasks"] == 2 * len(vs)
    assert n == len(vectors) and n >= 400


def _left(eng, vs):
    return eng.bwasw_extend_left([v[7] for v in vs], [v[4] for v in vs], [v[5] for v in vs], [v[8] for v in vs],
                                 dict(a=vs[0][0], b=vs[0][1], q=vs[0][2], r=vs[0][3]))


def test_every_left_vector(eng):
    vs = read_left_vectors()
    groups = {}
    for v in vs:
        groups.setdefault(v[:4], []).append(v)
    n = 0
    for part in groups.values():
        got = _left(eng, part)
        for v, g in zip(part, got):
            assert g == v[9], (v[6], len(v[8]), g[:3], v[9][:3])
            n += 1
        st = _stats_add_up(eng, sum(len(v[8]) for v in part))
        assert st["windows"] == sum((len(v[8]) + 63) // 64 for v in part)
    assert n == len(vs) and n >= 150
    # lists of more than one window, contained hits found before any DP, and speculative runs dropped
    big = [v for v in vs if len(v[8]) > 128]
    assert big
    _left(eng, big)
    st = eng.bwasw_hits_stats()
    assert st["contained"] > 0 and st["discarded"] > 0 and st["extended"] > 0


def test_batch_order_does_not_matter(eng, vectors):
    vs = [v for v in _by_optset(vectors)["defaults"] if len(v[5]) <= 1000]
    order = list(range(len(vs)))
    random.Random(7).shuffle(order)
    a = _hits(eng, vs)
    b = _hits(eng, [vs[i] for i in order])
    assert [a[i] for i in order] == b
    assert a == [v[6] for v in vs]


def test_one_wave_per_cu_equals_the_default(eng):
    """Few waves, so that each runs many lists one after another in the same scratch: nothing may carry
    over.  The left vectors' 204 lists go round three times, more tasks than one wave per CU."""
    vs = [v for v in read_left_vectors() if v[:4] == (1, 3, 5, 2)] * 3
    want = _left(eng, vs)
    eng.set_option("bsw2_ext_waves_per_cu", 1)
    try:
        got = _left(eng, vs)
    finally:
        eng.set_option("bsw2_ext_waves_per_cu", 0)
    assert got == want == [v[9] for v in vs]


@needs_gxx
def test_random_reads_equal_the_host_restatement(eng, checker, tmp_path):
    reads = random_reads(200, 17, min_len=30, max_len=400)
    reads = [reads[i - i % 25][:10] + r[10:] for i, r in enumerate(reads)]  # 25 reads share an option set: one call each
    want = run_stages(checker, tmp_path, reads)
    groups = {}
    for i, r in enumerate(reads):
        groups.setdefault(r[:10], []).append(i)
    assert len(groups) == 8
    for key, idx in groups.items():
        a, b, q, r, t, bw, z, is_, t_seeds, mask = key
        got = eng.bwasw_hits([reads[i][12] for i in idx], [reads[i][10] for i in idx],
                             dict(a=a, b=b, q=q, r=r, t=t, bw=bw, z=z, is_=is_, t_seeds=t_seeds, mask_level=mask), adjust=False,
                             u=[draw(reads[i][11]) for i in idx])
        for i, g in zip(idx, got):
            assert g == want[i][6], (i, reads[i][:12], len(reads[i][12]), g[:3], want[i][6][:3])
    assert sum(1 for w in want if w[6]) > 100


@needs_gxx
def test_n_seeds_ceiling_equals_the_host_restatement(eng, checker, tmp_path):
    seq, hits = nested_list()
    want = run_left(checker, tmp_path, [(1, 3, 5, 2, 50, 0, seq, hits)])[0]
    got = eng.bwasw_extend_left([seq], [50], [0], [hits])[0]
    assert got == want
    assert got[0][3] == 16382 and len(got) == 16400
    st = _stats_add_up(eng, 16400)
    assert st["windows"] == 257 and st["contained"] >= 16400 - 64


@needs_gxx
def test_wide_band_keeps_the_ring_in_hbm(eng, checker, tmp_path):
    """A band above 79 makes the eh ring wider than the 160 words a lane has in LDS: the launch then
    chooses per lane between LDS (short windows) and the wave's HBM scratch.  Both extensions, against
    the host restatement."""
    vs = [v for v in read_left_vectors() if v[:4] == (1, 3, 5, 2) and len(v[7]) >= 300 and v[8]]
    assert len(vs) >= 20
    want = run_left(checker, tmp_path, [(1, 3, 5, 2, 200, v[5], v[7], v[8]) for v in vs])
    got = eng.bwasw_extend_left([v[7] for v in vs], [200] * len(vs), [v[5] for v in vs], [v[8] for v in vs])
    assert got == want
    assert eng.bwasw_hits_stats()["extended"] > 0
    key = (1, 3, 5, 2, 30, 120, 1, 3, 5, 0.5)
    reads = [key + r[10:] for r in random_reads(24, 23, min_len=300, max_len=500)]
    want = run_stages(checker, tmp_path, reads)
    got = eng.bwasw_hits([r[12] for r in reads], [r[10] for r in reads], dict(t=30, bw=120), adjust=False,
                         u=[draw(r[11]) for r in reads])
    assert got == [w[6] for w in want]
    assert sum(1 for g in got if g) >= 8


def test_mixed_lengths_equal_each_alone(eng, vectors):
    """17 and 8 192 bases in one batch: the scratch is sized for the longest, the band follows each read."""
    short = [v for v in vectors if len(v[5]) == 17 and v[0] == "defaults"][:3]
    long_ = [v for v in vectors if len(v[5]) == 8192][:1]
    assert short and long_ and long_[0][0] == "defaults"
    vs = short + long_ + short[::-1]
    got = _hits(eng, vs)
    assert got == [_hits(eng, [v])[0] for v in vs] == [v[6] for v in vs]


def test_errors_and_empty(eng):
    assert eng.bwasw_hits([], []) == []
    assert eng.bwasw_extend_left([], [], [], []) == []
    assert eng.bwasw_extend_left([[0, 1, 2, 3]], [50], [0], [[]]) == [[]]
    with pytest.raises(E.IbwaError, match=r"task 1: seq\[0\] = 7"):
        eng.bwasw_hits([[0, 1], [7]], [0, 1])
    with pytest.raises(E.IbwaError, match="task 0: is_rev 3"):
        eng.bwasw_hits([[0, 1]], [3])
    with pytest.raises(E.IbwaError, match="t_seeds -1 < 0"):
        eng.bwasw_hits([[0, 1]], [0], {"t_seeds": -1})
    with pytest.raises(E.IbwaError, match="mask_level 1.5 outside"):
        eng.bwasw_hits([[0, 1]], [0], {"mask_level": 1.5})
    with pytest.raises(E.IbwaError, match="task 1: u 1 outside"):
        eng.bwasw_hits([[0, 1], [2, 3]], [0, 0], u=[0.5, 1.0])
    with pytest.raises(E.IbwaError, match="z 0 < 1"):
        eng.bwasw_hits([[0, 1]], [0], {"z": 0})
    E.bsw2_aln1_check([[0, 1]], [0], u=[0.25])  # the checks alone, no device
    with pytest.raises(E.IbwaError, match="task 0: u -0.5 outside"):
        E.bsw2_aln1_check([[0, 1]], [0], u=[-0.5])
    with pytest.raises(E.IbwaError, match=r"task 0: hit 0: beg 9 outside \[0, 4\]"):
        eng.bwasw_extend_left([[0, 1, 2, 3]], [50], [0], [[(100, 0, 0, 0, 2, 2, 0, 9, 11)]])
    with pytest.raises(E.IbwaError, match="task 0: hit 0: k .* past l_pac or G 0"):
        eng.bwasw_extend_left([[0, 1, 2, 3]], [50], [0], [[(100, 0, 0, 0, 2, 0, 0, 1, 3)]])
    with pytest.raises(E.IbwaError, match="task 0: bw 0 < 1"):
        eng.bwasw_extend_left([[0, 1, 2, 3]], [0], [0], [[]])
    bare = E.Engine(0)
    try:
        prefix = os.path.join(GOLD, "g1m")
        with pytest.raises(E.IbwaError, match="ibwa error -3"):
            bare.bwasw_hits([[0, 1, 2]], [0])
        bare.load_index_files(prefix)
        bare.load_sa_files(prefix)
        with pytest.raises(E.IbwaError, match="ibwa error -3.*ibwa_ctx_load_pac"):
            bare.bwasw_hits([[0, 1, 2]], [0])
        with pytest.raises(E.IbwaError, match="ibwa error -3.*ibwa_ctx_load_pac"):
            bare.bwasw_extend_left([[0, 1, 2, 3]], [50], [0], [[(100, 0, 0, 0, 2, 2, 0, 1, 3)]])
    finally:
        bare.close()


def test_seeding_still_answers_as_before(eng, vectors):
    """The same engine, after the calls above: bwasw_seeds gives the seed vectors."""
    _hits(eng, _by_optset(vectors)["defaults"][:20])
    vs = [v for v in read_vectors() if v[0] == "defaults"][:60]
    opt = {k: v for k, v in vs[0][1].items() if k != "adjust"}
    assert eng.bwasw_seeds([v[4] for v in vs], [v[2] for v in vs], opt) == [v[5] for v in vs]
