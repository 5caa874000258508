"""k_width after a reset (aln.hip; engine options width_tab and width_rec_stage).

* width_tab 2: after every reset (empty interval or N) a chain takes its next steps, down to depth
  gap_tab_k + 1, from the level tables (one 8 B entry per step) instead of Occ steps.  The width rows
  k_width wrote must be byte-equal to those of width_tab 1 (leading steps only) and 0 (Occ steps
  only, the path the golden .sai tests pin), whatever width_jump and gap_lw are.  Row equality also
  sees a bid that came out too small, which the hits cannot.
* width_rec_stage 1: a block's compact records are built in LDS and stored whole.  The records must be
  byte-equal to those the lanes store themselves (0), at read counts around the wave and block sizes.
* the hits of the whole batch equal the oracle's with the new defaults.
* ibwa_run_stats_t.n_width_tab_steps counts the table steps after resets: 0 with width_tab 1, and
  with 2 the count that the rows' bids and the read lengths give.

The batch: the golden 100 bp reads plus reads cut from the 1 Mb fixture's own sequence with lengths on
both sides of the table depth (7 and 9 at gap_tab_k 6 and 8), of the 16-step blocks and of the 32 bp
seed; one substitution or one N at walk positions around those boundaries; two substitutions closer
than the table depth (a reset inside the table steps); a k-mer absent from the fixture (an empty table
entry) at the start and after an N; a k-mer that occurs once right after an N (one row inside the
table steps: the hand-over to the text steps when width_jump has the text resident).
"""
import os

import numpy as np
import pytest

import oracle
from ibwa_amd import engine as E
from tests.test_scale_properties import eopt

pytestmark = pytest.mark.gpu

SEED_LEN = 32  # gap_init_opt's -l
LENGTHS = (100, 1, 6, 7, 8, 9, 10, 15, 16, 17, 31, 32, 33)


def _rc(x):
    return (3 - x[::-1]).astype(np.uint8)


def _kmer_counts(g, k):
    """occurrences of every k-mer code (first base most significant) in g"""
    code = np.zeros(len(g) - k + 1, np.int64)
    for j in range(k):
        code = code * 4 + g[j:len(g) - k + 1 + j]
    return code, np.bincount(code, minlength=4 ** k)


def _decode(code, k):
    return np.array([(code >> (2 * (k - 1 - j))) & 3 for j in range(k)], np.uint8)


def _absent_kmer(g):
    """the shortest string (k >= 8) that occurs in no orientation in the fixture"""
    for k in (8, 9, 10, 11):
        both = np.concatenate([g, _rc(g)])
        _, cnt = _kmer_counts(both, k)  # the few k-mers across the join only make the test stricter
        for code in np.flatnonzero(cnt == 0):
            x = _decode(int(code), k)
            rev = int(sum(int(b) << (2 * (k - 1 - j)) for j, b in enumerate(x[::-1])))
            if cnt[rev] == 0:
                return x
    raise AssertionError("no absent k-mer up to 11")


def _unique_site(g, k):
    """a position whose k-mer occurs once in the fixture, away from the ends"""
    code, cnt = _kmer_counts(g, k)
    pos = np.flatnonzero(cnt[code] == 1)
    pos = pos[(pos > 200) & (pos < len(g) - 200)]
    assert pos.size
    return int(pos[0])


def _crafted(g, tdeps=(7, 9)):
    """reads as walk-order code arrays (bwa_seq_t.seq: the read reversed); 4 stands for N"""
    rng = np.random.default_rng(11)
    out = []

    def cut(L):
        a = int(rng.integers(1000, len(g) - 1000))
        return g[a:a + L][::-1].copy()

    for L in LENGTHS:
        out.append(cut(L))
    spots = {0, 1, 15, 16}
    for t in tdeps:
        spots |= {t - 1, t, t + 1}
    for L in (17, 33, 100):
        for p in sorted(spots | {L - 1}):
            if p >= L:
                continue
            s = cut(L)
            s[p] = (s[p] + 1 + rng.integers(0, 3)) & 3
            out.append(s)
            s = cut(L)
            s[p] = 4
            out.append(s)
    # two substitutions fewer than the table depth apart, past the depth at which a prefix is unique
    for gap in (1, 3, 5, 6, 8):
        for p in (14, 20, 40):
            s = cut(100)
            s[p] ^= 1
            s[p + gap] ^= 2
            out.append(s)
    # an empty table entry: at the start, and inside the table steps after an N
    x = _absent_kmer(g)
    for y in (x, x[::-1].copy()):
        s = cut(100)
        s[:len(y)] = y
        out.append(s)
        s = cut(100)
        s[20] = 4
        s[21:21 + len(y)] = y
        out.append(s)
        s = cut(100)
        s[20] = 4
        s[23:23 + len(y)] = y
        out.append(s)
    # one row inside the table steps: a 9-mer that occurs once right after an N, in both walk
    # directions and on both strands
    for k in (9,):
        a = _unique_site(g, k)
        for src in (g, None):
            w = g[a - 40:a + k + 40]
            if src is None:
                w = _rc(w)
            for s in (w.copy(), w[::-1].copy()):
                q = s.copy()
                q[39] = 4
                out.append(q)
                q = s.copy()
                q[40 + k] = 4
                out.append(q)
    return out


def _encode(walks):
    lens = np.array([len(w) for w in walks], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    return np.concatenate(walks).astype(np.uint8), offs, lens


@pytest.fixture(scope="module")
def batch(golden_dir):
    g, _ = oracle.read_pac(os.path.join(golden_dir, "g1m"))
    opt, _ = oracle.parse_aln_args([])
    recs = oracle.read_fastq_records(os.path.join(golden_dir, "reads_r100.fq"))
    crafted = _crafted(g)
    recs = recs[:600 - len(crafted)]
    gs, go, gl = oracle.encode_reads(recs, opt.mode, opt.trim_qual)
    walks = crafted + [gs[int(o):int(o) + int(n)] for o, n in zip(go, gl)]
    assert len(walks) <= 600
    return _encode(walks)


@pytest.fixture(scope="module")
def eng(golden_dir):
    e = E.Engine(0)
    e.load_index_files(os.path.join(golden_dir, "g1m"))
    e.set_option("diag_width", 1)
    yield e
    e.close()


def _run(eng, batch, argv=(), **opts):
    """one run under the options; (n_aln, alns bytes, rows, records, stats)"""
    base = {"width_tab": 2, "width_rec_stage": 1, "width_jump": 1, "gap_lw": 1, "gap_tab_k": 8}
    base.update(opts)
    for k, v in base.items():
        eng.set_option(k, v)
    _, e = eopt(list(argv))
    n_aln, alns = eng.aln(*batch, e)
    st = eng.stats()
    assert st.path == 2
    return n_aln.copy(), alns.tobytes(), eng.width_rows(), eng.width_records(), st


def _chains(rows, lens, wlen1):
    """per read its four chains' (entries, length): the two full-length chains, then the seed's"""
    for r, L in enumerate(lens):
        L = int(L)
        yield r, rows[r, 0:L + 1], L
        yield r, rows[r, wlen1:wlen1 + L + 1], L
        if L > SEED_LEN:
            s0 = 2 * wlen1
            yield r, rows[r, s0:s0 + SEED_LEN + 1], SEED_LEN
            yield r, rows[r, s0 + SEED_LEN + 1:s0 + 2 * SEED_LEN + 2], SEED_LEN


def _resets(ent, L):
    """the positions at which the chain's interval was reset (its bid grows)"""
    return np.flatnonzero(np.diff(np.concatenate([[0], ent[:L, 1].astype(np.int64)])) > 0)


def _chain_steps(ent, L, tdep):
    """The table steps after resets that a chain's row implies when it takes no text steps: a reset at
    position i starts them at i + 1; they end after tdep steps without a reset, or with the chain.
    The leading table steps hold no reset and are not counted."""
    reset = np.zeros(L, bool)
    reset[_resets(ent, L)] = True
    n, m3, d = 0, False, 0
    for i in range(L):
        if m3:
            n += 1
            if reset[i]:
                d = 0
            else:
                d += 1
                m3 = d < tdep
        elif reset[i]:
            m3, d = True, 0
    return n


def _steps_from_rows(rows, lens, wlen1, tdep):
    """_chain_steps summed per read"""
    total = np.zeros(len(lens), np.int64)
    for r, ent, L in _chains(rows, lens, wlen1):
        total[r] += _chain_steps(ent, L, tdep)
    return total


@pytest.mark.parametrize("tab_k", [6, 8])
@pytest.mark.parametrize("gap_lw", [0, 1])
def test_width_rows_equal(eng, batch, tab_k, gap_lw):
    wlen1 = int(batch[2].max()) + 1
    ref = None
    for wj in (2, 1, 0):  # 2 first: it derives the text that 1 then finds resident
        for wt in (0, 1, 2):
            n_aln, alns, rows, _, st = _run(eng, batch, width_jump=wj, width_tab=wt, gap_lw=gap_lw, gap_tab_k=tab_k)
            assert rows.shape[0] == len(batch[2]) and rows.shape[1] >= 2 * wlen1
            assert (st.n_width_tab_steps > 0) == (wt == 2)
            if ref is None:
                ref = (n_aln, alns, rows)
                # the rows are there: every chain ends with {0, bid + 1}
                for r, ent, L in _chains(rows, batch[2], wlen1):
                    assert ent[L, 0] == 0 and ent[L, 1] >= 1, r
            else:
                assert (n_aln == ref[0]).all() and alns == ref[1], (wj, wt)
                bad = np.flatnonzero((rows != ref[2]).any(axis=(1, 2)))
                assert bad.size == 0, (wj, wt, bad[:8])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 300])
def test_records_equal(eng, batch, n):
    seq, off, lens = batch
    # the crafted reads of mixed lengths first, so every count holds them
    sub = (seq[:int(off[n - 1]) + int(lens[n - 1])], off[:n], lens[:n])
    got = {}
    for stage in (0, 1):
        n_aln, alns, rows, rec, _ = _run(eng, sub, width_rec_stage=stage)
        assert rec.shape[0] == n and rec.shape[1] > 0  # the first pass ran on the records
        got[stage] = (n_aln, alns, rows, rec)
    assert ((got[0][3][:, 0] & 0xFFFF) == lens[:n]).all()  # word 0 holds the length
    bad = np.flatnonzero((got[0][3] != got[1][3]).any(axis=1))
    assert bad.size == 0, bad[:8]
    assert (got[0][2] == got[1][2]).all()
    assert (got[0][0] == got[1][0]).all() and got[0][1] == got[1][1]


@pytest.mark.parametrize("argv", [(), ("-n", "3", "-o", "2", "-e", "3")])
def test_hits_equal_oracle(eng, batch, oracle_index, argv):
    o, _ = eopt(list(argv))
    rn, ra, _ = oracle.cal_sa_reg_gap(oracle_index[0], oracle_index[1], *batch, o, n_threads=8)
    for opts in ({"gap_tab_k": -1}, {"gap_tab_k": 6}):
        n_aln, alns, _, _, st = _run(eng, batch, argv, **opts)
        assert st.n_width_tab_steps > 0
        assert (n_aln == rn).all()
        assert alns == ra.tobytes()


@pytest.mark.parametrize("tab_k", [6, 8])
def test_counter(eng, batch, golden_dir, tab_k):
    tdep = tab_k + 1
    wlen1 = int(batch[2].max()) + 1
    # Occ steps only besides the tables (no text steps), so the rows give the count
    _, _, rows, _, st = _run(eng, batch, width_jump=0, gap_tab_k=tab_k)
    # the counter sums the run's k_width launches: a read handed on without its search state (pass 1)
    # has its widths computed once more
    ids, ps = eng.retry_info()
    assert ((ps == 1) | (ps == 4)).all()
    per_read = _steps_from_rows(rows, batch[2], wlen1, tdep)
    assert st.n_width_tab_steps == per_read.sum() + per_read[ids[ps == 1]].sum()
    _, _, _, _, st1 = _run(eng, batch, width_jump=0, gap_tab_k=tab_k, width_tab=1)
    assert st1.n_width_tab_steps == 0
    # One substitution at walk position p of a read no longer than the seed (two chains).  The chain
    # of the strand the read was cut from resets at p and nowhere else (a 20-symbol prefix of the 1 Mb
    # fixture is unique), so it takes min(tdep, L - 1 - p) table steps; the other strand's chain resets
    # wherever its string stops existing, and its row gives its steps.
    g, _ = oracle.read_pac(os.path.join(golden_dir, "g1m"))
    rng = np.random.default_rng(5)
    cases = ((32, 20), (31, 28), (32, 31), (30, 22), (32, 24))
    walks = []
    for L, p in cases:
        a = int(rng.integers(1000, len(g) - 1000))
        s = g[a:a + L][::-1].copy()
        s[p] ^= 2
        walks.append(s)
    b = _encode(walks)
    _, _, rows, _, st = _run(eng, b, width_jump=0, gap_tab_k=tab_k)
    ids, ps = eng.retry_info()
    assert ((ps == 1) | (ps == 4)).all()
    want, own = np.zeros(len(cases), np.int64), np.zeros(len(cases), int)
    for r, ent, L in _chains(rows, b[2], 33):
        if _resets(ent, L).tolist() == [cases[r][1]] and not own[r]:
            own[r] = 1
            want[r] += min(tdep, L - 1 - cases[r][1])
        else:
            want[r] += _chain_steps(ent, L, tdep)
    assert own.all()
    assert st.n_width_tab_steps == want.sum() + want[ids[ps == 1]].sum()
