"""The index builder, everything derived from an index, and the search kernels on repetitive,
tiny and edge-length texts (tests/index_ref.py TEXTS), bit-exact against a plain reference that
shares no code with the product (naive_index / occ4_table; the oracle only ever sees naive_index's
words, never export_bwt's).

What each text family is aimed at, i.e. where to look when a case fails:

  A4096, T129, A<n>       one base.  LCP n - 1: suffix_sort's doubling loop (sa_build.hip) runs 9
                          rounds at 4096 with every suffix tied until the last -- k_keys2's
                          rank[v + h] at the text's end, k_rank2's group starts, the in-place
                          compaction of (P, V).  primary == n: bwt_kk (occ.h) never subtracts below n,
                          inv_psi's `k == primary` is the last row (sa2pos.hip).  Three empty L2
                          ranges: l2of, the level / K-mer tables' empty entries (kmer.hip).  SA
                          intervals as wide as the text: k_width, the gapped search's Occ steps.
  AC2049, per3, per21-23, fib4181
                          short periods around the round-1 key width (21 symbols): large tied groups
                          that halve per round, so the compaction and `V = P + m2` run many times at
                          many sizes; many-row intervals with few distinct symbols per Occ block.
  dup1500                 two copies of a 1500-symbol unit: two tied groups of ~1500 suffixes that
                          must survive 7 rounds (21 * 2^6 < 1500) -- the second sort and k_rank2 on
                          a few thousand entries instead of the handful a random genome leaves.
  rand<n>, A<n>           lengths on the layout's boundaries: 16 symbols per word (k_bwt_pack,
                          k_pack_text2), 32 per SA sample (k_sample_sa, derive_sa, k_expand_sa), 128
                          per Occ block with the spare block at n % 128 == 0 (k_block_counts,
                          k_pack_blocks, k_relayout, export_bwt), texts below one block and below a
                          read's length (k_width's text windows, the exact path's jump, the level
                          tables' short-read rule, the builder's scratch sizing).
  AC4096, lastG1000       skewed alphabets: L2[c] == L2[c + 1]; a symbol whose only occurrence is
                          the text's last (the first BWT symbol, row 0).

test_builder            -> sa_build.hip (+ k_pack_blocks, export_bwt / export_sa in engine_index.hip)
test_occ4_every_row     -> occ.h on both layouts' producers: k_pack_blocks (built), k_relayout (loaded)
test_derived_sa_and_coordinates -> sa2pos.hip: k_sa_link / k_sa_jump / k_sa_sample, k_expand_sa,
                           k_sa2pos_full / k_sa2pos_walk
test_search             -> aln.hip k_width, exact.hip, gapped.hip, coop.hip, kmer.hip, occ64.hip
"""
import functools

import numpy as np
import pytest

import oracle
from ibwa_amd import engine as E
from tests import index_ref as R

pytestmark = pytest.mark.gpu

OPTION_SETS = ([], ["-n", "0"], ["-N"], ["-n", "3", "-o", "2", "-e", "3"], ["-m", "50"], ["-l", "20", "-k", "1"])
# (engine options of one run, their defaults to put back)
DEFAULTS = {"gap_iter_budget": 8000, "gap_coop": 1, "exact_path": 1, "width_jump": 1, "gap_tab_k": -1}
ENGINE_SETTINGS = ({}, {"gap_iter_budget": 1}, {"gap_iter_budget": 1, "gap_coop": 0}, {"exact_path": 0},
                   {"width_jump": 0}, {"width_jump": 2}, {"gap_tab_k": 12}, {"gap_tab_k": 0})


def _eopt(o):
    e = E.GapOpt()
    for f, _ in E.GapOpt._fields_:
        setattr(e, f, getattr(o, f))
    return e


class _Indexed:
    """One engine, re-indexed per text: `built` on the device (jump arrays kept), or `loaded` from
    the reference words of naive_index through load_index (k_relayout)."""

    def __init__(self, built):
        self.eng = E.Engine(0)
        self.built = built
        self.name = None

    def at(self, name):
        if self.name != name:
            self.name = None
            if self.built:
                self.eng.build_index(R.text(name), sa_intv=32)
            else:
                for s in (0, 1):
                    ix = R.text_index(name, s)
                    self.eng.load_index(s, ix.primary, ix.L2, ix.words)
            self.name = name
        return self.eng


@pytest.fixture(scope="module")
def built():
    x = _Indexed(True)
    yield x
    x.eng.close()


@pytest.fixture(scope="module")
def loaded():
    x = _Indexed(False)
    yield x
    x.eng.close()


# ---------------------------------------------------------------- a. the builder

@pytest.mark.parametrize("name", R.TEXT_NAMES)
def test_builder(built, name):
    codes = R.text(name)
    n = codes.size
    above = 1 << int(n).bit_length()  # the power of two just above n: n_sa == 1
    built.name = None                  # this test leaves the engine with another sa_intv
    for intv in (1, 32, above):
        built.eng.build_index(codes, sa_intv=intv)
        for s in (0, 1):
            ix = R.text_index(name, s)
            p, l2, w = built.eng.export_bwt(s)
            assert p == ix.primary and tuple(l2) == ix.L2, (intv, s)
            assert w.size == ix.words.size and w.tobytes() == ix.words.tobytes(), (intv, s)
            sa = built.eng.export_sa(s, intv)
            assert sa.size == (n + intv) // intv and sa[0] == R.MINUS1, (intv, s)
            assert sa[1:].tobytes() == ix.sa[intv::intv].tobytes(), (intv, s)
        assert (n + above) // above == 1
    if name == "A4096":
        assert min(built.eng.build_rounds(0), built.eng.build_rounds(1)) >= 9
    if name == "dup1500":
        assert min(built.eng.build_rounds(0), built.eng.build_rounds(1)) >= 7


def test_builder_refuses_empty_text(built):
    built.name = None
    with pytest.raises(E.IbwaError):
        built.eng.build_index(np.zeros(0, np.uint8), sa_intv=32)


def test_build_rounds_is_for_built_indexes(loaded):
    loaded.at("rand128")
    with pytest.raises(E.IbwaError):
        loaded.eng.build_rounds(0)


# ---------------------------------------------------------------- b. rank queries

@pytest.mark.parametrize("name", R.TEXT_NAMES)
def test_occ4_every_row(built, loaded, name):
    n = R.text(name).size
    ks = R.occ4_ks(n)
    for which, eng in (("built", built.at(name)), ("loaded", loaded.at(name))):
        for s in (0, 1):
            ix = R.text_index(name, s)
            exp = R.occ4_table(ix.bwt, ix.primary, n)
            got = eng.occ4(s, ks)
            bad = np.flatnonzero((got != exp).any(axis=1))
            assert bad.size == 0, (which, s, [(int(ks[i]), got[i].tolist(), exp[i].tolist()) for i in bad[:4]])


# ---------------------------------------------------------------- c. SA derivation and coordinates

def _oracle_pair(name):
    """oracle.Bwt objects made from naive_index alone, with the 32-sampled SA."""
    out = []
    for s in (0, 1):
        ix = R.text_index(name, s)
        sa = ix.sa[::32].copy()
        sa[0] = R.MINUS1
        out.append(oracle.Bwt(primary=ix.primary, L2=ix.L2, words=ix.words).set_sa(sa, 32))
    return out


@pytest.mark.parametrize("name", R.TEXT_NAMES)
def test_derived_sa_and_coordinates(loaded, name):
    n = R.text(name).size
    loaded.name = None  # reload: the sampled SA comes from derive_sa alone
    eng = loaded.at(name)
    eng.derive_sa(32)
    for s in (0, 1):
        exp = R.text_index(name, s).sa[::32].copy()
        exp[0] = R.MINUS1
        assert eng.export_sa(s, 32).tobytes() == exp.tobytes(), s
    b0, b1 = _oracle_pair(name)
    rows = np.arange(n + 1, dtype=np.uint32)
    lens = [L for L in (1, 12, min(36, n)) if L <= n]
    strand = np.repeat(np.array([0, 1], np.uint8), rows.size * len(lens))
    k = np.tile(np.tile(rows, len(lens)), 2)
    ln = np.tile(np.repeat(np.array(lens, np.uint32), rows.size), 2)
    exp = oracle.sa2seq(b0, b1, strand, k, ln)
    try:
        eng.set_option("sa_walk", 1)   # the LF walk on the sampled SA
        walk = eng.sa2pos(strand, k, ln)
    finally:
        eng.set_option("sa_walk", 0)
    assert walk.tobytes() == exp.tobytes()
    eng.expand_sa()                    # the full SA from the sampled one: one gather per hit
    assert eng.sa2pos(strand, k, ln).tobytes() == exp.tobytes()


# ---------------------------------------------------------------- d. search

def _records(name):
    """FASTQ records cut from the text: 12 / 36 / 100 bp at its start, middle (n // 2, or centred
    where a read from n // 2 would pass the end) and end, exact and
    with one or two substitutions at fixed positions, forward and reverse-complemented, plus one
    read with an N; for a text below 36 bp also one 36 bp read, which cannot be placed.
    -> (records, indexes of the unmodified reads, index of the unplaceable read or None)"""
    codes = R.text(name).astype(np.int64)
    n = codes.size
    recs, exact = [], []

    def add(u):
        recs.append((f"{name}_{len(recs)}", "".join("ACGT"[c] for c in u).encode(), b"I" * len(u)))

    lens = [L for L in (12, 36, 100) if L <= n]
    for L in lens:
        for start in (0, n // 2 if n // 2 + L <= n else (n - L) // 2, n - L):
            ref = codes[start:start + L]
            for nm in (0, 1, 2):
                t = ref.copy()
                for p in (L // 3, 2 * L // 3)[:nm]:
                    t[p] = (t[p] + 1) % 4
                for rc in (False, True):
                    if nm == 0:
                        exact.append(len(recs))
                    add(3 - t[::-1] if rc else t)
    if lens:
        L = lens[-1]
        u = bytearray("".join("ACGT"[c] for c in codes[(n - L) // 2:(n - L) // 2 + L]).encode())
        u[L // 2] = ord("N")
        recs.append((f"{name}_N", bytes(u), b"I" * L))
    long_read = None
    if n < 36:
        long_read = len(recs)
        add(np.random.default_rng(n).integers(0, 4, 36))
    return recs, exact, long_read


@functools.lru_cache(maxsize=None)
def _expected(name):
    """Per option set the encoded reads and the oracle's hits on naive_index's words (computed once
    per text, shared by both index kinds), with the conditions that keep the comparison from
    passing on empty results."""
    recs, exact, long_read = _records(name)
    n = R.text(name).size
    bw = [oracle.Bwt(primary=ix.primary, L2=ix.L2, words=ix.words)
          for ix in (R.text_index(name, 0), R.text_index(name, 1))]
    out = []
    for argv in OPTION_SETS:
        opt, _ = oracle.parse_aln_args(list(argv))
        seqs, offs, lens = oracle.encode_reads(recs, opt.mode, opt.trim_qual)
        assert lens.size == len(recs)
        rn, ra, _ = oracle.cal_sa_reg_gap(bw[0], bw[1], seqs, offs, lens, opt)
        if n >= 100 and list(argv) in ([], ["-n", "0"]):
            assert (rn[exact] >= 1).all(), (name, argv, rn[exact].tolist())
        if long_read is not None:
            assert rn[long_read] == 0, (name, argv)
        if name == "A4096":
            assert int((ra["l"].astype(np.int64) - ra["k"] + 1).max()) >= n - 100
        out.append((opt, seqs, offs, lens, rn, ra))
    return out


@pytest.mark.parametrize("kind", ["built", "loaded"])
@pytest.mark.parametrize("name", R.TEXT_NAMES)
def test_search(built, loaded, name, kind):
    eng = (built if kind == "built" else loaded).at(name)
    bad = []
    for setting in ENGINE_SETTINGS:
        try:
            for key, v in setting.items():
                eng.set_option(key, v)
            for argv, (opt, seqs, offs, lens, rn, ra) in zip(OPTION_SETS, _expected(name)):
                n_aln, alns = eng.aln(seqs, offs, lens, _eopt(opt))
                if not ((n_aln == rn).all() and alns.tobytes() == ra.tobytes()):
                    bad.append((setting, argv, int((n_aln != rn).sum()), int(n_aln.sum()), int(rn.sum())))
                # the run took the path the setting is meant to reach: the exact kernel with its
                # jump (3), else the persistent gapped search (2) -- with a budget of 1 through the
                # heavy-read pass, which the cooperative kernel serves unless switched off
                st = eng.stats()
                exact = list(argv) == ["-n", "0"] and setting.get("exact_path", 1)
                if st.path != (3 if exact else 2):
                    bad.append((setting, argv, "path", st.path))
                if not exact and setting.get("gap_iter_budget") == 1 and lens.size >= 50:
                    if st.n_heavy == 0 or (setting.get("gap_coop", 1) and st.n_coop == 0):
                        bad.append((setting, argv, "heavy", int(st.n_heavy), "coop", int(st.n_coop)))
        finally:
            for key in setting:
                eng.set_option(key, DEFAULTS[key])
    assert not bad, bad
