"""Tail jump of the first gapped pass (engine option gap_tail_tab, gapped.hip): the exact tail
(bwt_match_exact_alt, bwtgap.c:160-163) of a node stored by its string takes its steps down to depth
gap_tab_k + 1 from one level-table entry instead of one Occ round trip per symbol.

* every golden .sai of the option matrix, bit for bit, with the jump on (tables of K 12 and 6) and off;
* GPU == CPU restatement on the 31 Mb device-built genome with the jump on, under the options that
  reach it differently (K where every jump lands on a live interval, resume states left around a
  jump, seeds, -N, more gaps, the 64-lane workgroups of 150 bp reads, 70 bp without indels);
* the count of jumps taken (ibwa_run_stats_t.n_tail_jumps) is > 0 with the option on and 0 with it
  off, with identical hits -- so none of the above passes with the path never running.
"""
import os

import numpy as np
import pytest

import oracle
from ibwa_amd import engine as E
from tests.test_scale_properties import eopt, mid_genome, reads  # noqa: F401 (mid_genome: fixture)

pytestmark = pytest.mark.gpu

_REF = {}  # (argv, read length, substitution rate, reads) -> the reads and the restatement's hits


def _case(mid, argv, ln, sub, n):
    key = (tuple(argv), ln, sub, n)
    if key not in _REF:
        ascii_, lens, _, b0, b1 = mid
        seq, off, lns, _, _ = reads(ascii_, lens, 5 + n, n, ln, sub, 0.05)
        o, e = eopt(argv)
        rn, ra, _ = oracle.cal_sa_reg_gap(b0, b1, seq, off, lns, o, n_threads=8)
        _REF[key] = (seq, off, lns, e, rn, ra.tobytes())
    return _REF[key]


@pytest.mark.parametrize("tail_tab,tab_k", [(1, 12), (1, 6), (0, 12)])
def test_sai_goldens_tail_tab(golden_dir, sai_manifest, gpu_engine, tail_tab, tab_k):
    """-c, mixed.N (reads with N step symbol by symbol), seeds, -N, the 36 bp reads that never take
    string form, 150 bp: all as the reference wrote them."""
    bad = []
    jumps = 0
    try:
        gpu_engine.set_option("gap_tail_tab", tail_tab)
        gpu_engine.set_option("gap_tab_k", tab_k)
        for key, m in sorted(sai_manifest.items()):
            opt, _ = oracle.parse_aln_args(m["argv"])
            recs = oracle.read_fastq_records(os.path.join(golden_dir, m["reads"]))
            seqs, offs, lens = oracle.encode_reads(recs, opt.mode, opt.trim_qual)
            e = E.GapOpt()
            for f, _ in E.GapOpt._fields_:
                setattr(e, f, getattr(opt, f))
            n_aln, alns = gpu_engine.aln(seqs, offs, lens, e)
            st = gpu_engine.stats()
            if st.path == 2:
                jumps += st.n_tail_jumps
            exp = open(os.path.join(golden_dir, key + ".sai"), "rb").read()
            if not oracle.sai_body_equal(oracle.sai_bytes(opt, n_aln, alns), exp):
                bad.append(key)
    finally:
        gpu_engine.set_option("gap_tail_tab", 1)
        gpu_engine.set_option("gap_tab_k", -1)
    assert not bad, bad
    assert (jumps > 0) == bool(tail_tab)


@pytest.mark.parametrize("argv,ln,sub,n,tune", [
    # K auto (11 here): jumps land at the depth where strings stop existing in 31 Mb, so both outcomes occur
    ([], 100, 0.01, 8_000, {}),
    # every jump lands on a non-empty interval and goes on by Occ steps
    ([], 100, 0.02, 8_000, {"gap_tab_k": 6}), ([], 100, 0.02, 8_000, {"gap_tab_k": 8}),
    # reads handed on early: at 20 iterations no read has a hit yet, so no tail has started (the states
    # hold the string-stored nodes that would have jumped); at 120 a 100 bp read's first hit has lowered
    # max_diff, so reads are handed on while lanes are in and just past a jump
    ([], 100, 0.01, 8_000, {"gap_resume_iters": 20, "gap_resume_entries": 4}),
    ([], 100, 0.01, 8_000, {"gap_resume_iters": 120, "gap_resume_entries": 4}),
    (["-l", "20", "-k", "1"], 100, 0.02, 8_000, {}),
    (["-N", "-n", "2"], 100, 0.01, 4_000, {}),
    (["-n", "3", "-o", "2", "-e", "3"], 100, 0.02, 8_000, {}),
    ([], 150, 0.02, 4_000, {}),  # the 64-lane instantiation
    (["-i", "0", "-d", "0"], 70, 0.02, 8_000, {})])
def test_tail_jump_equals_oracle(mid_genome, argv, ln, sub, n, tune):
    _, _, eng, _, _ = mid_genome
    seq, off, lns, e, rn, ra = _case(mid_genome, argv, ln, sub, n)
    defaults = {"gap_tab_k": -1, "gap_resume_iters": 2000, "gap_resume_entries": 300}
    try:
        eng.set_option("gap_tail_tab", 1)
        for k, v in tune.items():
            eng.set_option(k, v)
        n_aln, alns = eng.aln(seq, off, lns, e)
        st = eng.stats()
    finally:
        for k in tune:
            eng.set_option(k, defaults[k])
    assert st.path == 2
    if tune.get("gap_resume_iters", 2000) > 100:
        assert st.n_tail_jumps > 0  # the jump ran
    if "gap_resume_iters" in tune:
        assert st.n_resumed > 0
    assert (n_aln == rn).all()
    assert alns.tobytes() == ra


def test_jump_count_follows_the_option(mid_genome):
    _, _, eng, _, _ = mid_genome
    seq, off, lns, e, rn, ra = _case(mid_genome, [], 100, 0.01, 8_000)
    got = {}
    try:
        for v in (1, 0):
            eng.set_option("gap_tail_tab", v)
            n_aln, alns = eng.aln(seq, off, lns, e)
            got[v] = (n_aln.copy(), alns.tobytes(), int(eng.stats().n_tail_jumps))
    finally:
        eng.set_option("gap_tail_tab", 1)
    assert got[1][2] > 0 and got[0][2] == 0
    assert (got[1][0] == got[0][0]).all() and got[1][1] == got[0][1]
    assert (got[0][0] == rn).all() and got[0][1] == ra
