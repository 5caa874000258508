"""Order of a k_coop wave-iteration (engine option coop_early, coop.hip): with 1 the claims and the
chains' loads are issued before the hit barrier and the commit, with 0 after them.  The order may
change when a chain is claimed, never what the search finds, so every case runs under both orders
and must give the same hits as the golden or the oracle:

* every gapped golden .sai through the heavy-read pass, which must have taken every heavy read;
* the tandem-repeat reads (every read has over 1 000 equal hits, many chains of a level end in
  hits) on a device-built index: chains claimed around hits and the barriers' discards;
* reads resumed from a first-pass state after 5 and 50 iterations, under the default options and
  with more differences and gaps allowed, on the 100 bp set and on the mixed-length set (whose
  reads over 150 bp can leave a state only under -n 3: see test_resumed_reads);
* the cut-offs that end a search inside a chain (-m 50, -l 1000) and -N.
"""
import os

import pytest

import oracle
from ibwa_amd import engine as E

pytestmark = pytest.mark.gpu

ORDERS = (0, 1)
_REF = {}  # (index prefix, reads file, argv) -> the reads and the oracle's hits


def _eopt(opt):
    e = E.GapOpt()
    for f, _ in E.GapOpt._fields_:
        setattr(e, f, getattr(opt, f))
    return e


def _case(golden_dir, prefix, fq, argv, max_len=None):
    key = (prefix, fq, tuple(argv), max_len)
    if key not in _REF:
        opt, _ = oracle.parse_aln_args(argv)
        recs = oracle.read_fastq_records(os.path.join(golden_dir, fq))
        if max_len is not None:
            recs = [r for r in recs if len(r[1]) <= max_len]
        seqs, offs, lens = oracle.encode_reads(recs, opt.mode, opt.trim_qual)
        b0 = oracle.Bwt(os.path.join(golden_dir, prefix + ".bwt"))
        b1 = oracle.Bwt(os.path.join(golden_dir, prefix + ".rbwt"))
        rn, ra, _ = oracle.cal_sa_reg_gap(b0, b1, seqs, offs, lens, opt)
        _REF[key] = (seqs, offs, lens, _eopt(opt), rn, ra.tobytes())
    return _REF[key]


def _golden_run(eng, golden_dir, sai_manifest, keys):
    """Runs the manifest cases `keys`; returns those whose .sai body differs from the golden or whose
    heavy reads did not all go through the cooperative pass."""
    bad = []
    for key in keys:
        m = sai_manifest[key]
        opt, _ = oracle.parse_aln_args(m["argv"])
        recs = oracle.read_fastq_records(os.path.join(golden_dir, m["reads"]))
        seqs, offs, lens = oracle.encode_reads(recs, opt.mode, opt.trim_qual)
        n_aln, alns = eng.aln(seqs, offs, lens, _eopt(opt))
        exp = open(os.path.join(golden_dir, key + ".sai"), "rb").read()
        if not oracle.sai_body_equal(oracle.sai_bytes(opt, n_aln, alns), exp):
            bad.append(key)
        st = eng.stats()
        if not (st.n_coop == st.n_heavy > 0):
            bad.append(key + f":heavy {st.n_heavy} coop {st.n_coop}")
    return bad


@pytest.mark.parametrize("early", ORDERS)
def test_goldens_same_hits_in_both_orders(golden_dir, sai_manifest, gpu_engine, early):
    keys = [k for k, m in sorted(sai_manifest.items()) if m["argv"] != ["-n", "0"]]
    try:
        gpu_engine.set_option("gap_iter_budget", 1)
        gpu_engine.set_option("gap_coop", 1)
        gpu_engine.set_option("coop_early", early)
        bad = _golden_run(gpu_engine, golden_dir, sai_manifest, keys)
    finally:
        gpu_engine.set_option("gap_iter_budget", 8000)
        gpu_engine.set_option("coop_early", 1)
    assert not bad, bad


@pytest.fixture(scope="module")
def tandem_engine(golden_dir):
    codes, _ = oracle.read_pac(os.path.join(golden_dir, "tandem"))
    eng = E.Engine(0)
    eng.build_index(codes)
    yield eng
    eng.close()


@pytest.mark.parametrize("early", ORDERS)
@pytest.mark.parametrize("fq", ["tandem_1.fq", "tandem_2.fq"])
def test_hits_inside_wide_levels(golden_dir, tandem_engine, fq, early):
    seqs, offs, lens, e, rn, ra = _case(golden_dir, "tandem", fq, [])
    assert int(rn.sum()) >= len(lens)  # the reads do hit
    try:
        tandem_engine.set_option("gap_iter_budget", 1)
        tandem_engine.set_option("coop_early", early)
        n_aln, alns = tandem_engine.aln(seqs, offs, lens, e)
        st = tandem_engine.stats()
    finally:
        tandem_engine.set_option("gap_iter_budget", 8000)
        tandem_engine.set_option("coop_early", 1)
    assert st.n_coop == st.n_heavy > 0
    assert (n_aln == rn).all()
    assert alns.tobytes() == ra


@pytest.mark.parametrize("early", ORDERS)
@pytest.mark.parametrize("iters", [5, 50])
@pytest.mark.parametrize("argv", [[], ["-n", "3", "-o", "2", "-e", "3"]], ids=["default", "n3o2e3"])
@pytest.mark.parametrize("fq", ["reads_r100.fq", "reads_mixed.fq"])
def test_resumed_reads(golden_dir, gpu_engine, fq, argv, iters, early):
    """The first pass leaves states only when its widths fit in LDS (engine_aln.hip, plan_first_pass: `lw`):
    at most 6 differences in the batch, and gap_lw_min_waves waves per CU with the batch's longest row.
    reads_mixed.fq reaches 250 bp.  Under -n 3 only the waves stand in the way, so the mixed batches run
    with gap_lw_min_waves 1 and their 200 and 250 bp reads are resumed too.  Under the default options a
    read over 156 bp allows 7 to 9 differences and no batch holding one can leave a state, in either
    order: there the case runs the file's reads up to 150 bp (165 of 181)."""
    mixed = fq == "reads_mixed.fq"
    seqs, offs, lens, e, rn, ra = _case(golden_dir, "g1m", fq, argv, 150 if mixed and not argv else None)
    try:
        if mixed:
            gpu_engine.set_option("gap_lw_min_waves", 1)
        gpu_engine.set_option("gap_resume_iters", iters)
        gpu_engine.set_option("gap_resume_entries", 1)
        gpu_engine.set_option("coop_early", early)
        n_aln, alns = gpu_engine.aln(seqs, offs, lens, e)
        st = gpu_engine.stats()
    finally:
        gpu_engine.set_option("gap_resume_iters", 2000)
        gpu_engine.set_option("gap_resume_entries", 300)
        gpu_engine.set_option("gap_lw_min_waves", 8)
        gpu_engine.set_option("coop_early", 1)
    print(f"{fq} {argv} iters {iters} early {early}: {len(lens)} reads up to {max(lens)} bp, heavy {st.n_heavy} "
          f"coop {st.n_coop} resumed {st.n_resumed} state records cap {st.resume_records_cap}")
    assert (n_aln == rn).all()
    assert alns.tobytes() == ra
    assert st.n_resumed > 0


@pytest.mark.parametrize("early", ORDERS)
def test_cutoffs_inside_a_chain(golden_dir, sai_manifest, gpu_engine, early):
    keys = [k for k, m in sorted(sai_manifest.items())
            if m["argv"] in (["-m", "50"], ["-l", "1000"], ["-N", "-n", "2"])]
    assert len(keys) == 6, keys
    try:
        gpu_engine.set_option("gap_iter_budget", 1)
        gpu_engine.set_option("coop_early", early)
        bad = _golden_run(gpu_engine, golden_dir, sai_manifest, keys)
    finally:
        # the last test of the file: the shared engine goes back to its defaults
        gpu_engine.set_option("gap_iter_budget", 8000)
        gpu_engine.set_option("gap_coop", 1)
        gpu_engine.set_option("gap_resume_iters", 2000)
        gpu_engine.set_option("gap_resume_entries", 300)
        gpu_engine.set_option("gap_lw_min_waves", 8)
        gpu_engine.set_option("coop_early", 1)
    assert not bad, bad
