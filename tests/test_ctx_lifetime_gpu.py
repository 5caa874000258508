"""A context gives back every device byte it took: after each pass's scratch, every post-alignment
service's buffers and the FASTQ ingest's have been allocated, closing the engine returns
ibwa_device_bytes to where it was; a lender closed before its borrower keeps the index alive until the
borrower goes; and a second round of the same calls reuses the buffers (the peak does not move)."""
import ctypes as c
import os

import numpy as np
import pytest

import oracle
from tests import index_ref as R
from tests import synth_util

pytestmark = pytest.mark.gpu

N_TEXT, N_READS, READ_LEN = 4096, 64, 36
# the defaults; every read handed to the cooperative pass (its scratch); ... to the wide pass (its scratch)
SETTINGS = [{}, {"gap_iter_budget": 1}, {"gap_iter_budget": 1, "gap_coop": 0}]
DEFAULTS = {"gap_iter_budget": 8000, "gap_coop": 1}


@pytest.fixture(scope="module")
def E():
    from ibwa_amd import engine
    return engine


@pytest.fixture(scope="module")
def case():
    """The text, its packed bytes, the reads (one substitution each) and the oracle's .sai for them,
    computed once on the plain index of tests/index_ref.py."""
    rng = np.random.default_rng(20261020)
    codes = rng.integers(0, 4, N_TEXT).astype(np.uint8)
    bw = []
    for t in (codes, codes[::-1].copy()):
        ix = R.naive_index(t)
        sa = ix.sa[::32].copy()
        sa[0] = R.MINUS1
        bw.append(oracle.Bwt(primary=ix.primary, L2=ix.L2, words=ix.words).set_sa(sa, 32))
    recs = []
    for i in range(N_READS):
        start = int(rng.integers(0, N_TEXT - READ_LEN + 1))
        t = codes[start:start + READ_LEN].astype(np.int64)
        p = int(rng.integers(0, READ_LEN))
        t[p] = (t[p] + 1 + int(rng.integers(0, 3))) % 4
        if i & 1:
            t = 3 - t[::-1]
        recs.append((f"r{i}", "".join("ACGT"[x] for x in t), "I" * READ_LEN))
    opt, _ = oracle.parse_aln_args([])
    seqs, offs, lens = oracle.encode_reads([(n, s.encode(), q.encode()) for n, s, q in recs], opt.mode, opt.trim_qual)
    rn, ra, _ = oracle.cal_sa_reg_gap(bw[0], bw[1], seqs, offs, lens, opt)
    assert int((rn > 0).sum()) > N_READS // 2
    pad = np.zeros((N_TEXT + 3) // 4 * 4, np.uint8)
    pad[:N_TEXT] = codes
    q = pad.reshape(-1, 4)
    pac = (q[:, 0] << 6 | q[:, 1] << 4 | q[:, 2] << 2 | q[:, 3]).astype(np.uint8)
    return dict(codes=codes, bw=bw, recs=recs, opt=opt, reads=(seqs, offs, lens), sai=oracle.sai_bytes(opt, rn, ra),
                rn=rn, ra=ra, pac=pac)


def _eopt(E, o):
    e = E.GapOpt()
    for f, _ in E.GapOpt._fields_:
        setattr(e, f, getattr(o, f))
    return e


def _aln_equals_oracle(E, eng, case):
    n_aln, alns = eng.aln(*case["reads"], _eopt(E, case["opt"]))
    assert oracle.sai_body_equal(oracle.sai_bytes(case["opt"], n_aln, alns), case["sai"])


def _three_runs(E, eng, case):
    try:
        for setting in SETTINGS:
            for k, v in setting.items():
                eng.set_option(k, v)
            _aln_equals_oracle(E, eng, case)
    finally:
        for k, v in DEFAULTS.items():
            eng.set_option(k, v)


def _fq_parse(E, eng, tmp_path, recs):
    path = os.path.join(tmp_path, "four.fq")
    synth_util.write_fastq(path, recs)
    raw = open(path, "rb").read()
    n_rec, consumed, not_strict = c.c_int64(), c.c_uint64(), c.c_int()
    lens = (c.c_int32 * 8)()
    buf = c.create_string_buffer(raw, len(raw))
    rc = E.lib().ibwa_fq_parse(eng.h, buf, len(raw), 0, 0, c.byref(n_rec), c.byref(consumed), c.byref(not_strict),
                               lens, None, 8)
    assert rc == 0, E.lib().ibwa_last_error()
    return n_rec.value, consumed.value, list(lens[:n_rec.value])


def _services(E, eng, case, tmp_path, load_pac=True):
    """One call of each service at its smallest shape -> everything they returned."""
    codes, rn, ra = case["codes"], case["rn"], case["ra"]
    out = {}
    # sa2pos on the oracle's hits (their first row each)
    first = np.concatenate([[0], np.cumsum(rn)[:-1]])[rn > 0]
    strand = ((ra["info"][first] >> 24) & 1).astype(np.uint8)  # bwt_aln1_t.a
    k = ra["k"][first].astype(np.uint32)
    ln = np.full(k.size, READ_LEN, np.uint32)
    pos = eng.sa2pos(strand, k, ln)
    assert pos.tobytes() == oracle.sa2seq(case["bw"][0], case["bw"][1], strand, k, ln).tobytes()
    out["sa2pos"] = pos.tobytes()
    # sw_batch on 2 pairs
    wins, reads = [codes[100:180], codes[900:980]], [codes[120:156], codes[930:966]]
    sw = eng.sw(wins, reads)
    assert sw == [oracle.sw_local(a, b) for a, b in zip(wins, reads)]
    out["sw"] = sw
    # the packed reference, then extract / refine / MD on 2 hits
    if load_pac:
        eng.load_pac([case["pac"]], [N_TEXT])
    got, n_got = eng.pac_extract([100, N_TEXT - 10], [80, 30])
    assert list(n_got) == [80, 10] and np.array_equal(got[0], codes[100:180]) and np.array_equal(got[1], codes[-10:])
    ins = np.concatenate([codes[500:518], [(codes[518] + 1) % 4], codes[518:535]]).astype(np.uint8)  # one inserted base
    p1, cig = eng.refine([120, 500], [1, 1], [codes[120:156], ins])
    out["refine"] = (p1.tobytes(), [x.tobytes() for x in cig])
    mm = codes[120:156].copy()
    mm[7] = (mm[7] + 1) % 4
    md, nm = eng.md([120, 120], [codes[120:156], mm])
    assert md == [str(READ_LEN), f"7{'ACGT'[codes[127]]}{READ_LEN - 8}"] and list(nm) == [0, 1]
    out["md"] = md
    # cs2nt_rows on 2 rows of 8 colours
    rng = np.random.default_rng(5)
    rows = eng.cs2nt_rows([rng.integers(0, 4, 9).astype(np.uint8) for _ in range(2)],
                          [rng.integers(0, 4, 8).astype(np.uint8) for _ in range(2)])
    assert [r.size for r in rows] == [7, 7]
    out["cs2nt"] = [r.tobytes() for r in rows]
    # fq_parse on 4 records
    n_rec, consumed, lens = _fq_parse(E, eng, tmp_path, case["recs"][:4])
    assert n_rec == 4 and lens == [READ_LEN] * 4 and consumed == sum(len(n) + 2 * READ_LEN + 6 for n, _, _ in case["recs"][:4])
    return out


def _built(E, case):
    eng = E.Engine(0)
    eng.build_index(case["codes"], sa_intv=32)
    return eng


def test_close_returns_every_byte(E, case, tmp_path):
    d0 = E.Engine.device_bytes()[0]
    eng = _built(E, case)
    _three_runs(E, eng, case)
    _services(E, eng, case, str(tmp_path))
    assert E.Engine.device_bytes()[0] > d0
    eng.close()
    assert E.Engine.device_bytes()[0] == d0


def test_lender_closed_first_lives_until_its_borrower_goes(E, case):
    d0 = E.Engine.device_bytes()[0]
    lender = _built(E, case)
    lender.prepare(_eopt(E, case["opt"]))  # a borrowed index cannot build its tables
    index_bytes = E.Engine.device_bytes()[0] - d0
    assert index_bytes >= 2 * (N_TEXT // 128 + 1) * 64
    bor = E.Engine(0)
    bor.share_index(lender)
    assert E.Engine.device_bytes()[0] == d0 + index_bytes  # lent, not copied
    lender.close()
    assert E.Engine.device_bytes()[0] == d0 + index_bytes  # the lender's buffers outlive its handle
    _aln_equals_oracle(E, bor, case)
    bor.close()
    assert E.Engine.device_bytes()[0] == d0


def test_second_round_reuses_the_buffers(E, case, tmp_path):
    """The reference is loaded once, with the index: ibwa_ctx_load_pac stages its input through two
    temporaries by design (test_refine_gpu.py asserts they are released again), and a second load would
    make them anew on top of everything the first round left (measured: the peak then rises by
    1 288 bytes, before and after the context's buffers became owning)."""
    eng = _built(E, case)
    try:
        peaks, outs = [], []
        for rnd in range(2):
            _three_runs(E, eng, case)
            outs.append(_services(E, eng, case, str(tmp_path), load_pac=rnd == 0))
            peaks.append(E.Engine.device_bytes()[1])
        assert outs[1] == outs[0]
        assert peaks[1] == peaks[0], peaks
    finally:
        eng.close()
