"""`aln` under the conditions that select a kernel: the options and the batch's longest read, not an
engine knob (engine_aln.hip run_setup / plan_first_pass).  Every case runs
Engine.aln with the engine's default options unless it says otherwise, compares the .sai body with
the reference's (tests/golden/aln_edges/, tools/make_aln_edges_golden.py; the g1m read sets are
rebuilt from their recipes by tests/aln_edges_util.py) and asserts which path ran
from ibwa_run_stats_t (path, first_pass_lw, first_pass_block, n_heavy, n_coop, n_resumed) and
retry_info()'s pass codes (1 k_coop, 2 wide k_gapped, 3 general kernels, 4 resumed).

The expected side of each boundary is computed here from the options: batch_md (or_cal_maxdiff of
the longest read under -n FLOAT), n_stacks as run_setup computes it, and the LDS bytes of the first
pass restated from gapped_lds_bytes with the engine's default page settings (engine_ctx.h).  Each
pair of cases straddles its boundary: one at the last admitted value, one just past it.

* entry bit fields of k_gapped (n_mm 5 bits, n_gapo 3, n_gape 4) filled to their last value, and
  the same reads one option past it on the general kernels; again through the heavy-read passes;
* the LDS-width first pass: batch max_diff 6 / 7, -k 2 / 3, the largest penalty 15 / 16;
* the workgroup size of the first pass without LDS widths: 256 / 128 / 64 by n_stacks.  (-M 16 alone
  gives n_stacks >= 124, past the 256-lane limit of 96, so the 256 -> 128 step is taken under -k 3,
  n_stacks 46 + 2 O; the 128 -> 64 step under both);
* k_coop's 128 buckets: n_stacks 128 / 130;
* n_stacks > 128 in k_gapped, whose non-empty mask has 128 bits (buckets beyond it are found by
  their heads; before that, the mask's "none" was taken for bucket 128 and its empty head loaded
  as a slot): every bit-field case, and hits reached only through buckets past the mask under
  -O 130, -M 16 -O 120 and at n_stacks 480 / 482, the last value whose bucket heads fit the first
  pass's LDS and the first that takes the general kernels;
* n_stacks far beyond it (-O 250, 700, 6200) and the refusal of n_stacks > 2^20;
* read length: 256 / 257 (k_coop), 4 095 / 4 096 (wide entries' 12-bit i), 5 000, the default
  -n 0.04 at 257 / 300 / 1 000 bases, one 300-base read among 100 bp reads, 65 535 / 65 536;
* the CLI on the long-read files, so that the device FASTQ ingest sees records of 5 000 and 65 535
  bases, and its refusal of 65 536.

Measured on an MI355X: the module's 37 cases take 5.2 s.  Every Engine.aln case is under 0.35 s (the
bit-field pairs 0.15 to 0.30 s, the n_stacks series 0.21 s, the rest 0.02 to 0.11 s) but the
65 535-base reads, 0.8 s for their three runs.  The CLI processes: 0.3 s on the 5 000-base file,
1.2 s on the 65 535-base file, 0.3 s for the refusal; each gets a limit of about ten times that.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
from ibwa_amd import engine as E
from tests import aln_edges_util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "ibwa_amd", "bin", "ibwa-amd")
GOLD = os.path.join(ROOT, "tests", "golden")
EDGES = os.path.join(GOLD, "aln_edges")
with open(os.path.join(EDGES, "manifest.json")) as _f:
    MAN = json.load(_f)

# engine defaults the plan depends on (engine_ctx.h): static slots per lane, pages per 256-lane pool,
# workgroups per CU, the fewest waves per CU the LDS-width variant accepts
GAP_CAP1, GAP_PAGES_PER_BLOCK, GAP_BLOCKS_PER_CU, GAP_LW_MIN_WAVES = 8192, 384, 3, 8
MAX_PAGES = min(7, (65536 - GAP_CAP1) >> 13)
COOP_MAXLEN, COOP_NSTK = 256, 128
LDS_MAX = 65536


# ---------------------------------------------------------------- the selection rules, restated

def batch_md(opt, max_len):
    return oracle.lib().or_cal_maxdiff(int(max_len), 0.02, opt.fnr) if opt.fnr > 0 else opt.max_diff


def n_stacks(opt, md):
    return (md + 1) * opt.s_mm + (min(md, opt.max_gapo) + 1) * opt.s_gapo + (opt.max_gape + 1) * opt.s_gape


def _bitmap(block):
    return (max(1, GAP_PAGES_PER_BLOCK * block // 256) + 31) // 32 * 4


def narrow_lds(nst, block):
    """gapped_lds_bytes(n_stacks, block, wide=false, ..., cw_words=0): 2 B heads and 8 free slots per lane,
    the page table, the pool bitmap, 8 words of packed read per lane."""
    b = (nst + 8) * block * 2 + MAX_PAGES * block * 2
    return ((b + 3) & ~3) + _bitmap(block) + 8 * block * 4


def lw_lds(block, cw_words):
    return (16 + 4) * block * 2 + _bitmap(block) + cw_words * block * 4


def plan(opt, max_len):
    """(path 2 admitted, first_pass_lw, first_pass_block) as run_setup and plan_first_pass decide them."""
    md = batch_md(opt, max_len)
    nst = n_stacks(opt, md)
    cw_words = 1 + (max_len + 15) // 16 + (max_len + 1 + (opt.seed_len + 1 if max_len > opt.seed_len else 0) + 3) // 4
    lw_block, lw_waves = 256, 0
    for blk in (256, 128, 64):
        b = lw_lds(blk, cw_words)
        if b > LDS_MAX:
            continue
        waves = min(GAP_BLOCKS_PER_CU * 4, (160 * 1024 // b) * (blk // 64))
        if waves > lw_waves:
            lw_waves, lw_block = waves, blk
    lw = (md <= 6 and 0 <= opt.max_seed_diff <= 2 and max(opt.s_mm, opt.s_gapo, opt.s_gape) <= 15 and
          lw_waves >= GAP_LW_MIN_WAVES)
    if lw:
        block, lds = lw_block, lw_lds(lw_block, cw_words)
    else:
        block = 256 if narrow_lds(nst, 256) <= LDS_MAX else 128 if narrow_lds(nst, 128) <= LDS_MAX else 64
        lds = narrow_lds(nst, block)
    v2 = (md + 1 <= 31 and min(md, opt.max_gapo) <= 7 and opt.max_gape <= 15 and (nst + 4096) * 4 <= LDS_MAX and
          max_len <= 65535 and lds <= LDS_MAX)
    return v2, lw, block


def heavy_pass(opt, max_len):
    """The pass that takes a read the persistent first pass hands on (gap_iter_budget=1)."""
    nst = n_stacks(opt, batch_md(opt, max_len))
    if max_len <= COOP_MAXLEN and nst <= COOP_NSTK:
        return 1
    return 2 if max_len < 4096 else 3


# ---------------------------------------------------------------- fixtures and helpers

@pytest.fixture(scope="module")
def stale_engine(golden_dir):
    eng = E.Engine(0)
    eng.load_index_files(os.path.join(golden_dir, "stale_alt"))
    yield eng
    eng.close()


def _eopt(opt):
    e = E.GapOpt()
    for f, _ in E.GapOpt._fields_:
        setattr(e, f, getattr(opt, f))
    return e


_CASES = {}


def load(key):
    """(opt, records, golden .sai bytes) of a manifest case, read once."""
    if key not in _CASES:
        m = MAN[key]
        opt, rest = oracle.parse_aln_args(m["argv"])
        assert not rest
        recs = aln_edges_util.records(GOLD, m["reads"])
        _CASES[key] = (opt, recs, open(os.path.join(EDGES, key + ".sai"), "rb").read())
    return _CASES[key]


def sai_records(sai):
    """The per-read records of a .sai body (int32 n_aln + n_aln x 16 B)."""
    out, p = [], 64
    while p < len(sai):
        n = int.from_bytes(sai[p:p + 4], "little", signed=True)
        out.append(sai[p:p + 4 + 16 * n])
        p += 4 + 16 * n
    return out


def run(eng, opt, recs, **knobs):
    """Engine.aln over the records -> (.sai bytes, stats, (ids, passes)); knobs are set for the run only."""
    seqs, offs, lens = oracle.encode_reads(recs, opt.mode, opt.trim_qual)
    defaults = {"gap_iter_budget": 8000}
    try:
        for k, v in knobs.items():
            eng.set_option(k, v)
        n_aln, alns = eng.aln(seqs, offs, lens, _eopt(opt))
        st, info = eng.stats(), eng.retry_info()
    finally:
        for k in knobs:
            eng.set_option(k, defaults[k])
    return oracle.sai_bytes(opt, n_aln, alns), st, info, int(lens.max())


def run_case(eng, key, **knobs):
    opt, recs, gold = load(key)
    sai, st, info, max_len = run(eng, opt, recs, **knobs)
    assert oracle.sai_body_equal(sai, gold), key
    return opt, st, info, max_len, sai


def assert_plan(key, opt, st, max_len, path=None, lw=None, block=None):
    """The run took the path the restated rules give; `path` / `lw` / `block`: what the case is built for."""
    v2, exp_lw, exp_block = plan(opt, max_len)
    if path is not None:
        assert (2 if v2 else 0) == path, (key, "the case is on the wrong side of its boundary")
    if lw is not None:
        assert v2 and int(exp_lw) == lw, (key, "the case is on the wrong side of its boundary")
    if block is not None:
        assert v2 and not exp_lw and exp_block == block, (key, "the case is on the wrong side of its boundary")
    assert st.path == (2 if v2 else 0), (key, st.path)
    assert st.first_pass_lw == (int(exp_lw) if v2 else 0), (key, st.first_pass_lw)
    assert st.first_pass_block == (exp_block if v2 else 0), (key, st.first_pass_block)


def max_fields(sai):
    info = np.concatenate([np.frombuffer(r[4:], dtype="<u4")[0::4] for r in sai_records(sai)])
    return {"n_mm": int((info & 0xff).max()), "n_gapo": int((info >> 8 & 0xff).max()),
            "n_gape": int((info >> 16 & 0xff).max())}


# ---------------------------------------------------------------- entry bit fields

BIT_FIELDS = [  # (last value admitted: path 2, one past: path 0)
    ("bf_mm.n30o0l1000", "bf_mm.n31o0l1000"),
    ("bf_gapo.n7o7i0d100l1000m20000", "bf_gapo.n8o8i0d100l1000m20000"),
    ("bf_gape.n16o1e15i0d100l1000M11O3E1m20000", "bf_gape.n17o1e16i0d100l1000M11O3E1m20000"),
]


@pytest.mark.parametrize("pair", BIT_FIELDS, ids=["n_mm", "n_gapo", "n_gape"])
def test_entry_bit_fields_at_and_past_their_last_value(stale_engine, pair):
    for key, path in zip(pair, (2, 0)):
        opt, st, _, max_len, sai = run_case(stale_engine, key)
        assert_plan(key, opt, st, max_len, path=path)
        assert max_fields(sai) == MAN[key]["max_fields"], key


@pytest.mark.parametrize("key", [p[0] for p in BIT_FIELDS], ids=["n_mm", "n_gapo", "n_gape"])
def test_entry_bit_fields_through_the_heavy_pass(stale_engine, key):
    opt, st, (ids, ps), max_len, sai = run_case(stale_engine, key, gap_iter_budget=1)
    assert st.path == 2 and st.n_heavy > 0 and len(ids) >= st.n_heavy
    want = heavy_pass(opt, max_len)
    assert (ps == want).all(), (key, want, np.bincount(ps))
    assert st.n_coop == (st.n_heavy if want == 1 else 0)
    assert max_fields(sai) == MAN[key]["max_fields"], key


# ---------------------------------------------------------------- first-pass variant and workgroup size

@pytest.mark.parametrize("a,b", [("n6", "n7"), ("k2", "k3"), ("M15", "M16"), ("O15", "O16"), ("E15", "E16")])
def test_lds_width_selection(gpu_engine, a, b):
    for tag, lw in ((a, 1), (b, 0)):
        key = "r100_200." + tag
        opt, st, _, max_len, _ = run_case(gpu_engine, key)
        assert_plan(key, opt, st, max_len, path=2, lw=lw)


@pytest.mark.parametrize("a,b,blocks", [("k3O25", "k3O26", (256, 128)), ("k3O89", "k3O90", (128, 64)),
                                        ("M16O50", "M16O51", (128, 64))])
def test_workgroup_size_by_n_stacks(gpu_engine, a, b, blocks):
    for tag, block in zip((a, b), blocks):
        key = "r100_200." + tag
        opt, st, _, max_len, _ = run_case(gpu_engine, key)
        assert_plan(key, opt, st, max_len, path=2, block=block)


def test_default_and_gap_extension_options(gpu_engine):
    """The sets' default-option run (LDS widths, 256 lanes) and -e 16 (max_gape past the 4-bit field: path 0)."""
    opt, st, _, max_len, _ = run_case(gpu_engine, "r100_200.default")
    assert_plan("r100_200.default", opt, st, max_len, path=2, lw=1)
    assert st.first_pass_block == 256
    opt, st, _, max_len, _ = run_case(gpu_engine, "r100_200.e16")
    assert_plan("r100_200.e16", opt, st, max_len, path=0)


# ---------------------------------------------------------------- k_coop's buckets, buckets past the mask

def test_coop_bucket_limit(gpu_engine):
    opt, st, (ids, ps), max_len, _ = run_case(gpu_engine, "r100_200.O41", gap_iter_budget=1)
    assert n_stacks(opt, batch_md(opt, max_len)) == COOP_NSTK
    assert st.path == 2 and st.n_coop == st.n_heavy > 0
    for key in ("r100_200.O42", "r100_200.O43", "r100_200.O50"):
        opt, st, (ids, ps), max_len, _ = run_case(gpu_engine, key, gap_iter_budget=1)
        assert n_stacks(opt, batch_md(opt, max_len)) > COOP_NSTK
        assert st.path == 2 and st.n_heavy > 0 and st.n_coop == 0, key
        assert len(ids) > 0 and (ps == 2).all(), (key, np.bincount(ps))
    # and with the default options: no state is left for a pass that could not resume it
    opt, st, _, max_len, _ = run_case(gpu_engine, "r100_200.O42")
    assert_plan("r100_200.O42", opt, st, max_len, path=2, lw=0)
    assert st.n_resumed == 0


@pytest.mark.parametrize("key", ["r100_200.O130", "r100_200.M16O120", "r100_40.O217"])
def test_scores_past_the_128th_bucket(gpu_engine, key):
    """A gap open alone scores 130 (217), or with one mismatch 136: hits k_gapped reaches only through
    buckets its 128-bit non-empty mask does not cover -- in the first pass (-M 16: no LDS widths;
    n_stacks 480: the last the first pass's LDS holds) and in the wide kernel (gap_iter_budget=1)."""
    opt, st, _, max_len, sai = run_case(gpu_engine, key)
    assert_plan(key, opt, st, max_len, path=2)
    assert max_fields(sai)["n_gapo"] == 1  # the set has reads whose best hit opens a gap
    opt, st, (ids, ps), max_len, _ = run_case(gpu_engine, key, gap_iter_budget=1)
    assert st.n_heavy > 0 and st.n_coop == 0 and (ps == 2).all(), (key, np.bincount(ps))


def test_n_stacks_beyond_the_first_pass_lds(gpu_engine):
    """run_setup admits the persistent kernel only when the first pass's bucket heads fit a workgroup's
    LDS (n_stacks <= 480 at 64 lanes); beyond it the batch takes the general kernels."""
    for key, nst, path in (("r100_40.O217", 480, 2), ("r100_40.O218", 482, 0), ("r100_40.O250", 546, 0),
                           ("r100_40.O700", 1446, 0), ("r100_40.O6200", 12446, 0)):
        opt, st, _, max_len, _ = run_case(gpu_engine, key)
        assert n_stacks(opt, batch_md(opt, max_len)) == nst
        assert_plan(key, opt, st, max_len, path=path)
    opt, recs, _ = load("r100_40.O250")
    bad = oracle.parse_aln_args(["-O", "600000"])[0]
    with pytest.raises(E.IbwaError, match="invalid stack size"):
        run(gpu_engine, bad, recs)


# ---------------------------------------------------------------- read length

def _by_length(key, lo, hi):
    opt, recs, gold = load(key)
    keep = [j for j, r in enumerate(recs) if lo <= len(r[1]) <= hi]
    rec = sai_records(gold)
    return opt, [recs[j] for j in keep], gold[:64] + b"".join(rec[j] for j in keep)


def test_long_reads_default_options(gpu_engine):
    opt, st, _, max_len, _ = run_case(gpu_engine, "long.n2")
    assert max_len == 5000
    assert_plan("long.n2", opt, st, max_len, path=2, lw=0)
    assert st.n_resumed == 0


@pytest.mark.parametrize("lo,hi,want", [(1, 256, 1), (257, 257, 2), (257, 4095, 2), (4095, 4095, 2), (4096, 4096, 3),
                                        (4096, 5000, 3), (256, 257, 2)])
def test_long_reads_heavy_pass_by_length(gpu_engine, lo, hi, want):
    """-n 2 keeps every record independent of the batch, so the golden's records of a length range are
    the golden of that batch.  The batch's longest read decides the pass for all of its reads."""
    opt, recs, gold = _by_length("long.n2", lo, hi)
    assert len(recs) >= 6
    sai, st, (ids, ps), _ = run(gpu_engine, opt, recs, gap_iter_budget=1)
    assert oracle.sai_body_equal(sai, gold)
    assert heavy_pass(opt, max(len(r[1]) for r in recs)) == want
    assert st.path == 2 and st.n_heavy > 0 and len(ids) > 0
    assert (ps == want).all(), np.bincount(ps)
    assert st.n_coop == (st.n_heavy if want == 1 else 0)


def test_long_reads_exact_path(gpu_engine):
    opt, st, _, max_len, _ = run_case(gpu_engine, "long.n0")
    assert st.path in (1, 3) and st.first_pass_block == 0 and max_len == 5000


@pytest.mark.parametrize("n", [257, 300, 1000])
def test_long_reads_default_fnr(gpu_engine, n):
    key = f"len{n}.default"
    opt, st, _, max_len, _ = run_case(gpu_engine, key)
    assert max_len == n and batch_md(opt, n) > 6
    assert_plan(key, opt, st, max_len, path=2, lw=0)


def test_one_long_read_in_a_batch_of_short_ones(gpu_engine):
    opt, st, _, max_len, sai = run_case(gpu_engine, "r100_plus300.default")
    assert max_len == 300
    assert_plan("r100_plus300.default", opt, st, max_len, path=2, lw=0)
    assert st.n_resumed == 0
    _, st0, _, _, sai0 = run_case(gpu_engine, "r100_200.default")
    assert st0.first_pass_lw == 1
    _, recs, _ = load("r100_plus300.default")
    at = [j for j, r in enumerate(recs) if len(r[1]) == 300]
    assert len(at) == 1
    rec = sai_records(sai)
    del rec[at[0]]
    assert rec == sai_records(sai0)


def test_longest_read(gpu_engine):
    for key, paths in (("len65535.n1", (2,)), ("len65535.n0", (1, 3))):
        opt, st, _, max_len, _ = run_case(gpu_engine, key)
        assert max_len == 65535 and st.path in paths, (key, st.path)
    opt, recs, _ = load("len65535.n1")
    longer = [(nm, s + s[:1], q + q[:1]) for nm, s, q in recs]
    with pytest.raises(E.IbwaError, match="read length 65536 > 65535"):
        run(gpu_engine, opt, longer)


# ---------------------------------------------------------------- the CLI on long records

def _cli(argv, prefix, reads, out, timeout):
    return subprocess.run([CLI, "aln"] + argv + ["-f", str(out), prefix, str(reads)], capture_output=True, text=True,
                          timeout=timeout)


@pytest.mark.parametrize("key,limit", [("long.n2", 4), ("len65535.n1", 15)])
def test_cli_long_records(golden_dir, key, limit, tmp_path):
    m = MAN[key]
    out = tmp_path / "out.sai"
    fq = aln_edges_util.write_fastq(str(tmp_path / m["reads"]), load(key)[1])  # (the set is kept as a recipe)
    r = _cli(m["argv"], os.path.join(golden_dir, "g1m"), fq, out, limit)
    assert r.returncode == 0, r.stderr[-2000:]
    assert oracle.sai_body_equal(out.read_bytes(), load(key)[2])


def test_cli_refuses_65536_bases(golden_dir, tmp_path):
    _, recs, _ = load("len65535.n1")
    fq = aln_edges_util.write_fastq(str(tmp_path / "len65536.fq"), [(nm, s + s[:1], q + q[:1]) for nm, s, q in recs])
    r = _cli(["-n", "1"], os.path.join(golden_dir, "g1m"), fq, tmp_path / "out.sai", 4)
    assert r.returncode != 0 and "read length 65536 > 65535" in r.stderr, r.stderr[-2000:]
