"""The CPU restatement against the reference on tests/golden/aln_edges/ (tools/make_aln_edges_golden.py):
`aln` at the option values and read lengths where the engine chooses another kernel.  This pins the
oracle on those ranges, and the conditions the GPU cases (test_aln_edges_gpu.py) rest on:

* every case's .sai body equals the reference's;
* the cases made to fill an entry bit field of k_gapped do: the largest n_mm among the reference's
  hits is 30 under -n 30 and -n 31, the largest n_gapo 7 under -o 7 and -o 8, the largest n_gape 15
  under -e 15 and -e 16 (one side of each pair runs the persistent kernel with the field at its last
  value, the other the general kernels);
* in every -m case at least one read's stack passes max_entries, so the cut-off (bwtgap.c:131) acts;
* no read makes more than 100 000 pops, which keeps every GPU case at seconds.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle
from tests import aln_edges_util

POP_CAP = 100_000


def edges_manifest(golden_dir):
    with open(os.path.join(golden_dir, "aln_edges", "manifest.json")) as f:
        return json.load(f)


_MAN = edges_manifest(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
_RUNS = {}


def _run(golden_dir, key):
    """(opt, n_aln, alns, per-read stats) of the oracle on one case, computed once."""
    if key not in _RUNS:
        m = _MAN[key]
        pre = os.path.join(golden_dir, m["index"])
        b0, b1 = oracle.Bwt(pre + ".bwt"), oracle.Bwt(pre + ".rbwt")
        opt, rest = oracle.parse_aln_args(m["argv"])
        assert not rest
        recs = aln_edges_util.records(golden_dir, m["reads"])
        seqs, offs, lens = oracle.encode_reads(recs, opt.mode, opt.trim_qual)
        st = np.zeros(len(lens), oracle.STATS_DTYPE)
        n_aln, alns, _ = oracle.cal_sa_reg_gap(b0, b1, seqs, offs, lens, opt, stats=st)
        _RUNS[key] = (opt, n_aln, alns, st)
    return _RUNS[key]


@pytest.mark.parametrize("key", sorted(_MAN))
def test_oracle_equals_reference(golden_dir, key):
    opt, n_aln, alns, st = _run(golden_dir, key)
    exp = open(os.path.join(golden_dir, "aln_edges", key + ".sai"), "rb").read()
    assert hashlib.sha1(exp).hexdigest() == _MAN[key]["sha1"]
    assert oracle.sai_body_equal(oracle.sai_bytes(opt, n_aln, alns), exp)
    assert int(st["pops"].max()) <= POP_CAP


def _arg(m, flag):
    return int(m["argv"][m["argv"].index(flag) + 1])


def test_bit_field_cases_fill_their_field():
    want = {"bf_mm.fq": ("n_mm", "-n", (30, 31), 30), "bf_gapo.fq": ("n_gapo", "-o", (7, 8), 7),
            "bf_gape.fq": ("n_gape", "-e", (15, 16), 15)}
    seen = set()
    for key, m in _MAN.items():
        if m["reads"] not in want:
            continue
        field, flag, values, top = want[m["reads"]]
        assert _arg(m, flag) in values, key
        assert m["max_fields"][field] == top, (key, m["max_fields"])
        seen.add((m["reads"], _arg(m, flag)))
    assert seen == {(r, v) for r, (_, _, vs, _) in want.items() for v in vs}


def test_sai_fields_are_the_manifest_maxima(golden_dir):
    """The recorded maxima are those of the committed .sai files (info = n_mm | n_gapo << 8 | n_gape << 16)."""
    for key, m in _MAN.items():
        if "max_fields" not in m:
            continue
        _, n_aln, alns, _ = _run(golden_dir, key)
        info = alns["info"]
        got = {"n_mm": int((info & 0xff).max()), "n_gapo": int((info >> 8 & 0xff).max()),
               "n_gape": int((info >> 16 & 0xff).max())}
        assert got == m["max_fields"], key


def test_max_entries_cut_off_is_reached(golden_dir):
    keys = [k for k, m in _MAN.items() if "-m" in m["argv"]]
    assert len(keys) == 4
    for key in keys:
        opt, _, _, st = _run(golden_dir, key)
        assert int((st["peak_entries"] > opt.max_entries).sum()) >= 1, key
