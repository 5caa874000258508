"""bench.py's plain / --full split and --dump-outputs (CPU; no device involved).

A plain run keeps every leg that takes runs of its own switched off whatever else is given;
--full gives the legs their defaults back.  dump_outputs writes float32 / float64 .npy files
of at most 64 MB, the same sample for the same batch size, and what it writes is what
ibwa_batch_fetch returned for the sampled reads.
"""
import os

import numpy as np
import pytest

import bench
from ibwa_amd.engine import ALN_DTYPE

LEGS = ("exact_leg", "sa2pos", "e2e_leg", "sw_leg")


def test_plain_run_has_no_legs():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full) == (7, 2, False)
    assert a.no_cpu and not any(getattr(a, k) for k in LEGS)
    a = bench.parse_args(["--exact-leg", "1", "--sw-leg", "1000", "--e2e-leg", "1", "--sa2pos", "1"])
    assert a.no_cpu and not any(getattr(a, k) for k in LEGS)


def test_full_run_keeps_the_legs():
    a = bench.parse_args(["--full"])
    assert not a.no_cpu and all(getattr(a, k) for k in LEGS) and a.e2e_gz and a.ref_budget > 0
    a = bench.parse_args(["--full", "--no-cpu", "--sw-leg", "0"])
    assert a.no_cpu and a.sw_leg == 0 and a.exact_leg


def _hits(n, seed, max_hits=4):
    rng = np.random.default_rng(seed)
    n_aln = rng.integers(0, max_hits + 1, n).astype(np.int32)
    alns = np.zeros(int(n_aln.sum()), ALN_DTYPE)
    alns["info"] = np.arange(alns.size, dtype=np.uint32)  # row number: tells which rows were taken
    alns["k"] = rng.integers(0, 1 << 32, alns.size, dtype=np.uint64).astype(np.uint32)
    alns["l"] = alns["k"] + 1
    alns["score"] = rng.integers(0, 60, alns.size)
    return n_aln, alns


def _load(d, suffix=".npy"):
    return {f[:-len(suffix)]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(suffix)}


@pytest.mark.parametrize("n", [0, 1, 1000, bench.DUMP_READS, bench.DUMP_READS + 1])
def test_dump_outputs(tmp_path, n):
    n_aln, alns = _hits(n, 1)
    bench.dump_outputs(str(tmp_path), n_aln, alns, 0, 1)
    o = _load(str(tmp_path))
    assert sorted(o) == ["alns", "n_aln", "read_ids", "summary"]
    assert all(v.dtype in (np.float32, np.float64) for v in o.values())
    assert sum(v.nbytes for v in o.values()) <= 64 << 20
    ids = o["read_ids"].astype(np.int64)
    assert ids.size == min(n, bench.DUMP_READS) and (np.diff(ids) > 0).all()
    assert (o["n_aln"] == n_aln[ids]).all()
    first = np.concatenate([[0], np.cumsum(n_aln, dtype=np.int64)])
    rows = np.array([r for i in ids for r in range(first[i], first[i + 1])], dtype=np.int64)[:bench.DUMP_HITS]
    exp = alns[rows]
    assert o["alns"].shape == (rows.size, 4)
    for j, f in enumerate(("info", "k", "l", "score")):
        assert (o["alns"][:, j] == exp[f]).all()
    s = o["summary"]
    assert s[:3].tolist() == [n, alns.size, int((n_aln > 0).sum())]
    assert s[3:].tolist() == [int(alns[f].astype(np.int64).sum()) % (1 << 40)  # < 2^63 at these sizes
                             for f in ("k", "l", "score", "info")]


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """Another build's hits for the same batch: the same reads are sampled; many hits per read: the
    hit rows stop at DUMP_HITS and the files stay under 64 MB."""
    n = bench.DUMP_READS + 12345
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, *_hits(n, 1), 0, 1)
    bench.dump_outputs(b, *_hits(n, 2, max_hits=9), 0, 1)
    oa, ob = _load(a), _load(b)
    assert (oa["read_ids"] == ob["read_ids"]).all()
    assert ob["alns"].shape == (bench.DUMP_HITS, 4)
    assert sum(v.nbytes for v in ob.values()) <= 64 << 20


def test_dump_outputs_per_rank_names(tmp_path):
    bench.dump_outputs(str(tmp_path), *_hits(10, 3), 1, 2)
    assert sorted(os.listdir(tmp_path)) == [f"{x}.rank1.npy" for x in ("alns", "n_aln", "read_ids", "summary")]
