"""Seed extension against the resident reference (Engine.extend_seeds / ibwa_extend_seeds): the seed
vectors of tests/golden/extend/seed_vectors.tsv.gz (tools/make_extend_golden.py: the reference's
aln_extend_core in end-cell mode over windows cut from the sets' .pac files), left and right, rev on and
off, on the one-reference set A and the two-reference set B of tests/golden/refine_vectors.json."""
import gzip
import os

import numpy as np
import pytest

from tests.test_extend_gpu import _param
from tests.test_refine_vectors import load_sets

pytestmark = pytest.mark.gpu

IBWA_EINVAL, IBWA_ENOINDEX = -2, -3


@pytest.fixture(scope="module")
def sets():
    return load_sets()


@pytest.fixture(scope="module")
def seeds(golden_dir):
    out = []
    for line in gzip.open(os.path.join(golden_dir, "extend", "seed_vectors.tsv.gz"), "rt"):
        if line.startswith("#"):
            continue
        f = line.rstrip("\n").split("\t")
        score = int(f[8])
        out.append({"set": f[0], "pname": f[1], "pos": int(f[2]), "dir": int(f[3]), "lt": int(f[4]), "rev": int(f[5]), "g0": int(f[6]),
                    "q": np.frombuffer(f[7].encode(), np.uint8) - ord("0"),
                    "exp": (score, (int(f[9]), int(f[10])) if score > 0 else None)})
    return out


@pytest.fixture(scope="module")
def eng():
    from ibwa_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _load(eng, sets, name):
    parts = sets[name][1]
    eng.load_pac([p[0] for p in parts], [p[1] for p in parts])
    return sets[name][0]


def _run(eng, vs, pname, rev):
    return eng.extend_seeds([v["pos"] for v in vs], [v["dir"] for v in vs], [v["lt"] for v in vs], [v["q"] for v in vs],
                            _param(pname, 50), g0=[v["g0"] for v in vs], rev=bool(rev))


@pytest.mark.parametrize("name", ["A", "B"])
def test_seed_vectors(eng, sets, seeds, name):
    text = _load(eng, sets, name)
    T, first = len(text), sets[name][1][0][1]
    mine = [v for v in seeds if v["set"] == name]
    assert len(mine) >= 150
    seen = set()
    for pname in ("bwasw", "bwa"):
        for rev in (0, 1):
            vs = [v for v in mine if v["pname"] == pname and v["rev"] == rev]
            got = _run(eng, vs, pname, rev)
            bad = [(v["pos"], v["dir"], v["lt"], v["g0"], g, v["exp"]) for v, g in zip(vs, got) if g != v["exp"]]
            assert not bad, (name, pname, rev, len(bad), bad[:5])
            seen |= {(v["dir"], rev) for v in vs}
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # seeds at base 1 and at the last base of the set, both directions
    assert {(v["pos"], v["dir"]) for v in mine} >= {(1, 0), (1, 1), (T - 1, 0), (T - 1, 1), (T, 1)}
    assert any(v["exp"][0] == -1 for v in mine)          # an empty window
    assert any(v["exp"][0] > v["g0"] for v in mine)      # an extension that gains
    if name == "B":  # windows that run from one reference of the set into the next
        assert any(v["dir"] == 0 and not v["rev"] and v["pos"] < first < v["pos"] + v["lt"] and v["exp"][1] is not None
                   and v["pos"] + v["exp"][1][0] > first for v in mine)
        assert any(v["dir"] == 1 and not v["rev"] and v["pos"] - v["lt"] < first < v["pos"] and v["exp"][1] is not None
                   and v["pos"] - v["exp"][1][0] < first for v in mine)


def test_right_seeds_equal_extend_over_extracted_windows(eng, sets, seeds):
    """A right-going seed is aln_extend_core over dbset_extract_sequence's window: extend_seeds must equal
    extend over pac_extract's output."""
    _load(eng, sets, "B")
    vs = [v for v in seeds if v["set"] == "B" and v["dir"] == 0 and v["rev"] == 0 and v["pname"] == "bwasw"]
    assert len(vs) >= 20
    wins, got_len = eng.pac_extract([v["pos"] for v in vs], [v["lt"] for v in vs])
    assert any(g < v["lt"] for g, v in zip(got_len, vs))  # clipped at the end of the set
    via_extend = eng.extend(wins, [v["q"] for v in vs], _param("bwasw", 50), g0=[v["g0"] for v in vs], mode="end")
    assert _run(eng, vs, "bwasw", 0) == via_extend == [v["exp"] for v in vs]


def test_errors_and_empty(sets):
    from ibwa_amd import engine as E
    bare = E.Engine(0)
    try:
        with pytest.raises(E.IbwaError, match=rf"ibwa error {IBWA_ENOINDEX}:.*no reference sequence loaded"):
            bare.extend_seeds([5], [0], [10], [[0, 1, 2]], "bwa")
        text = _load(bare, sets, "A")
        T = len(text)
        assert bare.extend_seeds([], [], [], [], "bwa") == []
        with pytest.raises(E.IbwaError, match=rf"ibwa error {IBWA_EINVAL}:.*seed 1: position {T + 1} > l_pac {T}"):
            bare.extend_seeds([5, T + 1], [1, 1], [10, 10], [[0, 1], [2, 3]], "bwa")
        with pytest.raises(E.IbwaError, match="seed 0: dir 2"):
            bare.extend_seeds([5], [2], [10], [[0, 1]], "bwa")
        with pytest.raises(E.IbwaError, match="seed 1: G0 0 outside|pair 1: G0 0 outside"):
            bare.extend_seeds([5, 9], [0, 0], [10, 10], [[0, 1], [2, 3]], "bwa", g0=[1, 0])
        with pytest.raises(E.IbwaError, match="row 2 < 4"):
            bare.extend_seeds([5], [0], [10], [[0, 1]], (5, 2, 2, np.array([1, -1, -1, 1], np.int32), 2, 50))
        # empty windows: right of the last base, left of base 0, lt = 0
        assert bare.extend_seeds([T, T + 7, 0, 40], [0, 0, 1, 0], [10, 10, 10, 0], [[0, 1]] * 4, "bwa") == [(-1, None)] * 4
        # the left window ends with base 0: the base itself, read leftwards from position 1
        q = [int(text[0])]
        assert bare.extend_seeds([1], [1], [5], [q], "bwa", g0=3) == [(3 + 11 - 1, (1, 1))]
        assert bare.extend_seeds([T - 1], [0], [5], [[int(text[T - 1])]], "bwa", g0=3) == [(13, (1, 1))]
        # rev reads base x as base T - x - 1 of the stored sequence
        assert bare.extend_seeds([0], [0], [5], [[int(text[T - 1])]], "bwa", g0=3, rev=True) == [(13, (1, 1))]
    finally:
        bare.close()
