"""GPU parity of the seed extension (extend.hip through Engine.extend and Engine.stdaln(mode="extend")).

tests/golden/extend/extend_vectors.tsv.gz (tools/make_extend_golden.py) holds the reference's
aln_extend_core in its three modes and aln_stdaln_aux(type 2) over the blast, bwa and aa2aa presets, the
custom 5 / -2 / 10 / 2 scheme and bwasw's 1 / -3 / 5 / 2, bands 1, 2, 3, 17, 50 and len1 + len2, G0 from 1 to
30 000, lengths 0 to 3 200: every row must come out equal, score, end cell, path length, path start and
CIGAR.  Then: a batch whose eh rings lie partly in LDS and partly in HBM, a batch cut into several
launches, the pairs whose score passes 32000, the count of pairs without a suitable band, and n = 0.
"""
import gzip
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_AA = "ARNDCQEGHILKMFPSTWYV"


def _tables():
    nt = np.full(256, 4, np.uint8)
    for k, ch in enumerate("AGCT"):
        nt[ord(ch)] = nt[ord(ch.lower())] = k
    aa = np.full(256, 21, np.uint8)
    for k, ch in enumerate(_AA):
        aa[ord(ch)] = aa[ord(ch.lower())] = k
    aa[ord("*")] = 20
    return {"aa2aa": aa, None: nt}


def _param(pname, band):
    import ibwa_amd
    if pname == "match5":
        base = {"gap_open": 10, "gap_ext": 2, "gap_end": 2, "row": 5,
                "matrix": np.where(np.eye(5, dtype=bool), 5, -2).astype(np.int32)}
    elif pname == "bwasw":
        m = np.full((5, 5), -3, np.int32)
        m[np.arange(4), np.arange(4)] = 1
        base = {"gap_open": 5, "gap_ext": 2, "gap_end": 2, "row": 5, "matrix": m}
    else:
        base = ibwa_amd.aln_param(pname)
    return dict(base, band_width=band)


def _encode(tab, s):
    return tab[np.frombuffer(s.encode(), dtype=np.uint8)] if s else np.zeros(0, np.uint8)


_vec_cache = []


def _vectors(golden_dir):
    """The TSV's rows, read once: the call's settings, the encoded pair and the expected tuple in the
    shape Engine.extend / Engine.stdaln return it."""
    if _vec_cache:
        return _vec_cache
    tabs = _tables()
    for line in gzip.open(os.path.join(golden_dir, "extend", "extend_vectors.tsv.gz"), "rt"):
        if line.startswith("#"):
            continue
        f = line.rstrip("\n").split("\t")
        tag, pname, mode, band, g0, s1, s2, score = f[0], f[1], f[2], int(f[3]), int(f[4]), f[5], f[6], int(f[7])
        if mode == "score":
            exp = (score, None)
        elif mode == "end":
            exp = (score, (int(f[8]), int(f[9])) if score > 0 else None)
        elif int(f[10]) == 0:  # no path
            exp = (score, None, 0, None) if mode == "path" else (score, 0, 0, None, None, None)
        elif mode == "path":
            exp = (score, (int(f[8]), int(f[9])), int(f[10]), f[13])
        else:  # std2: Engine.stdaln's tuple
            exp = (score, 0, int(f[10]), (int(f[11]), int(f[12])), (int(f[8]), int(f[9])), f[13])
        tab = tabs.get(pname, tabs[None])
        _vec_cache.append({"tag": tag, "pname": pname, "mode": mode, "band": band, "g0": g0, "pair": (pname, band, g0, s1, s2),
                           "s1": _encode(tab, s1), "s2": _encode(tab, s2), "exp": exp})
    return _vec_cache


def _run(eng, vecs, idx, pname, band, mode):
    s1, s2 = [vecs[k]["s1"] for k in idx], [vecs[k]["s2"] for k in idx]
    if mode == "std2":
        return eng.stdaln(s1, s2, _param(pname, band), mode="extend")
    return eng.extend(s1, s2, _param(pname, band), g0=[vecs[k]["g0"] for k in idx], mode=mode)


def _same(got, exp, mode):
    if mode == "std2" and exp[2] == 0:  # no path: the reference sets the score and nothing else
        return got[0] == exp[0] and got[2] == 0
    return got == exp


@pytest.fixture(scope="module")
def results(golden_dir, gpu_engine):
    """Every vector through the engine in its recorded mode, one batch per (parameters, band, mode);
    and per path-mode batch the engine's count of pairs without a suitable band."""
    vecs = _vectors(golden_dir)
    groups = {}
    for k, v in enumerate(vecs):
        groups.setdefault((v["pname"], v["band"], v["mode"]), []).append(k)
    got, no_band = [None] * len(vecs), {}
    for (pname, band, mode), idx in groups.items():
        for k, r in zip(idx, _run(gpu_engine, vecs, idx, pname, band, mode)):
            got[k] = r
        if mode in ("path", "std2"):
            no_band[(pname, band, mode)] = (gpu_engine.extend_stats()["no_band"], idx)
    return vecs, got, no_band


@pytest.mark.parametrize("mode", ["score", "end", "path", "std2"])
def test_library_vectors(results, mode):
    vecs, got, _ = results
    mine = [(k, v, g) for k, (v, g) in enumerate(zip(vecs, got)) if v["mode"] == mode]
    assert len(mine) >= 100
    bad = [(k, v["tag"], v["pname"], v["band"], v["g0"], g, v["exp"]) for k, v, g in mine if not _same(g, v["exp"], mode)]
    assert not bad, (len(bad), bad[:5])


def test_grid_covers_the_classes(golden_dir):
    vecs = _vectors(golden_dir)
    assert {v["band"] for v in vecs} >= {0, 1, 2, 3, 50}
    assert {v["pname"] for v in vecs} == {"blast", "bwa", "aa2aa", "match5", "bwasw"}
    assert {v["tag"] for v in vecs} >= {"1x1_match", "1x1_mismatch", "1xn", "nx1", "empty1", "empty2", "grid", "unrelated", "tie",
                                         "long_gap", "doubling", "rebasing"}
    assert any(v["g0"] == 1 for v in vecs) and any(1 < v["g0"] < 100 for v in vecs) and any(v["g0"] >= 20000 for v in vecs)
    assert any(4 in v["s1"] or 4 in v["s2"] for v in vecs if v["pname"] != "aa2aa")
    assert any(v["mode"] == "path" and v["g0"] > 1 and v["exp"][2] > 0 for v in vecs)


def test_pairs_without_a_suitable_band_are_counted(results):
    """Path mode returns the global fill's score; where it stays below the extension score (always for
    G0 > 1: the global score leaves G0 out) the reference prints a line and the engine counts."""
    vecs, got, no_band = results
    ext = {v["pair"]: v["exp"][0] for v in vecs if v["mode"] == "score"}
    total = 0
    for (pname, band, mode), (count, idx) in no_band.items():
        want = sum(1 for k in idx if vecs[k]["exp"][2] > 0 and vecs[k]["pair"] in ext and ext[vecs[k]["pair"]] > vecs[k]["exp"][0])
        known = all(vecs[k]["pair"] in ext for k in idx)
        if known:
            assert count == want, (pname, band, mode, count, want)
            total += count
    assert total > 50


def test_rebasing_past_32000(results):
    """The bwa preset over about 3 000 near-identical bases: the score passes 32000 and the rows are
    rebased by 16000 (stdaln.c:917-930), in every mode."""
    vecs, got, _ = results
    rows = [(v, g) for v, g in zip(vecs, got) if v["tag"] == "rebasing"]
    assert {v["mode"] for v, _ in rows} == {"score", "end", "path", "std2"}
    for v, g in rows:
        assert _same(g, v["exp"], v["mode"]), (v["mode"], v["g0"], g, v["exp"])
        assert g[0] > 32000
        assert v["s1"].size > 3000


def test_eh_in_lds_and_in_hbm_in_one_batch(golden_dir, gpu_engine):
    """Band len1 + len2: the ring is the whole eh row, len1 + 2 words, which lies in LDS up to 160 words
    per lane and in the wave's HBM scratch past that -- chosen per pair inside one launch."""
    vecs = [v for v in _vectors(golden_dir) if v["band"] == 0 and v["mode"] == "end" and v["pname"] == "blast"]
    sizes = [v["s1"].size + 2 for v in vecs]
    assert sum(1 for s in sizes if s <= 160) >= 10 and sum(1 for s in sizes if s > 160) >= 10 and {160, 161} <= set(sizes)
    got = gpu_engine.extend([v["s1"] for v in vecs], [v["s2"] for v in vecs], _param("blast", 0), g0=[v["g0"] for v in vecs])
    assert gpu_engine.stdaln_chunks()[0] == 1
    assert got == [v["exp"] for v in vecs]


def test_chunked_batch_is_identical(golden_dir):
    """Every nucleotide path-mode pair of up to 500 symbols, four times over, under one parameter set (the
    custom scheme, band len1 + len2): a scratch cap of 24 MiB holds one wave's traceback and the CIGAR
    rows of a few hundred pairs, so the batch runs in several launches, which must change nothing."""
    from ibwa_amd.engine import Engine
    vecs = [v for v in _vectors(golden_dir) if v["mode"] == "path" and v["pname"] != "aa2aa"
            and max(v["s1"].size, v["s2"].size) <= 500] * 4
    assert len(vecs) >= 600
    own = [v["pname"] == "match5" and v["band"] == 0 for v in vecs]
    assert sum(own) >= 20
    s1, s2, g0 = [v["s1"] for v in vecs], [v["s2"] for v in vecs], [v["g0"] for v in vecs]
    param = _param("match5", 0)
    eng = Engine(0)
    try:
        whole = eng.extend(s1, s2, param, g0=g0, mode="path")
        assert eng.stdaln_chunks()[0] == 1
        stats = eng.extend_stats()
        eng.set_option("stdaln_scratch_mb", 24)
        parts = eng.extend(s1, s2, param, g0=g0, mode="path")
        assert eng.stdaln_chunks()[0] > 1
        assert eng.extend_stats() == stats  # the count runs over the whole call
        std_whole = eng.stdaln(s1, s2, param, mode="extend")
        # a cap below one wave's scratch is refused, not truncated
        eng.set_option("stdaln_scratch_mb", 1)
        with pytest.raises(Exception, match="scratch"):
            eng.extend(s1, s2, param, g0=g0, mode="path")
        # end-cell mode needs none of it
        ends = eng.extend(s1, s2, param, g0=g0, mode="end")
    finally:
        eng.close()
    assert parts == whole
    assert [w for w, o in zip(whole, own) if o] == [v["exp"] for v, o in zip(vecs, own) if o]
    assert all(e[1] == w[1] for w, e in zip(whole, ends) if w[2] > 0)  # the path ends in the end cell
    # type 2 is G0 = 1: the same paths where the vector's G0 is 1
    for v, w, s in zip(vecs, whole, std_whole):
        if v["g0"] == 1 and w[2] > 0:
            assert (s[0], s[2], s[4], s[5]) == (w[0], w[2], w[1], w[3])


def test_empty_batches_and_refusals(gpu_engine):
    from ibwa_amd import engine as E
    for mode in ("score", "end", "path"):
        assert gpu_engine.extend([], [], "blast", mode=mode) == []
    assert gpu_engine.stdaln([], [], "blast", mode="extend") == []
    assert gpu_engine.extend([[], [1]], [[1], []], "blast") == [(-1, None)] * 2
    assert gpu_engine.extend([[], [1]], [[1], []], "blast", mode="path") == [(-1, None, 0, None)] * 2
    assert gpu_engine.stdaln([[], [1]], [[1], []], "blast", mode="extend") == [(-1, 0, 0, None, None, None)] * 2
    with pytest.raises(E.IbwaError, match="pair 1: G0 0 outside"):
        gpu_engine.extend([[0], [1]], [[0], [1]], "blast", g0=[1, 0])
    with pytest.raises(E.IbwaError, match=r"pair 0: seq2\[1\] = 7 is not below row"):
        gpu_engine.extend([[0, 1]], [[0, 7]], "blast")
    # one match from G0: best cell G0 + 1, returned less one
    assert gpu_engine.extend([[2]], [[2]], "blast", g0=41) == [(41, (1, 1))]
