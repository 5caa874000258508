"""GPU parity of the batched alignment with run-time scoring (stdaln.hip through Engine.stdaln).

* With the `bwa` preset it must reproduce what the project already pins for k_sw: every row of
  tests/golden/sw_vectors.tsv and sw_ties.tsv (local) and gsw_vectors.tsv (global, band 50, gap_end 5).
* tests/golden/stdsw/stdaln_vectors.tsv.gz (tools/make_stdsw_golden.py: the reference's aln_stdaln_aux with
  the blast and aa2aa presets, local and global, short lengths 1-200 against long lengths 1-4 096, the
  suboptimal-score, tie and threshold cases): score, subo, path length, ends and CIGAR, all equal.
* One batch that mixes the shapes gives the same results when the scratch cap forces several launches.
"""
import gzip
import os

import numpy as np
import pytest

import oracle

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
    return {"blast": nt, "aa2aa": aa, "match5": nt}


def _param(pname, **kw):
    """A preset, or the generator's custom scheme: match 5, anything else -2, gap open 10, extend 2."""
    import ibwa_amd
    if pname == "match5":
        base = {"gap_open": 10, "gap_ext": 2, "gap_end": 2, "row": 5, "band_width": 50,
                "matrix": np.where(np.eye(5, dtype=bool), 5, -2).astype(np.int32)}
    else:
        base = ibwa_amd.aln_param(pname)
    return dict(base, **kw)


def _encode(tab, s):
    return tab[np.frombuffer(s.encode(), dtype=np.uint8)] if s else np.zeros(0, np.uint8)


_vec_cache = []


def _vectors(golden_dir):
    """The TSV's rows, read once: dicts with the call's settings, the encoded pair and the expected tuple."""
    if _vec_cache:
        return _vec_cache
    tabs = _tables()
    for line in gzip.open(os.path.join(golden_dir, "stdsw", "stdaln_vectors.tsv.gz"), "rt"):
        if line.startswith("#"):
            continue
        f = line.rstrip("\n").split("\t")
        tag, pname, mode, thres, band, gap_end, s1, s2 = f[0], f[1], f[2], int(f[3]), int(f[4]), int(f[5]), f[6], f[7]
        score, plen = int(f[8]), int(f[10])
        if plen > 0:
            exp = (score, int(f[9]), plen, (int(f[11]), int(f[13])), (int(f[12]), int(f[14])), f[15])
        else:
            exp = (score, None, 0, None, None, None)  # no path: the reference sets nothing else
        _vec_cache.append({"tag": tag, "key": (pname, mode, thres, band, gap_end), "s1": _encode(tabs[pname], s1),
                           "s2": _encode(tabs[pname], s2), "exp": exp})
    return _vec_cache


def _run_groups(eng, vecs):
    """Every vector through Engine.stdaln, one batch per parameter set -> results in vecs' order."""
    groups = {}
    for k, v in enumerate(vecs):
        groups.setdefault(v["key"], []).append(k)
    got = [None] * len(vecs)
    for (pname, mode, thres, band, gap_end), idx in groups.items():
        param = _param(pname, band_width=band, gap_end=gap_end)
        res = eng.stdaln([vecs[k]["s1"] for k in idx], [vecs[k]["s2"] for k in idx], param, mode=mode, thres=thres)
        for k, r in zip(idx, res):
            got[k] = r
    return got


def _same(got, exp):
    if exp[2] == 0:  # no path: score and path_len only
        return got[0] == exp[0] and got[2] == 0
    return got == exp


def test_bwa_preset_reproduces_sw_vectors(golden_dir, gpu_engine):
    for name in ("sw_vectors.tsv", "sw_ties.tsv"):
        vecs = oracle.read_sw_vectors(os.path.join(golden_dir, name))
        got = gpu_engine.stdaln([oracle.nt4(v[0]) for v in vecs], [oracle.nt4(v[1]) for v in vecs], "bwa", mode="local", thres=1)
        assert len(got) == len(vecs)
        bad = []
        for k, (g, v) in enumerate(zip(got, vecs)):
            want = tuple(v[2:])  # score, path_len, start, end, cigar (the last three None without a path)
            mine = (g[0], g[2], g[3], g[4], g[5]) if want[2] is not None else (g[0], g[2], None, None, None)
            if mine != want:
                bad.append((k, g, want))
        assert not bad, (name, len(bad), bad[:5])


def test_bwa_preset_reproduces_global_vectors(golden_dir, gpu_engine):
    import ibwa_amd
    vecs = oracle.read_gsw_vectors(os.path.join(golden_dir, "gsw_vectors.tsv"))
    param = dict(ibwa_amd.aln_param("bwa"), band_width=50, gap_end=5)
    got = gpu_engine.stdaln([oracle.nt4(v[0]) for v in vecs], [oracle.nt4(v[1]) for v in vecs], param, mode="global")
    bad = [(k, g, v[2:]) for k, (g, v) in enumerate(zip(got, vecs)) if (g[0], g[2], g[5] or "") != tuple(v[2:])]
    assert not bad, (len(bad), bad[:3])
    assert all(g[1] == 0 for g in got)  # no suboptimal score in global mode


@pytest.fixture(scope="module")
def vector_results(golden_dir, gpu_engine):
    vecs = _vectors(golden_dir)
    return vecs, _run_groups(gpu_engine, vecs)


def test_library_vectors(vector_results):
    vecs, got = vector_results
    assert len(vecs) >= 224 + 24 + 12 + 48 + 9
    for pname in ("blast", "aa2aa"):
        for mode in ("local", "global"):
            shapes = {(v["s1"].size, v["s2"].size) for v in vecs if v["tag"] == "grid" and v["key"][:2] == (pname, mode)}
            assert shapes == {(a, b) for a in (1, 2, 31, 32, 33, 64, 65, 200) for b in (1, 63, 64, 65, 257, 1000, 4096)}
    bad = [(k, v["tag"], v["key"], g, v["exp"]) for k, (v, g) in enumerate(zip(vecs, got)) if not _same(g, v["exp"])]
    assert not bad, (len(bad), bad[:5])


def test_suboptimal_score_cases(vector_results):
    vecs, got = vector_results
    seen = set()
    for v, g in zip(vecs, got):
        if not v["tag"].startswith("subo_"):
            continue
        seen.add(v["tag"])
        assert _same(g, v["exp"]), (v["tag"], g, v["exp"])
        if v["tag"] in ("subo_far_copy", "subo_near_copy"):
            assert g[1] == g[0]  # a second copy outside the window: as good as the hit
        if v["tag"] in ("subo_window_tail", "subo_window_head", "subo_whole", "subo_no_other"):
            assert g[1] < g[0]   # what lies inside the window does not count
    assert seen == {"subo_far_copy", "subo_near_copy", "subo_window_tail", "subo_window_head", "subo_hit_first",
                    "subo_hit_last", "subo_whole", "subo_no_other"}


def test_long_internal_gaps(vector_results):
    """Blocks of one sequence separated in the other by linkers twice their length: the optimal local
    path bridges them, so the hit spans several times the shorter sequence (a custom scheme with cheap
    gaps, and BLOSUM62); the path fill's scratch is sized for the longest such region."""
    vecs, got = vector_results
    spans = []
    for v, g in zip(vecs, got):
        if v["tag"].startswith("long_gap"):
            assert g == v["exp"], (v["tag"], v["key"], g, v["exp"])
            spans.append(max(g[4][0] - g[3][0], g[4][1] - g[3][1]) + 1 - min(v["s1"].size, v["s2"].size))
    assert len(spans) == 12 and max(spans) >= 400  # a region 400 symbols longer than the shorter sequence


def test_ties_and_thresholds(vector_results):
    vecs, got = vector_results
    n = {"tie": 0, "thres_equal": 0, "thres_above": 0}
    for v, g in zip(vecs, got):
        if v["tag"].startswith("tie_"):
            n["tie"] += 1
            assert g == v["exp"], (v["tag"], g, v["exp"])
        elif v["tag"] == "thres_equal":
            n["thres_equal"] += 1
            assert g == v["exp"] and g[2] > 0 and g[0] == v["key"][2]
        elif v["tag"] == "thres_above":
            n["thres_above"] += 1
            assert g[2] == 0 and g[0] == v["exp"][0] == v["key"][2] - 1 and g[3] is None
    assert n["tie"] >= 48 and n["thres_equal"] == 3 and n["thres_above"] == 3


def test_chunked_global_batch_is_identical(golden_dir):
    """Global mode has its own scratch layout (traceback for the whole matrix): every blast global
    pair as one batch (full band, gap_end 0), four times over, whole and under a 56 MiB cap, which holds
    one wave's scratch for the 200 x 4 096 pair and the CIGAR rows of 213 such pairs."""
    from ibwa_amd.engine import Engine
    vecs = [v for v in _vectors(golden_dir) if v["key"][:2] == ("blast", "global")] * 4
    assert len(vecs) == 224
    s1, s2 = [v["s1"] for v in vecs], [v["s2"] for v in vecs]
    param = _param("blast", band_width=0, gap_end=0)
    eng = Engine(0)
    try:
        whole = eng.stdaln(s1, s2, param, mode="global")
        assert eng.stdaln_chunks()[0] == 1
        eng.set_option("stdaln_scratch_mb", 56)
        parts = eng.stdaln(s1, s2, param, mode="global")
        assert eng.stdaln_chunks()[0] > 1
    finally:
        eng.close()
    assert parts == whole
    same_key = [(g, v["exp"]) for v, g in zip(vecs, whole) if v["key"][3:] == (0, 0)]
    assert len(same_key) >= 20 and all(g == e for g, e in same_key)


def test_mixed_lengths_cut_the_run_not_the_batch():
    """(2 000 x 10) next to (10 x 2 000), local mode: sized together a run plans 2 001 x 2 001 cells per lane;
    under a cap that holds either pair alone the run is cut between them and both are aligned."""
    from ibwa_amd.engine import Engine
    a, b = np.arange(2000, dtype=np.uint8) % 4, np.array([0, 1, 2, 3, 0, 0, 1, 2, 3, 1], np.uint8)
    eng = Engine(0)
    try:
        whole = eng.stdaln([a, b], [b, a], "blast")
        assert eng.stdaln_chunks()[0] == 1
        eng.set_option("stdaln_scratch_mb", 16)
        parts = eng.stdaln([a, b], [b, a], "blast")
        assert eng.stdaln_chunks()[0] == 2
    finally:
        eng.close()
    assert parts == whole and whole[0][2] > 0


def test_chunked_batch_is_identical(golden_dir):
    """The blast / local / full-band vectors as one batch, four times over: a scratch cap of 8 MiB cuts
    it into several launches, which must change nothing."""
    import ibwa_amd
    from ibwa_amd.engine import Engine
    vecs = [v for v in _vectors(golden_dir) if v["key"][:4] == ("blast", "local", 1, 0)] * 4
    assert len(vecs) > 200
    s1, s2 = [v["s1"] for v in vecs], [v["s2"] for v in vecs]
    param = dict(ibwa_amd.aln_param("blast"), band_width=0, gap_end=0)
    eng = Engine(0)
    try:
        whole = eng.stdaln(s1, s2, param)
        assert eng.stdaln_chunks()[0] == 1
        eng.set_option("stdaln_scratch_mb", 8)
        parts = eng.stdaln(s1, s2, param)
        assert eng.stdaln_chunks()[0] > 1
        # a cap below one wave's scratch is refused, not truncated
        eng.set_option("stdaln_scratch_mb", 1)
        with pytest.raises(Exception, match="scratch"):
            eng.stdaln(s1, s2, param)
    finally:
        eng.close()
    assert parts == whole
    bad = [(k, g, v["exp"]) for k, (v, g) in enumerate(zip(vecs, whole)) if not _same(g, v["exp"])]
    assert not bad, bad[:5]


@pytest.mark.parametrize("rows", [0, 4095])
def test_rescan_path_is_identical(golden_dir, rows):
    """Past option stdaln_suba_rows rows of seq2 (8 192 by default, above every vector here) a launch
    keeps no per-row maxima and runs the forward pass a second time for the suboptimal score: every
    local vector again with the threshold at 0 (no pair keeps them) and just below the longest seq2."""
    from ibwa_amd.engine import Engine
    vecs = [v for v in _vectors(golden_dir) if v["key"][1] == "local"]
    eng = Engine(0)
    try:
        eng.set_option("stdaln_suba_rows", rows)
        got = _run_groups(eng, vecs)
    finally:
        eng.close()
    bad = [(k, v["tag"], g, v["exp"]) for k, (v, g) in enumerate(zip(vecs, got)) if not _same(g, v["exp"])]
    assert not bad, (len(bad), bad[:5])


def test_refusals_on_the_device_path(gpu_engine):
    from ibwa_amd import engine as E
    with pytest.raises(E.IbwaError, match="not below row"):
        gpu_engine.stdaln([[0, 7]], [[0, 1]], "blast")
    with pytest.raises(E.IbwaError, match="> 32000"):
        gpu_engine.stdaln([np.zeros(3000, np.uint8)], [np.zeros(3000, np.uint8)], "aa2aa")
    # empty sequences: local -1 and no path, global 0 and no path
    assert gpu_engine.stdaln([[], [1]], [[1], []], "blast") == [(-1, 0, 0, None, None, None)] * 2
    assert gpu_engine.stdaln([[], [1]], [[1], []], "blast", mode="global") == [(0, 0, 0, None, None, None)] * 2
    assert gpu_engine.stdaln([], [], "blast") == []
