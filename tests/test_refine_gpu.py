"""The device-resident reference and bwa_refine_gapped's two device stages (refine.hip): ibwa_ctx_load_pac /
ibwa_pac_extract against a Python unpack of the .pac files, ibwa_refine_batch and ibwa_md_batch against
the reference's own answers (tests/golden/refine_vectors.tsv.gz, tools/make_refine_golden.py), their
errors, a borrowing context, and the `samse` / `sampe` CLI on the device path (IBWA_REFINE_DEVICE=1) and
on the host path (IBWA_REFINE_HOST=1) against the golden SAM files of test_samse_gpu.py /
test_sampe_gpu.py."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import test_sampe_gpu as PE
from tests import test_samse_gpu as SE
from tests.test_refine_vectors import load_sets, load_vectors

pytestmark = pytest.mark.gpu

IBWA_EINVAL, IBWA_ENOINDEX = -2, -3


@pytest.fixture(scope="module")
def E():
    from ibwa_amd import engine
    return engine


@pytest.fixture(scope="module")
def vectors():
    return load_vectors()


@pytest.fixture(scope="module")
def sets():
    return load_sets()


@pytest.fixture(scope="module")
def eng(E, golden_dir):
    e = E.Engine(0)
    e.load_index_files(os.path.join(golden_dir, "g1m"))
    e.resident = None
    yield e
    e.close()


def use_set(eng, sets, name):
    """Make set `name` the engine's resident sequence (loading again replaces the other one)."""
    if eng.resident != name:
        parts = sets[name][1]
        eng.load_pac([p[0] for p in parts], [p[1] for p in parts])
        eng.resident = name
    return sets[name][0]


def jobs_of(vectors, name):
    return [v for v in vectors if v["set"] == name and v["ext"] != 0]


def check_refine(e, vs):
    pos1, cig = e.refine([v["pos"] for v in vs], [v["ext"] for v in vs], [v["codes"] for v in vs])
    bad = [(v, int(p), list(map(int, c))) for v, p, c in zip(vs, pos1, cig)
           if int(p) != v["pos1"] or list(map(int, c)) != v["cigar"]]
    assert not bad, f"{len(bad)} of {len(vs)} jobs differ; first: {bad[0]}"


@pytest.mark.parametrize("name", ["A", "B"])
def test_pac_extract_equals_unpacked_pac(eng, sets, name):
    text = use_set(eng, sets, name)
    T = len(text)
    first = sets[name][1][0][1]  # the first reference's l_pac: the boundary inside set B
    beg, lens = [], []
    for r in range(16):
        for ln in (0, 1, 3, 4, 5, 63, 64, 65):
            for b in (1600 + r, first - 40 + r, T - 30 + r):  # plain, across the boundary, across l_pac
                beg.append(b)
                lens.append(ln)
    for b in (0, T - 1, T, T + 1, T + 1000, 1 << 40):
        beg.append(b)
        lens.append(7)
    out, got = eng.pac_extract(beg, lens)
    for b, ln, o, g in zip(beg, lens, out, got):
        want = text[b:b + ln] if b < T else text[:0]
        assert g == len(want) and np.array_equal(o, want), (b, ln, g)
    assert all(g == 0 for b, g in zip(beg, got) if b >= T)
    if name == "B":
        assert any(b < first < b + g for b, g in zip(beg, got))


@pytest.mark.parametrize("name", ["A", "B"])
def test_refine_equals_reference(eng, sets, vectors, name):
    use_set(eng, sets, name)
    vs = jobs_of(vectors, name)
    assert len(vs) > 500
    check_refine(eng, vs)  # every vector in one call
    check_refine(eng, vs[::-1])  # order and batching do not matter
    check_refine(eng, vs[:len(vs) // 2])
    check_refine(eng, vs[len(vs) // 2:])


@pytest.mark.parametrize("name", ["A", "B"])
def test_md_equals_reference(eng, sets, vectors, name):
    use_set(eng, sets, name)
    vs = [v for v in vectors if v["set"] == name and v["md"] is not None]
    assert any(v["cigar"] is None for v in vs) and any(v["cigar"] is not None for v in vs)
    pos = [v["md_pos"] for v in vs]
    reads = [v["codes"] for v in vs]
    offs, text, nm = eng.md(pos, reads, [v["cigar"] for v in vs], raw=True)
    # compact, in read order, one NUL after each text
    want = b"".join(v["md"].encode() + b"\0" for v in vs)
    assert int(offs[0]) == 0 and int(offs[-1]) == len(text)
    assert [int(x) for x in np.diff(offs.astype(np.int64))] == [len(v["md"]) + 1 for v in vs]
    assert text == want
    assert [int(x) & 0xfff for x in nm] == [v["nm"] for v in vs]
    # the reads without a CIGAR alone, without a CIGAR array
    un = [v for v in vs if v["cigar"] is None]
    md, nm = eng.md([v["md_pos"] for v in un], [v["codes"] for v in un])
    assert md == [v["md"] for v in un] and [int(x) for x in nm] == [v["nm"] for v in un]
    # and the gapped ones alone, in reverse order
    ga = [v for v in vs if v["cigar"] is not None][::-1]
    md, nm = eng.md([v["md_pos"] for v in ga], [v["codes"] for v in ga], [v["cigar"] for v in ga])
    assert md == [v["md"] for v in ga] and [int(x) for x in nm] == [v["nm"] for v in ga]


def test_errors(E, eng, sets, vectors):
    # no sequence loaded -> IBWA_ENOINDEX from every call
    bare = E.Engine(0)
    one = [np.zeros(20, np.uint8)]
    for call in (lambda: bare.pac_extract([0], [4]), lambda: bare.refine([5], [1], one), lambda: bare.md([5], one),
                 lambda: bare.refine([], [], []), lambda: bare.md([], [])):
        with pytest.raises(E.IbwaError, match=f"ibwa error {IBWA_ENOINDEX}:"):
            call()
    bare.close()
    text = use_set(eng, sets, "A")
    T = len(text)
    # pos = l_pac + 1 fails the whole call, names the job and both numbers, and writes nothing
    vs = jobs_of(vectors, "A")[:8]
    pos = [v["pos"] for v in vs]
    pos[5] = T + 1
    po = np.full(len(vs), 0xDEADBEEF, np.uint64)
    nc = np.full(len(vs), -77, np.int32)
    with pytest.raises(E.IbwaError, match=rf"ibwa error {IBWA_EINVAL}:.*job 5.*position={T + 1} > l_pac={T}"):
        eng.refine(pos, [v["ext"] for v in vs], [v["codes"] for v in vs], pos_out=po, n_cigar=nc)
    assert (po == 0xDEADBEEF).all() and (nc == -77).all()
    # pos == l_pac is still a position (bwase.c:179: only pos > l_pac is fatal)
    edge = [v for v in jobs_of(vectors, "A") if v["pos"] == T]
    assert edge
    check_refine(eng, edge[:3])
    # n = 0 succeeds
    p, cg = eng.refine([], [], [])
    assert len(p) == 0 and cg == []
    md, nm = eng.md([], [])
    assert md == [] and len(nm) == 0
    offs, txt, nm = eng.md([], [], raw=True)
    assert list(offs) == [0] and txt == b""
    out, got = eng.pac_extract([], [])
    assert out == [] and len(got) == 0


def test_borrower_refines_without_loading(E, golden_dir, sets, vectors):
    parts = sets["B"][1]
    packed = sum(p[1] for p in parts) // 4
    lender = E.Engine(0)
    lender.load_index_files(os.path.join(golden_dir, "g1m"))
    d0 = E.Engine.device_bytes()[0]
    lender.load_pac([p[0] for p in parts], [p[1] for p in parts])
    d1 = E.Engine.device_bytes()[0]
    assert packed <= d1 - d0 <= packed + 4096  # the sequence once (the load's staging is released)
    lender.load_pac([p[0] for p in parts], [p[1] for p in parts])  # loading twice replaces it
    assert E.Engine.device_bytes()[0] == d1
    bor = E.Engine(0)
    bor.share_index(lender)
    assert E.Engine.device_bytes()[0] == d1  # lent, not copied
    with pytest.raises(E.IbwaError, match="shares another context's index"):
        bor.load_pac([p[0] for p in parts], [p[1] for p in parts])
    with pytest.raises(E.IbwaError, match="share this context's index"):
        lender.load_pac([p[0] for p in parts], [p[1] for p in parts])
    vs = jobs_of(vectors, "B")
    check_refine(bor, vs)
    md_vs = [v for v in vectors if v["set"] == "B" and v["md"] is not None][:200]
    md, nm = bor.md([v["md_pos"] for v in md_vs], [v["codes"] for v in md_vs], [v["cigar"] for v in md_vs])
    assert md == [v["md"] for v in md_vs]
    bor.close()
    lender.close()


def run_cli(cmd, args, host):
    """The CLI with refinement on the device (IBWA_REFINE_DEVICE=1; the host path is the measured
    default) or forced onto the host (IBWA_REFINE_HOST=1, which wins over the former)."""
    env = dict(os.environ, IBWA_REFINE_DEVICE="1")
    env.pop("IBWA_REFINE_HOST", None)
    if host:
        env["IBWA_REFINE_HOST"] = "1"
    r = subprocess.run([SE.CLI, cmd] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def same_sam(out, golden):
    want = SE._body(gzip.open(golden, "rt").read())
    got = SE._body(out.read_text())
    assert len(got) == len(want)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{len(bad)} lines differ; first:\n got {bad[0][1]}\nwant {bad[0][2]}"
    return got


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("key", ["mixed.n3o2e3", "r100.default.n10", "r150.default"])
def test_samse_cli_both_paths(golden_dir, key, host, tmp_path):
    m = SE.MANIFEST[key]
    g = lambda x: os.path.join(golden_dir, x)  # noqa: E731
    out = tmp_path / "out.sam"
    err = run_cli("samse", m["argv"] + ["-f", str(out), g(m.get("prefix", "g1m")), g(m["sai"]), g(m["reads"])], host)
    assert ("pac to device" in err) == (not host)
    got = same_sam(out, g(m["sam"]))
    assert any(ln.split("\t")[5].count("M") > 1 for ln in got if not ln.startswith("@")), "no gapped read in this case"


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("key", ["pe100.n5N20", "pe150.default", "pe70few.default"])
def test_sampe_cli_both_paths(golden_dir, key, host, tmp_path):
    m = PE.MANIFEST[key]
    g = lambda x: os.path.join(golden_dir, x)  # noqa: E731
    out = tmp_path / "out.sam"
    err = run_cli("sampe", m["argv"] + ["-f", str(out), g(m.get("prefix", "g1m")), *map(g, m["sai"]), *map(g, m["reads"])],
                  host)
    assert ("pac to device" in err) == (not host)
    same_sam(out, g(m["sam"]))


def test_sampe_two_workers_borrow_the_sequence(golden_dir, tmp_path):
    """`sampe -G 2` on one GPU with refinement on the device: the second worker's context borrows the
    sequence with the index (small batches, so that both workers refine)."""
    m = PE.MANIFEST["pe100.n5N20"]
    g = lambda x: os.path.join(golden_dir, x)  # noqa: E731
    out = tmp_path / "out.sam"
    os.environ["IBWA_SAMPE_BATCH"] = "211"
    try:
        err = run_cli("sampe", m["argv"] + ["-G", "2", "-f", str(out), g("g1m"), *map(g, m["sai"]), *map(g, m["reads"])],
                      host=False)
        one = tmp_path / "one.sam"
        run_cli("sampe", m["argv"] + ["-G", "1", "-f", str(one), g("g1m"), *map(g, m["sai"]), *map(g, m["reads"])],
                host=True)
    finally:
        del os.environ["IBWA_SAMPE_BATCH"]
    assert "pac to device" in err
    # small batches change the insert-size estimates, so the yardstick is one host worker on the same batches
    assert SE._body(out.read_text()) == SE._body(one.read_text())
    assert len(out.read_text().splitlines()) > 3000


def test_sampe_remap_keeps_host_path(golden_dir, tmp_path):
    m = PE.REMAP["remap.R"]
    g = lambda x: os.path.join(golden_dir, x)  # noqa: E731
    args = [g(m["prefixes"][0]), *map(g, m["sai"][0]), *map(g, m["reads"])]
    for pre, sai in zip(m["prefixes"][1:], m["sai"][1:]):
        args += [g(pre), *map(g, sai)]
    out = tmp_path / "out.sam"
    err = run_cli("sampe", m["argv"] + ["-f", str(out)] + args, host=False)
    assert "pac to device" not in err  # a set with a remap table: windows and CIGARs stay on the host
    got = same_sam(out, g(m["sam"]))
    assert any("\tZR:Z:" in ln for ln in got)
