"""Colour-space reads through the CLI: `aln -c` on the colour index, then `samse` / `sampe` with
bwa_refine_gapped's colour branch (bwase.c:367-388: bwa_cs2nt_core on the GPU, the second refinement
pass and MD/NM against <prefix>.nt) against the reference's own output on the colour fixtures
(tools/make_cs_golden.py, cs_manifest.json).  The .sai is compared past its header, every SAM line
byte for byte except @PG, which names the program that wrote the file."""
import gzip
import json
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "ibwa_amd", "bin", "ibwa-amd")
MANIFEST = json.load(open(os.path.join(ROOT, "tests", "golden", "cs_manifest.json")))
HDR = 64  # sizeof(gap_opt_t): the .sai header (its n_threads differs, bwtaln.c:192)


def _body(text):
    return [ln for ln in text.splitlines() if not ln.startswith("@PG")]


def _same_sam(out, golden_dir, m):
    want = _body(gzip.open(os.path.join(golden_dir, m["sam"]), "rt").read())
    got = _body(out.read_text())
    assert len(got) == len(want)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{len(bad)} lines differ; first:\n got {bad[0][1]}\nwant {bad[0][2]}"


@pytest.mark.parametrize("key", sorted(MANIFEST["aln"]))
def test_aln_c_sai_matches_reference(golden_dir, key, tmp_path):
    m = MANIFEST["aln"][key]
    sai = tmp_path / "out.sai"
    r = subprocess.run([CLI, "aln"] + m["argv"] + ["-f", str(sai), os.path.join(golden_dir, m["prefix"]),
                                                   os.path.join(golden_dir, m["reads"])],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    want = open(os.path.join(golden_dir, m["sai"]), "rb").read()
    got = sai.read_bytes()
    assert len(got) == len(want) > HDR and got[HDR:] == want[HDR:]


@pytest.mark.parametrize("key", sorted(MANIFEST["samse"]))
def test_samse_matches_reference(golden_dir, key, tmp_path):
    m = MANIFEST["samse"][key]
    out = tmp_path / "out.sam"
    r = subprocess.run([CLI, "samse"] + m["argv"] + ["-f", str(out), os.path.join(golden_dir, m["prefix"]),
                                                     os.path.join(golden_dir, m["sai"]),
                                                     os.path.join(golden_dir, m["reads"])],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    _same_sam(out, golden_dir, m)


def _sampe(golden_dir, m, out, extra=()):
    return subprocess.run([CLI, "sampe"] + m["argv"] + list(extra) +
                          ["-f", str(out), os.path.join(golden_dir, m["prefix"]),
                           *[os.path.join(golden_dir, x) for x in m["sai"]],
                           *[os.path.join(golden_dir, x) for x in m["reads"]]],
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("key", sorted(MANIFEST["sampe"]))
def test_sampe_matches_reference(golden_dir, key, tmp_path):
    m = MANIFEST["sampe"][key]
    out = tmp_path / "out.sam"
    r = _sampe(golden_dir, m, out)
    assert r.returncode == 0, r.stderr[-2000:]
    _same_sam(out, golden_dir, m)


def test_sampe_two_workers_equal_one(golden_dir, tmp_path):
    """-G 2: the second worker borrows the nucleotide sequence with the index (ibwa_ctx_share_index)."""
    m = MANIFEST["sampe"]["cs.R"]
    out = tmp_path / "out.sam"
    r = _sampe(golden_dir, m, out, ["-G", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    _same_sam(out, golden_dir, m)


def test_sampe_refuses_a_colour_set_with_a_remap_table(golden_dir, tmp_path):
    for f in MANIFEST["index"]:
        shutil.copy(os.path.join(golden_dir, f), tmp_path / f)
    (tmp_path / "csg.remap").write_text(">csA-csA|exact|\n\n")
    m = dict(MANIFEST["sampe"]["cs.R"], prefix=str(tmp_path / "csg"))
    r = _sampe(golden_dir, m, tmp_path / "out.sam")
    assert r.returncode != 0 and "remap table" in r.stderr


def test_samse_names_the_missing_nt_file(golden_dir, tmp_path):
    for f in MANIFEST["index"]:
        if f != "csg.nt.pac":
            shutil.copy(os.path.join(golden_dir, f), tmp_path / f)
    m = MANIFEST["samse"]["cs_edge.default"]
    r = subprocess.run([CLI, "samse", "-f", str(tmp_path / "out.sam"), str(tmp_path / "csg"),
                        os.path.join(golden_dir, m["sai"]), os.path.join(golden_dir, m["reads"])],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "csg.nt.pac" in r.stderr
