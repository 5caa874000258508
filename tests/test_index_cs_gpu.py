"""The colour index: `ibwa-amd index_cs` writes the eleven files of the reference's `index -c`
(bwtindex.c:85-101 and the common tail) and `ibwa-amd pac2cspac` the reference's colour .pac
(bwtmisc.c:221-246), byte for byte equal to the fixtures the reference built (tools/make_cs_golden.py)."""
import json
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "ibwa_amd", "bin", "ibwa-amd")
EXTS = [".nt.pac", ".nt.ann", ".nt.amb", ".pac", ".ann", ".amb", ".rpac", ".bwt", ".rbwt", ".sa", ".rsa"]


def _same(golden_dir, tmp_path, prefix, exts):
    for e in exts:
        got = (tmp_path / (prefix + e)).read_bytes()
        want = open(os.path.join(golden_dir, "csg" + e), "rb").read()
        assert got == want, f"{prefix}{e}: {len(got)} bytes, fixture {len(want)}"


def test_index_cs_writes_the_reference_file_set(golden_dir, tmp_path):
    man = json.load(open(os.path.join(golden_dir, "cs_manifest.json")))
    assert man["index"] == ["csg" + e for e in EXTS]
    r = subprocess.run([CLI, "index_cs", "-p", str(tmp_path / "out"), os.path.join(golden_dir, "csg.fa")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == sorted("out" + e for e in EXTS)
    _same(golden_dir, tmp_path, "out", EXTS)


def test_index_cs_default_prefix_and_algorithm(golden_dir, tmp_path):
    shutil.copy(os.path.join(golden_dir, "csg.fa"), tmp_path / "g.fa")
    r = subprocess.run([CLI, "index_cs", "-a", "is", str(tmp_path / "g.fa")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    _same(golden_dir, tmp_path, "g.fa", EXTS)
    r = subprocess.run([CLI, "index_cs", "-a", "nope", str(tmp_path / "g.fa")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "unknown algorithm" in r.stderr


def test_pac2cspac_command(golden_dir, tmp_path):
    r = subprocess.run([CLI, "pac2cspac", os.path.join(golden_dir, "csg.nt"), str(tmp_path / "cs")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == ["cs.amb", "cs.ann", "cs.pac"]
    _same(golden_dir, tmp_path, "cs", [".pac", ".ann", ".amb"])
    r = subprocess.run([CLI, "pac2cspac", str(tmp_path / "missing"), str(tmp_path / "cs2")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "missing.ann" in r.stderr
