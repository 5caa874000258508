"""stdaln_core.h's extend_core on the host: the statements k_extend runs (a lane's elements 64 apart)
instantiated with stride 1 and compared with the compiled reference's aln_extend_core
(oracle/_ref/libibwa_ref.so) in all three modes, with the eh ring and with the whole eh array, on
random pairs and on the fixed classes -- tests/host/extend_core_check.cpp, built here with g++."""
import os
import shutil
import subprocess

import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists(oracle.REF_LIB) or shutil.which("g++") is None,
                    reason="needs the compiled reference and g++")
def test_extend_core_equals_reference_on_host(tmp_path):
    exe = str(tmp_path / "extend_core_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "ibwa_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "extend_core_check.cpp"), "-ldl"], check=True)
    # the reference prints its "no suitable bandwidth" lines to stderr
    r = subprocess.run([exe, oracle.REF_LIB, "4000"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.strip().endswith(" 0 differ")
