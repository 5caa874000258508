"""`ibwa-amd stdsw` without a device: the usage text and the refusals that come before any alignment."""
import json
import os
import subprocess

import pytest

from ibwa_amd import _native


def _run(args):
    r = subprocess.run([_native.BIN_PATH, "stdsw"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture()
def fa(tmp_path):
    def write(name, recs):
        p = tmp_path / name
        p.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
        return str(p)
    return write


def test_usage_text_and_status(golden_dir):
    """No file, or one: the reference's usage text on stderr, nothing on stdout, exit status 1."""
    d = os.path.join(golden_dir, "stdsw")
    case = [c for c in json.load(open(os.path.join(d, "cases.json"))) if c["name"] == "usage"][0]
    want = open(os.path.join(d, "usage.err"), "rb").read()
    assert want.startswith(b"\nUsage:") and case["status"] == 1
    for args in ([], ["-f"], ["only_one.fa"]):
        assert _run(args) == (1, b"", want), args
    # -T shows in the text as the reference prints it
    assert _run(["-T", "7"]) == (1, b"", want.replace(b"[1]", b"[7]"))


def test_missing_file(fa):
    short = fa("s.fa", [("s", "ACGT")])
    rc, out, err = _run([os.path.join(os.path.dirname(short), "none.fa"), short])
    assert rc == 1 and out == b"" and b"none.fa" in err
    long_ = fa("l.fa", [("L", "ACGTACGT")])
    rc, out, err = _run([long_, os.path.join(os.path.dirname(short), "none.fa")])
    assert rc == 1 and out == b"" and b"none.fa" in err


@pytest.mark.parametrize("t", ["0", "-3"])
def test_threshold_below_one_is_refused(fa, t):
    rc, out, err = _run(["-T", t, fa("l.fa", [("L", "ACGTACGT")]), fa("s.fa", [("s", "ACGT")])])
    assert rc == 1 and out == b"" and b"-T" in err


def test_gap_character_is_refused(fa):
    long_ = fa("l.fa", [("L", "ACGTACGTAC")])
    rc, out, err = _run([long_, fa("s.fa", [("ok", "ACGT"), ("gappy", "AC-GT")])])
    assert rc == 1 and out == b"" and b"'gappy'" in err and b"'-'" in err
    rc, out, err = _run([fa("l2.fa", [("Lgap", "ACG-TACGT")]), fa("s2.fa", [("ok", "ACGT")])])
    assert rc == 1 and out == b"" and b"'Lgap'" in err
    rc, out, err = _run(["-p", fa("l3.fa", [("P", "ARNDC")]), fa("s3.fa", [("pg", "AR-ND")])])
    assert rc == 1 and out == b"" and b"'pg'" in err


def test_empty_sequence_with_global_is_refused(fa):
    long_ = fa("l.fa", [("L", "ACGTACGTAC")])
    rc, out, err = _run(["-g", long_, fa("s.fa", [("ok", "ACGT"), ("nothing", "")])])
    assert rc == 1 and out == b"" and b"'nothing'" in err
    rc, out, err = _run(["-g", fa("l2.fa", [("void", "")]), fa("s2.fa", [("ok", "ACGT")])])
    assert rc == 1 and out == b"" and b"'void'" in err


def test_overflow_rule_is_refused(fa):
    """A short of 32 001 bases against a longer sequence: max_score 1 * 32 001 > 32 000."""
    rc, out, err = _run([fa("l.fa", [("L", "ACGT" * 8100)]), fa("s.fa", [("big", "A" * 32001)])])
    assert rc == 1 and out == b"" and b"> 32000" in err
