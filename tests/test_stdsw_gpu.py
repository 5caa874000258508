"""`ibwa-amd stdsw` against the reference's `stdsw`: stdout, stderr and exit status, byte for byte
(tests/golden/stdsw/*.out / *.err, recorded from the compiled reference by tools/make_stdsw_golden.py).
"""
import json
import os
import subprocess

import pytest

from ibwa_amd import _native

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "stdsw")
CASES = [c for c in json.load(open(os.path.join(GOLD, "cases.json"))) if c["long"]]


def _run(args, long_, short):
    r = subprocess.run([_native.BIN_PATH, "stdsw"] + args + [os.path.join(GOLD, long_), os.path.join(GOLD, short)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return r.returncode, r.stdout, r.stderr


def _gold(name, ext):
    return open(os.path.join(GOLD, name + ext), "rb").read()


def test_cases_cover_the_issue():
    by = {c["name"]: c for c in CASES}
    assert by["default"]["args"] == [] and by["forward"]["args"] == ["-f"] and by["reverse"]["args"] == ["-r"]
    assert by["thres30"]["args"] == ["-T", "30"] and by["global_f"]["args"] == ["-g", "-f"] and by["protein"]["args"] == ["-p"]
    assert by["gzip"]["short"].endswith(".gz") and by["s300"]["short"] == "short300.fa.gz"
    assert _gold("thres30", ".out").count(b">") < _gold("default", ".out").count(b">")  # -T cuts records
    assert _gold("s300", ".out").count(b">L1\t") == 300
    mixed = open(os.path.join(GOLD, "short_mixed.fa")).read()
    assert any(ch in mixed for ch in "acgt") and "N" in mixed and any(ch in mixed for ch in "RYKMSWBDHV")
    assert max(len(x) for x in open(os.path.join(GOLD, "long_nt.fa")).read().split("\n")) <= 60  # multi-line


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cli_matches_reference(case):
    rc, out, err = _run(case["args"], case["long"], case["short"])
    want_out, want_err = _gold(case["name"], ".out"), _gold(case["name"], ".err")
    assert err == want_err
    assert rc == case["status"] == 0
    if out != want_out:
        a, b = out.split(b"\n"), want_out.split(b"\n")
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail(f"stdout differs at line {k + 1}: {a[k:k + 1]} != {b[k:k + 1]} ({len(a)} vs {len(b)} lines)")


def _records(text):
    """stdout -> {(short, strand): record text} (a record is its '>' line and three more)."""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    out = {}
    for k in range(0, len(lines) - 1, 4):
        f = lines[k].split(b"\t")
        assert lines[k].startswith(b">") and (f[3], f[4]) not in out
        out[(f[3], f[4])] = b"\n".join(lines[k:k + 4]) + b"\n"
    return out


def test_several_long_sequences(tmp_path):
    """Three long sequences in one file: every short and strand against every long, in the order short,
    strand, long -- assembled from the reference's outputs for each long alone."""
    singles = [_records(_gold(n, ".out")) for n in ("few_La", "few_Lb", "few_Lc")]
    shorts = [ln[1:].split()[0].encode() for ln in open(os.path.join(GOLD, "short_few.fa")) if ln.startswith(">")]
    want = b""
    for s in shorts:
        for strand in (b"+", b"-"):
            for one in singles:
                want += one.get((s, strand), b"")
    assert want.count(b">") >= 3 * len(shorts)
    long3 = tmp_path / "long3.fa"
    long3.write_text("".join(open(os.path.join(GOLD, f"long_{n}.fa")).read() for n in ("La", "Lb", "Lc")))
    rc, out, err = _run([], str(long3), "short_few.fa")
    assert err == b"[load_seqs] 3 sequences are loaded.\n"
    assert rc == 0 and out == want
