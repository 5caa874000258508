"""Read sets of tests/golden/aln_edges/ (tools/make_aln_edges_golden.py).

The small sets on the 300 bp text are committed as FASTQ.  The sets on g1m are not (they would be
half a megabyte): aln_edges/reads.json describes each as a list of items, rebuilt here from files
that are committed already --

  ["fastq", file, start, stop]            records start..stop-1 of tests/golden/<file>
  ["cut", name, pos, len, rc, [[offset, base], ...]]
                                          len bases of the g1m text (g1m.pac) from pos, the bases at
                                          the offsets replaced, then reverse-complemented if rc;
                                          quality 'I'

The same function gives the generator the reads it runs the reference on and the tests theirs.
"""
import json
import os

import oracle

_RC = bytes.maketrans(b"ACGT", b"TGCA")
_text = {}
_recipes = {}


def _g1m_text(golden_dir):
    if golden_dir not in _text:
        codes, _ = oracle.read_pac(os.path.join(golden_dir, "g1m"))
        _text[golden_dir] = bytes(b"ACGT"[c] for c in codes)
    return _text[golden_dir]


def records(golden_dir, name):
    """The records of read set `name` as oracle.read_fastq_records gives them: (name, seq, qual)."""
    path = os.path.join(golden_dir, "aln_edges", name)
    if os.path.exists(path):
        return oracle.read_fastq_records(path)
    if golden_dir not in _recipes:
        with open(os.path.join(golden_dir, "aln_edges", "reads.json")) as f:
            _recipes[golden_dir] = json.load(f)
    out = []
    for item in _recipes[golden_dir][name]:
        if item[0] == "fastq":
            out += oracle.read_fastq_records(os.path.join(golden_dir, item[1]))[item[2]:item[3]]
        else:
            _, nm, pos, n, rc, subs = item
            s = bytearray(_g1m_text(golden_dir)[pos:pos + n])
            assert len(s) == n
            for off, base in subs:
                assert s[off] != ord(base)
                s[off] = ord(base)
            s = bytes(s)
            out.append((nm, s[::-1].translate(_RC) if rc else s, b"I" * n))
    return out


def write_fastq(path, recs):
    with open(path, "wb") as f:
        for nm, s, q in recs:
            f.write(b"@" + nm.encode() + b"\n" + s + b"\n+\n" + q + b"\n")
    return path
