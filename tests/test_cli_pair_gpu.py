"""`ibwa-amd aln -f out1.sai -F out2.sai <prefix> <in1.fq> <in2.fq>` (aln_main.cpp, pair mode):
both ends of a pair aligned by one process sharing the arena, the index and the lanes.  Each
output is byte for byte what a single-input run on that input writes, so the bar is the
reference's own .sai for each end (tests/golden, sampe_manifest.json / sai_manifest.json /
bam_manifest.json), n_threads header field masked (bwtaln.c:192), whatever the interleaving of
the two inputs' groups on the lanes.  Every CLI run is its own process; they run one at a time."""
import gzip
import json
import os
import subprocess

import pytest

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "ibwa_amd", "bin", "ibwa-amd")
SMALL = {"IBWA_ALN_SUBBATCH": "64", "IBWA_ALN_GROUP": "2"}  # many small groups from both inputs


def gold(golden_dir, name):
    with open(os.path.join(golden_dir, name), "rb") as f:
        return f.read()


def run_pair(argv, inputs, tmp_path, env=None, name="p", prefix=None, golden_dir=None):
    """One pair-mode run -> (out1 bytes, out2 bytes, stderr)."""
    o1, o2 = tmp_path / (name + "_1.sai"), tmp_path / (name + "_2.sai")
    r = subprocess.run([CLI, "aln"] + argv + ["-f", str(o1), "-F", str(o2), prefix or os.path.join(golden_dir, "g1m")] +
                       [str(x) for x in inputs],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-2000:]
    return o1.read_bytes(), o2.read_bytes(), r.stderr


def run_single(argv, reads, tmp_path, golden_dir, env=None, name="s.sai", extra=()):
    out = tmp_path / name
    r = subprocess.run([CLI, "aln"] + argv + ["-f", str(out), os.path.join(golden_dir, "g1m"), str(reads)] + list(extra),
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_bytes()


@pytest.fixture(scope="module")
def sampe_manifest(golden_dir):
    with open(os.path.join(golden_dir, "sampe_manifest.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("key", ["pe100.default", "pe100.q20", "pe100.k0n3", "pe150.default", "pe70few.default"])
def test_pair_equals_reference(golden_dir, sampe_manifest, key, tmp_path):
    """One pair-mode run per golden paired case: both outputs are the reference's .sai."""
    m = sampe_manifest[key]
    a, b, err = run_pair(m["aln_argv"], [os.path.join(golden_dir, x) for x in m["reads"]], tmp_path, golden_dir=golden_dir)
    assert oracle.sai_body_equal(a, gold(golden_dir, m["sai"][0]))
    assert oracle.sai_body_equal(b, gold(golden_dir, m["sai"][1]))
    # the lines that count reads say which input they are about; the memory report comes once
    assert "sequences have been processed. [in1]" in err and "sequences have been processed. [in2]" in err
    assert err.count("device memory: peak") == 1


@pytest.mark.parametrize("extra", [["lanes", "1"], ["lanes", "2"], ["lanes", "3"], ["-G", "2"], ["-G", "3"]],
                         ids=lambda e: "".join(e))
def test_pair_order_under_interleaving(golden_dir, sampe_manifest, extra, tmp_path):
    """Small groups of both inputs taking turns on 1, 2 or 3 lanes, and on 2 or 3 GPU slices (the
    one-GPU rehearsal of -G): each output keeps its input's order and equals the reference's."""
    m = sampe_manifest["pe100.default"]
    env, argv = dict(SMALL), list(m["aln_argv"])
    if extra[0] == "lanes":
        env["IBWA_ALN_LANES"] = extra[1]
    else:
        env["IBWA_ALN_LANES"] = "2"
        argv += extra
    a, b, _ = run_pair(argv, [os.path.join(golden_dir, x) for x in m["reads"]], tmp_path, env, golden_dir=golden_dir)
    assert oracle.sai_body_equal(a, gold(golden_dir, m["sai"][0]))
    assert oracle.sai_body_equal(b, gold(golden_dir, m["sai"][1]))


def test_pair_unequal_inputs(golden_dir, tmp_path):
    """100 bp and 36 bp reads as the two inputs: read lengths and batch-level options (max_diff,
    bwtaln.c:86-93) differ and input 2's groups are smaller, so one input runs out of groups first
    and the other takes every lane."""
    for order in ((("reads_r100.fq", "r100.default.sai"), ("reads_r36.fq", "r36.default.sai")),
                  (("reads_r36.fq", "r36.default.sai"), ("reads_r100.fq", "r100.default.sai"))):
        a, b, _ = run_pair([], [os.path.join(golden_dir, order[0][0]), os.path.join(golden_dir, order[1][0])], tmp_path,
                           SMALL, golden_dir=golden_dir)
        assert oracle.sai_body_equal(a, gold(golden_dir, order[0][1]))
        assert oracle.sai_body_equal(b, gold(golden_dir, order[1][1]))


def test_pair_unequal_read_counts(golden_dir, tmp_path):
    """Inputs of different read counts (aln does not pair reads): the first 400 reads of the 100 bp
    file next to the whole file; out1 is the prefix of the golden records those reads have."""
    src = gold(golden_dir, "reads_r100.fq").split(b"\n")
    short = tmp_path / "short.fq"
    short.write_bytes(b"\n".join(src[:1600]) + b"\n")
    a, b, _ = run_pair([], [short, os.path.join(golden_dir, "reads_r100.fq")], tmp_path, SMALL, golden_dir=golden_dir)
    ref = gold(golden_dir, "r100.default.sai")
    assert oracle.sai_body_equal(b, ref)
    assert len(a) > 64 + 4 * 400 and ref[64:].startswith(a[64:])
    pos, n = 64, 0
    while pos < len(a):  # 400 records
        pos += 4 + 16 * int.from_bytes(a[pos:pos + 4], "little", signed=True)
        n += 1
    assert n == 400 and pos == len(a)


def test_pair_same_mixed_file_twice(golden_dir, tmp_path):
    """Mixed read lengths given as both inputs: groups split where the batch key changes, in both."""
    fq = os.path.join(golden_dir, "reads_mixed.fq")
    ref = gold(golden_dir, "mixed.default.sai")
    for env in (SMALL, {"IBWA_ALN_SUBBATCH": "16", "IBWA_ALN_GROUP": "4", "IBWA_ALN_LANES": "3"}):
        a, b, _ = run_pair([], [fq, fq], tmp_path, env, golden_dir=golden_dir)
        assert oracle.sai_body_equal(a, ref) and oracle.sai_body_equal(b, ref)


def test_pair_mixed_ingest_gzip(golden_dir, tmp_path):
    """Input 1 plain, input 2 the same reads as a single-member gzip file (inflated on one host
    thread ahead of the device parse): each output equals the single-input run of that file, on
    the device parse and with input 2 kept on the host readers (gzread, IBWA_GZ_PARALLEL=0)."""
    fq = os.path.join(golden_dir, "reads_r100.fq")
    gz = tmp_path / "r100.fq.gz"
    with open(gz, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as z:
        z.write(gold(golden_dir, "reads_r100.fq"))
    ref = gold(golden_dir, "r100.default.sai")
    env = {"IBWA_ALN_SUBBATCH": "200", "IBWA_ALN_GROUP": "3"}
    one = run_single([], gz, tmp_path, golden_dir, env)
    assert oracle.sai_body_equal(one, ref)
    for extra in ({}, {"IBWA_FQ_PIECE_BYTES": "30000"}, {"IBWA_GZ_PARALLEL": "0"}):
        a, b, _ = run_pair([], [fq, gz], tmp_path, dict(env, **extra), golden_dir=golden_dir)
        assert oracle.sai_body_equal(a, ref), extra
        assert b == one, extra
    b2, a2, _ = run_pair([], [gz, fq], tmp_path, env, golden_dir=golden_dir)  # and the other way round
    assert oracle.sai_body_equal(a2, ref) and b2 == one


def _irregular(golden_dir, path):
    """tests/test_cli_gpu.py's irregular file: strict records, then CRLF records, then records whose
    sequence is wrapped over two lines -- the host readers take over in the middle of the file."""
    src = gold(golden_dir, "reads_mixed.fq").split(b"\n")
    recs = [src[i:i + 4] for i in range(0, len(src) - 3, 4)]
    head, mid, tail = recs[:len(recs) // 2], recs[len(recs) // 2:len(recs) // 2 + 40], recs[len(recs) // 2 + 40:]
    text = b"".join(b"\n".join(r) + b"\n" for r in head)
    text += b"".join(b"\r\n".join(r) + b"\r\n" for r in mid)
    for r in tail:
        s = r[1]
        text += r[0] + b"\n" + s[:len(s) // 2] + b"\n" + s[len(s) // 2:] + b"\n" + r[2] + b"\n" + r[3] + b"\n"
    path.write_bytes(text)


def test_pair_handoff_in_one_input(golden_dir, tmp_path):
    """Input 1 hands over to the host readers mid-file (CRLF and wrapped records) while input 2
    stays on the device parse: each output equals the single-input run of its file, and input 2's
    the reference's."""
    bad = tmp_path / "irregular.fq"
    _irregular(golden_dir, bad)
    fq = os.path.join(golden_dir, "reads_r100.fq")
    env = {"IBWA_ALN_SUBBATCH": "96", "IBWA_ALN_GROUP": "3"}
    one = run_single([], bad, tmp_path, golden_dir, env)
    ser = run_single([], bad, tmp_path, golden_dir, dict(env, IBWA_ALN_SERIAL_READ="1"), "ser.sai")
    assert len(one) > 64 and one == ser
    a, b, err = run_pair([], [bad, fq], tmp_path, env, golden_dir=golden_dir)
    assert a == one
    assert oracle.sai_body_equal(b, gold(golden_dir, "r100.default.sai"))
    assert "the host readers take over at byte" in err and "[in1]" in err
    b2, a2, _ = run_pair([], [fq, bad], tmp_path, env, golden_dir=golden_dir)
    assert a2 == one and oracle.sai_body_equal(b2, gold(golden_dir, "r100.default.sai"))


def test_pair_empty_second_input(golden_dir, tmp_path):
    """An empty input 2: its output is the 64-byte header alone, input 1's output is complete."""
    empty = tmp_path / "empty.fq"
    empty.write_bytes(b"")
    a, b, _ = run_pair([], [os.path.join(golden_dir, "reads_r100.fq"), empty], tmp_path, SMALL, golden_dir=golden_dir)
    assert oracle.sai_body_equal(a, gold(golden_dir, "r100.default.sai"))
    assert len(b) == 64 and b == a[:64]


def test_pair_truncated_second_input(golden_dir, tmp_path):
    """Input 2 ends inside its last record (kseq_read's -2): every read before it is kept."""
    a, b, _ = run_pair([], [os.path.join(golden_dir, "reads_r100.fq"), os.path.join(golden_dir, "reads_trunc_q.fq")],
                       tmp_path, golden_dir=golden_dir)
    assert oracle.sai_body_equal(a, gold(golden_dir, "r100.default.sai"))
    assert oracle.sai_body_equal(b, gold(golden_dir, "trunc_q.default.sai"))


def test_pair_bam(golden_dir, tmp_path):
    """-b -f a -F b <prefix> reads.bam: the BAM's first reads to -f with the header -b -1 writes, its
    second reads to -F with the header of -b -2 (bwa_read_bam, bwaseqio.c:89-143)."""
    for env in ({}, SMALL):
        a, b, _ = run_pair(["-b"], [os.path.join(golden_dir, "reads.bam")], tmp_path, env, golden_dir=golden_dir)
        assert oracle.sai_body_equal(a, gold(golden_dir, "bam.r1.sai"))
        assert oracle.sai_body_equal(b, gold(golden_dir, "bam.r2.sai"))


def test_pair_errors(golden_dir, tmp_path):
    """Misuse of -F exits non-zero with a message, before any GPU work (no arena, no index load:
    HIP_VISIBLE_DEVICES hides every device and the message is still the usage error) and without
    output written."""
    P, fq = os.path.join(golden_dir, "g1m"), os.path.join(golden_dir, "reads_r100.fq")
    a, b = str(tmp_path / "a.sai"), str(tmp_path / "b.sai")
    cases = [
        (["-F", b, P, fq, fq], "-F needs -f"),
        (["-f", a, "-F", a, P, fq, fq], "same file"),
        (["-f", a, "-F", b, P, fq], "<in1.fq> <in2.fq>"),
        (["-b", "-1", "-f", a, "-F", b, P, os.path.join(golden_dir, "reads.bam")], "cannot be combined with -F"),
        (["-f", a, "-F", b, P, fq, str(tmp_path / "missing.fq")], "cannot open"),
    ]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    for argv, msg in cases:
        r = subprocess.run([CLI, "aln"] + argv, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode != 0, argv
        assert msg in r.stderr, (argv, r.stderr[-500:])
        assert "no HIP device" not in r.stderr and "arena" not in r.stderr, (argv, r.stderr[-500:])
        assert not os.path.exists(a) and not os.path.exists(b), argv


def test_single_mode_ignores_extra_positional(golden_dir, tmp_path):
    """Without -F nothing changes: a third positional argument is still ignored, and the lines that
    count reads carry no input tag."""
    out = tmp_path / "out.sai"
    r = subprocess.run([CLI, "aln", "-f", str(out), os.path.join(golden_dir, "g1m"),
                        os.path.join(golden_dir, "reads_r100.fq"), "extra_positional"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert oracle.sai_body_equal(out.read_bytes(), gold(golden_dir, "r100.default.sai"))
    assert "[in1]" not in r.stderr and "[in2]" not in r.stderr
    assert "sequences have been processed.\n" in r.stderr
