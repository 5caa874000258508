#!/usr/bin/env python3
"""Generate the colour-space fixtures under tests/golden/ (build container only).

TEST INFRASTRUCTURE.  Everything here is data the reference's own programs read or write:
  csg.fa and its eleven `index -c` files (csg.nt.{pac,ann,amb}, csg.{pac,ann,amb,rpac,bwt,rbwt,sa,rsa});
  cs_r1.fq / cs_r2.fq (pairs of 50 colours) and cs_edge.fq (reads at the sequence's edges), colours
  written as the letters ACGT for 0-3 and N for a missing colour;
  their `aln -c` .sai files;
  samse / sampe SAM texts, gzip'd, with cs_manifest.json (case -> command line, files, branch counts);
  cs2nt_vectors.tsv.gz: row pairs run through the reference's cs2nt_DP and cs2nt_nt_qual
  (oracle/_ref/libibwa_ref.so through ctypes), one per line: nt_ref digits, cs_read hex, result hex.
Seeded and deterministic.  Every reference command runs twice; a case whose two outputs differ is
dropped and the manifest says so.  The branch conditions at the end are asserted: when one fails,
adjust the read generator.
"""
import ctypes
import gzip
import json
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref", "ibwa_ref")
REFLIB = os.path.join(ROOT, "oracle", "_ref", "libibwa_ref.so")
SEED = 20261020
LIMIT = 400 * 1000  # bytes per committed file


def G(name):
    return os.path.join(GOLD, name)


def write_gz(name, data):
    with open(G(name), "wb") as raw:
        with gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
            f.write(data)
    assert os.path.getsize(G(name)) < LIMIT, name


# ---------------------------------------------------------------------------------------- genome
def make_genome(rnd):
    def rand_seq(n):
        return [rnd.randrange(4) for _ in range(n)]

    block = rand_seq(600)
    c1 = rand_seq(9000) + block + rand_seq(11000) + block + rand_seq(14403)
    c2 = rand_seq(8000) + block + rand_seq(16614)
    hole = (20000, 120)  # in contig 1, away from the blocks
    total = len(c1) + len(c2)
    assert total % 16 and total % 4, total
    names = ["csA", "csB"]
    with open(G("csg.fa"), "w") as f:
        for name, s, h in zip(names, (c1, c2), (hole, None)):
            txt = ["ACGT"[x] for x in s]
            if h:
                txt[h[0]:h[0] + h[1]] = "N" * h[1]
            txt = "".join(txt)
            f.write(f">{name}\n")
            for i in range(0, len(txt), 70):
                f.write(txt[i:i + 70] + "\n")
    blocks = [9000, 9000 + 600 + 11000, len(c1) + 8000]
    return c1, c2, hole, blocks


def unpack_pac(path):
    raw = open(path, "rb").read()
    l_pac = (len(raw) - 2) * 4 + raw[-1]
    return [(raw[i >> 2] >> ((~i & 3) << 1)) & 3 for i in range(l_pac)], l_pac


# ----------------------------------------------------------------------------------------- reads
def mutate(rnd, bases, n_sub=0, ins_at=None, del_at=None):
    b = list(bases)
    for _ in range(n_sub):
        i = rnd.randrange(3, len(b) - 3)
        b[i] = (b[i] + 1 + rnd.randrange(3)) & 3
    if ins_at is not None:
        b.insert(ins_at, rnd.randrange(4))
    if del_at is not None:
        del b[del_at]
    return b


def fq_record(rnd, name, cs, reverse, n_err=0, n_N=0, qlo=5, qhi=40):
    cs = list(cs)
    for _ in range(n_err):
        i = rnd.randrange(len(cs))
        cs[i] = (cs[i] + 1 + rnd.randrange(3)) & 3
    qual = [rnd.randint(qlo, qhi) for _ in cs]
    txt = ["ACGT"[x] for x in cs]
    for _ in range(n_N):
        txt[rnd.randrange(len(txt))] = "N"
    if reverse:
        txt.reverse()
    return f"@{name}\n{''.join(txt)}\n+\n{''.join(chr(33 + q) for q in qual)}\n"


def read_colours(rnd, nt, start, n_col, **mut):
    """n_col colours of a read whose first base is nt[start] (before mutation)."""
    extra = 1 if mut.get("del_at") is not None else 0
    short = 1 if mut.get("ins_at") is not None else 0
    bases = mutate(rnd, nt[start:start + n_col + 1 + extra - short], **mut)
    assert len(bases) == n_col + 1
    return [bases[j] ^ bases[j + 1] for j in range(n_col)]


def make_pairs(rnd, nt, l_pac, hole, blocks, n_pairs=600, n_col=50):
    r1, r2 = [], []
    lo_hole, hi_hole = hole[0] - 400, hole[0] + hole[1] + 400
    for i in range(n_pairs):
        kind = i % 12
        isize = rnd.randint(180, 320)
        if kind in (0, 1):  # from the repeated block, with an indel
            a = blocks[rnd.randrange(3)] + rnd.randrange(20, 250)
        else:
            while True:
                a = rnd.randrange(1, l_pac - isize - 2)
                if not (lo_hole < a < hi_hole):
                    break
        b = a + isize - (n_col + 1)
        m1, m2 = {}, {}
        if kind in (0, 1):
            m1 = {"ins_at": rnd.randrange(12, 40)} if kind == 0 else {"del_at": rnd.randrange(12, 40)}
        elif kind in (2, 3):
            m1 = {"del_at": rnd.randrange(10, 42)} if kind == 2 else {"ins_at": rnd.randrange(10, 42)}
            m2 = {"n_sub": 1}
        elif kind in (4, 5, 6):
            m2 = {"n_sub": rnd.choice((3, 4))}  # too far for aln: left to the mate rescue
            if kind == 6:
                m2["del_at"] = rnd.randrange(15, 35)
        elif kind == 7:
            m1 = {"n_sub": 1}
            m2 = {"ins_at": rnd.randrange(10, 42)}
        elif kind == 8:
            m1 = {"n_sub": 2}
        c1 = read_colours(rnd, nt, a, n_col, **m1)
        c2 = read_colours(rnd, nt, b, n_col, **m2)
        err1 = 1 if kind in (9, 10) else 0
        nn1 = 1 if kind == 11 else 0
        flip = rnd.random() < 0.5  # which end lies on the reverse strand
        r1.append(fq_record(rnd, f"p{i}", c1, flip, n_err=err1, n_N=nn1))
        r2.append(fq_record(rnd, f"p{i}", c2, not flip, n_err=1 if kind == 10 else 0, n_N=1 if i % 37 == 0 else 0))
    open(G("cs_r1.fq"), "w").write("".join(r1))
    open(G("cs_r2.fq"), "w").write("".join(r2))


def make_edge(rnd, nt, l_pac, len1, hole, n_col=50):
    recs = []

    def add(name, cs, rev, **kw):
        recs.append(fq_record(rnd, name, cs, rev, qlo=20, qhi=40, **kw))

    # position 0: the first symbol of the colour sequence is base 0 itself
    head = [nt[0]] + [nt[j - 1] ^ nt[j] for j in range(1, n_col)]
    add("start_f", head, False)
    add("start_r", head, True)
    # the last colour of the last contig
    tail = [nt[j - 1] ^ nt[j] for j in range(l_pac - n_col, l_pac)]
    add("end_f", tail, False)
    add("end_r", tail, True)
    # across the junction of the two contigs
    for d in (10, 25, 40):
        s = len1 - d
        add(f"junction_{d}_f", [nt[j - 1] ^ nt[j] for j in range(s, s + n_col)], False)
        add(f"junction_{d}_r", [nt[j - 1] ^ nt[j] for j in range(s, s + n_col)], True)
    # an insertion / deletion within 20 bases of either end
    for k, at in enumerate((8, 12, 17, 33, 38, 42)):
        for what in ("ins_at", "del_at"):
            for rev in (False, True):
                s = 3000 + 977 * len(recs)
                add(f"{what[:3]}_{at}_{'r' if rev else 'f'}", read_colours(rnd, nt, s, n_col, **{what: at}), rev)
    # over and next to the N hole (its bases are random in the .pac, so these are ordinary reads there)
    for d in (-60, -30, -10, 20, hole[1] - 20, hole[1] + 5):
        s = hole[0] + d
        add(f"hole_{d}", [nt[j - 1] ^ nt[j] for j in range(s, s + n_col)], d % 20 == 0)
    # substitutions at the read's first and last base, colour errors at the ends, N colours
    for k in range(12):
        s = 40000 + 731 * k
        cs = [nt[j - 1] ^ nt[j] for j in range(s, s + n_col)]
        if k % 4 == 0:
            cs[0] = (cs[0] + 1) & 3
        elif k % 4 == 1:
            cs[-1] = (cs[-1] + 2) & 3
        elif k % 4 == 2:
            cs[1] = (cs[1] + 1) & 3
            cs[2] = (cs[2] + 1) & 3
        add(f"tip_{k}", cs, k % 2 == 1, n_N=1 if k % 4 == 3 else 0)
    open(G("cs_edge.fq"), "w").write("".join(recs))


# ------------------------------------------------------------------------------ reference commands
def run_twice(argv):
    a = subprocess.run([REF] + argv, check=True, capture_output=True).stdout
    b = subprocess.run([REF] + argv, check=True, capture_output=True).stdout
    return a if a == b else None


def sam_counts(text, first_contig):
    n = {"own_indel": 0, "XT_M": 0, "XA_indel": 0, "strand1_cigar": 0, "pos0": 0, "mapped": 0}
    for line in text.decode().splitlines():
        if line.startswith("@"):
            continue
        f = line.split("\t")
        flag, cigar = int(f[1]), f[5]
        if flag & 4:
            continue
        n["mapped"] += 1
        gapped = any(ch in cigar for ch in "IDS")
        if "I" in cigar or "D" in cigar:
            n["own_indel"] += 1
        if gapped and flag & 16:
            n["strand1_cigar"] += 1
        if f[2] == first_contig and f[3] == "1":
            n["pos0"] += 1
        for tag in f[11:]:
            if tag == "XT:A:M":
                n["XT_M"] += 1
            if tag.startswith("XA:Z:"):
                for ent in tag[5:].split(";"):
                    if ent and any(ch in ent.split(",")[2] for ch in "ID"):
                        n["XA_indel"] += 1
    return n


# --------------------------------------------------------------------------------------- vectors
def make_vectors(rnd):
    L = ctypes.CDLL(REFLIB, mode=os.RTLD_LAZY)  # its @PG printer lives in the harness executable, not needed here
    L.cs2nt_DP.restype = None
    L.cs2nt_DP.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4
    L.cs2nt_nt_qual.restype = ctypes.c_void_p
    L.cs2nt_nt_qual.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3
    counts = {1: 100, 2: 150, 3: 201, 35: 350, 50: 400, 100: 150, 151: 130, 1000: 20}
    assert sum(counts.values()) == 1501
    jobs = [s for s, c in counts.items() for _ in range(c)]
    rnd.shuffle(jobs)
    lines = []
    for v, size in enumerate(jobs):
        kind = v % 3
        truth = [rnd.randrange(4) for _ in range(size + 1)]
        if kind == 0:  # a read near its reference: substitutions, unknown bases, colour errors, N colours
            ref = [x if rnd.random() > 0.04 else rnd.randrange(4) for x in truth]
            ref = [x if rnd.random() > 0.05 else 4 for x in ref]
            cs = []
            for j in range(size):
                col = truth[j] ^ truth[j + 1]
                if rnd.random() < 0.06:
                    col = rnd.randrange(4)
                q = rnd.randint(0, 60)
                if rnd.random() < 0.03:
                    col, q = 0, 63
                cs.append(col << 6 | q)
        elif kind == 1:  # adversarial ties: every quality 6, 19 or 25, so many paths score equally
            ref = [rnd.randrange(5) for _ in range(size + 1)]
            cs = [rnd.randrange(4) << 6 | rnd.choice((6, 19, 25)) for _ in range(size)]
        else:  # unrelated rows
            ref = [rnd.choice((0, 1, 2, 3, 3, 2, 1, 0, 4)) for _ in range(size + 1)]
            cs = [rnd.randrange(4) << 6 | rnd.choice(list(range(61)) + [63]) for _ in range(size)]
        if v % 7 == 0:
            ref[0] = 4
        nt_ref = (ctypes.c_uint8 * (size + 1))(*ref)
        cs_read = (ctypes.c_uint8 * size)(*cs)
        nt_read = (ctypes.c_uint8 * (size + 1))()
        bt = (ctypes.c_uint8 * (4 * (size + 2)))()
        tarray = (ctypes.c_uint8 * (2 * size + 2))()
        L.cs2nt_DP(size, nt_ref, cs_read, nt_read, bt)
        p = L.cs2nt_nt_qual(size, nt_read, cs_read, tarray)
        assert p == ctypes.addressof(tarray) + size + 1
        out = bytes(tarray[size + 1:size + 1 + size - 1])
        lines.append("%s\t%s\t%s\n" % ("".join(map(str, ref)), bytes(cs).hex(), out.hex()))
    write_gz("cs2nt_vectors.tsv.gz", "".join(lines).encode())
    return {"n": len(jobs), "sizes": {str(k): v for k, v in counts.items()}}


# ------------------------------------------------------------------------------------------ main
def main():
    rnd = random.Random(SEED)
    manifest = {"dropped": [], "aln": {}, "samse": {}, "sampe": {}}
    c1, c2, hole, blocks = make_genome(rnd)
    exts = [".nt.pac", ".nt.ann", ".nt.amb", ".pac", ".ann", ".amb", ".rpac", ".bwt", ".rbwt", ".sa", ".rsa"]
    built = []
    for _ in range(2):
        subprocess.run([REF, "index", "-c", "-p", G("csg"), G("csg.fa")], check=True, capture_output=True)
        built.append([open(G("csg" + e), "rb").read() for e in exts])
    assert built[0] == built[1], "index -c is not reproducible"
    manifest["index"] = ["csg" + e for e in exts]
    for e in exts:
        assert os.path.getsize(G("csg" + e)) < LIMIT
    nt, l_pac = unpack_pac(G("csg.nt.pac"))
    assert l_pac == len(c1) + len(c2) and l_pac % 16 and l_pac % 4
    manifest["l_pac"] = l_pac
    make_pairs(rnd, nt, l_pac, hole, blocks)
    make_edge(rnd, nt, l_pac, len(c1), hole)

    for key, reads, argv in (("cs_r1", "cs_r1.fq", []), ("cs_r2", "cs_r2.fq", []), ("cs_edge", "cs_edge.fq", []),
                             ("cs_r1.q15", "cs_r1.fq", ["-q", "15"]), ("cs_r2.q15", "cs_r2.fq", ["-q", "15"])):
        out = run_twice(["aln", "-c"] + argv + [G("csg"), G(reads)])
        if out is None:
            manifest["dropped"].append("aln " + key)
            continue
        open(G(key + ".sai"), "wb").write(out)
        manifest["aln"][key] = {"prefix": "csg", "reads": reads, "argv": ["-c"] + argv, "sai": key + ".sai"}

    rg = "@RG\\tID:g\\tSM:s"
    counts = {}
    for key, sai, reads, argv in (("cs_r1.default", "cs_r1.sai", "cs_r1.fq", []),
                                  ("cs_r1.n5", "cs_r1.sai", "cs_r1.fq", ["-n", "5"]),
                                  ("cs_r1.rg", "cs_r1.sai", "cs_r1.fq", ["-r", rg]),
                                  ("cs_r1.q15", "cs_r1.q15.sai", "cs_r1.fq", []),
                                  ("cs_edge.default", "cs_edge.sai", "cs_edge.fq", []),
                                  ("cs_edge.n5", "cs_edge.sai", "cs_edge.fq", ["-n", "5"])):
        if sai[:-4] not in manifest["aln"]:
            continue
        out = run_twice(["samse"] + argv + [G("csg"), G(sai), G(reads)])
        if out is None:
            manifest["dropped"].append("samse " + key)
            continue
        write_gz(f"samse_{key}.sam.gz", out)
        counts["samse " + key] = sam_counts(out, "csA")
        manifest["samse"][key] = {"prefix": "csg", "sai": sai, "reads": reads, "argv": argv,
                                  "sam": f"samse_{key}.sam.gz", "counts": counts["samse " + key]}
    for key, argv in (("cs.R", ["-R"]), ("cs.R.n5N20", ["-R", "-n", "5", "-N", "20"]), ("cs.R.s", ["-R", "-s"])):
        out = run_twice(["sampe"] + argv + [G("csg"), G("cs_r1.sai"), G("cs_r2.sai"), G("cs_r1.fq"), G("cs_r2.fq")])
        if out is None:
            manifest["dropped"].append("sampe " + key)
            continue
        write_gz(f"sampe_{key}.sam.gz", out)
        counts["sampe " + key] = sam_counts(out, "csA")
        manifest["sampe"][key] = {"prefix": "csg", "sai": ["cs_r1.sai", "cs_r2.sai"], "reads": ["cs_r1.fq", "cs_r2.fq"],
                                  "argv": argv, "sam": f"sampe_{key}.sam.gz", "counts": counts["sampe " + key]}

    manifest["vectors"] = make_vectors(rnd)
    with open(G("cs_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    for k, v in counts.items():
        print(k, v)
    print("dropped:", manifest["dropped"])
    # the goldens exercise every branch
    assert counts["samse cs_r1.default"]["own_indel"] >= 50
    assert counts["sampe cs.R"]["XT_M"] >= 50
    assert counts["samse cs_r1.n5"]["XA_indel"] >= 10
    assert counts["samse cs_r1.default"]["strand1_cigar"] + counts["samse cs_edge.default"]["strand1_cigar"] >= 1
    assert counts["samse cs_edge.default"]["pos0"] >= 1


if __name__ == "__main__":
    main()
