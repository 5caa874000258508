#!/usr/bin/env python3
"""Throughput of `ibwa-amd stdsw` and of the run-time-parameter kernel beside k_sw.

  stdsw leg   --shorts N shorts of 100 bases (2 % substitutions, half of them from the reverse strand)
              against one --long-bp long sequence from the synthetic genome, both strands, through the
              CLI: wall time, pairs/s and forward-pass cell updates/s (len_short x len_long per pair).
  sw leg      k_stdaln with the `bwa` preset on tools/sw_bench.py's mate-rescue shape (510 x 150,
              --sw-pairs pairs) beside k_sw on the same pairs: kernel times from HIP events.
  --reference builds the reference's `stdsw` as tools/make_stdsw_golden.py does (temporary directory;
              build container only) and times it on --ref-shorts of the same shorts, one thread.
              Needs no GPU; the other legs are skipped.
One JSON line on stdout.  Reported figures, not pass conditions.
"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COMP = str.maketrans("ACGT", "TGCA")


def workload(long_bp, n_shorts, tmp):
    from tests.synth_util import genome_ascii
    buf, _ = genome_ascii(11, max(1, long_bp // 500), 3_000_000)  # about twice long_bp
    g = buf.tobytes().decode().replace("N", "")
    assert len(g) >= long_bp, (len(g), long_bp)
    lng = g[:long_bp]
    rng = random.Random(3)
    lf, sf = os.path.join(tmp, "long.fa"), os.path.join(tmp, "short.fa")
    with open(lf, "w") as f:
        f.write(">long\n" + lng + "\n")
    with open(sf, "w") as f:
        for k in range(n_shorts):
            a = rng.randrange(0, long_bp - 100)
            s = "".join(rng.choice("ACGT") if rng.random() < 0.02 else ch for ch in lng[a:a + 100])
            f.write(f">r{k}\n{s.translate(COMP)[::-1] if k & 1 else s}\n")
    return lf, sf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shorts", type=int, default=100_000)
    ap.add_argument("--long-bp", type=int, default=1_000_000)
    ap.add_argument("--sw-pairs", type=int, default=200_000)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-shorts", type=int, default=1000)
    a = ap.parse_args()
    res = {"metric": "stdsw pairs/s (100 bp shorts, both strands, one long sequence)", "long_bp": a.long_bp}
    with tempfile.TemporaryDirectory() as tmp:
        if a.reference:
            from tools.make_stdsw_golden import build_ref_cli
            lf, sf = workload(a.long_bp, a.ref_shorts, tmp)
            exe = build_ref_cli(tmp)
            t = time.perf_counter()
            subprocess.run([exe, lf, sf], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            dt = time.perf_counter() - t
            pairs = 2 * a.ref_shorts
            res["reference_cpu"] = {"pairs": pairs, "seconds": dt, "pairs_per_s": pairs / dt,
                                    "forward_GCUPS": pairs * 100.0 * a.long_bp / dt / 1e9, "threads": 1}
            print(json.dumps(res), flush=True)
            return
        from ibwa_amd import _native
        from ibwa_amd import engine as E
        if a.shorts:
            lf, sf = workload(a.long_bp, a.shorts, tmp)
            t = time.perf_counter()
            r = subprocess.run([_native.BIN_PATH, "stdsw", lf, sf], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
            dt = time.perf_counter() - t
            pairs = 2 * a.shorts
            res.update({"value": pairs / dt, "unit": "pairs/s", "pairs": pairs, "wall_s": dt, "exit": r.returncode,
                        "records": r.stdout.count(b">long\t"), "forward_GCUPS": pairs * 100.0 * a.long_bp / dt / 1e9})
        if a.sw_pairs:
            import bench
            refs, reads = bench.make_sw_pairs(bench.make_genome(50_000, 1_000_000, 37, 16)[1], a.sw_pairs)[:2]
            eng = E.Engine(0)
            eng.sw(refs[:1000], reads[:1000])
            eng.stdaln(refs[:1000], reads[:1000], "bwa")
            x = eng.sw(refs, reads)
            ms_sw = eng.stats().ms_sw
            y = eng.stdaln(refs, reads, "bwa")
            chunks, ms_std = eng.stdaln_chunks()
            same = all((p[0], p[2], p[3], p[4], p[5]) == q or (q[2] is None and (p[0], p[2]) == q[:2]) for p, q in zip(y, x))
            res["sw_shape"] = {"pairs": a.sw_pairs, "k_sw_ms": ms_sw, "k_stdaln_ms": ms_std, "launches": chunks, "same_results": same}
            eng.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
