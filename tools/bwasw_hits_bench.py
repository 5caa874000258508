#!/usr/bin/env python3
"""Throughput of bwasw from reads to hits on the device, Engine.bwasw_hits.

  load        synthetic reads of 150, 400 and 1 000 bp at 2 % and 10 % error (substitutions, a fifth of
              the errors indels) from the synthetic genome tools/bwasw_seed_bench.py uses, its index
              built on the device; half the reads on the forward index, half reversed on the reverse
              index; bsw2_init_opt's options.
  device leg  Engine.bwasw_hits per (length, error): wall time around the call, and the share of each
              stage in it -- the seeding kernel (ibwa_run_stats_t.ms_bsw2_seed), the left and the right
              launch of k_bsw2_extend (ibwa_bsw2_aln1_stats), and the rest: copies and the host stages.
  DP runs     from the stats of the left launch: the runs the ordered kernel made (extended + discarded)
              against the runs a caller of ibwa_extend_seeds makes who extends every candidate
              (extended + contained + discarded).  A count, not a time.
  yardstick   the host restatement (ibwa_amd/csrc/bsw2_aln1.h through tests/host/bsw2_aln1_check.cpp,
              built here with g++ -O2) on a sample of the same reads over the exported index files, on
              one thread.
One JSON line on stdout.  Reported figures, not pass conditions.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bwasw_seed_bench import make_genome, make_reads, write_index  # noqa: E402


def pack_pac(text):
    """Codes 0-3 -> the bytes of a .pac file's sequence part, four bases a byte, the first in the top bits."""
    t = np.concatenate([text, np.zeros(-text.size % 4, np.uint8)]).reshape(-1, 4)
    return (t[:, 0] << 6 | t[:, 1] << 4 | t[:, 2] << 2 | t[:, 3]).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-bp", type=int, default=4_000_000)
    ap.add_argument("--reads", type=int, default=4096, help="reads per configuration at 150 bp (fewer for longer reads)")
    ap.add_argument("--host-reads", type=int, default=64, help="reads of each configuration the host yardstick runs")
    ap.add_argument("--lengths", default="150,400,1000")
    ap.add_argument("--sa-intv", type=int, default=32)
    a = ap.parse_args()
    from ibwa_amd import engine as E
    text = make_genome(a.genome_bp)
    eng = E.Engine(0)
    eng.build_index(text, a.sa_intv)
    pac = pack_pac(text)
    eng.load_pac([pac], [int(text.size)])
    res = {"metric": "bwasw reads/s from read to hits (bsw2_aln1_core per read)", "genome_bp": int(text.size), "configs": []}
    rng = np.random.default_rng(7)
    opt = E.bsw2_aln_opt("bwasw")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bsw2_aln1_check")
        subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "ibwa_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "host", "bsw2_aln1_check.cpp")], check=True)
        prefix = write_index(eng, tmp, a.sa_intv)
        with open(prefix + ".pac", "wb") as f:
            f.write(pac.tobytes() + b"\0")
        for ln in [int(x) for x in a.lengths.split(",")]:
            n = max(64, a.reads * 150 // ln)
            for err in (0.02, 0.10):
                seqs, is_rev = make_reads(text, n, ln, err, rng)
                eng.bwasw_hits(seqs[:64], is_rev[:64], opt)  # warm-up: the buffers grow once
                t0 = time.perf_counter()
                out = eng.bwasw_hits(seqs, is_rev, opt)
                wall = time.perf_counter() - t0
                st, hs = eng.stats(), eng.bwasw_hits_stats()
                seed_s, left_s, right_s = st.ms_bsw2_seed / 1e3, hs["us_left"] / 1e6, hs["us_right"] / 1e6
                made = hs["extended"] + hs["discarded"]
                every = made + hs["contained"]
                cfg = {"len": ln, "err": err, "reads": n, "wall_s": wall, "reads_per_s": n / wall,
                       "share_seed_kernel": seed_s / wall, "share_left_kernel": left_s / wall, "share_right_kernel": right_s / wall,
                       "share_host_and_copies": 1 - (seed_s + left_s + right_s) / wall,
                       "left_ms": left_s * 1e3, "right_ms": right_s * 1e3, "seed_ms": seed_s * 1e3,
                       "left_hits": every + hs["skipped"], "left_windows": hs["windows"], "dp_runs_ordered": made,
                       "dp_runs_discarded": hs["discarded"], "dp_runs_every_candidate": every,
                       "reads_with_hits": sum(1 for h in out if h), "hits": sum(len(h) for h in out)}
                # the yardstick on a sample of the same reads
                m = min(a.host_reads, n)
                tf = os.path.join(tmp, "reads.txt")
                with open(tf, "w") as f:
                    o = opt.seed
                    for i in range(m):
                        f.write(f"{o.a} {o.b} {o.q} {o.r} {o.t} {o.bw} {o.z} {o.is_} {o.coef} 1 {opt.t_seeds} {opt.mask_level} "
                                f"{int(is_rev[i])} 1 {''.join(map(str, seqs[i].tolist()))}\n")
                h = json.loads(subprocess.run([exe, "stages", prefix, tf, "time"], check=True, stdout=subprocess.PIPE, text=True).stdout)
                cfg["host_reads_per_s_1_thread"] = m / h["seconds"]
                cfg["device_vs_host_1_thread"] = cfg["reads_per_s"] / cfg["host_reads_per_s_1_thread"]
                res["configs"].append(cfg)
                print(json.dumps(cfg), file=sys.stderr, flush=True)
    eng.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
