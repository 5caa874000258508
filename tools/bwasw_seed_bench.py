#!/usr/bin/env python3
"""Throughput of bwasw's seeding on the device.

  load        synthetic reads of 200, 1 000 and 5 000 bp at 2 % and 5 % error (substitutions, a fifth
              of the errors indels) from a synthetic genome whose index is built on the device; half
              the tasks on the forward index, half reversed on the reverse index; bsw2_init_opt's
              options and the same with z = 10.
  device leg  Engine.bwasw_seeds per (length, error, option set): kernel time from HIP events
              (ibwa_run_stats_t.ms_bsw2_seed), wall time around the call; cells visited, the waves'
              time split in bwtl build / traversal / resolve, arena use and retries from
              ibwa_bsw2_seed_stats.
  yardstick   the host restatement (ibwa_amd/csrc/bsw2_core.h through tests/host/bsw2_seed_check.cpp,
              built here with g++ -O2) on a sample of the same tasks over the exported index files, on
              one thread and on 16.
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


def make_genome(bp):
    from tests.synth_util import genome_ascii
    buf, _ = genome_ascii(13, max(1, bp // 500), 3_000_000)
    g = np.frombuffer(buf.tobytes().replace(b"N", b""), np.uint8)[:bp]
    lut = np.zeros(256, np.uint8)
    for k, ch in enumerate(b"ACGT"):
        lut[ch] = k
    return lut[g]


def make_reads(text, n, ln, err, rng):
    seqs, strands = [], []
    for i in range(n):
        a = int(rng.integers(0, text.size - ln - 64))
        q = text[a:a + ln + 32].copy()
        sub = rng.random(q.size) < err * 0.8
        q[sub] = (q[sub] + rng.integers(1, 4, int(sub.sum()))) & 3
        for _ in range(rng.poisson(q.size * err * 0.2)):
            at = int(rng.integers(1, q.size - 1))
            q = np.delete(q, at) if rng.random() < 0.5 else np.insert(q, at, rng.integers(0, 4))
        q = q[:ln].astype(np.uint8)
        strands.append(i & 1)
        seqs.append(q[::-1].copy() if i & 1 else q)
    return seqs, np.array(strands, np.uint8)


def write_index(eng, tmp, intv):
    prefix = os.path.join(tmp, "bench")
    for s, (be, se) in enumerate(((".bwt", ".sa"), (".rbwt", ".rsa"))):
        primary, L2, words = eng.export_bwt(s)
        with open(prefix + be, "wb") as f:
            f.write(np.array([primary, *L2], np.uint32).tobytes())
            f.write(words.tobytes())
        sa = eng.export_sa(s, intv)
        with open(prefix + se, "wb") as f:
            f.write(np.array([primary, *L2, intv, L2[3]], np.uint32).tobytes())
            f.write(sa[1:].tobytes())
    return prefix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-bp", type=int, default=4_000_000)
    ap.add_argument("--tasks", type=int, default=4096, help="tasks per configuration at 200 bp (fewer for longer reads)")
    ap.add_argument("--host-tasks", type=int, default=64, help="tasks of each configuration the host yardstick runs")
    ap.add_argument("--lengths", default="200,1000,5000")
    ap.add_argument("--sa-intv", type=int, default=32)
    a = ap.parse_args()
    from ibwa_amd import engine as E
    text = make_genome(a.genome_bp)
    eng = E.Engine(0)
    eng.build_index(text, a.sa_intv)
    res = {"metric": "bwasw seeding tasks/s (bsw2_core per task)", "genome_bp": int(text.size), "configs": []}
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bsw2_seed_check")
        subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "ibwa_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "host", "bsw2_seed_check.cpp")], check=True)
        prefix = write_index(eng, tmp, a.sa_intv)
        for ln in [int(x) for x in a.lengths.split(",")]:
            n = max(64, a.tasks * 200 // ln)
            for err in (0.02, 0.05):
                seqs, strands = make_reads(text, n, ln, err, rng)
                for name, kw in (("defaults", {}), ("z10", {"z": 10})):
                    opt = E.bsw2_opt("bwasw", **kw)
                    eng.bwasw_seeds(seqs[:64], strands[:64], opt)  # warm-up: the buffers grow once
                    t0 = time.perf_counter()
                    out = eng.bwasw_seeds(seqs, strands, opt)
                    wall = time.perf_counter() - t0
                    st, ss = eng.stats(), eng.seed_stats()
                    ticks = max(1, ss["ticks_build"] + ss["ticks_walk"] + ss["ticks_resolve"])
                    cfg = {"len": ln, "err": err, "opt": name, "tasks": n, "kernel_ms": st.ms_bsw2_seed, "wall_s": wall,
                           "tasks_per_s_kernel": n / (st.ms_bsw2_seed / 1e3), "tasks_per_s_wall": n / wall,
                           "cells": ss["cells"], "cells_per_s_kernel": ss["cells"] / (st.ms_bsw2_seed / 1e3),
                           "share_bwtl": ss["ticks_build"] / ticks, "share_traversal": ss["ticks_walk"] / ticks,
                           "share_resolve": ss["ticks_resolve"] / ticks, "arena_bytes": ss["arena"],
                           "arena_peak_bytes": ss["arena_peak"], "retried": ss["retried"], "workgroups": ss["workgroups"],
                           "tasks_with_hits": sum(1 for h in out if h[0] or h[1])}
                    # the yardstick on a sample of the same tasks
                    m = min(a.host_tasks, n)
                    t, bw = zip(*[E.bsw2_opt_for_len(opt, ln)] * m)
                    tf = os.path.join(tmp, "tasks.txt")
                    with open(tf, "w") as f:
                        for i in range(m):
                            f.write(f"{opt.a} {opt.b} {opt.q} {opt.r} {t[i]} {bw[i]} {opt.z} {opt.is_} {int(strands[i])} "
                                    f"{''.join(map(str, seqs[i].tolist()))}\n")
                    for th in (1, 16):
                        h = json.loads(subprocess.run([exe, "run", prefix, tf, str(th)], check=True, stdout=subprocess.PIPE,
                                                      text=True).stdout)
                        cfg[f"host_tasks_per_s_{th}_threads"] = m / h["seconds"]
                        if th == 1:
                            cfg["host_cells_sample"] = h["cells"]
                    cfg["kernel_vs_host_16_threads"] = cfg["tasks_per_s_kernel"] / cfg["host_tasks_per_s_16_threads"]
                    res["configs"].append(cfg)
                    print(json.dumps(cfg), file=sys.stderr, flush=True)
    eng.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
