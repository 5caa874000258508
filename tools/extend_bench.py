#!/usr/bin/env python3
"""Throughput of the seed extension on a bwasw-shaped load.

  load        --seeds seeds on a synthetic genome, half extended rightwards and half leftwards: a = 1,
              b = 3, q = 5, r = 2, band 50, G0 = 1, queries of 200-1 000 bases with 5 % divergence from
              the genome (4 % substitutions, 1 % indels), targets of lq + lq / 2 bases, end-cell mode.
  batch leg   ibwa_extend_batch: the windows cut on the host and sent with the call.
  seeds leg   ibwa_extend_seeds: the windows read on the device from the resident sequence.
  yardstick   the reference's aln_extend_core (oracle/_ref/libibwa_ref.so, through ctypes) on one thread
              over the first --ref-pairs of the same pairs, and that figure times 16.
Kernel times come from ibwa_stdaln_chunks (HIP events around the launches), wall times around the C
calls.  One JSON line on stdout.  Reported figures, not pass conditions.
"""
import argparse
import ctypes as c
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REFLIB = os.path.join(ROOT, "oracle", "_ref", "libibwa_ref.so")


class RefParam(c.Structure):
    _fields_ = [("gap_open", c.c_int), ("gap_ext", c.c_int), ("gap_end", c.c_int), ("matrix", c.POINTER(c.c_int)),
                ("row", c.c_int), ("band_width", c.c_int)]


class RefPath(c.Structure):
    _fields_ = [("i", c.c_int), ("j", c.c_int), ("ctype", c.c_ubyte)]


def make_load(n_seeds, genome_bp):
    from tests.synth_util import genome_ascii
    buf, _ = genome_ascii(13, max(1, genome_bp // 500), 3_000_000)
    g = np.frombuffer(buf.tobytes().replace(b"N", b""), np.uint8)[:genome_bp]
    lut = np.zeros(256, np.uint8)
    for k, ch in enumerate(b"ACGT"):
        lut[ch] = k
    text = lut[g]
    T = text.size
    rng = np.random.default_rng(5)
    lq = rng.integers(200, 1001, n_seeds)
    lt = lq + lq // 2
    dirs = (np.arange(n_seeds) & 1).astype(np.uint8)
    pos = rng.integers(2000, T - 2000, n_seeds).astype(np.uint64)
    queries = []
    for p in range(n_seeds):
        a = int(pos[p])
        q = (text[a - int(lq[p]):a][::-1] if dirs[p] else text[a:a + int(lq[p])]).copy()
        sub = rng.random(q.size) < 0.04
        q[sub] = rng.integers(0, 4, int(sub.sum()))
        for _ in range(rng.poisson(q.size * 0.01)):
            at = int(rng.integers(1, q.size - 1))
            q = np.delete(q, at) if rng.random() < 0.5 else np.insert(q, at, rng.integers(0, 4))
        queries.append(q)
    pad = (-T) % 4
    t4 = np.concatenate([text, np.zeros(pad, np.uint8)]).reshape(-1, 4)
    pac = (t4[:, 0] << 6 | t4[:, 1] << 4 | t4[:, 2] << 2 | t4[:, 3]).astype(np.uint8)
    return text, pac, pos, dirs, lt.astype(np.uint32), queries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=100_000)
    ap.add_argument("--genome-bp", type=int, default=4_000_000)
    ap.add_argument("--ref-pairs", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from ibwa_amd import engine as E
    text, pac, pos, dirs, lt, queries = make_load(a.seeds, a.genome_bp)
    n, T = a.seeds, text.size
    wins = [text[int(p) - int(l):int(p)][::-1] if d else text[int(p):int(p) + int(l)] for p, d, l in zip(pos, dirs, lt)]
    mat = np.full((5, 5), -3, np.int32)
    mat[np.arange(4), np.arange(4)] = 1
    param = (5, 2, 2, mat, 5, 50)
    apar, _keep = E._aln_param_struct(param)
    _, s1, o1, l1, s2, o2, l2 = E._pair_arrays(wins, queries)
    res = {"metric": "seed extensions/s (bwasw shape: 1 / -3 / 5 / 2, band 50, queries 200-1000, end cell)", "seeds": n,
           "target_bases": int(l1.sum()), "query_bases": int(l2.sum())}

    # ---- the yardstick
    m = min(a.ref_pairs, n)
    L = c.CDLL(REFLIB, mode=os.RTLD_LAZY)
    L.aln_extend_core.restype = c.c_int
    L.aln_extend_core.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_int, c.POINTER(RefParam), c.POINTER(RefPath), c.c_void_p,
                                  c.c_int, c.c_void_p]
    rmat = (c.c_int * 25)(*[int(x) for x in mat.reshape(-1)])
    rp = RefParam(5, 2, 2, rmat, 5, 50)
    path = RefPath()
    ref = []
    t = time.perf_counter()
    for p in range(m):
        sc = L.aln_extend_core(s1.ctypes.data + int(o1[p]), int(l1[p]), s2.ctypes.data + int(o2[p]), int(l2[p]), c.byref(rp),
                               c.byref(path), None, 1, None)
        ref.append((sc, path.i, path.j) if sc > 0 else (sc, 0, 0))
    dt = time.perf_counter() - t
    res["reference_cpu"] = {"pairs": m, "seconds": dt, "pairs_per_s_1_thread": m / dt, "pairs_per_s_x16": 16 * m / dt}

    # ---- the two device legs
    eng = E.Engine(0)
    eng.load_pac([pac], [T])
    score, ends = np.zeros(n, np.int32), np.zeros((n, 2), np.int32)
    g0 = np.ones(n, np.int32)
    qs, qo, ql = s2, o2, l2

    def batch():
        E._chk(E.lib().ibwa_extend_batch(eng.h, c.byref(apar), 1, n, s1.ctypes.data, o1.ctypes.data, l1.ctypes.data, s2.ctypes.data,
                                         o2.ctypes.data, l2.ctypes.data, g0.ctypes.data, score.ctypes.data, ends.ctypes.data,
                                         None, None, None, None))

    def seeds():
        E._chk(E.lib().ibwa_extend_seeds(eng.h, c.byref(apar), n, pos.ctypes.data, dirs.ctypes.data, lt.ctypes.data, 0,
                                         qs.ctypes.data, qo.ctypes.data, ql.ctypes.data, g0.ctypes.data, score.ctypes.data,
                                         ends.ctypes.data))

    for name, fn in (("batch", batch), ("seeds", seeds)):
        fn()  # warm-up: the buffers grow once
        walls, kms = [], []
        for _ in range(a.reps):
            score[:] = 0
            t = time.perf_counter()
            fn()
            walls.append(time.perf_counter() - t)
            kms.append(eng.stdaln_chunks()[1])
        got = [(int(score[p]), int(ends[p, 0]), int(ends[p, 1])) for p in range(m)]
        w, k = float(np.median(walls)), float(np.median(kms))
        res[name] = {"wall_s": w, "kernel_ms": k, "launches": eng.stdaln_chunks()[0], "pairs_per_s_wall": n / w,
                     "pairs_per_s_kernel": n / (k / 1e3), "same_as_reference": got == ref,
                     "kernel_vs_ref_1_thread": (n / (k / 1e3)) / (m / dt), "kernel_vs_ref_x16": (n / (k / 1e3)) / (16 * m / dt),
                     "wall_vs_ref_x16": (n / w) / (16 * m / dt)}
    res["extended"] = int((score > 1).sum())
    res["mean_end_j"] = float(ends[:, 1].mean())
    eng.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
