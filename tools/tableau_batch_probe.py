"""blu_amd.tableau_row_batch (blu_hip_tableau_row_batch: the batched transposed solves of e_r[k], then A' y for all
members with one read of A per group of eight) timed on children that hold ONE matrix.  The protocol of
tools/tableau_probe.py: A = a bench basis (C2 10k by default) extended by `--extra` * m random columns of about 10 entries,
skip = isbasic, medians of `--reps`.  For each n of `--n` the root is forked by copy_batch + share_matrix into n children,
each with a row of its own, and four things are timed:
   (a) one tableau_row_batch call over the n children
   (b) the loop of single tableau_row calls over the same shared handles
   (c) solve_sparse_batch alone over them (what the product step adds to it is (a) - (c))
   (d) the device time of k_at_dot_batch (events around the kernel, a run of its own)
(a) and (b) must give the same bits for every member (compared outside the timed region).  The device memory held with the
shared matrix (hipMemGetInfo before and after the fork) is reported against the 20 bytes x entries x n private copies would
take.  The recorded run is profiles/tableau_batch_probe.txt.
   python tools/tableau_batch_probe.py C2"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import blu_amd
from blu_amd import keys as K
from blu_amd.matrices import CONFIGS

ap = argparse.ArgumentParser()
ap.add_argument("cfg", nargs="?", default="C2", choices=sorted(CONFIGS))
ap.add_argument("--m", type=int, default=0, help="rows, if not the configuration's")
ap.add_argument("--extra", type=float, default=2.0, help="non-basic columns, in multiples of m")
ap.add_argument("--n", type=int, nargs="+", default=[256, 1536])
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
c = CONFIGS[a.cfg]
m = a.m or c["m"]

cp, ri, v = blu_amd.gen_lp_basis(m, c["k"], c["bw"], c["tri_frac"], 5000, c["offscale"])
rng = np.random.default_rng(10_000)
nextra = int(a.extra * m)
lens = rng.integers(8, 13, nextra)
xi = np.concatenate([rng.choice(m, int(n), replace=False) for n in lens]).astype(np.uint64)
a_p = np.concatenate((cp.astype(np.int64), int(cp[-1]) + np.cumsum(lens))).astype(np.uint64)
a_i = np.concatenate((ri, xi))
a_x = np.concatenate((v, rng.standard_normal(len(xi))))
ncol = m + nextra
isbasic = np.concatenate((np.ones(m, np.int64), np.zeros(nextra, np.int64)))
print("leg %s: m=%d, ncol=%d, nnz=%d" % (a.cfg, m, ncol, len(a_i)), flush=True)


def free_bytes():
    hip = C.CDLL("libamdhip64.so")
    fr, tot = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
    return int(fr.value)


root = blu_amd.BLU(m, len(ri))
assert root.set_matrix(ncol, a_p, a_i, a_x) == K.OK
assert root.factorize_columns(np.arange(m)) == K.OK

for n in a.n:
    rows = [int(r) for r in rng.choice(m, n, replace=n > m)]
    skips = [isbasic] * n
    free0 = free_bytes()
    kids = [blu_amd.BLU(m, 1) for _ in range(n)]
    assert blu_amd.copy_batch(root, kids) == [K.OK] * n
    free1 = free_bytes()
    assert blu_amd.share_matrix(root, kids) == [K.OK] * n
    assert kids[0].dbg_matrix_holders() == n + 1

    def batch():
        t0 = time.perf_counter()
        sts, al = blu_amd.tableau_row_batch(kids, rows, False, skips)
        dt = time.perf_counter() - t0
        assert sts == [K.OK] * n
        return dt, al

    def loop():
        out = []
        t0 = time.perf_counter()
        for h, r in zip(kids, rows):
            st, alpha = h.tableau_row(r, False, isbasic)
            out.append(alpha)
        dt = time.perf_counter() - t0
        assert st == K.OK
        return dt, out

    def solves():
        t0 = time.perf_counter()
        sts = blu_amd.solve_sparse_batch(kids, [[r] for r in rows], [[1.0]] * n, "T")
        dt = time.perf_counter() - t0
        assert sts == [K.OK] * n
        return dt

    batch(), loop()  # (warm-up: the row-wise L of every child, the allocations, the block of the batched products)
    free2 = free_bytes()
    bat = [batch() if k == 0 else (batch()[0], None) for k in range(a.reps)]  # (the products of the first run are compared)
    lop = [loop() if k == 0 else (loop()[0], None) for k in range(a.reps)]
    sol = [solves() for _ in range(a.reps)]
    for x, y in zip(bat[0][1], lop[0][1]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), "tableau_row_batch and the loop of single calls differ in bits"
    kids[0].dbg_set_matrix_timing(True)
    kern = []
    for _ in range(a.reps):
        batch()
        kern.append(kids[0].dbg_matrix_kernel_seconds())
    kids[0].dbg_set_matrix_timing(False)
    counts = kids[0].dbg_matrix_counts()
    t_bat, t_loop, t_sol = (float(np.median([x[0] for x in bat])), float(np.median([x[0] for x in lop])), float(np.median(sol)))
    print(json.dumps(dict(leg=a.cfg, m=m, ncol=ncol, nnz=len(a_i), n=n, reps=a.reps, tableau_row_batch_ms=round(1e3 * t_bat, 2),
                          loop_of_single_calls_ms=round(1e3 * t_loop, 2), solve_sparse_batch_alone_ms=round(1e3 * t_sol, 2),
                          product_step_ms=round(1e3 * (t_bat - t_sol), 2), k_at_dot_batch_ms=round(1e3 * float(np.median(kern)), 3),
                          speedup_over_loop=round(t_loop / t_bat, 2), downloaded_MB=round(counts[3] / 1e6, 1), counts=counts,
                          device_MB_of_sharing_and_first_calls=round((free1 - free2) / 1e6, 1), device_MB_of_the_forks=round((free0 - free1) / 1e6, 1),
                          private_copies_would_take_MB=round(20 * len(a_i) * n / 1e6, 1), same_bits=True)), flush=True)
    for h in kids:
        h.close()
