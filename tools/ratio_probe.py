"""blu_amd.ratio_test_batch (blu_hip_ratio_test_batch: the batched transposed solves of e_r[k], A' y per group of eight,
then the pick of the entering column on the device) against the path it replaces, on the setting of
tools/tableau_batch_probe.py: A = a bench basis (C2 10k by default) extended by `--extra` * m random columns of about 10
entries, kind 0 on the basic columns and +1 / -1 / 2 on the others, medians of `--reps`.  For each n of `--n` the root is
forked by copy_batch + share_matrix + copy_duals_batch into n children, each with a row of its own, and timed are
   (a) tableau_row_batch plus the pick in numpy on the host, row by row (tests/util_ratio.ratio_pick)
   (b) ratio_test_batch
   (c) update_duals_batch with the thetas of (b) and two overrides per member
   (d) solve_sparse_batch alone (what is behind the solves is (a) - (d) and (b) - (d))
on the same library in the same run; (a) and (b) must name the same q with the same record for every member.  Also one
single ratio_test at this ncol with the device time of its one-workgroup pick (events around k_ratio_pick).  The recorded
run is profiles/ratio_probe.txt.
   python tools/ratio_probe.py C2"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import blu_amd
from blu_amd import keys as K
from blu_amd.matrices import CONFIGS
from tests.util_ratio import ratio_pick, same_record

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
kind = np.concatenate((np.zeros(m, np.int8), rng.choice(np.array([1, -1, 2], np.int8), nextra)))
d = np.abs(rng.standard_normal(ncol)) * (kind != 0)
PIVTOL, DUALTOL = 1e-7, 1e-9
print("leg %s: m=%d, ncol=%d, nnz=%d" % (a.cfg, m, ncol, len(a_i)), flush=True)

root = blu_amd.BLU(m, len(ri))
assert root.set_matrix(ncol, a_p, a_i, a_x) == K.OK
assert root.factorize_columns(np.arange(m)) == K.OK
assert root.set_duals(d, kind) == K.OK

# the single entry at this ncol: one workgroup over the row
root.dbg_set_matrix_timing(True)
single, pick = [], []
for _ in range(a.reps + 1):
    t0 = time.perf_counter()
    st, rec = root.ratio_test(m // 2, 1.0, PIVTOL, DUALTOL)
    single.append(time.perf_counter() - t0)
    pick.append(root.dbg_matrix_kernel_seconds())
    assert st == K.OK
root.dbg_set_matrix_timing(False)
print(json.dumps(dict(leg=a.cfg, ncol=ncol, single_ratio_test_ms=round(1e3 * float(np.median(single[1:])), 3),
                      k_ratio_pick_one_workgroup_ms=round(1e3 * float(np.median(pick[1:])), 4), counts=root.dbg_matrix_counts())), flush=True)

for n in a.n:
    rows = [int(r) for r in rng.choice(m, n, replace=n > m)]
    sigmas = [1.0 if k % 2 else -1.0 for k in range(n)]
    skips = [isbasic] * n
    kids = [blu_amd.BLU(m, 1) for _ in range(n)]
    assert blu_amd.copy_batch(root, kids) == [K.OK] * n
    assert blu_amd.share_matrix(root, kids) == [K.OK] * n
    assert blu_amd.copy_duals_batch(root, kids) == [K.OK] * n

    def host():
        t0 = time.perf_counter()
        sts, al = blu_amd.tableau_row_batch(kids, rows, False, skips)
        t1 = time.perf_counter()
        recs = [ratio_pick(x, d, kind, s, PIVTOL, DUALTOL) for x, s in zip(al, sigmas)]
        t2 = time.perf_counter()
        assert sts == [K.OK] * n
        return t2 - t0, t1 - t0, recs

    def device():
        t0 = time.perf_counter()
        sts, recs = blu_amd.ratio_test_batch(kids, rows, sigmas, PIVTOL, DUALTOL)
        dt = time.perf_counter() - t0
        assert sts == [K.OK] * n
        return dt, recs

    def solves():
        t0 = time.perf_counter()
        sts = blu_amd.solve_sparse_batch(kids, [[r] for r in rows], [[1.0]] * n, "T")
        dt = time.perf_counter() - t0
        assert sts == [K.OK] * n
        return dt

    host(), device()  # (warm-up: the row-wise L of every child, the allocations, the blocks of the batched products)
    hst = [host() for _ in range(a.reps)]
    dev = [device() for _ in range(a.reps)]
    counts = kids[0].dbg_matrix_counts()
    sol = [solves() for _ in range(a.reps)]
    for k, (x, y) in enumerate(zip(hst[0][2], dev[0][1])):
        assert same_record(x, y), ("the host pick and ratio_test_batch differ", k, x, y)
    thetas = [r[4] for r in dev[0][1]]
    sets = [([r[0], k % m], [0.0, 0.0], [0, 0]) if r[0] >= 0 else None for k, r in enumerate(dev[0][1])]
    step = []
    for _ in range(a.reps):
        device()
        t0 = time.perf_counter()
        sts = blu_amd.update_duals_batch(kids, thetas, sets)
        step.append(time.perf_counter() - t0)
        assert sts == [K.OK] * n
        assert blu_amd.copy_duals_batch(root, kids) == [K.OK] * n
    t_host, t_rows, t_dev, t_sol = (float(np.median([x[0] for x in hst])), float(np.median([x[1] for x in hst])),
                                    float(np.median([x[0] for x in dev])), float(np.median(sol)))
    print(json.dumps(dict(leg=a.cfg, m=m, ncol=ncol, n=n, reps=a.reps, a_tableau_row_batch_plus_host_pick_ms=round(1e3 * t_host, 2),
                          a_of_that_tableau_row_batch_ms=round(1e3 * t_rows, 2), b_ratio_test_batch_ms=round(1e3 * t_dev, 2),
                          c_update_duals_batch_ms=round(1e3 * float(np.median(step)), 2), d_solve_sparse_batch_alone_ms=round(1e3 * t_sol, 2),
                          a_behind_the_solves_ms=round(1e3 * (t_rows - t_sol), 2), b_behind_the_solves_ms=round(1e3 * (t_dev - t_sol), 2),
                          b_counts=counts, members_with_a_column=sum(r[0] >= 0 for r in dev[0][1]), same_q_and_record=True)), flush=True)
    for h in kids:
        h.close()
