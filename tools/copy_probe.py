"""blu_hip_copy_batch timing: one handle of a bench size is factorized and its state copied into n handles, three ways:
  * one blu_hip_copy_batch call: the first one, which allocates what the destinations lack, and warm repeats;
  * n calls with one destination each (warm destinations);
  * blu_hip_factorize_batch of the n handles on the same matrix -- the only route to n equal handles without the copy.
Host clock around the synchronizing calls of the Python layer; medians of three (the first call is one measurement), with
the bytes and launches of blu_hip_dbg_copy_counts.
   python tools/copy_probe.py C2 256      (C2 | C3 | C4 ..., number of destinations; --updates U: the source takes U update
                                          rounds first, so that the update workspace is part of the state)"""
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
from blu_amd.workloads import column_modifications

ap = argparse.ArgumentParser()
ap.add_argument("cfg", choices=sorted(CONFIGS))
ap.add_argument("n", type=int)
ap.add_argument("--updates", type=int, default=0)
a = ap.parse_args()
c = CONFIGS[a.cfg]
m, n = c["m"], a.n
mat = blu_amd.gen_lp_basis(m, c["k"], c["bw"], c["tri_frac"], 5000, c["offscale"])
src = blu_amd.BLU(m, len(mat[1]))
assert src.factorize(mat[0][:-1], mat[0][1:], mat[1], mat[2]) == K.OK
applied = 0
if a.updates:
    stream = column_modifications(mat[0], mat[1], 1 << 30, c["offscale"], seed=99)
    for _ in range(a.updates):
        j, rows, vals = next(stream)
        assert src.solve_for_update([j], None, "T") == K.OK and src.solve_for_update(rows, vals, "N") == K.OK
        applied += src.update(src.lhs[j]) == K.OK
dsts = [blu_amd.BLU(m, len(mat[1])) for _ in range(n)]


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def copy_all():
    assert blu_amd.copy_batch(src, dsts) == [K.OK] * n


def copy_one_by_one():
    for d in dsts:
        assert blu_amd.copy_batch(src, [d]) == [K.OK]


def factorize_all():
    assert blu_amd.factorize_batch(dsts, [mat] * n) == [K.OK] * n


first = timed(copy_all)
first_counts = src.dbg_copy_counts()
warm = [timed(copy_all) for _ in range(3)]
counts = src.dbg_copy_counts()
rhs = np.cos(np.arange(float(m)))
x = src.solve_dense(rhs)
assert all(np.array_equal(dsts[k].solve_dense(rhs), x) for k in (0, n // 2, n - 1))
singles = [timed(copy_one_by_one) for _ in range(3)]
single_counts = src.dbg_copy_counts()
fact = [timed(factorize_all) for _ in range(3)]
mw, ms, mf = float(np.median(warm)), float(np.median(singles)), float(np.median(fact))
print(json.dumps(dict(
    leg="%s x %d" % (a.cfg, n), m=m, updates_applied=int(applied),
    copy_batch_first_s=round(first, 4), first_allocations=first_counts[3],
    copy_batch_warm_s=round(mw, 5), copy_batch_warm_runs_s=[round(t, 5) for t in warm], warm_allocations=counts[3],
    launches_syncs_uploads=list(counts[:3]), bytes_read_per_destination=counts[4], bytes_written=counts[5],
    warm_write_GBps=round(counts[5] / mw / 1e9, 1),
    n_single_copies_s=round(ms, 4), n_single_copies_runs_s=[round(t, 4) for t in singles], single_copy_counts=list(single_counts[:3]),
    factorize_batch_s=round(mf, 3), factorize_batch_runs_s=[round(t, 3) for t in fact],
    warm_copy_vs_single_copies=round(ms / mw, 1), warm_copy_vs_factorize_batch=round(mf / mw, 1))), flush=True)
