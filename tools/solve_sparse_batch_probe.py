"""blu_hip_solve_sparse_batch timing against the loop of blu_hip_solve_sparse calls: handles of the 10k bench size
(gen_lp_basis(10_000, 10, 9, 0.5, seed, 0.3), 64 distinct seeded matrices assigned round-robin, factorized by
factorize_batch), one unit-vector right-hand side per handle, both systems.  Per system and per n: one cold call (the
workspaces and, for 'T', the row-wise L are built on the way), then three warm repetitions, host clock around the
synchronizing calls of the Python layer; the median is reported.  Statuses are checked and eight members are verified
against the CPU oracle outside the timed region.
   python tools/solve_sparse_batch_probe.py batch 256 1536     one solve_sparse_batch call per repetition
   python tools/solve_sparse_batch_probe.py loop 256 1536      n single solve_sparse calls per repetition (this mode uses
                                                               nothing newer than BLU.solve_sparse, so BLU_HIP_LIB may
                                                               point at the library of an older commit)
The n of a run are prefixes of one set of max(n) handles."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import blu_amd
from blu_amd import keys as K

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("batch", "loop"))
ap.add_argument("n", type=int, nargs="+")
ap.add_argument("--m", type=int, default=10_000)
ap.add_argument("--seeds", type=int, default=64)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--verify", type=int, default=8)
a = ap.parse_args()
m, nmax = a.m, max(a.n)
seeds = min(a.seeds, nmax)
mats = [blu_amd.gen_lp_basis(m, 10, 9, 0.5, 5000 + s, 0.3) for s in range(seeds)]
hs = [blu_amd.BLU(m, len(mats[k % seeds][1])) for k in range(nmax)]
t0 = time.perf_counter()
st = blu_amd.factorize_batch(hs, [mats[k % seeds] for k in range(nmax)])
print("%d handles of m = %d: factorize_batch %.3f s" % (nmax, m, time.perf_counter() - t0), flush=True)
assert st == [K.OK] * nmax, [s for s in st if s != K.OK][:4]
irs = [[(7919 * k + 13) % m] for k in range(nmax)]
xrs = [[1.0]] * nmax


def once(n, trans):
    t0 = time.perf_counter()
    if a.mode == "batch":
        s = blu_amd.solve_sparse_batch(hs[:n], irs[:n], xrs[:n], trans)
    else:
        s = [h.solve_sparse(i, x, trans) for h, i, x in zip(hs[:n], irs[:n], xrs[:n])]
    dt = time.perf_counter() - t0
    assert s == [K.OK] * n, [x for x in s if x != K.OK][:4]
    return dt


twins = {}


def verify(n, trans):
    if a.verify <= 0:
        return
    from oracle import orc
    orc.build()
    for k in range(0, n, max(1, n // a.verify)):
        if k % seeds not in twins:
            cp, ri, v = mats[k % seeds]
            o = orc.OracleBLU(m, 64 * len(ri) + 1024)
            o.set_fix_d3(True)
            assert o.factorize(cp[:-1], cp[1:], ri, v) == K.OK
            twins[k % seeds] = o
        o = twins[k % seeds]
        so, il, lhs = o.solve_sparse(irs[k], xrs[k], trans)
        h = hs[k]
        assert so == K.OK and h.nzlhs == len(il) and np.array_equal(h.ilhs[:h.nzlhs], il) and np.array_equal(h.lhs, lhs), (k, trans)


for n in sorted(a.n):
    out = dict(mode=a.mode, n=n, m=m)
    for trans in "NT":
        cold = once(n, trans)
        warm = [once(n, trans) for _ in range(a.reps)]
        verify(n, trans)
        out[trans] = dict(cold_s=round(cold, 4), warm_s=[round(x, 4) for x in warm], median_s=round(float(np.median(warm)), 4),
                          per_member_us=round(1e6 * float(np.median(warm)) / n, 1), nzlhs_mean=round(float(np.mean([h.nzlhs for h in hs[:n]])), 1),
                          branch=sorted(set(int(h.stat(43)) for h in hs[:n])))
    print(json.dumps(out), flush=True)
