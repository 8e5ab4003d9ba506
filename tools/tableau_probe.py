"""BLU.tableau_row (blu_hip_tableau_row: the transposed solve of e_r, then A' y on the device) timed against the route a
caller had before it on the SAME library: solve_sparse([r], [1.0], 'T'), the solution downloaded, and the walk over A on the
host in numpy.  A = a bench basis (C2 10k by default) extended by `--extra` * m random columns of about 10 entries, resident
through set_matrix; the factorized basis is the bench basis and skip = isbasic.  Each route makes `--rows` rows, three times;
the medians of the three are printed with the device time of k_at_dot (events around the kernel, a run of its own) and its
share of the call.  Both routes must give the same bits for every row (compared outside the timed region).  The host walk
is vectorized over the columns, position by position, which keeps the summation order of the contract.  The recorded run is
profiles/tableau_probe.txt.
   python tools/tableau_probe.py C2"""
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

ap = argparse.ArgumentParser()
ap.add_argument("cfg", nargs="?", default="C2", choices=sorted(CONFIGS))
ap.add_argument("--m", type=int, default=0, help="rows, if not the configuration's")
ap.add_argument("--extra", type=float, default=2.0, help="non-basic columns, in multiples of m")
ap.add_argument("--rows", type=int, default=100)
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
rows = [int(r) for r in rng.choice(m, a.rows, replace=False)]
print("leg %s: m=%d, ncol=%d, nnz=%d, rows=%d" % (a.cfg, m, ncol, len(a_i), len(rows)), flush=True)

# the host walk: the non-skipped columns, all of at most 64 entries here, summed position by position (s = +0.0, s = s + t_q)
beg = a_p[:-1].astype(np.int64)
clen = np.diff(a_p.astype(np.int64))
assert clen.max() <= 64
live = np.flatnonzero(isbasic == 0)
a_ii = a_i.astype(np.int64)
steps = [(live[clen[live] > k], beg[live[clen[live] > k]] + k) for k in range(int(clen[live].max()))]


def host_at_dot(y):
    out = np.zeros(ncol)
    for cols, pos in steps:
        out[cols] = out[cols] + a_x[pos] * y[a_ii[pos]]
    return out


def handle():
    h = blu_amd.BLU(m, len(ri))
    assert h.set_matrix(ncol, a_p, a_i, a_x) == K.OK
    assert h.factorize_columns(np.arange(m)) == K.OK
    return h


def native(h):
    out = []
    t0 = time.perf_counter()
    for r in rows:
        st, alpha = h.tableau_row(r, False, isbasic)
        out.append(alpha)
    dt = time.perf_counter() - t0
    assert st == K.OK
    return dt, out


def host_route(h):
    out = []
    t0 = time.perf_counter()
    for r in rows:
        st = h.solve_sparse([r], [1.0], "T")
        out.append(host_at_dot(h.lhs))
    dt = time.perf_counter() - t0
    assert st == K.OK
    return dt, out


def solves_only(h):
    t0 = time.perf_counter()
    for r in rows:
        h.solve_sparse([r], [1.0], "T")
    return time.perf_counter() - t0


h = handle()
native(h), host_route(h)  # (warm-up: the row-wise L, the allocations)
nat = [native(h) for _ in range(a.reps)]
hst = [host_route(h) for _ in range(a.reps)]
sol = [solves_only(h) for _ in range(a.reps)]
for x, y in zip(nat[0][1], hst[0][1]):
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), "tableau_row and the host route differ in bits"
h.dbg_set_matrix_timing(True)
kern = []
for r in rows:
    assert h.tableau_row(r, False, isbasic)[0] == K.OK
    kern.append(h.dbg_matrix_kernel_seconds())
t_nat, t_host, t_sol = (float(np.median([x[0] for x in nat])), float(np.median([x[0] for x in hst])), float(np.median(sol)))
k_us = 1e6 * float(np.median(kern))
call_us = 1e6 * t_nat / len(rows)
print(json.dumps(dict(leg=a.cfg, m=m, ncol=ncol, nnz=len(a_i), rows=len(rows), reps=a.reps, tableau_row_us_per_row=round(call_us, 1),
                      host_route_us_per_row=round(1e6 * t_host / len(rows), 1), solve_sparse_alone_us_per_row=round(1e6 * t_sol / len(rows), 1),
                      speedup_over_host_route=round(t_host / t_nat, 2), k_at_dot_us=round(k_us, 1),
                      k_at_dot_share_of_call=round(k_us / call_us, 3), same_bits=True)), flush=True)
