"""BLU.maxvolume (blu_hip_maxvolume: the candidates priced in chunks) timed against the loop blu_amd.maxvolume over the
single C entries on the SAME library: A = a bench basis (C2 10k by default) extended by `--extra` * m random columns of
about 10 entries; the start basis is the bench basis.  Two passes are timed, each as the median of `--reps` runs of either
kind from the same start (host clock around the whole pass, uploads of A included):
   first sweep      from the bench basis: pays one extra solve per hit plus the waves thrown away behind it
   hit-free sweep   from the basis the native sweeps converge to (or reach after --max-sweeps): (ncol - m) / chunk
                    synchronizes instead of ncol - m
Both kinds must take the same decisions (status, nupdate, basis, isbasic and the statistics NUPDATE, NFACTORIZE, NFORREST,
L / U / R_FLOPS, UPDATE_COST are compared outside the timed region); dbg_maxvolume_counts of the native passes is printed.
The recorded run is profiles/maxvolume_probe.txt.
   python tools/maxvolume_probe.py C2 --tol 3.0"""
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
ap.add_argument("--tol", type=float, default=3.0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--loop-reps", type=int, default=0, help="runs of the loop, if not --reps (a loop pass over 20000 columns takes minutes)")
ap.add_argument("--max-sweeps", type=int, default=30)
ap.add_argument("--chunk", type=int, default=0, help="fixed chunk (0: the policy)")
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
STATS = (K.STAT_NUPDATE, K.STAT_NFACTORIZE, K.STAT_NFORREST, K.STAT_L_FLOPS, K.STAT_U_FLOPS, K.STAT_R_FLOPS, K.STAT_UPDATE_COST)
print("leg %s: m=%d, ncol=%d, nnz=%d, volumetol=%g" % (a.cfg, m, ncol, len(a_i), a.tol), flush=True)


def one_pass(native, basis0, isbasic0):
    h = blu_amd.BLU(m, len(ri))
    h.dbg_set_maxvolume_chunk(a.chunk)
    basis, isbasic = basis0.copy(), isbasic0.copy()
    t0 = time.perf_counter()
    if native:
        st, nup = h.maxvolume(ncol, a_p, a_i, a_x, basis, isbasic, a.tol)
    else:
        st, nup = blu_amd.maxvolume(h, ncol, a_p, a_i, a_x, basis, isbasic, a.tol)
    dt = time.perf_counter() - t0
    assert st == K.OK, st
    return dt, (st, nup, basis.tolist(), isbasic.tolist(), [h.stat(k) for k in STATS]), h.dbg_maxvolume_counts()


def timed(name, native, basis0, isbasic0):
    r = one_pass(native, basis0, isbasic0)
    print("  %s, %s: %.3f s, %d updates" % (name, "native" if native else "loop", r[0], r[1][1]), flush=True)
    return r


def leg(name, basis0, isbasic0):
    nat = [timed(name, True, basis0, isbasic0) for _ in range(a.reps)]
    lop = [timed(name, False, basis0, isbasic0) for _ in range(a.loop_reps or a.reps)]
    assert all(x[1] == nat[0][1] for x in nat + lop), "the native pass and the loop took different decisions"
    t_nat, t_loop = float(np.median([x[0] for x in nat])), float(np.median([x[0] for x in lop]))
    counts = nat[0][2]
    r = dict(leg=a.cfg, m=m, ncol=ncol, sweep=name, volumetol=a.tol, nupdate=nat[0][1][1], refactorizations=int(nat[0][1][4][1]) - 1,
             native_s=round(t_nat, 4), loop_s=round(t_loop, 4), speedup_over_loop=round(t_loop / t_nat, 2), chunks=counts[0], priced=counts[1],
             discarded=counts[2], hits=counts[3], native_runs=len(nat), loop_runs=len(lop), same_decisions=True)
    print(json.dumps(r), flush=True)
    return r


basis0 = np.arange(m, dtype=np.int64)
isbasic0 = np.concatenate((np.ones(m, np.int64), np.zeros(nextra, np.int64)))
leg("first", basis0, isbasic0)
# the basis of the hit-free sweep: native sweeps on one handle until one changes nothing
h = blu_amd.BLU(m, len(ri))
basis, isbasic = basis0.copy(), isbasic0.copy()
t0 = time.perf_counter()
for sweep in range(a.max_sweeps):
    st, nup = h.maxvolume(ncol, a_p, a_i, a_x, basis, isbasic, a.tol)
    assert st == K.OK, st
    print("sweep %d: %d updates, counts %s, %.2f s so far" % (sweep, nup, h.dbg_maxvolume_counts(), time.perf_counter() - t0), flush=True)
    if nup == 0:
        break
if nup != 0:
    print("no hit-free sweep within %d sweeps: the next leg is not hit-free" % a.max_sweeps)
r = leg("hit-free" if nup == 0 else "late", basis, isbasic)
if nup == 0:
    assert r["hits"] == 0 and r["priced"] == ncol - m
    assert r["native_s"] < r["loop_s"], "the hit-free sweep is not faster than the loop: a defect to be found"
