"""blu_hip_solve_sparse_multi timing against the loop of blu_hip_solve_sparse calls on the SAME handle: one basis of a
bench size (C2 10k | C3 100k), fresh from a single factorize and again after a few dozen updates
(blu_amd.workloads.column_modifications); unit-vector and 10-entry right-hand sides; both systems.  For each state,
kind, system and nrhs: one cold multi call (the pool and, for 'T' on the fresh handle, the row-wise L are built on the
way), then the median of three warm BLU.solve_sparse_multi calls (blu_hip_solve_sparse_multi + blu_hip_get_sparse_multi;
host clock around the synchronizing calls of the Python layer) and the median of three warm loops of nrhs
BLU.solve_sparse calls (the clock around each call, summed).  Every right-hand side of the multi call is compared with
the loop's result, bit for bit, outside the timed region.
   python tools/solve_sparse_multi_probe.py C2 --nrhs 64,256,1536
   python tools/solve_sparse_multi_probe.py C3 --nrhs 64,256"""
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
ap.add_argument("--nrhs", default="64,256,1536")
ap.add_argument("--updates", type=int, default=40)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
c = CONFIGS[a.cfg]
m = c["m"]
counts = sorted(int(x) for x in a.nrhs.split(","))
nmax = max(counts)

cp, ri, v = blu_amd.gen_lp_basis(m, c["k"], c["bw"], c["tri_frac"], 5000, c["offscale"])
h = blu_amd.BLU(m, len(ri))
t0 = time.perf_counter()
assert h.factorize(cp[:-1], cp[1:], ri, v) == K.OK
print("leg %s: m=%d, factorize %.3f s" % (a.cfg, m, time.perf_counter() - t0), flush=True)
rng = np.random.default_rng(10_000)
RHS = {
    "unit": [(np.array([(7919 * k + 13) % m]), np.array([1.0])) for k in range(nmax)],
    "10-entry": [(rng.choice(m, 10, replace=False), rng.standard_normal(10)) for k in range(nmax)],
}


def multi(cols, tr):
    t0 = time.perf_counter()
    sts, sols = h.solve_sparse_multi([x[0] for x in cols], [x[1] for x in cols], tr)
    dt = time.perf_counter() - t0
    assert sts == [K.OK] * len(cols)
    return dt, sols


def loop(cols, tr):
    dt, sols = 0.0, []
    for ir, xr in cols:
        t0 = time.perf_counter()
        st = h.solve_sparse(ir, xr, tr)
        dt += time.perf_counter() - t0
        assert st == K.OK
        il = h.ilhs[:h.nzlhs].copy()
        sols.append((il, h.lhs[il]))
    return dt, sols


def leg(state):
    for kind, rhs in RHS.items():
        for tr in "NT":
            for nrhs in counts:
                cols = rhs[:nrhs]
                cold = multi(cols, tr)[0]
                warm = [multi(cols, tr) for _ in range(a.reps)]
                loops = [loop(cols, tr) for _ in range(a.reps)]
                t_multi, t_loop = float(np.median([w[0] for w in warm])), float(np.median([w[0] for w in loops]))
                same = sum(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(warm[-1][1], loops[-1][1]))
                r = dict(leg=a.cfg, m=m, state=state, rhs=kind, trans=tr, nrhs=nrhs, first_multi_s=round(cold, 5), warm_multi_s=round(t_multi, 5),
                         loop_s=round(t_loop, 4), per_rhs_multi_us=round(1e6 * t_multi / nrhs, 1), per_rhs_loop_us=round(1e6 * t_loop / nrhs, 1),
                         speedup_over_loop=round(t_loop / t_multi, 2), nzlhs_mean=round(float(np.mean([len(x[0]) for x in warm[-1][1]])), 1),
                         chunk=h.dbg_sparse_multi_last_chunk(), bit_identical="%d/%d" % (same, nrhs))
                print(json.dumps(r), flush=True)
                assert same == nrhs, "right-hand sides differ from the loop"


leg("fresh")
stream = column_modifications(cp, ri, 1 << 30, c["offscale"], seed=99)
done = 0
t0 = time.perf_counter()
while done < a.updates:
    j, rows, vals = next(stream)
    assert h.solve_for_update([j], None, "T") == K.OK
    assert h.solve_for_update(rows, vals, "N") == K.OK
    st = h.update(h.lhs[j])
    assert st in (K.OK, K.ERROR_SINGULAR_UPDATE), st
    done += st == K.OK
print("%d updates applied in %.3f s (nforrest %d)" % (done, time.perf_counter() - t0, int(h.stat(K.STAT_NFORREST))), flush=True)
leg("after %d updates" % done)
