"""blu_hip_solve_dense_multi timing: ONE handle of one size, fresh from a single factorize and again after 50 updates
(blu_amd.workloads.column_modifications), right-hand sides and solutions in device memory.  For each state, trans and
nrhs in {1, 8, 64, 512, 2048} it prints the cold multi-solve, the median of three warm ones (host clock around the
synchronizing call) and the loop of blu_hip_solve_dense calls on the same handle: the loop runs over the min(nrhs, 64)
distinct right-hand sides and is scaled to nrhs.  Right-hand side j is distinct right-hand side j mod 64, so EVERY
column of the multi-solve is compared with the loop's solution of its right-hand side, bit for bit.
   python tools/solve_multi_probe.py C2      (C2 10k | C4 50k | C3 100k; --nrhs 1,8,64 to choose the counts)"""
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
from blu_amd.workloads import column_modifications

ap = argparse.ArgumentParser()
ap.add_argument("cfg", choices=sorted(CONFIGS))
ap.add_argument("--nrhs", default="1,8,64,512,2048")
ap.add_argument("--updates", type=int, default=50)
a = ap.parse_args()
c = CONFIGS[a.cfg]
m = c["m"]
counts = [int(x) for x in a.nrhs.split(",")]
DISTINCT = 64
hip = blu_amd.lib()  # device buffers through the HIP runtime the library is linked with
hip.hipMalloc.argtypes = [C.c_void_p, C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]


def to_dev(x):
    x = np.ascontiguousarray(x)
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), max(x.nbytes, 8)) == 0
    assert hip.hipMemcpy(p.value, x.ctypes.data, x.nbytes, 1) == 0  # hipMemcpyHostToDevice
    return p.value


cp, ri, v = blu_amd.gen_lp_basis(m, c["k"], c["bw"], c["tri_frac"], 5000, c["offscale"])
h = blu_amd.BLU(m, len(ri))
t0 = time.perf_counter()
assert h.factorize(cp[:-1], cp[1:], ri, v) == K.OK
print("leg %s: m=%d, factorize %.3f s" % (a.cfg, m, time.perf_counter() - t0), flush=True)
nmax = max(counts)
rhs = np.random.default_rng(10_000).standard_normal((DISTINCT, m))
drhs = to_dev(rhs[np.arange(nmax) % DISTINCT])
dlhs = to_dev(np.zeros((nmax, m)))


def multi(nrhs, tr):
    t0 = time.perf_counter()
    h.solve_dense_multi(trans=tr, device_ptrs=(drhs, m, dlhs, m, nrhs))
    return time.perf_counter() - t0


def leg(state):
    for tr in "NT":
        loop_x, loop_t = [], []
        for j in range(DISTINCT):
            t0 = time.perf_counter()
            loop_x.append(h.solve_dense(rhs[j], tr))
            loop_t.append(time.perf_counter() - t0)
        loop_x = np.array(loop_x)
        single = float(np.median(loop_t))
        for nrhs in counts:
            cold = multi(nrhs, tr)
            warm = float(np.median([multi(nrhs, tr) for _ in range(3)]))
            got = np.empty((nrhs, m))
            assert hip.hipMemcpy(got.ctypes.data, dlhs, got.nbytes, 2) == 0  # hipMemcpyDeviceToHost
            same = int((got == loop_x[np.arange(nrhs) % DISTINCT]).all(axis=1).sum())
            t_loop = float(np.sum(loop_t[:min(nrhs, DISTINCT)])) * nrhs / min(nrhs, DISTINCT)
            r = dict(leg=a.cfg, m=m, state=state, trans=tr, nrhs=nrhs, first_multi_s=round(cold, 5), warm_multi_s=round(warm, 5),
                     loop_s=round(t_loop, 4), loop_timing="%d calls timed%s" % (min(nrhs, DISTINCT), ", scaled" if nrhs > DISTINCT else ""),
                     single_call_median_s=round(single, 5), per_rhs_warm_us=round(1e6 * warm / nrhs, 1),
                     speedup_over_loop=round(t_loop / warm, 2), chunk=h.dbg_multi_last_chunk(), bit_identical="%d/%d" % (same, nrhs))
            print(json.dumps(r), flush=True)
            assert same == nrhs, "columns differ from the loop"


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
