"""blu_hip_solve_dense_batch timing: one leg = n handles of one size, 64 distinct seeded matrices assigned round-robin
(as bench.py does), factorized by factorize_batch from device inputs, each handle with its own seeded right-hand side
in device memory.  For each trans it prints the cold batch solve (with the row-wise L build of a forward solve), the
median of three warm ones (host clock around the synchronizing call), the same handles solved by a loop of
blu_hip_solve_dense, and whether every member is bit-identical to the loop's solution of its handle.
   python tools/solve_batch_probe.py C2 4096      (C2 | C3 | C4, number of handles; --sample S: time S members of the
                                                   loop and scale, default: all when n < 4096, else 512)"""
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
ap.add_argument("cfg", choices=sorted(CONFIGS))
ap.add_argument("n", type=int)
ap.add_argument("--seeds", type=int, default=64)
ap.add_argument("--sample", type=int, default=None)
a = ap.parse_args()
c = CONFIGS[a.cfg]
m, n = c["m"], a.n
hip = blu_amd.lib()  # device buffers through the HIP runtime the library is linked with
hip.hipMalloc.argtypes = [C.c_void_p, C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]


def to_dev(a):
    a = np.ascontiguousarray(a)
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), max(a.nbytes, 8)) == 0
    assert hip.hipMemcpy(p.value, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice
    return p.value


mats = [blu_amd.gen_lp_basis(m, c["k"], c["bw"], c["tri_frac"], 5000 + s, c["offscale"]) for s in range(a.seeds)]
dmats = [tuple(to_dev(x) for x in (cp[:-1], cp[1:], ri, v)) + (len(ri),) for cp, ri, v in mats]
hs = [blu_amd.BLU(m, len(mats[k % a.seeds][1]) // 2) for k in range(n)]
t0 = time.perf_counter()
st = blu_amd.factorize_batch(hs, device_ptrs=[dmats[k % a.seeds] for k in range(n)])
t_fact = time.perf_counter() - t0
assert st == [K.OK] * n, [s for s in st if s != K.OK][:4]
rhs = [np.random.default_rng(10_000 + k).standard_normal(m) for k in range(n)]
drhs = to_dev(np.stack(rhs))
dlhs = to_dev(np.zeros((n, m)))
ptrs = [(drhs + 8 * m * k, dlhs + 8 * m * k) for k in range(n)]
sample = a.sample if a.sample else (n if n < 4096 else 512)
timed = set(range(0, n, max(1, n // sample)))
print("leg %s x %d: m=%d, factorize_batch %.3f s" % (a.cfg, n, m, t_fact))


def batch_solve(tr):
    t0 = time.perf_counter()
    st = blu_amd.solve_dense_batch(hs, trans=tr, device_ptrs=ptrs)
    dt = time.perf_counter() - t0
    assert st == [K.OK] * n, [s for s in st if s != K.OK][:4]
    return dt


for tr in "NT":
    cold = batch_solve(tr)
    warm = float(np.median([batch_solve(tr) for _ in range(3)]))
    got = np.empty((n, m))
    assert hip.hipMemcpy(got.ctypes.data, dlhs, got.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    t_loop, same = 0.0, 0
    for k, h in enumerate(hs):
        t0 = time.perf_counter()
        x = h.solve_dense(rhs[k], tr)
        if k in timed:
            t_loop += time.perf_counter() - t0
        same += bool(np.array_equal(x, got[k]))
    scaled = len(timed) < n
    t_loop *= n / len(timed)
    r = dict(leg="%s x %d" % (a.cfg, n), trans=tr, cold_batch_s=round(cold, 4), warm_batch_s=round(warm, 4),
             loop_s=round(t_loop, 3), loop_timing=("%d of %d members timed, scaled" % (len(timed), n)) if scaled else "all members timed",
             per_member_warm_us=round(1e6 * warm / n, 2), per_member_loop_us=round(1e6 * t_loop / n, 1),
             batch_solves_per_s=round(n / warm, 1), loop_solves_per_s=round(n / t_loop, 1), speedup_warm=round(t_loop / warm, 1),
             bit_identical="%d/%d" % (same, n))
    print(json.dumps(r), flush=True)
    assert same == n, "members differ from the loop"
