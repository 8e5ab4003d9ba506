"""blu_hip_solve_for_update_batch / blu_hip_update_batch timing: one leg = n handles of one size, 64 distinct seeded
matrices assigned round-robin (as bench.py does), factorized by factorize_batch.  One ROUND is what a simplex iteration
does on every basis: a transposed solve_for_update, a forward one and the update, all with solutions; every handle has a
column stream of its own (blu_amd.workloads.column_modifications).  The first round goes through the batch entries cold
(row-wise L and update workspace of every member built on the way); then three warm rounds through the batch entries
alternate with three through the loop of single-handle calls over the same handles, in the same process, and the
medians are compared: the batch counts as faster only if it beats the loop by more than the loop's own spread (max -
min of its three rounds).  Host clock around the synchronizing calls of the Python layer, on both sides.
   python tools/update_batch_probe.py C2 4096      (C2 | C3 | C4, number of handles; --sample S: the loop rounds run on S
                                                   of the handles and are scaled, default: min(n, 256))"""
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
ap.add_argument("--seeds", type=int, default=64)
ap.add_argument("--sample", type=int, default=None)
a = ap.parse_args()
c = CONFIGS[a.cfg]
m, n = c["m"], a.n
seeds = min(a.seeds, n)
mats = [blu_amd.gen_lp_basis(m, c["k"], c["bw"], c["tri_frac"], 5000 + s, c["offscale"]) for s in range(seeds)]
hs = [blu_amd.BLU(m, len(mats[k % seeds][1])) for k in range(n)]
t0 = time.perf_counter()
st = blu_amd.factorize_batch(hs, [mats[k % seeds] for k in range(n)])
t_fact = time.perf_counter() - t0
assert st == [K.OK] * n, [s for s in st if s != K.OK][:4]
streams = [column_modifications(mats[k % seeds][0], mats[k % seeds][1], 1 << 30, c["offscale"], seed=99 + k) for k in range(n)]
sample = a.sample if a.sample else min(n, 256)
looped = list(range(0, n, max(1, n // sample)))[:sample]
print("leg %s x %d: m=%d, factorize_batch %.3f s" % (a.cfg, n, m, t_fact), flush=True)
applied = 0


def batch_round(members):
    """-> seconds of the three calls (T, N, update)"""
    global applied
    H = [hs[k] for k in members]
    picks = [next(streams[k]) for k in members]
    t0 = time.perf_counter()
    s = blu_amd.solve_for_update_batch(H, [[p[0]] for p in picks], None, "T")
    t1 = time.perf_counter()
    assert s == [K.OK] * len(H), [x for x in s if x != K.OK][:4]
    s = blu_amd.solve_for_update_batch(H, [p[1] for p in picks], [p[2] for p in picks], "N")
    t2 = time.perf_counter()
    assert s == [K.OK] * len(H), [x for x in s if x != K.OK][:4]
    xtbl = [h.lhs[p[0]] for h, p in zip(H, picks)]
    t3 = time.perf_counter()
    s = blu_amd.update_batch(H, xtbl)
    t4 = time.perf_counter()
    assert set(s) <= {K.OK, K.ERROR_SINGULAR_UPDATE}, [x for x in s if x != K.OK][:4]
    applied += s.count(K.OK)
    return t1 - t0, t2 - t1, t4 - t3


def loop_round(members):
    global applied
    tt = tn = tu = 0.0
    for k in members:
        h = hs[k]
        j, rows, vals = next(streams[k])
        t0 = time.perf_counter()
        s = h.solve_for_update([j], None, "T")
        t1 = time.perf_counter()
        assert s == K.OK, s
        s = h.solve_for_update(rows, vals, "N")
        t2 = time.perf_counter()
        assert s == K.OK, s
        x = h.lhs[j]
        t3 = time.perf_counter()
        s = h.update(x)
        t4 = time.perf_counter()
        assert s in (K.OK, K.ERROR_SINGULAR_UPDATE), s
        applied += s == K.OK
        tt, tn, tu = tt + t1 - t0, tn + t2 - t1, tu + t4 - t3
    f = n / len(members)
    return tt * f, tn * f, tu * f


everyone = list(range(n))
cold = batch_round(everyone)
warm_b, warm_l = [], []
for _ in range(3):
    warm_b.append(batch_round(everyone))
    warm_l.append(loop_round(looped))
tb, tl = [sum(x) for x in warm_b], [sum(x) for x in warm_l]
mb, ml, spread = float(np.median(tb)), float(np.median(tl)), max(tl) - min(tl)
r = dict(leg="%s x %d" % (a.cfg, n), first_round_batch_s=round(sum(cold), 4), first_round_T_N_update_s=[round(x, 4) for x in cold],
         warm_batch_round_s=round(mb, 4), warm_batch_T_N_update_s=[round(float(np.median([x[q] for x in warm_b])), 4) for q in range(3)],
         warm_batch_rounds_s=[round(x, 4) for x in tb], loop_round_s=round(ml, 3),
         loop_T_N_update_s=[round(float(np.median([x[q] for x in warm_l])), 3) for q in range(3)], loop_rounds_s=[round(x, 3) for x in tl],
         loop_spread_s=round(spread, 3), loop_timing="all members" if len(looped) == n else "%d of %d members, scaled" % (len(looped), n),
         per_member_batch_us=round(1e6 * mb / n, 1), per_member_loop_us=round(1e6 * ml / n, 1), speedup=round(ml / mb, 1),
         batch_faster_by_more_than_the_loops_spread=bool(mb < ml - spread), updates_applied=int(applied))
print(json.dumps(r), flush=True)
