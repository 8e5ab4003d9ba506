"""blu_hip_copy_batch / blu_hip_clone on the CPU: the emulation build of the library (blu_amd/csrc `make emu`, as in
tests/test_emu_cpu.py) runs k_copy_fanout and the host side of the two entries.

A copy must be observably its source: every parameter and every statistic key 0..124 (bit patterns), and every later call
with the status, the pattern order and the bits the source gives.  The oracle has no clone, so the twin of a copy is a fresh
OracleBLU driven through the recorded history of the source (tests/util_copy.py).  Equalities only, over all members.
Each case runs in a child process: the library path is fixed when blu_amd is first imported."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")
REPLAY = os.path.join(ROOT, "blu_amd", "emu_replay")
REPLAY_ASAN = os.path.join(ROOT, "blu_amd", "emu_replay_asan")
OP_CLONE, OP_COPY_INTO = 17, 18  # tools/emu_replay.cpp

HEAD = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, sys.argv[1])
import blu_amd
from blu_amd import keys as K
from oracle import orc
from tests import util_update as U, util_copy as CP
L = blu_amd.lib()
assert b"gfx950" in L.blu_hip_version()
L.blu_hip_copy_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
INVARG, MISS, INVCALL = K.ERROR_INVALID_ARGUMENT, K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_CALL


def handle(mat, want=K.OK, b_nz=None):
    cp, ri, v = mat
    g = blu_amd.BLU(len(cp) - 1, len(ri) if b_nz is None else b_nz)
    st = g.factorize(cp[:-1], cp[1:], ri, v)
    assert st == want, (st, want)
    return g


def scaled(mat, cols):
    cp, ri, v = mat
    v = v.copy()
    for j in cols:
        v[int(cp[j]):int(cp[j + 1])] *= 1e-17
    return cp, ri, v


def busy_handle(m, seed):
    # holds an UPDATED factorization of another matrix, factorized once (the nfactorize of every source here), with its
    # row-wise L built by a transposed solve_sparse before the updates
    mat = orc.gen_lp_basis(m, 5, 5, 0.5, 40 + seed, 0.5)
    d = handle(mat)
    assert d.solve_sparse([0], [1.0], "T") == K.OK
    cols = U.columns_of(*mat)
    pr = CP.pair_rows(d.get_factors(), m)
    log = U.run_updates(d, cols, m, 6, np.random.default_rng(seed), pair_row=pr)
    assert log["done"] >= 1 and d.stat(K.STAT_NUPDATE) == log["done"] and d.stat(K.STAT_NFACTORIZE) == 1
    return d


def raw_copy(src, dsts, n=None, status=True):
    n = len(dsts) if n is None else n
    N = max(len(dsts), 1)
    hs = (C.c_void_p * N)(*[None if d is None else d._h for d in dsts])
    st = (C.c_int * N)(*([77] * N))
    rc = L.blu_hip_copy_batch(None if src is None else src._h, hs, n, st if status else None)
    return rc, [int(s) for s in st][:len(dsts)]
"""

CHILD_FRESH = r"""
which = sys.argv[2]
if which == "lp200":
    mat, want = orc.gen_lp_basis(200, 8, 8, 0.5, 1, 0.3), K.OK
elif which == "lp150":
    mat, want = orc.gen_lp_basis(150, 5, 4, 0.8, 3, 0.6), K.OK
elif which == "rankdef":
    mat, want = scaled(orc.gen_lp_basis(90, 4, 5, 0.3, 7, 0.5), (2, 45, 89)), K.WARNING_SINGULAR_MATRIX
else:  # an odd size: every segment ends with a tile of fewer than 16 bytes
    mat, want = orc.gen_lp_basis(203, 6, 6, 0.5, 5, 0.4), K.OK
m = len(mat[0]) - 1
g = handle(mat, want)
o = CP.twin_of(orc, *mat, want)
dsts = [blu_amd.BLU(m, len(mat[1])), blu_amd.BLU(m, 1), busy_handle(m, 3)]
assert dsts[2].stat(K.STAT_NFACTORIZE) == g.stat(K.STAT_NFACTORIZE)
before = CP.state_of(g)
assert blu_amd.copy_batch(g, dsts) == [K.OK] * 3
counts = g.dbg_copy_counts()
print(which, counts)
assert counts[:3] == (1, 1, 1) and counts[3] > 0 and counts[5] == 3 * counts[4]
after = CP.state_of(g)
assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "the source changed"
for k, d in enumerate(dsts):
    CP.same_state(g, d, (which, "destination", k))
    assert d.stat(K.STAT_NUPDATE) == 0 and d.stat(K.STAT_RANK) == o.stat(K.STAT_RANK)
twins = [o] + [CP.twin_of(orc, *mat, want) for d in dsts]
CP.check_members([g] + dsts, twins, 11, which)
for k, d in enumerate(dsts):  # the same calls since the copy: still the source's answers, flop counters and branch included
    CP.same_state(g, d, (which, "destination after the solves", k))
CP.check_members([g], [o], 12, which + ", the source again")
print("COPY FRESH OK")
"""

CHILD_UPDATED = r"""
mat = orc.gen_lp_basis(200, 8, 8, 0.5, 1, 0.3)
m, SEED, NUPD = 200, 22, 25
g = handle(mat)
o, cols, pr, log = CP.history(orc, mat, SEED, NUPD, handle=g)
assert log["done"] >= 10 and g.stat(K.STAT_NFORREST) > 0 and g.stat(K.STAT_NSYMPERM_TOTAL) > 0, (log, g.stat(K.STAT_NFORREST), g.stat(K.STAT_NSYMPERM_TOTAL))
print(log["done"], g.stat(K.STAT_NFORREST), g.stat(K.STAT_NSYMPERM_TOTAL), g.stat(K.STAT_DEV_NUNSYMPERM_TOTAL))
dsts = [blu_amd.BLU(m, len(mat[1])), blu_amd.BLU(m, 1), busy_handle(m, 4), blu_amd.BLU(m, len(mat[1]))]
assert blu_amd.copy_batch(g, dsts) == [K.OK] * 4
members = [g] + dsts
twins, colss = [o], [cols]
for d in dsts:
    CP.same_state(g, d, "updated")
    od, cd, _, logd = CP.history(orc, mat, SEED, NUPD)
    assert logd["done"] == log["done"]
    twins.append(od)
    colss.append(cd)
# every member goes its own way: 5 further rounds, different for each, in lock step with its own twin
for k, (h, t, c) in enumerate(zip(members, twins, colss)):
    lg = U.run_updates(h, c, m, 5, np.random.default_rng(100 + k), pair_row=pr, twin=t)
    assert lg["done"] >= 1, (k, lg)
assert len({h.stat(K.STAT_NFORREST_TOTAL) + 1000 * h.stat(K.STAT_R_NZ) for h in members}) > 1, "the members did not diverge"
CP.check_members(members, twins, 13, "updated, all")
g.close()
CP.check_members(dsts, twins[1:], 14, "updated, the source closed")
for k, (h, t, c) in enumerate(zip(dsts, twins[1:], colss[1:])):
    assert U.run_updates(h, c, m, 2, np.random.default_rng(200 + k), pair_row=pr, twin=t)["done"] >= 1
print("COPY UPDATED OK")
"""

CHILD_PENDING = r"""
mat = orc.gen_lp_basis(150, 5, 4, 0.8, 3, 0.6)
m, SEED, NUPD = 150, 31, 6
for hist in (0, NUPD):  # a pending update on a fresh factorization, and on one with updates behind it
    for moment, trs in CP.MOMENTS.items():
        g = handle(mat)
        o, cols, pr, log = CP.history(orc, mat, SEED, hist, handle=g)
        p = CP.replacement(cols, m, np.random.default_rng(7))
        CP.advance(g, o, p, trs)
        d = blu_amd.BLU(m, 1)
        assert blu_amd.copy_batch(g, [d]) == [K.OK]
        CP.same_state(g, d, (hist, moment))
        od, _, _, _ = CP.history(orc, mat, SEED, hist)
        pd = dict(p, done=[])
        CP.advance(None, od, pd, trs)
        if moment == "both":  # update() right after the copy is valid
            assert pd["xtbl"] == p["xtbl"]
        sg = CP.finish(g, o, p, (hist, moment, "source"))
        sd = CP.finish(d, od, pd, (hist, moment, "copy"))
        assert sg == sd == K.OK and p["xtbl"] == pd["xtbl"], (hist, moment, sg, sd)
        assert g.stat(K.STAT_PIVOT_ERROR) == d.stat(K.STAT_PIVOT_ERROR) == o.stat(K.STAT_PIVOT_ERROR)
        assert g.stat(K.STAT_NUPDATE) == d.stat(K.STAT_NUPDATE) == (log["done"] if log else 0) + 1
        CP.same_state(g, d, (hist, moment, "after the update"))
        CP.check_members([g, d], [o, od], 15, (hist, moment))
        CP.same_state(g, d, (hist, moment, "after the solves"))
        print(hist, moment, "ok")
print("COPY PENDING OK")
"""

CHILD_INVALID = r"""
mat = orc.gen_lp_basis(90, 4, 5, 0.3, 7, 0.5)
cp, ri, v = mat
m = 90
o = CP.twin_of(orc, *mat)
never = blu_amd.BLU(m, len(ri))
never.set_param(K.PARAM_DROPTOL, 1e-18)
refused = blu_amd.BLU(m, len(ri))
bad_i = ri.copy()
bad_i[3] = 999
assert refused.factorize(cp[:-1], cp[1:], bad_i, v) == INVARG
rhs = np.cos(np.arange(float(m)))
for src, droptol in ((never, 1e-18), (refused, 1e-20)):
    d = handle(mat)                      # holds a factorization of its own
    d.solve_sparse_multi([[1]], [[1.0]])
    assert blu_amd.copy_batch(src, [d]) == [K.OK]
    assert src.dbg_copy_counts()[:3] == (0, 0, 0)
    CP.same_state(src, d, "invalid source")
    assert d.stat(K.STAT_NUPDATE) == -1 and d.get_param(K.PARAM_DROPTOL) == droptol
    for call in (lambda: d.solve_dense(rhs), lambda: d.get_factors(), lambda: d.get_sparse_multi(0)):
        try:
            call()
        except blu_amd.BluError as err:
            assert err.status == INVCALL
        else:
            raise AssertionError("not refused")
    assert d.solve_sparse([1], [1.0]) == INVCALL and d.solve_for_update([1], [1.0]) == INVCALL and d.update(1.0) == INVCALL
    d.set_param(K.PARAM_DROPTOL, 1e-20)
    assert d.factorize(cp[:-1], cp[1:], ri, v) == K.OK   # ... and factorizes normally
    CP.check_members([d], [CP.twin_of(orc, *mat)], 16, "factorized after an invalid copy")
# m == 0: the host state, no launch
e = np.zeros(0, np.uint64)
z, zd = blu_amd.BLU(0, 1), blu_amd.BLU(0, 1)
assert z.factorize(e, e, e, np.zeros(0)) == K.OK
assert blu_amd.copy_batch(z, [zd]) == [K.OK] and z.dbg_copy_counts() == (0, 0, 0, 0, 0, 0)
CP.same_state(z, zd, "m == 0")
assert zd.stat(K.STAT_NUPDATE) == 0 and zd.solve_dense(np.zeros(0)).shape == (0,)
zc = z.clone()
CP.same_state(z, zc, "m == 0, clone")
# m == 1
one = (np.array([0, 1], np.uint64), np.array([0], np.uint64), np.array([-2.5]))
h1 = handle(one)
c1 = h1.clone()
CP.same_state(h1, c1, "m == 1")
o1 = CP.twin_of(orc, *one)
for tr in "NT":
    assert np.array_equal(c1.solve_dense(np.array([3.0]), tr), o1.solve_dense(np.array([3.0]), tr))
assert c1.solve_for_update([0], None, "T") == K.OK and c1.solve_for_update([0], [4.0], "N") == K.OK and c1.update(c1.lhs[0]) == K.OK
assert np.array_equal(c1.solve_dense(np.array([3.0])), np.array([0.75])) and np.array_equal(h1.solve_dense(np.array([3.0])), np.array([-1.2]))
print("COPY INVALID OK")
"""

CHILD_REFUSALS = r"""
mat = orc.gen_lp_basis(90, 4, 5, 0.3, 7, 0.5)
other = orc.gen_lp_basis(90, 5, 5, 0.5, 9, 0.5)
m = 90
g = handle(mat)
d1, d2 = handle(other), handle(other)
small = handle(orc.gen_lp_basis(60, 4, 4, 0.5, 2, 0.5))
oo = CP.twin_of(orc, *other)
rhs = np.sin(np.arange(float(m)))
x0 = {tr: d1.solve_dense(rhs, tr) for tr in "NT"}
held = d1.solve_sparse_multi([[2, 5]], [[1.0, -1.0]])
assert oo.solve_sparse([2, 5], [1.0, -1.0])[0] == K.OK  # (the twin's flop counters follow)
states = [CP.state_of(h) for h in (g, d1, d2, small)]
for want, src, dsts, n in ((MISS, None, [d1, d2], None), (MISS, g, [d1, None], None), (MISS, g, [None, d2], None), (MISS, g, [d1, d2], -1),
                           (INVARG, g, [d1, g], None), (INVARG, g, [g], None), (INVARG, g, [d1, d2, d1], None), (INVARG, g, [d1, small], None),
                           (INVARG, small, [d1, d2], None)):
    rc, st = raw_copy(src, dsts, n)
    assert rc == want and (n == -1 or st == [want] * len(dsts)), (want, rc, st)
    assert raw_copy(src, dsts, n, status=False)[0] == want
assert L.blu_hip_copy_batch(g._h, None, 2, None) == MISS
st = (C.c_int * 2)(77, 77)
assert L.blu_hip_copy_batch(g._h, None, 2, st) == MISS and list(st) == [MISS, MISS]
assert raw_copy(g, [], 0) == (K.OK, []) and raw_copy(g, [d1], 0) == (K.OK, [77])   # n == 0: nothing written
for want in (MISS, INVARG):
    try:
        blu_amd.copy_batch(g, [d1, g] if want == INVARG else [d1, type("H", (), {"_h": None})()])
    except blu_amd.BluError as err:
        assert err.status == want
    else:
        raise AssertionError("not raised")
# no handle was touched: statistics, the held multi result and the bits of the destination's own factorization
for h, s in zip((g, d1, d2, small), states):
    now = CP.state_of(h)
    assert np.array_equal(now[0], s[0]) and np.array_equal(now[1], s[1])
il, xl = d1.get_sparse_multi(len(held[1][0][0]))
assert np.array_equal(il, held[1][0][0]) and np.array_equal(xl, held[1][0][1])
for tr in "NT":
    assert np.array_equal(d1.solve_dense(rhs, tr), x0[tr]) and np.array_equal(x0[tr], oo.solve_dense(rhs, tr))
CP.check_members([d1, d2], [oo, CP.twin_of(orc, *other)], 17, "after the refusals")
print("COPY REFUSALS OK")
"""

CHILD_COUNTS = r"""
mat = orc.gen_lp_basis(150, 5, 4, 0.8, 3, 0.6)
m = 150
g = handle(mat)
o, cols, pr, log = CP.history(orc, mat, 5, 4, handle=g)
one = [blu_amd.BLU(m, 1)]
five = [blu_amd.BLU(m, 1 + 100 * k) for k in range(5)]
assert blu_amd.copy_batch(g, one) == [K.OK]
c1 = g.dbg_copy_counts()
assert blu_amd.copy_batch(g, five) == [K.OK] * 5
c5 = g.dbg_copy_counts()
print(c1, c5)
assert c1[:3] == c5[:3] == (1, 1, 1), "launches, synchronizes and uploads depend on n"
assert c1[3] > 0 and c5[3] > 0
assert c1[4] == c5[4] > 0 and c1[5] == c1[4] and c5[5] == 5 * c5[4]
assert c1[4] % 4 == 0
# a second copy into the same destinations: every array has room
assert blu_amd.copy_batch(g, five) == [K.OK] * 5
again = g.dbg_copy_counts()
assert again[3] == 0 and again[:3] == (1, 1, 1) and again[4:] == c5[4:], again
assert blu_amd.copy_batch(g, one) == [K.OK] and g.dbg_copy_counts()[3] == 0
# ... also after the source has moved on
assert U.run_updates(g, cols, m, 2, np.random.default_rng(6), pair_row=pr, twin=o)["done"] >= 1
assert blu_amd.copy_batch(g, five) == [K.OK] * 5
moved = g.dbg_copy_counts()
assert moved[3] == 0 and moved[4] != c5[4], moved
for d in five:
    CP.same_state(g, d, "second copy")
c = g.clone()
assert g.dbg_copy_counts()[:3] == (1, 1, 1)
CP.check_members([g] + five + [c], [o] * 7, 18, "counts")
print("COPY COUNTS OK")
"""

CHILD_BATCH = r"""
from tests import util_update_batch as UB
mat = orc.gen_lp_basis(150, 5, 4, 0.8, 3, 0.6)
m, SEED, NUPD, N = 150, 9, 5, 6
g = handle(mat)
o, cols, pr, log = CP.history(orc, mat, SEED, NUPD, handle=g)
assert log["done"] >= 2
dsts = [blu_amd.BLU(m, len(mat[1])) for k in range(N)]
assert blu_amd.copy_batch(g, dsts) == [K.OK] * N
members = [g] + dsts
twins = [o] + [CP.history(orc, mat, SEED, NUPD)[0] for d in dsts]
rng = np.random.default_rng(19)
# solve_for_update_batch: forward with 7 different columns, then transposed; update_batch
ps = [CP.replacement(cols, m, np.random.default_rng(300 + k)) for k in range(N + 1)]
assert len({(p["j"], tuple(p["ai"])) for p in ps}) == N + 1
sts = blu_amd.solve_for_update_batch(members, [p["ai"] for p in ps], [p["ax"] for p in ps], "N")
assert sts == [K.OK] * (N + 1)
for h, t, p in zip(members, twins, ps):
    st, il, lhs = t.solve_for_update(p["ai"], p["ax"], "N")
    assert st == K.OK and np.array_equal(h.ilhs[:h.nzlhs], il) and np.array_equal(h.lhs, lhs)
    p["xtbl"] = lhs[p["j"]]
sts = blu_amd.solve_for_update_batch(members, [[p["j"]] for p in ps], None, "T")
assert sts == [K.OK] * (N + 1)
for h, t, p in zip(members, twins, ps):
    st, il, lhs = t.solve_for_update([p["j"]], None, "T")
    assert st == K.OK and np.array_equal(h.ilhs[:h.nzlhs], il) and np.array_equal(h.lhs, lhs)
sts = blu_amd.update_batch(members, [p["xtbl"] for p in ps])
assert sts == [t.update(p["xtbl"]) for t, p in zip(twins, ps)] == [K.OK] * (N + 1)
for h, t in zip(members, twins):
    CP.same_twin_stats(h, t, "after update_batch")
# solve_dense_batch and solve_sparse_batch, every member with a right-hand side of its own
rhs = rng.standard_normal((N + 1, m))
for tr in "NT":
    sols, sts = blu_amd.solve_dense_batch(members, rhs, tr)
    assert sts == [K.OK] * (N + 1)
    for k, t in enumerate(twins):
        assert np.array_equal(sols[k], t.solve_dense(rhs[k], tr)), ("solve_dense_batch", tr, k)
    irs = [rng.choice(m, 1 + k, replace=False) for k in range(N + 1)]
    xrs = [rng.standard_normal(len(ir)) for ir in irs]
    assert blu_amd.solve_sparse_batch(members, irs, xrs, tr) == [K.OK] * (N + 1)
    for k, (h, t) in enumerate(zip(members, twins)):
        st, il, lhs = t.solve_sparse(irs[k], xrs[k], tr)
        assert st == K.OK and np.array_equal(h.ilhs[:h.nzlhs], il) and np.array_equal(h.lhs, lhs), ("solve_sparse_batch", tr, k)
for h, t in zip(members, twins):
    CP.same_twin_stats(h, t, "after the batch solves")
# factorize_batch of all seven on new matrices
mats = [orc.gen_lp_basis(150, 5, 4, 0.6, 50 + k, 0.6) for k in range(N + 1)]
assert blu_amd.factorize_batch(members, mats) == [K.OK] * (N + 1)
fresh = [CP.twin_of(orc, *mt) for mt in mats]
for k, (h, t) in enumerate(zip(members, fresh)):
    assert h.stat(K.STAT_NFACTORIZE) == 2 and h.stat(K.STAT_NFORREST_TOTAL) == twins[k].stat(K.STAT_NFORREST_TOTAL)
CP.check_members(members, fresh, 20, "factorize_batch after the copies", keys=CP.TWIN_STATS[:-3])  # (the totals: the handle's life)
print("COPY BATCH OK")
"""

CHILD_MAXVOLUME = r"""
from tests import util_maxvolume as MV
problem = (60, 150, 2, 1.5)
nrow, ncol, seed, tol = problem
a = MV._problem(*problem[:3])
g = blu_amd.BLU(nrow, len(a[1]))
o = MV.oracle_twin(orc, nrow, len(a[1]))
trace = MV.loop_trace(o, problem, a, max_sweeps=2)
basis, isbasic = MV.start(nrow, ncol)
st, nup = g.maxvolume(ncol, a[0], a[1], a[2], basis, isbasic, tol)
MV.same_snapshot(MV.snapshot(g, a, st, nup, basis, isbasic), trace[0], "first pass")
assert nup > 0 and len(trace) == 2
c = g.clone()
CP.same_state(g, c, "after the first pass")
snaps = []
for h in (c, g):  # one pass on the copy and on the source
    b, ib = list(basis), list(isbasic)
    st, nup = h.maxvolume(ncol, a[0], a[1], a[2], b, ib, tol)
    snaps.append(MV.snapshot(h, a, st, nup, b, ib))
MV.same_snapshot(snaps[0], snaps[1], "copy against source")
MV.same_snapshot(snaps[0], trace[1], "copy against the loop on the oracle")
assert snaps[0]["stats"][MV.BRANCH] == snaps[1]["stats"][MV.BRANCH]
CP.same_state(g, c, "after the second pass", skip=CP.TIMING)
print("COPY MAXVOLUME OK")
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def run_child(emu_lib, body, ok, *args, timeout=2400):
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1")
    out = subprocess.run([sys.executable, "-c", HEAD + body, ROOT] + [str(x) for x in args], env=env, capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0 and ok in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("which", ("lp200", "lp150", "rankdef", "odd203"))
def test_copy_of_a_fresh_factorization_on_the_cpu(emu_lib, which):
    """lp(200,8,8,0.5,1,0.3), lp(150,5,4,0.8,3,0.6), the rank-deficient lp(90) with three scaled columns and m = 203 (every
    segment ends with a tile shorter than 16 bytes), each copied into a new handle with the full hint, one with b_nz = 1
    (every growable array grows) and one that holds an updated factorization of another matrix with the same nfactorize and
    a row-wise L of its own: parameters, statistics 0..124, get_factors, the solves and the multi solves are the source's
    and the twin's; the source is unchanged and still its twin's afterwards"""
    run_child(emu_lib, CHILD_FRESH, "COPY FRESH OK", which)


def test_copy_of_an_updated_factorization_on_the_cpu(emu_lib):
    """m = 200 after 25 update rounds (Forrest-Tomlin and permutation updates present), copied into 4 destinations; every
    member then takes 5 rounds of its own in lock step with a twin of its own, and all solve; again after the source is
    closed"""
    run_child(emu_lib, CHILD_UPDATED, "COPY UPDATED OK")


def test_copy_with_a_pending_update_on_the_cpu(emu_lib):
    """copied after the forward solve_for_update, after the transposed one and after both, on a fresh factorization and on
    one with 6 update rounds behind it: source and copy finish the update separately with the same xtbl -- statuses,
    PIVOT_ERROR, every statistic and the solves afterwards are equal"""
    run_child(emu_lib, CHILD_PENDING, "COPY PENDING OK")


def test_copy_of_an_invalid_source_and_the_smallest_sizes_on_the_cpu(emu_lib):
    """a never-factorized source and one whose factorize was refused: the destination answers INVALID_CALL with NUPDATE -1,
    drops its held multi result, takes the parameters, and factorizes normally afterwards; m == 0 copies the host state
    without a launch; m == 1"""
    run_child(emu_lib, CHILD_INVALID, "COPY INVALID OK")


def test_copy_refusals_on_the_cpu(emu_lib):
    """NULL src / dst / dst[k] and n < 0 (ARGUMENT_MISSING); the source among the destinations, a destination twice, another
    m (INVALID_ARGUMENT): every status[k] carries the code and no handle is touched -- a destination's own factorization
    solves with unchanged bits, statistics and held multi result.  n == 0 is OK.  (Another device cannot be had on the one
    device of the emulation build: tests/test_gpu_copy.py covers it where the machine has two.)"""
    run_child(emu_lib, CHILD_REFUSALS, "COPY REFUSALS OK")


def test_copy_counts_on_the_cpu(emu_lib):
    """dbg_copy_counts: one launch, one synchronize, one upload for n = 1 and n = 5; a second copy into the same
    destinations allocates nothing, also after the source has moved on; bytes written = n * bytes read"""
    run_child(emu_lib, CHILD_COUNTS, "COPY COUNTS OK")


def test_copies_through_the_batch_entries_on_the_cpu(emu_lib):
    """the source and 6 copies through solve_for_update_batch (forward with 7 different columns, then transposed),
    update_batch, solve_dense_batch, solve_sparse_batch -- each member beside its twin -- and factorize_batch of all seven on
    new matrices"""
    run_child(emu_lib, CHILD_BATCH, "COPY BATCH OK")


def test_maxvolume_on_a_copy_on_the_cpu(emu_lib):
    """the 60 x 150 problem: after a first pass the handle is cloned, and one more pass runs on the copy and on the source --
    status, nupdate, basis, isbasic, statistics and the solves afterwards agree with each other and with the loop on the
    oracle"""
    run_child(emu_lib, CHILD_MAXVOLUME, "COPY MAXVOLUME OK")


def test_copy_replay_under_address_sanitizer(emu_lib, oracle, tmp_path):
    """A tape of tools/emu_replay.cpp recorded from the oracle alone, m = 60 and m = 12: factorize, solves, OP_COPY_INTO 1 (a
    new handle with b_nz = 1 receives the copy, the original is freed), solves, 10 update rounds, OP_CLONE (the original is
    freed), 10 update rounds, solves.  Whatever a copy still shared with its freed original, and every access of
    k_copy_fanout outside a segment, is an AddressSanitizer report.  Replayed with the plain build and with the sanitized
    one (the executable carries the sanitizer runtime; nothing is preloaded)."""
    import numpy as np

    from blu_amd import keys as K
    from tests import util_update as U
    from tests.test_emu_cpu_solves import Tape

    class CopyTape(Tape):
        def clone(self):
            self._i(OP_CLONE)

        def copy_into(self, b_nz):
            self._i(OP_COPY_INTO, b_nz)

        def solves(self, rng):
            m = self.m
            for tr in "NT":
                self.solve_dense(rng.standard_normal(m), tr)
                ir = rng.choice(m, max(1, m // 6), replace=False)
                assert self.solve_sparse(ir, rng.standard_normal(len(ir)), tr)[0] == K.OK
            for key in (K.STAT_NUPDATE, K.STAT_NFORREST, K.STAT_R_NZ, K.STAT_U_NZ, K.STAT_L_FLOPS, K.STAT_U_FLOPS, K.STAT_R_FLOPS,
                        K.STAT_NFORREST_TOTAL, K.STAT_NSYMPERM_TOTAL):
                self.stat(key)

    subprocess.check_call(["make", "-s", "-C", CSRC, "emu_replay", "emu_replay_asan"])
    t = CopyTape(oracle)
    for m, spec in ((60, (60, 4, 4, 0.4, 6, 0.5)), (12, (12, 3, 3, 0.4, 2, 0.5))):
        cp, ri, v = oracle.gen_lp_basis(*spec)
        rng = np.random.default_rng(m)
        t.new(m, len(ri), 64 * len(ri) + 1024)
        assert t.factorize(cp, ri, v) == K.OK
        t.solves(rng)
        t.copy_into(1)
        t.solves(rng)
        cols = U.columns_of(cp, ri, v)
        assert U.run_updates(t, cols, m, 10, rng)["done"] >= 2
        t.clone()
        assert U.run_updates(t, cols, m, 10, rng)["done"] >= 2
        t.solves(rng)
    tape = str(tmp_path / "copy.tape")
    t.write(tape)
    env = {k: v for k, v in os.environ.items() if k != "BLU_HIP_LIB"}
    env.update(BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    for exe in (REPLAY, REPLAY_ASAN):
        out = subprocess.run([exe, tape], env=env, capture_output=True, text=True, timeout=1800)
        assert "AddressSanitizer" not in out.stderr, out.stderr[-6000:]
        assert out.returncode == 0 and "REPLAY OK" in out.stdout, (exe, out.returncode, out.stdout[-500:] + out.stderr[-4000:])
