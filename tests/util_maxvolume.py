"""Shared by the tests of the native maxvolume pass (BLU.maxvolume, blu_hip_maxvolume): the problem generator of
tests/test_maxvolume.py restated unchanged, the problems with what the loop blu_amd.maxvolume does on them on the CPU
oracle, and the comparison of a handle driven by the native pass with a twin driven by the loop -- equalities only."""
import numpy as np

from blu_amd import keys as K
from blu_amd.maxvolume import maxvolume as loop

BRANCH = 43  # branch of the last sparse solve: 1 symbolic, 2 sequential
STATS = (K.STAT_NUPDATE, K.STAT_NFACTORIZE, K.STAT_NFORREST, K.STAT_PIVOT_ERROR, K.STAT_L_FLOPS, K.STAT_U_FLOPS, K.STAT_R_FLOPS,
         K.STAT_R_NZ, K.STAT_U_NZ, K.STAT_MAX_ETA, K.STAT_UPDATE_COST, K.STAT_NSYMPERM_TOTAL, K.STAT_NFORREST_TOTAL,
         K.STAT_DEV_NUNSYMPERM_TOTAL, BRANCH)

# (nrow, ncol, seed, volumetol) -> (updates, refactorizations inside the pass) of the FIRST sweep from the identity-like
# basis, as the loop takes them on the CPU oracle.  The refactorizations of the second, fourth and fifth problem are driven
# by UPDATE_COST, those of the third by nforrest == m: a pass that counts the flops of a candidate it did not reach in order
# refactorizes at another moment.
PROBLEMS = {
    (30, 90, 1, 2.0): (27, 0),
    (60, 150, 2, 1.5): (60, 1),
    (12, 40, 3, 1.0): (19, 1),
    (96, 400, 5, 1.2): (163, 3),
    (300, 1500, 11, 1.5): (465, 8),
}


def _problem(nrow, ncol, seed):
    rng = np.random.default_rng(seed)
    cols = [dict() for _ in range(ncol)]
    for j in range(nrow):  # an identity-like start so that the initial basis is nonsingular
        cols[j][j] = 1.0
    for j in range(ncol):
        for i in rng.choice(nrow, int(rng.integers(1, 5)), replace=False):
            cols[j][int(i)] = cols[j].get(int(i), 0.0) + float(rng.standard_normal()) * (3.0 if j >= nrow else 0.3)
    a_p, a_i, a_x = [0], [], []
    for c in cols:
        for i, x in c.items():
            a_i.append(i); a_x.append(x)
        a_p.append(len(a_i))
    return np.array(a_p, np.uint64), np.array(a_i, np.uint64), np.array(a_x)


def start(nrow, ncol):
    return list(range(nrow)), [1] * nrow + [0] * (ncol - nrow)


def oracle_twin(orc, nrow, nz):
    o = orc.OracleBLU(nrow, 64 * nz + 1024)
    o.set_fix_d3(True)
    return o


def _ss(h, irhs, xrhs, trans):
    out = h.solve_sparse(irhs, xrhs, trans)
    if isinstance(out, tuple):
        return out
    return out, h.ilhs[:h.nzlhs].copy(), h.lhs.copy()


def snapshot(h, a, st, nup, basis, isbasic, solve_cols=(0, 1, 2)):
    """What a pass left behind: its results, the statistics, then solve_sparse of three columns of A in both systems"""
    a_p, a_i, a_x = a
    ncol = len(a_p) - 1
    snap = dict(st=st, nup=nup, basis=[int(x) for x in basis], isbasic=[int(x) for x in isbasic], stats={k: h.stat(k) for k in STATS}, solves={})
    if st == K.OK and h.m > 0:
        for c in solve_cols:
            j = ncol - 1 - c
            b, e = int(a_p[j]), int(a_p[j + 1])
            for tr in "NT":
                snap["solves"][(j, tr)] = _ss(h, a_i[b:e], a_x[b:e], tr)
    return snap


def same_snapshot(x, y, what):
    """equalities only; the branch statistic is compared where both sides keep it (the oracle does not)"""
    assert (x["st"], x["nup"]) == (y["st"], y["nup"]), (what, x["st"], x["nup"], y["st"], y["nup"])
    assert x["basis"] == y["basis"] and x["isbasic"] == y["isbasic"], (what, "basis / isbasic")
    for key in STATS:
        u, v = x["stats"][key], y["stats"][key]
        if key == BRANCH and (u != u or v != v):
            continue
        assert u == v, (what, "statistic", key, u, v)
    assert x["solves"].keys() == y["solves"].keys()
    for k, (s1, il1, l1) in x["solves"].items():
        s2, il2, l2 = y["solves"][k]
        assert s1 == s2 == K.OK and np.array_equal(il1, il2) and np.array_equal(l1, l2), (what, "solve_sparse", k)


def loop_trace(h, problem, a, max_sweeps=40):
    """the loop blu_amd.maxvolume on h, sweep after sweep until one changes nothing: the snapshots"""
    nrow, ncol, seed, tol = problem
    basis, isbasic = start(nrow, ncol)
    out = []
    for sweep in range(max_sweeps):
        st, nup = loop(h, ncol, a[0], a[1], a[2], basis, isbasic, tol)
        out.append(snapshot(h, a, st, nup, basis, isbasic))
        if st != K.OK or nup == 0:
            break
    return out


def native_trace(g, problem, a, chunk=None, max_sweeps=40):
    """the same with BLU.maxvolume; every snapshot with the dbg_maxvolume_counts of its pass"""
    nrow, ncol, seed, tol = problem
    basis, isbasic = start(nrow, ncol)
    g.dbg_set_maxvolume_chunk(-1 if chunk is None else chunk)
    out = []
    for sweep in range(max_sweeps):
        nf0 = g.stat(K.STAT_NFACTORIZE)
        st, nup = g.maxvolume(ncol, a[0], a[1], a[2], basis, isbasic, tol)
        snap = snapshot(g, a, st, nup, basis, isbasic)
        snap["counts"] = g.dbg_maxvolume_counts()
        snap["nfact"] = int(g.stat(K.STAT_NFACTORIZE) - nf0) - 1
        out.append(snap)
        if st != K.OK or nup == 0:
            break
    return out


def check(native, traces, problem, chunk, whole=True):
    """a native trace against loop traces of the same problem (whole: to the sweep that changes nothing)"""
    nrow, ncol, seed, tol = problem
    for t in traces:
        assert len(native) == len(t) or not whole, (problem, chunk, len(native), len(t))
        for sweep, (x, y) in enumerate(zip(native, t)):
            same_snapshot(x, y, (problem, chunk, sweep))
    first = native[0]
    assert (first["nup"], first["nfact"]) == PROBLEMS[problem], (problem, first["nup"], first["nfact"])
    for x in native:
        assert x["counts"][3] == x["nup"], x["counts"]  # hits
    if chunk is None or chunk > 1:
        assert first["counts"][2] > 0, first["counts"]  # candidates were priced behind a hit and thrown away
    else:
        assert first["counts"][2] == 0 and first["counts"][0] == first["counts"][1], first["counts"]
    if whole:
        last = native[-1]
        assert last["st"] == K.OK and last["nup"] == 0, "no locally maximal basis"
        assert last["counts"][3] == 0 and last["counts"][1] == ncol - nrow, last["counts"]  # no hit: every non-basic column priced once
