"""Shared by the tests of blu_hip_copy_batch / blu_hip_clone (tests/test_emu_cpu_copy.py, tests/test_gpu_copy.py).

The oracle has no clone: the twin of a copy is a FRESH OracleBLU driven through the recorded history of the source -- the
same matrix and the same seeded tests.util_update.run_updates sequence (`history`).  A copy is then compared with the
source (every parameter, every statistic key 0..124, bit for bit) and, through `exercise`, with its twin: get_factors,
solve_dense, solve_sparse (pattern order, values, flop counters), solve_dense_multi and solve_sparse_multi.  Equalities
only (np.array_equal / ==), over all members."""
import numpy as np

from blu_amd import keys as K
from tests import util_update as U

PARAMS = tuple(range(11))
STATS = tuple(range(125))
# what a twin on the oracle keeps as well (NFACTORIZE only where the histories agree in it: every twin here factorizes once)
TWIN_STATS = (K.STAT_M, K.STAT_NUPDATE, K.STAT_L_NZ, K.STAT_U_NZ, K.STAT_MIN_PIVOT, K.STAT_MAX_PIVOT, K.STAT_RANK, K.STAT_NFORREST,
              K.STAT_PIVOT_ERROR, K.STAT_R_NZ, K.STAT_MAX_ETA, K.STAT_L_FLOPS, K.STAT_U_FLOPS, K.STAT_R_FLOPS, K.STAT_UPDATE_COST,
              K.STAT_NSYMPERM_TOTAL, K.STAT_NFORREST_TOTAL, K.STAT_DEV_NUNSYMPERM_TOTAL)
# the timing keys: copied with the rest, but every later factorize writes its own
TIMING = (24, 25, 26, 27, 40, 41, 44, 45, 46, 47, 108, 109)
FLOPS = (K.STAT_L_FLOPS, K.STAT_U_FLOPS, K.STAT_R_FLOPS)


def bits(xs):
    return np.array(xs, np.float64).view(np.uint64)


def state_of(h):
    """every parameter and every statistic key 0..124, as bit patterns (NaN of a key without a meaning included)"""
    return bits([h.get_param(k) for k in PARAMS]), bits([h.stat(k) for k in STATS])


def same_state(a, b, what, skip=()):
    """handle b answers every get_param and every get_stat key as handle a does"""
    pa, sa = state_of(a)
    pb, sb = state_of(b)
    assert np.array_equal(pa, pb), (what, "parameters", np.flatnonzero(pa != pb))
    keep = np.array([k not in skip for k in STATS])
    assert np.array_equal(sa[keep], sb[keep]), (what, "statistics", [k for k in STATS if k not in skip and sa[k] != sb[k]])


def same_twin_stats(h, o, what, keys=TWIN_STATS):
    for key in keys:
        assert h.stat(key) == o.stat(key), (what, "statistic", key, h.stat(key), o.stat(key))


def twin_of(orc, cp, ri, v, want=K.OK, params=()):
    o = orc.OracleBLU(len(cp) - 1, 64 * len(ri) + 1024)
    o.set_fix_d3(True)
    for key, value in params:
        o.set_param(key, value)
    st = o.factorize(cp[:-1], cp[1:], ri, v)
    assert st == want, (st, want)
    return o


def pair_rows(f, m):
    """row paired with every column in the factorization f = get_factors()"""
    pr = np.zeros(m, np.int64)
    pr[f["colperm"]] = f["rowperm"]
    return pr


def history(orc, mat, seed, nupd, handle=None, want=K.OK, params=()):
    """The recorded history of a source: factorize `mat`, then `nupd` rounds of run_updates seeded with `seed`.
    With `handle` (already factorized on mat) it is driven in lock step with the new twin; without, the twin alone is
    driven through the same history.  Returns (twin, cols, pair_row, log)."""
    cp, ri, v = mat
    m = len(cp) - 1
    o = twin_of(orc, cp, ri, v, want, params)
    cols = U.columns_of(cp, ri, v)
    pr = pair_rows(o.get_factors(), m)
    log = None
    if nupd:
        rng = np.random.default_rng(seed)
        if handle is None:
            log = U.run_updates(o, cols, m, nupd, rng, pair_row=pr)
        else:
            log = U.run_updates(handle, cols, m, nupd, rng, pair_row=pr, twin=o)
    return o, cols, pr, log


def _rhs_set(m, seed):
    rng = np.random.default_rng(seed)
    dense = rng.standard_normal((3, m))
    sparse = []
    for nz in (1, max(1, m // 12), max(1, m // 3)):
        ir = rng.choice(m, min(nz, m), replace=False)
        sparse.append((ir, rng.standard_normal(len(ir))))
    return dense, sparse


def exercise(h, seed):
    """The solves of a copy test on a handle of the library: a list of (name, value) with arrays and numbers.  Leaves
    L_FLOPS / U_FLOPS / R_FLOPS grown by what exercise_twin adds on the oracle."""
    m = h.m
    dense, sparse = _rhs_set(m, seed)
    out = []
    if h.stat(K.STAT_NUPDATE) == 0:
        f = h.get_factors()
        out += [("factors " + k, f[k]) for k in sorted(f)]
    for tr in "NT":
        out.append(("solve_dense " + tr, h.solve_dense(dense[0], tr)))
    for tr in "NT":
        for n, (ir, xr) in enumerate(sparse):
            st, il, lhs = U._ss(h, ir, xr, tr)
            assert st == K.OK
            out += [("solve_sparse pattern %s %d" % (tr, n), il), ("solve_sparse values %s %d" % (tr, n), lhs)]
            out.append(("flops %s %d" % (tr, n), np.array([h.stat(k) for k in FLOPS])))
    for tr in "NT":
        out.append(("solve_dense_multi " + tr, h.solve_dense_multi(dense, tr)))
    for tr in "NT":
        sts, sols = h.solve_sparse_multi([s[0] for s in sparse], [s[1] for s in sparse], tr)
        assert sts == [K.OK] * len(sparse)
        for n, (il, xl) in enumerate(sols):
            out += [("solve_sparse_multi pattern %s %d" % (tr, n), il), ("solve_sparse_multi values %s %d" % (tr, n), xl)]
        out.append(("flops multi " + tr, np.array([h.stat(k) for k in FLOPS])))
    return out


def exercise_twin(o, seed):
    """The same on the oracle, the multi calls as single calls in order"""
    m = o.m
    dense, sparse = _rhs_set(m, seed)
    out = []
    if o.stat(K.STAT_NUPDATE) == 0:
        f = o.get_factors()
        out += [("factors " + k, f[k]) for k in sorted(f)]
    for tr in "NT":
        out.append(("solve_dense " + tr, o.solve_dense(dense[0], tr)))
    for tr in "NT":
        for n, (ir, xr) in enumerate(sparse):
            st, il, lhs = o.solve_sparse(ir, xr, tr)
            assert st == K.OK
            out += [("solve_sparse pattern %s %d" % (tr, n), il), ("solve_sparse values %s %d" % (tr, n), lhs)]
            out.append(("flops %s %d" % (tr, n), np.array([o.stat(k) for k in FLOPS])))
    for tr in "NT":
        out.append(("solve_dense_multi " + tr, np.array([o.solve_dense(r, tr) for r in dense])))
    for tr in "NT":
        for n, (ir, xr) in enumerate(sparse):
            st, il, lhs = o.solve_sparse(ir, xr, tr)
            assert st == K.OK
            out += [("solve_sparse_multi pattern %s %d" % (tr, n), il), ("solve_sparse_multi values %s %d" % (tr, n), lhs[il])]
        out.append(("flops multi " + tr, np.array([o.stat(k) for k in FLOPS])))
    return out


def same_results(a, b, what):
    assert [n for n, _ in a] == [n for n, _ in b], what
    for (name, x), (_, y) in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y)), (what, name)


def check_members(handles, twins, seed, what, keys=TWIN_STATS):
    """every handle through exercise(), every result that of its twin (twins[k] may be shared by handles that ran the same
    calls since the copy: then it is exercised once); afterwards the statistics of TWIN_STATS agree as well"""
    done = {}
    for k, (h, o) in enumerate(zip(handles, twins)):
        if id(o) not in done:
            done[id(o)] = exercise_twin(o, seed)
        same_results(exercise(h, seed), done[id(o)], (what, "member", k))
        same_twin_stats(h, o, (what, "member", k), keys)


MOMENTS = {"ftran": ("N",), "btran": ("T",), "both": ("T", "N")}


def replacement(cols, m, rng):
    """A column to bring in at position j: 1.5 times the outgoing column plus 0.3 times another column of the basis, so
    that the forward solution has 1.5 at j (a pivot far from zero) whatever the basis is.  Returns a pending-update dict."""
    j, k = (int(x) for x in rng.choice(m, 2, replace=False))
    rows = {}
    for i, x in zip(*cols[j]):
        rows[int(i)] = 1.5 * float(x)
    for i, x in zip(*cols[k]):
        rows[int(i)] = rows.get(int(i), 0.0) + 0.3 * float(x)
    idx = np.array(sorted(rows), np.int64)
    return dict(j=j, ai=idx, ax=np.array([rows[int(i)] for i in idx]), xtbl=None, done=[])


def advance(h, o, p, trs):
    """the solve_for_update calls `trs` of the pending update p on handle h (None: the twin alone) and twin o, in lock step"""
    for tr in trs:
        args = (p["ai"], p["ax"], "N") if tr == "N" else ([p["j"]], None, "T")
        b = U._sfu(o, *args)
        assert b[0] == K.OK
        if h is not None:
            U._same(U._sfu(h, *args), b, ("solve_for_update", tr))
        if tr == "N":
            p["xtbl"] = b[2][p["j"]]
        p["done"].append(tr)


def finish(h, o, p, what):
    """what is still missing of the pending update p, then update() on handle and twin: the status of both"""
    advance(h, o, p, [tr for tr in "TN" if tr not in p["done"]])
    st = h.update(p["xtbl"])
    assert o.update(p["xtbl"]) == st, (what, "update status")
    return st
