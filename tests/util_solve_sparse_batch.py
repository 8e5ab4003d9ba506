"""Driver of the batched solve_sparse tests (blu_amd.solve_sparse_batch): members of one call, each compared with a CPU
oracle twin and with a second handle of the library, both driven by the single solve_sparse with the same right-hand
side.  Used by tests/test_emu_cpu_solve_sparse_batch.py (emulation build) and tests/test_gpu_solve_sparse_batch.py."""
import ctypes as C

import numpy as np

from blu_amd import keys as K
from tests import util_update as U, util_update_batch as UB

SIZES = (0, 1, 5, 70, -1)  # entries of a right-hand side; 70 = more than one wave of lanes, -1 = m / 2 (all capped at m)
BRANCH = 43                # statistic: branch of the second triangular solve, 1 symbolic + sparse, 2 sequential
FLOPS = (K.STAT_L_FLOPS, K.STAT_U_FLOPS, K.STAT_R_FLOPS)


def scaled(cp, v, cols, by=1e-17):
    """columns scaled down until the factorization drops them: WARNING_SINGULAR_MATRIX (tests/test_emu_cpu_solves.py)"""
    v = v.copy()
    for j in cols:
        v[int(cp[j]):int(cp[j + 1])] *= by
    return v


class Member:
    def __init__(self, h, single, twin, mat, seed):
        self.h, self.single, self.twin, self.m = h, single, twin, h.m
        self.cols = U.columns_of(*mat)
        self.rng = np.random.default_rng(seed)
        self.seed, self.moves, self.pair_row = seed, 0, None

    def rhs(self, size):
        nz = min(self.m // 2 if size < 0 else size, self.m)
        return self.rng.choice(self.m, nz, replace=False), self.rng.standard_normal(nz)


def make_members(blu, orc, mats, want, twins=True):
    """For every matrix a handle for the batch calls and one for the single calls, all factorized by ONE factorize_batch
    (the default dispatch), and an oracle twin."""
    hs = [blu.BLU(len(cp) - 1, len(ri)) for cp, ri, v in mats for _ in range(2)]
    st = blu.factorize_batch(hs, [mat for mat in mats for _ in range(2)])
    assert st == [w for w in want for _ in range(2)], st
    members = []
    for k, (mat, w) in enumerate(zip(mats, want)):
        cp, ri, v = mat
        o = None
        if twins:
            o = orc.OracleBLU(len(cp) - 1, 256 * len(ri) + 1024)
            o.set_fix_d3(True)
            assert o.factorize(cp[:-1], cp[1:], ri, v) == w
        members.append(Member(hs[2 * k], hs[2 * k + 1], o, mat, 1000 + k))
    return members


def set_thres(members, thres):
    for M in members:
        for x in (M.h, M.single, M.twin):
            if x is not None:
                x.set_param(K.PARAM_SPARSE_THRES, thres)


def move_to_updated(M, nupd, min_done):
    """Column replacements by the single calls (tests/util_update.py::run_updates: solve_for_update twice, update, then a
    solve_dense and a solve_sparse of both systems after every one), the twin in lock step and the second handle after it."""
    if M.pair_row is None:
        M.pair_row = UB.pair_rows(M.h)
    M.moves += 1
    cols2 = [(i.copy(), x.copy()) for i, x in M.cols]
    log = U.run_updates(M.h, M.cols, M.m, nupd, np.random.default_rng(M.seed + M.moves), pair_row=M.pair_row, twin=M.twin)
    log2 = U.run_updates(M.single, cols2, M.m, nupd, np.random.default_rng(M.seed + M.moves), pair_row=M.pair_row)
    assert log["done"] >= min_done and log["done"] == log2["done"], (log, log2)
    assert M.h.stat(K.STAT_NUPDATE) == M.single.stat(K.STAT_NUPDATE) > 0
    return log


def compare(M, a, ir, xr, trans, where, stats=UB.STATS_LIBRARY):
    """a = (status, pattern, values) of member M from the batch call: the twin's and the second handle's, bit for bit"""
    assert a[0] == K.OK, (where, a[0])
    assert np.array_equal(np.sort(a[1]), np.flatnonzero(a[2])), (where, "pattern")
    if M.twin is not None:
        b = U._ss(M.twin, ir, xr, trans)
        assert len(a[1]) == len(b[1]), (where, "nzlhs", len(a[1]), len(b[1]))
        U._same(a, b, (where, "oracle"))
        for key in FLOPS:
            assert M.h.stat(key) == M.twin.stat(key), (where, "oracle stat", key, M.h.stat(key), M.twin.stat(key))
    if M.single is not None:
        c = U._ss(M.single, ir, xr, trans)
        assert len(a[1]) == len(c[1]), (where, "nzlhs", len(a[1]), len(c[1]))
        U._same(a, c, (where, "single"))
        for key in stats + (BRANCH,):
            assert M.h.stat(key) == M.single.stat(key), (where, "single stat", key, M.h.stat(key), M.single.stat(key))


def batch_round(blu, members, trans, q, where):
    """One solve_sparse_batch over `members`, member k with a right-hand side of SIZES[(q + k) % 5] entries; returns the
    set of branches taken."""
    rhs = [M.rhs(SIZES[(q + k) % len(SIZES)]) for k, M in enumerate(members)]
    st = blu.solve_sparse_batch([M.h for M in members], [r[0] for r in rhs], [r[1] for r in rhs], trans)
    assert st == [K.OK] * len(members), (where, st)
    seen = set()
    for k, (M, (ir, xr)) in enumerate(zip(members, rhs)):
        compare(M, (st[k],) + UB.solution(M.h), ir, xr, trans, (where, k, len(ir)))
        seen.add(int(M.h.stat(BRANCH)))
    return seen


def _vp(xs):
    return (C.c_void_p * max(len(xs), 1))(*xs)


def raw_call(blu, handles, nzr, ir, xr, trans, n=None, H=True, NZ=True, NZL=True, IL=True, LH=True, il_null=(), lh_null=(), st=True):
    """blu_hip_solve_sparse_batch itself: ir / xr are lists of arrays (None = NULL) or None; returns (rc, statuses, nzlhs,
    patterns, values) with the statuses pre-filled with 77"""
    FN = blu.lib().blu_hip_solve_sparse_batch
    FN.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_char, C.c_void_p]
    N = max(len(handles), 1)
    n = len(handles) if n is None else n
    s = (C.c_int * N)(*([77] * N))
    nz = (C.c_int64 * N)(*nzr)
    nzl = (C.c_int64 * N)(*([55] * N))
    il = [np.zeros(max(1, h.m if h is not None else 1), np.int64) for h in handles]
    lh = [np.zeros(max(1, h.m if h is not None else 1)) for h in handles]
    ptr = lambda arrs: None if arrs is None else _vp([None if a is None else a.ctypes.data for a in arrs])
    rc = FN(_vp([h._h if h is not None else None for h in handles]) if H else None, n, nz if NZ else None, ptr(ir), ptr(xr),
            nzl if NZL else None, _vp([None if k in il_null else a.ctypes.data for k, a in enumerate(il)]) if IL else None,
            _vp([None if k in lh_null else a.ctypes.data for k, a in enumerate(lh)]) if LH else None, trans, s if st else None)
    return rc, list(s)[:len(handles)], list(nzl)[:len(handles)], il, lh


def refusals(blu, members):
    """Every refusal of the call as a whole: each status carries the code, n == 0 writes nothing, no handle is touched."""
    MISS, INVARG = K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_ARGUMENT
    hs = [members[0].h, members[1].h]
    keys = (K.STAT_NUPDATE,) + FLOPS
    before = [[h.stat(key) for key in keys] for h in hs]
    i3, x3 = np.array([3], np.uint64), np.array([1.0])
    one, two = [1, 1], [i3, i3]

    def refused(code, *a, **kw):
        rc, st = raw_call(blu, *a, **kw)[:2]
        assert rc == code and st == [code] * len(st), (a[1:], kw, rc, st)

    refused(MISS, hs, one, two, [x3, x3], b"N", H=False)
    refused(MISS, hs, one, two, [x3, x3], b"N", NZ=False)
    refused(MISS, hs, one, two, [x3, x3], b"N", NZL=False)
    refused(MISS, hs, one, two, [x3, x3], b"N", IL=False)
    refused(MISS, hs, one, two, [x3, x3], b"N", LH=False)
    refused(MISS, [hs[0], None], one, two, [x3, x3], b"N")
    refused(MISS, hs, one, two, [x3, x3], b"T", il_null=(1,))
    refused(MISS, hs, one, two, [x3, x3], b"T", lh_null=(0,))
    refused(MISS, hs, one, None, [x3, x3], b"N")
    refused(MISS, hs, one, two, None, b"N")
    refused(MISS, hs, one, [i3, None], [x3, x3], b"N")
    refused(MISS, hs, one, two, [None, x3], b"T")
    refused(MISS, hs, [0, 1], None, None, b"N")                       # NULL arrays excused for the empty member alone
    assert raw_call(blu, hs, one, two, [x3, x3], b"N", n=-1)[0] == MISS
    refused(INVARG, [hs[0], hs[1], hs[0]], [1, 1, 1], [i3] * 3, [x3] * 3, b"N")
    rc, st, nzl = raw_call(blu, hs, one, two, [x3, x3], b"N", n=0)[:3]
    assert rc == K.OK and st == [77, 77] and nzl == [55, 55], (rc, st, nzl)   # n == 0: nothing written
    for call in (lambda: blu.solve_sparse_batch([hs[0], hs[0]], [[1], [1]], [[1.0], [1.0]]),):
        try:
            call()
        except blu.BluError as e:
            assert e.status == INVARG
        else:
            raise AssertionError("not refused")
    assert before == [[h.stat(key) for key in keys] for h in hs], "a refused call touched a handle"
    rc, st, nzl = raw_call(blu, hs, [0, 0], None, None, b"N")[:3]         # empty right-hand sides may pass NULL, as the single call allows
    assert rc == K.OK and st == [K.OK] * 2 and nzl == [0, 0], (rc, st, nzl)


def mixed_statuses(blu, orc, m=200):
    """One call with a solvable member, a never-factorized handle, an m == 0 handle, an index out of range and nzrhs > m:
    each member its own status, the others run regardless."""
    INVARG = K.ERROR_INVALID_ARGUMENT
    cp, ri, v = orc.gen_lp_basis(m, 5, 5, 0.5, 2, 0.3)
    hp, hrange, hmany = (blu.BLU(m, len(ri)) for _ in range(3))
    op = orc.OracleBLU(m, 64 * len(ri))
    op.set_fix_d3(True)
    assert blu.factorize_batch([hp, hrange, hmany], [(cp, ri, v)] * 3) == [K.OK] * 3
    assert op.factorize(cp[:-1], cp[1:], ri, v) == K.OK
    hnone = blu.BLU(120, 500)                                         # never factorized
    hz = blu.BLU(0, 1)                                                # m = 0
    e = np.zeros(0, np.uint64)
    assert hz.factorize(e, e, e, np.zeros(0)) == K.OK
    mixed = [hp, hnone, hz, hrange, hmany]
    want = [K.OK, K.ERROR_INVALID_CALL, K.OK, INVARG, INVARG]
    irs = [np.array(a, np.uint64) for a in ([3, 17, 5], [3], [], [1, m], np.arange(m + 1) % m)]
    xrs = [np.ones(len(a)) for a in irs]
    for trans in "NT":
        st = blu.solve_sparse_batch(mixed, irs, xrs, trans)
        assert st == want, (trans, st)
        assert hz.nzlhs == 0
        U._same((st[0],) + UB.solution(hp), U._ss(op, irs[0], xrs[0], trans), ("mixed", trans))
        # the C entry's return value: the most negative member status; status may be NULL
        rc, st, nzl, il, lh = raw_call(blu, mixed, [len(a) for a in irs], [a if len(a) else None for a in irs],
                                       [a if len(a) else None for a in xrs], trans.encode())
        assert st == want and rc == min(st), (rc, st)
        so = U._ss(op, irs[0], xrs[0], trans)
        assert nzl[0] == len(so[1]) and nzl[2] == 0 and np.array_equal(il[0][:nzl[0]], so[1]) and np.array_equal(lh[0], so[2])
        assert nzl[1] == nzl[3] == nzl[4] == 55 and not any(lh[k].any() for k in (1, 2, 3, 4))
        assert raw_call(blu, mixed[:1], [3], irs[:1], xrs[:1], trans.encode(), st=False)[0] == K.OK
        assert U._ss(op, irs[0], xrs[0], trans)[0] == K.OK
    for key in (K.STAT_L_FLOPS, K.STAT_U_FLOPS):
        assert hp.stat(key) == op.stat(key), key
