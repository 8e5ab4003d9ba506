"""Driver of the solve_sparse_multi tests (BLU.solve_sparse_multi): the right-hand sides of one call on ONE handle, each
compared with a CPU oracle twin and with a second handle of the library, both driven by the single solve_sparse with the
same right-hand sides in the same order.  Used by tests/test_emu_cpu_solve_sparse_multi.py (emulation build) and
tests/test_gpu_solve_sparse_multi.py."""
import ctypes as C

import numpy as np

from blu_amd import keys as K
from tests import util_update as U
from tests.util_solve_sparse_batch import BRANCH, SIZES

FLOPS = (K.STAT_L_FLOPS, K.STAT_U_FLOPS, K.STAT_R_FLOPS, K.STAT_UPDATE_COST)
SENT = 77


def columns(rng, m, nrhs, q=0, sizes=SIZES):
    """nrhs right-hand sides, number j with sizes[(q + j) % len(sizes)] entries (-1 = m / 2, all capped at m)"""
    out = []
    for j in range(nrhs):
        size = sizes[(q + j) % len(sizes)]
        nz = min(m // 2 if size < 0 else size, m)
        out.append((rng.choice(m, nz, replace=False), rng.standard_normal(nz)))
    return out


def dense_of(m, il, xl):
    x = np.zeros(m)
    x[il] = xl
    return x


def same_column(m, st, sol, b, where):
    """(status, (ilhs, xlhs)) of one right-hand side of the multi call against (status, pattern, dense values) of a single
    call: status, nzlhs, pattern order and the bits of the values"""
    il, xl = sol
    assert st == b[0] == K.OK, (where, st, b[0])
    assert len(il) == len(xl) == len(b[1]), (where, "nzlhs", len(il), len(b[1]))
    U._same((st, il, dense_of(m, il, xl)), b, where)
    assert np.array_equal(xl, b[2][b[1]]), (where, "compressed values")


def check_multi(g, cols, trans, where, twin=None, single=None, stats=FLOPS):
    """One solve_sparse_multi of `cols` on g; every column the twin's and the second handle's, and afterwards the flop
    counters those have after their single calls.  Returns (statuses, solutions)."""
    m = g.m
    sts, sols = g.solve_sparse_multi([c[0] for c in cols], [c[1] for c in cols], trans)
    assert sts == [K.OK] * len(cols), (where, sts)
    for other, name in ((twin, "oracle"), (single, "single")):
        if other is None:
            continue
        for j, (ir, xr) in enumerate(cols):
            same_column(m, sts[j], sols[j], U._ss(other, ir, xr, trans), (where, trans, name, j, len(ir)))
        for key in stats:
            assert g.stat(key) == other.stat(key), (where, trans, name, "stat", key, g.stat(key), other.stat(key))
    if single is not None and cols:
        assert g.stat(BRANCH) == single.stat(BRANCH), (where, trans, "branch", g.stat(BRANCH), single.stat(BRANCH))
    return sts, sols


def set_thres(thres, *objs):
    for x in objs:
        if x is not None:
            x.set_param(K.PARAM_SPARSE_THRES, thres)


def slot_bytes(m):
    return 48 * m + 64  # blu_hip_dbg_set_sparse_multi_ws_bytes


def between_solves_and_update(g, o, cols3, m, j, ai, ax, where):
    """One replacement of column j by (ai, ax) by hand, with a multi call of cols3 between the two solve_for_update calls
    and update (the twin: the single solves): the update and the solves that follow are the twin's."""
    U._same(U._sfu(g, [j], None, "T"), U._sfu(o, [j], None, "T"), (where, "btran"))
    a = U._sfu(g, ai, ax, "N")
    U._same(a, U._sfu(o, ai, ax, "N"), (where, "ftran"))
    xtbl = a[2][j]
    check_multi(g, cols3, "N", (where, "between"), twin=o)
    check_multi(g, cols3, "T", (where, "between"), twin=o)
    st = g.update(xtbl)
    assert st == o.update(xtbl), (where, "update", st)
    for key in (K.STAT_PIVOT_ERROR, K.STAT_NFORREST, K.STAT_R_NZ, K.STAT_NUPDATE, K.STAT_U_NZ, K.STAT_MAX_ETA):
        assert g.stat(key) == o.stat(key), (where, "stat", key, g.stat(key), o.stat(key))
    ir, xr = cols3[-1]
    for trans in "NT":
        U._same(U._ss(g, ir, xr, trans), U._ss(o, ir, xr, trans), (where, "solve_sparse after", trans))
    return st


def raw_call(blu, h, ptr, ir, xr, trans=b"N", nrhs=None, P=True, LP=True, st=True):
    """blu_hip_solve_sparse_multi itself: ptr / ir / xr are arrays (None = NULL); returns (rc, lhs_ptr, statuses), both
    pre-filled with 77"""
    FN = blu.lib().blu_hip_solve_sparse_multi
    FN.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char, C.c_void_p, C.c_void_p]
    ptr = np.ascontiguousarray(ptr, np.int64)
    n = len(ptr) - 1 if nrhs is None else nrhs
    N = max(len(ptr) - 1, 1)
    lp = np.full(N + 1, SENT, np.int64)
    s = np.full(N, SENT, np.int32)
    ir = None if ir is None else np.ascontiguousarray(ir, np.uint64)
    xr = None if xr is None else np.ascontiguousarray(xr, np.float64)
    rc = FN(h, n, ptr.ctypes.data if P else None, None if ir is None else ir.ctypes.data, None if xr is None else xr.ctypes.data, trans,
            lp.ctypes.data if LP else None, s.ctypes.data if st else None)
    return rc, lp, s


def raw_get(blu, h, total, IL=True, XL=True):
    FN = blu.lib().blu_hip_get_sparse_multi
    FN.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    il, xl = np.full(max(total, 1), SENT, np.int64), np.full(max(total, 1), float(SENT))
    rc = FN(h, il.ctypes.data if IL else None, xl.ctypes.data if XL else None)
    return rc, il[:total], xl[:total]


def refusals(blu, g, hnone, keys=FLOPS + (K.STAT_NUPDATE, BRANCH)):
    """Every refusal of the call as a whole, in the order of the header: lhs_ptr, status, the held result and the counters
    stay as they were."""
    MISS, INVARG, INVCALL = K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_ARGUMENT, K.ERROR_INVALID_CALL
    before = [g.stat(key) for key in keys]
    ptr, ir, xr = [0, 1, 2], [3, 4], [1.0, 2.0]

    def refused(code, h, *a, **kw):
        rc, lp, s = raw_call(blu, h, *a, **kw)
        assert rc == code and (lp == SENT).all() and (s == SENT).all(), (a, kw, rc, lp, s)

    refused(MISS, None, ptr, ir, xr)
    refused(INVCALL, hnone._h, ptr, ir, xr)
    refused(INVCALL, hnone._h, ptr, ir, xr, P=False)          # the factorization is checked before the pointers
    refused(MISS, g._h, ptr, ir, xr, P=False)
    refused(MISS, g._h, ptr, ir, xr, LP=False)
    refused(MISS, g._h, ptr, None, xr)
    refused(MISS, g._h, ptr, ir, None)
    refused(MISS, g._h, [2, 1, 3], None, xr)                  # the pointers are checked before the counts
    refused(INVARG, g._h, ptr, ir, xr, nrhs=-1)
    refused(INVARG, g._h, [0, 2, 1], ir, xr)
    refused(INVARG, g._h, [2, 1, 1], ir, xr)
    assert before == [g.stat(key) for key in keys], "a refused call touched the handle"
