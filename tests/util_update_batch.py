"""Driver of the batched update tests: many bases kept in lock step, each round a batched transposed solve_for_update, a
batched forward one and a batched update (blu_amd.solve_for_update_batch / update_batch), every member compared with a
twin of its own that is driven by the single calls -- the CPU oracle, or a second handle of the library (a member without
a twin is checked by its statuses and backward errors alone).  The columns come from tests/util_update.py, one random
stream per member; members whose pivot |xtbl| is small sit the round's update out, so the set of members changes from
call to call."""
import numpy as np

from blu_amd import keys as K
from tests import util_update as U

# the statistics tests/util_update.py::run_updates compares after every update ...
STATS = (K.STAT_NFORREST, K.STAT_NUPDATE, K.STAT_R_NZ, K.STAT_PIVOT_ERROR, K.STAT_NSYMPERM_TOTAL, K.STAT_DEV_NUNSYMPERM_TOTAL,
         K.STAT_MIN_PIVOT, K.STAT_MAX_PIVOT, K.STAT_MAX_ETA, K.STAT_U_NZ)
# ... and, for two handles of the library (one driven by the batch entries, one by the single calls), the lifetime total
# and the flop counters on top
STATS_LIBRARY = STATS + (K.STAT_NFORREST_TOTAL, K.STAT_L_FLOPS, K.STAT_U_FLOPS, K.STAT_R_FLOPS, K.STAT_UPDATE_COST)
KINDS = (K.STAT_NFORREST_TOTAL, K.STAT_NSYMPERM_TOTAL, K.STAT_DEV_NUNSYMPERM_TOTAL)


def bidiagonal_cols(m, diag=2.0):
    """B = diag * I + superdiagonal of ones (tests/test_gpu_update.py::test_permutation_updates_on_a_bidiagonal_basis)"""
    return [(np.array([j] + ([j - 1] if j else []), np.int64), np.array([diag] + ([1.0] if j else []))) for j in range(m)]


# its two hand-predictable replacements: an UNsymmetric permutation update, then a SYMMETRIC one
BIDIAGONAL_SCRIPT = [(2, np.array([3], np.int64), np.array([3.0])), (5, np.array([5, 1], np.int64), np.array([7.0, 1.0]))]


def pair_rows(g):
    f = g.get_factors()
    pr = np.zeros(g.m, np.int64)
    pr[f["colperm"]] = f["rowperm"]
    return pr


def solution(h):
    return h.ilhs[:h.nzlhs].copy(), h.lhs.copy()


class Member:
    def __init__(self, h, twin, cols, seed, pair_row=None, script=()):
        self.h, self.twin, self.cols, self.m = h, twin, cols, h.m
        self.rng = np.random.default_rng(seed)
        self.pair_row = pair_row
        self.script = list(script)
        self.B = U.matrix_of(cols, self.m)
        self.done = self.singular = self.skipped = 0
        self.maxed = False
        self.max_residual = self.max_pivot_error = 0.0


def _twin_sfu(t, irhs, xrhs, trans):
    return U._sfu(t, irhs, xrhs, trans)


def lockstep_round(blu, members, stats=STATS, tol_xtbl=1e-3, where=""):
    """One round over `members` (those that already met ERROR_MAXIMUM_UPDATES take part in the transposed call only and
    must meet it again); an update may answer OK or ERROR_SINGULAR_UPDATE, every other status fails.  Returns the
    statuses of the three calls."""
    picks = []
    for M in members:
        if M.script:
            picks.append(M.script.pop(0))
        else:
            j = int(M.rng.integers(0, M.m))
            picks.append((j,) + tuple(U.new_column(M.rng, M.cols, M.m, j, M.pair_row)))
    # ---- transposed solves: every member
    st_t = blu.solve_for_update_batch([M.h for M in members], [[p[0]] for p in picks], None, "T")
    go = []
    for k, (M, (j, ai, ax), st) in enumerate(zip(members, picks, st_t)):
        a = (st,) + (solution(M.h) if st == K.OK else (None, None))
        if M.twin is not None:
            U._same(a, _twin_sfu(M.twin, [j], None, "T"), (where, "T", k))
        if st == K.ERROR_MAXIMUM_UPDATES:
            M.maxed = True
            continue
        assert st == K.OK and not M.maxed, (where, "T", k, st)
        ej = np.zeros(M.m)
        ej[j] = 1.0
        M.max_residual = max(M.max_residual, U.backward_error(M.B.T, a[2], ej))
        assert np.array_equal(np.sort(a[1]), np.flatnonzero(a[2])), (where, "pattern T", k)
        go.append(k)
    # ---- forward solves: the members that were prepared
    st_n = blu.solve_for_update_batch([members[k].h for k in go], [picks[k][1] for k in go], [picks[k][2] for k in go], "N")
    upd, xtbl = [], []
    for k, st in zip(go, st_n):
        M, (j, ai, ax) = members[k], picks[k]
        a = (st,) + (solution(M.h) if st == K.OK else (None, None))
        if M.twin is not None:
            U._same(a, _twin_sfu(M.twin, ai, ax, "N"), (where, "N", k))
        assert st == K.OK, (where, "N", k, st)
        rhs = np.zeros(M.m)
        rhs[ai] = ax
        M.max_residual = max(M.max_residual, U.backward_error(M.B, a[2], rhs))
        assert np.array_equal(np.sort(a[1]), np.flatnonzero(a[2])), (where, "pattern N", k)
        if abs(a[2][j]) < tol_xtbl:
            M.skipped += 1
            continue
        upd.append(k)
        xtbl.append(a[2][j])
    # ---- updates: the members with a usable pivot
    st_u = blu.update_batch([members[k].h for k in upd], xtbl)
    for k, x, st in zip(upd, xtbl, st_u):
        M, (j, ai, ax) = members[k], picks[k]
        if M.twin is not None:
            assert M.twin.update(x) == st, (where, "update status", k, st)
            for key in stats:
                assert M.h.stat(key) == M.twin.stat(key), (where, "stat", key, k, M.h.stat(key), M.twin.stat(key))
        if st == K.ERROR_SINGULAR_UPDATE:
            M.singular += 1
            continue
        assert st == K.OK, (where, "update", k, st)
        M.done += 1
        M.max_pivot_error = max(M.max_pivot_error, M.h.stat(K.STAT_PIVOT_ERROR))
        M.cols[j] = (ai, ax)
        M.B = U.matrix_of(M.cols, M.m)
    return st_t, st_n, st_u


def dense_after(blu, members, seed, where=""):
    """solve_dense_batch on the updated factorizations, both systems: the twins' bits, rounding-level backward errors"""
    rng = np.random.default_rng(seed)
    for trans in "NT":
        rhs = [rng.standard_normal(M.m) for M in members]
        sols, st = blu.solve_dense_batch([M.h for M in members], rhs, trans)
        assert st == [K.OK] * len(members), (where, st)
        for k, (M, x, b) in enumerate(zip(members, sols, rhs)):
            if M.twin is not None:
                assert np.array_equal(x, M.twin.solve_dense(b, trans)), (where, "solve_dense", trans, k)
            M.max_residual = max(M.max_residual, U.backward_error(M.B if trans == "N" else M.B.T, x, b))


def kinds(members, of=lambda M: M.h):
    return np.array([[of(M).stat(key) for key in KINDS] for M in members]).sum(axis=0)
