"""Shared by the tests of the resident constraint matrix (blu_hip_set_matrix, _factorize_columns, _solve_for_update_column,
_tableau_row, _price): the summation order of the contract restated in plain Python and numpy float64, the comparison of
bits, the two matrices of the tests, and the drivers that run a handle through the new entries beside a twin handle driven
by the single entries -- equalities only."""
import numpy as np

from blu_amd import keys as K
from tests import util_maxvolume as MV

FLOPS = (K.STAT_L_FLOPS, K.STAT_U_FLOPS, K.STAT_R_FLOPS, K.STAT_UPDATE_COST)
LONG_LENGTHS = (0, 1, 2, 5, 63, 64, 65, 127, 128, 129, 200)


def at_dot(a_p, a_i, a_x, y, skip=None):
    """out[j] = column j of A dotted with y in the order of the contract: every product rounded once; n <= 64: s = +0.0 and
    s = s + t_q in storage order; n > 64: 64 partial sums over q = l, l + 64, ..., then p[l] = p[l] + p[l + w] for
    w = 32 .. 1.  skip[j] != 0: +0.0."""
    ncol = len(a_p) - 1
    y = np.asarray(y, np.float64)
    out = np.zeros(ncol)
    with np.errstate(all="ignore"):
        for j in range(ncol):
            if skip is not None and skip[j]:
                continue
            b, e = int(a_p[j]), int(a_p[j + 1])
            t = np.asarray(a_x[b:e], np.float64) * y[np.asarray(a_i[b:e], np.int64)]
            if e - b <= 64:
                s = np.float64(0.0)
                for v in t:
                    s = s + v
            else:
                p = np.zeros(64)
                for k in range(0, e - b, 64):
                    c = t[k:k + 64]
                    p[:len(c)] = p[:len(c)] + c
                for w in (32, 16, 8, 4, 2, 1):
                    p[:w] = p[:w] + p[w:2 * w]
                s = p[0]
            out[j] = s
    return out


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def m0():
    """(m, ncol, (a_p, a_i, a_x))"""
    return 12, 40, MV._problem(12, 40, 3)


def m1():
    """m = 200, ncol = 331 (no multiple of 64): the identity-like start columns of util_maxvolume._problem, then columns
    whose lengths cycle through LONG_LENGTHS -- both sides of the 64 threshold, of 128, and a full column -- with distinct
    random rows and values 3 N(0, 1)"""
    m, ncol = 200, 331
    rng = np.random.default_rng(20240607)
    a_p, a_i, a_x = [0], [], []
    for j in range(m):
        col = {j: 1.0}
        for i in rng.choice(m, int(rng.integers(1, 5)), replace=False):
            col[int(i)] = col.get(int(i), 0.0) + float(rng.standard_normal()) * 0.3
        a_i += list(col.keys())
        a_x += list(col.values())
        a_p.append(len(a_i))
    for j in range(m, ncol):
        n = LONG_LENGTHS[(j - m) % len(LONG_LENGTHS)]
        a_i += [int(i) for i in rng.choice(m, n, replace=False)]
        a_x += [3.0 * float(x) for x in rng.standard_normal(n)]
        a_p.append(len(a_i))
    return m, ncol, (np.array(a_p, np.uint64), np.array(a_i, np.uint64), np.array(a_x))


MATRICES = {"M0": m0, "M1": m1}


def gathered(a, basis):
    """the columns A[:, basis] as arrays of their own: (b_begin, b_end, b_i, b_x)"""
    a_p, a_i, a_x = a
    bb, be, bi, bx = [], [], [], []
    for j in basis:
        b, e = int(a_p[j]), int(a_p[j + 1])
        bb.append(len(bi))
        bi += [int(i) for i in a_i[b:e]]
        bx += [float(x) for x in a_x[b:e]]
        be.append(len(bi))
    return np.array(bb, np.uint64), np.array(be, np.uint64), np.array(bi, np.uint64), np.array(bx)


def column(a, j):
    b, e = int(a[0][j]), int(a[0][j + 1])
    return a[1][b:e], a[2][b:e]


def solution(h):
    return int(h.nzlhs), h.ilhs[:h.nzlhs].copy(), h.lhs.copy()


def same_solution(x, y):
    return x[0] == y[0] and np.array_equal(x[1], y[1]) and same_bits(x[2], y[2])


def same_handles(g, s, a, what, stats=MV.STATS):
    """statistics, then solve_sparse of three columns of A in both systems"""
    for key in stats:
        u, v = g.stat(key), s.stat(key)
        assert u == v, (what, "statistic", key, u, v)
    ncol = len(a[0]) - 1
    for j in (ncol - 1, ncol - 2, 0):
        ci, cx = column(a, j)
        if len(ci) == 0:
            ci, cx = column(a, 1)
        for tr in "NT":
            assert g.solve_sparse(ci, cx, tr) == s.solve_sparse(ci, cx, tr) == K.OK, (what, j, tr)
            assert same_solution(solution(g), solution(s)), (what, "solve_sparse", j, tr)


def pick_leaving(h):
    """first largest entry of the solution in pattern order (blu_amd.maxvolume): (imax, xtbl)"""
    xmax, xtbl, imax = 0.0, 0.0, 0
    for i in h.ilhs[:h.nzlhs]:
        if abs(h.lhs[i]) > xmax:
            xtbl = float(h.lhs[i])
            xmax = abs(xtbl)
            imax = int(i)
    return imax, xtbl


def update_pair(g, s, a, basis, isbasic, nupdates, what):
    """nupdates basis changes: g through solve_for_update_column + tableau_row(p, 1) + update, the twin s through the two
    single solve_for_update calls + update; every returned piece and the tableau row are compared on the way"""
    ncol = len(a[0]) - 1
    done = 0
    for j in range(ncol - 1, -1, -1):
        if done == nupdates:
            break
        ci, cx = column(a, j)
        if isbasic[j] or len(ci) == 0:
            continue
        assert g.solve_for_update_column(j) == s.solve_for_update(ci, cx, "N", True) == K.OK, (what, j)
        assert same_solution(solution(g), solution(s)), (what, "spike solve", j)
        p, xtbl = pick_leaving(g)
        if abs(xtbl) < 0.05:
            continue  # (a poor pivot: the pending spike is replaced by the next forward solve, in both handles)
        st, alpha = g.tableau_row(p, True, isbasic, want_solution=True)
        assert st == s.solve_for_update([p], None, "T", True) == K.OK, (what, p)
        assert same_solution(solution(g), solution(s)), (what, "row solve", p)
        assert same_bits(alpha, at_dot(a[0], a[1], a[2], s.lhs, isbasic)), (what, "alpha of the leaving row", p)
        assert g.update(xtbl) == s.update(xtbl) == K.OK, (what, "update", j, p)
        isbasic[basis[p]] = 0
        isbasic[j] = 1
        basis[p] = j
        done += 1
    assert done == nupdates, (what, done)
    same_handles(g, s, a, what)


def rows_of(m):
    return sorted({0, 1, m - 1, m // 2, m // 3})


def check_tableau_rows(g, a, m, skip, what, twin=None):
    """tableau_row(r, 0, skip) of five rows against a clone taken before each call: alpha = at_dot of the clone's y, the
    solution and the flop counters those of the clone's single solve_sparse([r], [1.0], 'T'); a twin makes the single
    solves that keep it level with g"""
    for r in rows_of(m):
        c = g.clone()
        assert c.solve_sparse([r], [1.0], "T") == K.OK
        want = at_dot(a[0], a[1], a[2], c.lhs, skip)
        st, alpha = g.tableau_row(r, False, skip, want_solution=True)
        assert st == K.OK, (what, r, st)
        assert same_bits(alpha, want), (what, "alpha", r, np.flatnonzero(alpha != want)[:5])
        if skip is not None:
            assert not np.any(alpha.view(np.uint64)[np.asarray(skip) != 0]), (what, "skipped entries are +0.0", r)
        assert same_solution(solution(g), solution(c)), (what, "solution", r)
        for key in FLOPS:
            assert g.stat(key) == c.stat(key), (what, "statistic", key, r)
        st, again = g.tableau_row(r, False, skip)  # (without the download of the solution)
        assert st == K.OK and same_bits(again, want), (what, "alpha without the solution", r)
        if twin is not None:
            assert twin.solve_sparse([r], [1.0], "T") == twin.solve_sparse([r], [1.0], "T") == K.OK
        c.close()


def price_vectors(m, seed=5):
    """a random y; one with -0.0 and zeros among its entries"""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(m)
    z = rng.standard_normal(m)
    z[::3] = 0.0
    z[1::5] = -0.0
    return y, z


def check_price(g, a, m, isbasic, what):
    ncol = len(a[0]) - 1
    for y in price_vectors(m):
        for skip in (None, [1] * ncol, isbasic):
            assert same_bits(g.price(y, skip), at_dot(a[0], a[1], a[2], y, skip)), (what, "price", skip is None)
    if m:
        y = price_vectors(m)[0].copy()
        y[m // 2] = np.nan
        assert np.array_equal(g.price(y), at_dot(a[0], a[1], a[2], y), equal_nan=True), (what, "price with a NaN")
