"""Shared helpers of the parity tests."""
import glob
import os

import numpy as np
import scipy.sparse as sp

from blu_amd import keys as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT_KEYS = ("rowperm", "colperm", "l_colptr", "l_rowidx", "u_colptr", "u_rowidx")
VAL_KEYS = ("l_value", "u_value")
COUNTERS = ("RANK", "MATRIX_NZ", "BUMP_SIZE", "BUMP_NZ", "L_NZ", "U_NZ", "NSEARCH_PIVOT", "FACTOR_FLOPS", "RANKDEF")
RTOL = 1e-12  # north_star: L/U numeric values within 1e-12 relative


def golden_files():
    # factorize fixtures; solve_sparse.npz holds solve vectors and has its own tests
    return sorted(p for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if not os.path.basename(p).startswith("solve_"))


def csc(colptr, rowidx, values, m):
    return sp.csc_matrix((np.asarray(values, float), np.asarray(rowidx, np.int64), np.asarray(colptr, np.int64)), shape=(m, m))


def check_factors(colptr, rowidx, values, f, rank=None, tol=1e-10):
    """B[rowperm, colperm] == L*U (dependent columns replaced by unit columns), structure checks."""
    m = len(colptr) - 1
    B = csc(colptr, rowidx, values, m).tocsc()
    p, q = f["rowperm"], f["colperm"]
    assert sorted(p.tolist()) == list(range(m)) and sorted(q.tolist()) == list(range(m))
    L = csc(f["l_colptr"], f["l_rowidx"], f["l_value"], m)
    U = csc(f["u_colptr"], f["u_rowidx"], f["u_value"], m)
    # L unit lower with the diagonal first in each column, rows sorted; U upper with the diagonal last
    for k in range(m):
        a, b = f["l_colptr"][k], f["l_colptr"][k + 1]
        assert f["l_rowidx"][a] == k and f["l_value"][a] == 1.0
        assert np.all(np.diff(f["l_rowidx"][a:b]) > 0)
        a, b = f["u_colptr"][k], f["u_colptr"][k + 1]
        assert f["u_rowidx"][b - 1] == k
        assert np.all(np.diff(f["u_rowidx"][a:b]) > 0)
    PBQ = B[p, :][:, q].toarray() if m <= 4000 else None
    if rank is not None and rank < m and PBQ is not None:
        for k in range(rank, m):  # columns colperm[rank..] replaced by unit columns e_{rowperm[k]}
            PBQ[:, k] = 0.0
            PBQ[k, k] = 1.0
    if PBQ is not None:
        err = np.abs((L @ U).toarray() - PBQ).max()
        scale = max(1.0, np.abs(PBQ).max())
        assert err <= tol * scale * max(1.0, np.abs(U.toarray()).max()), err
    else:
        R = (L @ U) - B[p, :][:, q]
        assert abs(R).max() <= tol * max(1.0, abs(U).max())


def assert_same_factors(got, want, rtol=RTOL):
    """Bit-exact integer arrays; values within rtol relative (elementwise, with an absolute floor of rtol*max|.|)."""
    for k in INT_KEYS:
        assert np.array_equal(np.asarray(got[k], np.int64), np.asarray(want[k], np.int64)), k
    for k in VAL_KEYS:
        g, w = np.asarray(got[k], float), np.asarray(want[k], float)
        assert g.shape == w.shape, k
        assert np.all(np.abs(g - w) <= rtol * np.maximum(np.abs(w), 1e-300)), (k, np.abs(g - w).max())


def counters(stat):
    return {c: int(stat(getattr(K, "STAT_" + c))) for c in COUNTERS}


def oracle_factorize(orc, cp, ri, v, params=None, cap=None, allow_d3=False):
    """Factorize with the CPU oracle as the REFERENCE restates it (faithful i32 cancellation mask, D3).

    The faithful restatement has no defined result when a cancellation lands at pivot-column position
    >= 31 (the reference corrupts its row file there), so a first run with the 64-bit mask counts such
    events (d3_hits).  d3_hits == 0: the faithful oracle is run and returned -- the comparison is with
    the reference's own semantics.  d3_hits > 0: only callers that say allow_d3=True get the 64-bit-mask
    run back (the HIP path documents the same deviation); everyone else fails."""
    m = len(cp) - 1
    cap = cap if cap else 32 * len(ri) + 1024

    def run(fix):
        def setup(o):
            o.set_fix_d3(fix)
            for k, val in (params or {}).items():
                o.set_param(k, val)
        # (factorize_roomy: a capacity too small for the bump would send the faithful restatement into the
        # reference's endless Reallocate loop, defect D5; it is raised until W never grows inside the bump)
        return orc.OracleBLU.factorize_roomy(m, cap, cp[:-1], cp[1:], ri, v, setup)

    o, st = run(True)
    if o.d3_hits() == 0:
        o, st = run(False)
        assert o.d3_hits() == 0
        return o, st
    assert allow_d3, "reference defect D3 would be hit (%d times): choose another matrix or pass allow_d3" % o.d3_hits()
    return o, st


def basis_with_long_row(m, rowlen, seed, singular=False):
    """gen_lp_basis(m, 6, 8, 0.5, seed, 0.3) with row m // 2 filled to exactly `rowlen` entries in random columns,
    |values| = U(0.1, 1) * 10^U(-6, 2) with random signs, so that this row has the largest sum of |a|.
    singular: three columns holding an entry of that row are scaled by 1e-17, so rank < m and the long row has entries
    in columns that do not become pivotal.  Returns (colptr, rowidx, values) with the rows of a column ascending."""
    from oracle import orc
    cp, ri, v = orc.gen_lp_basis(m, 6, 8, 0.5, seed, 0.3)
    r = m // 2
    rng = np.random.default_rng(7919 * seed + rowlen)
    cols = [dict(zip(ri[cp[j]:cp[j + 1]].astype(np.int64).tolist(), v[cp[j]:cp[j + 1]].tolist())) for j in range(m)]
    have = [j for j in range(m) if r in cols[j]]
    assert len(have) <= rowlen, (len(have), rowlen)
    free = np.array([j for j in range(m) if r not in cols[j]], np.int64)
    for j in rng.choice(free, rowlen - len(have), replace=False):
        cols[int(j)][r] = float(rng.choice((-1.0, 1.0)) * rng.uniform(0.1, 1.0) * 10.0 ** rng.uniform(-6.0, 2.0))
    if singular:
        inrow = [j for j in range(m) if r in cols[j]]
        for j in rng.choice(inrow, 3, replace=False):
            cols[int(j)] = {i: x * 1e-17 for i, x in cols[int(j)].items()}
    ncp, nri, nv = [0], [], []
    for j in range(m):
        for i in sorted(cols[j]):
            nri.append(i)
            nv.append(cols[j][i])
        ncp.append(len(nri))
    return np.array(ncp, np.uint64), np.array(nri, np.uint64), np.array(nv)


def row_sums_two_orders(cp, ri, v, row, f, rank):
    """Sum of |a| over the entries of `row` in pivotal columns (colperm[0..rank)), plus 1 if the row itself is not pivotal
    (the unit column that replaces a dependent one), added sequentially in two orders: ascending column index (the order
    in which the row is stored) and ascending pivot position of the column (the reference's order, matrix_norm.rs).
    Returns (storage_order_sum, pivot_order_sum)."""
    m = len(cp) - 1
    cols = np.repeat(np.arange(m), np.diff(cp.astype(np.int64)))
    mask = ri.astype(np.int64) == row
    c, a = cols[mask], np.asarray(v)[mask]
    qinv = np.empty(m, np.int64)
    qinv[np.asarray(f["colperm"], np.int64)] = np.arange(m)
    pinv = np.empty(m, np.int64)
    pinv[np.asarray(f["rowperm"], np.int64)] = np.arange(m)
    keep = qinv[c] < rank
    c, a = c[keep], a[keep]
    sums = []
    for order in (np.argsort(c, kind="stable"), np.argsort(qinv[c], kind="stable")):
        s = 0.0
        for x in a[order]:
            s += abs(float(x))
        if pinv[row] >= rank:
            s += 1.0
        sums.append(s)
    return sums[0], sums[1]


def long_row_case(orc, m, rowlen, seed, singular=False, tries=60):
    """The first seed from `seed` on whose basis_with_long_row the two summation orders of row_sums_two_orders give
    different sums, that row has the largest sum of |a|, and the faithful oracle does not meet reference defect D3:
    a basis on which the statistics of a kernel that summed the long row in storage order would differ from the
    reference.  Returns (seed, (cp, ri, v), oracle handle, oracle status)."""
    for s in range(seed, seed + tries):
        cp, ri, v = basis_with_long_row(m, rowlen, s, singular)
        o, so = oracle_factorize(orc, cp, ri, v, allow_d3=True)
        if o.d3_hits() or so not in (K.OK, K.WARNING_SINGULAR_MATRIX):
            continue
        rank = int(o.stat(K.STAT_RANK))
        assert (rank < m) == singular, (rank, m)
        f = o.get_factors()
        a, b = row_sums_two_orders(cp, ri, v, m // 2, f, rank)
        rows = np.bincount(ri.astype(np.int64), weights=np.abs(v), minlength=m)
        if a != b and b == o.stat(K.STAT_INFNORM) and np.argmax(rows) == m // 2:
            return s, (cp, ri, v), o, so
    raise AssertionError("no seed in [%d, %d) separates the two orders of row %d (m %d, %d entries)" % (seed, seed + tries, m // 2, m, rowlen))


def gathered_basis(m, seed, k=6, bw=8, tri_frac=0.5, offscale=0.3, n_empty=0, twice=False, end_last=False, extra=None):
    """B as a simplex code passes it: columns gathered from a constraint matrix A by b_begin = A_begin[basis],
    b_end = A_end[basis], with b_i / b_x being A's whole arrays (include/blu_hip.h: blu_hip_factorize; the reference's
    singletons.rs:119-198 reads B only through the [b_begin[j], b_end[j]) ranges).

    A holds the gen_lp_basis(m, k, bw, tri_frac, seed, offscale) columns plus `extra` (default m) random columns of 1-5
    entries, in shuffled storage order, the rows of every column shuffled.  Between two columns lie 0-3 poison entries:
    row index >= m and a NaN value, so a kernel that reads outside a range returns ERROR_INVALID_ARGUMENT or a NaN
    statistic.  The basis is the gen_lp_basis columns in a random order, except:
      n_empty   that many basis columns are replaced by empty columns of A (begin == end; the basis is singular),
      twice     one basis column is listed a second time in place of another: two columns share storage (singular),
      end_last  the column stored last in A is a basis column and nothing follows it (b_end[j] == len(b_i)).
    Returns (b_begin, b_end, b_i, b_x): uint64, uint64, uint64, float64."""
    from oracle import orc
    cp, ri, v = orc.gen_lp_basis(m, k, bw, tri_frac, seed, offscale)
    rng = np.random.default_rng(104729 * seed + m)
    cols = [(ri[cp[j]:cp[j + 1]].astype(np.int64), v[cp[j]:cp[j + 1]].copy()) for j in range(m)]
    for _ in range(m if extra is None else extra):
        n = int(rng.integers(1, 6))
        cols.append((rng.choice(m, n, replace=False).astype(np.int64), rng.standard_normal(n)))
    for _ in range(n_empty):
        cols.append((np.zeros(0, np.int64), np.zeros(0)))
    order = rng.permutation(len(cols))  # storage position -> column of A
    if end_last:  # a basis column goes last
        last = int(np.flatnonzero(order < m)[-1])
        order[last], order[-1] = order[-1], order[last]
    a_begin = np.zeros(len(cols), np.uint64)
    a_end = np.zeros(len(cols), np.uint64)
    b_i, b_x = [], []
    for pos, c in enumerate(order):
        gap = int(rng.integers(0, 4))
        b_i += (m + rng.integers(0, 3 * m + 1, gap)).tolist()
        b_x += [np.nan] * gap
        idx, val = cols[int(c)]
        perm = rng.permutation(len(idx))
        a_begin[c] = len(b_i)
        b_i += idx[perm].tolist()
        b_x += val[perm].tolist()
        a_end[c] = len(b_i)
    if not end_last:  # poison after the last column too
        b_i += [m, 2 * m + 7]
        b_x += [np.nan, np.nan]
    basis = rng.permutation(m)  # basis position -> column of A
    if n_empty:
        for p, c in zip(rng.choice(m, n_empty, replace=False), range(len(cols) - n_empty, len(cols))):
            basis[p] = c
    if twice:
        p, q = rng.choice(m, 2, replace=False)
        basis[q] = basis[p]
    b_i, b_x = np.array(b_i, np.uint64), np.array(b_x, np.float64)
    assert not end_last or a_end[order[-1]] == len(b_i)
    return a_begin[basis].copy(), a_end[basis].copy(), b_i, b_x


def gathered_matrix(b_begin, b_end, b_i, b_x, m):
    """scipy CSC matrix assembled from the [b_begin[j], b_end[j]) ranges alone (nothing else of b_i / b_x is read)."""
    idx, val, ptr = [], [], [0]
    for j in range(m):
        a, b = int(b_begin[j]), int(b_end[j])
        idx.append(np.asarray(b_i[a:b], np.int64))
        val.append(np.asarray(b_x[a:b], np.float64))
        ptr.append(ptr[-1] + b - a)
    B = sp.csc_matrix((np.concatenate(val), np.concatenate(idx), np.array(ptr, np.int64)), shape=(m, m))
    B.sort_indices()
    return B


def gathered_csc(b_begin, b_end, b_i, b_x, m):
    """(colptr, rowidx, values) of gathered_matrix, the form util.check_factors takes."""
    B = gathered_matrix(b_begin, b_end, b_i, b_x, m)
    return B.indptr.astype(np.uint64), B.indices.astype(np.uint64), B.data.copy()


# Getters assert_same_getters leaves out, each for its reason.
GETTERS_NOT_COMPARED = {
    K.STAT_TIME_FACTORIZE: "wall-clock time",
    K.STAT_TIME_SINGLETONS: "device time",
    K.STAT_TIME_SEARCH_PIVOT: "device time",
    K.STAT_TIME_ELIM_PIVOT: "device time",
    K.STAT_L_MEM: "storage size: the device sizes its arenas its own way",
    K.STAT_U_MEM: "storage size",
    K.STAT_W_MEM: "storage size",
    K.STAT_DEV_TIME_PIVOT_LOOP: "device diagnostic without a reference counterpart",
    K.STAT_DEV_TIME_TOTAL: "device diagnostic",
    K.STAT_DEV_RELAUNCHES: "device diagnostic",
    K.STAT_NEXPAND: "counts line moves inside the file, so depends on the memory layout (include/blu_hip.h)",
    K.STAT_NGARBAGE: "counts compressions of the file, so depends on the memory layout (include/blu_hip.h)",
}
# Getters blu_hip_set_skip_stats turns to 0 by contract (include/blu_hip.h: the statistics tail, factorize.rs:121-147)
SKIPPED_STATS = (K.STAT_CONDEST_L, K.STAT_CONDEST_U, K.STAT_NORM_L, K.STAT_NORM_U, K.STAT_NORMEST_L_INV, K.STAT_NORMEST_U_INV,
                 K.STAT_ONENORM, K.STAT_INFNORM, K.STAT_RESIDUAL_TEST)


def getter_keys():
    return sorted((name, val) for name, val in vars(K).items() if name.startswith("STAT_"))


# Getters that count over the whole life of a handle (lu.rs:79-81): a handle with a past and a fresh one differ in them
HISTORY_GETTERS = (K.STAT_NFACTORIZE, K.STAT_NSYMPERM_TOTAL, K.STAT_NFORREST_TOTAL, K.STAT_DEV_NUNSYMPERM_TOTAL)


def assert_same_getters(h, o, where, skip_stats=False, history=True):
    """Every getter of blu_amd/keys.py but those of GETTERS_NOT_COMPARED equal on the device handle h and on o, the oracle
    or another device handle (NaN equal to NaN).  skip_stats: h has blu_hip_set_skip_stats on, so SKIPPED_STATS must read
    0 on it instead.  history=False: o is a fresh handle, so HISTORY_GETTERS are left out."""
    bad = []
    for name, key in getter_keys():
        if key in GETTERS_NOT_COMPARED or (not history and key in HISTORY_GETTERS):
            continue
        a = h.stat(key)
        b = 0.0 if skip_stats and key in SKIPPED_STATS else o.stat(key)
        if not (a == b or (np.isnan(a) and np.isnan(b))):
            bad.append((name, a, b))
    assert not bad, (where, bad)


def status_of(call):
    """The status of a BLU / OracleBLU call: what it returns (a status, or a tuple that starts with one), K.OK for a
    result that is not a status, or the status of the error it raised (blu_amd.BluError; the oracle's RuntimeError
    "... status <n>")."""
    from blu_amd import BluError
    try:
        r = call()
    except BluError as e:
        return e.status
    except RuntimeError as e:
        return int(str(e).split()[-1])
    if isinstance(r, tuple):
        return r[0]
    return r if isinstance(r, int) else K.OK


def spoil(b_begin, b_end, b_i, b_x, kind, seed=0):
    """A copy of a gathered B that factorize must refuse with ERROR_INVALID_ARGUMENT (singletons.rs:119-201):
    kind "index": one row index inside a column's range set to >= m; "order": b_end[j] < b_begin[j] for one column."""
    rng = np.random.default_rng(seed)
    bb, be, bi, bx = b_begin.copy(), b_end.copy(), b_i.copy(), b_x.copy()
    m = len(bb)
    j = int(rng.choice(np.flatnonzero(be > bb)))
    if kind == "index":
        bi[int(rng.integers(int(bb[j]), int(be[j])))] = m + int(rng.integers(0, 5))
    else:
        bb[j], be[j] = be[j], bb[j]
    return bb, be, bi, bx
