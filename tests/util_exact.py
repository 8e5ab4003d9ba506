"""Integer-valued bases, on which the threshold tests of the pivot search are decided at equality and elimination cancels
to exactly 0.0, and the checks that need no oracle: on the totally unimodular (TU) families every pivot is +-1, every
intermediate value an integer and IEEE double arithmetic exact, so L*U, the rank and every solve are checked in int64.

Plain numpy, deterministic by seed.  Every family returns (colptr, rowidx, values) as uint64 / uint64 / float64, like
oracle.gen_lp_basis, after a random row and a random column permutation; the interval families also return what the
exact checks and the update schedule need (IntervalRows, the edge list).

    tree_interval_basis     nonsingular, TU: the intervals form a spanning tree of the nodes 0..m
    random_interval_matrix  TU, exactly singular: rank = (m + 1) - components of the graph of its intervals
    small_integer_basis     sparse, entries from {+-1, +-2, 0.5}: ties and cancellations, arithmetic not exact (parity only)
    dense_integer_matrix    dense, entries from {+-1, +-2}, diagonal +-3 (parity only)
    with_stored_zeros       a basis with explicit 0.0 entries added
"""
import numpy as np

from blu_amd import keys as K
from tests import util

FSTATS = ("CONDEST_L", "CONDEST_U", "NORM_L", "NORM_U", "NORMEST_L_INV", "NORMEST_U_INV", "ONENORM", "INFNORM", "RESIDUAL_TEST")
PATHS = ("singleton_row", "singleton_col", "doubleton_col", "small", "any", "empty_col")  # statistics 51..56


# ---- generators -------------------------------------------------------------------------------------------------------
class IntervalRows:
    """The rows of an interval matrix over the nodes 0..m: row r (between node r and node r + 1) has the sign rowsign[r] and
    is stored as row rowpos[r].  column(a, b, sign) is the column of the interval (a, b): rows a..b-1, values
    sign * rowsign."""

    def __init__(self, m, rng):
        self.m = m
        self.rowsign = rng.choice((-1.0, 1.0), m)
        self.rowpos = rng.permutation(m).astype(np.int64)

    def column(self, a, b, sign):
        r = np.arange(a, b)
        return self.rowpos[r].copy(), sign * self.rowsign[r]


def _csc(cols):
    cp = np.zeros(len(cols) + 1, np.uint64)
    cp[1:] = np.cumsum([len(i) for i, _ in cols])
    return cp, np.concatenate([i for i, _ in cols]).astype(np.uint64), np.concatenate([x for _, x in cols]).astype(np.float64)


def _find(parent, a):
    while parent[a] != a:
        parent[a] = parent[parent[a]]
        a = parent[a]
    return a


def tree_interval_basis(m, span, seed):
    """Nodes 0..m; edges (a, a + d), d uniform in 1..span, accepted while a and a + d are unconnected, until m edges form
    a spanning tree.  Column k holds rows a..a+d-1, all with one random sign; every row then gets a random sign; random row
    and column permutations.  Returns (colptr, rowidx, values, rows, edges): edges[k] = (a, b, sign) of column k."""
    rng = np.random.default_rng(seed)
    parent = list(range(m + 1))
    edges = []
    while len(edges) < m:
        d = int(rng.integers(1, span + 1))
        a = int(rng.integers(0, m + 1 - d))
        ra, rb = _find(parent, a), _find(parent, a + d)
        if ra != rb:
            parent[ra] = rb
            edges.append((a, a + d, float(rng.choice((-1.0, 1.0)))))
    rows = IntervalRows(m, rng)
    edges = [edges[k] for k in rng.permutation(m)]
    return _csc([rows.column(*e) for e in edges]) + (rows, edges)


def random_interval_matrix(m, maxlen, seed):
    """m random intervals (a, a + d), d uniform in 1..maxlen, with random column and row signs and no tree condition:
    exactly singular in general.  Returns (colptr, rowidx, values, rows, edges)."""
    rng = np.random.default_rng(seed)
    edges = []
    for _ in range(m):
        d = int(rng.integers(1, maxlen + 1))
        a = int(rng.integers(0, m + 1 - d))
        edges.append((a, a + d, float(rng.choice((-1.0, 1.0)))))
    rows = IntervalRows(m, rng)
    edges = [edges[k] for k in rng.permutation(m)]
    return _csc([rows.column(*e) for e in edges]) + (rows, edges)


def components(m, edges):
    """Component label of each node 0..m in the graph of the edges (a, b, ...)."""
    parent = list(range(m + 1))
    for e in edges:
        ra, rb = _find(parent, e[0]), _find(parent, e[1])
        if ra != rb:
            parent[ra] = rb
    return np.array([_find(parent, a) for a in range(m + 1)], np.int64)


def interval_rank(m, edges):
    """Exact rank of the interval matrix of the edges: (m + 1) - components (the columns are the edge vectors of a graph
    on m + 1 nodes written in the basis of the path 0 - 1 - ... - m)."""
    return (m + 1) - len(set(components(m, edges).tolist()))


def _permuted(cols, m, rng):
    rowpos = rng.permutation(m).astype(np.int64)
    return _csc([(rowpos[cols[j][0]], cols[j][1]) for j in rng.permutation(m)])


def small_integer_basis(m, k, seed):
    """1..k entries per column in random rows, drawn from {+-1, +-2, 0.5}, plus a diagonal entry from {+-1, 2}."""
    rng = np.random.default_rng(seed)
    cols = []
    for j in range(m):
        n = int(rng.integers(1, k + 1))
        idx = rng.choice(m - 1, n, replace=False)
        idx = np.where(idx >= j, idx + 1, idx)  # not the diagonal
        val = rng.choice((1.0, -1.0, 2.0, -2.0, 0.5), n)
        cols.append((np.concatenate(([j], idx)).astype(np.int64), np.concatenate(([rng.choice((1.0, -1.0, 2.0))], val))))
    return _permuted(cols, m, rng)


def dense_integer_matrix(m, seed):
    """Every entry from {+-1, +-2}, the diagonal +-3."""
    rng = np.random.default_rng(seed)
    A = rng.choice((1.0, -1.0, 2.0, -2.0), (m, m))
    A[np.arange(m), np.arange(m)] = rng.choice((3.0, -3.0), m)
    return _permuted([(np.arange(m), A[:, j].copy()) for j in range(m)], m, rng)


def with_stored_zeros(basis, every, seed):
    """A stored 0.0 in a row the column lacks, added at a random place of every `every`-th column."""
    cp, ri, v = basis[:3]
    m = len(cp) - 1
    rng = np.random.default_rng(seed)
    cols = []
    for j in range(m):
        idx, val = ri[int(cp[j]):int(cp[j + 1])].astype(np.int64), v[int(cp[j]):int(cp[j + 1])]
        if j % every == 0 and len(idx) < m:
            free = np.setdiff1d(np.arange(m), idx)
            at = int(rng.integers(0, len(idx) + 1))
            idx, val = np.insert(idx, at, int(rng.choice(free))), np.insert(val, at, 0.0)
        cols.append((idx, val))
    return _csc(cols)


# ---- the committed cases ----------------------------------------------------------------------------------------------
TREE_SHAPES = ((64, 6), (96, 8), (200, 10), (300, 40), (300, 80))
INTERVAL_SHAPES = ((64, 5), (96, 6), (120, 6), (300, 20))
SMALLINT_SHAPES = ((120, 4), (300, 8))
DENSE_SHAPES = (100, 150)
UPDATE_SHAPES = ((64, 6), (120, 8), (200, 30))
SEEDS = {"tree": 1, "interval": 2, "smallint": 3, "dense": 4, "zeros": 5}
# of the update schedule: 150 steps at m = 64 meet ERROR_MAXIMUM_UPDATES (m Forrest-Tomlin updates since the last
# factorization) for about every second seed; with this one the oracle counts 45 / 62 / 80 Forrest-Tomlin updates at
# m = 64 / 120 / 200, and 126 replacements applied and 24 exactly singular ones at every shape
SCHEDULE_SEED = 12
_cache = {}


def case(name):
    """A committed input by name: "tree-64-6", "interval-64-5", "smallint-120-4", "dense-100", "zeros" (tree (96, 8) with a
    stored zero in every third column).  Returns the generator's tuple; [:3] is (colptr, rowidx, values).  Computed once."""
    if name not in _cache:
        kind, *shape = name.split("-")
        shape = [int(s) for s in shape]
        if kind == "tree":
            _cache[name] = tree_interval_basis(*shape, SEEDS["tree"])
        elif kind == "interval":
            _cache[name] = random_interval_matrix(*shape, SEEDS["interval"])
        elif kind == "smallint":
            _cache[name] = small_integer_basis(*shape, SEEDS["smallint"])
        elif kind == "dense":
            _cache[name] = dense_integer_matrix(*shape, SEEDS["dense"])
        elif kind == "zeros":
            _cache[name] = with_stored_zeros(case("tree-96-8"), 3, SEEDS["zeros"])
        else:
            raise KeyError(name)
    return _cache[name]


TREES = tuple("tree-%d-%d" % s for s in TREE_SHAPES)
INTERVALS = tuple("interval-%d-%d" % s for s in INTERVAL_SHAPES)
SMALLINTS = tuple("smallint-%d-%d" % s for s in SMALLINT_SHAPES)
DENSES = tuple("dense-%d" % s for s in DENSE_SHAPES)
ALL_CASES = TREES + INTERVALS + SMALLINTS + DENSES + ("zeros",)
EMU_CASES = ("tree-64-6", "tree-96-8", "interval-64-5", "smallint-120-4", "dense-100", "zeros")

TWO_M40 = 2.0 ** -40
# parameters that put the threshold tests of the search at equality on entries that are all +-1 (or +-1, +-2, 0.5)
EQUALITY_PARAMS = (
    {K.PARAM_RELTOL: 1.0}, {K.PARAM_RELTOL: 0.5}, {K.PARAM_NZBIAS: -1, K.PARAM_SEARCH_ROWS: 1}, {K.PARAM_MAXSEARCH: 1},
)


def param_id(p):
    return ",".join("%d=%g" % kv for kv in p.items())


# ---- bitwise comparison with the oracle -------------------------------------------------------------------------------
def oracle_run(orc, cp, ri, v, params=None):
    """The oracle with the 64-bit cancellation mask (what the device keeps) -> (handle, status)."""
    def setup(o):
        o.set_fix_d3(True)
        for key, val in (params or {}).items():
            o.set_param(key, val)
    return orc.OracleBLU.factorize_roomy(len(cp) - 1, 64 * len(ri) + 1024, cp[:-1], cp[1:], ri, v, setup)


def assert_bitwise(g, o, sg, so, where):
    """Status, the six integer arrays, L and U values by bit pattern (the sign of zero counts), util.COUNTERS, statistics 50
    and 51..56, MIN_PIVOT, MAX_PIVOT and the statistics tail: identical.  Returns the device's factors (None on error)."""
    assert sg == so, (where, sg, so)
    if so not in (K.OK, K.WARNING_SINGULAR_MATRIX):
        return None
    fg, fo = g.get_factors(), o.get_factors()
    for k in util.INT_KEYS:
        assert np.array_equal(np.asarray(fg[k], np.int64), np.asarray(fo[k], np.int64)), (where, k)
    for k in util.VAL_KEYS:
        a, b = np.ascontiguousarray(fg[k], np.float64).view(np.int64), np.ascontiguousarray(fo[k], np.float64).view(np.int64)
        assert np.array_equal(a, b), (where, k, np.flatnonzero(a != b)[:8] if a.shape == b.shape else (a.shape, b.shape))
    for c in util.COUNTERS:
        assert int(g.stat(getattr(K, "STAT_" + c))) == int(o.stat(getattr(K, "STAT_" + c))), (where, c)
    for key in range(50, 57):
        assert g.stat(key) == o.stat(key), (where, "statistic", key, g.stat(key), o.stat(key))
    for c in ("MIN_PIVOT", "MAX_PIVOT") + FSTATS:
        a, b = g.stat(getattr(K, "STAT_" + c)), o.stat(getattr(K, "STAT_" + c))
        assert np.float64(a).view(np.int64) == np.float64(b).view(np.int64) or (np.isnan(a) and np.isnan(b)), (where, c, a, b)
    return fg


# ---- exact checks, no oracle, no tolerance ----------------------------------------------------------------------------
def exact_int(x, what):
    """x as int64 after asserting that every entry is an integer: the exact checks never fall back to a tolerance."""
    x = np.asarray(x, np.float64)
    assert np.all(np.isfinite(x)) and np.all(x == np.rint(x)), (what, "not integer", x[x != np.rint(x)][:5])
    assert np.all(np.abs(x) < 2.0 ** 52), (what, "beyond exact integers")
    return np.rint(x).astype(np.int64)


def dense_int(cp, ri, v, m, what="B"):
    """The CSC matrix as a dense int64 array (duplicates would add; stored zeros vanish)."""
    A = np.zeros((m, m), np.int64)
    cols = np.repeat(np.arange(m), np.diff(np.asarray(cp, np.int64)))
    np.add.at(A, (np.asarray(ri, np.int64), cols), exact_int(v, what))
    return A


def exact_lu(cp, ri, v, f, rank):
    """L @ U == B[rowperm][:, colperm] in int64, the columns colperm[rank..] replaced by unit columns (as util.check_factors
    does), after the structure checks of util.check_factors.  Returns (B, L, U) as dense int64."""
    m = len(cp) - 1
    util.check_factors(cp, ri, v, f, rank=rank)
    B = dense_int(cp, ri, v, m)
    L = dense_int(f["l_colptr"], f["l_rowidx"], f["l_value"], m, "L")
    U = dense_int(f["u_colptr"], f["u_rowidx"], f["u_value"], m, "U")
    PBQ = B[np.asarray(f["rowperm"], np.int64)][:, np.asarray(f["colperm"], np.int64)]
    for k in range(rank, m):
        PBQ[:, k] = 0
        PBQ[k, k] = 1
    assert np.array_equal(L @ U, PBQ), ("L U != P B Q", int(np.abs(L @ U - PBQ).max()))
    return B, L, U


def exact_tree_factors(h, cp, ri, v, status, stored_zeros=False):
    """A tree basis: status OK, RANK = m, MIN_PIVOT = MAX_PIVOT = 1.0, every |L value| = |U value| = 1, L U = P B Q.
    stored_zeros: B holds explicit zeros, which L and U inherit: values 0 are allowed (and must occur)."""
    m = len(cp) - 1
    assert status == K.OK and int(h.stat(K.STAT_RANK)) == m, (status, h.stat(K.STAT_RANK))
    assert h.stat(K.STAT_MIN_PIVOT) == 1.0 and h.stat(K.STAT_MAX_PIVOT) == 1.0, (h.stat(K.STAT_MIN_PIVOT), h.stat(K.STAT_MAX_PIVOT))
    f = h.get_factors()
    a = np.abs(np.concatenate((f["l_value"], f["u_value"])))
    assert np.all((a == 1.0) | (a == 0.0)) and bool((a == 0.0).any()) == stored_zeros, (a.min(), a.max(), stored_zeros)
    return exact_lu(cp, ri, v, f, m)[0]


def exact_interval_factors(h, cp, ri, v, edges, status):
    """A random interval matrix: RANK = (m + 1) - components, whatever the oracle says; L U = P B Q with unit columns."""
    m = len(cp) - 1
    rank = interval_rank(m, edges)
    assert int(h.stat(K.STAT_RANK)) == rank, (h.stat(K.STAT_RANK), rank)
    assert status == (K.OK if rank == m else K.WARNING_SINGULAR_MATRIX), status
    return exact_lu(cp, ri, v, h.get_factors(), rank)[0]


def exact_dense_solves(h, B, rng, where):
    """solve_dense with an integer right-hand side (entries -3..3), both systems: the solution is integer, B x == b."""
    m = B.shape[0]
    for trans, A in (("N", B), ("T", B.T)):
        b = rng.integers(-3, 4, m)
        x = exact_int(h.solve_dense(b.astype(np.float64), trans), (where, "solve_dense", trans))
        assert np.array_equal(A @ x, b), (where, "solve_dense", trans)


def sparse_rhs(m, nz, rng):
    ir = rng.choice(m, nz, replace=False)
    xr = rng.integers(1, 4, nz) * rng.choice((-1, 1), nz)  # nonzero integers in -3..3
    return ir, xr.astype(np.float64)


def exact_sparse_solve(out, A, ir, xr, where):
    """(status, pattern, values) of a sparse solve: integer values, A x == b, and the pattern is exactly the nonzeros --
    entries that cancel to zero inside the solve leave it."""
    st, il, lhs = out
    assert st == K.OK, (where, st)
    b = np.zeros(A.shape[0], np.int64)
    b[ir] = exact_int(xr, where)
    x = exact_int(lhs, (where, "values"))
    assert np.array_equal(A @ x, b), (where, "A x != b")
    assert np.array_equal(np.sort(il), np.flatnonzero(lhs)), (where, "pattern")


# ---- updates that stay exact ------------------------------------------------------------------------------------------
class TreeColumns:
    """Column source of util_update.run_updates that keeps a tree basis a tree basis: the outgoing edge j splits the tree in
    two; with probability 0.85 the incoming edge (span <= span, random sign) reconnects the halves -- the new basis is again
    TU and xtbl is exactly +-1 -- and otherwise lies inside one half: xtbl == 0.0 exactly and update() must answer
    ERROR_SINGULAR_UPDATE.  accepted(j) is called when the replacement was applied."""

    def __init__(self, rows, edges, span):
        self.rows, self.edges, self.span = rows, list(edges), span
        self.m = rows.m
        self.pending = None
        self.want_singular = None

    def __call__(self, rng, cols, m, j, pair_row=None):
        comp = components(m, self.edges[:j] + self.edges[j + 1:])
        d = np.arange(1, self.span + 1)[:, None]
        a = np.arange(0, m + 1)[None, :]
        ok = a + d <= m
        cross = np.zeros_like(ok)
        cross[ok] = comp[np.broadcast_to(a, ok.shape)[ok]] != comp[(a + d)[ok]]
        self.want_singular = bool(rng.random() >= 0.85) and bool((ok & ~cross).any())
        dd, aa = np.nonzero(ok & ~cross if self.want_singular else cross)
        pick = int(rng.integers(0, len(aa)))
        e = (int(aa[pick]), int(aa[pick]) + int(dd[pick]) + 1, float(rng.choice((-1.0, 1.0))))
        self.pending = (j, e)
        return self.rows.column(*e)

    def accepted(self, j):
        assert self.pending[0] == j
        self.edges[j] = self.pending[1]


def _int_matrix(B):
    return exact_int(B.toarray(), "B")


def run_exact_updates(h, twin, cp, ri, v, rows, edges, span, nsteps, seed):
    """util_update.run_updates with TreeColumns as its column source, h in lock step with its twin (util_update._same), and
    after every step, in int64 against the current B: both solve_for_update results, both solve_dense results (integer
    right-hand sides), a solve_sparse of three entries per system, xtbl exactly +-1 or 0.0 as the schedule says, PIVOT_ERROR == 0.0; after an exactly singular
    replacement the old factorization keeps solving exactly.  Returns run_updates' log and the final edge list."""
    from tests import util_update as U
    m = len(cp) - 1
    src = TreeColumns(rows, edges, span)
    rng = np.random.default_rng(seed)
    irng = np.random.default_rng(seed + 1)

    def dense(B, where):
        Bi = _int_matrix(B)
        for trans, A in (("N", Bi), ("T", Bi.T)):
            b = irng.integers(-3, 4, m)
            x = h.solve_dense(b.astype(np.float64), trans)
            if twin is not None:
                assert np.array_equal(x, twin.solve_dense(b.astype(np.float64), trans)), (where, "twin", trans)
            assert np.array_equal(A @ exact_int(x, (where, trans)), b), (where, "solve_dense", trans)
            ir, xr = sparse_rhs(m, 3, irng)
            a = U._ss(h, ir, xr, trans)
            if twin is not None:
                U._same(a, U._ss(twin, ir, xr, trans), (where, "solve_sparse", trans))
            exact_sparse_solve(a, A, ir, xr, (where, "solve_sparse", trans))

    def on_step(event, j, B, **what):
        if event == "btran":
            e = np.zeros(m, np.int64)
            e[j] = 1
            assert np.array_equal(_int_matrix(B).T @ exact_int(what["x"], "btran"), e), ("btran", j)
        elif event == "ftran":
            a = np.zeros(m, np.int64)
            a[what["ai"]] = exact_int(what["ax"], "column")
            x = what["x"]
            assert np.array_equal(_int_matrix(B) @ exact_int(x, "ftran"), a), ("ftran", j)
            assert (x[j] == 0.0) if src.want_singular else (abs(x[j]) == 1.0), ("xtbl", j, x[j], src.want_singular)
        else:
            assert (what["status"] == K.ERROR_SINGULAR_UPDATE) == src.want_singular, (j, what["status"], src.want_singular)
            if what["status"] == K.OK:
                src.accepted(j)
                assert h.stat(K.STAT_PIVOT_ERROR) == 0.0, h.stat(K.STAT_PIVOT_ERROR)
            dense(B, ("after", event, j, what["status"]))

    # (check_every: run_updates' own solves on random right-hand sides are left out -- dense() above makes them with integer
    # ones -- so the stream of rng holds the schedule alone and exact_batch_round draws the same one from the same seed)
    log = U.run_updates(h, U.columns_of(cp, ri, v), m, nsteps, rng, tol_xtbl=0.0, twin=twin, column_source=src, on_step=on_step,
                        check_every=nsteps + 1)
    assert log["done"] + log["singular"] == nsteps and log["skipped"] == 0 and not log["hit_maximum_updates"], log
    assert log["max_pivot_error"] == 0.0, log
    return log, src.edges


class ExactMember:
    def __init__(self, h, twin, cp, ri, v, rows, edges, span, seed):
        from tests import util_update as U
        self.h, self.twin, self.m = h, twin, len(cp) - 1
        self.cols = U.columns_of(cp, ri, v)
        self.src = TreeColumns(rows, edges, span)
        self.rng = np.random.default_rng(seed)
        self.done = self.singular = 0

    def B(self):
        from tests import util_update as U
        return _int_matrix(U.matrix_of(self.cols, self.m))


def exact_batch_round(blu, members, where):
    """One step of the exact schedule for every member through solve_for_update_batch ('T', then 'N') and update_batch:
    every status, pattern and value equal to the twin's single calls, the exact checks of run_exact_updates."""
    from tests import util_update as U
    from tests.util_update_batch import STATS, solution
    hs = [M.h for M in members]
    picks = []
    for M in members:
        j = int(M.rng.integers(0, M.m))
        picks.append((j,) + tuple(M.src(M.rng, M.cols, M.m, j)))
    st = blu.solve_for_update_batch(hs, [[p[0]] for p in picks], None, "T")
    for k, (M, (j, ai, ax)) in enumerate(zip(members, picks)):
        a = (st[k],) + solution(M.h)
        assert st[k] == K.OK, (where, "T", k, st[k])
        U._same(a, U._sfu(M.twin, [j], None, "T"), (where, "T", k))
        e = np.zeros(M.m, np.int64)
        e[j] = 1
        assert np.array_equal(M.B().T @ exact_int(a[2], "btran"), e), (where, "btran", k)
        assert np.array_equal(np.sort(a[1]), np.flatnonzero(a[2])), (where, "pattern T", k)
    st = blu.solve_for_update_batch(hs, [p[1] for p in picks], [p[2] for p in picks], "N")
    xtbl = []
    for k, (M, (j, ai, ax)) in enumerate(zip(members, picks)):
        a = (st[k],) + solution(M.h)
        assert st[k] == K.OK, (where, "N", k, st[k])
        U._same(a, U._sfu(M.twin, ai, ax, "N"), (where, "N", k))
        rhs = np.zeros(M.m, np.int64)
        rhs[ai] = exact_int(ax, "column")
        assert np.array_equal(M.B() @ exact_int(a[2], "ftran"), rhs), (where, "ftran", k)
        assert np.array_equal(np.sort(a[1]), np.flatnonzero(a[2])), (where, "pattern N", k)
        x = a[2][j]
        assert (x == 0.0) if M.src.want_singular else (abs(x) == 1.0), (where, "xtbl", k, x)
        xtbl.append(x)
    st = blu.update_batch(hs, xtbl)
    for k, (M, (j, ai, ax)) in enumerate(zip(members, picks)):
        assert M.twin.update(xtbl[k]) == st[k] == (K.ERROR_SINGULAR_UPDATE if M.src.want_singular else K.OK), (where, "update", k, st[k])
        for key in STATS:
            assert M.h.stat(key) == M.twin.stat(key), (where, "stat", key, k, M.h.stat(key), M.twin.stat(key))
        if st[k] == K.OK:
            M.src.accepted(j)
            M.cols[j] = (ai, ax)
            M.done += 1
            assert M.h.stat(K.STAT_PIVOT_ERROR) == 0.0, (where, k)
        else:
            M.singular += 1


def exact_batch_solves(blu, members, seed, where):
    """One round of solve_dense_batch and solve_sparse_batch (1, 3 and m // 3 entries), both systems: the twins' bits and
    the exact integer checks against each member's current B."""
    from tests import util_update as U
    from tests.util_update_batch import solution
    rng = np.random.default_rng(seed)
    hs = [M.h for M in members]
    Bs = [M.B() for M in members]
    for trans in "NT":
        rhs = [rng.integers(-3, 4, M.m) for M in members]
        sols, st = blu.solve_dense_batch(hs, [b.astype(np.float64) for b in rhs], trans)
        assert st == [K.OK] * len(members), (where, st)
        for k, (M, x, b, B) in enumerate(zip(members, sols, rhs, Bs)):
            assert np.array_equal(x, M.twin.solve_dense(b.astype(np.float64), trans)), (where, "solve_dense", trans, k)
            assert np.array_equal((B if trans == "N" else B.T) @ exact_int(x, (where, k)), b), (where, "solve_dense", trans, k)
        for nzf in (lambda m: 1, lambda m: 3, lambda m: m // 3):
            rs = [sparse_rhs(M.m, nzf(M.m), rng) for M in members]
            st = blu.solve_sparse_batch(hs, [r[0] for r in rs], [r[1] for r in rs], trans)
            for k, (M, (ir, xr), B) in enumerate(zip(members, rs, Bs)):
                a = (st[k],) + solution(M.h)
                U._same(a, U._ss(M.twin, ir, xr, trans), (where, "solve_sparse", trans, k))
                exact_sparse_solve(a, B if trans == "N" else B.T, ir, xr, (where, "solve_sparse", trans, k))
                for c in (K.STAT_L_FLOPS, K.STAT_U_FLOPS):
                    assert M.h.stat(c) == M.twin.stat(c), (where, c, k)


def exact_solves(h, o, B, seed, where):
    """On a nonsingular TU basis B (dense int64), for the handle h -- and, when o is given, against the oracle o: solve_dense
    with integer right-hand sides, both systems; solve_sparse with 1, 3 and m // 3 integer entries, both systems, at
    SPARSE_THRES 0.05 and 1.0: exact values, the pattern exactly the nonzeros, and pattern order, L_FLOPS and U_FLOPS
    equal to the oracle's."""
    from tests import util_update as U
    m = B.shape[0]
    rng = np.random.default_rng(seed)
    for trans, A in (("N", B), ("T", B.T)):
        b = rng.integers(-3, 4, m)
        x = h.solve_dense(b.astype(np.float64), trans)
        assert np.array_equal(A @ exact_int(x, (where, "solve_dense", trans)), b), (where, "solve_dense", trans)
        if o is not None:
            assert np.array_equal(x, o.solve_dense(b.astype(np.float64), trans)), (where, "solve_dense", trans, "oracle")
    for thres in (0.05, 1.0):
        for t in (h, o):
            if t is not None:
                t.set_param(K.PARAM_SPARSE_THRES, thres)
        for trans, A in (("N", B), ("T", B.T)):
            for nz in (1, 3, m // 3):
                ir, xr = sparse_rhs(m, nz, rng)
                a = U._ss(h, ir, xr, trans)
                exact_sparse_solve(a, A, ir, xr, (where, thres, trans, nz))
                if o is not None:
                    U._same(a, U._ss(o, ir, xr, trans), (where, thres, trans, nz))
                    for c in (K.STAT_L_FLOPS, K.STAT_U_FLOPS):
                        assert h.stat(c) == o.stat(c), (where, thres, trans, nz, c, h.stat(c), o.stat(c))
    for t in (h, o):
        if t is not None:
            t.set_param(K.PARAM_SPARSE_THRES, 0.05)


def scaled(basis, factor):
    cp, ri, v = basis[:3]
    return cp, ri, v * factor


def honest_inputs(orc):
    """The conditions that keep the exact tests honest, checked on the oracle over the committed seeds: the branches are
    reached, every pivot path is taken, the tree bases have a bump.  Returns the measured counts by case."""
    out = {}
    paths = np.zeros(6, np.int64)
    for name in ALL_CASES:
        cp, ri, v = case(name)[:3]
        o, st = oracle_run(orc, cp, ri, v)
        assert st == (K.WARNING_SINGULAR_MATRIX if name.startswith("interval") else K.OK), (name, st)
        c = o.cancellations()
        kinds = np.array([int(o.stat(51 + k)) for k in range(6)])
        paths += kinds
        out[name] = dict(c, d3=o.d3_hits(), bump=int(o.stat(K.STAT_BUMP_SIZE)), paths=kinds.tolist())
        m = len(cp) - 1
        if name.startswith("tree"):
            assert c["small"] > 0 and c["doubleton"] > 0, (name, c)
            assert 2 * out[name]["bump"] >= m, (name, out[name]["bump"])
        if name.startswith("dense"):
            assert c["any_stored"] > 0 and kinds[4] > 0, (name, c, kinds)
        if name == "zeros":
            assert c["doubleton_fill"] > 0, (name, c)
        assert o.stat(50) == o.d3_hits(), name
    assert (paths > 0).all(), dict(zip(PATHS, paths.tolist()))
    assert kinds_of(orc, "interval-64-5")[5] > 0  # the empty-column step comes from the interval matrices
    assert any(out[n]["d3"] > 0 for n in SMALLINTS), [out[n]["d3"] for n in SMALLINTS]
    cp, ri, v = case("smallint-300-8")[:3]
    o, st = oracle_run(orc, cp, ri, v, {K.PARAM_RELTOL: 1.0})
    assert st == K.OK and o.stat(55) > 0, (st, o.stat(55))  # pivot_any taken at reltol = 1.0
    out["smallint-300-8,reltol=1"] = dict(o.cancellations(), d3=o.d3_hits(), paths=[int(o.stat(51 + k)) for k in range(6)])
    return out


def kinds_of(orc, name):
    cp, ri, v = case(name)[:3]
    o, _ = oracle_run(orc, cp, ri, v)
    return [int(o.stat(51 + k)) for k in range(6)]


# ---- one case on the library and on the oracle (the GPU tests and the children of the emulation tests share these) ----
def both(blu, orc, cp, ri, v, params=None, setup=None):
    """The library (blu: the blu_amd module) and the oracle on the same input -> (g, o, status, oracle status)."""
    g = blu.BLU(len(cp) - 1, len(ri))
    for key, val in (params or {}).items():
        g.set_param(key, val)
    if setup:
        setup(g)
    sg = g.factorize(cp[:-1], cp[1:], ri, v)
    o, so = oracle_run(orc, cp, ri, v, params)
    return g, o, sg, so


def check_factorized(g, o, sg, so, name, where, solves=True):
    """assert_bitwise, and by family the exact checks: tree bases -- factors, rank, pivots, solves; interval matrices --
    rank and factors; the small-integer and dense families are parity only."""
    c = case(name)
    cp, ri, v = c[:3]
    assert_bitwise(g, o, sg, so, where)
    if name.startswith("tree") or name == "zeros":
        B = exact_tree_factors(g, cp, ri, v, sg, stored_zeros=(name == "zeros"))
        if solves:
            exact_solves(g, o, B, 11, where)
    elif name.startswith("interval"):
        exact_interval_factors(g, cp, ri, v, c[4], sg)


def check_case(blu, orc, name, params=None, setup=None, kernel=None, solves=True):
    cp, ri, v = case(name)[:3]
    g, o, sg, so = both(blu, orc, cp, ri, v, params, setup)
    if kernel is not None:
        assert int(g.stat(118)) == kernel, (name, g.stat(118), kernel)
    check_factorized(g, o, sg, so, name, (name, param_id(params or {})), solves)
    return g, o


def check_batch(blu, orc, names, regs=None):
    """All the cases as members of one blu_hip_factorize_batch call, each against its own oracle run."""
    mats = [case(n)[:3] for n in names]
    hs = [blu.BLU(len(cp) - 1, len(ri)) for cp, ri, v in mats]
    sts = blu.factorize_batch(hs, mats=mats)
    for n, h, (cp, ri, v), st in zip(names, hs, mats, sts):
        if regs is not None:
            assert int(h.stat(118)) == 3 and int(h.stat(120)) == regs, (n, h.stat(118), h.stat(120))
        o, so = oracle_run(orc, cp, ri, v)
        check_factorized(h, o, st, so, n, ("batch", n))


def check_abstol_equality(blu, orc, setup=None):
    """A tree basis scaled by 2^-40 with ABSTOL = 2^-40: every column maximum equals abstol and `cmx < abstol` is false --
    status OK and the permutations of the unscaled basis; with ABSTOL one ulp larger every column is below: rank 0."""
    base = case("tree-96-8")
    cp, ri, v = scaled(base, TWO_M40)
    g0, o0, sg0, so0 = both(blu, orc, *base[:3], setup=setup)
    g, o, sg, so = both(blu, orc, cp, ri, v, {K.PARAM_ABSTOL: TWO_M40}, setup)
    f = assert_bitwise(g, o, sg, so, "scaled, abstol at equality")
    f0 = assert_bitwise(g0, o0, sg0, so0, "unscaled")
    assert sg == sg0 == K.OK
    assert np.array_equal(f["rowperm"], f0["rowperm"]) and np.array_equal(f["colperm"], f0["colperm"])
    assert g.stat(K.STAT_MIN_PIVOT) == g.stat(K.STAT_MAX_PIVOT) == TWO_M40
    g, o, sg, so = both(blu, orc, cp, ri, v, {K.PARAM_ABSTOL: float(np.nextafter(TWO_M40, 1.0))}, setup)
    assert_bitwise(g, o, sg, so, "scaled, abstol one ulp above")
    assert sg == K.WARNING_SINGULAR_MATRIX and int(g.stat(K.STAT_RANK)) == 0, (sg, g.stat(K.STAT_RANK))


def check_droptol_equality(blu, orc, setup=None):
    """DROPTOL = 1.0 on a tree basis: `|x| > droptol` is false at equality (parity only: the factors are not B's)."""
    cp, ri, v = case("tree-96-8")[:3]
    g, o, sg, so = both(blu, orc, cp, ri, v, {K.PARAM_DROPTOL: 1.0}, setup)
    assert_bitwise(g, o, sg, so, "droptol = 1")


def check_updates(blu, orc, m, span, nsteps):
    """The exact update schedule on one tree basis, the library in lock step with its oracle twin."""
    cp, ri, v, rows, edges = tree_interval_basis(m, span, SEEDS["tree"])
    g, o, sg, so = both(blu, orc, cp, ri, v)
    assert sg == so == K.OK
    log, edges = run_exact_updates(g, o, cp, ri, v, rows, edges, span, nsteps, SCHEDULE_SEED)
    kinds = [int(g.stat(k)) for k in (K.STAT_NFORREST_TOTAL, K.STAT_NSYMPERM_TOTAL, K.STAT_DEV_NUNSYMPERM_TOTAL)]
    assert kinds == [int(o.stat(k)) for k in (K.STAT_NFORREST_TOTAL, K.STAT_NSYMPERM_TOTAL, K.STAT_DEV_NUNSYMPERM_TOTAL)]
    assert log["singular"] > 0 and kinds[0] > 0 and kinds[1] + kinds[2] > 0, (log, kinds)
    return log, kinds


def check_updates_batch(blu, orc, shapes, nsteps):
    """The same schedule through solve_for_update_batch and update_batch, the bases as members of one call, and a round of
    solve_dense_batch / solve_sparse_batch on fresh members before it and on updated members plus a fresh one after it."""
    def member(m, span, seed):
        cp, ri, v, rows, edges = tree_interval_basis(m, span, SEEDS["tree"])
        g, o, sg, so = both(blu, orc, cp, ri, v)
        assert sg == so == K.OK
        return ExactMember(g, o, cp, ri, v, rows, edges, span, seed)
    members = [member(m, span, SCHEDULE_SEED) for m, span in shapes]
    exact_batch_solves(blu, members, 21, "fresh")
    for r in range(nsteps):
        exact_batch_round(blu, members, r)
    assert all(M.done > 0 and M.h.stat(K.STAT_NUPDATE) == M.done for M in members), [(M.done, M.singular) for M in members]
    assert sum(M.singular for M in members) > 0
    exact_batch_solves(blu, members + [member(shapes[0][0], shapes[0][1], 99)], 22, "updated")
    return [(M.done, M.singular) for M in members]
