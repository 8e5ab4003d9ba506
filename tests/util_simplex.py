"""A dual simplex run through the device entries beside an exact twin (tests/test_gpu_simplex.py on hardware,
tests/test_emu_cpu_simplex.py on the emulation build).

The LPs are  minimise c'x  subject to  A x = b, lo <= x <= up  (some columns free) on interval matrices: totally unimodular
(`tu`), the same with every row and every column multiplied by a power of two from 2^-2 .. 2^2 (`tu2`), and a `tu2` instance
with one right-hand side entry out of the reach of its row (`infeasible`).  Every basis inverse then has entries 0 or
+-2^k, every quantity of a dual simplex is an integer or a dyadic rational that a double holds exactly, and the device has to
reproduce a rational-arithmetic simplex WITHOUT ANY TOLERANCE, iteration by iteration.

    make_lp / lp        the families, seeded, computed once per name
    twin                the reference: a dense dual simplex in fractions.Fraction -- no float decision, no call into
                        blu_amd, the oracle, util_ratio or util_matrix
    Node, run_single    the same decisions taken from the device entries: factorize_columns, solve_dense, price, set_duals,
                        ratio_test(prepare_update), solve_for_update_column, update, update_duals
    run_generation      a generation of forked nodes in lock step through copy_batch, share_matrix, copy_duals_batch,
                        solve_dense_batch, ratio_test_batch, solve_for_update_batch, update_batch, update_duals_batch
    twin_properties     what keeps the cases from passing vacuously, asserted on the twin alone

Device values are converted with Fraction(float), which is exact, and compared with ==.  The only inexact comparison is
twin against scipy's HiGHS (highs_agrees), a check of this file and not of the device.

The conventions of an iteration, as the twin fixes them: position r leaves with sigma = -1 when x_B[r] is below its lower
bound and +1 when it is above its upper bound; t = d_q / alpha_q is the SIGNED step; update_duals(t, [q, leaving], [0, -t],
[0, k]) with k = +1 / -1 for a column that left at its lower / upper bound and 0 for a fixed one."""
from fractions import Fraction as F

import numpy as np

import blu_amd
from blu_amd import keys as K

PIVTOL = 2.0 ** -20
HARRIS = 0.25       # the dualtol of the runs compared with the twin only
REFACTOR = 5        # updates between two factorize_columns
NEVER = 10 ** 9     # ... or none (the eta file decides)
SPAN = 6            # longest interval
MAXITER = 600


# ---- the families -----------------------------------------------------------------------------------------------------
class LP:
    """cols[j] = ([rows], [values as Fraction]); c, b Fractions; lo / up Fractions or None (no bound); a = (a_p, a_i, a_x) the
    same matrix as compressed columns of doubles; columns 0..m-1 are the start basis."""

    def with_bounds(self, lo, up):
        out = LP()
        out.__dict__.update(self.__dict__)
        out.lo, out.up = list(lo), list(up)
        return out

    def is_free(self, j):
        return self.lo[j] is None and self.up[j] is None

    def is_fixed(self, j):
        return self.lo[j] is not None and self.lo[j] == self.up[j]


def exact_inverse(M):
    """Gauss-Jordan over Fractions; M a list of rows"""
    n = len(M)
    W = [list(row) + [F(int(i == k)) for k in range(n)] for i, row in enumerate(M)]
    for c in range(n):
        p = next(i for i in range(c, n) if W[i][c] != 0)
        W[c], W[p] = W[p], W[c]
        piv = W[c][c]
        W[c] = [x / piv for x in W[c]]
        for i in range(n):
            f = W[i][c]
            if i != c and f != 0:
                W[i] = [x - f * y if y != 0 else x for x, y in zip(W[i], W[c])]
    return [row[n:] for row in W]


def basis_matrix(lp, basis):
    B = [[F(0)] * lp.m for _ in range(lp.m)]
    for p, j in enumerate(basis):
        for i, v in zip(*lp.cols[j]):
            B[i][p] = v
    return B


def col_dot(lp, j, y):
    return sum((y[i] * v for i, v in zip(*lp.cols[j]) if y[i] != 0), F(0))


def exact_duals(lp, basis):
    """c - A' B^-T c_B from scratch"""
    Binv = exact_inverse(basis_matrix(lp, basis))
    y = [sum((lp.c[basis[p]] * Binv[p][i] for p in range(lp.m) if Binv[p][i] != 0), F(0)) for i in range(lp.m)]
    return [lp.c[j] - col_dot(lp, j, y) for j in range(lp.ncol)]


def make_lp(family, m, nextra, seed):
    rng = np.random.default_rng(seed)
    scaled = family != "tu"
    with_free = family != "infeasible"
    ncol = 2 * m + nextra
    # the spanning tree of the nodes 0..m: the start basis
    parent = list(range(m + 1))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    edges = []
    while len(edges) < m:
        d = int(rng.integers(1, SPAN + 1))
        a = int(rng.integers(0, m + 1 - d))
        ra, rb = find(a), find(a + d)
        if ra != rb:
            parent[ra] = rb
            edges.append((a, a + d))
    edges = [edges[k] for k in rng.permutation(m)]
    for _ in range(nextra):
        d = int(rng.integers(1, SPAN + 1))
        a = int(rng.integers(0, m + 1 - d))
        edges.append((a, a + d))
    edges += [(i, i + 1) for i in range(m)]  # the unit slacks
    colsign = [int(s) for s in rng.choice((-1, 1), ncol)]
    rowsign = [int(s) for s in rng.choice((-1, 1), m)]
    for j in range(ncol - m, ncol):
        colsign[j] = rowsign[j - (ncol - m)]  # a slack is +1 (times the scales)
    rs = [F(2) ** int(e) for e in (rng.integers(-2, 3, m) if scaled else np.zeros(m, int))]
    cs = [F(2) ** int(e) for e in (rng.integers(-2, 3, ncol) if scaled else np.zeros(ncol, int))]
    lp = LP()
    lp.family, lp.m, lp.nextra, lp.ncol, lp.seed = family, m, nextra, ncol, seed
    lp.cols = [(list(range(a, b)), [colsign[j] * rowsign[i] * rs[i] * cs[j] for i in range(a, b)]) for j, (a, b) in enumerate(edges)]
    # bounds: boxes of small integers; a few slacks and two tree columns fixed; a fifth of the tree columns and 2 to 6
    # extra columns free
    lo = [F(int(x)) for x in rng.integers(-3, 4, ncol)]
    up = [l + int(w) for l, w in zip(lo, rng.integers(1, 7, ncol))]
    tree = [int(j) for j in rng.permutation(m)]
    fixed = tree[:2] + [ncol - m + int(i) for i in rng.permutation(m)[:max(2, m // 6)]]
    free = (tree[2:2 + max(1, m // 5)] + [m + int(j) for j in rng.permutation(nextra)[:min(6, max(2, nextra // 12))]]) if with_free else []
    for j in fixed:
        up[j] = lo[j]
    for j in free:
        lo[j] = up[j] = None
    lp.lo, lp.up = lo, up
    x = [F(int(rng.integers(-3, 4))) if lo[j] is None else lo[j] + int(rng.integers(0, int(up[j] - lo[j]) + 1)) for j in range(ncol)]
    lp.c = [F(int(v)) for v in rng.integers(-4, 5, ncol)]
    d = exact_duals(lp, list(range(m)))
    for j in free:  # the free extra columns start nonbasic with a reduced cost of exactly 0
        if j >= m:
            lp.c[j] -= d[j]
    for j in range(4 * m, m + nextra):  # extra columns beyond the first 3 m (the wide shape): the feasible point has them
        if lo[j] is not None:           # at their start bound, so that their number adds candidates, not iterations
            x[j] = lo[j] if d[j] >= 0 else up[j]
    lp.b = [F(0)] * m
    for j in range(ncol):
        for i, v in zip(*lp.cols[j]):
            lp.b[i] += v * x[j]
    if family == "infeasible":  # one row asked for more than its columns can give
        i0 = int(rng.integers(0, m))
        reach = F(0)
        for j in range(ncol):
            for i, v in zip(*lp.cols[j]):
                if i == i0:
                    reach += max(v * lo[j], v * up[j])
        lp.b[i0] = reach + 1
    a_p = np.zeros(ncol + 1, np.uint64)
    a_p[1:] = np.cumsum([len(r) for r, _ in lp.cols])
    lp.a = (a_p, np.concatenate([r for r, _ in lp.cols]).astype(np.uint64), np.array([float(v) for _, vs in lp.cols for v in vs]))
    return lp


# (family, m, nextra): the seed -- chosen on the twin so that twin_properties holds
SEEDS = {("tu", 12, 36): 22, ("tu2", 12, 36): 2, ("infeasible", 12, 36): 2,
         ("tu", 24, 72): 51, ("tu2", 24, 72): 98, ("infeasible", 24, 72): 3,
         ("tu", 40, 120): 0, ("tu2", 40, 120): 0, ("infeasible", 40, 120): 5,
         ("tu2", 24, 1100): 1}
WIDE = 1100  # ncol = 1148: more than 1024, 17 * 64 + 60
_lps, _twins = {}, {}


def lp(family, m, nextra):
    key = (family, m, nextra)
    if key not in _lps:
        _lps[key] = make_lp(family, m, nextra, SEEDS[key])
    return _lps[key]


# ---- the exact twin ---------------------------------------------------------------------------------------------------
def leaving(lp, basis, xB):
    """(r, sigma): the largest bound violation, the smallest position among equals, never a free variable; (-1, 0): none"""
    best, r, sigma = 0, -1, 0
    for p, j in enumerate(basis):
        lo, up = lp.lo[j], lp.up[j]
        if lo is not None and xB[p] < lo:
            v, s = lo - xB[p], -1
        elif up is not None and xB[p] > up:
            v, s = xB[p] - up, 1
        else:
            continue
        if v > best:
            best, r, sigma = v, p, s
    return r, sigma


def entering(alpha, d, kind, sigma, pivtol, dualtol):
    """The selection rule of include/blu_hip.h in exact arithmetic: (q, ncand, alpha_q, d_q, step_q, theta, pool size,
    number of largest |alpha| in the pool, whether q beat a smaller index with a smaller |alpha|)"""
    cand = []
    for j, k in enumerate(kind):
        if k == 0:
            continue
        s, a = sigma * alpha[j], abs(alpha[j])
        if (k == 1 and s > pivtol) or (k == -1 and s < -pivtol) or (k == 2 and a > pivtol):
            cand.append(j)
    if not cand:
        return (-1, 0, F(0), F(0), F(0), F(0), 0, 0, False)
    theta = min((abs(d[j]) + dualtol) / abs(alpha[j]) for j in cand)
    pool = [j for j in cand if abs(d[j]) / abs(alpha[j]) <= theta]
    amax = max(abs(alpha[j]) for j in pool)
    top = [j for j in pool if abs(alpha[j]) == amax]
    q = min(top)
    return (q, len(cand), alpha[q], d[q], abs(d[q]) / abs(alpha[q]), theta, len(pool), len(top), min(pool) < q)


def start_state(lp, d):
    """kind and the nonbasic values for the start basis 0..m-1 and the reduced costs d; d of a fixed column is set to 0"""
    kind, xn = [0] * lp.ncol, [F(0)] * lp.ncol
    for j in range(lp.m, lp.ncol):
        if lp.is_free(j):
            assert d[j] == 0, ("a free column starts with a reduced cost of 0", j)
            kind[j] = 2
        elif lp.is_fixed(j):  # never a candidate: its reduced cost is not kept (see start_node)
            xn[j], d[j] = lp.lo[j], F(0)
        else:
            kind[j] = 1 if d[j] >= 0 else -1
            xn[j] = lp.lo[j] if d[j] >= 0 else lp.up[j]
    return kind, xn


def nonbasic_rhs(lp, isbasic, xn):
    """b - N x_N"""
    rhs = list(lp.b)
    for j in range(lp.ncol):
        if not isbasic[j] and xn[j] != 0:
            for i, v in zip(*lp.cols[j]):
                rhs[i] -= v * xn[j]
    return rhs


def basic_values(lp, Binv, isbasic, xn):
    rhs = nonbasic_rhs(lp, isbasic, xn)
    return [sum((Binv[p][i] * rhs[i] for i in range(lp.m) if Binv[p][i] != 0 and rhs[i] != 0), F(0)) for p in range(lp.m)]


class Run:
    pass


def twin(lp, dualtol, start=None):
    """The dense dual simplex.  start = (basis, d, kind, xn) continues from another run's final state (a forked node whose
    bounds were cut).  Returns a Run: status ('optimal' / 'infeasible'), iters (one dict per iteration: r, sigma, xB, q,
    ncand, alpha_q, d_q, step, bound, alpha, kind0 in front of the step, d and kind behind it, leave, t, kq), and the final basis, d, kind, xn, xB,
    x and objective."""
    m, ncol = lp.m, lp.ncol
    dualtol, pivtol = F(dualtol), F(PIVTOL)
    if start is None:
        basis = list(range(m))
        d = exact_duals(lp, basis)
        kind, xn = start_state(lp, d)
    else:
        basis, d, kind, xn = [list(v) for v in start]
    isbasic = [False] * ncol
    for j in basis:
        isbasic[j] = True
    Binv = exact_inverse(basis_matrix(lp, basis))
    run = Run()
    run.lp, run.dualtol, run.iters, run.d0, run.kind0 = lp, dualtol, [], list(d), list(kind)
    while True:
        assert len(run.iters) < MAXITER, "the twin does not end"
        xB = basic_values(lp, Binv, isbasic, xn)
        r, sigma = leaving(lp, basis, xB)
        if r < 0:
            run.status = "optimal"
            break
        y = Binv[r]
        alpha = [col_dot(lp, j, y) if kind[j] != 0 else F(0) for j in range(ncol)]
        q, ncand, alpha_q, d_q, step, bound, npool, ntop, beat = entering(alpha, d, kind, sigma, pivtol, dualtol)
        it = dict(r=r, sigma=sigma, xB=xB, q=q, ncand=ncand, alpha_q=alpha_q, d_q=d_q, step=step, bound=bound, alpha=alpha,
                  npool=npool, ntop=ntop, beat=beat, kind0=list(kind))
        run.iters.append(it)
        if q < 0:
            run.status = "infeasible"
            it.update(d=list(d), kind=list(kind))
            break
        t = d_q / alpha_q
        leave = basis[r]
        d = [d[j] - t * alpha[j] if kind[j] != 0 else d[j] for j in range(ncol)]
        kl = 0 if lp.is_fixed(leave) else (1 if sigma < 0 else -1)
        it.update(kq=kind[q], t=t, leave=leave, kleave=kl)
        d[q], kind[q] = F(0), 0
        d[leave], kind[leave] = -t, kl
        xn[leave] = lp.lo[leave] if sigma < 0 else lp.up[leave]
        xn[q] = F(0)
        w = [col_dot(lp, q, Binv[p]) for p in range(m)]  # the FTRAN column
        assert w[r] == alpha_q
        Binv[r] = [x / w[r] for x in Binv[r]]
        for p in range(m):
            if p != r and w[p] != 0:
                Binv[p] = [x - w[p] * z if z != 0 else x for x, z in zip(Binv[p], Binv[r])]
        basis[r], isbasic[leave], isbasic[q] = q, False, True
        it.update(d=list(d), kind=list(kind))
    assert Binv == exact_inverse(basis_matrix(lp, basis)), "the twin's own inverse"
    run.basis, run.d, run.kind, run.xn, run.xB = basis, d, kind, xn, xB
    run.x = list(xn)
    for p, j in enumerate(basis):
        run.x[j] = xB[p]
    run.objective = sum((c * x for c, x in zip(lp.c, run.x)), F(0))
    return run


def twin_of(family, m, nextra, dualtol):
    key = (family, m, nextra, dualtol)
    if key not in _twins:
        _twins[key] = twin(lp(family, m, nextra), dualtol)
    return _twins[key]


def feasible(lp, x):
    """x within its bounds and A x == b, exactly"""
    ax = [F(0)] * lp.m
    for j in range(lp.ncol):
        for i, v in zip(*lp.cols[j]):
            ax[i] += v * x[j]
    return ax == lp.b and all((lp.lo[j] is None or x[j] >= lp.lo[j]) and (lp.up[j] is None or x[j] <= lp.up[j]) for j in range(lp.ncol))


def dual_feasible(d, kind):
    return all((k != 1 or v >= 0) and (k != -1 or v <= 0) for v, k in zip(d, kind))


def highs(lp):
    from scipy.optimize import linprog
    from scipy.sparse import csc_matrix

    A = csc_matrix((lp.a[2], lp.a[1].astype(np.int64), lp.a[0].astype(np.int64)), shape=(lp.m, lp.ncol))
    bounds = [(None if l is None else float(l), None if u is None else float(u)) for l, u in zip(lp.lo, lp.up)]
    return linprog([float(v) for v in lp.c], A_eq=A, b_eq=[float(v) for v in lp.b], bounds=bounds, method="highs")


def highs_agrees(run):
    """Twin against HiGHS on the same LP -- both are references, so this checks the file.  An optimum is a multiple of 2^-8;
    HiGHS's value rounds to it and lies within 1e-6 (1 + |obj|) of it, HiGHS's own accuracy class.  Infeasible: status 2."""
    res = highs(run.lp)
    if run.status == "infeasible":
        assert res.status == 2, res.status
        return
    obj = run.objective
    assert res.status == 0 and (obj * 256).denominator == 1, (res.status, obj)
    assert F(round(res.fun * 256), 256) == obj and abs(res.fun - float(obj)) <= 1e-6 * (1 + abs(float(obj))), (res.fun, obj)


def refactorizations(run, every=REFACTOR):
    return sum(1 for it in run.iters if it["q"] >= 0) // every


def twin_properties(run):
    """What every committed run shows, on the twin alone: returns the counts the family-wide properties are summed from"""
    lp = run.lp
    piv = [it for it in run.iters if it["q"] >= 0]
    assert len(piv) >= lp.m and refactorizations(run) >= 2, (len(piv), lp.m)
    assert {it["sigma"] for it in run.iters} == {-1, 1}
    if run.dualtol == 0:
        assert all(dual_feasible(it["d"], it["kind"]) for it in run.iters)
        if run.status == "optimal":
            assert feasible(lp, run.x)
    ties = sum(1 for it in piv if it["npool"] > 1 and it["ntop"] > 1)
    if lp.family == "tu":
        assert 4 * ties >= len(piv), (ties, len(piv))
    return dict(iterations=len(piv), refactorizations=refactorizations(run), kinds={it["kq"] for it in piv},
                fixed_left=sum(1 for it in piv if lp.is_fixed(it["leave"]) and it["kleave"] == 0), ties=ties,
                by_size=sum(1 for it in piv if it["beat"]), far=sum(1 for it in piv if it["q"] >= 1024),
                winners=[it["q"] for it in piv])


# ---- the device driver ------------------------------------------------------------------------------------------------
def fr(a):
    return [F(float(x)) for x in a]


def exact_floats(v):
    out = np.array([float(x) for x in v])
    assert all(F(float(o)) == x for o, x in zip(out, v)), "a value of the LP that a double does not hold"
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Node:
    """The host side of one simplex run on a handle: the basis list, the nonbasic values, the bounds, what a caller of the
    entries keeps.  Every step is compared with the twin `tw` when one is given, and logged as the doubles it saw."""

    def __init__(self, lp, h, basis, xn, nupd=0, every=REFACTOR, dualtol=0.0, tw=None, what=""):
        self.lp, self.h, self.basis, self.xn, self.nupd, self.every, self.dualtol, self.tw, self.what = lp, h, list(basis), list(xn), nupd, every, dualtol, tw, what
        self.isbasic = [False] * lp.ncol
        for j in self.basis:
            self.isbasic[j] = True
        self.it, self.log, self.status, self.nrefactor, self.forced = 0, [], None, 0, 0
        st, self.d_last, self.kind_last = h.get_duals()
        assert st == K.OK

    def expect(self, ok, *what):
        assert ok, (self.what, "iteration", self.it) + what

    def tw_it(self):
        return self.tw.iters[self.it] if self.tw is not None and self.it < len(self.tw.iters) else None

    def rhs(self):
        return exact_floats(nonbasic_rhs(self.lp, self.isbasic, self.xn))

    def choose(self, xB):
        """the leaving position from the device's x_B: (r, sigma), r < 0 when the basis is optimal"""
        self.xB = fr(xB)
        self.r, self.sigma = leaving(self.lp, self.basis, self.xB)
        self.log.append(dict(xB=np.array(xB), r=self.r, sigma=self.sigma))
        if self.tw is not None:
            if self.it == len(self.tw.iters):
                self.expect(self.tw.status == "optimal" and self.r < 0 and self.xB == self.tw.xB, "the twin is optimal here", self.r)
            else:
                t = self.tw.iters[self.it]
                self.expect(self.xB == t["xB"], "x_B")
                self.expect((self.r, self.sigma) == (t["r"], t["sigma"]), "leaving", self.r, self.sigma, t["r"], t["sigma"])
        if self.r < 0:
            self.status = "optimal"
        return self.r, self.sigma

    def picked(self, st, rec):
        """the record and the kept row behind a ratio test: q"""
        self.expect(st == K.OK, "ratio_test", st)
        st, row = self.h.ratio_row()
        self.expect(st == K.OK, "ratio_row", st)
        self.rec, self.row = rec, row
        self.log[-1].update(rec=rec, row=row)
        t = self.tw_it()
        if t is not None:
            self.expect(rec[:2] == (t["q"], t["ncand"]), "q, ncand", rec[:2], t["q"], t["ncand"])
            self.expect(fr(rec[2:]) == [t["alpha_q"], t["d_q"], t["step"], t["bound"]], "alpha_q, d_q, step, bound", rec)
            self.expect(fr(row) == t["alpha"], "the kept row")
            self.expect(not np.signbit(row[np.array(t["kind0"]) == 0]).any(), "+0.0 where kind == 0")
        if rec[0] < 0:
            self.expect(rec == (-1, 0, 0.0, 0.0, 0.0, 0.0) and not np.signbit(rec[2:]).any(), "no candidate", rec)
            self.status = "infeasible"
        return rec[0]

    def spiked(self, st):
        """behind the forward solve of column q: xtbl"""
        self.expect(st == K.OK, "solve_for_update of the entering column", st)
        x = float(self.h.lhs[self.r])
        self.log[-1].update(lhs=self.h.lhs.copy())
        self.expect(F(x) == F(self.rec[2]), "lhs[r] of the FTRAN is alpha_q", x, self.rec[2])
        return x

    def step(self):
        """(t, (jset, dset, kset)) of update_duals"""
        q, leave = self.rec[0], self.basis[self.r]
        t = self.rec[3] / self.rec[2]
        self.expect(F(t) == F(self.rec[3]) / F(self.rec[2]), "d_q / alpha_q is exact")
        k = 0 if self.lp.is_fixed(leave) else (1 if self.sigma < 0 else -1)
        return t, ([q, leave], [0.0, -t], [0, k])

    def pivoted(self, st_update, st_duals):
        """behind update and update_duals: the bookkeeping, get_duals against the twin, the refactorization"""
        self.expect(st_update == K.OK, "update", st_update)
        self.expect(st_duals == K.OK, "update_duals", st_duals)
        q, leave = self.rec[0], self.basis[self.r]
        self.xn[leave] = self.lp.lo[leave] if self.sigma < 0 else self.lp.up[leave]
        self.xn[q] = F(0)
        self.basis[self.r], self.isbasic[leave], self.isbasic[q] = q, False, True
        st, d, kind = self.h.get_duals()
        self.expect(st == K.OK, "get_duals", st)
        self.log[-1].update(d=d, kind=kind)
        t = self.tw_it()
        if t is not None:
            self.expect(fr(d) == t["d"], "d behind the step")
            self.expect(kind.tolist() == t["kind"], "kind behind the step")
        if self.dualtol == 0:
            self.expect(dual_feasible(d, kind), "the duals stay feasible")
        self.expect(all(d[j] == 0 and kind[j] == 0 for j in self.basis), "basic columns: d == 0, kind == 0")
        alone = self.kind_last == 0
        alone[[q, leave]] = False
        self.expect(np.array_equal(bits(d)[alone], bits(self.d_last)[alone]), "the step leaves d alone where kind == 0, bit for bit")
        self.d_last, self.kind_last = d, kind
        self.nupd += 1
        self.it += 1
        if self.nupd >= self.every:
            self.refactorize()

    def refactorize(self):
        _, d0, k0 = self.h.get_duals()
        _, row0 = self.h.ratio_row()
        self.expect(self.h.factorize_columns(self.basis) == K.OK, "factorize_columns")
        st, d1, k1 = self.h.get_duals()
        st2, row1 = self.h.ratio_row()
        self.expect(st == st2 == K.OK and np.array_equal(bits(d0), bits(d1)) and np.array_equal(k0, k1) and np.array_equal(bits(row0), bits(row1)),
                    "factorize_columns leaves d, kind and the kept row alone")
        self.from_scratch(d1, k1)
        self.nupd = 0
        self.nrefactor += 1

    def from_scratch(self, d, kind):
        """d == c - A' B^-T c_B with B from the basis list, on every column the dual step maintains: the basic ones (0) and
        those with kind != 0.  A fixed nonbasic column (kind 0) is left out of the step by the contract and keeps the
        reduced cost it had when it became fixed-nonbasic, which is no longer its reduced cost."""
        want = exact_duals(self.lp, self.basis)
        bad = [j for j in range(self.lp.ncol) if (kind[j] != 0 or self.isbasic[j]) and F(float(d[j])) != want[j]]
        self.expect(not bad, "d == c - A' B^-T c_B from scratch", bad)
        self.expect(all(self.lp.is_fixed(j) for j in range(self.lp.ncol) if kind[j] == 0 and not self.isbasic[j]), "kind 0 and nonbasic: fixed")

    def finish(self):
        """the end of a run: status, iteration count and basis are the twin's; the invariants from scratch"""
        lp = self.lp
        st, d, kind = self.h.get_duals()
        self.expect(st == K.OK, "get_duals", st)
        self.from_scratch(d, kind)
        self.x = list(self.xn)
        for p, j in enumerate(self.basis):
            self.x[j] = self.xB[p]
        self.objective = sum((c * x for c, x in zip(lp.c, self.x)), F(0))
        if self.status == "optimal":
            self.expect(feasible(lp, self.x), "x within its bounds, A x == b")
        if self.tw is not None:
            self.expect((self.status, self.it + (self.status == "infeasible")) == (self.tw.status, len(self.tw.iters)), "status, iterations", self.status, self.it)
            self.expect(self.basis == self.tw.basis and kind.tolist() == self.tw.kind and fr(d) == self.tw.d, "the final basis, kind, d")
            if self.status == "optimal":
                self.expect(self.objective == self.tw.objective and self.x == self.tw.x, "the objective", self.objective, self.tw.objective)


def new_root(lp):
    h = blu_amd.BLU(lp.m, len(lp.a[1]))
    assert h.set_matrix(lp.ncol, *lp.a) == K.OK
    return h


def start_node(lp, h, tw=None, **kw):
    """factorize_columns of the start basis, the start duals through solve_dense('T') + price, set_duals once"""
    basis = list(range(lp.m))
    assert h.factorize_columns(basis) == K.OK
    c = exact_floats(lp.c)
    d = c - h.price(h.solve_dense(c[:lp.m], "T"))
    exact = fr(d)
    kind, xn = start_state(lp, exact)
    # a fixed column has kind 0 for good, and the dual step leaves d alone where kind == 0: it starts as -0.0, which a step
    # that touched it would turn into +0.0 (-0.0 - t * (+0.0) for t < 0) -- pivoted() looks at the bits
    d[[j for j in range(lp.m, lp.ncol) if lp.is_fixed(j)]] = -0.0
    if tw is not None:
        assert exact == tw.d0 and kind == tw.kind0, "the start duals"
    assert h.set_duals(d, np.array(kind, np.int8)) == K.OK
    return Node(lp, h, basis, xn, tw=tw, **kw)


def run_single(node):
    """the iterations of one node through the single entries, to the end"""
    h = node.h
    while True:
        r, sigma = node.choose(h.solve_dense(node.rhs()))
        if r < 0:
            break
        st, rec = h.ratio_test(r, float(sigma), PIVTOL, node.dualtol, prepare_update=True)
        if st == K.ERROR_MAXIMUM_UPDATES:  # the eta file is full: what a caller does
            node.forced += 1
            node.refactorize()
            st, rec = h.ratio_test(r, float(sigma), PIVTOL, node.dualtol, prepare_update=True)
        if node.picked(st, rec) < 0:
            break
        xtbl = node.spiked(h.solve_for_update_column(rec[0]))
        st = h.update(xtbl)
        t, sets = node.step()
        node.pivoted(st, h.update_duals(t, *sets))
    node.finish()
    return node


def check_single(family, m, nextra, dualtol, every=REFACTOR):
    """one run of a committed case beside its twin"""
    tw = twin_of(family, m, nextra, dualtol)
    h = new_root(tw.lp)
    node = run_single(start_node(tw.lp, h, tw=tw, every=every, dualtol=dualtol, what=(family, m, nextra, dualtol, every)))
    assert node.nrefactor - node.forced == (refactorizations(tw, every) if every != NEVER else 0), (node.nrefactor, node.forced)
    h.close()
    return node


# ---- a generation of forked nodes -------------------------------------------------------------------------------------
def cuts(root, n):
    """[(position, 'lo' / 'up', the new bound)]: for child k one bound of a basic boxed variable tightened past the root
    optimum, inside its box; lower and upper cuts alternate"""
    lp, out = root.lp, {"lo": [], "up": []}
    for p, j in enumerate(root.basis):
        if lp.is_free(j) or lp.is_fixed(j):
            continue
        x = root.xB[p]
        if x + 1 <= lp.up[j]:
            out["lo"].append((p, "lo", x + 1))
        if x - 1 >= lp.lo[j]:
            out["up"].append((p, "up", x - 1))
    assert out["lo"] and out["up"], "no variable to branch on"
    return [out[("lo", "up")[k % 2]][(k // 2) % len(out[("lo", "up")[k % 2]])] for k in range(n)]


def child_lp(root, cut):
    lp = root.lp
    p, side, v = cut
    lo, up = list(lp.lo), list(lp.up)
    (lo if side == "lo" else up)[root.basis[p]] = v
    return lp.with_bounds(lo, up)


def child_twins(family, m, nextra, n):
    key = ("children", family, m, nextra, n)
    if key not in _twins:
        tw = twin_of(family, m, nextra, 0)
        root = Run()
        root.lp, root.basis, root.xB = tw.lp, tw.basis, tw.xB
        _twins[key] = [twin(child_lp(root, cut), 0, start=(tw.basis, tw.d, tw.kind, tw.xn)) for cut in cuts(root, n)]
    return _twins[key]


def same_logs(a, b, what):
    """two runs saw the same bits"""
    assert len(a) == len(b), (what, len(a), len(b))
    for it, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys(), (what, it)
        for key in x:
            same = x[key] == y[key] if key in ("r", "sigma") else (x[key][:2] == y[key][:2] and np.array_equal(bits(x[key][2:]), bits(y[key][2:]))) if key == "rec" else (
                np.array_equal(x[key], y[key]) if key == "kind" else np.array_equal(bits(x[key]), bits(y[key])))
            assert same, (what, "iteration", it, key)


def run_generation(family, m, nextra, n, chunk_bytes=-1):
    """The root to optimality through the single entries, n children forked from its UPDATED factorization, iterated in
    lock step through the batch entries until each is optimal or infeasible; every child beside its twin and beside the
    single entries on a clone of the root with the same cut.  Returns the children's nodes."""
    tw = twin_of(family, m, nextra, 0)
    lp0 = tw.lp
    g = new_root(lp0)
    root = run_single(start_node(lp0, g, tw=tw, what=(family, m, nextra, "root")))
    assert root.status == "optimal" and root.nupd >= 1 and g.stat(K.STAT_NUPDATE) >= 1, "the children inherit an updated factorization"
    row0 = max(range(m), key=lambda p: (root.basis[p] >= m, p))
    before = (g.solve_dense(root.rhs()), g.ratio_test(row0, 1.0, PIVTOL, 0.0))
    twins = child_twins(family, m, nextra, n)
    the_cuts = cuts(root, n)

    def fork(k):
        return Node(twins[k].lp, hs[k], root.basis, root.xn, nupd=root.nupd, tw=twins[k], what=(family, m, nextra, "child", k, the_cuts[k][:2]))

    hs = [blu_amd.BLU(m, 8) for _ in range(n)]
    assert blu_amd.copy_batch(g, hs) == blu_amd.share_matrix(g, hs) == blu_amd.copy_duals_batch(g, hs) == [K.OK] * n
    assert g.dbg_matrix_holders() == n + 1
    assert g.dbg_set_matrix_batch_bytes(chunk_bytes) == K.OK
    nodes = [fork(k) for k in range(n)]
    active, sizes, first = list(nodes), [], True
    while active:
        sizes.append(len(active))
        hh = [c.h for c in active]
        sols, sts = blu_amd.solve_dense_batch(hh, [c.rhs() for c in active])
        assert sts == [K.OK] * len(active), sts
        picks = [c.choose(x) for c, x in zip(active, sols)]
        if first:
            assert all(r >= 0 for r, _ in picks) and (n == 1 or {s for _, s in picks} == {-1, 1}), "every child starts infeasible, both sigmas"
            first = False
        for c in active:
            if c.status:
                c.finish()
        active = [c for c in active if not c.status]
        if not active:
            break
        hh = [c.h for c in active]
        sts, recs = blu_amd.ratio_test_batch(hh, [c.r for c in active], [float(c.sigma) for c in active], PIVTOL, 0.0, prepare_update=True)
        for c, st, rec in zip(active, sts, recs):
            if c.picked(st, rec) < 0:
                c.finish()
        active = [c for c in active if not c.status]
        if not active:
            break
        hh = [c.h for c in active]
        sts = blu_amd.solve_for_update_batch(hh, [lp0.cols[c.rec[0]][0] for c in active], [[float(v) for v in lp0.cols[c.rec[0]][1]] for c in active], "N")
        xtbl = [c.spiked(st) for c, st in zip(active, sts)]
        st_upd = blu_amd.update_batch(hh, xtbl)
        steps = [c.step() for c in active]
        st_duals = blu_amd.update_duals_batch(hh, [t for t, _ in steps], [s for _, s in steps])
        for c, su, sd in zip(active, st_upd, st_duals):
            c.pivoted(su, sd)
    assert g.dbg_set_matrix_batch_bytes(-1) == K.OK
    # the same cuts through the single entries on clones of the root: the same bits
    for k in range(n):
        s = g.clone()
        assert blu_amd.share_matrix(g, [s]) == blu_amd.copy_duals_batch(g, [s]) == [K.OK]
        one = Node(twins[k].lp, s, root.basis, root.xn, nupd=root.nupd, what=(family, m, nextra, "clone", k))
        same_logs(run_single(one).log, nodes[k].log, (family, m, nextra, n, "child", k, "against the single entries"))
        s.close()
    # the root is where it was, and the holders are counted
    after = (g.solve_dense(root.rhs()), g.ratio_test(row0, 1.0, PIVTOL, 0.0))
    assert np.array_equal(bits(before[0]), bits(after[0])) and before[1][0] == after[1][0] == K.OK
    assert before[1][1][:2] == after[1][1][:2] and np.array_equal(bits(before[1][1][2:]), bits(after[1][1][2:])), "the root's ratio test"
    assert g.dbg_matrix_holders() == n + 1
    for k, h in enumerate(hs):
        h.close()
        assert g.dbg_matrix_holders() == n - k
    g.close()
    return nodes, sizes


def generation_properties(family, m, nextra, n):
    """on the twins alone: the children finish at three or more different iteration counts (n >= 9)"""
    twins = child_twins(family, m, nextra, n)
    ends = sorted(len(t.iters) for t in twins)
    assert n < 9 or len(set(ends)) >= 3, ends
    return ends, [t.status for t in twins]


# ---- the committed cases ----------------------------------------------------------------------------------------------
SHAPES = ((12, 36), (24, 72), (40, 120))
WIDE_CASE = ("tu2", 24, WIDE)
RUNS = tuple((f, m, x, 0) for f in ("tu", "tu2", "infeasible") for m, x in SHAPES) + (WIDE_CASE + (0,),) + tuple(("tu2", m, x, HARRIS) for m, x in SHAPES)
GENERATIONS = (("tu", 24, 72), ("tu2", 24, 72), WIDE_CASE, ("tu", 12, 36))


def committed_properties(runs=RUNS, generations=GENERATIONS):
    """Every property of the committed seeds that is asserted on the twin alone (a failure here is a defect of this file,
    not of the library), and twin against HiGHS.  Returns the table of DESIGN.md: one row per run."""
    table, seen = [], {}
    for family, m, nextra, dualtol in runs:
        tw = twin_of(family, m, nextra, dualtol)
        assert tw.status == ("infeasible" if family == "infeasible" else "optimal")
        pr = twin_properties(tw)
        if dualtol == 0:
            highs_agrees(tw)
        else:  # Harris changes the trajectory
            base = twin_of(family, m, nextra, 0)
            assert [(it["r"], it["q"]) for it in tw.iters] != [(it["r"], it["q"]) for it in base.iters], (family, m, nextra)
        if family == "tu2":
            assert pr["by_size"] >= 1, (family, m, nextra, "no pick decided by the larger |alpha| against a smaller index")
        if nextra == WIDE:  # a winner behind column 1024: past one stride of the single pick's workgroup, in the last, partial stride of both
            assert tw.lp.ncol > 1024 and tw.lp.ncol % 64 and pr["far"] >= 1, (tw.lp.ncol, pr["far"])
        acc = seen.setdefault(family, dict(kinds=set(), fixed_left=0))
        acc["kinds"] |= pr["kinds"]
        acc["fixed_left"] += pr["fixed_left"]
        table.append((family, m, nextra, float(dualtol), tw.status, pr["iterations"], pr["refactorizations"], sorted(pr["kinds"]), pr["ties"], pr["by_size"], pr["far"]))
    for family, acc in seen.items():
        assert acc["kinds"] == ({1, -1} if family == "infeasible" else {1, -1, 2}) and acc["fixed_left"] >= 1, (family, acc)
    ends = {}
    for family, m, nextra in generations:
        tw = twin_of(family, m, nextra, 0)
        assert sum(1 for it in tw.iters if it["q"] >= 0) % REFACTOR != 0, "the root ends with an update behind its last refactorization"
        for n in ((9,) if nextra != 72 else (1, 9, 17)):
            ends[(family, m, nextra, n)] = generation_properties(family, m, nextra, n)
    return table, ends
