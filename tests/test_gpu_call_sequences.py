"""The call pattern of a simplex code (run with -m gpu): bases gathered from a constraint matrix, one handle reused
across factorize / solve / update / factorize, factorize calls that fail, getters read after every call.

B is passed as a simplex code passes it: b_begin = A_begin[basis], b_end = A_end[basis], b_i / b_x = A's whole arrays
(util.gathered_basis: columns out of storage order, poison between them).  Every check drives the CPU oracle through the
same call sequence and compares after every call: statuses, canonical factors and solutions bit for bit, every getter
(util.assert_same_getters).  Where a reused handle must behave like a fresh one it is also compared with a fresh device
handle, bit for bit.  The factors, norms and solves are further checked against the matrix assembled from the
[b_begin, b_end) ranges alone: L U = P B Q, the norms against math.fsum, backward errors in extended precision.
The update path follows the CPU restatement of the intended algorithm (oracle/orc_update.c; tests/test_gpu_update.py)."""
import ctypes as C
import math

import numpy as np
import pytest

from blu_amd import keys as K
from tests import util
from tests import util_update as U

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


class Pair:
    """A device handle and the oracle driven through the same calls; every call is compared and followed by a comparison
    of every getter."""

    def __init__(self, blu, orc, m, b_nz_hint, cap, skip_stats=False, params=None):
        self.blu, self.m, self.skip = blu, m, skip_stats
        self.g = blu.BLU(m, b_nz_hint)
        self.o = orc.OracleBLU(m, cap)
        self.o.set_fix_d3(True)  # the 64-bit cancellation mask, as the device (defect D3)
        if skip_stats:
            self.g.set_skip_stats(True)
        self.set_params(params or {})
        self.q = None

    def set_params(self, params):
        for k, v in params.items():
            self.g.set_param(k, v)
            self.o.set_param(k, v)

    def same(self, where):
        util.assert_same_getters(self.g, self.o, where, skip_stats=self.skip)

    def after_factorize(self, st, q, where):
        """compare a factorize the device has done (status st) on B = q with the oracle's of the same q"""
        so = self.o.factorize(*q)
        assert st == so, (where, st, so)
        self.same(where)
        self.q = q if st >= 0 else None
        if st >= 0:
            util.assert_same_factors(self.g.get_factors(), self.o.get_factors(), rtol=0.0)
            self.same((where, "get_factors"))
        return st

    def factorize(self, q, where):
        return self.after_factorize(self.g.factorize(*q), q, where)

    def solves(self, rng, where):
        """solve_dense and solve_sparse, both systems: equal to the oracle's, small backward error against the assembled B"""
        m = self.m
        B = util.gathered_matrix(*self.q, m)
        # threshold pivoting lets |U| grow beyond |B|; the backward error of a stable solve grows with it
        growth = max(1.0, float(np.abs(self.g.get_factors()["u_value"]).max()) / float(abs(B).max()))
        bound = be_bound(m) * growth
        for trans in ("N", "T"):
            A = B if trans == "N" else B.T.tocsc()
            b = rng.standard_normal(m)
            x = self.g.solve_dense(b, trans)
            assert np.array_equal(x, self.o.solve_dense(b, trans)), (where, "solve_dense", trans)
            self.same((where, "solve_dense", trans))
            if self.full_rank():
                assert backward_error(A, x, b) <= bound, (where, trans, growth, backward_error(A, x, b))
            nz = int(rng.integers(1, max(2, m // 20)))
            ir = rng.choice(m, nz, replace=False)
            xr = rng.standard_normal(nz)
            got = U._ss(self.g, ir, xr, trans)
            U._same(got, U._ss(self.o, ir, xr, trans), (where, "solve_sparse", trans))
            self.same((where, "solve_sparse", trans))
            if self.full_rank():
                bs = np.zeros(m)
                bs[ir] = xr
                assert backward_error(A, got[2], bs) <= bound, (where, trans, growth, backward_error(A, got[2], bs))

    def full_rank(self):
        return int(self.g.stat(K.STAT_RANK)) == self.m

    def updates(self, n, rng, where, twins=()):
        """n column replacements (util_update.new_column, permutation updates among them) in lock step with the oracle
        and the extra twins; returns the number done"""
        m = self.m
        cols = [(np.asarray(self.q[2][int(a):int(b)], np.int64), np.asarray(self.q[3][int(a):int(b)])) for a, b in zip(self.q[0], self.q[1])]
        f = self.g.get_factors()
        pair_row = np.zeros(m, np.int64)
        pair_row[f["colperm"]] = f["rowperm"]
        done = 0
        for step in range(n):
            w = (where, "update step", step)
            j = int(rng.integers(0, m))
            ai, ax = U.new_column(rng, cols, m, j, pair_row)
            got = U._sfu(self.g, [j], None, "T")
            for t in (self.o,) + tuple(twins):
                U._same(got, U._sfu(t, [j], None, "T"), (w, "solve_for_update T"))
            self.same((w, "solve_for_update T"))
            if got[0] == K.ERROR_MAXIMUM_UPDATES:
                break
            assert got[0] == K.OK, (w, got[0])
            got = U._sfu(self.g, ai, ax, "N")
            for t in (self.o,) + tuple(twins):
                U._same(got, U._sfu(t, ai, ax, "N"), (w, "solve_for_update N"))
            self.same((w, "solve_for_update N"))
            xtbl = got[2][j]
            if abs(xtbl) < 1e-3:
                continue
            st = self.g.update(xtbl)
            for t in (self.o,) + tuple(twins):
                assert t.update(xtbl) == st, (w, "update")
            self.same((w, "update"))
            if st == K.OK:
                cols[j] = (ai, ax)
                done += 1
        B = U.matrix_of(cols, m)
        b = rng.standard_normal(m)
        for trans, A in (("N", B), ("T", B.T.tocsc())):
            x = self.g.solve_dense(b, trans)
            assert np.array_equal(x, self.o.solve_dense(b, trans)), (where, "solve_dense after updates", trans)
            self.same((where, "solve_dense after updates", trans))
            assert backward_error(A, x, b) <= be_bound(m), (where, trans, backward_error(A, x, b))
        return done


def be_bound(m):
    """backward error a stable solve stays below: rounding-level, growing with m (1e-12 up to m = 1000)"""
    return 1e-15 * max(m, 1000)


def backward_error(A, x, b):
    """|A x - b| / (|A| |x| + |b|) in infinity norms, the residual summed in extended precision"""
    C = A.tocoo()
    r = np.zeros(A.shape[0], np.longdouble)
    np.add.at(r, C.row, C.data.astype(np.longdouble) * np.asarray(x, np.longdouble)[C.col])
    r -= np.asarray(b, np.longdouble)
    den = float(abs(A).sum(axis=1).max()) * float(np.abs(x).max()) + float(np.abs(b).max())
    return float(np.abs(r).max()) / max(den, 1e-300)


def check_against_matrix(g, q, m, where):
    """L U = P B Q on the matrix assembled from the ranges; ONENORM / INFNORM against exactly rounded sums"""
    rank = int(g.stat(K.STAT_RANK))
    util.check_factors(*util.gathered_csc(*q, m), g.get_factors(), rank=rank)
    if rank < m:
        return
    B = util.gathered_matrix(*q, m)
    for key, M in ((K.STAT_ONENORM, B.tocsc()), (K.STAT_INFNORM, B.T.tocsc())):
        lines = [M.data[M.indptr[j]:M.indptr[j + 1]] for j in range(m)]
        want = max(math.fsum(abs(float(x)) for x in ln) for ln in lines)
        n = max(len(ln) for ln in lines)
        got = g.stat(key)
        assert abs(got - want) <= n * EPS * want, (where, key, got, want)


def cap_of(q):
    return 64 * len(q[2]) + 4096


def fresh_equal(blu, g, q, where, params=None, skip_stats=False):
    """g's last factorize equals that of a fresh device handle on the same B with the same parameters, bit for bit"""
    h = blu.BLU(g.m, len(q[2]))
    for k, v in (params or {}).items():
        h.set_param(k, v)
    if skip_stats:
        h.set_skip_stats(True)
    st = h.factorize(*q)
    assert st == (K.WARNING_SINGULAR_MATRIX if g.stat(K.STAT_RANK) < g.m else K.OK), (where, st)
    fa, fb = g.get_factors(), h.get_factors()
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), (where, "fresh handle", k)
    util.assert_same_getters(g, h, (where, "fresh handle"), history=False)


def quadruple(mat):
    """(b_begin, b_end, b_i, b_x) of a CSC triple or a quadruple"""
    if len(mat) == 3:
        cp, ri, v = mat
        return cp[:-1].copy(), cp[1:].copy(), ri, v
    return mat


class DeviceArrays:
    """B's four arrays copied into device memory (hipMalloc of the HIP runtime the library is linked with)"""

    def __init__(self, blu, q):
        self.hip = blu.lib()  # (its symbol lookup reaches the runtime it depends on)
        self.hip.hipMalloc.argtypes = [C.c_void_p, C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.ptrs, self.n = [], len(q[2])
        for a in q:
            a = np.ascontiguousarray(a)
            p = C.c_void_p()
            assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 8)) == 0
            self.ptrs.append(p.value)
            assert self.hip.hipMemcpy(p.value, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice

    def __del__(self):
        for p in self.ptrs:
            self.hip.hipFree(p)


SIZES = [(300, {}), (2000, {}), (6000, {}), (10_000, dict(k=8, bw=8))]  # the last: the size and pattern of C2


@pytest.mark.parametrize("m,gen", SIZES, ids=[str(m) for m, _ in SIZES])
def test_gathered_bases(blu, oracle, m, gen):
    """(a) a gathered basis through blu_hip_factorize (with a b_nz hint below the summed column lengths: k_prep asks for
    room), blu_hip_factorize_device and blu_hip_factorize_batch with host and device inputs (bench.py's entry) -- the batch mixing gathered
    and CSC members of different m; each followed by solves and a short update run in lock step with the oracle"""
    rng = np.random.default_rng(m)
    q = util.gathered_basis(m, 11, end_last=True, **gen)
    nupd = 12 if m <= 2000 else 4
    for entry in ("host", "device", "batch_host", "batch_device"):
        where = (m, entry)
        p = Pair(blu, oracle, m, m // 2 if entry == "host" else len(q[2]), cap_of(q))
        if entry == "host":
            st = p.g.factorize(*q)
        elif entry == "device":
            d = DeviceArrays(blu, q)
            st = p.g.factorize_device(*d.ptrs, d.n)
        else:
            others = [("csc", 500, blu.BLU(500, 3000)), ("gathered", 400, blu.BLU(400, 100))]  # the second asks for room
            mats = [q]
            for kind, mm, _ in others:
                if kind == "csc":
                    cp, ri, v = oracle.gen_lp_basis(mm, 6, 8, 0.5, 5, 0.3)
                    mats.append((cp, ri, v))
                else:
                    mats.append(util.gathered_basis(mm, 12, n_empty=1))
            hs = [p.g] + [h for _, _, h in others]
            if entry == "batch_host":
                sts = blu.factorize_batch(hs, mats)
            else:
                ds = [DeviceArrays(blu, quadruple(mt)) for mt in mats]
                sts = blu.factorize_batch(hs, device_ptrs=[tuple(d.ptrs) + (d.n,) for d in ds])
            st = sts[0]
            for (kind, mm, h), mt, s in zip(others, mats[1:], sts[1:]):
                qq = quadruple(mt)
                o = oracle.OracleBLU(mm, cap_of(qq))
                o.set_fix_d3(True)
                assert s == o.factorize(*qq), (where, kind)
                util.assert_same_getters(h, o, (where, kind))
                util.assert_same_factors(h.get_factors(), o.get_factors(), rtol=0.0)
        assert p.after_factorize(st, q, where) == K.OK
        check_against_matrix(p.g, q, m, where)
        p.solves(rng, where)
        p.updates(nupd, rng, where)


def test_gathered_bases_with_shared_and_empty_columns(blu, oracle):
    """(a) singular gathered bases: a column listed twice (two columns share storage), empty columns; single and batch"""
    rng = np.random.default_rng(5)
    qs = [util.gathered_basis(700, 21, twice=True), util.gathered_basis(900, 22, n_empty=3), util.gathered_basis(800, 23, n_empty=1, twice=True)]
    for q in qs:
        m = len(q[0])
        p = Pair(blu, oracle, m, len(q[2]), cap_of(q))
        assert p.factorize(q, m) == K.WARNING_SINGULAR_MATRIX
        check_against_matrix(p.g, q, m, m)
        p.solves(rng, m)
    ps = [Pair(blu, oracle, len(q[0]), len(q[2]), cap_of(q)) for q in qs]
    sts = blu.factorize_batch([p.g for p in ps], qs)
    for p, q, st in zip(ps, qs, sts):
        assert p.after_factorize(st, q, ("batch", p.m)) == K.WARNING_SINGULAR_MATRIX
        p.solves(rng, ("batch", p.m))


def test_handle_reuse(blu, oracle):
    """(b) one handle through a simplex code's life: single factorize (chain pipeline) and solve_sparse (row-wise L built);
    a batch factorize of a different basis, whose solves must use the new factors; single factorize again; 40 update
    attempts; re-factorize and updates in lock step with a fresh twin as well; a singular factorize, then a full-rank one;
    a parameter change between factorizes"""
    m = 1200
    rng = np.random.default_rng(17)
    qs = [util.gathered_basis(m, s) for s in range(40, 46)]
    p = Pair(blu, oracle, m, len(qs[0][2]), max(cap_of(q) for q in qs))
    assert p.factorize(qs[0], "first") == K.OK
    p.solves(rng, "first")
    other = blu.BLU(700, 5000)
    q_other = util.gathered_basis(700, 47)
    sts = blu.factorize_batch([other, p.g], [q_other, qs[1]])
    assert p.after_factorize(sts[1], qs[1], "batch") == K.OK
    fresh_equal(blu, p.g, qs[1], "batch")
    p.solves(rng, "batch")
    assert p.factorize(qs[2], "third") == K.OK
    fresh_equal(blu, p.g, qs[2], "third")
    p.solves(rng, "third")
    done = p.updates(40, rng, "updates")
    assert done >= 25, done
    assert p.g.stat(K.STAT_NSYMPERM_TOTAL) + p.g.stat(K.STAT_DEV_NUNSYMPERM_TOTAL) > 0  # permutation updates among them
    assert p.factorize(qs[3], "refactorize") == K.OK
    fresh_equal(blu, p.g, qs[3], "refactorize")
    twin = oracle.OracleBLU(m, cap_of(qs[3]))
    twin.set_fix_d3(True)
    assert twin.factorize(*qs[3]) == K.OK
    assert p.updates(15, rng, "updates after refactorize", twins=(twin,)) > 5
    singular = util.gathered_basis(m, 48, twice=True)
    assert p.factorize(singular, "singular") == K.WARNING_SINGULAR_MATRIX
    p.solves(rng, "singular")
    assert p.factorize(qs[4], "after singular") == K.OK
    fresh_equal(blu, p.g, qs[4], "after singular")
    p.solves(rng, "after singular")
    params = {K.PARAM_ABSTOL: 1e-11, K.PARAM_RELTOL: 0.3, K.PARAM_MAXSEARCH: 6, K.PARAM_NZBIAS: 0}
    p.set_params(params)
    assert p.factorize(qs[5], "new parameters") == K.OK
    fresh_equal(blu, p.g, qs[5], "new parameters", params=params)
    p.solves(rng, "new parameters")


@pytest.mark.parametrize("alias", [True, False], ids=["factors_in_arena", "no_out_alias"])
def test_large_then_small_matrix(blu, oracle, monkeypatch, alias):
    """(b) a dense basis, then a sparse one of the same m on the same handle: storage sized by the first, canonical factors
    in the dead column arena (default) or in buffers of their own (BLU_NO_OUT_ALIAS, read when the handle is created)"""
    if not alias:
        monkeypatch.setenv("BLU_NO_OUT_ALIAS", "1")
    m = 3000
    rng = np.random.default_rng(3)
    big = util.gathered_basis(m, 51, k=16, bw=40, tri_frac=0.1)
    small = util.gathered_basis(m, 52, k=3, bw=3)
    p = Pair(blu, oracle, m, len(small[2]), cap_of(big))
    for q, where in ((big, "large"), (small, "small"), (big, "large again")):
        assert p.factorize(q, where) == K.OK
        fresh_equal(blu, p.g, q, where)
        p.solves(rng, where)
    p.updates(6, rng, "updates")
    assert p.factorize(small, "small after updates") == K.OK
    fresh_equal(blu, p.g, small, "small after updates")


@pytest.mark.parametrize("kind", ["index", "order"])
@pytest.mark.parametrize("history", ["factorized", "updated"])
def test_failed_factorize(blu, oracle, kind, history):
    """(c) a factorize that is refused (a row index >= m; b_end < b_begin) after a fresh factorize or after updates: every
    getter is the oracle's (lu.reset(), lu.rs:329-359); get_factors, solve_dense, solve_sparse, solve_for_update and update
    return the reference's status; the next factorize equals a fresh handle's"""
    m = 600
    rng = np.random.default_rng(9)
    q = util.gathered_basis(m, 61)
    p = Pair(blu, oracle, m, len(q[2]), cap_of(q))
    assert p.factorize(q, "first") == K.OK
    if history == "updated":
        assert p.updates(10, rng, "updates") > 0
    bad = util.spoil(*q, kind, seed=3)
    assert p.factorize(bad, "refused") == K.ERROR_INVALID_ARGUMENT
    b = rng.standard_normal(m)
    calls = [("get_factors", lambda x: x.get_factors), ("solve_dense", lambda x: lambda: x.solve_dense(b)),
             ("solve_sparse", lambda x: lambda: x.solve_sparse([1, 5], [1.0, -2.0])),
             ("solve_for_update", lambda x: lambda: x.solve_for_update([3], None, "T")), ("update", lambda x: lambda: x.update(0.5))]
    for name, call in calls:
        sg, so = util.status_of(call(p.g)), util.status_of(call(p.o))
        assert sg == so and sg < 0, (name, sg, so)
        p.same(("after refused", name))
    q2 = util.gathered_basis(m, 62)
    assert p.factorize(q2, "next") == K.OK
    fresh_equal(blu, p.g, q2, "next")
    p.solves(rng, "next")
    p.updates(5, rng, "updates after")


def test_batch_of_members_with_different_histories(blu, oracle):
    """(d) one batch whose members are: fresh; updated; last call refused; previously a larger matrix; skip_stats on.  Each
    equals its own oracle sequence"""
    rng = np.random.default_rng(13)
    ms = [300, 350, 400, 450, 500]
    first = [util.gathered_basis(m, 70 + k, **(dict(k=14, bw=30) if k == 3 else {})) for k, m in enumerate(ms)]
    ps = [Pair(blu, oracle, m, len(q[2]), 2 * cap_of(q), skip_stats=(k == 4)) for k, (m, q) in enumerate(zip(ms, first))]
    assert ps[1].factorize(first[1], "updated member") == K.OK
    assert ps[1].updates(10, rng, "updated member") > 0
    assert ps[2].factorize(first[2], "refused member") == K.OK
    assert ps[2].factorize(util.spoil(*first[2], "index"), "refused member") == K.ERROR_INVALID_ARGUMENT
    assert ps[3].factorize(first[3], "larger member") == K.OK
    assert ps[4].factorize(first[4], "skip_stats member") == K.OK
    qs = [util.gathered_basis(m, 80 + k) for k, m in enumerate(ms)]
    sts = blu.factorize_batch([p.g for p in ps], qs)
    for k, (p, q, st) in enumerate(zip(ps, qs, sts)):
        assert p.after_factorize(st, q, ("batch member", k)) == K.OK
        fresh_equal(blu, p.g, q, ("batch member", k), skip_stats=p.skip)
        p.solves(rng, ("batch member", k))
        p.updates(5, rng, ("batch member", k))
