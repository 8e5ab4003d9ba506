"""blu_hip_solve_dense_batch on the MI355X (run with -m gpu): solve_dense for many handles in one call, one wave per
system.  Every member's solution must be bit-identical to the oracle's solve_dense and to blu_hip_solve_dense on the
same handle; the call must leave no trace on its members beyond the row-wise L it builds (which later single calls
reuse) and the marker it advances as solve_dense does."""
import ctypes as C

import numpy as np
import pytest

from blu_amd import keys as K
from blu_amd.matrices import CONFIGS
from tests import util
from tests import util_update as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


def quad(mat):
    if len(mat) == 4:
        return mat
    cp, ri, v = mat
    return cp[:-1].copy(), cp[1:].copy(), ri, v


def twin_of(orc, q):
    m = len(q[0])
    o = orc.OracleBLU(m, 64 * len(q[2]) + 1024)
    o.set_fix_d3(True)  # the 64-bit cancellation mask, as the device (defect D3)
    return o, o.factorize(*q)


def small_and_medium(orc, n):
    """n bases of 300..5000 rows: synthetic LP bases, gathered ones, singular ones (rank < m)"""
    mats = []
    for s in range(n):
        m = (300, 800, 1500, 3000, 5000)[s % 5]
        kind = s % 4
        if kind == 0:
            mats.append(quad(orc.gen_lp_basis(m, 6 + s % 4, 8, 0.5, 100 + s, 0.3)))
        elif kind == 1:
            mats.append(util.gathered_basis(m, 200 + s))
        elif kind == 2:
            mats.append(util.gathered_basis(m, 300 + s, n_empty=1 + s % 3))
        else:
            mats.append(util.gathered_basis(m, 400 + s, twice=True))
    return mats


class DevBuf:
    """float64 / int64 array in device memory (hipMalloc of the HIP runtime the library is linked with)"""

    def __init__(self, blu, a=None, n=None, dtype=np.float64):
        self.hip = blu.lib()  # (its symbol lookup reaches the runtime it depends on)
        self.hip.hipMalloc.argtypes = [C.c_void_p, C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.n, self.dtype = (len(a), a.dtype) if a is not None else (n, np.dtype(dtype))
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(self.n * self.dtype.itemsize, 8)) == 0
        self.ptr = p.value
        if a is not None:
            self.put(a)

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert self.hip.hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice

    def get(self):
        out = np.empty(self.n, self.dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptr, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def __del__(self):
        self.hip.hipFree(self.ptr)


def raw_call(blu, hs, rp, lp, trans="N", on_dev=0, n=None):
    L = blu.lib()
    L.blu_hip_solve_dense_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_char, C.c_int, C.c_void_p]
    k = len(hs)
    H = (C.c_void_p * max(k, 1))(*[h._h if h is not None else None for h in hs])
    R = (C.c_void_p * max(k, 1))(*rp)
    Lp = (C.c_void_p * max(k, 1))(*lp)
    st = (C.c_int * max(k, 1))(*([77] * max(k, 1)))
    rc = L.blu_hip_solve_dense_batch(H, k if n is None else n, R, Lp, trans.encode(), on_dev, st)
    return rc, list(st)[:k]


def test_bit_exact_against_oracle_and_single_solve(blu, oracle):
    """24 small and medium bases (gathered, singular ones among them), fresh from factorize_batch, each with its own
    right-hand side: both directions equal the oracle and blu_hip_solve_dense bit for bit, cold (the row-wise L built by
    the batch) and warm"""
    mats = small_and_medium(oracle, 24)
    hs = [blu.BLU(len(q[0]), len(q[2])) for q in mats]
    sts = blu.factorize_batch(hs, mats)
    twins = []
    for k, (q, s) in enumerate(zip(mats, sts)):
        o, so = twin_of(oracle, q)
        assert s == so and s >= 0, (k, s, so)
        twins.append(o)
    assert any(int(h.stat(K.STAT_RANK)) < h.m for h in hs)
    rng = np.random.default_rng(7)
    rhs = [rng.standard_normal(h.m) for h in hs]
    for tr in "NT":
        for rep in ("cold", "warm"):
            sols, st = blu.solve_dense_batch(hs, rhs, tr)
            assert st == [K.OK] * len(hs), (tr, st)
            for k, (h, o) in enumerate(zip(hs, twins)):
                assert np.array_equal(sols[k], o.solve_dense(rhs[k], tr)), (tr, rep, k)
                if rep == "warm":
                    assert np.array_equal(sols[k], h.solve_dense(rhs[k], tr)), (tr, rep, k)


def mixed_members(blu, oracle):
    """[(handle, twin or None, expected status)]: fresh from factorize_batch, from a single factorize (chain-pipeline row
    copies), after Forrest-Tomlin updates in lock step with the twin, last factorize refused, m = 0"""
    out = []
    mats = [quad(oracle.gen_lp_basis(m, 6, 8, 0.5, s, 0.3)) for m, s in ((600, 1), (2000, 2))] + [util.gathered_basis(1200, 3, n_empty=2)]
    hb = [blu.BLU(len(q[0]), len(q[2])) for q in mats]
    for h, q, s in zip(hb, mats, blu.factorize_batch(hb, mats)):
        o, so = twin_of(oracle, q)
        assert s == so
        out.append((h, o, K.OK))
    for m, seed in ((900, 4), (4000, 5)):
        q = util.gathered_basis(m, seed)
        h = blu.BLU(m, len(q[2]))
        o, so = twin_of(oracle, q)
        assert h.factorize(*q) == so
        out.append((h, o, K.OK))
    for m, seed in ((700, 6), (1500, 7)):
        cp, ri, v = oracle.gen_lp_basis(m, 6, 8, 0.5, seed, 0.3)
        cols = U.columns_of(cp, ri, v)
        h = blu.BLU(m, len(ri))
        assert h.factorize(cp[:-1], cp[1:], ri, v) == K.OK
        o = U.fresh_oracle(oracle, cols, m)
        log = U.run_updates(h, cols, m, 10, np.random.default_rng(seed), twin=o)
        assert log["done"] >= 2 and int(h.stat(K.STAT_NUPDATE)) == log["done"]
        out.append((h, o, K.OK))
    q = util.gathered_basis(800, 8)
    h = blu.BLU(800, len(q[2]))
    assert h.factorize(*util.spoil(*q, "index")) == K.ERROR_INVALID_ARGUMENT
    out.append((h, None, K.ERROR_INVALID_CALL))
    h = blu.BLU(0, 1)
    e = np.zeros(0, np.uint64)
    assert h.factorize(e, e, e, np.zeros(0)) == K.OK
    out.append((h, None, K.OK))
    return out


def test_mixed_states_in_one_call(blu, oracle):
    members = mixed_members(blu, oracle)
    order = np.random.default_rng(3).permutation(len(members))  # kinds interleaved
    members = [members[i] for i in order]
    hs = [h for h, _, _ in members]
    want = [w for _, _, w in members]
    rng = np.random.default_rng(11)
    rhs = [rng.standard_normal(h.m) for h in hs]
    for tr in "NTNT":
        sols, st = blu.solve_dense_batch(hs, rhs, tr)
        assert st == want, (tr, st)
        for k, (h, o, w) in enumerate(members):
            if o is None:
                assert not sols[k].any()
                continue
            assert np.array_equal(sols[k], o.solve_dense(rhs[k], tr)), (tr, k)
            assert np.array_equal(sols[k], h.solve_dense(rhs[k], tr)), (tr, k)
    outs = [np.zeros(max(h.m, 1)) for h in hs]
    rc, st = raw_call(blu, hs, [r.ctypes.data or 8 for r in rhs], [x.ctypes.data for x in outs])
    assert rc == K.ERROR_INVALID_CALL and st == want


def test_no_side_effects(blu, oracle):
    """Members that saw a batch solve and twins that never did: the same getters (and the oracle's), then the same bits
    from solve_dense, solve_sparse, solve_for_update and update -- the row-wise L the batch built and the marker it
    advanced are what the single calls would have used"""
    def make():
        return [(h, o) for h, o, w in mixed_members(blu, oracle) if o is not None]
    A, B = make(), make()
    rng = np.random.default_rng(13)
    rhs = [rng.standard_normal(h.m) for h, _ in A]
    for tr in "NT":
        _, st = blu.solve_dense_batch([h for h, _ in A], rhs, tr)
        assert st == [K.OK] * len(A)
    for k, ((ha, oa), (hb, ob)) in enumerate(zip(A, B)):
        util.assert_same_getters(ha, oa, ("after batch", k))
        util.assert_same_getters(ha, hb, ("after batch vs untouched", k))
        r = rhs[k]
        for tr in "NT":
            xa = ha.solve_dense(r, tr)
            assert np.array_equal(xa, hb.solve_dense(r, tr)) and np.array_equal(xa, oa.solve_dense(r, tr)), (k, tr)
            ob.solve_dense(r, tr)
        m = ha.m
        idx = np.sort(rng.choice(m, 5, replace=False))
        val = rng.standard_normal(5)
        for tr in "NT":
            a, b, c = U._ss(ha, idx, val, tr), U._ss(hb, idx, val, tr), U._ss(oa, idx, val, tr)
            U._ss(ob, idx, val, tr)
            U._same(a, b, ("solve_sparse", k, tr))
            U._same(a, c, ("solve_sparse vs oracle", k, tr))
        j = int(rng.integers(0, m))
        cols_i = np.array(sorted(set(rng.choice(m, 3, replace=False).tolist()) | {j}), np.int64)
        cols_x = rng.standard_normal(len(cols_i)) + 2.0
        a, b, c = U._sfu(ha, [j], None, "T"), U._sfu(hb, [j], None, "T"), U._sfu(oa, [j], None, "T")
        U._sfu(ob, [j], None, "T")
        U._same(a, b, ("solve_for_update T", k))
        U._same(a, c, ("solve_for_update T vs oracle", k))
        a, b, c = U._sfu(ha, cols_i, cols_x, "N"), U._sfu(hb, cols_i, cols_x, "N"), U._sfu(oa, cols_i, cols_x, "N")
        U._sfu(ob, cols_i, cols_x, "N")
        U._same(a, b, ("solve_for_update N", k))
        U._same(a, c, ("solve_for_update N vs oracle", k))
        xtbl = a[2][j]
        sa, sb, so = ha.update(xtbl), hb.update(xtbl), oa.update(xtbl)
        assert sa == sb == so, (k, sa, sb, so)
        for tr in "NT":
            xa = ha.solve_dense(r, tr)
            assert np.array_equal(xa, hb.solve_dense(r, tr)) and np.array_equal(xa, oa.solve_dense(r, tr)), (k, tr, "after update")
        util.assert_same_getters(ha, oa, ("after update", k))


def test_device_inputs_and_aliasing(blu, oracle):
    mats = small_and_medium(oracle, 10)
    hs = [blu.BLU(len(q[0]), len(q[2])) for q in mats]
    assert all(s >= 0 for s in blu.factorize_batch(hs, mats))
    rng = np.random.default_rng(17)
    rhs = [rng.standard_normal(h.m) for h in hs]
    for tr in "NT":
        host, st = blu.solve_dense_batch(hs, rhs, tr)
        assert st == [K.OK] * len(hs)
        # device pointers, separate arrays
        dr = [DevBuf(blu, r) for r in rhs]
        dl = [DevBuf(blu, np.full(h.m, np.nan)) for h in hs]
        assert blu.solve_dense_batch(hs, trans=tr, device_ptrs=[(a.ptr, b.ptr) for a, b in zip(dr, dl)]) == [K.OK] * len(hs)
        for k in range(len(hs)):
            assert np.array_equal(dl[k].get(), host[k]), (tr, k, "device")
            assert np.array_equal(dr[k].get(), rhs[k]), (tr, k, "rhs kept")
        # device pointers, rhs is lhs
        da = [DevBuf(blu, r) for r in rhs]
        assert blu.solve_dense_batch(hs, trans=tr, device_ptrs=[(a.ptr, a.ptr) for a in da]) == [K.OK] * len(hs)
        for k in range(len(hs)):
            assert np.array_equal(da[k].get(), host[k]), (tr, k, "device aliased")
        # host arrays, rhs is lhs
        ha = [r.copy() for r in rhs]
        rc, st = raw_call(blu, hs, [a.ctypes.data for a in ha], [a.ctypes.data for a in ha], tr)
        assert rc == K.OK and st == [K.OK] * len(hs)
        for k in range(len(hs)):
            assert np.array_equal(ha[k], host[k]), (tr, k, "host aliased")


def test_refusals_leave_handles_usable(blu, oracle):
    mats = small_and_medium(oracle, 4)
    hs = [blu.BLU(len(q[0]), len(q[2])) for q in mats]
    assert all(s >= 0 for s in blu.factorize_batch(hs, mats))
    twins = [twin_of(oracle, q)[0] for q in mats]
    rng = np.random.default_rng(19)
    rhs = [rng.standard_normal(h.m) for h in hs]
    lhs = [np.zeros(h.m) for h in hs]
    rp, lp = [r.ctypes.data for r in rhs], [x.ctypes.data for x in lhs]
    E = (K.ERROR_INVALID_ARGUMENT, K.ERROR_ARGUMENT_MISSING)
    assert raw_call(blu, [hs[0], hs[1], hs[0]], rp[:3], lp[:3]) == (E[0], [E[0]] * 3)
    assert raw_call(blu, [hs[0], None], rp[:2], lp[:2]) == (E[1], [E[1]] * 2)
    assert raw_call(blu, hs[:2], [rp[0], None], lp[:2]) == (E[1], [E[1]] * 2)
    assert raw_call(blu, hs[:2], rp[:2], [lp[0], None]) == (E[1], [E[1]] * 2)
    assert raw_call(blu, hs[:2], rp[:2], lp[:2], n=0) == (K.OK, [77, 77])
    assert raw_call(blu, hs[:2], rp[:2], lp[:2], n=-1)[0] == E[1]
    L = blu.lib()
    st = (C.c_int * 2)(77, 77)
    assert L.blu_hip_solve_dense_batch(None, 2, None, None, b"N", 0, st) == E[1] and list(st) == [E[1]] * 2
    assert not any(x.any() for x in lhs)  # nothing was solved
    with pytest.raises(blu.BluError):
        blu.solve_dense_batch([hs[1], hs[1]], [rhs[1], rhs[1]])
    if blu.lib().blu_hip_device_count() >= 2:
        q = mats[0]
        other = blu.BLU(len(q[0]), len(q[2]), device=1)
        assert other.factorize(*q) >= 0
        assert raw_call(blu, [hs[0], other], [rp[0], rp[0]], [lp[0], lp[0]]) == (E[0], [E[0]] * 2)
    for tr in "NT":
        sols, st = blu.solve_dense_batch(hs, rhs, tr)
        assert st == [K.OK] * len(hs)
        for k, (h, o) in enumerate(zip(hs, twins)):
            want = o.solve_dense(rhs[k], tr)
            assert np.array_equal(sols[k], want) and np.array_equal(h.solve_dense(rhs[k], tr), want), (tr, k)


def test_at_the_benched_size(blu, oracle):
    """2304 C2-size members of 64 seeds, factorized by factorize_batch from device inputs as bench.py does; device
    right-hand sides, the same one for the members of one seed.  A stratified sample (first, last, every 67th) against
    the oracle, the 64 first members against blu_hip_solve_dense of their handle, every member against the first member
    of its seed"""
    c = CONFIGS["C2"]
    n, nseeds = 2304, 64
    mats = [blu.gen_lp_basis(c["m"], c["k"], c["bw"], c["tri_frac"], 5000 + s, c["offscale"]) for s in range(nseeds)]
    dmats = [([DevBuf(blu, a) for a in (cp[:-1].copy(), cp[1:].copy(), ri, v)], len(ri)) for cp, ri, v in mats]
    hs = [blu.BLU(c["m"], len(mats[k % nseeds][1]) // 2) for k in range(n)]
    ptrs = [tuple(a.ptr for a in dmats[k % nseeds][0]) + (dmats[k % nseeds][1],) for k in range(n)]
    assert blu.factorize_batch(hs, device_ptrs=ptrs) == [K.OK] * n
    rng = np.random.default_rng(23)
    rhs = [rng.standard_normal(c["m"]) for _ in range(nseeds)]
    drhs = [DevBuf(blu, r) for r in rhs]
    sample = sorted(set([0, n - 1] + list(range(0, n, 67))))
    assert len(sample) >= 32
    twins = {}
    dl = DevBuf(blu, n=n * c["m"])
    for tr in "NT":
        dl.put(np.full(n * c["m"], np.nan))
        st = blu.solve_dense_batch(hs, trans=tr, device_ptrs=[(drhs[k % nseeds].ptr, dl.ptr + 8 * c["m"] * k) for k in range(n)])
        assert st == [K.OK] * n
        sols = dl.get().reshape(n, c["m"])
        for k in sample:
            s = k % nseeds
            if s not in twins:
                cp, ri, v = mats[s]
                twins[s] = util.oracle_factorize(oracle, cp, ri, v, cap=16 * len(ri))[0]
            assert np.array_equal(sols[k], twins[s].solve_dense(rhs[s], tr)), (tr, k)
        for k in range(nseeds):
            assert np.array_equal(sols[k], hs[k].solve_dense(rhs[k], tr)), (tr, k)
        for k in range(nseeds, n):
            assert np.array_equal(sols[k], sols[k % nseeds]), (tr, k)
    for h in hs:
        h.close()
