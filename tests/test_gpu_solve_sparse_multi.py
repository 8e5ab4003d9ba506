"""blu_hip_solve_sparse_multi on the MI355X (run with -m gpu): many sparse right-hand sides on ONE handle in one call, one
wave per right-hand side with a workspace of its own, the factors shared.  Every right-hand side must have the status,
pattern order and bits of the oracle's solve_sparse on a twin (an updated handle's twin is driven through the same
updates) and of the single blu_hip_solve_sparse on a second handle; the call must leave the handle as the single calls
in order would have, wherever that can be observed."""
import os

import numpy as np
import pytest

from blu_amd import keys as K
from tests import util
from tests import util_solve_sparse_multi as SM
from tests import util_update as U
from tests.util_solve_sparse_batch import BRANCH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


def golden(name):
    g = np.load(os.path.join(util.GOLDEN, name + ".npz"))
    return g["colptr"], g["rowidx"], g["values"]


def trio(blu, orc, cp, ri, v, batch=False, single=True):
    """handle of the multi calls, a second handle for the single calls and the oracle twin of one basis; batch: the first
    fresh from factorize_batch (no row-wise L yet: the transposed multi call builds it), else from a single factorize"""
    m = len(cp) - 1
    g = blu.BLU(m, len(ri))
    o = orc.OracleBLU(m, 64 * len(ri) + 1024)
    o.set_fix_d3(True)  # the 64-bit cancellation mask, as the device (defect D3)
    so = o.factorize(cp[:-1], cp[1:], ri, v)
    sg = blu.factorize_batch([g], [(cp, ri, v)])[0] if batch else g.factorize(cp[:-1], cp[1:], ri, v)
    assert sg == so and so >= 0, (sg, so)
    s = None
    if single:
        s = blu.BLU(m, len(ri))
        assert s.factorize(cp[:-1], cp[1:], ri, v) == so
    return g, s, o


@pytest.fixture(scope="module")
def m2000(blu, oracle):
    """one handle of the m = 2000 golden with its twin, shared by the tests that only solve on it"""
    g, s, o = trio(blu, oracle, *golden("lp_m2000_k8_bw8"), single=False)
    return g, o


@pytest.mark.parametrize("batch", (False, True), ids=("single", "batch"))
@pytest.mark.parametrize("name", ("lp_m200_k6_bw6", "lp_m500_k8_bw8_dense_end"))
def test_goldens_against_oracle_and_single_calls(blu, oracle, name, batch):
    """the golden bases, fresh from a single factorize and from factorize_batch (the transposed multi call then builds the
    row-wise L): nrhs 1, 3, 64 and 257 with columns of 0, 1, 5, 70 and m/2 entries in turn, both systems, SPARSE_THRES 0.0
    (sequential branch), 1.0 (symbolic branch) and the default: every column the twin's and the single-call handle's bits,
    the flop counters theirs after every call"""
    g, s, o = trio(blu, oracle, *golden(name), batch=batch)
    rng = np.random.default_rng(len(name))
    q = 0
    for thres in (0.0, 1.0, 0.05):
        SM.set_thres(thres, g, s, o)
        for tr in "TN":
            for nrhs in (1, 3, 64, 257):
                q += 1
                sts, sols = SM.check_multi(g, SM.columns(rng, g.m, nrhs, q), tr, (name, thres, nrhs), twin=o, single=s)
                assert g.dbg_sparse_multi_last_chunk() == nrhs
                if thres == 1.0:
                    assert g.stat(BRANCH) == 1, (name, nrhs, tr)
                if thres == 0.0 and len(sols[-1][0]) > 0:
                    assert g.stat(BRANCH) == 2, (name, nrhs, tr)
    assert g.lhs is None and g.nzlhs == 0


def test_many_waves_on_one_factorization(blu, m2000):
    """m = 2000, 2048 right-hand sides (unit vectors and 5-entry columns in turn) in one chunk, both systems: more
    workgroups than are resident at once, so later ones start on slots of their own while earlier ones still run.  Every
    column the twin's bits, the flop sums the twin's"""
    g, o = m2000
    g.dbg_set_sparse_multi_ws_bytes(-1)
    rng = np.random.default_rng(2000)
    for tr in "NT":
        SM.check_multi(g, SM.columns(rng, g.m, 2048, 0, sizes=(1, 5)), tr, "2048", twin=o)
        assert g.dbg_sparse_multi_last_chunk() == 2048


def test_forced_chunking(blu, m2000):
    """the byte limit set so that 7 slots fit, nrhs = 50: chunks of 7 (the last one partial) give the bits of the
    one-chunk call and of the twin"""
    g, o = m2000
    cols = SM.columns(np.random.default_rng(50), g.m, 50)
    ir, xr = [c[0] for c in cols], [c[1] for c in cols]
    try:
        for tr in "NT":
            g.dbg_set_sparse_multi_ws_bytes(-1)
            whole = g.solve_sparse_multi(ir, xr, tr)
            assert g.dbg_sparse_multi_last_chunk() == 50
            g.dbg_set_sparse_multi_ws_bytes(7 * SM.slot_bytes(g.m) + 100)
            sts, sols = g.solve_sparse_multi(ir, xr, tr)
            assert g.dbg_sparse_multi_last_chunk() == 7
            assert sts == whole[0]
            for j, (ir_j, xr_j) in enumerate(cols):
                assert np.array_equal(sols[j][0], whole[1][j][0]) and np.array_equal(sols[j][1], whole[1][j][1]), (tr, j)
                b = U._ss(o, ir_j, xr_j, tr)
                SM.same_column(g.m, sts[j], sols[j], b, ("chunked", tr, j))
                U._ss(o, ir_j, xr_j, tr)  # (the twin follows both calls: its counters stay those of the shared handle)
    finally:
        g.dbg_set_sparse_multi_ws_bytes(-1)
    for key in (K.STAT_L_FLOPS, K.STAT_U_FLOPS):
        assert g.stat(key) == o.stat(key), key


def updated_trio(blu, oracle):
    m = 300
    cp, ri, v = oracle.gen_lp_basis(m, 6, 8, 0.5, 31, 0.3)
    g, s, o = trio(blu, oracle, cp, ri, v, single=False)
    cols = U.columns_of(cp, ri, v)
    rng = np.random.default_rng(31)
    log = U.run_updates(g, cols, m, 12, rng, check_every=10 ** 9, twin=o)
    assert log["done"] >= 4 and int(g.stat(K.STAT_NUPDATE)) == log["done"] and g.stat(K.STAT_NFORREST) > 0, log
    return g, o, cols, rng, m


def test_updated_handle_in_lockstep(blu, oracle):
    """m = 300 after 12 update rounds in lock step with the twin, nrhs = 70, both systems, the three thresholds: patterns,
    values, L / U / R_FLOPS and UPDATE_COST the twin's; then 5 further lock-step rounds, every status, pattern, value and
    counter still the twin's, and every getter"""
    g, o, cols, rng, m = updated_trio(blu, oracle)
    for thres in (0.0, 1.0, 0.05):
        SM.set_thres(thres, g, o)
        for tr in "TN":
            SM.check_multi(g, SM.columns(rng, m, 70, 1), tr, ("updated", thres), twin=o)
    assert g.stat(K.STAT_R_FLOPS) > 0
    log = U.run_updates(g, cols, m, 5, rng, twin=o)
    assert log["done"] >= 1, log
    for tr in "NT":
        SM.check_multi(g, SM.columns(rng, m, 70, 2), tr, "again", twin=o)
    util.assert_same_getters(g, o, "after the multi calls on updated factors")


def test_multi_call_between_solve_for_update_and_update(blu, oracle):
    """m = 300, updated: transposed solve_for_update, forward solve_for_update, multi calls of 3 columns (the twin: the
    single solves), update -- status, PIVOT_ERROR, NFORREST, R_NZ and the sparse solves that follow are the twin's; the same
    on a fresh handle (the first update of a factorization)"""
    g, o, cols, rng, m = updated_trio(blu, oracle)
    cp, ri, v = oracle.gen_lp_basis(m, 6, 8, 0.5, 37, 0.3)
    gf, sf, of = trio(blu, oracle, cp, ri, v, single=False)
    for h, t, cl, where in ((g, o, cols, "updated"), (gf, of, U.columns_of(cp, ri, v), "fresh")):
        done = 0
        for attempt in range(20):
            j = int(rng.integers(0, m))
            ai, ax = U.new_column(rng, cl, m, j, None)
            x = h.solve_dense(SM.dense_of(m, ai, ax), "N")
            assert np.array_equal(x, t.solve_dense(SM.dense_of(m, ai, ax), "N"))
            if abs(x[j]) < 1e-3:
                continue
            if SM.between_solves_and_update(h, t, SM.columns(rng, m, 3, 1), m, j, ai, ax, (where, attempt)) == K.OK:
                cl[j] = (ai, ax)
                done = 1
                break
        assert done == 1, where
        log = U.run_updates(h, cl, m, 3, rng, twin=t)
        util.assert_same_getters(h, t, where)


@pytest.mark.parametrize("batch", (False, True), ids=("single", "batch"))
def test_handle_left_as_it_was(blu, oracle, batch):
    """after multi calls on a fresh handle: get_factors unchanged and the oracle's, every getter the oracle's; a following
    solve_sparse, a solve_dense_multi and a solve_sparse_batch that includes the handle give the twin's bits"""
    cp, ri, v = oracle.gen_lp_basis(800, 6, 8, 0.5, 33, 0.3)
    g, s, o = trio(blu, oracle, cp, ri, v, batch=batch, single=False)
    g2, s2, o2 = trio(blu, oracle, *golden("lp_m200_k6_bw6"), batch=True, single=False)
    before = g.get_factors()
    rng = np.random.default_rng(33)
    for tr in "NT":
        SM.check_multi(g, SM.columns(rng, g.m, 40), tr, "fresh", twin=o)
    after = g.get_factors()
    for key in util.INT_KEYS + util.VAL_KEYS:
        assert np.array_equal(before[key], after[key]), key
    util.assert_same_factors(after, o.get_factors())
    util.assert_same_getters(g, o, "after the multi calls")
    idx = np.sort(rng.choice(g.m, 5, replace=False))
    val = rng.standard_normal(5)
    rhs = rng.standard_normal((3, g.m))
    i2 = rng.choice(g2.m, 4, replace=False)
    v2 = rng.standard_normal(4)
    for tr in "NT":
        U._same(U._ss(g, idx, val, tr), U._ss(o, idx, val, tr), ("solve_sparse", tr))
        assert np.array_equal(g.solve_dense_multi(rhs, tr), np.array([o.solve_dense(r, tr) for r in rhs])), ("solve_dense_multi", tr)
        st = blu.solve_sparse_batch([g2, g], [i2, idx], [v2, val], tr)
        assert st == [K.OK, K.OK]
        for h, t, ir, xr in ((g2, o2, i2, v2), (g, o, idx, val)):
            U._same((K.OK, h.ilhs[:h.nzlhs].copy(), h.lhs.copy()), U._ss(t, ir, xr, tr), ("solve_sparse_batch", tr))
        SM.check_multi(g, SM.columns(rng, g.m, 10, 1), tr, "after the other entries", twin=o)
    util.assert_same_getters(g, o, "after the following calls")


def test_refusals_each_followed_by_a_successful_call(blu, oracle):
    """every refusal of the entry in the order of the header, lhs_ptr and status untouched; after each one a multi call on
    the good handle still gives the twin's bits and blu_hip_get_sparse_multi its result"""
    cp, ri, v = golden("lp_m200_k6_bw6")
    g, s, o = trio(blu, oracle, cp, ri, v, single=False)
    m = g.m
    MISS, INVARG, INVCALL = K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_ARGUMENT, K.ERROR_INVALID_CALL
    hnone = blu.BLU(120, 500)  # never factorized
    hbad = blu.BLU(m, len(ri))  # last factorize refused
    bad_i = ri.copy()
    bad_i[3] = 999
    assert hbad.factorize(cp[:-1], cp[1:], bad_i, v) == INVARG
    assert SM.raw_get(blu, g._h, 0)[0] == INVCALL  # no result held yet
    good = SM.columns(np.random.default_rng(5), m, 3, 1)
    ptr, ir, xr = [0, 1, 2], [3, 4], [1.0, 2.0]
    refusals = [
        ((None, ptr, ir, xr), {}, MISS),
        ((hnone._h, ptr, ir, xr), {}, INVCALL),
        ((hnone._h, ptr, ir, xr), dict(P=False), INVCALL),  # the factorization is checked before the pointers
        ((hbad._h, ptr, ir, xr), {}, INVCALL),
        ((g._h, ptr, ir, xr), dict(P=False), MISS),
        ((g._h, ptr, ir, xr), dict(LP=False), MISS),
        ((g._h, ptr, None, xr), {}, MISS),
        ((g._h, ptr, ir, None), {}, MISS),
        ((g._h, [2, 1, 3], None, xr), {}, MISS),            # the pointers are checked before the counts
        ((g._h, ptr, ir, xr), dict(nrhs=-1), INVARG),
        ((g._h, [0, 2, 1], ir, xr), {}, INVARG),
    ]
    for k, (args, kw, code) in enumerate(refusals):
        rc, lp, st = SM.raw_call(blu, *args, **kw)
        assert rc == code and (lp == SM.SENT).all() and (st == SM.SENT).all(), (k, rc, code, lp, st)
        sts, sols = SM.check_multi(g, good, "NT"[k % 2], (k, "after"), twin=o)
        total = sum(len(x[0]) for x in sols)
        rc, il, xl = SM.raw_get(blu, g._h, total)
        assert rc == K.OK and np.array_equal(il, np.concatenate([x[0] for x in sols])) and np.array_equal(xl, np.concatenate([x[1] for x in sols]))
    with pytest.raises(blu.BluError) as err:
        hnone.solve_sparse_multi([[1]], [[1.0]])
    assert err.value.status == INVCALL
    # per column: an index equal to m in the middle of a call whose other columns are solved
    cols = good[:1] + [(np.array([1, m]), np.ones(2))] + good[1:]
    sts, sols = g.solve_sparse_multi([c[0] for c in cols], [c[1] for c in cols], "N")
    assert sts == [K.OK, INVARG, K.OK, K.OK] and len(sols[1][0]) == 0
    for j in (0, 2, 3):
        SM.same_column(m, sts[j], sols[j], U._ss(o, cols[j][0], cols[j][1], "N"), ("mixed", j))
    for key in (K.STAT_L_FLOPS, K.STAT_U_FLOPS):
        assert g.stat(key) == o.stat(key), key
