"""blu_hip_copy_batch / blu_hip_clone on the MI355X (run with -m gpu): k_copy_fanout copies the complete state of one
handle into n others in one launch.  A copy must be observably its source -- every parameter, every statistic key 0..124,
and from every later call the status, the pattern order and the bits -- and independent of it afterwards.  The oracle has no
clone: the twin of a copy is a fresh OracleBLU driven through the recorded history of the source (tests/util_copy.py).
Equalities only (np.array_equal / ==), over all members."""
import ctypes as C
import os

import numpy as np
import pytest

from blu_amd import keys as K
from tests import util
from tests import util_copy as CP
from tests import util_update as U

pytestmark = pytest.mark.gpu
GOLDENS = ("lp_m200_k6_bw6", "lp_m500_k8_bw8_dense_end", "lp_m2000_k8_bw8")
SOURCES = ("single", "batch")  # a single factorize leaves the chain rows behind, factorize_batch no row caches at all


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    blu_amd.lib().blu_hip_copy_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return blu_amd


def golden(name):
    g = np.load(os.path.join(util.GOLDEN, name + ".npz"))
    return g["colptr"], g["rowidx"], g["values"]


def handle(blu, mat, how="single", b_nz=None):
    cp, ri, v = mat
    g = blu.BLU(len(cp) - 1, len(ri) if b_nz is None else b_nz)
    st = blu.factorize_batch([g], [mat])[0] if how == "batch" else g.factorize(cp[:-1], cp[1:], ri, v)
    assert st == K.OK, st
    return g


def busy_handle(blu, orc, m, seed):
    """holds an UPDATED factorization of another matrix, factorized once, with a row-wise L of its own"""
    mat = orc.gen_lp_basis(m, 5, 5, 0.5, 40 + seed, 0.5)
    d = handle(blu, mat)
    assert d.solve_sparse([0], [1.0], "T") == K.OK
    cols = U.columns_of(*mat)
    log = U.run_updates(d, cols, m, 4, np.random.default_rng(seed), pair_row=CP.pair_rows(d.get_factors(), m), check_every=10 ** 9)
    assert log["done"] >= 1 and d.stat(K.STAT_NUPDATE) == log["done"] and d.stat(K.STAT_NFACTORIZE) == 1
    return d


@pytest.mark.parametrize("how", SOURCES)
@pytest.mark.parametrize("name", GOLDENS)
def test_copy_of_a_fresh_factorization(blu, oracle, name, how):
    """into a new handle with the full hint, one with b_nz = 1 (every growable array grows) and one that holds an updated
    factorization of another matrix with the same nfactorize: parameters, statistics, get_factors, the solves and the
    multi solves are the source's and the twin's; the source is unchanged"""
    mat = golden(name)
    m = len(mat[0]) - 1
    g = handle(blu, mat, how)
    o = CP.twin_of(oracle, *mat)
    dsts = [blu.BLU(m, len(mat[1])), blu.BLU(m, 1), busy_handle(blu, oracle, m, 3)]
    before = CP.state_of(g)
    assert blu.copy_batch(g, dsts) == [K.OK] * 3
    counts = g.dbg_copy_counts()
    assert counts[:3] == (1, 1, 1) and counts[3] > 0 and counts[5] == 3 * counts[4] > 0
    after = CP.state_of(g)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "the source changed"
    for k, d in enumerate(dsts):
        CP.same_state(g, d, (name, how, "destination", k))
    CP.check_members([g] + dsts, [o] + [CP.twin_of(oracle, *mat) for d in dsts], 11, (name, how))
    for k, d in enumerate(dsts):
        CP.same_state(g, d, (name, how, "destination after the solves", k))
    CP.check_members([g], [o], 12, (name, how, "the source again"))


@pytest.mark.parametrize("how", SOURCES)
@pytest.mark.parametrize("name", GOLDENS)
def test_copy_of_an_updated_factorization(blu, oracle, name, how):
    """after update rounds in lock step (25 at m = 200, 10 above), copied into 4 destinations; every member then takes up
    to 3 updates of its own beside a twin of its own, and all solve; again after the source is closed"""
    mat = golden(name)
    m = len(mat[0]) - 1
    nupd, seed = (25, 22) if m == 200 else (10, 23)
    g = handle(blu, mat, how)
    o, cols, pr, log = CP.history(oracle, mat, seed, nupd, handle=g)
    assert log["done"] >= 3 and g.stat(K.STAT_NFORREST) > 0, log
    dsts = [blu.BLU(m, len(mat[1])), blu.BLU(m, 1), busy_handle(blu, oracle, m, 4), blu.BLU(m, len(mat[1]))]
    assert blu.copy_batch(g, dsts) == [K.OK] * 4
    members, twins, colss = [g] + dsts, [o], [cols]
    for d in dsts:
        CP.same_state(g, d, (name, how))
        od, cd, _, logd = CP.history(oracle, mat, seed, nupd)
        assert logd["done"] == log["done"]
        twins.append(od)
        colss.append(cd)
    for k, (h, t, c) in enumerate(zip(members, twins, colss)):
        rng, done = np.random.default_rng(100 + k), 0
        for attempt in range(12):  # (a round whose pivot is tiny is not applied: rounds until three were)
            done += U.run_updates(h, c, m, 1, rng, pair_row=pr, twin=t)["done"]
            if done == 3:
                break
        assert done >= 1, k
    CP.check_members(members, twins, 13, (name, how, "all"))
    g.close()
    CP.check_members(dsts, twins[1:], 14, (name, how, "the source closed"))


@pytest.mark.parametrize("moment", tuple(CP.MOMENTS))
@pytest.mark.parametrize("name", GOLDENS)
def test_copy_with_a_pending_update(blu, oracle, name, moment):
    """copied after the forward solve_for_update, after the transposed one, after both (4 update rounds behind it): source
    and copy finish the update separately with the same xtbl; statuses, PIVOT_ERROR, every statistic and the solves agree"""
    mat = golden(name)
    m = len(mat[0]) - 1
    how = SOURCES[(GOLDENS.index(name) + tuple(CP.MOMENTS).index(moment)) % 2]
    g = handle(blu, mat, how)
    o, cols, pr, log = CP.history(oracle, mat, 31, 4, handle=g)
    p = CP.replacement(cols, m, np.random.default_rng(7))
    CP.advance(g, o, p, CP.MOMENTS[moment])
    d = blu.BLU(m, 1)
    assert blu.copy_batch(g, [d]) == [K.OK]
    CP.same_state(g, d, (name, moment))
    od = CP.history(oracle, mat, 31, 4)[0]
    pd = dict(p, done=[])
    CP.advance(None, od, pd, CP.MOMENTS[moment])
    sg = CP.finish(g, o, p, (name, moment, "source"))
    sd = CP.finish(d, od, pd, (name, moment, "copy"))
    assert sg == sd == K.OK and p["xtbl"] == pd["xtbl"]
    assert g.stat(K.STAT_PIVOT_ERROR) == d.stat(K.STAT_PIVOT_ERROR) == o.stat(K.STAT_PIVOT_ERROR)
    assert g.stat(K.STAT_NUPDATE) == d.stat(K.STAT_NUPDATE) == log["done"] + 1
    CP.same_state(g, d, (name, moment, "after the update"))
    CP.check_members([g, d], [o, od], 15, (name, moment))
    CP.same_state(g, d, (name, moment, "after the solves"))


def test_copy_counts(blu, oracle):
    """one launch, one synchronize, one upload for n = 1 and n = 5; a second copy into the same destinations allocates
    nothing; bytes written = n * bytes read"""
    mat = golden(GOLDENS[1])
    m = len(mat[0]) - 1
    g = handle(blu, mat)
    o, cols, pr, log = CP.history(oracle, mat, 5, 3, handle=g)
    one, five = [blu.BLU(m, 1)], [blu.BLU(m, 1 + 1000 * k) for k in range(5)]
    assert blu.copy_batch(g, one) == [K.OK]
    c1 = g.dbg_copy_counts()
    assert blu.copy_batch(g, five) == [K.OK] * 5
    c5 = g.dbg_copy_counts()
    assert c1[:3] == c5[:3] == (1, 1, 1), (c1, c5)
    assert c1[3] > 0 and c5[3] > 0 and c1[4] == c5[4] > 0 and c1[5] == c1[4] and c5[5] == 5 * c5[4]
    assert blu.copy_batch(g, five) == [K.OK] * 5
    again = g.dbg_copy_counts()
    assert again[3] == 0 and again[:3] == (1, 1, 1) and again[4:] == c5[4:], again
    for d in five + one:
        CP.same_state(g, d, "counts")
    CP.check_members([g] + five + one, [o] * 7, 18, "counts")


def test_copies_through_the_batch_entries(blu, oracle):
    """the source (from factorize_batch) and 6 copies through solve_for_update_batch (forward with 7 different columns, then
    transposed), update_batch, solve_dense_batch, solve_sparse_batch, each member beside its twin; then factorize_batch of
    all seven on new matrices"""
    mat = golden(GOLDENS[0])
    m, n = len(mat[0]) - 1, 6
    g = handle(blu, mat, "batch")
    o, cols, pr, log = CP.history(oracle, mat, 9, 5, handle=g)
    dsts = [blu.BLU(m, len(mat[1])) for k in range(n)]
    assert blu.copy_batch(g, dsts) == [K.OK] * n
    members = [g] + dsts
    twins = [o] + [CP.history(oracle, mat, 9, 5)[0] for d in dsts]
    rng = np.random.default_rng(19)
    ps = [CP.replacement(cols, m, np.random.default_rng(300 + k)) for k in range(n + 1)]
    assert len({(p["j"], tuple(p["ai"])) for p in ps}) == n + 1
    assert blu.solve_for_update_batch(members, [p["ai"] for p in ps], [p["ax"] for p in ps], "N") == [K.OK] * (n + 1)
    for h, t, p in zip(members, twins, ps):
        st, il, lhs = t.solve_for_update(p["ai"], p["ax"], "N")
        assert st == K.OK and np.array_equal(h.ilhs[:h.nzlhs], il) and np.array_equal(h.lhs, lhs)
        p["xtbl"] = lhs[p["j"]]
    assert blu.solve_for_update_batch(members, [[p["j"]] for p in ps], None, "T") == [K.OK] * (n + 1)
    for h, t, p in zip(members, twins, ps):
        st, il, lhs = t.solve_for_update([p["j"]], None, "T")
        assert st == K.OK and np.array_equal(h.ilhs[:h.nzlhs], il) and np.array_equal(h.lhs, lhs)
    assert blu.update_batch(members, [p["xtbl"] for p in ps]) == [t.update(p["xtbl"]) for t, p in zip(twins, ps)] == [K.OK] * (n + 1)
    for h, t in zip(members, twins):
        CP.same_twin_stats(h, t, "after update_batch")
    rhs = rng.standard_normal((n + 1, m))
    for tr in "NT":
        sols, sts = blu.solve_dense_batch(members, rhs, tr)
        assert sts == [K.OK] * (n + 1)
        for k, t in enumerate(twins):
            assert np.array_equal(sols[k], t.solve_dense(rhs[k], tr)), ("solve_dense_batch", tr, k)
        irs = [rng.choice(m, 1 + k, replace=False) for k in range(n + 1)]
        xrs = [rng.standard_normal(len(ir)) for ir in irs]
        assert blu.solve_sparse_batch(members, irs, xrs, tr) == [K.OK] * (n + 1)
        for k, (h, t) in enumerate(zip(members, twins)):
            st, il, lhs = t.solve_sparse(irs[k], xrs[k], tr)
            assert st == K.OK and np.array_equal(h.ilhs[:h.nzlhs], il) and np.array_equal(h.lhs, lhs), ("solve_sparse_batch", tr, k)
    for h, t in zip(members, twins):
        CP.same_twin_stats(h, t, "after the batch solves")
    mats = [oracle.gen_lp_basis(m, 5, 4, 0.6, 50 + k, 0.6) for k in range(n + 1)]
    assert blu.factorize_batch(members, mats) == [K.OK] * (n + 1)
    fresh = [CP.twin_of(oracle, *mt) for mt in mats]
    CP.check_members(members, fresh, 20, "factorize_batch after the copies", keys=CP.TWIN_STATS[:-3])  # (the totals: the handle's life)


def test_fan_out_to_seventy_destinations(blu, oracle):
    """m = 64, one source (3 update rounds behind it) and 70 destinations -- more than one group of destinations in the
    grid of k_copy_fanout --: all 70 are solved in one solve_dense_batch, each with a right-hand side of its own, against the
    twin; still one launch"""
    mat = oracle.gen_lp_basis(64, 4, 4, 0.5, 8, 0.5)
    m, n = 64, 70
    g = handle(blu, mat)
    o, cols, pr, log = CP.history(oracle, mat, 4, 3, handle=g)
    assert log["done"] >= 1
    dsts = [blu.BLU(m, len(mat[1])) for k in range(n)]
    assert blu.copy_batch(g, dsts) == [K.OK] * n
    counts = g.dbg_copy_counts()
    assert counts[:3] == (1, 1, 1) and counts[5] == n * counts[4]
    rhs = np.random.default_rng(2).standard_normal((n, m))
    for tr in "NT":
        sols, sts = blu.solve_dense_batch(dsts, rhs, tr)
        assert sts == [K.OK] * n
        for k in range(n):
            assert np.array_equal(sols[k], o.solve_dense(rhs[k], tr)), (tr, k)
    for d in dsts:
        CP.same_state(g, d, "fan-out")


def test_clone_in_a_loop(blu, oracle):
    """lp_m2000: clone() three times, each clone from the one before and the one before closed; the last still solves as the
    twin and takes an update"""
    mat = golden(GOLDENS[2])
    m = len(mat[0]) - 1
    h = handle(blu, mat)
    o, cols, pr, log = CP.history(oracle, mat, 6, 3, handle=h)
    for k in range(3):
        c = h.clone()
        assert h.dbg_copy_counts()[:3] == (1, 1, 1)
        CP.same_state(h, c, ("clone", k))
        h.close()
        h = c
    CP.check_members([h], [o], 21, "third clone")
    rng = np.random.default_rng(9)
    assert sum(U.run_updates(h, cols, m, 1, rng, pair_row=pr, twin=o)["done"] for attempt in range(6)) >= 1


def test_copy_refusals(blu, oracle):
    """the refusals of the whole call on the device, with a destination on another device where the machine has one: every
    status[k] carries the code and the destination's own factorization answers with unchanged bits"""
    mat = golden(GOLDENS[0])
    m = len(mat[0]) - 1
    g, d1 = handle(blu, mat), handle(blu, oracle.gen_lp_basis(m, 5, 5, 0.5, 9, 0.5))
    small = blu.BLU(m - 1, 8)
    rhs = np.sin(np.arange(float(m)))
    x0 = d1.solve_dense(rhs)
    state = CP.state_of(d1)

    def raw(src, dsts, n=None):
        hs = (C.c_void_p * max(len(dsts), 1))(*[None if d is None else d._h for d in dsts])
        st = (C.c_int * max(len(dsts), 1))(*([77] * max(len(dsts), 1)))
        rc = blu.lib().blu_hip_copy_batch(None if src is None else src._h, hs, len(dsts) if n is None else n, st)
        return rc, [int(s) for s in st][:len(dsts)]

    miss, inv = K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_ARGUMENT
    cases = [(miss, None, [d1]), (miss, g, [d1, None]), (inv, g, [d1, g]), (inv, g, [d1, d1]), (inv, g, [d1, small])]
    if blu.lib().blu_hip_device_count() > 1:
        cases.append((inv, g, [d1, blu.BLU(m, 8, device=1)]))
    for want, src, dsts in cases:
        assert raw(src, dsts) == (want, [want] * len(dsts)), (want, raw(src, dsts))
    assert raw(g, [d1], -1)[0] == miss and raw(g, [d1], 0) == (K.OK, [77])
    now = CP.state_of(d1)
    assert np.array_equal(now[0], state[0]) and np.array_equal(now[1], state[1])
    assert np.array_equal(d1.solve_dense(rhs), x0)
