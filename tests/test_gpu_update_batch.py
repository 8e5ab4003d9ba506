"""GPU tests of blu_hip_solve_for_update_batch and blu_hip_update_batch (run with -m gpu): many bases kept in lock step,
each round a batched transposed solve_for_update, a batched forward one and a batched update, with a changing member
set (tests/util_update_batch.py).  Member k of a batch call must get exactly what the single call on its handle gives:
(a) against the CPU twin of every member, (b) against a second set of handles driven by the single calls, statistics
and flop counters included, (c) with more members than the card holds workgroups at once, (d) through the storage
requests of a tiny arena, ERROR_MAXIMUM_UPDATES, ERROR_SINGULAR_UPDATE and the call protocol."""
import ctypes as C

import numpy as np
import pytest

from blu_amd import keys as K
from tests import util_update as U
from tests import util_update_batch as UB

pytestmark = pytest.mark.gpu

# the four bases of tests/test_gpu_update.py::test_update_sequence_in_lockstep_with_the_cpu_twin ...
SPECS = [(300, 6, 6, 0.5, 1, 0.3), (1200, 8, 8, 0.5, 3, 0.3), (60, 4, 5, 0.3, 7, 0.5), (5000, 10, 9, 0.5, 2, 0.3)]
EXTRA_SEEDS = (0, 10, 20)  # ... each with its own generator seed and two more
TINY_SPEC = (24, 4, 4, 0.0, 5, 0.5)
ROUNDS_MIXED = 40
# the bounds of that test (and of test_maximum_updates_and_storage_growth for the tiny-arena member)
MAX_RESIDUAL, MAX_RESIDUAL_TINY, MAX_PIVOT_ERROR = 1e-8, 1e-7, 1e-8


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


def mixed_bases(gen_lp_basis):
    """(columns, b_nz hint or None, arena slack or None, script) of the members of the mixed batch"""
    out = []
    for spec in SPECS:
        for ds in EXTRA_SEEDS:
            out.append((U.columns_of(*gen_lp_basis(*(spec[:4] + (spec[4] + ds,) + spec[5:]))), None, None, ()))
    out.append((UB.bidiagonal_cols(8), None, None, UB.BIDIAGONAL_SCRIPT))
    out.append((U.columns_of(*gen_lp_basis(*TINY_SPEC)), 4, 8, ()))
    return out


def _handles(blu, bases):
    hs = []
    for cols, b_nz, extra, _ in bases:
        h = blu.BLU(len(cols), sum(len(c[0]) for c in cols) if b_nz is None else b_nz)
        if extra is not None:
            h.dbg_set_upd_extra(extra)  # forces UPD_NEED_R / NEED_UC / NEED_W round trips
        hs.append(h)
    mats = [U.csc_arrays(cols, len(cols)) for cols, _, _, _ in bases]
    assert blu.factorize_batch(hs, mats) == [K.OK] * len(hs)
    return hs


def _oracle_twin(oracle, cols):
    m, nz = len(cols), sum(len(c[0]) for c in cols)
    o = oracle.OracleBLU(m, 256 * nz + 1024)
    o.set_fix_d3(True)
    cp, ri, v = U.csc_arrays(cols, m)
    assert o.factorize(cp[:-1], cp[1:], ri, v) == K.OK
    return o


def _single_twin(blu, cols, b_nz, extra):
    m = len(cols)
    h = blu.BLU(m, sum(len(c[0]) for c in cols) if b_nz is None else b_nz)
    if extra is not None:
        h.dbg_set_upd_extra(extra)
    cp, ri, v = U.csc_arrays(cols, m)
    assert h.factorize(cp[:-1], cp[1:], ri, v) == K.OK
    return h


def _members(hs, twins, bases, seed0):
    return [UB.Member(h, t, [(i.copy(), x.copy()) for i, x in cols], seed0 + k, pair_row=UB.pair_rows(h), script=script)
            for k, (h, t, (cols, _, _, script)) in enumerate(zip(hs, twins, bases))]


def _bounds(members):
    for k, M in enumerate(members):
        tiny = M.m == TINY_SPEC[0]
        assert M.max_residual <= (MAX_RESIDUAL_TINY if tiny else MAX_RESIDUAL), (k, M.m, M.max_residual)
        assert M.max_pivot_error <= MAX_PIVOT_ERROR, (k, M.m, M.max_pivot_error)


def test_mixed_batch_in_lockstep_with_the_cpu_twins(blu, oracle):
    """(a) fourteen members -- the four bases of the single-handle lock-step test with three generator seeds each, the
    bidiagonal basis with its two hand-predictable permutation updates, and a member with a b_nz hint of 4 and 8 entries
    of arena slack -- for 40 rounds, each with an oracle twin: every status, pattern, value and statistic identical;
    Forrest-Tomlin, symmetric and unsymmetric permutation updates all occur (the twins alone reach that: they were run
    on the CPU for the same 40 rounds, totals 363 / 29 / 8); backward errors within the bounds of the single-handle test."""
    bases = mixed_bases(oracle.gen_lp_basis)
    hs = _handles(blu, bases)
    members = _members(hs, [_oracle_twin(oracle, b[0]) for b in bases], bases, 1000)
    for r in range(ROUNDS_MIXED):
        UB.lockstep_round(blu, members, where=r)
        if r == 1:
            assert members[-2].done == 2 and [members[-2].h.stat(key) for key in UB.KINDS] == [0, 1, 1]
    got = UB.kinds(members)
    print("kinds", got, "done", [M.done for M in members], "skipped", [M.skipped for M in members], "singular", [M.singular for M in members])
    assert (got > 0).all() and np.array_equal(got, UB.kinds(members, lambda M: M.twin)), got
    assert all(M.h.stat(K.STAT_NUPDATE) == M.done for M in members)
    assert sum(M.done for M in members) >= 0.5 * ROUNDS_MIXED * len(members)
    UB.dense_after(blu, members, 5)
    _bounds(members)


def test_batch_equals_the_single_calls(blu):
    """(b) two sets of handles on the same bases, one driven by the batch entries, the other by blu_hip_solve_for_update
    and blu_hip_update: every status, pattern, value and statistic equal after every update, NFORREST_TOTAL, L_FLOPS,
    U_FLOPS, R_FLOPS and UPDATE_COST included"""
    bases = mixed_bases(blu.gen_lp_basis)
    hs = _handles(blu, bases)
    twins = [_single_twin(blu, cols, b_nz, extra) for cols, b_nz, extra, _ in bases]
    members = _members(hs, twins, bases, 2000)
    for r in range(15):
        UB.lockstep_round(blu, members, stats=UB.STATS_LIBRARY, where=r)
    assert UB.kinds(members)[0] > 0 and sum(M.done for M in members) >= 7 * len(members)
    for M in members:
        for key in UB.STATS_LIBRARY + (K.STAT_DEV_NUNSYMPERM_TOTAL, 43):
            assert M.h.stat(key) == M.twin.stat(key), (key, M.m)
    UB.dense_after(blu, members, 6)
    _bounds(members)


N_MANY, M_MANY, SAMPLE_MANY, ROUNDS_MANY = 2048, 200, 64, 3


def test_more_members_than_resident_workgroups(blu, oracle):
    """(c) 2048 distinct bases of m = 200 (DfsRing allows 6 workgroups of k_solve_upd_batch per CU: 1536 on 256 CUs) for
    three rounds: every transposed and forward solve OK with a rounding-level backward error and a consistent pattern,
    every update OK or ERROR_SINGULAR_UPDATE with NUPDATE counting the former; 64 members chosen by a fixed seed have
    oracle twins and match them bit for bit"""
    colsets = [U.columns_of(*oracle.gen_lp_basis(M_MANY, 6, 6, 0.5, 7000 + k, 0.3)) for k in range(N_MANY)]
    bases = [(cols, None, None, ()) for cols in colsets]
    hs = _handles(blu, bases)
    sample = set(int(k) for k in np.random.default_rng(64).choice(N_MANY, SAMPLE_MANY, replace=False))
    assert len(sample) == SAMPLE_MANY
    twins = [_oracle_twin(oracle, colsets[k]) if k in sample else None for k in range(N_MANY)]
    members = [UB.Member(h, t, cols, 3000 + k) for k, (h, t, cols) in enumerate(zip(hs, twins, colsets))]
    for r in range(ROUNDS_MANY):
        st_t, st_n, st_u = UB.lockstep_round(blu, members, where=r)
        assert st_t == [K.OK] * N_MANY and st_n == [K.OK] * N_MANY and set(st_u) <= {K.OK, K.ERROR_SINGULAR_UPDATE}
    assert all(M.h.stat(K.STAT_NUPDATE) == M.done for M in members)
    assert sum(M.done for M in members) >= 0.5 * ROUNDS_MANY * N_MANY
    UB.dense_after(blu, members, 7)
    _bounds(members)


def test_growth_maximum_updates_and_protocol(blu, oracle):
    """(d) the tiny-arena member (storage requests inside the batch) run to ERROR_MAXIMUM_UPDATES beside a member that goes
    on; ERROR_SINGULAR_UPDATE leaves the member solvable; the per-member statuses of a mixed call, prepare-only calls
    and the refusals of the whole call"""
    bases = [(U.columns_of(*oracle.gen_lp_basis(*TINY_SPEC)), 4, 8, ()), (U.columns_of(*oracle.gen_lp_basis(*SPECS[2])), None, None, ())]
    hs = _handles(blu, bases)
    members = _members(hs, [_oracle_twin(oracle, b[0]) for b in bases], bases, 105)
    st_t = None
    for r in range(400):
        st_t, _, _ = UB.lockstep_round(blu, members, where=r)
        if members[0].maxed:
            break
    assert members[0].maxed and st_t == [K.ERROR_MAXIMUM_UPDATES, K.OK] and hs[0].stat(K.STAT_NFORREST) == TINY_SPEC[0], (st_t, r)
    UB.lockstep_round(blu, members, where="after")
    UB.dense_after(blu, members, 8)
    _bounds(members)

    # ---- protocol (tests/test_gpu_update.py::test_update_call_protocol), one mixed call each
    MISS, INVARG, INVCALL = K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_ARGUMENT, K.ERROR_INVALID_CALL
    cp, ri, v = oracle.gen_lp_basis(200, 5, 5, 0.5, 2, 0.3)
    hp, hrange = blu.BLU(200, len(ri)), blu.BLU(200, len(ri))
    op = oracle.OracleBLU(200, 64 * len(ri))
    assert hp.factorize(cp[:-1], cp[1:], ri, v) == hrange.factorize(cp[:-1], cp[1:], ri, v) == op.factorize(cp[:-1], cp[1:], ri, v) == K.OK
    hnone, hz = blu.BLU(120, 500), blu.BLU(0, 1)
    e = np.zeros(0, np.uint64)
    assert hz.factorize(e, e, e, np.zeros(0)) == K.OK
    mixed = [hp, hnone, hz, hrange]
    assert blu.update_batch(mixed, [1.0] * 4) == [INVCALL] * 4                                   # nothing prepared
    assert blu.solve_for_update_batch(mixed, [[3], [3], [0], [200]], None, "T", want_solution=False) == [K.OK, INVCALL, INVARG, INVARG]
    assert op.solve_for_update([3], None, "T", want_solution=False)[0] == K.OK and hp.nzlhs == 0  # prepare only
    assert blu.update_batch(mixed, [1.0] * 4) == [INVCALL] * 4                                   # forward solve missing
    a, b = int(cp[4]), int(cp[5])
    st = blu.solve_for_update_batch(mixed, [ri[a:b], [1], [0], [1, 999]], [v[a:b], [1.0], [1.0], [1.0, 2.0]], "N")
    assert st == [K.OK, INVCALL, INVARG, INVARG], st
    U._same((st[0],) + UB.solution(hp), op.solve_for_update(ri[a:b], v[a:b], "N"), "column 4")
    assert abs(hp.lhs[3]) < 1e-12
    st = blu.update_batch(mixed, [hp.lhs[3], 1.0, 1.0, 1.0])
    assert st == [K.ERROR_SINGULAR_UPDATE] + [INVCALL] * 3 and op.update(hp.lhs[3]) == K.ERROR_SINGULAR_UPDATE, st
    b1 = np.ones(200)
    assert np.array_equal(hp.solve_dense(b1), op.solve_dense(b1))  # the old factorization is still valid
    sols, st = blu.solve_dense_batch([hp, hrange], [b1, b1])
    assert st == [K.OK] * 2 and np.array_equal(sols[0], sols[1])

    # ---- refusals of the whole call: every status carries the code, no handle is touched
    L = blu.lib()
    FN, FU = L.blu_hip_solve_for_update_batch, L.blu_hip_update_batch
    FN.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_char, C.c_void_p]
    FU.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    i3, x3 = np.array([3], np.uint64), np.array([1.0])
    ip, xp = i3.ctypes.data, x3.ctypes.data
    two = [hp._h, hrange._h]

    def vp(xs):
        return (C.c_void_p * len(xs))(*xs)

    def sfu(H, n, nz, ir, xr, trans):
        s = (C.c_int * 3)(77, 77, 77)
        return FN(H, n, nz, ir, xr, None, None, None, trans, s), list(s)[:max(n, 0)]

    nz2 = (C.c_int64 * 3)(1, 1, 1)
    before = [h.stat(K.STAT_NUPDATE) for h in (hp, hrange)], hp.stat(K.STAT_L_FLOPS), hp.stat(K.STAT_U_FLOPS)
    assert sfu(None, 2, nz2, vp([ip, ip]), None, b"T") == (MISS, [MISS] * 2)
    assert sfu(vp(two), 2, nz2, None, None, b"T") == (MISS, [MISS] * 2)
    assert sfu(vp([two[0], None]), 2, nz2, vp([ip, ip]), None, b"T") == (MISS, [MISS] * 2)
    assert sfu(vp(two), 2, nz2, vp([ip, None]), None, b"T") == (MISS, [MISS] * 2)
    assert sfu(vp(two), 2, nz2, vp([ip, ip]), None, b"N") == (MISS, [MISS] * 2)
    assert sfu(vp(two), 2, nz2, vp([ip, ip]), vp([xp, None]), b"N") == (MISS, [MISS] * 2)
    assert sfu(vp(two), 2, None, vp([ip, ip]), vp([xp, xp]), b"N") == (MISS, [MISS] * 2)
    assert sfu(vp(two), -1, nz2, vp([ip, ip]), None, b"T")[0] == MISS
    assert sfu(vp(two + two[:1]), 3, nz2, vp([ip] * 3), None, b"T") == (INVARG, [INVARG] * 3)
    assert sfu(vp(two), 0, nz2, vp([ip, ip]), None, b"T") == (K.OK, [])
    xt, s2 = (C.c_double * 2)(1.0, 1.0), (C.c_int * 2)(77, 77)
    assert FU(None, 2, xt, s2) == MISS and list(s2) == [MISS] * 2
    assert FU(vp(two), 2, None, s2) == MISS and list(s2) == [MISS] * 2
    assert FU(vp([two[0], None]), 2, xt, s2) == MISS and list(s2) == [MISS] * 2
    assert FU(vp([two[0], two[0]]), 2, xt, s2) == INVARG and list(s2) == [INVARG] * 2
    assert FU(vp(two), -1, xt, s2) == MISS and FU(vp(two), 0, xt, s2) == K.OK
    assert before == ([h.stat(K.STAT_NUPDATE) for h in (hp, hrange)], hp.stat(K.STAT_L_FLOPS), hp.stat(K.STAT_U_FLOPS))
    with pytest.raises(blu.BluError):
        blu.solve_for_update_batch([hp, hp], [[1], [1]], None, "T")
    with pytest.raises(blu.BluError):
        blu.update_batch([hp, hp], [1.0, 1.0])
