"""GPU tests of blu_hip_solve_sparse_batch (run with -m gpu).  Member k of a batch call must get exactly what
blu_hip_solve_sparse on its handle gives (tests/util_solve_sparse_batch.py): (a) a mixed batch of fresh, rank-deficient
and updated members against the CPU twin of every member and against a second set of handles driven by the single
calls, statistics included, (b) a depth-first search deeper than the LDS ring beside a small member, (c) more members
than the card holds workgroups at once, (d) the call protocol: refusals, per-member statuses, single calls between two
batch calls."""
import numpy as np
import pytest

from blu_amd import keys as K
from tests import util_solve_sparse_batch as SB
from tests import util_update as U
from tests import util_update_batch as UB
from tests.test_emu_cpu_solves import DEEP_M, DFS_RING
from tests.test_gpu_update_batch import SPECS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


def _sweep(blu, members, where):
    seen = {0.05: set(), 0.0: set(), 1.0: set()}
    for thres in seen:
        SB.set_thres(members, thres)
        for trans in "NT":
            for q in range(len(SB.SIZES)):
                seen[thres] |= SB.batch_round(blu, members, trans, q, (where, thres, trans, q))
    assert seen[0.05] == {1, 2} and 2 in seen[0.0] and seen[1.0] == {1}, seen


def test_mixed_batch_equals_the_twins_and_the_single_calls(blu, oracle):
    """(a) six members from one factorize_batch -- m = 60, 300 and 1200, a rank-deficient m = 300
    (WARNING_SINGULAR_MATRIX), the bidiagonal basis with m = 8, and an m = 60 one with at least three updates done, so
    that one call runs k_solve_sparse_batch and k_solve_upd_batch -- each with an oracle twin and a second handle driven
    by blu_hip_solve_sparse: both systems, SPARSE_THRES 0.05, 0.0 and 1.0, right-hand sides of 0, 1, 5, 70 and m/2
    entries: status, nzlhs, pattern order, values, every statistic of UB.STATS_LIBRARY and the branch taken"""
    specs = sorted(s for s in SPECS if s[0] != 5000)
    assert [s[0] for s in specs] == [60, 300, 1200]
    mats = [oracle.gen_lp_basis(*s) for s in specs]
    cp, ri, v = oracle.gen_lp_basis(300, 6, 6, 0.5, 4, 0.3)
    mats.append((cp, ri, SB.scaled(cp, v, (3, 100, 299))))
    mats.append(U.csc_arrays(UB.bidiagonal_cols(8), 8))
    mats.append(oracle.gen_lp_basis(60, 4, 5, 0.3, 17, 0.5))
    members = SB.make_members(blu, oracle, mats, [K.OK, K.OK, K.OK, K.WARNING_SINGULAR_MATRIX, K.OK, K.OK])
    SB.move_to_updated(members[-1], 8, 3)
    _sweep(blu, members, "mixed")
    assert members[-1].h.stat(K.STAT_R_FLOPS) > 0


def test_ring_wraps_in_one_workgroup_beside_a_small_member(blu, oracle):
    """(b) B = I + superdiagonal of ones with m = 2300 > DFS_RING = 2048 next to an m = 60 member: the reach of e_{m-1}
    ('N') and of e_0 ('T') is one chain of m nodes, so the first workgroup wraps its LDS ring and refills it while its
    neighbour does not; nzlhs == m, everything equal to the twins'"""
    assert DEEP_M > DFS_RING + 64
    m = DEEP_M
    mats = [U.csc_arrays(UB.bidiagonal_cols(m, 1.0), m), oracle.gen_lp_basis(*SPECS[2])]
    members = SB.make_members(blu, oracle, mats, [K.OK, K.OK])
    deep, small = members
    for thres in (0.05, 1.0):
        SB.set_thres(members, thres)
        for trans, i in (("N", m - 1), ("T", 0), ("N", m // 2)):
            rhs = [(np.array([i]), np.array([1.0])), small.rhs(5)]
            st = blu.solve_sparse_batch([deep.h, small.h], [r[0] for r in rhs], [r[1] for r in rhs], trans)
            assert st == [K.OK] * 2, st
            if i != m // 2:
                assert deep.h.nzlhs == m, (thres, trans, deep.h.nzlhs)
            for M, (ir, xr) in zip(members, rhs):
                SB.compare(M, (K.OK,) + UB.solution(M.h), ir, xr, trans, (thres, trans, i, M.m))


N_MANY = 1600
MANY_SPECS = [(24, 4, 4, 0.0, 5, 0.5), (37, 4, 5, 0.3, 11, 0.5), (48, 5, 4, 0.8, 13, 0.6), (60, 4, 5, 0.3, 7, 0.5), (60, 6, 6, 0.5, 19, 0.3)]


def test_more_members_than_resident_workgroups(blu, oracle):
    """(c) 1600 handles (DfsRing allows 6 one-wave workgroups per CU: 1536 on 256 CUs) on five distinct matrices of
    m <= 60, factorized in one factorize_batch, every member with its own right-hand side of 1 to 6 entries: both
    systems, each member's pattern, values and flop counters equal to what the oracle twin of its matrix gives for that
    right-hand side (blockIdx indexing, packed right-hand-side offsets, gather offsets).  Of its 10 s on the MI355X 7.4 s
    are the creation and release of the 1600 handles (2.3 ms each way); the factorization takes 0.12 s, a batch call
    8-50 ms and the 3200 oracle solves 0.03 s"""
    mats = [oracle.gen_lp_basis(*s) for s in MANY_SPECS]
    twins = []
    for cp, ri, v in mats:
        o = oracle.OracleBLU(len(cp) - 1, 64 * len(ri) + 1024)
        o.set_fix_d3(True)
        assert o.factorize(cp[:-1], cp[1:], ri, v) == K.OK
        twins.append(o)
    which = [k % len(mats) for k in range(N_MANY)]
    hs = [blu.BLU(len(mats[w][0]) - 1, len(mats[w][1])) for w in which]
    assert blu.factorize_batch(hs, [mats[w] for w in which]) == [K.OK] * N_MANY
    rng = np.random.default_rng(1600)
    flops = np.zeros((N_MANY, 2))
    for trans in "NT":
        rhs = []
        for h in hs:
            nz = int(rng.integers(1, 7))
            rhs.append((rng.choice(h.m, nz, replace=False), rng.standard_normal(nz)))
        st = blu.solve_sparse_batch(hs, [r[0] for r in rhs], [r[1] for r in rhs], trans)
        assert st == [K.OK] * N_MANY
        for k, (h, (ir, xr)) in enumerate(zip(hs, rhs)):
            o = twins[which[k]]
            before = np.array([o.stat(K.STAT_L_FLOPS), o.stat(K.STAT_U_FLOPS)])
            U._same((K.OK,) + UB.solution(h), U._ss(o, ir, xr, trans), (trans, k))
            flops[k] += np.array([o.stat(K.STAT_L_FLOPS), o.stat(K.STAT_U_FLOPS)]) - before
            assert [h.stat(K.STAT_L_FLOPS), h.stat(K.STAT_U_FLOPS)] == list(flops[k]), (trans, k)


def test_call_protocol_and_single_calls_between_batches(blu, oracle):
    """(d) the refusals of the whole call (every status carries the code, n == 0 writes nothing, no handle touched), the
    per-member statuses of a mixed call ([OK, INVALID_CALL, OK, INVALID_ARGUMENT, INVALID_ARGUMENT], return value
    min(status), status NULL accepted), and single solve_sparse / solve_dense / solve_for_update / update calls on two
    members between two batch calls: marker, zero invariants and the row-wise L built by the batch are the single
    entry's"""
    mats = [oracle.gen_lp_basis(*SPECS[2]), oracle.gen_lp_basis(*SPECS[0]), oracle.gen_lp_basis(60, 4, 5, 0.3, 27, 0.5)]
    members = SB.make_members(blu, oracle, mats, [K.OK] * 3)
    SB.refusals(blu, members)
    SB.move_to_updated(members[2], 8, 3)
    for trans in "TN":
        for q in range(len(SB.SIZES)):
            SB.batch_round(blu, members, trans, q, ("before", trans, q))
    for k in (1, 2):
        SB.move_to_updated(members[k], 6, 1)
    for trans in "NT":
        for q in range(len(SB.SIZES)):
            SB.batch_round(blu, members, trans, q, ("after", trans, q))
    SB.mixed_statuses(blu, oracle)
