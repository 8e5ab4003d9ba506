"""BLU.maxvolume (blu_hip_maxvolume: k_price_multi + k_price_pick and the host side of the pass) on the GPU against the
loop blu_amd.maxvolume over the single entries -- on the CPU oracle and on a second HIP handle: after every sweep the same
status, nupdate, basis, isbasic, statistics (tests/util_maxvolume.STATS) and sparse solves, equalities only.  The loop's
traces are computed once per problem and shared by the chunk settings."""
import numpy as np
import pytest

from blu_amd import keys as K
from blu_amd.maxvolume import maxvolume as loop
from tests import util_maxvolume as MV

pytestmark = pytest.mark.gpu

_CACHE = {}


def _blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible")
    return blu_amd


def _reference(oracle, problem, max_sweeps):
    """(A, the loop's trace on the oracle, the loop's trace on a HIP handle)"""
    key = (problem, max_sweeps)
    if key not in _CACHE:
        blu_amd = _blu()
        a = MV._problem(*problem[:3])
        _CACHE[key] = (a, MV.loop_trace(MV.oracle_twin(oracle, problem[0], len(a[1])), problem, a, max_sweeps),
                       MV.loop_trace(blu_amd.BLU(problem[0], len(a[1])), problem, a, max_sweeps))
    return _CACHE[key]


@pytest.mark.parametrize("chunk", (1, 7, None), ids=("chunk1", "chunk7", "policy"))
@pytest.mark.parametrize("problem", ((30, 90, 1, 2.0), (60, 150, 2, 1.5), (96, 400, 5, 1.2)), ids=lambda p: "%dx%d" % p[:2])
def test_native_pass_is_the_loop(oracle, problem, chunk):
    """every sweep down to the one that changes nothing; chunks of 1 throw nothing away, larger ones do"""
    blu_amd = _blu()
    a, on_oracle, on_hip = _reference(oracle, problem, 40)
    g = blu_amd.BLU(problem[0], len(a[1]))
    MV.check(MV.native_trace(g, problem, a, chunk), (on_oracle, on_hip), problem, chunk)


def test_native_pass_with_growing_chunks(oracle):
    """300 x 1500 with the policy: 465 updates and 8 refactorizations in the first sweep; the second prices its 1200
    columns without a hit in chunks that grow past 64 (64, 256, 880)"""
    blu_amd = _blu()
    problem = (300, 1500, 11, 1.5)
    a, on_oracle, on_hip = _reference(oracle, problem, 2)
    g = blu_amd.BLU(problem[0], len(a[1]))
    native = MV.native_trace(g, problem, a, None, 2)
    MV.check(native, (on_oracle, on_hip), problem, None, whole=False)
    assert len(native) == 2 and native[1]["nup"] == 0 and native[1]["counts"] == (3, 1200, 0, 0), native[1]["counts"]


def test_native_pass_on_a_used_handle_and_what_follows(oracle):
    """a handle that holds an unrelated updated factorization (a pass over another A) runs the pass as its twins run the
    loop after the same history; afterwards solve_dense, solve_sparse_multi and one more pass give the twins' results"""
    blu_amd = _blu()
    problem, other = (30, 90, 1, 2.0), (30, 90, 7, 2.0)
    a, b = MV._problem(*problem[:3]), MV._problem(*other[:3])
    nz = max(len(a[1]), len(b[1]))
    g, s, o = blu_amd.BLU(30, nz), blu_amd.BLU(30, nz), MV.oracle_twin(oracle, 30, nz)
    g.dbg_set_maxvolume_chunk(5)
    runs = [(h, MV.start(30, 90)) for h in (g, s, o)]
    for h, (basis, isbasic) in runs:  # the unrelated history
        st, nup = h.maxvolume(90, b[0], b[1], b[2], basis, isbasic, 2.0) if h is g else loop(h, 90, b[0], b[1], b[2], basis, isbasic, 2.0)
        assert st == K.OK and nup > 0 and h.stat(K.STAT_NUPDATE) > 0
    g.dbg_set_maxvolume_chunk(-1)
    runs = [(h, MV.start(30, 90)) for h in (g, s, o)]
    for sweep in range(2):
        snaps = []
        for h, (basis, isbasic) in runs:
            st, nup = h.maxvolume(90, a[0], a[1], a[2], basis, isbasic, 2.0) if h is g else loop(h, 90, a[0], a[1], a[2], basis, isbasic, 2.0)
            snaps.append(MV.snapshot(h, a, st, nup, basis, isbasic))
        assert snaps[0]["st"] == K.OK and (sweep > 0 or snaps[0]["nup"] == MV.PROBLEMS[problem][0])
        MV.same_snapshot(snaps[0], snaps[1], ("used handle", sweep, "hip loop"))
        MV.same_snapshot(snaps[0], snaps[2], ("used handle", sweep, "oracle loop"))
        if sweep == 0:  # between two passes: the other entries answer with the twins' bits
            rhs = np.cos(np.arange(30.0))
            for tr in "NT":
                x = g.solve_dense(rhs, tr)
                assert np.array_equal(x, s.solve_dense(rhs, tr)) and np.array_equal(x, o.solve_dense(rhs, tr)), tr
            cols = [(a[1][int(a[0][j]):int(a[0][j + 1])], a[2][int(a[0][j]):int(a[0][j + 1])]) for j in (40, 55, 89)]
            sts, sols = g.solve_sparse_multi([c[0] for c in cols], [c[1] for c in cols], "N")
            assert sts == [K.OK] * 3
            for (ir, xr), (il, xl) in zip(cols, sols):
                for h in (s, o):
                    st, il2, lhs2 = MV._ss(h, ir, xr, "N")
                    assert st == K.OK and np.array_equal(il, il2) and np.array_equal(xl, lhs2[il2])
            for key in (K.STAT_L_FLOPS, K.STAT_U_FLOPS, K.STAT_R_FLOPS, K.STAT_UPDATE_COST):
                assert g.stat(key) == s.stat(key) == o.stat(key), key
