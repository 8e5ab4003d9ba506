"""The resident constraint matrix on the GPU (blu_hip_set_matrix, _factorize_columns, _solve_for_update_column, _tableau_row,
_price: k_scatter_lhs, k_at_dot and the host side) through the default library: beside a second HIP handle driven by the
single entries, and beside the summation order of the contract restated in numpy (tests/util_matrix.at_dot) -- equalities
of bits only.  The cases of tests/test_emu_cpu_matrix.py on hardware, and one larger problem after a maxvolume pass."""
import numpy as np
import pytest

from blu_amd import keys as K
from blu_amd.maxvolume import maxvolume as loop
from tests import util_matrix as MX
from tests import util_maxvolume as MV

pytestmark = pytest.mark.gpu

NAMES = ("M0", "M1")


def _blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible")
    return blu_amd


def _pair(name, factorize=True):
    blu_amd = _blu()
    m, ncol, a = MX.MATRICES[name]()
    g, s = blu_amd.BLU(m, len(a[1])), blu_amd.BLU(m, len(a[1]))
    assert g.set_matrix(ncol, *a) == K.OK
    basis, isbasic = MV.start(m, ncol)
    if factorize:
        assert g.factorize_columns(basis) == s.factorize(*MX.gathered(a, basis)) == K.OK
    return m, ncol, a, g, s, basis, isbasic


@pytest.mark.parametrize("name", NAMES)
def test_factorize_columns_is_factorize_of_the_gathered_columns(name):
    """status, canonical factors, statistics and three solves in both systems; once more with another basis"""
    m, ncol, a, g, s, basis, isbasic = _pair(name)
    fg, fs = g.get_factors(), s.get_factors()
    for k in fg:
        assert np.array_equal(fg[k], fs[k]) and (fg[k].dtype != np.float64 or MX.same_bits(fg[k], fs[k])), k
    more = MV.STATS + (K.STAT_L_NZ, K.STAT_MIN_PIVOT, K.STAT_MAX_PIVOT, K.STAT_UPDATE_COST_DENOM, K.STAT_MATRIX_NZ, K.STAT_RANK,
                       K.STAT_BUMP_SIZE, K.STAT_BUMP_NZ, K.STAT_NSEARCH_PIVOT, K.STAT_FACTOR_FLOPS, K.STAT_CONDEST_L, K.STAT_CONDEST_U,
                       K.STAT_RESIDUAL_TEST)
    MX.same_handles(g, s, a, name, more)
    other = [j for j in range(ncol - 1, -1, -1) if a[0][j + 1] > a[0][j]][:m]
    assert g.factorize_columns(other) == s.factorize(*MX.gathered(a, other))
    MX.same_handles(g, s, a, name + ", another basis", MV.STATS + (K.STAT_L_NZ, K.STAT_RANK))


@pytest.mark.parametrize("name", NAMES)
def test_tableau_row_fresh_and_after_three_updates(name):
    """five rows with skip NULL and isbasic on fresh factors; three updates through solve_for_update_column +
    tableau_row(p, 1) + update beside the twin's single calls; five rows again; the handle equals its twin"""
    m, ncol, a, g, s, basis, isbasic = _pair(name)
    for skip in (None, isbasic):
        MX.check_tableau_rows(g, a, m, skip, (name, "fresh", skip is None), s)
    MX.update_pair(g, s, a, basis, isbasic, 3, name)
    assert g.stat(K.STAT_NUPDATE) == 3
    for skip in (None, isbasic):
        MX.check_tableau_rows(g, a, m, skip, (name, "updated", skip is None), s)
    MX.same_handles(g, s, a, (name, "after the rows"))


def test_price_and_the_cost_of_the_calls():
    """price against at_dot without and with a factorization (random y; -0.0 and zeros; a NaN; skip NULL, all ones,
    isbasic); launches and synchronizes of price and tableau_row the same for both matrices, with or without skip"""
    for name in NAMES:
        m, ncol, a, g, s, basis, isbasic = _pair(name, factorize=False)
        MX.check_price(g, a, m, isbasic, name)
        assert g.factorize_columns(basis) == K.OK
        MX.check_price(g, a, m, isbasic, name + ", factorized")
        y = MX.price_vectors(m)[0]
        for skip in (None, isbasic):
            up = 0 if skip is None else 1
            g.price(y, skip)
            assert g.dbg_matrix_counts() == (1, 1, 1 + up, 8 * ncol), (name, "price", g.dbg_matrix_counts())
            for want in (False, True):
                assert g.tableau_row(1, False, skip, want_solution=want)[0] == K.OK
                assert g.dbg_matrix_counts() == (2, 1, up, 8 * ncol), (name, "tableau_row", g.dbg_matrix_counts())


def test_tableau_rows_after_a_maxvolume_pass():
    """m = 300, ncol = 1500: one maxvolume pass changes the basis -- the native pass on the handle, the loop over the single
    entries on the twin --, the matrix is set again (the pass took it away), then five rows with skip = isbasic"""
    blu_amd = _blu()
    m, ncol, seed, tol = 300, 1500, 11, 1.5
    a = MV._problem(m, ncol, seed)
    g, s = blu_amd.BLU(m, len(a[1])), blu_amd.BLU(m, len(a[1]))
    assert g.set_matrix(ncol, *a) == K.OK
    bg, ig = MV.start(m, ncol)
    bs, is_ = MV.start(m, ncol)
    rg = g.maxvolume(ncol, a[0], a[1], a[2], bg, ig, tol)
    assert rg == loop(s, ncol, a[0], a[1], a[2], bs, is_, tol) == (K.OK, MV.PROBLEMS[(m, ncol, seed, tol)][0])
    assert bg == bs and ig == is_
    assert g.tableau_row(0, False)[0] == K.ERROR_INVALID_CALL
    assert g.set_matrix(ncol, *a) == K.OK
    for r in MX.rows_of(m):
        assert s.solve_sparse([r], [1.0], "T") == K.OK
        want = MX.at_dot(a[0], a[1], a[2], s.lhs, ig)
        st, alpha = g.tableau_row(r, False, ig, want_solution=True)
        assert st == K.OK and MX.same_bits(alpha, want), (r, np.flatnonzero(alpha != want)[:5])
        assert MX.same_solution(MX.solution(g), MX.solution(s)), r
        for key in MX.FLOPS:
            assert g.stat(key) == s.stat(key), (key, r)
    z = g.price(s.lhs, ig)
    assert MX.same_bits(z, want)
