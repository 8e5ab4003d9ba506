"""The statistics of factorize at every row length of B, on every path that computes them.

k_stats.hip sums a row of B by one of three code paths, chosen by its length: registers (up to 16 / 32 entries, the
workgroups of a batch), selection by repeated minimum (up to 256), and the long-row pass (more than 256: one wave per row,
the entries put in pivot order through a position-indexed array).  The reference adds a row's terms in the pivot order of
their columns (matrix_norm.rs:26-36, residual_test.rs:68-76), so INFNORM and RESIDUAL_TEST depend on that order in the last
bits.  Every basis here has one row of a prescribed length on which the storage order and the pivot order give different
sums (util.long_row_case checks that before anything runs on the GPU), and goes through the single-basis chain pipeline
(k_stats_tail_a / _b), the one-workgroup kernel (k_stats, BLU_HIP_NO_CHAIN) and the batch tail (k_stats_tail<512> and <256>,
one workgroup per matrix or two workgroups for the whole batch).  Each result must equal the oracle bit for bit and agree
with sums in exact arithmetic (math.fsum) of the same rows and columns."""
import math

import numpy as np
import pytest

from blu_amd import keys as K
from tests import util

pytestmark = pytest.mark.gpu
FSTATS = ("CONDEST_L", "CONDEST_U", "NORM_L", "NORM_U", "NORMEST_L_INV", "NORMEST_U_INV", "ONENORM", "INFNORM")
EPS = np.finfo(float).eps
CASES = [(3000, n, False) for n in (16, 17, 32, 33, 64, 65, 256, 257, 400, 1100, 3000)] + [(6000, 6000, False)] + \
        [(3000, n, True) for n in (33, 257, 1100)]


def _id(c):
    return "m%d-row%d%s" % (c[0], c[1], "-singular" if c[2] else "")


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


@pytest.fixture(scope="module")
def cases(oracle):
    return {c: util.long_row_case(oracle, c[0], c[1], 1, c[2]) for c in CASES}


def _max_sum(lines):
    """max over the lines of the exactly rounded sum of |x|, and the length of the longest line"""
    return max(math.fsum(abs(float(x)) for x in ln) for ln in lines), max(len(ln) for ln in lines)


def _near(got, want, n):
    assert abs(got - want) <= n * EPS * want, (got, want, n)


def _check(h, st, case):
    seed, (cp, ri, v), o, so = case
    m = len(cp) - 1
    assert st == so, (seed, st, so)
    fg, fo = h.get_factors(), o.get_factors()
    util.assert_same_factors(fg, fo)
    for c in util.COUNTERS:
        assert int(h.stat(getattr(K, "STAT_" + c))) == int(o.stat(getattr(K, "STAT_" + c))), c
    for c in FSTATS + ("RESIDUAL_TEST", "MIN_PIVOT", "MAX_PIVOT"):
        a, b = h.stat(getattr(K, "STAT_" + c)), o.stat(getattr(K, "STAT_" + c))
        assert a == b, (c, a, b)
    assert 0.0 < h.stat(K.STAT_RESIDUAL_TEST) < 1e-12
    # the norms against exact sums: B with its dependent columns replaced by unit columns (the matrix that was factorized),
    # rows and columns; L and U column sums (L with its unit diagonal)
    rank = int(o.stat(K.STAT_RANK))
    rows = [[] for _ in range(m)]
    colsum = []
    q = np.asarray(fg["colperm"], np.int64)
    p = np.asarray(fg["rowperm"], np.int64)
    cols = [None] * m
    for k in range(m):
        j = int(q[k])
        cols[j] = (ri[int(cp[j]):int(cp[j + 1])].astype(np.int64), v[int(cp[j]):int(cp[j + 1])]) if k < rank else \
            (np.array([p[k]]), np.array([1.0]))
    for j in range(m):
        for i, x in zip(*cols[j]):
            rows[int(i)].append(x)
        colsum.append(cols[j][1])
    _near(h.stat(K.STAT_INFNORM), *_max_sum(rows))
    _near(h.stat(K.STAT_ONENORM), *_max_sum(colsum))
    lcp, ucp = np.asarray(fg["l_colptr"], np.int64), np.asarray(fg["u_colptr"], np.int64)
    _near(h.stat(K.STAT_NORM_L), *_max_sum([fg["l_value"][lcp[k]:lcp[k + 1]] for k in range(m)]))
    _near(h.stat(K.STAT_NORM_U), *_max_sum([fg["u_value"][ucp[k]:ucp[k + 1]] for k in range(m)]))
    # the solves on these factors
    rhs = np.random.default_rng(seed).standard_normal(m)
    for trans in "NT":
        assert np.array_equal(h.solve_dense(rhs, trans), o.solve_dense(rhs, trans)), trans
    ir = np.array([m // 2, 5, m - 7], np.uint64)  # (m // 2: the long row)
    xr = np.array([1.0, -0.5, 2.0])
    for trans in "NT":
        st_o, il, lhs = o.solve_sparse(ir, xr, trans)
        assert h.solve_sparse(ir, xr, trans) == st_o == K.OK, trans
        assert np.array_equal(h.ilhs[:h.nzlhs], il) and np.array_equal(h.lhs, lhs), trans


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("path", ["chain", "nochain-1024", "nochain-128"])
def test_statistics_single_basis(blu, cases, monkeypatch, case, path):
    """one basis: the chain pipeline (k_stats_tail_a / _b; statistic 108 > 0 says k_rows_grid ran) or, with
    BLU_HIP_NO_CHAIN, the one-workgroup kernel k_stats, at two workgroup sizes of the pivot loop"""
    seed, (cp, ri, v), o, so = cases[case]
    if path != "chain":
        monkeypatch.setenv("BLU_HIP_NO_CHAIN", "1")
    h = blu.BLU(len(cp) - 1, len(ri))
    monkeypatch.delenv("BLU_HIP_NO_CHAIN", raising=False)
    if path != "chain":
        h.dbg_set_block(int(path.split("-")[1]))
    st = h.factorize(cp[:-1], cp[1:], ri, v)
    assert (h.stat(108) > 0.0) == (path == "chain")
    _check(h, st, cases[case])


@pytest.mark.parametrize("grid", [None, 2], ids=["grid-per-CU", "grid-2"])
@pytest.mark.parametrize("other", [512, 256])
def test_statistics_batch(blu, cases, monkeypatch, other, grid):
    """all the bases in one batch: k_stats (chains) then k_stats_tail<512> or <256> (rows up to 32 entries in registers),
    one workgroup per CU or two workgroups that take matrix after matrix"""
    monkeypatch.setenv("BLU_BATCH_OTHER", str(other))
    if grid:
        monkeypatch.setenv("BLU_BATCH_GRID", str(grid))
    mats = [cases[c][1] for c in CASES]
    hs = [blu.BLU(len(cp) - 1, len(ri)) for cp, ri, v in mats]
    for name in ("BLU_BATCH_OTHER", "BLU_BATCH_GRID"):
        monkeypatch.delenv(name, raising=False)
    sts = blu.blu.factorize_batch(hs, mats=mats)
    for c, h, st in zip(CASES, hs, sts):
        _check(h, st, cases[c])
