"""The integer-valued families of tests/util_exact.py on the CPU oracle alone: the generators, the conditions that keep the
GPU tests on them honest (every cancellation branch and every pivot path is reached by the committed seeds), and the checks
that need no oracle -- the rank formula, L U = P B Q in int64, exact solves, the exact update schedule -- applied to the
oracle itself.  A disagreement between the oracle and the integer arithmetic is a finding about the oracle."""
import numpy as np
import pytest

from blu_amd import keys as K
from tests import util
from tests import util_exact as X


def test_generators_are_deterministic_and_well_formed():
    for name in X.ALL_CASES:
        cp, ri, v = X.case(name)[:3]
        m = len(cp) - 1
        assert cp.dtype == np.uint64 and ri.dtype == np.uint64 and v.dtype == np.float64 and int(cp[-1]) == len(ri) == len(v)
        for j in range(m):
            rows = ri[int(cp[j]):int(cp[j + 1])]
            assert len(set(rows.tolist())) == len(rows) and (len(rows) == 0 or int(rows.max()) < m), (name, j)
    a, b = X.tree_interval_basis(64, 6, 1), X.tree_interval_basis(64, 6, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[4] == b[4]
    assert not np.array_equal(a[2], X.tree_interval_basis(64, 6, 2)[2])
    for name in X.TREES + X.INTERVALS:
        assert set(np.abs(X.case(name)[2]).tolist()) == {1.0}, name
    for name, (m, span) in zip(X.TREES, X.TREE_SHAPES):
        edges = X.case(name)[4]
        assert len(edges) == m and X.interval_rank(m, edges) == m and max(b - a for a, b, _ in edges) <= span
    assert set(X.case("smallint-300-8")[2].tolist()) == {1.0, -1.0, 2.0, -2.0, 0.5}
    z, t = X.case("zeros"), X.case("tree-96-8")
    assert len(z[2]) == len(t[2]) + 32 and int((z[2] == 0.0).sum()) == 32
    assert np.array_equal(X.dense_int(*z[:3], 96), X.dense_int(*t[:3], 96))


def test_committed_seeds_reach_every_branch(oracle):
    counts = X.honest_inputs(oracle)
    for name, c in counts.items():
        print(name, c)


@pytest.mark.parametrize("name", X.TREES + ("zeros",))
def test_tree_bases_exact_on_the_oracle(oracle, name):
    cp, ri, v = X.case(name)[:3]
    o, st = X.oracle_run(oracle, cp, ri, v)
    B = X.exact_tree_factors(o, cp, ri, v, st, stored_zeros=(name == "zeros"))
    X.exact_solves(o, None, B, 11, name)


@pytest.mark.parametrize("name", X.INTERVALS)
def test_interval_matrices_rank_and_factors_exact_on_the_oracle(oracle, name):
    cp, ri, v, _, edges = X.case(name)
    o, st = X.oracle_run(oracle, cp, ri, v)
    assert st == K.WARNING_SINGULAR_MATRIX
    X.exact_interval_factors(o, cp, ri, v, edges, st)


@pytest.mark.parametrize("params", X.EQUALITY_PARAMS, ids=X.param_id)
def test_thresholds_at_equality_on_the_oracle(oracle, params):
    for name in X.TREES:
        cp, ri, v = X.case(name)[:3]
        o, st = X.oracle_run(oracle, cp, ri, v, params)
        X.exact_tree_factors(o, cp, ri, v, st)
    for name in X.SMALLINTS:
        cp, ri, v = X.case(name)[:3]
        o, st = X.oracle_run(oracle, cp, ri, v, params)
        assert st == K.OK
        util.check_factors(cp, ri, v, o.get_factors(), tol=1e-9)


def test_abstol_at_equality_on_the_oracle(oracle):
    """A tree basis scaled by 2^-40: with ABSTOL = 2^-40 every column maximum EQUALS abstol and `cmx < abstol` is false --
    status OK and the permutations of the unscaled basis; one ulp more and every column is below: rank 0."""
    base = X.case("tree-96-8")
    cp, ri, v = X.scaled(base, X.TWO_M40)
    o0, st0 = X.oracle_run(oracle, *base[:3])
    o, st = X.oracle_run(oracle, cp, ri, v, {K.PARAM_ABSTOL: X.TWO_M40})
    assert st == st0 == K.OK
    f, f0 = o.get_factors(), o0.get_factors()
    assert np.array_equal(f["rowperm"], f0["rowperm"]) and np.array_equal(f["colperm"], f0["colperm"])
    assert o.stat(K.STAT_MIN_PIVOT) == o.stat(K.STAT_MAX_PIVOT) == X.TWO_M40
    o, st = X.oracle_run(oracle, cp, ri, v, {K.PARAM_ABSTOL: np.nextafter(X.TWO_M40, 1.0)})
    assert st == K.WARNING_SINGULAR_MATRIX and int(o.stat(K.STAT_RANK)) == 0


def test_droptol_at_equality_on_the_oracle(oracle):
    """DROPTOL = 1.0 on entries that are all +-1: `|x| > droptol` is false at equality, so the bump keeps nothing beside
    its pivots (the singleton phases do not drop): the factors are no factorization of B any more -- parity only."""
    cp, ri, v = X.case("tree-96-8")[:3]
    o0, _ = X.oracle_run(oracle, cp, ri, v)
    o, st = X.oracle_run(oracle, cp, ri, v, {K.PARAM_DROPTOL: 1.0})
    assert st in (K.OK, K.WARNING_SINGULAR_MATRIX)
    assert o.stat(K.STAT_L_NZ) + o.stat(K.STAT_U_NZ) < o0.stat(K.STAT_L_NZ) + o0.stat(K.STAT_U_NZ)


@pytest.mark.parametrize("m,span", X.UPDATE_SHAPES)
def test_exact_update_schedule_on_the_oracle(oracle, m, span):
    cp, ri, v, rows, edges = X.tree_interval_basis(m, span, X.SEEDS["tree"])
    o, st = X.oracle_run(oracle, cp, ri, v)
    assert st == K.OK
    log, edges = X.run_exact_updates(o, None, cp, ri, v, rows, edges, span, 150, X.SCHEDULE_SEED)
    kinds = [int(o.stat(k)) for k in (K.STAT_NFORREST_TOTAL, K.STAT_NSYMPERM_TOTAL, K.STAT_DEV_NUNSYMPERM_TOTAL)]
    print((m, span), log["done"], log["singular"], kinds)
    assert log["done"] >= 100 and log["singular"] >= 10 and kinds[0] > 0 and kinds[1] + kinds[2] > 0, (log, kinds)
    assert X.interval_rank(m, edges) == m
