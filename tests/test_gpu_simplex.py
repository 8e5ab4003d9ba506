"""A dual simplex run as an algorithm through the device entries, on hardware with the default library, beside the exact
twin of tests/util_simplex.py: interval LPs (`tu`), the same scaled by powers of two (`tu2`) and an infeasible `tu2`
instance, on which every quantity of the iteration is an integer or a dyadic rational that a double holds exactly.  The
device therefore has to reproduce the rational-arithmetic simplex with no tolerance, iteration by iteration: the leaving
position and sigma from its x_B, the 64-byte record of ratio_test field by field, ratio_row against the twin's alpha,
lhs[r] of the FTRAN against alpha_q, get_duals behind update_duals, d and the kept row across every factorize_columns in
mid-run, d == c - A' B^-T c_B from scratch at every refactorization, and at the end status, iteration count, basis and
objective.  What keeps this from passing vacuously (enough iterations, refactorizations, every kind entering, a fixed column
leaving, both sigmas, ties decided by index and by |alpha|, winners behind column 1024) is asserted on the twin alone, and
the twin's optima against scipy's HiGHS -- the only inexact comparison in these files.

Shapes (m, extra columns): (12, 36) with 60 columns, fewer than a wave; (24, 72); (40, 120); (24, 1100) with 1148 columns,
more than the 1024 of the single pick's workgroup and no multiple of 64.  A refactorization every 5 updates."""
import pytest

from tests import util_simplex as S

pytestmark = pytest.mark.gpu


def test_the_committed_seeds_show_their_properties():
    """on the twin alone, with twin against HiGHS: a failure is a defect of tests/util_simplex.py"""
    S.committed_properties()


@pytest.mark.parametrize("m,nextra", S.SHAPES)
@pytest.mark.parametrize("family", ("tu", "tu2", "infeasible"))
def test_a_run_is_the_twins(family, m, nextra):
    """dualtol = 0, a refactorization every 5 updates; `infeasible` ends with q == -1, ncand == 0 at the twin's iteration"""
    S.check_single(family, m, nextra, 0)


def test_a_wide_run_is_the_twins():
    """1148 columns: the single pick past one stride of its workgroup"""
    S.check_single(*S.WIDE_CASE, 0)


@pytest.mark.parametrize("m,nextra", S.SHAPES)
def test_a_run_with_a_harris_tolerance_is_the_twins(m, nextra):
    """dualtol = 0.25 on `tu2`: another trajectory, not dual feasible on the way and not necessarily optimal for the LP,
    only the twin's"""
    S.check_single("tu2", m, nextra, S.HARRIS)


@pytest.mark.parametrize("family", ("tu", "tu2", "infeasible"))
def test_a_run_without_refactorizations_is_the_twins(family):
    """the eta file alone decides: ERROR_MAXIMUM_UPDATES, if it comes, is answered with a factorize_columns"""
    S.check_single(family, 24, 72, 0, every=S.NEVER)


@pytest.mark.parametrize("n", (1, 9, 17))
@pytest.mark.parametrize("family", ("tu", "tu2"))
def test_a_generation_of_forked_nodes(family, n):
    """The root solved through the single entries ends with updates behind its last refactorization; n children get that
    UPDATED factorization through copy_batch, the matrix through share_matrix, the duals through copy_duals_batch, and one
    bound of a basic variable cut past the root optimum (lower and upper cuts alternate: both sigmas in the first call).
    They iterate in lock step through solve_dense_batch, ratio_test_batch(prepare_update), solve_for_update_batch,
    update_batch and update_duals_batch, dropping out as they become optimal or infeasible, each beside a twin started
    from the root's final state and, bit for bit, beside the single entries on a clone of the root.  On `tu2` a child
    of the first nine ends infeasible; among the first hundred `tu` seeds none has such a child together with three
    different finishing iterations, so the `tu` generation has optimal children only."""
    nodes, sizes = S.run_generation(family, 24, 72, n)
    assert sizes[0] == n and (n == 1 or len(set(sizes)) >= 3), sizes
    for c in nodes:
        if c.status == "optimal":
            S.highs_agrees(c.tw)
    assert family != "tu2" or n == 1 or "infeasible" in {c.status for c in nodes}


@pytest.mark.parametrize("case,chunk_bytes", ((S.WIDE_CASE, -1), (("tu2", 24, 72), 1)), ids=("wide", "chunks-of-one-group"))
def test_a_generation_wide_and_in_chunks(case, chunk_bytes):
    """n = 9 on 1148 columns (the batched pick past several strides), and with the byte limit of the batched products set so
    that every call takes chunks of one group"""
    nodes, sizes = S.run_generation(*case, 9, chunk_bytes=chunk_bytes)
    assert sizes[0] == 9 and len(set(sizes)) >= 3, sizes
    for c in nodes:
        if c.status == "optimal":
            S.highs_agrees(c.tw)
