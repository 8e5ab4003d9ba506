"""The shared matrix and its batched products on the GPU (default library): blu_hip_share_matrix,
blu_hip_tableau_row_batch and blu_hip_price_batch -- k_scatter_lhs_batch and k_at_dot_batch -- beside clones driven by the
single entries and beside the summation order of the contract restated in numpy (tests/util_matrix.at_dot).  The drivers
of tests/util_matrix_batch.py, which tests/test_emu_cpu_matrix_batch.py runs on the CPU emulation.  Equalities of bits
only."""
import pytest

from tests import util_matrix_batch as MB

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ("M0", "M1"))
def test_share_matrix_one_matrix_many_holders(name):
    """a root and 9 children hold one matrix: every holder answers the entries that read it as a twin that called
    set_matrix itself; the holder counts beside a freed root, a set_matrix and a maxvolume of one holder; sharing into
    handles that have a matrix; copy_batch in either role; every refusal with what it leaves alone"""
    MB.check_sharing(name)


@pytest.mark.parametrize("n", MB.GROUP_SIZES)
@pytest.mark.parametrize("name", ("M0", "M1"))
def test_tableau_row_batch_is_the_single_entry_per_member(name, n):
    """n holders, clones of one root after 0 to 3 updates, rows of their own; skips None, all isbasic and mixed per member;
    prepare_update 0 and 1 (then update_batch beside update): status, bits of alpha, solution, flop statistics and later
    behaviour of the single tableau_row on a clone, alpha = at_dot of the clone's y; permuted and in chunks of one group
    the same bits; the counts of the part behind the solves"""
    MB.check_rows(name, n)


@pytest.mark.parametrize("name", ("M0", "M1"))
def test_tableau_row_batch_members_with_a_status_of_their_own(name):
    """an out-of-range row, a member without a factorization, one without a matrix: each its own status, the others their
    rows; the refusals of both batch entries as a whole; one unshared handle alone is served"""
    MB.check_rows_bad_members(name)


def test_tableau_row_batch_with_a_rank_deficient_member():
    """a member factorized on a basis with one column twice beside regular members: what the single entry gives"""
    MB.check_rows_rank_deficient()


def test_price_batch_and_the_cost_of_the_calls():
    """price_batch of 18 holders against at_dot and the single price (a random y, -0.0 and zeros, a NaN), skips None, mixed
    and all isbasic; nothing observable changes; chunked and permuted the same bits; dbg_matrix_counts of both batch entries
    independent of n within a chunk and of the matrix"""
    MB.check_pricing()
