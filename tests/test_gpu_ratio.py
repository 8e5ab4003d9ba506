"""The ratio test on the device, on hardware with the default library: blu_hip_set_duals, _get_duals, _get_ratio_row,
_ratio_test, _update_duals, _copy_duals_batch, _ratio_test_batch and _update_duals_batch against the numpy restatements of
tests/util_ratio.py (ratio_pick, duals_step) applied to the reference alpha -- at_dot of a clone's
solve_sparse([r], [1.0], 'T') solution -- and beside clones driven by the existing single entries.  Equalities of bits
and of integers only.  Every driver runs the cases
  (a) a unique minimum ratio                      (b) equal ratios (step == 2.0 exactly) decided by |alpha|
  (c) equal ratio and |alpha|: the smallest index (the twin columns of M2)
  (d) no candidate: kind all 0, pivtol above all  (e) a dualtol that changes the winner against dualtol = 0
  (f) the winner in the first stride, in the last partial stride, at column ncol - 1
  (g) both signs of sigma, all four kinds         (h) a NaN in d on the column that would otherwise win
and asserts on the restatement that each shows its property.  M0 is 12 x 40 (fewer columns than a wave), M2 200 x 1131
(more than any workgroup, no multiple of 64, twins of short and long columns)."""
import pytest

from tests import util_ratio as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nupdates", (0, 1, 3))
@pytest.mark.parametrize("name", ("M0", "M2"))
def test_ratio_test_is_the_restatement_on_the_reference_row(name, nupdates):
    """fresh factors and after 1 to 3 updates made through ratio_test(p, prepare_update) + solve_for_update_column(q) +
    update + update_duals beside a twin driven by the existing single entries: the record, ratio_row against tableau_row's
    alpha on a fork bit for bit, the solution, the flop statistics, the later behaviour, get_duals after update_duals
    against duals_step; 3 launches, 1 synchronize, 0 uploads, 64 bytes"""
    R.check_single(name, nupdates)


@pytest.mark.parametrize("n", (1, 7, 8, 9, 17))
@pytest.mark.parametrize("name", ("M0", "M2"))
def test_ratio_test_batch_is_the_single_entry_per_member(name, n):
    """members after 0 to 3 updates with rows, sigmas, kinds and d of their own (copy_duals_batch, then set_duals): member k
    equals the restatement and the single entry on a fork; the call permuted and in chunks of one group gives the same
    records and kept rows; per chunk 3 launches, 1 synchronize, 3 uploads, 64 bytes per member; then one iteration with
    prepare_update, update_batch and update_duals_batch beside the single entries"""
    R.check_batch(name, n)


@pytest.mark.parametrize("name", ("M0", "M2"))
def test_members_with_a_status_of_their_own(name):
    """no matrix, no duals, an out-of-range row, no factorization, a bad sigma[k]; bad overrides of one member"""
    R.check_bad_members(name)


@pytest.mark.parametrize("name", ("M0", "M2"))
def test_refusals_and_the_lifetime_of_the_state(name):
    """every refusal with what it leaves alone; the state through set_matrix, share_matrix, maxvolume, copy_batch in either
    role and factorize_columns; ncol == 0"""
    R.check_refusals_and_lifetime(name)
