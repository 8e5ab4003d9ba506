"""The inputs of the maxvolume tests, pinned on the CPU oracle alone (no GPU, no library): the loop blu_amd.maxvolume on
the problems of tests/util_maxvolume.py makes the basis changes and the refactorizations recorded there.  The
refactorizations driven by UPDATE_COST are what catches wrong flop accounting in the native pass -- a pass that counts a
candidate it threw away refactorizes at another moment --, so a changed generator must not quietly lose them."""
import pytest

from blu_amd import keys as K
from blu_amd.maxvolume import maxvolume
from tests import util_maxvolume as MV


@pytest.mark.parametrize("problem", sorted(MV.PROBLEMS), ids=lambda p: "%dx%d" % p[:2])
def test_first_sweep_updates_and_refactorizations_on_the_oracle(oracle, problem):
    nrow, ncol, seed, tol = problem
    a_p, a_i, a_x = MV._problem(nrow, ncol, seed)
    o = MV.oracle_twin(oracle, nrow, len(a_i))
    basis, isbasic = MV.start(nrow, ncol)
    st, nupdate = maxvolume(o, ncol, a_p, a_i, a_x, basis, isbasic, tol)
    assert st == K.OK
    assert o.stat(K.STAT_NUPDATE) >= 0 and o.stat(K.STAT_NFACTORIZE) >= 1
    assert (nupdate, int(o.stat(K.STAT_NFACTORIZE)) - 1) == MV.PROBLEMS[problem]
    assert sorted(j for j in range(ncol) if isbasic[j]) == sorted(basis)


class _Recording:
    """the oracle object with the reason of every refactorization inside a pass written down"""

    def __init__(self, o, m):
        self.o, self.m, self.reasons = o, m, []

    def factorize(self, *args):
        if self.o.stat(K.STAT_NUPDATE) > 0:  # (not the factorization at the start of a pass)
            self.reasons.append((self.o.stat(K.STAT_NFORREST) == self.m, self.o.stat(K.STAT_PIVOT_ERROR) > 1e-8, self.o.stat(K.STAT_UPDATE_COST) > 1.0))
        return self.o.factorize(*args)

    def __getattr__(self, name):
        return getattr(self.o, name)


def test_cost_driven_refactorizations_are_among_them(oracle):
    """the refactorizations of 60 x 150 and 96 x 400 are asked for by UPDATE_COST > 1 alone, that of 12 x 40 by the full eta
    file; 30 x 90 ends its first sweep just below the threshold, at 0.90"""
    reasons = {}
    for problem in sorted(MV.PROBLEMS)[:4]:
        nrow, ncol, seed, tol = problem
        a_p, a_i, a_x = MV._problem(nrow, ncol, seed)
        o = _Recording(MV.oracle_twin(oracle, nrow, len(a_i)), nrow)
        basis, isbasic = MV.start(nrow, ncol)
        assert maxvolume(o, ncol, a_p, a_i, a_x, basis, isbasic, tol)[0] == K.OK
        reasons[nrow] = o.reasons
        if nrow == 30:
            assert 0.85 < o.stat(K.STAT_UPDATE_COST) < 1.0, o.stat(K.STAT_UPDATE_COST)
    assert reasons[30] == []
    assert reasons[60] == [(False, False, True)]
    assert reasons[96] == [(False, False, True)] * 3
    assert len(reasons[12]) == 1 and reasons[12][0][0]
