"""The early set-up of a small pivot on two waves, and the length of a singleton-column run (run with -m gpu on an MI355X).

After a whole speculative search the speculating wave of k_pivot_loop keeps the winner in registers, issues the load of the
pivot row, publishes the key and goes on with the row side of the set-up; wave 0 takes the column side meanwhile
(k_pivot_fast.hip: small_setup_next, small_setup_help).  The two hand over through two LDS words with bounded waits.
Statistic 127 counts the set-ups of small pivots completed on two waves -- every small pivot entered through a merged
barrier is one, so it equals statistic 123 -- and statistic 128 the hand-overs that ran into the bound of a wait, which is a
defect and 0 everywhere.  The bases, the builders and assert_identical are those of test_gpu_small_run.py and
test_gpu_scol_run.py: the smallest on which every branch of the merged path is taken, each compared with the CPU oracle bit
for bit; the references are computed once, in the cache of test_gpu_small_run.py.

Inside a run of singleton-column pivots wave 0 could issue the load of the next pivot row from registers, before it stages the
search (early_search, scol_setup_next); that was built, timed and taken out again (no gain), and its condition stays: nothing
here may shorten a run.  The library before this change gave, on an MI355X:
  (2000, 8, 8, 0.5, 7, 0.3)   statistic 121 = 998, statistic 122 = 998   (999 singleton-column pivots)
  (1500, 10, 9, 0.5, 1, 0.3)  statistic 121 = 748, statistic 122 = 748   (749 singleton-column pivots)
(PARENT_RUN below) and the library must give at least as many.  Statistics 121, 122, 123 and 125 of the change are those of
the parent on every basis of this file."""
import os
import subprocess
import sys

import pytest

from blu_amd import keys as K
from tests import test_gpu_small_run as S
from tests.test_gpu_scol_run import assert_identical, rebuild

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO, ABANDONED = K.DEVSTAT_SETUP_TWO_WAVES, K.DEVSTAT_SETUP_ABANDONED  # statistics 127 and 128
# statistics (121, 122) of the library before this change on the two bases with a singleton-column run
PARENT_RUN = {(2000, 8, 8, 0.5, 7, 0.3): (998, 998), (1500, 10, 9, 0.5, 1, 0.3): (748, 748)}


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


def show(name, g, sg):
    print(name, "status", sg, "launches", g.stat(K.STAT_DEV_RELAUNCHES), "small", g.stat(54), "scol", g.stat(52),
          " ".join("%d: %s" % (k, g.stat(k)) for k in (121, 122, 123, 125, 127, 128)))


@pytest.mark.parametrize("spec", S.RUN_SPECS, ids=S.RUN_IDS)
def test_runs_of_every_kind_on_two_waves(blu, oracle, spec):
    cp, ri, v = oracle.gen_lp_basis(*spec)
    o, so = S.reference(oracle, "spec%r" % (spec,), cp, ri, v)
    g, sg = S.factorize(blu, spec[0], cp, ri, v)
    show("spec %r" % (spec,), g, sg)
    assert sg == K.OK
    assert_identical(g, sg, o, so)
    assert g.stat(K.STAT_DEV_RELAUNCHES) == 1 and g.stat(118) == 0  # one launch of k_pivot_loop
    assert g.stat(ABANDONED) == 0
    assert g.stat(TWO) == g.stat(123) > 0
    if spec[3] == 0.0:  # the bound of test_gpu_small_run.py: the split must not lower the share of merged barriers
        assert g.stat(54) == 998 and g.stat(123) >= S.SHARE_MIN * g.stat(54)


@pytest.mark.parametrize("name", sorted(S.EXITS) + ["storage-runs-out"])
def test_every_way_out_of_the_hand_over(blu, oracle, name):
    """The ways out on which the go word must read 2, or on which the row side fails after the helper is done: a
    cancellation, a column that sinks below abstol, an emptied column, long rows and columns, and the handle whose L, U and
    arenas run out (hint nnz / 8: the kernel leaves with NEED_* and is launched again)."""
    if name == "storage-runs-out":
        cp, ri, v = rebuild(S.small_basis(oracle))
        o, so = S.reference(oracle, "exit-plain", cp, ri, v)
        g, sg = S.factorize(blu, S.EXIT_M, cp, ri, v, hint=len(ri) // 8)
        assert sg == K.OK and g.stat(K.STAT_DEV_RELAUNCHES) > 1
    else:
        make, params = S.EXITS[name]
        cp, ri, v = make(oracle)
        o, so = S.reference(oracle, name, cp, ri, v, params)
        g, sg = S.factorize(blu, S.EXIT_M, cp, ri, v, params=params)
    show(name, g, sg)
    assert_identical(g, sg, o, so)
    assert g.stat(ABANDONED) == 0


@pytest.mark.parametrize("block", [64, 256, 512, 1024])
def test_two_waves_at_every_workgroup_size(blu, oracle, block):
    """Fewer than 8 waves: nothing is speculated, nothing handed over.  With 8 or 16 the speculating wave is the last one,
    wave 7 or wave 15, and the helper wave 0."""
    cp, ri, v = rebuild(S.small_basis(oracle))
    o, so = S.reference(oracle, "exit-plain", cp, ri, v)
    g, sg = S.factorize(blu, S.EXIT_M, cp, ri, v, block=block)
    show("block %d" % block, g, sg)
    assert sg == K.OK
    assert_identical(g, sg, o, so)
    assert g.stat(ABANDONED) == 0
    if block < 512:
        assert g.stat(123) == 0 and g.stat(TWO) == 0
    else:
        assert g.stat(TWO) == g.stat(123) > 0


@pytest.mark.parametrize("spec", sorted(PARENT_RUN))
def test_the_singleton_run_is_as_long_as_before(blu, oracle, spec):
    cp, ri, v = oracle.gen_lp_basis(*spec)
    o, so = S.reference(oracle, "spec%r" % (spec,), cp, ri, v)
    g, sg = S.factorize(blu, spec[0], cp, ri, v)
    show("spec %r" % (spec,), g, sg)
    assert sg == K.OK
    assert_identical(g, sg, o, so)
    assert g.stat(121) >= PARENT_RUN[spec][0] and g.stat(122) >= PARENT_RUN[spec][1]


_CHILD = r"""
import sys
sys.path.insert(0, %r)
import blu_amd
from blu_amd import keys as K
from oracle import orc
from tests import util, test_gpu_small_run as S
assert b"self-checking build" in blu_amd.lib().blu_hip_version()
for spec in S.RUN_SPECS:
    cp, ri, v = orc.gen_lp_basis(*spec)
    o, so = util.oracle_factorize(orc, cp, ri, v)
    g = blu_amd.BLU(spec[0], len(ri))
    sg = g.factorize(cp[:-1], cp[1:], ri, v)
    assert sg == K.OK, (spec, sg, g.last_error(), g.stat(58), g.stat(57))
    S.assert_identical(g, sg, o, so)
    print("checked", spec, g.stat(54), g.stat(123), g.stat(127), g.stat(128))
    assert g.stat(127) > 0 and g.stat(128) == 0
print("self-checking build: no check fired")
"""


def test_two_waves_under_the_self_checking_library(blu):
    """The four bases on libblu_hip_ewcheck.so (a child process: the library is chosen when it is loaded).  small_setup_check
    recomputes every set-up with the ordinary search and mk_pick and compares the whole working set and both hashes -- the
    words the helper wrote among them: status OK means that no check fired."""
    libpath = blu.build_library(selfcheck=True)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], cwd=ROOT, env=dict(os.environ, BLU_HIP_LIB=libpath),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "self-checking build: no check fired" in text, text[-3000:]
