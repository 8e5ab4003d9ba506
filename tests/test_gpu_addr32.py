"""The two addressings of k_pivot_loop on the MI355X (run with -m gpu).

k_pivot_loop reaches its arrays by 32-bit byte offsets off scalar bases (blu_dev.h: Arr32, RecField32, LinkField32,
ColdArr32); k_pivot_loop_w64 is the same kernel with pointers indexed in 64 bits, for storage of 4 GB and more in one
array.  The host chooses before every launch: narrow while every byte extent (statistic 151) is below BLU_ADDR32_LIMIT
(read when a handle is created; default and ceiling 2^32, 0 = always wide).  Statistic 129 tells which kernel the last
launch was, 130 how many launches of the last factorize were narrow.

Every case is compared with the CPU oracle bit for bit through the assert_identical of test_gpu_scol_run.py, on the bases
of test_gpu_small_run.py: the four RUN_SPECS narrow and wide (and the addressing must not change which path a pivot takes:
statistics 121, 122, 123, 125, 127, 128), every way out of the merged path (the lines of more than 64 entries are the
chunked loops, the only places where an index is not begin + lane), storage that runs out (every relaunch sees new bases
and capacities; once more with a limit that the growing storage crosses), every workgroup size, and the RUN_SPECS under the
self-checking build, whose accessor refuses a negative index or an offset that does not fit and reports it as a device
error."""
import os
import subprocess
import sys

import pytest

from blu_amd import keys as K
from tests.test_gpu_scol_run import assert_identical, rebuild
from tests.test_gpu_small_run import EXIT_M, EXITS, RUN_IDS, RUN_SPECS, factorize, reference, small_basis

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH_STATS = (121, 122, 123, 125, 127, 128)


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


@pytest.fixture
def limit(monkeypatch):
    """sets BLU_ADDR32_LIMIT for the handles created afterwards (None: the default)"""
    def set_limit(value):
        if value is None:
            monkeypatch.delenv("BLU_ADDR32_LIMIT", raising=False)
        else:
            monkeypatch.setenv("BLU_ADDR32_LIMIT", str(value))
    set_limit(None)
    return set_limit


@pytest.mark.parametrize("spec", RUN_SPECS, ids=RUN_IDS)
def test_runs_of_every_kind_narrow_and_wide(blu, oracle, limit, spec):
    cp, ri, v = oracle.gen_lp_basis(*spec)
    o, so = reference(oracle, "spec%r" % (spec,), cp, ri, v)
    paths = []
    for lim, wide in ((None, 0), (0, 1)):
        limit(lim)
        g, sg = factorize(blu, spec[0], cp, ri, v)
        print("spec", spec, "limit", lim, "129:", g.stat(129), "130:", g.stat(130), "paths", [g.stat(k) for k in PATH_STATS])
        assert sg == K.OK
        assert_identical(g, sg, o, so)
        assert g.stat(K.STAT_DEV_RELAUNCHES) == 1 and g.stat(118) == 0  # one launch of k_pivot_loop
        assert g.stat(129) == wide and g.stat(130) == 1 - wide
        paths.append([g.stat(k) for k in PATH_STATS])
    assert paths[0] == paths[1]  # the addressing does not change which path a pivot takes
    assert paths[0][2] > 0


@pytest.mark.parametrize("name", sorted(EXITS))
def test_every_way_out_narrow(blu, oracle, limit, name):
    make, params = EXITS[name]
    cp, ri, v = make(oracle)
    o, so = reference(oracle, name, cp, ri, v, params)
    g, sg = factorize(blu, EXIT_M, cp, ri, v, params=params)
    print(name, "status", sg, "kinds", [g.stat(51 + k) for k in range(6)], "129:", g.stat(129))
    assert_identical(g, sg, o, so)
    assert g.stat(129) == 0 and g.stat(130) == g.stat(K.STAT_DEV_RELAUNCHES)
    assert g.stat(123) > 0


def test_storage_runs_out_narrow(blu, oracle, limit):
    """hint nnz / 8: L, U and both arenas grow, every relaunch of the narrow kernel sees new bases and capacities"""
    cp, ri, v = rebuild(small_basis(oracle))
    o, so = reference(oracle, "exit-plain", cp, ri, v)
    g, sg = factorize(blu, EXIT_M, cp, ri, v, hint=len(ri) // 8)
    print("launches", g.stat(K.STAT_DEV_RELAUNCHES), "narrow", g.stat(130), "extent", g.stat(151))
    assert sg == K.OK
    assert_identical(g, sg, o, so)
    assert g.stat(K.STAT_DEV_RELAUNCHES) > 1 and g.stat(130) == g.stat(K.STAT_DEV_RELAUNCHES) and g.stat(129) == 0


def test_storage_growth_crosses_the_limit(blu, oracle, limit):
    """The same with the limit one byte above the largest extent of the handle as created, as in
    tests/test_emu_cpu_addr32.py (there 67 584 bytes for m = 300; here the slab of m = EXIT_M, read from statistic 151 of a
    handle made the same way): the arenas outgrow it, so the factorize starts narrow and ends wide."""
    cp, ri, v = rebuild(small_basis(oracle))
    o, so = reference(oracle, "exit-plain", cp, ri, v)
    e0 = int(blu.BLU(EXIT_M, len(ri) // 8).stat(151))
    assert e0 >= EXIT_M * 32
    limit(e0 + 1)
    g, sg = factorize(blu, EXIT_M, cp, ri, v, hint=len(ri) // 8)
    print("extent at creation", e0, "at the end", g.stat(151), "launches", g.stat(K.STAT_DEV_RELAUNCHES), "narrow", g.stat(130))
    assert sg == K.OK
    assert_identical(g, sg, o, so)
    assert g.stat(151) > e0 + 1
    assert g.stat(129) == 1 and 1 <= g.stat(130) < g.stat(K.STAT_DEV_RELAUNCHES)


@pytest.mark.parametrize("block", [64, 256, 512, 1024])
def test_every_workgroup_size_narrow(blu, oracle, limit, block):
    cp, ri, v = oracle.gen_lp_basis(*RUN_SPECS[0])  # all-small
    o, so = reference(oracle, "spec%r" % (RUN_SPECS[0],), cp, ri, v)
    g, sg = factorize(blu, RUN_SPECS[0][0], cp, ri, v, block=block)
    print("block", block, "129:", g.stat(129), "123:", g.stat(123))
    assert sg == K.OK
    assert_identical(g, sg, o, so)
    assert g.stat(129) == 0 and g.stat(118) == 0


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
    print("checked", spec, g.stat(54), g.stat(123), g.stat(129), g.stat(130))
    assert g.stat(129) == 0 and g.stat(130) == 1 and g.stat(123) > 0
print("self-checking build: no check fired")
"""


def test_narrow_under_the_self_checking_library(blu):
    """The four bases on libblu_hip_ewcheck.so (a child process: the library is chosen when it is loaded).  There the
    accessor of the narrow kernel replaces an index that is negative or whose byte offset does not fit in 32 bits by 0 and
    raises a device error like a failed check: status OK means that no check fired, the index check included."""
    libpath = blu.build_library(selfcheck=True)
    env = dict(os.environ, BLU_HIP_LIB=libpath)
    env.pop("BLU_ADDR32_LIMIT", None)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "self-checking build: no check fired" in text, text[-3000:]
