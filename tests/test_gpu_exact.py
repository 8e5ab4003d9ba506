"""Exact cancellation and pivot ties on integer-valued bases (run with -m gpu on an MI355X).

The other parity tests draw continuous values, so no threshold test is ever decided at equality and elimination never
cancels to exactly 0.0.  The bases of tests/util_exact.py have entries +-1 (interval matrices: slack, network and
interval rows), or small integers: every entry of a column equals the column maximum, pivot_small and
pivot_doubleton_col take their cancellation branches all the time, pivot_any leaves stored zeros behind, a dependent
column ends with a maximum of exactly 0.0.  Every factorization is compared with the oracle (64-bit cancellation mask, as
on the device) BIT FOR BIT -- status, the six integer arrays, L and U values by bit pattern, the counters, statistics 50
and 51..56, the pivots and the statistics tail -- on every pivot kernel.  On the totally unimodular families the arithmetic
is exact, and L U = P B Q, the rank and every solve are also checked in int64 with no oracle and no tolerance.
tests/test_exact_oracle.py proves on the oracle that the committed seeds reach every branch."""
import os
import subprocess
import sys

import pytest

from blu_amd import keys as K
from tests import util_exact as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


def _kernel_env(monkeypatch, kernel):
    """BLU_PIVOT_KERNEL is read when a handle is created: set for the handles setup() sees, statistic 118 shows it held."""
    if kernel:
        monkeypatch.setenv("BLU_PIVOT_KERNEL", str(kernel))
    else:
        monkeypatch.delenv("BLU_PIVOT_KERNEL", raising=False)


SINGLE = [("default", False, 1024), ("default", False, 256), ("default", False, 64), ("default", True, 1024), ("default", True, 256),
          ("default", True, 64), ("wave", False, None), ("wave2", False, None)]
KERNEL = {"default": 0, "wave": 1, "wave2": 3}


def _setup(no_fast, block):
    def setup(g):
        g.dbg_set_no_fast(no_fast)
        if block:
            g.dbg_set_block(block)
    return setup


def test_the_inputs_reach_every_branch(oracle):
    X.honest_inputs(oracle)


@pytest.mark.parametrize("name", X.ALL_CASES)
@pytest.mark.parametrize("kernel,no_fast,block", SINGLE, ids=lambda x: str(x))
def test_every_pivot_kernel(blu, oracle, monkeypatch, kernel, no_fast, block, name):
    """k_pivot_loop with the LDS fast paths and with the general paths only, at three workgroup sizes, k_pivot_loop_wave and
    k_pivot_loop_wave2, on every committed input."""
    _kernel_env(monkeypatch, KERNEL[kernel])
    X.check_case(blu, oracle, name, setup=_setup(no_fast, block), kernel=KERNEL[kernel])


@pytest.mark.parametrize("regs", [3, 4])
def test_batch_of_all_inputs(blu, oracle, monkeypatch, regs):
    """All inputs as members of one blu_hip_factorize_batch call, with the default register budget (the `_r3` variants) and
    with BLU_PIVOT_REGS=4; statistics 118 and 120 as in test_gpu_parity.py::test_batch_of_independent_bases."""
    monkeypatch.delenv("BLU_PIVOT_KERNEL", raising=False)
    if regs == 4:
        monkeypatch.setenv("BLU_PIVOT_REGS", "4")
    else:
        monkeypatch.delenv("BLU_PIVOT_REGS", raising=False)
    X.check_batch(blu, oracle, X.ALL_CASES, regs=regs)


@pytest.mark.parametrize("kernel", ["default", "wave", "wave2"])
@pytest.mark.parametrize("params", X.EQUALITY_PARAMS, ids=X.param_id)
def test_thresholds_at_equality(blu, oracle, monkeypatch, params, kernel):
    """RELTOL 1.0 and 0.5 (`x >= reltol * cmx` with every entry equal to the column maximum), the row search with a negative
    bias, MAXSEARCH 1: tree and small-integer bases.  small-integer (300, 8) takes pivot_any at RELTOL 1.0 (asserted)."""
    _kernel_env(monkeypatch, KERNEL[kernel])
    for name in X.TREES + X.SMALLINTS:
        g, o = X.check_case(blu, oracle, name, params=params, kernel=KERNEL[kernel], solves=(name == "tree-200-10"))
        if name == "smallint-300-8" and params == {K.PARAM_RELTOL: 1.0}:
            assert g.stat(55) == o.stat(55) > 0


@pytest.mark.parametrize("kernel", ["default", "wave", "wave2"])
def test_abstol_and_droptol_at_equality(blu, oracle, monkeypatch, kernel):
    _kernel_env(monkeypatch, KERNEL[kernel])
    X.check_abstol_equality(blu, oracle)
    X.check_droptol_equality(blu, oracle)
    if kernel == "default":
        X.check_abstol_equality(blu, oracle, setup=_setup(True, 256))
        X.check_droptol_equality(blu, oracle, setup=_setup(True, 256))


@pytest.mark.parametrize("m,span", X.UPDATE_SHAPES)
def test_updates_that_stay_exact(blu, oracle, m, span):
    """150 replacements that keep a tree basis a tree basis (xtbl exactly +-1) or make it exactly singular (xtbl == 0.0,
    ERROR_SINGULAR_UPDATE, the old factorization keeps solving exactly), in lock step with the oracle twin; after every step
    both solve_for_update results and both solve_dense results are exact in integers against the current B and
    PIVOT_ERROR == 0.0.  Measured on the oracle: 126 applied and 24 exactly singular at every shape."""
    log, kinds = X.check_updates(blu, oracle, m, span, 150)
    assert log["done"] >= 100 and log["singular"] >= 10, log


def test_updates_that_stay_exact_batched(blu, oracle):
    """The same schedule (same seed: the same replacements) through solve_for_update_batch and update_batch with the three
    bases as members of one call, and solve_dense_batch / solve_sparse_batch on fresh and updated members."""
    counts = X.check_updates_batch(blu, oracle, X.UPDATE_SHAPES, 150)
    assert all(done >= 100 and singular >= 10 for done, singular in counts), counts


SELFCHECK_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import blu_amd
from oracle import orc
from tests import util_exact as X
print(blu_amd.lib().blu_hip_version().decode())
names = X.TREES + X.SMALLINTS + X.DENSES + ("zeros",)
for name in names:
    print("start", name, flush=True)
    X.check_case(blu_amd, orc, name)
    X.check_case(blu_amd, orc, name, setup=lambda g: g.dbg_set_no_fast(True), solves=False)
X.check_batch(blu_amd, orc, names)
print("all %%d exact cases identical" %% len(names))
"""


def test_slice_under_the_self_checking_library():
    """The tree, small-integer and dense-integer inputs under libblu_hip_ewcheck.so, in which the pivot loop compares every
    early and every speculative search of the next pivot with the ordinary search -- here on tied keys and stored zeros --
    and ends the factorization with an error on the first difference.  A fresh child process under a timeout."""
    import blu_amd
    libpath = blu_amd.build_library(selfcheck=True)  # (a no-op when __graft_entry__.build() has run)
    env = dict(os.environ, BLU_HIP_LIB=libpath)
    env.pop("BLU_PIVOT_KERNEL", None)
    cmd = [sys.executable, "-c", SELFCHECK_CHILD % {"root": ROOT}]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    except subprocess.TimeoutExpired as e:
        pytest.fail("self-checking slice hung; output so far: %s" % (e.stdout or b"").decode(errors="replace")[-1500:])
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-3000:]
    assert "self-checking build" in text, text[:300]  # (the child really ran on that library)
    assert "all 10 exact cases identical" in text
