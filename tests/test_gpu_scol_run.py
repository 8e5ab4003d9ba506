"""Runs of singleton-column pivots in k_pivot_loop (run with -m gpu on an MI355X).

Inside such a run the set-up of the next pivot is made during the finalize step of the current one, on a second LDS
working set, and the barrier that ends the finalize step is also the barrier after that set-up (k_pivot_fast.hip:
scol_setup_next).  Statistic 121 counts the singleton-column pivots whose search was found early, 122 those whose set-up
was made early as well.  Every case here is compared with the CPU oracle bit for bit -- the six integer arrays, the
values, the counters, the pivots per routine and every statistic of the tail -- on bases with runs of every kind and with
every way out of a run; then in lock step with the oracle, and once more under the self-checking build, which compares
each early set-up with the ordinary one inside the kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

from blu_amd import keys as K
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = ("CONDEST_L", "CONDEST_U", "NORM_L", "NORM_U", "NORMEST_L_INV", "NORMEST_U_INV", "ONENORM", "INFNORM", "RESIDUAL_TEST",
        "MIN_PIVOT", "MAX_PIVOT")
RUN_SPECS = [(2000, 8, 8, 1.0, 7, 0.3), (2000, 8, 8, 0.5, 7, 0.3), (1000, 8, 8, 0.0, 7, 0.3)]
RUN_IDS = ["one-run", "run-then-small", "no-run"]
EXIT_M = 1200  # the hand-made bases: a run of EXIT_M - 3 singleton-column pivots, disturbed in one place (EVENT)


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


_REF = {}  # name -> (oracle handle, status): every reference is computed once and only read afterwards


def reference(oracle, name, cp, ri, v):
    if name not in _REF:
        _REF[name] = util.oracle_factorize(oracle, cp, ri, v)
    return _REF[name]


def assert_identical(g, sg, o, so):
    assert sg == so, (sg, so, g.last_error())
    fg, fo = g.get_factors(), o.get_factors()
    for k in util.INT_KEYS:
        assert np.array_equal(np.asarray(fg[k], np.int64), np.asarray(fo[k], np.int64)), k
    for k in util.VAL_KEYS:
        assert np.array_equal(fg[k], fo[k]), k
    for c in util.COUNTERS:
        assert g.stat(getattr(K, "STAT_" + c)) == o.stat(getattr(K, "STAT_" + c)), c
    for kind in range(6):  # pivots per routine: singleton row, singleton column, doubleton, small, any, empty column
        assert g.stat(51 + kind) == o.stat(51 + kind), kind
    for c in TAIL:
        a, b = g.stat(getattr(K, "STAT_" + c)), o.stat(getattr(K, "STAT_" + c))
        assert a == b, (c, a, b)
    assert g.stat(50) == o.d3_hits() == 0


def rebuild(cols):
    cp, ri, v = [0], [], []
    for c in cols:
        for i in sorted(c):
            ri.append(i)
            v.append(c[i])
        cp.append(len(ri))
    return np.array(cp, np.uint64), np.array(ri, np.uint64), np.array(v)


def run_basis(oracle):
    """The basis of one long run, as a list of {row: value} per column."""
    cp, ri, v = oracle.gen_lp_basis(EXIT_M, 8, 8, 1.0, 7, 0.3)
    cp = cp.astype(np.int64)
    return [dict(zip(ri[cp[j]:cp[j + 1]].astype(np.int64).tolist(), v[cp[j]:cp[j + 1]].tolist())) for j in range(EXIT_M)]


def run_order(oracle, cols):
    """Pivot order of the undisturbed run basis: it is a permuted triangular matrix, column colperm[k] has its entries in
    rows rowperm[0..k], and pivot k of the run takes the one entry that is left of it, in row rowperm[k].  The bases below
    change it at or after position EVENT only, so the run is what it was up to there."""
    o, so = reference(oracle, "exit-plain", *rebuild(cols))
    assert so == K.OK and o.stat(52) >= EXIT_M - 5
    f = o.get_factors()
    return np.asarray(f["rowperm"], np.int64), np.asarray(f["colperm"], np.int64)


EVENT = 400


def basis_long_row(oracle):
    """Row rowperm[EVENT] filled to 70 entries, in columns that are pivotal later (the matrix stays triangular): when the
    run reaches it, the pivot row is too long for the early set-up."""
    cols = run_basis(oracle)
    rp, cq = run_order(oracle, cols)
    r = int(rp[EVENT])
    have = sum(1 for c in cols if r in c)
    rng = np.random.default_rng(70)
    later = np.array([j for j in cq[EVENT + 1:] if r not in cols[int(j)]], np.int64)
    for j in rng.choice(later, 70 - have, replace=False):
        cols[int(j)][r] = float(rng.choice((-1.0, 1.0)) * rng.uniform(0.1, 1.0))
    return rebuild(cols)


def basis_sinking_column(oracle):
    """A column that is pivotal a little later (the basis is banded in pivot order) keeps its entries of ordinary size only
    in rows that are pivotal up to position EVENT; the others are scaled by 1e-20, so its maximum falls below abstol in the middle of the run (flag_small,
    remove_col)."""
    cols = run_basis(oracle)
    rp, cq = run_order(oracle, cols)
    pinv = np.empty(EXIT_M, np.int64)
    pinv[rp] = np.arange(EXIT_M)
    j = next(int(j) for j in cq[EVENT + 3:] if sum(1 for i in cols[int(j)] if pinv[i] <= EVENT) >= 2)
    cols[j] = {i: (x if pinv[i] <= EVENT else x * 1e-20) for i, x in cols[j].items()}
    return rebuild(cols)


def basis_emptied_column(oracle):
    """Two columns with the same pattern: when one of them is the singleton pivot column (position EVENT), the other
    becomes empty."""
    cols = run_basis(oracle)
    rp, cq = run_order(oracle, cols)
    cols[int(cq[EVENT + 1])] = {i: 1.25 * x for i, x in cols[int(cq[EVENT])].items()}
    return rebuild(cols)


EXITS = {"long-row": basis_long_row, "sinking-column": basis_sinking_column, "emptied-column": basis_emptied_column}


@pytest.mark.parametrize("spec", RUN_SPECS, ids=RUN_IDS)
def test_runs_of_every_kind(blu, oracle, spec):
    cp, ri, v = oracle.gen_lp_basis(*spec)
    o, so = reference(oracle, "spec%r" % (spec,), cp, ri, v)
    g = blu.BLU(spec[0], len(ri))
    sg = g.factorize(cp[:-1], cp[1:], ri, v)
    print("spec", spec, "scol pivots", g.stat(52), "found early (121)", g.stat(121), "set up early (122)", g.stat(122))
    assert sg == K.OK
    assert_identical(g, sg, o, so)
    assert g.stat(K.STAT_DEV_RELAUNCHES) == 1 and g.stat(118) == 0  # one launch of k_pivot_loop
    if spec[3] == 0.0:
        assert g.stat(122) == 0
    else:
        assert g.stat(52) >= {1.0: 1997, 0.5: 999}[spec[3]]  # (one run of that length: the generator's triangular part)
        assert g.stat(122) >= 0.95 * g.stat(121)
        assert g.stat(121) >= 0.9 * g.stat(52)


@pytest.mark.parametrize("name", sorted(EXITS))
def test_every_way_out_of_a_run(blu, oracle, name):
    cp, ri, v = EXITS[name](oracle)
    o, so = reference(oracle, name, cp, ri, v)
    g = blu.BLU(EXIT_M, len(ri))
    sg = g.factorize(cp[:-1], cp[1:], ri, v)
    print(name, "status", sg, "scol pivots", g.stat(52), "121:", g.stat(121), "122:", g.stat(122), "rankdef", g.stat(K.STAT_RANKDEF))
    assert_identical(g, sg, o, so)
    assert o.stat(52) >= EVENT and g.stat(122) > 0  # (the run is there up to the event, and barriers were merged in it)
    if name == "long-row":
        assert sg == K.OK
        f = o.get_factors()
        urows = np.bincount(np.asarray(f["u_rowidx"], np.int64), minlength=EXIT_M)  # entries per row of U, diagonal included
        k = int(np.argmax(urows))
        assert urows[k] >= 65 and f["l_colptr"][k + 1] - f["l_colptr"][k] == 1  # a singleton-column pivot with a row of >= 65
    else:
        assert sg == K.WARNING_SINGULAR_MATRIX and g.stat(K.STAT_RANKDEF) >= 1
        if name == "emptied-column":
            assert g.stat(56) >= 1  # the empty-column step was taken


def test_u_storage_runs_out_inside_a_run(blu, oracle):
    """A handle created with a hint of nnz / 8: U fills up in the middle of the run, the kernel leaves with NEED_U and a
    pivot pending, the host grows U and launches again."""
    cp, ri, v = rebuild(run_basis(oracle))
    o, so = reference(oracle, "exit-plain", cp, ri, v)
    g = blu.BLU(EXIT_M, len(ri) // 8)
    sg = g.factorize(cp[:-1], cp[1:], ri, v)
    print("relaunches", g.stat(K.STAT_DEV_RELAUNCHES), "121:", g.stat(121), "122:", g.stat(122))
    assert sg == K.OK
    assert_identical(g, sg, o, so)
    assert g.stat(K.STAT_DEV_RELAUNCHES) > 1
    assert g.stat(122) > 0


@pytest.mark.parametrize("block", [64, 256, 512, 1024])
def test_run_at_every_workgroup_size(blu, oracle, block):
    """Fewer than 8 waves: no wave is set aside for the unlinks, nothing is searched or set up early, no barrier is merged."""
    cp, ri, v = rebuild(run_basis(oracle))
    o, so = reference(oracle, "exit-plain", cp, ri, v)
    g = blu.BLU(EXIT_M, len(ri))
    g.dbg_set_block(block)
    sg = g.factorize(cp[:-1], cp[1:], ri, v)
    print("block", block, "121:", g.stat(121), "122:", g.stat(122))
    assert sg == K.OK
    assert_identical(g, sg, o, so)
    if block < 512:
        assert g.stat(122) == 0
    else:
        assert g.stat(122) >= 0.95 * g.stat(121) > 0


@pytest.mark.parametrize("step", [1, 7, 40])
def test_run_in_lock_step_with_the_oracle(step):
    """tools/gpu_stepcheck.py stops the library every `step` pivots and compares its complete active submatrix with the
    oracle's.  step 1: every pivot is a stop, so the merged path must never run past one; step 7: stops inside the run."""
    env = dict(os.environ, BLU_PIVOT_KERNEL="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_stepcheck.py"), "1500,8,8,1.0,0.3,7", "--step", str(step)],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "FACTORS IDENTICAL" in out.stdout and "MISMATCH" not in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("ok through") >= 5


_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import blu_amd
from blu_amd import keys as K
from oracle import orc
from tests import util, test_gpu_scol_run as T
assert b"self-checking build" in blu_amd.lib().blu_hip_version()
for spec in T.RUN_SPECS:
    cp, ri, v = orc.gen_lp_basis(*spec)
    o, so = util.oracle_factorize(orc, cp, ri, v)
    g = blu_amd.BLU(spec[0], len(ri))
    sg = g.factorize(cp[:-1], cp[1:], ri, v)
    assert sg == K.OK, (spec, sg, g.last_error(), g.stat(58), g.stat(57))
    T.assert_identical(g, sg, o, so)
    print("checked", spec, g.stat(52), g.stat(121), g.stat(122))
    assert spec[3] == 0.0 or g.stat(122) >= 0.95 * g.stat(121) > 0
print("self-checking build: no check fired")
"""


def test_runs_under_the_self_checking_library(blu):
    """The first group once more on libblu_hip_ewcheck.so (a child process: the library is chosen when it is loaded).  In
    that build every early set-up is recomputed by mk_express + mk_pick before the waves go on, and a difference raises a
    device error: status OK means that no check fired."""
    libpath = blu.build_library(selfcheck=True)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], cwd=ROOT, env=dict(os.environ, BLU_HIP_LIB=libpath),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "self-checking build: no check fired" in text, text[-3000:]
