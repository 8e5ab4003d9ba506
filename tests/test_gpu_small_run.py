"""Small pivots entered through a merged barrier in k_pivot_loop (run with -m gpu on an MI355X).

When the speculative search of the next pivot ran to its end during the finalize step of a small pivot, the same wave goes
on with the set-up of that pivot on the second LDS working set, and the barrier that ends the finalize step is also the
barrier after the set-up (k_pivot_fast.hip: small_setup_next); a column singleton that wave 0 found early is set up the
same way (scol_setup_next).  Statistic 123 counts the small pivots entered through such a barrier, statistic 125 the
singleton-column pivots entered so after a small pivot.  Every case here is compared with the CPU oracle bit for bit through
the assert_identical of test_gpu_scol_run.py, on bases with runs of every kind and with every way out of the merged path;
then in lock step with the oracle, and once more under the self-checking build, which recomputes each early set-up with the
ordinary search inside the kernel.

Pivots per routine of the oracle on the bases of the first group (singleton row, singleton column, doubleton, small, any,
empty column): (1000, 8, 8, 0.0, 7, 0.3) 1/0/1/998/0/0; (2000, 8, 8, 0.5, 7, 0.3) 1/999/1/998/0/0; (1500, 10, 9, 0.5, 1,
0.3) 1/749/1/748/0/0; (400, 6, 20, 0.2, 3, 1.0) 2/77/2/312/0/0 (its singleton rows and doubletons take the general paths in
between)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from blu_amd import keys as K
from tests import util, util_exact
from tests.test_gpu_scol_run import assert_identical, rebuild

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_SPECS = [(1000, 8, 8, 0.0, 7, 0.3), (2000, 8, 8, 0.5, 7, 0.3), (1500, 10, 9, 0.5, 1, 0.3), (400, 6, 20, 0.2, 3, 1.0)]
RUN_IDS = ["all-small", "run-then-small", "c3-like", "wide-rows"]
# share of the small pivots of the all-small basis that must be entered through the merged barrier: the first run on the
# MI355X gave SHARE_SEEN, the bound is that rounded down with a margin
SHARE_SEEN = 953 / 998
SHARE_MIN = 0.90
EXIT_M = 1200  # the hand-made bases: gen_lp_basis(EXIT_M, 8, 8, 0.0, 7, 0.3), all small pivots, disturbed at position EVENT
EVENT = 600


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


_REF = {}  # name -> (oracle handle, status): every reference is computed once and only read afterwards


def reference(oracle, name, cp, ri, v, params=None):
    if name not in _REF:
        _REF[name] = util.oracle_factorize(oracle, cp, ri, v, params=params)
    return _REF[name]


def columns(cp, ri, v):
    cp = cp.astype(np.int64)
    return [dict(zip(ri[cp[j]:cp[j + 1]].astype(np.int64).tolist(), v[cp[j]:cp[j + 1]].tolist())) for j in range(len(cp) - 1)]


def small_basis(oracle):
    """The basis of small pivots only, as a list of {row: value} per column."""
    return columns(*oracle.gen_lp_basis(EXIT_M, 8, 8, 0.0, 7, 0.3))


def pivot_order(oracle, cols):
    o, so = reference(oracle, "exit-plain", *rebuild(cols))
    assert so == K.OK and o.stat(54) >= EXIT_M - 5
    f = o.get_factors()
    return np.asarray(f["rowperm"], np.int64), np.asarray(f["colperm"], np.int64)


def basis_cancellation(oracle):
    """A tree interval basis (entries +-1, totally unimodular): elimination cancels to exactly 0.0 all the time (the oracle
    counts 12 618 cancelled entries in its 543 small pivots), so fast_fixrow runs and nothing is set up early there."""
    return util_exact.tree_interval_basis(EXIT_M, 40, 1)[:3]


def basis_sinking_column(oracle):
    """The column that is pivotal at position EVENT + 1 becomes twice the pivot column of position EVENT, one entry larger
    by 2^-48: the pivot at EVENT cancels it to that one entry, of about 1e-15, below abstol (flag_small, remove_col)."""
    cols = small_basis(oracle)
    rp, cq = pivot_order(oracle, cols)
    src = cols[int(cq[EVENT])]
    k0 = sorted(src)[0]
    cols[int(cq[EVENT + 1])] = {i: 2.0 * x * (1.0 + 2.0 ** -48 if i == k0 else 1.0) for i, x in src.items()}
    return rebuild(cols)


def basis_emptied_column(oracle):
    """Two columns with the same pattern, one twice the other: the pivot on the first cancels the second to nothing."""
    cols = small_basis(oracle)
    rp, cq = pivot_order(oracle, cols)
    cols[int(cq[EVENT + 1])] = {i: 2.0 * x for i, x in cols[int(cq[EVENT])].items()}
    return rebuild(cols)


def basis_long_row(oracle):
    """Three rows filled to 70 entries and a column (EVENT) with entries in these three rows only; with maxsearch = 1 the
    search cannot prefer another column, so the first pivot has a row of 70 and a column of 3, and the fill of the long rows
    gives small pivots with rows of 65 and more again later (positions 1044 and on in the oracle)."""
    cols = small_basis(oracle)
    rng = np.random.default_rng(65)
    for r in (300, 600, 900):
        free = np.array([j for j in range(EXIT_M) if r not in cols[j] and j != EVENT], np.int64)
        have = sum(1 for c in cols if r in c)
        for j in rng.choice(free, 70 - have, replace=False):
            cols[int(j)][r] = float(rng.choice((-1.0, 1.0)) * rng.uniform(0.1, 1.0))
    cols[EVENT] = {300: 0.9, 600: -0.8, 900: 0.7}
    return rebuild(cols)


def basis_long_column(oracle):
    """Small pivots first (a block of EXIT_M - 80 rows), then a dense block of 80 x 80 normal deviates: when the search gets
    there, every column has 80 entries -- pivot columns and rows of 65 and more, the speculative search gives up (more
    staged entries than it has room for) and the general path takes the first of them."""
    cols = columns(*oracle.gen_lp_basis(EXIT_M - 80, 8, 8, 0.0, 7, 0.3))
    rng = np.random.default_rng(66)
    for j in range(80):
        cols.append({EXIT_M - 80 + i: float(rng.normal()) for i in range(80)})
    return rebuild(cols)


EXITS = {"cancellation": (basis_cancellation, None), "sinking-column": (basis_sinking_column, None),
         "emptied-column": (basis_emptied_column, None), "long-row": (basis_long_row, {K.PARAM_MAXSEARCH: 1}),
         "long-column": (basis_long_column, None)}


def factorize(blu, m, cp, ri, v, hint=None, params=None, block=None):
    g = blu.BLU(m, hint if hint else len(ri))
    for key, val in (params or {}).items():
        g.set_param(key, val)
    if block:
        g.dbg_set_block(block)
    return g, g.factorize(cp[:-1], cp[1:], ri, v)


@pytest.mark.parametrize("spec", RUN_SPECS, ids=RUN_IDS)
def test_runs_of_every_kind(blu, oracle, spec):
    cp, ri, v = oracle.gen_lp_basis(*spec)
    o, so = reference(oracle, "spec%r" % (spec,), cp, ri, v)
    g, sg = factorize(blu, spec[0], cp, ri, v)
    print("spec", spec, "scol", g.stat(52), "small", g.stat(54), "121:", g.stat(121), "122:", g.stat(122), "merged small (123):", g.stat(123),
          "small -> scol (125):", g.stat(125), "share of small pivots %.4f" % (g.stat(123) / max(1, g.stat(54))))
    assert sg == K.OK
    assert_identical(g, sg, o, so)
    assert g.stat(K.STAT_DEV_RELAUNCHES) == 1 and g.stat(118) == 0  # one launch of k_pivot_loop
    assert g.stat(123) > 0
    if spec[3] == 0.0:
        assert g.stat(54) == 998 and g.stat(123) >= SHARE_MIN * g.stat(54)


@pytest.mark.parametrize("name", sorted(EXITS))
def test_every_way_out(blu, oracle, name):
    make, params = EXITS[name]
    cp, ri, v = make(oracle)
    o, so = reference(oracle, name, cp, ri, v, params)
    g, sg = factorize(blu, EXIT_M, cp, ri, v, params=params)
    print(name, "status", sg, "kinds", [g.stat(51 + k) for k in range(6)], "123:", g.stat(123), "125:", g.stat(125), "rankdef", g.stat(K.STAT_RANKDEF))
    assert_identical(g, sg, o, so)
    assert g.stat(123) > 0  # (barriers were merged before and after the event)
    f = o.get_factors()
    urow = np.bincount(np.asarray(f["u_rowidx"], np.int64), minlength=EXIT_M)  # entries per row of U, diagonal included
    lcol = np.diff(np.asarray(f["l_colptr"], np.int64))                        # entries per column of L, diagonal included
    if name == "cancellation":
        assert sg == K.OK and o.cancellations()["small"] > 10000 and o.stat(54) > 500
    elif name == "long-row":
        assert sg == K.OK
        assert np.count_nonzero((urow >= 65) & (lcol >= 3)) >= 10  # small pivots with a row of 65 or more
    elif name == "long-column":
        assert sg == K.OK and np.count_nonzero(lcol >= 65) >= 10 and o.stat(55) >= 10 and o.stat(54) > 1100
    else:
        assert sg == K.WARNING_SINGULAR_MATRIX and g.stat(K.STAT_RANKDEF) == 1 and o.stat(54) >= EXIT_M - 5
        assert g.stat(56) == 1  # the column went through the empty-column step in the end
        # (the sinking column keeps one entry that the emptied column loses as well)
        plain = reference(oracle, "exit-plain", *rebuild(small_basis(oracle)))[0].cancellations()["small"]
        assert o.cancellations()["small"] > plain


def test_storage_runs_out(blu, oracle):
    """A handle created with a hint of nnz / 8 (1 200 entries): L, U and the two arenas fill up among the small pivots, the
    kernel leaves with NEED_* and a pivot pending, the host grows the storage and launches again.  Seen on the MI355X: 11
    launches; L ends with 12 158 entries, U with 15 869, the column arena handed out 32 737 entries and the row arena 31 250,
    each many times the hint, so all four kinds of storage grew.  Which NEED_* ended which launch is not recorded by the
    library, nor whether a launch ended right after an early set-up's room bound had sent the pivot to the ordinary head."""
    cp, ri, v = rebuild(small_basis(oracle))
    o, so = reference(oracle, "exit-plain", cp, ri, v)
    g, sg = factorize(blu, EXIT_M, cp, ri, v, hint=len(ri) // 8)
    print("relaunches", g.stat(K.STAT_DEV_RELAUNCHES), "123:", g.stat(123), "125:", g.stat(125), "column arena used / capacity", g.stat(112), g.stat(114),
          "row arena used", g.stat(113), "L capacity", g.stat(115), "L nz", g.stat(K.STAT_L_NZ), "U nz", g.stat(K.STAT_U_NZ), "hint", len(ri) // 8)
    assert sg == K.OK
    assert_identical(g, sg, o, so)
    assert g.stat(K.STAT_DEV_RELAUNCHES) > 1
    assert g.stat(123) > 0


@pytest.mark.parametrize("block", [64, 256, 512, 1024])
def test_every_workgroup_size(blu, oracle, block):
    """Fewer than 8 waves: no wave is set aside for the unlinks, nothing is searched or set up early, no barrier is merged."""
    cp, ri, v = rebuild(small_basis(oracle))
    o, so = reference(oracle, "exit-plain", cp, ri, v)
    g, sg = factorize(blu, EXIT_M, cp, ri, v, block=block)
    print("block", block, "123:", g.stat(123), "125:", g.stat(125))
    assert sg == K.OK
    assert_identical(g, sg, o, so)
    if block < 512:
        assert g.stat(123) == 0 and g.stat(125) == 0
    else:
        assert g.stat(123) > 0


@pytest.mark.parametrize("step", [1, 7, 40])
def test_in_lock_step_with_the_oracle(step):
    """tools/gpu_stepcheck.py stops the library every `step` pivots and compares its complete active submatrix with the
    oracle's.  step 1: every pivot is a stop, so the merged path must never run past one."""
    env = dict(os.environ, BLU_PIVOT_KERNEL="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_stepcheck.py"), "1500,8,8,0.0,0.3,7", "--step", str(step)],
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
from tests import util, test_gpu_small_run as T
assert b"self-checking build" in blu_amd.lib().blu_hip_version()
for spec in T.RUN_SPECS:
    cp, ri, v = orc.gen_lp_basis(*spec)
    o, so = util.oracle_factorize(orc, cp, ri, v)
    g = blu_amd.BLU(spec[0], len(ri))
    sg = g.factorize(cp[:-1], cp[1:], ri, v)
    assert sg == K.OK, (spec, sg, g.last_error(), g.stat(58), g.stat(57))
    T.assert_identical(g, sg, o, so)
    print("checked", spec, g.stat(54), g.stat(123), g.stat(125))
    assert g.stat(123) > 0
print("self-checking build: no check fired")
"""


def test_under_the_self_checking_library(blu):
    """The first group once more on libblu_hip_ewcheck.so (a child process: the library is chosen when it is loaded).  In
    that build every early set-up is recomputed by the ordinary search and mk_pick before the waves go on, and a difference
    raises a device error: status OK means that no check fired."""
    libpath = blu.build_library(selfcheck=True)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], cwd=ROOT, env=dict(os.environ, BLU_HIP_LIB=libpath),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "self-checking build: no check fired" in text, text[-3000:]
