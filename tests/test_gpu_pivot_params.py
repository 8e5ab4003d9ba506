"""Every parameter reaches every path of the pivot kernels (run with -m gpu on an MI355X).

k_pivot_loop does not hold the parameters and capacities of the descriptor in registers: each use fetches its word from
the descriptor (blu_dev.h: ColdVal, DevGPDiet); the batch kernels hold them (DevGP).  What can go wrong silently with
either is a parameter that no longer reaches a path -- a
wrong slot, a stale copy, a copy written after its first reader.  So every parameter is moved away from its default, one at
a time, on a basis with a run of singleton columns followed by small pivots and on one with wide rows, and each result is
compared with the CPU oracle under the same parameters, bit for bit: factors, counters, pivots per routine, every
statistic (assert_identical of test_gpu_scol_run.py).  Each case runs at 1024 threads, at 256 threads (fewer than 8
waves: nothing speculative), and from a handle created with a hint of nnz / 8, which leaves the kernel with NEED_* and
launches it again.  Then one handle with three parameter sets in a row, and the nine sets through the batch kernels.

PAD and STRETCH change no factor, only how often a line is moved to the end of its arena.  The counter of those moves
(NEXPAND) depends on the storage layout and is no part of the parity with the oracle (tests/util.py:
GETTERS_NOT_COMPARED), so it is compared with itself: a line that gets more room at every move is moved at most as often,
hence moves(less room) > moves(default: PAD 4, STRETCH 0.3) > moves(more room) on the same basis, on the device and in the
oracle alike, for PAD moved alone (0, 9), for STRETCH moved alone (0.0, 1.0) and for both together.  A kernel that ignored
one of the two would give equal counts where that one is moved alone."""
import numpy as np
import pytest

from blu_amd import keys as K
from tests import util
from tests.test_gpu_scol_run import assert_identical

pytestmark = pytest.mark.gpu

BASES = {"run-then-small": (1500, 10, 9, 0.5, 1, 0.3), "wide-rows": (400, 6, 20, 0.2, 3, 1.0)}
PARAM_SETS = {
    "default": {},
    "droptol": {K.PARAM_DROPTOL: 0.02},
    "abstol": {K.PARAM_ABSTOL: 0.15},
    "reltol": {K.PARAM_RELTOL: 0.5},
    "pad0-stretch0": {K.PARAM_PAD: 0, K.PARAM_STRETCH: 0.0},
    "pad9-stretch1": {K.PARAM_PAD: 9, K.PARAM_STRETCH: 1.0},
    "maxsearch1": {K.PARAM_MAXSEARCH: 1},
    "maxsearch8": {K.PARAM_MAXSEARCH: 8},
    "nzbias0": {K.PARAM_NZBIAS: 0},
}
CHANGES_FACTORS = ("droptol", "abstol", "reltol", "maxsearch1", "maxsearch8")


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


_BASIS, _REF = {}, {}  # every basis and every reference is computed once and only read afterwards


def basis(oracle, name):
    if name not in _BASIS:
        _BASIS[name] = oracle.gen_lp_basis(*BASES[name])
    return _BASIS[name]


def reference(oracle, bname, params):
    key = (bname, tuple(sorted(params.items())))
    if key not in _REF:
        cp, ri, v = basis(oracle, bname)
        o, so = util.oracle_factorize(oracle, cp, ri, v, params=params)
        assert so == K.OK and o.d3_hits() == 0, (bname, params, so)  # (a case the oracle rejects is a defect of this file)
        _REF[key] = (o, so)
    return _REF[key]


def device_run(blu, oracle, bname, params, block=None, hint=None):
    cp, ri, v = basis(oracle, bname)
    g = blu.BLU(BASES[bname][0], hint if hint else len(ri))
    for k, val in params.items():
        g.set_param(k, val)
    if block:
        g.dbg_set_block(block)
    return g, g.factorize(cp[:-1], cp[1:], ri, v)


@pytest.mark.parametrize("pname", list(PARAM_SETS))
@pytest.mark.parametrize("bname", list(BASES))
def test_every_parameter_on_every_path(blu, oracle, bname, pname):
    params = PARAM_SETS[pname]
    o, so = reference(oracle, bname, params)
    nnz = len(basis(oracle, bname)[1])
    moves = {}
    for how, kw in (("1024", {"block": 1024}), ("256", {"block": 256}), ("relaunch", {"hint": nnz // 8})):
        g, sg = device_run(blu, oracle, bname, params, **kw)
        moves[how] = g.stat(K.STAT_NEXPAND)
        print(bname, pname, how, "status", sg, "l_nz", g.stat(K.STAT_L_NZ), "u_nz", g.stat(K.STAT_U_NZ), "launches",
              g.stat(K.STAT_DEV_RELAUNCHES), "line moves", moves[how], "(oracle %d)" % o.stat(K.STAT_NEXPAND))
        assert_identical(g, sg, o, so)
        if how == "relaunch":
            assert g.stat(K.STAT_DEV_RELAUNCHES) > 1
    if pname in CHANGES_FACTORS:  # (the case tells a kernel that ignores the parameter from one that does not)
        od, _ = reference(oracle, bname, {})
        assert (o.stat(K.STAT_L_NZ), o.stat(K.STAT_U_NZ), o.stat(K.STAT_NSEARCH_PIVOT)) != \
               (od.stat(K.STAT_L_NZ), od.stat(K.STAT_U_NZ), od.stat(K.STAT_NSEARCH_PIVOT))


# each of the two parameters moved alone, then both together: (less room, default, more room)
ROOM = {
    "pad": ({K.PARAM_PAD: 0}, {}, {K.PARAM_PAD: 9}),
    "stretch": ({K.PARAM_STRETCH: 0.0}, {}, {K.PARAM_STRETCH: 1.0}),
    "both": (PARAM_SETS["pad0-stretch0"], {}, PARAM_SETS["pad9-stretch1"]),
}


@pytest.mark.parametrize("block", [1024, 256])
@pytest.mark.parametrize("which", list(ROOM))
@pytest.mark.parametrize("bname", list(BASES))
def test_pad_and_stretch_change_how_often_lines_move(blu, oracle, bname, which, block):
    n, no = [], []
    for params in ROOM[which]:
        g, sg = device_run(blu, oracle, bname, params, block=block)
        o, so = reference(oracle, bname, params)
        assert_identical(g, sg, o, so)
        n.append(g.stat(K.STAT_NEXPAND))
        no.append(o.stat(K.STAT_NEXPAND))
    print(bname, which, block, "line moves on the device (less room, default, more room)", n, "in the oracle", no)
    assert no[0] > no[1] > no[2]
    assert n[0] > n[1] > n[2]


def test_no_copy_of_a_parameter_survives_a_launch(blu, oracle):
    """One handle, three factorizations of the same basis: DROPTOL 0.02, then DROPTOL 0, then ABSTOL 0.15 on top."""
    bname = "run-then-small"
    cp, ri, v = basis(oracle, bname)
    g = blu.BLU(BASES[bname][0], len(ri))
    have = {}
    for step in ({K.PARAM_DROPTOL: 0.02}, {K.PARAM_DROPTOL: 0.0}, {K.PARAM_ABSTOL: 0.15}):
        have.update(step)
        for k, val in step.items():
            g.set_param(k, val)
        sg = g.factorize(cp[:-1], cp[1:], ri, v)
        o, so = reference(oracle, bname, dict(have))
        print("parameters", have, "status", sg, "l_nz", g.stat(K.STAT_L_NZ), "u_nz", g.stat(K.STAT_U_NZ))
        assert_identical(g, sg, o, so)


@pytest.mark.parametrize("pname", list(PARAM_SETS))
def test_every_parameter_in_the_batch_kernels(blu, oracle, pname):
    bname, params = "wide-rows", PARAM_SETS[pname]
    cp, ri, v = basis(oracle, bname)
    o, so = reference(oracle, bname, params)
    hs = [blu.BLU(BASES[bname][0], len(ri)) for _ in range(8)]
    for h in hs:
        for k, val in params.items():
            h.set_param(k, val)
    sts = blu.factorize_batch(hs, mats=[(cp, ri, v)] * 8)
    for h, sg in zip(hs, sts):
        assert_identical(h, sg, o, so)
