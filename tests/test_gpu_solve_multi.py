"""blu_hip_solve_dense_multi on the MI355X (run with -m gpu): many right-hand sides on ONE handle in one call, one wave
per right-hand side, the factors shared.  Every column must have the bits of the oracle's solve_dense on a twin (an
updated handle's twin is driven through the same updates); the call must leave the handle where ONE blu_hip_solve_dense
call would have: the row-wise L kept, the pivot sequence compacted once, the marker advanced once."""
import ctypes as C
import os

import numpy as np
import pytest

from blu_amd import keys as K
from tests import util
from tests import util_update as U

pytestmark = pytest.mark.gpu
SENT = -7.25e300
GOLDENS = ("lp_m200_k6_bw6", "lp_m500_k8_bw8_dense_end", "lp_m2000_k8_bw8")


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    blu_amd.lib().blu_hip_solve_dense_multi.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_char, C.c_int]
    return blu_amd


def golden(name):
    g = np.load(os.path.join(util.GOLDEN, name + ".npz"))
    return g["colptr"], g["rowidx"], g["values"]


def pair(blu, orc, cp, ri, v, batch=False):
    """device handle and oracle twin of one basis; batch: fresh from factorize_batch (no row-wise L yet: the forward
    multi-solve builds it), else from a single factorize"""
    m = len(cp) - 1
    g = blu.BLU(m, len(ri))
    o = orc.OracleBLU(m, 64 * len(ri) + 1024)
    o.set_fix_d3(True)  # the 64-bit cancellation mask, as the device (defect D3)
    so = o.factorize(cp[:-1], cp[1:], ri, v)
    sg = blu.factorize_batch([g], [(cp, ri, v)])[0] if batch else g.factorize(cp[:-1], cp[1:], ri, v)
    assert sg == so and so >= 0, (sg, so)
    return g, o


def oracle_columns(o, rhs, tr):
    return np.array([o.solve_dense(r, tr) for r in rhs]).reshape(rhs.shape)


def stride_of(m):
    return (m + 2 + 31) // 32 * 32


class DevBuf:
    """float64 array in device memory (hipMalloc of the HIP runtime the library is linked with)"""

    def __init__(self, blu, a):
        self.hip = blu.lib()  # (its symbol lookup reaches the runtime it depends on)
        self.hip.hipMalloc.argtypes = [C.c_void_p, C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.n = len(a)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 8)) == 0
        self.ptr = p.value
        assert self.hip.hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice

    def get(self):
        out = np.empty(self.n)
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptr, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def __del__(self):
        self.hip.hipFree(self.ptr)


def raw(blu, h, nrhs, r, ldr, x, ldl, tr="N", on_dev=0):
    return blu.lib().blu_hip_solve_dense_multi(h._h if h is not None else None, nrhs, r, ldr, x, ldl, tr.encode(), on_dev)


@pytest.fixture(scope="module")
def m2000(blu, oracle):
    """one handle of the m = 2000 golden with its twin, 2048 right-hand sides and the oracle's solutions of both systems:
    computed once, shared, never modified"""
    g, o = pair(blu, oracle, *golden("lp_m2000_k8_bw8"))
    rhs = np.random.default_rng(2000).standard_normal((2048, g.m))
    want = {tr: oracle_columns(o, rhs, tr) for tr in "NT"}
    return g, o, rhs, want


@pytest.mark.parametrize("batch", (False, True), ids=("single", "batch"))
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_against_oracle_and_single_calls(blu, oracle, name, batch):
    """the golden bases, fresh from a single factorize and from factorize_batch (the forward multi-solve then builds the
    row-wise L): nrhs 1, 3, 64 and 257, both systems, host inputs, every column the oracle's bits; nrhs = 3 also against
    three blu_hip_solve_dense calls"""
    g, o = pair(blu, oracle, *golden(name), batch=batch)
    rhs = np.random.default_rng(len(name)).standard_normal((257, g.m))
    for tr in "NT":
        want = oracle_columns(o, rhs, tr)
        for nrhs in (1, 3, 64, 257):
            x = g.solve_dense_multi(rhs[:nrhs], tr)
            assert np.array_equal(x, want[:nrhs]), (name, tr, nrhs, np.flatnonzero((x != want[:nrhs]).any(axis=1))[:5])
        for j in range(3):
            assert np.array_equal(g.solve_dense(rhs[j], tr), want[j]), (name, tr, j, "single")
        assert np.array_equal(g.solve_dense_multi(rhs[:3], tr), want[:3]), (name, tr, "after the single calls")


DEVICE_CHILD = r"""
import sys
import numpy as np
import torch
torch.zeros(1, device="cuda")  # torch's HIP runtime first, as bench.py has it: the other order leaves torch without a device
sys.path.insert(0, %(root)r)
import blu_amd
from blu_amd import keys as K
from oracle import orc
from tests import util, util_update as U
SENT = %(sent)r
g_ = np.load(%(golden)r)
cp, ri, v = g_["colptr"], g_["rowidx"], g_["values"]
m = len(cp) - 1
g = blu_amd.BLU(m, len(ri))
o = orc.OracleBLU(m, 64 * len(ri) + 1024)
o.set_fix_d3(True)
assert g.factorize(cp[:-1], cp[1:], ri, v) == o.factorize(cp[:-1], cp[1:], ri, v) == K.OK
nrhs, guard = 37, 1000
rng = np.random.default_rng(41)
rhs = rng.standard_normal((nrhs, m))
for state in ("fresh", "updated"):
    if state == "updated":
        log = U.run_updates(g, U.columns_of(cp, ri, v), m, 6, rng, check_every=10 ** 9, twin=o)
        assert log["done"] >= 2
    for tr in "NT":
        want = np.array([o.solve_dense(r, tr) for r in rhs])
        # in place, leading dimension m, a guard region behind the last column
        a = np.full(nrhs * m + guard, SENT)
        a[:nrhs * m] = rhs.ravel()
        t = torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        assert g.solve_dense_multi(trans=tr, device_ptrs=(t.data_ptr(), m, t.data_ptr(), m, nrhs)) is None
        got = t.cpu().numpy()
        assert np.array_equal(got[:nrhs * m].reshape(nrhs, m), want), (state, tr, "in place")
        assert (got[nrhs * m:] == SENT).all(), (state, tr, "guard")
        # out of place, padded leading dimensions
        ldr, ldl = m + 3, m + 5
        R = np.full((nrhs, ldr), np.nan)
        R[:, :m] = rhs
        tR = torch.from_numpy(R).cuda()
        tX = torch.full((nrhs * ldl + guard,), SENT, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        g.solve_dense_multi(trans=tr, device_ptrs=(tR.data_ptr(), ldr, tX.data_ptr(), ldl, nrhs))
        got = tX.cpu().numpy()
        X = got[:nrhs * ldl].reshape(nrhs, ldl)
        assert np.array_equal(X[:, :m], want), (state, tr, "padded")
        assert (X[:, m:] == SENT).all() and (got[nrhs * ldl:] == SENT).all(), (state, tr, "padding / guard")
        back = tR.cpu().numpy()
        assert np.array_equal(back[:, :m], rhs) and np.isnan(back[:, m:]).all(), (state, tr, "rhs kept")
print("MULTI DEVICE OK")
"""


def test_device_inputs_in_place_and_padded(blu, oracle):
    """torch tensors' data_ptr(): in place, and out of place with padded leading dimensions -- the padding (NaN on the
    right-hand sides: not read; a sentinel on the solutions: not written) intact and a guard region behind the last column
    untouched; fresh and updated handle, every column the oracle's bits.  In a child process, because torch has to
    initialise its HIP runtime before the library initialises the one it is linked with (the order bench.py has)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    body = DEVICE_CHILD % {"root": root, "sent": SENT, "golden": os.path.join(util.GOLDEN, "lp_m500_k8_bw8_dense_end.npz")}
    out = subprocess.run([sys.executable, "-c", body], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "MULTI DEVICE OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_many_waves_on_one_factorization(blu, m2000):
    """m = 2000, 2048 right-hand sides in one launch, both systems: every column the oracle's bits"""
    g, o, rhs, want = m2000
    for tr in "NT":
        x = g.solve_dense_multi(rhs, tr)
        assert g.dbg_multi_last_chunk() == 2048
        bad = np.flatnonzero((x != want[tr]).any(axis=1))
        assert len(bad) == 0, (tr, len(bad), bad[:8])


def test_forced_chunking(blu, m2000):
    """the byte limit set so that 7 columns fit, nrhs = 50: chunks of 7 (the last one partial) give the bits of the
    one-chunk call, with host and with device inputs"""
    g, o, rhs, want = m2000
    m = g.m
    try:
        for tr in "NT":
            g.dbg_set_multi_ws_bytes(-1)
            whole = g.solve_dense_multi(rhs[:50], tr)
            assert g.dbg_multi_last_chunk() == 50 and np.array_equal(whole, want[tr][:50])
            g.dbg_set_multi_ws_bytes(7 * 2 * 8 * stride_of(m))  # host inputs: work vectors + staging block
            x = g.solve_dense_multi(rhs[:50], tr)
            assert g.dbg_multi_last_chunk() == 7
            assert np.array_equal(x, whole), (tr, "host")
            g.dbg_set_multi_ws_bytes(7 * 8 * stride_of(m))  # device inputs: work vectors alone
            t = DevBuf(blu, rhs[:50].ravel())
            g.solve_dense_multi(trans=tr, device_ptrs=(t.ptr, m, t.ptr, m, 50))
            assert g.dbg_multi_last_chunk() == 7
            assert np.array_equal(t.get().reshape(50, m), whole), (tr, "device")
    finally:
        g.dbg_set_multi_ws_bytes(-1)


def test_updated_handle_in_lockstep(blu, oracle):
    """m = 300 after 12 update rounds in lock step with the twin and no dense solve in between (the garbage permutation of
    the multi call has work to do), nrhs = 70, both systems; then 5 further lock-step rounds, every status, pattern, value
    and counter still the twin's, and the multi-solves again"""
    m = 300
    cp, ri, v = oracle.gen_lp_basis(m, 6, 8, 0.5, 31, 0.3)
    g, o = pair(blu, oracle, cp, ri, v)
    cols = U.columns_of(cp, ri, v)
    rng = np.random.default_rng(31)
    log = U.run_updates(g, cols, m, 12, rng, check_every=10 ** 9, twin=o)
    assert log["done"] >= 4 and int(g.stat(K.STAT_NUPDATE)) == log["done"] and g.stat(K.STAT_NFORREST) > 0, log
    rhs = rng.standard_normal((70, m))
    for tr in "TN":
        assert np.array_equal(g.solve_dense_multi(rhs, tr), oracle_columns(o, rhs, tr)), tr
    log = U.run_updates(g, cols, m, 5, rng, twin=o)
    assert log["done"] >= 1, log
    for tr in "NT":
        assert np.array_equal(g.solve_dense_multi(rhs, tr), oracle_columns(o, rhs, tr)), (tr, "again")
        assert np.array_equal(g.solve_dense(rhs[0], tr), o.solve_dense(rhs[0], tr)), (tr, "single")
    util.assert_same_getters(g, o, "after the multi-solves on updated factors")


def test_refactorized_after_updates_is_solved_as_fresh(blu, oracle):
    """m = 600: updates, a multi-solve on the updated factors, then a new factorize of the current basis -- the multi-solve
    runs the fresh path again (row-wise L of the NEW factors) and gives the bits of a fresh twin"""
    m = 600
    cp, ri, v = oracle.gen_lp_basis(m, 6, 8, 0.5, 32, 0.3)
    g, o = pair(blu, oracle, cp, ri, v)
    cols = U.columns_of(cp, ri, v)
    rng = np.random.default_rng(32)
    rhs = rng.standard_normal((20, m))
    assert np.array_equal(g.solve_dense_multi(rhs, "N"), oracle_columns(o, rhs, "N"))
    log = U.run_updates(g, cols, m, 6, rng, check_every=10 ** 9, twin=o)
    assert log["done"] >= 2
    assert np.array_equal(g.solve_dense_multi(rhs, "N"), oracle_columns(o, rhs, "N"))
    cp2, ri2, v2 = U.csc_arrays(cols, m)
    o2 = oracle.OracleBLU(m, 64 * len(ri2) + 1024)
    o2.set_fix_d3(True)
    assert g.factorize(cp2[:-1], cp2[1:], ri2, v2) == o2.factorize(cp2[:-1], cp2[1:], ri2, v2) == K.OK
    assert int(g.stat(K.STAT_NUPDATE)) == 0
    for tr in "NT":
        assert np.array_equal(g.solve_dense_multi(rhs, tr), oracle_columns(o2, rhs, tr)), tr


@pytest.mark.parametrize("batch", (False, True), ids=("single", "batch"))
def test_handle_left_as_it_was(blu, oracle, batch):
    """after multi calls on a fresh handle: get_factors unchanged and the oracle's, every getter the oracle's; a following
    solve_sparse and a solve_dense_batch that includes the handle give the oracle's bits"""
    cp, ri, v = oracle.gen_lp_basis(800, 6, 8, 0.5, 33, 0.3)
    g, o = pair(blu, oracle, cp, ri, v, batch=batch)
    cp2, ri2, v2 = golden("lp_m200_k6_bw6")
    g2, o2 = pair(blu, oracle, cp2, ri2, v2, batch=True)
    before = g.get_factors()
    rng = np.random.default_rng(33)
    rhs = rng.standard_normal((40, g.m))
    for tr in "NT":
        assert np.array_equal(g.solve_dense_multi(rhs, tr), oracle_columns(o, rhs, tr)), tr
    after = g.get_factors()
    for key in util.INT_KEYS + util.VAL_KEYS:
        assert np.array_equal(before[key], after[key]), key
    util.assert_same_factors(after, o.get_factors())
    util.assert_same_getters(g, o, "after the multi-solves")
    idx = np.sort(rng.choice(g.m, 5, replace=False))
    val = rng.standard_normal(5)
    for tr in "NT":
        U._same(U._ss(g, idx, val, tr), U._ss(o, idx, val, tr), ("solve_sparse", tr))
    r2 = rng.standard_normal(g2.m)
    for tr in "NT":
        sols, st = blu.solve_dense_batch([g2, g], [r2, rhs[0]], tr)
        assert st == [K.OK, K.OK]
        assert np.array_equal(sols[0], o2.solve_dense(r2, tr)) and np.array_equal(sols[1], o.solve_dense(rhs[0], tr)), tr
    util.assert_same_getters(g, o, "after the following calls")


def test_refusals_each_followed_by_a_successful_call(blu, oracle):
    """every refusal of the entry in the order of the single call, nothing written; after each one a multi call on the
    good handle still gives the oracle's bits"""
    cp, ri, v = golden("lp_m200_k6_bw6")
    g, o = pair(blu, oracle, cp, ri, v)
    m = g.m
    rhs = np.random.default_rng(5).standard_normal((2, m))
    want = oracle_columns(o, rhs, "N")
    X = np.full((2, m), SENT)
    rp, xp = rhs.ctypes.data, X.ctypes.data
    hnone = blu.BLU(120, 500)  # never factorized
    hbad = blu.BLU(m, len(ri))  # last factorize refused
    bad_i = ri.copy()
    bad_i[3] = 999
    assert hbad.factorize(cp[:-1], cp[1:], bad_i, v) == K.ERROR_INVALID_ARGUMENT
    hz = blu.BLU(0, 1)
    e = np.zeros(0, np.uint64)
    assert hz.factorize(e, e, e, np.zeros(0)) == K.OK
    refusals = [
        ((None, 2, rp, m, xp, m), K.ERROR_ARGUMENT_MISSING),
        ((hnone, 2, rp, 120, xp, 120), K.ERROR_INVALID_CALL),
        ((hnone, 2, None, 120, xp, 120), K.ERROR_INVALID_CALL),  # the factorization is checked before the pointers
        ((hbad, 2, rp, m, xp, m), K.ERROR_INVALID_CALL),
        ((g, 2, None, m, xp, m), K.ERROR_ARGUMENT_MISSING),
        ((g, 2, rp, m, None, m), K.ERROR_ARGUMENT_MISSING),
        ((g, -1, None, m, xp, m), K.ERROR_ARGUMENT_MISSING),  # the pointers are checked before the counts
        ((g, -1, rp, m, xp, m), K.ERROR_INVALID_ARGUMENT),
        ((g, 2, rp, m - 1, xp, m), K.ERROR_INVALID_ARGUMENT),
        ((g, 2, rp, m, xp, m - 1), K.ERROR_INVALID_ARGUMENT),
        ((g, 0, rp, 0, xp, 0), K.OK),   # nrhs == 0: nothing written
        ((hz, 2, rp, 0, xp, 0), K.OK),  # m == 0: nothing written
    ]
    for k, (args, code) in enumerate(refusals):
        assert raw(blu, *args) == code, (k, code)
        assert (X == SENT).all(), k
        assert np.array_equal(g.solve_dense_multi(rhs, "N"), want), (k, "after")
    with pytest.raises(blu.BluError) as err:
        hnone.solve_dense_multi(np.zeros((2, 120)))
    assert err.value.status == K.ERROR_INVALID_CALL
    assert raw(blu, g, 1, rp, 0, xp, 0) == K.OK  # one right-hand side: the leading dimensions are not used
    assert np.array_equal(X[0], want[0]) and (X[1] == SENT).all()
    assert np.array_equal(g.solve_dense(rhs[1], "N"), want[1])
