"""blu_hip_solve_for_update_batch and blu_hip_update_batch on the CPU: the emulation build of the library (blu_amd/csrc
`make emu`, as in tests/test_emu_cpu_solves.py) runs k_upd_init_batch, k_solve_upd_batch, k_update_batch,
k_gather_lhs_batch and the host side of blu_update_batch.inc on six small bases kept in lock step, every member with
an oracle twin driven by the single calls: every status, pattern (order included), value and the statistics of
tests/util_update.py::run_updates identical, bit for bit (tests/util_update_batch.py).  Each case runs in a child
process: the library path is fixed when blu_amd is first imported."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")

CHILD = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, %(root)r)
import blu_amd
from blu_amd import keys as K
from oracle import orc
from tests import util_update as U, util_update_batch as UB
L = blu_amd.lib()
assert b"gfx950" in L.blu_hip_version()


def twin_of(cols, m, cap):
    o = orc.OracleBLU(m, cap)
    o.set_fix_d3(True)
    cp, ri, v = U.csc_arrays(cols, m)
    assert o.factorize(cp[:-1], cp[1:], ri, v) == K.OK
    return o


# ---- six bases, factorized by factorize_batch: four synthetic LP bases, the bidiagonal one, one with a tiny arena
specs = [(60, 4, 5, 0.3, 7, 0.5), (150, 5, 4, 0.8, 3, 0.6), (200, 6, 6, 0.5, 1, 0.3), (90, 4, 5, 0.3, 9, 0.5)]
colsets = [U.columns_of(*orc.gen_lp_basis(*s)) for s in specs]
colsets.append(UB.bidiagonal_cols(8))
TINY = len(colsets)
colsets.append(U.columns_of(*orc.gen_lp_basis(24, 4, 4, 0.0, 5, 0.5)))
hs = []
for k, cols in enumerate(colsets):
    nz = sum(len(c[0]) for c in cols)
    hs.append(blu_amd.BLU(len(cols), 4 if k == TINY else nz))
hs[TINY].dbg_set_upd_extra(8)   # forces UPD_NEED_R / NEED_UC / NEED_W round trips inside the batch
mats = [U.csc_arrays(cols, len(cols)) for cols in colsets]
assert blu_amd.factorize_batch(hs, mats) == [K.OK] * len(hs)
members = []
for k, (h, cols) in enumerate(zip(hs, colsets)):
    nz = sum(len(c[0]) for c in cols)
    members.append(UB.Member(h, twin_of(cols, h.m, 256 * nz + 1024), cols, 100 + k, pair_row=UB.pair_rows(h),
                             script=UB.BIDIAGONAL_SCRIPT if k == 4 else ()))

# ---- whole-call refusals, before anything is prepared: every status carries the code, no handle is touched
FN = L.blu_hip_solve_for_update_batch
FN.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_char, C.c_void_p]
FU = L.blu_hip_update_batch
FU.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
i3 = np.array([3], np.uint64)
x3 = np.array([1.0])


def vp(xs):
    return (C.c_void_p * max(len(xs), 1))(*xs)


def sfu(handles, ir, xr, trans, n=None, nzr=True, H=True, st=True):
    n = len(handles) if n is None else n
    s = (C.c_int * max(len(handles), 1))(*([77] * max(len(handles), 1)))
    nz = (C.c_int64 * max(len(handles), 1))(*([1] * max(len(handles), 1)))
    rc = FN(vp([h._h if h is not None else None for h in handles]) if H else None, n, nz if nzr else None, None if ir is None else vp(ir),
            None if xr is None else vp(xr), None, None, None, trans, s if st else None)
    return rc, list(s)[:len(handles)]


MISS, INVARG = K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_ARGUMENT
ip, xp = i3.ctypes.data, x3.ctypes.data
assert sfu(hs[:2], [ip, ip], None, b"T", H=False) == (MISS, [MISS] * 2)
assert sfu(hs[:2], None, None, b"T") == (MISS, [MISS] * 2)
assert sfu([hs[0], None], [ip, ip], None, b"T") == (MISS, [MISS] * 2)
assert sfu(hs[:2], [ip, None], None, b"T") == (MISS, [MISS] * 2)
assert sfu(hs[:2], [ip, ip], None, b"N") == (MISS, [MISS] * 2)                 # forward without xrhs
assert sfu(hs[:2], [ip, ip], [xp, None], b"N") == (MISS, [MISS] * 2)           # ... without an xrhs[k]
assert sfu(hs[:2], [ip, ip], [xp, xp], b"N", nzr=False) == (MISS, [MISS] * 2)  # ... without nzrhs
assert sfu(hs[:2], [ip, ip], None, b"T", n=-1)[0] == MISS
assert sfu([hs[0], hs[1], hs[0]], [ip] * 3, None, b"T") == (INVARG, [INVARG] * 3)
assert sfu(hs[:2], [ip, ip], None, b"T", n=0) == (K.OK, [77, 77])              # n == 0: nothing written
s2 = (C.c_int * 2)(77, 77)
xt = (C.c_double * 2)(1.0, 1.0)
assert FU(None, 2, xt, s2) == MISS and list(s2) == [MISS] * 2
assert FU(vp([hs[0]._h, hs[1]._h]), 2, None, s2) == MISS and list(s2) == [MISS] * 2
assert FU(vp([hs[0]._h, None]), 2, xt, s2) == MISS and list(s2) == [MISS] * 2
assert FU(vp([hs[0]._h, hs[0]._h]), 2, xt, s2) == INVARG and list(s2) == [INVARG] * 2
assert FU(vp([hs[0]._h, hs[1]._h]), -1, xt, s2) == MISS
s2 = (C.c_int * 2)(77, 77)
assert FU(vp([hs[0]._h, hs[1]._h]), 0, xt, s2) == K.OK and list(s2) == [77, 77]
for call in (lambda: blu_amd.solve_for_update_batch([hs[0], hs[0]], [[1], [1]], None, "T"), lambda: blu_amd.update_batch([hs[1], hs[1]], [1.0, 1.0]),
             lambda: blu_amd.solve_for_update_batch(hs[:2], [[1], [1]], None, "N")):
    try:
        call()
    except blu_amd.BluError as e:
        assert e.status in (INVARG, MISS)
    else:
        raise AssertionError("not refused")
assert all(h.stat(K.STAT_NUPDATE) == 0 for h in hs)

# ---- the per-member statuses in one mixed call (the protocol of tests/test_gpu_update.py::test_update_call_protocol)
cp, ri, v = orc.gen_lp_basis(200, 5, 5, 0.5, 2, 0.3)
hp = blu_amd.BLU(200, len(ri))
op = orc.OracleBLU(200, 64 * len(ri))
op.set_fix_d3(True)
assert hp.factorize(cp[:-1], cp[1:], ri, v) == op.factorize(cp[:-1], cp[1:], ri, v) == K.OK
hnone = blu_amd.BLU(120, 500)                                        # never factorized
hz = blu_amd.BLU(0, 1)                                               # m = 0
e = np.zeros(0, np.uint64)
assert hz.factorize(e, e, e, np.zeros(0)) == K.OK
hrange = blu_amd.BLU(200, len(ri))                                   # gets an index out of range
assert hrange.factorize(cp[:-1], cp[1:], ri, v) == K.OK
mixed = [hp, hnone, hz, hrange]
assert blu_amd.update_batch(mixed, [1.0] * 4) == [K.ERROR_INVALID_CALL] * 4                        # nothing prepared
assert blu_amd.solve_for_update_batch(mixed, [[3], [3], [0], [200]], None, "T", want_solution=False) == \
    [K.OK, K.ERROR_INVALID_CALL, INVARG, INVARG]
assert op.solve_for_update([3], None, "T", want_solution=False)[0] == K.OK and hp.nzlhs == 0        # prepare only
assert blu_amd.update_batch(mixed, [1.0] * 4) == [K.ERROR_INVALID_CALL] * 4                        # forward solve missing
a, b = int(cp[4]), int(cp[5])
st = blu_amd.solve_for_update_batch(mixed, [ri[a:b], [1], [0], [1, 999]], [v[a:b], [1.0], [1.0], [1.0, 2.0]], "N")
assert st == [K.OK, K.ERROR_INVALID_CALL, INVARG, INVARG], st
U._same((st[0],) + UB.solution(hp), op.solve_for_update(ri[a:b], v[a:b], "N"), "column 4")
assert abs(hp.lhs[3]) < 1e-12
st = blu_amd.update_batch(mixed, [hp.lhs[3], 1.0, 1.0, 1.0])
assert st == [K.ERROR_SINGULAR_UPDATE] + [K.ERROR_INVALID_CALL] * 3 and op.update(hp.lhs[3]) == K.ERROR_SINGULAR_UPDATE, st
b1 = np.ones(200)
assert np.array_equal(hp.solve_dense(b1), op.solve_dense(b1))         # the old factorization is still valid
# the C entry's return value: the most negative member status; status may be NULL
ir = [np.array([q], np.uint64) for q in (3, 3, 0, 200)]
rc, st = sfu(mixed, [x.ctypes.data for x in ir], None, b"T")
assert st == [K.OK, K.ERROR_INVALID_CALL, INVARG, INVARG] and rc == min(st), (rc, st)
assert sfu(mixed[:1], [ir[0].ctypes.data], None, b"T", st=False)[0] == K.OK
assert op.solve_for_update([3], None, "T", want_solution=False)[0] == K.OK
assert op.solve_for_update([3], None, "T", want_solution=False)[0] == K.OK
# prepare only, then with solutions for some members: ilhs[k] NULL = prepared without a solution
pm = [hp, hrange]
nzl = (C.c_int64 * 2)(55, 55)
il = [np.zeros(200, np.int64) for _ in pm]
lh = [np.zeros(200) for _ in pm]
s2 = (C.c_int * 2)(77, 77)
rc = FN(vp([h._h for h in pm]), 2, None, vp([ir[0].ctypes.data, ir[1].ctypes.data]), None, nzl, vp([il[0].ctypes.data, None]),
        vp([lh[0].ctypes.data, lh[1].ctypes.data]), b"t", s2)
assert rc == K.OK and list(s2) == [K.OK] * 2 and nzl[1] == 55 and not lh[1].any()
so = op.solve_for_update([3], None, "T")
assert so[0] == K.OK and nzl[0] == len(so[1]) and np.array_equal(il[0][:nzl[0]], so[1]) and np.array_equal(lh[0], so[2])

# ---- lock-step rounds; the tiny-arena member meets ERROR_MAXIMUM_UPDATES on the way, the others go on
assert UB.kinds(members).sum() == 0
ROUNDS, LATE = 7, 200
for r in range(ROUNDS):
    UB.lockstep_round(blu_amd, members, where=r)
    if r == 1:  # the two hand-predictable replacements of the bidiagonal basis: neither needs a row eta
        assert members[4].done == 2 and [hs[4].stat(key) for key in UB.KINDS] == [0, 1, 1], members[4].done
small = [members[TINY], members[0]]
for r in range(ROUNDS, LATE):
    st_t, _, _ = UB.lockstep_round(blu_amd, small, where=r)
    if members[TINY].maxed:
        break
assert members[TINY].maxed and st_t == [K.ERROR_MAXIMUM_UPDATES, K.OK] and hs[TINY].stat(K.STAT_NFORREST) == 24, (st_t, r)
UB.lockstep_round(blu_amd, members, where="after maximum updates")    # again in a full call: refused alone
got = UB.kinds(members)
print("KINDS", got, [M.done for M in members], [M.skipped for M in members], [M.singular for M in members])
assert (got > 0).all() and np.array_equal(got, UB.kinds(members, lambda M: M.twin))
assert all(M.done >= 3 and M.h.stat(K.STAT_NUPDATE) == M.done for M in members if M.m > 8), [M.done for M in members]
UB.dense_after(blu_amd, members, 17)
assert max(M.max_residual for M in members) <= 1e-7 and max(M.max_pivot_error for M in members) <= 1e-8, [M.max_residual for M in members]
print("EMU UPDATE BATCH OK")
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def test_update_batch_in_lockstep_on_the_cpu(emu_lib):
    """six bases of m <= 200 from factorize_batch (four synthetic LP bases, the bidiagonal basis with its two
    hand-predictable permutation updates, one with a b_nz hint of 4 and dbg_set_upd_extra(8)), each with an oracle twin:
    the refusals of the whole call, the per-member statuses of a mixed call, prepare-only calls, lock-step rounds of
    batched T-solve, N-solve and update with a changing member set, the tiny member run to ERROR_MAXIMUM_UPDATES
    while another goes on, and solve_dense_batch on the updated factors"""
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1")
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "EMU UPDATE BATCH OK" in out.stdout
