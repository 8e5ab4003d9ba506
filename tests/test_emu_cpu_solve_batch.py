"""blu_hip_solve_dense_batch on the CPU: the emulation build of the library (blu_amd/csrc `make emu`, as in
tests/test_emu_cpu.py) runs the host side of the batch solve on small bases -- per-member statuses of a mixed call,
refusals of the whole call, and handles that stay usable afterwards.

The solutions of the batch and of blu_hip_solve_dense on the same handles are compared with the oracle's bit for bit
(the sweeps of k_sweep.h run in lockstep under the emulator where they rely on it: DESIGN.md section 4b); members with an
updated factorization are in tests/test_emu_cpu_solves.py.  Each case runs in a child process: the library
path is fixed when blu_amd is first imported."""
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
L = blu_amd.lib()
assert b"gfx950" in L.blu_hip_version()
specs = [(200, 8, 8, 0.5, 1, 0.3), (150, 5, 4, 0.8, 3, 0.6), (180, 6, 6, 0.5, 4, 0.3)]
mats = [orc.gen_lp_basis(*s) for s in specs]


def oracle_of(cp, ri, v):
    o = orc.OracleBLU(len(cp) - 1, 64 * len(ri) + 1024)
    o.set_fix_d3(True)
    assert o.factorize(cp[:-1], cp[1:], ri, v) == K.OK
    return o


def oracle_factors(cp, ri, v):
    return oracle_of(cp, ri, v).get_factors()


def same_factors(h, cp, ri, v):
    fg, fo = h.get_factors(), oracle_factors(cp, ri, v)
    for key in ("rowperm", "colperm", "l_colptr", "l_rowidx", "u_colptr", "u_rowidx", "l_value", "u_value"):
        assert np.array_equal(fg[key], fo[key]), key


hb = [blu_amd.BLU(len(cp) - 1, len(ri)) for cp, ri, v in mats]
assert blu_amd.factorize_batch(hb, mats) == [K.OK] * 3                # fresh from factorize_batch
cp, ri, v = mats[0]
hs1 = blu_amd.BLU(200, len(ri))
assert hs1.factorize(cp[:-1], cp[1:], ri, v) == K.OK                # fresh from a single factorize
hnone = blu_amd.BLU(120, 500)                                        # never factorized
hz = blu_amd.BLU(0, 1)                                               # m = 0
e = np.zeros(0, np.uint64)
assert hz.factorize(e, e, e, np.zeros(0)) == K.OK
hbad = blu_amd.BLU(150, len(mats[1][1]))                             # last factorize refused
cp1, ri1, v1 = mats[1]
bad_i = ri1.copy()
bad_i[3] = 999
assert hbad.factorize(cp1[:-1], cp1[1:], bad_i, v1) == K.ERROR_INVALID_ARGUMENT
hs = hb + [hs1, hnone, hz, hbad]
n = len(hs)
want = [K.OK, K.OK, K.OK, K.OK, K.ERROR_INVALID_CALL, K.OK, K.ERROR_INVALID_CALL]
rng = np.random.default_rng(5)
rhs = [rng.standard_normal(h.m) for h in hs]
oracles = {0: oracle_of(*mats[0]), 1: oracle_of(*mats[1]), 2: oracle_of(*mats[2]), 3: oracle_of(*mats[0])}
for tr in "NTnt":
    sols, st = blu_amd.solve_dense_batch(hs, rhs, tr)
    assert st == want, (tr, st)
    assert [len(x) for x in sols] == [h.m for h in hs]
    assert not sols[4].any() and not sols[6].any()                   # members that were not solved: untouched
    assert all(np.isfinite(x).all() for x in sols)
    for k, o in oracles.items():                                     # the members that were solved: the oracle's bits
        assert np.array_equal(sols[k], o.solve_dense(rhs[k], tr.upper())), (tr, k)

# the C entry itself: return value and statuses
L.blu_hip_solve_dense_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_char, C.c_int, C.c_void_p]
rs = [np.ascontiguousarray(r) for r in rhs]
ls = [np.zeros(max(h.m, 1)) for h in hs]


def call(handles, rp, lp, count=None):
    k = len(handles) if count is None else count
    H = (C.c_void_p * max(len(handles), 1))(*[h._h if h is not None else None for h in handles])
    R = (C.c_void_p * max(len(rp), 1))(*rp)
    Lp = (C.c_void_p * max(len(lp), 1))(*lp)
    st = (C.c_int * max(len(handles), 1))(*([77] * max(len(handles), 1)))
    rc = L.blu_hip_solve_dense_batch(H, k, R, Lp, b"N", 0, st)
    return rc, list(st)[:len(handles)]


rp = [r.ctypes.data for r in rs]
lp = [x.ctypes.data for x in ls]
rc, st = call(hs, rp, lp)
assert rc == K.ERROR_INVALID_CALL and st == want, (rc, st)           # the most negative member status
rc, st = call(hb, rp[:3], lp[:3])
assert rc == K.OK and st == [K.OK] * 3, (rc, st)
# refusals: every status carries the code
rc, st = call([hb[0], hb[1], hb[0]], rp[:3], lp[:3])
assert rc == K.ERROR_INVALID_ARGUMENT and st == [K.ERROR_INVALID_ARGUMENT] * 3, (rc, st)
rc, st = call([hb[0], None], rp[:2], lp[:2])
assert rc == K.ERROR_ARGUMENT_MISSING and st == [K.ERROR_ARGUMENT_MISSING] * 2, (rc, st)
rc, st = call(hb[:2], [rp[0], None], lp[:2])
assert rc == K.ERROR_ARGUMENT_MISSING and st == [K.ERROR_ARGUMENT_MISSING] * 2, (rc, st)
rc, st = call(hb[:2], rp[:2], [None, lp[1]])
assert rc == K.ERROR_ARGUMENT_MISSING and st == [K.ERROR_ARGUMENT_MISSING] * 2, (rc, st)
st = (C.c_int * 2)(77, 77)
H = (C.c_void_p * 2)(hb[0]._h, hb[1]._h)
R = (C.c_void_p * 2)(*rp[:2])
assert L.blu_hip_solve_dense_batch(None, 2, R, R, b"N", 0, st) == K.ERROR_ARGUMENT_MISSING and list(st) == [K.ERROR_ARGUMENT_MISSING] * 2
st = (C.c_int * 2)(77, 77)
assert L.blu_hip_solve_dense_batch(H, 2, None, R, b"N", 0, st) == K.ERROR_ARGUMENT_MISSING and list(st) == [K.ERROR_ARGUMENT_MISSING] * 2
st = (C.c_int * 2)(77, 77)
assert L.blu_hip_solve_dense_batch(H, 0, R, R, b"N", 0, st) == K.OK and list(st) == [77, 77]        # n == 0: nothing written
assert L.blu_hip_solve_dense_batch(H, -1, R, R, b"N", 0, st) == K.ERROR_ARGUMENT_MISSING
assert L.blu_hip_solve_dense_batch(H, 2, R, R, b"N", 0, None) == K.OK                                # status may be NULL
try:
    blu_amd.solve_dense_batch([hb[0], hb[0]], [rhs[0], rhs[0]])
except blu_amd.BluError as e:
    assert e.status == K.ERROR_INVALID_ARGUMENT
else:
    raise AssertionError("duplicate handle not refused")

# afterwards every handle is usable: the single solves answer as before, and a new factorize gives the oracle's factors
for k, (h, w) in enumerate(zip(hs, want)):
    for tr in "NT":
        try:
            x = h.solve_dense(rhs[k], tr)
        except blu_amd.BluError as e:
            assert e.status == w == K.ERROR_INVALID_CALL, (k, e.status)
        else:
            assert w == K.OK and len(x) == h.m, k
            if k in oracles:
                assert np.array_equal(x, oracles[k].solve_dense(rhs[k], tr)), (k, tr)
for h, (cp, ri, v) in zip(hb, mats):
    assert h.factorize(cp[:-1], cp[1:], ri, v) == K.OK
    same_factors(h, cp, ri, v)
assert hbad.factorize(cp1[:-1], cp1[1:], ri1, v1) == K.OK
same_factors(hbad, cp1, ri1, v1)
sols, st = blu_amd.solve_dense_batch(hb + [hbad], rhs[:3] + [rhs[6]], "N")
assert st == [K.OK] * 4, st
for x, r, mat in zip(sols, rhs[:3] + [rhs[6]], mats + [mats[1]]):
    assert np.array_equal(x, oracle_of(*mat).solve_dense(r, "N"))
print("EMU SOLVE BATCH OK")
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def test_solve_dense_batch_statuses_refusals_and_reuse_on_the_cpu(emu_lib):
    """a mixed call (fresh from factorize_batch and from factorize, never factorized, m = 0, last factorize refused):
    per-member statuses and return values of the C entry, the refusals of the whole call, handles usable afterwards;
    every solution, of the batch and of the single solves, equal to the oracle's bit for bit"""
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1")
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "EMU SOLVE BATCH OK" in out.stdout
