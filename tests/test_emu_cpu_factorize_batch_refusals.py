"""The refusals of blu_hip_factorize_batch as a whole call, at the C ABI, on the CPU: the emulation build of the library
(blu_amd/csrc `make emu`, as in tests/test_emu_cpu.py) runs the host side of the entry.

Every return value, every status[k] and the state of the handles afterwards are pinned: a refused call leaves the
factorizations its handles hold alone, except the call that names a handle twice, which invalidates that handle (it is
refused behind the point from which "the factors every handle holds are invalid") and no other.  Equalities only.
The case runs in a child process: the library path is fixed when blu_amd is first imported."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")

CHILD = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, sys.argv[1])
import blu_amd
from blu_amd import keys as K
from oracle import orc
L = blu_amd.lib()
assert b"gfx950" in L.blu_hip_version()
L.blu_hip_factorize_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
MISS, INVARG, INVCALL = K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_ARGUMENT, K.ERROR_INVALID_CALL
assert (MISS, INVARG, INVCALL) == (-3, -4, -2)

mats = [orc.gen_lp_basis(60, 4, 4, 0.5, 1, 0.3), orc.gen_lp_basis(50, 4, 4, 0.8, 3, 0.6)]
hs = [blu_amd.BLU(len(cp) - 1, len(ri)) for cp, ri, v in mats]
twins = []
for cp, ri, v in mats:
    o = orc.OracleBLU(len(cp) - 1, 64 * len(ri) + 1024)
    o.set_fix_d3(True)
    assert o.factorize(cp[:-1], cp[1:], ri, v) == K.OK
    twins.append(o)
rhs = [np.sin(1.0 + np.arange(float(h.m))) for h in hs]


def same_factors(k):
    fg, fo = hs[k].get_factors(), twins[k].get_factors()
    for key in ("rowperm", "colperm", "l_colptr", "l_rowidx", "u_colptr", "u_rowidx", "l_value", "u_value"):
        assert np.array_equal(fg[key], fo[key]), (k, key)


def solutions(k):
    return [hs[k].solve_dense(rhs[k], tr) for tr in "NT"]


def as_before(ks, where):
    for k in ks:
        for tr, x, x0 in zip("NT", solutions(k), before[k]):
            assert np.array_equal(x, x0), (where, k, tr)


def raw(members, n=2, null=None, hs_null=False, status=True):
    # the host inputs of both bases; `null` names the one array of arrays handed over as NULL
    cols = {"b_begin": [], "b_end": [], "b_i": [], "b_x": []}
    for cp, ri, v in mats:
        for key, a in zip(cols, (cp[:-1], cp[1:], ri, v)):
            cols[key].append(np.ascontiguousarray(a))
    arrs = {key: (C.c_void_p * 2)(*[a.ctypes.data for a in cols[key]]) for key in cols}
    arrs["b_i_len"] = (C.c_uint64 * 2)(*[len(ri) for cp, ri, v in mats])
    handles = (C.c_void_p * 2)(*[None if h is None else h._h for h in members])
    st = (C.c_int * 2)(77, 77)
    args = [None if key == null else arrs[key] for key in ("b_begin", "b_end", "b_i", "b_x", "b_i_len")]
    rc = L.blu_hip_factorize_batch(None if hs_null else handles, n, *args, 0, st if status else None)
    return rc, list(st)


for h, (cp, ri, v) in zip(hs, mats):
    assert h.factorize(cp[:-1], cp[1:], ri, v) == K.OK
for k in range(2):
    same_factors(k)
before = [solutions(k) for k in range(2)]
for k in range(2):
    for tr, x in zip("NT", before[k]):
        assert np.array_equal(x, twins[k].solve_dense(rhs[k], tr)), (k, tr)

assert raw(hs, hs_null=True) == (MISS, [MISS, MISS])
as_before((0, 1), "hs == NULL")
assert raw(hs, n=-1) == (MISS, [77, 77])       # nothing written
as_before((0, 1), "n = -1")
assert raw(hs, n=0) == (K.OK, [77, 77])
as_before((0, 1), "n = 0")
for null in ("b_begin", "b_end", "b_i", "b_x", "b_i_len"):
    assert raw(hs, null=null) == (MISS, [MISS, MISS]), null
    as_before((0, 1), null)
assert raw([hs[0], None]) == (MISS, [MISS, MISS])
as_before((0, 1), "hs[1] == NULL")
assert raw(hs, status=False)[0] == K.OK          # status == NULL, a valid call
for k in range(2):
    same_factors(k)
as_before((0, 1), "status == NULL")
# the same handle twice: refused, and that handle holds no factorization any more
assert raw([hs[0], hs[0]]) == (INVARG, [INVARG, INVARG])
try:
    hs[0].solve_dense(rhs[0])
except blu_amd.BluError as err:
    assert err.status == INVCALL, err.status
else:
    raise AssertionError("the duplicated handle still solves")
as_before((1,), "[h0, h0]")
assert blu_amd.factorize_batch(hs, mats) == [K.OK, K.OK]
for k in range(2):
    same_factors(k)
as_before((0, 1), "factorized again")
print("FACTORIZE BATCH REFUSALS OK")
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def test_factorize_batch_refusals_on_the_cpu(emu_lib):
    """two factorized handles, lp(60,4,4,0.5,1,0.3) and lp(50,4,4,0.8,3,0.6), host inputs, status prefilled with 77:
    hs == NULL, each of b_begin / b_end / b_i / b_x / b_i_len NULL and hs[1] == NULL give ARGUMENT_MISSING in the return
    value and in every status[k]; n = -1 gives it and writes nothing; n = 0 is OK and writes nothing; status == NULL on a
    valid call factorizes both.  After each, both handles hold the oracle's factors and solve with the bits they gave
    before.  [h0, h0] gives INVALID_ARGUMENT everywhere, h0 then refuses solve_dense with INVALID_CALL and h1 solves as
    before; factorize_batch([h0, h1]) afterwards gives OK, OK, the oracle's factors and the solutions as before."""
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "FACTORIZE BATCH REFUSALS OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
