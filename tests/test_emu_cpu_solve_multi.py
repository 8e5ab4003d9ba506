"""blu_hip_solve_dense_multi on the CPU: the emulation build of the library (blu_amd/csrc `make emu`, as in
tests/test_emu_cpu.py) runs many right-hand sides on ONE handle -- k_solve_dense_multi on fresh factorizations,
k_garbage_perm + k_solve_dense_upd_multi on updated ones, the chunking and the host side of the entry.

Every column is compared with the oracle's solve_dense on a twin, bit for bit (np.array_equal; the oracle with the
64-bit cancellation mask, set_fix_d3, as elsewhere); an updated handle has its twin driven through the same updates.
Each case runs in a child process: the library path is fixed when blu_amd is first imported."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")

HEAD = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, %(root)r)
import blu_amd
from blu_amd import keys as K
from oracle import orc
from tests import util, util_update as U
L = blu_amd.lib()
assert b"gfx950" in L.blu_hip_version()
L.blu_hip_solve_dense_multi.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_char, C.c_int]
SENT = -7.25e300


def pair(cp, ri, v, want=K.OK):
    m = len(cp) - 1
    g = blu_amd.BLU(m, len(ri))
    o = orc.OracleBLU(m, 64 * len(ri) + 1024)
    o.set_fix_d3(True)
    sg, so = g.factorize(cp[:-1], cp[1:], ri, v), o.factorize(cp[:-1], cp[1:], ri, v)
    assert sg == so == want, (sg, so, want)
    return g, o


def stride_of(m):
    return (m + 2 + 31) // 32 * 32


def same_columns(x, o, rhs, trans, where):
    assert x.shape == rhs.shape, where
    for j in range(len(rhs)):
        assert np.array_equal(x[j], o.solve_dense(rhs[j], trans.upper())), (where, trans, j)


def pair_rows(g):
    f = g.get_factors()
    pr = np.zeros(g.m, np.int64)
    pr[f["colperm"]] = f["rowperm"]
    return pr
"""

CHILD_FRESH = r"""
def scaled(cp, v, cols):
    v = v.copy()
    for j in cols:
        v[int(cp[j]):int(cp[j + 1])] *= 1e-17
    return v


def with_long_column(cp, ri, v, col, collen, seed):
    # column `col` filled to `collen` entries in random rows
    m = len(cp) - 1
    rng = np.random.default_rng(seed)
    cols = [dict(zip(ri[cp[j]:cp[j + 1]].astype(np.int64).tolist(), v[cp[j]:cp[j + 1]].tolist())) for j in range(m)]
    free = np.array([i for i in range(m) if i not in cols[col]])
    for i in rng.choice(free, collen - len(cols[col]), replace=False):
        cols[col][int(i)] = float(rng.choice((-1.0, 1.0)) * rng.uniform(0.1, 1.0))
    nri = np.concatenate([sorted(c) for c in cols]).astype(np.uint64)
    nv = np.concatenate([[c[i] for i in sorted(c)] for c in cols])
    ncp = np.concatenate(([0], np.cumsum([len(c) for c in cols]))).astype(np.uint64)
    return ncp, nri, nv


rng = np.random.default_rng(17)
cases = []
for spec in ((200, 8, 8, 0.5, 1, 0.3), (150, 5, 4, 0.8, 3, 0.6)):
    cases.append(("lp%%d" %% spec[0], orc.gen_lp_basis(*spec), K.OK))
cp, ri, v = orc.gen_lp_basis(90, 4, 5, 0.3, 7, 0.5)
cases.append(("rank deficient", (cp, ri, scaled(cp, v, (2, 45, 89))), K.WARNING_SINGULAR_MATRIX))
cases.append(("long lines", with_long_column(*util.basis_with_long_row(240, 100, 3), 60, 100, 3), K.OK))
for name, (cp, ri, v), want in cases:
    g, o = pair(cp, ri, v, want)
    m = g.m
    if name == "long lines":  # the tail loops of the sweeps: lines of more than 64 entries in three of the four line sets
        f = o.get_factors()
        ucol = int(np.diff(f["u_colptr"]).max()) - 1
        lrow = int(np.bincount(f["l_rowidx"], minlength=m).max()) - 1
        urow = int(np.bincount(f["u_rowidx"], minlength=m).max()) - 1
        print("LONG", ucol, lrow, urow)
        assert min(ucol, lrow, urow) > 64, (ucol, lrow, urow)
    for nrhs in (1, 2, 65):
        rhs = rng.standard_normal((nrhs, m))
        for tr in "NTnt":
            same_columns(g.solve_dense_multi(rhs, tr), o, rhs, tr, (name, nrhs))
        assert g.dbg_multi_last_chunk() == nrhs
    # in place, through the C entry
    rhs = rng.standard_normal((3, m))
    for tr in "NT":
        x = rhs.copy()
        assert L.blu_hip_solve_dense_multi(g._h, 3, x.ctypes.data, m, x.ctypes.data, m, tr.encode(), 0) == K.OK
        same_columns(x, o, rhs, tr, (name, "in place"))
    # out of place with padded leading dimensions: the padding is neither read (NaN would spread) nor written
    ldr, ldl = m + 3, m + 5
    R = np.full((3, ldr), np.nan)
    R[:, :m] = rhs
    for tr in "NT":
        X = np.full((3, ldl), SENT)
        assert L.blu_hip_solve_dense_multi(g._h, 3, R.ctypes.data, ldr, X.ctypes.data, ldl, tr.encode(), 0) == K.OK
        same_columns(X[:, :m], o, rhs, tr, (name, "padded"))
        assert (X[:, m:] == SENT).all() and np.isnan(R[:, m:]).all() and np.array_equal(R[:, :m], rhs), (name, "padding")
    # the single call answers as before
    for tr in "NT":
        assert np.array_equal(g.solve_dense(rhs[0], tr), o.solve_dense(rhs[0], tr)), (name, "single after")
print("MULTI FRESH OK")
"""

CHILD_CHUNK = r"""
cp, ri, v = orc.gen_lp_basis(150, 5, 4, 0.8, 3, 0.6)
g, o = pair(cp, ri, v)
m = g.m
rhs = np.random.default_rng(23).standard_normal((23, m))
whole = {tr: g.solve_dense_multi(rhs, tr) for tr in "NT"}
assert g.dbg_multi_last_chunk() == 23
g.dbg_set_multi_ws_bytes(5 * 2 * 8 * stride_of(m) + 8)  # host inputs: work vectors and staging block, five columns of each
for tr in "NT":
    x = g.solve_dense_multi(rhs, tr)
    assert g.dbg_multi_last_chunk() == 5  # chunks of 5, 5, 5, 5, 3
    assert np.array_equal(x, whole[tr]), tr
    same_columns(x, o, rhs, tr, "chunked")
g.dbg_set_multi_ws_bytes(1)  # less than one column: one at a time
x = g.solve_dense_multi(rhs[:4], "N")
assert g.dbg_multi_last_chunk() == 1 and np.array_equal(x, whole["N"][:4])
g.dbg_set_multi_ws_bytes(-1)
assert np.array_equal(g.solve_dense_multi(rhs, "T"), whole["T"]) and g.dbg_multi_last_chunk() == 23
print("MULTI CHUNK OK")
"""

CHILD_UPDATED = r"""
spec = (120, 5, 5, 0.4, 6, 0.5)
cp, ri, v = orc.gen_lp_basis(*spec)
m = spec[0]
g, o = pair(cp, ri, v)
cols = U.columns_of(cp, ri, v)
pr = pair_rows(g)
rng = np.random.default_rng(8)
# 8 update rounds in lock step WITHOUT a solve_dense in between (check_every beyond the count): the pivot sequence has grown
# past m when the multi call comes, so its garbage permutation has work to do
log = U.run_updates(g, cols, m, 8, rng, check_every=10 ** 9, pair_row=pr, twin=o)
assert log["done"] >= 3 and g.stat(K.STAT_NUPDATE) == log["done"], log
assert g.stat(K.STAT_NFORREST) > 0, "no Forrest-Tomlin update among them: the row etas would not be exercised"
rhs = rng.standard_normal((9, m))
x = g.solve_dense_multi(rhs, "T")   # the twin's first solve_dense does the garbage permutation, as the prelude did
same_columns(x, o, rhs, "T", "updated")
same_columns(g.solve_dense_multi(rhs, "N"), o, rhs, "N", "updated")
# 4 more lock-step rounds (solve_for_update both ways with solutions, update, and run_updates' own dense and sparse solves):
# pattern, bits and statistics still the twin's, so the one garbage permutation and the one marker step left the handle
# where one single call would have
log2 = U.run_updates(g, cols, m, 4, rng, pair_row=pr, twin=o)
assert log2["done"] >= 1, log2
same_columns(g.solve_dense_multi(rhs, "N"), o, rhs, "N", "updated again")
x = rhs.copy()
assert L.blu_hip_solve_dense_multi(g._h, 9, x.ctypes.data, m, x.ctypes.data, m, b"T", 0) == K.OK
same_columns(x, o, rhs, "T", "updated again, in place")
for key in (K.STAT_NFORREST, K.STAT_NUPDATE, K.STAT_R_NZ, K.STAT_U_NZ, K.STAT_NSYMPERM_TOTAL, K.STAT_NFORREST_TOTAL, K.STAT_DEV_NUNSYMPERM_TOTAL):
    assert g.stat(key) == o.stat(key), key
print("MULTI UPDATED OK")
"""

CHILD_STATUS = r"""
cp, ri, v = orc.gen_lp_basis(150, 5, 4, 0.8, 3, 0.6)
g, o = pair(cp, ri, v)
m = g.m
rhs = np.random.default_rng(3).standard_normal((2, m))


def call(h, nrhs, r, ldr, x, ldl, tr=b"N"):
    return L.blu_hip_solve_dense_multi(h, nrhs, r, ldr, x, ldl, tr, 0)


X = np.full((2, m), SENT)
rp, xp = rhs.ctypes.data, X.ctypes.data
assert call(None, 2, rp, m, xp, m) == K.ERROR_ARGUMENT_MISSING
hnone = blu_amd.BLU(120, 500)                                        # never factorized
assert call(hnone._h, 2, rp, 120, xp, 120) == K.ERROR_INVALID_CALL
assert call(hnone._h, 2, None, 120, xp, 120) == K.ERROR_INVALID_CALL  # the factorization is checked before the pointers
hbad = blu_amd.BLU(150, len(ri))                                     # last factorize refused
bad_i = ri.copy()
bad_i[3] = 999
assert hbad.factorize(cp[:-1], cp[1:], bad_i, v) == K.ERROR_INVALID_ARGUMENT
assert call(hbad._h, 2, rp, m, xp, m) == K.ERROR_INVALID_CALL
assert call(g._h, 2, None, m, xp, m) == K.ERROR_ARGUMENT_MISSING
assert call(g._h, 2, rp, m, None, m) == K.ERROR_ARGUMENT_MISSING
assert call(g._h, -1, None, m, xp, m) == K.ERROR_ARGUMENT_MISSING      # the pointers are checked before the counts
assert call(g._h, -1, rp, m, xp, m) == K.ERROR_INVALID_ARGUMENT
assert call(g._h, 2, rp, m - 1, xp, m) == K.ERROR_INVALID_ARGUMENT
assert call(g._h, 2, rp, m, xp, m - 1) == K.ERROR_INVALID_ARGUMENT
assert call(g._h, 0, rp, 0, xp, 0) == K.OK                           # nrhs == 0: nothing written, leading dimensions not looked at
assert (X == SENT).all()
hz = blu_amd.BLU(0, 1)                                               # m == 0
e = np.zeros(0, np.uint64)
assert hz.factorize(e, e, e, np.zeros(0)) == K.OK
assert call(hz._h, 2, rp, 0, xp, 0) == K.OK and (X == SENT).all()
assert hz.solve_dense_multi(np.zeros((3, 0))).shape == (3, 0)
assert call(g._h, 1, rp, 0, xp, 0) == K.OK                           # one right-hand side: the leading dimensions are not used
assert np.array_equal(X[0], o.solve_dense(rhs[0], "N")) and (X[1] == SENT).all()
for h, w in ((hnone, K.ERROR_INVALID_CALL), (hbad, K.ERROR_INVALID_CALL)):
    try:
        h.solve_dense_multi(np.zeros((2, h.m)))
    except blu_amd.BluError as err:
        assert err.status == w
    else:
        raise AssertionError("not refused")
# afterwards the single call and the multi call answer with the oracle's bits
for tr in "NT":
    assert np.array_equal(g.solve_dense(rhs[1], tr), o.solve_dense(rhs[1], tr)), tr
    same_columns(g.solve_dense_multi(rhs, tr), o, rhs, tr, "after the refusals")
assert hbad.factorize(cp[:-1], cp[1:], ri, v) == K.OK
same_columns(hbad.solve_dense_multi(rhs, "N"), o, rhs, "N", "refactorized")
print("MULTI STATUS OK")
"""


REPLAY = os.path.join(ROOT, "blu_amd", "emu_replay")
REPLAY_ASAN = os.path.join(ROOT, "blu_amd", "emu_replay_asan")
OP_MULTI_WS, OP_DENSE_MULTI = 10, 11  # tools/emu_replay.cpp


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def run_child(emu_lib, body, ok):
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1")
    out = subprocess.run([sys.executable, "-c", (HEAD + body) % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and ok in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


def test_multi_fresh_factorizations_on_the_cpu(emu_lib):
    """k_solve_dense_multi: two LP bases, a rank-deficient one and one whose U columns, L rows and U rows exceed 64 entries
    (asserted: the tail loops of k_sweep.h); nrhs 1, 2 and 65, all four trans letters; in place and out of place with
    ldrhs = m + 3, ldlhs = m + 5 (NaN padding not read, sentinel padding not written); every column the oracle's bits"""
    run_child(emu_lib, CHILD_FRESH, "MULTI FRESH OK")


def test_multi_chunking_on_the_cpu(emu_lib):
    """dbg_set_multi_ws_bytes so that 5 columns fit, nrhs = 23: chunks of 5, 5, 5, 5 and 3 give the bits of the one-chunk
    call and of the oracle; a limit below one column works them one at a time"""
    run_child(emu_lib, CHILD_CHUNK, "MULTI CHUNK OK")


def test_multi_after_updates_in_lockstep_on_the_cpu(emu_lib):
    """k_garbage_perm + k_solve_dense_upd_multi after 8 update rounds in lock step with the twin (no dense solve in
    between, so the garbage permutation has work to do), both systems; then 4 more lock-step rounds with every status,
    pattern, value and counter still the twin's, and the multi-solves again"""
    run_child(emu_lib, CHILD_UPDATED, "MULTI UPDATED OK")


def test_multi_statuses_on_the_cpu(emu_lib):
    """every refusal of blu_hip_solve_dense_multi in the order of the single entry, nrhs == 0 and m == 0 writing nothing,
    INVALID_CALL for a never-factorized handle and one whose last factorize was refused; afterwards solve_dense and
    solve_dense_multi still answer with the oracle's bits"""
    run_child(emu_lib, CHILD_STATUS, "MULTI STATUS OK")


def test_multi_replay_under_address_sanitizer(emu_lib, oracle, tmp_path):
    """A tape of tools/emu_replay.cpp recorded from the oracle alone: multi-solves on a fresh factorization (in one chunk
    with padded leading dimensions, and in chunks of 4 with the last one partial), 8 update rounds, multi-solves of both
    systems on the updated factors, further update rounds and single solves.  The replayer builds host blocks that end
    with the last column, so a read or write of the entry or of k_solve_dense_multi / k_garbage_perm /
    k_solve_dense_upd_multi outside them, outside the work vectors or outside the staging block is an AddressSanitizer
    report.  Replayed with the plain build (tape and replayer are right) and with the sanitized one (the executable
    carries the sanitizer runtime; nothing is preloaded)."""
    import numpy as np

    from blu_amd import keys as K
    from tests import util_update as U
    from tests.test_emu_cpu_solves import Tape

    class MultiTape(Tape):
        def set_multi_ws_bytes(self, n):
            self._i(OP_MULTI_WS, n)

        def solve_dense_multi(self, rhs, trans, ldr, ldl):
            x = np.array([self.o.solve_dense(r, trans) for r in rhs])
            self._i(OP_DENSE_MULTI, ord(trans), len(rhs), ldr, ldl)
            self._f(rhs.ravel())
            self._i(K.OK)
            self._f(x.ravel())

    subprocess.check_call(["make", "-s", "-C", CSRC, "emu_replay", "emu_replay_asan"])
    m = 96
    cp, ri, v = oracle.gen_lp_basis(m, 5, 5, 0.4, 6, 0.5)
    t = MultiTape(oracle)
    t.new(m, len(ri), 64 * len(ri) + 1024)
    assert t.factorize(cp, ri, v) == K.OK
    rng = np.random.default_rng(12)
    rhs = rng.standard_normal((11, m))
    stride = (m + 2 + 31) // 32 * 32
    for tr in "NT":
        t.solve_dense_multi(rhs, tr, m + 3, m + 5)
    t.set_multi_ws_bytes(4 * 2 * 8 * stride)
    for tr in "NT":
        t.solve_dense_multi(rhs, tr, m, m)
    cols = U.columns_of(cp, ri, v)
    assert U.run_updates(t, cols, m, 8, rng, check_every=10 ** 9)["done"] >= 3
    for tr in "TN":
        t.solve_dense_multi(rhs, tr, m + 1, m)
    t.set_multi_ws_bytes(-1)
    assert U.run_updates(t, cols, m, 3, rng)["done"] >= 1
    for tr in "NT":
        t.solve_dense_multi(rhs[:5], tr, m, m + 2)
    for key in (K.STAT_NUPDATE, K.STAT_NFORREST, K.STAT_R_NZ, K.STAT_U_NZ):
        t.stat(key)
    tape = str(tmp_path / "multi.tape")
    t.write(tape)
    env = {k: v for k, v in os.environ.items() if k != "BLU_HIP_LIB"}
    env.update(BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    for exe in (REPLAY, REPLAY_ASAN):
        out = subprocess.run([exe, tape], env=env, capture_output=True, text=True, timeout=900)
        assert "AddressSanitizer" not in out.stderr, out.stderr[-6000:]
        assert out.returncode == 0 and "REPLAY OK" in out.stdout, (exe, out.returncode, out.stdout[-500:] + out.stderr[-4000:])
