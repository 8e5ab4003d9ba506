"""The resident constraint matrix on the CPU: the emulation build of the library (blu_amd/csrc `make emu`, as in
tests/test_emu_cpu_maxvolume.py) runs blu_hip_set_matrix, _factorize_columns, _solve_for_update_column, _tableau_row and
_price -- k_scatter_lhs, k_at_dot and the host side -- beside a second handle driven by the single entries and beside the
summation order of the contract restated in numpy (tests/util_matrix.at_dot).  Equalities of bits only.  Each case runs in
a child process: the library path is fixed when blu_amd is first imported."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")
REPLAY = os.path.join(ROOT, "blu_amd", "emu_replay")
REPLAY_ASAN = os.path.join(ROOT, "blu_amd", "emu_replay_asan")
OP_SET_MATRIX, OP_FACT_COLUMNS, OP_FORUPD_COLUMN, OP_TABLEAU_ROW, OP_PRICE = 19, 20, 21, 22, 23  # tools/emu_replay.cpp

HEAD = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, sys.argv[1])
import blu_amd
from blu_amd import keys as K
from tests import util_maxvolume as MV
from tests import util_matrix as MX
assert b"gfx950" in blu_amd.lib().blu_hip_version()
INVARG, MISS, INVCALL = K.ERROR_INVALID_ARGUMENT, K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_CALL


def pair(name):
    # the matrix, the handle of the new entries with A set, a second handle for the single entries, the start basis
    m, ncol, a = MX.MATRICES[name]()
    g, s = blu_amd.BLU(m, len(a[1])), blu_amd.BLU(m, len(a[1]))
    assert g.set_matrix(ncol, *a) == K.OK
    basis, isbasic = MV.start(m, ncol)
    return m, ncol, a, g, s, basis, isbasic


def factorized(name):
    m, ncol, a, g, s, basis, isbasic = pair(name)
    assert g.factorize_columns(basis) == s.factorize(*MX.gathered(a, basis)) == K.OK
    return m, ncol, a, g, s, basis, isbasic
"""

CHILD_FACTORIZE = r"""
m, ncol, a, g, s, basis, isbasic = factorized(sys.argv[2])
fg, fs = g.get_factors(), s.get_factors()
for k in fg:
    assert np.array_equal(fg[k], fs[k]) and (fg[k].dtype != np.float64 or MX.same_bits(fg[k], fs[k])), k
ALL = MV.STATS + (K.STAT_L_NZ, K.STAT_MIN_PIVOT, K.STAT_MAX_PIVOT, K.STAT_UPDATE_COST_DENOM, K.STAT_MATRIX_NZ, K.STAT_RANK, K.STAT_BUMP_SIZE,
                  K.STAT_BUMP_NZ, K.STAT_NSEARCH_PIVOT, K.STAT_FACTOR_FLOPS, K.STAT_CONDEST_L, K.STAT_CONDEST_U, K.STAT_RESIDUAL_TEST)
MX.same_handles(g, s, a, "factorize_columns", ALL)
# a basis that is not the start: the last m columns with entries, in descending order
other = [j for j in range(ncol - 1, -1, -1) if a[0][j + 1] > a[0][j]][:m]
assert g.factorize_columns(other) == s.factorize(*MX.gathered(a, other))
MX.same_handles(g, s, a, "factorize_columns, another basis", MV.STATS + (K.STAT_L_NZ, K.STAT_RANK))
print("MATRIX FACTORIZE OK")
"""

CHILD_ROWS = r"""
m, ncol, a, g, s, basis, isbasic = factorized(sys.argv[2])
for skip in (None, isbasic):
    MX.check_tableau_rows(g, a, m, skip, ("fresh", skip is None), s)
MX.update_pair(g, s, a, basis, isbasic, int(sys.argv[3]), "updates")
assert g.stat(K.STAT_NUPDATE) == int(sys.argv[3])
for skip in (None, isbasic):
    MX.check_tableau_rows(g, a, m, skip, ("updated", skip is None), s)
MX.same_handles(g, s, a, "after the rows")
print("MATRIX ROWS OK")
"""

CHILD_PRICE = r"""
counts = {}
for name in ("M0", "M1"):
    m, ncol, a, g, s, basis, isbasic = pair(name)
    before = [g.stat(k) for k in MV.STATS]
    MX.check_price(g, a, m, isbasic, name)  # (no factorization)
    assert np.array_equal([g.stat(k) for k in MV.STATS], before, equal_nan=True)  # (UPDATE_COST of a handle without factors is 0 / 0)
    assert g.factorize_columns(basis) == K.OK
    MX.check_price(g, a, m, isbasic, name + ", factorized")
    y = MX.price_vectors(m)[0]
    for skip in (None, isbasic):
        g.price(y, skip)
        counts[(name, "price", skip is None)] = g.dbg_matrix_counts()
        assert g.tableau_row(1, False, skip)[0] == K.OK
        counts[(name, "row", skip is None)] = g.dbg_matrix_counts()
        assert g.tableau_row(2, False, skip, want_solution=True)[0] == K.OK
        assert g.dbg_matrix_counts() == counts[(name, "row", skip is None)]
    # the cost claim: launches and synchronizes the same for both matrices and with or without skip
    for what, launches, uploads in (("price", 1, 1), ("row", 2, 0)):
        for no_skip in (True, False):
            c = counts[(name, what, no_skip)]
            assert c == (launches, 1, uploads + (0 if no_skip else 1), 8 * ncol), (name, what, no_skip, c)
print(counts)
print("MATRIX PRICE OK")
"""

CHILD_REFUSALS = r"""
L = blu_amd.lib()
SET, FACT, COL, ROW, PRICE = L.blu_hip_set_matrix, L.blu_hip_factorize_columns, L.blu_hip_solve_for_update_column, L.blu_hip_tableau_row, L.blu_hip_price
SET.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 3
FACT.argtypes = [C.c_void_p, C.c_void_p]
COL.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 3
ROW.argtypes = [C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 5
PRICE.argtypes = [C.c_void_p] * 4
ptr = lambda x: None if x is None else x.ctypes.data

m, ncol, a = MX.MATRICES["M0"]()
g = blu_amd.BLU(m, len(a[1]))
basis, isbasic = MV.start(m, ncol)
b64 = np.array(basis, np.int64)
y = MX.price_vectors(m)[0]
alpha = np.zeros(ncol)


def four(h):
    # the four entries that need a set matrix, with arguments that are otherwise in order
    return [FACT(h, ptr(b64)), COL(h, ncol - 1, None, None, None), ROW(h, 0, 0, None, ptr(alpha), None, None, None),
            ROW(h, 0, 1, None, ptr(alpha), None, None, None), PRICE(h, ptr(y), None, ptr(alpha))]


# ---- before any set_matrix: INVALID_CALL, also on a handle with a factorization
assert four(g._h) == [INVCALL] * 5
assert g.factorize(*MX.gathered(a, basis)) == K.OK
assert four(g._h) == [INVCALL] * 5
assert FACT(None, ptr(b64)) == COL(None, 0, None, None, None) == ROW(None, 0, 0, None, ptr(alpha), None, None, None) == MISS
assert PRICE(None, ptr(y), None, ptr(alpha)) == SET(None, ncol, ptr(a[0]), ptr(a[1]), ptr(a[2])) == MISS

# ---- set_matrix refusals: nothing is touched -- statistics, a held solve_sparse_multi result, the previous matrix
assert g.set_matrix(ncol, *a) == K.OK
sts, sols = g.solve_sparse_multi([MX.column(a, ncol - 1)[0], [0]], [MX.column(a, ncol - 1)[1], [1.0]], "T")
total = sum(len(il) for il, _ in sols)
held = g.get_sparse_multi(total)
ALL = MV.STATS + (K.STAT_L_NZ, K.STAT_MIN_PIVOT, K.STAT_MAX_PIVOT, K.STAT_UPDATE_COST_DENOM)
stats = [g.stat(k) for k in ALL]
z0 = g.price(y)
assert MX.same_bits(z0, MX.at_dot(a[0], a[1], a[2], y))


def untouched(what):
    assert [g.stat(k) for k in ALL] == stats, what
    again = g.get_sparse_multi(total)
    assert np.array_equal(again[0], held[0]) and MX.same_bits(again[1], held[1]), what
    assert MX.same_bits(g.price(y), z0), what


down = a[0].copy()
down[20] = down[21] + 1
huge = np.array([0, 2 ** 31], np.uint64)
at_m = a[1].copy()
at_m[len(at_m) // 2] = m
for want, args in ((MISS, (ncol, None, a[1], a[2])), (INVARG, (-1, a[0], a[1], a[2])), (INVARG, (2 ** 31, a[0], a[1], a[2])),
                   (INVARG, (ncol, down, a[1], a[2])), (INVARG, (1, huge, a[1], a[2])), (MISS, (ncol, a[0], None, a[2])),
                   (MISS, (ncol, a[0], a[1], None)), (INVARG, (ncol, a[0], at_m, a[2]))):
    assert SET(g._h, args[0], ptr(args[1]), ptr(args[2]), ptr(args[3])) == want, (want, args[0])
    untouched(("set_matrix", want, args[0]))

# ---- the other entries
off, neg = b64.copy(), b64.copy()
off[3] = ncol
neg[0] = -1
assert FACT(g._h, None) == MISS and FACT(g._h, ptr(off)) == INVARG and FACT(g._h, ptr(neg)) == INVARG
untouched("factorize_columns")
assert COL(g._h, -1, None, None, None) == INVARG and COL(g._h, ncol, None, None, None) == INVARG
for prep in (0, 1):
    assert ROW(g._h, 0, prep, None, None, None, None, None) == MISS
    assert ROW(g._h, m, prep, None, ptr(alpha), None, None, None) == INVARG and ROW(g._h, -1, prep, None, ptr(alpha), None, None, None) == INVARG
assert PRICE(g._h, None, None, ptr(alpha)) == MISS and PRICE(g._h, ptr(y), None, None) == MISS
untouched("solve_for_update_column, tableau_row, price")
f = blu_amd.BLU(m, len(a[1]))  # a matrix but no factorization: the solves refuse, price works
assert f.set_matrix(ncol, *a) == K.OK
assert COL(f._h, 0, None, None, None) == ROW(f._h, 0, 0, None, ptr(alpha), None, None, None) == ROW(f._h, 0, 1, None, ptr(alpha), None, None, None) == INVCALL
assert MX.same_bits(f.price(y), z0)

# ---- the matrix survives factorize, the solves, an update, copy_batch in either role; a destination keeps its own
m1, ncol1, a1 = MX.MATRICES["M1"]()
assert g.factorize_columns(basis) == K.OK
s = blu_amd.BLU(m, len(a[1]))
assert s.factorize(*MX.gathered(a, basis)) == s.factorize(*MX.gathered(a, basis)) == K.OK  # (g's second factorization as well)
MX.update_pair(g, s, a, basis, isbasic, 2, "survives")
c = g.clone()
assert four(c._h) == [INVCALL] * 5  # (not copied)
sub = (a[0][:ncol - 4], a[1], a[2])
assert c.set_matrix(ncol - 5, *sub) == K.OK
assert blu_amd.copy_batch(g, [c]) == [K.OK] and blu_amd.copy_batch(c, [s]) == [K.OK]
assert MX.same_bits(c.price(y), z0[:ncol - 5]) and MX.same_bits(g.price(y), z0)
r1, r2 = c.tableau_row(1, False), g.tableau_row(1, False)
assert r1[0] == r2[0] == K.OK and MX.same_bits(r1[1], r2[1][:ncol - 5])

# ---- after blu_hip_maxvolume the matrix is gone until the next set_matrix
b2, i2 = MV.start(m, ncol)
assert g.maxvolume(ncol, a[0], a[1], a[2], b2, i2, 1.0)[0] == K.OK
assert four(g._h) == [INVCALL] * 5
assert g.set_matrix(ncol, *a) == K.OK and MX.same_bits(g.price(y), z0) and g.tableau_row(0, False)[0] == K.OK

# ---- ncol == 0
e_u, e_f = np.zeros(0, np.uint64), np.zeros(0)
assert g.set_matrix(0, np.zeros(1, np.uint64), e_u, e_f) == K.OK
st, al = g.tableau_row(0, False, want_solution=True)
assert st == K.OK and len(al) == 0 and g.nzlhs > 0 and g.dbg_matrix_counts() == (0, 0, 0, 0)
assert ROW(g._h, 0, 0, None, None, None, None, None) == K.OK  # (alpha may be NULL)
assert len(g.price(y)) == 0 and FACT(g._h, ptr(b64)) == INVARG and COL(g._h, 0, None, None, None) == INVARG

# ---- m == 0
z = blu_amd.BLU(0, 1)
assert z.set_matrix(1, np.array([0, 1], np.uint64), np.zeros(1, np.uint64), np.ones(1)) == INVARG  # (row 0 is not below m)
assert four(z._h)[4] == INVCALL
assert z.set_matrix(3, np.zeros(4, np.uint64), e_u, e_f) == K.OK
pz = z.price(e_f, [0, 1, 0])
assert len(pz) == 3 and not np.any(pz.view(np.uint64))
assert COL(z._h, 0, None, None, None) == INVCALL
assert z.factorize_columns([]) == K.OK and z.stat(K.STAT_NFACTORIZE) == 1
assert COL(z._h, 0, None, None, None) == INVARG
assert z.tableau_row(0, False)[0] == INVARG and z.tableau_row(0, True)[0] == INVARG
print("MATRIX REFUSALS OK")
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def run_child(emu_lib, body, ok, *args, timeout=1200):
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1")
    cmd = [sys.executable, "-c", HEAD + body, ROOT] + [str(x) for x in args]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and ok in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("name", ("M0", "M1"))
def test_factorize_columns_is_factorize_of_the_gathered_columns(emu_lib, name):
    """set_matrix, then factorize_columns(start basis) beside a second handle given the gathered columns: status, the
    canonical factors, every statistic of util_maxvolume.STATS and more, then solve_sparse of three columns in both systems;
    once more with a basis in another order"""
    run_child(emu_lib, CHILD_FACTORIZE, "MATRIX FACTORIZE OK", name)


@pytest.mark.parametrize("name,nupdates", (("M0", 3), ("M1", 3)))
def test_tableau_row_is_the_single_solve_and_the_numpy_order(emu_lib, name, nupdates):
    """tableau_row(r, 0, skip) for r in 0, 1, m - 1 and two more, with skip NULL and isbasic, on fresh factors and after
    updates made through solve_for_update_column + tableau_row(p, 1) + update beside a twin driven by the two single
    solve_for_update calls: alpha has the bits of at_dot of the y a clone's solve_sparse([r], [1.0], 'T') gives, skipped
    entries are +0.0, the solution and the flop counters are the clone's; the updated handle equals its twin"""
    run_child(emu_lib, CHILD_ROWS, "MATRIX ROWS OK", name, nupdates)


def test_price_and_the_cost_of_the_calls(emu_lib):
    """price with a random y, with -0.0 and zeros, with skip NULL, all ones and isbasic, with and without a factorization:
    the bits of at_dot (a NaN in y: equal_nan); dbg_matrix_counts of price and tableau_row -- launches, synchronizes,
    uploads, bytes -- are the same for M0 and M1 and with or without skip, up to the one upload of skip"""
    run_child(emu_lib, CHILD_PRICE, "MATRIX PRICE OK")


def test_refusals_and_the_lifetime_of_the_matrix(emu_lib):
    """every refusal of the five entries with what it must leave alone; INVALID_CALL before set_matrix and after
    blu_hip_maxvolume; a row index equal to m; the matrix survives factorize, solves, updates and copy_batch and is not
    copied; ncol == 0; m == 0"""
    run_child(emu_lib, CHILD_REFUSALS, "MATRIX REFUSALS OK")


def test_matrix_replay_under_address_sanitizer(emu_lib, oracle, tmp_path):
    """One tape of the five entries on M1, recorded from the oracle and at_dot alone: set_matrix, factorize_columns, rows with
    and without skip and solution, prices, three updates through solve_for_update_column + tableau_row(p, 1), rows again.
    The replayer's host arrays end with their last entry, so an access of k_at_dot or k_scatter_lhs outside A, y, skip or
    alpha is an AddressSanitizer report.  Replayed with the plain build and with the sanitized one (the executable carries
    the sanitizer runtime; nothing is preloaded)."""
    import numpy as np

    from blu_amd import keys as K
    from tests import util_matrix as MX
    from tests import util_maxvolume as MV
    from tests.test_emu_cpu_solves import Tape

    class MatrixTape(Tape):
        def set_matrix(self, a):
            self.a = a
            self.ncol = len(a[0]) - 1
            self._i(OP_SET_MATRIX, self.ncol)
            self._u(a[0])
            self._u(a[1])
            self._f(a[2])
            self._i(K.OK)

        def factorize_columns(self, basis):
            b = np.asarray(basis, np.int64)
            st = self.o.factorize(self.a[0][b], self.a[0][b + 1], self.a[1], self.a[2])
            self._i(OP_FACT_COLUMNS, *basis)
            self._i(st)
            return st

        def solve_for_update_column(self, j, want=True):
            self._i(OP_FORUPD_COLUMN, j, 1 if want else 0)
            ci, cx = MX.column(self.a, j)
            return self._solution(*self.o.solve_for_update(ci, cx, "N", want), want=want)

        def tableau_row(self, r, prepare, skip, want):
            self._i(OP_TABLEAU_ROW, r, 1 if prepare else 0, 0 if skip is None else 1)
            if skip is not None:
                self._i(*skip)
            self._i(1 if want else 0)
            st, il, lhs = self.o.solve_for_update([r], None, "T", True) if prepare else self.o.solve_sparse([r], [1.0], "T")
            self._i(st)
            assert st == K.OK
            self._f(MX.at_dot(self.a[0], self.a[1], self.a[2], lhs, skip))
            if want:
                self._i(len(il))
                self._i(*il)
                self._f(lhs)
            return il, lhs

        def price(self, y, skip):
            self._i(OP_PRICE, 0 if skip is None else 1)
            if skip is not None:
                self._i(*skip)
            self._f(y)
            self._i(K.OK)
            self._f(MX.at_dot(self.a[0], self.a[1], self.a[2], y, skip))

    subprocess.check_call(["make", "-s", "-C", CSRC, "emu_replay", "emu_replay_asan"])
    m, ncol, a = MX.m1()
    t = MatrixTape(oracle)
    t.new(m, len(a[1]), 64 * len(a[1]) + 1024)
    t.set_matrix(a)
    basis, isbasic = MV.start(m, ncol)
    assert t.factorize_columns(basis) == K.OK
    y = MX.price_vectors(m)[0]

    def rows():
        for r in MX.rows_of(m):
            t.tableau_row(r, False, isbasic if r % 2 else None, want=r != 1)
            for key in MX.FLOPS:
                t.stat(key)
        t.price(y, None)
        t.price(y, isbasic)

    rows()
    done = 0
    for j in range(ncol - 1, m - 1, -1):
        if len(MX.column(a, j)[0]) == 0:
            continue
        st, il, lhs = t.solve_for_update_column(j)
        assert st == K.OK
        p = int(il[np.argmax(np.abs(lhs[il]))])
        if abs(lhs[p]) < 0.05:
            continue
        xtbl = float(lhs[p])
        t.tableau_row(p, True, isbasic, want=done != 1)
        assert t.update(xtbl) == K.OK
        isbasic[basis[p]], isbasic[j], basis[p] = 0, 1, j
        done += 1
        if done == 3:
            break
    assert done == 3
    for key in MV.STATS[:-1]:
        t.stat(key)
    rows()
    tape = str(tmp_path / "matrix.tape")
    t.write(tape)
    env = {k: v for k, v in os.environ.items() if k != "BLU_HIP_LIB"}
    env.update(BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    for exe in (REPLAY, REPLAY_ASAN):
        out = subprocess.run([exe, tape], env=env, capture_output=True, text=True, timeout=1800)
        assert "AddressSanitizer" not in out.stderr, out.stderr[-6000:]
        assert out.returncode == 0 and "REPLAY OK" in out.stdout, (exe, out.returncode, out.stdout[-500:] + out.stderr[-4000:])
