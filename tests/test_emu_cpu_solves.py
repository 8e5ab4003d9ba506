"""What a simplex code calls between two factorizations, on the CPU: solve_dense (single and batched), the triangular
sweeps of the statistics, solve_sparse, solve_for_update, update and the solves on updated factors, run by the emulation
build of the library (blu_amd/csrc `make emu`, as in tests/test_emu_cpu.py) and compared with the oracle BIT FOR BIT
(np.array_equal; the oracle with the 64-bit cancellation mask, set_fix_d3, as elsewhere).  The emulator's scheduler
reports lanes that meet in different collectives, and the last test replays the same calls under AddressSanitizer
(tools/emu_replay.cpp, `make emu_replay_asan`: the sanitized executable carries the runtime, nothing is preloaded).

Single handles with the one-wave pivot kernel (BLU_PIVOT_KERNEL=1) and the one-workgroup statistics and solves
(BLU_HIP_NO_CHAIN=1): the chain pipeline (k_chain.hip) spins on LDS flags and is not validated under the emulator
(DESIGN.md section 4b).  Each case runs in a child process: the library path is fixed when blu_amd is first imported."""
import os
import subprocess
import sys

import numpy as np
import pytest

from blu_amd import keys as K
from tests import util_update as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")
REPLAY = os.path.join(ROOT, "blu_amd", "emu_replay")
REPLAY_ASAN = os.path.join(ROOT, "blu_amd", "emu_replay_asan")
DFS_RING = 2048  # k_solve_sparse.hip
DEEP_M = 2300

HEAD = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
import blu_amd
from blu_amd import keys as K
from oracle import orc
from tests import util, util_update as U
assert b"gfx950" in blu_amd.lib().blu_hip_version()
FSTATS = ("CONDEST_L", "CONDEST_U", "NORM_L", "NORM_U", "NORMEST_L_INV", "NORMEST_U_INV", "ONENORM", "INFNORM", "RESIDUAL_TEST")


def pair(cp, ri, v, want=K.OK, b_nz=None, params=None):
    m = len(cp) - 1
    g = blu_amd.BLU(m, len(ri) if b_nz is None else b_nz)
    o = orc.OracleBLU(m, 64 * len(ri) + 1024)
    o.set_fix_d3(True)
    for key, val in (params or {}).items():
        g.set_param(key, val)
        o.set_param(key, val)
    sg, so = g.factorize(cp[:-1], cp[1:], ri, v), o.factorize(cp[:-1], cp[1:], ri, v)
    assert sg == so == want, (sg, so, want)
    return g, o


def same_stats(g, o, where):
    for c in FSTATS:
        a, b = g.stat(getattr(K, "STAT_" + c)), o.stat(getattr(K, "STAT_" + c))
        assert a == b, (where, c, a, b)


def same_sparse(g, o, ir, xr, trans, where, flops=True):
    a, b = U._ss(g, ir, xr, trans), U._ss(o, ir, xr, trans)
    assert a[0] == b[0] == K.OK, (where, a[0], b[0])
    assert g.nzlhs == len(b[1]), (where, g.nzlhs, len(b[1]))
    U._same(a, b, where)
    if flops:
        for c in (K.STAT_L_FLOPS, K.STAT_U_FLOPS):
            assert g.stat(c) == o.stat(c), (where, c, g.stat(c), o.stat(c))
    return int(g.stat(43))  # branch of the second triangular solve: 1 symbolic + sparse, 2 sequential


def bidiagonal(m, diag=1.0):
    # B = diag * I + superdiagonal of ones: column j holds rows j - 1 and j
    cp = np.concatenate(([0], np.arange(1, 2 * m, 2))).astype(np.uint64)
    ri = np.concatenate([[j - 1, j] if j else [0] for j in range(m)]).astype(np.uint64)
    v = np.where(np.concatenate([[0, 1] if j else [1] for j in range(m)]) == 1, diag, 1.0)
    return cp, ri, v


def pair_rows(g):
    f = g.get_factors()
    pr = np.zeros(g.m, np.int64)
    pr[f["colperm"]] = f["rowperm"]
    return pr
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def emu_env(emu_lib):
    return dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1")


def run_child(emu_lib, body, ok, timeout=900):
    out = subprocess.run([sys.executable, "-c", (HEAD + body) % {"root": ROOT, "deep_m": DEEP_M}], env=emu_env(emu_lib), capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0 and ok in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


CHILD_DENSE = r"""
rng = np.random.default_rng(5)


def dense_block_basis(m, lo, hi, seed):
    # gen_lp_basis plus a dense block on rows / columns lo..hi-1: U columns, U rows, L columns and L rows of up to hi - lo entries
    cp, ri, v = orc.gen_lp_basis(m, 5, 5, 0.5, seed, 0.3)
    r = np.random.default_rng(seed)
    cols = [dict(zip(ri[cp[j]:cp[j + 1]].astype(np.int64).tolist(), v[cp[j]:cp[j + 1]].tolist())) for j in range(m)]
    for j in range(lo, hi):
        for i in range(lo, hi):
            cols[j][i] = cols[j].get(i, 0.0) + float(r.uniform(-1.0, 1.0))
    nri = np.concatenate([sorted(c) for c in cols]).astype(np.uint64)
    nv = np.concatenate([[c[i] for i in sorted(c)] for c in cols])
    ncp = np.concatenate(([0], np.cumsum([len(c) for c in cols]))).astype(np.uint64)
    return ncp, nri, nv


def scaled(cp, v, cols):
    v = v.copy()
    for j in cols:
        v[int(cp[j]):int(cp[j + 1])] *= 1e-17
    return v


def check_single(cp, ri, v, want, where):
    g, o = pair(cp, ri, v, want)
    same_stats(g, o, where)
    for trans in "NT":
        b = rng.standard_normal(len(cp) - 1)
        assert np.array_equal(g.solve_dense(b, trans), o.solve_dense(b, trans)), (where, trans)
    return g, o


# ---- single handles: full rank and rank deficient
cp, ri, v = orc.gen_lp_basis(200, 6, 6, 0.5, 1, 0.3)
check_single(cp, ri, v, K.OK, "m200")
check_single(cp, ri, scaled(cp, v, (3, 200 // 3, 199)), K.WARNING_SINGULAR_MATRIX, "m200 singular")
# ---- lines of more than 64 entries: the tail loops of k_sweep.h
cp, ri, v = dense_block_basis(130, 20, 110, 3)
g, o = check_single(cp, ri, v, K.OK, "dense block")
f = o.get_factors()
ucol = int(np.diff(f["u_colptr"]).max()) - 1                      # without the pivot
lrow = int(np.bincount(f["l_rowidx"], minlength=130).max()) - 1   # without the unit diagonal
lcol = int(np.diff(f["l_colptr"]).max()) - 1
urow = int(np.bincount(f["u_rowidx"], minlength=130).max()) - 1
assert min(ucol, lrow, lcol, urow) > 64, (ucol, lrow, lcol, urow)
print("LONG", ucol, lrow, lcol, urow)
check_single(cp, ri, scaled(cp, v, (5, 60, 129)), K.WARNING_SINGULAR_MATRIX, "dense block singular")

# ---- a batch of three members of different m, full rank and rank deficient, one of them after updates
specs = [(200, 6, 6, 0.5, 1, 0.3), (150, 5, 4, 0.8, 3, 0.6), (90, 4, 5, 0.3, 7, 0.5)]
mats = [orc.gen_lp_basis(*s) for s in specs]
mats[1] = (mats[1][0], mats[1][1], scaled(mats[1][0], mats[1][2], (2, 75)))
hs, os_ = [], []
for (cp, ri, v), want in zip(mats, (K.OK, K.WARNING_SINGULAR_MATRIX, K.OK)):
    g, o = pair(cp, ri, v, want)
    same_stats(g, o, len(cp) - 1)
    hs.append(g)
    os_.append(o)
for round_ in range(2):
    for trans in "NT":
        rhs = [rng.standard_normal(h.m) for h in hs]
        sols, st = blu_amd.solve_dense_batch(hs, rhs, trans)
        assert st == [K.OK] * 3, st
        for k, (x, o, r, h) in enumerate(zip(sols, os_, rhs, hs)):
            assert np.array_equal(x, o.solve_dense(r, trans)), (round_, trans, k)
            assert np.array_equal(x, h.solve_dense(r, trans)), (round_, trans, k, "single")
    if round_ == 0:  # the third member goes on with an updated factorization: k_solve_dense_upd_batch
        cp, ri, v = mats[2]
        log = U.run_updates(hs[2], U.columns_of(cp, ri, v), 90, 8, np.random.default_rng(2), pair_row=pair_rows(hs[2]), twin=os_[2])
        assert log["done"] >= 3 and hs[2].stat(K.STAT_NUPDATE) == log["done"], log
print("DENSE OK")
"""


def test_solve_dense_and_statistics_on_the_cpu(emu_lib):
    """k_solve_dense, k_solve_dense_batch, k_build_lt(_batch), k_solve_dense_upd(_batch) and every sweep of k_stats: both
    systems and all nine statistics (the condition estimates and RESIDUAL_TEST included) on full-rank and rank-deficient
    factors (columns scaled by 1e-17), a basis with a dense block whose U columns, U rows, L columns and L rows exceed 64
    entries (asserted: the tail loops of k_sweep.h), and a batch of three members of different m, one of which is solved
    again after updates."""
    out = run_child(emu_lib, CHILD_DENSE, "DENSE OK")
    assert all(int(x) > 64 for x in out.split("LONG")[1].split()[:4]), out[-500:]


CHILD_SPARSE = r"""
m = 240
cp, ri, v = orc.gen_lp_basis(m, 6, 6, 0.5, 1, 0.3)
g, o = pair(cp, ri, v)
seen = {0.05: set(), 0.0: set(), 1.0: set()}
for state in ("fresh", "updated"):
    if state == "updated":
        log = U.run_updates(g, U.columns_of(cp, ri, v), m, 6, np.random.default_rng(3), check_every=3, pair_row=pair_rows(g), twin=o)
        assert log["done"] >= 3 and g.stat(K.STAT_NUPDATE) == log["done"] > 0, log
    for thres in seen:
        g.set_param(K.PARAM_SPARSE_THRES, thres)
        o.set_param(K.PARAM_SPARSE_THRES, thres)
        for trans in "NT":
            for q, nz in enumerate((1, 2, 5, 17, m // 8, m // 2)):
                r = np.random.default_rng(100 * q + 7)
                ir, xr = r.choice(m, nz, replace=False), r.standard_normal(nz)
                seen[thres].add(same_sparse(g, o, ir, xr, trans, (thres, state, trans, nz)))
print("BRANCHES", seen)
assert seen[0.05] == {1, 2} and 2 in seen[0.0] and seen[1.0] == {1}, seen
print("SPARSE OK")
"""


def test_solve_sparse_on_the_cpu(emu_lib):
    """k_solve_sparse and k_solve_upd (mode 0): right-hand sides of 1, 2, 5, 17, m/8 and m/2 entries, both systems, on a fresh
    and on an updated factorization, SPARSE_THRES 0.05, 0.0 and 1.0: pattern order, nzlhs, values, L_FLOPS and U_FLOPS.
    Statistic 43 shows the symbolic and the sequential branch of the second triangular solve both taken with
    SPARSE_THRES 0.05, the sequential one with 0.0, and only the symbolic one with 1.0."""
    run_child(emu_lib, CHILD_SPARSE, "SPARSE OK")


CHILD_DEEP = r"""
m = %(deep_m)d
cp, ri, v = bidiagonal(m)
g, o = pair(cp, ri, v)
for thres in (0.05, 1.0):
    g.set_param(K.PARAM_SPARSE_THRES, thres)
    o.set_param(K.PARAM_SPARSE_THRES, thres)
    for trans, i, want in (("N", m - 1, m), ("T", 0, m), ("N", m // 2, m // 2 + 1), ("T", m // 2, m - m // 2)):
        same_sparse(g, o, [i], [1.0], trans, (thres, trans, i))
        assert g.nzlhs == want, (thres, trans, i, g.nzlhs, want)
print("DEEP OK")
"""


def test_dfs_deeper_than_the_lds_ring_on_the_cpu(emu_lib):
    """B = I + superdiagonal of ones, m = 2300 > DFS_RING = 2048: the reach of e_{m-1} ('N') and of e_0 ('T') is one chain of
    m nodes, so dfs_reach_wave wraps its LDS ring on the way down and refills it, 64 levels at a time, on the way back
    (nzlhs == m, nothing below droptol); e_{m/2} gives 1151 / 1150.  Pattern, values and flop counters equal the oracle's
    for SPARSE_THRES 0.05 and 1.0."""
    assert DEEP_M > DFS_RING + 64
    run_child(emu_lib, CHILD_DEEP, "DEEP OK")


CHILD_UPDATE = r"""
kinds = np.zeros(3)
for spec, nupd in (((60, 4, 5, 0.3, 7, 0.5), 60), ((280, 6, 6, 0.5, 1, 0.3), 10)):
    cp, ri, v = orc.gen_lp_basis(*spec)
    m = spec[0]
    g, o = pair(cp, ri, v)
    log = U.run_updates(g, U.columns_of(cp, ri, v), m, nupd, np.random.default_rng(spec[4]), pair_row=pair_rows(g), twin=o)
    assert log["done"] >= nupd * 0.5 and int(g.stat(K.STAT_NUPDATE)) == log["done"], log
    assert log["max_residual"] <= 1e-8 and log["max_pivot_error"] <= 1e-8, log
    now = np.array([g.stat(K.STAT_NFORREST_TOTAL), g.stat(K.STAT_NSYMPERM_TOTAL), g.stat(K.STAT_DEV_NUNSYMPERM_TOTAL)])
    assert np.array_equal(now, [o.stat(K.STAT_NFORREST_TOTAL), o.stat(K.STAT_NSYMPERM_TOTAL), o.stat(K.STAT_DEV_NUNSYMPERM_TOTAL)])
    print("KINDS", m, now)
    if m == 60:
        assert (now > 0).all(), now  # Forrest-Tomlin, symmetric and unsymmetric permutation updates all occurred
    assert util.status_of(g.get_factors) == K.ERROR_INVALID_CALL

# ---- maximum updates with host regrowth: tiny b_nz hint, 8 entries of arena slack (NEED_R / NEED_UC / NEED_W round trips)
spec = (24, 4, 4, 0.0, 5, 0.5)
cp, ri, v = orc.gen_lp_basis(*spec)
m = spec[0]
g = blu_amd.BLU(m, 4)
g.dbg_set_upd_extra(8)
o = orc.OracleBLU(m, 256 * len(ri))
o.set_fix_d3(True)
assert g.factorize(cp[:-1], cp[1:], ri, v) == o.factorize(cp[:-1], cp[1:], ri, v) == K.OK
log = U.run_updates(g, U.columns_of(cp, ri, v), m, 400, np.random.default_rng(11), check_every=5, stop_on_max=True, twin=o)
assert log["hit_maximum_updates"] and int(g.stat(K.STAT_NFORREST)) == m, log
assert log["max_residual"] <= 1e-7, log

# ---- call protocol: the statuses of tests/test_gpu_update.py::test_update_call_protocol, the oracle alongside
cp, ri, v = orc.gen_lp_basis(200, 5, 5, 0.5, 2, 0.3)
g = blu_amd.BLU(200, len(ri))
o = orc.OracleBLU(200, 64 * len(ri))
o.set_fix_d3(True)
assert g.solve_for_update([3], None, "T") == K.ERROR_INVALID_CALL
assert g.factorize(cp[:-1], cp[1:], ri, v) == o.factorize(cp[:-1], cp[1:], ri, v) == K.OK
assert g.update(1.0) == o.update(1.0) == K.ERROR_INVALID_CALL
assert g.solve_for_update([200], None, "T") == o.solve_for_update([200], None, "T")[0] == K.ERROR_INVALID_ARGUMENT
assert g.solve_for_update([1, 999], [1.0, 2.0], "N") == o.solve_for_update([1, 999], [1.0, 2.0], "N")[0] == K.ERROR_INVALID_ARGUMENT
assert g.solve_for_update([1], None, "N") == K.ERROR_ARGUMENT_MISSING
assert g.solve_for_update([3], None, "T", want_solution=False) == o.solve_for_update([3], None, "T", want_solution=False)[0] == K.OK
assert g.nzlhs == 0
assert g.update(1.0) == o.update(1.0) == K.ERROR_INVALID_CALL
a, b = int(cp[4]), int(cp[5])
U._same(U._sfu(g, ri[a:b], v[a:b], "N"), U._sfu(o, ri[a:b], v[a:b], "N"), "column 4")
assert abs(g.lhs[3]) < 1e-12
assert g.update(g.lhs[3]) == o.update(g.lhs[3]) == K.ERROR_SINGULAR_UPDATE
b1 = np.ones(200)
assert np.array_equal(g.solve_dense(b1), o.solve_dense(b1))  # the old factorization is still valid

# ---- hand-predictable: B = 2 I + superdiagonal; column 2 := 3 e_3 is an UNsymmetric permutation update, column 5 :=
# 7 e_5 + e_1 a SYMMETRIC one; neither needs a row eta
m = 8
cp, ri, v = bidiagonal(m, 2.0)
g, o = pair(cp, ri, v)
cols = U.columns_of(cp, ri, v)
for j, (ai, ax), key in ((2, ([3], [3.0]), K.STAT_DEV_NUNSYMPERM_TOTAL), (5, ([5, 1], [7.0, 1.0]), K.STAT_NSYMPERM_TOTAL)):
    U._same(U._sfu(g, [j], None, "T"), U._sfu(o, [j], None, "T"), ("T", j))
    U._same(U._sfu(g, ai, ax, "N"), U._sfu(o, ai, ax, "N"), ("N", j))
    before = g.stat(key)
    assert g.update(g.lhs[j]) == o.update(g.lhs[j]) == K.OK
    assert g.stat(key) == before + 1 == o.stat(key) and g.stat(K.STAT_NFORREST) == 0
    cols[j] = (np.array(ai, np.int64), np.array(ax))
    B = U.matrix_of(cols, m)
    b = np.arange(1.0, m + 1)
    for trans, A in (("N", B), ("T", B.T)):
        x = g.solve_dense(b, trans)
        assert np.array_equal(x, o.solve_dense(b, trans)) and U.backward_error(A, x, b) < 1e-15
        same_sparse(g, o, [4], [1.0], trans, ("bidiagonal", j, trans), flops=False)
        assert U.backward_error(A, g.lhs, np.eye(m)[4]) < 1e-15
print("UPDATE OK")
"""


def test_update_path_in_lockstep_on_the_cpu(emu_lib):
    """k_upd_init, k_solve_upd, k_update and the solves on updated factors, driven by util_update.run_updates in lockstep
    with the oracle (every status, pattern, value and ten counters after every update identical): bases of m = 60 (on
    which Forrest-Tomlin, symmetric and unsymmetric permutation updates all occur: asserted) and m = 280; a handle
    with a b_nz hint of 4 and dbg_set_upd_extra(8) run to ERROR_MAXIMUM_UPDATES (m = 24: the NEED_R / NEED_UC / NEED_W
    regrowth of blu_update.inc); the statuses of the call protocol; the hand-predictable permutation updates of a
    bidiagonal basis."""
    run_child(emu_lib, CHILD_UPDATE, "UPDATE OK")


FUZZ_SLICE = ("--seed", "4242", "--start", "4", "--count", "3")


def test_update_fuzz_slice_on_the_cpu(emu_lib, tmp_path):
    """tools/fuzz_update_gpu.py, unchanged, under the emulation build: random bases of m up to 400 with random
    parameters, capacity hints and arena slack, each with a random sequence of column replacements in lockstep with the
    oracle.  The slice is sized by the time budget of this file: cases 4 to 6 of seed 4242 (m = 121,
    92 and 91; 14, 34 and 79 replacements; arena slack 3, 3 and 0; SPARSE_THRES 0.05, 0.5 and 0.0) -- case 0 alone takes
    as long as the rest of this file's update tests together."""
    log = str(tmp_path / "fuzz.log")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_update_gpu.py"), "--log", log] + list(FUZZ_SLICE),
                         env=emu_env(emu_lib), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "all %s update cases" % FUZZ_SLICE[-1] in out.stdout, open(log).read()[-2000:] + out.stdout[-500:] + out.stderr[-4000:]
    assert int(out.stdout.split(";")[-1].split()[0]) >= 30, out.stdout  # "...; N updates applied"


# ---- the tape of tools/emu_replay.cpp ------------------------------------------------------------------------------------
OP_END, OP_NEW, OP_EXTRA, OP_PARAM, OP_FACT, OP_DENSE, OP_SPARSE, OP_FORUPD, OP_UPDATE, OP_STAT = range(10)


class Tape:
    """Drives the oracle alone and records every call with its result as 8-byte words (the format is described in
    tools/emu_replay.cpp)."""

    def __init__(self, orc):
        self.orc = orc
        self.words = [np.frombuffer(b"BLUTAPE1", np.int64)]
        self.o = None
        self.m = 0
        self.lhs = None
        self.nzlhs = 0

    def _i(self, *xs):
        self.words.append(np.array(xs, np.int64))

    def _f(self, xs):
        self.words.append(np.ascontiguousarray(xs, np.float64).view(np.int64))

    def _u(self, xs):
        self.words.append(np.ascontiguousarray(xs, np.uint64).view(np.int64))

    def new(self, m, b_nz, cap, extra=None):
        self.o = self.orc.OracleBLU(m, cap)
        self.o.set_fix_d3(True)
        self.m = m
        self._i(OP_NEW, m, b_nz)
        if extra is not None:
            self._i(OP_EXTRA, extra)

    def set_param(self, key, value):
        self.o.set_param(key, value)
        self._i(OP_PARAM, key)
        self._f([value])
        self._i(K.OK)

    def factorize(self, cp, ri, v):
        st = self.o.factorize(cp[:-1], cp[1:], ri, v)
        self._i(OP_FACT, len(ri))
        self._u(cp[:-1])
        self._u(cp[1:])
        self._u(ri)
        self._f(v)
        self._i(st)
        return st

    def solve_dense(self, rhs, trans="N"):
        x = self.o.solve_dense(rhs, trans)
        self._i(OP_DENSE, ord(trans))
        self._f(rhs)
        self._i(K.OK)
        self._f(x)
        return x

    def _solution(self, st, il, lhs, want=True):
        self._i(st)
        if st == K.OK and want:
            self._i(len(il))
            self._i(*il)
            self._f(lhs)
            self.lhs = lhs
        return st, il, lhs

    def solve_sparse(self, irhs, xrhs, trans="N"):
        self._i(OP_SPARSE, ord(trans), len(irhs))
        self._u(irhs)
        self._f(xrhs)
        return self._solution(*self.o.solve_sparse(irhs, xrhs, trans))

    def solve_for_update(self, irhs, xrhs=None, trans="N", want_solution=True):
        self._i(OP_FORUPD, ord(trans), len(irhs))
        self._u(irhs)
        self._i(0 if xrhs is None else 1)
        if xrhs is not None:
            self._f(xrhs)
        self._i(1 if want_solution else 0)
        return self._solution(*self.o.solve_for_update(irhs, xrhs, trans, want_solution), want=want_solution)

    def update(self, xtbl):
        st = self.o.update(xtbl)
        self._i(OP_UPDATE)
        self._f([xtbl])
        self._i(st)
        return st

    def stat(self, key):
        x = self.o.stat(key)
        self._i(OP_STAT, key)
        self._f([x])
        return x

    def write(self, path):
        self._i(OP_END)
        np.concatenate(self.words).tofile(path)


def write_tape(orc, path):
    t = Tape(orc)
    # the deep depth-first search
    m = DEEP_M
    cp = np.concatenate(([0], np.arange(1, 2 * m, 2))).astype(np.uint64)
    ri = np.concatenate([[j - 1, j] if j else [0] for j in range(m)]).astype(np.uint64)
    t.new(m, len(ri), 64 * len(ri) + 1024)
    t.set_param(K.PARAM_SPARSE_THRES, 1.0)
    assert t.factorize(cp, ri, np.ones(len(ri))) == K.OK
    for trans, i in (("N", m - 1), ("T", 0)):
        st, il, _ = t.solve_sparse([i], [1.0], trans)
        assert st == K.OK and len(il) == m
        t.stat(K.STAT_L_FLOPS)
        t.stat(K.STAT_U_FLOPS)
    # an update sequence to ERROR_MAXIMUM_UPDATES with a tiny b_nz hint and 8 entries of arena slack; xtbl is the oracle's
    # own lhs[j]: the library's is bit-identical (test_update_path_in_lockstep_on_the_cpu)
    spec = (24, 4, 4, 0.0, 5, 0.5)
    cp, ri, v = orc.gen_lp_basis(*spec)
    m = spec[0]
    t.new(m, 4, 256 * len(ri), extra=8)
    assert t.factorize(cp, ri, v) == K.OK
    log = U.run_updates(t, U.columns_of(cp, ri, v), m, 400, np.random.default_rng(11), check_every=5, stop_on_max=True)
    assert log["hit_maximum_updates"] and int(t.stat(K.STAT_NFORREST)) == m, log
    for key in (K.STAT_NUPDATE, K.STAT_NFORREST_TOTAL, K.STAT_NSYMPERM_TOTAL, K.STAT_DEV_NUNSYMPERM_TOTAL, K.STAT_R_NZ, K.STAT_U_NZ,
                K.STAT_MAX_ETA, K.STAT_PIVOT_ERROR):
        t.stat(key)
    # a sweep of sparse solves, fresh and after a few updates
    m = 160
    cp, ri, v = orc.gen_lp_basis(m, 6, 6, 0.5, 1, 0.3)
    t.new(m, len(ri), 64 * len(ri) + 1024)
    assert t.factorize(cp, ri, v) == K.OK
    for key in (K.STAT_CONDEST_L, K.STAT_CONDEST_U, K.STAT_RESIDUAL_TEST, K.STAT_NORMEST_L_INV, K.STAT_NORMEST_U_INV):
        t.stat(key)
    cols = U.columns_of(cp, ri, v)
    for state in ("fresh", "updated"):
        if state == "updated":
            assert U.run_updates(t, cols, m, 5, np.random.default_rng(3), check_every=2)["done"] >= 2
        for trans in "NT":
            for q, nz in enumerate((1, 2, 5, 17, m // 8, m // 2)):
                r = np.random.default_rng(100 * q + 7)
                assert t.solve_sparse(r.choice(m, nz, replace=False), r.standard_normal(nz), trans)[0] == K.OK
                t.stat(K.STAT_L_FLOPS)
                t.stat(K.STAT_U_FLOPS)
            b = np.random.default_rng(9).standard_normal(m)
            t.solve_dense(b, trans)
    t.write(path)


def test_replay_under_address_sanitizer(emu_lib, oracle, tmp_path):
    """The deep depth-first search, an update sequence run to ERROR_MAXIMUM_UPDATES through the host regrowth of the arenas,
    and a sweep of sparse solves on fresh and updated factors: recorded from the oracle alone as a tape of C-ABI calls
    with their results, replayed once by tools/emu_replay.cpp against libblu_emu.so (tape and replayer are right: every
    status, nzlhs, pattern, value and statistic identical) and once by its sanitized build against libblu_emu_asan.so.
    An AddressSanitizer report -- an access outside an arena of the kernels or of the host code -- fails the test."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu_replay", "emu_replay_asan"])
    tape = str(tmp_path / "calls.tape")
    write_tape(oracle, tape)
    env = {k: v for k, v in emu_env(emu_lib).items() if k != "BLU_HIP_LIB"}
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0:exitcode=23"
    for exe in (REPLAY, REPLAY_ASAN):
        out = subprocess.run([exe, tape], env=env, capture_output=True, text=True, timeout=1800)
        assert "AddressSanitizer" not in out.stderr, out.stderr[-6000:]
        assert out.returncode == 0 and "REPLAY OK" in out.stdout, (exe, out.returncode, out.stdout[-500:] + out.stderr[-4000:])
