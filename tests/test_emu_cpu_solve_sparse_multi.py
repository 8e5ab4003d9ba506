"""blu_hip_solve_sparse_multi on the CPU: the emulation build of the library (blu_amd/csrc `make emu`, as in
tests/test_emu_cpu.py) runs many sparse right-hand sides on ONE handle -- k_solve_sparse_multi on fresh factorizations,
k_solve_upd_multi + k_upd_add_flops on updated ones, k_gather_lhs_multi, the chunking and the host side of the entry.

Every right-hand side is compared with the oracle's solve_sparse on a twin and with the single blu_hip_solve_sparse on a
second handle, bit for bit (tests/util_update._ss / _same: np.array_equal on pattern and values; the oracle with the
64-bit cancellation mask, set_fix_d3, as elsewhere); an updated handle has its twin driven through the same updates.
Each case runs in a child process: the library path is fixed when blu_amd is first imported."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")
REPLAY = os.path.join(ROOT, "blu_amd", "emu_replay")
REPLAY_ASAN = os.path.join(ROOT, "blu_amd", "emu_replay_asan")
OP_SPARSE_MULTI_WS, OP_SPARSE_MULTI, OP_SPARSE_MULTI_GET = 12, 13, 14  # tools/emu_replay.cpp

HEAD = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, %(root)r)
import blu_amd
from blu_amd import keys as K
from oracle import orc
from tests import util, util_update as U, util_solve_sparse_multi as SM
from tests.util_solve_sparse_batch import BRANCH, scaled
assert b"gfx950" in blu_amd.lib().blu_hip_version()


def trio(cp, ri, v, want=K.OK):
    # the handle of the multi calls, a second one for the single calls, and the oracle twin
    m = len(cp) - 1
    g, s = blu_amd.BLU(m, len(ri)), blu_amd.BLU(m, len(ri))
    o = orc.OracleBLU(m, 64 * len(ri) + 1024)
    o.set_fix_d3(True)
    st = [x.factorize(cp[:-1], cp[1:], ri, v) for x in (g, s, o)]
    assert st == [want] * 3, (st, want)
    return g, s, o


def pair_rows(g):
    f = g.get_factors()
    pr = np.zeros(g.m, np.int64)
    pr[f["colperm"]] = f["rowperm"]
    return pr
"""

CHILD_FRESH = r"""
def with_long_column(cp, ri, v, col, collen, seed):
    # column `col` filled to `collen` entries in random rows: the "long lines" basis of tests/test_emu_cpu_solve_multi.py
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
for name, (cp, ri, v), want in cases[%(case)d:%(case)d + 1]:
    g, s, o = trio(cp, ri, v, want)
    m = g.m
    q = 0
    for thres in (0.0, 1.0, 0.05):
        SM.set_thres(thres, g, s, o)
        for nrhs in (1, 2, 65):
            for tr in "NT":
                q += 1
                cols = SM.columns(rng, m, nrhs, q)
                sts, sols = SM.check_multi(g, cols, tr, (name, thres, nrhs), twin=o, single=s)
                assert g.dbg_sparse_multi_last_chunk() == nrhs
                # the branch of the last right-hand side: sequential for every solve whose intermediate vector is not
                # empty with SPARSE_THRES 0, symbolic for every solve with 1
                if thres == 1.0:
                    assert g.stat(BRANCH) == 1, (name, nrhs, tr)
                if thres == 0.0 and len(sols[-1][0]) > 0:
                    assert g.stat(BRANCH) == 2, (name, nrhs, tr)
    assert g.lhs is None and g.nzlhs == 0  # the object's own solve_sparse result is not touched
print("SPARSE MULTI FRESH OK")
"""

CHILD_CHUNK = r"""
cp, ri, v = orc.gen_lp_basis(150, 5, 4, 0.8, 3, 0.6)
g, s, o = trio(cp, ri, v)
m = g.m
cols = SM.columns(np.random.default_rng(23), m, 23)
ir, xr = [c[0] for c in cols], [c[1] for c in cols]


def same(a, b):
    return a[0] == b[0] and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a[1], b[1]))


whole = {tr: g.solve_sparse_multi(ir, xr, tr) for tr in "NT"}
assert g.dbg_sparse_multi_last_chunk() == 23
g.dbg_set_sparse_multi_ws_bytes(5 * SM.slot_bytes(m) + 8)  # five slots
for tr in "NT":
    sts, sols = SM.check_multi(g, cols, tr, "chunked", twin=o, stats=())
    assert g.dbg_sparse_multi_last_chunk() == 5  # chunks of 5, 5, 5, 5, 3
    assert same((sts, sols), whole[tr]), tr
g.dbg_set_sparse_multi_ws_bytes(SM.slot_bytes(m) - 1)  # less than one slot: one at a time
x = g.solve_sparse_multi(ir[:4], xr[:4], "N")
assert g.dbg_sparse_multi_last_chunk() == 1 and same(x, (whole["N"][0][:4], whole["N"][1][:4]))
g.dbg_set_sparse_multi_ws_bytes(-1)
assert same(g.solve_sparse_multi(ir, xr, "T"), whole["T"]) and g.dbg_sparse_multi_last_chunk() == 23
print("SPARSE MULTI CHUNK OK")
"""

CHILD_UPDATED = r"""
spec = (120, 5, 5, 0.4, 6, 0.5)
cp, ri, v = orc.gen_lp_basis(*spec)
m = spec[0]
g, s, o = trio(cp, ri, v)
cols = U.columns_of(cp, ri, v)
pr = pair_rows(g)
rng = np.random.default_rng(8)
log = U.run_updates(g, cols, m, 8, rng, check_every=10 ** 9, pair_row=pr, twin=o)
assert log["done"] >= 3 and g.stat(K.STAT_NUPDATE) == log["done"], log
assert g.stat(K.STAT_NFORREST) > 0, "no Forrest-Tomlin update among them: the row etas would not be exercised"
# 9 columns, both systems: patterns, values, L / U / R_FLOPS and UPDATE_COST those of the twin's 9 single solves
for thres in (0.05, 0.0, 1.0, 0.05):
    SM.set_thres(thres, g, o)
    for tr in "NT":
        SM.check_multi(g, SM.columns(rng, m, 9, 1), tr, ("updated", thres), twin=o)
assert g.stat(K.STAT_R_FLOPS) > 0
# between solve_for_update and update: one replacement by hand, a multi call of 3 columns in between
done = 0
for attempt in range(20):
    j = int(rng.integers(0, m))
    ai, ax = U.new_column(rng, cols, m, j, pr)
    x = g.solve_dense(SM.dense_of(m, ai, ax), "N")
    assert np.array_equal(x, o.solve_dense(SM.dense_of(m, ai, ax), "N"))
    if abs(x[j]) < 1e-3:
        continue
    st = SM.between_solves_and_update(g, o, SM.columns(rng, m, 3, 1), m, j, ai, ax, ("by hand", attempt))
    if st == K.OK:
        cols[j] = (ai, ax)
        done += 1
        break
assert done == 1
# 4 more lock-step rounds: everything after the multi calls is still the twin's
log2 = U.run_updates(g, cols, m, 4, rng, pair_row=pr, twin=o)
assert log2["done"] >= 1, log2
for tr in "NT":
    SM.check_multi(g, SM.columns(rng, m, 9, 2), tr, "updated again", twin=o)
for key in (K.STAT_NFORREST, K.STAT_NUPDATE, K.STAT_R_NZ, K.STAT_U_NZ, K.STAT_NSYMPERM_TOTAL, K.STAT_NFORREST_TOTAL, K.STAT_DEV_NUNSYMPERM_TOTAL):
    assert g.stat(key) == o.stat(key), key
print("SPARSE MULTI UPDATED OK")
"""

CHILD_STATUS = r"""
cp, ri, v = orc.gen_lp_basis(150, 5, 4, 0.8, 3, 0.6)
g, s, o = trio(cp, ri, v)
m = g.m
INVARG, INVCALL, MISS = K.ERROR_INVALID_ARGUMENT, K.ERROR_INVALID_CALL, K.ERROR_ARGUMENT_MISSING
hnone = blu_amd.BLU(120, 500)                                        # never factorized
# blu_hip_get_sparse_multi before any multi call
assert SM.raw_get(blu_amd, g._h, 0)[0] == INVCALL and SM.raw_get(blu_amd, None, 0)[0] == MISS
SM.refusals(blu_amd, g, hnone)
assert SM.raw_get(blu_amd, g._h, 0)[0] == INVCALL                    # ... and a refused call leaves no result
hbad = blu_amd.BLU(150, len(ri))                                     # last factorize refused
bad_i = ri.copy()
bad_i[3] = 999
assert hbad.factorize(cp[:-1], cp[1:], bad_i, v) == INVARG
assert SM.raw_call(blu_amd, hbad._h, [0, 1], [3], [1.0])[0] == INVCALL

# per column: an index equal to m, and more than m entries, each in the middle of a call whose other columns are solved
rng = np.random.default_rng(3)
good = SM.columns(rng, m, 4, 1)
for bad in ((np.array([1, m]), np.ones(2)), (np.arange(m + 1) %% m, np.ones(m + 1))):
    cols = good[:2] + [bad] + good[2:]
    for tr in "NT":
        sts, sols = g.solve_sparse_multi([c[0] for c in cols], [c[1] for c in cols], tr)
        assert sts == [K.OK, K.OK, INVARG, K.OK, K.OK], sts
        assert len(sols[2][0]) == 0 and len(sols[2][1]) == 0
        for j in (0, 1, 3, 4):
            SM.same_column(m, sts[j], sols[j], U._ss(o, cols[j][0], cols[j][1], tr), ("mixed", tr, j))
        for key in (K.STAT_L_FLOPS, K.STAT_U_FLOPS):                  # the bad column counts nothing
            assert g.stat(key) == o.stat(key), key
# the C entry: return value = the most negative status, status may be NULL
ptr = np.concatenate(([0], np.cumsum([len(c[0]) for c in cols])))
ir, xr = np.concatenate([c[0] for c in cols]), np.concatenate([c[1] for c in cols])
rc, lp, st = SM.raw_call(blu_amd, g._h, ptr, ir, xr)
assert rc == INVARG and list(st) == [K.OK, K.OK, INVARG, K.OK, K.OK] and lp[0] == 0 and lp[3] == lp[2], (rc, lp, st)
rc, lp2, st = SM.raw_call(blu_amd, g._h, ptr, ir, xr, st=False)
assert rc == INVARG and np.array_equal(lp, lp2)
for j in (0, 1, 3, 4):  # (the twin follows the two raw calls)
    U._ss(o, cols[j][0], cols[j][1], "N")
    so = U._ss(o, cols[j][0], cols[j][1], "N")

# blu_hip_get_sparse_multi: twice the same arrays; NULL arrays refused while the total is above 0; the new result after a later call
total = int(lp[-1])
assert total > 0
a, b = SM.raw_get(blu_amd, g._h, total), SM.raw_get(blu_amd, g._h, total)
assert a[0] == b[0] == K.OK and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
assert np.array_equal(a[1][lp[4]:lp[5]], so[1]) and np.array_equal(a[2][lp[4]:lp[5]], so[2][so[1]])
assert SM.raw_get(blu_amd, g._h, total, IL=False)[0] == MISS and SM.raw_get(blu_amd, g._h, total, XL=False)[0] == MISS
sts, sols = SM.check_multi(g, good[:1], "T", "later call", twin=None)
c = SM.raw_get(blu_amd, g._h, len(sols[0][0]))
assert c[0] == K.OK and np.array_equal(c[1], sols[0][0]) and np.array_equal(c[2], sols[0][1])
U._ss(o, good[0][0], good[0][1], "T")

# nrhs == 0: BLU_OK, lhs_ptr[0] = 0, an empty result held (NULL arrays allowed)
rc, lp, st = SM.raw_call(blu_amd, g._h, [0], None, None)
assert rc == K.OK and lp[0] == 0 and (st == SM.SENT).all()
assert SM.raw_get(blu_amd, g._h, 0, IL=False, XL=False)[0] == K.OK
assert g.solve_sparse_multi([], []) == ([], [])
# all columns empty: NULL irhs / xrhs allowed
rc, lp, st = SM.raw_call(blu_amd, g._h, [0, 0, 0], None, None)
assert rc == K.OK and list(lp) == [0, 0, 0] and list(st) == [K.OK, K.OK]
# m == 0
hz = blu_amd.BLU(0, 1)
e = np.zeros(0, np.uint64)
assert hz.factorize(e, e, e, np.zeros(0)) == K.OK
rc, lp, st = SM.raw_call(blu_amd, hz._h, [0, 0, 0], None, None)
assert rc == K.OK and list(lp) == [0, 0, 0] and list(st) == [K.OK, K.OK]
sts, sols = hz.solve_sparse_multi([[], [], []], [[], [], []], "T")
assert sts == [K.OK] * 3 and all(len(x[0]) == 0 for x in sols)
# the Python wrapper's exceptions
for h in (hnone, hbad):
    try:
        h.solve_sparse_multi([[1]], [[1.0]])
    except blu_amd.BluError as err:
        assert err.status == INVCALL
    else:
        raise AssertionError("not refused")
try:
    hnone.get_sparse_multi(0)
except blu_amd.BluError as err:
    assert err.status == INVCALL
else:
    raise AssertionError("not refused")
# afterwards the single call and the multi call answer with the oracle's bits, counters included
for tr in "NT":
    U._same(U._ss(g, good[1][0], good[1][1], tr), U._ss(o, good[1][0], good[1][1], tr), ("single after", tr))
    SM.check_multi(g, good, tr, "after the refusals", twin=o, stats=(K.STAT_L_FLOPS, K.STAT_U_FLOPS))
assert hbad.factorize(cp[:-1], cp[1:], ri, v) == K.OK
SM.check_multi(hbad, good, "N", "refactorized", twin=None, single=s, stats=())
print("SPARSE MULTI STATUS OK")
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def run_child(emu_lib, body, ok, case=0):
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1")
    out = subprocess.run([sys.executable, "-c", (HEAD + body) % {"root": ROOT, "case": case}], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and ok in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("case", range(4), ids=("lp200", "lp150", "rank-deficient", "long-lines"))
def test_sparse_multi_fresh_factorizations_on_the_cpu(emu_lib, case):
    """k_solve_sparse_multi + k_gather_lhs_multi, one basis per case (a child process each): two LP bases, a rank-deficient
    one and the "long lines" basis of tests/test_emu_cpu_solve_multi.py; nrhs 1, 2 and 65 with columns of 0, 1, 5, 70 and m/2 entries in turn, both systems,
    SPARSE_THRES 0.0 (sequential branch: statistic 43 == 2 after a non-empty last column), 1.0 (symbolic branch: == 1) and the
    default; every column the twin's and the single-call handle's bits, L_FLOPS / U_FLOPS the twin's after every call"""
    run_child(emu_lib, CHILD_FRESH, "SPARSE MULTI FRESH OK", case)


def test_sparse_multi_chunking_on_the_cpu(emu_lib):
    """dbg_set_sparse_multi_ws_bytes so that 5 slots fit, m = 150, nrhs = 23: chunks of 5, 5, 5, 5 and 3 give the bits of
    the one-chunk call and of the oracle; a limit below one slot works them one at a time; -1 restores the default"""
    run_child(emu_lib, CHILD_CHUNK, "SPARSE MULTI CHUNK OK")


def test_sparse_multi_after_updates_in_lockstep_on_the_cpu(emu_lib):
    """k_solve_upd_multi + k_upd_add_flops after 8 update rounds in lock step with the twin: 9 columns, both systems, three
    thresholds -- patterns, values, L / U / R_FLOPS and UPDATE_COST the twin's; a replacement by hand with multi calls of 3
    columns between the two solve_for_update calls and update (status, PIVOT_ERROR, NFORREST, R_NZ and the sparse solves
    that follow are the twin's); then 4 more lock-step rounds"""
    run_child(emu_lib, CHILD_UPDATED, "SPARSE MULTI UPDATED OK")


def test_sparse_multi_statuses_on_the_cpu(emu_lib):
    """every refusal of blu_hip_solve_sparse_multi in the order of the header with lhs_ptr, status, the held result and
    the counters untouched; per-column INVALID_ARGUMENT (an index equal to m, more than m entries) in the middle of a call
    whose other columns are solved and which counts nothing; nrhs == 0, m == 0; blu_hip_get_sparse_multi before any call,
    twice, with NULL arrays and after a later call; the wrapper's exceptions"""
    run_child(emu_lib, CHILD_STATUS, "SPARSE MULTI STATUS OK")


def test_sparse_multi_replay_under_address_sanitizer(emu_lib, oracle, tmp_path):
    """A tape of tools/emu_replay.cpp recorded from the oracle alone, m = 96: multi calls on a fresh factorization in one
    chunk and in chunks of 4 with the last one partial, 8 update rounds, multi calls of both systems on the updated factors,
    further rounds and the repeated fetch.  The replayer builds host arrays that end with their last entry, so a read
    behind the packed right-hand sides or a write behind the fetched solutions -- or an access of k_solve_sparse_multi /
    k_solve_upd_multi / k_gather_lhs_multi outside a slot, the staging block or the result buffer -- is an AddressSanitizer
    report.  Replayed with the plain build and with the sanitized one (the executable carries the sanitizer runtime;
    nothing is preloaded)."""
    import numpy as np

    from blu_amd import keys as K
    from tests import util_solve_sparse_multi as SM, util_update as U
    from tests.test_emu_cpu_solves import Tape

    class MultiTape(Tape):
        def set_sparse_multi_ws_bytes(self, n):
            self._i(OP_SPARSE_MULTI_WS, n)

        def solve_sparse_multi(self, cols, trans):
            sols = [self.o.solve_sparse(ir, xr, trans) for ir, xr in cols]
            assert all(s[0] == K.OK for s in sols)
            self._i(OP_SPARSE_MULTI, ord(trans), len(cols))
            self._i(0, *np.cumsum([len(c[0]) for c in cols]))
            self._u(np.concatenate([c[0] for c in cols]))
            self._f(np.concatenate([c[1] for c in cols]))
            self._i(K.OK, *[K.OK] * len(cols))
            self._i(0, *np.cumsum([len(s[1]) for s in sols]))
            self.last = (np.concatenate([s[1] for s in sols]).astype(np.int64), np.concatenate([s[2][s[1]] for s in sols]))
            self._i(*self.last[0])
            self._f(self.last[1])

        def fetch_twice(self):
            self._i(OP_SPARSE_MULTI_GET, len(self.last[0]))
            self._i(*self.last[0])
            self._f(self.last[1])

    subprocess.check_call(["make", "-s", "-C", CSRC, "emu_replay", "emu_replay_asan"])
    m = 96
    cp, ri, v = oracle.gen_lp_basis(m, 5, 5, 0.4, 6, 0.5)
    t = MultiTape(oracle)
    t.new(m, len(ri), 64 * len(ri) + 1024)
    assert t.factorize(cp, ri, v) == K.OK
    rng = np.random.default_rng(12)
    for tr in "NT":
        t.solve_sparse_multi(SM.columns(rng, m, 11, 1), tr)
    t.set_sparse_multi_ws_bytes(4 * SM.slot_bytes(m))
    for tr in "NT":
        t.solve_sparse_multi(SM.columns(rng, m, 11, 2), tr)
    t.fetch_twice()
    cols = U.columns_of(cp, ri, v)
    assert U.run_updates(t, cols, m, 8, rng, check_every=10 ** 9)["done"] >= 3
    for tr in "TN":
        t.solve_sparse_multi(SM.columns(rng, m, 11, 3), tr)
    t.set_sparse_multi_ws_bytes(-1)
    assert U.run_updates(t, cols, m, 3, rng)["done"] >= 1
    for tr in "NT":
        t.solve_sparse_multi(SM.columns(rng, m, 5, 1), tr)
    t.fetch_twice()
    for key in (K.STAT_NUPDATE, K.STAT_NFORREST, K.STAT_R_NZ, K.STAT_U_NZ, K.STAT_L_FLOPS, K.STAT_U_FLOPS, K.STAT_R_FLOPS, K.STAT_UPDATE_COST):
        t.stat(key)
    tape = str(tmp_path / "sparse_multi.tape")
    t.write(tape)
    env = {k: v for k, v in os.environ.items() if k != "BLU_HIP_LIB"}
    env.update(BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    for exe in (REPLAY, REPLAY_ASAN):
        out = subprocess.run([exe, tape], env=env, capture_output=True, text=True, timeout=900)
        assert "AddressSanitizer" not in out.stderr, out.stderr[-6000:]
        assert out.returncode == 0 and "REPLAY OK" in out.stdout, (exe, out.returncode, out.stdout[-500:] + out.stderr[-4000:])
