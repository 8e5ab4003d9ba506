"""blu_hip_maxvolume on the CPU: the emulation build of the library (blu_amd/csrc `make emu`, as in tests/test_emu_cpu.py)
runs the native pass -- k_price_multi, k_price_pick, the mode-1 solves and the update of every hit, the refactorization
rule and the host side -- beside the loop blu_amd.maxvolume on an oracle twin.  After every sweep the status, nupdate,
basis, isbasic and the statistics of tests/util_maxvolume.STATS are the twin's, then solve_sparse of three columns in both
systems, bit for bit; equalities only.  Each case runs in a child process: the library path is fixed when blu_amd is first
imported."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")
REPLAY = os.path.join(ROOT, "blu_amd", "emu_replay")
REPLAY_ASAN = os.path.join(ROOT, "blu_amd", "emu_replay_asan")
OP_MAXVOLUME, OP_MAXVOLUME_CHUNK = 15, 16  # tools/emu_replay.cpp

HEAD = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, sys.argv[1])
import blu_amd
from blu_amd import keys as K
from blu_amd.maxvolume import maxvolume as loop
from oracle import orc
from tests import util_maxvolume as MV
assert b"gfx950" in blu_amd.lib().blu_hip_version()
INVARG, MISS = K.ERROR_INVALID_ARGUMENT, K.ERROR_ARGUMENT_MISSING


def trio(m, nz):
    # the handle of the native pass, a second one for the loop over the single entries, and the oracle twin
    return blu_amd.BLU(m, nz), blu_amd.BLU(m, nz), MV.oracle_twin(orc, m, nz)
"""

CHILD_SWEEPS = r"""
problem = (int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5]))
chunk = None if sys.argv[6] == "policy" else int(sys.argv[6])
a = MV._problem(*problem[:3])
g, s, o = trio(problem[0], len(a[1]))
traces = [MV.loop_trace(o, problem, a)]
if problem[0] == 12:  # the smallest problem also beside the loop over the single entries of the library: the branch statistic
    traces.append(MV.loop_trace(s, problem, a))
native = MV.native_trace(g, problem, a, chunk)
MV.check(native, traces, problem, chunk)
print([(x["nup"], x["counts"]) for x in native])
print("MAXVOLUME SWEEPS OK")
"""

CHILD_STORAGE = r"""
problem = (60, 150, 2, 1.5)
a = MV._problem(*problem[:3])
o = MV.oracle_twin(orc, 60, len(a[1]))
trace = MV.loop_trace(o, problem, a)
for chunk in (7, None):
    g = blu_amd.BLU(60, 4)
    g.dbg_set_upd_extra(8)  # forces UPD_NEED_R / NEED_UC / NEED_W round trips in the mode-1 solves and the updates of the pass
    native = MV.native_trace(g, problem, a, chunk)
    assert g.dbg_upd_grows() > 0, "no storage request during the pass"
    MV.check(native, [trace], problem, chunk)
    print(chunk, g.dbg_upd_grows())
print("MAXVOLUME STORAGE OK")
"""

CHILD_ERRORS = r"""
def with_column(a, j, idx, val):
    a_p, a_i, a_x = a
    b, e = int(a_p[j]), int(a_p[j + 1])
    n_i = np.concatenate((a_i[:b], np.asarray(idx, np.uint64), a_i[e:]))
    n_x = np.concatenate((a_x[:b], np.asarray(val, float), a_x[e:]))
    n_p = a_p.astype(np.int64).copy()
    n_p[j + 1:] += len(idx) - (e - b)
    return n_p.astype(np.uint64), n_i, n_x


def three(a, m, ncol, tol, chunk, basis0=None, isbasic0=None, hs=None):
    # the native pass on a fresh handle beside the loop on a second handle and on the oracle: the snapshots
    g, s, o = hs or trio(m, len(a[1]))
    g.dbg_set_maxvolume_chunk(-1 if chunk is None else chunk)
    snaps = []
    for h in (g, s, o):
        basis, isbasic = MV.start(m, ncol) if basis0 is None else (list(basis0), list(isbasic0))
        st, nup = h.maxvolume(ncol, a[0], a[1], a[2], basis, isbasic, tol) if h is g else loop(h, ncol, a[0], a[1], a[2], basis, isbasic, tol)
        snaps.append(MV.snapshot(h, a, st, nup, basis, isbasic))
    return snaps, (g, s, o)


m, ncol, seed, tol = 30, 90, 1, 2.0
a = MV._problem(m, ncol, seed)
# ---- a column the solves refuse, at a non-basic position behind hits: the pass ends there as the loop does
long_idx = np.arange(m + 1) % m
for what, bad in (("index m", with_column(a, 70, [3, m], [1.0, 2.0])), ("m + 1 entries", with_column(a, 70, long_idx, np.ones(m + 1)))):
    for chunk in (7, 64, None):
        snaps, hs = three(bad, m, ncol, tol, chunk)
        assert snaps[2]["st"] == INVARG and snaps[2]["nup"] > 0 and not snaps[2]["isbasic"][70], (what, snaps[2]["st"], snaps[2]["nup"])
        MV.same_snapshot(snaps[0], snaps[1], (what, chunk, "library loop"))
        MV.same_snapshot(snaps[0], snaps[2], (what, chunk, "oracle loop"))
        # the refused column was priced in a chunk with columns behind it; it counts as reached only when its turn comes
        assert hs[0].dbg_maxvolume_counts()[3] == snaps[0]["nup"]

# ---- refusals before anything is touched: statistics and the held factorization stay
snaps, (g, s, o) = three(a, m, ncol, tol, 7)
MV.same_snapshot(snaps[0], snaps[2], "first sweep")
FN = blu_amd.lib().blu_hip_maxvolume
FN.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_double, C.c_void_p]
basis = np.array(snaps[0]["basis"], np.int64)
isbasic = np.array(snaps[0]["isbasic"], np.int64)
ALL = MV.STATS + (K.STAT_L_NZ, K.STAT_MIN_PIVOT, K.STAT_MAX_PIVOT, K.STAT_UPDATE_COST_DENOM)
before = [g.stat(k) for k in ALL]
rhs = np.sin(np.arange(float(m)))
x0 = g.solve_dense(rhs, "N")


def raw(h=g._h, n=ncol, ap=a[0], ai=a[1], ax=a[2], b=basis, ib=isbasic, t=tol, nup=True):
    b0, ib0 = b, ib
    b, ib = b.copy() if b is not None else None, ib.copy() if ib is not None else None
    out = C.c_int64(99)
    ptr = lambda x: None if x is None else x.ctypes.data
    rc = FN(h, n, ptr(ap), ptr(ai), ptr(ax), ptr(b), ptr(ib), t, C.addressof(out) if nup else None)
    assert b is None or np.array_equal(b, b0)  # (a refused call writes nothing)
    assert ib is None or np.array_equal(ib, ib0)
    return rc, out.value


down = a[0].copy()
down[40] = down[41] + 1
off = basis.copy()
off[3] = ncol
neg = basis.copy()
neg[0] = -1
for want, kw in ((MISS, dict(h=None)), (MISS, dict(ap=None)), (MISS, dict(b=None)), (MISS, dict(ib=None)), (MISS, dict(ai=None)), (MISS, dict(ax=None)),
                 (INVARG, dict(n=-1)), (INVARG, dict(ap=down)), (INVARG, dict(b=off)), (INVARG, dict(b=neg))):
    assert raw(**kw) == (want, 99), (kw.keys(), raw(**kw))
assert raw(t=0.5) == (INVARG, 0) and raw(t=0.5, nup=False)[0] == INVARG and raw(t=-np.inf) == (INVARG, 0)
assert [g.stat(k) for k in ALL] == before
assert np.array_equal(g.solve_dense(rhs, "N"), x0)
assert g.maxvolume(ncol, a[0], a[1], a[2], list(basis), list(isbasic), 0.5) == (INVARG, 0)
# an A without entries may come with NULL a_i / a_x (m == 0 below); p_nupdate may be NULL for a pass that runs
b2, ib2 = basis.copy(), isbasic.copy()
assert FN(g._h, ncol, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, b2.ctypes.data, ib2.ctypes.data, tol, None) == K.OK
ob, oi = list(basis), list(isbasic)
sto, nupo = loop(o, ncol, a[0], a[1], a[2], ob, oi, tol)
assert sto == K.OK and list(b2) == ob and list(ib2) == oi and g.stat(K.STAT_NUPDATE) == o.stat(K.STAT_NUPDATE)
MV.same_snapshot(MV.snapshot(g, a, K.OK, nupo, b2, ib2), MV.snapshot(o, a, sto, nupo, ob, oi), "NULL p_nupdate")

# ---- a NaN tolerance is not below 1.0: the loop takes every candidate, an empty solution included; so does the pass
for chunk in (5, None):
    snaps, _ = three(MV._problem(12, 40, 3), 12, 40, float("nan"), chunk)
    assert snaps[2]["nup"] > 0
    MV.same_snapshot(snaps[0], snaps[1], ("NaN", chunk, "library loop"))
    MV.same_snapshot(snaps[0], snaps[2], ("NaN", chunk, "oracle loop"))

# ---- a singular start basis: the same column twice
b0, i0 = MV.start(m, ncol)
b0[1] = 0
i0[1] = 0
snaps, _ = three(a, m, ncol, tol, None, b0, i0)
assert snaps[0]["st"] == K.WARNING_SINGULAR_MATRIX and snaps[0]["nup"] == 0
MV.same_snapshot(snaps[0], snaps[1], "singular, library loop")
MV.same_snapshot(snaps[0], snaps[2], "singular, oracle loop")

# ---- m == 0: as the loop over the single entries of the library (the oracle's solve_for_update answers an empty basis
# with ERROR_MAXIMUM_UPDATES, the library's with ERROR_INVALID_ARGUMENT: an older difference between the two, kept)
e_u, e_f = np.zeros(0, np.uint64), np.zeros(0)
for ncol0, ap0, ai0, ax0 in ((0, np.zeros(1, np.uint64), e_u, e_f), (2, np.zeros(3, np.uint64), e_u, e_f),
                             (2, np.array([0, 1, 2], np.uint64), np.zeros(2, np.uint64), np.ones(2))):
    g0, s0 = blu_amd.BLU(0, 1), blu_amd.BLU(0, 1)
    bg, ig, bs, is_ = [], [0] * ncol0, [], [0] * ncol0
    rg = g0.maxvolume(ncol0, ap0, ai0, ax0, bg, ig, 2.0)
    rs = loop(s0, ncol0, ap0, ai0, ax0, bs, is_, 2.0)
    assert rg == rs and rg == ((K.OK, 0) if ncol0 == 0 else (INVARG, 0)), (ncol0, rg, rs)
    assert ig == is_ and g0.stat(K.STAT_NFACTORIZE) == s0.stat(K.STAT_NFACTORIZE) == 1
print("MAXVOLUME ERRORS OK")
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def start_child(emu_lib, body, *args, timeout=2400, running=None):
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1")
    cmd = [sys.executable, "-c", HEAD + body, ROOT] + [str(x) for x in args]
    with subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) as proc:
        if running is not None:
            running.append(proc)
        try:
            stdout, stderr = proc.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            proc.kill()
            stdout, stderr = proc.communicate()
            stderr += "\nchild ended at its time limit"
    return subprocess.CompletedProcess(cmd, proc.returncode, stdout, stderr)


def run_child(emu_lib, body, ok, *args, timeout=2400):
    out = start_child(emu_lib, body, *args, timeout=timeout)
    assert out.returncode == 0 and ok in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


SWEEP_PROBLEMS = ((30, 90, 1, 2.0), (60, 150, 2, 1.5), (12, 40, 3, 1.0), (96, 400, 5, 1.2))
SWEEP_CHUNKS = (1, 3, 7, 64, "policy")


@pytest.fixture(scope="module")
def sweep_children(emu_lib):
    """The children of the sweep cases, started together on a few threads: the emulator runs one fiber per GPU thread, and
    a pass that throws 60 candidates away per hit is minutes of it; the longest cases go first."""
    from concurrent.futures import ThreadPoolExecutor

    pool = ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1)))
    cases = sorted(((p, c) for p in SWEEP_PROBLEMS for c in SWEEP_CHUNKS), key=lambda pc: (-pc[0][1], pc[1] in (1, 3, 7)))
    running = []
    futures = {pc: pool.submit(start_child, emu_lib, CHILD_SWEEPS, *pc[0], pc[1], running=running) for pc in cases}
    yield futures
    pool.shutdown(wait=False, cancel_futures=True)  # (a run of a few cases only: the others are not waited for)
    for proc in running:
        if proc.poll() is None:
            proc.kill()
    pool.shutdown(wait=True)


@pytest.mark.parametrize("chunk", SWEEP_CHUNKS)
@pytest.mark.parametrize("problem", SWEEP_PROBLEMS, ids=lambda p: "%dx%d" % p[:2])
def test_native_pass_is_the_loop_on_the_cpu(sweep_children, problem, chunk):
    """sweeps until one changes nothing, with forced chunks of 1, 3, 7 and 64 candidates and with the policy: every sweep the
    oracle twin's; the first sweep makes the updates and refactorizations of util_maxvolume.PROBLEMS (cost-driven ones among
    them) and, with chunks above 1, throws priced candidates away; the last sweep has no hit and prices ncol - m columns"""
    out = sweep_children[(problem, chunk)].result()
    assert out.returncode == 0 and "MAXVOLUME SWEEPS OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_native_pass_with_storage_requests_on_the_cpu(emu_lib):
    """a b_nz hint of 4 and dbg_set_upd_extra(8): the mode-1 solves and the updates of the hits ask for storage (counted),
    the results stay the twin's"""
    run_child(emu_lib, CHILD_STORAGE, "MAXVOLUME STORAGE OK")


def test_native_pass_statuses_on_the_cpu(emu_lib):
    """a column with an index equal to m, and one with m + 1 entries, at a non-basic position behind hits: INVALID_ARGUMENT
    with the loop's nupdate, basis, isbasic and statistics; the refusals before anything is touched leave statistics and the
    held factorization alone; volumetol below 1, NaN and NULL p_nupdate; a singular start basis; m == 0"""
    run_child(emu_lib, CHILD_ERRORS, "MAXVOLUME ERRORS OK")


def test_native_pass_replay_under_address_sanitizer(emu_lib, oracle, tmp_path):
    """A tape of tools/emu_replay.cpp recorded from the oracle alone: m = 60 and m = 12, sweeps until nothing changes, with
    chunks of 5 and with the policy, the statistics after every sweep.  The replayer builds host arrays that end with their
    last entry, so a read behind A, basis or isbasic -- or an access of k_price_multi / k_price_pick outside a slot, the
    resident A, the candidate list or the record -- is an AddressSanitizer report.  Replayed with the plain build and with the
    sanitized one (the executable carries the sanitizer runtime; nothing is preloaded)."""
    import numpy as np

    from blu_amd import keys as K
    from blu_amd.maxvolume import maxvolume as loop
    from tests import util_maxvolume as MV
    from tests.test_emu_cpu_solves import Tape

    class PassTape(Tape):
        def set_chunk(self, n):
            self._i(OP_MAXVOLUME_CHUNK, n)

        def maxvolume(self, a, basis, isbasic, tol, with_nupdate=True):
            ncol = len(a[0]) - 1
            self._i(OP_MAXVOLUME, ncol)
            self._u(a[0])
            self._u(a[1])
            self._f(a[2])
            self._i(*basis)
            self._i(*isbasic)
            self._f([tol])
            st, nup = loop(self.o, ncol, a[0], a[1], a[2], basis, isbasic, tol)
            self._i(1 if with_nupdate else 0, st, nup)
            self._i(*basis)
            self._i(*isbasic)
            return st, nup

    subprocess.check_call(["make", "-s", "-C", CSRC, "emu_replay", "emu_replay_asan"])
    t = PassTape(oracle)
    for problem in ((60, 150, 2, 1.5), (12, 40, 3, 1.0)):
        nrow, ncol, seed, tol = problem
        a = MV._problem(nrow, ncol, seed)
        for chunk in (5, -1):
            t.new(nrow, len(a[1]), 64 * len(a[1]) + 1024)
            t.set_chunk(chunk)
            basis, isbasic = MV.start(nrow, ncol)
            for sweep in range(40):
                st, nup = t.maxvolume(a, basis, isbasic, tol, with_nupdate=sweep != 1)
                assert st == K.OK
                for key in MV.STATS[:-1]:
                    t.stat(key)
                if nup == 0:
                    break
            assert nup == 0 and sweep > 0
    tape = str(tmp_path / "maxvolume.tape")
    t.write(tape)
    env = {k: v for k, v in os.environ.items() if k != "BLU_HIP_LIB"}
    env.update(BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    for exe in (REPLAY, REPLAY_ASAN):
        out = subprocess.run([exe, tape], env=env, capture_output=True, text=True, timeout=1800)
        assert "AddressSanitizer" not in out.stderr, out.stderr[-6000:]
        assert out.returncode == 0 and "REPLAY OK" in out.stdout, (exe, out.returncode, out.stdout[-500:] + out.stderr[-4000:])
