"""The ratio test on the device, on the CPU: the emulation build of the library (blu_amd/csrc `make emu`) runs
k_at_dot_kind, k_ratio_pick, k_ratio_pick_batch, the dual-step kernels, k_duals_fanout and the host side of the eight new
entries through the drivers of tests/util_ratio.py, which tests/test_gpu_ratio.py runs on hardware: against the numpy
restatements ratio_pick and duals_step on the reference alpha, and beside clones driven by the existing single entries.
The cases (a) to (h) are listed in tests/test_gpu_ratio.py.  Equalities of bits and of integers only.  Each case runs in
a child process: the library path is fixed when blu_amd is first imported.  M0 runs everywhere; M2 (200 x 1131, the twin
columns and more columns than a workgroup) runs through the single entry here and through the batch entries in the replayed
tape (9 members), the sizes the emulator does in its usual time; the batch driver on M2 runs on hardware."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")

HEAD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import blu_amd
from tests import util_ratio as R
assert b"gfx950" in blu_amd.lib().blu_hip_version()
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def run_child(emu_lib, body, *args, timeout=1200):
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1")
    cmd = [sys.executable, "-c", HEAD + body + '\nprint("RATIO OK")\n', ROOT] + [str(x) for x in args]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and "RATIO OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.parametrize("name,nupdates", (("M0", 0), ("M0", 2), ("M2", 1)))
def test_ratio_test_is_the_restatement_on_the_reference_row(emu_lib, name, nupdates):
    """the single entry on fresh factors and after updates made through it beside a twin: record, kept row, solution,
    statistics, the dual step, the call counts"""
    run_child(emu_lib, "R.check_single(sys.argv[2], int(sys.argv[3]))", name, nupdates)


@pytest.mark.parametrize("name,n", (("M0", 1), ("M0", 7), ("M0", 8), ("M0", 9), ("M0", 17)))
def test_ratio_test_batch_is_the_single_entry_per_member(emu_lib, name, n):
    """member k equals the restatement and the single entry on a fork; permuted and chunked calls give the same bits; one
    iteration with prepare_update, update_batch and update_duals_batch"""
    run_child(emu_lib, "R.check_batch(sys.argv[2], int(sys.argv[3]))", name, n)


def test_members_with_a_status_of_their_own(emu_lib):
    run_child(emu_lib, "R.check_bad_members('M0')")


def test_refusals_and_the_lifetime_of_the_state(emu_lib):
    run_child(emu_lib, "R.check_refusals_and_lifetime('M0')")


REPLAY = os.path.join(ROOT, "blu_amd", "emu_replay")
REPLAY_ASAN = os.path.join(ROOT, "blu_amd", "emu_replay_asan")
OP_SHARE_MATRIX = 24  # tools/emu_replay.cpp
OP_SET_DUALS, OP_RATIO_TEST, OP_UPDATE_DUALS, OP_COPY_DUALS, OP_RATIO_TEST_BATCH, OP_UPDATE_DUALS_BATCH = 27, 28, 29, 30, 31, 32


def test_ratio_replay_under_address_sanitizer(emu_lib, oracle, tmp_path):
    """One tape of the new entries on M2, recorded from the oracle, at_dot, ratio_pick and duals_step alone: set_matrix,
    factorize_columns, set_duals, ratio_test with every case of util_ratio.cases and the kept row behind it, update_duals
    with overrides, share_matrix into 8 holders, copy_duals_batch, ratio_test_batch over 9 members with sigmas of their own
    in one chunk and in chunks of one group, update_duals_batch.  The replayer's host arrays end with their last entry and
    the device arrays of the emulation are host allocations, so an access of the pick, the dual-step kernels or the
    fan-out outside d, kind, the kept row, the products or the records is an AddressSanitizer report.  Replayed with the
    plain build and with the sanitized one (the executable carries the sanitizer runtime; nothing is preloaded)."""
    import numpy as np

    from blu_amd import keys as K
    from tests import util_matrix as MX
    from tests import util_maxvolume as MV
    from tests import util_ratio as R
    from tests.test_emu_cpu_matrix import OP_FACT_COLUMNS, OP_SET_MATRIX
    from tests.test_emu_cpu_solves import Tape

    class RatioTape(Tape):
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

        def row(self, r):
            st, il, lhs = self.o.solve_sparse([r], [1.0], "T")
            assert st == K.OK
            return MX.at_dot(self.a[0], self.a[1], self.a[2], lhs)

        def set_duals(self, d, kind):
            self.d, self.kind = np.array(d, np.float64), np.array(kind, np.int8)
            self._i(OP_SET_DUALS)
            self._f(d)
            self._i(*kind)
            self._i(K.OK)

        def _pick(self, r, sigma, pivtol, dualtol):
            alpha = self.row(r)
            rec = R.ratio_pick(alpha, self.d, self.kind, sigma, pivtol, dualtol)
            self._i(K.OK, rec[0], rec[1])
            self._f(rec[2:])
            self._f(R.kept(alpha, self.kind))
            return rec, R.kept(alpha, self.kind)

        def ratio_test(self, r, sigma, pivtol, dualtol):
            self._i(OP_RATIO_TEST, r, 0)
            self._f([sigma, pivtol, dualtol])
            self.rec, self.kept = self._pick(r, sigma, pivtol, dualtol)
            return self.rec

        def _sets(self, sets):
            self._i(len(sets[0]), *sets[0])
            self._f(sets[1])
            self._i(*sets[2])

        def update_duals(self, theta, sets):
            self._i(OP_UPDATE_DUALS)
            self._f([theta])
            self._sets(sets)
            self.d, self.kind = R.duals_step(self.d, self.kind, self.kept, theta, *sets)
            self._i(K.OK)
            self._f(self.d)
            self._i(*self.kind)

        def share_and_copy(self, n):
            self._i(OP_SHARE_MATRIX, n)
            self._i(OP_COPY_DUALS)

        def ratio_test_batch(self, rows, sigmas, pivtol, dualtol, nbytes):
            self._i(OP_RATIO_TEST_BATCH, nbytes, len(rows))
            for r, s in zip(rows, sigmas):
                self._i(r)
                self._f([s])
            self._f([pivtol, dualtol])
            self._i(K.OK)
            return [self._pick(r, s, pivtol, dualtol) for r, s in zip(rows, sigmas)]  # (all members hold the root's d and kind)

        def update_duals_batch(self, picks, thetas, sets):
            self._i(OP_UPDATE_DUALS_BATCH, len(picks))
            for th, st in zip(thetas, sets):
                self._f([th])
                self._sets(st)
            self._i(K.OK)
            for (rec, kept), th, st in zip(picks, thetas, sets):
                d, kind = R.duals_step(self.d, self.kind, kept, th, *st)
                self._i(K.OK)
                self._f(d)
                self._i(*kind)

    subprocess.check_call(["make", "-s", "-C", CSRC, "emu_replay", "emu_replay_asan"])
    m, ncol, a = R.m2()
    t = RatioTape(oracle)
    t.new(m, len(a[1]), 64 * len(a[1]) + 1024)
    t.set_matrix(a)
    basis, isbasic = MV.start(m, ncol)
    assert t.factorize_columns(basis) == K.OK
    r = int(MX.column(a, ncol - 1)[0][0])
    alpha = t.row(r)
    none = ([], [], [])
    for case in R.cases("M2", alpha):
        label, d, kind, sigma, pivtol, dualtol = case
        t.set_duals(d, kind)
        rec = t.ratio_test(r, sigma, pivtol, dualtol)
        t.update_duals(rec[4], ([rec[0], ncol - 1], [0.0, -1.5], [0, 2]) if rec[0] not in (-1, ncol - 1) else none)
    t.share_and_copy(8)
    rows = [(7 * k + r) % m for k in range(9)]
    sigmas = [1.0 if k % 2 else -1.0 for k in range(9)]
    for nbytes in (-1, 1):
        picks = t.ratio_test_batch(rows, sigmas, 1e-9, 1e-7, nbytes)
    t.update_duals_batch(picks, [p[0][4] for p in picks], [([p[0][0]], [0.0], [0]) if p[0][0] >= 0 and k % 2 else none for k, p in enumerate(picks)])
    tape = str(tmp_path / "ratio.tape")
    t.write(tape)
    env = {k: v for k, v in os.environ.items() if k != "BLU_HIP_LIB"}
    env.update(BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    for exe in (REPLAY, REPLAY_ASAN):
        out = subprocess.run([exe, tape], env=env, capture_output=True, text=True, timeout=1800)
        assert "AddressSanitizer" not in out.stderr, out.stderr[-6000:]
        assert out.returncode == 0 and "REPLAY OK" in out.stdout, (exe, out.returncode, out.stdout[-500:] + out.stderr[-4000:])
