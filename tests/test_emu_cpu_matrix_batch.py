"""The shared matrix and its batched products on the CPU: the emulation build of the library (blu_amd/csrc `make emu`, as in
tests/test_emu_cpu_matrix.py) runs blu_hip_share_matrix, blu_hip_tableau_row_batch and blu_hip_price_batch --
k_scatter_lhs_batch, k_at_dot_batch and the host side -- beside clones driven by the single entries and beside the
summation order of the contract restated in numpy (tests/util_matrix.at_dot).  The drivers are those of
tests/util_matrix_batch.py, which tests/test_gpu_matrix_batch.py runs on hardware.  Equalities of bits only.  Each case
runs in a child process: the library path is fixed when blu_amd is first imported."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")
REPLAY = os.path.join(ROOT, "blu_amd", "emu_replay")
REPLAY_ASAN = os.path.join(ROOT, "blu_amd", "emu_replay_asan")
OP_SHARE_MATRIX, OP_TABLEAU_ROW_BATCH, OP_PRICE_BATCH = 24, 25, 26  # tools/emu_replay.cpp

HEAD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import blu_amd
from tests import util_matrix_batch as MB
assert b"gfx950" in blu_amd.lib().blu_hip_version()
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def run_child(emu_lib, body, *args, timeout=1200):
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1")
    cmd = [sys.executable, "-c", HEAD + body + '\nprint("MATRIX BATCH OK")\n', ROOT] + [str(x) for x in args]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and "MATRIX BATCH OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_share_matrix_one_matrix_many_holders(emu_lib, name="M0"):
    """set_matrix on a root, factorize_columns, copy_batch into 9 children, share_matrix: every holder answers
    factorize_columns, solve_for_update_column, tableau_row, price and the batch entries as a twin that called set_matrix
    itself; dbg_matrix_holders is 10, then 9 after the root is freed, 8 beside a set_matrix of one child (which follows its
    new matrix), 7 beside a maxvolume of another (which answers INVALID_CALL); sharing into handles that have a matrix of
    their own, a shared one, or maxvolume's buffers; copy_batch in either role; every refusal with what it leaves alone.
    On M0: sharing is host code that does not depend on the matrix; M1 runs on the GPU."""
    run_child(emu_lib, "MB.check_sharing(sys.argv[2])", name)


@pytest.mark.parametrize("n", (1, 7, 8, 9, 17))
def test_tableau_row_batch_is_the_single_entry_per_member(emu_lib, n, name="M0"):
    """n holders of one matrix, clones of one root after 0 to 3 updates, each with a row of its own: for skips None, all
    isbasic and mixed per member, and prepare_update 0 and 1, tableau_row_batch gives every member the status, the bits of
    alpha, the solution and the flop statistics of the single tableau_row on a clone taken before the call, alpha is at_dot
    of that clone's y, the handles go on alike (with prepare_update through update_batch and update); the same call with
    the handle list permuted and with one group per chunk gives the same bits per member; the counts of the part behind
    the solves are two launches, one synchronize and one or two uploads per chunk.  On M0; the long columns of M1 run
    on the emulator in the replay and the pricing test below, and through this driver on the GPU (the emulator needs
    minutes for it)."""
    run_child(emu_lib, "MB.check_rows(sys.argv[2], int(sys.argv[3]))", name, n)


def test_tableau_row_batch_members_with_a_status_of_their_own(emu_lib, name="M0"):
    """one member with an out-of-range row, one without a factorization and one without a matrix get their own status
    while the others get their rows; every refusal of the two batch entries as a whole leaves the handles alone; one
    unshared handle alone is served"""
    run_child(emu_lib, "MB.check_rows_bad_members(sys.argv[2])", name)


def test_tableau_row_batch_with_a_rank_deficient_member(emu_lib):
    """a member factorized on a basis with one column twice beside regular members: what the single entry gives"""
    run_child(emu_lib, "MB.check_rows_rank_deficient()")


def test_price_batch_and_the_cost_of_the_calls(emu_lib):
    """price_batch of 18 holders, one of them without a factorization, against at_dot and the single price: a random y, one
    with -0.0 and zeros, one member's y with a NaN (equal_nan), skips None, mixed per member and all isbasic; nothing
    observable on the handles changes; three chunks and a permuted list give the same bits; dbg_matrix_counts of both batch
    entries does not depend on n within a chunk and is the same for M0 and M1"""
    run_child(emu_lib, "MB.check_pricing()")


def test_matrix_batch_replay_under_address_sanitizer(emu_lib, oracle, tmp_path):
    """One tape of the three entries on M1, recorded from the oracle and at_dot alone: set_matrix, factorize_columns,
    share_matrix into 9 holders, tableau_row_batch over 10 and over 3 members with rows, skips and wanted solutions mixed per
    member, in one chunk and in chunks of one group, price_batch with a NaN in one y; an update on the root, share_matrix
    again, and the same calls on the updated factors.  The replayer's host arrays end with their last entry, so an access
    of k_at_dot_batch or k_scatter_lhs_batch outside A, the tiles, the masks or the products is an AddressSanitizer report.
    Replayed with the plain build and with the sanitized one (the executable carries the sanitizer runtime; nothing is
    preloaded)."""
    import numpy as np

    from blu_amd import keys as K
    from tests import util_matrix as MX
    from tests import util_maxvolume as MV
    from tests.test_emu_cpu_matrix import OP_FACT_COLUMNS, OP_SET_MATRIX
    from tests.test_emu_cpu_solves import Tape

    class BatchTape(Tape):
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

        def share_matrix(self, n):
            self._i(OP_SHARE_MATRIX, n)

        def _skip(self, skip):
            self._i(0 if skip is None else 1)
            if skip is not None:
                self._i(*skip)

        def tableau_row_batch(self, rows, skips, wants, nbytes):
            self._i(OP_TABLEAU_ROW_BATCH, 0, nbytes, len(rows))
            for r, sk, w in zip(rows, skips, wants):
                self._i(r)
                self._skip(sk)
                self._i(1 if w else 0)
            self._i(K.OK)
            for r, sk, w in zip(rows, skips, wants):  # (a transposed solve_sparse leaves the factors alone: one oracle for all)
                st, il, lhs = self.o.solve_sparse([r], [1.0], "T")
                assert st == K.OK
                self._i(st)
                self._f(MX.at_dot(self.a[0], self.a[1], self.a[2], lhs, sk))
                if w:
                    self._i(len(il))
                    self._i(*il)
                    self._f(lhs)

        def price_batch(self, ys, skips, nbytes):
            self._i(OP_PRICE_BATCH, nbytes, len(ys))
            for y, sk in zip(ys, skips):
                self._skip(sk)
                self._f(y)
            self._i(K.OK)
            for y, sk in zip(ys, skips):
                self._i(K.OK)
                self._f(MX.at_dot(self.a[0], self.a[1], self.a[2], y, sk))

    subprocess.check_call(["make", "-s", "-C", CSRC, "emu_replay", "emu_replay_asan"])
    m, ncol, a = MX.m1()
    t = BatchTape(oracle)
    t.new(m, len(a[1]), 64 * len(a[1]) + 1024)
    t.set_matrix(a)
    basis, isbasic = MV.start(m, ncol)
    assert t.factorize_columns(basis) == K.OK
    y, z = MX.price_vectors(m)
    bad = y.copy()
    bad[m // 2] = np.nan

    def batches():
        t.share_matrix(9)
        rows = [(7 * k + 3) % m for k in range(10)]
        skips = [None if k % 3 == 0 else ([1] * ncol if k % 3 == 1 else list(isbasic)) for k in range(10)]
        wants = [k % 2 == 0 for k in range(10)]
        t.tableau_row_batch(rows, skips, wants, -1)
        t.tableau_row_batch(rows[:3], [None] * 3, [False] * 3, -1)
        t.tableau_row_batch(rows[::-1], skips[::-1], wants[::-1], 1)  # two chunks
        ys = [(y if k % 2 else z) * (1.0 + k) for k in range(10)]
        ys[4] = bad
        t.price_batch(ys, skips, -1)
        t.price_batch(ys[:9], [None] * 9, 1)

    batches()
    for j in range(ncol - 1, m - 1, -1):
        ci, cx = MX.column(a, j)
        if len(ci) == 0:
            continue
        st, il, lhs = t.solve_for_update(ci, cx, "N")
        assert st == K.OK
        p = int(il[np.argmax(np.abs(lhs[il]))])
        if abs(lhs[p]) < 0.05:
            continue
        xtbl = float(lhs[p])
        assert t.solve_for_update([p], None, "T")[0] == K.OK and t.update(xtbl) == K.OK
        isbasic[basis[p]], isbasic[j], basis[p] = 0, 1, j
        break
    assert t.o.stat(K.STAT_NUPDATE) == 1
    batches()
    tape = str(tmp_path / "matrix_batch.tape")
    t.write(tape)
    env = {k: v for k, v in os.environ.items() if k != "BLU_HIP_LIB"}
    env.update(BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    for exe in (REPLAY, REPLAY_ASAN):
        out = subprocess.run([exe, tape], env=env, capture_output=True, text=True, timeout=1800)
        assert "AddressSanitizer" not in out.stderr, out.stderr[-6000:]
        assert out.returncode == 0 and "REPLAY OK" in out.stdout, (exe, out.returncode, out.stdout[-500:] + out.stderr[-4000:])
