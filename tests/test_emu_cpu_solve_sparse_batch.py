"""blu_hip_solve_sparse_batch on the CPU: the emulation build of the library (blu_amd/csrc `make emu`, as in
tests/test_emu_cpu_solves.py) runs k_solve_sparse_batch, k_solve_upd_batch in mode 0, k_build_lt_batch, k_gather_lhs_batch
and the host side of blu_solve_sparse_batch.inc on six small bases in one call, every member with an oracle twin and a
second handle of the library, both driven by the single solve_sparse: every status, nzlhs, pattern (order included),
value and flop counter identical, bit for bit (tests/util_solve_sparse_batch.py).  The case runs in a child process: the
library path is fixed when blu_amd is first imported."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")

CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
import blu_amd
from blu_amd import keys as K
from oracle import orc
from tests import util_update as U, util_update_batch as UB, util_solve_sparse_batch as SB
assert b"gfx950" in blu_amd.lib().blu_hip_version()

# ---- six members: three synthetic LP bases of different m, a rank-deficient one, the bidiagonal basis, and one that an
# update sequence moves to an updated factorization (k_solve_upd_batch) while the others stay fresh (k_solve_sparse_batch)
mats = [orc.gen_lp_basis(240, 6, 6, 0.5, 1, 0.3), orc.gen_lp_basis(150, 5, 4, 0.8, 3, 0.6), orc.gen_lp_basis(90, 4, 5, 0.3, 7, 0.5)]
cp, ri, v = orc.gen_lp_basis(200, 6, 6, 0.5, 2, 0.3)
mats.append((cp, ri, SB.scaled(cp, v, (3, 200 // 3, 199))))
mats.append(U.csc_arrays(UB.bidiagonal_cols(8), 8))
mats.append(orc.gen_lp_basis(60, 4, 5, 0.3, 7, 0.5))
want = [K.OK, K.OK, K.OK, K.WARNING_SINGULAR_MATRIX, K.OK, K.OK]
UPD = 5
members = SB.make_members(blu_amd, orc, mats, want)
SB.refusals(blu_amd, members)
SB.move_to_updated(members[UPD], 8, 3)

seen = {0.05: set(), 0.0: set(), 1.0: set()}
for thres in seen:
    SB.set_thres(members, thres)
    for trans in "NT":
        for q in range(len(SB.SIZES)):
            seen[thres] |= SB.batch_round(blu_amd, members, trans, q, (thres, trans, q))
print("BRANCHES", seen)
assert seen[0.05] == {1, 2} and 2 in seen[0.0] and seen[1.0] == {1}, seen
assert members[UPD].h.stat(K.STAT_R_FLOPS) > 0

# ---- single calls between two batch calls: solve_sparse, solve_dense, solve_for_update / update on a fresh member (it goes
# on as an updated one) and on the updated one; then the batch again: marker, zero invariants, row-wise L reuse
SB.set_thres(members, 0.05)
for k in (0, UPD):
    SB.move_to_updated(members[k], 6, 1)
for trans in "NT":
    for q in range(len(SB.SIZES)):
        SB.batch_round(blu_amd, members, trans, q, ("after single calls", trans, q))
SB.mixed_statuses(blu_amd, orc)
print("EMU SOLVE SPARSE BATCH OK")
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def test_solve_sparse_batch_on_the_cpu(emu_lib):
    """six bases of m <= 240 from factorize_batch (three synthetic LP bases, a rank-deficient one with
    WARNING_SINGULAR_MATRIX, the bidiagonal basis with m = 8, one with at least three updates done), each with an
    oracle twin and a library handle driven by single calls: the refusals of the whole call; batched solves of both
    systems with SPARSE_THRES 0.05, 0.0 and 1.0 and right-hand sides of 0, 1, 5, 70 and m/2 entries, different per
    member (status, nzlhs, pattern order, values, L_FLOPS, U_FLOPS, R_FLOPS, statistic 43; both branches seen under
    0.05, the sequential one under 0.0, only the symbolic one under 1.0); single solve_sparse, solve_dense,
    solve_for_update and update calls on two members and the batch again; the per-member statuses of a mixed call."""
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1")
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "EMU SOLVE SPARSE BATCH OK" in out.stdout
