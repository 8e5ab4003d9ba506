"""The dual simplex of tests/util_simplex.py on the CPU: the emulation build of the library (blu_amd/csrc `make emu`) runs the
single driver on `tu`, `tu2` and `infeasible` at (12, 36) and a generation of 9 forked nodes at (12, 36) beside the exact
twin, with no tolerance anywhere -- the drivers tests/test_gpu_simplex.py runs on hardware, so that a failure there is
localized without a GPU.  Each case runs in a child process: the library path is fixed when blu_amd is first imported.
The larger shapes stay on hardware.  The properties of the committed seeds that are asserted on the twin alone, and the
twin against HiGHS, need no library and run here for every committed case."""
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
from tests import util_simplex as S
assert b"gfx950" in blu_amd.lib().blu_hip_version()
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def run_child(emu_lib, body, *args, timeout=1200):
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="1", BLU_HIP_NO_CHAIN="1")
    cmd = [sys.executable, "-c", HEAD + body + '\nprint("SIMPLEX OK")\n', ROOT] + [str(x) for x in args]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and "SIMPLEX OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_the_committed_seeds_show_their_properties():
    """enough iterations and refactorizations, every kind entering, a fixed column leaving, both sigmas, ties by index and
    by |alpha|, Harris changing the trajectory, winners behind column 1024, children finishing at three iteration counts;
    every optimum against HiGHS"""
    from tests import util_simplex as S

    S.committed_properties()


@pytest.mark.parametrize("family,dualtol", (("tu", 0.0), ("tu2", 0.0), ("tu2", 0.25), ("infeasible", 0.0)))
def test_a_run_is_the_twins(emu_lib, family, dualtol):
    """every iteration of the single driver against the twin, a refactorization every 5 updates"""
    run_child(emu_lib, "S.check_single(sys.argv[2], 12, 36, float(sys.argv[3]))", family, dualtol)


def test_a_run_without_refactorizations_is_the_twins(emu_lib):
    run_child(emu_lib, "S.check_single('tu2', 12, 36, 0, every=S.NEVER)")


def test_a_generation_of_forked_nodes(emu_lib):
    """9 children of an updated root in lock step through the batch entries, each beside its twin and beside the single
    entries on a clone; the active set shrinks from a full group and one to partial groups"""
    run_child(emu_lib, "nodes, sizes = S.run_generation('tu', 12, 36, 9)\nassert sizes[0] == 9 and len(set(sizes)) >= 3, sizes\n"
                       "assert 'infeasible' in {c.status for c in nodes}")
