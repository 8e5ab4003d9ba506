"""The integer-valued bases of tests/util_exact.py without a GPU: the emulation build of the library (blu_amd/csrc `make emu`,
as in tests/test_emu_cpu_solves.py) runs k_pivot_loop_wave, k_pivot_loop_wave2, the batch form, the one-workgroup solves and
the update path on the host, with the assertions of tests/test_gpu_exact.py: bit for bit against the oracle, and on the
totally unimodular families exact in int64 with no oracle and no tolerance.  The default single-basis pivot kernel and the
chain pipeline are not emulated.  This is where a device bug that the GPU tests find is localized, and where the mutation
checks of DESIGN.md (a strict comparison in wv_search, the doubleton cancellation branch dropped) were made.
Each case runs in a child process: the library path is fixed when blu_amd is first imported."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")

HEAD = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
import blu_amd
from blu_amd import keys as K
from oracle import orc
from tests import util_exact as X
assert b"gfx950" in blu_amd.lib().blu_hip_version()
kernel = %(kernel)d
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def run_child(emu_lib, body, kernel, ok):
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL=str(kernel), BLU_HIP_NO_CHAIN="1")
    out = subprocess.run([sys.executable, "-c", (HEAD + body) % {"root": ROOT, "kernel": kernel}], env=env, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0 and ok in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


CHILD_CASES = r"""
for name in X.EMU_CASES:
    X.check_case(blu_amd, orc, name, kernel=kernel)
print("CASES OK")
"""


@pytest.mark.parametrize("kernel", [1, 3], ids=["wave", "wave2"])
def test_exact_cases_on_the_cpu(emu_lib, kernel):
    """tree bases (64, 6) and (96, 8), interval matrix (64, 5), small-integer (120, 4), dense-integer 100 and the basis with
    stored zeros, one basis at a time with k_pivot_loop_wave and k_pivot_loop_wave2"""
    run_child(emu_lib, CHILD_CASES, kernel, "CASES OK")


CHILD_GENERAL = r"""
for name in ("tree-96-8", "interval-64-5", "smallint-120-4", "zeros"):
    X.check_case(blu_amd, orc, name, setup=lambda g: g.dbg_set_no_fast(True), kernel=kernel, solves=False)
print("GENERAL OK")
"""


def test_exact_cases_general_paths_on_the_cpu(emu_lib):
    """the general pivot paths alone (k_pivot.hip as a workgroup of one wave)"""
    run_child(emu_lib, CHILD_GENERAL, 1, "GENERAL OK")


CHILD_BATCH = r"""
X.check_batch(blu_amd, orc, X.EMU_CASES)
print("BATCH OK")
"""


def test_exact_cases_as_a_batch_on_the_cpu(emu_lib):
    """the same inputs as members of one blu_hip_factorize_batch call (the emulated device has a batch take the one-wave kernel;
    which register budget and kernel a batch takes on the MI355X is asserted in tests/test_gpu_exact.py)"""
    run_child(emu_lib, CHILD_BATCH, 0, "BATCH OK")


CHILD_THRESHOLDS = r"""
for params in X.EQUALITY_PARAMS:
    for name in ("tree-64-6", "tree-96-8", "smallint-120-4"):
        X.check_case(blu_amd, orc, name, params=params, kernel=kernel, solves=False)
X.check_abstol_equality(blu_amd, orc)
X.check_droptol_equality(blu_amd, orc)
print("THRESHOLDS OK")
"""


@pytest.mark.parametrize("kernel", [1, 3], ids=["wave", "wave2"])
def test_thresholds_at_equality_on_the_cpu(emu_lib, kernel):
    """RELTOL 1.0 and 0.5, NZBIAS -1 with the row search, MAXSEARCH 1; ABSTOL equal to every column maximum and one ulp
    above; DROPTOL 1.0"""
    run_child(emu_lib, CHILD_THRESHOLDS, kernel, "THRESHOLDS OK")


CHILD_UPDATES = r"""
log, kinds = X.check_updates(blu_amd, orc, 64, 6, 40)
print("SINGLE", log["done"], log["singular"], kinds)
print("BATCH", X.check_updates_batch(blu_amd, orc, ((64, 6), (64, 6)), 40))
print("UPDATES OK")
"""


def test_exact_updates_on_the_cpu(emu_lib):
    """40 steps of the exact update schedule at m = 64, through the single calls and through the batched ones"""
    run_child(emu_lib, CHILD_UPDATES, 1, "UPDATES OK")
