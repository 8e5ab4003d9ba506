"""The two addressings of k_pivot_loop on the CPU (the emulation build, blu_amd/csrc `make emu`).

The narrow kernel reaches its arrays by 32-bit byte offsets off scalar bases (blu_dev.h: Arr32, RecField32, LinkField32,
ColdArr32); in the emulation build that accessor asserts, at every access, that the index is non-negative and the byte
offset below the limit of the launch.  k_pivot_loop_w64 is the same kernel with pointers indexed in 64 bits; the host
chooses before every launch (BLU_ADDR32_LIMIT: the limit in bytes, 0 = always wide).  Here the general paths of
k_pivot_loop (dbg_set_no_fast: the low-latency paths of k_pivot_fast.hip are not validated by the emulator) run as
workgroups of 64 and of 128 threads, narrow and wide, and are compared with the oracle bit for bit; statistic 129 tells
which kernel the last launch was.  Each case runs in a child process: the library path is fixed when blu_amd is first
imported, the limit when a handle is created."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")
EMU = os.path.join(ROOT, "blu_amd", "libblu_emu.so")
SPECS = [(300, 8, 8, 0.5, 1, 0.3), (250, 11, 30, 0.0, 5, 0.1)]

CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
import blu_amd
from blu_amd import keys as K
from oracle import orc
assert b"gfx950" in blu_amd.lib().blu_hip_version()
spec, hint_div = %(spec)r, %(hint_div)r
cp, ri, v = orc.gen_lp_basis(*spec)
m = len(cp) - 1
o = orc.OracleBLU(m, 64 * len(ri) + 1024)
o.set_fix_d3(True)
so = o.factorize(cp[:-1], cp[1:], ri, v)
fo = o.get_factors()
for block in (64, 128):
    g = blu_amd.BLU(m, len(ri) // hint_div)
    g.dbg_set_block(block)
    g.dbg_set_no_fast(True)
    before = [g.stat(k) for k in (151, 114, K.STAT_W_MEM, K.STAT_L_MEM, K.STAT_U_MEM)]
    s = g.factorize(cp[:-1], cp[1:], ri, v)
    assert s == so == K.OK, (s, so, g.last_error())
    fg = g.get_factors()
    for key in ("rowperm", "colperm", "l_colptr", "l_rowidx", "u_colptr", "u_rowidx", "l_value", "u_value"):
        assert np.array_equal(fg[key], fo[key]), (block, key)
    for cn in ("RANK", "L_NZ", "U_NZ", "NSEARCH_PIVOT", "FACTOR_FLOPS", "BUMP_NZ", "MATRIX_NZ"):
        assert g.stat(getattr(K, "STAT_" + cn)) == o.stat(getattr(K, "STAT_" + cn)), (block, cn)
    for kind in range(6):
        assert g.stat(51 + kind) == o.stat(51 + kind), (block, "pivot kind", kind)
    assert g.stat(118) == 0  # k_pivot_loop, not a wave kernel
    after = [g.stat(k) for k in (151, 114, K.STAT_W_MEM, K.STAT_L_MEM, K.STAT_U_MEM)]
    print("RUN block %%d wide %%d narrow_launches %%d launches %%d" %% (block, g.stat(129), g.stat(130), g.stat(K.STAT_DEV_RELAUNCHES)))
    print("CAPS block %%d before %%r after %%r" %% (block, before, after))
"""


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"])
    assert os.path.exists(EMU)
    return EMU


def run_child(emu_lib, spec, limit=None, hint_div=1):
    """-> per workgroup size (64, 128): (statistic 129, narrow launches, launches), and the capacities before / after"""
    env = dict(os.environ, BLU_HIP_LIB=emu_lib, BLU_PIVOT_KERNEL="0")
    env.pop("BLU_ADDR32_LIMIT", None)
    if limit is not None:
        env["BLU_ADDR32_LIMIT"] = str(limit)
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "spec": spec, "hint_div": hint_div}], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    runs = [tuple(int(x) for x in l.split()[4::2]) for l in out.stdout.splitlines() if l.startswith("RUN")]
    caps = [l for l in out.stdout.splitlines() if l.startswith("CAPS")]
    assert len(runs) == 2, out.stdout[-2000:]
    return runs, caps


@pytest.mark.parametrize("spec", SPECS, ids=["banded", "no-triangle"])
def test_narrow_general_paths_on_the_cpu(emu_lib, spec):
    """default limit: every launch is the narrow kernel, and its asserting accessor sees every index of the general paths"""
    runs, _ = run_child(emu_lib, spec)
    for wide, narrow, launches in runs:
        assert wide == 0 and narrow == launches >= 1


@pytest.mark.parametrize("spec", SPECS, ids=["banded", "no-triangle"])
def test_wide_general_paths_on_the_cpu(emu_lib, spec):
    """BLU_ADDR32_LIMIT=0: k_pivot_loop_w64 always"""
    runs, _ = run_child(emu_lib, spec, limit=0)
    for wide, narrow, launches in runs:
        assert wide == 1 and narrow == 0 and launches >= 1


# The 300-row basis (2372 entries) in a handle created with a hint of nnz / 8 = 296.  Largest byte extent that is compared
# with the limit (statistic 151: line records, arenas, factors), as the emulation build printed it (CAPS lines of the child):
#   at creation   GROW_E0 = 33 920 bytes: the column arena, 4240 entries x 8; the others are smaller -- row arena 4770 x 4 =
#                 19 080 (W_MEM 9010), L 1256 x 8 = 10 048, U 1700 x 8 = 13 600, line records 300 x 32 = 9600
#   at the end    GROW_E1 = 52 912 bytes: the column arena, grown to 6614 entries x 8 (W_MEM 9010 -> 14 160, U 1700 -> 2626,
#                 L as it was); four launches
# With the limit one byte above GROW_E0 the first launch is narrow, and the launches after the column arena has grown are wide.
# (The slab, 67 328 bytes here, never grows and is compared with 2^32 only: blu_hip.hip, addr32_fits.)
GROW_E0 = 33920
GROW_E1 = 52912


def test_growth_between_launches_crosses_the_limit_on_the_cpu(emu_lib):
    runs, caps = run_child(emu_lib, SPECS[0], limit=GROW_E0 + 1, hint_div=8)
    print("\n".join(caps))
    for (wide, narrow, launches), line in zip(runs, caps):
        before, after = eval(line.split("before")[1].split("after")[0]), eval(line.split("after")[1])
        assert before[0] == GROW_E0 and after[0] == GROW_E1, line  # (the figures the limit was worked out from)
        assert wide == 1 and 1 <= narrow < launches, (wide, narrow, launches)  # started narrow, ended wide
