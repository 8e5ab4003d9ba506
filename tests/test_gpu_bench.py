"""bench.py on the GPU box under the launcher the driver uses (`python -m torch.distributed.run`), at world size 1:
the child is started before anything in this process touches the GPU API on its behalf, initialises the `nccl`
(= RCCL) process group, and runs the barrier / MAX / SUM reductions of blu_amd/shard.py around the timed region --
the N > 1 code path, executed on real hardware with the one GPU a box has."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_under_torch_distributed_run_world_size_one():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29541", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C4", "--steps", "1", "--warmup", "0",
           "--batch", "0", "--no-cpu-baseline"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["n_gpus"] == 1 and rec["scaling"] == "weak" and rec["value"] > 0
    assert rec["config"]["workload"].startswith("C4") and rec["roofline"]["bound"] == "hbm"
    assert "process group: nccl" in out.stderr + out.stdout


def test_bench_batched_leg_verifies_its_members():
    """The secondary (batched) measurement of bench.py end to end on a small batch: 64 distinct matrices with per-handle
    device inputs, cold step + three warm steps, and -- after the timed steps -- eight members checked against the CPU
    oracle (`verified_members`); the roofline object of the leg names the batch pivot kernel the library chose."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C2", "--steps", "2", "--warmup", "1", "--full", "--batch", "300",
           "--no-batch-sizes", "--no-cpu-baseline"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    b = rec["batched"]
    assert b["bases_in_flight_per_gpu"] == 300 and b["distinct_matrices"] == 64 and b["verified_members"] == 8
    assert len(b["seconds_warm_steps"]) == 3 and b["cold_first_step"]["seconds"] > 0
    assert "k_pivot_loop_wave2" in b["roofline"]["kernel"] and 0 < b["roofline"]["frac"] < 1
    assert rec["config"]["generator_note"].startswith("bw = 8, not SURVEY.md 8d's provisional 16")  # (C2 is lp_basis(10 000, 8, bw 8, ...))


def test_bench_plain_run_dumps_its_last_step(tmp_path, oracle):
    """A plain run (no --full) does the timed steps and prints the line: no batched legs, no CPU baseline.  With
    --dump-outputs it writes what its last step computed -- the factors and the result statistics, float64 -- and those
    are the oracle's on the same basis (integer arrays and statistics bit for bit, values within 1e-12 relative)."""
    import numpy as np
    from blu_amd import keys as K
    from blu_amd import shard
    from blu_amd.matrices import CONFIGS
    from tests import util
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C2", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert not {"batched", "batched_other_sizes", "cpu_baseline", "vs_cpu_baseline_per_gpu"} & set(rec)
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(got) == set(util.INT_KEYS + util.VAL_KEYS) | {"stats"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    c = CONFIGS["C2"]
    cp, ri, v = oracle.gen_lp_basis(c["m"], c["k"], c["bw"], c["tri_frac"], shard.seed_of_basis(c, 0), c["offscale"])
    o, so = util.oracle_factorize(oracle, cp, ri, v)
    assert so == K.OK
    util.assert_same_factors(got, o.get_factors())
    keys = [K.STAT_RANK, K.STAT_MATRIX_NZ, K.STAT_BUMP_SIZE, K.STAT_BUMP_NZ, K.STAT_L_NZ, K.STAT_U_NZ, K.STAT_NSEARCH_PIVOT,
            K.STAT_FACTOR_FLOPS, K.STAT_RANKDEF, 50, 51, 52, 53, 54, 55, 56, K.STAT_MIN_PIVOT, K.STAT_MAX_PIVOT,
            K.STAT_CONDEST_L, K.STAT_CONDEST_U, K.STAT_NORM_L, K.STAT_NORM_U, K.STAT_NORMEST_L_INV, K.STAT_NORMEST_U_INV,
            K.STAT_ONENORM, K.STAT_INFNORM, K.STAT_RESIDUAL_TEST]
    assert len(got["stats"]) == len(keys)
    # (51..56, pivots per pivot routine: the batched legs compare those with the oracle, this test does not)
    sel = [i for i, k in enumerate(keys) if not 51 <= k <= 56]
    assert np.array_equal(got["stats"][sel], np.array([o.stat(keys[i]) for i in sel]))
