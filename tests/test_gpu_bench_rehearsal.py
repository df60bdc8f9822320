"""bench.py's N > 1 orchestration, rehearsed on ONE GPU: the ranks share cuda:0 and talk over gloo with
host-staged halos (T8GPU_REHEARSAL=1). Covers process-group set-up, SFC partitioning, per-rank plans, the
native-RCCL attempt and its agreed fall-back, the split interior / ghost-reading stage launches, the
MAX-over-ranks timing and the JSON contract; only the RCCL transport itself is not reached (it needs one
GPU per rank, which the driver's 8-GPU run provides)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(world, extra):
    env = dict(os.environ, T8GPU_REHEARSAL="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    # the plain command, as the driver issues it: bench.py starts its own N ranks (a child torchrun)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "3", "--warmup", "1",
           "--reps", "2", "--prewarm-seconds", "0.05"] + extra
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "rank 0 must print exactly one JSON line"
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("world,workload", [(2, "c1"), (3, "c2")])
def test_bench_multirank_rehearsal(world, workload):
    rec = run_bench(world, ["--workload", workload])
    assert rec["n_gpus"] == world and rec["steps"] == 3 and rec["warmup"] == 1 and rec["repetitions"] == 2
    assert rec["ms_per_step_min"] <= rec["ms_per_step"] <= rec["ms_per_step_max"]
    assert rec["scaling"] == "strong" and rec["higher_is_better"] is True and rec["vs_baseline"] is None
    assert rec["config"]["finite"] is True
    assert rec["config"]["partition"] == f"sfc-contiguous x{world}"
    assert "REHEARSAL" in rec["config"]["halo"]
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    assert rec["roofline"]["bound"] == "hbm" and 0 < rec["roofline"]["frac"] < 1.2
    assert rec["cpu_baseline"] is None            # timed on rank 0 at N = 1 only


@pytest.mark.gpu
def test_adaptive_example_on_three_ranks_rehearsal(tmp_path):
    """examples/kelvin_helmholtz_amr.py with 3 ranks sharing the GPU (uneven element counts: the criteria
    all-gather must cope), adapt + repartition cycles, CFL all-reduce, per-rank .vtu pieces and the .pvtu."""
    env = dict(os.environ, T8GPU_REHEARSAL="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    prefix = str(tmp_path / "kh")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr", "127.0.0.1",
           "--master-port", "29671", os.path.join(ROOT, "examples", "kelvin_helmholtz_amr.py"), "--steps", "45", "--adapt-every", "20",
           "--min-level", "4", "--max-level", "6", "--vtk", prefix]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "conservation drift" in out.stdout and "wrote" in out.stdout
    for r in range(3):
        assert os.path.exists(f"{prefix}_{r:04d}.vtu")
    assert os.path.exists(prefix + ".pvtu")
    drift = float(out.stdout.split("conservation drift")[-1].split()[0])
    assert drift < 1e-9
    # refinement must not depend on the rank count: amr.adapt_partitioned refreshes the ghost slots of the current
    # state itself (the example no longer does), so the same run on ONE rank reports the same indicator sums and the
    # same element counts at every adapt
    one = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "kelvin_helmholtz_amr.py"), "--steps", "45", "--adapt-every",
                          "20", "--min-level", "4", "--max-level", "6"], cwd=ROOT, capture_output=True, text=True, timeout=280,
                         env={k: v for k, v in os.environ.items() if k not in ("T8GPU_REHEARSAL", "RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert one.returncode == 0, one.stdout[-1500:] + one.stderr[-3000:]

    def adapts(text):
        return [(float(ln.split("criteria sum")[1].split()[0]), int(ln.split("elements")[1].split()[0]))
                for ln in text.splitlines() if ln.startswith("adapt at it")]
    a3, a1 = adapts(out.stdout), adapts(one.stdout)
    assert len(a3) == len(a1) == 2
    # first adapt: both runs are on the same mesh with bitwise equal states, so the indicator sums agree to rounding --
    # with stale ghost slots they differ in the third digit. (Afterwards the meshes may differ legitimately: a family
    # cut by a rank boundary is not coarsened in a partitioned run.)
    assert abs(a3[0][0] - a1[0][0]) <= 1e-9 * abs(a1[0][0]), (a3, a1)
    assert abs(a3[0][1] - a1[0][1]) <= 0.02 * a1[0][1], (a3, a1)


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["c1", "c3q"])
def test_bench_distributed_path_on_real_rccl_with_one_rank(workload):
    """T8GPU_BENCH_FORCE_DIST=1: a one-rank run through the N > 1 branch of bench.py on the REAL backend -- nccl (=RCCL)
    process group bound to the device, barrier / all-reduce on device tensors, the native communicator made from an
    id broadcast through torch.distributed, both collective bring-up decisions and the C++ stepper constructed with
    a halo descriptor. (A rank has no peer here, so no message is sent: that part is the self-exchange test's.)"""
    env = dict(os.environ, T8GPU_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("T8GPU_REHEARSAL", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", "29655", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--prewarm-seconds", "0.05", "--no-cpu-baseline", "--workload", workload]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 1 and rec["config"]["finite"] is True and rec["value"] > 0
    assert "unavailable" not in out.stderr, out.stderr[-3000:]          # no fall-back was taken
    # plain tiles (c1) and Subgrid blocks (c3q) both run on the C++ step driver with the native RCCL exchange
    assert rec["config"]["halo"] == "native rccl (C++ stepper)" and rec["config"]["driver"] == "native C++ stepper"


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2])
def test_bench_adaptive_workload_small(world):
    """bench.py --workload c5a (BASELINE config 5's loop: adapt + repartition every 20 steps inside the timed region) on a
    small forest: one rank, and two ranks sharing the GPU over gloo (adapt_partitioned + new halo lists per cycle)."""
    env = dict(os.environ, T8GPU_C5A_LEVELS="4,6", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    if world > 1:
        env["T8GPU_REHEARSAL"] = "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--workload", "c5a", "--steps", "45",
                          "--warmup", "2"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    cfg = rec["config"]
    assert rec["n_gpus"] == world and rec["steps"] == 45 and cfg["adapt_cycles_timed"] == 2 and cfg["finite"] is True
    assert cfg["step_ms"] > 0 and cfg["cycle_ms"] > 0 and rec["value"] > 0 and cfg["elements_at_end"] > 16 ** 3
    assert rec["value"] <= cfg["stepping_only_M_cell_updates_per_s"]


@pytest.mark.gpu
def test_bench_adaptive_distributed_path_on_real_rccl_with_one_rank():
    """The adaptive loop's N > 1 branch on the REAL backend with one rank (T8GPU_BENCH_FORCE_DIST=1, as above): one native
    communicator for the run, cross-check + trial steps with collective decisions, then a new halo descriptor and C++ stepper
    for every adapted mesh -- no fall-back to the python-driven stages."""
    env = dict(os.environ, T8GPU_BENCH_FORCE_DIST="1", T8GPU_C5A_LEVELS="4,6", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("T8GPU_REHEARSAL", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", "29656", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "45", "--warmup", "2",
           "--workload", "c5a"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    cfg = rec["config"]
    assert "unavailable" not in out.stderr, out.stderr[-3000:]
    assert cfg["driver"] == "native C++ stepper (native rccl halo)" and cfg["adapt_cycles_timed"] == 2 and cfg["finite"] is True


def test_bench_refuses_a_world_size_that_differs_from_gpus():
    """WORLD_SIZE != --gpus is an error, not a silently mislabelled run (needs no GPU: it exits before any GPU call)."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "WORLD_SIZE=2" in out.stderr


def test_bench_self_launch_reports_missing_gpus():
    """`python bench.py --gpus N` starts its own ranks; with fewer than N GPUs visible it says so and returns 2
    (before any GPU call, so this runs on the CPU-only build container too)."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a box with fewer than 2 GPUs")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "T8GPU_REHEARSAL")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "needs 2 GPUs" in out.stderr


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_last_timed_step_and_repeat(tmp_path):
    """--dump-outputs DIR: the state and speed estimates of the last timed step, in the solver's float type and within the
    size budget; the warm-up and the K timed steps start from the initial state whatever the wall-clock pre-warm ran (two
    runs with different pre-warm budgets write the same bits), so the dump is the oracle's state after W + K steps. --steps K
    is the step count of the one timed region."""
    import numpy as np
    import _oracle as O
    from _gpu import rel_err
    from t8gpu_amd.synth import SynthMesh
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "T8GPU_REHEARSAL")}
    dumps = []
    for i, prewarm in enumerate(("0.05", "0.5")):
        d = tmp_path / f"out{i}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c1", "--steps", "7",
                              "--warmup", "2", "--prewarm-seconds", prewarm, "--no-cpu-baseline", "--dump-outputs", str(d)],
                             cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
        rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        assert rec["steps"] == 7 and rec["repetitions"] == 1 and rec["ms_per_step"] > 0 and rec["config"]["finite"] is True
        assert sorted(os.listdir(d)) == ["speed.npy", "state.npy"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
        dumps.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    assert all(np.array_equal(dumps[0][k], dumps[1][k]) for k in ("state", "speed"))
    mesh = SynthMesh(2, 8, 8, band=0.0)                # c1
    part = mesh.partition()
    o = O.PlainCase(part, np.float64)
    for _ in range(2 + 7):
        o.iterate(0.1 * 2.0 ** -mesh.finest_level)
    state, speed = dumps[0]["state"], dumps[0]["speed"]
    assert state.dtype == np.float64 and state.shape == (5, part.N) and speed.shape == (part.F + part.B,)
    assert rel_err(state, o.current()[:, :part.N]) < 1e-10
    assert rel_err(speed[None], o.speed[None]) < 1e-10
