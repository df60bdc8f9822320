"""-m gpu: the native step driver writes the per-face speed estimates in the third stage of a call's LAST step only
(stepper.hip: stage_args; t8gpu_hip_stepper_set_speed_every_step). After any iterate_steps(n) call the state and
speed[:F + B] must hold, bit for bit, what n single-step calls leave there and what the every-step mode leaves there; the last
step must still write every face; and the intermediate writes must really be gone (speed_stages()).

Every equality is on the raw bits (the arrays viewed as integers). Meshes, each holding every kernel form of its kind:
  2d      SynthMesh(2, 5, 7, band=0.2): 13 696 quadrilaterals, 24 patch tiles beside generic tiles; z-momentum +0, so that
          set_planar(2) runs the planar stage (auto mode would never pick it at this size) and set_planar(0) the general one
  3d      SynthMesh(3, 4, 5, band=0.15): 25 600 hexahedra, 16 regular + 48 irregular 3D patches beside generic tiles (fp32: the 16 regular
          ones, the rest in generic tiles)
  curved  PrismHexMesh((8, 8, 8), split=0.5, shell_map): prisms and hexahedra with walls; no patches, and too many distinct face
          geometries for a dictionary
"""
import functools
import types

import numpy as np
import pytest
import torch

from _gpu import perturbed_state, rel_err
from t8gpu_amd import hip, native
from t8gpu_amd.solver import PlainSolver
from t8gpu_amd.synth import SynthMesh
from t8gpu_amd.unstructured import PrismHexMesh, shell_map

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
_BITS = {torch.float64: torch.int64, torch.float32: torch.int32}
# a quiet NaN with a payload no kernel produces
_MARK = {torch.float64: 0x7FF8_0000_DEAD_BEEF, torch.float32: 0x7FC0_BEEF}

# (mesh, flux, planar mode of the stepper or None)
CASES = [("2d", hip.KEPES, 2), ("2d", hip.KEPES, 0), ("2d", hip.HLLC, 2), ("2d", hip.HLLC, 0), ("3d", hip.KEPES, None),
         ("curved", hip.KEPES, None)]
CASE_IDS = ["2d-kepes-planar", "2d-kepes-general", "2d-hllc-planar_asked", "2d-hllc-general", "3d-kepes", "curved-kepes"]


@functools.lru_cache(maxsize=None)
def problem(name):
    """(partition, initial state, delta_t, plan options)"""
    if name == "2d":
        part = SynthMesh(2, 5, 7, band=0.2).partition()
        rng = np.random.default_rng(11)
        n = part.N + part.G
        rho = 1.0 + 0.3 * rng.uniform(-1, 1, n)
        v = 0.4 * rng.standard_normal((2, n))
        p = 1.0 + 0.2 * rng.uniform(-1, 1, n)
        st = np.stack([rho, rho * v[0], rho * v[1], np.zeros(n), p / 0.4 + 0.5 * rho * (v ** 2).sum(0)])
        return part, st, 0.1 * 2.0 ** -7, None
    if name == "3d":
        part = SynthMesh(3, 4, 5, band=0.15).partition()
        return part, perturbed_state(part, 12), 0.1 * 2.0 ** -5, None
    part = PrismHexMesh((8, 8, 8), split=0.5, mapping=shell_map).partition()
    return part, perturbed_state(part, 13), 0.1 * float(np.cbrt(part.volumes.min())), None


def bits(t):
    return t.contiguous().view(_BITS[t.dtype])


def make(case, dtype, every_step=False, graph=False):
    name, kind, planar = case
    part, st, dt, opts = problem(name)
    s = PlainSolver(part, dtype, flux_kind=kind, mode="fused", state=st, plan_options=opts)
    s.use_native_stepper()
    if planar is not None:
        s.stepper.set_planar(planar)
    if every_step:
        s.stepper.set_speed_every_step(True)
    if graph:
        s.stepper.graph(True)
    return s, dt


def snapshot(s):
    torch.cuda.synchronize()
    nf = s.F + s.B
    return (s.next, s.prev), bits(s.state()).clone(), bits(s.speed[:nf]).clone()


def assert_same(got, want):
    assert got[0] == want[0]
    assert torch.equal(got[1], want[1]), "state"
    assert torch.equal(got[2], want[2]), "speed"


def assert_form(s, case):
    """the 2D KEPES cases ran the stage form they are named after"""
    if case[0] == "2d" and case[1] == hip.KEPES:
        assert s.stepper.planar() == (1 if case[2] == 2 else 0)


@functools.lru_cache(maxsize=None)
def single_steps(case, dtype):
    """The reference, computed once per case: snapshots after 1, 2, 3 and 4 calls of iterate_steps(1), and compute_timestep()
    after the fourth."""
    s, dt = make(case, dtype)
    out = []
    for _ in range(4):
        s.iterate_steps(1, dt)
        assert s.stepper.speed_stages() == 1
        out.append(snapshot(s))
    return out, s.compute_timestep(max_level=0)


def test_meshes_hold_every_kernel_form():
    c = make(CASES[0], torch.float64)[0].plan.c
    assert c.patch_dim != 3 and sum(c.n_patch_tiles) == 24 and c.ntiles - sum(c.n_patch_tiles) >= 2
    c = make(CASES[4], torch.float64)[0].plan.c
    assert c.patch_dim == 3 and sum(c.n_patch_tiles) == 64 and sum(c.n_irregular_tiles) == 48 and c.ntiles - 64 >= 2
    c = make(CASES[4], torch.float32)[0].plan.c
    assert c.patch_dim == 3 and sum(c.n_patch_tiles) >= 16 and c.ntiles - sum(c.n_patch_tiles) >= 2
    s = make(CASES[5], torch.float64)[0]
    assert sum(s.plan.c.n_patch_tiles) == 0 and s.B > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_multi_step_call_equals_single_step_calls(case, dtype):
    """1. iterate_steps(n), n = 1 .. 4 (odd and even: the prev / next swap), against n calls of iterate_steps(1) and against
    the every-step mode"""
    ref, _ = single_steps(case, dtype)
    for n in (1, 2, 3, 4):
        a, dt = make(case, dtype)
        a.iterate_steps(n, dt)
        b, _ = make(case, dtype, every_step=True)
        b.iterate_steps(n, dt)
        got, every = snapshot(a), snapshot(b)
        assert_form(a, case)
        assert_form(b, case)
        assert_same(got, ref[n - 1])
        assert_same(got, every)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_last_step_writes_every_face(case, dtype):
    """2. no entry of speed[:F + B] keeps the mark it was filled with before the call"""
    s, dt = make(case, dtype)
    bits(s.speed).fill_(_MARK[dtype])
    assert int((bits(s.speed) == _MARK[dtype]).sum()) == s.speed.numel() and bool(torch.isnan(s.speed).all())
    s.iterate_steps(3, dt)
    torch.cuda.synchronize()
    nf = s.F + s.B
    assert nf > 0 and int((bits(s.speed[:nf]) == _MARK[dtype]).sum()) == 0
    assert_same(snapshot(s), single_steps(case, dtype)[0][2])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_intermediate_writes_are_gone(case, dtype):
    """3. the stages of a call that were handed the array: one by default, one per step in every-step mode"""
    s, dt = make(case, dtype)
    assert s.stepper.speed_stages() == 0
    s.iterate_steps(3, dt)
    assert s.stepper.speed_stages() == 1
    s.stepper.set_speed_every_step(True)
    s.iterate_steps(3, dt)
    assert s.stepper.speed_stages() == 3
    s.iterate_steps(1, dt)
    assert s.stepper.speed_stages() == 1
    s.stepper.set_speed_every_step(False)
    s.iterate_steps(1, dt)
    assert s.stepper.speed_stages() == 1
    s.iterate(dt)
    assert s.stepper.speed_stages() == 1
    torch.cuda.synchronize()


def test_mode_from_the_environment(monkeypatch):
    """the initial mode of a stepper is T8GPU_SPEED_EVERY_STEP at the time it is created"""
    for value, want in (("1", 2), ("0", 1), ("", 1)):
        monkeypatch.setenv("T8GPU_SPEED_EVERY_STEP", value)
        s, dt = make(CASES[1], torch.float64)
        s.iterate_steps(2, dt)
        assert s.stepper.speed_stages() == want, value
    monkeypatch.delenv("T8GPU_SPEED_EVERY_STEP")
    s, dt = make(CASES[1], torch.float64)
    s.iterate_steps(2, dt)
    assert s.stepper.speed_stages() == 1
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[4], CASES[5]], ids=[CASE_IDS[0], CASE_IDS[3], CASE_IDS[4], CASE_IDS[5]])
def test_graph_replay(case, dtype):
    """4. a replayed graph against the direct enqueue, and the mode as part of the graph's key: a toggled mode is never served
    by the graph captured for the other one"""
    a, dt = make(case, dtype)
    b, _ = make(case, dtype, graph=True)
    for _ in range(2):                      # (6 steps: the roles do not swap, the second call replays the first one's graph)
        a.iterate_steps(6, dt)
        b.iterate_steps(6, dt)
    assert b.stepper.graph() == (1, 2) and b.stepper.speed_stages() == 1
    assert_form(b, case)
    assert_same(snapshot(b), snapshot(a))
    for on, stages, captures, replays in ((True, 6, 2, 3), (False, 1, 2, 4), (True, 6, 2, 5)):
        b.stepper.set_speed_every_step(on)
        a.iterate_steps(6, dt)
        b.iterate_steps(6, dt)
        assert b.stepper.speed_stages() == stages
        assert b.stepper.graph() == (captures, replays)
        assert_same(snapshot(b), snapshot(a))


@pytest.mark.parametrize("dtype,classes", [(torch.float64, 2), (torch.float64, 3), (torch.float32, 2)], ids=["f64-2", "f64-3", "f32-2"])
def test_two_lane_driver(dtype, classes):
    """5. A stepper with peers on one GPU: rank 0 of a shift-symmetric two-way split exchanging with itself through a one-rank
    RCCL communicator (test_gpu_halo.py). iterate_steps(3) then iterate_steps(2) through the two lanes:
      * bit for bit the state and speed[:F + B] of the same stepper driven one step per call (what the driver did before for
        every step) and of the every-step mode;
      * speed_stages() is 1 after each call, however many lanes and tile classes a stage is launched in;
      * against the single-lane stepper of the whole mesh on this rank's half. That comparison cannot be on the bits: the
        single-rank mesh lists the faces at y = 1/2 and at the periodic seam with the opposite orientation and numbers its faces
        differently (test_gpu_halo.py), so the state agrees to rounding (1e-12 / 1e-5 relative after 5 steps, the bound used
        there for 19) and of the speed array only the maximum, which is what compute_timestep reads, can be compared."""
    mesh = SynthMesh(2, 5, 8, band=0.05)
    whole, half = mesh.partition(), mesh.partition(0, 2)
    assert half.N * 2 == whole.N and half.peers.tolist() == [1]
    x, y = whole.centres[:, 0], whole.centres[:, 1]
    rho = 1.5 + 0.4 * np.sin(4 * np.pi * y) * np.cos(2 * np.pi * x)
    v1, v2 = 0.3 * np.cos(4 * np.pi * y), 0.2 * np.sin(2 * np.pi * x) * np.sin(4 * np.pi * y)
    st = np.stack([rho, rho * v1, rho * v2, 0 * rho, 2.5 / 0.4 + 0.5 * rho * (v1 * v1 + v2 * v2)])
    n2 = whole.N // 2
    st[:, n2:] = st[:, :n2]
    gidx = np.concatenate([np.arange(half.N), half.ghost_global])
    dt = 0.1 * 2.0 ** -mesh.finest_level
    comm = native.NativeComm(0, 1, lambda b, src: b)
    fake = types.SimpleNamespace(N=half.N, G=half.G, cells_per_element=1, peers=np.zeros(1, np.int32), send_off=half.send_off,
                                 recv_off=half.recv_off, send_idx=half.send_idx)

    def run(calls, every_step):
        local = st[:, gidx].copy()
        local[:, half.N:] = np.nan                                            # ghosts must arrive through RCCL
        g = PlainSolver(half, dtype, mode="fused", state=local, plan_options=dict(tmax=64, fcap=160, two_classes=classes == 2))
        hp = g.plan.host
        assert 0 < hp.n_interior < hp.ntiles and (hp.n_deep == hp.n_interior if classes == 2 else 0 < hp.n_deep < hp.n_interior)
        g.use_native_stepper(native.NativeHalo(fake, dtype, comm))
        g.stepper.set_speed_every_step(every_step)
        bits(g.speed).fill_(_MARK[dtype])
        stages = []
        for n in calls:
            g.iterate_steps(n, dt)
            stages.append(g.stepper.speed_stages())
        assert native.stream_wait(torch.cuda.current_stream(), 30.0) == 0
        snap = snapshot(g)
        top = g.max_speed()
        g.stepper = None
        return snap, stages, top

    got, stages, top = run((3, 2), False)
    assert stages == [1, 1]
    assert int((got[2] == _MARK[dtype]).sum()) == 0                         # the last step wrote every face of both lanes
    single, stages1, _ = run((1, 1, 1, 1, 1), False)
    assert stages1 == [1] * 5
    every, stages3, _ = run((3, 2), True)
    assert stages3 == [3, 2]
    comm.destroy()
    assert_same(got, single)
    assert_same(got, every)
    one = PlainSolver(whole, dtype, mode="fused", state=st)                   # the single-lane stepper
    one.use_native_stepper()
    one.iterate_steps(3, dt)
    one.iterate_steps(2, dt)
    torch.cuda.synchronize()
    assert one.stepper.speed_stages() == 1
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    state = got[1].view(dtype).cpu().numpy()
    assert np.isfinite(state).all()
    assert rel_err(state, one.state().cpu().numpy()[:, :half.N]) < tol
    assert abs(top - one.max_speed()) < tol * one.max_speed()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_compute_timestep(case, dtype):
    """6. compute_timestep() after iterate_steps(4) is the value after four single steps"""
    _, want = single_steps(case, dtype)
    s, dt = make(case, dtype)
    s.iterate_steps(4, dt)
    got = s.compute_timestep(max_level=0)
    assert np.isfinite(got) and got > 0
    assert np.float64(got).view(np.int64) == np.float64(want).view(np.int64)
