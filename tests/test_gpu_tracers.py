"""-m gpu: tracer particles on the device (t8gpu_hip_tracers_*, _Solver.tracers) against the numpy definitions
of t8gpu_amd/tracers.py on the inputs of _tracers_ref.py. Everything is compared BITWISE: x, xs, k1 as 64-bit patterns (hence
NaN payloads and infinities too), status and flag as bytes. test_tracers_host.py asserts what those inputs cover."""
import functools
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _tracers_ref as ref
from _gpu import NP
from t8gpu_amd import amr, sample, tracers
from t8gpu_amd.solver import PlainSolver, SubgridSolver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float64, torch.float32]
MESHES = ref.NAMES
INT32_MAX = 2 ** 31 - 1


def make_solver(part, dtype, state, mode="compat"):
    if part.subgrid:
        return SubgridSolver(part, dtype, mode=mode, state=state, open_boundaries=True, farfield=True,
                             inflow_states=ref.INFLOW_STATES)
    return PlainSolver(part, dtype, mode=mode, state=state, inflow_states=ref.INFLOW_STATES)


def host(t):
    return t.cpu().numpy()


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def two_state_solver(mesh, subgrid, dtype, part=None):
    """a solver that holds u^n in state(next) and u^(n+1) in state(prev): begin_step() swaps which one the tracers read"""
    u = ref.states_of(mesh, subgrid)
    part = ref.partition(mesh, subgrid) if part is None else part
    u = [ref.rank_state(mesh, subgrid, s, part) for s in u]
    solver = make_solver(part, dtype, u[0])
    solver.planes[5 * solver.prev:5 * solver.prev + 5, :u[1].shape[1]] = dev(u[1], dtype)
    return solver


@functools.lru_cache(maxsize=None)
def case(mesh, subgrid, dtype):
    """(solver, points): built once; the tests make their own Tracers and leave the solver's two states as they are (an even
    number of begin_step calls)"""
    return two_state_solver(mesh, subgrid, dtype), ref.points_of(mesh, subgrid)[0]


def assert_phase(tr, want, names, where):
    got = {n: host(getattr(tr, n)) for n in names}
    for n in names:
        assert ref.bits_equal(got[n], want[n]), (where, n, np.flatnonzero(np.any(np.atleast_2d(got[n].T != want[n].T), axis=0))[:8])


MID, END = ("xs", "k1", "flag", "status", "x"), ("x", "status", "xs", "k1", "flag")


def run_rounds(tr, solver, mesh, subgrid, dtype, rounds=ref.ROUNDS, **kw):
    """predict / swap state / correct, compared with the host rounds after every phase"""
    dt = ref.DT[mesh]
    want = ref.reference(mesh, subgrid, NP[dtype])
    x = ref.points_of(mesh, subgrid)[0]
    for r in range(rounds):
        mid, end, _ = want[r]
        tr.predict(dt, **kw)
        solver.begin_step()
        assert_phase(tr, dict(mid, x=x), MID, (r, "predict"))
        tr.correct(dt, **kw)
        assert_phase(tr, end, END, (r, "correct"))
        x = end["x"]
    if rounds % 2:
        solver.begin_step()


# ---- 1: velocity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_velocity_equals_host_velocity(mesh, subgrid, dtype):
    solver, points = case(mesh, subgrid, dtype)
    part = solver.part
    tr = solver.tracers(points)
    assert tr.x.dtype == torch.float64 and tr.status.dtype == torch.uint8 and tuple(tr.x.shape) == points.shape
    k, held = tr.velocity("x")
    assert k.dtype == torch.float64 and held.dtype == torch.int32 and tuple(k.shape) == points.shape
    u = ref.states_of(mesh, subgrid)[0].astype(NP[dtype])
    want_k, want_held = tracers.host_velocity(part, u, points)
    cells = sample.host_locate(part, points)
    assert np.array_equal(host(held), (cells >= 0).astype(np.int32)) and np.array_equal(host(held), want_held)
    assert ref.bits_equal(host(k), want_k)
    assert np.isinf(want_k).any() and np.isnan(want_k).any() and (want_held == 0).any()          # the planted cells, the seeds
    # the hint now holds the element found
    S = part.cells_per_element
    assert np.array_equal(host(tr.hint_x), np.where(cells >= 0, cells // S, -1))
    # the other state, from xs (still the seeds)
    k, held = tr.velocity("xs", step=solver.prev)
    want_k, _ = tracers.host_velocity(part, ref.states_of(mesh, subgrid)[1].astype(NP[dtype]), points)
    assert ref.bits_equal(host(k), want_k) and np.array_equal(host(held), want_held)


# ---- 2, 3: rounds, fused and unfused ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_rounds_equal_the_host_rounds(mesh, subgrid, dtype):
    solver, points = case(mesh, subgrid, dtype)
    tr = solver.tracers(points)
    run_rounds(tr, solver, mesh, subgrid, dtype)
    c = tr.counts()
    assert sum(c) == points.shape[0] and c[0] > 0 and c[2] > 0
    h = tr.host()
    assert ref.bits_equal(h["x"], host(tr.x)) and h["status"].dtype == np.uint8
    # fields at the particles: the sampler on tr.x
    got = tr.sample(["density"])["density"]
    assert ref.bits_equal(host(got), host(solver.sample_points(tr.x, ["density"])["density"]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_fused_step_equals_velocity_plus_move(mesh, subgrid, dtype):
    solver, points = case(mesh, subgrid, dtype)
    fused, split = solver.tracers(points), solver.tracers(points)
    dt = ref.DT[mesh]
    for r in range(ref.ROUNDS):
        fused.predict(dt)
        k, held = split.velocity("x")
        split.predict(dt, k=k, held=held)
        solver.begin_step()
        for n in MID:
            assert ref.bits_equal(host(getattr(fused, n)), host(getattr(split, n))), (r, n)
        fused.correct(dt)
        k, held = split.velocity("xs")
        split.correct(dt, k=k, held=held)
        for n in END:
            assert ref.bits_equal(host(getattr(fused, n)), host(getattr(split, n))), (r, n)
    solver.begin_step()
    # and both are the host's
    want = ref.reference(mesh, subgrid, NP[dtype])[-1][1]
    assert_phase(split, want, END, "split")


# ---- 4: hints -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", ["refined-2d-walls", "band-2d", "walls-open-3d"])
def test_result_does_not_depend_on_the_hints(mesh, subgrid):
    dtype = torch.float64
    solver, points = case(mesh, subgrid, dtype)
    m, n = points.shape[0], solver.part.N
    rng = np.random.default_rng(9)
    true = solver.tracers(points)
    true.velocity("x")
    true.velocity("xs")                                             # (both hint arrays now hold the true elements)
    fills = {"minus one": np.full(m, -1), "n": np.full(m, n), "int32 max": np.full(m, INT32_MAX), "int32 min": np.full(m, -2 ** 31),
             "random": rng.integers(0, n, m), "true": host(true.hint_x)}
    want = ref.reference(mesh, subgrid, NP[dtype])
    for name, fill in fills.items():
        tr = solver.tracers(points)
        hint = torch.from_numpy(fill.astype(np.int32)).cuda()
        for r in range(2):
            if r == 0:
                tr.hint_x.copy_(hint)
                tr.hint_xs.copy_(hint)
            tr.predict(ref.DT[mesh])
            solver.begin_step()
            assert_phase(tr, want[r][0], ("xs", "k1", "flag", "status"), (name, r, "predict"))
            tr.correct(ref.DT[mesh])
            assert_phase(tr, want[r][1], END, (name, r, "correct"))
        # what the pass leaves in the hints: the elements of the active particles' points
        S = solver.part.cells_per_element
        cells = sample.host_locate(solver.part, want[1][0]["xs"])
        still = want[1][0]["status"] == 0
        got = host(tr.hint_xs)
        assert np.array_equal(got[still], np.where(cells >= 0, cells // S, -1)[still]), name
    # the unfused velocity takes the same hints
    for name, fill in fills.items():
        tr = solver.tracers(points)
        tr.hint_x.copy_(torch.from_numpy(fill.astype(np.int32)).cuda())
        k, held = tr.velocity("x")
        k0, held0 = true.velocity("x")
        assert ref.bits_equal(host(k), host(k0)) and np.array_equal(host(held), host(held0)), name
        assert np.array_equal(host(tr.hint_x), host(true.hint_x)), name


# ---- 5: loopback ranks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3, 5])
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", ["refined-2d-periodic", "open-2d", "walls-open-3d"])
def test_loopback_ranks_give_the_single_rank_bits(mesh, subgrid, nranks):
    dtype = torch.float64
    points = ref.points_of(mesh, subgrid)[0]
    solvers = [two_state_solver(mesh, subgrid, dtype, ref.partition(mesh, subgrid, r, nranks)) for r in range(nranks)]
    trs = [s.tracers(points) for s in solvers]
    want = ref.reference(mesh, subgrid, NP[dtype])
    inside = sample.host_locate(ref.partition(mesh, subgrid), points) >= 0
    dt = ref.DT[mesh]
    for r in range(ref.ROUNDS):
        for phase, which in (("predict", "x"), ("correct", "xs")):
            ks, helds = zip(*[t.velocity(which) for t in trs])
            k, held = torch.stack(ks).sum(dim=0), torch.stack(helds).sum(dim=0, dtype=torch.int32)
            if r == 0 and phase == "predict":
                assert np.array_equal(host(held), inside.astype(np.int32))       # exactly one rank holds a point inside
            assert int(held.max()) == 1
            for t in trs:
                getattr(t, phase)(dt, k=k, held=held)
            if phase == "predict":
                for s in solvers:
                    s.begin_step()
            for t in trs:
                assert_phase(t, want[r][0 if phase == "predict" else 1], END, (r, phase))


@pytest.mark.parametrize("subgrid", [False, True])
def test_dist_argument_on_a_one_rank_group(tmp_path, subgrid):
    """velocity, the all_reduce of the k / held block and move on a gloo group of one rank: the rounds of the fused path"""
    import datetime

    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/store", rank=0, world_size=1,
                            timeout=datetime.timedelta(seconds=30))
    try:
        mesh, dtype = "walls-open-3d", torch.float32
        solver, points = case(mesh, subgrid, dtype)
        run_rounds(solver.tracers(points), solver, mesh, subgrid, dtype, rounds=2, dist=dist)
    finally:
        dist.destroy_process_group()


# ---- 6: a real flow step between the phases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
def test_flow_step_between_the_phases(subgrid, dtype):
    """fused mode, the native stepper, no host sync between predict, the step and correct: the result is the host round on
    the states read back before and after"""
    mesh = "refined-2d-periodic"
    part, kinds = ref.partition(mesh, subgrid), ref.kinds_of(mesh)
    points = ref.points_of(mesh, subgrid)[0]
    cls = SubgridSolver if subgrid else PlainSolver
    solver = cls(part, dtype, mode="fused")
    solver.use_native_stepper()
    tr = solver.tracers(points)
    dt = 0.1 * 2.0 ** -(part.mesh.finest_level + (2 if subgrid else 0))
    t = ref.initial(points)
    before = solver.state().clone()
    for r in range(2):
        span = dt if r == 0 else 3 * dt                              # (the second round spans one call of three steps)
        tr.predict(span)
        if r == 0:
            solver.iterate(dt)
        else:
            solver.iterate_steps(3, dt)
        tr.correct(span)
        after = solver.state().clone()
        ua, ub = host(before), host(after)
        mid, end, _ = ref.host_round(part, kinds, ua, ub, span, t)
        assert_phase(tr, end, END, r)
        t, before = end, after
    moved = t["x"] != points
    assert np.count_nonzero(moved.any(axis=1)) > 1000


# ---- 7: adapt, rebind ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_adapt_then_rebind(dtype):
    mesh = "refined-2d-periodic"
    part, kinds = ref.partition(mesh, False), ref.kinds_of(mesh)
    points = ref.points_of(mesh, False)[0]
    solver = PlainSolver(part, dtype, mode="fused")
    tr = solver.tracers(points)
    dt = 0.05
    tr.predict(dt)
    solver.iterate(1e-3)
    tr.correct(dt)
    keep = {n: host(getattr(tr, n)) for n in ("x", "status", "k1")}
    new = amr.adapt(solver, threshold=-1.0, min_level=2, max_level=5)[0]         # (every criterion is >= 0: all refine)
    assert new.part.N != part.N
    assert tr.rebind(new) is tr and tr.solver is new
    for n, a in keep.items():
        assert ref.bits_equal(host(getattr(tr, n)), a), n
    assert (host(tr.hint_x) == -1).all() and (host(tr.hint_xs) == -1).all()
    u = host(new.state())
    t = {"x": keep["x"], "status": keep["status"], "xs": host(tr.xs), "k1": keep["k1"], "flag": host(tr.flag)}
    mid, end, _ = ref.host_round(new.part, kinds, u, u, dt, t)
    tr.predict(dt)
    assert_phase(tr, mid, ("xs", "k1", "flag", "status"), "predict on the new mesh")
    tr.correct(dt)
    assert_phase(tr, end, END, "correct on the new mesh")
    # another dimension, other sides: refused, and the object stays with its solver
    with pytest.raises(ValueError):
        tr.rebind(case("refined-2d-walls", False, dtype)[0])
    with pytest.raises(ValueError):
        tr.rebind(case("refined-3d-periodic", False, dtype)[0])
    assert tr.solver is new


# ---- 8: no allocation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
def test_calls_do_not_allocate(subgrid):
    solver, points = case("refined-3d-periodic", subgrid, torch.float32)
    tr = solver.tracers(points)
    tr.predict(0.1)
    tr.correct(0.1)
    torch.cuda.synchronize()
    gc.collect()                                                    # (tensors of earlier tests that only a cycle still holds)
    before = torch.cuda.memory_allocated()
    for _ in range(5):
        tr.predict(0.1)
        tr.correct(0.1)
        k, held = tr.velocity("x")
        tr.predict(0.1, k=k, held=held)
        k, held = tr.velocity("xs")
        tr.correct(0.1, k=k, held=held)
    assert torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before


# ---- 9: no particle, one particle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
def test_empty_and_single(subgrid):
    mesh, dtype = "refined-2d-walls", torch.float64
    solver, points = case(mesh, subgrid, dtype)
    none = solver.tracers(np.zeros((0, 2)))
    none.predict(0.1)
    none.correct(0.1)
    k, held = none.velocity("x")
    assert tuple(k.shape) == (0, 2) and tuple(held.shape) == (0,) and none.counts() == (0, 0, 0)
    assert none.host()["x"].shape == (0, 2)
    want = ref.reference(mesh, subgrid, NP[dtype])[0]
    i = 7
    one = solver.tracers(torch.from_numpy(points[i:i + 1].copy()).cuda())                # a device tensor of points
    one.predict(ref.DT[mesh])
    solver.begin_step()
    one.correct(ref.DT[mesh])
    solver.begin_step()
    assert ref.bits_equal(host(one.x), want[1]["x"][i:i + 1]) and ref.bits_equal(host(one.k1), want[0]["k1"][i:i + 1])


# ---- the examples ---------------------------------------------------------------------------------------------------------------------------
def test_riemann_example_carries_tracers_through_adapts(tmp_path):
    """--toy: levels 3-5, an adapt every 5 steps, t = 0.05. The three moving quadrants flow towards the centre at 1.206 per
    axis, so the lattice moves by up to 0.06 per axis, and whoever is outside has status 1 (here usually nobody)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "riemann2d_amr.py"), "--toy", "--tracers", "24", "--out",
                          str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    x, status = np.load(tmp_path / "riemann2d_tracers_x.npy"), np.load(tmp_path / "riemann2d_tracers_status.npy")
    assert x.shape == (576, 2) and status.shape == (576,) and status.dtype == np.uint8 and np.all(np.isfinite(x))
    inside = np.all((x >= 0.0) & (x < 1.0), axis=1)
    assert np.array_equal(inside, status != 1) and not (status == 2).any()
    assert np.count_nonzero(status == 0) > 288
    assert f"{np.count_nonzero(status == 1)} left through the open sides" in out.stdout
    moved = np.abs(x - tracers.lattice(2, 24)).max(axis=1)
    assert 0.02 < moved.max() < 0.1 and np.count_nonzero(moved > 0.02) > 100


# ---- 10: refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from _gpu import perturbed_state
    from t8gpu_amd.unstructured import PrismHexMesh
    solver, points = case("refined-2d-walls", False, torch.float64)
    with pytest.raises(ValueError):
        solver.tracers(np.zeros((4, 3)))
    with pytest.raises(ValueError):
        solver.tracers(np.zeros(4))
    tr = solver.tracers(points)
    keep = host(tr.x)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            tr.predict(bad)
        with pytest.raises(ValueError):
            tr.correct(bad)
    with pytest.raises(ValueError):
        tr.predict(0.1, k=tr.k)
    with pytest.raises(ValueError):
        tr.predict(0.1, k=tr.k[:5], held=tr.held[:5])
    with pytest.raises(ValueError):
        tr.velocity("k1")
    torch.cuda.synchronize()
    assert ref.bits_equal(host(tr.x), keep) and (host(tr.status) == 0).all()
    part = PrismHexMesh(5).partition()
    curved = PlainSolver(part, torch.float64, mode="compat", state=perturbed_state(part, 11))
    with pytest.raises(TypeError):
        curved.tracers(np.zeros((1, 3)))
    with pytest.raises(TypeError):
        tr.rebind(curved)
    assert tr.solver is solver
