"""-m gpu: the state monitor (t8gpu_hip_state_monitor_*, _Solver.monitor / cfl_timestep, SubgridSolver.compute_integral)
against numpy. The reference is computed in float64 from the very arrays uploaded (for fp32 from the float32 values); the
kernel's arithmetic is in double for both float types, so one tolerance serves both: 1e-12 (TOL1[float64]) on the scale
sum vol |term| for the sums and the value itself for maxima and minima -- a fixed tree over 4e5 terms costs about 20 eps and
the device log / sqrt / divide a few ulp per term, which leaves a margin of about 100. Slot 9 (min rho) selects an input
and must be exact; so must the counts."""
import ctypes as C

import numpy as np
import pytest
import torch

from _gpu import NP, perturbed_state
from t8gpu_amd import amr, hip
from t8gpu_amd.solver import Monitor, PlainSolver, SubgridSolver
from t8gpu_amd.synth import SynthMesh

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
TOL = 1e-12
SUMS, EXACT = (0, 1, 2, 3, 4, 5, 6), (9, 11, 12, 13, 14, 15)


def reference(u, volume, cpe, dim):
    """(block[16], scale[16]) of the slot table in float64 from the arrays as uploaded: u (5, n), volume per element"""
    u = np.asarray(u).astype(np.float64)
    n = u.shape[1]
    vol = np.repeat(np.asarray(volume).astype(np.float64)[: (n + cpe - 1) // cpe], cpe)[:n] / cpe
    rho, mx, my, mz, E = u
    with np.errstate(all="ignore"):
        fin = np.isfinite(u).all(axis=0)
        pos = fin & (rho > 0)
        m2 = mx * mx + my * my + mz * mz
        ke = 0.5 * m2 / rho
        p = 0.4 * (E - ke)
        phys = pos & (p > 0)
        s = np.sqrt(m2) / rho + np.sqrt(1.4 * p / rho)
        rate = s / vol ** (1.0 / dim)
        terms = [np.where(fin, vol * u[k], 0.0) for k in range(5)]
        terms.append(np.where(pos, vol * ke, 0.0))
        terms.append(np.where(phys, vol * rho * (np.log(p) - 1.4 * np.log(rho)), 0.0))
    block, scale = np.zeros(16), np.zeros(16)
    for k, t in enumerate(terms):
        block[k], scale[k] = t.sum(), np.abs(t).sum()
    block[7] = s[phys].max() if phys.any() else 0.0
    block[8] = rate[phys].max() if phys.any() else 0.0
    block[9] = rho[fin].min() if fin.any() else np.inf
    block[10] = p[pos].min() if pos.any() else np.inf
    block[11], block[12] = (~fin).sum(), (fin & ~phys).sum()
    scale[7:11] = np.abs(block[7:11])
    return block, scale


def check_block(got, want, scale, what=""):
    got = np.asarray(got, np.float64)
    assert got.shape == (16,)
    worst = 0.0
    for k in range(16):
        if k in EXACT or not np.isfinite(want[k]):
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            err = abs(got[k] - want[k])
            worst = max(worst, err / scale[k] if scale[k] > 0 else (0.0 if err == 0 else np.inf))
            assert err <= TOL * scale[k], (what, k, got[k], want[k], err / max(scale[k], 1e-300))
    print(f"{what}: worst error / scale = {worst:.2e}")


def random_state(rng, n, npdt):
    """physical states at moderate Mach numbers (perturbed_state style), in the dtype that is uploaded"""
    rho = rng.uniform(0.5, 2.0, n)
    v = 0.5 * rng.standard_normal((3, n))
    p = rng.uniform(0.5, 2.0, n)
    E = p / 0.4 + 0.5 * rho * (v ** 2).sum(0)
    return np.stack([rho, rho * v[0], rho * v[1], rho * v[2], E]).astype(npdt)


_WS = {}


def workspace():
    if "ws" not in _WS:
        f = hip.lib().t8gpu_hip_state_monitor_workspace_bytes
        f.restype = C.c_size_t
        _WS["ws"] = torch.zeros(f() // 8, dtype=torch.float64, device="cuda")
    return _WS["ws"]


def upload(u, layout):
    """the five planes on the device and their T8gpuVars. "planes": one allocation each (16-byte aligned: the wide loads with
    their tail); "rows": rows of one (5, n) tensor as in the solvers (aligned only when the row length allows); "shifted":
    every plane one value past an aligned address (always the one-value-per-lane path)."""
    dtype = torch.from_numpy(u[:, :0]).dtype
    n = u.shape[1]
    if layout == "planes":
        keep = [torch.from_numpy(np.ascontiguousarray(u[k])).cuda() for k in range(5)]
        planes = keep
    elif layout == "rows":
        keep = torch.from_numpy(np.ascontiguousarray(u)).cuda()
        planes = [keep[k] for k in range(5)]
    else:
        pitch = (n + 1 + 3) // 4 * 4
        keep = torch.zeros((5, pitch), dtype=dtype, device="cuda")
        keep[:, 1:n + 1] = torch.from_numpy(np.ascontiguousarray(u)).cuda()
        planes = [keep[k, 1:n + 1] for k in range(5)]
    v = (hip.Vars32 if dtype == torch.float32 else hip.Vars64)()
    for k in range(5):
        v.p[k] = planes[k].data_ptr()
    return keep, v


def run_kernel(u, volume, cpe, dim, layout, result=None):
    dtype = torch.float32 if u.dtype == np.float32 else torch.float64
    keep, v = upload(u, layout)
    dv = torch.from_numpy(np.ascontiguousarray(volume)).cuda()
    res = torch.full((16,), -7.0, dtype=torch.float64, device="cuda") if result is None else result
    hip.call("t8gpu_hip_state_monitor", dtype, C.c_size_t(u.shape[1]), cpe, dim, v, hip.ptr(dv), hip.ptr(workspace()), hip.ptr(res),
             hip.stream_ptr())
    out = res.cpu().numpy().copy()
    del keep
    return out


ELEMENTS = [0, 1, 3, 4, 5, 63, 64, 65, 257, 6251]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("cpe", [1, 16, 64])
@pytest.mark.parametrize("elements", ELEMENTS)
def test_kernel_matches_numpy(elements, cpe, dim, dtype):
    """sub-wavefront, wavefront edge, workgroup edge, the tail behind the last 16-byte vector, and (400 064 cells on the
    one-value-per-lane path) more workgroups' worth of cells than the grid cap"""
    rng = np.random.default_rng(1000 * elements + 10 * cpe + dim)
    n = elements * cpe
    u = random_state(rng, n, NP[dtype])
    volume = rng.uniform(0.1, 1.0, max(elements, 1)).astype(NP[dtype])
    want, scale = reference(u, volume, cpe, dim)
    for layout in ("planes", "rows", "shifted"):
        check_block(run_kernel(u, volume, cpe, dim, layout), want, scale, f"{layout} n={n} cpe={cpe} dim={dim}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_grid_cap_on_the_wide_path(dtype):
    """1 100 003 cells: more 16-byte vectors than 1024 workgroups take in one trip, for both float types, and a tail"""
    rng = np.random.default_rng(5)
    n = 1100003
    u = random_state(rng, n, NP[dtype])
    volume = rng.uniform(0.1, 1.0, n).astype(NP[dtype])
    want, scale = reference(u, volume, 1, 3)
    check_block(run_kernel(u, volume, 1, 3, "planes"), want, scale, f"planes n={n}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["planes", "shifted"])
def test_same_bits_twice(dtype, layout):
    rng = np.random.default_rng(8)
    n = 6251 * 16
    u = random_state(rng, n, NP[dtype])
    volume = rng.uniform(0.1, 1.0, 6251).astype(NP[dtype])
    a = run_kernel(u, volume, 16, 3, layout)
    b = run_kernel(u, volume, 16, 3, layout)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert np.isfinite(a).all() and a[0] > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("places", [(10, 11, 12, 13), (5, 64 + 17, 128 + 40, 256)], ids=["one wavefront", "four wavefronts and the last cell"])
def test_cell_classes(dtype, places):
    """one NaN density, one +inf energy (non-finite); one rho < 0, one rho > 0 with p < 0 (finite, non-physical)"""
    rng = np.random.default_rng(9)
    n = 257
    u = random_state(rng, n, NP[dtype])
    volume = rng.uniform(0.1, 1.0, n).astype(NP[dtype])
    i_nan, i_inf, i_neg, i_cold = places
    u[0, i_nan] = np.nan
    u[4, i_inf] = np.inf
    u[0, i_neg] = -0.3
    ke = 0.5 * float((u[1:4, i_cold].astype(np.float64) ** 2).sum()) / float(u[0, i_cold])
    u[4, i_cold] = 0.1 * ke
    p_cold = 0.4 * (float(u[4, i_cold]) - ke)
    assert u[0, i_cold] > 0 and p_cold < 0
    want, scale = reference(u, volume, 1, 2)
    assert want[11] == 2 and want[12] == 2
    for layout in ("planes", "shifted"):
        got = run_kernel(u, volume, 1, 2, layout)
        check_block(got, want, scale, f"{layout} classes")
        m = Monitor(got)
        assert (m.nonfinite, m.unphysical) == (2, 2)
        assert m.min_density == float(u[0, i_neg]) == NP[dtype](-0.3)
        assert abs(m.min_pressure - p_cold) <= TOL * abs(p_cold)
        assert np.isfinite(got).all()


def test_only_owned_cells_are_read():
    mesh = SynthMesh(2, 3, 5, band=0.1)
    part = mesh.partition(0, 2)
    assert part.G > 0
    g = PlainSolver(part, torch.float64, capacity=part.N + part.G + 1000, state=perturbed_state(part, 3))
    before = g.monitor()
    g.planes[:25, part.N:] = float("nan")              # ghost slots and the slack of every state plane
    after = g.monitor()
    assert after.nonfinite == 0 and after.unphysical == 0
    assert np.array_equal(after.block.view(np.int64), before.block.view(np.int64))
    u = g.state().cpu().numpy()
    want, scale = reference(u, part.volumes[:part.N], 1, 2)
    check_block(after.block, want, scale, "owned cells")


def numpy_rate(u, cell_volume, dim):
    u = np.asarray(u, np.float64)
    p = 0.4 * (u[4] - 0.5 * (u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0])
    s = np.sqrt(u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0] + np.sqrt(1.4 * p / u[0])
    return float((s / cell_volume ** (1.0 / dim)).max())


@pytest.mark.parametrize("mesh_args", [dict(dim=2, base=3, lmax=5, band=0.1), dict(dim=3, base=2, lmax=3, band=0.2)], ids=["2d", "3d"])
def test_plain_solver(mesh_args):
    dim = mesh_args["dim"]
    mesh = SynthMesh(dim, mesh_args["base"], mesh_args["lmax"], band=mesh_args["band"])
    part = mesh.partition()
    st = perturbed_state(part, 21)
    g = PlainSolver(part, torch.float64, mode="fused", state=st)
    vol = np.asarray(part.volumes, np.float64)[:part.N]
    m0 = g.monitor()
    for k in range(5):                                  # the two reductions use different trees: not bitwise
        assert abs(m0.integrals[k] - g.compute_integral(k)) <= 1e-13 * float((vol * np.abs(st[k, :part.N])).sum())
    want, scale = reference(st[:, :part.N], vol, 1, dim)
    check_block(m0.block, want, scale, f"plain {dim}d")
    dt7 = g.cfl_timestep(0.7)
    want7 = 0.7 / numpy_rate(g.state().cpu().numpy(), vol, dim)
    assert abs(dt7 - want7) <= TOL * want7
    dt = g.cfl_timestep(0.35)
    for _ in range(5):
        g.iterate(dt)
    m1 = g.monitor()
    assert np.abs(m1.integrals - m0.integrals).max() < 1e-12 * np.abs(m0.integrals).max()    # periodic: conservative to rounding
    assert m1.entropy >= m0.entropy                     # KEPES
    assert m1.nonfinite == 0 and m1.unphysical == 0
    u = g.state()
    p = 0.4 * (u[4] - 0.5 * (u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0])
    assert m1.min_density == float(u[0].min())
    assert abs(m1.min_pressure - float(p.min())) <= TOL * float(p.min())
    assert abs(m1.kinetic_energy - float((0.5 * (u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0] * g.planes[25, :part.N]).sum())) <= 1e-12 * m1.kinetic_energy


def test_plain_solver_uniform_mesh_step_is_the_reference_rule():
    mesh = SynthMesh(2, 4, 4)
    g = PlainSolver(mesh.partition(), torch.float64, mode="fused", state=perturbed_state(mesh.partition(), 4))
    want = 0.7 * 0.5 ** 4 / g.monitor().max_speed
    assert abs(g.cfl_timestep(0.7) - want) <= TOL * want


def test_plain_solver_on_a_curved_mesh():
    from t8gpu_amd.unstructured import PrismHexMesh, shell_map
    part = PrismHexMesh((8, 8, 4), split="checker", mapping=shell_map).partition()
    st = perturbed_state(part, 5)
    g = PlainSolver(part, torch.float64, state=st)
    want, scale = reference(st[:, :part.N], np.asarray(part.volumes)[:part.N], 1, 3)
    check_block(g.monitor().block, want, scale, "curved prisms and hexahedra")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mesh_args", [dict(dim=2, base=2, lmax=3, band=0.2), dict(dim=3, base=1, lmax=2, band=0.3)], ids=["2d", "3d"])
def test_subgrid_solver(mesh_args, dtype):
    dim = mesh_args["dim"]
    mesh = SynthMesh(dim, mesh_args["base"], mesh_args["lmax"], band=mesh_args["band"])
    part = mesh.partition(subgrid=True)
    S = 4 ** dim
    st = perturbed_state(part, 31).astype(NP[dtype])
    volumes = np.asarray(part.volumes).astype(NP[dtype])[:part.N]
    g = SubgridSolver(part, dtype, mode="fused", state=st)
    assert g.owned_cells == part.N * S
    want, scale = reference(st[:, :part.N * S], volumes, S, dim)
    m = g.monitor()
    check_block(m.block, want, scale, f"subgrid {dim}d")
    for k in range(5):
        assert abs(g.compute_integral(k) - want[k]) <= TOL * scale[k]
    cell = np.repeat(volumes.astype(np.float64), S) / S
    want7 = 0.7 / numpy_rate(st[:, :part.N * S], cell, dim)
    assert abs(g.cfl_timestep(0.7) - want7) <= TOL * want7
    # a solver fresh from an adapt has run no stage: the face-based rule has nothing to reduce, this one needs nothing
    new = amr.adapt_subgrid(g, threshold=0.0, min_level=mesh_args["base"], max_level=mesh_args["lmax"] + 1)[0]
    assert new.N != g.N
    cell = np.repeat(new.volumes.double().cpu().numpy()[:new.N], S) / S
    want_new = 0.7 / numpy_rate(new.state().cpu().numpy(), cell, dim)
    assert abs(new.cfl_timestep(0.7) - want_new) <= TOL * want_new


def rank_solvers(mesh, world, st):
    out = []
    for r in range(world):
        part = mesh.partition(r, world)
        gidx = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global]).astype(np.int64)
        out.append(PlainSolver(part, torch.float64, state=st[:, gidx].copy()))
    return out


def test_ranks_combine_to_the_single_rank_monitor():
    mesh = SynthMesh(2, 3, 5, band=0.1)
    whole = mesh.partition()
    st = perturbed_state(whole, 21)
    single = PlainSolver(whole, torch.float64, state=st).monitor()
    want, scale = reference(st[:, :whole.N], np.asarray(whole.volumes)[:whole.N], 1, 2)
    blocks = [s.monitor() for s in rank_solvers(mesh, 3, st)]
    both = Monitor.combine(blocks)
    for k in Monitor.MAX_SLOTS + Monitor.MIN_SLOTS + (11, 12):
        assert both.block[k] == single.block[k], k
    check_block(both.block, want, scale, "three ranks")
    assert np.all(np.abs(both.block[:7] - single.block[:7]) <= TOL * scale[:7])


def test_rank_that_owns_nothing():
    mesh = SynthMesh(2, 1, 1)
    whole = mesh.partition()
    st = perturbed_state(whole, 2)
    solvers = rank_solvers(mesh, 6, st)
    empties = [s for s in solvers if s.N == 0]
    assert len(empties) == 2
    want_empty = np.zeros(16)
    want_empty[9:11] = np.inf
    for s in empties:
        assert np.array_equal(s.monitor().block, want_empty)
        assert s.cfl_timestep() == float("inf")
    single = PlainSolver(whole, torch.float64, state=st).monitor()
    both = Monitor.combine([s.monitor() for s in solvers])
    want, scale = reference(st[:, :whole.N], np.asarray(whole.volumes)[:whole.N], 1, 2)
    check_block(both.block, want, scale, "six ranks, two empty")
    for k in Monitor.MAX_SLOTS + Monitor.MIN_SLOTS:
        assert both.block[k] == single.block[k], k


def test_dist_argument_on_a_one_rank_group(tmp_path):
    """the three all_reduce calls of monitor(dist=...) on a gloo group of one rank: the block comes back unchanged"""
    import datetime

    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/store", rank=0, world_size=1,
                            timeout=datetime.timedelta(seconds=30))
    try:
        mesh = SynthMesh(2, 3, 5, band=0.1)
        g = PlainSolver(mesh.partition(), torch.float64, state=perturbed_state(mesh.partition(), 21))
        alone = g.monitor()
        assert np.array_equal(g.monitor(dist=dist).block, alone.block)
        assert g.cfl_timestep(0.7, dist=dist) == 0.7 / alone.max_rate
    finally:
        dist.destroy_process_group()


def test_cfl_timestep_refuses_a_broken_state():
    mesh = SynthMesh(2, 3, 5, band=0.1)
    part = mesh.partition()
    st = perturbed_state(part, 21)
    st[0, 17] = np.nan
    st[0, 40] = -1.0
    st[0, 41] = -2.0
    g = PlainSolver(part, torch.float64, state=st)
    with pytest.raises(hip.T8gpuHipError, match=r"1 non-finite and 2 non-physical"):
        g.cfl_timestep()
    dev = g.monitor_device()                            # the same pass without copy or sync: the solver's device block
    assert dev.is_cuda and tuple(dev.shape) == (16,) and dev.dtype == torch.float64
    assert (float(dev[11]), float(dev[12])) == (1.0, 2.0)
    assert g.monitor_device().data_ptr() == dev.data_ptr()       # made once, kept
