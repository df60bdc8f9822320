"""-m gpu: open boundaries (outflow, prescribed-state inflow) on Subgrid<4,4> / Subgrid<4,4,4> meshes, compat and fused
tiers, against a CPU reference composed from the oracle's existing entry points: its inner-block loop, its wall loop on arrays
that hold only the wall faces, its xyz face flux for every subcell on an open face (outside state = inside state, or the inflow
state; no mirror) times area / sub-faces, its outer-face loop and its RK stage."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _oracle as O
from _gpu import NP, TOL1, TOL10, perturbed_state, rel_err
from test_subgrid_open_boundaries_host import boundary_flux_by_enumeration
from t8gpu_amd import amr, hip
from t8gpu_amd.solver import SubgridSolver
from t8gpu_amd.synth import SynthMesh

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS = [hip.KEPES, hip.HLL, hip.HLLC]
SIDES = {2: (0, "outflow", "periodic", "periodic"),                                  # x: inflow / outflow, y periodic
         3: (0, "outflow", "periodic", "periodic", "wall", "wall")}                  # ... z walls


def inflow_states(dim):
    rho, v, p = 1.2, (0.4, 0.1, 0.05 if dim == 3 else 0.0), 1.1
    return np.array([[rho, rho * v[0], rho * v[1], rho * v[2], p / 0.4 + 0.5 * rho * sum(c * c for c in v)]])


def mesh_of(dim, sides=None):
    """AMR meshes with hanging faces, families in the interior and open-face blocks on both x sides"""
    sides = SIDES[dim] if sides is None else sides
    return SynthMesh(2, 3, 5, band=0.05, sides=sides) if dim == 2 else SynthMesh(3, 3, 4, band=0.05, sides=sides)


def dt_of(mesh):
    return 0.1 * 2.0 ** -(mesh.finest_level + 2)


class SubgridOpenCase(O.SubgridCase):
    """O.SubgridCase with open boundary faces: per stage the oracle's inner loop, its wall loop on the wall faces alone, the
    open sub-faces from oracle_xyz_face_flux, its outer loop and its RK stage."""

    def __init__(self, part, dtype, state, inflow):
        super().__init__(part, dtype, state=state)
        kinds = np.asarray(part.boundary_kinds)
        F, rank = part.F, self.rank
        fn = np.asarray(part.face_neighbors)
        wall = kinds == 0
        nr = np.asarray(part.normals).reshape(-1, rank)
        self.Bw = int(wall.sum())
        self.fn_w = np.ascontiguousarray(np.concatenate([fn[:2 * F], fn[2 * F:][wall]]).astype(np.int32))
        self.normals_w = np.ascontiguousarray(np.concatenate([nr[:F], nr[F:][wall]]).reshape(-1).astype(dtype))
        self.areas_w = np.ascontiguousarray(np.concatenate([part.areas[:F], part.areas[F:][wall]]).astype(dtype))
        self.open_faces = np.flatnonzero(~wall)
        self.kinds = kinds
        self.inflow = None if inflow is None else np.asarray(inflow, np.float64).astype(dtype)

    def _outside(self, b, sL):
        k = int(self.kinds[b])
        return sL.copy() if k == 1 else np.repeat(self.inflow[k - 2][None, :], sL.shape[0], 0)

    def iterate(self, dt, kind=0, omp=False):
        self.prev, self.next = self.next, self.prev
        P, T, rank = self.part, self.dtype, self.rank
        sf = O.suf(T)
        lib = O.lib()
        ncell = P.N * self.S
        src, dst = (self.prev, 1, 2), (1, 2, self.next)
        for s in range(3):
            st = self.planes[5 * src[s]:5 * src[s] + 5]
            fl = self.planes[20:25]
            fl[:] = 0
            getattr(lib, "oracle_subgrid_inner_" + sf)(kind, rank, P.N, O.p(st), O.p(fl), C.c_size_t(self.stride), O.p(self.volumes))
            if self.Bw:
                getattr(lib, "oracle_subgrid_boundary_" + sf)(kind, rank, P.F, self.Bw, O.p(self.fn_w), O.p(self.normals_w),
                                                               O.p(self.areas_w), O.p(st), O.p(fl), C.c_size_t(self.stride))
            if self.open_faces.size:
                fl[:, :ncell] += boundary_flux_by_enumeration(P, T, kind, np.ascontiguousarray(st[:, :ncell]), self.open_faces,
                                                              self._outside)
            getattr(lib, "oracle_subgrid_outer_" + sf)(kind, rank, P.F, O.p(self.fn), O.p(P.indices), O.p(P.level_diff),
                                                        O.p(P.nb_offset), O.p(self.normals), O.p(self.areas), O.p(st), O.p(fl),
                                                        C.c_size_t(self.stride))
            pv, md, ot = (self.planes[5 * x:5 * x + 5] for x in (self.prev, src[s], dst[s]))
            getattr(lib, "oracle_subgrid_rk_stage_" + sf)(s + 1, rank, P.N, O.p(pv), O.p(md), O.p(ot), O.p(fl),
                                                           C.c_size_t(self.stride), O.p(self.volumes), O.fs(T, dt))


def _solver(part, dtype, kind, mode, state, inflow):
    return SubgridSolver(part, dtype, flux_kind=kind, mode=mode, state=state, open_boundaries=True, inflow_states=inflow)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("mode", ["compat", "fused"])
def test_subgrid_open_boundaries_follow_the_oracle_composed_reference(dim, kind, dtype, mode):
    mesh = mesh_of(dim)
    part = mesh.partition(subgrid=True)
    st, inflow = perturbed_state(part, 21), inflow_states(dim)
    g = _solver(part, dtype, kind, mode, st, inflow)
    if mode == "fused":
        assert g.plan.c.has_open_faces and g.plan.host.n_families > 0
    o = SubgridOpenCase(part, NP[dtype], st, inflow)
    dt = dt_of(mesh)
    g.iterate(dt)
    o.iterate(dt, kind)
    torch.cuda.synchronize()
    assert rel_err(g.state().cpu().numpy(), o.current()[:, :g.owned_cells]) < TOL1[dtype]
    for _ in range(9):
        g.iterate(dt)
        o.iterate(dt, kind)
    torch.cuda.synchronize()
    assert rel_err(g.state().cpu().numpy(), o.current()[:, :g.owned_cells]) < TOL10[dtype]


_SWITCH_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from test_gpu_subgrid_open_boundaries import mesh_of, inflow_states, dt_of
from _gpu import perturbed_state
from t8gpu_amd import hip
from t8gpu_amd.solver import SubgridSolver
out = []
for dim in (2, 3):
    mesh = mesh_of(dim)
    part = mesh.partition(subgrid=True)
    for dtype in (torch.float32, torch.float64):
        for kind in (hip.KEPES, hip.HLL, hip.HLLC):
            g = SubgridSolver(part, dtype, flux_kind=kind, mode="fused", state=perturbed_state(part, 22), open_boundaries=True,
                              inflow_states=inflow_states(dim))
            assert g.plan.host.n_families > 0 and g.plan.c.has_open_faces
            for _ in range(3):
                g.iterate(dt_of(mesh))
            torch.cuda.synchronize()
            out.append(g.state().double().cpu().numpy().ravel())
np.save(sys.argv[1], np.concatenate(out))
"""


def test_family_and_addressing_switches_give_the_same_bits(tmp_path):
    """T8GPU_SG_FAMILY=0 (every block through the block kernel) and T8GPU_SG_WIDE=1 (64-bit plane addressing) against the
    default, in child processes (the switches are read once per process)."""
    script = tmp_path / "child.py"
    script.write_text(_SWITCH_CHILD.format(root=ROOT, tests=HERE))
    res = []
    for tag, env in (("default", {}), ("block", dict(T8GPU_SG_FAMILY="0")), ("wide", dict(T8GPU_SG_WIDE="1"))):
        out = tmp_path / f"state_{tag}.npy"
        subprocess.run([sys.executable, str(script), str(out)], env=dict(os.environ, **env), check=True, timeout=600)
        res.append(np.load(out))
    assert np.isfinite(res[0]).all()
    for other in res[1:]:
        assert np.array_equal(res[0], other), int((res[0] != other).sum())


def _uniform(part, w):
    S = 4 ** part.mesh.dim
    return np.repeat(np.asarray(w, np.float64).reshape(5, 1), (part.N + part.G) * S, axis=1)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("mode", ["compat", "fused"])
def test_inflow_of_the_cell_state_equals_outflow_bitwise(dim, kind, dtype, mode):
    """From a uniform state, an inflow face whose state is that state gives the bits of an outflow face: the kernels convert
    the prescribed state with the routine they run for every far cell. Compat tier: the same up to the order of its atomic
    sums. (One RK stage: after it the cells next to a boundary
    differ from the uniform state in the last bits -- a sub-face area is face_surfaces / sub-faces, an inner face's the
    block edge squared --, and from then on the two runs see different outside states.)"""
    w = inflow_states(dim)
    rest = SIDES[dim][2:]
    a_part = mesh_of(dim, (0, "outflow") + rest).partition(subgrid=True)
    b_part = mesh_of(dim, ("outflow", "outflow") + rest).partition(subgrid=True)
    a = _solver(a_part, dtype, kind, mode, _uniform(a_part, w[0]), w)
    b = _solver(b_part, dtype, kind, mode, _uniform(b_part, w[0]), None)
    dt = dt_of(a_part.mesh)
    for g in (a, b):
        g.begin_step()
        g.run_stage(0, dt)
    torch.cuda.synchronize()
    step1 = a.stage_steps(0)[1]
    sa, sb = a.step_planes(step1)[:, :a.owned_cells], b.step_planes(step1)[:, :b.owned_cells]
    if mode == "fused":
        assert torch.equal(sa, sb)
    else:
        assert rel_err(sa.cpu().numpy(), sb.cpu().numpy()) < TOL1[dtype]


@pytest.mark.parametrize("dim", [2, 3])
def test_native_driver_equals_python_stages(dim):
    part = mesh_of(dim).partition(subgrid=True)
    st, inflow = perturbed_state(part, 23), inflow_states(dim)
    py, nat = (_solver(part, torch.float64, hip.KEPES, "fused", st, inflow) for _ in range(2))
    nat.use_native_stepper()
    dt = dt_of(part.mesh)
    for n in (3, 2):
        for _ in range(n):
            py.iterate(dt)
        nat.iterate_steps(n, dt)
    torch.cuda.synchronize()
    assert torch.equal(py.state(), nat.state())


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("mode", ["fused", "compat"])
def test_three_way_loopback_partition_equals_single_rank(dim, mode):
    """All three ranks on one GPU, the exchange a loopback copy of whole ghost blocks (test_gpu_halo.py). Boundary faces never
    touch ghosts: bitwise the one-rank run in the fused tier."""
    from t8gpu_amd.halo import HaloExchange
    from test_gpu_halo import loopback
    mesh = mesh_of(dim)
    whole = mesh.partition(subgrid=True)
    S = 4 ** dim
    st, inflow = perturbed_state(whole, 24), inflow_states(dim)
    dtype = torch.float64
    ref = _solver(whole, dtype, hip.KEPES, mode, st, inflow)
    solvers, halos = [], []
    for r in range(3):
        part = mesh.partition(r, 3, subgrid=True)
        blocks = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
        cells = (blocks[:, None] * S + np.arange(S)[None, :]).reshape(-1)
        local = st[:, cells].copy()
        local[:, part.N * S:] = np.nan
        solvers.append(_solver(part, dtype, hip.KEPES, mode, local, inflow))
        halos.append(HaloExchange(part, dtype, dist=None, overlap=False))
    if mode == "fused":
        assert all(0 < s.plan.host.n_interior < s.N for s in solvers)
        assert sum(int(s.plan.c.has_open_faces) for s in solvers) >= 2
    dt = dt_of(mesh)
    for _ in range(2):
        ref.iterate(dt)
        for s in solvers:
            s.begin_step()
        for k in range(3):
            for s, h in zip(solvers, halos):
                h._pack(s.step_planes(s.stage_steps(k)[0]))
            loopback(halos)
            for s, h in zip(solvers, halos):
                h._unpack(s.step_planes(s.stage_steps(k)[0]))
            torch.cuda.synchronize()
            for s in solvers:
                s.run_stage(k, dt, split=True)
            torch.cuda.synchronize()
    full = torch.cat([s.state() for s in solvers], dim=1).cpu().numpy()
    assert not np.isnan(full).any()
    assert rel_err(full, ref.state().cpu().numpy()) < 1e-13
    if mode == "fused":
        assert np.array_equal(full, ref.state().cpu().numpy())      # (compat: atomics, the order of the sums varies)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("mode", ["compat", "fused"])
def test_free_stream_stays_uniform(dim, mode):
    """A uniform moving state with inflow = that state on -x and outflow elsewhere stays uniform for 50 fp64 steps."""
    sides = (0,) + ("outflow",) * (2 * dim - 1)
    mesh = mesh_of(dim, sides)
    part = mesh.partition(subgrid=True)
    w = inflow_states(dim)
    g = _solver(part, torch.float64, hip.KEPES, mode, _uniform(part, w[0]), w)
    dt = 2 * dt_of(mesh)
    for _ in range(50):
        g.iterate(dt)
    torch.cuda.synchronize()
    got = g.state().cpu().numpy()
    err = float((np.abs(got - w[0][:, None]) / np.abs(w[0]).max()).max())
    print(f"free stream {dim}D {mode}: relative drift after 50 steps {err:.2e}")
    assert err < 1e-12, err


def test_sod_tube_lets_the_shock_out():
    """2D Subgrid<4,4> Sod tube, x outflow, y periodic, 128 subcells across (uniform level 5): at t = 0.4 the shock (speed
    1.75) has left through x = 1 and the post-shock state fills the right end; a wall there would have reflected it."""
    from test_gpu_open_boundaries import sod_exact
    mesh = SynthMesh(2, 5, 5, sides=("outflow", "outflow", "periodic", "periodic"))
    part = mesh.partition(subgrid=True)
    S = 16
    h = 1.0 / 128
    blk = np.asarray(part.centres)[:, 0] - 2 * h                       # x of the blocks' low edges
    x = (blk[:part.N, None] + (np.arange(S)[None, :] % 4 + 0.5) * h).reshape(-1)
    left = x < 0.5
    rho = np.where(left, 1.0, 0.125)
    p = np.where(left, 1.0, 0.1)
    st = np.stack([rho, 0 * rho, 0 * rho, 0 * rho, p / 0.4])
    g = SubgridSolver(part, torch.float64, mode="fused", state=st, open_boundaries=True)
    t, dt = 0.0, 0.2 * h
    while t < 0.4 - 1e-12:
        step = min(dt, 0.4 - t)
        g.iterate(step)
        t += step
    torch.cuda.synchronize()
    u = g.state().cpu().numpy()
    rho_g = u[0]
    p_g = 0.4 * (u[4] - 0.5 * (u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0])
    end = (x > 0.90) & (x < 0.98)
    r_end, p_end = rho_g[end].mean(), p_g[end].mean()
    print(f"subgrid sod: mean rho {r_end:.4f} (exact 0.2656), mean p {p_end:.4f} (exact 0.3031) over x in [0.90, 0.98]")
    assert abs(r_end - 0.2656) < 0.08 * 0.2656 and abs(p_end - 0.3031) < 0.03 * 0.3031
    inner = x < 0.85
    rho_x, _, _ = sod_exact(x[inner], 0.4)
    l1 = float(np.abs(rho_g[inner] - rho_x).mean() * 0.85)
    print(f"subgrid sod: L1(rho) over [0, 0.85] = {l1:.4f}")
    assert l1 < 0.03


def test_adapt_keeps_the_open_boundaries_and_follows_the_reference():
    """iterate / adapt_subgrid / iterate on the device against the same sequence on the host (oracle-composed reference, the
    oracle's indicator and block transfer): the kinds, the inflow states and the open kernels survive adapt."""
    dim = 2
    mesh = SynthMesh(2, 3, 5, band=0.05, sides=SIDES[2])
    part = mesh.partition(subgrid=True)
    S = 16
    inflow = inflow_states(dim)
    st = perturbed_state(part, 25)
    g = _solver(part, torch.float64, hip.KEPES, "fused", st, inflow)
    o = SubgridOpenCase(part, np.float64, st, inflow)
    for cycle in range(2):
        dt = dt_of(g.part.mesh)
        for _ in range(3):
            g.iterate(dt)
            o.iterate(dt)
        torch.cuda.synchronize()
        assert rel_err(g.state().cpu().numpy(), o.current()[:, :g.owned_cells]) < TOL10[torch.float64]
        g, marks, _ = amr.adapt_subgrid(g, threshold=0.02, min_level=3, max_level=5)
        assert g.open_boundaries and np.array_equal(g.inflow_states, inflow) and g.plan.c.has_open_faces
        opart = o.part
        rho = np.ascontiguousarray(o.current()[0, :opart.N * S])
        crit = np.zeros(opart.N)
        O.lib().oracle_subgrid_refinement_criteria_f64(dim, opart.N, O.p(rho), O.p(o.volumes), O.p(crit))
        omarks = opart.mesh.marks_from_criteria(crit, 0.02, 3, 5)
        assert np.array_equal(omarks, marks)
        nmesh, oad = opart.mesh.adapt(omarks)
        npart = nmesh.partition(subgrid=True)
        cur = np.ascontiguousarray(o.current()[:, :opart.N * S])
        nst = np.zeros((5, npart.N * S))
        nvol = np.zeros(npart.N)
        O.lib().oracle_subgrid_adapt_variables_and_volume_f64(dim, npart.N, O.p(oad), O.p(cur), C.c_size_t(opart.N * S), O.p(nst),
                                                              C.c_size_t(npart.N * S), O.p(np.ascontiguousarray(o.volumes)), O.p(nvol))
        nxt, prv = o.next, o.prev
        o = SubgridOpenCase(npart, np.float64, np.zeros((5, npart.N * S)), inflow)
        o.next, o.prev = nxt, prv
        o.planes[5 * o.next:5 * o.next + 5, :npart.N * S] = nst
        o.volumes = nvol
        assert g.N == npart.N
        assert rel_err(g.state().cpu().numpy(), o.current()[:, :g.owned_cells]) < TOL10[torch.float64]
    dt = dt_of(g.part.mesh)
    for _ in range(3):
        g.iterate(dt)
        o.iterate(dt)
    torch.cuda.synchronize()
    assert rel_err(g.state().cpu().numpy(), o.current()[:, :g.owned_cells]) < TOL10[torch.float64]


def test_open_boundaries_are_opt_in_and_validated():
    part = SynthMesh(2, 2, 3, sides=(0, "outflow", "periodic", "periodic")).partition(subgrid=True)
    with pytest.raises(ValueError, match="walls only"):
        SubgridSolver(part, torch.float32)
    with pytest.raises(ValueError, match="required"):
        SubgridSolver(part, torch.float32, open_boundaries=True)
    with pytest.raises(ValueError):
        SubgridSolver(part, torch.float32, open_boundaries=True, inflow_states=np.array([[1.0, 0, 0, 0, -1.0]]))
    # a partition without open faces (walls, or periodic) takes open_boundaries=True: the wall-only kernels run
    for p in (SynthMesh(2, 2, 3, periodic=False).partition(subgrid=True), SynthMesh(2, 2, 3).partition(subgrid=True)):
        for mode in ("compat", "fused"):
            a = SubgridSolver(p, torch.float64, mode=mode, state=perturbed_state(p, 26), open_boundaries=True,
                              inflow_states=inflow_states(2))
            b = SubgridSolver(p, torch.float64, mode=mode, state=perturbed_state(p, 26))
            if mode == "fused":
                assert not a.plan.c.has_open_faces
            for _ in range(2):
                a.iterate(1e-3)
                b.iterate(1e-3)
            torch.cuda.synchronize()
            assert torch.equal(a.state(), b.state())
