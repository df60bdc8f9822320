"""-m gpu: far-field boundaries (the characteristic condition, kinds 10 + k) on Subgrid<4,4> / Subgrid<4,4,4> meshes, compat and
fused tiers, against the oracle-composed reference of test_gpu_subgrid_open_boundaries.SubgridOpenCase with the outside state
of every far-field sub-face from the numpy restatement of the condition (tests/_farfield.py, fp64, cast to the dtype); bitwise
identities with outflow and inflow sides, the family and addressing switches, the native driver and partitions; free stream;
adapt; the opt-in."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _oracle as O
from _farfield import BRANCHES, farfield_outside
from _gpu import NP, TOL1, TOL10, rel_err
from test_gpu_farfield import cons, far_states
from test_gpu_subgrid_open_boundaries import SubgridOpenCase, dt_of, mesh_of
from t8gpu_amd import amr, hip
from t8gpu_amd.solver import FLUXES, SubgridSolver
from t8gpu_amd.synth import SynthMesh

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS = [hip.KEPES, hip.HLL, hip.HLLC]
SIDES = {2: (("farfield", 0), ("farfield", 1), "periodic", "periodic"),
         3: (("farfield", 0), ("farfield", 1), "periodic", "periodic", "wall", ("farfield", 0))}
FREE_STREAM_BOUND = 1e-12   # the open-boundary bound of DESIGN.md §4


def subcell_centres(part):
    """[(N + G) * S, 3] centres of the subcells: the block centre plus (i + 0.5 - 2) * edge / 4 per axis, edge = volume ** (1 /
    dim); subcell (i, j, k) of block e at e * S + i + 4 j + 16 k"""
    dim = part.mesh.dim
    S = 4 ** dim
    c = np.asarray(part.centres, np.float64)
    c = np.concatenate([c, np.zeros((c.shape[0], 3 - c.shape[1]))], 1) if c.shape[1] < 3 else c
    edge = np.asarray(part.volumes, np.float64) ** (1.0 / dim)
    cell = np.arange(S)
    off = np.zeros((S, 3))
    for a in range(dim):
        off[:, a] = ((cell >> (2 * a)) & 3) + 0.5 - 2
    return (c[:, None, :] + off[None, :, :] * (edge[:, None, None] / 4)).reshape(-1, 3)


def subgrid_far_state(part, seed):
    """test_gpu_farfield.far_state on the subcell centres: x velocity 2.2 sin(2 pi y) against a sound speed of ~1.18 drives the
    +-x sub-faces through all four branches"""
    rng = np.random.default_rng(seed)
    x, y, z = subcell_centres(part).T
    n = x.size
    rho = 1.0 + 0.1 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) + 0.02 * rng.standard_normal(n)
    v = np.stack([2.2 * np.sin(2 * np.pi * y) + 0.1 * rng.standard_normal(n), 0.3 * np.cos(2 * np.pi * x) + 0.05 * rng.standard_normal(n),
                  (0.2 * np.sin(2 * np.pi * y) if part.mesh.dim == 3 else 0 * x) + 0.05 * rng.standard_normal(n)])
    p = 1.0 + 0.1 * rng.uniform(-1, 1, n)
    return cons(rho, v, p)


def subgrid_split_state(part, u_left, u_right):
    """test_gpu_farfield._split_state on subcells: x velocity u_left for x < 1/2 and u_right beyond, rho = p = 1"""
    x = subcell_centres(part)[:, 0]
    v = np.zeros((3, x.size))
    v[0] = np.where(x < 0.5, u_left, u_right)
    return cons(np.ones_like(x), v, np.ones_like(x))


class SubgridFarCase(SubgridOpenCase):
    """SubgridOpenCase whose open faces may be far-field faces: their sub-faces' outside states from farfield_outside in fp64
    with the block face's outward normal and row k - 10 of the states (`inflow`, as the device table holds them), cast to the dtype. `branches` counts sub-faces."""

    def __init__(self, part, dtype, state, inflow):
        super().__init__(part, dtype, state, inflow)
        self.branches = np.zeros(4, np.int64)
        self._n3 = np.zeros((part.B, 3))
        self._n3[:, :self.rank] = np.asarray(part.normals, np.float64).reshape(-1, self.rank)[part.F:]

    def _outside(self, b, sL):
        k = int(self.kinds[b])
        if k < 10:
            return super()._outside(b, sL)
        m = sL.shape[0]
        out, br = farfield_outside(sL, np.repeat(self._n3[b][None], m, 0), np.repeat(self.inflow[k - 10][None], m, 0))
        self.branches += np.bincount(br, minlength=4)
        return out.astype(sL.dtype)


def _solver(part, dtype, kind, mode, state, states, **kw):
    return SubgridSolver(part, dtype, flux_kind=kind, mode=mode, state=state, open_boundaries=True, farfield=True,
                         inflow_states=states, **kw)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("mode", ["compat", "fused"])
def test_subgrid_farfield_follows_the_reference(dim, kind, dtype, mode):
    mesh = mesh_of(dim, SIDES[dim])
    part = mesh.partition(subgrid=True)
    st, states = subgrid_far_state(part, 21), far_states()
    g = _solver(part, dtype, kind, mode, st, states)
    if mode == "fused":
        assert g.plan.c.has_open_faces and g.plan.c.has_farfield_faces and g.plan.host.n_families > 0
    o = SubgridFarCase(part, NP[dtype], st, states)
    dt = dt_of(mesh)
    g.iterate(dt)
    o.iterate(dt, kind)
    torch.cuda.synchronize()
    if mode == "fused":
        name = hip.lib().t8gpu_hip_last_stage_kernel
        name.restype = C.c_char_p
        assert name().startswith(b"k_subgrid_family") and name().endswith(b", 2>"), name()   # MODE 2: the far-field kernels
    e1 = rel_err(g.state().cpu().numpy(), o.current()[:, :g.owned_cells])
    print(f"subgrid far field {dim}D kind {kind} {dtype} {mode}: 1 step {e1:.2e}")
    assert e1 < TOL1[dtype]
    for _ in range(9):
        g.iterate(dt)
        o.iterate(dt, kind)
    torch.cuda.synchronize()
    e10 = rel_err(g.state().cpu().numpy(), o.current()[:, :g.owned_cells])
    print(f"subgrid far field {dim}D kind {kind} {dtype} {mode}: 10 steps {e10:.2e}, branches {o.branches.tolist()}")
    assert e10 < TOL10[dtype]
    assert (o.branches > 0).all(), dict(zip(BRANCHES, o.branches.tolist()))


def _boundary_fluxes(s):
    """the flux planes of the compat boundary kernel alone, from zeroed planes (one block face per boundary subcell and axis;
    a corner subcell of the 3D mesh takes two faces: the wall / far-field z sides are the same in both runs)"""
    s.planes[5 * FLUXES:5 * FLUXES + 5].zero_()
    name = "t8gpu_hip_subgrid_boundary_far" if s._far_kinds else "t8gpu_hip_subgrid_boundary_bc"
    hip.call(name, s.dtype, s.kind, s.rank, s.F, s.B, hip.ptr(s.fn), hip.ptr(s.kinds), hip.ptr(s.inflow_table), hip.ptr(s.normals),
             hip.ptr(s.areas), s.get_own_variables(s.next), s.get_own_variables(FLUXES), hip.stream_ptr())
    torch.cuda.synchronize()
    return s.planes[5 * FLUXES:5 * FLUXES + 5].clone()


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("mode", ["compat", "fused"])
def test_supersonic_outflow_and_inflow_give_the_outflow_and_inflow_bits(dim, kind, dtype, mode):
    """Every far-field sub-face supersonic outflow (the flow leaves through both x sides at Mach 2.5): the bits of outflow
    sides. Every one supersonic inflow: the bits of inflow sides with the same states. (x sides only: the other sides are
    periodic, or walls.)"""
    states = far_states()
    rest = ("periodic", "periodic") + (("wall", "wall") if dim == 3 else ())
    far = mesh_of(dim, (("farfield", 0), ("farfield", 1)) + rest).partition(subgrid=True)
    outflow = mesh_of(dim, ("outflow", "outflow") + rest).partition(subgrid=True)
    inflow = mesh_of(dim, (0, 1) + rest).partition(subgrid=True)
    dt = 0.5 * dt_of(far.mesh)
    for (ul, ur), other in (((-3.0, 3.0), outflow), ((3.0, -3.0), inflow)):
        a = _solver(far, dtype, kind, mode, subgrid_split_state(far, ul, ur), states)
        b = SubgridSolver(other, dtype, flux_kind=kind, mode=mode, state=subgrid_split_state(other, ul, ur), open_boundaries=True,
                          inflow_states=states)
        if mode == "compat":   # (the compat face kernels sum by atomics: compare the boundary kernel's planes of one launch)
            assert a._far_kinds and not b._far_kinds
            assert torch.equal(_boundary_fluxes(a), _boundary_fluxes(b)), (ul, ur)
            continue
        assert a.plan.c.has_farfield_faces and not b.plan.c.has_farfield_faces
        for _ in range(2):
            a.iterate(dt)
            b.iterate(dt)
        torch.cuda.synchronize()
        assert torch.isfinite(a.state()).all()
        assert torch.equal(a.state(), b.state()), (ul, ur)


_SWITCH_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from test_gpu_subgrid_farfield import SIDES, subgrid_far_state, mesh_of, dt_of, far_states
from t8gpu_amd import hip
from t8gpu_amd.solver import SubgridSolver
out = []
for dim in (2, 3):
    mesh = mesh_of(dim, SIDES[dim])
    part = mesh.partition(subgrid=True)
    for dtype in (torch.float32, torch.float64):
        for kind in (hip.KEPES, hip.HLL, hip.HLLC):
            g = SubgridSolver(part, dtype, flux_kind=kind, mode="fused", state=subgrid_far_state(part, 22), open_boundaries=True,
                              farfield=True, inflow_states=far_states())
            assert g.plan.host.n_families > 0 and g.plan.c.has_farfield_faces
            for _ in range(3):
                g.iterate(dt_of(mesh))
            torch.cuda.synchronize()
            out.append(g.state().double().cpu().numpy().ravel())
np.save(sys.argv[1], np.concatenate(out))
"""


def test_family_and_addressing_switches_give_the_same_bits(tmp_path):
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


@pytest.mark.parametrize("dim", [2, 3])
def test_native_driver_equals_python_stages(dim):
    part = mesh_of(dim, SIDES[dim]).partition(subgrid=True)
    st, states = subgrid_far_state(part, 23), far_states()
    py, nat = (_solver(part, torch.float64, hip.KEPES, "fused", st, states) for _ in range(2))
    nat.use_native_stepper()
    dt = dt_of(part.mesh)
    for n in (3, 2):
        for _ in range(n):
            py.iterate(dt)
        nat.iterate_steps(n, dt)
    torch.cuda.synchronize()
    assert torch.isfinite(py.state()).all()
    assert torch.equal(py.state(), nat.state())


@pytest.mark.parametrize("dim", [2, 3])
def test_three_way_loopback_partition_equals_single_rank(dim):
    """All three ranks on one GPU, the exchange a loopback copy of whole ghost blocks. Boundary faces never touch ghosts."""
    from t8gpu_amd.halo import HaloExchange
    from test_gpu_halo import loopback
    mesh = mesh_of(dim, SIDES[dim])
    whole = mesh.partition(subgrid=True)
    S = 4 ** dim
    st, states = subgrid_far_state(whole, 24), far_states()
    dtype = torch.float64
    ref = _solver(whole, dtype, hip.KEPES, "fused", st, states)
    solvers, halos = [], []
    for r in range(3):
        part = mesh.partition(r, 3, subgrid=True)
        blocks = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
        cells = (blocks[:, None] * S + np.arange(S)[None, :]).reshape(-1)
        local = st[:, cells].copy()
        local[:, part.N * S:] = np.nan
        solvers.append(_solver(part, dtype, hip.KEPES, "fused", local, states))
        halos.append(HaloExchange(part, dtype, dist=None, overlap=False))
    assert all(0 < s.plan.host.n_interior < s.N for s in solvers)
    assert sum(int(s.plan.c.has_farfield_faces) for s in solvers) >= 2
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
    assert np.array_equal(full, ref.state().cpu().numpy())


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("mode", ["compat", "fused"])
def test_free_stream_stays_uniform(dim, mode):
    """A uniform state equal to far-field state 0 (at rest) on every open side stays uniform for 50 fp64 steps."""
    mesh = mesh_of(dim, (("farfield", 0),) * (2 * dim))
    part = mesh.partition(subgrid=True)
    states = far_states()
    w = states[0]
    st = np.repeat(w.reshape(5, 1), (part.N + part.G) * 4 ** dim, axis=1)
    g = _solver(part, torch.float64, hip.KEPES, mode, st, states)
    dt = 2 * dt_of(mesh)
    for _ in range(50):
        g.iterate(dt)
    torch.cuda.synchronize()
    got = g.state().cpu().numpy()
    err = float((np.abs(got - w[:, None]) / np.abs(w).max()).max())
    print(f"subgrid far-field free stream {dim}D {mode}: relative drift after 50 steps {err:.2e}")
    assert err <= FREE_STREAM_BOUND, err


def test_adapt_keeps_farfield_and_follows_the_reference():
    dim, S = 2, 16
    mesh = SynthMesh(2, 3, 5, band=0.05, sides=SIDES[2])
    part = mesh.partition(subgrid=True)
    states = far_states()
    st = subgrid_far_state(part, 25)
    g = _solver(part, torch.float64, hip.KEPES, "fused", st, states)
    o = SubgridFarCase(part, np.float64, st, states)
    for cycle in range(2):
        dt = dt_of(g.part.mesh)
        for _ in range(3):
            g.iterate(dt)
            o.iterate(dt)
        torch.cuda.synchronize()
        assert rel_err(g.state().cpu().numpy(), o.current()[:, :g.owned_cells]) < TOL10[torch.float64]
        g, marks, _ = amr.adapt_subgrid(g, threshold=0.02, min_level=3, max_level=5)
        assert g.open_boundaries and g.farfield and np.array_equal(g.inflow_states, states)
        assert g.plan.c.has_open_faces and g.plan.c.has_farfield_faces
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
        o = SubgridFarCase(npart, np.float64, np.zeros((5, npart.N * S)), states)
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


def test_farfield_is_opt_in_and_validated():
    part = SynthMesh(2, 2, 3, sides=(("farfield", 0), ("farfield", 1), "periodic", "periodic")).partition(subgrid=True)
    for kw in (dict(), dict(open_boundaries=True, inflow_states=far_states())):
        with pytest.raises(ValueError, match="far-field"):
            SubgridSolver(part, torch.float32, **kw)
    with pytest.raises(ValueError, match="open_boundaries"):
        SubgridSolver(part, torch.float32, farfield=True, inflow_states=far_states())
    with pytest.raises(ValueError, match="required"):
        SubgridSolver(part, torch.float32, open_boundaries=True, farfield=True)
    with pytest.raises(ValueError):
        SubgridSolver(part, torch.float32, open_boundaries=True, farfield=True, inflow_states=far_states()[:1])
    # a partition without far-field faces takes farfield=True: the kernels of a plan without them run
    from _gpu import perturbed_state
    p = SynthMesh(2, 2, 3, sides=(0, "outflow", "periodic", "periodic")).partition(subgrid=True)
    for mode in ("compat", "fused"):
        a = SubgridSolver(p, torch.float64, mode=mode, state=perturbed_state(p, 26), open_boundaries=True, farfield=True,
                          inflow_states=far_states())
        b = SubgridSolver(p, torch.float64, mode=mode, state=perturbed_state(p, 26), open_boundaries=True, inflow_states=far_states())
        if mode == "fused":
            assert a.plan.c.has_open_faces and not a.plan.c.has_farfield_faces
        for _ in range(2):
            a.iterate(1e-3)
            b.iterate(1e-3)
        torch.cuda.synchronize()
        if mode == "fused":
            assert torch.equal(a.state(), b.state())
        else:
            assert rel_err(a.state().cpu().numpy(), b.state().cpu().numpy()) < TOL1[torch.float64]


def test_subgrid_acoustic_pulse_example_writes_a_readable_vtu(tmp_path):
    from _vtu import read_vtu
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "acoustic_pulse_subgrid_farfield.py"), "--toy", "--ramp",
                          "--out", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    files = sorted(tmp_path.glob("*.vtu"))
    assert files
    v = read_vtu(str(files[-1]))
    assert v["n_cells"] > 0 and v["arrays"]["density"].size == v["n_cells"]
    assert np.isfinite(v["arrays"]["density"]).all() and (v["arrays"]["density"] > 0).all()
