"""-m gpu: the derived output fields (t8gpu_hip_plain_fields_*, t8gpu_hip_subgrid_fields_*, _Solver.derived_fields,
vtk.get_host_derived_variable) against numpy.

The reference (tests/_fields_ref.py) forms the gradient fields by face scatter with the forward sub-face map, the kernels
gather per cell through the CSR with the inverse map; both start from the arrays as uploaded (for fp32 the float32 values)
taken to double. The kernels' arithmetic is in double for both float types, so one tolerance serves both: 1e-12 of
max |want| per field (TOL1[float64]): a cell sums at most a few dozen terms of one magnitude, each a few ulp off, which
leaves a margin of about 1000.

Meshes. SynthMesh refines in bands of the LAST axis only, and the three meshes first named for these tests
(SynthMesh(2, 2, 4, band=0.2) periodic and walled, SynthMesh(3, 1, 3, band=0.3)) come out uniform at their finest level with
256 / 512 elements: they run here as the same-level cases. The conditions the tests need -- 2:1 faces in both orientations
along EVERY axis, walls or a periodic wrap, an element count that is no multiple of 64 (so none of 256), a 2D Subgrid count
that is no multiple of 4 -- are met by the "refined" meshes, a uniform mesh with a box of elements (and element 0, at the
periodic wrap) refined once; `check_mesh_conditions` asserts them, so a mesh change cannot hide a case."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _fields_ref as ref
from _gpu import NP, perturbed_state
from _vtu import read_vtu
from t8gpu_amd import fields, hip, vtk
from t8gpu_amd.solver import PlainSolver, SubgridSolver
from t8gpu_amd.synth import SynthMesh
from t8gpu_amd.unstructured import PrismHexMesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float64, torch.float32]
TOL = 1e-12
NAMES = list(fields.FIELDS)
SENTINEL = -7.25


def refined(dim, level, periodic, lo, hi):
    """a uniform mesh with the elements whose centres lie in the box (lo, hi)^dim, and element 0, refined once"""
    mesh = SynthMesh(dim, level, level, periodic=periodic)
    part = mesh.partition()
    c = part.centres[: part.N, :dim]
    marks = np.all((c > lo) & (c < hi), axis=1).astype(np.int8)
    marks[0] = 1
    return mesh.adapt(marks)[0]


MESHES = {
    "named-2d-periodic": lambda: SynthMesh(2, 2, 4, band=0.2),
    "named-2d-walls": lambda: SynthMesh(2, 2, 4, band=0.2, periodic=False),
    "named-3d-periodic": lambda: SynthMesh(3, 1, 3, band=0.3),
    "refined-2d-periodic": lambda: refined(2, 3, True, 0.3, 0.8),
    "refined-2d-walls": lambda: refined(2, 3, False, 0.3, 0.8),
    "refined-3d-periodic": lambda: refined(3, 2, True, 0.2, 0.8),
    "refined-3d-walls": lambda: refined(3, 2, False, 0.2, 0.8),
}
REFINED = [m for m in MESHES if m.startswith("refined")]


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    return MESHES[name]()


def check_mesh_conditions(part):
    """what the refined meshes are there for (module docstring)"""
    dim, F = part.mesh.dim, part.F
    fn = np.asarray(part.face_neighbors)
    l, r = fn[0:2 * F:2], fn[1:2 * F:2]
    n = np.asarray(part.normals).reshape(-1, part.normal_dim)[:F]
    two_to_one = np.asarray(part.level_diff) != 0 if part.subgrid else part.levels[l] != part.levels[r]
    for a in range(dim):
        for sign in (1.0, -1.0):
            assert np.any(two_to_one & (n[:, a] == sign)), f"no 2:1 face with normal {sign:+.0f} e_{a}"
    assert part.N % 64 != 0 and part.N > 64                     # more than one workgroup, a ragged last one
    if dim == 2:
        assert part.N % 4 != 0                                  # a 2D Subgrid wavefront with fewer than four blocks
    periodic = bool(np.all(part.mesh.sides == -1))
    assert (part.B == 0) if periodic else (part.B > 0)


def make_solver(part, dtype, state):
    cls = SubgridSolver if part.subgrid else PlainSolver
    return cls(part, dtype, mode="compat", state=state)


class Case:
    """a partition, its perturbed state, the solver holding it and the numpy reference: built once, never written"""

    def __init__(self, mesh, subgrid, dtype, part=None):
        self.part = mesh_of(mesh).partition(subgrid=subgrid) if part is None else part
        if mesh in REFINED:
            check_mesh_conditions(self.part)
        self.dtype, self.cells = dtype, self.part.N * self.part.cells_per_element
        self.state = perturbed_state(self.part, 11)
        self.solver = make_solver(self.part, dtype, self.state)
        self.want = ref.reference(self.state, self.part, NP[dtype])
        assert self.want.shape == (ref.PLANES, self.cells) and np.all(np.isfinite(self.want))


@functools.lru_cache(maxsize=None)
def case(mesh, subgrid, dtype):
    if mesh == "prism":
        return Case(mesh, False, dtype, PrismHexMesh(5).partition())
    return Case(mesh, subgrid, dtype)


def planes_of(got):
    """{name: tensor} of derived_fields -> {name: [planes, cells] numpy}"""
    return {k: np.atleast_2d(v.cpu().numpy()) for k, v in got.items()}


def check_fields(got, want, what):
    for name, planes in got.items():
        w = want[ref.SLOTS[name]]
        assert planes.shape == w.shape and planes.dtype == np.float64, (what, name, planes.shape)
        scale = np.abs(w).max()
        err = np.abs(planes - w).max()
        print(f"{what} {name}: max error / max |want| = {err / max(scale, 1e-300):.2e}")
        assert err <= TOL * scale, (what, name, err, scale)


def call_kernel(solver, planes, connectivity=True):
    """the C entry itself, into `planes` [11, cells] (a row asked for <=> its index in `rows`)"""
    return lambda rows: _call_kernel(solver, planes, rows, connectivity)


def _call_kernel(solver, planes, rows, connectivity):
    fp = fields.FieldPlanes()
    for k in rows:
        fp.p[k] = planes[k].data_ptr()
    none = [None] * 8
    st, sp = solver.get_own_variables(solver.next), hip.stream_ptr()
    if connectivity:
        off, ent = fields._csr(solver)
    if hasattr(solver, "S"):
        conn = [hip.ptr(solver.volumes), hip.ptr(solver.fn), hip.ptr(solver.level_diff), hip.ptr(solver.nb_offset),
                hip.ptr(solver.normals), hip.ptr(solver.areas), hip.ptr(off), hip.ptr(ent)] if connectivity else none
        hip.call("t8gpu_hip_subgrid_fields", solver.dtype, solver.rank, solver.N, st, *conn, fp, sp)
    else:
        conn = [hip.ptr(solver.get_own_volume()), hip.ptr(solver.fn), hip.ptr(solver.normals), hip.ptr(solver.areas), hip.ptr(off),
                hip.ptr(ent)] if connectivity else none[:6]
        hip.call("t8gpu_hip_plain_fields", solver.dtype, solver.N, solver.ndim, st, *conn, fp, sp)
    torch.cuda.synchronize()


# ---- 1: every field against numpy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_every_field_matches_numpy(mesh, subgrid, dtype):
    c = case(mesh, subgrid, dtype)
    got = c.solver.derived_fields(NAMES)
    assert list(got) == NAMES
    for name, t in got.items():
        assert t.dtype == torch.float64 and t.is_cuda
        assert tuple(t.shape) == ((3, c.cells) if len(ref.SLOTS[name]) == 3 else (c.cells,))
    check_fields(planes_of(got), c.want, f"{mesh} subgrid={subgrid}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_curved_prism_and_hexahedron_mesh(dtype):
    """faces of any direction, triangles and quadrilaterals, three-component normals that are no axis"""
    c = case("prism", False, dtype)
    assert 100 <= c.part.N < 1000 and c.part.N % 64 != 0 and c.part.B > 0
    check_fields(planes_of(c.solver.derived_fields(NAMES)), c.want, "prism")


def test_unknown_names_raise():
    c = case("refined-2d-walls", False, torch.float64)
    with pytest.raises(ValueError):
        c.solver.derived_fields(["pressure", "enstrophy"])
    one = c.solver.derived_fields("schlieren")                  # a single name as a string
    check_fields(planes_of(one), c.want, "one name")


# ---- 2: a uniform state has no gradient, exactly -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mesh,subgrid", [(m, sg) for m in MESHES for sg in (False, True)] + [("prism", False)])
def test_uniform_state_gives_exact_zeros(mesh, subgrid, dtype):
    part = case(mesh, subgrid, dtype).part
    tot = (part.N + part.G) * part.cells_per_element
    rho, v, p = 1.3, (0.4, -0.7, 0.2), 0.9
    one = np.array([rho, rho * v[0], rho * v[1], rho * v[2], p / 0.4 + 0.5 * rho * sum(x * x for x in v)])
    solver = make_solver(part, dtype, np.repeat(one[:, None], tot, axis=1))
    got = solver.derived_fields(fields.GRADIENT_FIELDS)
    for name, t in got.items():
        assert bool((t == 0.0).all()), (mesh, name, float(t.abs().max()))


# ---- 3: linear density and rigid rotation on uniform walled meshes --------------------------------------------------------
def cell_centres(part):
    """centres and edge lengths of the cells (subcells of Subgrid blocks, storage order), owned and ghost"""
    dim, tot = part.mesh.dim, part.N + part.G
    edge = 0.5 ** part.levels[:tot].astype(np.float64)
    if not part.subgrid:
        return part.centres[:tot].copy(), edge
    S = 4 ** dim
    c = np.arange(S)
    rel = np.stack([(((c >> (2 * a)) & 3) + 0.5) / 4 - 0.5 if a < dim else np.zeros(S) for a in range(3)], axis=1)   # [S, 3]
    x = part.centres[:tot, None, :] + rel[None, :, :] * edge[:, None, None]
    return x.reshape(-1, 3), np.repeat(edge / 4, S)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("dim", [2, 3])
def test_linear_density_and_rigid_rotation(dim, subgrid, dtype):
    """rho = 1 + slope . x and u = Omega x x at the cell centres: away from the walls the central difference is exact, so
    schlieren = |slope|, vorticity = 2 Omega, dilatation = 0. In 2D Omega = Omega_z e_z (u has no z dependence to take
    d/dz of). Slopes, Omega and the centres are short dyadic numbers, so rho, u and the momentum rho u (at most 20
    significant bits) are exact in float32 too and m / rho gives u back exactly: 1e-12 relative holds for both float types."""
    mesh = SynthMesh(2, 3, 3, periodic=False) if dim == 2 else SynthMesh(3, 2, 2, periodic=False)
    part = mesh.partition(subgrid=subgrid)
    assert np.all(part.levels == part.levels[0]) and part.B > 0
    x, edge = cell_centres(part)
    slope = np.array([0.5, -0.25, 0.125 if dim == 3 else 0.0])
    omega = np.array([0.5, -0.25, 0.75]) if dim == 3 else np.array([0.0, 0.0, 0.75])
    rho = 1.0 + x @ slope
    u = np.cross(omega[None, :], x).T                                          # [3, cells]
    state = np.stack([rho, rho * u[0], rho * u[1], rho * u[2], 2.5 + 0.5 * rho * (u ** 2).sum(0)])
    assert np.array_equal(state[:4].astype(NP[dtype]).astype(np.float64), state[:4])      # exact in the uploaded type
    solver = make_solver(part, dtype, state)
    got = planes_of(solver.derived_fields(fields.GRADIENT_FIELDS))
    cells = part.N * part.cells_per_element
    inner = np.all((x[:cells, :dim] - edge[:cells, None] > 1e-9) & (x[:cells, :dim] + edge[:cells, None] < 1 - 1e-9), axis=1)
    assert 0 < inner.sum() < cells
    want_s = np.linalg.norm(slope)
    assert np.abs(got["schlieren"][0, inner] - want_s).max() <= TOL * want_s
    assert np.abs(got["vorticity"][:, inner] - 2 * omega[:, None]).max() <= TOL * np.abs(2 * omega).max()
    assert np.abs(got["dilatation"][0, inner]).max() <= TOL * np.abs(2 * omega).max()


# ---- 4, 5: NULL planes, connectivity-free pointwise calls, determinism -----------------------------------------------------
SMALL = ["refined-2d-walls", "refined-3d-periodic"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", SMALL)
def test_null_planes_are_left_alone(mesh, subgrid, dtype):
    c = case(mesh, subgrid, dtype)
    for rows in ((0, 2, 7, 10), (5,), (9,), (1, 2, 3, 6, 8)):
        planes = torch.full((ref.PLANES, c.cells), SENTINEL, dtype=torch.float64, device="cuda")
        call_kernel(c.solver, planes)(rows)
        got = planes.cpu().numpy()
        for k in range(ref.PLANES):
            if k in rows:
                scale = np.abs(c.want[ref.SLOTS[slot_name(k)]]).max()          # (of the whole field, as everywhere)
                assert np.abs(got[k] - c.want[k]).max() <= TOL * scale, (rows, k)
            else:
                assert np.all(got[k] == SENTINEL), (rows, k)


def slot_name(k):
    return next(name for name, slots in ref.SLOTS.items() if k in slots)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", SMALL)
def test_pointwise_call_needs_no_connectivity(mesh, subgrid, dtype):
    c = case(mesh, subgrid, dtype)
    planes = torch.full((ref.PLANES, c.cells), SENTINEL, dtype=torch.float64, device="cuda")
    call_kernel(c.solver, planes, connectivity=False)(range(6))
    got = planes.cpu().numpy()
    check_fields({name: got[ref.SLOTS[name]] for name in ("pressure", "velocity", "mach", "entropy")}, c.want, "pointwise only")
    assert np.all(got[6:] == SENTINEL)
    with pytest.raises(hip.T8gpuHipError):                      # a gradient plane without connectivity: refused, nothing written
        call_kernel(c.solver, planes, connectivity=False)((0, 9))
    assert np.array_equal(planes.cpu().numpy(), got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", REFINED)
def test_two_calls_give_identical_bits(mesh, subgrid, dtype):
    c = case(mesh, subgrid, dtype)
    a, b = c.solver.derived_fields(NAMES), c.solver.derived_fields(NAMES)
    for name in NAMES:
        assert a[name].data_ptr() != b[name].data_ptr()
        assert torch.equal(a[name].view(torch.int64), b[name].view(torch.int64)), name


# ---- 6: ghost faces -----------------------------------------------------------------------------------------------------
def smooth_state(part):
    """a smooth, non-periodic function of the cell centres, for every slot (owned and ghost)"""
    x, _ = cell_centres(part)
    x, y, z = x.T
    rho = 1.0 + 0.3 * np.sin(2.0 * x + 1.0) * np.cos(3.0 * y) + 0.1 * z
    v = np.stack([0.4 * np.sin(3.0 * y + z), 0.3 * np.cos(2.0 * x) + 0.1 * z, 0.2 * np.sin(x + 2.0 * y + 3.0 * z)])
    p = 1.0 + 0.2 * np.cos(x - y + z)
    return np.stack([rho, rho * v[0], rho * v[1], rho * v[2], p / 0.4 + 0.5 * rho * (v ** 2).sum(0)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", ["named-2d-periodic", "refined-2d-periodic", "refined-3d-walls"])
def test_three_ranks_equal_one_rank(mesh, subgrid, dtype):
    """a 3-way partition on one GPU, ghost slots filled like owned ones: every rank's owned cells get the one-rank fields"""
    m = mesh_of(mesh)
    whole = m.partition(subgrid=subgrid)
    S = whole.cells_per_element
    one = planes_of(make_solver(whole, dtype, smooth_state(whole)).derived_fields(NAMES))
    ghost_sides = 0
    for r in range(3):
        part = m.partition(r, 3, subgrid=subgrid)
        assert part.G > 0
        fn = np.asarray(part.face_neighbors)[: 2 * part.F]
        ghost_sides += int((fn >= part.N).sum())
        got = planes_of(make_solver(part, dtype, smooth_state(part)).derived_fields(NAMES))
        lo, hi = part.first_global * S, (part.first_global + part.N) * S
        for name in NAMES:
            want = one[name][:, lo:hi]
            assert np.abs(got[name] - want).max() <= TOL * np.abs(one[name]).max(), (mesh, r, name)
    assert ghost_sides > 0


# ---- 7: VTK ----------------------------------------------------------------------------------------------------------------
def z_order_permutation(dim):
    """to[morton(i, j, k)] = from[i + 4 j + 16 k]: the cell order of a block in the file"""
    S = 4 ** dim
    perm = np.zeros(S, np.int64)
    for flat in range(S):
        c = [(flat >> (2 * a)) & 3 for a in range(3)]
        m = 0
        for lbit in range(2):
            for a in range(dim):
                m |= ((c[a] >> lbit) & 1) << (dim * lbit + a)
        perm[m] = flat
    return perm


@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", SMALL)
def test_vtk_round_trip(mesh, subgrid, tmp_path):
    c = case(mesh, subgrid, torch.float32)
    dev = planes_of(c.solver.derived_fields(["mach", "vorticity"]))
    infos = [vtk.get_host_derived_variable(c.solver, "mach"), vtk.get_host_derived_variable(c.solver, "vorticity")]
    assert (infos[0].type, infos[1].type) == (vtk.SCALAR, vtk.VECTOR)
    assert infos[0].data.shape == (c.cells,) and infos[1].data.shape == (c.cells, 3)
    v = read_vtu(vtk.save_variables_to_vtk(c.solver, infos, str(tmp_path / "fields")))
    assert v["n_cells"] == c.cells
    if subgrid:
        S, perm = c.part.cells_per_element, z_order_permutation(c.part.mesh.dim)
        order = (np.arange(c.part.N)[:, None] * S + perm[None, :]).reshape(-1)
    else:
        order = np.arange(c.cells)
    assert np.array_equal(v["arrays"]["mach"], dev["mach"][0][order])
    assert np.array_equal(v["arrays"]["vorticity"], dev["vorticity"][:, order].T)


def test_riemann_example_writes_a_schlieren_array(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "riemann2d_amr.py"), "--toy", "--out", str(tmp_path)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    v = read_vtu(str(tmp_path / "riemann2d.vtu"))
    for name in ("density", "energy", "momentum", "pressure", "schlieren"):
        assert name in v["arrays"], (name, list(v["arrays"]))
    s = v["arrays"]["schlieren"]
    assert s.shape == (v["n_cells"],) and np.all(np.isfinite(s)) and s.max() > 0 and s.min() >= 0
    assert np.all(v["arrays"]["pressure"] > 0)
