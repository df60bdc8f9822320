"""-m gpu: the scale-free refinement indicator (t8gpu_hip_plain_indicator_*, t8gpu_hip_subgrid_indicator_*,
t8gpu_hip_indicator_spread, amr.Loehner, the indicator= / coarsen_below= arguments of the adapt functions,
vtk.get_host_indicator_variable) against numpy.

The reference (tests/_indicator_ref.py) scatters per face with the forward sub-face map, the kernels gather per cell through
the CSR with the inverse map; both start from the arrays as uploaded taken to double, and the kernels' arithmetic is in
double for both float types. Tolerance 1e-12 ABSOLUTE (E is bounded by 1): a cell sums a few dozen terms (float64 and 80-bit
sums of the prototype differ by at most 5e-16 on these meshes), and the device's log / sqrt may differ from numpy's by an ulp
in q, which the eps = 0.01 floor in D_a bounds at about 100 ulp of E -- a margin of about 50.

Meshes as in test_gpu_fields.py: the "refined" meshes (115 / 127 elements, 1 840 / 8 128 subcells), whose conditions
`check_mesh_conditions` asserts, and the uniform walled meshes of the closed-form tests."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _indicator_ref as ref
from _gpu import NP, perturbed_state
from _vtu import read_vtu
from t8gpu_amd import amr, fields, hip, vtk
from t8gpu_amd.solver import PlainSolver, SubgridSolver
from t8gpu_amd.unstructured import PrismHexMesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float64, torch.float32]
TOL = 1e-12
EPS = 0.01
SENTINEL = -7.25
ALL = ref.QUANTITIES
SELECTIONS = [(q,) for q in ALL] + [ALL]


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    return ref.REFINED[name]()


def check_mesh_conditions(part):
    """what the refined meshes are there for: 2:1 faces of both orientations on every axis, a ragged last workgroup, a 2D
    Subgrid wavefront with fewer than four blocks"""
    dim, F = part.mesh.dim, part.F
    fn = np.asarray(part.face_neighbors)
    l, r = fn[0:2 * F:2], fn[1:2 * F:2]
    n = np.asarray(part.normals).reshape(-1, part.normal_dim)[:F]
    two_to_one = np.asarray(part.level_diff) != 0 if part.subgrid else part.levels[l] != part.levels[r]
    for a in range(dim):
        for sign in (1.0, -1.0):
            assert np.any(two_to_one & (n[:, a] == sign)), f"no 2:1 face with normal {sign:+.0f} e_{a}"
    assert part.N % 64 != 0 and part.N > 64
    if dim == 2:
        assert part.N % 4 != 0


def make_solver(part, dtype, state):
    cls = SubgridSolver if part.subgrid else PlainSolver
    return cls(part, dtype, mode="compat", state=state)


class Case:
    """a partition, its perturbed state and the solver holding it: built once, never written"""

    def __init__(self, mesh, subgrid, dtype):
        self.part = PrismHexMesh(5).partition() if mesh == "prism" else mesh_of(mesh).partition(subgrid=subgrid)
        if mesh in ref.REFINED:
            check_mesh_conditions(self.part)
        self.dtype, self.cells = dtype, self.part.N * self.part.cells_per_element
        self.state = perturbed_state(self.part, 11)
        self.solver = make_solver(self.part, dtype, self.state)
        self._want = {}

    def want(self, names, eps=EPS):
        key = (tuple(names), eps)
        if key not in self._want:
            w = ref.reference(self.state, self.part, NP[self.dtype], names, eps)
            assert w.shape == (self.cells,) and np.all(np.isfinite(w))
            self._want[key] = w
        return self._want[key]


@functools.lru_cache(maxsize=None)
def case(mesh, subgrid, dtype):
    return Case(mesh, subgrid, dtype)


def run_kernel(solver, mask, eps, cell_out, block_out, connectivity=True):
    """the C entries themselves (plain: cell_out is the output)"""
    off, ent = fields._csr(solver) if connectivity else (None, None)
    st, sp = solver.get_own_variables(solver.next), hip.stream_ptr()
    if hasattr(solver, "S"):
        hip.call("t8gpu_hip_subgrid_indicator", solver.dtype, solver.rank, solver.N, C.c_uint(mask), C.c_double(eps), st,
                 hip.ptr(solver.volumes), hip.ptr(solver.fn), hip.ptr(solver.level_diff), hip.ptr(solver.nb_offset),
                 hip.ptr(solver.normals), hip.ptr(solver.areas), hip.ptr(off), hip.ptr(ent), hip.ptr(cell_out), hip.ptr(block_out), sp)
    else:
        hip.call("t8gpu_hip_plain_indicator", solver.dtype, solver.N, solver.ndim, int(solver.part.mesh.dim), C.c_uint(mask),
                 C.c_double(eps), st, hip.ptr(solver.get_own_volume()), hip.ptr(solver.fn), hip.ptr(solver.normals),
                 hip.ptr(solver.areas), hip.ptr(off), hip.ptr(ent), hip.ptr(cell_out), sp)
    torch.cuda.synchronize()


def run_spread(solver, values):
    """t8gpu_hip_indicator_spread on `values` [N + G] (device): [N]"""
    off, ent = fields._csr(solver)
    out = torch.full((solver.N,), SENTINEL, dtype=torch.float64, device="cuda")
    hip.check(hip.lib().t8gpu_hip_indicator_spread(solver.N, hip.ptr(values), hip.ptr(solver.fn), hip.ptr(off), hip.ptr(ent),
                                                   hip.ptr(out), hip.stream_ptr()))
    torch.cuda.synchronize()
    return out


def check_values(c, what):
    """every selection of quantities: the cell values and, for a Subgrid case, the block maxima"""
    for names in SELECTIONS:
        ind = amr.Loehner(names, filter=EPS)
        got = ind.cell_values(c.solver)
        assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (c.cells,)
        got, want = got.cpu().numpy(), c.want(names)
        err = np.abs(got - want).max()
        print(f"{what} {'+'.join(names)}: max |E - want| = {err:.2e}, E in [{got.min():.3g}, {got.max():.3g}]")
        assert err <= TOL, (what, names, err)
        crit = ind.criteria(c.solver).cpu().numpy()
        assert crit.shape == (c.part.N,)
        assert np.abs(crit - ref.block_max(want, c.part)).max() <= TOL, (what, names, "block max")
        if c.part.subgrid:
            assert np.array_equal(crit, ref.block_max(got, c.part))             # max is exact
    one = amr.Loehner("pressure").cell_values(c.solver).cpu().numpy()           # a single name as a string
    assert np.abs(one - c.want(("pressure",))).max() <= TOL


# ---- 1: kernel against numpy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", list(ref.REFINED))
def test_kernel_matches_numpy(mesh, subgrid, dtype):
    check_values(case(mesh, subgrid, dtype), f"{mesh} subgrid={subgrid}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_curved_prism_and_hexahedron_mesh(dtype):
    """faces of any direction, triangles and quadrilaterals: no k_a is exactly 0 or 1"""
    c = case("prism", False, dtype)
    assert 100 <= c.part.N < 1000 and c.part.N % 64 != 0 and c.part.B > 0
    check_values(c, "prism")


# ---- 2: a uniform state gives exactly +0 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mesh,subgrid", [(m, sg) for m in ref.REFINED for sg in (False, True)] + [("prism", False)])
def test_uniform_state_gives_exact_zeros(mesh, subgrid, dtype):
    part = case(mesh, subgrid, dtype).part
    tot = (part.N + part.G) * part.cells_per_element
    rho, v, p = 1.3, (0.4, -0.7, 0.2), 0.9
    one = np.array([rho, rho * v[0], rho * v[1], rho * v[2], p / 0.4 + 0.5 * rho * sum(x * x for x in v)])
    solver = make_solver(part, dtype, np.repeat(one[:, None], tot, axis=1))
    for eps in (EPS, 0.0):                                      # (eps = 0: the zero-denominator branch)
        for names in (("density",), ALL):
            ind = amr.Loehner(names, filter=eps)
            for t in (ind.cell_values(solver), ind.criteria(solver)):
                bits = t.view(torch.int64)
                assert bool((bits == 0).all()), (mesh, eps, names, float(t.abs().max()))


# ---- 3: dyadic linear density on uniform walled meshes ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("dim", [2, 3])
def test_linear_density_is_annihilated(dim, subgrid, dtype):
    """rho = 1 + slope . x with short dyadic slopes and centres (and a rigid rotation in the momentum, which the density
    indicator does not read): every difference is exact and the two opposite faces of a cell cancel, so E == 0 exactly in
    every cell -- at a wall through the closure k_a = 0"""
    part = ref.uniform_walled(dim).partition(subgrid=subgrid)
    assert np.all(part.levels == part.levels[0]) and part.B > 0
    x, _ = ref.cell_centres(part)
    slope = np.array([0.5, -0.25, 0.125 if dim == 3 else 0.0])
    omega = np.array([0.5, -0.25, 0.75]) if dim == 3 else np.array([0.0, 0.0, 0.75])
    rho = 1.0 + x @ slope
    u = np.cross(omega[None, :], x).T
    state = np.stack([rho, rho * u[0], rho * u[1], rho * u[2], 2.5 + 0.5 * rho * (u ** 2).sum(0)])
    assert np.array_equal(state[:4].astype(NP[dtype]).astype(np.float64), state[:4])
    solver = make_solver(part, dtype, state)
    for eps in (EPS, 0.0):
        E = amr.Loehner("density", filter=eps).cell_values(solver)
        assert bool((E == 0.0).all()), (dim, subgrid, eps, float(E.max()))


# ---- 4: the step state: closed form and marks -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("dim", [2, 3])
def test_step_state_closed_form_and_marks(dim, subgrid, dtype):
    mesh = ref.uniform_walled(dim)
    part = mesh.partition(subgrid=subgrid)
    solver = make_solver(part, dtype, ref.step_state(part))
    want = ref.step_expected(part, EPS)
    got = amr.Loehner("density", filter=EPS).cell_values(solver).cpu().numpy()
    print(f"step {dim}D subgrid={subgrid}: max |E - closed form| = {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= TOL
    assert np.all(got[want == 0] == 0.0)
    level = int(part.levels[0])
    edge = 0.5 ** level
    for buffer in (0, 1, 2):
        crit = amr.Loehner("density", filter=EPS, buffer=buffer).criteria(solver).cpu().numpy()
        marks = mesh.marks_from_criteria(crit, 0.8, level, level + 1, coarsen_below=0.2)
        near = np.abs(part.centres[: part.N, 0] - 0.5) < (1 + buffer) * edge
        assert 0 < near.sum() and (buffer > 0 or near.sum() < part.N)
        assert np.array_equal(marks, near.astype(np.int8)), (dim, subgrid, buffer)


# ---- 5: NULL outputs, refused arguments --------------------------------------------------------------------------------------
SMALL = ["refined-2d-walls", "refined-3d-periodic"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mesh", SMALL)
def test_null_outputs_are_left_alone(mesh, dtype):
    c = case(mesh, True, dtype)
    want = c.want(ALL)
    cells = torch.full((c.cells,), SENTINEL, dtype=torch.float64, device="cuda")
    blocks = torch.full((c.part.N,), SENTINEL, dtype=torch.float64, device="cuda")
    run_kernel(c.solver, 15, EPS, cells, None)
    assert np.abs(cells.cpu().numpy() - want).max() <= TOL and bool((blocks == SENTINEL).all())
    cells.fill_(SENTINEL)
    run_kernel(c.solver, 15, EPS, None, blocks)
    assert np.abs(blocks.cpu().numpy() - ref.block_max(want, c.part)).max() <= TOL and bool((cells == SENTINEL).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", SMALL)
def test_bad_arguments_are_refused_and_nothing_is_written(mesh, subgrid, dtype):
    c = case(mesh, subgrid, dtype)
    cells = torch.full((c.cells,), SENTINEL, dtype=torch.float64, device="cuda")
    blocks = torch.full((c.part.N,), SENTINEL, dtype=torch.float64, device="cuda")
    for mask, eps, conn in ((0, EPS, True), (16, EPS, True), (1 | 32, EPS, True), (1, -0.5, True), (1, EPS, False)):
        with pytest.raises(hip.T8gpuHipError):
            run_kernel(c.solver, mask, eps, cells, blocks if subgrid else None, connectivity=conn)
    torch.cuda.synchronize()
    assert bool((cells == SENTINEL).all()) and bool((blocks == SENTINEL).all())
    values = torch.zeros(c.part.N + c.part.G, dtype=torch.float64, device="cuda")
    off, ent = fields._csr(c.solver)
    lib = hip.lib()
    assert lib.t8gpu_hip_indicator_spread(c.part.N, hip.ptr(values), None, hip.ptr(off), hip.ptr(ent), hip.ptr(blocks), hip.stream_ptr()) != 0
    assert lib.t8gpu_hip_indicator_spread(0, None, None, None, None, None, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((blocks == SENTINEL).all())


# ---- 6: determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", list(ref.REFINED))
def test_two_calls_give_identical_bits(mesh, subgrid, dtype):
    c = case(mesh, subgrid, dtype)
    ind = amr.Loehner(ALL, filter=EPS, buffer=2)
    for f in (ind.cell_values, ind.criteria, amr.Loehner(ALL, filter=EPS).criteria):
        a, b = f(c.solver), f(c.solver)
        assert a.data_ptr() != b.data_ptr()
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


# ---- 7: three ranks against one rank ----------------------------------------------------------------------------------------
def smooth_state(part):
    """a smooth, non-periodic function of the cell centres, for every slot (owned and ghost)"""
    x, _ = ref.cell_centres(part)
    x, y, z = x.T
    rho = 1.0 + 0.3 * np.sin(2.0 * x + 1.0) * np.cos(3.0 * y) + 0.1 * z
    v = np.stack([0.4 * np.sin(3.0 * y + z), 0.3 * np.cos(2.0 * x) + 0.1 * z, 0.2 * np.sin(x + 2.0 * y + 3.0 * z)])
    p = 1.0 + 0.2 * np.cos(x - y + z)
    return np.stack([rho, rho * v[0], rho * v[1], rho * v[2], p / 0.4 + 0.5 * rho * (v ** 2).sum(0)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", ["refined-2d-periodic", "refined-3d-walls"])
def test_three_ranks_equal_one_rank(mesh, subgrid, dtype):
    """a 3-way partition on one GPU, ghost slots filled like owned ones: every rank's owned cells get the one-rank values
    within 1e-12 (the CSR order differs per partition); the spread of an array given by global index is exact"""
    m = mesh_of(mesh)
    whole = m.partition(subgrid=subgrid)
    S = whole.cells_per_element
    ind = amr.Loehner(ALL, filter=EPS)
    whole_solver = make_solver(whole, dtype, smooth_state(whole))
    one = ind.cell_values(whole_solver).cpu().numpy()
    rng = np.random.default_rng(3)
    by_global = rng.uniform(0.0, 1.0, whole.N)
    one_spread = run_spread(whole_solver, torch.from_numpy(by_global).cuda()).cpu().numpy()
    assert np.array_equal(one_spread, ref.spread(by_global, whole))
    ghost_sides = 0
    for r in range(3):
        part = m.partition(r, 3, subgrid=subgrid)
        assert part.G > 0
        ghost_sides += int((np.asarray(part.face_neighbors)[: 2 * part.F] >= part.N).sum())
        solver = make_solver(part, dtype, smooth_state(part))
        got = ind.cell_values(solver).cpu().numpy()
        lo, hi = part.first_global, part.first_global + part.N
        assert np.abs(got - one[lo * S:hi * S]).max() <= TOL, (mesh, r)
        gidx = np.concatenate([np.arange(lo, hi), part.ghost_global])
        got_spread = run_spread(solver, torch.from_numpy(by_global[gidx]).cuda()).cpu().numpy()
        assert np.array_equal(got_spread, one_spread[lo:hi]), (mesh, r)
    assert ghost_sides > 0


# ---- 8: end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("dim", [2, 3])
def test_adapt_by_the_indicator(dim, subgrid):
    mesh = ref.uniform_walled(dim)
    part = mesh.partition(subgrid=subgrid)
    solver = make_solver(part, torch.float64, ref.step_state(part))
    level = int(part.levels[0])
    old = [solver.compute_integral(k) for k in range(5)]
    adapt = amr.adapt_subgrid if subgrid else amr.adapt
    new, marks, adapt_data = adapt(solver, 0.8, level, level + 1, indicator=amr.Loehner(buffer=1), coarsen_below=0.2)
    near_old = np.abs(part.centres[: part.N, 0] - 0.5) < 2 * 0.5 ** level
    assert np.array_equal(marks, near_old.astype(np.int8))
    p = new.part
    assert p.mesh.finest_level == level + 1 and adapt_data.size == p.N + 1
    near_new = np.abs(p.centres[: p.N, 0] - 0.5) < 2 * 0.5 ** level
    assert np.array_equal(p.levels[: p.N] == level + 1, near_new)              # the finest level covers the step columns
    for k in range(5):
        assert abs(new.compute_integral(k) - old[k]) <= 1e-12 * max(1.0, abs(old[k])), (k, old[k])
    assert bool(torch.isfinite(new.state()).all())


@pytest.mark.parametrize("subgrid", [False, True])
def test_no_indicator_is_the_path_of_today(subgrid):
    """indicator=None, coarsen_below=None: the marks and adapt_data of a call without the new arguments, byte for byte"""
    c = case("refined-2d-walls", subgrid, torch.float64)
    crit = (amr.subgrid_refinement_criteria if subgrid else amr.refinement_criteria)(c.solver).double().cpu().numpy()
    s = np.sort(crit)
    k = len(s) // 4 + int(np.argmax(np.diff(s[len(s) // 4: 3 * len(s) // 4])))
    threshold = 0.5 * (s[k] + s[k + 1])                         # in the widest gap of the middle half: no mark hangs on a last bit
    adapt = amr.adapt_subgrid if subgrid else amr.adapt
    a = adapt(c.solver, threshold, 1, 6)
    b = adapt(c.solver, threshold, 1, 6, indicator=None, coarsen_below=None)
    assert (a[1] == 1).any()
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert torch.equal(a[0].state(), b[0].state())
    if not subgrid:
        assert abs(a[0].last_adapt_criteria_sum - b[0].last_adapt_criteria_sum) <= 1e-12 * abs(a[0].last_adapt_criteria_sum)


# ---- 9: VTK and the example -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
def test_vtk_variable(subgrid, tmp_path):
    c = case("refined-2d-walls", subgrid, torch.float32)
    ind = amr.Loehner(("density", "pressure"))
    info = vtk.get_host_indicator_variable(c.solver, ind)
    assert (info.type, info.name) == (vtk.SCALAR, "indicator") and info.data.shape == (c.cells,)
    dev = ind.cell_values(c.solver).cpu().numpy()
    assert np.array_equal(np.sort(info.data), np.sort(dev))
    if not subgrid:
        assert np.array_equal(info.data, dev)
    v = read_vtu(vtk.save_variables_to_vtk(c.solver, [info], str(tmp_path / "indicator")))
    assert np.array_equal(v["arrays"]["indicator"], info.data)


def test_riemann_example_writes_an_indicator_array(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "riemann2d_amr.py"), "--toy", "--indicator", "loehner",
                          "--out", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    v = read_vtu(str(tmp_path / "riemann2d.vtu"))
    assert "indicator" in v["arrays"], list(v["arrays"])
    s = v["arrays"]["indicator"]
    assert s.shape == (v["n_cells"],) and np.all(np.isfinite(s)) and s.min() >= 0.0 and s.max() <= 1.0 and s.max() > 0.0
