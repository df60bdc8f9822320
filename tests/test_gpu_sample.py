"""-m gpu: sampling on the device (t8gpu_hip_sample_*, _Solver.locate / sample_points / sample_grid / resample_uniform;
DESIGN.md §12) against host_locate and the brute force of _sample_ref.py.

Sampled values are a cell's value cast to double and are compared BITWISE, NaN fill included. The conservative resample
sums, per pixel, at most 64 terms w q (256 at the coarsest level of band-2d) in double, each product exact or one rounding
off, against a brute force that sums overlap volume times value in another order: both are within a few hundred ulp of
max |q|, so 1e-12 of max |q| per plane leaves a margin above 100 (the argument of test_gpu_fields.py)."""
import functools

import numpy as np
import pytest
import torch

import _sample_ref as ref
from _gpu import NP, perturbed_state
from t8gpu_amd import hip, sample
from t8gpu_amd.solver import PlainSolver, SubgridSolver

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
MESHES = list(ref.MESHES)
TOL = 1e-12
SENTINEL = -7.25
CONSERVED = ["density", "momentum", "energy"]
NAMES = CONSERVED + ["pressure", "schlieren"]
LO, HI = (0.1, 0.05, 0.2), (0.93, 1.2, 0.9)                     # a box that sticks out of the domain
GRID = {2: (37, 21), 3: (9, 7, 5)}                              # ragged 8 x 8 tiles
LEVELS = {2: (2, 3, 4, 5), 3: (1, 2, 3, 4)}


def make_solver(part, dtype, state):
    cls = SubgridSolver if part.subgrid else PlainSolver
    return cls(part, dtype, mode="compat", state=state)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64))


def host(t):
    return t.cpu().numpy()


class Case:
    """a partition, its perturbed state, the solver holding it, the point set and the brute-force cells: built once, never
    written"""

    def __init__(self, mesh, subgrid, dtype):
        self.part = ref.partition(mesh, subgrid)
        self.dim, self.dtype = self.part.mesh.dim, dtype
        self.cells = self.part.N * self.part.cells_per_element
        self.state = perturbed_state(self.part, 11)
        self.solver = make_solver(self.part, dtype, self.state)
        self.points, self.cls = points_of(mesh, subgrid)
        self.want_cells = brute_cells(mesh, subgrid)

    @functools.cached_property
    def values(self):
        """{name: [planes, cells] float64}: the state as uploaded cast to double, derived_fields copied to the host"""
        st = self.state[:, :self.cells].astype(NP[self.dtype]).astype(np.float64)
        assert np.array_equal(st, host(self.solver.state()).astype(np.float64))
        v = {"density": st[0:1], "momentum": st[1:4], "energy": st[4:5]}
        for name, t in self.solver.derived_fields(["pressure", "schlieren"]).items():
            v[name] = np.atleast_2d(host(t))
        return v

    def expected(self, name, cells, fill):
        v = self.values[name]
        out = np.where(cells >= 0, v[:, np.maximum(cells, 0)], fill)
        return out if v.shape[0] == 3 else out[0]


@functools.lru_cache(maxsize=None)
def points_of(mesh, subgrid):
    points, cls = ref.point_set(ref.partition(mesh, subgrid), 5)
    assert points.shape[0] % 64 != 0 and cls["random"].stop == 1003
    return points, cls


@functools.lru_cache(maxsize=None)
def brute_cells(mesh, subgrid):
    part = ref.partition(mesh, subgrid)
    return ref.locate(part, points_of(mesh, subgrid)[0])


@functools.lru_cache(maxsize=None)
def case(mesh, subgrid, dtype):
    return Case(mesh, subgrid, dtype)


def pixel_centres(dim, shape, lo, hi):
    """[pixels, dim], x fastest: lo + (i + 0.5) (hi - lo) / n per axis"""
    axes = [lo[a] + (np.arange(shape[a]) + 0.5) * (hi[a] - lo[a]) / shape[a] for a in range(dim)]
    grids = np.meshgrid(*axes[::-1], indexing="ij")                 # slowest axis first
    return np.stack([g.reshape(-1) for g in grids[::-1]], axis=1)


# ---- 1: locate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_locate_equals_host_and_brute_force(mesh, subgrid):
    c = case(mesh, subgrid, torch.float64)
    got = c.solver.locate(c.points)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (c.points.shape[0],)
    got = host(got)
    assert np.array_equal(got, sample.host_locate(c.part, c.points))
    assert np.array_equal(got, c.want_cells)
    cls = c.cls
    assert np.array_equal(got[cls["corner"]], cls["pick"]) and np.array_equal(got[cls["face"]], cls["pick"])      # the tie rule
    assert np.all(got[cls["inside_edge"]] >= 0) and np.all(got[cls["random"]] >= 0)
    assert np.all(got[cls["outside"]] == -1) and np.all(got[cls["bad"]] == -1)
    bad = c.points[cls["bad"]]
    assert np.isnan(bad).any() and np.isposinf(bad).any() and (bad == 1e300).any()
    # every cell centre gives that very cell; a device tensor of points is taken as it is
    lo, edge, _ = ref.cell_boxes(c.part)
    centres = torch.from_numpy(lo + 0.5 * edge[:, None]).cuda()
    assert np.array_equal(host(c.solver.locate(centres)), np.arange(c.cells, dtype=np.int32))
    # one point, no point
    assert host(c.solver.locate(c.points[:1])).tolist() == [int(c.want_cells[0])]
    empty = c.solver.locate(np.zeros((0, c.dim)))
    assert tuple(empty.shape) == (0,) and empty.dtype == torch.int32
    with pytest.raises(ValueError):
        c.solver.locate(np.zeros((4, c.dim + 1)))


# ---- 2: sample_points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_sample_points_is_the_cell_value_bitwise(mesh, subgrid, dtype):
    c = case(mesh, subgrid, dtype)
    m = c.points.shape[0]
    for fill in (np.nan, SENTINEL):
        got = c.solver.sample_points(c.points, NAMES) if np.isnan(fill) else c.solver.sample_points(c.points, NAMES, fill=fill)
        assert list(got) == NAMES
        for name, t in got.items():
            assert t.dtype == torch.float64 and t.is_cuda
            assert tuple(t.shape) == ((3, m) if name == "momentum" else (m,))
            assert bits_equal(host(t), c.expected(name, c.want_cells, fill)), (name, fill)
    one = c.solver.sample_points(c.points[:1], "energy")
    assert bits_equal(host(one["energy"]), c.expected("energy", c.want_cells[:1], np.nan))
    none = c.solver.sample_points(np.zeros((0, c.dim)), ["momentum", "pressure"])
    assert tuple(none["momentum"].shape) == (3, 0) and tuple(none["pressure"].shape) == (0,)
    with pytest.raises(ValueError, match="density"):
        c.solver.sample_points(c.points, ["density", "enstrophy"])


# ---- 3: sample_grid ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_sample_grid_equals_sample_points_on_the_pixel_centres(mesh, subgrid, dtype):
    c = case(mesh, subgrid, dtype)
    dim, shape = c.dim, GRID[c.dim]
    lo, hi = LO[:dim], HI[:dim]
    pts = pixel_centres(dim, shape, lo, hi)
    assert (pts[:, 1] >= 1.0).any() and (pts[:, 1] < 1.0).any()     # the box does stick out
    want = c.solver.sample_points(pts, NAMES)
    got = c.solver.sample_grid(NAMES, shape, lo, hi, cells=True)
    assert list(got) == NAMES + ["cell"]
    image = shape[::-1]
    for name in NAMES:
        assert tuple(got[name].shape) == ((3,) + image if name == "momentum" else image)
        assert bits_equal(host(got[name]).reshape(-1, pts.shape[0]), np.atleast_2d(host(want[name]))), name
    cells = host(got["cell"])
    assert cells.dtype == np.int32 and cells.shape == image
    assert np.array_equal(cells.reshape(-1), host(c.solver.locate(pts)))
    assert (cells == -1).any() and (cells >= 0).any()
    # the default box is the domain: no pixel is outside
    whole = c.solver.sample_grid("density", shape, cells=True, fill=SENTINEL)
    assert (host(whole["cell"]) >= 0).all() and "cell" not in c.solver.sample_grid("density", shape)
    assert bits_equal(host(whole["density"]).reshape(-1),
                      c.expected("density", sample.host_locate(c.part, pixel_centres(dim, shape, (0.0,) * dim, (1.0,) * dim)), SENTINEL))
    # a zero extent: empty tensors
    zero = c.solver.sample_grid(["momentum"], (0,) + shape[1:], cells=True)
    assert tuple(zero["momentum"].shape) == (3,) + image[:-1] + (0,) and zero["cell"].numel() == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
def test_slice_plane_on_a_cell_face(subgrid, dtype):
    """lo[2] == hi[2] == 0.375: a face of the level-3 cells of the refined box (and of every Subgrid cell), so the pixels
    there are ties in z"""
    c = case("refined-3d-periodic", subgrid, dtype)
    lo, hi, shape = (0.1, 0.05, 0.375), (0.93, 1.2, 0.375), (9, 7, 1)
    pts = pixel_centres(3, shape, lo, hi)
    assert np.all(pts[:, 2] == 0.375)
    cells = sample.host_locate(c.part, pts)
    boxes, edge, _ = ref.cell_boxes(c.part)
    held = cells[cells >= 0]
    assert (boxes[held, 2] == 0.375).any()                          # ties: the cell ABOVE the plane ...
    assert not (boxes[held, 2] + edge[held] == 0.375).any()         # ... never the one below
    got = c.solver.sample_grid(NAMES, shape, lo, hi, cells=True)
    assert np.array_equal(host(got["cell"]).reshape(-1), cells)
    want = c.solver.sample_points(pts, NAMES)
    for name in NAMES:
        assert bits_equal(host(got[name]).reshape(-1, pts.shape[0]), np.atleast_2d(host(want[name]))), name
    thick = c.solver.sample_grid(NAMES, (9, 7, 3), lo, hi)          # whatever its n
    for name in NAMES:
        for k in range(3):
            assert bits_equal(host(thick[name])[..., k, :, :], host(got[name])[..., 0, :, :]), name


# ---- 4: resample_uniform --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def brute_image(mesh, subgrid, dtype, level):
    c = case(mesh, subgrid, dtype)
    q = np.concatenate([c.values[name] for name in NAMES])
    sums, weights = ref.resample(c.part, q, level)
    assert np.all(weights > 0)
    return sums / weights


def split_planes(images):
    """{name: tensor} -> [planes, pixels...] numpy in the order of NAMES"""
    return np.concatenate([host(images[name]).reshape((-1,) + tuple(images["density"].shape)) for name in NAMES])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_resample_uniform_against_the_brute_force(mesh, subgrid, dtype):
    c = case(mesh, subgrid, dtype)
    dim = c.dim
    q = np.concatenate([c.values[name] for name in NAMES])
    scale = np.abs(q).max(axis=1)
    _, edge, level = ref.cell_boxes(c.part)
    vol = edge ** dim
    block_levels = set(np.unique(c.part.levels[:c.part.N]).tolist())
    if subgrid and mesh in ref.REFINED:                             # L below, at, one and two above a block's level
        assert any({l - 1, l, l + 1, l + 2} <= set(LEVELS[dim]) for l in block_levels), block_levels
    for L in LEVELS[dim]:
        got = c.solver.resample_uniform(NAMES, L)
        assert tuple(got["density"].shape) == (1 << L,) * dim and tuple(got["momentum"].shape) == (3,) + (1 << L,) * dim
        planes = split_planes(got)
        want = brute_image(mesh, subgrid, dtype, L)
        err = np.abs(planes - want).reshape(planes.shape[0], -1).max(axis=1)
        print(f"{mesh} subgrid={subgrid} L={L}: max error / max |q| = {(err / scale).max():.2e}")
        assert np.all(err <= TOL * scale), (L, err / scale)
        for k in (0, 4):                                            # density and energy: the integral is kept
            total, cells_total = planes[k].sum() * 0.5 ** (dim * L), (vol * q[k]).sum()
            assert abs(total - cells_total) <= TOL * scale[k], (L, k, total, cells_total)
        again = split_planes(c.solver.resample_uniform(NAMES, L))
        assert bits_equal(planes, again), L
    # at the finest cell level every pixel lies inside one cell: the image is sample_grid on that grid, bitwise
    fine = int(level.max())
    a = c.solver.resample_uniform(NAMES, fine, fill=SENTINEL)
    b = c.solver.sample_grid(NAMES, (1 << fine,) * dim)
    for name in NAMES:
        assert bits_equal(host(a[name]), host(b[name])), name
    with pytest.raises(ValueError):
        c.solver.resample_uniform(NAMES, sample.DEPTH + 1)


# ---- 5: three ranks in one process ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", ["refined-2d-periodic", "refined-3d-periodic"])
def test_three_ranks_merge_to_one_rank(mesh, subgrid, dtype):
    """the pointwise names: their values do not depend on the partition, so the merged result is the single-rank one bitwise"""
    names = CONSERVED + ["pressure"]
    c = case(mesh, subgrid, dtype)
    dim, shape, S = c.dim, GRID[c.dim], c.part.cells_per_element
    lo, hi = LO[:dim], HI[:dim]
    one_pts, one_grid = c.solver.sample_points(c.points, names), c.solver.sample_grid(names, shape, lo, hi)
    m, pixels = c.points.shape[0], int(np.prod(shape))
    claims_pts, claims_grid = np.zeros(m, np.int64), np.zeros(pixels, np.int64)
    merged_pts = {n: np.full(host(one_pts[n]).shape, np.nan) for n in names}
    merged_grid = {n: np.full((host(one_grid[n]).size // pixels, pixels), np.nan) for n in names}
    L = LEVELS[dim][0]
    sums, weights, rank_weights = 0.0, 0.0, []
    for r in range(3):
        part = ref.partition(mesh, subgrid, r, 3)
        assert part.G > 0
        gidx = np.concatenate([np.arange(part.first_global, part.first_global + part.N), part.ghost_global])
        cols = (gidx[:, None] * S + np.arange(S)[None, :]).reshape(-1)
        solver = make_solver(part, dtype, c.state[:, cols])
        mine = host(solver.locate(c.points)) >= 0
        claims_pts += mine
        got = solver.sample_points(c.points, names)
        grid = solver.sample_grid(names, shape, lo, hi, cells=True)
        mine_grid = host(grid["cell"]).reshape(-1) >= 0
        claims_grid += mine_grid
        for n in names:
            g = host(got[n])
            assert np.array_equal(~np.isnan(np.atleast_2d(g)).any(axis=0), mine), (r, n)      # `fill` exactly where not owned
            merged_pts[n][..., mine] = g[..., mine]
            g = host(grid[n]).reshape(-1, pixels)
            assert np.array_equal(~np.isnan(g).any(axis=0), mine_grid), (r, n)
            merged_grid[n][:, mine_grid] = g[:, mine_grid]
        s, w = solver.resample_uniform(names, L, partial=True)
        assert tuple(w.shape) == (1 << L,) * dim
        sums = sums + np.concatenate([host(s[n]).reshape((-1,) + tuple(w.shape)) for n in names])
        weights = weights + host(w)
        rank_weights.append(host(w))
    inside = c.want_cells >= 0
    assert np.array_equal(claims_pts, inside.astype(np.int64))      # no point claimed twice, none left out
    assert np.array_equal(claims_grid, (host(c.solver.locate(pixel_centres(dim, shape, lo, hi))) >= 0).astype(np.int64))
    for n in names:
        assert bits_equal(merged_pts[n], host(one_pts[n])), n
        assert bits_equal(merged_grid[n], host(one_grid[n]).reshape(-1, pixels)), n
    # the partial sums: the split cuts coarse pixels between ranks
    shared = sum((w > 0).astype(np.int64) for w in rank_weights)
    assert (shared >= 2).any() and np.all(weights == 0.5 ** (dim * L))
    one = c.solver.resample_uniform(names, L)
    want = np.concatenate([host(one[n]).reshape((-1,) + (1 << L,) * dim) for n in names])
    q = np.concatenate([c.values[n] for n in names])
    scale = np.abs(q).max(axis=1).reshape((-1,) + (1,) * dim)
    assert np.all(np.abs(sums / weights - want) <= TOL * scale)


# ---- 6: a side stream ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
def test_side_stream_gives_the_same_bits(subgrid):
    c = case("refined-2d-walls", subgrid, torch.float32)
    dim, shape = c.dim, GRID[c.dim]
    want = (c.solver.locate(c.points), c.solver.sample_points(c.points, NAMES), c.solver.sample_grid(NAMES, shape, LO[:dim], HI[:dim]),
            c.solver.resample_uniform(NAMES, 4))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = (c.solver.locate(c.points, stream=side), c.solver.sample_points(c.points, NAMES, stream=side),
           c.solver.sample_grid(NAMES, shape, LO[:dim], HI[:dim], stream=side), c.solver.resample_uniform(NAMES, 4, stream=side))
    side.synchronize()
    assert np.array_equal(host(got[0]), host(want[0]))
    for g, w in zip(got[1:], want[1:]):
        for name in NAMES:
            assert bits_equal(host(g[name]), host(w[name])), name


# ---- refusals and the C entry points -------------------------------------------------------------------------------------
def test_refusals():
    from t8gpu_amd.unstructured import PrismHexMesh
    part = PrismHexMesh(5).partition()
    curved = PlainSolver(part, torch.float64, mode="compat", state=perturbed_state(part, 11))
    with pytest.raises(TypeError):
        curved.locate(np.zeros((1, 3)))
    c = case("refined-2d-walls", False, torch.float64)
    s = sample.sampler(c.solver)
    assert sample.sampler(c.solver) is s                            # built once, kept on the solver
    lib = hip.lib()
    cells = torch.full((4,), 5, dtype=torch.int32, device="cuda")
    pts = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    bad = lib.t8gpu_hip_sample_locate(4, hip.C.c_size_t(4), hip.ptr(pts), hip.ptr(s.keys), hip.ptr(s.levels), s.N, 1, hip.ptr(cells),
                                      hip.stream_ptr())
    assert bad != 0                                                 # dim = 4: refused before any launch
    g = sample.SampleGrid()
    g.n[0], g.n[1] = 0, 8
    g.hi[0] = g.hi[1] = 1.0
    with pytest.raises(hip.T8gpuHipError):                          # a grid of size 0 is a launch error at the C entry
        hip.call("t8gpu_hip_sample_grid", torch.float64, 2, g, hip.ptr(s.keys), hip.ptr(s.levels), s.N, 1, 0, sample.SamplePlanes(),
                 hip.C.c_double(0.0), None, hip.ptr(cells), hip.stream_ptr())
    torch.cuda.synchronize()
    assert host(cells).tolist() == [5, 5, 5, 5]
