"""Brute-force reference of the sampling tests (test_sample_host.py, test_gpu_sample.py): cell boxes from `centres` and
`levels`, containment and overlap box by box. It knows nothing of Morton keys, searches or index ranges.

Meshes. `refined` and `check_mesh_conditions` are those of test_gpu_fields.py: a uniform mesh with a box of elements (and
element 0, at the periodic wrap) refined once has 2:1 faces along every axis in both orientations and an element count above
64 that is no multiple of 64; the conditions are asserted for these meshes, so a mesh change cannot hide a case.
SynthMesh(2, 3, 6, band=0.1) refines in bands of y only and has 2368 = 37 * 64 elements: it is here for its three levels and
its size (a search of twelve rounds), not for those conditions."""
import functools

import numpy as np

from t8gpu_amd.synth import SynthMesh


def refined(dim, level, periodic, lo, hi):
    """a uniform mesh with the elements whose centres lie in the box (lo, hi)^dim, and element 0, refined once"""
    mesh = SynthMesh(dim, level, level, periodic=periodic)
    part = mesh.partition()
    c = part.centres[: part.N, :dim]
    marks = np.all((c > lo) & (c < hi), axis=1).astype(np.int8)
    marks[0] = 1
    return mesh.adapt(marks)[0]


MESHES = {
    "refined-2d-periodic": lambda: refined(2, 3, True, 0.3, 0.8),
    "refined-2d-walls": lambda: refined(2, 3, False, 0.3, 0.8),
    "refined-3d-periodic": lambda: refined(3, 2, True, 0.2, 0.8),
    "band-2d": lambda: SynthMesh(2, 3, 6, band=0.1),
}
REFINED = [m for m in MESHES if m.startswith("refined")]
SIZES = {"refined-2d-periodic": 115, "refined-2d-walls": 115, "refined-3d-periodic": 127, "band-2d": 2368}


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    mesh = MESHES[name]()
    assert mesh.num_elements == SIZES[name]
    return mesh


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
        assert part.N % 4 != 0
    periodic = bool(np.all(part.mesh.sides == -1))
    assert (part.B == 0) if periodic else (part.B > 0)


@functools.lru_cache(maxsize=None)
def partition(mesh, subgrid, rank=0, nranks=1):
    part = mesh_of(mesh).partition(rank, nranks, subgrid=subgrid)
    if mesh in REFINED and nranks == 1:
        check_mesh_conditions(part)
    return part


def cell_boxes(part, subgrid=None):
    """(lo[cells, dim], edge[cells], level[cells]) of the owned cells in storage order; the subcells of a Subgrid block from
    their in-block index i + 4 j (+ 16 k)"""
    subgrid = part.subgrid if subgrid is None else subgrid
    dim, N = part.mesh.dim, part.N
    level = part.levels[:N].astype(np.int64)
    edge = 0.5 ** level.astype(np.float64)
    lo = part.centres[:N, :dim] - 0.5 * edge[:, None]
    if not subgrid:
        return lo, edge, level
    S = 4 ** dim
    c = np.arange(S)
    off = np.stack([(c >> (2 * a)) & 3 for a in range(dim)], axis=1).astype(np.float64)          # [S, dim]
    lo = lo[:, None, :] + off[None, :, :] * (edge[:, None, None] / 4)
    return lo.reshape(-1, dim), np.repeat(edge / 4, S), np.repeat(level + 2, S)


def locate(part, points, subgrid=None, chunk=512):
    """int32[M]: the cell with lo <= x < hi on every axis, by testing every cell box; -1 when there is none. Asserts that no
    point lies in two boxes."""
    lo, edge, _ = cell_boxes(part, subgrid)
    hi = lo + edge[:, None]
    pts = np.asarray(points, np.float64).reshape(-1, lo.shape[1])
    out = np.full(pts.shape[0], -1, np.int32)
    with np.errstate(invalid="ignore"):
        for a in range(0, pts.shape[0], chunk):
            p = pts[a:a + chunk, None, :]
            inside = np.all((lo[None] <= p) & (p < hi[None]), axis=2)          # [chunk, cells]
            count = inside.sum(axis=1)
            assert count.max(initial=0) <= 1
            out[a:a + chunk] = np.where(count == 1, inside.argmax(axis=1), -1)
    return out


def resample(part, values, level, subgrid=None):
    """(sums[planes, pixels...], weights[pixels...]) of values[planes, cells] on the 2^level pixels per axis (shape [ny, nx]
    or [nz, ny, nx]): per pixel the sum of overlap volume times value, and of overlap volume, over all cell boxes"""
    lo, edge, _ = cell_boxes(part, subgrid)
    dim, n = lo.shape[1], 1 << level
    plo = np.arange(n) / n
    ov = []                                                             # per axis [pixels, cells]: overlap length
    for a in range(dim):
        left = np.maximum(plo[:, None], lo[None, :, a])
        right = np.minimum(plo[:, None] + 1.0 / n, lo[None, :, a] + edge[None, :])
        ov.append(np.maximum(right - left, 0.0))
    q = np.asarray(values, np.float64)
    if dim == 2:
        return np.einsum("yc,xc,pc->pyx", ov[1], ov[0], q), np.einsum("yc,xc->yx", ov[1], ov[0])
    return np.einsum("zc,yc,xc,pc->pzyx", ov[2], ov[1], ov[0], q), np.einsum("zc,yc,xc->zyx", ov[2], ov[1], ov[0])


def point_set(part, seed, m=1003, subgrid=None, max_cells=256):
    """(points[M, dim], classes): m uniform random points plus the special points, classes = {name: slice of points}.
    "corner" / "face" / "upper" points come from up to max_cells cells chosen by seed: the lower corner of a cell (a tie
    in every axis: the cell itself), the middle of its lower x face, and per axis the middle of its upper face (the
    neighbour across, at a 2:1 face too, or outside the domain)."""
    lo, edge, _ = cell_boxes(part, subgrid)
    dim = lo.shape[1]
    rng = np.random.default_rng(seed)
    pick = np.sort(rng.choice(lo.shape[0], min(max_cells, lo.shape[0]), replace=False))
    mid = lo[pick] + 0.5 * edge[pick, None]
    face = mid.copy()
    face[:, 0] = lo[pick, 0]
    upper = []
    for a in range(dim):
        u = mid.copy()
        u[:, a] = lo[pick, a] + edge[pick]
        upper.append(u)
    inside_edge = np.full((3, dim), 0.3)
    inside_edge[0, 0], inside_edge[1, dim - 1] = 0.0, np.nextafter(1.0, 0.0)
    inside_edge[2] = 0.0                                                # (the origin)
    outside = np.full((2 * dim, dim), 0.4)
    for a in range(dim):
        outside[2 * a, a], outside[2 * a + 1, a] = 1.0, -1e-300
    bad = np.full((3, dim), 0.6)
    bad[0, 0], bad[1, dim - 1], bad[2, 0] = np.nan, np.inf, 1e300
    groups = {"random": rng.uniform(0.0, 1.0, (m, dim)), "corner": lo[pick], "face": face, "upper": np.concatenate(upper),
              "inside_edge": inside_edge, "outside": outside, "bad": bad}
    classes, start = {}, 0
    for name, g in groups.items():
        classes[name] = slice(start, start + g.shape[0])
        start += g.shape[0]
    classes["pick"] = pick
    return np.concatenate(list(groups.values())), classes
