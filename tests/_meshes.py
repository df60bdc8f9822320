"""Fixture meshes refined across EVERY axis, and the censuses that prove it (CPU only).

SynthMesh(dim, base, max, band=...) refines in bands around 0.25 and 0.75 of the LAST coordinate only: its hanging faces all
have that normal, its patches meet coarser elements across that axis only. The shapes here are built by repeated
SynthMesh.adapt from a uniform mesh, refined inside boxes, bands and corners aligned to 16-cell (2D) / 8-cell (3D) boundaries,
so that whole patches lie against a level interface in x, y and z. Anything orientation-dependent is tested on these."""
import functools

import numpy as np

from t8gpu_amd.synth import SynthMesh


def refined_where(dim, base, finest, inside, periodic=True, sides=None):
    """A uniform level-`base` mesh refined `finest - base` times where inside(centres[n, 3]) holds (2:1 balance by adapt)."""
    mesh = SynthMesh(dim, base, finest, band=0.0, periodic=periodic, sides=sides)
    for _ in range(finest - base):
        part = mesh.partition()
        marks = (np.asarray(inside(part.centres[:part.N]), bool) & (part.levels[:part.N] < finest)).astype(np.int8)
        mesh, _ = mesh.adapt(marks)
    return mesh


def _box(lo, hi, dim):
    return lambda c: np.all((c[:, :dim] >= lo) & (c[:, :dim] < hi), axis=1)


# name -> (dim, base, finest, inside, subgrid); walled / sides variants through the arguments of shape()
SHAPES = {
    "box2": (2, 4, 7, _box(0.25, 0.75, 2), False),
    "xband2": (2, 4, 7, _box(0.25, 0.75, 1), False),
    "corner2": (2, 4, 7, _box(0.0, 0.25, 2), False),
    "box3": (3, 3, 5, _box(0.25, 0.75, 3), False),
    "corner3": (3, 3, 5, _box(0.0, 0.5, 3), False),
    "sbox2": (2, 3, 5, _box(0.25, 0.75, 2), True),
    "sbox3": (3, 2, 4, _box(0.25, 0.75, 3), True),
    "scorner3": (3, 2, 4, _box(0.0, 0.3, 3), True),
}


@functools.lru_cache(maxsize=None)
def shape(name, periodic=True, sides=None):
    """The named mesh (cached: a mesh is never changed by its users). `sides` as SynthMesh takes it (a tuple)."""
    dim, base, finest, inside, _ = SHAPES[name]
    return refined_where(dim, base, finest, inside, periodic=periodic, sides=sides)


def is_subgrid(name):
    return SHAPES[name][4]


def partition(name, rank=0, nranks=1, periodic=True, sides=None):
    return shape(name, periodic, sides).partition(rank, nranks, subgrid=is_subgrid(name))


class Scaled:
    """A partition of the box [0, s_x] x [0, s_y] (x [0, s_z]) with the connectivity of `part` (see scaled): its own areas,
    volumes and centres; every other attribute is the one of `part`."""

    def __init__(self, part, s):
        dim = part.mesh.dim
        s = np.asarray(s, np.float64)
        if s.ndim == 0:
            s = np.full(dim, float(s))
        elif part.subgrid:
            raise ValueError("a Subgrid block has one inner sub-face area, derived from its volume: no per-axis stretch")
        if s.shape != (dim,) or not (s > 0).all():
            raise ValueError(f"one positive factor, or one per axis of a {dim}D mesh")
        normals = np.asarray(part.normals, np.float64).reshape(part.F + part.B, part.normal_dim)
        axis = np.abs(normals).argmax(1)
        assert (np.abs(normals[np.arange(axis.size), axis]) == 1.0).all() and (np.abs(normals).sum(1) == 1.0).all() and (axis < dim).all()
        self._part, self.scale = part, s
        self.areas = np.asarray(part.areas, np.float64) * (s.prod() / s[axis])
        self.volumes = np.asarray(part.volumes, np.float64) * s.prod()
        self.centres = np.asarray(part.centres, np.float64).copy()
        self.centres[:, :dim] *= s

    def __getattr__(self, name):
        return getattr(self.__dict__["_part"], name)


def scaled(part, s):
    """`part` (a SynthMesh partition: Cartesian, unit square / cube) as the same forest of a box with the edge lengths `s` (one
    factor, or one per axis): areas[f] * prod(s) / s[axis of f], volumes * prod(s), centres * s; connectivity, normals, the 2:1
    maps, boundary kinds, halo arrays, mesh and initial state are those of `part`. Every normal must be an exact axis normal.
    Subgrid partitions take a single factor only (ValueError otherwise): the reference derives the area of a block's inner
    sub-faces from its volume, so a stretched block has no defined answer."""
    return Scaled(part, s)


def _interior_faces(part):
    """(left, right, axis, positive, hanging) of the F interior faces"""
    F, dim = part.F, part.mesh.dim
    fn = np.asarray(part.face_neighbors, np.int64).reshape(-1)
    left, right = fn[0:2 * F:2], fn[1:2 * F:2]
    normals = np.asarray(part.normals, np.float64).reshape(part.F + part.B, part.normal_dim)[:F, :dim]
    axis = np.abs(normals).argmax(1)
    positive = normals[np.arange(F), axis] > 0
    if part.subgrid:
        hanging = np.asarray(part.level_diff).reshape(-1)[:F] != 0
    else:
        hanging = part.levels[left] != part.levels[right]
    return left, right, axis, positive, hanging


def hanging_census(part):
    """{(axis, sign): count} of the hanging interior faces by the axis and sign (+1 / -1) of their stored normal. Plain
    partitions: the levels of the two elements differ; Subgrid partitions: level_diff != 0."""
    _, _, axis, positive, hanging = _interior_faces(part)
    return {(a, s): int((hanging & (axis == a) & (positive == (s > 0))).sum()) for a in range(part.mesh.dim) for s in (1, -1)}


def hanging_by_axis(part):
    c = hanging_census(part)
    return [c[(a, 1)] + c[(a, -1)] for a in range(part.mesh.dim)]


def ghost_hanging_faces(part, axis=0):
    """number of hanging faces with normal `axis` one of whose two elements is a ghost (index >= N)"""
    left, right, ax, _, hanging = _interior_faces(part)
    return int((hanging & (ax == axis) & ((left >= part.N) | (right >= part.N))).sum())


SIDES2 = ("-x", "+x", "-y", "+y")
SIDES3 = ("-x", "+x", "-y", "+y", "-z", "+z")


def _patch_tiles(host_plan):
    """(tile index, halo segment start, is irregular) of every patch tile"""
    pos_of = np.empty(host_plan.ntiles, np.int64)
    pos_of[host_plan.tile_order] = np.arange(host_plan.ntiles)
    for t in np.flatnonzero(host_plan.tile_patch):
        flags = int(host_plan.tile_desc[pos_of[t], 5])
        yield int(t), int(host_plan.halo_off[t]), bool(flags & 0x800)


def patch_coarse_sides(host_plan, part):
    """{side: number of patches with a coarser element across it} from the halo_ids segments of the patch tiles:
    2D [-x 16 | +x 16 | -y 16 | +y 16], 3D [-x 32 | +x 32 | -y 32 | +y 32 | -z 64 | +z 64]."""
    if host_plan.patch_dim == 3:
        names, seg = SIDES3, (0, 32, 64, 96, 128, 192, 256)
    else:
        names, seg = SIDES2, (0, 16, 32, 48, 64)
    out = dict.fromkeys(names, 0)
    levels = np.asarray(part.levels)
    for t, h0, _ in _patch_tiles(host_plan):
        own = levels[host_plan.elem_off[t]]
        for k, name in enumerate(names):
            ids = host_plan.halo_ids[h0 + seg[k]:h0 + seg[k + 1]]
            ids = ids[(ids >= 0) & (ids < levels.size)]
            out[name] += int(ids.size > 0 and (levels[ids] < own).any())
    return out


def tile_kind_of_elements(host_plan):
    """per owned element: "patch", "irregular patch" or "generic" """
    kind = np.full(host_plan.N, "generic", dtype=object)
    for t, _, irregular in _patch_tiles(host_plan):
        kind[host_plan.elem_off[t]:host_plan.elem_off[t + 1]] = "irregular patch" if irregular else "patch"
    return kind


def block_kind_of_elements(host_subgrid_plan, part):
    """per owned block: "family" or "single block" """
    dim = part.mesh.dim
    fam_rec, _ = host_subgrid_plan.family_records(part.areas, 8)
    kind = np.full(part.N, "single block", dtype=object)
    for q in range(host_subgrid_plan.n_families):
        e0 = int(fam_rec[q][0])
        kind[e0:e0 + 2 ** dim] = "family"
    return kind


def worst_cell_report(part, got, want, host_plan=None):
    """What a failing parity check says: the worst cell's index, level and tile kind (patch, irregular patch, generic, family,
    single block) and the axis and sign of the hanging faces of its element, seen from it (+: across its + side)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.maximum(np.abs(want).max(axis=1, keepdims=True), 1e-300)
    err = np.where(np.isnan(got), np.inf, np.abs(got - want) / scale)
    var, cell = np.unravel_index(int(err.argmax()), err.shape)
    S = part.cells_per_element
    e = int(cell) // S
    left, right, axis, positive, hanging = _interior_faces(part)
    sides = []
    for f in np.flatnonzero(hanging & ((left == e) | (right == e))):
        outward_positive = bool(positive[f]) == (int(left[f]) == e)
        other = int(right[f]) if int(left[f]) == e else int(left[f])
        finer = "finer" if part.levels[other] > part.levels[e] else "coarser"
        sides.append(f"{'+' if outward_positive else '-'}{'xyz'[axis[f]]}({finer})")
    kind = "?"
    if host_plan is not None:
        kind = (block_kind_of_elements(host_plan, part) if part.subgrid else tile_kind_of_elements(host_plan))[e]
    return (f"worst cell {int(cell)} (element {e}, subcell {int(cell) % S}) variable {int(var)}: err {err[var, cell]:.3e}, "
            f"level {int(part.levels[e])}, centre {part.centres[e].tolist()}, kind {kind}, hanging faces {sorted(set(sides)) or 'none'}; "
            f"{int((err.max(axis=0) > 0).sum())} cells differ")
