"""Open boundaries on the host side (no GPU): the per-side boundary spec of the synthetic provider, the boundary_kinds
array it fills, and how the tile planner encodes open faces and keeps their cells out of patches."""
import numpy as np
import pytest
import torch

from t8gpu_amd.fused import PlainPlan
from t8gpu_amd.plan import HostPlainPlan
from t8gpu_amd.synth import SynthMesh, side_codes

SIDE_NAMES = ("-x", "+x", "-y", "+y", "-z", "+z")


def _side_of(part, b):
    """t8code face number (0 -x .. 5 +z) that boundary face b's normal points to"""
    n = np.asarray(part.normals).reshape(-1, part.normal_dim)[part.F + b]
    ax = int(np.flatnonzero(n != 0)[0])
    return 2 * ax + (1 if n[ax] > 0 else 0)


def _global_boundary(part):
    """{(global element, side): kind} over the partition's boundary faces"""
    fn = np.asarray(part.face_neighbors)
    out = {}
    for b in range(part.B):
        e = int(fn[2 * part.F + b])
        key = (part.first_global + e, _side_of(part, b))
        assert key not in out
        out[key] = int(part.boundary_kinds[b])
    return out


@pytest.mark.parametrize("dim", [2, 3])
def test_periodic_and_wall_sides_reproduce_the_old_meshes(dim):
    for periodic, name in ((True, "periodic"), (False, "wall")):
        a = SynthMesh(dim, 2, 4, band=0.1, periodic=periodic).partition()
        b = SynthMesh(dim, 2, 4, band=0.1, sides=(name,) * (2 * dim)).partition()
        assert (a.N, a.G, a.F, a.B) == (b.N, b.G, b.F, b.B)
        for k in ("face_neighbors", "normals", "areas", "levels", "volumes", "centres"):
            assert np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes(), k
        assert a.boundary_kinds.size == a.B and not np.any(a.boundary_kinds)
        assert np.array_equal(a.boundary_kinds, b.boundary_kinds)


@pytest.mark.parametrize("dim,sides", [(2, (0, "outflow", "periodic", "periodic")),
                                       (2, ("outflow", "wall", 3, "outflow")),
                                       (3, (1, "outflow", "periodic", "periodic", "wall", "wall"))])
def test_boundary_kinds_follow_the_side_of_the_normal(dim, sides):
    m = SynthMesh(dim, 2, 4, band=0.1, sides=sides)
    codes = side_codes(dim, sides)
    assert np.array_equal(m.sides, codes)
    p = m.partition()
    assert p.B > 0 and p.boundary_kinds.dtype == np.uint8
    seen = set()
    for b in range(p.B):
        s = _side_of(p, b)
        assert codes[s] >= 0, f"boundary face on periodic side {SIDE_NAMES[s]}"
        assert p.boundary_kinds[b] == codes[s]
        seen.add(s)
    assert seen == {s for s in range(2 * dim) if codes[s] >= 0}


def test_invalid_sides_are_rejected():
    with pytest.raises(ValueError, match="paired"):
        SynthMesh(2, 2, 3, sides=("periodic", "outflow", "periodic", "periodic"))
    with pytest.raises(ValueError, match="paired"):
        SynthMesh(3, 2, 3, sides=("outflow",) * 4 + ("wall", "periodic"))
    for bad in [("outflow",) * 3, ("outflow", "outflow", "open", "wall"), ("outflow", "outflow", 8, "wall"),
                ("outflow", "outflow", -1, "wall"), ("outflow", "outflow", True, "wall")]:
        with pytest.raises(ValueError):
            SynthMesh(2, 2, 3, sides=bad)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("by_rounds", [False, True])
def test_kinds_survive_adaptation(dim, by_rounds):
    sides = (2, "outflow", "periodic", "periodic") + (("wall", "outflow") if dim == 3 else ())
    m = SynthMesh(dim, 2, 4, band=0.1, sides=sides)
    rng = np.random.default_rng(3)
    marks = m.marks_from_criteria(rng.uniform(0, 2, m.num_elements), 1.0, 1, 5)
    new, _ = m.adapt(marks, by_rounds=by_rounds)
    assert new.num_elements != m.num_elements
    assert np.array_equal(new.sides, m.sides)
    p = new.partition()
    codes = side_codes(dim, sides)
    assert p.B > 0
    for b in range(p.B):
        assert p.boundary_kinds[b] == codes[_side_of(p, b)]
    if not by_rounds:    # the two adaptation procedures give the same forest, so the same kinds
        q = m.adapt(marks, by_rounds=True)[0].partition()
        assert np.array_equal(p.boundary_kinds, q.boundary_kinds)


@pytest.mark.parametrize("dim", [2, 3])
def test_kinds_survive_partitioning(dim):
    sides = (4, "outflow", "periodic", "periodic") + (("outflow", "wall") if dim == 3 else ())
    m = SynthMesh(dim, 2, 4, band=0.1, sides=sides)
    whole = _global_boundary(m.partition())
    union = {}
    for r in range(3):
        part = m.partition(r, 3)
        assert part.boundary_kinds.size == part.B
        d = _global_boundary(part)
        assert not set(d) & set(union)
        union.update(d)
    assert union == whole


def _plan(part, **kw):
    return PlainPlan.on_host(part, torch.float64, **kw).host


def _open_elements(part):
    fn = np.asarray(part.face_neighbors)
    return set(int(e) for e in fn[2 * part.F:][np.asarray(part.boundary_kinds) != 0])


@pytest.mark.parametrize("dim,base,maxl,sides", [
    (2, 4, 7, ("outflow", 1, "periodic", "periodic")),
    (2, 5, 7, ("wall", "outflow", 0, "wall")),
    (3, 4, 5, (0, "outflow", "periodic", "periodic", "wall", "wall")),
    (3, 4, 4, ("outflow", "wall", "wall", 2, "periodic", "periodic"))])
def test_planner_encodes_open_faces_and_keeps_them_out_of_patches(dim, base, maxl, sides):
    part = SynthMesh(dim, base, maxl, band=0.12, sides=sides).partition()
    kinds = np.asarray(part.boundary_kinds)
    h = _plan(part, irregular=True)
    assert h.open_faces
    r16 = h.face_lr >> 16
    bnd = r16 >= 0xFFF0
    orig = h.face_orig[bnd]
    assert np.all(orig >= part.F), "a boundary code on an interior face"
    want = np.where(kinds == 0, 0xFFFF, np.where(kinds == 1, 0xFFFE, 0xFFF0 + kinds.astype(np.int64) - 2))
    assert np.array_equal(r16[bnd], want[orig - part.F])
    # every open face is in exactly one generic tile (walls may sit in patches instead)
    open_ids = np.flatnonzero(kinds != 0) + part.F
    assert np.array_equal(np.sort(orig[r16[bnd] != 0xFFFF]), open_ids)
    # no patch tile holds a cell with an open face
    assert h.n_patches > 0, "the mesh should still have patches away from the open sides"
    opened = _open_elements(part)
    for t in np.flatnonzero(h.tile_patch):
        cells = set(range(int(h.elem_off[t]), int(h.elem_off[t + 1])))
        assert not cells & opened
    if dim == 3:   # (irregular 3D patches take wall cells: the same mesh with walls where these sides are open has more)
        walled = tuple("wall" if s not in ("periodic", "wall") else s for s in sides)
        hw = _plan(SynthMesh(dim, base, maxl, band=0.12, sides=walled).partition(), irregular=True)
        assert hw.n_patches > h.n_patches


@pytest.mark.parametrize("dim,base,maxl", [(2, 5, 6), (3, 4, 5)])
def test_wall_mesh_plans_identically_through_both_entry_points(dim, base, maxl):
    part = SynthMesh(dim, base, maxl, band=0.1, periodic=False).partition()
    args = (part.N, part.G, part.F, part.B, part.normal_dim, part.face_neighbors, part.normals, part.areas)
    kw = dict(patches=True, volumes=part.volumes, irregular=True)
    a = HostPlainPlan(*args, **kw)
    b = HostPlainPlan(*args, boundary_kinds=np.zeros(part.B, np.uint8), **kw)
    assert not a.open_faces and not b.open_faces
    for k in HostPlainPlan.FIELDS + ("ell", "geo_idx", "geo_table", "tile_desc", "tile_patch"):
        assert np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes(), k
    assert (a.ntiles, a.n_patch_class, a.n_irregular_class) == (b.ntiles, b.n_patch_class, b.n_irregular_class)


def test_open_plans_are_not_taken_by_the_persistent_kernel():
    part = SynthMesh(2, 7, 7, sides=("outflow", "outflow", "periodic", "periodic")).partition()
    walls = SynthMesh(2, 7, 7, periodic=False).partition()
    h_open, h_wall = _plan(part, patches=False), _plan(walls, patches=False)
    assert h_open.open_faces and not h_wall.open_faces
    n = 100000    # (a tile count at which the persistent kernel takes a plan)
    assert PlainPlan._persistent_accepts(h_wall, torch.float64, 0, n_generic=n)
    assert not PlainPlan._persistent_accepts(h_open, torch.float64, 0, n_generic=n)
