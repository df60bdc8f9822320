"""Far-field boundaries on the host side (no GPU): the ("farfield", k) side spec of the synthetic provider, the kinds it fills
and keeps through adaptation and partitioning, how the tile planner encodes far-field faces, and the per-side kinds of the
curved providers (PrismHexMesh, TetHexMesh)."""
import numpy as np
import pytest
import torch

from t8gpu_amd.fused import PlainPlan
from t8gpu_amd.solver import check_inflow_states
from t8gpu_amd.synth import SynthMesh, side_codes
from t8gpu_amd.unstructured import PrismHexMesh, TetHexMesh


def _side_of(part, b):
    """t8code face number (0 -x .. 5 +z) that boundary face b's normal points to"""
    n = np.asarray(part.normals).reshape(-1, part.normal_dim)[part.F + b]
    ax = int(np.flatnonzero(n != 0)[0])
    return 2 * ax + (1 if n[ax] > 0 else 0)


def _global_boundary(part):
    fn = np.asarray(part.face_neighbors)
    return {(part.first_global + int(fn[2 * part.F + b]), _side_of(part, b)): int(part.boundary_kinds[b]) for b in range(part.B)}


def test_side_codes_accept_farfield_states():
    for k in range(6):
        codes = side_codes(2, (("farfield", k), "outflow", "periodic", "periodic"))
        assert codes[0] == 10 + k
    assert list(side_codes(3, (("farfield", np.int64(5)), 0, "wall", ("farfield", 0), "periodic", "periodic"))) == [15, 2, 0, 10, -1, -1]


@pytest.mark.parametrize("bad", [("farfield", 6), ("farfield", -1), ("farfield", True), "farfield", ("farfield",),
                                 ["farfield", 0], ("farfield", 1.0), ("far", 0)])
def test_invalid_farfield_spellings_are_rejected(bad):
    with pytest.raises(ValueError):
        side_codes(2, (bad, "outflow", "periodic", "periodic"))
    with pytest.raises(ValueError):
        SynthMesh(2, 2, 3, sides=(bad, "outflow", "periodic", "periodic"))


@pytest.mark.parametrize("dim,sides", [(2, (("farfield", 0), ("farfield", 5), "periodic", "periodic")),
                                       (2, ("wall", ("farfield", 1), 3, "outflow")),
                                       (3, (("farfield", 2), "outflow", "periodic", "periodic", ("farfield", 0), "wall"))])
def test_farfield_kinds_follow_the_side_of_the_normal(dim, sides):
    m = SynthMesh(dim, 2, 4, band=0.1, sides=sides)
    codes = side_codes(dim, sides)
    assert np.array_equal(m.sides, codes)
    p = m.partition()
    seen = set()
    for b in range(p.B):
        s = _side_of(p, b)
        assert p.boundary_kinds[b] == codes[s]
        seen.add(int(p.boundary_kinds[b]))
    assert {c for c in codes if c >= 10} <= seen


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("by_rounds", [False, True])
def test_farfield_kinds_survive_adaptation(dim, by_rounds):
    sides = (("farfield", 1), ("farfield", 0), "periodic", "periodic") + ((("farfield", 2), "outflow") if dim == 3 else ())
    m = SynthMesh(dim, 2, 4, band=0.1, sides=sides)
    marks = m.marks_from_criteria(np.random.default_rng(5).uniform(0, 2, m.num_elements), 1.0, 1, 5)
    new, _ = m.adapt(marks, by_rounds=by_rounds)
    assert new.num_elements != m.num_elements and np.array_equal(new.sides, m.sides)
    p, codes = new.partition(), side_codes(dim, sides)
    assert p.B > 0 and any(k >= 10 for k in p.boundary_kinds)
    for b in range(p.B):
        assert p.boundary_kinds[b] == codes[_side_of(p, b)]


@pytest.mark.parametrize("dim", [2, 3])
def test_farfield_kinds_survive_partitioning(dim):
    sides = (("farfield", 3), 1, "periodic", "periodic") + ((("farfield", 0), "wall") if dim == 3 else ())
    m = SynthMesh(dim, 2, 4, band=0.1, sides=sides)
    whole = _global_boundary(m.partition())
    union = {}
    for r in range(3):
        d = _global_boundary(m.partition(r, 3))
        assert not set(d) & set(union)
        union.update(d)
    assert union == whole


def _plan(part, **kw):
    return PlainPlan.on_host(part, torch.float64, **kw).host


@pytest.mark.parametrize("dim,base,maxl,sides", [
    (2, 4, 7, (("farfield", 0), ("farfield", 5), "periodic", "periodic")),
    (2, 5, 7, ("wall", ("farfield", 2), 0, "outflow")),
    (3, 4, 5, (("farfield", 1), "outflow", "periodic", "periodic", "wall", ("farfield", 0)))])
def test_planner_encodes_farfield_faces_and_keeps_them_out_of_patches(dim, base, maxl, sides):
    part = SynthMesh(dim, base, maxl, band=0.12, sides=sides).partition()
    kinds = np.asarray(part.boundary_kinds).astype(np.int64)
    h = _plan(part, irregular=True)
    assert h.open_faces and h.farfield_faces
    r16 = h.face_lr >> 16
    bnd = r16 >= 0xFFF0
    orig = h.face_orig[bnd]
    want = np.where(kinds == 0, 0xFFFF, np.where(kinds == 1, 0xFFFE, np.where(kinds >= 10, 0xFFF8 + kinds - 10, 0xFFF0 + kinds - 2)))
    assert np.array_equal(r16[bnd], want[orig - part.F])
    assert np.any((r16 >= 0xFFF8) & (r16 <= 0xFFFD))
    assert h.n_patches > 0
    fn = np.asarray(part.face_neighbors)
    opened = set(int(e) for e in fn[2 * part.F:][kinds != 0])
    for t in np.flatnonzero(h.tile_patch):
        assert not set(range(int(h.elem_off[t]), int(h.elem_off[t + 1]))) & opened
    # a plan without far-field faces does not set the flag
    assert not _plan(SynthMesh(dim, base, maxl, band=0.12, sides=tuple(s if not isinstance(s, tuple) else "outflow" for s in sides)).partition()).farfield_faces


def test_kinds_of_16_and_above_are_refused():
    from t8gpu_amd.plan import HostPlainPlan
    part = SynthMesh(2, 3, 4, sides=("wall",) * 4).partition()
    args = (part.N, part.G, part.F, part.B, part.normal_dim, part.face_neighbors, part.normals, part.areas)
    HostPlainPlan(*args, boundary_kinds=np.full(part.B, 15, np.uint8))
    for k in (16, 17, 255):
        with pytest.raises(ValueError):
            HostPlainPlan(*args, boundary_kinds=np.full(part.B, k, np.uint8))


def test_farfield_plans_are_not_taken_by_the_persistent_kernel():
    part = SynthMesh(2, 7, 7, sides=(("farfield", 0), ("farfield", 0), "periodic", "periodic")).partition()
    walls = SynthMesh(2, 7, 7, periodic=False).partition()
    n = 100000
    assert PlainPlan._persistent_accepts(_plan(walls, patches=False), torch.float64, 0, n_generic=n)
    assert not PlainPlan._persistent_accepts(_plan(part, patches=False), torch.float64, 0, n_generic=n)


def test_farfield_states_are_required_and_counted():
    part = SynthMesh(2, 3, 4, sides=(("farfield", 2), "outflow", "periodic", "periodic")).partition()
    with pytest.raises(ValueError, match="required"):
        check_inflow_states(part, None)
    with pytest.raises(ValueError):
        check_inflow_states(part, np.tile([[1.0, 0, 0, 0, 2.5]], (2, 1)))
    assert check_inflow_states(part, np.tile([[1.0, 0, 0, 0, 2.5]], (3, 1))).shape == (3, 5)


# ---- curved providers ------------------------------------------------------------------------------------------------
CURVED_SIDES = ("wall", ("farfield", 0), ("farfield", 1), 0, "outflow", ("farfield", 0))


def _geometric_side(mesh):
    """side of the reference cube (0 -x .. 5 +z) of every boundary face of a shell_map mesh, recovered from the geometry: the
    outward normal at the centroid points along -e_r on the inner radius (0.6) and +e_r on the outer one (1.0), along -+e_theta
    on the two angular sides in (x, y) and along -+e_phi on the two in z"""
    c = mesh.face_centroid[mesh.F:]
    a = mesh.area_vec[mesh.F:]
    n = a / np.linalg.norm(a, axis=1, keepdims=True)
    r = np.linalg.norm(c, axis=1)
    th, ph = np.arctan2(c[:, 1], c[:, 0]), np.arcsin(c[:, 2] / r)
    e_r = c / r[:, None]
    e_th = np.stack([-np.sin(th), np.cos(th), 0 * th], 1)
    e_ph = np.stack([-np.sin(ph) * np.cos(th), -np.sin(ph) * np.sin(th), np.cos(ph)], 1)
    d = np.stack([(n * e).sum(1) for e in (e_r, e_th, e_ph)], 1)
    ax = np.argmax(np.abs(d), axis=1)
    dd = d[np.arange(ax.size), ax]
    assert np.abs(dd).min() > 0.9
    side = 2 * ax + (dd > 0)
    # ... and the radius of the two radial sides
    assert np.allclose(r[side == 0], 0.6, atol=0.05) and np.allclose(r[side == 1], 1.0, atol=0.05)   # (chords of the coarse cells)
    return side


@pytest.mark.parametrize("make", [lambda s: PrismHexMesh(6, split="checker", sides=s), lambda s: TetHexMesh(4, tets="blocks", sides=s)],
                         ids=["prism_hex", "tet_hex"])
def test_curved_kinds_match_the_geometric_side(make):
    m = make(CURVED_SIDES)
    side = _geometric_side(m)
    assert np.array_equal(side, m.boundary_side)
    codes = np.array([0, 10, 11, 2, 1, 10])
    assert np.array_equal(m.boundary_kinds, codes[side])
    p = m.partition()
    assert np.array_equal(p.boundary_kinds, m.boundary_kinds)


@pytest.mark.parametrize("make", [lambda s: PrismHexMesh((8, 6, 4), split=0.5, sides=s), lambda s: TetHexMesh((4, 4, 2), sides=s)],
                         ids=["prism_hex", "tet_hex"])
def test_curved_partition_gives_the_single_rank_kinds(make):
    m = make(CURVED_SIDES)
    whole = m.partition()
    fnw = np.asarray(whole.face_neighbors)
    ref = {(int(fnw[2 * whole.F + b]), tuple(np.round(whole.normals.reshape(-1, 3)[whole.F + b], 12))): int(whole.boundary_kinds[b])
           for b in range(whole.B)}
    union = {}
    for r in range(3):
        p = m.partition(r, 3)
        assert p.boundary_kinds.size == p.B
        fn = np.asarray(p.face_neighbors)
        for b in range(p.B):
            key = (p.first_global + int(fn[2 * p.F + b]), tuple(np.round(p.normals.reshape(-1, 3)[p.F + b], 12)))
            assert key not in union
            union[key] = int(p.boundary_kinds[b])
    assert union == ref


@pytest.mark.parametrize("cls,kw", [(PrismHexMesh, dict(n=5, split="checker")), (PrismHexMesh, dict(n=4, split="all", periodic=True)),
                                    (TetHexMesh, dict(n=3, tets="blocks"))])
def test_curved_meshes_without_sides_are_unchanged(cls, kw):
    a, b = cls(**kw), cls(**kw, sides=None)
    assert a.boundary_kinds is None and b.boundary_kinds is None
    for k in ("face_left", "face_right", "area_vec", "face_centroid", "volumes", "centres"):
        assert np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes(), k
    pa = a.partition()
    assert pa.boundary_kinds is None
    if not kw.get("periodic"):
        c = cls(**kw, sides=("wall",) * 6)
        for k in ("face_left", "face_right", "area_vec", "face_centroid", "volumes", "centres"):
            assert np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(c, k)).tobytes(), k
        assert not np.any(c.boundary_kinds)


def test_curved_sides_are_validated():
    for bad in [("wall",) * 5, ("periodic",) + ("wall",) * 5, (("farfield", 6),) + ("wall",) * 5, (8,) + ("wall",) * 5]:
        with pytest.raises(ValueError):
            PrismHexMesh(3, sides=bad)
        with pytest.raises(ValueError):
            TetHexMesh(2, sides=bad)
    with pytest.raises(ValueError):
        PrismHexMesh(3, periodic=True, sides=("wall",) * 6)
