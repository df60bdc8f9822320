"""_meshes.scaled (a SynthMesh partition as the forest of a box that is not the unit cube) and the ground the GPU tests of
tests/test_gpu_scaled_geometry.py stand on, all on the CPU: the helper's arithmetic, what the tile planner makes of scaled and
stretched boxes, and how the oracle itself answers a change of length unit."""
import functools

import numpy as np
import pytest

import _meshes as M
import _oracle as O
from _gpu import perturbed_state
from t8gpu_amd import plan

SEED = 31
POW2 = [2.0 ** -12, 2.0 ** 9]
NON_DYADIC = [3.7, 1 / 3]
ROUNDING = {np.float64: 2e-15, np.float32: 1e-6}      # of max|u| after three steps: twice the worst measured (9e-16, 5e-7)
STRETCH = {"box2": [(1, 0.37)], "box3": [(1, 0.37, 2.9), (3.7, 3.7, 1.3)]}


# ---- the helper --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,s", [("box2", 3.7), ("box2", (1, 0.37)), ("box3", (1, 0.37, 2.9)), ("sbox2", 1 / 3), ("sbox3", 3.7)])
def test_scaled_arithmetic_against_the_provider_arrays(name, s):
    part = M.partition(name, periodic=False)
    q = M.scaled(part, s)
    dim = part.mesh.dim
    f = np.full(dim, float(s)) if np.isscalar(s) else np.asarray(s, np.float64)
    normals = np.asarray(part.normals).reshape(-1, part.normal_dim)
    # every face: the product of the factors of the axes it spans
    for axis in range(dim):
        on = np.abs(normals[:, axis]) == 1.0
        assert on.any()
        spans = np.prod([f[a] for a in range(dim) if a != axis])
        assert np.allclose(q.areas[on], part.areas[on] * spans, rtol=4e-16, atol=0)
    assert np.allclose(q.volumes, part.volumes * f.prod(), rtol=4e-16, atol=0)
    assert np.array_equal(q.centres[:, :dim], part.centres[:, :dim] * f) and np.array_equal(q.centres[:, dim:], part.centres[:, dim:])
    assert q.areas.dtype == q.volumes.dtype == q.centres.dtype == np.float64
    # the provider's own arrays are untouched, everything else IS the provider's
    assert np.array_equal(part.areas, M.partition(name, periodic=False).areas)
    for same in ("face_neighbors", "normals", "level_diff", "nb_offset", "boundary_kinds", "levels", "indices", "send_idx",
                 "ghost_global", "mesh"):
        assert getattr(q, same) is getattr(part, same), same
    assert (q.N, q.G, q.F, q.B, q.normal_dim, q.subgrid, q.cells_per_element) == (
        part.N, part.G, part.F, part.B, part.normal_dim, part.subgrid, part.cells_per_element)
    assert q.kh_initial_state() is part.kh_initial_state()
    # a Cartesian cell of a box: its volume is the product of its face areas over ... (2D: the two edges; 3D: sqrt of the three)
    fn = np.asarray(part.face_neighbors).reshape(-1)
    left = fn[0:2 * part.F:2]
    hanging = (np.asarray(part.level_diff)[:part.F] != 0) if part.subgrid else (part.levels[left] != part.levels[fn[1:2 * part.F:2]])
    own = np.flatnonzero((left < part.N) & ~hanging)[:64]
    for face in own:
        e, axis = left[face], int(np.abs(normals[face]).argmax())
        edge = q.volumes[e] / q.areas[face]
        assert np.isclose(edge, f[axis] * part.volumes[e] / part.areas[face], rtol=4e-15)


def test_a_power_of_two_scale_is_exact():
    part = M.partition("box3")
    for s in POW2:
        q = M.scaled(part, s)
        assert np.array_equal(q.areas, part.areas * s * s) and np.array_equal(q.volumes, part.volumes * s ** 3)


def test_scaled_refuses_what_has_no_answer():
    with pytest.raises(ValueError):
        M.scaled(M.partition("sbox2"), (1, 0.37))          # a stretched Subgrid block: no defined inner sub-face area
    with pytest.raises(ValueError):
        M.scaled(M.partition("box2"), (1, 0.37, 2.9))
    with pytest.raises(ValueError):
        M.scaled(M.partition("box2"), -1.0)

    class Skewed:
        def __init__(self, part):
            self.__dict__.update(part.__dict__)
            self.normals = np.array(part.normals)
            self.normals[:2] = np.sqrt(0.5)

    with pytest.raises(AssertionError):
        M.scaled(Skewed(M.partition("box2")), 3.7)


# ---- the planner -------------------------------------------------------------------------------------------------------------------
def census(part, **kw):
    h = plan.HostPlainPlan.from_partition(part, patches=True, **kw)
    return dict(tiles=h.ntiles, patches=h.n_patches, uniform=h.n_patches_uniform_volume, irregular=sum(h.n_irregular_class))


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("s", [1.0] + NON_DYADIC + POW2)
def test_an_isotropic_scale_keeps_the_plan_form(s, periodic):
    """256-element tiles, 512-face cap (the planner's defaults): the censuses of the unit mesh"""
    assert census(M.scaled(M.partition("box2", periodic=periodic), s)) == dict(tiles=22, patches=9, uniform=9, irregular=0)
    assert census(M.scaled(M.partition("box3", periodic=periodic), s)) == dict(tiles=32, patches=16, uniform=16, irregular=13)


@pytest.mark.parametrize("periodic", [True, False])
def test_a_per_axis_stretch_gives_no_patch_tile(periodic):
    """A patch carries ONE area: on a stretched box every element goes through the generic tiles. A planner that learns per-axis
    areas changes this test knowingly (and tests/test_gpu_scaled_geometry.py: test_stretched_boxes...)."""
    for name, tiles in (("box2", 20), ("box3", 42)):
        for s in STRETCH[name]:
            assert census(M.scaled(M.partition(name, periodic=periodic), s)) == dict(tiles=tiles, patches=0, uniform=0, irregular=0), (name, s)
            h = plan.HostPlainPlan.from_partition(M.scaled(M.partition(name, periodic=periodic), s), patches=True)
            assert h.patch_dim == 0 and not h.tile_patch.any()


# ---- the oracle under a change of length unit ---------------------------------------------------------------------------------------
def oracle_steps(name, s, dtype, kind, steps=3):
    base = M.partition(name)
    part = base if s is None else M.scaled(base, s)
    case = (O.SubgridCase if M.is_subgrid(name) else O.PlainCase)(part, dtype, state=_state(name))
    dt = 0.1 * 2.0 ** -(M.SHAPES[name][2] + (2 if M.is_subgrid(name) else 0)) * (1.0 if s is None else s)
    for _ in range(steps):
        case.iterate(dt, kind=kind)
    cells = part.N * part.cells_per_element
    return case.current()[:, :cells].copy(), (None if M.is_subgrid(name) else case.speed.copy())


@functools.lru_cache(maxsize=None)
def _state(name):
    return perturbed_state(M.partition(name), SEED)


@functools.lru_cache(maxsize=None)
def unit_run(name, dtype, kind):
    return oracle_steps(name, None, dtype, kind)


def rel(u, u0):
    return float((np.abs(u.astype(np.float64) - u0) / np.abs(u0).max(axis=1, keepdims=True)).max())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("name", ["box2", "box3", "sbox2", "sbox3"])
def test_oracle_under_a_power_of_two_scale(name, kind, dtype):
    """Lengths * s and dt * s with s a power of two: three steps give the bits of the unit run (states, and speed estimates on
    plain meshes) on box2, box3 and sbox2. 3D Subgrid (sbox3) is EXCLUDED from the invariance: the oracle takes the edge of a 3D
    block from the C library's cbrt(volume), and cbrt(2^27 v) need not be 2^9 cbrt(v) to the last bit (measured: fp64 at
    s = 2^9 moves by 7e-16 of max|u|; fp64 at 2^-12 and fp32 gave the unit bits). There the run is only asserted to stay within
    rounding of the unit run, the bound of test_oracle_under_a_non_dyadic_scale."""
    u0, sp0 = unit_run(name, dtype, kind)
    for s in POW2:
        u, sp = oracle_steps(name, s, dtype, kind)
        if name == "sbox3":
            assert rel(u, u0) < ROUNDING[dtype], (s, rel(u, u0))
            continue
        assert np.array_equal(u, u0), (s, rel(u, u0))
        assert sp is None or np.array_equal(sp, sp0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["box2", "box3", "sbox2", "sbox3"])
def test_oracle_under_a_non_dyadic_scale(name, dtype):
    """s = 3.7 and 1/3: the oracle moves by rounding only -- measured at most 9e-16 (fp64) and 5e-7 (fp32) of max|u| after
    three steps, asserted at twice that: TOL1 / TOL10 remain the bounds for GPU against oracle on the same scaled arrays."""
    for kind in (0, 1, 2):
        u0, _ = unit_run(name, dtype, kind)
        for s in NON_DYADIC:
            u, _ = oracle_steps(name, s, dtype, kind)
            assert not np.array_equal(u, u0)
            assert rel(u, u0) < ROUNDING[dtype], (kind, s, rel(u, u0))
