"""The fixture meshes of tests/_meshes.py have what the GPU tests on them rely on: hanging faces with every normal, patches
with coarser elements across x AND y (AND z), Subgrid plans with families and single blocks. The band meshes do not, and the
census can tell: the negative control at the end."""
import numpy as np
import pytest

import _meshes as M
from t8gpu_amd.plan import HostPlainPlan, HostSubgridPlan
from t8gpu_amd.synth import SynthMesh

# (name, periodic). Walled corner shapes have their fine cells on the - walls: every level interface faces +, so the census is
# asked per axis there; xband2 is refined in a band of x alone (the transpose of the band meshes): no hanging face with normal y.
BOTH_SIGNS = [("box2", True), ("box2", False), ("corner2", True), ("box3", True), ("box3", False), ("sbox2", True), ("sbox3", True),
              ("scorner3", True)]
PER_AXIS = [("corner2", False), ("corner3", False), ("scorner3", False)]


@pytest.mark.parametrize("name,periodic", BOTH_SIGNS + PER_AXIS)
def test_hanging_faces_with_every_normal(name, periodic):
    part = M.partition(name, periodic=periodic)
    census = M.hanging_census(part)
    assert set(census) == {(a, s) for a in range(part.mesh.dim) for s in (1, -1)}
    if (name, periodic) in BOTH_SIGNS:
        assert all(n > 0 for n in census.values()), census
    else:
        assert all(n > 0 for n in M.hanging_by_axis(part)), census
        assert all(census[(a, -1)] == 0 for a in range(part.mesh.dim)), census


def test_xband2_is_the_transpose_of_a_band_mesh():
    census = M.hanging_census(M.partition("xband2"))
    assert census[(0, 1)] > 0 and census[(0, -1)] > 0 and census[(1, 1)] == census[(1, -1)] == 0


@pytest.mark.parametrize("name,periodic,sides", [("box2", True, ("+x", "+y")), ("box2", False, ("+x", "+y")), ("corner2", True, ("+x", "+y")),
                                                 ("corner2", False, ("+x", "+y")), ("xband2", True, ("+x",)),
                                                 ("box3", True, M.SIDES3), ("box3", False, M.SIDES3),
                                                 ("corner3", False, ("+x", "+y", "+z"))])
def test_patches_meet_coarser_elements_across_the_named_sides(name, periodic, sides):
    """2D patches: a coarser element across +x and +y (a block with one across a - side is no patch); 3D: across all six
    sides (the irregular form), walled corner: the three + sides (its - sides are walls). With the caps of a small mesh's
    device plan."""
    part = M.partition(name, periodic=periodic)
    plan = HostPlainPlan.from_partition(part, tmax=128, fcap=256, patches=True)
    coarse = M.patch_coarse_sides(plan, part)
    assert plan.n_patches > 0 and plan.n_patches < plan.ntiles
    assert all(coarse[s] > 0 for s in sides), coarse
    if name == "xband2":
        assert coarse["+y"] == coarse["-y"] == 0
    if part.mesh.dim == 3:
        n_irr = sum(plan.n_irregular_class)
        assert 0 < n_irr < plan.n_patches          # regular and irregular patches side by side
        kinds = M.tile_kind_of_elements(plan)
        assert {"patch", "irregular patch", "generic"} == set(kinds)


def test_corner2_has_fine_cells_on_the_minus_walls_and_across_the_wrap():
    walled, periodic = M.partition("corner2", periodic=False), M.partition("corner2")
    finest = walled.mesh.finest_level
    fn = np.asarray(walled.face_neighbors).reshape(-1)
    on_wall = fn[2 * walled.F:]
    nrm = np.asarray(walled.normals).reshape(-1, walled.normal_dim)[walled.F:]
    for axis in (0, 1):
        assert (walled.levels[on_wall[nrm[:, axis] < 0]] == finest).any()
    # periodic: the fine corner meets the coarse far side across the wrap -- hanging faces the walled mesh does not have
    assert sum(M.hanging_by_axis(periodic)) > sum(M.hanging_by_axis(walled))


@pytest.mark.parametrize("name,periodic", [("sbox2", True), ("sbox3", True), ("scorner3", True), ("scorner3", False)])
def test_subgrid_plans_have_families_and_single_blocks(name, periodic):
    part = M.partition(name, periodic=periodic)
    plan = HostSubgridPlan(part)
    assert plan.n_families > 0 and plan.n_rest > 0
    assert 2 ** part.mesh.dim * plan.n_families + plan.n_rest == part.N
    assert set(M.block_kind_of_elements(plan, part)) == {"family", "single block"}


def test_the_band_meshes_refine_across_the_last_axis_only():
    """The negative control: the provider's own band meshes have no hanging face with normal x (2D) or x, y (3D), and no
    patch of theirs meets a coarser element across +x."""
    part = SynthMesh(2, 4, 8, band=0.12).partition()
    assert M.hanging_by_axis(part)[0] == 0 and M.hanging_by_axis(part)[1] > 0
    plan = HostPlainPlan.from_partition(part, tmax=128, fcap=256, patches=True)
    coarse = M.patch_coarse_sides(plan, part)
    assert plan.n_patches > 0 and coarse["+x"] == coarse["-x"] == 0 and coarse["+y"] > 0
    part3 = SynthMesh(3, 3, 5, band=0.1).partition()
    assert M.hanging_by_axis(part3)[:2] == [0, 0] and M.hanging_by_axis(part3)[2] > 0
    sub = SynthMesh(3, 3, 4, band=0.03).partition(subgrid=True)
    assert M.hanging_by_axis(sub)[:2] == [0, 0] and M.hanging_by_axis(sub)[2] > 0


def test_partitions_cut_through_x_oriented_level_interfaces():
    """What the partitioned GPU runs rely on: some rank has a ghost across a hanging face with normal x. The 3-way split of
    box2 and sbox2 cuts inside the fine box and along its symmetry lines only (no such ghost); their 5-way split has them."""
    for name, world in (("box3", 3), ("sbox3", 3), ("xband2", 3), ("box2", 5), ("sbox2", 5)):
        assert sum(M.ghost_hanging_faces(M.partition(name, r, world)) for r in range(world)) > 0, (name, world)
    for name in ("box2", "sbox2"):
        assert sum(M.ghost_hanging_faces(M.partition(name, r, 3)) for r in range(3)) == 0
