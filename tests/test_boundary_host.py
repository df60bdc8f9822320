"""Boundary budgets on the host side (no GPU): the groupings of boundary faces (by kind, by side on Cartesian and curved
partitions, caller-supplied labels and their validation), the sorted face list the C calls take, BoundaryFluxes.combine /
total and the attribute map, the step weights, and the C calls' argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from t8gpu_amd import boundary, build
from t8gpu_amd.boundary import BoundaryFluxes
from t8gpu_amd.synth import SynthMesh
from t8gpu_amd.unstructured import PrismHexMesh, TetHexMesh

SIDES2 = (0, "outflow", "wall", ("farfield", 1))
SIDES3 = (0, "outflow", "periodic", "periodic", "wall", ("farfield", 1))
CODES = {0: 2, "outflow": 1, "wall": 0, ("farfield", 1): 11}


@pytest.mark.parametrize("subgrid", [False, True])
def test_side_groups_of_cartesian_partitions_follow_the_sides_they_were_built_with(subgrid):
    for dim, sides in ((2, SIDES2), (3, SIDES3)):
        part = SynthMesh(dim, 2, 4, band=0.1, sides=sides).partition(subgrid=subgrid)
        side = boundary.side_groups(part)
        kinds = np.asarray(part.boundary_kinds)
        assert side.dtype == np.uint8 and side.shape == (part.B,) and part.B > 0
        open_sides = [s for s in range(2 * dim) if sides[s] != "periodic"]
        assert sorted(set(side.tolist())) == open_sides
        for s in open_sides:
            assert np.all(kinds[side == s] == CODES[sides[s]]), s
        # and from the geometry: a face of side 2 a + 1 lies on x_a = 1 with normal +e_a, its areas add up to the side's measure
        nr = np.asarray(part.normals).reshape(-1, part.normal_dim)[part.F:]
        for s in open_sides:
            n = nr[side == s]
            assert np.all(n[:, s // 2] == (1.0 if s % 2 else -1.0))
            assert abs(np.asarray(part.areas)[part.F:][side == s].sum() - 1.0) < 1e-14
        key, labels, count = boundary.resolve_groups(part, "side")
        assert key == "side" and count == 2 * dim and np.array_equal(labels, side)


@pytest.mark.parametrize("mesh_cls", [PrismHexMesh, TetHexMesh])
def test_side_groups_of_curved_partitions_are_the_meshes_boundary_sides(mesh_cls):
    sides = ("wall", ("farfield", 0), "outflow", "outflow", "wall", "wall")
    mesh = mesh_cls((4, 4, 2), sides=sides)
    whole = mesh.partition()
    assert np.array_equal(boundary.side_groups(whole), mesh.boundary_side)
    assert np.array_equal(np.asarray(whole.boundary_kinds)[boundary.side_groups(whole) == 1], np.full((whole.boundary_side == 1).sum(), 10))
    parts = [mesh.partition(r, 3) for r in range(3)]
    assert sum(p.B for p in parts) == whole.B
    for p in parts:
        side = boundary.side_groups(p)
        assert side.shape == (p.B,) and side.dtype == np.uint8
        want = np.array([0, 10, 1, 1, 0, 0], np.uint8)[side]
        assert np.array_equal(np.asarray(p.boundary_kinds), want)
    # the per-side areas of the ranks add up to the mesh's
    tot = np.zeros(6)
    for p in parts:
        np.add.at(tot, boundary.side_groups(p), np.asarray(p.areas)[p.F:])
    ref = np.zeros(6)
    np.add.at(ref, mesh.boundary_side, np.asarray(whole.areas)[whole.F:])
    assert np.allclose(tot, ref, rtol=1e-13, atol=0)
    assert boundary.resolve_groups(whole, "side")[2] == 6
    # a mesh without sides: every face a wall, the side is known all the same
    plain = mesh_cls((4, 4, 2)).partition()
    assert plain.boundary_kinds is None and np.array_equal(boundary.side_groups(plain), plain.mesh.boundary_side)
    assert np.array_equal(boundary.kind_groups(plain), np.zeros(plain.B, np.uint8))


def test_kind_groups_are_the_kind_codes():
    part = SynthMesh(2, 2, 4, band=0.1, sides=SIDES2).partition()
    key, labels, count = boundary.resolve_groups(part, None)
    assert key == "kind" and count == 16
    assert np.array_equal(labels, np.asarray(part.boundary_kinds)) and set(labels.tolist()) == {0, 1, 2, 11}
    periodic = SynthMesh(2, 2, 3).partition()
    assert periodic.B == 0 and boundary.resolve_groups(periodic, None)[1].shape == (0,)
    assert boundary.side_groups(periodic).shape == (0,)


def test_rejected_group_arrays():
    part = SynthMesh(2, 2, 3, periodic=False).partition()
    ok = np.zeros(part.B, np.uint8)
    ok[::2] = 31
    key, labels, count = boundary.resolve_groups(part, ok)
    assert count == 32 and np.array_equal(labels, ok) and key == ok.tobytes()
    for bad in (np.zeros(part.B + 1, np.uint8),                 # wrong length
                np.zeros((part.B, 1), np.uint8),
                np.full(part.B, 32, np.uint8),                  # value >= 32
                np.zeros(part.B, np.int32),                     # wrong dtype
                np.zeros(part.B, np.float64),
                "kind", "sides", 3, [0] * part.B, ("side",)):
        with pytest.raises(ValueError):
            boundary.resolve_groups(part, bad)


def test_sorted_faces_are_a_stable_sort_with_offsets():
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 7, 1000).astype(np.uint8)
    labels[labels == 4] = 5                                     # an empty group in the middle
    order, off = boundary.sorted_faces(labels, 9)
    assert order.dtype == np.int32 and off.dtype == np.int32 and off[0] == 0 and off[-1] == 1000
    assert sorted(order.tolist()) == list(range(1000))
    for g in range(9):
        mine = order[off[g]:off[g + 1]]
        assert np.all(labels[mine] == g) and np.all(np.diff(mine) > 0)
    assert off[4] == off[5] and off[7] == off[8] == off[9]
    order, off = boundary.sorted_faces(np.zeros(0, np.uint8), 4)
    assert order.size == 0 and off.tolist() == [0] * 5


def test_combine_total_and_the_attribute_map():
    rng = np.random.default_rng(4)
    blocks = [rng.standard_normal((6, 16)) for _ in range(3)]
    for b in blocks:
        b[:, 0] = np.abs(b[:, 0]) + 1
        b[:, 11:13] = rng.integers(0, 9, (6, 2))
        b[:, 13:] = 0
    blocks[2][4] = 0                                             # a group this rank has no face of
    c = BoundaryFluxes.combine([BoundaryFluxes(blocks[0]), blocks[1], BoundaryFluxes(blocks[2])])
    want = blocks[0] + blocks[1] + blocks[2]
    assert np.array_equal(c.block, want)
    assert np.array_equal(c.area, want[:, 0]) and np.array_equal(c.flux, want[:, 1:6])
    assert np.array_equal(c.mass_flow, want[:, 1]) and np.array_equal(c.momentum_flux, want[:, 2:5])
    assert np.array_equal(c.energy_flow, want[:, 5]) and np.array_equal(c.pressure_force, want[:, 6:9])
    assert np.array_equal(c.mean_pressure, want[:, 9] / want[:, 0])
    assert np.array_equal(c.mass_out, want[:, 10]) and np.array_equal(c.mass_in, want[:, 10] - want[:, 1])
    assert np.array_equal(c.faces, want[:, 11].astype(np.int64)) and np.array_equal(c.nonfinite, want[:, 12].astype(np.int64))
    t = c.total()
    assert t.block.shape == (1, 16) and np.allclose(t.block[0], want.sum(0), rtol=1e-15, atol=1e-15)
    assert "BoundaryFluxes(groups=6" in repr(c) and "faces=" in repr(c)
    empty = BoundaryFluxes(np.zeros((2, 16)))
    assert np.isnan(empty.mean_pressure).all() and repr(empty) == "BoundaryFluxes(groups=2, {})"
    with pytest.raises(ValueError):
        BoundaryFluxes.combine([np.zeros((2, 16)), np.zeros((3, 16))])


def test_step_weights_reproduce_the_three_stage_formulas():
    """I3 from the stage identities with arbitrary B0, B1, B2 equals (c31 + c32) I0 - sum w_k B_k"""
    dt = 0.0371
    w = boundary.step_weights(torch.float64, dt)
    c31, c32, c33 = 0.33333333333333, 0.66666666666666, 0.66666666666666
    I0, B0, B1, B2 = 3.1, 0.7, -1.3, 2.9
    I1 = I0 - dt * B0
    I2 = 0.75 * I0 + 0.25 * I1 - 0.25 * dt * B1
    I3 = c31 * I0 + c32 * I2 - c33 * dt * B2
    assert abs(I3 - ((c31 + c32) * I0 - (w[0] * B0 + w[1] * B1 + w[2] * B2))) < 1e-14          # (a dozen roundings of O(1) numbers)
    assert abs(sum(w) - dt) < 1e-13 * dt                        # consistent: the weights add up to dt (literals truncated at 1e-14)
    w32 = boundary.step_weights(torch.float32, dt)
    assert w32[2] == float(np.float32(0.66666666666666)) * dt and abs(sum(w32) - dt) < 1e-7 * dt


def test_c_calls_refuse_bad_arguments_without_a_gpu():
    """the checks run before any launch: hipErrorInvalidValue (1) with no device present"""
    lib = C.CDLL(build.build_hip())
    nbytes = lib.t8gpu_hip_boundary_fluxes_workspace_bytes
    nbytes.restype = C.c_size_t
    assert nbytes(0, 1) >= 16 * 8 and nbytes(1000, 32) >= 16 * 8 * (1000 // 16 + 32)

    class V(C.Structure):
        _fields_ = [("p", C.c_void_p * 5)]

    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)

    def offs(*v):
        return (C.c_int32 * len(v))(*v)

    for name, dims in (("t8gpu_hip_boundary_fluxes_f64", (2, 3)), ("t8gpu_hip_boundary_fluxes_f32", (2, 3)),
                       ("t8gpu_hip_subgrid_boundary_fluxes_f64", (2, 3)), ("t8gpu_hip_subgrid_boundary_fluxes_f32", (2, 3))):
        f = getattr(lib, name)
        f.restype = C.c_int
        sub = "subgrid" in name

        def call(kind=0, F=0, B=8, dim=dims[0], G=2, order=p, offsets=offs(0, 3, 8), ws=p, res=p):
            head = (kind, dim, F, B) if sub else (kind, F, B, dim)
            return f(*head, p, None, None, p, p, V(), G, order, offsets, ws, res, 0, C.c_double(0.0), None)

        assert call(kind=3) == 1 and call(kind=-1) == 1
        assert call(dim=1) == 1 and call(dim=4) == 1
        assert call(G=0) == 1 and call(G=33, offsets=offs(*([0] * 33 + [8]))) == 1
        assert call(offsets=offs(1, 3, 8)) == 1                  # does not start at 0
        assert call(offsets=offs(0, 3, 7)) == 1                  # does not end at B
        assert call(offsets=offs(0, 9, 8)) == 1                  # not ascending
        assert call(offsets=None) == 1 and call(res=None) == 1
        assert call(ws=None) == 1 and call(order=None) == 1
        assert call(B=-1, offsets=offs(0, 0, -1)) == 1
