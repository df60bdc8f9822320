"""The host side of the sampler (t8gpu_amd/sample.py): Morton keys of a partition and host_locate, the numpy form of the
definition the device kernels follow, against the brute force of _sample_ref.py. No GPU."""
import numpy as np
import pytest

import _sample_ref as ref
from t8gpu_amd import sample
from t8gpu_amd.synth import SynthMesh
from t8gpu_amd.unstructured import PrismHexMesh

# the meshes of the GPU tests and the two the key properties were first checked on
MESHES = list(ref.MESHES) + ["fields-2d", "fields-3d"]
EXTRA = {"fields-2d": lambda: SynthMesh(2, 3, 6, band=0.1), "fields-3d": lambda: SynthMesh(3, 2, 4, band=0.2)}


def mesh_of(name):
    return EXTRA[name]() if name in EXTRA else ref.mesh_of(name)


def spans(part):
    return np.uint64(1) << (part.mesh.dim * (sample.DEPTH - part.levels[:part.N].astype(np.int64))).astype(np.uint64)


@pytest.mark.parametrize("mesh", MESHES)
def test_keys_ascend_and_are_contiguous(mesh):
    part = mesh_of(mesh).partition()
    keys = sample.morton_keys(part)
    assert keys.dtype == np.uint64 and keys.shape == (part.N,)
    assert keys[0] == 0
    assert np.all(keys[1:] > keys[:-1])
    assert np.array_equal(keys[1:], keys[:-1] + spans(part)[:-1])
    assert int(keys[-1]) + int(spans(part)[-1]) == 1 << (part.mesh.dim * sample.DEPTH)      # the forest fills the domain


def test_interleave_puts_x_in_the_lowest_bit():
    for dim in (2, 3):
        for a in range(dim):
            for bit in (0, 7, sample.DEPTH - 1):
                c = np.zeros((1, dim), np.uint64)
                c[0, a] = 1 << bit
                assert int(sample.interleave(c, dim)[0]) == 1 << (dim * bit + a)
        full = np.full((1, dim), (1 << sample.DEPTH) - 1, np.uint64)
        assert int(sample.interleave(full, dim)[0]) == (1 << (dim * sample.DEPTH)) - 1


@pytest.mark.parametrize("mesh", MESHES)
def test_a_partition_holds_its_slice_of_the_global_keys(mesh):
    m = mesh_of(mesh)
    whole = sample.morton_keys(m.partition())
    total = 0
    for r in range(3):
        part = m.partition(r, 3)
        assert np.array_equal(sample.morton_keys(part), whole[part.first_global:part.first_global + part.N])
        total += part.N
    assert total == whole.size


@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", list(ref.MESHES))
def test_host_locate_equals_the_brute_force(mesh, subgrid):
    part = ref.partition(mesh, subgrid)
    points, cls = ref.point_set(part, 5)
    want = ref.locate(part, points)
    got = sample.host_locate(part, points)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # the special points are there and land where the definition says
    lo, edge, _ = ref.cell_boxes(part)
    cells = lo.shape[0]
    centres = lo + 0.5 * edge[:, None]
    assert np.array_equal(sample.host_locate(part, centres), np.arange(cells, dtype=np.int32))
    assert np.array_equal(got[cls["corner"]], cls["pick"]) and np.array_equal(got[cls["face"]], cls["pick"])      # the tie rule
    assert np.all(got[cls["inside_edge"]] >= 0) and np.all(got[cls["random"]] >= 0)
    assert np.all(got[cls["outside"]] == -1) and np.all(got[cls["bad"]] == -1)
    assert cls["outside"].stop - cls["outside"].start == 2 * part.mesh.dim and np.isnan(points[cls["bad"]]).any()
    upper = got[cls["upper"]].reshape(part.mesh.dim, -1)
    level = ref.cell_boxes(part)[2]
    for a in range(part.mesh.dim):
        inside = upper[a] >= 0
        assert inside.any() and (~inside).any()                     # neighbours across, and the domain's upper side
        assert np.all(upper[a][inside] != cls["pick"][inside])
        if mesh in ref.REFINED:                                     # 2:1 faces from both sides
            diff = level[upper[a][inside]] - level[cls["pick"][inside]]
            assert (diff > 0).any() and (diff < 0).any(), (mesh, a)


@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", ["refined-2d-periodic", "refined-3d-periodic", "band-2d"])
def test_each_rank_claims_exactly_its_own_points(mesh, subgrid):
    whole = ref.partition(mesh, subgrid)
    points, _ = ref.point_set(whole, 5)
    S = whole.cells_per_element
    one = sample.host_locate(whole, points)
    claimed = np.zeros(points.shape[0], np.int64)
    for r in range(3):
        part = ref.partition(mesh, subgrid, r, 3)
        got = sample.host_locate(part, points)
        assert np.array_equal(got, ref.locate(part, points))
        mine = got >= 0
        assert mine.any()
        assert np.array_equal(got[mine] + part.first_global * S, one[mine])      # the same cell, by its global index
        claimed += mine
    assert np.array_equal(claimed, (one >= 0).astype(np.int64))     # every in-domain point has exactly one owner


def test_refusals():
    with pytest.raises(TypeError):
        sample.morton_keys(PrismHexMesh(5).partition())
    with pytest.raises(TypeError):
        sample.host_locate(PrismHexMesh(5).partition(), np.zeros((1, 3)))
    with pytest.raises(ValueError, match="density.*schlieren"):
        sample.check_names(["pressure", "enstrophy"])
    assert sample.check_names("density") == ["density"]
    assert sample.check_names(["energy", "mach", "energy"]) == ["energy", "mach"]
    deep = SynthMesh(2, 1, 1).partition()
    deep.levels = deep.levels + 20                                  # level 21: above the depth
    with pytest.raises(ValueError):
        sample.check_partition(deep)
    sub = SynthMesh(2, 1, 1).partition(subgrid=True)
    sub.levels = sub.levels + 18                                    # blocks of level 19: cells of level 21
    with pytest.raises(ValueError):
        sample.check_partition(sub)
    assert sample.check_partition(SynthMesh(2, 1, 1).partition(subgrid=True)) == (2, 4)
