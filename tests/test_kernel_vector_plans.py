"""The meshes of tests/golden/reference_kernel_vectors.npz as the host planners see them (no GPU).

tests/test_gpu_reference_kernels.py runs the fused tier on these meshes and counts on what is asserted here: that a plain
case cut into small tiles gives several tiles that read each other's cells, and that every Subgrid case runs the family
kernel AND the block kernel and has hanging faces. These are conditions, not measurements: if the planner's rules move, this
file says that the GPU tests no longer reach what they are there for. (Today: 3 / 21 / 4 tiles with tmax=8, fcap=24; 2 / 2 /
1 / 5 families beside 11 / 14 / 7 / 38 single blocks; 8 / 12 / 24 / 44 hanging faces.)"""
import numpy as np
import pytest
import torch

import _kernel_vectors as KV
from t8gpu_amd.fused import PlainPlan
from t8gpu_amd.plan import HostPlainPlan, HostSubgridPlan

SMALL_TILES = dict(tmax=8, fcap=24)          # what test_gpu_reference_kernels.py passes for "several tiles with halos"


def test_the_fixture_partition_is_the_fixture():
    for case in KV.case_names():
        for tag in KV.TAGS:
            ins, _ = KV.load(case, tag)
            part = KV.FixturePartition(case, ins)
            S = 4 ** part.mesh.dim if part.subgrid else 1
            assert part.G == 0 and part.stride == (part.N + part.G) * S == ins["state"].shape[1]
            assert part.face_neighbors.size == 2 * part.F + part.B
            assert part.normals.size == part.normal_dim * (part.F + part.B) and part.areas.size == part.F + part.B
            assert part.volumes.dtype == np.float64 and part.volumes.shape == (part.N,)
            assert np.array_equal(part.volumes.astype(ins["volume"].dtype), ins["volume"])      # exact in the case's type
            assert np.array_equal(part.indices, np.arange(part.N))                              # the stored map: identity
            assert 0 <= part.face_neighbors.min() and part.face_neighbors.max() < part.N
            assert part.mesh.dim == (3 if "3d" in case else 2)
            assert not hasattr(part, "boundary_kinds")
            assert part.subgrid == case.startswith("sub") == hasattr(part, "level_diff")


@pytest.mark.parametrize("tag", KV.TAGS)
@pytest.mark.parametrize("case", KV.plain_cases())
def test_plain_fixture_meshes_give_the_plans_the_gpu_tests_need(case, tag):
    part = KV.partition(case, tag)
    dtype = torch.float64 if tag == "f64" else torch.float32
    for options in ({}, dict(dictionary=False), dict(compressed=False)):
        default = PlainPlan.on_host(part, dtype, **options).host                # the default plan builds
        assert default.ntiles >= 1 and default.n_patches == 0
        assert int(default.elem_off[-1]) == part.N
        small = PlainPlan.on_host(part, dtype, **options, **SMALL_TILES).host
        assert small.ntiles > 1 and small.halo_ids.size > 0                     # tiles read each other's cells
        assert small.max_elems <= SMALL_TILES["tmax"] and small.n_patches == 0
        assert int(small.elem_off[-1]) == part.N
    direct = HostPlainPlan.from_partition(part, **SMALL_TILES)
    assert direct.ntiles > 1 and direct.halo_ids.size > 0
    assert not direct.open_faces                                                # walls only


@pytest.mark.parametrize("tag", KV.TAGS)
@pytest.mark.parametrize("case", KV.subgrid_cases())
def test_subgrid_fixture_meshes_give_the_plans_the_gpu_tests_need(case, tag):
    part = KV.partition(case, tag)
    plan = HostSubgridPlan(part)
    assert plan.rank == part.mesh.dim and plan.N == part.N
    assert plan.n_families > 0 and plan.n_rest > 0          # the family kernel and the block kernel both run
    assert plan.n_families * 2 ** plan.rank + plan.n_rest == part.N
    assert int((part.level_diff != 0).sum()) > 0            # hanging faces
    assert not plan.has_open_faces
