"""-m gpu: the identities between the compat tier's boundary kernels that hold because they share one face routine
(csrc/hip/compat_faces.hpp: boundary_face_flux), bit for bit, so that a later edit cannot quietly fork the kernels again.

The C entry points run on the hand-built face lists of tests/_compat_boundary.py -- every boundary face a cell (block) of its
own, no interior faces, zeroed flux planes: no two atomic adds meet, and the comparison is torch.equal on the words. Lists:
13 plain faces in 2D and 3D (axis and oblique normals), 5 faces of Subgrid<4,4,4> blocks (four per wavefront: one full, one
ragged; two lists, which hold the six normals and the six kinds 0, 1, 2, 3, 10, 11 between them), 17 faces of Subgrid<4,4>
blocks (sixteen per wavefront). Random physical states, normal velocities over +-2.5 sound speeds."""
import functools

import numpy as np
import pytest
import torch

import _compat_boundary as CB
from _farfield import farfield_outside
from _gpu import NP
from t8gpu_amd import hip

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
KINDS = [hip.KEPES, hip.HLL, hip.HLLC]
PLAIN, SUBGRID = ("plain2", "plain3"), ("subgrid3a", "subgrid3b", "subgrid2")


@functools.lru_cache(maxsize=None)
def cases(dtype, kind):
    """every kernel run of one (dtype, flux kind), made once and shared by the tests below"""
    geos = CB.geometries(NP[dtype])
    return geos, CB.run_cases(dtype, kind, geos)


def same_bits(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    words = torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.shape == b.shape and torch.equal(a.contiguous().view(words), b.contiguous().view(words))


def flux_of(value):
    return value[0] if isinstance(value, tuple) else value


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_list_of_wall_kinds_and_no_list_give_the_bits_of_the_wall_kernel(dtype, kind):
    geos, out = cases(dtype, kind)
    for name in PLAIN + SUBGRID:
        walls = out[name + "/walls"]
        assert bool((flux_of(walls)[1:4] != 0).any()) and bool(torch.isfinite(flux_of(walls)).all())
        assert same_bits(out[name + "/bc_zero"], walls), name
        assert same_bits(out[name + "/bc_null"], walls), name
        assert not same_bits(out[name + "/mixed"], walls), name              # (the kinds are read where they are given)
    for name in PLAIN:
        assert bool((out[name + "/walls"][1] > 0).all())                       # a speed estimate for every face
    for name in SUBGRID:
        assert same_bits(out[name + "/far_null"], out[name + "/walls"]), name


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_subgrid_far_kernel_on_kinds_below_ten_gives_the_bits_of_the_bc_kernel(dtype, kind):
    geos, out = cases(dtype, kind)
    seen = set()
    for name in SUBGRID:
        seen |= set(geos[name].open.tolist())
        assert same_bits(out[name + "/far_open"], out[name + "/bc_open"]), name
        assert not same_bits(out[name + "/bc_open"], out[name + "/walls"]), name
    assert seen == {0, 1, 2, 3}


def face_cells(geo, out, name):
    """the cells that own a boundary (sub-)face, and the face of each: plain, cell i owns face i; Subgrid, the cells the wall
    kernel wrote a momentum flux to (the wall flux is p n), 4^(rank - 1) per block"""
    if isinstance(geo, CB.PlainList):
        return np.arange(geo.B), np.arange(geo.B)
    S = 4 ** geo.rank
    cells = np.nonzero((out[name + "/walls"][1:4] != 0).any(0).cpu().numpy())[0]
    assert len(cells) == geo.B * S // 4 and np.array_equal(np.bincount(cells // S, minlength=geo.B), np.full(geo.B, S // 4))
    return cells, cells // S


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_supersonic_farfield_face_has_the_bits_of_the_inflow_or_outflow_face(dtype, kind):
    """Far field 10 + k where the flow enters faster than sound takes table row k: the inflow face 2 + k; where it leaves
    faster than sound it takes the inside state: the outflow face. In the plain kernel and in the Subgrid _far kernel, for
    the flux planes and (plain) the speed estimates. The branch of every face: tests/_farfield.py on the states as the
    kernel reads them; no face lies within 1e-3 of the sonic point, so fp32 and fp64 decide alike."""
    geos, out = cases(dtype, kind)
    rows = CB.inflow_states().astype(NP[dtype]).astype(np.float64)
    kinds_seen = set()
    for name in PLAIN + SUBGRID:
        geo = geos[name]
        kinds_seen |= set(geo.mixed.tolist())
        cells, face = face_cells(geo, out, name)
        k = geo.mixed[face].astype(np.int64)
        far = k >= 10
        state, n3 = geo.state.astype(np.float64)[cells], geo.n3[cells]
        rho, v, p = state[:, 0], state[:, 1:4] / state[:, 0:1], 0.4 * (state[:, 4] - 0.5 * (state[:, 1:4] ** 2).sum(1) / state[:, 0])
        mach = (v * n3).sum(1) / np.sqrt(1.4 * p / rho)
        assert np.abs(np.abs(mach[far]) - 1).min() > 1e-3 and mach.min() < -2 and mach.max() > 2
        branch = np.full(len(cells), -1)
        _, branch[far] = farfield_outside(state[far], n3[far], rows[k[far] - 10])
        assert (branch == 0).any() and (branch == 1).any() and (branch >= 2).any(), (name, np.bincount(branch[far]))
        mixed, inflow, outflow = (out[f"{name}/{c}"] for c in ("mixed", "far_as_inflow", "far_as_outflow"))

        def at(value, sel):            # the words of the selected faces: flux columns of their cells (plain: and their speeds)
            idx = torch.from_numpy(cells[sel]).cuda()
            return tuple(x.index_select(x.dim() - 1, idx) for x in (value if isinstance(value, tuple) else (value,)))

        assert same_bits(at(mixed, branch == 0), at(inflow, branch == 0)), name
        assert same_bits(at(mixed, branch == 1), at(outflow, branch == 1)), name
        assert same_bits(at(mixed, ~far), at(inflow, ~far)) and same_bits(at(mixed, ~far), at(outflow, ~far)), name
        # the subsonic faces carry a state of their own
        assert not same_bits(at(mixed, branch >= 2), at(inflow, branch >= 2)), name
        assert not same_bits(at(mixed, branch >= 2), at(outflow, branch >= 2)), name
    assert kinds_seen == set(CB.ALL_KINDS)
