"""Host reference of the boundary budgets (t8gpu_amd/boundary.py), composed from the oracle's xyz face flux as
test_gpu_open_boundaries.OpenCase / _farfield.FarCase build a boundary face: inside state, outside state by the face's kind
(mirror=True on walls), times the area; Subgrid blocks by the sub-face enumeration of test_subgrid_open_boundaries_host. The
sums per group are plain numpy in fp64. Needs no GPU."""
import numpy as np

import _oracle as O
from _farfield import farfield_outside
from test_subgrid_open_boundaries_host import boundary_subcells

SLOTS = 16


def boundary_terms(part, dtype, kind, state, inflow):
    """Per boundary face (Subgrid: sub-face), in fp64: (face index b, area A, flux g[., 5] along the outward normal from the
    oracle in `dtype`, inside pressure p, normal n3[., 3]). `state` (5, cells) host array; geometry and states are cast to
    `dtype` first, as the device holds them."""
    dtype = np.dtype(dtype).type
    F, B = part.F, part.B
    subgrid = bool(part.subgrid)
    rank = part.mesh.dim
    nd = part.normal_dim
    kinds = getattr(part, "boundary_kinds", None)
    kinds = np.zeros(B, np.int64) if kinds is None else np.asarray(kinds).astype(np.int64)
    nr = np.asarray(part.normals).reshape(-1, nd)[F:].astype(dtype)
    areas = np.asarray(part.areas)[F:].astype(dtype).astype(np.float64)
    fn = np.asarray(part.face_neighbors)[2 * F:].astype(np.int64)
    st = np.asarray(state).astype(dtype)
    table = None if inflow is None else np.asarray(inflow, np.float64).astype(dtype)
    if subgrid:
        SF = 4 ** (rank - 1)
        face = np.repeat(np.arange(B), SF)
        cells = np.concatenate([boundary_subcells(part, b) for b in range(B)]) if B else np.zeros(0, np.int64)
        A = areas[face] / SF
    else:
        face, cells, A = np.arange(B), fn, areas
    n3 = np.zeros((face.size, 3), dtype)
    n3[:, :nd] = nr[face]
    sL = np.ascontiguousarray(st[:, cells].T)
    k = kinds[face]
    g = np.zeros((face.size, 5), dtype)
    wall = k == 0
    if wall.any():
        g[wall] = O.xyz_face_flux(kind, n3[wall], sL[wall], sL[wall], mirror=True)
    if (~wall).any():
        sR = sL.copy()
        inf = (k >= 2) & (k < 10)
        if inf.any():
            sR[inf] = table[k[inf] - 2]
        far = k >= 10
        if far.any():
            sR[far] = farfield_outside(sL[far], n3[far], table[k[far] - 10])[0].astype(dtype)
        g[~wall] = O.xyz_face_flux(kind, n3[~wall], sL[~wall], sR[~wall])
    s64 = sL.astype(np.float64)
    with np.errstate(all="ignore"):
        p = 0.4 * (s64[:, 4] - 0.5 * (s64[:, 1:4] ** 2).sum(1) / s64[:, 0])
    return face, A, g.astype(np.float64), p, n3.astype(np.float64)


def reference_block(part, dtype, kind, state, inflow, labels, num_groups):
    """(block[G, 16], scale[G, 16]): the slots of include/t8gpu_hip.h per group and, per slot, the sum of the absolute values of
    its terms -- what an error of that slot is normalised by, so that cancellation cannot hide one"""
    face, A, g, p, n3 = boundary_terms(part, dtype, kind, state, inflow)
    grp = np.asarray(labels, np.int64)[face]
    fin = np.isfinite(g).all(1)
    finp = fin & np.isfinite(p)
    terms = np.zeros((face.size, SLOTS))
    terms[:, 0] = A
    terms[:, 1:6] = np.where(fin[:, None], A[:, None] * np.where(fin[:, None], g, 0.0), 0.0)
    pz = np.where(finp, p, 0.0)
    terms[:, 6:9] = (A * pz)[:, None] * n3
    terms[:, 9] = A * pz
    terms[:, 10] = np.where(fin, A * np.maximum(np.where(fin, g[:, 0], 0.0), 0.0), 0.0)
    terms[:, 11] = 1.0
    terms[:, 12] = ~fin
    block, scale = np.zeros((num_groups, SLOTS)), np.zeros((num_groups, SLOTS))
    np.add.at(block, grp, terms)
    np.add.at(scale, grp, np.abs(terms))
    return block, scale


def slot_error(got, want, scale):
    """max over groups and slots 0-10 of |got - want| / (sum of |terms|); a slot without terms must be exactly 0"""
    got, want, scale = (np.asarray(a, np.float64)[..., :11] for a in (got, want, scale))
    assert np.all(got[scale == 0] == 0.0)
    return float((np.abs(got - want) / np.where(scale > 0, scale, 1.0)).max())
