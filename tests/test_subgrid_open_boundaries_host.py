"""Open boundaries of Subgrid meshes on the host side (no GPU): how the Subgrid planner carries the kind of every boundary
face into the records the kernels read (bits 23-26 of the code word, far = -1 as for walls), that a wall-only plan is
byte-identical to the plan without kinds, that no family holds a block with an open face, and that the sub-face enumeration
the GPU tests build their reference with reproduces the oracle's wall loop."""
import ctypes as C
import types

import numpy as np
import pytest

import _oracle as O
from t8gpu_amd.plan import HostSubgridPlan
from t8gpu_amd.synth import SynthMesh

OPEN_SIDES = {2: (0, "outflow", "periodic", "periodic"),
              3: (0, "outflow", "periodic", "periodic", "wall", "wall")}
MESHES = [(2, dict(base_level=3, max_level=5, band=0.05)), (3, dict(base_level=2, max_level=3, band=0.1)),
          (3, dict(base_level=3, max_level=3))]


def _without_kinds(part):
    """the partition's arrays with boundary_kinds = None: HostSubgridPlan then calls t8gpu_plan_subgrid_create"""
    return types.SimpleNamespace(subgrid=True, mesh=part.mesh, N=part.N, F=part.F, B=part.B, face_neighbors=part.face_neighbors,
                                 normals=part.normals, level_diff=part.level_diff, nb_offset=part.nb_offset, boundary_kinds=None)


def _all_records(h, part, float_size):
    block_rec, bf_rec = h.records(part.areas, float_size)
    out = dict(block_rec=block_rec, bf_rec=bf_rec, face_rec=h.face_rec, bf_off=h.bf_off, bf_ent=h.bf_ent, plus=h.plus,
               block_order=h.block_order)
    if h.n_families:
        out["fam_rec"], out["rest_rec"] = h.family_records(part.areas, float_size)
    return out


@pytest.mark.parametrize("dim,args", MESHES)
@pytest.mark.parametrize("periodic", [True, False])
def test_wall_only_kinds_give_the_plan_without_kinds(dim, args, periodic):
    part = SynthMesh(dim, periodic=periodic, **args).partition(subgrid=True)
    old = HostSubgridPlan(_without_kinds(part))
    zeros = HostSubgridPlan(part, boundary_kinds=np.zeros(part.B, np.uint8))
    assert not old.has_open_faces and not zeros.has_open_faces
    assert (old.n_families, old.n_rest, old.n_interior, old.n_deep) == (zeros.n_families, zeros.n_rest, zeros.n_interior, zeros.n_deep)
    if not periodic:
        assert part.B > 0
    if dim == 3 and args.get("band") is None:
        assert old.n_families > 0
    for fs in (4, 8):
        a, b = _all_records(old, part, fs), _all_records(zeros, part, fs)
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k


def _rows_of_boundary_faces(h, part, rec):
    """(block, code) of every far = -1 row of block_rec-shaped records (+ and - faces) and of bf_rec"""
    out = []
    for row in rec:
        for q in range(6):
            w = row[4 + 4 * q:8 + 4 * q]
            if w[0] == -1:
                out.append((int(row[0]), int(w[1])))
    return out


@pytest.mark.parametrize("dim", [2, 3])
def test_open_faces_carry_their_kind_and_stay_out_of_families(dim):
    mesh = SynthMesh(dim, 3, 4, band=0.1, sides=OPEN_SIDES[dim])
    part = mesh.partition(subgrid=True)
    kinds = np.asarray(part.boundary_kinds)
    assert set(np.unique(kinds)) >= {1, 2}
    h = HostSubgridPlan(part)
    assert h.has_open_faces
    F = part.F
    fn = np.asarray(part.face_neighbors)
    # face_rec: far slot -1 and the kind in bits 23-26; nothing else of the code changes
    ref = HostSubgridPlan(_without_kinds(part))
    fr = h.face_rec[F:]
    assert np.array_equal(fr[:, 1], np.full(part.B, -1))
    assert np.array_equal((fr[:, 2] >> 23) & 15, kinds)
    assert np.array_equal(fr[:, 2] & ((1 << 23) - 1), ref.face_rec[F:, 2])
    assert np.array_equal(h.face_rec[:F], ref.face_rec[:F])
    # every block row that names a boundary face carries the kind of that block's face on that side
    open_blocks = set(int(e) for e in fn[2 * F:][kinds != 0])
    want = {}
    for b in range(part.B):
        want.setdefault(int(fn[2 * F + b]), []).append(int(kinds[b]))
    block_rec, bf_rec = h.records(part.areas, 8)
    got = {}
    for e, code in _rows_of_boundary_faces(h, part, block_rec):
        got.setdefault(e, []).append((code >> 23) & 15)
    assert bf_rec.shape[0] == max(1, h.n_entries)
    assert {e: sorted(v) for e, v in got.items()} == {e: sorted(v) for e, v in want.items()}
    # families: none holds an open-face block; the rest records hold every open-face block with its kinds
    nb = 1 << dim
    if h.n_families:
        fam_rec, rest_rec = h.family_records(part.areas, 8)
        fam_blocks = {int(r[0]) + w for r in fam_rec[:h.n_families] for w in range(nb)}
        assert not fam_blocks & open_blocks
        rest = {}
        for e, code in _rows_of_boundary_faces(h, part, rest_rec[:h.n_rest]):
            rest.setdefault(e, []).append((code >> 23) & 15)
        assert {e: sorted(v) for e, v in rest.items()} == {e: sorted(v) for e, v in want.items()}
    # and the same mesh fully periodic does have families where the open blocks now are not
    per = HostSubgridPlan(SynthMesh(dim, 3, 4, band=0.1).partition(subgrid=True))
    assert per.n_families >= h.n_families


def test_kinds_out_of_range_are_refused():
    part = SynthMesh(2, 2, 3, periodic=False).partition(subgrid=True)
    with pytest.raises(ValueError):
        HostSubgridPlan(part, boundary_kinds=np.full(part.B, 10, np.uint8))


def boundary_subcells(part, b):
    """the subcells of boundary face b (block * S + cell, one per sub-face): coordinate 3 (outward normal +e_d) or 0 (-e_d)
    along the face's axis, all 4 x 4 (3D) / 4 (2D) across it"""
    rank = part.mesh.dim
    S = 4 ** rank
    n = np.asarray(part.normals).reshape(-1, rank)[part.F + b]
    ax = int(np.flatnonzero(n != 0)[0])
    plane = 3 if n[ax] > 0 else 0
    e = int(np.asarray(part.face_neighbors)[2 * part.F + b])
    cells = np.arange(S)
    return e * S + cells[(cells >> (2 * ax)) & 3 == plane]


def boundary_flux_by_enumeration(part, dtype, kind, st, faces, outside):
    """flux planes of boundary faces `faces` from oracle_xyz_face_flux per sub-face: left = the inside subcell, outward
    normal, right = outside(subcells, inside states) (mirror=True: the oracle's reflected state), times area / sub-faces"""
    rank = part.mesh.dim
    SF = 4 ** (rank - 1)
    dtype = np.dtype(dtype).type
    fl = np.zeros_like(st)
    nr = np.asarray(part.normals).reshape(-1, rank)
    for b in faces:
        sub = boundary_subcells(part, b)
        n3 = np.zeros((sub.size, 3), dtype)
        n3[:, :rank] = nr[part.F + b]
        sL = np.ascontiguousarray(st[:, sub].T)
        if outside is None:
            g = O.xyz_face_flux(kind, n3, sL, sL, mirror=True)
        else:
            g = O.xyz_face_flux(kind, n3, sL, outside(b, sL))
        g = g * (np.asarray(part.areas, dtype)[part.F + b] / dtype(SF))
        for k in range(5):
            np.subtract.at(fl[k], sub, g[:, k])
    return fl


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_subcell_enumeration_reproduces_the_oracle_wall_loop(dim, kind, dtype):
    """The GPU tests' reference evaluates open sub-faces by this enumeration; with mirror=True it must be the oracle's own
    wall loop (oracle_subgrid_boundary)."""
    from _gpu import perturbed_state
    part = SynthMesh(dim, 2, 3, band=0.1, periodic=False).partition(subgrid=True)
    S = 4 ** dim
    st = np.ascontiguousarray(perturbed_state(part, 5).astype(dtype))
    assert st.shape[1] == part.N * S and part.B > 0
    want = np.zeros_like(st)
    getattr(O.lib(), "oracle_subgrid_boundary_" + O.suf(dtype))(kind, dim, part.F, part.B, O.p(part.face_neighbors),
                                                                 O.p(np.ascontiguousarray(part.normals, dtype)),
                                                                 O.p(np.ascontiguousarray(part.areas, dtype)), O.p(st), O.p(want),
                                                                 C.c_size_t(st.shape[1]))
    got = boundary_flux_by_enumeration(part, dtype, kind, st, range(part.B), None)
    assert np.abs(want).max() > 0
    assert np.array_equal(got, want)
