"""Far-field faces of Subgrid meshes on the host side (no GPU): the planner entry that takes kinds 10 + k
(t8gpu_plan_subgrid_create_far, HostSubgridPlan(..., farfield=True)) gives the plan of t8gpu_plan_subgrid_create_bc byte for
byte when no kind is above 9, writes a far-field kind into every record that holds the face, keeps far-field blocks out of
families, and refuses kinds of 16 and above; the entry without far field keeps refusing kind 10. Also the sub-cell centre
helper of the GPU tests and the branch coverage of their initial state (the numpy restatement of the condition alone)."""
import numpy as np
import pytest

from test_subgrid_open_boundaries_host import MESHES, OPEN_SIDES, _all_records, _rows_of_boundary_faces
from t8gpu_amd.plan import HostSubgridPlan
from t8gpu_amd.synth import SynthMesh

FAR_SIDES = {2: (("farfield", 0), ("farfield", 1), "periodic", "periodic"),
             3: (("farfield", 0), ("farfield", 1), "periodic", "periodic", "wall", ("farfield", 0))}


@pytest.mark.parametrize("dim,args", MESHES)
@pytest.mark.parametrize("sides", ["walls", "open"])
def test_kinds_up_to_nine_give_the_bc_plan_array_for_array(dim, args, sides):
    mesh = SynthMesh(dim, periodic=False, **args) if sides == "walls" else SynthMesh(dim, sides=OPEN_SIDES[dim], **args)
    part = mesh.partition(subgrid=True)
    bc, far = HostSubgridPlan(part), HostSubgridPlan(part, farfield=True)
    assert bc.has_open_faces == far.has_open_faces == (sides == "open")
    assert not far.has_farfield_faces and not bc.has_farfield_faces
    assert (bc.n_families, bc.n_rest, bc.n_interior, bc.n_deep, bc.n_addressed, bc.max_bf) == \
        (far.n_families, far.n_rest, far.n_interior, far.n_deep, far.n_addressed, far.max_bf)
    for fs in (4, 8):
        a, b = _all_records(bc, part, fs), _all_records(far, part, fs)
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("dim", [2, 3])
def test_farfield_faces_carry_their_kind_and_stay_out_of_families(dim):
    mesh = SynthMesh(dim, 3, 4, band=0.1, sides=FAR_SIDES[dim])
    part = mesh.partition(subgrid=True)
    kinds = np.asarray(part.boundary_kinds)
    assert set(np.unique(kinds)) >= {10, 11}
    h = HostSubgridPlan(part, farfield=True)
    assert h.has_open_faces and h.has_farfield_faces
    F = part.F
    fn = np.asarray(part.face_neighbors)
    # the same partition with the far-field kinds replaced by outflow: the plan differs in the kind bits alone
    ref = HostSubgridPlan(part, boundary_kinds=np.where(kinds >= 10, 1, kinds).astype(np.uint8))
    fr = h.face_rec[F:]
    assert np.array_equal(fr[:, 1], np.full(part.B, -1))
    assert np.array_equal((fr[:, 2] >> 23) & 15, kinds)
    assert np.array_equal(fr[:, 2] & ((1 << 23) - 1), ref.face_rec[F:, 2] & ((1 << 23) - 1))
    assert np.array_equal(h.face_rec[:F], ref.face_rec[:F])
    assert np.array_equal(h.block_order, ref.block_order) and (h.n_families, h.n_rest) == (ref.n_families, ref.n_rest)
    want = {}
    for b in range(part.B):
        want.setdefault(int(fn[2 * F + b]), []).append(int(kinds[b]))
    block_rec, bf_rec = h.records(part.areas, 8)
    got = {}
    for e, code in _rows_of_boundary_faces(h, part, block_rec):
        got.setdefault(e, []).append((code >> 23) & 15)
    assert {e: sorted(v) for e, v in got.items()} == {e: sorted(v) for e, v in want.items()}
    # generic rows (bf_rec): a boundary face there carries its kind too (none on these meshes: every boundary face folds)
    for row in bf_rec[:h.n_entries]:
        assert row[0] != -1 or ((row[1] >> 23) & 15) in (0, 10, 11)
    far_blocks = set(int(e) for e in fn[2 * F:][kinds >= 10])
    assert h.n_families > 0
    fam_rec, rest_rec = h.family_records(part.areas, 8)
    fam_blocks = {int(r[0]) + w for r in fam_rec[:h.n_families] for w in range(1 << dim)}
    assert not fam_blocks & far_blocks
    rest = {}
    for e, code in _rows_of_boundary_faces(h, part, rest_rec[:h.n_rest]):
        rest.setdefault(e, []).append((code >> 23) & 15)
    assert {e: sorted(v) for e, v in rest.items()} == {e: sorted(v) for e, v in want.items()}


def test_a_rank_without_farfield_faces_says_so():
    mesh = SynthMesh(2, 3, 5, band=0.05, sides=FAR_SIDES[2])
    flags = [HostSubgridPlan(mesh.partition(r, 3, subgrid=True), farfield=True).has_farfield_faces for r in range(3)]
    assert any(flags)
    whole = mesh.partition(subgrid=True)
    assert HostSubgridPlan(whole, farfield=True).has_farfield_faces


def test_the_bc_entry_still_refuses_farfield_kinds_and_the_far_entry_kinds_of_sixteen():
    part = SynthMesh(2, 2, 3, periodic=False).partition(subgrid=True)
    with pytest.raises(ValueError):
        HostSubgridPlan(part, boundary_kinds=np.full(part.B, 10, np.uint8))
    far = SynthMesh(2, 2, 3, sides=FAR_SIDES[2]).partition(subgrid=True)
    with pytest.raises(ValueError):
        HostSubgridPlan(far)
    assert HostSubgridPlan(part, boundary_kinds=np.full(part.B, 15, np.uint8), farfield=True).has_farfield_faces
    for k in (16, 17, 255):
        with pytest.raises(ValueError):
            HostSubgridPlan(part, boundary_kinds=np.full(part.B, k, np.uint8), farfield=True)


def test_subcell_centres_and_branch_coverage_of_the_initial_state():
    """The initial state of the GPU tests, built from subcell centres, puts sub-faces of each x side into every branch of the
    condition already at the initial state (what the GPU tests require of their reference over a run), on the coarsest side
    the tests could meet (level-3 blocks: 32 subcells per side), for the seeds the tests use. The smallest count is 1
    (subsonic with far-field reference on +x, seed 22); the tests' finer meshes only add samples."""
    from _farfield import farfield_outside
    from test_gpu_farfield import far_states
    from test_gpu_subgrid_farfield import subcell_centres, subgrid_far_state
    from test_subgrid_open_boundaries_host import boundary_subcells
    for dim in (2, 3):
        part = SynthMesh(dim, 3, 3, sides=FAR_SIDES[dim]).partition(subgrid=True)
        S = 4 ** dim
        x = subcell_centres(part)
        assert x.shape == ((part.N + part.G) * S, 3)
        # subcell (i, j, k) of block e at e * S + i + 4 j + 16 k; the subcells tile the unit box
        e = 5
        assert np.allclose(x[e * S:(e + 1) * S].mean(0)[:dim], np.asarray(part.centres)[e, :dim])
        assert np.allclose(x[e * S + 1] - x[e * S], [2.0 ** -3 / 4, 0, 0])
        assert np.allclose(x[e * S + 4] - x[e * S], [0, 2.0 ** -3 / 4, 0])
        assert np.unique(np.round(x[:part.N * S, :dim] * 64).astype(int), axis=0).shape[0] == part.N * S
    part = SynthMesh(2, 3, 3, sides=FAR_SIDES[2]).partition(subgrid=True)
    kinds = np.asarray(part.boundary_kinds)
    nr = np.asarray(part.normals).reshape(-1, 2)
    states = far_states()
    for seed in (21, 22, 23):
        st = subgrid_far_state(part, seed)
        for sign in (-1.0, 1.0):
            counts = np.zeros(4, np.int64)
            for b in np.flatnonzero((kinds >= 10) & (nr[part.F:, 0] == sign)):
                sub = boundary_subcells(part, b)
                n3 = np.zeros((sub.size, 3))
                n3[:, 0] = sign
                _, br = farfield_outside(st[:, sub].T, n3, np.repeat(states[kinds[b] - 10][None], sub.size, 0))
                counts += np.bincount(br, minlength=4)
            assert counts.sum() == 32 and (counts >= 1).all(), (seed, sign, counts)
