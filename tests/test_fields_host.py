"""The derived output fields' host side, without a GPU: the CSR element -> interior faces of t8gpu_host_cell_faces against a
numpy argsort construction, its refusals, the four t8gpu_hip_*_fields_* entries (they load and refuse bad arguments before
any launch), and the kernel source hash, which this pass must leave where the committed c4 profile recorded it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from t8gpu_amd import build, fields, synth
from t8gpu_amd.synth import SynthMesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = {
    "2d-periodic": lambda: SynthMesh(2, 2, 4, band=0.2).partition(),
    "2d-walls": lambda: SynthMesh(2, 2, 4, band=0.2, periodic=False).partition(),
    "3d-periodic": lambda: SynthMesh(3, 1, 3, band=0.3).partition(),
    "2d-subgrid-blocks": lambda: SynthMesh(2, 2, 4, band=0.2).partition(subgrid=True),
    "2d-rank1of3": lambda: SynthMesh(2, 2, 4, band=0.2).partition(1, 3),
}


def csr_by_argsort(n_owned, num_faces, fn):
    """rows of 2 f + side for every side of an interior face that is an owned element, ascending: a stable sort by element"""
    sides = np.asarray(fn[: 2 * num_faces], np.int64)           # index k = 2 f + side
    keep = np.nonzero(sides < n_owned)[0]
    order = keep[np.argsort(sides[keep], kind="stable")]
    counts = np.bincount(sides[keep], minlength=n_owned)[:n_owned]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), order.astype(np.int32)


@pytest.mark.parametrize("name", list(MESHES))
def test_csr_matches_an_argsort_construction(name):
    part = MESHES[name]()
    off, ent = fields.cell_faces(part.N, part.F, part.face_neighbors)
    want_off, want_ent = csr_by_argsort(part.N, part.F, part.face_neighbors)
    assert off.dtype == np.int32 and ent.dtype == np.int32 and off.shape == (part.N + 1,)
    assert np.array_equal(off, want_off)
    assert np.array_equal(ent, want_ent)
    for e in (0, part.N // 2, part.N - 1):                       # within a row the entries ascend in f
        row = ent[off[e]:off[e + 1]]
        assert np.all(np.diff(row >> 1) >= 0) and np.all(part.face_neighbors[row] == e)


def test_ghosts_get_no_rows_and_a_ghost_face_has_one_entry():
    part = SynthMesh(2, 2, 4, band=0.2).partition(1, 3)
    assert part.G > 0
    off, ent = fields.cell_faces(part.N, part.F, part.face_neighbors)
    fn = part.face_neighbors[: 2 * part.F].reshape(-1, 2)
    ghost_sides = int((fn >= part.N).sum())
    assert ghost_sides > 0 and off[-1] == ent.size == 2 * part.F - ghost_sides
    per_face = np.bincount(ent >> 1, minlength=part.F)
    assert np.array_equal(per_face, (fn < part.N).sum(axis=1))   # one entry where a side is a ghost, two otherwise
    assert np.all(part.face_neighbors[ent] < part.N)


def test_large_meshes_take_the_threaded_scan_and_give_the_same_rows():
    """above the size where the element range is split over the OpenMP threads"""
    part = SynthMesh(2, 6, 7, band=0.2).partition()
    assert part.N >= 4096 and part.F >= 4096
    off, ent = fields.cell_faces(part.N, part.F, part.face_neighbors)
    want_off, want_ent = csr_by_argsort(part.N, part.F, part.face_neighbors)
    assert np.array_equal(off, want_off) and np.array_equal(ent, want_ent)


def test_cell_faces_refuses_invalid_arguments():
    f = synth.lib().t8gpu_host_cell_faces
    f.restype = C.c_int64
    f.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    fn = np.array([0, 1, 1, 2], np.int32)
    off, ent = np.zeros(4, np.int32), np.zeros(4, np.int32)
    assert f(3, 2, fn.ctypes.data, off.ctypes.data, ent.ctypes.data) == 4
    assert f(3, 2, None, off.ctypes.data, ent.ctypes.data) < 0
    assert f(3, 2, fn.ctypes.data, None, ent.ctypes.data) < 0
    assert f(3, 2, fn.ctypes.data, off.ctypes.data, None) < 0
    assert f(-1, 2, fn.ctypes.data, off.ctypes.data, ent.ctypes.data) < 0
    assert f(3, -1, fn.ctypes.data, off.ctypes.data, ent.ctypes.data) < 0
    assert f(3, 1 << 30, fn.ctypes.data, off.ctypes.data, ent.ctypes.data) < 0     # 2 f + side would not fit
    bad = np.array([0, 1, -1, 2], np.int32)
    assert f(3, 2, bad.ctypes.data, off.ctypes.data, ent.ctypes.data) < 0
    assert f(0, 0, None, off.ctypes.data, None) == 0 and off[0] == 0               # nothing owned, no faces: an empty CSR
    with pytest.raises(ValueError):
        fields.cell_faces(3, 2, bad)
    with pytest.raises(ValueError):
        fields.cell_faces(3, 4, fn)


class _Vars(C.Structure):
    _fields_ = [("p", C.c_void_p * 5)]


def _vars(addr):
    v = _Vars()
    for k in range(5):
        v.p[k] = addr
    return v


def _planes(slots, addr=4096):
    p = fields.FieldPlanes()
    for k in slots:
        p.p[k] = addr
    return p


def test_the_field_entries_load_and_refuse_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) from the host-side checks; the fake addresses below are never dereferenced, and n <= 0 is 0"""
    lib = C.CDLL(build.build_hip())
    for name in ("t8gpu_hip_plain_fields_f32", "t8gpu_hip_plain_fields_f64", "t8gpu_hip_subgrid_fields_f32",
                 "t8gpu_hip_subgrid_fields_f64"):
        assert hasattr(lib, name), name
        getattr(lib, name).restype = C.c_int
    assert C.sizeof(fields.FieldPlanes) == 11 * 8
    buf, st = C.c_void_p(4096), _vars(4096)
    for f in (lib.t8gpu_hip_plain_fields_f32, lib.t8gpu_hip_plain_fields_f64):
        plain = lambda n, ndim, conn, csr, planes: f(n, ndim, st, conn, conn, conn, conn, csr, csr, planes, None)
        assert plain(0, 3, None, None, _planes([10])) == 0                         # n <= 0
        assert plain(-5, 7, None, None, _planes([10])) == 0
        assert plain(8, 1, buf, buf, _planes([0])) == 1                            # normal_dim outside {2, 3}
        assert plain(8, 4, buf, buf, _planes([6])) == 1
        assert plain(8, 3, buf, None, _planes([9])) == 1                           # a gradient plane without the CSR
        assert plain(8, 2, None, buf, _planes([0, 10])) == 1                       # ... without the face arrays
    for f in (lib.t8gpu_hip_subgrid_fields_f32, lib.t8gpu_hip_subgrid_fields_f64):
        sub = lambda rank, n, conn, csr, planes: f(rank, n, st, conn, conn, conn, conn, conn, conn, csr, csr, planes, None)
        assert sub(3, 0, None, None, _planes([6])) == 0
        assert sub(1, 8, buf, buf, _planes([0])) == 1                              # rank outside {2, 3}
        assert sub(4, 8, buf, buf, _planes([6])) == 1
        assert sub(3, 8, buf, None, _planes([6, 7, 8])) == 1
        assert sub(2, 8, None, buf, _planes([10])) == 1


def test_field_names_and_slots():
    assert fields.FIELDS == {"pressure": (0, 1), "velocity": (1, 3), "mach": (4, 1), "entropy": (5, 1), "vorticity": (6, 3),
                             "dilatation": (9, 1), "schlieren": (10, 1)}
    assert sorted(k for first, n in fields.FIELDS.values() for k in range(first, first + n)) == list(range(11))


def test_kernel_source_hash_is_the_one_of_the_committed_c4_profile():
    """fields.hip is an output pass, not a stage kernel: it and its helpers stay out of the hashed sources, so the c4
    traffic record (tied to the hash) stays valid. The record is the one scripts/commit_profile.py wrote for
    profiles/r12_c4_f64_stage.md, taken when the Subgrid stage kernels became three templates with a MODE argument
    (kernels_subgrid_fused.hip, and BoundaryMode moved from compat_faces.hpp to fused_common.hpp, among the hashed files; c4
    launches none of the changed kernels: its kernels are those of r09, their device code unchanged)."""
    records = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    tied = [r for r in records.values() if isinstance(r, dict) and r.get("source") == "profiles/r12_c4_f64_stage.md"]
    assert len(tied) == 1 and tied[0]["kernel_source_hash"] == "84e6587bfd4c805f"
    assert build.kernel_source_hash() == tied[0]["kernel_source_hash"]
    assert os.path.exists(os.path.join(build.CSRC, "hip", "fields.hip"))
