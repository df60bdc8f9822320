"""Derived output fields on the device (csrc/hip/fields.hip, include/t8gpu_hip.h: t8gpu_hip_plain_fields_*,
t8gpu_hip_subgrid_fields_*): pressure, velocity, Mach number and entropy cell by cell, vorticity,
dilatation and schlieren from the jump form of the Green-Gauss gradient over a cell's interior faces. All in double,
gamma = 1.4, for both solver classes; boundary faces contribute no term. `_Solver.derived_fields` is the entry point,
`vtk.get_host_derived_variable` the way into a .vtu file.
"""
import ctypes as C

import numpy as np
import torch

from . import hip, synth

PLANES = 11
# name -> (first plane, planes): the slot table of include/t8gpu_hip.h
FIELDS = {"pressure": (0, 1), "velocity": (1, 3), "mach": (4, 1), "entropy": (5, 1),
          "vorticity": (6, 3), "dilatation": (9, 1), "schlieren": (10, 1)}
GRADIENT_FIELDS = ("vorticity", "dilatation", "schlieren")      # planes 6-10: the ones that read neighbours


class FieldPlanes(C.Structure):
    """T8gpuFieldPlanes: the eleven output planes, NULL = not asked for"""
    _fields_ = [("p", C.c_void_p * PLANES)]


def cell_faces(n_owned, num_faces, face_neighbors):
    """(offsets[n_owned + 1], entries) of t8gpu_host_cell_faces: the CSR element -> interior faces, entry 2 f + side (side 0:
    the element is l of face f), ascending in f; rows for the owned elements only. Host arrays in, host arrays out."""
    lib = synth.lib()
    f = lib.t8gpu_host_cell_faces
    f.restype = C.c_int64
    f.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    fn = np.ascontiguousarray(face_neighbors, np.int32)
    if fn.size < 2 * num_faces:
        raise ValueError(f"face_neighbors holds {fn.size} entries, {num_faces} interior faces need {2 * num_faces}")
    offsets = np.empty(n_owned + 1, np.int32)
    entries = np.empty(max(1, 2 * num_faces), np.int32)
    count = f(n_owned, num_faces, fn.ctypes.data, offsets.ctypes.data, entries.ctypes.data)
    if count < 0:
        raise ValueError(f"t8gpu_host_cell_faces refused its arguments ({count})")
    return offsets, entries[:count]


def _csr(solver):
    """the solver's CSR on the device: built and uploaded on the first gradient request, then kept (a solver's mesh never
    changes; an adapt makes a new solver)"""
    if getattr(solver, "_cell_faces", None) is None:
        offsets, entries = cell_faces(solver.N, solver.F, solver.part.face_neighbors)
        if entries.size == 0:
            entries = np.zeros(1, np.int32)                       # (no interior face: a valid pointer all the same)
        solver._cell_faces = (torch.from_numpy(offsets).cuda(), torch.from_numpy(entries).cuda())
    return solver._cell_faces


def derived_fields(solver, names, step=None, stream=None, halo=None):
    """{name: float64 device tensor} of the fields `names` (FIELDS) for the owned cells of state(step) in storage order:
    shape [cells], or [3, cells] for velocity and vorticity. One kernel launch enqueued on `stream` (default: the current
    stream), no sync; only the planes asked for are computed. The gradient fields read the cells across a cell's interior
    faces, ghost slots included: `halo` (a HaloExchange) refreshes the ghost slots of that step's planes first; without it
    the caller vouches that they are current, as for the AMR indicator. An unknown name raises ValueError."""
    names = [names] if isinstance(names, str) else list(names)
    for name in names:
        if name not in FIELDS:
            raise ValueError(f"unknown derived field {name!r}: one of {', '.join(FIELDS)}")
    s = solver.next if step is None else step
    stream = torch.cuda.current_stream() if stream is None else stream
    cells = solver.owned_cells
    out, planes = {}, FieldPlanes()
    with torch.cuda.stream(stream):
        for name in dict.fromkeys(names):
            first, count = FIELDS[name]
            t = torch.empty((count, cells), dtype=torch.float64, device="cuda")
            for k in range(count):
                planes.p[first + k] = t[k].data_ptr()
            out[name] = t if count == 3 else t[0]
        gradient = any(name in GRADIENT_FIELDS for name in names)
        if gradient and halo is not None:
            halo.exchange(solver.step_planes(s))
    off, ent = _csr(solver) if gradient else (None, None)
    st, sp = solver.get_own_variables(s), hip.stream_ptr(stream)
    if hasattr(solver, "S"):
        hip.call("t8gpu_hip_subgrid_fields", solver.dtype, solver.rank, solver.N, st, hip.ptr(solver.volumes), hip.ptr(solver.fn),
                 hip.ptr(solver.level_diff), hip.ptr(solver.nb_offset), hip.ptr(solver.normals), hip.ptr(solver.areas),
                 hip.ptr(off), hip.ptr(ent), planes, sp)
    elif gradient:
        hip.call("t8gpu_hip_plain_fields", solver.dtype, solver.N, solver.ndim, st, hip.ptr(solver.get_own_volume()),
                 hip.ptr(solver.fn), hip.ptr(solver.normals), hip.ptr(solver.areas), hip.ptr(off), hip.ptr(ent), planes, sp)
    else:       # (no neighbour is read: the per-face geometry of a fused run stays on the host)
        hip.call("t8gpu_hip_plain_fields", solver.dtype, solver.N, solver.ndim, st, None, None, None, None, None, None, planes, sp)
    return out
