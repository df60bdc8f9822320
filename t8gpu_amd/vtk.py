"""VTK output and host read-back: mirrors of
  MeshManager::get_host_scalar_variable / get_host_vector_variable / save_variables_to_vtk
      t8gpu/mesh/mesh_manager.inl:516-623
  SubgridMeshManager::save_variable_to_vtk / save_mesh_to_vtk / get_host_*_variable
      t8gpu/mesh/subgrid_mesh_manager.inl:1051-1206
The device side (cast to double, xyz interleave, column-major -> z-order) runs in
csrc/hip/kernels_readback.hip; the file is written by csrc/host/vtk_writer.cpp (a .vtu piece per rank and
a .pvtu from rank 0), which stands where the reference calls t8_forest_write_vtk_ext.
"""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import hip, synth

SCALAR, VECTOR = 1, 3   # T8_VTK_SCALAR / T8_VTK_VECTOR: components per cell


@dataclass
class HostVariableInfo:
    """mesh_manager.h: HostVariableInfo -- a named host array of doubles ready for the writer."""
    type: int
    data: np.ndarray
    name: str


def _host_lib():
    lib = synth.lib()
    lib.t8gpu_host_write_vtu.restype = C.c_int
    lib.t8gpu_host_write_vtu.argtypes = [C.c_char_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.t8gpu_host_write_pvtu.restype = C.c_int
    lib.t8gpu_host_write_pvtu.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def _own_cells(solver):
    return solver.N * getattr(solver, "S", 1)


def _variable(solver, step, variable):
    return solver.step_planes(step)[variable][: _own_cells(solver)]


def get_host_scalar_variable(solver, step, variable, name):
    """One variable of one step as doubles on the host (owned cells, storage order)."""
    n = _own_cells(solver)
    v = _variable(solver, step, variable)
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    hip.call("t8gpu_hip_host_scalar_variable", v.dtype, C.c_size_t(n), hip.ptr(v), hip.ptr(out), hip.stream_ptr())
    return HostVariableInfo(SCALAR, out.cpu().numpy(), name)


def get_host_vector_variable(solver, step, variables, name):
    """Three variables as interleaved xyz doubles on the host."""
    n = _own_cells(solver)
    v = [_variable(solver, step, k) for k in variables]
    out = torch.empty(3 * n, dtype=torch.float64, device="cuda")
    hip.call("t8gpu_hip_host_vector_variable", v[0].dtype, C.c_size_t(n), hip.ptr(v[0]), hip.ptr(v[1]), hip.ptr(v[2]), hip.ptr(out),
             hip.stream_ptr())
    return HostVariableInfo(VECTOR, out.cpu().numpy().reshape(n, 3), name)


def column_major_to_z_order(solver, values):
    """Per-cell device array of a Subgrid solver, storage order -> z-order of the twice-refined blocks."""
    out = torch.empty_like(values)
    hip.call("t8gpu_hip_column_major_to_z_order", values.dtype, C.c_int(solver.rank), C.c_int(solver.N), hip.ptr(values), hip.ptr(out),
             hip.stream_ptr())
    return out


def get_host_derived_variable(solver, name, step=None, halo=None):
    """One derived output field (solver.derived_fields: "pressure", "vorticity", ...) as doubles on the host, ready for
    save_variables_to_vtk: a scalar as it is, a vector interleaved xyz; for a Subgrid solver every plane in z-order first."""
    t = solver.derived_fields([name], step, halo=halo)[name]
    planes = [t] if t.dim() == 1 else [t[k] for k in range(3)]
    if hasattr(solver, "S"):
        planes = [column_major_to_z_order(solver, p.contiguous()) for p in planes]
    n = _own_cells(solver)
    if len(planes) == 1:
        return HostVariableInfo(SCALAR, planes[0].cpu().numpy(), name)
    out = torch.empty(3 * n, dtype=torch.float64, device="cuda")
    hip.call("t8gpu_hip_host_vector_variable", torch.float64, C.c_size_t(n), hip.ptr(planes[0]), hip.ptr(planes[1]), hip.ptr(planes[2]),
             hip.ptr(out), hip.stream_ptr())
    return HostVariableInfo(VECTOR, out.cpu().numpy().reshape(n, 3), name)


def get_host_statistics_variable(stats, name):
    """One result of a stats.Statistics (stats.RESULTS: "mean_density", "mean_velocity", "tke", ...) as doubles on the host,
    ready for save_variables_to_vtk: a scalar as it is, a 3-vector interleaved xyz; the 6-component "reynolds_stress" as a
    list of six scalars reynolds_stress_xx .. _yz (the writer knows scalars and 3-vectors). For a Subgrid solver every
    plane in z-order first."""
    from . import stats as st
    solver = stats.solver
    t = stats.results([name])[name]
    planes = [t] if t.dim() == 1 else [t[k] for k in range(t.shape[0])]
    if hasattr(solver, "S"):
        planes = [column_major_to_z_order(solver, p.contiguous()) for p in planes]
    n = _own_cells(solver)
    if len(planes) == 3:
        out = torch.empty(3 * n, dtype=torch.float64, device="cuda")
        hip.call("t8gpu_hip_host_vector_variable", torch.float64, C.c_size_t(n), hip.ptr(planes[0]), hip.ptr(planes[1]),
                 hip.ptr(planes[2]), hip.ptr(out), hip.stream_ptr())
        return HostVariableInfo(VECTOR, out.cpu().numpy().reshape(n, 3), name)
    infos = [HostVariableInfo(SCALAR, p.cpu().numpy(), label) for p, label in zip(planes, st.plane_names(name))]
    return infos[0] if len(infos) == 1 else infos


def get_host_indicator_variable(solver, indicator, name="indicator", halo=None, step=None):
    """The per-cell values of a refinement indicator (amr.Loehner.cell_values) as doubles on the host, ready for
    save_variables_to_vtk; for a Subgrid solver in z-order, as get_host_derived_variable."""
    t = indicator.cell_values(solver, step, halo=halo)
    if hasattr(solver, "S"):
        t = column_major_to_z_order(solver, t)
    return HostVariableInfo(SCALAR, t.cpu().numpy(), name)


def _write(solver, fields, prefix, dist, ascii):
    part = solver.part
    rank, nranks = part.rank, part.nranks
    piece = f"{prefix}_{rank:04d}.vtu" if nranks > 1 else f"{prefix}.vtu"
    names = (C.c_char_p * len(fields))(*[f.name.encode() for f in fields])
    comps = np.array([f.type for f in fields], np.int32)
    arrays = [np.ascontiguousarray(f.data, np.float64) for f in fields]
    ptrs = (C.c_void_p * len(fields))(*[a.ctypes.data for a in arrays])
    centres = np.ascontiguousarray(part.centres[: part.N])
    levels = np.ascontiguousarray(part.levels[: part.N])
    rc = _host_lib().t8gpu_host_write_vtu(piece.encode(), part.mesh.dim, part.N, centres.ctypes.data, levels.ctypes.data,
                                          4 if part.subgrid else 1, rank, part.first_global, len(fields), names,
                                          comps.ctypes.data, ptrs, int(ascii))
    if rc != 0:
        raise OSError(f"t8gpu_host_write_vtu({piece}) failed with code {rc}")
    if nranks > 1:
        if dist is not None:
            dist.barrier()
        if rank == 0:
            files = (C.c_char_p * nranks)(*[os.path.basename(f"{prefix}_{r:04d}.vtu").encode() for r in range(nranks)])
            rc = _host_lib().t8gpu_host_write_pvtu(f"{prefix}.pvtu".encode(), nranks, files, len(fields), names, comps.ctypes.data)
            if rc != 0:
                raise OSError(f"t8gpu_host_write_pvtu({prefix}.pvtu) failed with code {rc}")
    return piece


def save_variables_to_vtk(solver, host_variables, prefix, dist=None, ascii=False):
    """MeshManager::save_variables_to_vtk (mesh_manager.inl:588-623). For a Subgrid solver the arrays must
    already be in z-order (see save_variable_to_vtk)."""
    return _write(solver, list(host_variables), prefix, dist, ascii)


def save_variable_to_vtk(solver, step, variable, prefix, dist=None, ascii=False):
    """SubgridMeshManager::save_variable_to_vtk (subgrid_mesh_manager.inl:1051-1138): the variable on the
    twice-refined forest, field name "variables"."""
    z = column_major_to_z_order(solver, _variable(solver, step, variable).contiguous())
    out = torch.empty(z.numel(), dtype=torch.float64, device="cuda")
    hip.call("t8gpu_hip_host_scalar_variable", z.dtype, C.c_size_t(z.numel()), hip.ptr(z), hip.ptr(out), hip.stream_ptr())
    return _write(solver, [HostVariableInfo(SCALAR, out.cpu().numpy(), "variables")], prefix, dist, ascii)


def save_mesh_to_vtk(solver, prefix, dist=None, ascii=False):
    """SubgridMeshManager::save_mesh_to_vtk (subgrid_mesh_manager.inl:1185-1206): the forest, no data."""
    part = solver.part
    centres = np.ascontiguousarray(part.centres[: part.N])
    levels = np.ascontiguousarray(part.levels[: part.N])
    piece = f"{prefix}_{part.rank:04d}.vtu" if part.nranks > 1 else f"{prefix}.vtu"
    rc = _host_lib().t8gpu_host_write_vtu(piece.encode(), part.mesh.dim, part.N, centres.ctypes.data, levels.ctypes.data, 1, part.rank,
                                          part.first_global, 0, None, None, None, int(ascii))
    if rc != 0:
        raise OSError(f"t8gpu_host_write_vtu({piece}) failed with code {rc}")
    return piece
