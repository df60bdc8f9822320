"""Boundary budgets: what crosses the boundary of a solver's state, per group of boundary faces, from one pass
of t8gpu_hip_boundary_fluxes_* / t8gpu_hip_subgrid_boundary_fluxes_* (csrc/hip/kernels_boundary.hip) -- the scheme's own
numerical flux through every boundary face along the outward normal, the wall pressure force, the mass leaving and entering.
monitor() gives the change of the five integrals; with these sums the conservation check extends to domains with open sides:
change of the integral + dt * boundary flux = 0, stage by stage.

The public entry points are methods of both solver classes (solver.py): boundary_fluxes_device, boundary_fluxes,
boundary_step_fluxes. Grouping: by boundary kind (the default), by side (side_groups), or by any uint8 label per face."""
import ctypes as C

import numpy as np
import torch

from . import hip

SLOTS = 16                       # T8GPU_BOUNDARY_SLOTS
GROUPS_MAX = 32                  # T8GPU_BOUNDARY_GROUPS_MAX
KIND_GROUPS = 16                 # boundary kinds are codes 0 .. 15 (t8gpu_host.h): group index = kind code
ACCUMULATED = slice(0, 11)       # the slots the accumulating form adds to; 11-12 are those of the last call

# SSP-RK3 as the stage kernels run it (csrc/hip/flux_math.hpp: rk3c), with the truncated literals of the reference
_RK3C = {torch.float64: (0.25, 0.25, 0.66666666666666, 0.66666666666666),
         torch.float32: tuple(float(np.float32(x)) for x in (0.25, 0.25, 0.66666666666666, 0.66666666666666))}


def step_weights(dtype, delta_t):
    """The weights of the three stage source states (prev, STEP1, STEP2) in the boundary flux of one step: with the stages
    I1 = I0 - dt B0, I2 = c21 I0 + c22 I1 - c23 dt B1, I3 = c31 I0 + c32 I2 - c33 dt B2 the step is
    I3 = (c31 + c32 (c21 + c22)) I0 - dt (c32 c22 B0 + c32 c23 B1 + c33 B2)."""
    c22, c23, c32, c33 = _RK3C[dtype]
    return (c32 * c22 * delta_t, c32 * c23 * delta_t, c33 * delta_t)


class BoundaryFluxes:
    """What one pass of t8gpu_hip_boundary_fluxes_* says about a state (include/t8gpu_hip.h): `block[G, 16]` holds
    the raw doubles of the G groups, the attributes name its slots, one entry per group. Every slot is a sum over the faces
    (Subgrid: sub-faces) of the group; fluxes are along the OUTWARD normal, so a positive mass_flow leaves the domain.
    momentum_flux is the force the fluid exerts on that part of the boundary as the scheme sees it (on a wall the scheme's wall
    pressure times the area vector), pressure_force the same from the inside cells' pressures. Faces with a non-finite flux are
    counted in `nonfinite` and add nothing to the other sums."""
    SLOTS = SLOTS
    __slots__ = ("block",)

    def __init__(self, block):
        self.block = np.array(block, np.float64, copy=True).reshape(-1, SLOTS)

    area = property(lambda self: self.block[:, 0])
    flux = property(lambda self: self.block[:, 1:6])
    mass_flow = property(lambda self: self.block[:, 1])
    momentum_flux = property(lambda self: self.block[:, 2:5])
    energy_flow = property(lambda self: self.block[:, 5])
    pressure_force = property(lambda self: self.block[:, 6:9])
    mass_out = property(lambda self: self.block[:, 10])
    mass_in = property(lambda self: self.block[:, 10] - self.block[:, 1])
    faces = property(lambda self: self.block[:, 11].astype(np.int64))
    nonfinite = property(lambda self: self.block[:, 12].astype(np.int64))

    @property
    def mean_pressure(self):
        a = self.block[:, 0]
        return np.divide(self.block[:, 9], a, out=np.full(a.shape, np.nan), where=a > 0)

    def total(self):
        """the sum over the groups: a BoundaryFluxes of one group"""
        return BoundaryFluxes(self.block.sum(axis=0))

    def __repr__(self):
        live = np.flatnonzero(self.block[:, 11] > 0)
        rows = ", ".join(f"{g}: area={self.area[g]:.6g} flux={self.flux[g].tolist()} mass_out={self.mass_out[g]:.6g} "
                         f"pressure_force={self.pressure_force[g].tolist()} faces={self.faces[g]} nonfinite={self.nonfinite[g]}"
                         for g in live)
        return f"BoundaryFluxes(groups={self.block.shape[0]}, {{{rows}}})"

    @staticmethod
    def combine(blocks):
        """The fluxes of several ranks' blocks (BoundaryFluxes objects or arrays [G, 16] of the same grouping): every slot is
        a sum. A rank without boundary faces contributes zeros. Pure numpy: needs no GPU."""
        b = [np.asarray(getattr(x, "block", x), np.float64).reshape(-1, SLOTS) for x in blocks]
        if len({x.shape for x in b}) != 1:
            raise ValueError("combine needs blocks of one grouping (the same number of groups)")
        return BoundaryFluxes(np.sum(np.stack(b), axis=0))


def kind_groups(part):
    """uint8 [B]: the boundary kind code of every boundary face (0 where the partition sets none: walls)"""
    kinds = getattr(part, "boundary_kinds", None)
    return np.zeros(part.B, np.uint8) if kinds is None else np.array(kinds, np.uint8, copy=True)


def side_groups(part):
    """uint8 [B]: the side of every boundary face. Cartesian partitions (synth.Partition): 2 * axis + (1 if the outward
    normal points along +axis), so -x, +x, -y, +y, -z, +z are 0 .. 5. Curved meshes (unstructured.py): the mesh's
    boundary_side, which the partition carries (under shell_map 0 is the inner radius and 1 the outer)."""
    side = getattr(part, "boundary_side", None)
    if side is not None:
        return np.array(side, np.uint8, copy=True)
    nd = part.normal_dim
    n = np.asarray(part.normals, np.float64).reshape(-1, nd)[part.F:]
    if n.shape[0] == 0:
        return np.zeros(0, np.uint8)
    axis = np.abs(n).argmax(axis=1)
    along = n[np.arange(n.shape[0]), axis]
    if not np.all(np.abs(along) == 1.0):
        raise ValueError("side groups need axis-aligned boundary normals or a partition with boundary_side")
    return (2 * axis + (along > 0)).astype(np.uint8)


def resolve_groups(part, groups):
    """(cache key, uint8 labels [B], number of groups) of a `groups` argument: None = by kind (16 groups, index = kind code),
    "side" (2 * dim groups), or a uint8 array [B] with values < 32 (32 groups). Anything else raises ValueError. The number of
    groups depends on the grouping only, never on the faces a rank happens to own, so ranks' blocks combine."""
    if groups is None:
        return "kind", kind_groups(part), KIND_GROUPS
    if isinstance(groups, str):
        if groups != "side":
            raise ValueError(f"groups must be None, \"side\" or a uint8 array [B], got {groups!r}")
        return "side", side_groups(part), 2 * int(part.mesh.dim)
    if not isinstance(groups, (np.ndarray, torch.Tensor)):
        raise ValueError(f"groups must be None, \"side\" or a uint8 array [B], got {type(groups).__name__}")
    g = groups.cpu().numpy() if isinstance(groups, torch.Tensor) else groups
    if g.dtype != np.uint8:
        raise ValueError(f"groups must be uint8, got {g.dtype}")
    if g.shape != (part.B,):
        raise ValueError(f"groups must have one entry per boundary face: shape ({part.B},), got {g.shape}")
    if g.size and int(g.max()) >= GROUPS_MAX:
        raise ValueError(f"group ids must be < {GROUPS_MAX}, got {int(g.max())}")
    g = np.ascontiguousarray(g)
    return g.tobytes(), g, GROUPS_MAX


def sorted_faces(labels, num_groups):
    """(order int32 [B], offsets int32 [num_groups + 1]): the boundary faces in a stable sort by group and the first position
    of every group in it -- the face_order / group_offsets of the C calls"""
    labels = np.asarray(labels, np.uint8)
    order = np.argsort(labels, kind="stable").astype(np.int32)
    offsets = np.zeros(num_groups + 1, np.int32)
    offsets[1:] = np.cumsum(np.bincount(labels, minlength=num_groups)[:num_groups])
    return order, offsets


class _Entry:
    """what one grouping of one solver keeps on the device: the sorted face list, the offsets (host), the workspace, the
    result block, the block the step integral accumulates in, and a pinned host block"""

    def __init__(self, solver, labels, num_groups):
        order, offsets = sorted_faces(labels, num_groups)
        self.num_groups = num_groups
        self.order = torch.from_numpy(order).cuda() if order.size else None
        self.offsets = (C.c_int32 * (num_groups + 1))(*offsets.tolist())
        n = hip.lib().t8gpu_hip_boundary_fluxes_workspace_bytes
        n.restype = C.c_size_t
        self.workspace = torch.zeros(n(int(solver.B), num_groups) // 8, dtype=torch.float64, device="cuda")
        self.result = torch.zeros((num_groups, SLOTS), dtype=torch.float64, device="cuda")
        self.integral = torch.zeros((num_groups, SLOTS), dtype=torch.float64, device="cuda")
        self.host = torch.zeros((num_groups, SLOTS), dtype=torch.float64).pin_memory()


def _entry(solver, groups):
    cache = solver.__dict__.setdefault("_boundary_cache", {})
    key, labels, num_groups = resolve_groups(solver.part, groups)
    if key not in cache:
        cache[key] = _Entry(solver, labels, num_groups)
    return cache[key]


def _launch(solver, entry, step, stream, result, accumulate, weight):
    s = solver.next if step is None else step
    subgrid = hasattr(solver, "S")
    head = (solver.kind, solver.rank, solver.F, solver.B) if subgrid else (solver.kind, solver.F, solver.B, solver.ndim)
    hip.call("t8gpu_hip_subgrid_boundary_fluxes" if subgrid else "t8gpu_hip_boundary_fluxes", solver.dtype, *head,
             hip.ptr(solver.fn), hip.ptr(solver.kinds),
             hip.ptr(solver.inflow_table), hip.ptr(solver.normals), hip.ptr(solver.areas), solver.get_own_variables(s),
             entry.num_groups, hip.ptr(entry.order), entry.offsets, hip.ptr(entry.workspace), hip.ptr(result),
             int(accumulate), C.c_double(weight), hip.stream_ptr(stream))


def boundary_fluxes_device(solver, step=None, groups=None, stream=None, out=None, weight=None):
    entry = _entry(solver, groups)
    if weight is not None and out is None:
        raise ValueError("weight selects the accumulating form: it needs `out`")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or not out.is_cuda or
                            not out.is_contiguous() or tuple(out.shape) != (entry.num_groups, SLOTS)):
        raise ValueError(f"out must be a contiguous float64 device tensor [{entry.num_groups}, {SLOTS}]")
    result = entry.result if out is None else out
    _launch(solver, entry, step, stream, result, weight is not None, 0.0 if weight is None else float(weight))
    return result


def _to_host(entry, block, stream, dist):
    with torch.cuda.stream(stream):
        entry.host.copy_(block, non_blocking=True)
    stream.synchronize()
    host = entry.host.numpy().copy()
    if dist is not None:
        t = torch.from_numpy(host).to("cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        host = t.cpu().numpy()
    return BoundaryFluxes(host)


def boundary_fluxes(solver, step=None, groups=None, stream=None, dist=None):
    stream = torch.cuda.current_stream() if stream is None else stream
    entry = _entry(solver, groups)
    _launch(solver, entry, step, stream, entry.result, False, 0.0)
    return _to_host(entry, entry.result, stream, dist)


class Budget:
    """A run loop's conservation budget on a domain with open sides: the boundary flux of every step taken, integrated in time
    on the device (the accumulating form: three passes per step, no copy, no sync), against the change of monitor()'s five
    integrals. groups = None or "side": the block keeps its shape across an adapt, so the budget outlives the solver it was
    started with (an adapt conserves the integrals).

        budget = Budget(solver)
        ... solver.iterate(dt); budget.add_step(solver, dt) ...
        print(budget.line(solver))            # per report interval: one copy, one sync; starts the next interval"""

    def __init__(self, solver, groups=None):
        if not (groups is None or groups == "side"):
            raise ValueError("a Budget groups by kind (None) or by \"side\"")
        self.groups = groups
        count = resolve_groups(solver.part, groups)[2]
        self.integral = torch.zeros((count, SLOTS), dtype=torch.float64, device="cuda")
        self.start = solver.monitor().integrals.copy()

    def add_step(self, solver, delta_t, stream=None):
        """after solver.iterate(delta_t) (or the last step of iterate_steps): that step's boundary flux into the integral"""
        from .solver import STEP1, STEP2
        for step, w in zip((solver.prev, STEP1, STEP2), step_weights(solver.dtype, float(delta_t))):
            boundary_fluxes_device(solver, step, self.groups, stream, out=self.integral, weight=w)

    def report(self, solver):
        """(change of the five integrals since the last report, time-integrated boundary flux summed over the groups, their
        sum -- 0 to rounding in a closed budget --, the BoundaryFluxes of the interval); starts the next interval"""
        now = solver.monitor().integrals.copy()
        fluxes = BoundaryFluxes(self.integral.cpu().numpy())
        through = fluxes.total().flux[0].copy()
        change = now - self.start
        self.start = now
        self.integral.zero_()
        return change, through, change + through, fluxes

    def line(self, solver):
        change, through, residual, _ = self.report(solver)
        return (f"budget: d(mass) {change[0]:+.6e} = -boundary {-through[0]:+.6e}, difference {residual[0]:+.2e} | "
                f"d(energy) {change[4]:+.6e} = -boundary {-through[4]:+.6e}, difference {residual[4]:+.2e}")


def boundary_step_fluxes(solver, delta_t, groups=None, stream=None, dist=None):
    from .solver import STEP1, STEP2
    stream = torch.cuda.current_stream() if stream is None else stream
    entry = _entry(solver, groups)
    with torch.cuda.stream(stream):
        entry.integral.zero_()
    for step, w in zip((solver.prev, STEP1, STEP2), step_weights(solver.dtype, float(delta_t))):
        _launch(solver, entry, step, stream, entry.integral, True, w)
    return _to_host(entry, entry.integral, stream, dist)
