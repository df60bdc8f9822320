"""Host-side mirrors of the reference solvers' hot loop, driving the C-ABI of include/t8gpu_hip.h.

PlainSolver   <-> t8gpu::CompressibleEulerSolver::iterate   (examples/compressible_euler/solver.cu:75-175)
SubgridSolver <-> SubgridCompressibleEulerSolver::iterate   (examples/subgrid/solver.inl:152-266)

Same member names and step bookkeeping (`next`/`prev` swap, Step0..Step3 + Fluxes planes,
plane = step*5 + var, stride = capacity). torch is used for device memory and streams only; every
flux / RK computation is a HIP kernel behind the C-ABI. There is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import hip, native
from .synth import FARFIELD

STEP0, STEP1, STEP2, STEP3, FLUXES = range(5)


def _timer_begin(solver):
    """bench.py sets solver.kernel_timer to a list to get (start, end) HIP events around the
    dominant kernel, recorded on the stream the kernel is launched on (torch's current stream)."""
    if getattr(solver, "kernel_timer", None) is None:
        return None
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    return ev


def _timer_end(solver, ev):
    if ev is not None:
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        solver.kernel_timer.append((ev, end))


def _dev(a, dtype=None):
    from . import hostmem
    return hostmem.to_device(a, dtype)          # (tensor.cuda(), or the application's pinned staging buffer: hostmem.py)


def boundary_kinds_of(part):
    """part.boundary_kinds as uint8 (None: the provider sets none -- every boundary face a wall)"""
    kinds = getattr(part, "boundary_kinds", None)
    return None if kinds is None else np.asarray(kinds, np.uint8)


def check_inflow_states(part, inflow_states):
    """The (K, 5) conservative inflow states as float64, or None. Required iff part.boundary_kinds holds an inflow code
    (2 + k) or a far-field code (10 + k: the far-field state is inflow state k); then K <= 8, every code has its state, and
    every state is a physical one (rho > 0, p > 0, finite). A partition without inflow or far-field faces takes them too (a
    rank of a partitioned mesh, an adapted mesh: the states travel with the run)."""
    from .synth import FARFIELD, INFLOW, MAX_INFLOW_STATES
    kinds = boundary_kinds_of(part)
    kinds = np.zeros(0, np.uint8) if kinds is None else kinds.astype(np.int64)
    inflow_k = kinds[(kinds >= INFLOW) & (kinds < FARFIELD)] - INFLOW
    far_k = kinds[kinds >= FARFIELD] - FARFIELD
    need = max(int(inflow_k.max()) + 1 if inflow_k.size else 0, int(far_k.max()) + 1 if far_k.size else 0)
    if inflow_states is None:
        if inflow_k.size:
            raise ValueError(f"the partition has inflow faces (states 0..{need - 1}): inflow_states is required")
        if far_k.size:
            raise ValueError(f"the partition has far-field faces (states 0..{need - 1}): inflow_states is required")
        return None
    s = np.array(inflow_states, np.float64, copy=True)
    if s.ndim != 2 or s.shape[1] != 5 or not 1 <= s.shape[0] <= MAX_INFLOW_STATES:
        raise ValueError(f"inflow_states must be a (K, 5) array of conservative states, 1 <= K <= {MAX_INFLOW_STATES}")
    if s.shape[0] < need:
        raise ValueError(f"the partition uses inflow / far-field state {need - 1}, inflow_states has {s.shape[0]}")
    if not np.all(np.isfinite(s)):
        raise ValueError("inflow_states must be finite")
    p = 0.4 * (s[:, 4] - 0.5 * (s[:, 1] ** 2 + s[:, 2] ** 2 + s[:, 3] ** 2) / np.where(s[:, 0] > 0, s[:, 0], 1.0))
    if np.any(s[:, 0] <= 0) or np.any(p <= 0):
        raise ValueError("inflow_states must have positive density and pressure (gamma = 1.4)")
    return s


class Monitor:
    """What one pass of t8gpu_hip_state_monitor_* says about a state (include/t8gpu_hip.h): `block` holds the raw
    16 doubles, the attributes name its slots. Sums run over the finite cells (kinetic energy: rho > 0 as well; entropy,
    max_speed, max_rate: the physical cells, finite with rho > 0 and p > 0; min_pressure: finite with rho > 0).
    entropy = sum vol * rho * (log p - 1.4 log rho): never decreases under the KEPES flux. max_rate = max (|v| + c) / h with the
    cell length h = vol^(1/dim); a CFL step is cfl / max_rate. With no qualifying cell the maxima are 0 and the minima +inf."""
    SLOTS = 16
    SUM_SLOTS, MAX_SLOTS, MIN_SLOTS = (0, 1, 2, 3, 4, 5, 6, 11, 12), (7, 8), (9, 10)
    __slots__ = ("block",)

    def __init__(self, block):
        self.block = np.array(block, np.float64, copy=True).reshape(self.SLOTS)

    integrals = property(lambda self: self.block[0:5])
    kinetic_energy = property(lambda self: float(self.block[5]))
    entropy = property(lambda self: float(self.block[6]))
    max_speed = property(lambda self: float(self.block[7]))
    max_rate = property(lambda self: float(self.block[8]))
    min_density = property(lambda self: float(self.block[9]))
    min_pressure = property(lambda self: float(self.block[10]))
    nonfinite = property(lambda self: int(self.block[11]))
    unphysical = property(lambda self: int(self.block[12]))

    def __repr__(self):
        return (f"Monitor(integrals={self.integrals.tolist()}, kinetic_energy={self.kinetic_energy}, entropy={self.entropy}, "
                f"max_speed={self.max_speed}, max_rate={self.max_rate}, min_density={self.min_density}, "
                f"min_pressure={self.min_pressure}, nonfinite={self.nonfinite}, unphysical={self.unphysical})")

    @staticmethod
    def combine(blocks):
        """The monitor of several ranks' blocks (Monitor objects or arrays of 16 doubles): sums, maxima and minima per slot
        class. A rank that owns nothing contributes its block of zeros and +inf minima. Pure numpy: needs no GPU."""
        b = np.stack([np.asarray(getattr(x, "block", x), np.float64).reshape(Monitor.SLOTS) for x in blocks])
        out = np.zeros(Monitor.SLOTS)
        out[list(Monitor.SUM_SLOTS)] = b[:, list(Monitor.SUM_SLOTS)].sum(axis=0)
        out[list(Monitor.MAX_SLOTS)] = b[:, list(Monitor.MAX_SLOTS)].max(axis=0)
        out[list(Monitor.MIN_SLOTS)] = b[:, list(Monitor.MIN_SLOTS)].min(axis=0)
        return Monitor(out)


class _Solver:
    """What PlainSolver and SubgridSolver share: the step roles (`next` / `prev`, solver.h:100-101), the stage loop with its
    halo overlap and both step drivers, and the state monitor. A solver supplies `owned_cells` (the columns of state()),
    `_units()` (tiles or blocks of its fused plan), `_stage_compat`, `_native_stepper`, and what the monitor and amr.py ask
    of it: `cell_geometry()` (dim, cells per element, the volume tensor) and `like(part)` (an empty solver of the same
    configuration on another partition)."""

    def __init__(self, part, dtype, flux_kind, mode):
        if not torch.cuda.is_available():
            raise hip.T8gpuHipError(f"{type(self).__name__} needs a GPU: the hot path has no CPU implementation")
        if mode not in ("compat", "fused"):
            raise ValueError(mode)
        hip.lib()
        self.part, self.dtype, self.kind, self.mode = part, dtype, flux_kind, mode
        self.N, self.G, self.F, self.B = part.N, part.G, part.F, part.B
        self.fn = _dev(part.face_neighbors)
        self.next, self.prev = STEP0, STEP3  # solver.h:100-101
        self.plan = self.stepper = None

    _STATE_SLOTS = 4    # pinned host copies of the states that may be on their way to the device at once (set_inflow_states)

    def _upload_open_boundaries(self, kinds, inflow_states):
        """device copies of the boundary kinds (compat kernels) and the inflow table (t8gpu_hip_plain_inflow_table_*), made once
        when self.open_boundaries is set (launches never allocate or copy); None otherwise. With them the staging buffers of
        set_inflow_states: a device block of (K, 5) states and a few pinned host copies of it."""
        self.inflow_states = inflow_states
        self.kinds = self.inflow_table = self._states_dev = None
        if self.open_boundaries:
            self.kinds = _dev(kinds) if kinds is not None and bool(np.any(kinds != 0)) else None   # (all walls: the wall kernel)
            states = inflow_states if inflow_states is not None else np.zeros((1, 5))   # (an outflow-only plan: never read)
            K = int(states.shape[0])
            self._states_dev = torch.from_numpy(np.ascontiguousarray(states)).to(self.dtype).cuda()
            self._states_host = torch.zeros((self._STATE_SLOTS, K, 5), dtype=self.dtype).pin_memory()
            self._states_sent = [torch.cuda.Event() for _ in range(self._STATE_SLOTS)]
            self._states_slot = 0
            self.inflow_table = torch.zeros((K, 16), dtype=self.dtype, device="cuda")
            hip.call("t8gpu_hip_plain_inflow_table", self.dtype, hip.ptr(self._states_dev), K, hip.ptr(self.inflow_table),
                     hip.stream_ptr())
            torch.cuda.current_stream().synchronize()

    def set_inflow_states(self, states, stream=None):
        """New inflow / far-field states for a running solver: a (K, 5) array of conservative states with the K of the
        constructor (check_inflow_states). The device table is refilled in place (t8gpu_hip_plain_inflow_table_*), ordered on
        `stream` (default: the current stream), so its address never changes and every later launch on that stream reads the
        new values: compat and fused stages, the native step driver, a replayed graph. Nothing is allocated and the host does
        not wait for the device (the states travel through a pinned host copy and a device staging block made with the solver;
        only a caller more than a few updates ahead of the device waits for the oldest copy). A rank of a partitioned run calls
        it like every other rank."""
        if self.inflow_table is None or self.inflow_states is None:
            raise ValueError("set_inflow_states needs a solver built with open boundaries and inflow_states")
        new = check_inflow_states(self.part, states)
        if new is None or new.shape != self.inflow_states.shape:
            raise ValueError(f"inflow_states must keep the shape {self.inflow_states.shape} of the states the solver was built with "
                             "(the device table's size and address are fixed)")
        stream = torch.cuda.current_stream() if stream is None else stream
        slot = self._states_slot
        self._states_slot = (slot + 1) % self._STATE_SLOTS
        self._states_sent[slot].synchronize()          # (a no-op unless this slot's last copy is still queued)
        self._states_host[slot].copy_(torch.from_numpy(new))
        with torch.cuda.stream(stream):
            self._states_dev.copy_(self._states_host[slot], non_blocking=True)
            self._states_sent[slot].record(stream)
        hip.call("t8gpu_hip_plain_inflow_table", self.dtype, hip.ptr(self._states_dev), int(new.shape[0]), hip.ptr(self.inflow_table),
                 hip.stream_ptr(stream))
        self.inflow_states = new

    def _like(self, part, **options):
        """like(part) of both solvers: what they share of "the same configuration" (dtype, flux kind, mode, inflow states),
        the class's own `options`, an all-zero state and the step roles. No stepper is attached."""
        new = type(self)(part, self.dtype, flux_kind=self.kind, mode=self.mode, state="zeros", inflow_states=self.inflow_states,
                         **options)
        new.next, new.prev = self.next, self.prev
        return new

    # -- accessors named after the reference API ------------------------------------------------
    def get_own_variables(self, step):
        return hip.vars_of(self.planes, step)

    def state(self, step=None):
        s = self.next if step is None else step
        return self.planes[5 * s:5 * s + 5, :self.owned_cells]

    def step_planes(self, step):
        return self.planes[5 * step:5 * step + 5]

    def begin_step(self):
        self.next, self.prev = self.prev, self.next  # solver.cu:76, solver.inl:154

    def stage_steps(self, k):
        """(source step, destination step) of RK stage k = 0, 1, 2 (solver.cu:81-174)."""
        return (self.prev, STEP1, STEP2)[k], (STEP1, STEP2, self.next)[k]

    def run_stage(self, k, delta_t, stream=None, halo=None, split=False):
        """Flux evaluation on the stage's source state + RK update. With a halo exchange (or split=True) the fused kernels run
        the interior tiles / blocks (those that read no ghost) first and the others after finish()."""
        s = hip.stream_ptr(stream)
        src, dst = self.stage_steps(k)
        ni, nt = (self.plan.host.n_interior, self._units()) if self.mode == "fused" else (0, 0)

        def stage(stream, *units):
            if self.mode == "compat":
                self._stage_compat(k + 1, src, dst, delta_t, stream)
            else:
                self.plan.stage(self, k + 1, src, dst, delta_t, stream, *units)

        if halo is not None and halo.overlapped and 0 < ni < nt:
            # boundary pipeline on the comm stream: ghosts, then the units that read them; the interior ones beside it
            halo.start(self.step_planes(src), then=lambda: stage(hip.stream_ptr(), ni, nt - ni))
            stage(s, 0, ni)
            halo.finish()
            return
        if halo is not None:
            halo.start(self.step_planes(src))
        if (halo is None and not split) or ni == nt or ni == 0:     # one launch (the compat tier: always)
            if halo is not None:
                halo.finish()
            stage(s)
            return
        stage(s, 0, ni)
        if halo is not None:
            halo.finish()
        stage(s, ni, nt - ni)

    def use_native_stepper(self, native_halo=None):
        """Drive iterate() through the C++ stepper (one C call per run of steps, RCCL called natively)."""
        assert self.mode == "fused"
        self.stepper = self._native_stepper(self.plan, native_halo)
        return self.stepper

    def iterate_steps(self, n_steps, delta_t, stream=None, halo=None):
        """n_steps steps with a fixed delta_t. With the native stepper this is ONE call: the exchange stream and
        the compute stream then meet only at its entry and exit (see csrc/hip/stepper.hip). `speed` then holds the
        estimates of the call's last step, as after n_steps single steps; those of the steps before are not written."""
        if n_steps <= 0:
            return
        if self.stepper is None:
            for _ in range(n_steps):
                self.iterate(delta_t, stream, halo)
            return
        self.begin_step()
        first_prev, first_next = self.prev, self.next
        for _ in range(n_steps - 1):
            self.begin_step()
        self.stepper.iterate_steps(self, delta_t, n_steps, first_prev, first_next, stream)

    def iterate(self, delta_t, stream=None, halo=None):
        """One SSP-RK3 step (CompressibleEulerSolver::iterate, SubgridCompressibleEulerSolver::iterate). `halo` (a
        halo.HaloExchange) refreshes the ghost slots of each stage's source state while the interior tiles are already running."""
        self.begin_step()
        if self.stepper is not None:
            self.stepper.iterate(self, delta_t, stream)
            return
        for k in range(3):
            self.run_stage(k, delta_t, stream, halo)

    # -- scalar diagnostics, computed on the device ------------------------------------------------
    def _reduce_buffers(self):
        if not hasattr(self, "_ws"):
            n = hip.lib().t8gpu_hip_reduce_workspace_bytes
            n.restype = C.c_size_t
            self._ws = torch.zeros(n() // 8, dtype=torch.float64, device="cuda")
            self._scalar = torch.zeros(1, dtype=torch.float64, device="cuda")
        return self._ws, self._scalar

    def _monitor_buffers(self):
        """workspace, device result and pinned host block of the monitor: made on first use and kept"""
        if not hasattr(self, "_mon"):
            n = hip.lib().t8gpu_hip_state_monitor_workspace_bytes
            n.restype = C.c_size_t
            self._mon = (torch.zeros(n() // 8, dtype=torch.float64, device="cuda"),
                         torch.zeros(Monitor.SLOTS, dtype=torch.float64, device="cuda"),
                         torch.zeros(Monitor.SLOTS, dtype=torch.float64).pin_memory())
        return self._mon

    def monitor_device(self, step=None, stream=None):
        """One pass of t8gpu_hip_state_monitor_* over the owned cells of state(step) (ghost slots and spare capacity are not
        read), enqueued on `stream` (default: the current stream): the solver's 16-double device block (slots: Monitor,
        include/t8gpu_hip.h). No copy, no sync -- for callers that poll or all-reduce on the device. The block is
        overwritten by the next call."""
        ws, res, _ = self._monitor_buffers()
        s = self.next if step is None else step
        dim, cells_per_element, volumes = self.cell_geometry()
        hip.call("t8gpu_hip_state_monitor", self.dtype, C.c_size_t(self.owned_cells), cells_per_element, dim,
                 self.get_own_variables(s), hip.ptr(volumes), hip.ptr(ws), hip.ptr(res), hip.stream_ptr(stream))
        return res

    def monitor(self, step=None, stream=None, dist=None):
        """The Monitor of state(step): one kernel pass, one 128-byte copy to the host, one sync. `dist` combines the ranks'
        blocks (Monitor.combine) with three all_reduce calls, on the GPU for nccl and on the CPU otherwise."""
        stream = torch.cuda.current_stream() if stream is None else stream
        res = self.monitor_device(step, stream)
        host = self._monitor_buffers()[2]
        with torch.cuda.stream(stream):
            host.copy_(res, non_blocking=True)
        stream.synchronize()
        block = host.numpy().copy()
        if dist is not None:
            mine = torch.from_numpy(block).to("cuda" if dist.get_backend() == "nccl" else "cpu")
            for op, slots in ((dist.ReduceOp.SUM, Monitor.SUM_SLOTS), (dist.ReduceOp.MAX, Monitor.MAX_SLOTS),
                              (dist.ReduceOp.MIN, Monitor.MIN_SLOTS)):
                t = mine.clone()
                dist.all_reduce(t, op=op)
                block[list(slots)] = t.cpu().numpy()[list(slots)]
        return Monitor(block)

    # -- boundary budgets (boundary.py): what crosses the boundary, per group of boundary faces ----------------
    def boundary_fluxes_device(self, step=None, groups=None, stream=None, out=None, weight=None):
        """One pass of t8gpu_hip_boundary_fluxes_* over the boundary faces of state(step), enqueued on `stream` with no copy and
        no sync: the float64 device block [num_groups, 16] of this grouping (slots: boundary.BoundaryFluxes, include/t8gpu_hip.h),
        overwritten by the next call. groups: None = by boundary kind (group index = kind code), "side" (boundary.side_groups)
        or a uint8 array [B] with values < 32; anything else raises ValueError. The sorted face list, the offsets and the
        workspace are made on first use per grouping and kept. `out` (a block of the same shape) receives the result instead;
        with `weight` as well the call accumulates: out[:, 0:11] += weight * value, slots 11-12 those of this call -- a loop
        integrates in time on the device. The inflow table is read where set_inflow_states refills it: nothing is rebuilt."""
        from . import boundary
        return boundary.boundary_fluxes_device(self, step, groups, stream, out, weight)

    def boundary_fluxes(self, step=None, groups=None, stream=None, dist=None):
        """The boundary.BoundaryFluxes of state(step): one pass, one pinned copy to the host, one sync. `dist` all-reduces the
        block with SUM (every slot is a sum), on the GPU for nccl and on the CPU otherwise."""
        from . import boundary
        return boundary.boundary_fluxes(self, step, groups, stream, dist)

    def boundary_step_fluxes(self, delta_t, groups=None, stream=None, dist=None):
        """The boundary flux integrated over the LAST step taken with `delta_t` (iterate, or the last step of iterate_steps), as
        a boundary.BoundaryFluxes whose slots 0-10 carry the time integral: three accumulating passes over the step's source
        states prev, STEP1 and STEP2, which the planes still hold, with the weights of the stage formulas
        (boundary.step_weights). In a closed budget integrals(next) - integrals(prev) = -(flux summed over the
        groups) to rounding."""
        from . import boundary
        return boundary.boundary_step_fluxes(self, delta_t, groups, stream, dist)

    def derived_fields(self, names, step=None, stream=None, halo=None):
        """{name: float64 device tensor} of the derived output fields `names` -- "pressure", "velocity", "mach", "entropy",
        "vorticity", "dilatation", "schlieren" (fields.py) -- for the owned cells of state(step) in storage
        order, [cells] or [3, cells]. One pass of t8gpu_hip_*_fields_* enqueued on `stream`, no sync. `halo` refreshes the
        ghost slots of that step first (the gradient fields read them); without it the caller vouches that they are current."""
        from . import fields
        return fields.derived_fields(self, names, step, stream, halo)

    def statistics(self):
        """A stats.Statistics of this solver (stats.py): float64 running sums [15, owned_cells] on the device,
        zeroed, and the calls on them -- accumulate(weight) after a step, results(names) for means, rms values, Reynolds
        stresses and tke, reset(). Needs no geometry: every mesh class. Hand it to the adapt functions of amr.py as
        carry=(stats,) and it follows the run onto the new mesh."""
        from . import stats
        return stats.Statistics(self)

    # -- sampling on Cartesian forests (sample.py): cell values cast to double, never interpolated ----------------
    def locate(self, points, stream=None):
        """int32 device tensor [M]: the storage index among the owned cells of the cell that holds each of points[M, dim] (a host
        or device array, taken to float64) under the half-open rule lo <= x < hi; -1 for a point outside [0, 1)^dim, NaN or
        infinite, or owned by another rank. Enqueued on `stream`, no sync. A mesh that is no SynthMesh raises TypeError."""
        from . import sample
        return sample.sampler(self).locate(points, stream)

    def sample_points(self, points, names, step=None, stream=None, halo=None, fill=float("nan"), extra=None):
        """{name: float64 device tensor [M] or [3, M]} of `names` -- "density", "momentum", "energy" of state(step) and every name
        of derived_fields -- at points[M, dim]: the value of the holding cell, `fill` where locate gives -1. Derived names cost
        one derived_fields pass over the owned cells first, with `halo` handed on. extra = {name: float64 device tensor over
        the owned cells, [cells] or [C, cells]}: names of the caller's own that may be asked for beside the built-in ones (here
        and in sample_grid / resample_uniform), e.g. the results of a stats.Statistics."""
        from . import sample
        return sample.sampler(self).sample_points(points, names, step, stream, halo, fill, extra)

    def sample_grid(self, names, shape, lo=None, hi=None, step=None, stream=None, halo=None, fill=float("nan"), cells=False,
                    extra=None):
        """sample_points on the pixel centres lo + (i + 0.5) (hi - lo) / n of a grid of shape (nx, ny[, nz]) over the box lo..hi
        (default: the whole domain), in one fused launch that forms no point array: tensors [ny, nx], [nz, ny, nx] or [3, ...],
        x fastest. An axis with lo == hi is a slice plane at that coordinate. cells=True adds "cell": the int32 indices."""
        from . import sample
        return sample.sampler(self).sample_grid(names, shape, lo, hi, step, stream, halo, fill, cells, extra)

    def resample_uniform(self, names, level, step=None, stream=None, halo=None, fill=float("nan"), partial=False, extra=None):
        """Conservative resampling onto the 2^level pixels per axis of a uniform level, shapes as sample_grid: per pixel
        sum(w q) / sum(w) over the owned cells that meet it, w = 2^(-dim level of the smaller of pixel and cell), summed in
        ascending storage order in double; `fill` where no owned cell meets the pixel. partial=True: ({name: sums}, weights)
        instead, for ranks to add up and divide once."""
        from . import sample
        return sample.sampler(self).resample_uniform(names, level, step, stream, halo, fill, partial, extra)

    def average_along(self, names, axes, level, step=None, stream=None, halo=None, fill=float("nan"), partial=False, extra=None):
        """resample_uniform at `level` averaged along the mesh axes `axes` (an int or a tuple: a non-empty proper subset of the
        axes), without the image being written: {name: float64 device tensor} over the kept axes, highest first
        -- 3D with axes=(2,) gives [ny, nx], with axes=(0, 2) [ny], 2D with axes=(0,) [ny]; [3, ...] for vectors. Per bin
        sum(w q) / sum(w) over the pixels of the slab, added in the fixed order sample.host_average states, so two calls give
        the same bits; `fill` where this rank owns nothing of the slab. partial=True: ({name: sums}, weights) instead, for
        ranks to add up and divide once."""
        from . import sample
        return sample.sampler(self).average_along(names, axes, level, step, stream, halo, fill, partial, extra)

    # -- tracer particles (tracers.py): coordinates advected by Heun's method around the flow step --------------
    def tracers(self, points, stream=None):
        """A tracers.Tracers of points[M, dim] (a host or device array, taken to float64) on this solver's mesh: predict(dt)
        before the flow step and correct(dt) after it move them with the velocity m / rho of the holding cell; rebind(new
        solver) after an adapt. All device arrays are made here, later calls are enqueued without allocation or sync. A mesh that
        is no SynthMesh raises TypeError, another shape ValueError."""
        from . import tracers
        return tracers.Tracers(self, points, stream)

    def cfl_timestep(self, cfl=0.7, step=None, dist=None):
        """cfl / max over the cells of (|v| + c) / h, h = vol^(1/dim), from the state itself: needs no stage to have run (a new
        solver, a solver fresh from an adapt). On Cartesian cells h is the edge; on curved cells it is cbrt(volume), not an
        inradius. A state with non-finite or non-physical cells raises instead of giving a step size."""
        m = self.monitor(step, dist=dist)
        if m.nonfinite + m.unphysical > 0:
            raise hip.T8gpuHipError(f"cfl_timestep: the state has {m.nonfinite} non-finite and {m.unphysical} non-physical cells "
                                    "(rho <= 0 or p <= 0)")
        return cfl / m.max_rate if m.max_rate > 0 else float("inf")      # (no cells anywhere: no limit)


class PlainSolver(_Solver):
    """Plain elements. mode = "compat": reference data flow (face kernel + atomics, RK kernel);
    mode = "fused": tile kernels (flux + RK in one pass, no flux planes in HBM).
    Boundary faces follow part.boundary_kinds (0 wall, 1 outflow, 2 + k inflow with state k, 10 + k far field against state k;
    absent: walls). A far-field face takes its outside state from the Riemann invariants: the outgoing one from the inside
    cell, the incoming one from state k; it switches by itself between inflow and outflow, subsonic and supersonic
    (DESIGN.md §4). inflow_states = (K, 5) conservative states, required iff some face is an inflow or far-field face."""
    _native_stepper = native.NativeStepper

    def __init__(self, part, dtype=torch.float64, flux_kind=hip.KEPES, mode="compat", capacity=None, state=None,
                 device=None, plan_options=None, inflow_states=None):
        inflow_states = check_inflow_states(part, inflow_states)
        super().__init__(part, dtype, flux_kind, mode)
        tot = part.N + part.G
        self.ndim, self.owned_cells = part.normal_dim, part.N
        self.stride = capacity or tot
        self.planes = torch.zeros((26, self.stride), dtype=dtype, device="cuda")
        if not (isinstance(state, str) and state == "zeros"):     # "zeros": the caller fills the planes on the device (amr.adapt)
            ic = part.kh_initial_state() if state is None else state
            self.planes[0:5, :tot] = _dev(ic, dtype)
        self.planes[25, :tot] = _dev(part.volumes, dtype)
        self.indices = None  # ghosts already resolve to local slots
        self._normals = self._areas = None     # per-face geometry of the compat kernels: uploaded when first asked for
        self.speed = torch.zeros(max(1, part.F + part.B), dtype=dtype, device="cuda")
        # open boundaries: the kinds (compat kernels) and the inflow table, uploaded once here (launches never allocate or copy)
        kinds = boundary_kinds_of(part)
        self.open_boundaries = kinds is not None and bool(np.any(kinds != 0))
        self._upload_open_boundaries(kinds, inflow_states)
        if mode == "fused":
            from . import fused
            import time
            t0 = time.perf_counter()
            self.plan = fused.PlainPlan(part, dtype, **dict(dict(flux_kind=flux_kind), **(plan_options or {})))
            if self.plan.c.has_open_faces:
                self.plan.attach_inflow(self.inflow_table)
            self.plan_build_s = time.perf_counter() - t0          # host tile plan + its upload (amr.adapt reports it)

    @property
    def normals(self):
        """device copy of face_normals (the fused kernels read the tile plan's geometry instead: an adaptive fused run never
        uploads these 24 bytes per face)"""
        if self._normals is None:
            self._normals = _dev(self.part.normals, self.dtype)
        return self._normals

    @property
    def areas(self):
        if self._areas is None:
            self._areas = _dev(self.part.areas, self.dtype)
        return self._areas

    def get_own_volume(self):
        return self.planes[25]

    # -- one flux evaluation + RK stage in the reference's data flow -----------------------------
    def _stage_compat(self, stage, src, dst, dt, stream):
        st, fl = self.get_own_variables(src), self.get_own_variables(FLUXES)
        ev = _timer_begin(self)
        hip.call("t8gpu_hip_flux_faces", self.dtype, self.kind, self.F, self.ndim, hip.ptr(self.fn), None,
                 hip.ptr(self.normals), hip.ptr(self.areas), st, fl, hip.ptr(self.speed), stream)
        _timer_end(self, ev)
        if self.B > 0 and self.open_boundaries:
            hip.call("t8gpu_hip_flux_boundary_bc", self.dtype, self.kind, self.F, self.B, self.ndim, hip.ptr(self.fn),
                     hip.ptr(self.kinds), hip.ptr(self.inflow_table), hip.ptr(self.normals), hip.ptr(self.areas), st, fl,
                     hip.ptr(self.speed), stream)
        elif self.B > 0:
            hip.call("t8gpu_hip_flux_boundary", self.dtype, self.kind, self.F, self.B, self.ndim, hip.ptr(self.fn),
                     hip.ptr(self.normals), hip.ptr(self.areas), st, fl, hip.ptr(self.speed), stream)
        hip.call("t8gpu_hip_rk3_stage", self.dtype, stage, self.N, self.get_own_variables(self.prev), st,
                 self.get_own_variables(dst), fl, hip.ptr(self.planes[25]), hip.fscalar(self.dtype, dt), stream)

    def cell_geometry(self):
        """(dim, cells per element, the elements' volumes on the device): for the monitor and the transfer of amr.py"""
        return int(self.part.mesh.dim), 1, self.planes[25]     # (the curved meshes of unstructured.py: dim = 3)

    def like(self, part):
        """An empty PlainSolver of this one's configuration on `part` (an adapted or repartitioned mesh): dtype, flux kind,
        mode, inflow states, the options a tile plan hands on, `next` / `prev`; all-zero state, no stepper."""
        return self._like(part, plan_options=None if self.plan is None else self.plan.inherited_options())

    # -- scalar diagnostics of the reference solver, computed on the device -----------------------
    def compute_integral(self, variable=0, step=None):
        """sum(volume * variable) over the owned elements (CompressibleEulerSolver::compute_integral)."""
        ws, res = self._reduce_buffers()
        s = self.next if step is None else step
        hip.call("t8gpu_hip_integral", self.dtype, C.c_size_t(self.N), 1, hip.ptr(self.planes[5 * s + variable]),
                 hip.ptr(self.planes[25]), hip.ptr(ws), hip.ptr(res), hip.stream_ptr())
        return float(res.item())

    def max_speed(self):
        """max of the per-face wave-speed estimates of the last stage (input of compute_timestep). Starts from 0; NaN if any
        estimate is NaN, wherever it sits."""
        ws, res = self._reduce_buffers()
        hip.call("t8gpu_hip_max_speed", self.dtype, C.c_size_t(self.F + self.B), hip.ptr(self.speed), hip.ptr(ws),
                 hip.ptr(res), hip.stream_ptr())
        return float(res.item())

    def compute_timestep(self, cfl=0.7, max_level=None, dist=None):
        """cfl * 0.5^max_level / max speed (solver.cu:213-229); `dist` all-reduces the maximum over ranks. Without `dist`, a NaN
        speed estimate (a blown-up state) gives NaN, never a finite step; what the all-reduce makes of one rank's NaN is the
        backend's business and is not pinned."""
        speed = torch.tensor([self.max_speed()], dtype=torch.float64, device="cuda" if dist is None or dist.get_backend() == "nccl" else "cpu")
        if dist is not None:
            dist.all_reduce(speed, op=dist.ReduceOp.MAX)
        level = self.part.mesh.finest_level if max_level is None else max_level
        return cfl * 0.5 ** level / float(speed.item())

    def _units(self):
        return self.plan.host.ntiles


class SubgridSolver(_Solver):
    """Subgrid<4,4> / Subgrid<4,4,4>: planes[25, (N+G)*S] in subcells + per-block volumes.
    open_boundaries=True: boundary faces follow part.boundary_kinds (0 wall, 1 outflow, 2 + k inflow with state k; absent:
    walls), every subcell on an open face with its own sub-face flux; inflow_states = (K, 5) conservative states, required iff
    some face is an inflow or far-field face. A partition without open faces takes it too (a rank that owns no boundary, an
    adapted mesh). By default a partition with open faces is refused.
    farfield=True (needs open_boundaries=True): far-field faces (10 + k, the characteristic condition against state k,
    DESIGN.md §4) are taken too, per sub-face with the outward normal of the block face; without it a partition with far-field
    faces is refused. A partition without far-field faces takes the flag too."""
    _native_stepper = native.NativeSubgridStepper

    def __init__(self, part, dtype=torch.float32, flux_kind=hip.KEPES, mode="compat", state=None, open_boundaries=False,
                 inflow_states=None, farfield=False):
        kinds = boundary_kinds_of(part)
        if farfield and not open_boundaries:
            raise ValueError("farfield=True needs open_boundaries=True")
        if not farfield and kinds is not None and np.any(kinds >= FARFIELD):
            raise ValueError("SubgridSolver without farfield=True takes no far-field boundary faces: the partition has far-field "
                             "kinds (10 + k) (pass open_boundaries=True, farfield=True and inflow_states)")
        if not open_boundaries and kinds is not None and np.any(kinds != 0):
            raise ValueError("SubgridSolver without open_boundaries=True takes walls only: the partition has outflow / inflow "
                             "boundary faces (pass open_boundaries=True and, for inflow faces, inflow_states)")
        if not open_boundaries and inflow_states is not None:
            raise ValueError("inflow_states needs open_boundaries=True")
        inflow_states = check_inflow_states(part, inflow_states) if open_boundaries else None
        assert part.subgrid
        super().__init__(part, dtype, flux_kind, mode)
        self.open_boundaries, self.farfield = bool(open_boundaries), bool(farfield)
        self._far_kinds = self.farfield and kinds is not None and bool(np.any(kinds >= FARFIELD))
        self._upload_open_boundaries(kinds, inflow_states)
        self.rank = part.mesh.dim
        self.S = 4 ** self.rank
        tot = part.N + part.G
        self.owned_cells = part.N * self.S
        self.stride = tot * self.S
        self.planes = torch.zeros((25, self.stride), dtype=dtype, device="cuda")
        if not (isinstance(state, str) and state == "zeros"):     # "zeros": as for PlainSolver
            ic = part.kh_initial_state() if state is None else state
            self.planes[0:5] = _dev(ic, dtype)
        self.volumes = _dev(part.volumes, dtype)
        self.level_diff = _dev(part.level_diff)
        self.nb_offset = _dev(part.nb_offset)
        self.normals = _dev(part.normals, dtype)
        self.areas = _dev(part.areas, dtype)
        if mode == "fused":
            from . import fused
            self.plan = fused.SubgridPlan(part, dtype, farfield=self.farfield)
            if self.plan.c.has_open_faces:
                self.plan.attach_inflow(self.inflow_table)

    def _stage_compat(self, stage, src, dst, dt, stream):
        st, fl = self.get_own_variables(src), self.get_own_variables(FLUXES)
        ev = _timer_begin(self)
        hip.call("t8gpu_hip_subgrid_inner", self.dtype, self.kind, self.rank, self.N, st, fl, hip.ptr(self.volumes),
                 stream)
        _timer_end(self, ev)
        if self.B > 0 and self.kinds is not None:
            # (far-field kinds: the kernel that decodes them; plans without them keep the _bc kernel)
            hip.call("t8gpu_hip_subgrid_boundary_far" if self._far_kinds else "t8gpu_hip_subgrid_boundary_bc", self.dtype, self.kind, self.rank, self.F, self.B, hip.ptr(self.fn),
                     hip.ptr(self.kinds), hip.ptr(self.inflow_table), hip.ptr(self.normals), hip.ptr(self.areas), st, fl, stream)
        elif self.B > 0:
            hip.call("t8gpu_hip_subgrid_boundary", self.dtype, self.kind, self.rank, self.F, self.B,
                     hip.ptr(self.fn), hip.ptr(self.normals), hip.ptr(self.areas), st, fl, stream)
        hip.call("t8gpu_hip_subgrid_outer", self.dtype, self.kind, self.rank, self.F, hip.ptr(self.fn), None,
                 hip.ptr(self.level_diff), hip.ptr(self.nb_offset), hip.ptr(self.normals), hip.ptr(self.areas),
                 st, fl, stream)
        hip.call("t8gpu_hip_subgrid_rk3_stage", self.dtype, stage, self.rank, self.N,
                 self.get_own_variables(self.prev), st, self.get_own_variables(dst), fl, hip.ptr(self.volumes),
                 hip.fscalar(self.dtype, dt), stream)

    def cell_geometry(self):
        """(dim, cells per element, the blocks' volumes on the device): for the monitor and the transfer of amr.py"""
        return self.rank, self.S, self.volumes

    def like(self, part):
        """An empty SubgridSolver of this one's configuration on `part`: as PlainSolver.like, with open_boundaries and
        farfield in place of the plan options."""
        return self._like(part, open_boundaries=self.open_boundaries, farfield=self.farfield)

    def compute_integral(self, variable=0, step=None):
        """sum(volume / S * variable) over the owned subcells (SubgridCompressibleEulerSolver::compute_integral,
        examples/subgrid/solver.inl:281-305, for any variable as on PlainSolver)."""
        ws, res = self._reduce_buffers()
        s = self.next if step is None else step
        hip.call("t8gpu_hip_integral", self.dtype, C.c_size_t(self.owned_cells), self.S, hip.ptr(self.planes[5 * s + variable]),
                 hip.ptr(self.volumes), hip.ptr(ws), hip.ptr(res), hip.stream_ptr())
        return float(res.item())

    def _units(self):
        return self.N
