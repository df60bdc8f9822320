"""Time-averaged flow statistics on the device (csrc/hip/stats.hip, include/t8gpu_hip.h: t8gpu_hip_stats_accumulate_*,
t8gpu_hip_stats_results): weighted running sums of fifteen per-cell quantities of the state, and from them
means, rms values, Reynolds stresses and turbulent kinetic energy. `_Solver.statistics()` is the entry point; the sums ride
through an adapt with `carry=(stats,)` (amr.py), `vtk.get_host_statistics_variable` is the way into a .vtu file.

The usual weight is the step's dt; with `iterate_steps(n, dt)` accumulate once per call with `n * dt`. A call reads the five
state planes and reads and writes fifteen doubles per cell, about 280 B per fp64 cell of memory traffic: of the order of a
whole step at the c4 size (derived from the byte count, measured by nobody), so most loops sample every k steps.
Nothing is filtered: a non-finite cell makes that cell's sums non-finite; the state monitor is the guard. Second moments
are raw sums, so an rms far below about 1e-7 of the mean is rounding, and values are clamped at 0.
"""
import ctypes as C
import math

PLANES = 15                     # T8GPU_STATS_PLANES
RESULT_PLANES = 19              # T8GPU_STATS_RESULT_PLANES
# the accumulator slots of include/t8gpu_hip.h
SLOTS = ("rho", "mx", "my", "mz", "E", "p", "rho2", "p2", "mxmx", "mymy", "mzmz", "mxmy", "mxmz", "mymz", "mach")
# name -> (first output plane, planes): the result table of include/t8gpu_hip.h
RESULTS = {"mean_density": (0, 1), "mean_momentum": (1, 3), "mean_energy": (4, 1), "mean_pressure": (5, 1), "mean_mach": (6, 1),
           "mean_velocity": (7, 3), "density_rms": (10, 1), "pressure_rms": (11, 1), "reynolds_stress": (12, 6), "tke": (18, 1)}
STRESS_COMPONENTS = ("xx", "yy", "zz", "xy", "xz", "yz")


class StatsPlanes(C.Structure):
    """T8gpuStatsPlanes: the nineteen output planes, NULL = not asked for"""
    _fields_ = [("p", C.c_void_p * RESULT_PLANES)]


def check_names(names):
    """`names` (one name or several) as a list without repeats; an unknown name raises ValueError listing the valid ones"""
    names = [names] if isinstance(names, str) else list(names)
    for name in names:
        if name not in RESULTS:
            raise ValueError(f"unknown statistic {name!r}: one of {', '.join(RESULTS)}")
    return list(dict.fromkeys(names))


def check_weight(weight):
    """the weight of one accumulation as a float: finite and > 0, ValueError otherwise"""
    try:
        w = float(weight)
    except (TypeError, ValueError):
        raise ValueError(f"weight must be a finite number > 0, got {weight!r}") from None
    if not (math.isfinite(w) and w > 0.0):
        raise ValueError(f"weight must be finite and > 0, got {weight!r}")
    return w


class Statistics:
    """The running sums of one solver: `sums`, a float64 device tensor [15, owned_cells] in storage order (slots: SLOTS),
    zeroed here, and `weight`, the host float of the weights added so far. Every call is enqueued on `stream` (default: the
    current stream) without a host sync. After `amr.adapt*(..., carry=(stats,))` the object refers to the new solver and
    `sums` holds the transferred values."""

    def __init__(self, solver):
        import torch
        self.solver = solver
        self.sums = torch.zeros((PLANES, solver.owned_cells), dtype=torch.float64, device="cuda")
        self.weight = 0.0

    def accumulate(self, weight, step=None, stream=None):
        """sums[k] += weight q_k of state(step) (default: solver.next) for the owned cells: one launch, no sync, no
        allocation. Raises ValueError unless weight is finite and > 0."""
        from . import hip
        w = check_weight(weight)
        solver = self.solver
        if tuple(self.sums.shape) != (PLANES, solver.owned_cells):
            raise ValueError(f"sums has shape {tuple(self.sums.shape)}, the solver owns {solver.owned_cells} cells")
        s = solver.next if step is None else step
        hip.call("t8gpu_hip_stats_accumulate", solver.dtype, C.c_size_t(solver.owned_cells), solver.get_own_variables(s),
                 C.c_double(w), hip.ptr(self.sums), C.c_size_t(self.sums.stride(0)), hip.stream_ptr(stream))
        self.weight += w

    def results(self, names, stream=None, out=None):
        """{name: float64 device tensor} of the statistics `names` (RESULTS) for the owned cells in storage order: [cells],
        [3, cells] for mean_momentum and mean_velocity, [6, cells] (xx yy zz xy xz yz) for reynolds_stress. One launch; only
        the planes asked for are written. `out` ({name: tensor of that shape}) receives them instead of new tensors. An
        unknown name raises ValueError (listing the valid ones), and so does a call before any accumulate."""
        names = check_names(names)
        if not self.weight > 0.0:
            raise ValueError("results() needs weight > 0: nothing has been accumulated")
        return self._results(self.sums, (self.solver.owned_cells,), names, self.weight, stream, out)

    @staticmethod
    def _results(sums, shape, names, weight, stream=None, out=None):
        """the result kernel over sums [15, cells] (rows contiguous), each result in the shape `shape` of one plane"""
        import torch
        from . import hip
        stream = torch.cuda.current_stream() if stream is None else stream
        cells = sums.shape[1]
        res, planes = {}, StatsPlanes()
        with torch.cuda.stream(stream):
            for name in names:
                first, count = RESULTS[name]
                if out is not None and name in out:
                    t = out[name].view(count, cells)
                    if t.dtype != torch.float64 or not t.is_cuda or t.stride(1) != 1:
                        raise ValueError(f"out[{name!r}] must be a float64 device tensor with contiguous rows")
                else:
                    t = torch.empty((count, cells), dtype=torch.float64, device="cuda")
                for k in range(count):
                    planes.p[first + k] = t[k].data_ptr()
                res[name] = t[0].view(shape) if count == 1 else t.view((count,) + tuple(shape))
        lib = hip.lib()
        lib.t8gpu_hip_stats_results.restype = C.c_int
        hip.check(lib.t8gpu_hip_stats_results(C.c_size_t(cells), hip.ptr(sums), C.c_size_t(sums.stride(0)),
                                              C.c_double(weight), planes, hip.stream_ptr(stream)))
        return res

    def results_of(self, sums15, names, weight=None, stream=None):
        """`results` formed from any float64 device tensor sums15 [15, ...] of sums in the slots SLOTS, e.g. the space-averaged
        sums of average_along(partial=True) after the ranks' all-reduce and the division by the added weights: {name: tensor
        over the trailing shape}, [3, ...] / [6, ...] as in results. weight (default: this object's) is the time weight the
        sums carry; it must be > 0 (ValueError)."""
        import torch
        names = check_names(names)
        w = self.weight if weight is None else check_weight(weight)
        if not w > 0.0:
            raise ValueError("results_of() needs weight > 0: nothing has been accumulated")
        ok = isinstance(sums15, torch.Tensor) and sums15.is_cuda and sums15.dtype == torch.float64 and sums15.dim() >= 1 and \
            sums15.shape[0] == PLANES
        if not ok:
            raise ValueError(f"sums15 must be a float64 device tensor [{PLANES}, ...]")
        shape = tuple(sums15.shape[1:])
        flat = sums15.reshape(PLANES, -1)
        if flat.shape[1] and flat.stride(1) != 1:
            flat = flat.contiguous()
        return self._results(flat, shape, names, w, stream)

    def average_along(self, names, axes, level, stream=None, fill=math.nan, partial=False):
        """The statistics `names` of the slabs of solver.average_along(axes, level): the fifteen running sums go
        through one averaging call as an extra [15, cells] field, are divided by the bin weights, and the result formulas
        run over the bins -- so the Favre mean, the rms values, the Reynolds stress and tke of a bin are formed from the
        space-and-time averaged SUMS, not averaged per cell (the formulas are nonlinear; a mean of per-cell stresses would miss
        the part of the fluctuation that is the cells' means differing along the axis). Bins this rank owns nothing of get
        `fill`. partial=True: (sums [15, bins...], weights [bins...]) instead; ranks add both up, divide, and call
        results_of. Raises ValueError before any accumulate, as results does."""
        import torch
        names = check_names(names)
        if not self.weight > 0.0:
            raise ValueError("average_along() needs weight > 0: nothing has been accumulated")
        stream = torch.cuda.current_stream() if stream is None else stream
        got, weights = self.solver.average_along("stats_sums", axes, level, stream=stream, partial=True,
                                                 extra={"stats_sums": self.sums})
        if partial:
            return got["stats_sums"], weights
        with torch.cuda.stream(stream):
            res = self.results_of(got["stats_sums"] / weights, names, stream=stream)
            empty = weights == 0.0
            for t in res.values():
                t.masked_fill_(empty, fill)
        return res

    def reset(self, stream=None):
        """zero the sums (on the stream) and the weight"""
        import torch
        with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
            self.sums.zero_()
        self.weight = 0.0

    # -- consumers: the statistics as extra planes of the solver's sampler (sample.py) -----------------------------------
    def sample_grid(self, names, shape, **kw):
        """solver.sample_grid of the statistics `names` (arguments as there): one results pass, one sampling launch"""
        names = check_names(names)
        return self.solver.sample_grid(names, shape, extra=self.results(names, kw.get("stream")), **kw)

    def sample_points(self, points, names, **kw):
        """solver.sample_points of the statistics `names` at points[M, dim]"""
        names = check_names(names)
        return self.solver.sample_points(points, names, extra=self.results(names, kw.get("stream")), **kw)


def plane_names(name):
    """the scalar names one result is written under where only scalars and 3-vectors exist (VTK): the six stress components
    as reynolds_stress_xx .. _yz"""
    count = RESULTS[name][1]
    return [f"{name}_{c}" for c in STRESS_COMPONENTS] if count == 6 else [name]
