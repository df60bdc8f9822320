"""Sampling of cell data on Cartesian forests (csrc/hip/sample.hip, include/t8gpu_hip.h: t8gpu_hip_sample_*):
probe points, image grids and slices, conservative resampling onto a uniform level. Piecewise-constant finite-volume values
cast to double, no interpolation, no atomics; results are bitwise defined.

The geometry is one array of Morton keys. With D = DEPTH = 20 the integer coordinate of x in [0, 1) is floor(x 2^D), the key
of a point the bit-interleave of its integer coordinates (x in the lowest bit), the key of an element that of its lower
corner. In storage order the keys of a SynthMesh partition ascend strictly and are contiguous, key[i + 1] = key[i] +
2^(dim (D - level[i])), so the cell of a point is upper_bound(keys, key(point)) - 1 plus one containment check, and the
leaves inside a dyadic pixel are one contiguous index range. `morton_keys`, `host_locate` and `host_average` (the definition
of the averages along homogeneous axes) are numpy and need no GPU; `Sampler` is what `_Solver.locate /
sample_points / sample_grid / resample_uniform / average_along` forward to.
"""
import ctypes as C
import math

import numpy as np

from . import fields
from .synth import SynthMesh

DEPTH = 20                      # T8GPU_SAMPLE_DEPTH
MAX_PLANES = 16                 # T8GPU_SAMPLE_PLANES: planes of one launch
AVERAGE_CHUNK = 4096            # T8GPU_SAMPLE_AVERAGE_CHUNK: reduced pixels one wavefront adds up (host_average)
# name -> (first plane of a step's five, planes): the conserved names; the derived ones are fields.FIELDS
STATE = {"density": (0, 1), "momentum": (1, 3), "energy": (4, 1)}
NAMES = tuple(STATE) + tuple(fields.FIELDS)


class SamplePlanes(C.Structure):
    """T8gpuSamplePlanes_f32 / _f64: plane k is read from q[k] (the state's float type) or, q[k] NULL, from d[k] (doubles)"""
    _fields_ = [("q", C.c_void_p * MAX_PLANES), ("d", C.c_void_p * MAX_PLANES)]


class SampleGrid(C.Structure):
    """T8gpuSampleGrid"""
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3), ("n", C.c_int32 * 3), ("pad", C.c_int32)]


def check_names(names, extra=None):
    """`names` (one name or several) as a list without repeats; an unknown name raises ValueError listing the valid ones.
    extra: the caller's own planes (check_extra), whose names are valid too"""
    names = [names] if isinstance(names, str) else list(names)
    valid = NAMES + tuple(extra or ())
    for name in names:
        if name not in valid:
            raise ValueError(f"unknown field {name!r}: one of {', '.join(valid)}")
    return list(dict.fromkeys(names))


def check_extra(extra, cells):
    """{name: tensor [planes, cells]} of extra = {name: float64 device tensor over the owned cells, [cells] or [C, cells]}
    (None: {}). A name of the built-in ones, another dtype, device or length raises ValueError."""
    import torch
    out = {}
    for name, t in (extra or {}).items():
        if name in NAMES:
            raise ValueError(f"extra field {name!r} has the name of a built-in one")
        ok = isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() in (1, 2) and t.shape[-1] == cells
        if not ok:
            raise ValueError(f"extra field {name!r} must be a float64 device tensor [{cells}] or [C, {cells}]")
        t = t.reshape(-1, cells)
        out[name] = t if t.stride(1) == 1 or cells == 0 else t.contiguous()
    return out


def plane_count(name, extra=None):
    if extra and name in extra:
        return int(extra[name].shape[0])
    return (STATE.get(name) or fields.FIELDS[name])[1]


def _spread(v, dim):
    """bit b of v (uint64, below 2^21) to bit dim * b: the constant-step "magic bits" """
    x = v.astype(np.uint64)                  # (a copy: the steps below work in place, with one scratch array)
    tmp = np.empty_like(x)
    if dim == 2:
        steps = ((16, 0x0000FFFF0000FFFF), (8, 0x00FF00FF00FF00FF), (4, 0x0F0F0F0F0F0F0F0F), (2, 0x3333333333333333),
                 (1, 0x5555555555555555))
    else:
        steps = ((32, 0x001F00000000FFFF), (16, 0x001F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3),
                 (2, 0x1249249249249249))
    for shift, mask in steps:                # x = (x | (x << shift)) & mask
        np.left_shift(x, np.uint64(shift), out=tmp)
        np.bitwise_or(x, tmp, out=x)
        np.bitwise_and(x, np.uint64(mask), out=x)
    return x


def interleave(coords, dim):
    """keys of integer coordinates [M, >= dim] (each below 2^DEPTH): x in the lowest bit"""
    key = _spread(coords[:, 0], dim)
    for a in range(1, dim):
        s = _spread(coords[:, a], dim)
        np.left_shift(s, np.uint64(a), out=s)
        key |= s
    return key


def check_partition(part, subgrid=None):
    """(dim, cells per block axis) of a partition the sampler takes: a SynthMesh partition (TypeError otherwise: the curved
    meshes of unstructured.py have no keys) with its owned levels within DEPTH (Subgrid: level + 2; ValueError otherwise)
    and fewer than 2^31 owned cells (ValueError)."""
    if not isinstance(getattr(part, "mesh", None), SynthMesh):
        raise TypeError(f"sampling needs a Cartesian SynthMesh partition, not one of {type(getattr(part, 'mesh', None)).__name__}")
    sub = 4 if (part.subgrid if subgrid is None else subgrid) else 1
    dim = part.mesh.dim
    top = int(part.levels[:part.N].max()) + (2 if sub == 4 else 0) if part.N else 0
    if top > DEPTH:
        raise ValueError(f"cell level {top} is above the sampling depth {DEPTH}")
    if part.N * sub ** dim >= 2 ** 31:
        raise ValueError(f"{part.N * sub ** dim} owned cells: the cell index is an int32")
    return dim, sub


def morton_keys(part):
    """uint64[N]: the key of every owned element's anchor, floor((centre - 2^-(level + 1)) 2^DEPTH) per axis, interleaved"""
    dim, _ = check_partition(part, subgrid=False)
    half = np.ldexp(0.5, DEPTH - part.levels[:part.N])              # 2^-(level + 1) 2^DEPTH; products and differences are exact
    anchor = np.floor(part.centres[:part.N, :dim] * 2.0 ** DEPTH - half[:, None])
    return interleave(anchor.astype(np.uint64), dim)


def host_locate(part, points, subgrid=None, keys=None):
    """int32[M]: the storage index among the owned cells of the cell that holds each of points[M, dim], by the half-open rule
    lo <= x < hi; -1 for a point outside [0, 1)^dim, NaN or infinite, or in no owned element. subgrid (default: the
    partition's): cells are the 4^dim subcells of a block, index e S + i + 4 j (+ 16 k). The definition the device
    kernels follow, in numpy."""
    dim, sub = check_partition(part, subgrid)
    pts = np.asarray(points, np.float64).reshape(-1, dim)
    out = np.full(pts.shape[0], -1, np.int32)
    if part.N == 0 or pts.shape[0] == 0:
        return out
    keys = morton_keys(part) if keys is None else keys
    ok = np.all((pts >= 0.0) & (pts < 1.0), axis=1)                 # (before any conversion: NaN compares false)
    idx = np.floor(pts[ok] * 2.0 ** DEPTH).astype(np.uint64)
    key = interleave(idx, dim)
    e = np.searchsorted(keys, key, side="right").astype(np.int64) - 1
    lev = part.levels[:part.N].astype(np.int64)
    ec = np.maximum(e, 0)
    held = (e >= 0) & (key - keys[ec] < (np.uint64(1) << (dim * (DEPTH - lev[ec])).astype(np.uint64)))
    cell = ec.copy()
    if sub == 4:
        sh = (DEPTH - lev[ec] - 2).astype(np.uint64)
        cell = ec * 4 ** dim
        for a in range(dim):
            cell += (((idx[:, a] >> sh) & np.uint64(3)).astype(np.int64)) << (2 * a)
    out[ok] = np.where(held, cell, -1).astype(np.int32)
    return out


def check_axes(axes, dim):
    """`axes` (one mesh axis or several) as an ascending tuple: non-empty, without repeats, each in 0..dim-1 and not all of
    them (the mean over every axis is monitor()'s); ValueError otherwise"""
    try:
        given = [axes] if isinstance(axes, (int, np.integer)) else list(axes)
        ax = [int(a) for a in given]
        if any(a != g for a, g in zip(ax, given)):
            raise TypeError
    except TypeError:
        raise ValueError(f"axes must be a mesh axis or a tuple of them, got {axes!r}") from None
    if not ax or len(set(ax)) != len(ax) or any(not 0 <= a < dim for a in ax) or len(ax) >= dim:
        raise ValueError(f"axes must be a non-empty proper subset of 0..{dim - 1} without repeats, got {axes!r}")
    return tuple(sorted(ax))


def host_average(sums, weights, axes, level, fill=math.nan, partial=False):
    """The definition of average_along in numpy: sums[planes, n, ...] and weights[n, ...] per pixel of the
    n = 2^level grid, as resample_uniform(partial=True) gives them (mesh axis a is array axis dim - 1 - a), added along the
    mesh axes `axes` (check_axes). The result runs over the kept axes in image order, highest kept axis first: sums / weights
    [planes, bins...], `fill` where the weight is 0, or with partial=True (sums, weights) over the bins.
    The order of the additions is what the device follows bit for bit. With A the averaged axes ascending, a reduced pixel has
    index r = sum p_A[i] n^i < R = n^|A|. Chunk c holds the AVERAGE_CHUNK = 4096 indices from 4096 c on: lane j (0..63) adds to
    +0, for t = 0..63 ascending, the pixel r = 4096 c + 64 t + j (r >= R: +0); the lanes are combined by the xor butterfly
    v[j] = v[j] + v[j ^ s] for s = 32, 16, 8, 4, 2, 1; the chunk values of a bin are added to +0 in ascending chunk order."""
    weights = np.asarray(weights, np.float64)
    dim, n = weights.ndim, 1 << int(level)
    sums = np.asarray(sums, np.float64)
    if weights.shape != (n,) * dim or sums.ndim != dim + 1 or sums.shape[1:] != weights.shape:
        raise ValueError(f"sums [planes, ...] and weights must be level-{level} images, got {sums.shape} and {weights.shape}")
    avg = check_axes(axes, dim)
    kept = [a for a in range(dim) if a not in avg]
    # array axes: the kept ones highest mesh axis first, then the averaged ones highest first, so that r runs lowest axis fastest
    order = [dim - 1 - a for a in reversed(kept)] + [dim - 1 - a for a in reversed(avg)]
    bins, R = (n,) * len(kept), n ** len(avg)
    chunks = -(-R // AVERAGE_CHUNK)
    x = np.concatenate([sums, weights[None]]).transpose([0] + [1 + o for o in order]).reshape(sums.shape[0] + 1, -1, R)
    pad = np.zeros(x.shape[:2] + (chunks * AVERAGE_CHUNK,))
    pad[..., :R] = x
    pad = pad.reshape(x.shape[:2] + (chunks, 64, 64))               # [..., chunk, t, lane]
    lanes = np.zeros(x.shape[:2] + (chunks, 64))
    for t in range(64):
        lanes = lanes + pad[..., t, :]
    j = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., j ^ s]
    total = np.zeros(x.shape[:2])
    for c in range(chunks):
        total = total + lanes[..., c, 0]
    total = total.reshape((-1,) + bins)
    s, w = total[:-1], total[-1]
    if partial:
        return s, w
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w > 0.0, s / w, fill)


class Sampler:
    """Keys and levels of a solver's owned elements on the device, built and uploaded once, and the sampling calls on them.
    Made on first use by `sampler(solver)` and kept on the solver (a solver's mesh never changes; an adapt makes a new
    solver). Every call is enqueued on `stream` (default: the current stream) without a host sync; a rank of a partitioned
    run samples its owned cells only and returns cell -1 / `fill` / weight 0 for the rest. extra = {name: float64 device
    tensor over the owned cells, [cells] or [C, cells]} adds names of the caller's own (check_extra), read as double planes."""

    def __init__(self, solver):
        import torch
        from . import hip
        self.solver, part = solver, solver.part
        self.dim, self.sub = check_partition(part, hasattr(solver, "S"))
        self.N = part.N
        keys = morton_keys(part)
        if keys.size == 0:
            keys = np.zeros(1, np.uint64)                           # (owns nothing: a valid pointer all the same)
        levels = np.ascontiguousarray(part.levels[:max(1, part.N)], np.int32)
        self.keys = torch.from_numpy(keys.view(np.int64)).cuda()
        self.levels = torch.from_numpy(levels).cuda()
        self._hip = hip

    # -- arguments -------------------------------------------------------------------------------------------------
    def _forest(self):
        return self._hip.ptr(self.keys), self._hip.ptr(self.levels), self.N, self.sub

    def _points(self, points):
        import torch
        if isinstance(points, torch.Tensor):
            p = points.to(device="cuda", dtype=torch.float64)
        else:
            p = torch.from_numpy(np.ascontiguousarray(points, np.float64)).cuda()
        if p.ndim != 2 or p.shape[1] != self.dim:
            raise ValueError(f"points must have shape [M, {self.dim}], got {tuple(p.shape)}")
        return p.contiguous()

    def _sources(self, names, step, stream, halo, extra=None):
        """(names, SamplePlanes, number of planes, what to keep alive): state planes by pointer, derived names through one
        derived_fields pass over the owned cells, the names of `extra` (check_extra) from the caller's double planes"""
        names = check_names(names, extra)
        total = sum(plane_count(n, extra) for n in names)
        if total > MAX_PLANES:
            raise ValueError(f"{total} planes asked for, one call takes {MAX_PLANES}")
        s = self.solver.next if step is None else step
        derived = [n for n in names if n in fields.FIELDS]
        got = self.solver.derived_fields(derived, s, stream, halo) if derived else {}
        src, k = SamplePlanes(), 0
        for name in names:
            if extra and name in extra:
                count = plane_count(name, extra)
                for j in range(count):
                    src.d[k + j] = extra[name][j].data_ptr()
            elif name in STATE:
                first, count = STATE[name]
                for j in range(count):
                    src.q[k + j] = self.solver.planes[5 * s + first + j].data_ptr()
            else:
                count = fields.FIELDS[name][1]
                planes = got[name].reshape(count, -1)
                for j in range(count):
                    src.d[k + j] = planes[j].data_ptr()
            k += count
        return names, src, total, (got, extra)

    @staticmethod
    def _split(names, out, shape, extra=None):
        """{name: view of out[planes, ...]} in the shape of one plane, [3, ...] for a vector ([C, ...] for C extra planes)"""
        res, k = {}, 0
        for name in names:
            count = plane_count(name, extra)
            res[name] = out[k].view(shape) if count == 1 else out[k:k + count].view((count,) + tuple(shape))
            k += count
        return res

    def _stream(self, stream):
        import torch
        return torch.cuda.current_stream() if stream is None else stream

    # -- the calls ---------------------------------------------------------------------------------------------------
    def _locate(self, p, stream):
        import torch
        cells = torch.empty(p.shape[0], dtype=torch.int32, device="cuda")
        if p.shape[0]:
            lib = self._hip.lib()
            lib.t8gpu_hip_sample_locate.restype = C.c_int
            self._hip.check(lib.t8gpu_hip_sample_locate(self.dim, C.c_size_t(p.shape[0]), self._hip.ptr(p), *self._forest(),
                                                        self._hip.ptr(cells), self._hip.stream_ptr(stream)))
        return cells

    def locate(self, points, stream=None):
        import torch
        stream = self._stream(stream)
        with torch.cuda.stream(stream):
            return self._locate(self._points(points), stream)

    def sample_points(self, points, names, step=None, stream=None, halo=None, fill=math.nan, extra=None):
        import torch
        stream = self._stream(stream)
        extra = check_extra(extra, self.solver.owned_cells)
        with torch.cuda.stream(stream):
            p = self._points(points)
            m = p.shape[0]
            names = check_names(names, extra)
            if m == 0:
                planes = sum(plane_count(n, extra) for n in names)
                return self._split(names, torch.empty((planes, 0), dtype=torch.float64, device="cuda"), (0,), extra)
            names, src, total, keep = self._sources(names, step, stream, halo, extra)
            cells = self._locate(p, stream)
            out = torch.empty((total, m), dtype=torch.float64, device="cuda")
            self._hip.call("t8gpu_hip_sample_gather", self.solver.dtype, C.c_size_t(m), self._hip.ptr(cells), total, src,
                           C.c_double(fill), self._hip.ptr(out), self._hip.stream_ptr(stream))
            del keep
        return self._split(names, out, (m,), extra)

    def sample_grid(self, names, shape, lo=None, hi=None, step=None, stream=None, halo=None, fill=math.nan, cells=False,
                    extra=None):
        import torch
        dim = self.dim
        shape = tuple(int(n) for n in shape)
        lo = (0.0,) * dim if lo is None else tuple(float(x) for x in lo)
        hi = (1.0,) * dim if hi is None else tuple(float(x) for x in hi)
        if not (len(shape) == len(lo) == len(hi) == dim):
            raise ValueError(f"shape, lo and hi need {dim} entries each")
        if any(n < 0 for n in shape):
            raise ValueError(f"negative grid extent in {shape}")
        extra = check_extra(extra, self.solver.owned_cells)
        names = check_names(names, extra)
        image, pixels = shape[::-1], math.prod(shape)
        stream = self._stream(stream)
        with torch.cuda.stream(stream):
            cell = torch.empty(image, dtype=torch.int32, device="cuda") if cells else None
            if pixels == 0:
                planes = sum(plane_count(n, extra) for n in names)
                res = self._split(names, torch.empty((planes, 0), dtype=torch.float64, device="cuda"), image, extra)
            else:
                names, src, total, keep = self._sources(names, step, stream, halo, extra)
                g = SampleGrid()
                for a in range(dim):
                    g.lo[a], g.hi[a], g.n[a] = lo[a], hi[a], shape[a]
                out = torch.empty((total, pixels), dtype=torch.float64, device="cuda")
                self._hip.call("t8gpu_hip_sample_grid", self.solver.dtype, dim, g, *self._forest(), total, src, C.c_double(fill),
                               self._hip.ptr(out), self._hip.ptr(cell), self._hip.stream_ptr(stream))
                del keep
                res = self._split(names, out, image, extra)
        if cells:
            res["cell"] = cell
        return res

    def resample_uniform(self, names, level, step=None, stream=None, halo=None, fill=math.nan, partial=False, extra=None):
        import torch
        level = int(level)
        if not 0 <= level <= DEPTH:
            raise ValueError(f"level must lie in 0..{DEPTH}, got {level}")
        image = (1 << level,) * self.dim
        stream = self._stream(stream)
        extra = check_extra(extra, self.solver.owned_cells)
        with torch.cuda.stream(stream):
            names, src, total, keep = self._sources(names, step, stream, halo, extra)
            if total == 0:
                raise ValueError("resample_uniform needs at least one name")
            out = torch.empty((total, 1 << (self.dim * level)), dtype=torch.float64, device="cuda")
            weights = torch.empty(image, dtype=torch.float64, device="cuda") if partial else None
            self._hip.call("t8gpu_hip_sample_uniform", self.solver.dtype, self.dim, level, *self._forest(), total, src,
                           C.c_double(fill), self._hip.ptr(out), self._hip.ptr(weights), self._hip.stream_ptr(stream))
            del keep
        res = self._split(names, out, image, extra)
        return (res, weights) if partial else res

    def average_along(self, names, axes, level, step=None, stream=None, halo=None, fill=math.nan, partial=False, extra=None):
        import torch
        level = int(level)
        if not 0 <= level <= DEPTH:
            raise ValueError(f"level must lie in 0..{DEPTH}, got {level}")
        avg = check_axes(axes, self.dim)
        if self.dim * level > 36:
            raise ValueError(f"level {level} has 2^{self.dim * level} pixels: one call takes 2^36")
        kept = self.dim - len(avg)
        bins, count = (1 << level,) * kept, 1 << (level * kept)
        chunks = -(-(1 << (level * len(avg))) // AVERAGE_CHUNK)
        stream = self._stream(stream)
        extra = check_extra(extra, self.solver.owned_cells)
        with torch.cuda.stream(stream):
            names, src, total, keep = self._sources(names, step, stream, halo, extra)
            if total == 0:
                raise ValueError("average_along needs at least one name")
            out = torch.empty((total, count), dtype=torch.float64, device="cuda")
            weights = torch.empty(bins, dtype=torch.float64, device="cuda") if partial else None
            scratch = torch.empty((count, chunks, total + 1), dtype=torch.float64, device="cuda") if chunks > 1 else None
            self._hip.call("t8gpu_hip_sample_average", self.solver.dtype, self.dim, level, sum(1 << a for a in avg), *self._forest(),
                           total, src, C.c_double(fill), self._hip.ptr(out), self._hip.ptr(weights), self._hip.ptr(scratch),
                           self._hip.stream_ptr(stream))
            del keep, scratch                       # (freed on this stream: the next allocation there follows the kernels)
        res = self._split(names, out, bins, extra)
        return (res, weights) if partial else res


def sampler(solver):
    """the solver's Sampler: built on the first sampling call, then kept (as fields._csr keeps the CSR)"""
    if getattr(solver, "_sampler", None) is None:
        solver._sampler = Sampler(solver)
    return solver._sampler
