"""Passive tracer particles on Cartesian forests, advected by Heun's method (csrc/hip/tracers.hip, include/t8gpu_hip.h:
t8gpu_hip_tracers_*). `Tracers` is what `_Solver.tracers(points)` returns; one step of a run reads

    tr.predict(dt)          # before the flow step: k1 = u^n(x), xs = map(x + dt k1)
    solver.iterate(dt)      # any driver: the tracer calls read states, they do not touch the step
    tr.correct(dt)          # after it: k2 = u^(n+1)(xs), x = map(x + (dt / 2) (k1 + k2))

A particle is a coordinate, not a member of a cell: the velocity at a point is m / rho of the cell that holds it (sample.py's
half-open locate), in double, never interpolated. An adapt does not touch particle data (`rebind` hands the object the new
solver), and no particle migrates between ranks: every rank holds all particles, and between velocity and move the velocities
are summed over the ranks -- the one rank that holds a point contributes, the others add zeros -- so a k-way run gives the bits
of the single-rank run. That costs one collective of M (dim + 1) words per phase and is meant for up to a few million particles.

`host_velocity`, `host_map`, `host_predict` and `host_correct` are numpy, need no GPU and are the definition of the arithmetic:
the kernels give their bits. status: 0 active, 1 left through an open side (x = the raw point outside), 2 lost (non-finite, still
outside after one mirror, or held by no cell; x = the last position inside). A left or lost particle is frozen.

Not covered: curved meshes, interpolated velocity, inertial particles, particle VTK output, per-rank particle ownership.
"""
import ctypes as C
import math

import numpy as np

from . import sample

ACTIVE, LEFT, LOST = 0, 1, 2                    # T8GPU_TRACER_ACTIVE / _LEFT / _LOST
PERIODIC, WALL, OPEN = 0, 1, 2                  # T8GPU_TRACER_PERIODIC / _WALL / _OPEN
PREDICT, CORRECT = 0, 1                         # T8GPU_TRACER_PREDICT / _CORRECT
OK = 0                                          # host_map's outcome beside LEFT and LOST
BELOW_ONE = np.nextafter(1.0, 0.0)


class TracerSides(C.Structure):
    """T8gpuTracerSides"""
    _fields_ = [("kind", C.c_int32 * 6)]


def side_kinds(codes):
    """int32[2 dim] of tracer kinds from a mesh's provider codes (SynthMesh.sides: -1 periodic, 0 wall, anything else --
    outflow, inflow, far field, any index -- open)"""
    codes = np.asarray(codes, np.int64)
    return np.where(codes == -1, PERIODIC, np.where(codes == 0, WALL, OPEN)).astype(np.int32)


# ---- seeds ----------------------------------------------------------------------------------------------------------------
def lattice(dim, n, lo=None, hi=None):
    """float64 [n^dim, dim]: the cell-centred lattice lo + (i + 0.5) (hi - lo) / n per axis over the box lo..hi (default: the
    domain), x fastest. n: one count or one per axis."""
    n = (int(n),) * dim if np.isscalar(n) else tuple(int(v) for v in n)
    lo = (0.0,) * dim if lo is None else tuple(float(v) for v in lo)
    hi = (1.0,) * dim if hi is None else tuple(float(v) for v in hi)
    if not (len(n) == len(lo) == len(hi) == dim) or any(v < 0 for v in n):
        raise ValueError(f"n, lo and hi need {dim} entries each, n >= 0")
    axes = [lo[a] + (np.arange(n[a]) + 0.5) * (hi[a] - lo[a]) / n[a] for a in range(dim)]
    grids = np.meshgrid(*axes[::-1], indexing="ij")                 # slowest axis first
    return np.stack([g.reshape(-1) for g in grids[::-1]], axis=1)


def cell_centres(solver):
    """float64 [owned cells, dim]: the centre of every owned cell in storage order (Subgrid: of every subcell)"""
    part = solver.part
    dim, sub = sample.check_partition(part, hasattr(solver, "S"))
    centres = part.centres[:part.N, :dim]
    if sub == 1:
        return np.array(centres, np.float64)
    edge = 0.5 ** part.levels[:part.N].astype(np.float64)
    c = np.arange(4 ** dim)
    off = np.stack([(c >> (2 * a)) & 3 for a in range(dim)], axis=1).astype(np.float64)              # [S, dim]
    pts = centres[:, None, :] + (off[None, :, :] - 1.5) * (edge[:, None, None] / 4)
    return pts.reshape(-1, dim)


# ---- the definition, in numpy ------------------------------------------------------------------------------------------------
def host_velocity(part, state, points, subgrid=None, keys=None):
    """(k float64 [M, dim], held int32 [M]): with c = sample.host_locate(part, points) and state[5, >= cells] in the solver's
    float type, k[:, a] = double(state[1 + a, c]) / double(state[0, c]) and held = 1 where c >= 0, k = +0 and held = 0
    elsewhere"""
    dim, _ = sample.check_partition(part, subgrid)
    pts = np.asarray(points, np.float64).reshape(-1, dim)
    c = sample.host_locate(part, pts, subgrid, keys)
    held = c >= 0
    k = np.zeros((pts.shape[0], dim))
    cc = c[held]
    with np.errstate(all="ignore"):
        rho = np.asarray(state[0])[cc].astype(np.float64)
        for a in range(dim):
            k[held, a] = np.asarray(state[1 + a])[cc].astype(np.float64) / rho
    return k, held.astype(np.int32)


def host_map(p, kinds):
    """(y [M, dim], outcome [M]) of raw points p and kinds = side_kinds(mesh.sides). Per axis: periodic y = p - floor(p), 0 when
    that is >= 1; wall p < 0 -> -p, p >= 1 -> 2 - p, exactly 1 -> the largest double below 1; an open side crossed on any axis:
    outcome LEFT, y = p on every axis. LOST: p non-finite on any axis (this first) or, not having left, some y outside
    [0, 1). OK otherwise."""
    p = np.asarray(p, np.float64)
    dim = p.shape[1]
    y = p.copy()
    left = np.zeros(p.shape[0], bool)
    with np.errstate(all="ignore"):
        for a in range(dim):
            lo, hi, pa = int(kinds[2 * a]), int(kinds[2 * a + 1]), p[:, a]
            if lo == PERIODIC:
                q = pa - np.floor(pa)
                q[q >= 1.0] = 0.0
            else:
                q = pa.copy()
                below, above = pa < 0.0, pa >= 1.0
                if lo == WALL:
                    q[below] = -pa[below]
                else:
                    left |= below
                if hi == WALL:
                    q[above] = 2.0 - pa[above]
                else:
                    left |= above
            q[q == 1.0] = BELOW_ONE
            y[:, a] = q
        finite = np.all(np.isfinite(p), axis=1)
        outside = ~np.all((y >= 0.0) & (y < 1.0), axis=1)
    outcome = np.where(~finite, LOST, np.where(left, LEFT, np.where(outside, LOST, OK))).astype(np.uint8)
    y[outcome == LEFT] = p[outcome == LEFT]
    return y, outcome


def host_predict(x, status, xs, k1, flag, k, held, dt, kinds):
    """(xs, k1, flag, status) after PREDICT with the velocities k, held at x (summed over the ranks): for the active particles
    k1 = k; held = 0: LOST, xs = x; else xs = map(x + dt k1) with flag = 0, or left: xs = the raw point and flag = 1, or lost:
    status LOST, xs = x, flag = 0. The others keep every entry."""
    x = np.asarray(x, np.float64)
    xs, k1, flag, status = np.array(xs, np.float64), np.array(k1, np.float64), np.array(flag, np.uint8), np.array(status, np.uint8)
    act = status == ACTIVE
    with np.errstate(all="ignore"):
        raw = x + dt * np.asarray(k, np.float64)
    y, out = host_map(raw, kinds)
    out = np.where(np.asarray(held) != 0, out, LOST)
    lost = out == LOST
    y[lost] = x[lost]
    k1[act] = np.asarray(k, np.float64)[act]
    xs[act] = y[act]
    flag[act] = (out == LEFT)[act]
    status[act & lost] = LOST
    return xs, k1, flag, status


def host_correct(x, status, k1, flag, k, held, dt, kinds):
    """(x, status) after CORRECT with the velocities k, held at xs: for the active particles k2 = k1 where flag is set, else k;
    flag = 0 and held = 0: LOST; else x = map(x + (0.5 dt) (k1 + k2)), or left: status LEFT and x = the raw point, or lost:
    status LOST and x stays."""
    x, status = np.array(x, np.float64), np.array(status, np.uint8)
    k1, left = np.asarray(k1, np.float64), np.asarray(flag) != 0
    act = status == ACTIVE
    with np.errstate(all="ignore"):
        k2 = np.where(left[:, None], k1, np.asarray(k, np.float64))
        h = 0.5 * dt
        s = k1 + k2
        raw = x + h * s
    y, out = host_map(raw, kinds)
    out = np.where(left | (np.asarray(held) != 0), out, LOST)
    moved = act & (out != LOST)
    x[moved] = y[moved]
    status[act & (out == LOST)] = LOST
    status[act & (out == LEFT)] = LEFT
    return x, status


# ---- the device object ---------------------------------------------------------------------------------------------------------
class Tracers:
    """M particles on a solver's mesh. Device tensors, all made here: x float64 [M, dim], status uint8 [M], the work arrays
    xs, k1 [M, dim], flag uint8 [M] (PREDICT's map said "left"), the element hints hint_x, hint_xs int32 [M] and the velocity
    block k float64 [M, dim] / held int32 [M] (one buffer: what the ranks sum). No later call allocates or waits for the
    device; every call is enqueued on `stream` (default: the current stream at the call).

    Hints: a particle under a CFL-limited step mostly stays in its element, so each velocity pass first tries the element
    found last time (one array for x, one for xs) and searches only when that one does not cover the point. The result does
    not depend on the hints; `rebind` drops them."""

    def __init__(self, solver, points, stream=None):
        import torch
        from . import hip
        self._hip = hip
        self.stream = stream
        self._bind(solver)
        if isinstance(points, torch.Tensor):
            p = points.detach().to(device="cuda", dtype=torch.float64)
        else:
            p = torch.from_numpy(np.array(points, np.float64, order="C")).cuda()          # (a copy: a read-only array is fine)
        if p.ndim != 2 or p.shape[1] != self.dim:
            raise ValueError(f"points must have shape [M, {self.dim}], got {tuple(p.shape)}")
        m, dim = int(p.shape[0]), self.dim
        self.M = m
        self.x = p.contiguous().clone()
        self.status = torch.zeros(m, dtype=torch.uint8, device="cuda")
        self.xs = self.x.clone()
        self.k1 = torch.zeros((m, dim), dtype=torch.float64, device="cuda")
        self.flag = torch.zeros(m, dtype=torch.uint8, device="cuda")
        self.hint_x = torch.full((m,), -1, dtype=torch.int32, device="cuda")
        self.hint_xs = torch.full((m,), -1, dtype=torch.int32, device="cuda")
        # k and held in one block of 8-byte words, so that the ranks combine them in one collective (_combine)
        self._kh = torch.zeros(m * dim + (m + 1) // 2, dtype=torch.int64, device="cuda")
        self.k = self._kh[:m * dim].view(torch.float64).view(m, dim)
        self.held = self._kh[m * dim:].view(torch.int32)[:m]

    def _bind(self, solver):
        part = solver.part
        dim, sub = sample.check_partition(part, hasattr(solver, "S"))
        kinds = side_kinds(part.mesh.sides)
        if getattr(self, "solver", None) is not None:
            if dim != self.dim or not np.array_equal(kinds, self.kinds):
                raise ValueError("rebind needs a solver on a mesh of the same dimension and sides")
        self.dim, self.sub, self.kinds = dim, sub, kinds
        self._sides = TracerSides()
        for a in range(2 * dim):
            self._sides.kind[a] = int(kinds[a])
        self._sampler = sample.sampler(solver)                      # keys and levels on the device, built once per solver
        self.solver = solver

    # -- arguments -----------------------------------------------------------------------------------------------------
    def _stream(self, stream):
        import torch
        stream = self.stream if stream is None else stream
        return torch.cuda.current_stream() if stream is None else stream

    @staticmethod
    def _dt(dt):
        dt = float(dt)
        if not math.isfinite(dt):
            raise ValueError(f"dt must be finite, got {dt}")
        return dt

    def _state(self, step):
        return self.solver.get_own_variables(self.solver.next if step is None else step)

    def _arrays(self):
        p = self._hip.ptr
        return p(self.x), p(self.xs), p(self.k1), p(self.flag), p(self.status)

    def _given(self, k, held):
        import torch
        ok = (isinstance(k, torch.Tensor) and isinstance(held, torch.Tensor) and k.is_cuda and held.is_cuda
              and k.dtype == torch.float64 and held.dtype == torch.int32 and tuple(k.shape) == (self.M, self.dim)
              and tuple(held.shape) == (self.M,) and k.is_contiguous() and held.is_contiguous())
        if not ok:
            raise ValueError(f"k must be a contiguous float64 device tensor [{self.M}, {self.dim}] and held an int32 one [{self.M}]")
        return k, held

    # -- the calls -------------------------------------------------------------------------------------------------------
    def velocity(self, which="x", step=None, stream=None):
        """(k, held): the velocity at every x (which="x") or xs ("xs") from state(step) (default: the solver's current state)
        and whether an owned cell holds the point, in the object's own block -- overwritten by the next velocity, predict or
        correct call with `dist`. One launch of t8gpu_hip_tracers_velocity_*, with the hints of that array."""
        if which not in ("x", "xs"):
            raise ValueError(f"which must be 'x' or 'xs', got {which!r}")
        points, hint = (self.x, self.hint_x) if which == "x" else (self.xs, self.hint_xs)
        p, s = self._hip.ptr, self._sampler
        self._hip.call("t8gpu_hip_tracers_velocity", self.solver.dtype, self.dim, C.c_size_t(self.M), p(points), p(s.keys),
                       p(s.levels), s.N, s.sub, self._state(step), p(hint), p(self.k), p(self.held),
                       self._hip.stream_ptr(self._stream(stream)))
        return self.k, self.held

    def _combine(self, dist, stream):
        """k and held summed over the ranks, in place, in one all_reduce of the block as 8-byte integers: all ranks but the one
        that holds a point contribute words of zero bits (+0.0, held 0), so the integer sum is that rank's words bit for bit,
        NaN payloads and -0.0 included, and two packed held counts cannot carry into each other. On the GPU for nccl; any
        other backend (gloo: several ranks rehearsed on one GPU) goes through a host copy, which waits for the device."""
        import torch
        with torch.cuda.stream(stream):
            if dist.get_backend() == "nccl":
                dist.all_reduce(self._kh, op=dist.ReduceOp.SUM)
            else:
                staged = self._kh.cpu()
                dist.all_reduce(staged, op=dist.ReduceOp.SUM)
                self._kh.copy_(staged)

    def _move(self, phase, dt, k, held, stream):
        lib = self._hip.lib()
        lib.t8gpu_hip_tracers_move.restype = C.c_int
        self._hip.check(lib.t8gpu_hip_tracers_move(self.dim, phase, C.c_size_t(self.M), C.c_double(dt), self._sides, self._hip.ptr(k),
                                                   self._hip.ptr(held), *self._arrays(), self._hip.stream_ptr(stream)))

    def _phase(self, phase, dt, dist, k, held, step, stream):
        dt, stream = self._dt(dt), self._stream(stream)
        if (k is None) != (held is None):
            raise ValueError("k and held come together")
        if k is not None:
            self._move(phase, dt, *self._given(k, held), stream)
        elif dist is not None:
            self.velocity("x" if phase == PREDICT else "xs", step, stream)
            self._combine(dist, stream)
            self._move(phase, dt, self.k, self.held, stream)
        else:
            p, s = self._hip.ptr, self._sampler
            hint = self.hint_x if phase == PREDICT else self.hint_xs
            self._hip.call("t8gpu_hip_tracers_step", self.solver.dtype, self.dim, phase, C.c_size_t(self.M), C.c_double(dt),
                           self._sides, p(s.keys), p(s.levels), s.N, s.sub, self._state(step), p(hint), *self._arrays(),
                           self._hip.stream_ptr(stream))

    def predict(self, dt, dist=None, k=None, held=None, step=None, stream=None):
        """Before the flow step: k1 = u^n(x), xs = map(x + dt k1), from state(step) (default: the solver's current state). One
        fused launch on a single-rank partition; dist= (torch.distributed, every rank holding all particles): velocity, one
        all_reduce, move; k=, held=: move alone on velocities the caller combined. dt finite (ValueError), negative: backwards."""
        self._phase(PREDICT, dt, dist, k, held, step, stream)

    def correct(self, dt, dist=None, k=None, held=None, step=None, stream=None):
        """After the flow step: k2 = u^(n+1)(xs), x = map(x + (dt / 2) (k1 + k2)); arguments as predict"""
        self._phase(CORRECT, dt, dist, k, held, step, stream)

    def rebind(self, new_solver, stream=None):
        """After amr.adapt*: go on with `new_solver`, which must be on a mesh of the same dimension and sides (ValueError; no
        SynthMesh partition: TypeError). x, status and k1 keep their bits; only the hints are dropped. Builds the new solver's
        keys on first use, as any sampling call would; nothing else is allocated."""
        import torch
        self._bind(new_solver)
        with torch.cuda.stream(self._stream(stream)):
            self.hint_x.fill_(-1)
            self.hint_xs.fill_(-1)
        return self

    def sample(self, names, **kw):
        """solver.sample_points(tr.x, names, ...): fields at the particles (`fill` where no owned cell holds one)"""
        return self.solver.sample_points(self.x, names, **kw)

    def host(self):
        """{"x", "status", "xs", "k1"}: numpy copies (this one waits for the device)"""
        return {n: getattr(self, n).cpu().numpy() for n in ("x", "status", "xs", "k1")}

    def counts(self):
        """(active, left, lost) particle counts (this one waits for the device)"""
        c = np.bincount(self.status.cpu().numpy(), minlength=3)
        return int(c[ACTIVE]), int(c[LEFT]), int(c[LOST])
