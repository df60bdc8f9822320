"""Adaptation of a running solver: CompressibleEulerSolver::adapt (examples/compressible_euler/solver.cu:243-277) +
MeshManager::adapt (t8gpu/mesh/mesh_manager.inl:196-330), and their Subgrid counterparts (examples/subgrid/solver.inl:327-345,
t8gpu/mesh/subgrid_mesh_manager.inl).

Indicator and data transfer are HIP kernels behind the C-ABI (estimate_gradient, refinement criteria,
adapt_variables_and_volume); the forest operations (adapt callback, refine / coarsen, 2:1 balance, the
old->new correspondence) run on the host in the mesh provider, where the reference calls t8code.

Plain and Subgrid solvers go through one single-rank body (_adapt), one repartition (_Repartition) and one collective body
(_adapt_collective). The solver supplies what differs between them: like(part), the empty solver of its configuration on
the new partition, and cell_geometry(), the (dim, cells per element, volumes) that pick and feed the transfer kernel
(_transfer). The public functions add their defaults and reference criterion, the two Partitioned classes the wire format
of their state message.
"""
import ctypes as C
import time

import numpy as np
import torch

from . import hip
from .solver import FLUXES


def refinement_criteria(solver):
    """estimate_gradient + compute_refinement_criteria (solver.cu:245-263); returns a device tensor [N]."""
    s = hip.stream_ptr()
    grad = solver.planes[5 * FLUXES]          # the reference reuses the Fluxes/Rho plane (solver.cu:249)
    rho = solver.planes[5 * solver.next]
    hip.call("t8gpu_hip_estimate_gradient", solver.dtype, solver.F, hip.ptr(solver.fn), None, hip.ptr(rho), hip.ptr(grad), s)
    crit = torch.empty(solver.N, dtype=solver.dtype, device="cuda")
    hip.call("t8gpu_hip_refinement_criteria", solver.dtype, solver.N, hip.ptr(grad), hip.ptr(solver.planes[25]), hip.ptr(crit), s)
    grad[:solver.N + solver.G].zero_()        # solver.cu:269-270
    return crit


def subgrid_refinement_criteria(solver):
    """compute_refinement_criteria<Subgrid> (examples/subgrid/solver.inl:329-340); device tensor [N]."""
    crit = torch.empty(solver.N, dtype=solver.dtype, device="cuda")
    hip.call("t8gpu_hip_subgrid_refinement_criteria", solver.dtype, solver.rank, solver.N, hip.ptr(solver.planes[5 * solver.next]),
             hip.ptr(solver.volumes), hip.ptr(crit), hip.stream_ptr())
    return crit


class Loehner:
    """The scale-free refinement indicator of csrc/hip/indicator.hip (include/t8gpu_hip.h): Loehner's estimator
    without cross terms, per axis, on the maximum over `quantities` ("density", "pressure", "mach", "entropy"), with the noise
    filter `filter` (eps) and `buffer` layers of face neighbours added to every flagged element / block. Dimensionless, in
    [0, 1], independent of the level: one pair of thresholds serves every problem and every max_level. Pass it as
    `indicator=` to the adapt functions of this module; `threshold` is then the refine threshold (customarily 0.8) and
    `coarsen_below` the coarsen threshold (customarily 0.2)."""
    QUANTITIES = {"density": 1, "pressure": 2, "mach": 4, "entropy": 8}       # T8GPU_INDICATOR_* of include/t8gpu_hip.h

    def __init__(self, quantities=("density",), filter=0.01, buffer=0):
        names = [quantities] if isinstance(quantities, str) else list(quantities)
        if not names:
            raise ValueError("Loehner needs at least one quantity")
        for name in names:
            if name not in self.QUANTITIES:
                raise ValueError(f"unknown indicator quantity {name!r}: one of {', '.join(self.QUANTITIES)}")
        if not float(filter) >= 0.0:
            raise ValueError(f"filter must be >= 0, got {filter}")
        if int(buffer) != buffer or buffer < 0:
            raise ValueError(f"buffer must be a number of layers >= 0, got {buffer}")
        self.quantities, self.filter, self.buffer = tuple(names), float(filter), int(buffer)
        self.mask = 0
        for name in names:
            self.mask |= self.QUANTITIES[name]

    def _launch(self, solver, step, stream, halo, cell_out, block_out):
        from . import fields
        s = solver.next if step is None else step
        stream = torch.cuda.current_stream() if stream is None else stream
        if halo is not None:
            with torch.cuda.stream(stream):
                halo.exchange(solver.step_planes(s))
        off, ent = fields._csr(solver)
        st, sp = solver.get_own_variables(s), hip.stream_ptr(stream)
        mask, eps = C.c_uint(self.mask), C.c_double(self.filter)
        if hasattr(solver, "S"):
            hip.call("t8gpu_hip_subgrid_indicator", solver.dtype, solver.rank, solver.N, mask, eps, st, hip.ptr(solver.volumes),
                     hip.ptr(solver.fn), hip.ptr(solver.level_diff), hip.ptr(solver.nb_offset), hip.ptr(solver.normals),
                     hip.ptr(solver.areas), hip.ptr(off), hip.ptr(ent), hip.ptr(cell_out), hip.ptr(block_out), sp)
        else:
            hip.call("t8gpu_hip_plain_indicator", solver.dtype, solver.N, solver.ndim, int(solver.part.mesh.dim), mask, eps, st,
                     hip.ptr(solver.get_own_volume()), hip.ptr(solver.fn), hip.ptr(solver.normals), hip.ptr(solver.areas),
                     hip.ptr(off), hip.ptr(ent), hip.ptr(cell_out), sp)

    def cell_values(self, solver, step=None, stream=None, halo=None):
        """float64 device tensor [owned_cells] of the indicator of state(step) in storage order (Subgrid: per subcell). One
        launch on `stream`, no sync. `halo` refreshes the ghost slots of that step first, as for derived_fields; without it
        the caller vouches that they are current."""
        stream = torch.cuda.current_stream() if stream is None else stream
        with torch.cuda.stream(stream):
            out = torch.empty(solver.owned_cells, dtype=torch.float64, device="cuda")
        self._launch(solver, step, stream, halo, out, None)
        return out

    def criteria(self, solver, halo=None, ghosts_current=False):
        """float64 device tensor [N] of the `next` state: one value per element / block (Subgrid: the maximum over the block's
        subcells), after `buffer` spread passes (t8gpu_hip_indicator_spread). On several ranks `halo` (the run's HaloExchange)
        also refreshes the ghost entries of the criteria before every pass, so that the marks do not depend on the number
        of ranks. ghosts_current: the caller has just exchanged the state through `halo`; it is not exchanged again."""
        from . import fields
        N, G = solver.N, solver.G
        cur = torch.zeros(N + G, dtype=torch.float64, device="cuda")
        state_halo = None if ghosts_current else halo
        if hasattr(solver, "S"):
            self._launch(solver, None, None, state_halo, None, cur)
        else:
            self._launch(solver, None, None, state_halo, cur, None)
        if self.buffer and N > 0:
            off, ent = fields._csr(solver)
            nxt = torch.zeros_like(cur)
            for _ in range(self.buffer):
                if G > 0:
                    if halo is None:
                        raise ValueError("buffer layers on a partition with ghosts need halo= (the ghost entries of the criteria "
                                         "are exchanged between the passes)")
                    halo.exchange_elements(cur)
                hip.check(hip.lib().t8gpu_hip_indicator_spread(N, hip.ptr(cur), hip.ptr(solver.fn), hip.ptr(off), hip.ptr(ent),
                                                               hip.ptr(nxt), hip.stream_ptr()))
                cur, nxt = nxt, cur
        return cur[:N]


def _criteria(solver, reference, indicator, halo=None):
    """the criteria [N] on the device: reference(solver) (indicator None) or indicator.criteria(); with a `halo` the caller has
    exchanged the state's ghosts already"""
    if indicator is not None:
        return indicator.criteria(solver, halo, ghosts_current=halo is not None)
    return reference(solver)


def _check_carry(carry, solver):
    """`carry` as a tuple of objects with .sums (float64 device tensor [P, owned_cells]) and .solver (this solver): per-cell
    payload that rides through the adapt beside the state, e.g. a stats.Statistics. ValueError otherwise."""
    carry = tuple(carry)
    for c in carry:
        if c.solver is not solver:
            raise ValueError("a carried object must belong to the solver that is adapted")
        t = c.sums
        if not (t.is_cuda and t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == solver.owned_cells):
            raise ValueError(f"carried sums must be a float64 device tensor [P, {solver.owned_cells}], got {tuple(t.shape)} {t.dtype}")
    return carry


def _transfer(adapt_dev, n_new, dim, S, dtype, old, new, vol_old, vol_new):
    """adapt_variables_and_volume of five planes onto n_new new elements (child = parent, coarsened = mean of the family,
    kept = copy) for elements of S cells: the plain entry (S == 1) or the block-wise one of Subgrid. old / new: T8gpuVars."""
    name, sizes = (("t8gpu_hip_adapt_variables_and_volume", (n_new, dim)) if S == 1 else
                   ("t8gpu_hip_subgrid_adapt_variables_and_volume", (dim, n_new)))
    hip.call(name, dtype, *sizes, hip.ptr(adapt_dev), old, new, hip.ptr(vol_old), hip.ptr(vol_new), hip.stream_ptr())


def _transfer_carry(sums, adapt_dev, n_new, dim, S):
    """sums [P, n_old S] -> [P, n_new S] by the state's own transfer through the _f64 entries, five planes a call. The entries'
    volume arguments get scratch; a last group of fewer than five planes is filled up with scratch planes."""
    P, n_old = sums.shape[0], sums.shape[1] // S
    groups = (P + 4) // 5
    old = sums.contiguous()
    if 5 * groups != P:
        old = torch.cat([old, torch.zeros((5 * groups - P, old.shape[1]), dtype=torch.float64, device=old.device)])
    new = torch.zeros((5 * groups, n_new * S), dtype=torch.float64, device=old.device)
    if n_new > 0 and P > 0:
        vol_old = torch.ones(max(1, n_old), dtype=torch.float64, device=old.device)
        vol_new = torch.empty(n_new, dtype=torch.float64, device=old.device)
        for g in range(groups):
            _transfer(adapt_dev, n_new, dim, S, torch.float64, hip.vars_of(old, g), hip.vars_of(new, g), vol_old, vol_new)
    return new[:P]


def _hand_over(carry, new_sums, new_solver):
    """each carried object now refers to the new solver and holds its transferred sums"""
    for c, t in zip(carry, new_sums):
        c.sums, c.solver = t, new_solver


def _adapt(solver, reference, keep_stepper, threshold, min_level, max_level, family_members_averaged, volume_dim, indicator,
           coarsen_below, carry):
    """adapt() and adapt_subgrid(): criteria, marks, forest adapt, the new partition and its empty solver, the transfer
    straight into that solver's planes and volumes, the carried sums, one sync."""
    carry = _check_carry(carry, solver)
    part = solver.part
    assert part.nranks == 1, "multi-rank adaptation goes through amr.adapt_partitioned / amr.adapt_subgrid_partitioned"
    mesh = part.mesh
    t0 = time.perf_counter()
    crit = _criteria(solver, reference, indicator).double().cpu().numpy()
    t1 = time.perf_counter()
    marks = mesh.marks_from_criteria(crit, threshold, min_level, max_level, family_members_averaged, coarsen_below=coarsen_below)
    new_mesh, adapt_data = mesh.adapt(marks)
    new_part = new_mesh.partition(0, 1, subgrid=part.subgrid, normal_dim=part.normal_dim)
    t2 = time.perf_counter()
    new = solver.like(new_part)
    t3 = time.perf_counter()
    dim, S, volumes = solver.cell_geometry()
    dim = dim if volume_dim is None else volume_dim
    ad = torch.from_numpy(adapt_data).cuda()
    _transfer(ad, new_part.N, dim, S, solver.dtype, solver.get_own_variables(solver.next), new.get_own_variables(new.next),
              volumes, new.cell_geometry()[2])
    _hand_over(carry, [_transfer_carry(c.sums, ad, new_part.N, dim, S) for c in carry], new)
    torch.cuda.synchronize()
    if keep_stepper and solver.stepper is not None:
        new.use_native_stepper()
    t4 = time.perf_counter()
    new.last_adapt_criteria_sum = float(crit.sum())
    # where the cycle went (seconds): the indicator kernels + read-back, the mesh provider (forest adapt + balance,
    # partition + connectivity: t8code's share in the reference), this backend's tile plan + upload + new planes, the
    # transfer kernel + step driver
    plan_s = getattr(new, "plan_build_s", 0.0)
    new.last_adapt_split = {"indicator": t1 - t0, "provider": t2 - t1, "plan": plan_s, "planes_upload": (t3 - t2) - plan_s,
                            "transfer": t4 - t3}
    return new, marks, adapt_data


def adapt(solver, threshold=10.0, min_level=1, max_level=4, family_members_averaged=4, volume_dim=None, indicator=None,
          coarsen_below=None, carry=()):
    """Refine / coarsen the mesh of a single-rank PlainSolver by the reference's criterion and transfer the
    current solution. Returns the new solver (same dtype, flux, kernel tier, step bookkeeping; the native stepper again if
    the old one had it), the marks and the old -> new correspondence.
    indicator (a Loehner): its criteria instead of the reference's, `threshold` the refine threshold; coarsen_below: the
    coarsen threshold of the two-threshold marks (None: `threshold`, the reference's walk).
    carry: objects with .sums (float64 device tensor [P, owned_cells]) and .solver, e.g. a stats.Statistics: their sums are
    transferred like the state and they refer to the new solver afterwards. The return values do not change."""
    return _adapt(solver, refinement_criteria, True, threshold, min_level, max_level, family_members_averaged, volume_dim,
                  indicator, coarsen_below, carry)


def adapt_subgrid(solver, threshold=0.02, min_level=1, max_level=6, family_members_averaged=4, indicator=None, coarsen_below=None,
                  carry=()):
    """SubgridCompressibleEulerSolver::adapt (examples/subgrid/solver.inl:327-345) for a single-rank SubgridSolver:
    H1-seminorm indicator, the forest adapt, block-wise data transfer (subgrid_mesh_manager.inl:246-425).
    indicator (a Loehner): its block maxima instead, `threshold` the refine threshold; coarsen_below and carry: as for
    adapt(); carried sums follow the subcell rule of the block transfer."""
    return _adapt(solver, subgrid_refinement_criteria, False, threshold, min_level, max_level, family_members_averaged, None,
                  indicator, coarsen_below, carry)


def _runs(planes, first, n, S, per_element=()):
    """the views of elements [first, first + n) of every tensor of `planes` ([P, elements S]) and of `per_element` ([elements])"""
    return [t[:, first * S:(first + n) * S] for t in planes] + [t[first:first + n] for t in per_element]


def _pieces(buf, runs):
    """the views of the message `buf` that hold `runs` one after the other"""
    at, out = 0, []
    for r in runs:
        out.append(buf[at:at + r.numel()].view(r.shape))
        at += r.numel()
    return out


def _pack(runs):
    """one message of the runs, one after the other"""
    buf = torch.empty(sum(r.numel() for r in runs), dtype=runs[0].dtype, device=runs[0].device)
    for piece, r in zip(_pieces(buf, runs), runs):
        piece.copy_(r)
    return buf


def _unpack(buf, runs):
    for piece, r in zip(_pieces(buf, runs), runs):
        r.copy_(piece)


class _Repartition:
    """adapt() + partition() of an SFC-partitioned run (MeshManager::adapt followed by MeshManager::partition), one rank per
    GPU. Every rank holds the (cheap) forest description, so the forest operations are replicated and only the
    element payloads travel: marks that would split a family over two ranks are dropped, the forest is adapted, each rank
    transfers its own elements on the device into temporary planes and ships contiguous runs of them (one message per
    destination) to their owners in the new equal split -- the reference instead lets the new owner PULL through CUDA-IPC
    pointers (partition_data<<<>>>, mesh_manager.inl:626-643). Split in prepare (the constructor) / transport / finish so that
    the transport can be RCCL (torch.distributed P2P), gloo (CPU tests) or a loopback (one-GPU tests).

    sends / recvs: (peer, first, count) in the temporary / the new planes. sendbufs / recvbufs[peer]: the state message,
    5 S + 1 values per element in the solver's type, in the format of the subclass (_pack_state / _unpack_state).
    carry_sendbufs / carry_recvbufs[peer]: one more message per peer for the objects of `carry` (_check_carry), float64, the
    objects' runs [P, count S] one after the other; finish() hands the objects over to the new solver."""

    def __init__(self, solver, all_criteria, threshold, min_level, max_level, family_members_averaged, coarsen_below, carry):
        self.carry = _check_carry(carry, solver)
        part = solver.part
        self.solver, self.rank, self.world = solver, part.rank, part.nranks
        mesh = part.mesh
        marks = mesh.marks_from_criteria(all_criteria, threshold, min_level, max_level, family_members_averaged,
                                         coarsen_below=coarsen_below)
        old_off = mesh.partition_offsets(self.world)
        self.marks = mesh.unmark_split_families(marks, old_off[1:-1])
        self.new_mesh, adapt_data = mesh.adapt(self.marks)
        # new elements made from rank p's old elements: [have_off[p], have_off[p+1])
        self.have_off = np.searchsorted(adapt_data[:-1], old_off, side="left").astype(np.int64)
        self.have_off[-1] = self.new_mesh.num_elements
        self.new_off = self.new_mesh.partition_offsets(self.world)
        a, b = int(self.have_off[self.rank]), int(self.have_off[self.rank + 1])
        self.n_have = b - a
        # the old -> new correspondence of this rank's adapted elements, relative to its old ones (the transfer kernels' input)
        self.adapt_local = (adapt_data[a:b + 1] - old_off[self.rank]).astype(np.int32)
        # message plan: intersections of what I have with what every rank will own (and vice versa)
        self.sends, self.recvs = [], []
        lo_r, hi_r = int(self.new_off[self.rank]), int(self.new_off[self.rank + 1])
        for q in range(self.world):
            s0, s1 = max(a, int(self.new_off[q])), min(b, int(self.new_off[q + 1]))
            if s1 > s0:
                self.sends.append((q, s0 - a, s1 - s0))                  # (peer, first in the temporary planes, count)
            r0, r1 = max(int(self.have_off[q]), lo_r), min(int(self.have_off[q + 1]), hi_r)
            if r1 > r0:
                self.recvs.append((q, r0 - lo_r, r1 - r0))               # (peer, first in the new planes, count)
        # 1. local data transfer into temporary planes: one allocation, the state's five planes and the volumes behind them
        dim, S, volumes = solver.cell_geometry()
        dtype, dev, room = solver.dtype, solver.planes.device, max(1, self.n_have)
        tmp = torch.zeros((5 * S + 1) * room, dtype=dtype, device=dev)
        self.S, self.tmp, self.tmp_vol = S, tmp[:5 * S * room].view(5, S * room), tmp[5 * S * room:]
        ad_local = torch.from_numpy(self.adapt_local).to(dev)
        if self.n_have:
            _transfer(ad_local, self.n_have, dim, S, dtype, solver.get_own_variables(solver.next), hip.vars_of(self.tmp),
                      volumes, self.tmp_vol)
        self.carry_tmp = [_transfer_carry(c.sums, ad_local, self.n_have, dim, S) for c in self.carry]
        # 2. the new partition and an empty solver for it
        self.new_part = self.new_mesh.partition(self.rank, self.world, subgrid=part.subgrid, normal_dim=part.normal_dim)
        self.new_solver = solver.like(self.new_part)
        # 3. the messages
        out = [(q, first, n) for q, first, n in self.sends if q != self.rank]
        into = [(q, n) for q, _, n in self.recvs if q != self.rank]
        self.sendbufs = {q: self._pack_state(first, n) for q, first, n in out}
        self.recvbufs = {q: torch.empty((5 * S + 1) * n, dtype=dtype, device=dev) for q, n in into}
        self.carry_sendbufs, self.carry_recvbufs = {}, {}
        if self.carry:
            width = sum(t.shape[0] for t in self.carry_tmp) * S
            self.carry_sendbufs = {q: _pack(_runs(self.carry_tmp, first, n, S)) for q, first, n in out}
            self.carry_recvbufs = {q: torch.empty(width * n, dtype=torch.float64, device=dev) for q, n in into}

    def kept_first(self):
        """first element of the temporary planes that stays on this rank (its receive from itself)"""
        return [f for p, f, m in self.sends if p == self.rank][0]

    def transport(self, dist, host_staged=False):
        """host_staged: move the messages through host memory (gloo, which cannot send device buffers). Ships the state's
        messages and, behind them in the same order, the carried ones."""
        torch.cuda.synchronize()
        pairs = [(self.recvbufs, self.sendbufs)]
        if self.carry:
            pairs.append((self.carry_recvbufs, self.carry_sendbufs))
        staged, ops = [], []
        for recvbufs, sendbufs in pairs:
            rbuf = {q: (b.cpu() if host_staged else b) for q, b in recvbufs.items()}
            sbuf = {q: (b.cpu() if host_staged else b) for q, b in sendbufs.items()}
            staged.append((recvbufs, rbuf))
            for q, _, n in self.recvs:
                if q != self.rank:
                    ops.append(dist.P2POp(dist.irecv, rbuf[q], q))
            for q, _, n in self.sends:
                if q != self.rank:
                    ops.append(dist.P2POp(dist.isend, sbuf[q], q))
        if ops:
            for req in dist.batch_isend_irecv(ops):
                req.wait()
        if host_staged:
            for recvbufs, rbuf in staged:
                for q, b in recvbufs.items():
                    b.copy_(rbuf[q])

    def finish(self):
        """the new solver with its state, volumes and the carried sums put together from the kept run and the received messages"""
        new, S = self.new_solver, self.S
        sums = [torch.zeros((t.shape[0], new.owned_cells), dtype=torch.float64, device=t.device) for t in self.carry_tmp]
        state, volumes = [new.step_planes(new.next)], [new.cell_geometry()[2]]
        for q, first, n in self.recvs:
            if q == self.rank:       # stays here: straight from the temporary planes
                kept = _runs([self.tmp] + self.carry_tmp, self.kept_first(), n, S, [self.tmp_vol])
                for dst, src in zip(_runs(state + sums, first, n, S, volumes), kept):
                    dst.copy_(src)
            else:
                self._unpack_state(self.recvbufs[q], first, n)
                if self.carry:
                    _unpack(self.carry_recvbufs[q], _runs(sums, first, n, S))
        _hand_over(self.carry, sums, new)
        torch.cuda.synchronize()
        return new


class PartitionedAdapt(_Repartition):
    """adapt() + partition() for an SFC-partitioned plain-element run (MeshManager::adapt followed by
    MeshManager::partition, t8gpu/mesh/mesh_manager.inl:196-330, 645-723): a message is 5 variables + volume per element,
    packed by a gather kernel."""

    def __init__(self, solver, all_criteria, threshold=10.0, min_level=1, max_level=4, family_members_averaged=4, indicator=None,
                 coarsen_below=None, carry=()):
        """indicator: where all_criteria came from (adapt_partitioned evaluates it; nothing here depends on it);
        coarsen_below: the coarsen threshold of the two-threshold marks (None: `threshold`); carry: as for adapt()"""
        super().__init__(solver, all_criteria, threshold, min_level, max_level, family_members_averaged, coarsen_below, carry)

    def _pack_state(self, first, n):
        buf = torch.empty(6 * n, dtype=self.tmp.dtype, device=self.tmp.device)
        hip.call("t8gpu_hip_gather_elements", buf.dtype, n, first, hip.vars_of(self.tmp), hip.ptr(self.tmp_vol), hip.ptr(buf),
                 hip.stream_ptr())
        return buf

    def _unpack_state(self, buf, first, n):
        new = self.new_solver
        hip.call("t8gpu_hip_scatter_elements", buf.dtype, n, first, hip.ptr(buf), new.get_own_variables(new.next),
                 hip.ptr(new.planes[25]), hip.stream_ptr())


class PartitionedSubgridAdapt(_Repartition):
    """adapt() + partition() for an SFC-partitioned Subgrid run (SubgridMeshManager::adapt followed by
    SubgridMeshManager::partition, t8gpu/mesh/subgrid_mesh_manager.inl:428-558, 1217-1369): the transfer is block-wise
    injection / mean (subgrid_mesh_manager.inl:246-425), a message is 5 x 4^rank values + one volume per block. A run of
    blocks is contiguous in every variable plane, so a message is six slices; no gather kernel is needed."""

    def __init__(self, solver, all_criteria, threshold=0.02, min_level=1, max_level=6, family_members_averaged=4, indicator=None,
                 coarsen_below=None, carry=()):
        """indicator / coarsen_below / carry: as for PartitionedAdapt"""
        super().__init__(solver, all_criteria, threshold, min_level, max_level, family_members_averaged, coarsen_below, carry)

    def _pack_state(self, first, n):
        return _pack(_runs([self.tmp], first, n, self.S, [self.tmp_vol]))

    def _unpack_state(self, buf, first, n):
        new = self.new_solver
        _unpack(buf, _runs([new.step_planes(new.next)], first, n, self.S, [new.volumes]))


def _gather_criteria(crit, solver, dist, host_staged):
    world = solver.part.nranks
    off = solver.part.mesh.partition_offsets(world)
    crit = crit.cpu() if host_staged else crit
    sizes = [int(off[r + 1] - off[r]) for r in range(world)]
    width = max(sizes)                       # all_gather wants equal contributions: pad to the largest share
    mine = torch.zeros(width, dtype=torch.float64, device=crit.device)
    mine[: crit.numel()] = crit
    chunks = [torch.empty(width, dtype=torch.float64, device=crit.device) for _ in range(world)]
    dist.all_gather(chunks, mine)
    return torch.cat([c[:n] for c, n in zip(chunks, sizes)]).cpu().numpy()


def _adapt_collective(repartition, reference, reads_ghosts, solver, dist, host_staged, halo, kw):
    """adapt_partitioned() and adapt_subgrid_partitioned(): the state's ghosts exchanged where the criteria read them
    (`reads_ghosts`: the reference criterion does; an indicator always does), the criteria of every rank gathered, then
    prepare / transport / finish of `repartition`."""
    indicator = kw.get("indicator")
    if solver.part.nranks > 1 and (reads_ghosts or indicator is not None):
        if halo is None:
            from .halo import HaloExchange
            halo = HaloExchange(solver.part, solver.dtype, dist, overlap=False, stage_through_host=host_staged)
        halo.exchange(solver.step_planes(solver.next))
    all_crit = _gather_criteria(_criteria(solver, reference, indicator, halo).double(), solver, dist, host_staged)
    pa = repartition(solver, all_crit, **kw)
    pa.transport(dist, host_staged)
    new = pa.finish()
    new.last_adapt_criteria_sum = float(all_crit.sum())      # diagnostic: equal (to rounding) for every rank count
    return new


def adapt_partitioned(solver, dist, host_staged=False, halo=None, **kw):
    """Collective: every rank calls it with its own solver; returns the rank's new solver.
    host_staged: collectives and messages through host memory (gloo).

    The indicator (estimate_gradient, solver.cu:245-263) reads rho of GHOST elements of the `next` state, and neither
    step driver refreshes those slots -- a stage only exchanges the ghosts of its SOURCE state, so after a step the
    last stage's output carries ghost values two stages old. The exchange is therefore part of this function (through
    `halo`, the run's HaloExchange of this partition, or a temporary one): refinement marks must not depend on the
    number of ranks. indicator= (a Loehner), coarsen_below= and carry= go to PartitionedAdapt; the indicator's buffer passes
    exchange the ghost entries of the criteria through the same `halo`. carry: as for adapt(): every rank's carried objects
    travel with its elements and refer to its new solver afterwards."""
    return _adapt_collective(PartitionedAdapt, refinement_criteria, True, solver, dist, host_staged, halo, kw)


def adapt_subgrid_partitioned(solver, dist, host_staged=False, halo=None, **kw):
    """Collective: every rank calls it with its own SubgridSolver; returns the rank's new solver.
    The reference's criterion reads no other block, so without indicator= nothing is exchanged. A Loehner indicator reads the
    ghost blocks of the `next` state: they are exchanged first, through `halo` (the run's HaloExchange of this partition) or a
    temporary one, as in adapt_partitioned. carry= goes to PartitionedSubgridAdapt, as there."""
    return _adapt_collective(PartitionedSubgridAdapt, subgrid_refinement_criteria, False, solver, dist, host_staged, halo, kw)
