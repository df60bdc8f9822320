"""-m gpu: run-time boundary states. PlainSolver.set_inflow_states / SubgridSolver.set_inflow_states refill the device inflow
table in place: a solver built with states s1 continues, after set_inflow_states(s2), like a solver built with s2 from the same
state -- in the compat and fused tiers, through the native step driver and a replayed graph; a ramp (new states every step)
follows the composed reference whose table changes at the same steps; amr.adapt hands on the current states."""
import numpy as np
import pytest
import torch

from _farfield import FarCase
from _gpu import NP, TOL1, TOL10, perturbed_state, rel_err
from test_gpu_farfield import mesh_of as plain_mesh_of
from test_gpu_subgrid_farfield import SubgridFarCase
from test_gpu_subgrid_open_boundaries import dt_of as subgrid_dt_of, mesh_of as subgrid_mesh_of
from t8gpu_amd import amr, hip
from t8gpu_amd.solver import PlainSolver, SubgridSolver
from t8gpu_amd.synth import SynthMesh

pytestmark = pytest.mark.gpu

SIDES = (0, ("farfield", 1), "periodic", "periodic")     # -x inflow with state 0, +x far field against state 1


def states_of(rows):
    return np.array([[rho, rho * v[0], rho * v[1], rho * v[2], p / 0.4 + 0.5 * rho * sum(c * c for c in v)] for rho, v, p in rows])


S1 = states_of([(1.0, (0.3, 0.0, 0.0), 1.0), (1.2, (0.4, 0.1, 0.05), 1.1)])
S2 = states_of([(1.1, (0.5, 0.05, 0.0), 1.2), (0.9, (-0.2, 0.1, 0.0), 0.95)])


def ramp(t):
    """states moving linearly from S1 (t = 0) to S2 (t = 1)"""
    return (1 - t) * S1 + t * S2


class Case:
    """one solver class with its mesh, step size and composed reference"""

    def __init__(self, cls):
        self.cls = cls
        if cls == "plain":
            self.mesh = plain_mesh_of(2, SIDES)
            self.part = self.mesh.partition()
            self.dt = 0.1 * 2.0 ** -self.mesh.finest_level
        else:
            self.mesh = subgrid_mesh_of(2, SIDES)
            self.part = self.mesh.partition(subgrid=True)
            self.dt = subgrid_dt_of(self.mesh)

    def state(self, seed):
        return perturbed_state(self.part, seed)

    def solver(self, dtype, mode, state, states, part=None):
        part = self.part if part is None else part
        if self.cls == "plain":
            return PlainSolver(part, dtype, mode=mode, state=state, inflow_states=states)
        return SubgridSolver(part, dtype, mode=mode, state=state, open_boundaries=True, farfield=True, inflow_states=states)

    def reference(self, dtype, state, states):
        return (FarCase if self.cls == "plain" else SubgridFarCase)(self.part, NP[dtype], state, states)


def _continue_from(case, a, dtype, mode, states):
    """a solver built with `states` on the current state of `a`"""
    torch.cuda.synchronize()
    st = a.planes[5 * a.next:5 * a.next + 5].cpu().numpy()
    return case.solver(dtype, mode, st if case.cls == "subgrid" else st[:, :a.N + a.G], states)


@pytest.mark.parametrize("cls", ["plain", "subgrid"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("mode", ["compat", "fused"])
def test_updated_states_act_like_states_given_at_construction(cls, dtype, mode):
    case = Case(cls)
    a = case.solver(dtype, mode, case.state(31), S1)
    keep = case.solver(dtype, mode, case.state(31), S1)          # (never updated: the update must matter)
    table = a.inflow_table.data_ptr()
    for _ in range(2):
        a.iterate(case.dt)
        keep.iterate(case.dt)
    b = _continue_from(case, a, dtype, mode, S2)
    a.set_inflow_states(S2)
    assert a.inflow_table.data_ptr() == table and np.array_equal(a.inflow_states, S2)
    if mode == "fused":
        assert a.plan.c.inflow == table
    assert torch.equal(a.inflow_table, b.inflow_table)
    for _ in range(3):
        a.iterate(case.dt)
        b.iterate(case.dt)
        keep.iterate(case.dt)
    torch.cuda.synchronize()
    assert torch.isfinite(a.state()).all()
    if mode == "fused":
        assert torch.equal(a.state(), b.state())
    else:                                                        # (the compat tier sums by atomics)
        assert rel_err(a.state().cpu().numpy(), b.state().cpu().numpy()) < TOL1[dtype]
    assert rel_err(keep.state().cpu().numpy(), b.state().cpu().numpy()) > 100 * TOL1[dtype]


@pytest.mark.parametrize("cls", ["plain", "subgrid"])
def test_native_driver_and_graph_replay_read_the_updated_table(cls):
    """iterate_steps of the native driver, directly enqueued and as a replayed graph (captured before the update: the graph
    reads the table by pointer), against the python stages with the same sequence of updates. Default queue settings."""
    case = Case(cls)
    dtype = torch.float64
    py, nat, gr = (case.solver(dtype, "fused", case.state(32), S1) for _ in range(3))
    nat.use_native_stepper()
    gr.use_native_stepper()
    gr.stepper.graph(True)
    seq = [None, None, S2, None, ramp(0.5)]                      # the update before each run of two steps (None: none)
    for s in seq:
        for g in (py, nat, gr):
            if s is not None:
                g.set_inflow_states(s)
        for _ in range(2):
            py.iterate(case.dt)
        nat.iterate_steps(2, case.dt)
        gr.iterate_steps(2, case.dt)
    torch.cuda.synchronize()
    captures, replays = gr.stepper.graph()
    assert captures == 1 and replays == len(seq), (captures, replays)
    assert torch.isfinite(py.state()).all()
    assert torch.equal(py.state(), nat.state())
    assert torch.equal(nat.state(), gr.state())
    fresh = case.solver(dtype, "fused", case.state(32), S1)      # ... and the updates did change the run
    for _ in range(2 * len(seq)):
        fresh.iterate(case.dt)
    torch.cuda.synchronize()
    assert not torch.equal(fresh.state(), py.state())


@pytest.mark.parametrize("cls", ["plain", "subgrid"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("mode", ["compat", "fused"])
def test_a_ramp_is_followed(cls, dtype, mode):
    """per step set_inflow_states(s(t)) against the composed reference whose table is changed at the same steps"""
    case = Case(cls)
    st = case.state(33)
    g = case.solver(dtype, mode, st, S1)
    o = case.reference(dtype, st, S1)
    for step in range(10):
        s = ramp(step / 9)
        g.set_inflow_states(s)
        o.inflow = s.astype(NP[dtype])
        g.iterate(case.dt)
        o.iterate(case.dt)
    torch.cuda.synchronize()
    err = rel_err(g.state().cpu().numpy(), o.current()[:, :g.owned_cells])
    print(f"ramp {cls} {dtype} {mode}: 10 steps {err:.2e}")
    assert err < TOL10[dtype]
    assert np.array_equal(g.inflow_states, S2)


def test_every_rank_of_a_partitioned_run_updates_its_table():
    """3-way loopback partition of the Subgrid mesh: each rank calls set_inflow_states; bitwise the single-rank run"""
    from t8gpu_amd.halo import HaloExchange
    from test_gpu_halo import loopback
    case = Case("subgrid")
    mesh, whole, S, dtype = case.mesh, case.part, 16, torch.float64
    st = case.state(34)
    ref = case.solver(dtype, "fused", st, S1)
    solvers, halos = [], []
    for r in range(3):
        part = mesh.partition(r, 3, subgrid=True)
        blocks = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
        cells = (blocks[:, None] * S + np.arange(S)[None, :]).reshape(-1)
        solvers.append(case.solver(dtype, "fused", st[:, cells].copy(), S1, part=part))
        halos.append(HaloExchange(part, dtype, dist=None, overlap=False))
    for step in range(3):
        for g in [ref] + solvers:
            g.set_inflow_states(ramp(step / 2))
        ref.iterate(case.dt)
        for s in solvers:
            s.begin_step()
        for k in range(3):
            for s, h in zip(solvers, halos):
                h._pack(s.step_planes(s.stage_steps(k)[0]))
            loopback(halos)
            for s, h in zip(solvers, halos):
                h._unpack(s.step_planes(s.stage_steps(k)[0]))
            torch.cuda.synchronize()
            for s in solvers:
                s.run_stage(k, case.dt, split=True)
            torch.cuda.synchronize()
    full = torch.cat([s.state() for s in solvers], dim=1)
    assert torch.equal(full, ref.state())


@pytest.mark.parametrize("cls", ["plain", "subgrid"])
def test_wrong_shapes_unphysical_rows_and_closed_solvers_raise(cls):
    case = Case(cls)
    g = case.solver(torch.float64, "fused", case.state(35), S1)
    table = g.inflow_table.clone()
    for bad in (S1[:1], np.concatenate([S1, S1[:1]]), S1[:, :4], np.array([[1.0, 0, 0, 0, -1.0], S1[1]]),
                np.array([[-1.0, 0, 0, 0, 2.5], S1[1]]), np.full((2, 5), np.nan)):
        with pytest.raises(ValueError):
            g.set_inflow_states(bad)
    torch.cuda.synchronize()
    assert torch.equal(g.inflow_table, table) and np.array_equal(g.inflow_states, S1)
    if cls == "plain":
        closed = PlainSolver(SynthMesh(2, 3, 4, band=0.1).partition(), torch.float64, mode="fused")
    else:
        closed = SubgridSolver(SynthMesh(2, 2, 3).partition(subgrid=True), torch.float64, mode="fused")
    with pytest.raises(ValueError, match="open boundaries"):
        closed.set_inflow_states(S1)


def test_adapt_hands_on_the_updated_states():
    case = Case("plain")
    g = case.solver(torch.float64, "fused", case.state(36), S1)
    g.iterate(case.dt)
    g.set_inflow_states(S2)
    new, _, _ = amr.adapt(g, threshold=10.0, min_level=3, max_level=7)
    assert np.array_equal(new.inflow_states, S2)
    ref = case.solver(torch.float64, "fused", case.state(36), S2)
    torch.cuda.synchronize()
    assert torch.equal(new.inflow_table, ref.inflow_table)
    case = Case("subgrid")
    g = case.solver(torch.float64, "fused", case.state(36), S1)
    g.iterate(case.dt)
    g.set_inflow_states(S2)
    new, _, _ = amr.adapt_subgrid(g, threshold=0.02, min_level=3, max_level=5)
    assert new.farfield and np.array_equal(new.inflow_states, S2)
    ref = case.solver(torch.float64, "fused", case.state(36), S2)
    torch.cuda.synchronize()
    assert torch.equal(new.inflow_table, ref.inflow_table)
