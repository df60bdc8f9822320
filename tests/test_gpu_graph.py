"""-m gpu: hipGraph replay of the native step driver (t8gpu_hip_plain_stepper_graph): a whole iterate_steps() call of a
single-rank stepper -- its tile / block launches -- captured once and replayed with one hipGraphLaunch must give bitwise the
result of the direct enqueue. A stepper with a halo always enqueues directly."""
import types

import numpy as np
import pytest
import torch

from _gpu import perturbed_state
from t8gpu_amd import native
from t8gpu_amd.solver import PlainSolver, SubgridSolver
from t8gpu_amd.synth import SynthMesh

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["plain", "subgrid"])
def test_graph_replay_equals_direct_enqueue_single_rank(kind):
    if kind == "plain":
        mesh = SynthMesh(2, 4, 7, band=0.06)
        part = mesh.partition()
        st = perturbed_state(part, 3)
        make = lambda: PlainSolver(part, torch.float64, mode="fused", state=st)
        dt = 0.1 * 2.0 ** -mesh.finest_level
    else:
        mesh = SynthMesh(3, 3, 4, band=0.05)
        part = mesh.partition(subgrid=True)
        make = lambda: SubgridSolver(part, torch.float32, mode="fused")
        dt = 0.1 * 2.0 ** -(mesh.finest_level + 2)
    a, b = make(), make()
    a.use_native_stepper()
    b.use_native_stepper()
    b.stepper.graph(True)
    for n in (5, 5, 5, 2, 5, 5, 5):      # an odd step count swaps the roles of the Step0 / Step3 planes from call to call
        a.iterate_steps(n, dt)
        b.iterate_steps(n, dt)
    torch.cuda.synchronize()
    captures, replays = b.stepper.graph()
    # three argument sets -- (5, roles A), (5, roles B), (2, roles B) -- and the stepper keeps four executables: every set
    # is captured exactly once however the calls alternate (one cached executable re-captured on every call)
    assert replays == 7 and captures == 3, (captures, replays)
    assert torch.equal(a.state(), b.state())
    assert a.stepper.graph() == (0, 0)



def test_graph_mode_is_off_by_default_for_steppers_with_a_halo():
    """A stepper with a halo enqueues directly -- the two-lane driver -- whatever the graph switch says: zero captures, zero
    replays, the same bits as without the switch. (Rank 0 of a shift-symmetric two-way split exchanging with itself through a
    one-rank RCCL communicator, as in test_gpu_halo.py, so the ghost values matter.)"""
    mesh = SynthMesh(2, 5, 8, band=0.05)
    whole, half = mesh.partition(), mesh.partition(0, 2)
    x, y = whole.centres[:, 0], whole.centres[:, 1]
    rho = 1.5 + 0.4 * np.sin(4 * np.pi * y) * np.cos(2 * np.pi * x)
    v1, v2 = 0.3 * np.cos(4 * np.pi * y), 0.2 * np.sin(2 * np.pi * x) * np.sin(4 * np.pi * y)
    st = np.stack([rho, rho * v1, rho * v2, 0 * rho, 2.5 / 0.4 + 0.5 * rho * (v1 * v1 + v2 * v2)])
    n2 = whole.N // 2
    st[:, n2:] = st[:, :n2]
    gidx = np.concatenate([np.arange(half.N), half.ghost_global])
    comm = native.NativeComm(0, 1, lambda b, src: b)
    fake = types.SimpleNamespace(N=half.N, G=half.G, cells_per_element=1, peers=np.zeros(1, np.int32), send_off=half.send_off,
                                 recv_off=half.recv_off, send_idx=half.send_idx)

    def run(graph):
        local = st[:, gidx].copy()
        g = PlainSolver(half, torch.float64, mode="fused", state=local, plan_options=dict(tmax=64, fcap=160))
        g.use_native_stepper(native.NativeHalo(fake, torch.float64, comm))
        g.stepper.graph(graph)
        dt = 0.1 * 2.0 ** -mesh.finest_level
        for _ in range(4):
            g.iterate_steps(6, dt)
        assert native.stream_wait(torch.cuda.current_stream(), 60.0) == 0
        out, counts = g.state().clone(), g.stepper.graph()
        g.stepper = None
        return out, counts

    direct, _ = run(False)
    replayed, counts = run(True)
    assert counts == (0, 0), counts
    assert torch.equal(direct, replayed)
    comm.destroy()
