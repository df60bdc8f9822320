"""The scale-free refinement indicator without a GPU: the numpy reference (tests/_indicator_ref.py) against closed forms, its
bounds and level independence, the two-threshold marks of the mesh provider, HaloExchange.exchange_elements over gloo, and the
argument checks of the Python layer. The kernels are compared with the same reference in test_gpu_indicator.py."""
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _indicator_ref as ref
from _gpu import perturbed_state
from t8gpu_amd import amr
from t8gpu_amd.synth import SynthMesh

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EPS = 0.01


# ---- the reference against closed forms -------------------------------------------------------------------------------------
def test_closed_form_values_of_the_2d_step():
    """the values a prototype of the definition gave for qL = 1, qR = 0.25, eps = 0.01 in 2D"""
    assert abs(ref.step_closed_form(1.0, 0.25, EPS, (2,)) - 0.957216631868556) < 1e-14
    assert abs(ref.step_closed_form(0.25, 1.0, EPS, (2,)) - 0.9771157615002408) < 1e-14


@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("dim", [2, 3])
def test_density_step_meets_the_closed_form(dim, subgrid):
    """A density step at x = 0.5 on a uniform walled mesh: x = 0.5 is a block edge, the cross-block case the reference's Subgrid
    criterion cannot see. The two columns of cells beside the step meet the closed form within 1e-14 (a tangential axis of a
    cell at a wall tangent to the step normal has one interior face, else two); every other cell is exactly 0."""
    part = ref.uniform_walled(dim).partition(subgrid=subgrid)
    assert part.B > 0 and np.all(part.levels == part.levels[0])
    got = ref.reference(ref.step_state(part), part, np.float64, "density", EPS)
    want = ref.step_expected(part, EPS)
    x, edge = ref.cell_centres(part)
    per_axis = (4 if subgrid else 1) * 2 ** int(part.levels[0])
    assert (want > 0).sum() == 2 * per_axis ** (dim - 1)
    assert np.all(got[want == 0] == 0.0)
    assert np.abs(got - want).max() <= 1e-14
    inner = (want > 0) & np.all((x[: got.size, 1:dim] > edge[: got.size, None]) & (x[: got.size, 1:dim] < 1 - edge[: got.size, None]), axis=1)
    left = inner & (x[: got.size, 0] < 0.5)
    assert left.any() and (inner & ~left).any()
    m = (2,) * (dim - 1)
    assert np.abs(got[left] - ref.step_closed_form(ref.Q_LEFT, ref.Q_RIGHT, EPS, m)).max() <= 1e-14
    assert np.abs(got[inner & ~left] - ref.step_closed_form(ref.Q_RIGHT, ref.Q_LEFT, EPS, m)).max() <= 1e-14


# ---- bounds -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh_of(name):
    return ref.REFINED[name]()


@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", list(ref.REFINED))
def test_values_lie_in_the_unit_interval(mesh, subgrid):
    part = mesh_of(mesh).partition(subgrid=subgrid)
    u = perturbed_state(part, 11)
    lo, hi = np.inf, -np.inf
    for name in ref.QUANTITIES:
        E = ref.reference(u, part, np.float64, name, EPS)
        assert E.shape == (part.N * part.cells_per_element,) and np.all(np.isfinite(E)), (mesh, name)
        assert E.min() >= 0.0 and E.max() <= 1.0, (mesh, name, E.min(), E.max())
        lo, hi = min(lo, E.min()), max(hi, E.max())
    allq = ref.reference(u, part, np.float64, ref.QUANTITIES, EPS)
    assert np.all(allq >= 0.0) and np.all(allq <= 1.0)
    print(f"{mesh} subgrid={subgrid}: E in [{lo:.3g}, {hi:.3g}]")
    assert hi > 0.5 and lo < 0.1                                # the data exercises the range


# ---- level independence -----------------------------------------------------------------------------------------------------
def test_kelvin_helmholtz_maximum_does_not_depend_on_the_level():
    """rho = 2 inside |y - 0.5| < 0.25, 1 outside: the same maximum at every level (the closed form of the lighter side), and
    exactly two rows of cells per interface are non-zero"""
    want = ref.step_closed_form(1.0, 2.0, EPS, (2,))
    for L in range(5, 9):
        part = SynthMesh(2, L, L).partition()
        E = ref.reference(part.kh_initial_state(), part, np.float64, "density", EPS)
        assert abs(E.max() - want) <= 1e-14, (L, E.max(), want)
        assert int((E != 0).sum()) == 4 * 2 ** L, (L, int((E != 0).sum()))


# ---- marks with two thresholds ----------------------------------------------------------------------------------------------
def family_walk(part, crit, refine_above, coarsen_below, min_level, max_level, averaged):
    """the provider's walk in plain numpy: own refinement test, then every complete family whose first member does not refine"""
    dim, n = part.mesh.dim, part.N
    nsub = 2 ** dim
    navg = min(averaged, nsub) if averaged > 0 else nsub
    levels = part.levels[:n]
    first = ((levels < max_level) & (crit > refine_above)).astype(np.int8)
    marks = first.copy()
    parent = np.floor(part.centres[:n, :dim] / (2.0 * 0.5 ** levels[:, None])).astype(np.int64)
    child = np.floor(part.centres[:n, :dim] / (0.5 ** levels[:, None])).astype(np.int64) & 1
    for e in range(n - nsub + 1):
        if first[e] != 0 or levels[e] <= min_level or levels[e] == 0 or child[e].any():
            continue
        if not (np.all(levels[e:e + nsub] == levels[e]) and np.all(parent[e:e + nsub] == parent[e])):
            continue
        mean = 0.0
        for ch in range(navg):
            mean += crit[e + ch] / navg
        if mean < coarsen_below:
            marks[e:e + nsub] = -1
    return marks


@pytest.mark.parametrize("averaged", [4, 0])
@pytest.mark.parametrize("mesh", ["refined-2d-walls", "refined-3d-periodic"])
def test_marks_with_two_thresholds(mesh, averaged):
    m = mesh_of(mesh)
    part = m.partition()
    rng = np.random.default_rng(5)
    crit = rng.uniform(0.0, 1.0, part.N)
    lo_level, hi_level = int(part.levels.min()), int(part.levels.max())
    for t in (0.3, 0.5, 0.8):
        for min_level, max_level in ((1, 6), (lo_level, hi_level), (hi_level, hi_level + 1)):
            old = m.marks_from_criteria(crit, t, min_level, max_level, averaged)
            same = m.marks_from_criteria(crit, t, min_level, max_level, averaged, coarsen_below=t)
            assert old.dtype == same.dtype == np.int8 and old.tobytes() == same.tobytes()
            assert np.array_equal(old, family_walk(part, crit, t, t, min_level, max_level, averaged))
    seen = set()
    for hi, lo in ((0.8, 0.2), (0.6, 0.45), (0.5, 0.0)):
        old = m.marks_from_criteria(crit, hi, 1, 6, averaged)
        got = m.marks_from_criteria(crit, hi, 1, 6, averaged, coarsen_below=lo)
        want = family_walk(part, crit, hi, lo, 1, 6, averaged)
        assert np.array_equal(got, want), (hi, lo)
        assert np.all(got[old == 1] == 1)                       # the +1 set is unchanged
        assert np.all(old[got == -1] == -1) and (got == -1).sum() <= (old == -1).sum()
        seen |= set(np.unique(got).tolist())
    assert seen == {-1, 0, 1}


# ---- exchange_elements over gloo --------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _exchange_rank_main(rank, world, port, subgrid, out_path):
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    from t8gpu_amd.halo import HaloExchange
    from t8gpu_amd.synth import SynthMesh

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    mesh = SynthMesh(2, 3, 5, band=0.05)
    part = mesh.partition(rank, world, subgrid=subgrid)
    halo = HaloExchange(part, torch.float64, dist, device="cpu")
    values = torch.full((part.N + part.G,), -1.0, dtype=torch.float64)
    values[: part.N] = torch.arange(part.first_global, part.first_global + part.N, dtype=torch.float64)
    owned = values[: part.N].clone()
    halo.exchange_elements(values)
    ok = part.G > 0 and torch.equal(values[: part.N], owned) and \
        np.array_equal(values[part.N:].numpy(), part.ghost_global.astype(np.float64))
    flags = [None] * world if rank == 0 else None
    dist.gather_object(bool(ok), flags, dst=0)
    if rank == 0:
        np.save(out_path, np.array(flags, np.int64))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_exchange_elements_over_gloo(world, subgrid, tmp_path):
    """values = the global element index: afterwards the ghost entries equal ghost_global and the owned ones are untouched"""
    out = str(tmp_path / "ok.npy")
    mp.spawn(_exchange_rank_main, args=(world, _free_port(), subgrid, out), nprocs=world, join=True)
    flags = np.load(out)
    assert flags.shape == (world,) and np.all(flags == 1)


def test_exchange_elements_checks_its_argument():
    from t8gpu_amd.halo import HaloExchange
    part = SynthMesh(2, 3, 4, band=0.1).partition()
    h = HaloExchange(part, torch.float64, dist, device="cpu")
    x = torch.arange(part.N, dtype=torch.float64)
    h.exchange_elements(x)                                      # one rank: nothing to do
    assert torch.equal(x, torch.arange(part.N, dtype=torch.float64))
    with pytest.raises(ValueError):
        h.exchange_elements(torch.zeros(part.N, dtype=torch.float32))
    with pytest.raises(ValueError):
        h.exchange_elements(torch.zeros(part.N + 1, dtype=torch.float64))


# ---- argument checks of the Python layer -------------------------------------------------------------------------------------
def test_loehner_checks_its_arguments():
    ind = amr.Loehner()
    assert (ind.quantities, ind.filter, ind.buffer, ind.mask) == (("density",), 0.01, 0, 1)
    assert amr.Loehner(("density", "pressure", "mach", "entropy")).mask == 15
    assert amr.Loehner("entropy", filter=0.0, buffer=2).mask == 8
    for bad in (dict(quantities=("density", "enstrophy")), dict(quantities=()), dict(filter=-0.01), dict(filter=float("nan")),
                dict(buffer=-1), dict(buffer=1.5)):
        with pytest.raises(ValueError):
            amr.Loehner(**bad)
