"""-m gpu: the time statistics (t8gpu_hip_stats_accumulate_*, t8gpu_hip_stats_results, _Solver.statistics, carry= of the adapt
functions, extra= of the sampler, vtk.get_host_statistics_variable) against numpy (tests/_stats_ref.py).

Tolerances. The kernels' arithmetic is in double for both float types and starts from the state as the device holds it, so
one tolerance serves both: 1e-12 of max |want| per plane (the argument of test_gpu_fields.py: a handful of double operations
per value). The rms and stress planes are differences of two nearly equal terms and are measured against the raw second
moment, max A_k / W (ref.scales). The transfer of the sums forms the mean of at most 8 doubles: 1e-14 relative.

Meshes. The "refined" construction of test_gpu_fields.py gives 115 (2D) and 127 (3D) elements: odd, so every accumulator row
of the plain solvers after the first is off 16 bytes and the scalar form runs; more than 64 and no multiple of 64.
SynthMesh(2, 4, 4) has 256: the 16-byte form. Subgrid solvers have 16 / 64 cells per block and always take the 16-byte form.
`check_alignment` asserts all this, so a mesh change cannot hide a path."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _stats_ref as ref
from _gpu import NP, perturbed_state
from _vtu import read_vtu
from test_gpu_fields import refined, z_order_permutation
from t8gpu_amd import amr, hip, stats as stats_mod, vtk
from t8gpu_amd.solver import PlainSolver, SubgridSolver
from t8gpu_amd.synth import SynthMesh
from t8gpu_amd.unstructured import PrismHexMesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float64, torch.float32]
TOL, TOL_TRANSFER, TOL_VOLUME = 1e-12, 1e-14, 1e-13
SENTINEL = -7.25
WEIGHTS = (0.3, 1.7, 0.05)
NAMES = list(stats_mod.RESULTS)

MESHES = {
    "refined-2d": lambda: refined(2, 3, True, 0.3, 0.8),
    "refined-3d": lambda: refined(3, 2, True, 0.2, 0.8),
    "aligned-2d": lambda: SynthMesh(2, 4, 4),
}
ODD = {"refined-2d": 115, "refined-3d": 127}
CASES = [(m, sg) for m in MESHES for sg in (False, True)] + [("prism", False)]


def make_solver(part, dtype, state):
    cls = SubgridSolver if getattr(part, "subgrid", False) else PlainSolver
    return cls(part, dtype, mode="compat", state=state)


def partition_of(mesh, subgrid):
    if mesh == "prism":
        return PrismHexMesh(5).partition()
    return MESHES[mesh]().partition(subgrid=subgrid)


def time_step(part):
    return 0.1 * 2.0 ** -(part.mesh.finest_level + (2 if getattr(part, "subgrid", False) else 0))


def C_size(n):
    return ctypes.c_size_t(n)


def C_double(x):
    return ctypes.c_double(x)


def bits(t):
    return t.contiguous().view(torch.int64)


def aligned16(t):
    return t.data_ptr() % 16 == 0


def check_alignment(mesh, subgrid, solver, st):
    """which form of the accumulate kernel this case runs (module docstring)"""
    rows = [st.sums[k] for k in range(stats_mod.PLANES)] + [solver.planes[5 * solver.next + k] for k in range(5)]
    if mesh in ODD and not subgrid:
        assert solver.N == ODD[mesh] and solver.N > 64 and solver.N % 64 != 0 and solver.N % 2 == 1
        assert not all(aligned16(r) for r in rows)
    elif mesh != "prism":
        assert all(aligned16(r) for r in rows) and st.sums.stride(0) % 2 == 0
        if mesh == "aligned-2d" and not subgrid:
            assert solver.N == 256


def check_planes(got, want, scale, what, tol=TOL):
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    for k in range(want.shape[0]):
        s = scale[k] if scale is not None else np.abs(want[k]).max()
        err = np.abs(got[k] - want[k]).max() if want.shape[1] else 0.0
        print(f"{what} plane {k}: max error / scale = {err / max(s, 1e-300):.2e}")
        assert err <= tol * s, (what, k, err, s)


class Run:
    """three steps with three weights on one case: after each step the device sums and the reference sums accumulated from
    solver.state(); two Statistics objects fed the same sequence. Built once, never written afterwards."""

    def __init__(self, mesh, subgrid, dtype):
        self.part = partition_of(mesh, subgrid)
        self.solver = make_solver(self.part, dtype, perturbed_state(self.part, 21))
        self.a, self.b = self.solver.statistics(), self.solver.statistics()
        check_alignment(mesh, subgrid, self.solver, self.a)
        self.cells = self.solver.owned_cells
        assert tuple(self.a.sums.shape) == (15, self.cells) and self.a.sums.dtype == torch.float64 and self.a.weight == 0.0
        assert bool((self.a.sums == 0).all())
        dt = time_step(self.part)
        want = np.zeros((ref.PLANES, self.cells))
        self.steps = []
        for w in WEIGHTS:
            self.solver.iterate(dt)
            self.a.accumulate(w)
            self.b.accumulate(w)
            want = ref.accumulate(want, self.solver.state().double().cpu().numpy(), w)
            self.steps.append((self.a.sums.cpu().numpy().copy(), want))
        self.W = sum(WEIGHTS)
        self.sums = self.steps[-1][0]


@functools.lru_cache(maxsize=None)
def run(mesh, subgrid, dtype):
    return Run(mesh, subgrid, dtype)


# ---- accumulate ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mesh,subgrid", CASES)
def test_sums_follow_the_reference_step_by_step(mesh, subgrid, dtype):
    r = run(mesh, subgrid, dtype)
    for n, (got, want) in enumerate(r.steps):
        assert np.all(np.isfinite(want))
        check_planes(got, want, None, f"{mesh} subgrid={subgrid} step {n}")
    assert r.a.weight == pytest.approx(r.W, rel=1e-15) and r.a.weight == r.b.weight
    assert r.a.sums.data_ptr() != r.b.sums.data_ptr()
    assert torch.equal(bits(r.a.sums), bits(r.b.sums))             # the same sequence: identical bits


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_kernel_forms_give_the_same_bits_and_stop_at_num_cells(dtype):
    """the aligned mesh through the C entry: rows on 16 bytes (the 16-byte form), rows 8 bytes off (the scalar form), and
    255 of the 256 cells (127 whole pairs, then the one cell behind them) -- cell 255 stays as it was"""
    r = run("aligned-2d", False, dtype)
    solver, n = r.solver, r.cells
    st = solver.get_own_variables(solver.next)

    def call(sums, cells):
        hip.call("t8gpu_hip_stats_accumulate", dtype, C_size(cells), st, C_double(0.625), hip.ptr(sums), C_size(sums.stride(0)),
                 hip.stream_ptr())
        torch.cuda.synchronize()

    wide = torch.full((15, n), 0.5, dtype=torch.float64, device="cuda")
    flat = torch.full((15 * n + 1,), 0.5, dtype=torch.float64, device="cuda")
    off = flat[1:].view(15, n)
    assert aligned16(wide) and not aligned16(off)
    call(wide, n)
    call(off, n)
    assert torch.equal(bits(wide), bits(off))
    want = 0.5 + 0.625 * ref.quantities(solver.state().double().cpu().numpy())
    check_planes(wide.cpu().numpy(), want, None, "C entry")
    part = torch.full((15, n), 0.5, dtype=torch.float64, device="cuda")
    call(part, n - 1)
    assert torch.equal(bits(part[:, :n - 1]), bits(wide[:, :n - 1])) and bool((part[:, n - 1] == 0.5).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_ghost_slots_are_neither_read_nor_written(dtype):
    """rank 1 of 3 of the 115-element mesh: 38 owned elements, ghost slots behind them filled with NaN"""
    mesh = MESHES["refined-2d"]()
    assert list(mesh.partition_offsets(3)) == [0, 38, 76, 115]
    part = mesh.partition(1, 3)
    assert part.N == 38 and part.G > 0
    whole = perturbed_state(mesh.partition(), 21)
    gidx = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
    solver = make_solver(part, dtype, whole[:, gidx])
    solver.planes[:, part.N:] = float("nan")
    before = solver.planes.clone()
    st = solver.statistics()
    assert tuple(st.sums.shape) == (15, 38)
    st.accumulate(0.7)
    st.accumulate(0.2)
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int64 if dtype == torch.float64 else torch.int32),
                       solver.planes.view(torch.int64 if dtype == torch.float64 else torch.int32))
    own = ref.uploaded(whole[:, part.first_global:part.first_global + part.N], NP[dtype])
    want = ref.accumulate(ref.accumulate(np.zeros((15, 38)), own, 0.7), own, 0.2)
    got = st.sums.cpu().numpy()
    assert np.all(np.isfinite(got))
    check_planes(got, want, None, "rank 1 of 3")


def test_weights_and_names_are_validated():
    r = run("refined-2d", False, torch.float64)
    st = r.solver.statistics()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            st.accumulate(bad)
    with pytest.raises(ValueError):
        st.results(["tke"])                                     # weight == 0
    assert st.weight == 0.0 and bool((st.sums == 0).all())
    with pytest.raises(ValueError) as e:
        r.a.results(["tke", "kurtosis"])
    assert "mean_velocity" in str(e.value)
    st.accumulate(1.5)
    st.reset()
    torch.cuda.synchronize()
    assert st.weight == 0.0 and bool((st.sums == 0).all())


# ---- results ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mesh,subgrid", CASES)
def test_every_result_matches_the_reference(mesh, subgrid, dtype):
    r = run(mesh, subgrid, dtype)
    got = r.a.results(NAMES)
    assert list(got) == NAMES
    want, scale = ref.results(r.sums, r.W), ref.scales(r.sums, r.W)
    assert np.all(np.isfinite(want))
    for name, t in got.items():
        rows = ref.SLOTS[name]
        assert t.dtype == torch.float64 and t.is_cuda
        assert tuple(t.shape) == ((r.cells,) if len(rows) == 1 else (len(rows), r.cells)), name
        check_planes(np.atleast_2d(t.cpu().numpy()), want[rows], scale[rows], f"{mesh} subgrid={subgrid} {name}")
    one = r.a.results("density_rms")                            # a single name as a string
    assert torch.equal(bits(one["density_rms"]), bits(got["density_rms"]))


@pytest.mark.parametrize("mesh,subgrid", [("refined-2d", False), ("refined-3d", True)])
def test_planes_not_asked_for_stay_untouched(mesh, subgrid):
    r = run(mesh, subgrid, torch.float64)
    want = ref.results(r.sums, r.W)
    scale = ref.scales(r.sums, r.W)
    for names in (["tke"], ["mean_momentum", "pressure_rms"], ["reynolds_stress", "mean_mach"], ["mean_velocity", "density_rms"]):
        block = torch.full((ref.RESULT_PLANES, r.cells), SENTINEL, dtype=torch.float64, device="cuda")
        out = {name: block[ref.SLOTS[name][0]:ref.SLOTS[name][-1] + 1] for name in NAMES}    # a tensor for EVERY plane
        full = stats_mod.StatsPlanes()
        asked = [k for name in names for k in ref.SLOTS[name]]
        for k in asked:
            full.p[k] = block[k].data_ptr()
        lib = hip.lib()
        hip.check(lib.t8gpu_hip_stats_results(C_size(r.cells), hip.ptr(r.a.sums), C_size(r.a.sums.stride(0)), C_double(r.W), full,
                                              hip.stream_ptr()))
        torch.cuda.synchronize()
        got = block.cpu().numpy()
        for k in range(ref.RESULT_PLANES):
            if k in asked:
                assert np.abs(got[k] - want[k]).max() <= TOL * scale[k], (names, k)
            else:
                assert np.all(got[k] == SENTINEL), (names, k)
        block.fill_(SENTINEL)                                   # the front end: out= for the names asked for, nothing else
        res = r.a.results(names, out={name: out[name] for name in names})
        torch.cuda.synchronize()
        got = block.cpu().numpy()
        for k in range(ref.RESULT_PLANES):
            assert np.all(got[k] == SENTINEL) == (k not in asked), (names, k)
        for name in names:
            assert res[name].data_ptr() == block[ref.SLOTS[name][0]].data_ptr()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
def test_steady_state_has_no_fluctuation(subgrid, dtype):
    """a uniform state, 50 accumulations with unequal weights: rms <= 1e-6 of the mean (two terms, each with about
    100 * 2^-53 relative rounding, under a square root), |stress| <= 1e-12 rho |u|^2 (linear in the same terms)"""
    part = partition_of("refined-2d", subgrid)
    tot = (part.N + part.G) * part.cells_per_element
    rho, v, p = 1.3, (0.4, -0.7, 0.2), 0.9
    one = np.array([rho, rho * v[0], rho * v[1], rho * v[2], p / 0.4 + 0.5 * rho * sum(x * x for x in v)])
    solver = make_solver(part, dtype, np.repeat(one[:, None], tot, axis=1))
    st = solver.statistics()
    for w in np.random.default_rng(4).uniform(0.01, 3.0, 50):
        st.accumulate(float(w))
    got = st.results(["mean_density", "mean_pressure", "density_rms", "pressure_rms", "reynolds_stress", "tke"])
    held = ref.uploaded(one[:, None], NP[dtype])[:, 0]
    rho_d = held[0]
    p_d = 0.4 * (held[4] - 0.5 * (held[1:4] ** 2).sum() / rho_d)
    u2 = (held[1:4] ** 2).sum() / rho_d ** 2
    assert float((got["mean_density"] - rho_d).abs().max()) <= 1e-13 * rho_d
    assert float((got["mean_pressure"] - p_d).abs().max()) <= 1e-12 * p_d
    print(f"density_rms / mean {float(got['density_rms'].max()) / rho_d:.2e}  pressure_rms / mean "
          f"{float(got['pressure_rms'].max()) / p_d:.2e}  |stress| / rho |u|^2 "
          f"{float(got['reynolds_stress'].abs().max()) / (rho_d * u2):.2e}")
    assert float(got["density_rms"].max()) <= 1e-6 * rho_d and float(got["pressure_rms"].max()) <= 1e-6 * p_d
    assert float(got["reynolds_stress"].abs().max()) <= 1e-12 * rho_d * u2
    assert float(got["tke"].abs().max()) <= 1e-12 * u2


# ---- carry -----------------------------------------------------------------------------------------------------------------
def adapt_marks(mesh):
    """one mark set: coarsen the refined families, refine some of the other elements"""
    part = mesh.partition()
    lev = part.levels[:part.N]
    marks = np.where(lev == lev.max(), -1, 0).astype(np.int8)
    coarse = np.flatnonzero(lev == lev.min())
    marks[coarse[len(coarse) // 2::7]] = 1
    return marks


def steer(mesh, marks):
    """the adapt functions ask the mesh for the marks of their criteria: give them this mark set instead"""
    mesh.marks_from_criteria = lambda *a, **k: np.array(marks, np.int8)


def cell_volumes(part):
    S = part.cells_per_element
    return np.repeat(part.volumes[:part.N] / S, S)


def filled(solver, seed):
    """a Statistics of `solver` with two accumulations behind it, and a second, 7-plane payload of random numbers"""
    st = solver.statistics()
    st.accumulate(0.4)
    solver.iterate(time_step(solver.part))
    st.accumulate(1.1)

    class Payload:
        pass

    extra = Payload()
    extra.solver = solver
    extra.sums = torch.from_numpy(np.random.default_rng(seed).uniform(0.5, 2.0, (7, solver.owned_cells))).cuda()
    return st, extra


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", list(ODD))
def test_sums_ride_through_an_adapt(mesh, subgrid, dtype):
    m = MESHES[mesh]()
    part = m.partition(subgrid=subgrid)
    assert part.N == ODD[mesh]
    dim, S = m.dim, part.cells_per_element
    solver = make_solver(part, dtype, perturbed_state(part, 5))
    st, extra = filled(solver, 6)
    old = [st.sums.cpu().numpy().copy(), extra.sums.cpu().numpy().copy()]
    old_tensors = (st.sums, extra.sums)
    steer(m, adapt_marks(m))
    fn = amr.adapt_subgrid if subgrid else amr.adapt
    new, marks, ad = fn(solver, carry=(st, extra))
    assert np.array_equal(marks, adapt_marks(m))
    children, kept, coarsened = ref.cases_of(ad)
    assert children > 0 and kept > 0 and coarsened > 0
    assert st.solver is new and extra.solver is new and new is not solver
    assert tuple(st.sums.shape) == (15, new.owned_cells) and tuple(extra.sums.shape) == (7, new.owned_cells)
    assert st.weight == pytest.approx(1.5, rel=1e-15)
    for c, before, kept_tensor in zip((st, extra), old, old_tensors):
        assert np.array_equal(kept_tensor.cpu().numpy(), before)               # the old sums are left as they were
        want = ref.transfer(before, ad, S, dim)
        got = c.sums.cpu().numpy()
        check_planes(got, want, None, f"{mesh} subgrid={subgrid} transfer", TOL_TRANSFER)
        vol_old = (before * cell_volumes(part)).sum(axis=1)
        vol_new = (got * cell_volumes(new.part)).sum(axis=1)
        assert np.abs(vol_new - vol_old).max() <= TOL_VOLUME * np.abs(vol_old).max()
    # the new mesh goes on accumulating
    new.iterate(time_step(new.part))
    want = ref.accumulate(st.sums.cpu().numpy(), new.state().double().cpu().numpy(), 0.6)
    st.accumulate(0.6)
    check_planes(st.sums.cpu().numpy(), want, None, "after the adapt")
    assert st.weight == pytest.approx(2.1, rel=1e-15)
    # carry=() changes nothing, and a payload of another solver is refused
    with pytest.raises(ValueError):
        fn(solver, carry=(st,))


@pytest.mark.parametrize("world", [2, 5])
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", list(ODD))
def test_partitioned_carry_equals_the_single_rank_carry(mesh, subgrid, world):
    """`world` loopback ranks on one GPU, as test_gpu_amr.py drives PartitionedAdapt: the carried messages copied by hand from
    carry_sendbufs to carry_recvbufs; the concatenated sums are bitwise those of the single-rank carry with the same marks"""
    m = MESHES[mesh]()
    whole = m.partition(subgrid=subgrid)
    dim, S = m.dim, whole.cells_per_element
    state = perturbed_state(whole, 9)
    single = make_solver(whole, torch.float64, state)
    st, extra = filled(single, 10)
    state = single.state().cpu().numpy()                                       # what the ranks hold: the single rank's state now
    steer(m, adapt_marks(m))
    cls = amr.PartitionedSubgridAdapt if subgrid else amr.PartitionedAdapt
    pas, carried = [], []
    for r in range(world):
        part = m.partition(r, world, subgrid=subgrid)
        gidx = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
        cells = (gidx[:, None] * S + np.arange(S)[None, :]).reshape(-1)
        s = make_solver(part, torch.float64, state[:, cells])
        lo, hi = part.first_global * S, (part.first_global + part.N) * S
        mine = s.statistics()
        mine.sums.copy_(st.sums[:, lo:hi])
        mine.weight = st.weight

        class Payload:
            pass

        other = Payload()
        other.solver, other.sums = s, extra.sums[:, lo:hi].clone()
        carried.append((mine, other))
        pas.append(cls(s, np.zeros(whole.N), carry=(mine, other)))
    by_rank = {p.rank: p for p in pas}
    width = 6 if not subgrid else 5 * S + 1
    for p in pas:
        assert set(p.carry_sendbufs) == set(p.sendbufs) and set(p.carry_recvbufs) == set(p.recvbufs)
        for q, _, n in p.sends:
            if q != p.rank:
                assert p.sendbufs[q].numel() == width * n and p.carry_sendbufs[q].numel() == 22 * S * n
                assert p.carry_sendbufs[q].dtype == torch.float64
                by_rank[q].recvbufs[p.rank].copy_(p.sendbufs[q])
                by_rank[q].carry_recvbufs[p.rank].copy_(p.carry_sendbufs[q])
    news = [p.finish() for p in pas]
    assert any(len(p.sends) > 1 for p in pas)                                  # elements really changed owner
    steer(m, pas[0].marks)                                                     # the split-family-aware marks of the ranks
    fn = amr.adapt_subgrid if subgrid else amr.adapt
    new, marks, ad = fn(single, carry=(st, extra))
    assert np.array_equal(marks, pas[0].marks) and len(set(np.diff(ad).tolist())) >= 2
    assert sum(n.owned_cells for n in news) == new.owned_cells
    for (mine, other), n in zip(carried, news):
        assert mine.solver is n and other.solver is n and mine.sums.shape[1] == n.owned_cells
    assert torch.equal(bits(torch.cat([c[0].sums for c in carried], dim=1)), bits(st.sums))
    assert torch.equal(bits(torch.cat([c[1].sums for c in carried], dim=1)), bits(extra.sums))
    assert torch.equal(torch.cat([n.state() for n in news], dim=1), new.state())


# ---- consumers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
def test_sampling_takes_extra_planes(subgrid):
    r = run("refined-2d", subgrid, torch.float64)
    solver = r.solver
    res = r.a.results(["tke", "reynolds_stress"])
    plain = solver.sample_grid(["density", "mach"], (8, 8), cells=True)
    again = solver.sample_grid(["density", "mach"], (8, 8), cells=True, extra=None)
    unused = solver.sample_grid(["density", "mach"], (8, 8), cells=True, extra={"tke": res["tke"]})
    for name in ("density", "mach", "cell"):
        assert torch.equal(plain[name], again[name]) and torch.equal(plain[name], unused[name])
    cell = plain["cell"].long()
    assert bool((cell >= 0).all())
    assert torch.equal(plain["density"], solver.state()[0][cell])
    got = solver.sample_grid(["density", "tke"], (8, 8), extra={"tke": res["tke"]}, cells=True)
    assert list(got) == ["density", "tke", "cell"] and tuple(got["tke"].shape) == (8, 8)
    assert torch.equal(got["cell"], plain["cell"]) and torch.equal(got["density"], plain["density"])
    assert torch.equal(bits(got["tke"]), bits(res["tke"][cell]))
    six = solver.sample_grid(["reynolds_stress"], (8, 8), extra=res)["reynolds_stress"]
    assert tuple(six.shape) == (6, 8, 8) and torch.equal(bits(six), bits(res["reynolds_stress"][:, cell]))
    # the one-liners of the Statistics object
    assert torch.equal(bits(r.a.sample_grid(["tke"], (8, 8))["tke"]), bits(got["tke"]))
    pts = np.random.default_rng(8).uniform(0.0, 1.0, (37, 2))
    where = solver.locate(pts).long()
    at = r.a.sample_points(pts, ["mean_velocity", "tke"])
    mv = r.a.results(["mean_velocity"])["mean_velocity"]
    assert tuple(at["mean_velocity"].shape) == (3, 37)
    assert torch.equal(bits(at["mean_velocity"]), bits(mv[:, where])) and torch.equal(bits(at["tke"]), bits(res["tke"][where]))
    up = solver.resample_uniform(["tke"], 2, extra={"tke": res["tke"]})["tke"]
    assert tuple(up.shape) == (4, 4) and bool(torch.isfinite(up).all())
    # refusals: a built-in name, a wrong length, too many planes
    with pytest.raises(ValueError):
        solver.sample_grid(["density"], (8, 8), extra={"density": res["tke"]})
    with pytest.raises(ValueError):
        solver.sample_grid(["tke"], (8, 8), extra={"tke": res["tke"][:-1]})
    with pytest.raises(ValueError):
        solver.sample_grid(["tke"], (8, 8))
    many = {f"s{k}": res["reynolds_stress"] for k in range(3)}
    with pytest.raises(ValueError):
        solver.sample_grid(list(many), (8, 8), extra=many)                      # 18 planes, one call takes 16


@pytest.mark.parametrize("subgrid", [False, True])
def test_vtk_round_trip(subgrid, tmp_path):
    r = run("refined-2d", subgrid, torch.float32)
    dev = r.a.results(["mean_velocity", "tke", "reynolds_stress"])
    infos = [vtk.get_host_statistics_variable(r.a, "mean_velocity"), vtk.get_host_statistics_variable(r.a, "tke")]
    assert (infos[0].type, infos[1].type) == (vtk.VECTOR, vtk.SCALAR)
    assert infos[0].data.shape == (r.cells, 3) and infos[1].data.shape == (r.cells,)
    stress = vtk.get_host_statistics_variable(r.a, "reynolds_stress")
    assert [i.name for i in stress] == stats_mod.plane_names("reynolds_stress") and all(i.type == vtk.SCALAR for i in stress)
    v = read_vtu(vtk.save_variables_to_vtk(r.solver, infos + stress, str(tmp_path / "stats")))
    assert v["n_cells"] == r.cells
    if subgrid:
        S, perm = r.part.cells_per_element, z_order_permutation(r.part.mesh.dim)
        order = (np.arange(r.part.N)[:, None] * S + perm[None, :]).reshape(-1)
    else:
        order = np.arange(r.cells)
    assert np.array_equal(v["arrays"]["mean_velocity"], dev["mean_velocity"].cpu().numpy()[:, order].T)
    assert np.array_equal(v["arrays"]["tke"], dev["tke"].cpu().numpy()[order])
    for k, name in enumerate(stats_mod.plane_names("reynolds_stress")):
        assert np.array_equal(v["arrays"][name], dev["reynolds_stress"][k].cpu().numpy()[order])


def test_kelvin_helmholtz_example_writes_the_statistics(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "kelvin_helmholtz_amr.py"), "--steps", "12", "--adapt-every", "6",
                          "--min-level", "3", "--max-level", "5", "--stats", "--stats-every", "2", "--vtk", str(tmp_path / "kh"),
                          "--image", "16"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "adapt at it 6" in out.stdout
    v = read_vtu(str(tmp_path / "kh.vtu"))
    for name in ("density", "mean_density", "mean_velocity", "tke", "pressure_rms"):
        assert name in v["arrays"], (name, list(v["arrays"]))
    assert v["arrays"]["mean_velocity"].shape == (v["n_cells"], 3)
    assert np.all(v["arrays"]["mean_density"] > 0) and np.all(v["arrays"]["tke"] >= -1e-12) and np.all(v["arrays"]["pressure_rms"] >= 0)
    image = np.load(str(tmp_path / "kh_tke_000012.npy"))
    assert image.shape == (16, 16) and np.all(np.isfinite(image))
