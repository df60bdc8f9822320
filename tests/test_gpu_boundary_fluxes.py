"""-m gpu: boundary budgets (solver.boundary_fluxes*, csrc/hip/kernels_boundary.hip) against the oracle-composed
host reference of tests/_boundary_ref.py -- plain 2D / 3D, Subgrid blocks, the curved shell --, the analytic cases (hydrostatic
box, free stream), the stage budgets with monitor(), determinism and the accumulating form, run-time states, the non-finite
guard, partitions and adapted solvers. A slot's error is normalised by the sum of the absolute values of its terms."""
import numpy as np
import pytest
import torch

from _boundary_ref import boundary_terms, reference_block, slot_error
from _gpu import NP, TOL1, perturbed_state
from test_gpu_farfield import SHELL_SIDES, _curved_state, far_state, far_states
from test_gpu_subgrid_farfield import subgrid_far_state
from t8gpu_amd import amr, boundary, hip
from t8gpu_amd.boundary import BoundaryFluxes
from t8gpu_amd.solver import STEP1, STEP2, PlainSolver, SubgridSolver
from t8gpu_amd.synth import SynthMesh
from t8gpu_amd.unstructured import PrismHexMesh, shell_map

pytestmark = pytest.mark.gpu

KINDS = [hip.KEPES, hip.HLL, hip.HLLC]
# every kind on one mesh: -x inflow state 1, +x outflow, -y (3D: -z) wall, +y (3D: +z) far field against state 0
MIXED = {2: (1, "outflow", "wall", ("farfield", 0)),
         3: (1, "outflow", "periodic", "periodic", "wall", ("farfield", 0))}
C31, C32, C33 = 0.33333333333333, 0.66666666666666, 0.66666666666666       # csrc/hip/flux_math.hpp: rk3c<double>


def plain_mesh(dim, sides=None, **kw):
    sides = MIXED[dim] if sides is None and not kw else sides
    return SynthMesh(2, 4, 7, band=0.12, sides=sides, **kw) if dim == 2 else SynthMesh(3, 3, 5, band=0.12, sides=sides, **kw)


def subgrid_mesh(dim, sides=None, **kw):
    sides = MIXED[dim] if sides is None and not kw else sides
    return SynthMesh(2, 3, 5, band=0.05, sides=sides, **kw) if dim == 2 else SynthMesh(3, 3, 4, band=0.05, sides=sides, **kw)


def make(part, dtype, kind, state, states, mode="compat"):
    if part.subgrid:
        return SubgridSolver(part, dtype, flux_kind=kind, mode=mode, state=state, open_boundaries=True, farfield=True,
                             inflow_states=states)
    return PlainSolver(part, dtype, flux_kind=kind, mode=mode, state=state, inflow_states=states)


def host_state(g, step=None):
    torch.cuda.synchronize()
    return g.state(step).double().cpu().numpy()


def check_against_reference(g, state, states, dtype, tag, tol=None):
    """kind groups and side groups of solver g against the reference on `state`; the sums over the groups of the two agree"""
    part = g.part
    tol = TOL1[dtype] if tol is None else tol
    totals = []
    for groups in (None, "side"):
        _, labels, count = boundary.resolve_groups(part, groups)
        want, scale = reference_block(part, NP[dtype], g.kind, state, states, labels, count)
        got = g.boundary_fluxes(groups=groups)
        assert got.block.shape == (count, 16)
        err = slot_error(got.block, want, scale)
        print(f"{tag} groups={groups}: slot error {err:.2e}")
        assert err < tol, (groups, err)
        assert np.array_equal(got.block[:, 11:13], want[:, 11:13]) and np.all(got.block[:, 13:] == 0)
        assert np.array_equal(got.faces, want[:, 11].astype(np.int64)) and not got.nonfinite.any()
        totals.append((got.total().block[0], scale.sum(0)))
    (a, sa), (b, _) = totals
    assert float((np.abs(a - b)[:11] / np.where(sa[:11] > 0, sa[:11], 1.0)).max()) < tol
    assert a[11] == b[11] > 0


# ---- 1, 2: against the oracle-composed reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_plain_follows_the_reference(dim, kind, dtype):
    part = plain_mesh(dim).partition()
    kinds = np.asarray(part.boundary_kinds)
    assert set(np.unique(kinds)) == {0, 1, 3, 10}
    assert dim == 2 or np.bincount(kinds).max() > 512               # 3D: groups of several 256-face chunks, the last not full
    st, states = far_state(part, 31), far_states()
    g = make(part, dtype, kind, st, states)
    check_against_reference(g, st, states, dtype, f"plain {dim}D kind {kind} {dtype}")


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_subgrid_follows_the_reference(dim, kind, dtype):
    part = subgrid_mesh(dim).partition(subgrid=True)
    kinds = np.asarray(part.boundary_kinds)
    assert set(np.unique(kinds)) == {0, 1, 3, 10}
    assert dim == 2 or np.bincount(kinds).max() > 32                # 3D: groups of several 16-face chunks
    st, states = subgrid_far_state(part, 32), far_states()
    g = make(part, dtype, kind, st, states)
    check_against_reference(g, st, states, dtype, f"subgrid {dim}D kind {kind} {dtype}")


# ---- 3: curved shell --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_curved_shell_by_side(dtype):
    mesh = PrismHexMesh((8, 8, 4), split="checker", mapping=shell_map, sides=SHELL_SIDES)
    part = mesh.partition()
    st, states = _curved_state(part, 33), far_states()
    g = PlainSolver(part, dtype, flux_kind=hip.KEPES, mode="fused", state=st, inflow_states=states)
    check_against_reference(g, st, states, dtype, f"shell {dtype}")
    got = g.boundary_fluxes(groups="side")
    side = boundary.side_groups(part)
    areas = np.asarray(part.areas)[part.F:].astype(NP[dtype]).astype(np.float64)
    kinds = np.asarray(part.boundary_kinds)
    assert np.all(kinds[side == 0] == 0) and np.all(kinds[side == 1] == 10)               # inner wall, outer far field
    for s in (0, 1):
        want = areas[side == s].sum()
        assert abs(got.area[s] - want) <= 1e-13 * want and got.faces[s] == (side == s).sum()
    assert got.area[1] > got.area[0] > 0


# ---- 4: hydrostatic box -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("subgrid", [False, True])
def test_hydrostatic_box(dim, kind, subgrid):
    p0 = 1.7
    mesh = (subgrid_mesh if subgrid else plain_mesh)(dim, periodic=False)
    part = mesh.partition(subgrid=subgrid)
    cells = (part.N + part.G) * (4 ** dim if subgrid else 1)
    st = np.repeat(np.array([1.3, 0.0, 0.0, 0.0, p0 / 0.4]).reshape(5, 1), cells, axis=1)
    if subgrid:
        g = SubgridSolver(part, torch.float64, flux_kind=kind, state=st)
    else:
        g = PlainSolver(part, torch.float64, flux_kind=kind, state=st)
    got = g.boundary_fluxes(groups="side")
    assert got.block.shape == (2 * dim, 16)
    for s in range(2 * dim):
        n = np.zeros(3)
        n[s // 2] = 1.0 if s % 2 else -1.0
        assert abs(got.area[s] - 1.0) < 1e-13                                             # a side of the unit square / cube
        assert got.mass_flow[s] == 0.0 and got.energy_flow[s] == 0.0 and got.mass_out[s] == 0.0
        assert np.abs(got.momentum_flux[s] - p0 * n).max() < 1e-12 * p0
        assert np.abs(got.pressure_force[s] - p0 * n).max() < 1e-12 * p0
        assert abs(got.mean_pressure[s] - p0) < 1e-12 * p0
    by_kind = g.boundary_fluxes()
    assert by_kind.faces[0] == got.faces.sum() and not by_kind.faces[1:].any()


# ---- 5: free stream ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("subgrid", [False, True])
def test_free_stream_gives_the_analytic_euler_flux(dim, kind, subgrid):
    states = far_states()
    w = states[1]                                                                         # moving: rho 1.2, v (.4, .1, .05), p 1.1
    if dim == 2:
        states[1, 3] = 0.0
        states[1, 4] = 1.1 / 0.4 + 0.5 * (w[1] ** 2 + w[2] ** 2) / w[0]
    sides = (1, ("farfield", 1), "outflow", ("farfield", 1)) + ((1, "outflow") if dim == 3 else ())
    mesh = (subgrid_mesh if subgrid else plain_mesh)(dim, sides)
    part = mesh.partition(subgrid=subgrid)
    cells = (part.N + part.G) * (4 ** dim if subgrid else 1)
    g = make(part, torch.float64, kind, np.repeat(w.reshape(5, 1), cells, axis=1), states)
    got = g.boundary_fluxes(groups="side")
    rho, v, E = w[0], w[1:4] / w[0], w[4]
    p = 0.4 * (E - 0.5 * rho * (v * v).sum())
    for s in range(2 * dim):
        n = np.zeros(3)
        n[s // 2] = 1.0 if s % 2 else -1.0
        un = float(v @ n)
        want = np.concatenate([[rho * un], rho * un * v + p * n, [(E + p) * un]])         # A = 1
        assert np.abs(got.flux[s] - want).max() < 1e-12 * np.abs(want).max(), (s, got.flux[s], want)
        assert abs(got.mass_out[s] - max(rho * un, 0.0)) < 1e-12 and abs(got.mass_in[s] - max(-rho * un, 0.0)) < 1e-12


# ---- 6: stage budgets close -------------------------------------------------------------------------------------------------
def _abs_flux(g, step, states):
    """sum over the boundary faces of |A g_k| of state(step), from the host reference"""
    _, A, flux, _, _ = boundary_terms(g.part, np.float64, g.kind, host_state(g, step), states)
    return np.abs(A[:, None] * flux).sum(0)


@pytest.mark.parametrize("mode", ["compat", "fused"])
@pytest.mark.parametrize("case", ["plain2", "plain3", "subgrid2", "subgrid3"])
def test_stage_budgets_close(case, mode):
    dim, subgrid = int(case[-1]), case.startswith("subgrid")
    part = (subgrid_mesh if subgrid else plain_mesh)(dim).partition(subgrid=subgrid)
    st, states = perturbed_state(part, 34), far_states()
    g = make(part, torch.float64, hip.KEPES, st, states, mode)
    dt = g.cfl_timestep(0.5)
    # where the 1e-8 comes from: the integrals carry at most 1e-12 relative rounding (the monitor sums at most 2^18 cells one
    # per lane and then by a tree of depth 18: 18 * 2^-53 = 2e-15 of the sum of |terms|, far inside that allowance), and dt >=
    # 1e-3 with O(1) open area puts dt sum |A g| at >= 1e-4 of them even with the stage coefficient 1/4: 1e-8 at the worst
    assert g.owned_cells <= 2 ** 18
    assert dt >= 1e-3
    open_area = np.asarray(part.areas)[part.F:][np.asarray(part.boundary_kinds) != 0].sum()
    assert open_area >= 1.0
    vol = np.repeat(np.asarray(part.volumes)[:part.N], g.owned_cells // part.N) / (g.owned_cells // part.N)
    abs_integrals = (vol[None, :] * np.abs(st[:, :g.owned_cells])).sum(1)
    g.iterate(dt)
    src = (g.prev, STEP1, STEP2)
    I = [g.monitor(s).integrals.copy() for s in src + (g.next,)]
    B = [g.boundary_fluxes(s).total().flux[0].copy() for s in src]
    norm = [dt * _abs_flux(g, s, states) for s in src]
    res = [I[1] - (I[0] - dt * B[0]),
           I[2] - (0.75 * I[0] + 0.25 * I[1] - 0.25 * dt * B[1]),
           I[3] - (C31 * I[0] + C32 * I[2] - C33 * dt * B[2])]
    coef = (1.0, 0.25, C33)
    for k in range(3):
        assert np.all(dt * np.abs(B[k])[[0, 4]] > 0)                                      # mass and energy do cross the boundary
        assert np.all(1e-12 * abs_integrals <= 1e-8 * coef[k] * norm[k])                  # the allowance sits under the bound
        r = np.abs(res[k]) / np.where(norm[k] > 0, coef[k] * norm[k], 1.0)
        print(f"{case} {mode} stage {k + 1}: residual / (dt sum |A g|) = {r.tolist()}")
        assert np.all(np.abs(res[k])[norm[k] == 0] == 0.0)
        assert r.max() <= 1e-8, (k, r)
        dropped = np.abs(res[k] - coef[k] * dt * B[k]) / np.where(norm[k] > 0, coef[k] * norm[k], 1.0)
        assert dropped.max() > 1e-3                                                        # without B the budget is open
    step = g.boundary_step_fluxes(dt)
    total = step.total().flux[0]
    w = boundary.step_weights(torch.float64, dt)
    nstep = sum(wk * nk / dt for wk, nk in zip(w, norm))
    r = np.abs((I[0] - I[3]) - total) / np.where(nstep > 0, nstep, 1.0)
    print(f"{case} {mode} step: |I0 - I3 - flux| / (sum w |A g|) = {r.tolist()}")
    assert r.max() <= 1e-8, r
    want = sum(wk * bk for wk, bk in zip(w, B))
    assert np.abs(total - want).max() <= 1e-12 * nstep.max()


@pytest.mark.parametrize("case", ["plain2", "plain3", "subgrid2", "subgrid3"])
def test_step_fluxes_after_the_native_driver_equal_those_after_python_stages(case):
    dim, subgrid = int(case[-1]), case.startswith("subgrid")
    part = (subgrid_mesh if subgrid else plain_mesh)(dim).partition(subgrid=subgrid)
    st, states = perturbed_state(part, 35), far_states()
    py, nat = (make(part, torch.float64, hip.KEPES, st, states, "fused") for _ in range(2))
    nat.use_native_stepper()
    dt = py.cfl_timestep(0.5)
    for _ in range(3):
        py.iterate(dt)
    nat.iterate_steps(3, dt)
    a, b = py.boundary_step_fluxes(dt), nat.boundary_step_fluxes(dt)
    assert a.faces.sum() > 0 and np.abs(a.flux).max() > 0
    assert np.array_equal(a.block, b.block)


# ---- 7: determinism and the accumulating form -------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_two_calls_give_equal_bits_and_the_accumulating_form_adds_weighted_blocks(subgrid, dtype):
    part = (subgrid_mesh if subgrid else plain_mesh)(2).partition(subgrid=subgrid)
    st, states = perturbed_state(part, 36), far_states()
    g = make(part, dtype, hip.HLLC, st, states)
    g.iterate(1e-3)
    b1 = g.boundary_fluxes_device(g.prev, "side").clone()
    b1_again = g.boundary_fluxes_device(g.prev, "side").clone()
    b2 = g.boundary_fluxes_device(g.next, "side").clone()
    assert torch.equal(b1, b1_again) and not torch.equal(b1, b2)
    w1, w2 = 0.37, -1.9
    out = torch.zeros_like(b1)
    assert g.boundary_fluxes_device(g.prev, "side", out=out, weight=w1) is out
    g.boundary_fluxes_device(g.next, "side", out=out, weight=w2)
    torch.cuda.synchronize()
    got, h1, h2 = out.cpu().numpy(), b1.cpu().numpy(), b2.cpu().numpy()
    want = w1 * h1 + w2 * h2
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    assert np.all(np.abs(got - want)[:, :11] <= 4 * ulp[:, :11])
    assert np.array_equal(got[:, 11:13], h2[:, 11:13]) and np.all(got[:, 13:] == 0)       # counts: those of the last call
    # `out` alone overwrites; weight alone is refused
    plain_out = torch.full_like(b1, 7.0)
    g.boundary_fluxes_device(g.prev, "side", out=plain_out)
    assert torch.equal(plain_out, b1)
    with pytest.raises(ValueError):
        g.boundary_fluxes_device(g.prev, "side", weight=1.0)
    with pytest.raises(ValueError):
        g.boundary_fluxes_device(g.prev, "side", out=torch.zeros((3, 16), dtype=torch.float64, device="cuda"), weight=1.0)
    with pytest.raises(ValueError):
        g.boundary_fluxes(groups=np.zeros(part.B, np.int32))
    # caller-supplied labels: the face index modulo 5 (32 groups, 27 of them empty), against the reference
    labels = (np.arange(part.B) % 5).astype(np.uint8)
    want5, scale5 = reference_block(part, NP[dtype], g.kind, host_state(g), states, labels, 32)
    got5 = g.boundary_fluxes(groups=labels)
    assert got5.block.shape == (32, 16) and slot_error(got5.block, want5, scale5) < TOL1[dtype]
    assert not got5.block[5:].any() and len(g._boundary_cache) == 2


# ---- 8: run-time states -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_set_inflow_states_is_followed_without_a_rebuild(subgrid, dtype):
    part = (subgrid_mesh if subgrid else plain_mesh)(2).partition(subgrid=subgrid)
    st = subgrid_far_state(part, 37) if subgrid else far_state(part, 37)
    states = far_states()
    g = make(part, dtype, hip.HLL, st, states)
    before = g.boundary_fluxes().block
    entry = g._boundary_cache["kind"]
    new = states.copy()
    new[0] = [0.9, 0.09, -0.18, 0.0, 0.8 / 0.4 + 0.5 * 0.9 * (0.1 ** 2 + 0.2 ** 2)]
    new[1] = [1.5, 0.9, 0.3, 0.0, 1.4 / 0.4 + 0.5 * 1.5 * (0.6 ** 2 + 0.2 ** 2)]
    g.set_inflow_states(new)
    after = g.boundary_fluxes().block
    assert g._boundary_cache["kind"] is entry
    want, scale = reference_block(part, NP[dtype], g.kind, st, new, boundary.kind_groups(part), 16)
    assert slot_error(after, want, scale) < TOL1[dtype]
    for k in (0, 1):                                                                       # walls and outflow: the same bits
        assert before[k, 11] > 0 and np.array_equal(after[k], before[k])
    for k in (3, 10):                                                                      # inflow 1, far field 0: they moved
        assert not np.array_equal(after[k, 1:6], before[k, 1:6])


# ---- 9: non-finite guard ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("kind_code", [1, 10])
def test_a_nan_cell_is_counted_and_kept_out_of_the_sums(subgrid, kind_code):
    part = (subgrid_mesh if subgrid else plain_mesh)(2).partition(subgrid=subgrid)
    st, states = perturbed_state(part, 38), far_states()
    clean = make(part, torch.float64, hip.KEPES, st, states).boundary_fluxes().block
    face, _, _, _, _ = boundary_terms(part, np.float64, 0, st, states)
    kinds = np.asarray(part.boundary_kinds).astype(np.int64)
    fn = np.asarray(part.face_neighbors)[2 * part.F:]
    if subgrid:
        from test_subgrid_open_boundaries_host import boundary_subcells
        cells = np.concatenate([boundary_subcells(part, b) for b in range(part.B)])
    else:
        cells = fn.astype(np.int64)
    term_kind = kinds[face]
    # a cell on the chosen side all of whose boundary (sub-)faces are of that kind
    mixed = set(cells[term_kind != kind_code].tolist())
    cell = next(int(c) for c in cells[term_kind == kind_code] if int(c) not in mixed)
    count = int((cells == cell).sum())
    bad = st.copy()
    bad[0, cell] = np.nan
    got = make(part, torch.float64, hip.KEPES, bad, states).boundary_fluxes()
    assert got.nonfinite[kind_code] == count >= 1 and got.nonfinite.sum() == count
    for k in range(16):
        if k != kind_code:
            assert np.array_equal(got.block[k], clean[k])
    row = got.block[kind_code]
    assert np.isfinite(row).all() and row[0] == clean[kind_code, 0] and row[11] == clean[kind_code, 11]
    assert not np.array_equal(row[1:11], clean[kind_code, 1:11])


# ---- 10: partitions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_combined_ranks_equal_the_single_rank(dtype):
    mesh = plain_mesh(2)
    whole = mesh.partition()
    st, states = far_state(whole, 39), far_states()
    single = make(whole, dtype, hip.KEPES, st, states)
    for groups in (None, "side"):
        _, labels, count = boundary.resolve_groups(whole, groups)
        _, scale = reference_block(whole, NP[dtype], hip.KEPES, st, states, labels, count)
        blocks = []
        for r in range(3):
            part = mesh.partition(r, 3)
            gidx = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
            blocks.append(make(part, dtype, hip.KEPES, st[:, gidx], states).boundary_fluxes(groups=groups))
            assert blocks[-1].faces.sum() == part.B
        both = BoundaryFluxes.combine(blocks)
        want = single.boundary_fluxes(groups=groups).block
        assert slot_error(both.block, want, scale) < TOL1[dtype]
        assert np.array_equal(both.block[:, 11:13], want[:, 11:13])


def test_no_boundary_faces_give_zeros():
    periodic = SynthMesh(2, 3, 5, band=0.1).partition()
    assert periodic.B == 0
    g = PlainSolver(periodic, torch.float64, state=perturbed_state(periodic, 40))
    for groups in (None, "side", np.zeros(0, np.uint8)):
        assert not g.boundary_fluxes(groups=groups).block.any()
    g.iterate(1e-3)
    assert not g.boundary_step_fluxes(1e-3).block.any()
    sg = SynthMesh(2, 2, 3).partition(subgrid=True)
    assert not SubgridSolver(sg, torch.float32).boundary_fluxes(groups="side").block.any()
    # a rank of an open mesh that owns no boundary face
    mesh = SynthMesh(2, 3, 3, sides=("outflow", "outflow", "wall", ("farfield", 0)))
    inner = [p for p in (mesh.partition(r, 16) for r in range(16)) if p.B == 0]
    assert inner
    part = inner[0]
    st = perturbed_state(mesh.partition(), 41)
    gidx = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
    r = PlainSolver(part, torch.float64, state=st[:, gidx], inflow_states=far_states())
    assert not r.boundary_fluxes().block.any() and r.boundary_fluxes(groups="side").block.shape == (4, 16)


# ---- 11: after adapt --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
def test_a_solver_from_adapt_works_from_its_first_call(subgrid):
    states = far_states()
    if subgrid:
        part = SynthMesh(2, 3, 5, band=0.05, sides=MIXED[2]).partition(subgrid=True)
        g = make(part, torch.float64, hip.KEPES, subgrid_far_state(part, 42), states, "fused")
    else:
        part = SynthMesh(2, 4, 6, band=0.03, sides=MIXED[2]).partition()
        g = make(part, torch.float64, hip.KEPES, far_state(part, 42), states, "fused")
    before = g.boundary_fluxes(groups="side")
    dt = 0.25 * g.cfl_timestep(0.5)
    for _ in range(3):
        g.iterate(dt)
    if subgrid:
        new, marks, _ = amr.adapt_subgrid(g, threshold=0.02, min_level=3, max_level=5)
    else:
        new, marks, _ = amr.adapt(g, threshold=10.0, min_level=3, max_level=7)
    assert np.any(marks != 0) and new is not g and new.N != g.N
    after = new.boundary_fluxes(groups="side")
    assert np.abs(after.area - before.area).max() < 1e-13 and np.all(after.area > 0.99)
    check_against_reference(new, host_state(new), states, torch.float64, f"adapted subgrid={subgrid}")
