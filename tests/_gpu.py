"""Helpers shared by the -m gpu parity tests: everything on the device goes through the C-ABI."""
import numpy as np
import torch

# Parity tolerances: max error normalised by max|u| per variable.
TOL1 = {torch.float64: 1e-12, torch.float32: 2e-5}     # after 1 step / one kernel
TOL10 = {torch.float64: 1e-10, torch.float32: 2e-4}    # after 10 steps
NP = {torch.float64: np.float64, torch.float32: np.float32}


def rel_err(got, want):
    """max_k max_i |got - want| / max_i |want| over the 5 variables (rows)."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    scale = np.maximum(np.abs(want).max(axis=1, keepdims=True), 1e-300)
    return float((np.abs(got - want) / scale).max())


def perturbed_state(part, seed, cells=1):
    """KH state plus a smooth random perturbation so that no flux component is identically zero."""
    u = part.kh_initial_state().copy()
    rng = np.random.default_rng(seed)
    n = u.shape[1]
    rho = u[0] * (1 + 0.05 * rng.standard_normal(n))
    v = np.stack([u[1] / u[0], u[2] / u[0], u[3] / u[0]]) + 0.2 * rng.standard_normal((3, n))
    p = 1.0 + 0.1 * rng.uniform(-1, 1, n)
    E = p / 0.4 + 0.5 * rho * (v ** 2).sum(0)
    return np.stack([rho, rho * v[0], rho * v[1], rho * v[2], E])


def subgrid_boundary_notes():
    """(MODE, dim, noted kernel) of one step on the test-sized open (MODE 1) and far-field (MODE 2) Subgrid meshes, 3D and 2D,
    along the launch path of this process; the MODE is the one the solver's plan calls for, which must be the mesh's"""
    import ctypes
    import test_gpu_subgrid_farfield as far
    import test_gpu_subgrid_open_boundaries as opn
    from t8gpu_amd import hip
    from t8gpu_amd.solver import SubgridSolver
    q = hip.lib().t8gpu_hip_last_stage_kernel
    q.restype = ctypes.c_char_p
    out = []
    for dim in (3, 2):
        for want, mesh, kw in ((1, opn.mesh_of(dim), dict(inflow_states=opn.inflow_states(dim))),
                               (2, far.mesh_of(dim, far.SIDES[dim]), dict(farfield=True, inflow_states=far.far_states()))):
            g = SubgridSolver(mesh.partition(subgrid=True), torch.float64, mode="fused", open_boundaries=True, **kw)
            mode = 0 if not g.plan.c.has_open_faces else (2 if g.plan.c.has_farfield_faces else 1)
            assert mode == want and g.plan.host.n_families > 0
            g.iterate(opn.dt_of(mesh))
            torch.cuda.synchronize()
            out.append((mode, dim, q().decode()))
    return out
