"""-m gpu: open boundaries (outflow, prescribed-state inflow) through every plain kernel tier, against a CPU reference
composed from the oracle's existing entry points: its interior-face and wall-face loops on arrays that hold only the interior
and wall faces, its xyz face flux for the open faces (outside state = inside state, or the inflow state; no mirror), and its
RK stage."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _oracle as O
from _gpu import NP, TOL1, TOL10, perturbed_state, rel_err
from t8gpu_amd import amr, hip
from t8gpu_amd.solver import PlainSolver, SubgridSolver
from t8gpu_amd.synth import SynthMesh

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS = [hip.KEPES, hip.HLL, hip.HLLC]
SIDES = {2: (0, "outflow", "periodic", "periodic"),                                  # x: inflow / outflow, y periodic
         3: (0, "outflow", "periodic", "periodic", "wall", "wall")}                  # ... z walls


def inflow_states(dim):
    rho, v, p = 1.2, (0.4, 0.1, 0.05 if dim == 3 else 0.0), 1.1
    return np.array([[rho, rho * v[0], rho * v[1], rho * v[2], p / 0.4 + 0.5 * rho * sum(c * c for c in v)]])


def mesh_of(dim, sides=None):
    sides = SIDES[dim] if sides is None else sides
    return SynthMesh(2, 4, 7, band=0.12, sides=sides) if dim == 2 else SynthMesh(3, 3, 5, band=0.12, sides=sides)


def _frame(n):
    """an orthonormal face frame (n, t1, t2) per face: the speed estimates do not depend on the tangent directions"""
    n = np.asarray(n, np.float64)
    a = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    t1 = a - (a * n).sum(1, keepdims=True) * n
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    return n, t1, np.cross(n, t1)


def _to_frame(n, t1, t2, s):
    m = s[:, 1:4]
    return np.stack([s[:, 0], (m * n).sum(1), (m * t1).sum(1), (m * t2).sum(1), s[:, 4]], 1)


class OpenCase(O.PlainCase):
    """O.PlainCase with open boundary faces: per stage the oracle's interior loop, its wall loop on the wall faces alone,
    the open faces from oracle_xyz_face_flux (times the area), and its RK stage."""

    def __init__(self, part, dtype, state, inflow):
        super().__init__(part, dtype, state=state)
        kinds = np.asarray(part.boundary_kinds)
        F, nd = part.F, part.normal_dim
        fn = np.asarray(part.face_neighbors)
        wall = kinds == 0
        nr = np.asarray(part.normals).reshape(-1, nd)
        self.Bw = int(wall.sum())
        self.fn_w = np.ascontiguousarray(np.concatenate([fn[:2 * F], fn[2 * F:][wall]]).astype(np.int32))
        self.normals_w = np.ascontiguousarray(np.concatenate([nr[:F], nr[F:][wall]]).reshape(-1).astype(dtype))
        self.areas_w = np.ascontiguousarray(np.concatenate([part.areas[:F], part.areas[F:][wall]]).astype(dtype))
        self.wall_ids = F + np.flatnonzero(wall)
        op = np.flatnonzero(~wall)
        self.open_ids = F + op
        self.open_e = fn[2 * F:][op].astype(np.int64)
        n3 = np.zeros((op.size, 3))
        n3[:, :nd] = nr[F:][op]
        self.open_n3 = np.ascontiguousarray(n3.astype(dtype))
        self.open_area = np.asarray(part.areas)[F:][op].astype(dtype)
        self.open_kind = kinds[op].astype(np.int64)
        self.inflow = None if inflow is None else np.asarray(inflow, np.float64).astype(dtype)

    def _outside(self, sL):
        sR = sL.copy()
        inf = self.open_kind >= 2
        if inf.any():
            sR[inf] = self.inflow[self.open_kind[inf] - 2]
        return sR

    def iterate(self, dt, kind=0, omp=False):
        self.next, self.prev = self.prev, self.next
        P, T = self.part, self.dtype
        sf = O.suf(T)
        lib = O.lib()
        vol = self.planes[25]
        src, dst = (self.prev, 1, 2), (1, 2, self.next)
        for s in range(3):
            st = self.planes[5 * src[s]:5 * src[s] + 5]
            fl = self.planes[20:25]
            fl[:] = 0
            getattr(lib, "oracle_plain_interior_faces_" + sf)(kind, P.F, P.normal_dim, O.p(self.fn), None, O.p(self.normals),
                                                               O.p(self.areas), O.p(st), O.p(fl), C.c_size_t(self.stride),
                                                               O.p(self.speed))
            if self.Bw:
                sp = np.zeros(P.F + self.Bw, T)
                getattr(lib, "oracle_plain_boundary_faces_" + sf)(kind, P.F, self.Bw, P.normal_dim, O.p(self.fn_w),
                                                                   O.p(self.normals_w), O.p(self.areas_w), O.p(st), O.p(fl),
                                                                   C.c_size_t(self.stride), O.p(sp))
                self.speed[self.wall_ids] = sp[P.F:]
            if self.open_e.size:
                sL = np.ascontiguousarray(st[:, self.open_e].T)
                sR = self._outside(sL)
                g = O.xyz_face_flux(kind, self.open_n3, sL, sR) * self.open_area[:, None]
                for k in range(5):
                    np.subtract.at(fl[k], self.open_e, g[:, k])
                n, t1, t2 = _frame(self.open_n3.astype(np.float64))
                _, spd = O.face_frame_flux(kind, _to_frame(n, t1, t2, sL.astype(np.float64)).astype(T),
                                           _to_frame(n, t1, t2, sR.astype(np.float64)).astype(T), want_speed=True)
                self.speed[self.open_ids] = spd
            pv, md, ot = (self.planes[5 * x:5 * x + 5] for x in (self.prev, src[s], dst[s]))
            getattr(lib, "oracle_plain_rk_stage_" + sf)(s + 1, P.N, O.p(pv), O.p(md), O.p(ot), O.p(fl), C.c_size_t(self.stride),
                                                         O.p(vol), O.fs(T, dt))


TIERS = {"compat": dict(mode="compat"),
         "patches": dict(mode="fused"),                                               # mixed k_plain_stage / patch + tiles
         "one_tile": dict(mode="fused", plan_options=dict(patches=False)),            # k_plain_fused_p
         "generic": dict(mode="fused", plan_options=dict(compressed=False))}          # k_plain_fused (CSR lists)


def _solver(part, dtype, kind, tier, state, inflow):
    return PlainSolver(part, dtype, flux_kind=kind, state=state, inflow_states=inflow, **TIERS[tier])


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("tier", list(TIERS))
def test_every_tier_follows_the_oracle_composed_reference(dim, kind, dtype, tier):
    mesh = mesh_of(dim)
    part = mesh.partition()
    st = perturbed_state(part, 11)
    inflow = inflow_states(dim)
    g = _solver(part, dtype, kind, tier, st, inflow)
    if tier == "patches":
        assert g.plan.host.n_patches > 0 and g.plan.c.has_open_faces
    o = OpenCase(part, NP[dtype], st, inflow)
    dt = 0.1 * 2.0 ** -mesh.finest_level
    g.iterate(dt)
    o.iterate(dt, kind)
    torch.cuda.synchronize()
    assert rel_err(g.state().cpu().numpy(), o.current()[:, :part.N]) < TOL1[dtype]
    spd = g.speed[:part.F + part.B].cpu().numpy()
    bnd = np.arange(part.F, part.F + part.B)
    assert np.abs(spd[bnd] - o.speed[bnd]).max() / np.abs(o.speed[bnd]).max() < TOL1[dtype]   # walls and open faces
    assert np.abs(spd - o.speed).max() / np.abs(o.speed).max() < TOL1[dtype]
    for _ in range(9):
        g.iterate(dt)
        o.iterate(dt, kind)
    torch.cuda.synchronize()
    assert rel_err(g.state().cpu().numpy(), o.current()[:, :part.N]) < TOL10[dtype]


_TIER_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from test_gpu_open_boundaries import mesh_of, inflow_states, perturbed_state
from t8gpu_amd.solver import PlainSolver
out = []
for dim in (2, 3):
    mesh = mesh_of(dim)
    part = mesh.partition()
    g = PlainSolver(part, torch.float64, mode="fused", state=perturbed_state(part, 11), inflow_states=inflow_states(dim),
                    plan_options=dict(patches=False))
    for _ in range(3):
        g.iterate(0.1 * 2.0 ** -mesh.finest_level)
    torch.cuda.synchronize()
    out += [g.state().cpu().numpy().ravel(), g.speed.cpu().numpy()]
np.save(sys.argv[1], np.concatenate(out))
"""


def test_persistent_switch_gives_the_same_bits(tmp_path):
    """T8GPU_PERSISTENT=2 / 0 in child processes: the persistent kernel refuses plans with open faces (its launches run the
    one-tile kernels), so both give the same bits."""
    script = tmp_path / "child.py"
    script.write_text(_TIER_CHILD.format(root=ROOT, tests=HERE))
    res = []
    for mode in ("2", "0"):
        out = tmp_path / f"r{mode}.npy"
        subprocess.run([sys.executable, str(script), str(out)], env=dict(os.environ, T8GPU_PERSISTENT=mode, T8GPU_PERSISTENT_WGS="3"),
                       check=True, timeout=600)
        res.append(np.load(out))
    assert np.isfinite(res[0]).all() and np.array_equal(res[0], res[1])


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_patches_on_and_off_give_the_same_bits(dim, dtype):
    part = mesh_of(dim).partition()
    st, inflow = perturbed_state(part, 12), inflow_states(dim)
    a = _solver(part, dtype, hip.KEPES, "patches", st, inflow)
    b = _solver(part, dtype, hip.KEPES, "one_tile", st, inflow)
    assert a.plan.host.n_patches > 0 and b.plan.host.n_patches == 0
    dt = 0.1 * 2.0 ** -part.mesh.finest_level
    for _ in range(3):
        a.iterate(dt)
        b.iterate(dt)
    torch.cuda.synchronize()
    assert torch.equal(a.state(), b.state()) and torch.equal(a.speed, b.speed)


def _uniform(part, w):
    return np.repeat(np.asarray(w, np.float64).reshape(5, 1), part.N + part.G, axis=1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("tier", list(TIERS))
def test_inflow_of_the_cell_state_equals_outflow_bitwise(kind, dtype, tier):
    """From a uniform state, an inflow face whose state is that state gives the bits of an outflow face: the inflow table's
    KEPES record comes from the routine the tiles run for their cells."""
    w = inflow_states(2)
    a_part = mesh_of(2, (0, "outflow", "periodic", "periodic")).partition()
    b_part = mesh_of(2, ("outflow", "outflow", "periodic", "periodic")).partition()
    a = _solver(a_part, dtype, kind, tier, _uniform(a_part, w[0]), w)
    b = _solver(b_part, dtype, kind, tier, _uniform(b_part, w[0]), None)
    dt = 0.1 * 2.0 ** -a_part.mesh.finest_level
    a.iterate(dt)
    b.iterate(dt)
    torch.cuda.synchronize()
    assert torch.equal(a.state(), b.state())


@pytest.mark.parametrize("dim", [2, 3])
def test_native_driver_equals_python_stages_and_graph_replay_equals_direct(dim):
    part = mesh_of(dim).partition()
    st, inflow = perturbed_state(part, 13), inflow_states(dim)
    make = lambda: _solver(part, torch.float64, hip.KEPES, "patches", st, inflow)   # noqa: E731
    py, nat, gr = make(), make(), make()
    nat.use_native_stepper()
    gr.use_native_stepper()
    gr.stepper.graph(True)
    dt = 0.1 * 2.0 ** -part.mesh.finest_level
    for n in (5, 2, 5):
        for _ in range(n):
            py.iterate(dt)
        nat.iterate_steps(n, dt)
        gr.iterate_steps(n, dt)
    torch.cuda.synchronize()
    assert gr.stepper.graph()[1] == 3
    assert torch.equal(py.state(), nat.state())
    assert torch.equal(nat.state(), gr.state())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("ghost_window", [False, True])
def test_three_way_loopback_partition_equals_single_rank(dtype, ghost_window):
    """All three ranks on one GPU, the exchange a loopback copy (test_gpu_halo.py); with ghost_window the ghost-reading tiles
    read the receive buffer and fill the send buffer themselves. Boundary faces never touch ghosts: bitwise the one-rank run."""
    from t8gpu_amd import fused
    from t8gpu_amd.halo import HaloExchange
    from test_gpu_halo import loopback, send_map_of
    mesh = SynthMesh(2, 4, 8, band=0.08, sides=SIDES[2])
    whole = mesh.partition()
    st, inflow = perturbed_state(whole, 14), inflow_states(2)
    ref = PlainSolver(whole, dtype, mode="fused", state=st, inflow_states=inflow)
    solvers, halos, windows, keep = [], [], [], []
    for r in range(3):
        part = mesh.partition(r, 3)
        gidx = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
        local = st[:, gidx].copy()
        local[:, part.N:] = np.nan
        s = PlainSolver(part, dtype, mode="fused", state=local, inflow_states=inflow)
        h = HaloExchange(part, dtype, dist=None, overlap=False)
        assert 0 < s.plan.host.n_interior < s.plan.host.ntiles
        w = fused.T8gpuPlainPlan()
        C.pointer(w)[0] = s.plan.c
        if ghost_window:
            smap, slist = send_map_of(part.send_idx, part.N)
            dm, dl = torch.from_numpy(smap).cuda(), torch.from_numpy(slist).cuda()
            w.ghost_buf, w.send_map, w.send_list, w.send_buf, w.n_owned = (h.recvbuf.data_ptr(), dm.data_ptr(), dl.data_ptr(),
                                                                          h.sendbuf.data_ptr(), part.N)
            keep.append((dm, dl))
        solvers.append(s)
        halos.append(h)
        windows.append(w)
    assert sum(int(s.plan.c.has_open_faces) for s in solvers) >= 2
    dt = 0.1 * 2.0 ** -mesh.finest_level
    for step in range(3):
        ref.iterate(dt)
        for s in solvers:
            s.begin_step()
        for k in range(3):
            if not ghost_window or (step == 0 and k == 0):
                for s, h in zip(solvers, halos):
                    h._pack(s.step_planes(s.stage_steps(k)[0]))
            loopback(halos)
            if not ghost_window:
                for s, h in zip(solvers, halos):
                    h._unpack(s.step_planes(s.stage_steps(k)[0]))
            torch.cuda.synchronize()
            for s, w in zip(solvers, windows):
                src, dst = s.stage_steps(k)
                ni, nt = s.plan.host.n_interior, s.plan.host.ntiles
                args = (s.get_own_variables(s.prev), s.get_own_variables(src), s.get_own_variables(dst), hip.ptr(s.planes[25]),
                        hip.fscalar(dtype, dt), hip.ptr(s.speed) if k == 2 else None, hip.stream_ptr())
                hip.call("t8gpu_hip_plain_fused_stage", dtype, s.kind, k + 1, C.byref(s.plan.c), 0, ni, *args)
                hip.call("t8gpu_hip_plain_fused_stage", dtype, s.kind, k + 1, C.byref(w), ni, nt - ni, *args)
            torch.cuda.synchronize()
    full = torch.cat([s.state() for s in solvers], dim=1).cpu().numpy()
    assert not np.isnan(full).any()
    assert np.array_equal(full, ref.state().cpu().numpy())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("amr_mesh", [False, True])
@pytest.mark.parametrize("tier", ["compat", "patches"])
def test_free_stream_stays_uniform(dtype, amr_mesh, tier):
    """A uniform moving state with inflow = that state on -x and outflow elsewhere stays uniform for 50 steps."""
    sides = (0, "outflow", "outflow", "outflow")
    mesh = SynthMesh(2, 4, 7, band=0.12, sides=sides) if amr_mesh else SynthMesh(2, 6, 6, sides=sides)
    part = mesh.partition()
    w = inflow_states(2)
    g = _solver(part, dtype, hip.KEPES, tier, _uniform(part, w[0]), w)
    dt = 0.2 * 2.0 ** -mesh.finest_level
    for _ in range(50):
        g.iterate(dt)
    torch.cuda.synchronize()
    got = g.state().double().cpu().numpy()
    want = np.asarray(w[0], NP[dtype]).astype(np.float64)[:, None]
    err = float((np.abs(got - want) / np.abs(want).max()).max())
    # (measured on MI355X: 5.0e-13 in fp64 on both meshes and in both tiers -- the outward-oriented boundary faces and the
    # interior faces round the same physical flux differently; not bitwise)
    tol = {torch.float64: 1e-12, torch.float32: TOL1[torch.float32]}[dtype]
    assert err < tol, err


def sod_exact(x, t, x0=0.5, gamma=1.4, left=(1.0, 0.0, 1.0), right=(0.125, 0.0, 0.1)):
    """exact solution of the Riemann problem (rho, u, p) at positions x, time t (Toro, ch. 4)"""
    rl, ul, pl = left
    rr, ur, pr = right
    cl, cr = np.sqrt(gamma * pl / rl), np.sqrt(gamma * pr / rr)

    def f(p, rk, pk, ck):
        if p > pk:
            A, B = 2 / ((gamma + 1) * rk), (gamma - 1) / (gamma + 1) * pk
            return (p - pk) * np.sqrt(A / (p + B))
        return 2 * ck / (gamma - 1) * ((p / pk) ** ((gamma - 1) / (2 * gamma)) - 1)

    lo, hi = 1e-8, 10.0
    for _ in range(200):
        p = 0.5 * (lo + hi)
        if f(p, rl, pl, cl) + f(p, rr, pr, cr) + ur - ul > 0:
            hi = p
        else:
            lo = p
    ps = 0.5 * (lo + hi)
    us = 0.5 * (ul + ur) + 0.5 * (f(ps, rr, pr, cr) - f(ps, rl, pl, cl))
    rsl = rl * (ps / pl) ** (1 / gamma)                                   # left rarefaction
    rsr = rr * ((ps / pr + (gamma - 1) / (gamma + 1)) / ((gamma - 1) / (gamma + 1) * ps / pr + 1))   # right shock
    sh = ur + cr * np.sqrt((gamma + 1) / (2 * gamma) * ps / pr + (gamma - 1) / (2 * gamma))
    csl = cl * (ps / pl) ** ((gamma - 1) / (2 * gamma))
    s = (np.asarray(x) - x0) / t
    rho, u, p = np.empty_like(s), np.empty_like(s), np.empty_like(s)
    head, tail = ul - cl, us - csl
    for i, si in enumerate(s):
        if si < head:
            rho[i], u[i], p[i] = rl, ul, pl
        elif si < tail:
            u[i] = 2 / (gamma + 1) * (cl + (gamma - 1) / 2 * ul + si)
            c = 2 / (gamma + 1) * (cl + (gamma - 1) / 2 * (ul - si))
            rho[i], p[i] = rl * (c / cl) ** (2 / (gamma - 1)), pl * (c / cl) ** (2 * gamma / (gamma - 1))
        elif si < us:
            rho[i], u[i], p[i] = rsl, us, ps
        elif si < sh:
            rho[i], u[i], p[i] = rsr, us, ps
        else:
            rho[i], u[i], p[i] = rr, ur, pr
    return rho, u, p


SOD_L1_BOUND = 0.03   # L1 error of rho over x in [0, 0.85] at t = 0.4, uniform level 7, KEPES (measured on MI355X: 0.0140)


def test_sod_tube_lets_the_shock_out():
    """2D Sod tube, x outflow, y periodic, uniform level 7: at t = 0.4 the shock (speed 1.75) has left through x = 1 and the
    post-shock state fills the right end; a wall there would have reflected the shock back into it."""
    mesh = SynthMesh(2, 7, 7, sides=("outflow", "outflow", "periodic", "periodic"))
    part = mesh.partition()
    x = part.centres[:, 0]
    left = x < 0.5
    rho = np.where(left, 1.0, 0.125)
    p = np.where(left, 1.0, 0.1)
    st = np.stack([rho, 0 * rho, 0 * rho, 0 * rho, p / 0.4])
    g = PlainSolver(part, torch.float64, mode="fused", state=st)
    t, dt = 0.0, 0.2 * 2.0 ** -7
    while t < 0.4 - 1e-12:
        step = min(dt, 0.4 - t)
        g.iterate(step)
        t += step
    torch.cuda.synchronize()
    u = g.state().cpu().numpy()
    xo = x[:part.N]
    rho_g = u[0]
    p_g = 0.4 * (u[4] - 0.5 * (u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0])
    end = (xo > 0.90) & (xo < 0.98)
    r_end, p_end = rho_g[end].mean(), p_g[end].mean()
    print(f"sod: mean rho {r_end:.4f} (exact 0.2656), mean p {p_end:.4f} (exact 0.3031) over x in [0.90, 0.98]")
    # measured: rho 0.2810 (+5.8 %: the window starts 0.03 right of the contact at x = 0.871, which the first-order scheme
    # smears into it), p 0.3029 (-0.1 %). A reflected shock would raise p there far above 0.3031.
    assert abs(r_end - 0.2656) < 0.08 * 0.2656 and abs(p_end - 0.3031) < 0.03 * 0.3031
    inner = xo < 0.85
    rho_x, _, _ = sod_exact(xo[inner], 0.4)
    l1 = float(np.abs(rho_g[inner] - rho_x).mean() * 0.85)
    print(f"sod: L1(rho) over [0, 0.85] = {l1:.4f}")
    assert l1 < SOD_L1_BOUND


def test_adaptive_run_with_open_sides_follows_the_oracle():
    """iterate / adapt / iterate on the device against the same sequence on the host (oracle-composed reference, the
    oracle's indicator and transfer), in the manner of test_gpu_amr.py: the kinds and the inflow states survive adapt."""
    mesh = SynthMesh(2, 4, 6, band=0.03, sides=SIDES[2])
    part = mesh.partition()
    inflow = inflow_states(2)
    st = perturbed_state(part, 15)
    g = PlainSolver(part, torch.float64, mode="fused", state=st, inflow_states=inflow)
    g.use_native_stepper()
    o = OpenCase(part, np.float64, st, inflow)
    for cycle in range(3):
        dt = 0.1 * 2.0 ** -g.part.mesh.finest_level
        for _ in range(5):
            g.iterate(dt)
            o.iterate(dt)
        g, marks, _ = amr.adapt(g, threshold=10.0, min_level=3, max_level=7)
        assert g.plan.c.has_open_faces and np.array_equal(g.inflow_states, inflow)
        opart = o.part
        rho = o.current()[0, :opart.N].copy()
        grad = np.zeros(opart.N)
        O.lib().oracle_estimate_gradient_f64(opart.F, O.p(opart.face_neighbors), None, O.p(rho), O.p(grad))
        crit = np.zeros(opart.N)
        O.lib().oracle_refinement_criteria_f64(opart.N, O.p(grad), O.p(opart.volumes), O.p(crit))
        omarks = opart.mesh.marks_from_criteria(crit, 10.0, 3, 7)
        assert np.array_equal(omarks, marks)
        nmesh, oad = opart.mesh.adapt(omarks)
        npart = nmesh.partition()
        cur = np.ascontiguousarray(o.current()[:, :opart.N])
        nst = np.zeros((5, npart.N))
        nvol = np.zeros(npart.N)
        O.lib().oracle_adapt_variables_and_volume_f64(npart.N, 2, O.p(oad), O.p(cur), C.c_size_t(opart.N), O.p(nst), C.c_size_t(npart.N),
                                                      O.p(opart.volumes), O.p(nvol))
        nxt, prv = o.next, o.prev
        o = OpenCase(npart, np.float64, np.zeros((5, npart.N)), inflow)
        o.next, o.prev = nxt, prv
        o.planes[5 * o.next:5 * o.next + 5, :npart.N] = nst
        assert g.N == npart.N
        assert rel_err(g.state().cpu().numpy(), o.current()[:, :npart.N]) < TOL10[torch.float64]


def test_riemann2d_example_writes_a_readable_vtu(tmp_path):
    from _vtu import read_vtu
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "riemann2d_amr.py"), "--toy", "--out", str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    files = sorted(tmp_path.glob("*.vtu"))
    assert files
    v = read_vtu(str(files[-1]))
    assert v["n_cells"] > 0 and v["arrays"]["density"].size == v["n_cells"]
    assert np.isfinite(v["arrays"]["density"]).all() and (v["arrays"]["density"] > 0).all()


def test_subgrid_solver_refuses_open_kinds():
    part = SynthMesh(2, 2, 3, sides=("outflow", "outflow", "periodic", "periodic")).partition(subgrid=True)
    with pytest.raises(ValueError, match="walls only"):
        SubgridSolver(part, torch.float32)
    walls = SynthMesh(2, 2, 3, periodic=False).partition(subgrid=True)
    SubgridSolver(walls, torch.float32)


def test_inflow_states_are_validated():
    part = mesh_of(2).partition()
    with pytest.raises(ValueError, match="required"):
        PlainSolver(part, torch.float64)
    for bad in (np.zeros((1, 4)), np.zeros((9, 5)), np.array([[-1.0, 0, 0, 0, 2.5]]), np.array([[1.0, 0, 0, 0, -1.0]])):
        with pytest.raises(ValueError):
            PlainSolver(part, torch.float64, inflow_states=bad)
