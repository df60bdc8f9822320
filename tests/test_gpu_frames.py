"""-m gpu: the face frames the kernels build, against the long-double reference of tests/_frame_ref.py.

  * t8gpu_hip_plain_geo_frames_{f32,f64} (k_geo_frames -> flux_math.hpp: face_basis_fast): defect of orthonormality and tangent
    angle on the generated normals (axes, planar, the bad direction +-(1, -1, 1) / sqrt 3 of the reference's seed, a sweep
    around it, the boundary of the second seed's cone, the sphere, the golden normals), the table's layout, the launcher's
    argument checks, and agreement with the host dictionary's frames (tile_plan.cpp).
  * the compat face kernels (flux_math.hpp: face_basis, IEEE square root and division): with uL = uR = u the flux through a
    face is the physical flux area (rho vn, rho vn v + p n, vn (E + p)), whatever the tangents; a frame that is not orthonormal
    shows as an error of the order of its defect.

Limits (tests/_frame_ref.py): defect 64 eps, tangent angle 32 eps radians. The measured worst values are printed."""
import ctypes as C

import numpy as np
import pytest
import torch

import _frame_ref as FR
from _gpu import NP
from t8gpu_amd import hip
from t8gpu_amd.solver import FLUXES

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
SENTINEL = -777.25
INVALID = 1                                   # hipErrorInvalidValue
CHUNKS = (1, 127, 128, 129, 257)             # n_geo of the launches: one lane, around the 128-thread block, three blocks
LD = FR.LD


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def geo_frames(dtype, table, n_geo, null=False):
    fn = getattr(hip.lib(), "t8gpu_hip_plain_geo_frames_" + hip.suffix(dtype))
    fn.restype = C.c_int
    rc = fn(None if null else hip.ptr(table), int(n_geo), hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


_frames = {}


def device_frames(dtype):
    """(n, layout violations, t1, t2) of every generated normal, computed once per type: tables of n_geo + 3 rows pre-filled
    with a sentinel, n_geo cycling through CHUNKS; test_geo_frames_leave_the_rest_of_the_table_alone asserts the layout"""
    if dtype in _frames:
        return _frames[dtype]
    T = NP[dtype]
    normals = FR.all_normals(T)
    areas = np.random.default_rng(11).uniform(0.5, 2.0, len(normals)).astype(T)
    t1, t2 = np.empty_like(normals), np.empty_like(normals)
    at, k, layout = 0, 0, []
    while at < len(normals):
        n_geo = min(CHUNKS[k % len(CHUNKS)], len(normals) - at)
        k += 1
        host = np.full((n_geo + 3, 12), SENTINEL, T)
        host[:n_geo, 0:3], host[:n_geo, 3] = normals[at:at + n_geo], areas[at:at + n_geo]
        dev = torch.from_numpy(host.copy()).cuda()
        assert geo_frames(dtype, dev, n_geo) == 0
        got = dev.cpu().numpy()
        if not np.array_equal(bits(got[:, [0, 1, 2, 3, 7, 11]]), bits(host[:, [0, 1, 2, 3, 7, 11]])):   # n, area, padding
            layout.append(f"n_geo = {n_geo}: words 0-3, 7 or 11 of a row changed")
        if not np.array_equal(bits(got[n_geo:]), bits(host[n_geo:])):
            layout.append(f"n_geo = {n_geo}: a row at or beyond n_geo changed")
        t1[at:at + n_geo], t2[at:at + n_geo] = got[:n_geo, 4:7], got[:n_geo, 8:11]
        at += n_geo
    assert k > 2 * len(CHUNKS)
    _frames[dtype] = (normals, layout, t1, t2)
    return _frames[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_geo_frames_are_rotations_near_the_reference(dtype):
    normals, _, t1, t2 = device_frames(dtype)
    at = 0
    for name, fam in FR.normals(NP[dtype]).items():
        sl = slice(at, at + len(fam))
        FR.check_frames(normals[sl], t1[sl], t2[sl], f"k_geo_frames {name}")
        at += len(fam)
    assert at == len(normals)


@pytest.mark.parametrize("dtype", DTYPES)
def test_geo_frames_leave_the_rest_of_the_table_alone(dtype):
    """words 0-3 (n, area), 7 and 11 of every row and every row at or beyond n_geo keep the bits they had (a sentinel where the
    planner writes 0), for n_geo = 1, 127, 128, 129, 257 and a shorter last table"""
    assert device_frames(dtype)[1] == []


@pytest.mark.parametrize("dtype", DTYPES)
def test_geo_frames_of_axis_normals_are_axis_basis(dtype):
    """+-e_k: the frame of axis_basis, and bit for bit the construction's (which leaves -0 where axis_basis writes +0: -n[0],
    and (-0) - (+0) in the cross product; see test_frames_host.py)"""
    normals, _, t1, t2 = device_frames(dtype)
    n, a1, a2 = FR.axis_frames(NP[dtype])
    assert np.array_equal(normals[:6], n)
    assert np.array_equal(t1[:6], a1) and np.array_equal(t2[:6], a2)
    e1, e2 = FR.emulate(n, fast=True)
    assert np.array_equal(bits(t1[:6]), bits(e1)) and np.array_equal(bits(t2[:6]), bits(e2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_geo_frames_agree_with_the_host_dictionary(dtype):
    """the dictionary's frames as the planner computes them (double, IEEE square root and division) against the device's (one
    reciprocal square root): within the tangent-angle limit, 32 eps of the device's type. fp32: the planner decides on the seed in
    double, the device on |r|^2 rounded to fp32, so the normals within SWITCH_BAND of the cone's boundary are left out there."""
    T = NP[dtype]
    normals, _, t1, t2 = device_frames(dtype)
    keep = np.sort(np.unique(normals, axis=0, return_index=True)[1])
    if T == np.float32:
        keep = keep[np.abs(FR.exact_r2(normals[keep]) - LD(FR.SWITCH)) > FR.SWITCH_BAND * FR.eps(T)]
    n = normals[keep]
    table = FR.dictionary_rows(n.astype(np.float64), np.ones(len(n)))
    assert len(table) == len(n)
    row = {bits(r[:3]).tobytes(): r for r in table}
    host = np.stack([row[bits(x.astype(np.float64)).tobytes()] for x in n])
    ang = (FR.pair_angle(t1[keep], t2[keep], host[:, 4:7], host[:, 8:11]) / LD(FR.eps(T))).astype(np.float64)
    i = int(np.argmax(ang))
    print(f"device against host dictionary {T.__name__}: worst tangent angle {ang[i]:.1f} eps of {FR.ANGLE_LIMIT:.0f} at n = {n[i]}")
    assert ang[i] <= FR.ANGLE_LIMIT


@pytest.mark.parametrize("dtype", DTYPES)
def test_geo_frames_argument_checks(dtype):
    T = NP[dtype]
    host = np.full((4, 12), SENTINEL, T)
    host[:, 0:3] = FR.normals(T)["sphere"][:4]
    dev = torch.from_numpy(host.copy()).cuda()
    assert geo_frames(dtype, dev, 0) == 0                       # launches nothing
    assert geo_frames(dtype, dev, -1) == INVALID
    assert geo_frames(dtype, dev, 4, null=True) == INVALID
    assert geo_frames(dtype, dev, 0, null=True) == 0
    assert np.array_equal(bits(dev.cpu().numpy()), bits(host))
    assert torch.cuda.current_stream().query()


# ---- the compat kernels: face_basis through the flux of a uniform state ---------------------------------------------------
RHO, P = 1.1, 0.9
DIRECTION = np.array([0.48, -0.6, 0.64])                        # unit, oblique to every axis and to the bad direction
MACH = {"at rest": 0.0, "Mach 0.5": 0.5, "Mach 3": 3.0}
# Roundings on the longest path from the state to an xyz flux component, half an ulp each, relative to rho |v|^2 + p: the
# rotation into the frame (5), velocities and kinetic energy (6), pressure and beta (5), the means (4; the logarithmic mean of
# two equal values is its series, (2 a) 52.5 / 105), the flux (4), gamma - 1 as rounded (1), the rotation back (5): 30 roundings,
# 15 eps; HLL / HLLC replace the means by their wave-speed combination (8 more). 16 + 4.
OPS = 20.0


def conservative(T, v):
    """[k, 5] states of velocity v [k, 3], rounded to T"""
    v = np.asarray(v, np.float64)
    E = P / 0.4 + 0.5 * RHO * (v * v).sum(1)
    return np.concatenate([np.full((len(v), 1), RHO), RHO * v, E[:, None]], 1).astype(T)


def physical_flux(state, n, area, wall):
    """area (rho vn, rho vn v + p n, vn (E + p)) in long double from the rounded state, normal and area; wall: (0, p n area, 0).
    Also rho |v|^2 + p, the sound speed and vn."""
    s, n, area = state.astype(LD), n.astype(LD), area.astype(LD)
    rho, E = s[:, 0], s[:, 4]
    v = s[:, 1:4] / rho[:, None]
    v2 = (v * v).sum(1)
    p = LD(0.4) * (E - LD(0.5) * rho * v2)                       # (LD(0.4): the double nearest 0.4; gamma - 1 as rounded is in OPS)
    vn = (v * n).sum(1)
    F = np.zeros((len(s), 5), LD)
    if wall:
        F[:, 1:4] = p[:, None] * n
    else:
        F[:, 0] = rho * vn
        F[:, 1:4] = (rho * vn)[:, None] * v + p[:, None] * n
        F[:, 4] = vn * (E + p)
    return F * area[:, None], rho * v2 + p, np.sqrt(LD(1.4) * p / rho), vn, np.sqrt(v2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,name", [(hip.KEPES, "kepes"), (hip.HLL, "hll"), (hip.HLLC, "hllc")])
@pytest.mark.parametrize("wall", [False, True])
def test_compat_flux_of_a_uniform_state_is_the_physical_flux(dtype, kind, name, wall):
    """One face per generated normal, as in test_gpu_compat.py::test_compat_flux_kernels_on_the_reference_vectors: an interior
    face i joins elements 2i and 2i + 1, both in state u; a wall face i belongs to element i.
    Bound per component: (64 + OPS) eps (rho |v|^2 + p) area.
    Walls: the reflective flux is (0, p n area, 0) only for a velocity tangent to the wall (with vn != 0 every one of the three
    fluxes adds an impedance term of the order rho (a + |v|) vn to the pressure), so each wall element carries the Mach 0.5 /
    Mach 3 velocity with its normal component removed in long double; the vn that rounding the state leaves, ~eps |v|, enters the
    bound as 2 rho (a + |v|) |vn| area."""
    T = NP[dtype]
    normals = FR.all_normals(T)
    k = len(normals)
    areas = np.random.default_rng(12).uniform(0.5, 2.0, k).astype(T)
    d_n, d_a = torch.from_numpy(np.ascontiguousarray(normals)).cuda(), torch.from_numpy(areas).cuda()
    a0 = np.sqrt(1.4 * P / RHO)
    for label, mach in MACH.items():
        v = np.tile(mach * a0 * DIRECTION, (k, 1))
        if wall:
            nl = normals.astype(LD)
            v = (v - ((v * nl).sum(1) / (nl * nl).sum(1))[:, None] * nl).astype(np.float64)
        state = conservative(T, v)
        want, scale, snd, vn, speed = physical_flux(state, normals, areas, wall)
        if wall:
            elems, fn, F, B = state, np.arange(k, dtype=np.int32), 0, k
        else:
            elems, fn, F, B = np.repeat(state, 2, axis=0), np.arange(2 * k, dtype=np.int32), k, 0
        planes = torch.zeros((26, len(elems)), dtype=dtype, device="cuda")
        planes[0:5] = torch.from_numpy(np.ascontiguousarray(elems.T)).cuda()
        d_fn = torch.from_numpy(fn).cuda()
        out = torch.zeros(k, dtype=dtype, device="cuda")
        st, fl = hip.vars_of(planes, 0), hip.vars_of(planes, FLUXES)
        if wall:
            hip.call("t8gpu_hip_flux_boundary", dtype, kind, 0, B, 3, hip.ptr(d_fn), hip.ptr(d_n), hip.ptr(d_a), st, fl, hip.ptr(out),
                     hip.stream_ptr())
            torch.cuda.synchronize()
            got = -planes[20:25].cpu().numpy().T
        else:
            hip.call("t8gpu_hip_flux_faces", dtype, kind, F, 3, hip.ptr(d_fn), None, hip.ptr(d_n), hip.ptr(d_a), st, fl, hip.ptr(out),
                     hip.stream_ptr())
            torch.cuda.synchronize()
            fluxes = planes[20:25].cpu().numpy()
            got = fluxes[:, 1::2].T
            assert np.array_equal(fluxes[:, 0::2], -fluxes[:, 1::2])
        e = LD(FR.eps(T))
        bound = LD(FR.DEFECT_LIMIT + OPS) * e * scale * areas.astype(LD)
        if wall:
            bound = bound + 2 * LD(RHO) * (snd + speed) * np.abs(vn) * areas.astype(LD)
        err = np.abs(got.astype(LD) - want)
        err = np.where(np.isfinite(err), err, np.inf)
        ratio = (err / bound[:, None]).astype(np.float64)
        i, c = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        print(f"compat {name} {'wall' if wall else 'interior'} {T.__name__} {label}: worst error / bound {ratio[i, c]:.3f} "
              f"(component {c}, n = {normals[i]})")
        assert ratio[i, c] <= 1.0, (label, ratio[i, c], normals[i], int(c))
