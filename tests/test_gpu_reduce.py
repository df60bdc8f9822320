"""-m gpu: device-side max-speed and conservation-integral reductions against numpy."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _scalar_ref as R
from t8gpu_amd import hip
from t8gpu_amd.solver import PlainSolver, SubgridSolver
from t8gpu_amd.synth import SynthMesh

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [0, 1, 255, 100003, 1 << 21, 256, 257, 262143, 262144, 262145, 524305])
def test_reductions_match_numpy(dtype, n):
    rng = np.random.default_rng(n + 1)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    x = rng.uniform(0, 5, max(n, 1)).astype(npdt)
    v = rng.uniform(0.1, 1, max(n, 1)).astype(npdt)
    dx, dv = torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda()
    f = hip.lib().t8gpu_hip_reduce_workspace_bytes
    f.restype = C.c_size_t
    ws = torch.zeros(f() // 8, dtype=torch.float64, device="cuda")
    res = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    hip.call("t8gpu_hip_max_speed", dtype, C.c_size_t(n), hip.ptr(dx), hip.ptr(ws), hip.ptr(res), hip.stream_ptr())
    assert float(res.item()) == (float(x[:n].max()) if n else 0.0)
    hip.call("t8gpu_hip_integral", dtype, C.c_size_t(n), 1, hip.ptr(dx), hip.ptr(dv), hip.ptr(ws), hip.ptr(res), hip.stream_ptr())
    want = float((x[:n].astype(np.float64) * v[:n].astype(np.float64)).sum())
    assert abs(float(res.item()) - want) <= 1e-12 * max(1.0, abs(want))
    first = float(res.item())
    hip.call("t8gpu_hip_integral", dtype, C.c_size_t(n), 1, hip.ptr(dx), hip.ptr(dv), hip.ptr(ws), hip.ptr(res), hip.stream_ptr())
    assert float(res.item()) == first                                   # fixed tree: bitwise reproducible


# ---- signed data, the grid-stride threshold, cells per element, NaN ------------------------------------------------------------
# 262 144 = kReduceBlocks x 256 is the size from which a lane takes more than one element (the grid-stride loop starts).
SIZES = [1, 255, 256, 257, 100003, 262143, 262144, 262145, 524305]
NPDT = {torch.float64: np.float64, torch.float32: np.float32}


def buffers():
    f = hip.lib().t8gpu_hip_reduce_workspace_bytes
    f.restype = C.c_size_t
    assert f() == 8 * 1024                                              # kReduceBlocks = 1024: what R.integral_terms assumes
    return torch.zeros(f() // 8, dtype=torch.float64, device="cuda"), torch.full((1,), -1.0, dtype=torch.float64, device="cuda")


def max_speed(dtype, n, dx, ws, res):
    hip.call("t8gpu_hip_max_speed", dtype, C.c_size_t(n), hip.ptr(dx), hip.ptr(ws), hip.ptr(res), hip.stream_ptr())
    return float(res.item())


def integral(dtype, n, cpe, dx, dv, ws, res):
    hip.call("t8gpu_hip_integral", dtype, C.c_size_t(n), cpe, hip.ptr(dx), hip.ptr(dv), hip.ptr(ws), hip.ptr(res), hip.stream_ptr())
    return float(res.item())


def assert_integral(dtype, n, cpe, x, vol):
    """x: [n] cells, vol: [ceil(n / cpe)] element volumes. Reference: math.fsum (exact, rounded once) of the float64 products
    (vol / cpe) * x. Bound: (ceil(n / (blocks 256)) + 24) 2^-53 sum |vol / cpe * x| -- R.integral_terms counts the roundings on
    the longest path of the device sum, each at most 2^-53 of a partial sum, which never exceeds the sum of the magnitudes."""
    ws, res = buffers()
    dx, dv = torch.from_numpy(x).cuda(), torch.from_numpy(vol).cuda()
    prod = np.repeat(vol.astype(np.float64) / cpe, cpe)[:n] * x.astype(np.float64)
    want, scale = math.fsum(prod), math.fsum(np.abs(prod))
    got = integral(dtype, n, cpe, dx, dv, ws, res)
    bound = R.integral_terms(n) * 2.0 ** -53 * scale
    print(f"FIG integral {hip.suffix(dtype)} n={n} cpe={cpe}: |got - want| / bound = {abs(got - want) / bound:.3f}, want / sum|.| = {want / scale:.2e}")
    assert abs(got - want) <= bound, (got, want, bound)
    assert integral(dtype, n, cpe, dx, dv, ws, res) == got               # the bits of a second call


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", SIZES)
def test_integral_of_signed_data(dtype, n):
    """x ~ N(0, 1): the integral cancels to about sqrt(n) of the sum of magnitudes (a momentum integral), where a bound
    relative to max(1, |want|) checks nothing"""
    rng = np.random.default_rng(1000 + n)
    assert_integral(dtype, n, 1, rng.standard_normal(n).astype(NPDT[dtype]), rng.uniform(0.1, 1, n).astype(NPDT[dtype]))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("cpe", [16, 64])
@pytest.mark.parametrize("elements", [1, 4099])
def test_integral_cells_per_element(dtype, cpe, elements):
    """Subgrid blocks: cells_per_element 16 and 64, per-element volumes 2^-k of mixed k (an adapted mesh), one element and a
    number of elements that is no multiple of 4 (4 099 x 64 = 262 336 cells: past the grid-stride threshold)"""
    rng = np.random.default_rng(cpe + elements)
    n = elements * cpe
    vol = (2.0 ** -rng.integers(6, 19, elements)).astype(NPDT[dtype])
    assert elements == 1 or len(set(vol.tolist())) > 4
    assert_integral(dtype, n, cpe, rng.standard_normal(n).astype(NPDT[dtype]), vol)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", SIZES)
def test_max_speed_identity_and_last_element(dtype, n):
    """all-negative data give 0.0, the documented identity (speeds are >= 0); a maximum in the LAST element is found at every
    size (the end of the grid-stride loop), and one in the first"""
    rng = np.random.default_rng(2000 + n)
    ws, res = buffers()
    x = -rng.uniform(0.5, 5, n).astype(NPDT[dtype])
    dx = torch.from_numpy(x).cuda()
    assert max_speed(dtype, n, dx, ws, res) == 0.0
    dx.neg_()
    assert max_speed(dtype, n, dx, ws, res) == float((-x).max())
    for at in (n - 1, 0):
        dx[at] = 7.5
        assert max_speed(dtype, n, dx, ws, res) == 7.5
        dx[at] = 0.25


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [1, 255, 100003, 524305])
def test_max_speed_propagates_nan(dtype, n):
    """One NaN speed estimate (a blown-up state) gives NaN wherever it sits: at index 0, n // 2, n - 1, and in each of the four
    wavefronts of a 256-thread workgroup, in the first and in the last workgroup's share. With `a > b ? a : b` the result
    depended on the position, and compute_timestep returned a finite step on some layouts."""
    rng = np.random.default_rng(3000 + n)
    ws, res = buffers()
    dx = torch.from_numpy(rng.uniform(0, 5, n).astype(NPDT[dtype])).cuda()
    clean = max_speed(dtype, n, dx, ws, res)
    assert clean == float(dx.max().item())
    last = ((n - 1) // 256) * 256
    spots = {0, n // 2, n - 1} | {w * 64 + 5 for w in range(4)} | {last + w * 64 + 9 for w in range(4)}
    for at in sorted(s for s in spots if s < n):
        keep = float(dx[at].item())
        dx[at] = float("nan")
        got = max_speed(dtype, n, dx, ws, res)
        assert math.isnan(got), (at, got)
        dx[at] = keep
    assert max_speed(dtype, n, dx, ws, res) == clean                     # and nothing of it stays behind in the workspace


def test_solver_timestep_is_nan_for_a_nan_speed():
    part = SynthMesh(2, 4, 5, band=0.06).partition()
    g = PlainSolver(part, torch.float64, mode="fused")
    g.iterate(0.1 * 2.0 ** -5)
    assert math.isfinite(g.compute_timestep())
    for at in (0, part.F // 2, part.F + part.B - 1):
        keep = float(g.speed[at].item())
        g.speed[at] = float("nan")
        assert math.isnan(g.max_speed()) and math.isnan(g.compute_timestep()), at
        g.speed[at] = keep
    assert math.isfinite(g.compute_timestep())


def test_solver_diagnostics_conservation_and_cfl():
    mesh = SynthMesh(2, 4, 7, band=0.06)
    part = mesh.partition()
    g = PlainSolver(part, torch.float64, mode="fused")
    m0 = [g.compute_integral(k) for k in range(5)]
    assert abs(m0[0] - (part.kh_initial_state()[0] * part.volumes).sum()) < 1e-13
    dt = 0.1 * 2.0 ** -7
    for _ in range(5):
        g.iterate(dt)
    m1 = [g.compute_integral(k) for k in range(5)]
    assert max(abs(a - b) for a, b in zip(m0, m1)) < 1e-12 * max(abs(x) for x in m0)   # periodic mesh: conservative to rounding
    smax = g.max_speed()
    assert smax == float(g.speed[:part.F].max().item()) and 1.0 < smax < 3.0
    assert np.isclose(g.compute_timestep(), 0.7 * 0.5 ** 7 / smax)
