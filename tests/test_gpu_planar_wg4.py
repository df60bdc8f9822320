"""The planar fp64 stage at FOUR workgroups per CU (kernels_fused_patch.hip: packed, rotated LDS records; a register budget of
four workgroups; plain_patch_stage: per_cu = 4 where the LDS window is at most 40 960 bytes) against the general form.

The reference of every case is the python-driven iterate(), which runs the general form at three workgroups per CU with the
unpacked records. Every comparison is on the raw bits (-0.0 != +0.0) of all 25 state planes over the owned slots and of the
speed estimates, as in test_gpu_planar.py.

  small mesh   SynthMesh(2, 5, 7, band=0.13): 9 856 quadrilaterals, 24 patches and 39 generic tiles in one mixed launch -- every
               patch workgroup has one patch, the generic tiles run the tile body behind them under the four-workgroup budget
  c2 mesh      SynthMesh(2, 6, 11, band=0.0596): ~1.03 M quadrilaterals, ~3 900 patches -- more than 4 x CUs, so the workgroups
               walk several patches each with the prefetch live: the smallest shape at which the pipelined walk at the new
               residency can go wrong
"""
import ctypes as C

import numpy as np
import pytest
import torch

from t8gpu_amd import hip
from t8gpu_amd.solver import PlainSolver
from t8gpu_amd.synth import SynthMesh

pytestmark = pytest.mark.gpu

_BITS = {torch.float64: torch.int64, torch.float32: torch.int32}
LDS_QUARTER_CU = 160 * 1024 // 4          # four workgroups in a CU's 160 KiB


def planar_state(part, seed=3):
    """A 2D state (z-momentum +0 everywhere) with a random in-plane perturbation."""
    rng = np.random.default_rng(seed)
    n = part.N + part.G
    rho = 1.0 + 0.3 * rng.uniform(-1, 1, n)
    v = 0.4 * rng.standard_normal((2, n))
    p = 1.0 + 0.2 * rng.uniform(-1, 1, n)
    E = p / 0.4 + 0.5 * rho * (v ** 2).sum(0)
    return np.stack([rho, rho * v[0], rho * v[1], np.zeros(n), E])


def adversarial_state(part):
    """Equal neighbouring states over whole regions (all jumps zero: the series branch of the logarithmic mean, zero
    dissipation), momentum entries of -0.0 and +0.0, cells at rest beside moving ones."""
    st = planar_state(part, 5)
    n = st.shape[1]
    e = np.arange(n)
    block = (e // 700) % 3               # runs of the space-filling curve: whole regions
    for k in (0, 1, 2, 4):
        st[k, block == 0] = st[k, 0]      # one state everywhere in the region
    st[1, block == 1] = np.where(e[block == 1] % 2 == 0, -0.0, 0.0)     # x-momentum +-0, y-momentum as it is
    st[2, (block == 2) & (e % 3 == 0)] = -0.0
    st[1, (block == 2) & (e % 5 == 0)] = 0.0
    rest = (e % 11 == 0)
    st[1, rest], st[2, rest] = 0.0, -0.0
    st[4] = np.maximum(st[4], 0.5 * (st[1] ** 2 + st[2] ** 2) / st[0] + 1.0)    # pressure stays positive
    assert not np.signbit(st[3]).any()
    return st


def bits(t):
    return t.contiguous().view(_BITS[t.dtype])


def last_kernel():
    """the kernel that carried most of the last stage call's work on this thread (t8gpu_hip_last_stage_kernel)"""
    q = hip.lib().t8gpu_hip_last_stage_kernel
    q.restype = C.c_char_p
    return (q() or b"").decode()


def assert_same_bits(a, b):
    assert (a.next, a.prev) == (b.next, b.prev)
    n = a.owned_cells
    assert torch.equal(bits(a.planes[:25, :n]), bits(b.planes[:25, :n]))
    assert torch.equal(bits(a.speed), bits(b.speed))


def run_pair(part, dtype, state, steps, dt, kind=hip.KEPES):
    """(general solver driven from python, native-stepper solver with set_planar(2), their last kernels) after `steps` steps"""
    a = PlainSolver(part, dtype, flux_kind=kind, mode="fused", state=state)
    b = PlainSolver(part, dtype, flux_kind=kind, mode="fused", state=state)
    b.use_native_stepper().set_planar(2)
    for _ in range(steps):
        a.iterate(dt)
    torch.cuda.synchronize()
    ka = last_kernel()
    b.iterate_steps(steps, dt)
    torch.cuda.synchronize()
    return a, b, ka, last_kernel()


def patch_lds_bytes(plan_c, kind, float_size, planar):
    q = hip.lib().t8gpu_hip_plain_patch_lds_bytes
    q.restype = C.c_int
    return q(C.byref(plan_c) if plan_c is not None else None, C.c_int(kind), C.c_int(float_size), C.c_int(planar))


@pytest.fixture(scope="module", params=[True, False], ids=["periodic", "walled"])
def small(request):
    return SynthMesh(2, 5, 7, band=0.13, periodic=request.param).partition()


@pytest.fixture(scope="module")
def c2():
    return SynthMesh(2, 6, 11, band=0.0596).partition()


# ---- host only: the launcher's LDS windows ---------------------------------------------------------------------------------------
def test_planar_fp64_patch_window_fits_four_per_cu():
    got = patch_lds_bytes(None, hip.KEPES, 8, 1)
    assert 0 < got <= LDS_QUARTER_CU
    assert got == 8 * 4 * 544 + 64 * 320 + 2048                      # flux slots, 320 packed records, the logarithm table
    # every other form keeps its records: general fp64, fp32 (general and planar), HLL / HLLC (a planar request is not honoured)
    assert patch_lds_bytes(None, hip.KEPES, 8, 0) == 8 * (5 * 544 + 10 * 320) + 2048
    assert patch_lds_bytes(None, hip.KEPES, 4, 0) == 4 * (5 * 544 + 12 * 320)
    assert patch_lds_bytes(None, hip.KEPES, 4, 1) == 4 * (4 * 544 + 12 * 320)
    for kind in (hip.HLL, hip.HLLC):
        assert patch_lds_bytes(None, kind, 8, 1) == patch_lds_bytes(None, kind, 8, 0) == 8 * (5 * 544 + 6 * 320)
    assert patch_lds_bytes(None, 3, 8, 1) == -1 and patch_lds_bytes(None, hip.KEPES, 2, 1) == -1


def test_mixed_window_of_the_small_mesh_fits_four_per_cu(small):
    c = PlainSolver(small, torch.float64, mode="fused").plan.c
    patches = sum(c.n_patch_tiles)
    assert c.patch_dim != 3 and patches >= 4 and c.ntiles - patches >= 2
    tile = 8 * (9 * c.max_slots + 1280) + 2064
    assert patch_lds_bytes(c, hip.KEPES, 8, 1) == max(tile, 39936) <= LDS_QUARTER_CU


# ---- case 1: one mixed launch, a patch per workgroup ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["random", "adversarial"])
def test_small_mesh_equals_general(small, case):
    st = planar_state(small) if case == "random" else adversarial_state(small)
    a, b, ka, kb = run_pair(small, torch.float64, st, 3, 0.1 * 2.0 ** -7)
    assert b.stepper.planar() == 1
    assert ka == "k_plain_stage<double, 0, 3, false, false, false>", ka
    assert kb == "k_plain_stage<double, 0, 3, false, false, true>", kb
    assert_same_bits(a, b)
    assert not bits(b.planes[:20, :b.owned_cells])[3::5].any()      # the z-momentum of every step slot: +0


# ---- case 2: workgroups walk several patches at four per CU ---------------------------------------------------------------------
@pytest.mark.parametrize("case", ["random", "adversarial"])
def test_c2_mesh_pipelined_walk_equals_general(c2, case):
    st = planar_state(c2, 7) if case == "random" else adversarial_state(c2)
    a, b, ka, kb = run_pair(c2, torch.float64, st, 2, 0.1 * 2.0 ** -11)
    c = b.plan.c
    patches = sum(c.n_patch_tiles)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert patches > 4 * cus and c.ntiles - patches >= 2, (patches, cus)
    assert patch_lds_bytes(c, hip.KEPES, 8, 1) <= LDS_QUARTER_CU
    assert b.stepper.planar() == 1
    assert kb.startswith("k_plain_stage<double, 0, 3, ") and kb.endswith(", false, true>"), kb
    assert_same_bits(a, b)


# ---- case 3: everything else as before -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,kind,native_kernel", [
    (torch.float32, hip.KEPES, "k_plain_stage<float, 0, 3, false, false, true>"),      # the fp32 planar form: five per CU, its records
    (torch.float32, hip.HLLC, "k_plain_stage<float, 2, 3, false, false, false>"),
    (torch.float64, hip.HLLC, "k_plain_stage<double, 2, 3, false, false, false>"),
], ids=["f32_kepes", "f32_hllc", "f64_hllc"])
def test_fp32_and_hllc_run_as_before(small, dtype, kind, native_kernel):
    a, b, ka, kb = run_pair(small, dtype, planar_state(small), 3, 0.1 * 2.0 ** -7, kind=kind)
    assert kb == native_kernel, kb
    if kind == hip.HLLC:                     # no planar form: the python path's kernel
        assert ka == kb
    assert_same_bits(a, b)
