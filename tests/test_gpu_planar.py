"""The planar form of the 2D patch stage (kernels_fused_patch.hip: PLANAR; stepper.hip: planar_decide) against the general form.

The native stepper proves at the start of a call that the z-momentum planes are all +0 and then runs a stage that neither moves
nor computes that plane; the python-driven iterate() always runs the general form and is the reference here. Every comparison is
on the raw bits (-0.0 != +0.0) of all 25 state planes over the owned slots and of the speed estimates.

Mesh: SynthMesh(2, 5, 7, band=0.13) -- 9 856 quadrilaterals on levels 5-7, 24 patches of 16 x 16 and 39 generic tiles with hanging
faces between them (one mixed launch per stage); band=0.125 gives 12 patches beside 58 generic tiles (patch and generic tiles in
launches of their own)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from t8gpu_amd import hip
from t8gpu_amd.solver import PlainSolver
from t8gpu_amd.synth import SynthMesh

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
DT = 0.1 * 2.0 ** -7
STEPS = 3
_BITS = {torch.float64: torch.int64, torch.float32: torch.int32}


@pytest.fixture(scope="module", params=[True, False], ids=["periodic", "walled"])
def part(request):
    return SynthMesh(2, 5, 7, band=0.13, periodic=request.param).partition()


def planar_state(part, seed=3, rest=False):
    """A 2D state (z-momentum +0 everywhere) with a random in-plane perturbation, or a fluid at rest."""
    rng = np.random.default_rng(seed)
    n = part.N + part.G
    rho = 1.0 + 0.3 * rng.uniform(-1, 1, n)
    v = np.zeros((2, n)) if rest else 0.4 * rng.standard_normal((2, n))
    p = 1.0 + 0.2 * rng.uniform(-1, 1, n)
    if rest:
        rho[:], p[:] = 1.25, 0.8
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


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(t):
    return t.contiguous().view(_BITS[t.dtype])


def last_kernel():
    """the kernel that carried most of the last stage call's work on this thread (t8gpu_hip_last_stage_kernel); its last template
    argument is PLANAR -- what the LAUNCHER ran, where stepper.planar() is only the stepper's decision"""
    import ctypes as C
    q = hip.lib().t8gpu_hip_last_stage_kernel
    q.restype = C.c_char_p
    return (q() or b"").decode()


def assert_no_planar_kernel():
    """(where the heaviest launch may be a generic-tile kernel of another name: no planar patch kernel carried the stage)"""
    k = last_kernel()
    assert k and not (k.startswith(("k_plain_stage<", "k_plain_patch<")) and k.endswith(", true>")), k


def assert_ran(planar):
    k = last_kernel()
    assert k.startswith("k_plain_stage<") and k.endswith(", true>" if planar else ", false>"), k


def assert_same_bits(a, b):
    assert (a.next, a.prev) == (b.next, b.prev)
    n = a.owned_cells
    assert torch.equal(bits(a.planes[:25, :n]), bits(b.planes[:25, :n]))
    assert torch.equal(bits(a.speed), bits(b.speed))


def make_pair(part, dtype, state, kind=hip.KEPES, mode=2):
    """(python-driven general solver, native-stepper solver) over one state"""
    a = PlainSolver(part, dtype, flux_kind=kind, mode="fused", state=state)
    b = PlainSolver(part, dtype, flux_kind=kind, mode="fused", state=state)
    b.use_native_stepper().set_planar(mode)
    return a, b


def run_pair(a, b, steps=STEPS):
    for _ in range(steps):
        a.iterate(DT)
    b.iterate_steps(steps, DT)
    torch.cuda.synchronize()


def test_mesh_has_patches_and_generic_tiles(part):
    c = PlainSolver(part, torch.float64, mode="fused").plan.c
    patches = sum(c.n_patch_tiles)
    assert c.patch_dim != 3 and patches >= 4 and c.ntiles - patches >= 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_planar_equals_general(part, dtype):
    a, b = make_pair(part, dtype, planar_state(part))
    run_pair(a, b)
    assert b.stepper.planar() == 1
    assert_ran(True)
    assert_same_bits(a, b)
    assert not bits(b.planes[:20, :b.owned_cells])[3::5].any()     # the z-momentum of every step slot: +0


@pytest.mark.parametrize("dtype", DTYPES)
def test_planar_patch_kernel_beside_generic_launch(dtype):
    """few patches among many generic tiles: the patch tiles get a launch of their own (k_plain_patch)"""
    part = SynthMesh(2, 5, 7, band=0.125).partition()
    a, b = make_pair(part, dtype, planar_state(part, 4))
    c = b.plan.c
    assert sum(c.n_patch_tiles) >= 4 and sum(c.n_patch_tiles) * 256 < (c.ntiles - sum(c.n_patch_tiles)) * 128
    run_pair(a, b)
    assert b.stepper.planar() == 1
    assert_same_bits(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["adversarial", "rest"])
def test_signed_zeros_and_equal_neighbours(part, dtype, case):
    st = adversarial_state(part) if case == "adversarial" else planar_state(part, rest=True)
    a, b = make_pair(part, dtype, st)
    run_pair(a, b)
    assert b.stepper.planar() == 1
    assert_ran(True)
    assert_same_bits(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("value", [1e-300, -0.0], ids=["tiny", "minus_zero"])
def test_z_momentum_not_all_plus_zero_runs_general(part, dtype, value):
    planted_z_momentum_runs_general(part, dtype, value, part.N // 2)


def planted_z_momentum_runs_general(part, dtype, value, slot):
    st = planar_state(part)
    st[3, slot] = value if value == 0 or dtype == torch.float64 else 1e-30     # (1e-300 is 0 in fp32)
    a, b = make_pair(part, dtype, st)
    assert bits(b.planes[3, :b.owned_cells]).any()
    run_pair(a, b)
    assert b.stepper.planar() == 0
    assert_ran(False)
    assert_same_bits(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("value", [1e-300, -0.0], ids=["tiny", "minus_zero"])
@pytest.mark.parametrize("slot", ["first", "last"])
def test_z_momentum_in_an_edge_slot_runs_general(part, dtype, value, slot):
    """the same with the value in the first and in the last slot the plan addresses: the ends of the range the reduction reads
    (its head and tail words; tests/test_gpu_planes_or_bits.py has every position of the reduction alone)"""
    assert part.G == 0 and part.N > 2
    planted_z_momentum_runs_general(part, dtype, value, 0 if slot == "first" else part.N + part.G - 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("value", [1e-300, -0.0], ids=["tiny", "minus_zero"])
def test_z_momentum_behind_the_addressed_slots_runs_planar(part, dtype, value):
    """planes with a stride beyond the slots the plan addresses (a solver with spare capacity): a value in the first slot that is
    NOT addressed is no cell's z-momentum. The call runs planar, with the bits of the general form, and leaves the value alone."""
    st = planar_state(part)
    tot = part.N + part.G
    a = PlainSolver(part, dtype, mode="fused", state=st, capacity=tot + 3)
    b = PlainSolver(part, dtype, mode="fused", state=st, capacity=tot + 3)
    b.use_native_stepper().set_planar(2)
    assert b.plan.c.n_slots_addressed == tot and b.planes.shape[1] == tot + 3
    v = value if value == 0 or dtype == torch.float64 else 1e-30
    for s in (a, b):
        for k in range(4):                       # the z-momentum plane of every step slot
            s.planes[5 * k + 3, tot] = v
    planted = bits(b.planes[3, tot:tot + 1]).clone()
    assert planted.item() != 0 and not bits(b.planes[3, :tot]).any()
    run_pair(a, b)
    assert b.stepper.planar() == 1
    assert_ran(True)
    assert_same_bits(a, b)
    for k in range(4):
        assert torch.equal(bits(b.planes[5 * k + 3, tot:tot + 1]), planted)


@pytest.mark.parametrize("dtype", DTYPES)
def test_garbage_in_the_stage_slots(part, dtype):
    a, b = make_pair(part, dtype, planar_state(part))
    for s in (1, 2, 3):                    # Step1, Step2 and the next slot of the first step (the state is in slot 0)
        b.planes[5 * s + 3] = float("nan")
    run_pair(a, b)
    assert b.stepper.planar() == 1
    assert_ran(True)
    assert_same_bits(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_state_changed_between_calls(part, dtype):
    a, b = make_pair(part, dtype, planar_state(part))
    run_pair(a, b, 2)
    assert b.stepper.planar() == 1
    assert_ran(True)
    assert_same_bits(a, b)
    for s in (a, b):
        s.state()[3, 17] = 0.25
    run_pair(a, b, 2)
    assert b.stepper.planar() == 0
    assert_ran(False)
    assert_same_bits(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mode_0_never_planar(part, dtype):
    a, b = make_pair(part, dtype, planar_state(part), mode=0)
    run_pair(a, b)
    assert b.stepper.planar() == 0
    assert_ran(False)
    assert_same_bits(a, b)


def test_auto_mode_skips_the_check_on_small_calls(part):
    """mode 1 (the default): 3 steps x 9 856 elements are far below the threshold -- no check, no synchronisation, general form"""
    a = PlainSolver(part, torch.float64, mode="fused", state=planar_state(part))
    b = PlainSolver(part, torch.float64, mode="fused", state=planar_state(part))
    b.use_native_stepper()
    run_pair(a, b)
    assert b.stepper.planar() == 0
    assert_same_bits(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_launcher_falls_back_for_hll(part, dtype):
    a, b = make_pair(part, dtype, planar_state(part), kind=hip.HLL)
    run_pair(a, b)
    assert_no_planar_kernel()
    assert_same_bits(a, b)
    # and a planar request handed straight to the launcher is ignored for HLL: same bits as the plain entry point
    import ctypes as C
    c, d = (PlainSolver(part, dtype, flux_kind=hip.HLL, mode="fused", state=planar_state(part)) for _ in range(2))
    for s, planar in ((c, None), (d, 1)):
        args = [s.kind, 1, C.byref(s.plan.c), 0, s.plan.c.ntiles, s.get_own_variables(0), s.get_own_variables(0), s.get_own_variables(1),
                hip.ptr(s.planes[25]), hip.fscalar(dtype, DT), hip.ptr(s.speed), hip.stream_ptr()]
        if planar is None:
            hip.call("t8gpu_hip_plain_fused_stage", dtype, *args)
        else:
            hip.call("t8gpu_hip_plain_fused_stage_planar", dtype, *args, C.c_int(planar))
            assert_no_planar_kernel()
    torch.cuda.synchronize()
    assert torch.equal(bits(c.planes[:25]), bits(d.planes[:25])) and torch.equal(bits(c.speed), bits(d.speed))


# ---- open boundaries: never planar ------------------------------------------------------------------------------------------------
# The generic tiles of a launch evaluate inflow and far-field faces against a prescribed state, which may carry a z-momentum (a
# 2.5D setup). The initial z-plane is all +0, so the reduction alone would pass; stage 1 then writes a z-momentum beside the
# boundary which planar stages 2 and 3 would never read. Plans with open faces therefore run the general form in every mode.
def _open_states():
    rows = [(1.0, (0.3, 0.0, 0.2), 1.0), (1.2, (0.4, 0.1, -0.15), 1.1)]       # both carry a z-velocity
    return np.array([[rho, rho * v[0], rho * v[1], rho * v[2], p / 0.4 + 0.5 * rho * sum(c * c for c in v)] for rho, v, p in rows])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sides", [(0, "outflow", "periodic", "periodic"), (0, ("farfield", 1), "wall", "wall"),
                                   ("outflow", "outflow", "periodic", "periodic")], ids=["inflow_outflow", "inflow_farfield", "outflow"])
def test_open_boundaries_run_general(dtype, sides):
    part = SynthMesh(2, 5, 7, band=0.13, sides=sides).partition()
    st = planar_state(part)
    states = _open_states() if sides[0] == 0 else None
    a = PlainSolver(part, dtype, mode="fused", state=st, inflow_states=states)
    b = PlainSolver(part, dtype, mode="fused", state=st, inflow_states=states)
    b.use_native_stepper().set_planar(2)
    assert sum(b.plan.c.n_patch_tiles) >= 4 and b.plan.c.has_open_faces
    assert not bits(b.planes[3, :b.owned_cells]).any()                       # the check alone would pass
    run_pair(a, b)
    assert b.stepper.planar() == 0
    assert_no_planar_kernel()
    assert_same_bits(a, b)
    if sides[0] == 0:                                                        # the case is the real one: z-momentum came in
        assert bits(b.state()[3]).any()
    # and a planar request handed straight to the launcher is refused for such a plan: the general kernel runs
    import ctypes as C
    args = [b.kind, 1, C.byref(b.plan.c), 0, b.plan.c.ntiles, b.get_own_variables(0), b.get_own_variables(0), b.get_own_variables(1),
            hip.ptr(b.planes[25]), hip.fscalar(dtype, DT), hip.ptr(b.speed), hip.stream_ptr()]
    hip.call("t8gpu_hip_plain_fused_stage_planar", dtype, *args, C.c_int(1))
    torch.cuda.synchronize()
    assert_no_planar_kernel()


# ---- the non-temporal instantiations (what the benchmark's 9.93 M-element plan runs) ------------------------------------------------
# k_plain_stage<T, 0, S, NT = true, OPEN, PLANAR = true> is chosen where the 15 planes of a stage exceed T8GPU_STREAM_MB (default
# 384 MB); the threshold is read once per process, so a child process with 1 MB runs it on a 21 760-element mesh (1.3 MB of fp32
# planes). Same comparison as above: mode 2 against the python-driven general iterate, on the raw bits.
_NT_CHILD = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
import test_gpu_planar as P
from t8gpu_amd import hip
part = P.SynthMesh(2, 6, 8, band=0.07).partition()
for dtype in P.DTYPES:
    for st in (P.planar_state(part), P.adversarial_state(part)):
        a, b = P.make_pair(part, dtype, st)
        c = b.plan.c
        assert sum(c.n_patch_tiles) >= 4 and c.ntiles - sum(c.n_patch_tiles) >= 2
        P.run_pair(a, b)
        assert b.stepper.planar() == 1
        P.assert_same_bits(a, b)
        print("kernel", P.last_kernel())
"""


def test_non_temporal_planar_instantiation(tmp_path):
    script = tmp_path / "nt_child.py"
    script.write_text(_NT_CHILD)
    res = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=280,
                         env=dict(os.environ, T8GPU_STREAM_MB="1"))
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    names = [ln.split(" ", 1)[1] for ln in res.stdout.splitlines() if ln.startswith("kernel ")]
    assert names == ["k_plain_stage<double, 0, 3, true, false, true>"] * 2 + ["k_plain_stage<float, 0, 3, true, false, true>"] * 2, names
