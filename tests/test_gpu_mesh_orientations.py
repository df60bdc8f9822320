"""-m gpu: every kernel tier on meshes refined across EVERY axis (tests/_meshes.py), against the CPU oracle and against each other.

The provider's band meshes refine across the last axis only, so the code that differs by orientation -- the side-cell and
minus-face rounds of the 2D patch body, the per-side halo segments of the 3D patch kernels, the sides of irregular patches, the
per-axis 2:1 recipes of the Subgrid kernels, the hanging-face rows of the generic tile kernels, ghost classes cut through an
x-oriented level interface -- never met a level interface in x (or y, in 3D) in the other GPU tests. Here it does. Every test
first asserts the plan form it claims to exercise, then compares: within TOL1 / TOL10 of the oracle (tests/_gpu.py), bit for bit
between the tiers where the other tests are bit for bit. A failure names the worst cell, its tile kind and the orientation of its
hanging faces (_meshes.worst_cell_report)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _meshes as M
import _oracle as O
from _gpu import NP, TOL1, TOL10, perturbed_state, rel_err
from t8gpu_amd import hip
from t8gpu_amd.solver import PlainSolver, SubgridSolver

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DTYPES = [torch.float64, torch.float32]
KINDS = [hip.KEPES, hip.HLL, hip.HLLC]
SEED = 31


def last_kernel():
    """the kernel that carried most of the last stage call's work on this thread (t8gpu_hip_last_stage_kernel)"""
    q = hip.lib().t8gpu_hip_last_stage_kernel
    q.restype = C.c_char_p
    return (q() or b"").decode()


# ---- shared fixtures: partitions, states and oracle runs are made once and never changed ---------------------------------------
@functools.lru_cache(maxsize=None)
def part_of(name, periodic=True, sides=None):
    return M.partition(name, periodic=periodic, sides=sides)


@functools.lru_cache(maxsize=None)
def state_of(name, periodic=True, sides=None, planar=False):
    """perturbed_state of the whole mesh; planar: with the z-velocity set to zero (z-momentum +0 everywhere)"""
    st = perturbed_state(part_of(name, periodic, sides), SEED)
    if planar:
        st[4] -= 0.5 * st[3] ** 2 / st[0]
        st[3] = 0.0
    return st


def step_size(name):
    finest = M.SHAPES[name][2]
    return 0.1 * 2.0 ** -(finest + (2 if M.is_subgrid(name) else 0))


@functools.lru_cache(maxsize=None)
def oracle_run(name, periodic, kind, dtype, steps, planar=False):
    """{n: (state after n steps, speed estimates after n steps)} for n in `steps`, by O.PlainCase / O.SubgridCase"""
    part = part_of(name, periodic)
    case = (O.SubgridCase if M.is_subgrid(name) else O.PlainCase)(part, NP[dtype], state=state_of(name, periodic, planar=planar))
    cells = part.N * part.cells_per_element
    out, dt = {}, step_size(name)
    for n in range(1, max(steps) + 1):
        case.iterate(dt, kind=kind)
        if n in steps:
            out[n] = (case.current()[:, :cells].copy(), None if M.is_subgrid(name) else case.speed.copy())
    return out


def assert_close(part, solver, want, tol, what):
    got = solver.state().cpu().numpy()
    err = rel_err(got, want)
    assert err < tol, f"{what}: rel err {err:.3e} (bound {tol:g}). " + M.worst_cell_report(part, got, want, solver.plan.host if solver.plan else None)


def assert_speeds_close(solver, want, tol, what):
    part = solver.part
    err = rel_err(solver.speed.cpu().numpy()[None, :part.F + part.B], want[None])
    assert err < tol, f"{what}: speed estimates rel err {err:.3e} (bound {tol:g})"


def assert_same_bits(part, a, b, what):
    """states (and, on plain solvers, speed estimates) of a and b, bit for bit"""
    if not torch.equal(a.state(), b.state()):
        raise AssertionError(f"{what}: states differ. " + M.worst_cell_report(part, a.state().cpu().numpy(), b.state().cpu().numpy(), a.plan.host))
    if hasattr(a, "speed"):
        diff = torch.nonzero(a.speed != b.speed).flatten()
        assert diff.numel() == 0, f"{what}: {diff.numel()} speed estimates differ, first face {int(diff[0])}"


def plain(name, periodic, dtype, kind, planar=False, mode="fused", **plan_options):
    return PlainSolver(part_of(name, periodic), dtype, flux_kind=kind, mode=mode, state=state_of(name, periodic, planar=planar),
                       plan_options=plan_options if mode == "fused" else None)


def assert_patch_form(solver, name, sides):
    """the 2D patch plan the test claims: patches beside generic tiles, some patch with a coarser element across each of `sides`"""
    h = solver.plan.host
    assert h.patch_dim == 2 and 0 < h.n_patches < h.ntiles and sum(h.n_irregular_class) == 0
    coarse = M.patch_coarse_sides(h, solver.part)
    assert all(coarse[s] > 0 for s in sides), (name, coarse)


# ---- plain 2D ---------------------------------------------------------------------------------------------------------------------
MESHES2 = [("box2", True), ("box2", False), ("xband2", True), ("corner2", True), ("corner2", False)]
COARSE2 = {"box2": ("+x", "+y"), "xband2": ("+x",), "corner2": ("+x", "+y")}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,periodic", MESHES2)
def test_patch_and_tile_plans_vs_oracle_and_bitwise_each_other(name, periodic, kind, dtype):
    """The body of test_patch_kernel_vs_oracle_and_bitwise_vs_tile_kernels where patches have coarser elements across +x (and
    +y): patch plan (k_plain_patch beside the generic tiles) and tile plan each against the oracle, and bit for bit each other."""
    part = part_of(name, periodic)
    a = plain(name, periodic, dtype, kind, patches=True)
    b = plain(name, periodic, dtype, kind, patches=False)
    assert_patch_form(a, name, COARSE2[name])
    assert b.plan.host.n_patches == 0
    want = oracle_run(name, periodic, kind, dtype, (1, 3, 10))
    dt = step_size(name)
    a.iterate(dt)
    b.iterate(dt)
    torch.cuda.synchronize()
    for s, what in ((a, "patch plan"), (b, "tile plan")):
        assert_close(part, s, want[1][0], TOL1[dtype], what + ", 1 step")
        assert_speeds_close(s, want[1][1], TOL1[dtype] * 10, what)
    assert_same_bits(part, a, b, "patch plan vs tile plan, 1 step")
    assert (a.planes[20:25] == 0).all()
    for _ in range(9):
        a.iterate(dt)
        b.iterate(dt)
    torch.cuda.synchronize()
    for s, what in ((a, "patch plan"), (b, "tile plan")):
        assert_close(part, s, want[10][0], TOL10[dtype], what + ", 10 steps")
    assert_same_bits(part, a, b, "patch plan vs tile plan, 10 steps")


def iterate_in_pieces(g, dt, cuts, expect):
    """One step of g as partial launches [cuts[i], cuts[i + 1]) of every stage (what a class-split multi-rank stage launches:
    never a persistent grid), each asked for the kernel it ran: expect[i] is the start of its noted name."""
    s = hip.stream_ptr()
    g.begin_step()
    for k in range(3):
        src, dst = g.stage_steps(k)
        for lo, hi, name in zip(cuts[:-1], cuts[1:], expect):
            g.plan.stage(g, k + 1, src, dst, dt, s, tile_begin=lo, tile_count=hi - lo)
            assert last_kernel().startswith(name), (last_kernel(), name)


FORMS = [("k_plain_stage", dict(tmax=256)),                                  # patches + generic tiles in one launch
         ("k_plain_patch", dict(dictionary=False)),                          # (the mixed kernel needs a dictionary)
         ("k_plain_fused_p", dict(patches=False)),
         ("k_plain_fused", dict(compressed=False, patches=False))]           # CSR lists


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("expect,options", FORMS, ids=[f[0] for f in FORMS])
def test_launch_forms_on_box2(expect, options, dtype):
    """Every launch form of the plain 2D stage on box2, asserted by the name the launcher notes, against the oracle; all forms
    give the bits of the default plan."""
    part = part_of("box2")
    assert all(n > 0 for n in M.hanging_by_axis(part))
    g = plain("box2", True, dtype, hip.KEPES, **options)
    ref = plain("box2", True, dtype, hip.KEPES)
    h = g.plan.host
    assert (h.n_patches > 0) == ("patches" not in options)
    if "patches" not in options:
        assert_patch_form(g, "box2", COARSE2["box2"])
    dt = step_size("box2")
    if expect == "k_plain_patch":
        # 9 patches beside 25 generic tiles: the note keeps the heavier launch, the generic one, so the step runs in two
        # launches per stage and each is asked for its name
        iterate_in_pieces(g, dt, [0, h.n_patches, h.ntiles], ["k_plain_patch<", "k_plain_fused_p<"])
        assert ", false, 2," in last_kernel(), last_kernel()                                      # DICT = false: per-face geometry rows
        whole = plain("box2", True, dtype, hip.KEPES, **options)
        whole.iterate(dt)
        torch.cuda.synchronize()
        assert_same_bits(part, g, whole, "k_plain_patch in two launches vs the whole-plan call")
    elif expect == "k_plain_fused_p":
        # (a whole-plan launch of this small plan may go to the persistent tile kernel: partial launches never do)
        iterate_in_pieces(g, dt, [0, h.ntiles // 2, h.ntiles], ["k_plain_fused_p<", "k_plain_fused_p<"])
    else:
        if expect == "k_plain_stage":
            assert h.n_patches * 256 >= (h.ntiles - h.n_patches) * 128          # the launcher's own condition for one launch
        g.iterate(dt)
        torch.cuda.synchronize()
        assert last_kernel().startswith(expect + "<"), last_kernel()
    ref.iterate(dt)
    torch.cuda.synchronize()
    want = oracle_run("box2", True, hip.KEPES, dtype, (1, 3, 10))
    assert_close(part, g, want[1][0], TOL1[dtype], expect)
    assert_speeds_close(g, want[1][1], TOL1[dtype] * 10, expect)
    assert_same_bits(part, g, ref, expect + " vs the default plan")


_PERSISTENT_CHILD = """
import ctypes, sys
import numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_mesh_orientations as T
out = []
for dtype in T.DTYPES:
    g = T.plain("box2", True, dtype, T.hip.KEPES, patches=False)
    g.iterate(T.step_size("box2"))
    torch.cuda.synchronize()
    print("kernel", T.last_kernel())
    out += [g.state().double().cpu().numpy().ravel(), g.speed.double().cpu().numpy()]
np.save(sys.argv[1], np.concatenate(out))
"""


def test_persistent_tile_kernel_on_box2(tmp_path):
    """k_plain_persistent (T8GPU_PERSISTENT=2 T8GPU_PERSISTENT_WGS=3, read once per process: a child) on the generic tiles of
    box2: within TOL1 of the oracle and the bits of the one-tile kernel."""
    assert all(n > 0 for n in M.hanging_by_axis(part_of("box2")))
    script = tmp_path / "child.py"
    script.write_text(_PERSISTENT_CHILD.format(root=ROOT, tests=HERE))
    out = tmp_path / "state.npy"
    res = subprocess.run([sys.executable, str(script), str(out)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, T8GPU_PERSISTENT="2", T8GPU_PERSISTENT_WGS="3"))
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    names = [ln.split(" ", 1)[1] for ln in res.stdout.splitlines() if ln.startswith("kernel ")]
    assert len(names) == 2 and all(n.startswith("k_plain_persistent<") for n in names), names
    got = np.load(out)
    part = part_of("box2")
    here = []
    for dtype in DTYPES:
        b = plain("box2", True, dtype, hip.KEPES, patches=False)
        nt = b.plan.host.ntiles
        iterate_in_pieces(b, step_size("box2"), [0, nt // 2, nt], ["k_plain_fused_p<", "k_plain_fused_p<"])
        torch.cuda.synchronize()
        here += [b.state().double().cpu().numpy().ravel(), b.speed.double().cpu().numpy()]
    assert np.array_equal(got, np.concatenate(here))
    n64 = 5 * part.N
    assert rel_err(got[:n64].reshape(5, -1), oracle_run("box2", True, hip.KEPES, torch.float64, (1, 3, 10))[1][0]) < TOL1[torch.float64]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("options,expect", [(dict(), None), (dict(tmax=256), "k_plain_stage<")], ids=["patch", "stage"])
@pytest.mark.parametrize("name", ["box2", "xband2"])
def test_planar_form_vs_oracle_and_bitwise_the_general_form(name, options, expect, dtype):
    """A state whose z-momentum is +0 everywhere through the planar instantiation (native stepper, mode 2; detected as
    tests/test_gpu_planar.py does: the stepper's decision and the last template argument of the noted kernel): against the
    oracle, and the bits of the general instantiation that the python-driven stages run. Default caps: the patches in a launch
    of their own (k_plain_patch) beside the heavier generic launch, which is the one the note keeps; 256-element tiles: one
    launch (k_plain_stage), asserted by name."""
    part = part_of(name)
    a = plain(name, True, dtype, hip.KEPES, planar=True, **options)
    b = plain(name, True, dtype, hip.KEPES, planar=True, **options)
    assert_patch_form(b, name, COARSE2[name])
    h = b.plan.host
    assert (h.n_patches * 256 >= (h.ntiles - h.n_patches) * 128) == (expect is not None)      # the launcher's condition for one launch
    b.use_native_stepper().set_planar(2)
    assert not b.planes[3, :part.N].contiguous().view(torch.int64 if dtype == torch.float64 else torch.int32).any()      # +0, not -0
    dt = step_size(name)
    want = oracle_run(name, True, hip.KEPES, dtype, (1, 3, 10), planar=True)
    a.iterate(dt)
    b.iterate_steps(1, dt)
    torch.cuda.synchronize()
    assert b.stepper.planar() == 1
    k = last_kernel()
    assert expect is None or (k.startswith(expect) and k.endswith(", true>")), k
    assert_close(part, b, want[1][0], TOL1[dtype], "planar form, 1 step")
    assert_speeds_close(b, want[1][1], TOL1[dtype] * 10, "planar form")
    assert_same_bits(part, a, b, "planar vs general form, 1 step")
    for _ in range(2):
        a.iterate(dt)
    assert not (last_kernel().startswith(("k_plain_stage<", "k_plain_patch<")) and last_kernel().endswith(", true>")), last_kernel()   # general form
    b.iterate_steps(2, dt)
    torch.cuda.synchronize()
    assert b.stepper.planar() == 1
    assert_close(part, b, want[3][0], TOL10[dtype], "planar form, 3 steps")
    assert_same_bits(part, a, b, "planar vs general form, 3 steps")
    bits = torch.int64 if dtype == torch.float64 else torch.int32
    assert torch.equal(a.planes[:25, :part.N].contiguous().view(bits), b.planes[:25, :part.N].contiguous().view(bits))   # (-0.0 != +0.0)
    assert not b.planes[:20, :part.N].contiguous().view(bits)[3::5].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_compat_tier_on_box2(kind, dtype):
    """The reference data flow (face kernel + atomics, RK kernel) on box2: separates a flux-math problem from an addressing one."""
    part = part_of("box2")
    assert all(n > 0 for n in M.hanging_by_axis(part))
    g = plain("box2", True, dtype, kind, mode="compat")
    want = oracle_run("box2", True, kind, dtype, (1, 3, 10))
    dt = step_size("box2")
    g.iterate(dt)
    torch.cuda.synchronize()
    assert_close(part, g, want[1][0], TOL1[dtype], "compat, 1 step")
    assert_speeds_close(g, want[1][1], TOL1[dtype] * 10, "compat")
    for _ in range(9):
        g.iterate(dt)
    torch.cuda.synchronize()
    assert_close(part, g, want[10][0], TOL10[dtype], "compat, 10 steps")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["box2", "xband2"])
def test_partial_launches_and_the_native_stepper_give_the_same_bits(name, dtype):
    """One stage in pieces that cut the patch range and the generic range (what a class-split multi-rank stage launches: one
    patch per workgroup) is bitwise the whole-plan launch; iterate_steps(3) through the C++ step driver is bitwise three
    python-driven steps."""
    part = part_of(name)
    a, b, c, d = (plain(name, True, dtype, hip.KEPES, patches=True) for _ in range(4))
    assert_patch_form(a, name, COARSE2[name])
    dt = step_size(name)
    a.use_native_stepper()
    a.iterate_steps(3, dt)
    for _ in range(3):
        b.iterate(dt)
    torch.cuda.synchronize()
    assert_same_bits(part, a, b, "native stepper vs python-driven stages")
    assert_close(part, a, oracle_run(name, True, hip.KEPES, dtype, (1, 3, 10))[3][0], TOL10[dtype], "native stepper, 3 steps")
    nt, npatch = c.plan.host.ntiles, c.plan.host.n_patches
    cuts = [0, npatch // 3, npatch + (nt - npatch) // 2, nt]
    assert 0 < cuts[1] < npatch < cuts[2] < nt
    s = hip.stream_ptr()
    c.begin_step()
    d.begin_step()
    c.plan.stage(c, 1, c.prev, 1, dt, s)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        d.plan.stage(d, 1, d.prev, 1, dt, s, tile_begin=lo, tile_count=hi - lo)
    torch.cuda.synchronize()
    assert not torch.isnan(c.planes).any() and torch.equal(c.planes, d.planes)


# ---- plain 3D ---------------------------------------------------------------------------------------------------------------------
MESHES3 = [("box3", True), ("box3", False), ("corner3", False)]
COARSE3 = {"box3": M.SIDES3, "corner3": ("+x", "+y", "+z")}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,periodic", MESHES3)
def test_patch3_forms_vs_oracle_and_bitwise_each_other(name, periodic, kind, dtype):
    """8 x 8 x 4 patches with coarser elements across all six sides (corner3: the three + sides, walls on the others): regular
    and irregular patches, regular patches only, tiles only -- bit for bit each other, the first within tolerance of the oracle."""
    part = part_of(name, periodic)
    a = plain(name, periodic, dtype, kind, patches=True, irregular=True)
    b = plain(name, periodic, dtype, kind, patches=True, irregular=False)
    c = plain(name, periodic, dtype, kind, patches=False)
    ha, hb = a.plan.host, b.plan.host
    assert ha.patch_dim == 3 and hb.patch_dim == 3 and c.plan.host.n_patches == 0
    assert 0 < sum(ha.n_irregular_class) < ha.n_patches < ha.ntiles                  # regular AND irregular patches AND tiles
    assert sum(hb.n_irregular_class) == 0 and 0 < hb.n_patches < ha.n_patches
    coarse = M.patch_coarse_sides(ha, part)
    assert all(coarse[s] > 0 for s in COARSE3[name]), coarse
    want = oracle_run(name, periodic, kind, dtype, (1, 10))
    dt = step_size(name)
    for s in (a, b, c):
        s.iterate(dt)
    torch.cuda.synchronize()
    assert_close(part, a, want[1][0], TOL1[dtype], "regular + irregular patches, 1 step")
    assert_speeds_close(a, want[1][1], TOL1[dtype] * 10, "regular + irregular patches")
    assert_same_bits(part, a, b, "irregular=True vs irregular=False, 1 step")
    assert_same_bits(part, a, c, "patches vs tiles, 1 step")
    for _ in range(9):
        for s in (a, b, c):
            s.iterate(dt)
    torch.cuda.synchronize()
    assert_close(part, a, want[10][0], TOL10[dtype], "regular + irregular patches, 10 steps")
    assert_same_bits(part, a, b, "irregular=True vs irregular=False, 10 steps")
    assert_same_bits(part, a, c, "patches vs tiles, 10 steps")


def test_patch3_kernels_are_the_ones_that_run_on_box3():
    """The launcher's note. A whole-plan call launches the regular and the irregular patches one after the other (the combined
    kernel takes only plans with two resident grids of patches: full-size meshes), and with 256-element, 768-face tiles the 13
    irregular patches outweigh the generic launch, so the note keeps theirs; partial ranges run each kind alone."""
    part = part_of("box3")
    a = plain("box3", True, torch.float64, hip.KEPES, patches=True, irregular=True, tmax=256, fcap=768)
    ref = plain("box3", True, torch.float64, hip.KEPES, patches=False)
    h = a.plan.host
    n_irr, dt = sum(h.n_irregular_class), step_size("box3")
    assert 0 < h.n_patches - n_irr < n_irr and h.ntiles - h.n_patches < n_irr
    a.iterate(dt)
    assert last_kernel().startswith("k_plain_patch3<") and ", true," in last_kernel(), last_kernel()        # IRR = true
    ref.iterate(dt)
    torch.cuda.synchronize()
    assert_same_bits(part, a, ref, "256-element tiles with both patch kinds vs tiles")
    s = hip.stream_ptr()
    a.begin_step()
    a.plan.stage(a, 1, a.prev, 1, dt, s, tile_begin=0, tile_count=h.n_patches - n_irr)
    assert last_kernel().startswith("k_plain_patch3<") and ", false," in last_kernel(), last_kernel()
    a.plan.stage(a, 1, a.prev, 1, dt, s, tile_begin=h.n_patches - n_irr, tile_count=n_irr)
    assert last_kernel().startswith("k_plain_patch3<") and ", true," in last_kernel(), last_kernel()
    torch.cuda.synchronize()


# ---- Subgrid ----------------------------------------------------------------------------------------------------------------------
SMESHES = [("sbox2", True), ("sbox3", True), ("scorner3", False), ("scorner3", True)]


def subgrid(name, periodic, dtype, kind, mode="fused"):
    return SubgridSolver(part_of(name, periodic), dtype, flux_kind=kind, mode=mode, state=state_of(name, periodic))


def assert_subgrid_form(solver):
    """families and single blocks, 2:1 block faces across every axis"""
    h = solver.plan.host
    assert h.n_families > 0 and h.n_rest > 0
    assert all(n > 0 for n in M.hanging_by_axis(solver.part))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,periodic", SMESHES)
def test_fused_subgrid_kernels_vs_oracle(name, periodic, kind, dtype):
    """The body of test_fused_block_kernel_vs_oracle with 2:1 block faces across every axis: the family kernel's pooled outward
    cells and the block kernel's level_diff / nb_offset sub-face map in x and y as well."""
    part = part_of(name, periodic)
    g = subgrid(name, periodic, dtype, kind)
    assert_subgrid_form(g)
    want = oracle_run(name, periodic, kind, dtype, (1, 5))
    dt = step_size(name)
    g.iterate(dt)
    torch.cuda.synchronize()
    assert last_kernel().startswith("k_subgrid_family<" if part.mesh.dim == 3 else "k_subgrid_family2<"), last_kernel()
    assert_close(part, g, want[1][0], TOL1[dtype], "fused, 1 step")
    assert (g.planes[20:25] == 0).all()
    for _ in range(4):
        g.iterate(dt)
    torch.cuda.synchronize()
    assert_close(part, g, want[5][0], TOL10[dtype], "fused, 5 steps")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_compat_subgrid_tier_on_sbox3(kind, dtype):
    """The reference data flow (inner, boundary, outer with the 2:1 map, RK kernels) with 2:1 block faces across every axis."""
    part = part_of("sbox3")
    g = subgrid("sbox3", True, dtype, kind, mode="compat")
    assert all(n > 0 for n in M.hanging_by_axis(part))
    want = oracle_run("sbox3", True, kind, dtype, (1, 5))
    dt = step_size("sbox3")
    g.iterate(dt)
    torch.cuda.synchronize()
    assert_close(part, g, want[1][0], TOL1[dtype], "compat, 1 step")
    for _ in range(4):
        g.iterate(dt)
    torch.cuda.synchronize()
    assert_close(part, g, want[5][0], TOL10[dtype], "compat, 5 steps")


_SWITCH_CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_mesh_orientations as T
out = []
for name, periodic in T.SMESHES:
    for dtype in T.DTYPES:
        for kind in T.KINDS:
            g = T.subgrid(name, periodic, dtype, kind)
            T.assert_subgrid_form(g)
            for _ in range(3):
                g.iterate(T.step_size(name))
            torch.cuda.synchronize()
            print("kernel", name, T.last_kernel())
            out.append(g.state().double().cpu().numpy().ravel())
np.save(sys.argv[1], np.concatenate(out))
"""


def test_family_block_and_wide_addressing_agree_bitwise(tmp_path):
    """What test_family_kernel_and_block_kernel_agree_bitwise and test_32_bit_and_64_bit_plane_addressing_agree_bitwise do, on
    2:1 block faces across every axis: the family kernels (default), every block through the block kernel (T8GPU_SG_FAMILY=0)
    and 64-bit plane offsets (T8GPU_SG_WIDE=1) give the same bits. Child processes: the switches are read once."""
    script = tmp_path / "child.py"
    script.write_text(_SWITCH_CHILD.format(root=ROOT, tests=HERE))
    res, names = {}, {}
    for tag, env in (("default", {}), ("block", dict(T8GPU_SG_FAMILY="0")), ("wide", dict(T8GPU_SG_WIDE="1"))):
        out = tmp_path / f"state_{tag}.npy"
        env = dict({k: v for k, v in os.environ.items() if k not in ("T8GPU_SG_FAMILY", "T8GPU_SG_WIDE")}, **env)
        run = subprocess.run([sys.executable, str(script), str(out)], capture_output=True, text=True, timeout=180, env=env)
        assert run.returncode == 0, (tag, run.stdout[-1500:] + run.stderr[-3000:])
        res[tag] = np.load(out)
        names[tag] = [ln.split(" ", 2)[2] for ln in run.stdout.splitlines() if ln.startswith("kernel ")]
        assert len(names[tag]) == len(SMESHES) * len(DTYPES) * len(KINDS)
    # each child ran what its switch asks for: k_subgrid_family[2]<T, K, S, WIDE, NT>, k_subgrid_fused<T, K, S, R, early, WIDE>
    args = lambda n: n[n.index("<") + 1:-1].split(", ")
    assert all(n.startswith("k_subgrid_family") and args(n)[3] == "false" for n in names["default"]), names["default"][:3]
    assert all(n.startswith("k_subgrid_fused<") and args(n)[5] == "false" for n in names["block"]), names["block"][:3]
    assert all(n.startswith("k_subgrid_family") and args(n)[3] == "true" for n in names["wide"]), names["wide"][:3]
    assert np.isfinite(res["default"]).all()
    for tag in ("block", "wide"):
        assert np.array_equal(res["default"], res[tag]), (tag, int((res["default"] != res[tag]).sum()))


# ---- partitions ---------------------------------------------------------------------------------------------------------------------
# (name, ranks). The 3-way split of box2 and sbox2 cuts the fine box inside and along its symmetry lines only: no ghost lies
# across a hanging face with normal x there (pinned below and in tests/test_mesh_shapes.py); their 5-way split has such ghosts.
NO_X_GHOSTS = {("box2", 3), ("sbox2", 3)}


def _poisoned_ranks(name, world, make_solver):
    from t8gpu_amd.halo import HaloExchange
    mesh, S = M.shape(name), 4 ** M.SHAPES[name][0] if M.is_subgrid(name) else 1
    st = state_of(name)
    parts = [mesh.partition(r, world, subgrid=M.is_subgrid(name)) for r in range(world)]
    ghosts_x = sum(M.ghost_hanging_faces(p, axis=0) for p in parts)
    assert (ghosts_x == 0) if (name, world) in NO_X_GHOSTS else (ghosts_x > 0), ghosts_x
    solvers, halos = [], []
    for part in parts:
        elems = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
        cells = (elems[:, None] * S + np.arange(S)[None, :]).reshape(-1)
        local = st[:, cells].copy()
        local[:, part.N * S:] = np.nan                              # ghost values must arrive through the exchange
        solvers.append(make_solver(part, local))
        halos.append(HaloExchange(part, torch.float64, dist=None, overlap=False))
    return parts, solvers, halos


def _split_steps(ref, solvers, halos, dt, steps=3):
    from test_gpu_halo import loopback
    for _ in range(steps):
        ref.iterate(dt)
        for s in solvers:
            s.begin_step()
        for k in range(3):
            for s, h in zip(solvers, halos):
                h._pack(s.step_planes(s.stage_steps(k)[0]))
            loopback(halos)
            for s, h in zip(solvers, halos):
                h._unpack(s.step_planes(s.stage_steps(k)[0]))
            for s in solvers:
                s.run_stage(k, dt, split=True)
    torch.cuda.synchronize()
    full = torch.cat([s.state() for s in solvers], dim=1)
    assert not torch.isnan(full).any()
    return full


@pytest.mark.parametrize("name,world", [("box2", 3), ("box2", 5), ("xband2", 3), ("box3", 3)])
def test_plain_partition_through_level_interfaces_is_bitwise_the_single_rank_run(name, world):
    """An SFC split with patches on the ranks and ghosts across hanging faces with normal x, through the loopback transport of
    tests/test_gpu_halo.py, ghost slots poisoned with NaN before the first exchange: three steps with split stages are bitwise
    the single-rank run without patches."""
    ref = plain(name, True, torch.float64, hip.KEPES, patches=False)
    parts, solvers, halos = _poisoned_ranks(name, world, lambda part, local: PlainSolver(
        part, torch.float64, mode="fused", state=local, plan_options=dict(patches=True, irregular=True)))
    with_patches = [s.plan.host.n_patches > 0 for s in solvers]
    assert all(with_patches) if world == 3 else any(with_patches), with_patches
    assert any(0 < s.plan.host.n_interior < s.plan.host.ntiles for s in solvers)
    assert sum(s.plan.host.n_patch_class[1] + s.plan.host.n_patch_class[2] for s in solvers) > 0   # not only deep patches
    full = _split_steps(ref, solvers, halos, step_size(name))
    assert torch.equal(full, ref.state())
    assert_close(part_of(name), ref, oracle_run(name, True, hip.KEPES, torch.float64, (1, 3, 10))[3][0], TOL10[torch.float64], "single rank")


@pytest.mark.parametrize("name,world", [("sbox2", 3), ("sbox2", 5), ("sbox3", 3)])
def test_subgrid_partition_through_level_interfaces_is_bitwise_the_single_rank_run(name, world):
    ref = subgrid(name, True, torch.float64, hip.KEPES)
    assert_subgrid_form(ref)
    parts, solvers, halos = _poisoned_ranks(name, world, lambda part, local: SubgridSolver(part, torch.float64, mode="fused", state=local))
    assert any(0 < s.plan.host.n_interior < s.N for s in solvers)
    full = _split_steps(ref, solvers, halos, step_size(name))
    assert torch.equal(full, ref.state())


# ---- one open-boundary case -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sides", ["x_open", "all_open"])
def test_open_boundaries_on_corner2(sides, kind, dtype):
    """corner2 with the inflow / outflow sides and the inflow state of tests/test_gpu_open_boundaries.py: the fine corner sits on
    the inflow side (x_open: SIDES[2], y periodic -- hanging faces across the y wrap) or on the inflow side and an outflow side
    (all_open). Patch plan and tile plan against that file's composed reference, and bit for bit each other."""
    from test_gpu_open_boundaries import SIDES, OpenCase, inflow_states
    spec = SIDES[2] if sides == "x_open" else (0, "outflow", "outflow", "outflow")
    part = part_of("corner2", True, spec)
    st, inflow = state_of("corner2", True, spec), inflow_states(2)
    finest = part.mesh.finest_level
    on_side = np.asarray(part.face_neighbors).reshape(-1)[2 * part.F:]
    kinds = np.asarray(part.boundary_kinds)
    assert (part.levels[on_side[kinds == 2]] == finest).any()                          # fine cells on the inflow side
    if sides == "all_open":
        assert (part.levels[on_side[kinds == 1]] == finest).any()                      # ... and on an outflow side
    a = PlainSolver(part, dtype, flux_kind=kind, mode="fused", state=st, inflow_states=inflow, plan_options=dict(patches=True))
    b = PlainSolver(part, dtype, flux_kind=kind, mode="fused", state=st, inflow_states=inflow, plan_options=dict(patches=False))
    assert a.plan.host.n_patches > 0 and b.plan.host.n_patches == 0 and a.plan.c.has_open_faces and b.plan.c.has_open_faces
    assert all(n > 0 for n in M.hanging_by_axis(part))
    o = OpenCase(part, NP[dtype], st, inflow)
    dt = step_size("corner2")
    a.iterate(dt)
    b.iterate(dt)
    o.iterate(dt, kind)
    torch.cuda.synchronize()
    for s, what in ((a, "patch plan"), (b, "tile plan")):
        assert_close(part, s, o.current()[:, :part.N], TOL1[dtype], what + ", open boundaries")
        assert_speeds_close(s, o.speed, TOL1[dtype], what + ", open boundaries")
    assert_same_bits(part, a, b, "patch plan vs tile plan, open boundaries")
