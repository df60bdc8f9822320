"""-m gpu: every kernel tier on Cartesian meshes whose areas and volumes are NO powers of two (tests/_meshes.py: scaled).

SynthMesh meshes the unit square / cube: every area and volume the other GPU tests hand to a Cartesian kernel is a power of two,
so multiplying by an area and dividing by a volume never rounded there. Here the same forests (box2, box3, sbox2, sbox3: the
smallest shapes on which every plan form exists) are boxes with edges 3.7 and 1/3 (isotropic: the plan form of the unit mesh,
patches of uniform volume whose rk_scale divides), stretched boxes (per-axis factors: no patch, every element through the
generic tiles), and boxes with edges 2^-12 and 2^9 (a change of length unit that must give back the bits of the unit run). Every
test asserts the plan form it claims first, then compares: against the oracle on the SAME scaled arrays within TOL1 / TOL10
(tests/_gpu.py; tests/test_scaled_meshes_host.py pins that the oracle itself moves by rounding only), and bit for bit between
the tiers that are bit for bit on the unit mesh. Worst errors are printed before they are asserted (FIG lines, pytest -s)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _meshes as M
import _oracle as O
import test_gpu_mesh_orientations as T
from _gpu import NP, TOL1, TOL10, rel_err
from t8gpu_amd import hip
from t8gpu_amd.solver import PlainSolver, SubgridSolver

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DTYPES, KINDS = T.DTYPES, T.KINDS
NON_DYADIC = [3.7, 1 / 3]
POW2 = [2.0 ** -12, 2.0 ** 9]
STRETCH = {"box2": (1, 0.37), "box3": (1, 0.37, 2.9)}
SCALE_ID = {3.7: "x3.7", 1 / 3: "x1/3", 2.0 ** -12: "x2^-12", 2.0 ** 9: "x2^9"}.get


def fig(what, value, bound=None):
    print(f"FIG {what}: {value:.3e}" + ("" if bound is None else f" (bound {bound:g})"))


# ---- shared fixtures: partitions, states and oracle runs are made once and never changed ---------------------------------------
@functools.lru_cache(maxsize=None)
def part_of(name, s=None, periodic=True, sides=None):
    base = T.part_of(name, periodic, sides)
    return base if s is None else M.scaled(base, s)


def step_size(name, s=None):
    """0.1 * 2^-(finest level, + 2 for Subgrid) * min(s)"""
    return T.step_size(name) * (1.0 if s is None else float(np.min(s)))


@functools.lru_cache(maxsize=None)
def oracle_run(name, s, periodic, kind, dtype, steps, planar=False):
    """{n: (state after n steps, speed estimates after n steps)} on the scaled arrays, by O.PlainCase / O.SubgridCase"""
    part = part_of(name, s, periodic)
    case = (O.SubgridCase if M.is_subgrid(name) else O.PlainCase)(part, NP[dtype], state=T.state_of(name, periodic, planar=planar))
    cells = part.N * part.cells_per_element
    out, dt = {}, step_size(name, s)
    for n in range(1, max(steps) + 1):
        case.iterate(dt, kind=kind)
        if n in steps:
            out[n] = (case.current()[:, :cells].copy(), None if M.is_subgrid(name) else case.speed.copy())
    return out


def plain(name, s, periodic, dtype, kind, planar=False, mode="fused", **plan_options):
    return PlainSolver(part_of(name, s, periodic), dtype, flux_kind=kind, mode=mode, state=T.state_of(name, periodic, planar=planar),
                       plan_options=plan_options if mode == "fused" else None)


def subgrid(name, s, periodic, dtype, kind, mode="fused"):
    return SubgridSolver(part_of(name, s, periodic), dtype, flux_kind=kind, mode=mode, state=T.state_of(name, periodic))


def check_close(solver, want, tol, what, speed_tol=None):
    """state (and speed estimates) of `solver` against the oracle's (state, speeds): printed, then asserted"""
    part = solver.part
    got = solver.state().cpu().numpy()
    err = rel_err(got, want[0])
    fig(what, err, tol)
    assert err < tol, f"{what}: rel err {err:.3e} (bound {tol:g}). " + M.worst_cell_report(part, got, want[0], solver.plan.host if solver.plan else None)
    if speed_tol is not None:
        es = rel_err(solver.speed.cpu().numpy()[None, :part.F + part.B], want[1][None])
        fig(what + ", speed estimates", es, speed_tol)
        assert es < speed_tol, f"{what}: speed estimates rel err {es:.3e} (bound {speed_tol:g})"


def assert_divides(solver):
    """patches of uniform volume (descriptor flag 0x400) whose volume is no power of two: rk_scale takes its division branch"""
    h = solver.plan.host
    assert h.n_patches_uniform_volume > 0
    mant, _ = np.frexp(np.asarray(solver.part.volumes)[:solver.part.N])
    assert (mant != 0.5).all()


def run_tiers(tiers, part, want, dtype, dt, steps=10):
    """tiers {name: solver}: every one within TOL1 of want[1] after one step (speed estimates: 10 TOL1) and TOL10 of
    want[steps] after `steps`, and the bits of the first one at both points"""
    names = list(tiers)
    for done, tol in ((1, TOL1[dtype]), (steps, TOL10[dtype])):
        for g in tiers.values():
            for _ in range(done - (0 if done == 1 else 1)):
                g.iterate(dt)
        torch.cuda.synchronize()
        for n in names:
            check_close(tiers[n], want[done], tol, f"{n}, {done} step(s)", 10 * TOL1[dtype] if done == 1 and hasattr(tiers[n], "speed") else None)
        for n in names[1:]:
            T.assert_same_bits(part, tiers[names[0]], tiers[n], f"{names[0]} vs {n}, {done} step(s)")


# ---- a. plain tiers on an isotropic non-dyadic scale ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("s", NON_DYADIC, ids=SCALE_ID)
def test_box2_tiers_on_a_non_dyadic_scale(s, kind, dtype):
    """2D patch plan (k_plain_patch beside the generic tiles; uniform-volume patches, dividing rk_scale), tile plan and compat
    tier against the oracle; patch plan and tile plan bit for bit."""
    part = part_of("box2", s)
    a = plain("box2", s, True, dtype, kind, patches=True)
    b = plain("box2", s, True, dtype, kind, patches=False)
    c = plain("box2", s, True, dtype, kind, mode="compat")
    T.assert_patch_form(a, "box2", T.COARSE2["box2"])
    assert_divides(a)
    assert b.plan.host.n_patches == 0 and b.plan.host.n_patches_uniform_volume == 0
    want = oracle_run("box2", s, True, kind, dtype, (1, 3, 10))
    dt = step_size("box2", s)
    run_tiers({"patch plan": a, "tile plan": b}, part, want, dtype, dt)
    c.iterate(dt)
    torch.cuda.synchronize()
    check_close(c, want[1], TOL1[dtype], "compat, 1 step", 10 * TOL1[dtype])
    for _ in range(9):
        c.iterate(dt)
    torch.cuda.synchronize()
    check_close(c, want[10], TOL10[dtype], "compat, 10 steps")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", NON_DYADIC, ids=SCALE_ID)
def test_box2_one_launch_stage_kernel_on_a_non_dyadic_scale(s, dtype):
    """256-element tiles: patches and generic tiles in ONE launch (k_plain_stage, the benchmark's kernel form), asserted by
    name; the bits of the default plan."""
    part = part_of("box2", s)
    g = plain("box2", s, True, dtype, hip.KEPES, tmax=256)
    ref = plain("box2", s, True, dtype, hip.KEPES)
    T.assert_patch_form(g, "box2", T.COARSE2["box2"])
    assert_divides(g)
    dt = step_size("box2", s)
    g.iterate(dt)
    torch.cuda.synchronize()
    assert T.last_kernel().startswith("k_plain_stage<"), T.last_kernel()
    ref.iterate(dt)
    torch.cuda.synchronize()
    check_close(g, oracle_run("box2", s, True, hip.KEPES, dtype, (1, 3, 10))[1], TOL1[dtype], "k_plain_stage, 1 step", 10 * TOL1[dtype])
    T.assert_same_bits(part, g, ref, "k_plain_stage vs the default plan")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "walled"])
@pytest.mark.parametrize("s", NON_DYADIC, ids=SCALE_ID)
def test_box3_patch_forms_on_a_non_dyadic_scale(s, periodic, kind, dtype):
    """8 x 8 x 4 patches: regular and irregular, regular only, every patch in the irregular form, tiles only -- each against the
    oracle, bit for bit each other."""
    part = part_of("box3", s, periodic)
    tiers = {"regular + irregular patches": plain("box3", s, periodic, dtype, kind, patches=True, irregular=True),
             "irregular=False": plain("box3", s, periodic, dtype, kind, patches=True, irregular=False),
             "irregular='all'": plain("box3", s, periodic, dtype, kind, patches=True, irregular="all"),
             "tile plan": plain("box3", s, periodic, dtype, kind, patches=False)}
    ha, hb, hc, hd = (g.plan.host for g in tiers.values())
    assert ha.patch_dim == 3 and hb.patch_dim == 3 and hc.patch_dim == 3 and hd.n_patches == 0
    assert 0 < sum(ha.n_irregular_class) < ha.n_patches < ha.ntiles                  # regular AND irregular patches AND tiles
    assert sum(hb.n_irregular_class) == 0 and 0 < hb.n_patches < ha.n_patches
    assert sum(hc.n_irregular_class) == hc.n_patches == ha.n_patches
    assert_divides(tiers["regular + irregular patches"])
    want = oracle_run("box3", s, periodic, kind, dtype, (1, 10))
    run_tiers(tiers, part, want, dtype, step_size("box3", s))


# ---- b. plain tiers on stretched boxes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["box2", "box3"])
def test_stretched_boxes_run_generic_tiles_only(name, kind, dtype):
    """Per-axis factors: a patch carries one area, so the planner leaves none (pinned on the host too: a planner that learns
    per-axis areas changes this knowingly). The plan asked for patches, the plan asked for none (both: generic tiles) and the
    compat tier against the oracle; the two fused plans bit for bit."""
    s = STRETCH[name]
    part = part_of(name, s)
    a = plain(name, s, True, dtype, kind, patches=True)
    b = plain(name, s, True, dtype, kind, patches=False)
    c = plain(name, s, True, dtype, kind, mode="compat")
    for g in (a, b):
        assert g.plan.host.n_patches == 0 and g.plan.host.patch_dim == 0 and g.plan.host.ntiles > 1
    assert all(n > 0 for n in M.hanging_by_axis(part))
    ratios = np.unique(np.round(np.asarray(part.areas) / np.asarray(T.part_of(name).areas), 12))
    assert len(ratios) == part.mesh.dim and (np.frexp(np.asarray(part.volumes))[0] != 0.5).all()       # one area factor per axis
    want = oracle_run(name, s, True, kind, dtype, (1, 10))
    dt = step_size(name, s)
    run_tiers({"generic tiles (patches asked for)": a, "generic tiles": b}, part, want, dtype, dt)
    c.iterate(dt)
    torch.cuda.synchronize()
    check_close(c, want[1], TOL1[dtype], "compat, 1 step", 10 * TOL1[dtype])
    for _ in range(9):
        c.iterate(dt)
    torch.cuda.synchronize()
    check_close(c, want[10], TOL10[dtype], "compat, 10 steps")


# ---- persistent kernel always / never, on scaled and stretched boxes (the switch is read once per process: children) -------------
PERSISTENT_CASES = [("box2", 3.7), ("box2", 1 / 3), ("box2", STRETCH["box2"]), ("box3", 3.7), ("box3", STRETCH["box3"])]

_PERSISTENT_CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_scaled_geometry as G
np.save(sys.argv[1], G.persistent_cases(True))
"""


def persistent_cases(names=False):
    """three steps of the tile plan (every tile generic: the persistent kernel's) on PERSISTENT_CASES, KEPES and HLL, both
    types: states and speed estimates in one array; each whole-plan launch's kernel printed"""
    out = []
    for name, s in PERSISTENT_CASES:
        for dtype in DTYPES:
            for kind in (hip.KEPES, hip.HLL):
                g = plain(name, s, True, dtype, kind, patches=False)
                for _ in range(3):
                    g.iterate(step_size(name, s))
                torch.cuda.synchronize()
                if names:
                    print("kernel", T.last_kernel())
                out += [g.state().double().cpu().numpy().ravel(), g.speed.double().cpu().numpy()]
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def persistent_cases_here():
    """persistent_cases() of this process (whatever kernel its launcher chooses): made once, never changed"""
    return persistent_cases()


@pytest.mark.parametrize("mode", ["2", "0"], ids=["always", "never"])
def test_persistent_switch_on_scaled_and_stretched_boxes(mode, tmp_path):
    """T8GPU_PERSISTENT=2 (k_plain_persistent, asserted by name) / =0 (the one-tile kernels) on scaled and stretched boxes, in
    a child process: the bits of this process's run of the same cases -- so always = never = default."""
    script = tmp_path / "child.py"
    script.write_text(_PERSISTENT_CHILD.format(root=ROOT, tests=HERE))
    out = tmp_path / "state.npy"
    run = subprocess.run([sys.executable, str(script), str(out)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, T8GPU_PERSISTENT=mode, T8GPU_PERSISTENT_WGS="3"))
    assert run.returncode == 0, (mode, run.stdout[-1500:] + run.stderr[-3000:])
    got = np.load(out)
    kernels = [ln.split(" ", 1)[1] for ln in run.stdout.splitlines() if ln.startswith("kernel ")]
    assert len(kernels) == len(PERSISTENT_CASES) * 4
    assert all(k.startswith("k_plain_persistent<") == (mode == "2") for k in kernels), (mode, kernels)
    here = persistent_cases_here()
    assert np.isfinite(got).all() and got.shape == here.shape
    assert np.array_equal(got, here), int((got != here).sum())


def test_persistent_cases_vs_oracle():
    """the run the two switch cases are held against: within TOL10 of the oracle after three steps"""
    res = persistent_cases_here()
    at = 0
    for name, s in PERSISTENT_CASES:
        part = part_of(name, s)
        for dtype in DTYPES:
            for kind in (hip.KEPES, hip.HLL):
                want = oracle_run(name, s, True, kind, dtype, (1, 3, 10) if name == "box2" and not isinstance(s, tuple) else (1, 3))[3]
                got = res[at:at + 5 * part.N].reshape(5, part.N)
                at += 5 * part.N + part.F + part.B
                err = rel_err(got, want[0])
                fig(f"tile plan, {name} x {s}, {dtype}, flux {kind}, 3 steps", err, TOL10[dtype])
                assert err < TOL10[dtype], (name, s, dtype, kind, err)
    assert at == res.size


# ---- c. a power-of-two scale gives back the bits of the unit run ------------------------------------------------------------------
def _three_steps(g, dt):
    for _ in range(3):
        g.iterate(dt)
    torch.cuda.synchronize()
    return g


PLAIN_TIERS = {"box2": [dict(patches=True), dict(patches=False), dict(tmax=256)],
               "box3": [dict(patches=True, irregular=True), dict(patches=True, irregular=False), dict(patches=True, irregular="all"),
                        dict(patches=False)]}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["box2", "box3", "sbox2"])
def test_a_power_of_two_scale_gives_the_bits_of_the_unit_run(name, kind, dtype):
    """Lengths * s, dt * s, s = 2^-12 and 2^9: every fused tier gives bitwise the state and the speed estimates of its own
    unit-mesh run after three steps (multiplying by an area and dividing by a volume only move exponents)."""
    options = PLAIN_TIERS.get(name, [dict()])
    make = (lambda s, o: subgrid(name, s, True, dtype, kind)) if M.is_subgrid(name) else (lambda s, o: plain(name, s, True, dtype, kind, **o))
    for o in options:
        unit = _three_steps(make(None, o), step_size(name))
        if o.get("patches", True) and not M.is_subgrid(name):
            assert unit.plan.host.n_patches > 0 and unit.plan.host.n_patches_uniform_volume > 0
        for s in POW2:
            g = _three_steps(make(s, o), step_size(name, s))
            assert np.array_equal(np.asarray(g.part.volumes), np.asarray(unit.part.volumes) * s ** unit.part.mesh.dim)
            if unit.plan.host.__class__.__name__ == "HostPlainPlan":
                assert g.plan.host.n_patches == unit.plan.host.n_patches and g.plan.host.ntiles == unit.plan.host.ntiles
            T.assert_same_bits(part_of(name), g, unit, f"{name} x {s} vs the unit mesh, plan {o}")
        if o == options[0]:
            check_close(unit, oracle_run(name, None, True, kind, dtype, (1, 3))[3], TOL10[dtype], f"{name}, unit mesh, 3 steps")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_sbox3_on_a_power_of_two_scale_vs_oracle(kind, dtype):
    """3D Subgrid is excluded from the bit invariance (the oracle's edge is the C library's cbrt(volume), which does not scale
    exactly: tests/test_scaled_meshes_host.py): fused kernels against the oracle on the same arrays, TOL1 / TOL10."""
    for s in POW2:
        g = subgrid("sbox3", s, True, dtype, kind)
        T.assert_subgrid_form(g)
        want = oracle_run("sbox3", s, True, kind, dtype, (1, 5))
        dt = step_size("sbox3", s)
        g.iterate(dt)
        torch.cuda.synchronize()
        check_close(g, want[1], TOL1[dtype], f"sbox3 x {s}, 1 step")
        for _ in range(4):
            g.iterate(dt)
        torch.cuda.synchronize()
        check_close(g, want[5], TOL10[dtype], f"sbox3 x {s}, 5 steps")


# ---- d. planar form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("options,expect", [(dict(), None), (dict(tmax=256), "k_plain_stage<")], ids=["patch", "stage"])
def test_planar_form_on_box2_x37(options, expect, dtype):
    """z-momentum +0 everywhere, native stepper, set_planar(2): the planar instantiation ran (planar() == 1, the noted kernel's
    last template argument), gives the bits of the general form, and is within tolerance of the oracle."""
    s = 3.7
    part = part_of("box2", s)
    a = plain("box2", s, True, dtype, hip.KEPES, planar=True, **options)
    b = plain("box2", s, True, dtype, hip.KEPES, planar=True, **options)
    T.assert_patch_form(b, "box2", T.COARSE2["box2"])
    assert_divides(b)
    a.use_native_stepper().set_planar(0)
    b.use_native_stepper().set_planar(2)
    dt = step_size("box2", s)
    want = oracle_run("box2", s, True, hip.KEPES, dtype, (1, 3), planar=True)
    a.iterate_steps(1, dt)
    assert a.stepper.planar() == 0
    b.iterate_steps(1, dt)
    torch.cuda.synchronize()
    assert b.stepper.planar() == 1
    k = T.last_kernel()
    assert expect is None or (k.startswith(expect) and k.endswith(", true>")), k
    check_close(b, want[1], TOL1[dtype], "planar form, 1 step", 10 * TOL1[dtype])
    T.assert_same_bits(part, a, b, "planar vs general form, 1 step")
    a.iterate_steps(2, dt)
    b.iterate_steps(2, dt)
    torch.cuda.synchronize()
    assert a.stepper.planar() == 0 and b.stepper.planar() == 1
    check_close(b, want[3], TOL10[dtype], "planar form, 3 steps")
    T.assert_same_bits(part, a, b, "planar vs general form, 3 steps")
    bits = torch.int64 if dtype == torch.float64 else torch.int32
    assert not b.planes[:20, :part.N].contiguous().view(bits)[3::5].any()


# ---- e. Subgrid on s = 3.7 ---------------------------------------------------------------------------------------------------------
SUBGRID_CASES = [("sbox2", 3.7), ("sbox3", 3.7)]

_SUBGRID_CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_scaled_geometry as G
np.save(sys.argv[1], G.subgrid_cases(True))
"""


def subgrid_cases(names=False):
    """three fused steps on SUBGRID_CASES, the three fluxes, both types: the states in one array; kernels printed"""
    out = []
    for name, s in SUBGRID_CASES:
        for dtype in DTYPES:
            for kind in KINDS:
                g = subgrid(name, s, True, dtype, kind)
                T.assert_subgrid_form(g)
                _three_steps(g, step_size(name, s))
                if names:
                    print("kernel", T.last_kernel())
                out.append(g.state().double().cpu().numpy().ravel())
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def subgrid_cases_here():
    """subgrid_cases() of this process (the form its environment asks for): made once, never changed"""
    return subgrid_cases()


SWITCHES = {"family": {}, "block": dict(T8GPU_SG_FAMILY="0"), "family wide": dict(T8GPU_SG_WIDE="1"),
            "block wide": dict(T8GPU_SG_FAMILY="0", T8GPU_SG_WIDE="1")}


@pytest.mark.parametrize("tag", list(SWITCHES))
def test_subgrid_block_family_and_wide_addressing_on_x37(tag, tmp_path):
    """Family kernels and block kernels (T8GPU_SG_FAMILY=0), narrow and 64-bit (T8GPU_SG_WIDE=1) plane addressing, on blocks
    whose inner sub-face area (cbrt(vol) / 4 squared, sqrt(vol) / 4) and outer sub-face area (area / SF) agree to rounding
    only. Each form in a child process (the switches are read once), asserted by kernel name, gives the bits of this
    process's run of the same cases: the four forms bit for bit."""
    script = tmp_path / "child.py"
    script.write_text(_SUBGRID_CHILD.format(root=ROOT, tests=HERE))
    args = lambda n: n[n.index("<") + 1:-1].split(", ")
    out = tmp_path / "state.npy"
    env = dict({k: v for k, v in os.environ.items() if k not in ("T8GPU_SG_FAMILY", "T8GPU_SG_WIDE")}, **SWITCHES[tag])
    run = subprocess.run([sys.executable, str(script), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, (tag, run.stdout[-1500:] + run.stderr[-3000:])
    got = np.load(out)
    kernels = [ln.split(" ", 1)[1] for ln in run.stdout.splitlines() if ln.startswith("kernel ")]
    assert len(kernels) == len(SUBGRID_CASES) * len(DTYPES) * len(KINDS)
    # k_subgrid_family[2]<T, K, S, WIDE, NT>, k_subgrid_fused<T, K, S, R, early, WIDE>
    wide = "true" if "wide" in tag else "false"
    if tag.startswith("family"):
        assert all(k.startswith("k_subgrid_family") and args(k)[3] == wide for k in kernels), (tag, kernels[:3])
    else:
        assert all(k.startswith("k_subgrid_fused<") and args(k)[5] == wide for k in kernels), (tag, kernels[:3])
    here = subgrid_cases_here()
    assert np.isfinite(got).all() and got.shape == here.shape
    assert np.array_equal(got, here), (tag, int((got != here).sum()))


def test_subgrid_cases_vs_oracle():
    """the run the four switch cases are held against: within TOL10 of the oracle after three steps"""
    res = subgrid_cases_here()
    at = 0
    for name, s in SUBGRID_CASES:
        part = part_of(name, s)
        cells = part.N * part.cells_per_element
        for dtype in DTYPES:
            for kind in KINDS:
                want = oracle_run(name, s, True, kind, dtype, (1, 3, 5))[3][0]
                err = rel_err(res[at:at + 5 * cells].reshape(5, cells), want)
                at += 5 * cells
                fig(f"fused Subgrid, {name} x {s}, {dtype}, flux {kind}, 3 steps", err, TOL10[dtype])
                assert err < TOL10[dtype], (name, s, dtype, kind, err)
    assert at == res.size


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["fused", "compat"])
@pytest.mark.parametrize("name,s", SUBGRID_CASES + [("sbox3", 1 / 3)], ids=lambda v: SCALE_ID(v) if isinstance(v, float) else v)
def test_subgrid_tiers_on_a_non_dyadic_scale_vs_oracle(name, s, mode, kind, dtype):
    part = part_of(name, s)
    g = subgrid(name, s, True, dtype, kind, mode=mode)
    assert all(n > 0 for n in M.hanging_by_axis(part))
    mant, _ = np.frexp(np.asarray(part.volumes))
    assert (mant != 0.5).all()
    if mode == "fused":
        T.assert_subgrid_form(g)
    want = oracle_run(name, s, True, kind, dtype, (1, 3, 5))
    dt = step_size(name, s)
    g.iterate(dt)
    torch.cuda.synchronize()
    if mode == "fused":
        assert T.last_kernel().startswith("k_subgrid_family<" if part.mesh.dim == 3 else "k_subgrid_family2<"), T.last_kernel()
    check_close(g, want[1], TOL1[dtype], f"{mode}, {name} x {s}, 1 step")
    for _ in range(4):
        g.iterate(dt)
    torch.cuda.synchronize()
    check_close(g, want[5], TOL10[dtype], f"{mode}, {name} x {s}, 5 steps")


# ---- g. partition -----------------------------------------------------------------------------------------------------------------
def test_three_way_partition_of_box2_x37_is_bitwise_the_single_rank_run():
    """box2 x 3.7 split three ways (loopback transport of tests/test_gpu_halo.py, ghost slots poisoned with NaN): patches on
    every rank, generic tiles where the cut went through what is a patch on the single rank. Three steps with split stages are
    bitwise the single-rank patch plan AND the single-rank tile plan: patch and tile kernels agree on non-dyadic geometry."""
    from t8gpu_amd.halo import HaloExchange
    s, world = 3.7, 3
    mesh, st = M.shape("box2"), T.state_of("box2")
    ref = plain("box2", s, True, torch.float64, hip.KEPES, patches=False)
    whole = plain("box2", s, True, torch.float64, hip.KEPES, patches=True)
    assert_divides(whole)
    solvers, halos = [], []
    for r in range(world):
        part = M.scaled(mesh.partition(r, world), s)
        elems = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
        local = st[:, elems].copy()
        local[:, part.N:] = np.nan                                   # ghost values must arrive through the exchange
        solvers.append(PlainSolver(part, torch.float64, mode="fused", state=local, plan_options=dict(patches=True, irregular=True)))
        halos.append(HaloExchange(part, torch.float64, dist=None, overlap=False))
    assert all(g.plan.host.n_patches > 0 and g.plan.host.n_patches_uniform_volume > 0 for g in solvers)
    assert any(0 < g.plan.host.n_interior < g.plan.host.ntiles for g in solvers)
    dt = step_size("box2", s)
    full = T._split_steps(ref, solvers, halos, dt)
    _three_steps(whole, dt)
    assert torch.equal(full, ref.state())
    assert torch.equal(full, whole.state())
    check_close(ref, oracle_run("box2", s, True, hip.KEPES, torch.float64, (1, 3, 10))[3], TOL10[torch.float64], "single rank, box2 x 3.7, 3 steps")


# ---- f. boundaries ------------------------------------------------------------------------------------------------------------------
# -x inflow state 0, +x outflow, -y far field against state 1, +y wall (3D: y periodic, -z wall, +z far field against state 1);
# the states of tests/test_gpu_farfield.py (row 0 at rest, row 1 moving)
OPEN_SIDES = {2: (0, "outflow", ("farfield", 1), "wall"),
              3: (0, "outflow", "periodic", "periodic", "wall", ("farfield", 1))}
BOUNDARY_CASES = [(name, sides) for name in ("box2", "box3", "sbox2", "sbox3") for sides in ("walled", "open")]


def boundary_case(name, sides, s, dtype, kind, **how):
    """(partition, state, inflow states, solver, oracle case) of `name` x s, walled or with OPEN_SIDES"""
    from _farfield import FarCase
    from test_gpu_farfield import far_states
    from test_gpu_open_boundaries import OpenCase
    from test_gpu_subgrid_farfield import SubgridFarCase
    dim = M.SHAPES[name][0]
    periodic, spec = (False, None) if sides == "walled" else (True, OPEN_SIDES[dim])
    part = part_of(name, s, periodic, spec)
    st = T.state_of(name, periodic, spec)
    states = None if sides == "walled" else far_states()
    kinds = set(np.unique(np.asarray(part.boundary_kinds)))
    assert kinds == ({0} if sides == "walled" else {0, 1, 2, 11}) and part.B > 0
    if M.is_subgrid(name):
        g = SubgridSolver(part, dtype, flux_kind=kind, state=st, open_boundaries=True, farfield=True, inflow_states=states, **how)
        o = (O.SubgridCase(part, NP[dtype], state=st) if sides == "walled" else SubgridFarCase(part, NP[dtype], st, states))
    else:
        g = PlainSolver(part, dtype, flux_kind=kind, state=st, inflow_states=states, **how)
        o = (O.PlainCase(part, NP[dtype], state=st) if sides == "walled" else FarCase(part, NP[dtype], st, states))
    return part, st, states, g, o


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,sides", BOUNDARY_CASES)
def test_boundaries_on_x37_stages_vs_oracle(name, sides, kind, dtype):
    """Walls, and inflow / outflow / far-field / wall sides, on s = 3.7: one step and five of the fused tiers (plain: patch
    plan and tile plan, bit for bit; Subgrid: family kernels) and of the compat tier against the oracle-composed references of
    the open-boundary and far-field tests."""
    s = 3.7
    subgrid_mesh = M.is_subgrid(name)
    hows = ([("fused", dict(mode="fused")), ("compat", dict(mode="compat"))] if subgrid_mesh else
            [("patch plan", dict(mode="fused", plan_options=dict(patches=True))), ("tile plan", dict(mode="fused", plan_options=dict(patches=False))),
             ("compat", dict(mode="compat"))])
    built = {tag: boundary_case(name, sides, s, dtype, kind, **how) for tag, how in hows}
    part, _, _, first, o = built[hows[0][0]]
    if subgrid_mesh:
        assert first.plan.host.n_families > 0 and first.plan.host.n_rest > 0
        assert first.plan.c.has_open_faces == (sides == "open") and first.plan.c.has_farfield_faces == (sides == "open")
    else:
        assert built["patch plan"][3].plan.host.n_patches > 0 and built["tile plan"][3].plan.host.n_patches == 0
        assert_divides(built["patch plan"][3])
        assert built["patch plan"][3].plan.c.has_open_faces == (sides == "open")
    dt = step_size(name, s)
    cells = part.N * part.cells_per_element
    for done, tol in ((1, TOL1[dtype]), (5, TOL10[dtype])):
        for _ in range(1 if done == 1 else 4):
            o.iterate(dt, kind)
            for b in built.values():
                b[3].iterate(dt)
        torch.cuda.synchronize()
        want = (o.current()[:, :cells], None if subgrid_mesh else o.speed)
        for tag, b in built.items():
            check_close(b[3], want, tol, f"{name} x 3.7 {sides}, {tag}, {done} step(s)",
                        None if subgrid_mesh or done > 1 else 10 * TOL1[dtype])
        if not subgrid_mesh:
            T.assert_same_bits(part, built["patch plan"][3], built["tile plan"][3], f"{sides}: patch plan vs tile plan, {done} step(s)")
    if sides == "open":
        assert o.branches.sum() > 0, o.branches                       # far-field faces went through the condition


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,sides", BOUNDARY_CASES)
def test_boundary_fluxes_on_x37(name, sides, kind, dtype):
    """boundary_fluxes() by kind and by side against _boundary_ref.reference_block on the scaled partition (areas 3.7 and
    3.7^2 times those of the unit mesh), at the tolerance of tests/test_gpu_boundary_fluxes.py"""
    from test_gpu_boundary_fluxes import check_against_reference
    part, st, states, g, _ = boundary_case(name, sides, 3.7, dtype, kind, mode="compat")
    check_against_reference(g, st, states, dtype, f"FIG boundary_fluxes {name} x 3.7 {sides} kind {kind} {dtype}")
    by_side = g.boundary_fluxes(groups="side")
    want = 3.7 ** (part.mesh.dim - 1)                                    # a side of the box (a periodic side has no faces)
    sides_with_faces = by_side.faces > 0
    assert sides_with_faces.sum() == (2 * part.mesh.dim if sides == "walled" or part.mesh.dim == 2 else 4)
    # fp32: the areas are rounded to float32 before they are summed in fp64
    assert np.abs(by_side.area[sides_with_faces] - want).max() < (1e-13 if dtype == torch.float64 else 1e-6) * want


# ---- h. diagnostics that read geometry --------------------------------------------------------------------------------------------
DIAG_CASES = ["box2", "sbox3"]


def diag_solver(name, s, dtype):
    part = part_of(name, s)
    return (SubgridSolver if part.subgrid else PlainSolver)(part, dtype, mode="compat", state=T.state_of(name))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", DIAG_CASES)
def test_derived_fields_on_x37(name, dtype):
    """vorticity, dilatation and schlieren (area-weighted Green-Gauss sums over 2 V) and the pointwise fields against
    _fields_ref.reference on the scaled arrays, at the tolerance of tests/test_gpu_fields.py"""
    import _fields_ref as ref
    from test_gpu_fields import NAMES, check_fields, planes_of
    g = diag_solver(name, 3.7, dtype)
    want = ref.reference(T.state_of(name), g.part, NP[dtype])
    assert np.all(np.isfinite(want)) and all(np.abs(want[ref.SLOTS[k]]).max() > 0 for k in ("vorticity", "dilatation", "schlieren"))
    check_fields(planes_of(g.derived_fields(NAMES)), want, f"FIG derived_fields {name} x 3.7 {dtype}")
    unit = ref.reference(T.state_of(name), part_of(name), NP[dtype])
    assert np.abs(want[ref.SLOTS["schlieren"]] * 3.7 - unit[ref.SLOTS["schlieren"]]).max() < 1e-6 * np.abs(unit[ref.SLOTS["schlieren"]]).max()   # a gradient: 1 / length


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", DIAG_CASES)
def test_monitor_on_x37(name, dtype):
    """monitor(): volume-weighted integrals and the CFL rate (|v| + c) / vol^(1/dim) against the numpy reference of
    tests/test_gpu_monitor.py on the scaled volumes; cfl_timestep scales with the length"""
    from test_gpu_monitor import TOL, check_block, numpy_rate, reference
    s = 3.7
    g = diag_solver(name, s, dtype)
    part, dim = g.part, g.part.mesh.dim
    S = part.cells_per_element
    st = T.state_of(name).astype(NP[dtype])[:, :part.N * S]
    volumes = np.asarray(part.volumes).astype(NP[dtype])[:part.N]
    want, scale = reference(st, volumes, S, dim)
    check_block(g.monitor().block, want, scale, f"FIG monitor {name} x 3.7 {dtype}")
    cell = np.repeat(volumes.astype(np.float64), S) / S
    want7 = 0.7 / numpy_rate(st, cell, dim)
    assert abs(g.cfl_timestep(0.7) - want7) <= TOL * want7
    unit7 = diag_solver(name, None, dtype).cfl_timestep(0.7)
    assert abs(g.cfl_timestep(0.7) - s * unit7) <= (1e-12 if dtype == torch.float64 else 1e-6) * s * unit7


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", DIAG_CASES)
def test_loehner_indicator_on_x37_and_scale_free(name, dtype):
    """The Loehner indicator against _indicator_ref.reference on the scaled arrays at the tolerance of
    tests/test_gpu_indicator.py, and -- it is scale-free -- against its own unit-mesh values at the same tolerance."""
    import _indicator_ref as ref
    from t8gpu_amd import amr
    from test_gpu_indicator import EPS, SELECTIONS, TOL
    g, unit = diag_solver(name, 3.7, dtype), diag_solver(name, None, dtype)
    worst = worst_unit = 0.0
    for names in SELECTIONS:
        ind = amr.Loehner(names, filter=EPS)
        got = ind.cell_values(g).cpu().numpy()
        want = ref.reference(T.state_of(name), g.part, NP[dtype], names, EPS)
        assert want.shape == got.shape and np.all(np.isfinite(want)) and want.max() > 0.01
        worst = max(worst, float(np.abs(got - want).max()))
        worst_unit = max(worst_unit, float(np.abs(got - ind.cell_values(unit).cpu().numpy()).max()))
        crit = ind.criteria(g).cpu().numpy()
        assert np.abs(crit - ref.block_max(want, g.part)).max() <= TOL, (names, "block max")
    fig(f"Loehner indicator {name} x 3.7 {dtype} vs numpy", worst, TOL)
    fig(f"Loehner indicator {name} x 3.7 {dtype} vs the unit mesh", worst_unit, TOL)
    assert worst <= TOL and worst_unit <= TOL
