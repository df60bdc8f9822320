"""-m gpu: the MULTI-TILE WALKS of the persistent kernels at test-sized meshes.

k_plain_persistent, k_plain_patch / k_plain_stage and k_plain_patch3 / k_plain_patch3_both size their grid as min(tiles, resident
workgroups), and a chip has hundreds of resident workgroups: on the parity meshes of the other files every workgroup has one
tile and the software pipeline -- the next tile's loads in flight, descriptors two tiles ahead, the previous tile's results
stored behind the next tile's first wait, the rotating wavefront roles of the 2D patch body -- never runs a second iteration.
Here every case puts a limit on the resident workgroups (hip.resident_limit: t8gpu_hip_set_resident_limit) and ASSERTS FROM THE
LAUNCH NOTE (hip.last_stage_launches) the kernel it expects with the grid it expects: `limit` workgroups for more tiles than that
(or, for the controls at limit = count and count + 1, one tile each).

What a walk is compared with:
  bits      all 25 state planes over the owned slots and the speed estimates, against the same solver run without a limit (one
            tile per workgroup), which the reference builder first holds against a patches=False plan (the tile kernels): the
            kernels' headers promise the same arithmetic in the same order. A differing word is named by plane and slot.
  oracle    the CPU oracle at the suite's TOL1 after one step and TOL10 after ten (tests/_gpu.py).

Meshes (counts from PlainPlan.on_host, asserted below so that a planner change cannot empty a case):
  u7 / u7w   SynthMesh(2, 7, 7), periodic / walled      16 384 cells   36 patches, 73 generic tiles     k_plain_patch, tiles apart
  b20        SynthMesh(2, 5, 7, band=0.2)               13 696         24, 81                           k_plain_patch, tiles apart
  b13        SynthMesh(2, 5, 7, band=0.13)               9 856         24, 39                           mixed k_plain_stage
  b12        SynthMesh(2, 4, 8, band=0.12)              34 240         84, 130                          mixed k_plain_stage
  h5 / h5w   SynthMesh(3, 5, 5), periodic / walled      32 768         24 regular + 104 irregular, 0    k_plain_patch3
  h45        SynthMesh(3, 4, 5, band=0.15)              25 600         16 + 48, 185 (ELL 16)            k_plain_patch3; _both at limit 16
  t2         b13 with patches=False, tmax=64, fcap=160   9 856         0, 155 (ELL 8)                   k_plain_persistent<.., 1>
  t3         SynthMesh(3, 3, 5, band=0.05), no patches   9 472         0, 158 (ELL 16)                  k_plain_persistent<.., 3>
(3D plans are built with irregular=True, as in test_gpu_patch.py: left alone, fp32 plans may drop the irregular form. With it the
counts are the same in fp32 and fp64.)

Plans are built OUTSIDE the limit: the planner's rules ask the launcher what it would run."""
import os

import numpy as np
import pytest
import torch

import _oracle as O
from _gpu import NP, TOL1, TOL10, perturbed_state, rel_err
from t8gpu_amd import hip
from t8gpu_amd.solver import STEP0, STEP3, PlainSolver
from t8gpu_amd.synth import SynthMesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
_BITS = {F64: torch.int64, F32: torch.int32}
KINDS = {"kepes": hip.KEPES, "hll": hip.HLL, "hllc": hip.HLLC}
ALL = [(dt, k) for dt in (F64, F32) for k in ("kepes", "hll", "hllc")]
TWO = [(F64, "kepes"), (F32, "hllc")]

# name -> SynthMesh arguments, plan options, (cells, regular patches, irregular patches, generic tiles, ELL width)
MESHES = {
    "u7": (dict(dim=2, base_level=7, max_level=7), {}, (16384, 36, 0, 73, 8)),
    "u7w": (dict(dim=2, base_level=7, max_level=7, periodic=False), {}, (16384, 36, 0, 73, 8)),
    "b20": (dict(dim=2, base_level=5, max_level=7, band=0.2), {}, (13696, 24, 0, 81, 8)),
    "b13": (dict(dim=2, base_level=5, max_level=7, band=0.13), {}, (9856, 24, 0, 39, 8)),
    "b12": (dict(dim=2, base_level=4, max_level=8, band=0.12), {}, (34240, 84, 0, 130, 8)),
    "h5": (dict(dim=3, base_level=5, max_level=5), dict(irregular=True), (32768, 24, 104, 0, 8)),
    "h5w": (dict(dim=3, base_level=5, max_level=5, periodic=False), dict(irregular=True), (32768, 24, 104, 0, 8)),
    "h45": (dict(dim=3, base_level=4, max_level=5, band=0.15), dict(irregular=True), (25600, 16, 48, 185, 16)),
    "t2": (dict(dim=2, base_level=5, max_level=7, band=0.13), dict(patches=False, tmax=64, fcap=160), (9856, 0, 0, 155, 8)),
    "t3": (dict(dim=3, base_level=3, max_level=5, band=0.05), dict(patches=False), (9472, 0, 0, 158, 16)),
}
MIXED = ("b13", "b12")          # patches and generic tiles in one k_plain_stage launch
STEPS = (1, 3, 10)              # oracle at TOL1 | bits | bits and oracle at TOL10


def dname(dtype):
    return "f64" if dtype == F64 else "f32"


def tname(dtype):
    return "double" if dtype == F64 else "float"


def bits(t):
    return t.contiguous().view(_BITS[t.dtype])


# ---- meshes, solvers and references: built once per mesh, shared by its cases ----------------------------------------------------
_parts = {}


def partition(mesh):
    if mesh not in _parts:
        m = SynthMesh(**MESHES[mesh][0])
        _parts[mesh] = (m, m.partition())
    return _parts[mesh]


def reset(s, st):
    """the solver as it was built: state `st` in step 0, every other step plane and the speeds zero"""
    tot = s.part.N + s.part.G
    s.planes[:25].zero_()
    s.planes[0:5, :tot] = torch.from_numpy(np.ascontiguousarray(st)).to(s.dtype).cuda()
    s.speed.zero_()
    s.next, s.prev = STEP0, STEP3


def snapshot(s):
    return bits(s.planes[:25, :s.owned_cells]).cpu(), bits(s.speed).cpu()


def differing_words(got, want, what):
    """number of differing words -- 0, or the test fails naming how many and the first one"""
    (gp, gs), (wp, ws) = got, want
    d = (gp != wp).nonzero()
    if len(d):
        plane, slot = (int(x) for x in d[0])
        pytest.fail(f"{what}: {len(d)} differing state words, first in plane {plane} (step {plane // 5}, variable {plane % 5}) slot {slot}")
    d = (gs != ws).nonzero()
    if len(d):
        pytest.fail(f"{what}: {len(d)} differing speed estimates, first at face {int(d[0][0])}")
    return 0


class Reference:
    """One (mesh, dtype, flux): the solver the cases re-run under their limits, and what it gives WITHOUT a limit after each of
    STEPS steps -- held against the patches=False plan bit for bit where the mesh has patches -- and the oracle's states."""

    def __init__(self, mesh, dtype, kind):
        m, part = partition(mesh)
        cells, reg, irr, generic, ell = MESHES[mesh][2]
        opts = dict(dict(patches=True), **MESHES[mesh][1])
        self.part, self.dt = part, 0.1 * 2.0 ** -m.finest_level
        self.st = perturbed_state(part, 31)
        self.solver = PlainSolver(part, dtype, flux_kind=KINDS[kind], mode="fused", state=self.st, plan_options=opts)
        h = self.solver.plan.host
        # (a planner change must not empty a case)
        assert (part.N, h.n_patches - sum(h.n_irregular_class), sum(h.n_irregular_class), h.ntiles - h.n_patches, h.ell_width) == \
            (cells, reg, irr, generic, ell), (mesh, dname(dtype), kind)
        assert part.N <= 35000
        self.free, self.launches = run(self.solver, self.st, self.dt, 0)
        if h.n_patches:
            tiles = PlainSolver(part, dtype, flux_kind=KINDS[kind], mode="fused", state=self.st, plan_options=dict(opts, patches=False))
            assert tiles.plan.host.n_patches == 0
            other, _ = run(tiles, self.st, self.dt, 0)
            for n in STEPS:
                differing_words(self.free[n], other[n], f"{mesh} {dname(dtype)} {kind}: patch plan against tile plan, no limit, step {n}")
        o = O.PlainCase(part, NP[dtype], state=self.st)
        self.oracle = {}
        for n in range(1, STEPS[-1] + 1):
            o.iterate(self.dt, kind=KINDS[kind])
            if n in (1, STEPS[-1]):
                self.oracle[n] = (o.current()[:, :part.N].copy(), o.speed.copy())


def run(s, st, dt, limit):
    """{steps: snapshot} after each of STEPS steps from state `st` under `limit`, and the launches of the last stage call"""
    reset(s, st)
    out = {}
    with hip.resident_limit(limit):
        for n in range(1, STEPS[-1] + 1):
            s.iterate(dt)
            if n in STEPS:
                torch.cuda.synchronize()
                out[n] = snapshot(s)
        launches = hip.last_stage_launches()
        assert hip.last_stage_kernel() in [k for k, _ in launches]
    return out, launches


_refs = {}


def reference(mesh, dtype, kind):
    key = (mesh, dtype, kind)
    if key not in _refs:
        for k in [k for k in _refs if k[0] != mesh]:      # (the cases of a mesh run together: one mesh's references at a time)
            del _refs[k]
        _refs[key] = Reference(mesh, dtype, kind)
    return _refs[key]


def launches_of(launches, kernel, dtype, kind, **where):
    """[(template arguments behind <T, K, S>, workgroups)] of the launches of `kernel` at the third stage of flux `kind`"""
    head = f"{kernel}<{tname(dtype)}, {KINDS[kind]}, 3, "
    got = [(k[len(head):-1].split(", "), w) for k, w in launches if k.startswith(head) and k.endswith(">")]
    return got


def check_walk(ref, mesh, dtype, kind, limit, expect):
    """Runs the reference's solver under `limit`; `expect(launches)` asserts the walk from the note. Bits against the run without
    a limit, states and speeds against the oracle. Prints the oracle errors as fractions of the tolerances."""
    part, what = ref.part, f"{mesh} {dname(dtype)} {kind} limit {limit}"
    got, launches = run(ref.solver, ref.st, ref.dt, limit)
    expect(launches)
    for n in STEPS:
        differing_words(got[n], ref.free[n], f"{what}: walk against one tile per workgroup, step {n}")
    fl = {F64: torch.float64, F32: torch.float32}[dtype]
    state = lambda n: got[n][0].view(fl)[5 * ((STEP0, STEP3)[n % 2]):][:5].numpy()   # (`next` after n steps: 3, 0, 3, ...)
    e1 = rel_err(state(1), ref.oracle[1][0]) / TOL1[dtype]
    e10 = rel_err(state(10), ref.oracle[10][0]) / TOL10[dtype]
    es = rel_err(got[1][1].view(fl).numpy()[None, :part.F + part.B], ref.oracle[1][1][None]) / (10 * TOL1[dtype])   # (as test_gpu_patch.py)
    print(f"WALKFIG {what}: state error {e1:.2e} of TOL1, {e10:.2e} of TOL10; speeds {es:.2e} of 10 TOL1; 0 differing words")
    assert e1 < 1 and e10 < 1 and es < 1, what


# ---- walk shapes: 2D patches -----------------------------------------------------------------------------------------------------
def patch_limits(count, small):
    """1: one workgroup walks everything (every wavefront role); small = 3 | 5: G < 8, so nxcd = G; 8; 12: XCDs 0-3 have two
    workgroups, 4-7 one; count - 1: some workgroups walk two tiles; count: the < / >= boundary; count + 1: the control"""
    return [1, small, 8, 12, count - 1, count, count + 1]


def walk_cases(meshes, small):
    out = []
    for mesh in meshes:
        _, reg, irr, _, _ = MESHES[mesh][2]
        count = irr if irr else reg
        for limit in patch_limits(count, small[mesh]):
            for dtype, kind in (ALL if limit in (1, 12) else TWO):      # 1 and 12 in every combination, the others in two
                out.append(pytest.param(mesh, dtype, kind, limit, id=f"{mesh}-{dname(dtype)}-{kind}-limit{limit}"))
    return out


# (36 patches: 5 and 8 leave count % nxcd != 0; 24: 5; 84: 5 and 8)
@pytest.mark.parametrize("mesh,dtype,kind,limit", walk_cases(("u7", "u7w", "b20", "b13", "b12"), dict(u7=5, u7w=3, b20=5, b13=5, b12=3)))
def test_patch_walk_2d(mesh, dtype, kind, limit):
    ref = reference(mesh, dtype, kind)
    _, count, _, generic, _ = MESHES[mesh][2]
    wgs = min(limit, count)
    assert (wgs < count) == (limit < count)

    def expect(launches):
        if mesh in MIXED:
            got = launches_of(launches, "k_plain_stage", dtype, kind)
            assert [w for _, w in got] == [wgs + generic], (launches, wgs + generic)
        else:
            got = launches_of(launches, "k_plain_patch", dtype, kind)
            assert [w for _, w in got] == [wgs], (launches, wgs)
        assert got[0][0][-1] == "false"                                  # (the general form: no planar request here)

    check_walk(ref, mesh, dtype, kind, limit, expect)


# ---- walk shapes: 3D patches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,dtype,kind,limit", walk_cases(("h5", "h5w", "h45"), dict(h5=5, h5w=3, h45=5)))
def test_patch_walk_3d(mesh, dtype, kind, limit):
    """regular and irregular patches in a launch each; the limits follow the irregular count (the larger), so the regular launch
    walks at 1, 3 | 5, 8 and 12 (24 or 16 patches) and has a patch per workgroup at the others"""
    ref = reference(mesh, dtype, kind)
    _, reg, irr, _, _ = MESHES[mesh][2]

    def expect(launches):
        got = launches_of(launches, "k_plain_patch3", dtype, kind)
        assert [(a[0], w) for a, w in got] == [("false", min(limit, reg)), ("true", min(limit, irr))], launches
        assert not launches_of(launches, "k_plain_patch3_both", dtype, kind)

    check_walk(ref, mesh, dtype, kind, limit, expect)


@pytest.mark.parametrize("dtype,kind", ALL, ids=[f"{dname(d)}-{k}" for d, k in ALL])
def test_patch3_both_kernels_in_one_launch(dtype, kind):
    """k_plain_patch3_both is taken from 2 x resident patches on, resident a multiple of 8 and at least 16: 16 + 48 patches under a
    limit of 16 -- 8 workgroups walk the 16 regular patches, 8 the 48 irregular ones -- against the two separate launches
    (no limit) and the oracle. (fp32: the same counts as fp64, with irregular=True.)"""
    ref = reference("h45", dtype, kind)
    assert not launches_of(ref.launches, "k_plain_patch3_both", dtype, kind) and len(launches_of(ref.launches, "k_plain_patch3", dtype, kind)) == 2

    def expect(launches):
        got = launches_of(launches, "k_plain_patch3_both", dtype, kind)
        assert [w for _, w in got] == [16] and 16 < 16 + 48, launches
        assert not launches_of(launches, "k_plain_patch3", dtype, kind)

    check_walk(ref, "h45", dtype, kind, 16, expect)
    # a limit the split cannot take (not a multiple of 8; below 16) is declined: the two launches
    for limit in (12, 20, 8):
        with hip.resident_limit(limit):
            ref.solver.iterate(ref.dt)
            assert len(launches_of(hip.last_stage_launches(), "k_plain_patch3", dtype, kind)) == 2
    torch.cuda.synchronize()


# ---- the persistent tile kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [1, 5, 8, 12])
@pytest.mark.parametrize("dtype,kind", ALL, ids=[f"{dname(d)}-{k}" for d, k in ALL])
@pytest.mark.parametrize("mesh", ["t2", "t3"])
def test_persistent_tile_walk(mesh, dtype, kind, limit):
    """A plan of at least 8 x limit generic tiles takes k_plain_persistent by the launcher's own size rule: 155 tiles with 8-entry
    ELL rows (one chunk), 158 with 16-entry rows (the second chunk prefetched, the third on demand). Against the launch without
    a limit -- one tile per workgroup -- and the oracle."""
    ref = reference(mesh, dtype, kind)
    tiles, chunks = MESHES[mesh][2][3], {"t2": "1", "t3": "3"}[mesh]
    assert tiles >= 8 * limit and all(w == tiles for _, w in ref.launches)          # no limit: a tile per workgroup

    def expect(launches):
        got = launches_of(launches, "k_plain_persistent", dtype, kind)
        assert got == [([chunks], limit)] and limit < tiles, launches

    check_walk(ref, mesh, dtype, kind, limit, expect)


# ---- planar forms under a walk ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["random", "adversarial"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("mesh", ["b13", "u7"])
def test_planar_walk_equals_general(mesh, dtype, case):
    """The native stepper with set_planar(2) under a limit of 8 (fp64: the four-workgroup form with split records; fp32: its own
    records) against the python-driven general form without a limit: raw bits of 25 planes and the speeds, on the random and the
    adversarial state of test_gpu_planar_wg4.py."""
    from test_gpu_planar_wg4 import adversarial_state, assert_same_bits, planar_state
    _, part = partition(mesh)
    _, count, _, generic, _ = MESHES[mesh][2]
    st = planar_state(part) if case == "random" else adversarial_state(part)
    dt = 0.1 * 2.0 ** -7
    a = PlainSolver(part, dtype, mode="fused", state=st)
    b = PlainSolver(part, dtype, mode="fused", state=st)
    assert b.plan.host.n_patches == count and b.plan.host.ntiles - count == generic
    b.use_native_stepper().set_planar(2)
    for _ in range(3):
        a.iterate(dt)
    with hip.resident_limit(8):
        b.iterate_steps(3, dt)
        launches = hip.last_stage_launches()
    torch.cuda.synchronize()
    assert b.stepper.planar() == 1
    if mesh in MIXED:
        got = launches_of(launches, "k_plain_stage", dtype, "kepes")
        assert [(a_[-1], w) for a_, w in got] == [("true", 8 + generic)], launches
    else:
        got = launches_of(launches, "k_plain_patch", dtype, "kepes")
        assert [(a_[-1], w) for a_, w in got] == [("true", 8)] and 8 < count, launches
    assert_same_bits(a, b)
    assert not bits(b.planes[:20, :b.owned_cells])[3::5].any()


# ---- speed-free launches under a walk --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("mesh", ["u7", "b13", "h5", "t2"])
def test_speed_free_steps_under_a_walk(mesh, dtype):
    """iterate_steps(3, dt) of the native stepper writes the speed estimates in its last step only: the first two steps launch the
    kernels with speed = NULL. Under a limit of 5, against three python-driven iterate() calls without a limit: the bits of the
    25 planes and of the last step's speeds."""
    from test_gpu_planar_wg4 import assert_same_bits
    m, part = partition(mesh)
    st = perturbed_state(part, 9)
    opts = dict(dict(patches=True), **MESHES[mesh][1])
    dt = 0.1 * 2.0 ** -m.finest_level
    a = PlainSolver(part, dtype, mode="fused", state=st, plan_options=opts)
    b = PlainSolver(part, dtype, mode="fused", state=st, plan_options=opts)
    b.use_native_stepper()
    for _ in range(3):
        a.iterate(dt)
    with hip.resident_limit(5):
        b.iterate_steps(3, dt)
        launches = hip.last_stage_launches()
    torch.cuda.synchronize()
    kernel = {"u7": "k_plain_patch", "b13": "k_plain_stage", "h5": "k_plain_patch3", "t2": "k_plain_persistent"}[mesh]
    extra = MESHES[mesh][2][3] if mesh in MIXED else 0
    got = launches_of(launches, kernel, dtype, "kepes")
    assert got and all(w == 5 + extra for _, w in got), launches
    assert_same_bits(a, b)


# ---- the chunked walk ------------------------------------------------------------------------------------------------------------
def test_chunked_walk_on_a_partition_is_bitwise_the_single_rank_run():
    """The 3-way loopback partition of test_gpu_patch.py: the interior range of a rank is launched on its own, beside the other
    lane's kernels, and from `resident` patches on it hands out chunks of 3 (plain_patch_stage). Under a limit of 8 every rank's
    19 / 14 / 25 interior patches do: 8 x ceil(ceil(n / 8) / 3) workgroups, the generic interior tiles behind them in the same
    launch. Rank 2: XCD shares of 4, 3, 3, ... patches and two workgroups per XCD -- the second one of XCDs 1-7 finds nothing to do
    and leaves at once. Bitwise the single-rank run without patches and without a limit."""
    from test_gpu_halo import loopback
    from t8gpu_amd.halo import HaloExchange
    mesh = SynthMesh(2, 4, 8, band=0.12)
    whole = mesh.partition()
    st = perturbed_state(whole, 17)
    ref = PlainSolver(whole, F64, mode="fused", state=st, plan_options=dict(patches=False))
    parts = [mesh.partition(r, 3) for r in range(3)]
    assert [p.N for p in parts] == [11413, 11413, 11414]
    solvers, halos = [], []
    for part in parts:
        gidx = np.concatenate([part.first_global + np.arange(part.N), part.ghost_global])
        local = st[:, gidx].copy()
        local[:, part.N:] = np.nan
        solvers.append(PlainSolver(part, F64, mode="fused", state=local, plan_options=dict(patches=True)))
        halos.append(HaloExchange(part, F64, dist=None, overlap=False))
    hosts = [s.plan.host for s in solvers]
    assert [h.n_patch_class[0] + h.n_patch_class[1] for h in hosts] == [19, 14, 25] and [h.n_interior for h in hosts] == [51, 34, 45]
    limit, chunk = 8, 3
    ceil = lambda a, b: -(-a // b)
    grids = [8 * ceil(ceil(n, 8), chunk) for n in (19, 14, 25)]
    assert grids == [8, 8, 16] and all(n >= limit for n in (19, 14, 25))
    # rank 2: XCD x >= 1 has 25 // 8 = 3 patches, its second workgroup starts at patch 3 of the share: none left
    assert grids[2] // 8 == 2 and 25 // 8 <= chunk * (grids[2] // 8 - 1) and 25 % 8 == 1
    dt = 0.1 * 2.0 ** -mesh.finest_level
    stream = hip.stream_ptr()
    noted = []
    for _ in range(3):
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
                src, dst = s.stage_steps(k)
                ni, nt = s.plan.host.n_interior, s.plan.host.ntiles
                with hip.resident_limit(limit):
                    s.plan.stage(s, k + 1, src, dst, dt, stream, 0, ni)          # the interior range: the chunked walk
                    noted.append(hip.last_stage_launches())
                s.plan.stage(s, k + 1, src, dst, dt, stream, ni, nt - ni)
    torch.cuda.synchronize()
    for r, (launches, h) in enumerate(zip(noted[-3:], hosts)):                    # the third stage of the last step
        patches = h.n_patch_class[0] + h.n_patch_class[1]
        got = launches_of(launches, "k_plain_stage", F64, "kepes")
        assert [w for _, w in got] == [grids[r] + h.n_interior - patches], (r, launches)
    full = torch.cat([s.state() for s in solvers], dim=1)
    d = (bits(full) != bits(ref.state())).nonzero()
    assert len(d) == 0, f"{len(d)} differing words, first in variable {int(d[0][0])} at global slot {int(d[0][1])}"


# ---- the non-temporal instantiations under a walk --------------------------------------------------------------------------------
_STREAM_CHILD = r"""
import hashlib, sys
import torch
sys.path.insert(0, sys.argv[1])
from t8gpu_amd import hip
from t8gpu_amd.solver import PlainSolver
from t8gpu_amd.synth import SynthMesh
for what, mesh, opts in (("patch", SynthMesh(2, 7, 7), {}), ("stage", SynthMesh(2, 4, 8, band=0.12), {}), ("patch3", SynthMesh(3, 5, 5), dict(irregular=True))):
    for dt_ in (torch.float64, torch.float32):
        s = PlainSolver(mesh.partition(), dt_, mode="fused", plan_options=dict(patches=True, **opts))
        dt = 0.1 * 2.0 ** -mesh.finest_level
        with hip.resident_limit(5):
            for _ in range(3):
                s.iterate(dt)
            launches = [f"{k}@{w}" for k, w in hip.last_stage_launches() if k.startswith("k_plain_" + what + "<")]
        torch.cuda.synchronize()
        h = hashlib.sha256(s.planes[:25, :s.owned_cells].cpu().numpy().tobytes() + s.speed.cpu().numpy().tobytes()).hexdigest()
        print(f"{what} {s.planes.element_size()} {s.owned_cells} {h} {';'.join(launches)}")
"""


def test_non_temporal_instantiations_give_the_same_bits_under_a_walk(tmp_path):
    """T8GPU_STREAM_MB (read once per process) picks the instantiations with non-temporal stores of the stage results and loads of
    the previous state. In a walk those stores are the deferred ones. A child per setting (1 MB: always, 0: never), one at a time,
    under a limit of 5: 2D patches, the mixed kernel and 3D patches hash equal (25 planes and speeds), and the note names the other instantiation."""
    import subprocess
    import sys
    script = tmp_path / "walk_stream_child.py"
    script.write_text(_STREAM_CHILD)
    outs = {}
    for mb in ("0", "1"):
        res = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=280, env=dict(os.environ, T8GPU_STREAM_MB=mb))
        assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
        outs[mb] = [ln.split(" ", 4) for ln in res.stdout.strip().splitlines() if ln.split(" ", 1)[0] in ("patch", "stage", "patch3")]
    assert len(outs["0"]) == len(outs["1"]) == 6
    streamed = 0
    for (what, size, cells, h0, l0), (_, _, _, h1, l1) in zip(outs["0"], outs["1"]):
        assert h0 == h1, (what, size)
        generic = 130 if what == "stage" else 0
        # (flux_math.hpp: stream_hint -- the 15 planes of a stage against the threshold; the 16 384 cells of the 2D patch mesh stay
        #  below 1 MB in fp32, every other case lies above)
        over = 15 * int(cells) * int(size) > 1 << 20
        assert over == ((what, size) != ("patch", "4"))
        streamed += over
        for launches, flag in ((l0, "false"), (l1, "true" if over else "false")):
            names = launches.split(";")
            assert len(names) == (2 if what == "patch3" else 1), launches
            for name in names:
                kernel, wgs = name.rsplit("@", 1)
                assert int(wgs) == 5 + generic, launches                       # 36, 84 or 24 + 104 patches on 5 workgroups
                args = kernel[kernel.index("<") + 1:-1].split(", ")
                assert args[4 if what == "patch3" else 3] == flag, launches    # <T, K, S, NT, ..> | k_plain_patch3<T, K, S, IRR, NT>
    assert streamed == 5
