"""-m gpu: the HIP tiers on tests/golden/reference_kernel_vectors.npz -- inputs and outputs of the reference's own kernel bodies,
executed on tiny AMR meshes (tests/golden/make_reference_kernel_vectors.py) -- directly, not through the CPU oracle.

* compat tier, kernel by kernel: what kepes_compute_fluxes, reflective_boundary_condition, compute_inner / boundary /
  outer_fluxes and the six SSP-RK3 kernels of the reference wrote is what t8gpu_hip_flux_faces / _flux_boundary /
  _subgrid_inner / _subgrid_boundary / _subgrid_outer / _rk3_stage / _subgrid_rk3_stage write on the same inputs (the RK
  stages bit for bit);
* the element -> slot map `indices` of t8gpu_hip_flux_faces, t8gpu_hip_subgrid_outer and t8gpu_hip_estimate_gradient, which the
  solvers of this package never pass: elements stored in a permuted order give the same stored outputs;
* fused tier: one stage on the fixture meshes equals the reference's RK update (the oracle's restatement, which
  test_oracle_reference_kernels.py and the RK test here hold to the reference's bits) of the reference's own flux planes.

Every expected value is a stored output of the reference, or the oracle's RK stage applied to one. The plans the fused
tests count on (several tiles with halos; families and single blocks; hanging faces) are asserted without a GPU in
test_kernel_vector_plans.py."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import _kernel_vectors as KV
import _oracle as O
from _gpu import NP, TOL1, rel_err
from t8gpu_amd import hip
from t8gpu_amd.solver import FLUXES, STEP1, STEP2, STEP3, PlainSolver, SubgridSolver

pytestmark = pytest.mark.gpu
DTYPE = {"f64": torch.float64, "f32": torch.float32}
KEPES = KV.KEPES
SMALL_TILES = dict(tmax=8, fcap=24)             # several tiles that read each other's cells (test_kernel_vector_plans.py)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def flux_err(got, want, face_area):
    """max over variables and cells of |got - want| / (max|want| + face_area): fluxes are differences of O(area) terms, so
    the error is normalised by the largest single-face contribution as well (test_plain_flux_kernels_vs_oracle,
    test_subgrid_kernels_individually of test_gpu_compat.py)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max(axis=1, keepdims=True) + face_area
    return float((np.abs(got - want) / scale).max())


def seeded_permutation(case, n):
    """element id -> slot: a permutation that moves (nearly) every element, seeded by the case name"""
    perm = np.random.default_rng(zlib.crc32(case.encode())).permutation(n).astype(np.int32)
    assert int((perm != np.arange(n)).sum()) > n // 2
    return perm


def sizes(ins):
    return tuple(int(x) for x in ins["sizes"])


# ---- compat tier, kernel by kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", KV.TAGS)
@pytest.mark.parametrize("case", KV.plain_cases())
def test_plain_flux_kernels_on_the_executed_reference_kernels(case, tag):
    """kepes_compute_fluxes, then reflective_boundary_condition on the same planes (kernels.cu:135-469). The kernels keep the
    reference's operation order; the order of the atomic adds and the device's log / sqrt / division sequences differ."""
    ins, outs = KV.load(case, tag)
    dtype = DTYPE[tag]
    N, G, F, B, stride = sizes(ins)
    ndim = int(ins["normal_dim"][0])
    planes = torch.zeros((26, stride), dtype=dtype, device="cuda")
    planes[0:5] = dev(ins["state"].reshape(5, stride))
    fn, normals, areas = dev(ins["fn"]), dev(ins["normals"]), dev(ins["areas"])
    speed = torch.zeros(F + B, dtype=dtype, device="cuda")
    st, fl, s = hip.vars_of(planes, 0), hip.vars_of(planes, FLUXES), hip.stream_ptr()
    area = float(ins["areas"].max())
    hip.call("t8gpu_hip_flux_faces", dtype, KEPES, F, ndim, hip.ptr(fn), None, hip.ptr(normals), hip.ptr(areas), st, fl,
             hip.ptr(speed), s)
    err = flux_err(host(planes)[20:25, :N], outs["flux_interior"].reshape(5, stride)[:, :N], area)
    assert err < TOL1[dtype], (case, "interior faces", err)
    hip.call("t8gpu_hip_flux_boundary", dtype, KEPES, F, B, ndim, hip.ptr(fn), hip.ptr(normals), hip.ptr(areas), st, fl,
             hip.ptr(speed), s)
    after = host(planes)
    err = flux_err(after[20:25, :N], outs["flux_all"].reshape(5, stride)[:, :N], area)
    assert err < TOL1[dtype], (case, "interior + wall faces", err)
    assert outs["speed"].min() > 0
    err = rel_err(host(speed)[None], outs["speed"][None])
    assert err < TOL1[dtype], (case, "speed estimates of all F + B faces", err)
    assert np.array_equal(after[0:5], ins["state"].reshape(5, stride)) and (after[5:20] == 0).all() and (after[25] == 0).all()


def run_subgrid_flux_kernels(ins, dtype, planes, which, indices=None):
    N, G, F, B, stride = sizes(ins)
    rank = int(ins["rank"][0])
    keep = [dev(ins[k]) for k in ("fn", "normals", "areas", "level_diff", "nb_offset", "volume")]
    fn, normals, areas, level_diff, nb_offset, volume = keep
    st, fl, s = hip.vars_of(planes, 0), hip.vars_of(planes, FLUXES), hip.stream_ptr()
    if which == "inner":
        hip.call("t8gpu_hip_subgrid_inner", dtype, KEPES, rank, N, st, fl, hip.ptr(volume), s)
    elif which == "boundary":
        hip.call("t8gpu_hip_subgrid_boundary", dtype, KEPES, rank, F, B, hip.ptr(fn), hip.ptr(normals), hip.ptr(areas), st, fl, s)
    else:
        idx = None if indices is None else dev(indices)
        keep.append(idx)
        hip.call("t8gpu_hip_subgrid_outer", dtype, KEPES, rank, F, hip.ptr(fn), hip.ptr(idx), hip.ptr(level_diff),
                 hip.ptr(nb_offset), hip.ptr(normals), hip.ptr(areas), st, fl, s)
    torch.cuda.synchronize()            # (the arrays of `keep` live until the kernel is done)


def outer_alone(outs, stride):
    """what compute_outer_fluxes alone added: flux_all - flux_inner_boundary, formed in float64 (as the CPU test does)"""
    return outs["flux_all"].reshape(5, stride).astype(np.float64) - outs["flux_inner_boundary"].reshape(5, stride).astype(np.float64)


def subface_area(ins):
    return float(ins["areas"].max()) / 4 ** (int(ins["rank"][0]) - 1)        # / 16 in 3D, / 4 in 2D: one sub-face


@pytest.mark.parametrize("tag", KV.TAGS)
@pytest.mark.parametrize("case", KV.subgrid_cases())
def test_subgrid_flux_kernels_on_the_executed_reference_kernels(case, tag):
    """compute_inner_fluxes, compute_boundary_fluxes, compute_outer_fluxes (kernels.inl:335-1107) one after the other on the
    same planes, and the outer kernel ALONE on zeroed planes against flux_all - flux_inner_boundary: a wrong far cell on a
    hanging sub-face would drown in the inner fluxes otherwise. That difference of two stored arrays carries their rounding
    (half an ulp of an accumulated flux each), which is far inside TOL1 of the same scale: the inner, wall and outer fluxes of
    a cell are all of the size of one sub-face's flux."""
    ins, outs = KV.load(case, tag)
    dtype = DTYPE[tag]
    N, G, F, B, stride = sizes(ins)
    S = 4 ** int(ins["rank"][0])
    n, area = N * S, subface_area(ins)
    assert int((ins["level_diff"] != 0).sum()) > 0
    planes = torch.zeros((25, stride), dtype=dtype, device="cuda")
    planes[0:5] = dev(ins["state"].reshape(5, stride))
    for which, name in (("inner", "flux_inner"), ("boundary", "flux_inner_boundary"), ("outer", "flux_all")):
        run_subgrid_flux_kernels(ins, dtype, planes, which)
        err = flux_err(host(planes)[20:25, :n], outs[name].reshape(5, stride)[:, :n], area)
        assert err < TOL1[dtype], (case, name, err)
    planes[20:25] = 0
    run_subgrid_flux_kernels(ins, dtype, planes, "outer")
    after = host(planes)
    want = outer_alone(outs, stride)[:, :n]
    assert np.abs(want).max(axis=1).min() > 0
    err = flux_err(after[20:25, :n], want, area)
    assert err < TOL1[dtype], (case, "outer faces alone", err)
    assert np.array_equal(after[0:5], ins["state"].reshape(5, stride)) and (after[5:20] == 0).all()


@pytest.mark.parametrize("tag", KV.TAGS)
@pytest.mark.parametrize("case", KV.case_names())
def test_rk_stages_on_the_executed_reference_kernels(case, tag):
    """SSP_3RK_step1 / 2 / 3 and their Subgrid forms (ssp_runge_kutta.inl:30-221): same operation order, no contraction, so
    every bit of rk_out{1,2,3}; the flux planes come back zero; nothing is written past the N (N * S) owned cells."""
    ins, outs = KV.load(case, tag)
    dtype = DTYPE[tag]
    N, G, F, B, stride = sizes(ins)
    rank = int(ins["rank"][0])
    n = N * 4 ** rank if rank else N
    cap = n + 13                                                  # ragged: spare capacity behind the owned cells
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    fill = rng.standard_normal((20, cap)).astype(NP[dtype])       # prev | mid | out | flux
    fill[0:5, :n] = ins["state"].reshape(5, stride)[:, :n]
    fill[5:10, :n] = ins["rk_mid"].reshape(5, stride)[:, :n]
    fill[15:20, :n] = ins["rk_flux"].reshape(5, stride)[:, :n]
    volume = dev(ins["volume"])
    dt = hip.fscalar(dtype, float(ins["dt"][0]))
    for stage in (1, 2, 3):
        d = dev(fill)
        v = [hip.vars_of(d, k) for k in range(4)]
        if rank:
            hip.call("t8gpu_hip_subgrid_rk3_stage", dtype, stage, rank, N, v[0], v[1], v[2], v[3], hip.ptr(volume), dt, hip.stream_ptr())
        else:
            hip.call("t8gpu_hip_rk3_stage", dtype, stage, N, v[0], v[1], v[2], v[3], hip.ptr(volume), dt, hip.stream_ptr())
        got = host(d)
        want = outs[f"rk_out{stage}"].reshape(5, stride)[:, :n]
        assert np.array_equal(got[10:15, :n], want), (case, f"RK stage {stage}", rel_err(got[10:15, :n], want))
        assert (got[15:20, :n] == 0).all() and (outs[f"rk_flux_after{stage}"] == 0).all()
        assert np.array_equal(got[:, n:], fill[:, n:])            # nothing written past the owned cells
        assert np.array_equal(got[0:10], fill[0:10])              # the two source states untouched


# ---- the element -> slot map `indices` ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", KV.TAGS)
@pytest.mark.parametrize("case", KV.plain_cases())
def test_flux_faces_with_an_element_to_slot_map(case, tag):
    """Elements stored in slot order, face_neighbors in element ids, `indices` = element -> slot (kernels.cu:164-168): the
    fluxes read back through the map are the reference's flux_interior; the speed estimates are per face and do not move."""
    ins, outs = KV.load(case, tag)
    dtype = DTYPE[tag]
    N, G, F, B, stride = sizes(ins)
    ndim = int(ins["normal_dim"][0])
    perm = seeded_permutation(case, N)
    state = np.zeros((5, stride), NP[dtype])
    state[:, perm] = ins["state"].reshape(5, stride)[:, :N]
    planes = torch.zeros((26, stride), dtype=dtype, device="cuda")
    planes[0:5] = dev(state)
    fn, idx, normals, areas = dev(ins["fn"]), dev(perm), dev(ins["normals"]), dev(ins["areas"])
    speed = torch.zeros(F + B, dtype=dtype, device="cuda")
    hip.call("t8gpu_hip_flux_faces", dtype, KEPES, F, ndim, hip.ptr(fn), hip.ptr(idx), hip.ptr(normals), hip.ptr(areas),
             hip.vars_of(planes, 0), hip.vars_of(planes, FLUXES), hip.ptr(speed), hip.stream_ptr())
    got = host(planes)[20:25][:, perm]
    err = flux_err(got, outs["flux_interior"].reshape(5, stride)[:, :N], float(ins["areas"].max()))
    assert err < TOL1[dtype], (case, "interior faces through the map", err)
    err = rel_err(host(speed)[None, :F], outs["speed"][None, :F])
    assert err < TOL1[dtype], (case, "speed estimates of the F interior faces", err)


@pytest.mark.parametrize("tag", KV.TAGS)
@pytest.mark.parametrize("case", KV.subgrid_cases())
def test_subgrid_outer_with_an_element_to_slot_map(case, tag):
    """Blocks move whole: the subcells of block e lie in [perm[e] * S, (perm[e] + 1) * S). The map applies to the block, the
    sub-face's cell offset (and the far-cell map of a hanging face) inside it (kernels.inl:664-911)."""
    ins, outs = KV.load(case, tag)
    dtype = DTYPE[tag]
    N, G, F, B, stride = sizes(ins)
    S = 4 ** int(ins["rank"][0])
    perm = seeded_permutation(case, N)
    state = np.zeros((5, N, S), NP[dtype])
    state[:, perm] = ins["state"].reshape(5, N, S)
    planes = torch.zeros((25, stride), dtype=dtype, device="cuda")
    planes[0:5] = dev(state.reshape(5, stride))
    run_subgrid_flux_kernels(ins, dtype, planes, "outer", indices=perm)
    got = host(planes)[20:25].reshape(5, N, S)[:, perm].reshape(5, stride)
    err = flux_err(got, outer_alone(outs, stride), subface_area(ins))
    assert err < TOL1[dtype], (case, "outer faces alone through the map", err)


@pytest.mark.parametrize("tag", KV.TAGS)
@pytest.mark.parametrize("case", KV.case_names())
def test_estimate_gradient_with_an_element_to_slot_map(case, tag):
    """estimate_gradient (kernels.cu:471-501): |rho_r - rho_l| added to both cells of every face. rho = the first N values of
    the case's first state plane (on a Subgrid mesh simply a field over its blocks: the kernel is per element). Reference:
    numpy in float64 on the unpermuted arrays. A cell sums at most 24 non-negative terms (6 sides, 4 finer neighbours
    each), each the rounded difference of two stored values: 1 + 23 roundings at most, so 32 eps max(gradient) holds with
    room. With and without the map (identity layout) the same bound."""
    ins, _ = KV.load(case, tag)
    dtype = DTYPE[tag]
    N, G, F, B, stride = sizes(ins)
    rho = np.ascontiguousarray(ins["state"].reshape(5, stride)[0, :N])
    l, r = ins["fn"][0:2 * F:2], ins["fn"][1:2 * F:2]
    jump = np.abs(rho[r].astype(np.float64) - rho[l].astype(np.float64))
    want = np.zeros(N)
    np.add.at(want, l, jump)
    np.add.at(want, r, jump)
    assert want.min() > 0 and int(np.bincount(np.concatenate([l, r]), minlength=N).max()) <= 24
    bound = 32 * float(np.finfo(NP[dtype]).eps) * want.max()
    perm = seeded_permutation(case, N)
    moved = np.zeros(N, NP[dtype])
    moved[perm] = rho
    fn = dev(ins["fn"])
    got = {}
    for name, field, idx in (("map", moved, dev(perm)), ("identity", rho, None)):
        d_rho, grad = dev(field), torch.zeros(N, dtype=dtype, device="cuda")
        hip.call("t8gpu_hip_estimate_gradient", dtype, F, hip.ptr(fn), hip.ptr(idx), hip.ptr(d_rho), hip.ptr(grad), hip.stream_ptr())
        got[name] = host(grad).astype(np.float64)
    got["map"] = got["map"][perm]
    for name in got:
        err = np.abs(got[name] - want).max()
        assert err <= bound, (case, name, err, bound)
    assert np.abs(got["map"] - got["identity"]).max() <= bound


# ---- fused tier: one stage against the reference's executed flux kernels -------------------------------------------------
def last_stage_kernel():
    q = hip.lib().t8gpu_hip_last_stage_kernel
    q.restype = C.c_char_p
    return q().decode()


def expected_stage(ins, outs, stage):
    """(expected, increment) of RK stage `stage` in float64, [5, owned cells]: the oracle's RK stage (the reference's, bit for
    bit) of the STORED flux planes flux_all -- the fluxes of the stored `state` by the reference's own flux kernels. For
    stage 1 `prev` is `state` too; for stages 2 and 3 `prev` is the stored rk_mid (it enters linearly only) and `state` is
    the stage's source (`mid`). increment = expected - the same stage with zero fluxes: the part the flux evaluation made."""
    N, G, F, B, stride = sizes(ins)
    rank = int(ins["rank"][0])
    n = N * 4 ** rank if rank else N
    np_t = ins["state"].dtype
    state = np.ascontiguousarray(ins["state"].reshape(5, stride))
    prev = state if stage == 1 else np.ascontiguousarray(ins["rk_mid"].reshape(5, stride))
    vol = np.ascontiguousarray(ins["volume"])
    res = []
    for flux in (outs["flux_all"].reshape(5, stride).copy(), np.zeros((5, stride), np_t)):       # (the oracle zeroes its flux planes)
        out = np.zeros((5, stride), np_t)
        mid = O.p(state) if stage > 1 else None
        if rank:
            getattr(O.lib(), "oracle_subgrid_rk_stage_" + O.suf(np_t))(stage, rank, N, O.p(prev), mid, O.p(out), O.p(flux), C.c_size_t(stride),
                                                                      O.p(vol), O.fs(np_t, float(ins["dt"][0])))
        else:
            getattr(O.lib(), "oracle_plain_rk_stage_" + O.suf(np_t))(stage, N, O.p(prev), mid, O.p(out), O.p(flux), C.c_size_t(stride), O.p(vol),
                                                                    O.fs(np_t, float(ins["dt"][0])))
        res.append(out[:, :n].astype(np.float64))
    return res[0], res[0] - res[1]


def stage_excess(got, expected, incr, dtype):
    """max_k  max_i |got_k - expected_k|  /  (TOL1 max_i |incr_k| + 2 eps max_i |expected_k|): must not exceed 1. A stage
    result is dominated by the state it started from, so the bound is sized to the flux part: the project's one-kernel
    tolerance applied to the increment, plus the rounding of the stored result itself."""
    eps = float(np.finfo(NP[dtype]).eps)
    top = np.abs(incr).max(axis=1)
    assert top.min() > 0, top                                     # the bound cannot collapse: every variable has a flux
    bound = TOL1[dtype] * top + 2 * eps * np.abs(expected).max(axis=1)
    return float((np.abs(np.asarray(got, np.float64) - expected).max(axis=1) / bound).max())


def check_fused_stages(solver, ins, outs, what):
    """Stages 1, 2, 3 of `solver` (fused mode, built on the case's stored state), each from the stored inputs. Returns the
    kernel names noted per stage."""
    dtype = solver.dtype
    N, G, F, B, stride = sizes(ins)
    n = solver.owned_cells
    state, mid = dev(ins["state"].reshape(5, stride)), dev(ins["rk_mid"].reshape(5, stride))
    dt = float(ins["dt"][0])
    names = []
    for stage in (1, 2, 3):
        solver.planes[0:25] = 0
        solver.planes[0:5] = state                                # Step0: the flux source
        solver.planes[15:20] = mid                                # Step3: `prev` of stages 2 and 3
        # (the step roles of _Solver.run_stage: `prev` summand, source, destination; stage 1 has prev == source)
        solver.prev = 0 if stage == 1 else STEP3
        dst = STEP1 if stage == 1 else STEP2
        solver.plan.stage(solver, stage, 0, dst, dt, hip.stream_ptr())
        got = host(solver.planes)
        names.append(last_stage_kernel())
        expected, incr = expected_stage(ins, outs, stage)
        excess = stage_excess(got[5 * dst:5 * dst + 5, :n], expected, incr, dtype)
        assert excess <= 1.0, (what, f"stage {stage}", names[-1], "error / bound", excess)
        assert (got[20:25] == 0).all(), (what, stage, names[-1])   # the Fluxes planes stay zero
        assert np.array_equal(got[0:5], host(state)) and np.array_equal(got[15:20], host(mid)), (what, stage, names[-1])
        other = STEP2 if stage == 1 else STEP1
        assert (got[5 * other:5 * other + 5] == 0).all(), (what, stage, names[-1])
        if stage == 3 and hasattr(solver, "speed"):               # PlainPlan.stage: the speed estimates are stage 3's
            err = rel_err(host(solver.speed)[None, :F + B], outs["speed"][None])
            assert err < TOL1[dtype], (what, "speed estimates", names[-1], err)
    return names


def plain_fused_solver(case, tag, options):
    ins, outs = KV.load(case, tag)
    part = KV.FixturePartition(case, ins)
    solver = PlainSolver(part, DTYPE[tag], flux_kind=KEPES, mode="fused", state=ins["state"].reshape(5, part.stride),
                         plan_options=options)
    return solver, ins, outs


def subgrid_fused_solver(case, tag):
    ins, outs = KV.load(case, tag)
    part = KV.FixturePartition(case, ins)
    return SubgridSolver(part, DTYPE[tag], flux_kind=KEPES, mode="fused", state=ins["state"].reshape(5, part.stride)), ins, outs


PLAN_FORMS = {"dictionary": {}, "face_rows": dict(dictionary=False), "csr": dict(compressed=False)}


@pytest.mark.parametrize("tiles", ["one_tile", "small_tiles"])
@pytest.mark.parametrize("form", list(PLAN_FORMS))
@pytest.mark.parametrize("tag", KV.TAGS)
@pytest.mark.parametrize("case", KV.plain_cases())
def test_plain_fused_stage_on_the_executed_reference_kernels(case, tag, form, tiles):
    """Every form of the plain tile kernels -- geometry dictionary, per-face geometry rows, CSR lists; the default tiling
    (one tile) and tiles of 8 elements with halos -- through stages 1, 2, 3."""
    options = dict(PLAN_FORMS[form], **(SMALL_TILES if tiles == "small_tiles" else {}))
    solver, ins, outs = plain_fused_solver(case, tag, options)
    assert solver.plan.host.n_patches == 0
    assert (solver.plan.host.ntiles > 1 and solver.plan.host.halo_ids.size > 0) == (tiles == "small_tiles")
    check_fused_stages(solver, ins, outs, (case, tag, form, tiles))


@pytest.mark.parametrize("tag", KV.TAGS)
@pytest.mark.parametrize("case", KV.subgrid_cases())
def test_subgrid_fused_stage_on_the_executed_reference_kernels(case, tag):
    """The default Subgrid plan: families (the family kernel) and single blocks (the block kernel) in one mesh, hanging
    faces in every case."""
    solver, ins, outs = subgrid_fused_solver(case, tag)
    assert solver.plan.host.n_families > 0 and solver.plan.host.n_rest > 0
    check_fused_stages(solver, ins, outs, (case, tag))


_SWITCHES_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_reference_kernels as T
for tag in T.KV.TAGS:
    for options in (dict(patches=False), dict(T.SMALL_TILES, patches=False)):
        solver, ins, outs = T.plain_fused_solver("plain3d_wall", tag, options)
        for name in T.check_fused_stages(solver, ins, outs, ("plain3d_wall", tag, options)):
            print("plain:" + name)
    solver, ins, outs = T.subgrid_fused_solver("sub3d_wall", tag)
    for name in T.check_fused_stages(solver, ins, outs, ("sub3d_wall", tag)):
        print("subgrid:" + name)
print("done")
"""


def test_fused_stage_under_the_process_wide_switches(tmp_path):
    """The persistent tile kernel (T8GPU_PERSISTENT=2 with T8GPU_PERSISTENT_WGS=3: every launch, whatever the plan's size)
    and the Subgrid block kernel on every block (T8GPU_SG_FAMILY=0) in the same comparison: plain3d_wall (one tile, and
    tiles of 8 elements) and sub3d_wall, fp64 and fp32. The switches are read once per process, hence a fresh child
    process; it prints the kernels that ran."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "child.py"
    script.write_text(_SWITCHES_CHILD.format(root=os.path.dirname(here), tests=here))
    res = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, T8GPU_PERSISTENT="2", T8GPU_PERSISTENT_WGS="3", T8GPU_SG_FAMILY="0"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.splitlines()
    assert lines[-1] == "done"
    plain = [line[len("plain:"):] for line in lines if line.startswith("plain:")]
    subgrid = [line[len("subgrid:"):] for line in lines if line.startswith("subgrid:")]
    assert len(plain) == 12 and all(k.startswith("k_plain_persistent<") for k in plain), plain
    assert len(subgrid) == 6 and all(k.startswith("k_subgrid_fused") for k in subgrid), subgrid
