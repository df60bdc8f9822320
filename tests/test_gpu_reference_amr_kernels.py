"""-m gpu: the AMR transfer, indicator, z-order and partition entries of the HIP library on tests/golden/reference_amr_vectors.npz
(+ _rank3) -- inputs and outputs of the reference's own kernel bodies, executed on real forests
(tests/golden/make_reference_amr_vectors.py) -- directly, not through the CPU oracle. The forests reach what the one mark
pattern of test_gpu_amr.py never does: a coarsened family and a refined family at element 0, two refined parents back to
back at the end of the curve, a new mesh of one element.

* transfers (plain at dim = 3, Subgrid rank 2 and 3), z-order, partition (gather + scatter run by run; the repartition entry
  with every run addressed to this rank): copies, sums in a fixed order and one division, so BIT FOR BIT; output planes
  start as a sentinel and every owned slot, and nothing else, is written;
* criteria: the bounds the same kernels have against the oracle in test_gpu_amr.py (the kernels contract to FMA and use the
  device's cbrt / sqrt, the reference build does neither); estimate_gradient: 32 eps max(gradient), the bound of
  test_estimate_gradient_with_an_element_to_slot_map (the order of the atomics differs);
* the Python layer: amr.adapt / amr.adapt_subgrid with the marks of `ends`, and a carried `sums` tensor.
Every expected value is a stored output of the reference. Each test prints its measured error / bound (pytest -s)."""
import zlib

import numpy as np
import pytest
import torch

import _amr_vectors as AV
from _gpu import NP
from t8gpu_amd import amr, hip
from t8gpu_amd.solver import PlainSolver, SubgridSolver
from t8gpu_amd.synth import SynthMesh

pytestmark = pytest.mark.gpu
DTYPE = {"f64": torch.float64, "f32": torch.float32}
SENTINEL = -12345.0                      # no stored value: densities and volumes are positive, |momentum| and energy below 10
SPARE = 13                               # ragged spare capacity behind the owned slots


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def np_ptr(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p)


def sentinel_planes(rows, owned, dtype):
    return torch.full((rows, owned + SPARE), SENTINEL, dtype=dtype, device="cuda")


def check_planes(got, want, owned, what):
    """got [rows, owned + SPARE] against want [rows, owned]: every bit, every owned slot written, nothing behind them"""
    assert (got[:, :owned] != SENTINEL).all(), (what, "owned slots left unwritten", int((got[:, :owned] == SENTINEL).sum()))
    assert (got[:, owned:] == SENTINEL).all(), (what, "written past the owned slots")
    assert np.array_equal(got[:, :owned], want), (what, "max difference", float(np.abs(got[:, :owned].astype(np.float64) - want).max()))


# ---- transfers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", AV.case_names())
def test_plain_transfer_on_the_executed_reference_kernel(case, tag):
    """adapt_variables_and_volume (mesh_manager.inl:164-193) at dim = 3, the reference's hard-coded 0.125 / 8.0, on the 2D
    forests too."""
    ins, outs = AV.load(case, tag)
    dtype = DTYPE[tag]
    n_old, n_new, _, _, _ = AV.sizes(ins)
    old = dev(np.vstack([ins["state"], ins["volume"][None]]))
    new = sentinel_planes(6, n_new, dtype)
    ad = dev(ins["adapt_data"])
    hip.call("t8gpu_hip_adapt_variables_and_volume", dtype, n_new, 3, hip.ptr(ad), hip.vars_of(old), hip.vars_of(new), hip.ptr(old[5]),
             hip.ptr(new[5]), hip.stream_ptr())
    got = host(new)
    check_planes(got[:5], outs["variables"].reshape(5, n_new), n_new, (case, "variables"))
    check_planes(got[5:], outs["volumes"][None], n_new, (case, "volumes"))
    assert np.array_equal(host(old), np.vstack([ins["state"], ins["volume"][None]]))


@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", AV.subgrid_cases())
def test_subgrid_transfer_on_the_executed_reference_kernels(case, tag):
    """adapt_volume + adapt_variables (subgrid_mesh_manager.inl:245-425): the octant a child takes from its position in the
    family, the z-order of a coarsened family's members, rank 2 and rank 3."""
    ins, outs = AV.load(case, tag)
    dtype = DTYPE[tag]
    n_old, n_new, _, _, rank = AV.sizes(ins)
    S = 4 ** rank
    old, vol = dev(ins["sub_state"]), dev(ins["volume"])
    new = sentinel_planes(5, n_new * S, dtype)
    nvol = sentinel_planes(1, n_new, dtype)
    ad = dev(ins["adapt_data"])
    hip.call("t8gpu_hip_subgrid_adapt_variables_and_volume", dtype, rank, n_new, hip.ptr(ad), hip.vars_of(old), hip.vars_of(new),
             hip.ptr(vol), hip.ptr(nvol), hip.stream_ptr())
    check_planes(host(new), outs["sub_variables"].reshape(5, n_new * S), n_new * S, (case, "Subgrid variables"))
    check_planes(host(nvol), outs["sub_volumes"][None], n_new, (case, "Subgrid volumes"))
    assert np.array_equal(host(old), ins["sub_state"]) and np.array_equal(host(vol), ins["volume"])


# ---- indicators ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", AV.subgrid_cases())
def test_subgrid_criteria_on_the_executed_reference_kernel(case, tag):
    """compute_refinement_criteria<Subgrid> (kernels.inl:1109-1168); bound: test_subgrid_indicator_and_transfer_vs_oracle's."""
    ins, outs = AV.load(case, tag)
    dtype = DTYPE[tag]
    n_old, _, _, _, rank = AV.sizes(ins)
    rho, vol = dev(ins["sub_state"][0]), dev(ins["volume"])
    crit = sentinel_planes(1, n_old, dtype)
    hip.call("t8gpu_hip_subgrid_refinement_criteria", dtype, rank, n_old, hip.ptr(rho), hip.ptr(vol), hip.ptr(crit), hip.stream_ptr())
    got, want = host(crit), outs["sub_criteria"].astype(np.float64)
    assert (got[0, n_old:] == SENTINEL).all() and (got[0, :n_old] != SENTINEL).all()
    bound = (1e-12 if tag == "f64" else 2e-5) * np.abs(want).max()
    err = float(np.abs(got[0, :n_old] - want).max())
    print(f"\n{case} {tag}: Subgrid criteria error / bound = {err / bound:.3g}")
    assert err <= bound, (case, err, bound)


@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", AV.case_names())
def test_plain_criteria_on_the_executed_reference_kernel(case, tag):
    """compute_refinement_criteria (solver.cu:231-241) on the STORED gradient; bound: test_indicator_kernels_vs_oracle's."""
    ins, outs = AV.load(case, tag)
    dtype = DTYPE[tag]
    n_old = AV.sizes(ins)[0]
    grad, vol = dev(outs["gradient"]), dev(ins["volume"])
    crit = sentinel_planes(1, n_old, dtype)
    hip.call("t8gpu_hip_refinement_criteria", dtype, n_old, hip.ptr(grad), hip.ptr(vol), hip.ptr(crit), hip.stream_ptr())
    got, want = host(crit), outs["criteria"].astype(np.float64)
    assert (got[0, n_old:] == SENTINEL).all() and (got[0, :n_old] != SENTINEL).all()
    bound = (1e-12 if tag == "f64" else 1e-4) * np.abs(want).max()
    err = float(np.abs(got[0, :n_old] - want).max())
    print(f"\n{case} {tag}: plain criteria error / bound = {err / bound:.3g}")
    assert err <= bound, (case, err, bound)


@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", AV.case_names())
def test_estimate_gradient_on_the_executed_reference_kernel(case, tag):
    """estimate_gradient (kernels.cu:471-501) over the faces of the old mesh, with and without an element -> slot map. A cell
    sums at most 24 non-negative terms (6 sides, 4 finer neighbours each) on either side, in different orders: at most 23
    roundings of half an ulp of a partial sum each, so 32 eps max(gradient) holds with room."""
    ins, outs = AV.load(case, tag)
    dtype = DTYPE[tag]
    n_old, _, F, _, _ = AV.sizes(ins)
    rho = np.ascontiguousarray(ins["state"][0])
    want = outs["gradient"].astype(np.float64)
    assert int(np.bincount(ins["fn"], minlength=n_old).max()) <= 24
    bound = 32 * float(np.finfo(NP[dtype]).eps) * want.max()
    perm = np.random.default_rng(zlib.crc32(case.encode())).permutation(n_old).astype(np.int32)
    moved = np.zeros(n_old, NP[dtype])
    moved[perm] = rho
    fn = dev(ins["fn"])
    for name, field, idx in (("map", moved, dev(perm)), ("identity", rho, None)):
        d_rho = dev(field)
        grad = torch.zeros(n_old + SPARE, dtype=dtype, device="cuda")
        hip.call("t8gpu_hip_estimate_gradient", dtype, F, hip.ptr(fn), hip.ptr(idx), hip.ptr(d_rho), hip.ptr(grad), hip.stream_ptr())
        got = host(grad).astype(np.float64)
        assert (got[n_old:] == 0).all()
        got = got[:n_old][perm] if name == "map" else got[:n_old]
        err = float(np.abs(got - want).max())
        print(f"\n{case} {tag} {name}: gradient error / bound = {err / bound:.3g}")
        assert err <= bound, (case, name, err, bound)


# ---- z-order ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", AV.subgrid_cases())
def test_z_order_on_the_executed_reference_kernels(case, tag):
    """column_major_to_z_order (subgrid_mesh_manager.inl:1007-1049), the bit order of the Morton index: `one` is 4 or 8 blocks (a
    single partial workgroup in 2D), mixed2d 4 096 cells in sixteen full workgroups."""
    ins, outs = AV.load(case, tag)
    dtype = DTYPE[tag]
    n_old, _, _, _, rank = AV.sizes(ins)
    S = 4 ** rank
    src = dev(ins["sub_state"][0])
    out = sentinel_planes(1, n_old * S, dtype)
    hip.call("t8gpu_hip_column_major_to_z_order", dtype, rank, n_old, hip.ptr(src), hip.ptr(out), hip.stream_ptr())
    check_planes(host(out), outs["sub_zorder"][None], n_old * S, (case, "z-order"))
    assert np.array_equal(host(src), ins["sub_state"][0])


# ---- partition ----------------------------------------------------------------------------------------------------------
def checked_runs(ins, R):
    """the runs (old owner, first there, new owner, first there, count) of the case with R ranks, inside their owners' ranges"""
    runs, have, noff = ins[f"part{R}_runs"], ins[f"part{R}_have_off"], ins[f"part{R}_new_off"]
    for p, sf, q, df, n in runs:
        assert 0 <= p < R and 0 <= q < R and n > 0 and 0 <= sf and sf + n <= have[p + 1] - have[p] and 0 <= df and df + n <= noff[q + 1] - noff[q]
    return [tuple(int(x) for x in r) for r in runs], have, noff


@pytest.mark.parametrize("R", AV.PART_RANKS)
@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", AV.case_names())
def test_gather_and_scatter_run_by_run(case, tag, R):
    """partition_data (mesh_manager.inl:625-643) as this package moves elements: the old owner gathers a run into a message of six
    planes, the new owner scatters it. R ranks on one GPU; rank p holds the new elements the adapt made from its old ones, rank q
    receives its share of the equal split. The new owners' planes, rank after rank, are the stored variables and volumes."""
    ins, outs = AV.load(case, tag)
    dtype = DTYPE[tag]
    n_new = AV.sizes(ins)[1]
    runs, have, noff = checked_runs(ins, R)
    whole = np.vstack([outs["variables"].reshape(5, n_new), outs["volumes"][None]])
    olds = [dev(np.pad(whole[:, have[p]:have[p + 1]], ((0, 0), (0, 1)))) for p in range(R)]      # (one spare slot: no empty tensor)
    news = [sentinel_planes(6, int(noff[q + 1] - noff[q]), dtype) for q in range(R)]
    s = hip.stream_ptr()
    for p, src_first, q, dst_first, n in runs:
        msg = torch.full((6 * n + SPARE,), SENTINEL, dtype=dtype, device="cuda")
        hip.call("t8gpu_hip_gather_elements", dtype, n, src_first, hip.vars_of(olds[p]), hip.ptr(olds[p][5]), hip.ptr(msg), s)
        m = host(msg)
        assert (m[6 * n:] == SENTINEL).all() and np.array_equal(m[:6 * n].reshape(6, n), whole[:, have[p] + src_first:have[p] + src_first + n])
        hip.call("t8gpu_hip_scatter_elements", dtype, n, dst_first, hip.ptr(msg), hip.vars_of(news[q]), hip.ptr(news[q][5]), s)
    for q in range(R):
        check_planes(host(news[q]), whole[:, noff[q]:noff[q + 1]], int(noff[q + 1] - noff[q]), (case, R, "new owner", q))


def repartition_on_one_rank(ins, dtype, R, cells, vars_whole, vol_whole):
    """t8gpu_hip_repartition with comm = NULL and every run addressed to my_rank (device copies). The R old owners' buffers lie
    in ONE source allocation in reverse rank order with gaps, the new owners' in one destination allocation in rank order with
    other gaps, so that a run moves and a wrong offset lands in a gap or in another rank. Returns the destination planes and
    volumes (host) and the element offset of every new owner in them."""
    runs, have, noff = checked_runs(ins, R)
    n_new = int(have[-1])
    src_base, dst_base, at = {}, {}, 2
    for p in reversed(range(R)):
        src_base[p], at = at, at + int(have[p + 1] - have[p]) + 3
    src_cap, at = at, 1
    for q in range(R):
        dst_base[q], at = at, at + int(noff[q + 1] - noff[q]) + 2
    dst_cap = at
    src = np.full((5, src_cap, cells), SENTINEL, NP[dtype])
    svol = np.full(src_cap, SENTINEL, NP[dtype])
    for p in range(R):
        src[:, src_base[p]:src_base[p] + have[p + 1] - have[p]] = vars_whole.reshape(5, n_new, cells)[:, have[p]:have[p + 1]]
        svol[src_base[p]:src_base[p] + have[p + 1] - have[p]] = vol_whole[have[p]:have[p + 1]]
    d_src, d_svol = dev(src.reshape(5, src_cap * cells)), dev(svol)
    d_dst = torch.full((5, dst_cap * cells), SENTINEL, dtype=dtype, device="cuda")
    d_dvol = torch.full((dst_cap,), SENTINEL, dtype=dtype, device="cuda")
    me = 1
    peer = np.full(len(runs), me, np.int32)
    send_first = np.array([src_base[p] + sf for p, sf, q, df, n in runs], np.int32)
    recv_first = np.array([dst_base[q] + df for p, sf, q, df, n in runs], np.int32)
    count = np.array([n for p, sf, q, df, n in runs], np.int32)
    assert (send_first + count <= src_cap).all() and (recv_first + count <= dst_cap).all()
    hip.call("t8gpu_hip_repartition", dtype, None, me, len(runs), np_ptr(peer), np_ptr(send_first), np_ptr(count), len(runs), np_ptr(peer),
             np_ptr(recv_first), np_ptr(count), hip.vars_of(d_src), hip.ptr(d_svol), hip.vars_of(d_dst), hip.ptr(d_dvol), cells,
             hip.stream_ptr())
    got, gvol = host(d_dst).reshape(5, dst_cap, cells), host(d_dvol)
    assert np.array_equal(host(d_src), src.reshape(5, src_cap * cells))
    return got, gvol, dst_base, noff


def check_repartition(case, tag, R, cells, vars_whole, vol_whole):
    ins, _ = AV.load(case, tag)
    n_new = AV.sizes(ins)[1]
    got, gvol, dst_base, noff = repartition_on_one_rank(ins, DTYPE[tag], R, cells, vars_whole, vol_whole)
    want = np.full_like(got, SENTINEL)
    wvol = np.full_like(gvol, SENTINEL)
    for q in range(R):
        n = int(noff[q + 1] - noff[q])
        want[:, dst_base[q]:dst_base[q] + n] = vars_whole.reshape(5, n_new, cells)[:, noff[q]:noff[q + 1]]
        wvol[dst_base[q]:dst_base[q] + n] = vol_whole[noff[q]:noff[q + 1]]
    assert np.array_equal(got, want) and np.array_equal(gvol, wvol), (case, tag, R, cells)


@pytest.mark.parametrize("R", AV.PART_RANKS)
@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", AV.case_names())
def test_repartition_of_plain_elements(case, tag, R):
    """partition_data (mesh_manager.inl:625-643) through t8gpu_hip_repartition, cells_per_element = 1"""
    _, outs = AV.load(case, tag)
    check_repartition(case, tag, R, 1, outs["variables"], outs["volumes"])


@pytest.mark.parametrize("R", AV.PART_RANKS)
@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("case", AV.subgrid_cases())
def test_repartition_of_subgrid_blocks(case, tag, R):
    """partition_variable_data / partition_volume_data (subgrid_mesh_manager.inl:1216-1280) through t8gpu_hip_repartition,
    cells_per_element = 16 (rank 2) and 64 (rank 3)"""
    ins, outs = AV.load(case, tag)
    check_repartition(case, tag, R, 4 ** AV.sizes(ins)[4], outs["sub_variables"], outs["sub_volumes"])


# ---- the Python layer ---------------------------------------------------------------------------------------------------
def ends_mesh(dim):
    """the old forest of `ends`, as the generator makes it: uniform level 1, refined once everywhere"""
    coarse = SynthMesh(dim, 1, 2, band=0.0)
    return coarse.adapt(np.ones(coarse.num_elements, np.int8))[0]


def carried_sums(stats, state64):
    """plane k of the sums = variable k % 5 of the (float64) state: three groups of five planes"""
    for k in range(stats.sums.shape[0]):
        stats.sums[k] = dev(state64[k % 5])


@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("dim", [2, 3])
def test_amr_adapt_with_the_marks_of_ends(dim, tag, monkeypatch):
    """amr.adapt on a PlainSolver with the marks of `ends` (the criteria walk replaced by the stored marks) reproduces the stored
    variables -- and the stored volumes with volume_dim = 3; carry=(stats,) transfers the float64 sums by the same rule: the
    stored float64 variables, whatever the solver's type."""
    ins, outs = AV.load(f"ends{dim}d", tag)
    ins64, outs64 = AV.load(f"ends{dim}d", "f64")
    n_old, n_new, _, _, _ = AV.sizes(ins)
    mesh = ends_mesh(dim)
    assert mesh.num_elements == n_old
    g = PlainSolver(mesh.partition(), DTYPE[tag], state=ins["state"])
    stats = g.statistics()
    carried_sums(stats, ins64["state"])
    monkeypatch.setattr(mesh, "marks_from_criteria", lambda *a, **k: ins["marks"].copy(), raising=False)
    new, marks, ad = amr.adapt(g, volume_dim=3, carry=(stats,))
    assert np.array_equal(marks, ins["marks"]) and np.array_equal(ad, ins["adapt_data"]) and new.N == n_new
    assert np.array_equal(host(new.state()), outs["variables"].reshape(5, n_new))
    assert np.array_equal(host(new.planes[25, :n_new]), outs["volumes"])
    assert stats.solver is new and stats.sums.shape == (15, n_new)
    assert np.array_equal(host(stats.sums), np.tile(outs64["variables"].reshape(5, n_new), (3, 1)))


@pytest.mark.parametrize("tag", AV.TAGS)
@pytest.mark.parametrize("dim", [2, 3])
def test_amr_adapt_subgrid_with_the_marks_of_ends(dim, tag, monkeypatch):
    """amr.adapt_subgrid on a SubgridSolver with the marks of `ends`: the stored Subgrid variables and volumes, and the carried
    sums by the subcell rule of the block transfer."""
    ins, outs = AV.load(f"ends{dim}d", tag)
    ins64, outs64 = AV.load(f"ends{dim}d", "f64")
    n_old, n_new, _, _, rank = AV.sizes(ins)
    S = 4 ** rank
    mesh = ends_mesh(dim)
    assert mesh.num_elements == n_old and rank == dim
    g = SubgridSolver(mesh.partition(subgrid=True), DTYPE[tag], state=ins["sub_state"])
    stats = g.statistics()
    carried_sums(stats, ins64["sub_state"])
    monkeypatch.setattr(mesh, "marks_from_criteria", lambda *a, **k: ins["marks"].copy(), raising=False)
    new, marks, ad = amr.adapt_subgrid(g, carry=(stats,))
    assert np.array_equal(marks, ins["marks"]) and np.array_equal(ad, ins["adapt_data"]) and new.N == n_new
    assert np.array_equal(host(new.state()), outs["sub_variables"].reshape(5, n_new * S))
    assert np.array_equal(host(new.volumes[:n_new]), outs["sub_volumes"])
    assert stats.solver is new and stats.sums.shape == (15, n_new * S)
    assert np.array_equal(host(stats.sums), np.tile(outs64["sub_variables"].reshape(5, n_new * S), (3, 1)))
