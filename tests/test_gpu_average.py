"""-m gpu: averages along homogeneous axes on the device (t8gpu_hip_sample_average_*, _Solver.average_along,
Statistics.average_along / results_of).

The pin is bitwise: average_along equals sample.host_average -- the numpy statement of the summation order -- applied to the
host copy of resample_uniform(partial=True), which the existing sampling tests tie to their brute force. Where the image is
too large to form (2D, level 13) and for the statistics the reference is the brute force of _average_ref.py, at the
tolerance of test_gpu_sample.py (1e-12 of max |q| per plane on the mean; the argument is in test_average_host.py) and of
test_gpu_stats.py (1e-12 of _stats_ref.scales)."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _average_ref as aref
import _sample_ref as ref
import _stats_ref as sref
import test_gpu_sample as tgs
from _gpu import perturbed_state
from t8gpu_amd import hip, sample, stats as stats_mod
from t8gpu_amd.solver import PlainSolver
from t8gpu_amd.synth import SynthMesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = tgs.DTYPES
MESHES = tgs.MESHES
NAMES = tgs.NAMES
TOL = tgs.TOL
TOL_STATS = 1e-12                                               # test_gpu_stats.TOL
SENTINEL = tgs.SENTINEL
RESULTS = list(stats_mod.RESULTS)
case, host, bits_equal = tgs.case, tgs.host, tgs.bits_equal


def stack(res, names=NAMES):
    """{name: tensor over the bins} -> [planes, bins...] numpy in the order of names"""
    out = []
    for n in names:
        t = host(res[n])
        out.append(t[None] if sample.plane_count(n) == 1 else t)
    return np.concatenate(out)


def cases_of(c):
    """[(axes, L)]: every path of the reduction"""
    if c.dim == 3:
        out = [((0, 1), L) for L in (2, 5, 6, 7)]               # R = 16 (idle lanes), 1024 (a short chunk), 4096, 16384 (finish)
        out += [(axes, L) for axes in ((2,), (0, 2)) for L in (3, 4)]      # the strides of non-leading axes
        return out + [(axes, 3) for axes in ((0,), (1,), (1, 2))]
    top = int(ref.cell_boxes(c.part)[2].max()) + 1              # (Subgrid: the blocks' finest level + 2 + 1)
    return [(axes, L) for axes in ((0,), (1,)) for L in (0, 3, top)]


@functools.lru_cache(maxsize=None)
def image(mesh, subgrid, dtype, L):
    """(sums[planes, n...], weights[n...]) of resample_uniform(NAMES, L, partial=True) on the host: formed once per level"""
    s, w = case(mesh, subgrid, dtype).solver.resample_uniform(NAMES, L, partial=True)
    return stack(s), host(w)


# ---- 1: the main pin -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", MESHES)
def test_average_along_is_host_average_of_the_image_bitwise(mesh, subgrid, dtype):
    c = case(mesh, subgrid, dtype)
    for axes, L in cases_of(c):
        sums, weights = image(mesh, subgrid, dtype, L)
        want_s, want_w = sample.host_average(sums, weights, axes, L, partial=True)
        got, w = c.solver.average_along(NAMES, axes, L, partial=True)
        bins = (1 << L,) * (c.dim - len(axes))
        assert list(got) == NAMES and tuple(w.shape) == bins and w.dtype == torch.float64 and w.is_cuda
        assert tuple(got["density"].shape) == bins and tuple(got["momentum"].shape) == (3,) + bins
        assert bits_equal(host(w), want_w), (axes, L)
        assert bits_equal(stack(got), want_s), (axes, L)
        assert np.all(want_w == 0.5 ** (L * len(bins)))
        mean = c.solver.average_along(NAMES, axes, L)
        assert bits_equal(stack(mean), sample.host_average(sums, weights, axes, L)), (axes, L)
    one = c.solver.average_along("energy", 0, 3)                                   # one name, one axis as an int
    assert bits_equal(host(one["energy"]), sample.host_average(*image(mesh, subgrid, dtype, 3), (0,), 3)[4])


@pytest.mark.parametrize("mesh,subgrid", [("refined-2d-periodic", False), ("refined-2d-walls", True), ("band-2d", False)])
def test_two_chunks_in_2d_at_level_13(mesh, subgrid):
    """R = 8192: two chunks and the finish kernel in the 2D instantiation; the 2^26-pixel image is not formed"""
    c = case(mesh, subgrid, torch.float64)
    L = 13
    q = c.values["density"]
    bs, bw = aref.average(c.part, q, (0,), L)
    s, w = c.solver.average_along("density", (0,), L, partial=True)
    assert tuple(s["density"].shape) == (1 << L,)
    assert np.all(host(w) == 0.5 ** L) and np.all(bw == 0.5 ** L)
    mean = host(c.solver.average_along("density", (0,), L)["density"])
    assert bits_equal(mean, host(s["density"]) / host(w))
    err = np.abs(mean - bs[0] / bw).max() / np.abs(q).max()
    print(f"{mesh} subgrid={subgrid} L={L}: max error / max |q| = {err:.2e}")
    assert err <= TOL


# ---- 2: reproducibility ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,axes,L", [("refined-3d-periodic", (0, 1), 7), ("refined-3d-periodic", (2,), 4), ("refined-2d-walls", (0,), 5)])
@pytest.mark.parametrize("subgrid", [False, True])
def test_two_calls_and_a_side_stream_give_the_same_bits(mesh, axes, L, subgrid):
    c = case(mesh, subgrid, torch.float32)
    a, wa = c.solver.average_along(NAMES, axes, L, partial=True)
    b, wb = c.solver.average_along(NAMES, axes, L, partial=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    s, ws = c.solver.average_along(NAMES, axes, L, partial=True, stream=side)
    side.synchronize()
    assert bits_equal(host(wa), host(wb)) and bits_equal(host(wa), host(ws))
    assert bits_equal(stack(a), stack(b)) and bits_equal(stack(a), stack(s))


# ---- 3: three ranks in one process --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh", ["refined-2d-periodic", "refined-3d-periodic"])
def test_three_ranks_add_up_to_one_rank(mesh, subgrid, dtype):
    names = tgs.CONSERVED + ["pressure"]                            # the pointwise names: no dependence on the partition
    c = case(mesh, subgrid, dtype)
    dim, S = c.dim, c.part.cells_per_element
    L = tgs.LEVELS[dim][1]
    q = np.concatenate([c.values[n] for n in names])
    scale = np.abs(q).max(axis=1)
    solvers = []
    for r in range(3):
        part = ref.partition(mesh, subgrid, r, 3)
        gidx = np.concatenate([np.arange(part.first_global, part.first_global + part.N), part.ghost_global])
        cols = (gidx[:, None] * S + np.arange(S)[None, :]).reshape(-1)
        solvers.append((part, tgs.make_solver(part, dtype, c.state[:, cols])))
    empty_bins = 0
    for axes in aref.axis_sets(dim):
        one_s, one_w = c.solver.average_along(names, axes, L, partial=True)
        one = stack(c.solver.average_along(names, axes, L), names)
        sums, weights = 0.0, 0.0
        for part, solver in solvers:
            s, w = solver.average_along(names, axes, L, partial=True)
            w = host(w)
            _, bw = aref.average(part, np.zeros((1, part.N * S)), axes, L)
            assert np.array_equal(w == 0.0, bw == 0.0) and np.all(w == bw), axes       # weight 0 exactly where it owns nothing
            empty_bins += int((w == 0.0).sum())
            mean = stack(solver.average_along(names, axes, L, fill=SENTINEL), names)
            assert np.all((mean == SENTINEL) == (w == 0.0)[None]), axes
            assert bits_equal(mean, np.where(w > 0.0, stack(s, names) / np.where(w > 0.0, w, 1.0), SENTINEL))
            sums, weights = sums + stack(s, names), weights + w
        assert bits_equal(weights, host(one_w)), axes
        err = np.abs(sums / weights - one).reshape(len(scale), -1).max(axis=1)
        assert np.all(err <= TOL * scale), (axes, err / scale)
        assert bits_equal(one, stack(one_s, names) / host(one_w))
    assert empty_bins > 0


# ---- 4: extra planes and a derived name ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh,axes,L", [("refined-2d-walls", (1,), 4), ("refined-3d-periodic", (0, 2), 3)])
def test_a_derived_name_equals_its_field_passed_as_an_extra(mesh, axes, L, subgrid):
    c = case(mesh, subgrid, torch.float32)
    p = c.solver.derived_fields("pressure")["pressure"]
    a = c.solver.average_along(["pressure", "density"], axes, L)
    b = c.solver.average_along(["mine", "density"], axes, L, extra={"mine": p})
    assert bits_equal(host(a["pressure"]), host(b["mine"])) and bits_equal(host(a["density"]), host(b["density"]))
    two = c.solver.average_along("pair", axes, L, extra={"pair": torch.stack([p, 2.0 * p])})
    assert tuple(two["pair"].shape) == (2,) + tuple(a["pressure"].shape)
    assert bits_equal(host(two["pair"][0]), host(a["pressure"]))
    with pytest.raises(ValueError):
        c.solver.average_along("density", axes, L, extra={"density": p})


# ---- 5: statistics -----------------------------------------------------------------------------------------------------------
def check_results(got, want, scale, what):
    """got {name: tensor over the bins}, want [19, bins] (flattened bins), scale [19]"""
    for name in RESULTS:
        rows = sref.SLOTS[name]
        g = host(got[name]).reshape(len(rows), -1)
        for i, k in enumerate(rows):
            err = np.abs(g[i] - want[k]).max()
            print(f"{what} {name}[{i}]: max error / scale = {err / max(scale[k], 1e-300):.2e}")
            assert err <= TOL_STATS * scale[k], (what, name, i, err, scale[k])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("subgrid", [False, True])
@pytest.mark.parametrize("mesh,axes,L", [("refined-2d-periodic", (0,), 3), ("refined-3d-periodic", (0, 2), 3), ("refined-3d-periodic", (2,), 2)])
def test_statistics_are_formed_from_the_bin_averaged_sums(mesh, axes, L, subgrid, dtype):
    part = ref.partition(mesh, subgrid)
    solver = tgs.make_solver(part, dtype, perturbed_state(part, 21))
    st = solver.statistics()
    with pytest.raises(ValueError):
        st.average_along(RESULTS, axes, L)                          # before any accumulate
    dt = 0.1 * 2.0 ** -(part.mesh.finest_level + (2 if subgrid else 0))
    for w in (0.3, 1.7):
        solver.iterate(dt)
        st.accumulate(w)
    bs, bw = aref.average(part, host(st.sums), axes, L)
    mean = (bs / bw).reshape(sref.PLANES, -1)
    got = st.average_along(RESULTS, axes, L)
    bins = (1 << L,) * (part.mesh.dim - len(axes))
    assert tuple(got["tke"].shape) == bins and tuple(got["reynolds_stress"].shape) == (6,) + bins
    check_results(got, sref.results(mean, st.weight), sref.scales(mean, st.weight), f"{mesh} {axes} L={L}")
    # the partial form, divided, through results_of: the non-partial call bit for bit
    s15, w = st.average_along(RESULTS, axes, L, partial=True)
    assert tuple(s15.shape) == (15,) + bins and tuple(w.shape) == bins
    again = st.results_of(s15 / w, RESULTS)
    for name in RESULTS:
        assert bits_equal(host(again[name]), host(got[name])), name
    assert bits_equal(host(st.results_of(s15 / w, "tke", weight=st.weight)["tke"]), host(got["tke"]))
    with pytest.raises(ValueError):
        st.results_of(s15[:14], RESULTS)
    with pytest.raises(ValueError):
        st.average_along(["tke", "enstrophy"], axes, L)


@pytest.mark.parametrize("subgrid", [False, True])
def test_a_state_uniform_along_x_gives_the_cell_statistics_of_its_row(subgrid):
    part = SynthMesh(2, 3, 3).partition(subgrid=subgrid)
    lo, _, level = ref.cell_boxes(part)
    cells = lo.shape[0]
    state = perturbed_state(part, 5)
    assert state.shape[1] == cells
    first = {}                                                      # y -> the row's cell of smallest x
    for i in np.argsort(lo[:, 0], kind="stable"):
        first.setdefault(lo[i, 1], i)
    row = np.array([first[y] for y in lo[:, 1]])
    solver = tgs.make_solver(part, torch.float64, state[:, row])
    st = solver.statistics()
    for k, w in enumerate((0.3, 1.7)):                              # two different states, both uniform along x
        solver.planes[5 * solver.next + 4] *= 1.0 + 0.1 * k
        st.accumulate(w)
    cellwise = np.concatenate([host(t).reshape(-1, cells) for t in st.results(RESULTS).values()])
    scale = sref.scales(host(st.sums), st.weight)
    fine = int(level.max())
    for L in (fine, fine + 1):                                      # a bin is a row of cells, or half of one
        ys = (np.arange(1 << L) + 0.5) / (1 << L)
        pick = np.array([first[lo[(lo[:, 1] <= y) & (y < lo[:, 1] + 0.5 ** fine), 1][0]] for y in ys])
        check_results(st.average_along(RESULTS, (0,), L), cellwise[:, pick], scale, f"uniform rows L={L}")


# ---- 6: refusals and the C entry point ----------------------------------------------------------------------------------------
def test_refusals():
    from t8gpu_amd.unstructured import PrismHexMesh
    part = PrismHexMesh(5).partition()
    curved = PlainSolver(part, torch.float64, mode="compat", state=perturbed_state(part, 11))
    with pytest.raises(TypeError):
        curved.average_along("density", (0,), 2)
    for dim, mesh in ((2, "refined-2d-walls"), (3, "refined-3d-periodic")):
        c = case(mesh, False, torch.float64)
        for bad in ((), tuple(range(dim)), (0, 0), (dim,), (-1,)):
            with pytest.raises(ValueError):
                c.solver.average_along("density", bad, 2)
        for level in (-1, sample.DEPTH + 1):
            with pytest.raises(ValueError):
                c.solver.average_along("density", (0,), level)
        with pytest.raises(ValueError, match="16"):
            c.solver.average_along("many", (0,), 2, extra={"many": torch.zeros((17, c.cells), dtype=torch.float64, device="cuda")})
        with pytest.raises(ValueError, match="density"):
            c.solver.average_along(["density", "enstrophy"], (0,), 2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_c_entry_refuses_bad_masks_and_a_missing_scratch_before_any_launch(dtype):
    c = case("refined-2d-walls", False, dtype)
    s = sample.sampler(c.solver)
    fn = getattr(hip.lib(), f"t8gpu_hip_sample_average_{hip.suffix(dtype)}")
    fn.restype = ctypes.c_int
    src = sample.SamplePlanes()
    src.q[0] = c.solver.planes[5 * c.solver.next].data_ptr()
    invalid = 1                                                     # hipErrorInvalidValue

    def call(dim, level, mask, planes=1, bins=8):
        """the entry point with outputs of `bins` sentinels and no scratch: (return code, sums, weights) afterwards"""
        sums = torch.full((bins,), SENTINEL, dtype=torch.float64, device="cuda")
        weights = torch.full((bins,), SENTINEL, dtype=torch.float64, device="cuda")
        code = fn(dim, level, mask, hip.ptr(s.keys), hip.ptr(s.levels), s.N, 1, planes, src, ctypes.c_double(0.0), hip.ptr(sums),
                  hip.ptr(weights), None, hip.stream_ptr())
        torch.cuda.synchronize()
        return code, host(sums), host(weights)

    refused = [(2, 3, mask, 1) for mask in (0, 3, 4, 7, -1)]        # empty, full, an axis the mesh has not
    refused += [(2, 13, 1, 1)]                                      # R = 8192 > 4096 and no scratch
    refused += [(2, -1, 1, 1), (2, sample.DEPTH + 1, 1, 1), (2, 19, 1, 1), (4, 3, 1, 1), (2, 3, 1, 0), (2, 3, 1, 17)]
    for dim, level, mask, planes in refused:
        code, sums, weights = call(dim, level, mask, planes)
        assert code == invalid and np.all(sums == SENTINEL) and np.all(weights == SENTINEL), (dim, level, mask, planes)
    code, sums, weights = call(2, 3, 1)                             # the same call with a good mask runs
    want = c.solver.average_along("density", (0,), 3, partial=True)
    assert code == 0 and bits_equal(sums, host(want[0]["density"])) and bits_equal(weights, host(want[1]))


# ---- 7: the example ----------------------------------------------------------------------------------------------------------
def test_kelvin_helmholtz_example_writes_profiles_that_keep_the_mass(tmp_path):
    L = 5
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "kelvin_helmholtz_amr.py"), "--steps", "12", "--adapt-every", "6",
                          "--min-level", "3", "--max-level", "5", "--stats", "--stats-every", "2", "--vtk", str(tmp_path / "kh"),
                          "--profile", str(L), "--profile-every", "6"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = re.findall(r"profiles at it (\d+): .* mass (\S+)  momentum thickness (\S+)", out.stdout)
    assert [int(l[0]) for l in lines] == [6, 12], out.stdout
    for it, mass, theta in lines:
        rho = np.load(str(tmp_path / f"kh_profile_mean_density_{int(it):06d}.npy"))
        u = np.load(str(tmp_path / f"kh_profile_favre_velocity_x_{int(it):06d}.npy"))
        assert rho.shape == (1 << L,) and u.shape == (1 << L,) and np.all(rho > 0) and np.all(np.isfinite(u))
        # the integral of the profile is the mass: both sum the same cell values, in another order
        assert abs(rho.sum() * 0.5 ** L - float(mass)) <= TOL * rho.max(), (it, rho.sum() * 0.5 ** L, mass)
        assert u.max() > u.min() and 0.0 < float(theta) < 1.0       # two streams; theta <= max rho / (4 mean rho)
        stress = np.load(str(tmp_path / f"kh_profile_reynolds_stress_{int(it):06d}.npy"))
        tke = np.load(str(tmp_path / f"kh_profile_tke_{int(it):06d}.npy"))
        assert stress.shape == (6, 1 << L) and tke.shape == (1 << L,) and np.all(np.isfinite(stress)) and np.all(tke >= -1e-12)
    plain = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "kelvin_helmholtz_amr.py"), "--steps", "2", "--min-level", "3",
                            "--max-level", "4"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert plain.returncode == 0 and "profiles" not in plain.stdout
