"""include/t8gpu/: code written in the style of the reference's examples must compile against the
HIP-backed headers (CPU check: hipcc cross-compiles gfx950) and, on the GPU box, give the oracle's answer
through all three routes (user-launched kernels on the accessor API, C-ABI compat kernels, fused driver)."""
import os
import subprocess

import numpy as np
import pytest

from t8gpu_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, "tests", "compat")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def compile_example(src, out, defines=()):
    build.build_host()
    build.build_hip()
    srcp, outp = os.path.join(COMPAT, src), os.path.join(COMPAT, out)
    deps = [srcp] + [os.path.join(b, f) for b, _, fs in os.walk(os.path.join(ROOT, "include")) for f in fs]
    if os.path.exists(outp) and all(os.path.getmtime(d) <= os.path.getmtime(outp) for d in deps):
        return outp
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O2", "-DNDEBUG", *defines, "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "t8gpu_amd", "csrc", "hip"), srcp, "-o", outp, "-L", build.LIB, "-lt8gpu_hip",
           "-lt8gpu_host", "-Wl,-rpath," + build.LIB]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return outp


@pytest.mark.parametrize("ft", ["float", "double"])
def test_reference_style_solver_compiles_against_the_headers(ft):
    compile_example("plain_example.hip", f"plain_example_{ft}", (f"-DT8GPU_FLOAT_TYPE={ft}",))


FLOAT_TYPES = ["float", "double"]   # double: nothing else instantiates the fp64 side of adapt / partition / refresh_ghost_layer


def compile_example_for(name, ft):
    return compile_example(f"{name}.hip", f"{name}_{ft}", (f"-DT8GPU_FLOAT_TYPE={ft}",))


@pytest.mark.parametrize("ft", FLOAT_TYPES)
def test_adapt_example_compiles(ft):
    compile_example_for("adapt_example", ft)


@pytest.mark.parametrize("ft", FLOAT_TYPES)
def test_partition_example_compiles(ft):
    compile_example_for("partition_example", ft)


@pytest.mark.parametrize("ft", FLOAT_TYPES)
def test_subgrid_partition_example_compiles(ft):
    compile_example_for("subgrid_partition_example", ft)


def test_subgrid_api_compiles():
    compile_example("subgrid_api.hip", "subgrid_api")


@pytest.mark.gpu
@pytest.mark.parametrize("ft,tol", [("double", 1e-12), ("float", 2e-5)])
@pytest.mark.parametrize("args", [(2, 3, 6, 0.06, 1), (2, 3, 5, 0.06, 0)])
def test_reference_style_solver_matches_the_oracle(ft, tol, args, tmp_path):
    import _oracle as O
    from _gpu import rel_err
    from t8gpu_amd.synth import SynthMesh
    exe = compile_example("plain_example.hip", f"plain_example_{ft}", (f"-DT8GPU_FLOAT_TYPE={ft}",))
    out = str(tmp_path / "out.bin")
    steps = 3
    dim, base, lmax, band, periodic = args
    vtk_prefix = str(tmp_path / "kh")
    subprocess.run([exe, str(dim), str(base), str(lmax), str(band), str(periodic), str(steps), out, vtk_prefix], check=True, timeout=300)
    raw = open(out, "rb").read()
    n, fsz, nsteps = np.frombuffer(raw[:12], np.int32)
    npdt = np.float32 if ft == "float" else np.float64
    assert fsz == np.dtype(npdt).itemsize and nsteps == steps
    res = np.frombuffer(raw[12:], npdt).reshape(3, 5, n)
    mesh = SynthMesh(dim, base, lmax, band=band, periodic=bool(periodic))
    part = mesh.partition()
    assert part.N == n
    o = O.PlainCase(part, npdt)
    dt = npdt(0.1 * 0.5 ** mesh.finest_level)
    for _ in range(steps):
        o.iterate(float(dt))
    want = o.current()[:, :n]
    for name, got in zip(("user kernels on the accessor API", "C-ABI compat kernels", "fused step driver"), res):
        assert rel_err(got, want) < tol * 5, name
    # save_conserved_variables_to_vtk of the fused solver: the file holds exactly its state
    from _vtu import read_vtu
    v = read_vtu(vtk_prefix + ".vtu")
    assert v["n_cells"] == n
    assert np.array_equal(v["arrays"]["density"], res[2][0].astype(np.float64))
    assert np.array_equal(v["arrays"]["energy"], res[2][4].astype(np.float64))
    assert np.array_equal(v["arrays"]["momentum"], res[2][1:4].T.astype(np.float64))


@pytest.mark.gpu
def test_subgrid_api_runs(tmp_path):
    exe = compile_example("subgrid_api.hip", "subgrid_api")
    prefix = str(tmp_path / "sg")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, T8GPU_TEST_VTK_PREFIX=prefix))
    assert res.returncode == 0 and "subgrid_api OK" in res.stdout, res.stdout + res.stderr
    # SyntheticSubgridMeshManager::save_variable_to_vtk / save_mesh_to_vtk: twice-refined blocks in z-order
    from _vtu import read_vtu
    v, mesh = read_vtu(prefix + "_rho.vtu"), read_vtu(prefix + "_mesh.vtu")
    assert v["n_cells"] == 64 * mesh["n_cells"] and set(np.unique(v["arrays"]["variables"])) <= {1.0, 2.0}
    mid = v["arrays"]["Position"].reshape(-1, 8, 3).mean(axis=1)
    inside = np.abs(mid[:, 2] - 0.5) < 0.25
    assert (v["arrays"]["variables"][inside] == 2).all() and (v["arrays"]["variables"][~inside] == 1).all()
    # get_host_{scalar,vector}_variable + save_variables_to_vtk: the same density, and momentum as xyz triples
    f = read_vtu(prefix + "_fields.vtu")
    assert f["n_cells"] == v["n_cells"] and np.array_equal(f["arrays"]["density"], v["arrays"]["variables"])
    assert f["arrays"]["momentum"].shape == (f["n_cells"], 3)
    assert set(np.unique(f["arrays"]["momentum"][:, 0])) <= {-0.5, 0.5}


@pytest.mark.gpu
@pytest.mark.parametrize("ft", FLOAT_TYPES)
def test_partition_example_runs(ft):
    """MeshManager::adapt -> partition -> compute_connectivity_information on 2 and 3 ranks (host threads of one process, loopback
    transport: tests/compat/loopback_transport.h) with fused steps in between: bitwise the single-rank run, shares balanced to one
    element (t8gpu/mesh/mesh_manager.inl:196-330, 626-723). Three further scenarios on 2 - 5 ranks -- coarsening below the initial
    level, where a family cut by a rank boundary stays and the forests legitimately differ -- for the invariants: mass conserved,
    balanced shares, every ghost slot equal to its owner's value after refresh_ghost_layer(). The product's transport is t8gpu::RcclTransport over the same interface
    (t8gpu_hip_repartition_*, t8gpu_hip_comm_allgatherv_f64, t8gpu_hip_halo_exchange_*)."""
    exe = compile_example_for("partition_example", ft)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0 and "partition_example OK" in res.stdout, res.stdout + res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("ft", FLOAT_TYPES)
def test_subgrid_partition_example_runs(ft):
    """SubgridMeshManager::adapt -> partition -> compute_connectivity_information on 2 and 3 ranks (loopback transport), whole
    Subgrid<4,4,4> blocks on the wire (cells_per_element = 64), fused block-kernel steps with the ghost blocks refreshed per stage:
    bitwise the single-rank run (t8gpu/mesh/subgrid_mesh_manager.inl:428-558, 1217-1369); the reference's threshold and half of it
    on 2 - 4 ranks (forests differ where a family is cut) for mass, balance and ghost blocks."""
    exe = compile_example_for("subgrid_partition_example", ft)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0 and "subgrid_partition_example OK" in res.stdout, res.stdout + res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("ft", FLOAT_TYPES)
def test_adapt_example_runs(ft, tmp_path):
    """MeshManager::adapt + the adaptive main loop in C++ (tests/compat/adapt_example.hip): mesh changes, mass is kept."""
    exe = compile_example_for("adapt_example", ft)
    prefix = str(tmp_path / "adapted")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, T8GPU_TEST_VTK_PREFIX=prefix))
    assert res.returncode == 0 and "adapt_example OK" in res.stdout, res.stdout + res.stderr
    from _vtu import read_vtu
    v = read_vtu(prefix + ".vtu")                      # MeshManager::save_variable_to_vtk
    assert v["n_cells"] > 0 and 0.9 < v["arrays"]["variable"].min() and v["arrays"]["variable"].max() < 2.2
