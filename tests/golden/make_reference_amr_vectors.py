#!/usr/bin/env python3
"""Generates tests/golden/reference_amr_vectors.npz and reference_amr_vectors_rank3.npz (the Subgrid arrays of the rank-3 cases,
apart so that each file stays below the size limit of a committed file): outputs of the REFERENCE's own AMR, indicator, read-back and partition
KERNEL BODIES on tiny forests.

Build container only (needs the reference tree; tests read the committed .npz). make_reference_kernel_vectors.py executes the
reference's flux and Runge-Kutta kernels; this script executes the other half of its device code, the kernels that carry the
state through every adapt and repartition:
  * adapt_variables_and_volume                     t8gpu/mesh/mesh_manager.inl:164-193
  * adapt_volume / adapt_variables, rank 2 and 3   t8gpu/mesh/subgrid_mesh_manager.inl:245-425
  * compute_refinement_criteria<Subgrid>           examples/subgrid/kernels.inl:1109-1168
  * estimate_gradient                              examples/compressible_euler/kernels.cu:471-501
  * compute_refinement_criteria                    examples/compressible_euler/solver.cu:231-241
  * column_major_to_z_order, rank 2 and 3          t8gpu/mesh/subgrid_mesh_manager.inl:1007-1049
  * partition_data                                 t8gpu/mesh/mesh_manager.inl:625-643
  * partition_variable_data / partition_volume_data  t8gpu/mesh/subgrid_mesh_manager.inl:1216-1280
Those line ranges go into a TEMPORARY directory beside the accessor classes the other generator extracts (COMMON, lines and
between are imported from it); nothing of the reference's text is written into this repository, the .npz holds input and
output arrays and one provenance string. The stand-ins are the other generator's: CUDA built-ins as plain structs, atomicAdd as
a sequential read-modify-write, builder classes of the accessors' friend names, two-line solver structs. None of these kernels
has a barrier: a launch is a plain loop over blocks and threads (so estimate_gradient accumulates in face order). fp64 by the
same `= float;` -> `= double;` edit of variable_traits. Parity stays "unpinned" for the same reason as there.

Cases (fp32 and fp64 each; every adapt_data comes from SynthMesh.adapt and is a real forest; states are seeded perturbed()
values). The plain kernels run on 2D and 3D forests, the Subgrid kernels on the same forests with rank = dim; the rank-3
`mixed` forest would be too large for a committed fixture and `refined_ends` is for the plain kernels only:
  mixed          uniform SynthMesh(dim, 2, 4 | 3, band=0.2); -1 where x < 0.5, a seeded 0/1 where x > 0.75, last element refined
  ends           uniform level 1 refined once everywhere; then the first family -1 and the last two elements +1: a coarsened
                 family at e = 0, two refined parents back to back, the last child at e = n_new - 1
  one            uniform level 1, every element -1: one new element, adapt_data = [0, 2^dim]
  refined_ends   SynthMesh(dim, 2, 3, band=0.2); a seeded -1/0/+1, the first family and the last element forced to +1: a refined
                 family at e = 0
Per case: the transfer (new variables and volumes), the indicators on the OLD mesh (estimate_gradient's rho-flux plane over its
faces, both criteria arrays), the z-order of the old Subgrid density plane, and the partition kernels with two and three
"ranks" as arrays of per-rank pointers. The partition moves the adapted elements from where the adapt left them (rank p holds
the new elements made from its old ones) to the equal split of the new curve: ranks[] / indices[] per new element and the
contiguous runs they form are stored as inputs. The partition kernels copy, so what they write, rank after rank, IS the stored
new variables and volumes: the script asserts that of the executed reference kernels and does not store the same arrays twice.
The step censuses below are asserted, so a change of the mesh provider cannot empty a case silently.
"""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_reference_kernel_vectors import COMMON, REF, between, lines, perturbed  # noqa: E402

PART_RANKS = (2, 3)

# name -> (n_old, n_new, {step of adapt_data: count}): what each case reaches
CENSUS = {
    "mixed2d": (256, 289, {0: 111, 1: 152, 4: 26}),
    "mixed3d": (512, 750, {0: 357, 1: 376, 8: 17}),
    "ends2d": (16, 19, {0: 6, 1: 12, 4: 1}),
    "ends3d": (64, 71, {0: 14, 1: 56, 8: 1}),
    "one2d": (4, 1, {4: 1}),
    "one3d": (8, 1, {8: 1}),
    "refined_ends2d": (64, 181, {0: 117, 1: 64}),
    "refined_ends3d": (512, 1702, {0: 1190, 1: 512}),
}

DRIVER = COMMON + r"""
#include "ref_meta.inl"
namespace t8gpu {
  enum VariableList { Rho, Rho_v1, Rho_v2, Rho_v3, Rho_e, nb_variables };   // examples/compressible_euler/solver.h:14-21
#include "ref_mem.inl"
#include "ref_submem.inl"
  // the friends that may construct the accessors: builders only
  template<typename VT, typename ST> class MemoryManager {
   public:
    using ft = typename variable_traits<VT>::float_type;
    static MemoryAccessorOwn<VT> own(std::array<ft*, 5> a) { return MemoryAccessorOwn<VT>(a); }
    static MemoryAccessorAll<VT> all(std::array<ft* const*, 5> a) { return MemoryAccessorAll<VT>(a); }
  };
  template<typename VT, typename ST, typename SG> class SubgridMemoryManager {
   public:
    using ft = typename variable_traits<VT>::float_type;
    static SubgridMemoryAccessorOwn<VT, SG> own(std::array<ft*, 5> a) { return SubgridMemoryAccessorOwn<VT, SG>(a); }
    static SubgridMemoryAccessorAll<VT, SG> all(std::array<ft* const*, 5> a) { return SubgridMemoryAccessorAll<VT, SG>(a); }
  };
#include "ref_conn.inl"
  template<typename VT, typename ST, size_t dim_> class MeshManager {
   public:
    using ft = typename variable_traits<VT>::float_type;
    static MeshConnectivityAccessor<ft, dim_> conn(int const* ranks, t8_locidx_t const* idx, t8_locidx_t const* fn, ft const* nrm,
                                                   ft const* ar, t8_locidx_t F, t8_locidx_t B) {
      return MeshConnectivityAccessor<ft, dim_>(ranks, idx, fn, nrm, ar, F, B);
    }
  };
  struct CompressibleEulerSolver { static constexpr size_t dim = 3; };      // compressible_euler/solver.h:36
#include "ref_kernels_h.inl"
}
template<typename SG> struct SubgridCompressibleEulerSolver {                 // subgrid/solver.h:35
  using float_type = typename t8gpu::variable_traits<t8gpu::VariableList>::float_type;
};
using namespace t8gpu;
#include "ref_adapt_plain.inl"
#include "ref_partition_plain.inl"
#include "ref_estimate_gradient.inl"
#include "ref_criteria_plain.inl"
#include "ref_adapt_subgrid.inl"
#include "ref_zorder.inl"
#include "ref_partition_subgrid.inl"
#include "ref_criteria_subgrid.inl"
using FT = variable_traits<VariableList>::float_type;
using Restricted = std::array<FT* __restrict__, 5>;
static const Dim3 line{256, 1, 1};
static unsigned blocks(int n) { return (n + 255) / 256; }

// The partition kernels with R "ranks": rank p holds new elements [have[p], have[p+1]) in buffers of its own, the new owner q
// pulls its elements [noff[q], noff[q+1]) through arrays of per-rank pointers. cells = values per element and variable.
template<class Launch>
static void partition(const std::string& d, const std::string& pre, int R, int n_new, size_t cells, const std::vector<FT>& vars,
                      const std::vector<FT>& vol, Launch&& pull) {
  const std::string p = d + "/part" + std::to_string(R);
  auto rk = rd<int32_t>(p + "_ranks.bin"), ix = rd<int32_t>(p + "_indices.bin"), have = rd<int32_t>(p + "_have_off.bin"),
       noff = rd<int32_t>(p + "_new_off.bin");
  std::vector<std::vector<FT>> buf(5 * R), vbuf(R);
  std::vector<FT*> ptr(5 * R), vptr(R);
  for (int q = 0; q < R; q++) {
    for (int k = 0; k < 5; k++) {
      buf[k * R + q].assign(vars.begin() + (k * (size_t)n_new + have[q]) * cells, vars.begin() + (k * (size_t)n_new + have[q + 1]) * cells);
      ptr[k * R + q] = buf[k * R + q].data();
    }
    vbuf[q].assign(vol.begin() + have[q], vol.begin() + have[q + 1]);
    vptr[q] = vbuf[q].data();
  }
  std::array<FT* const*, 5> all;
  for (int k = 0; k < 5; k++) all[k] = ptr.data() + k * R;
  std::vector<FT> out(5 * (size_t)n_new * cells, FT(-1)), ovol(n_new, FT(-1));
  for (int q = 0; q < R; q++) {
    const int nq = noff[q + 1] - noff[q];
    Restricted nv;
    for (int k = 0; k < 5; k++) nv[k] = out.data() + (k * (size_t)n_new + noff[q]) * cells;
    pull(rk.data() + noff[q], ix.data() + noff[q], nv, all, ovol.data() + noff[q], vptr.data(), nq);
  }
  wr(d + "/" + pre + "part" + std::to_string(R) + "_variables.bin", out);
  wr(d + "/" + pre + "part" + std::to_string(R) + "_volumes.bin", ovol);
}

template<class SG> static void subgrid(const std::string& d, int n_old, int n_new, std::vector<int32_t>& ad, std::vector<FT>& vol) {
  constexpr int S = SG::size, R = SG::rank;
  auto st = rd<FT>(d + "/sub_state.bin");
  std::vector<FT> out(5 * (size_t)n_new * S, FT(-1)), nvol(n_new, FT(-1)), crit(n_old, FT(-1)), zo((size_t)n_old * S, FT(-1));
  std::array<FT*, 5> sp;
  Restricted op;
  for (int k = 0; k < 5; k++) { sp[k] = st.data() + (size_t)k * n_old * S; op[k] = out.data() + (size_t)k * n_new * S; }
  using MM = SubgridMemoryManager<VariableList, int, SG>;
  const auto v = MM::own(sp);
  const Dim3 cell = R == 3 ? Dim3{4, 4, 4} : Dim3{4, 4, 1};
  // SubgridMeshManager::adapt (subgrid_mesh_manager.inl:486-499), SubgridCompressibleEulerSolver::adapt (solver.inl:329-340),
  // save_variable_to_vtk (subgrid_mesh_manager.inl:1060-1063)
  launch(blocks(n_new), line, [&] { adapt_volume<VariableList, SG>(vol.data(), nvol.data(), ad.data(), n_new); }, false);
  launch(n_new, cell, [&] { adapt_variables<VariableList, SG>(v, op, ad.data()); }, false);
  launch(blocks(n_old), line, [&] { compute_refinement_criteria<SG>(v.get(Rho), crit.data(), vol.data(), n_old); }, false);
  launch(n_old, cell, [&] { column_major_to_z_order<FT, SG>(st.data(), zo.data()); }, false);
  wr(d + "/sub_variables.bin", out);
  wr(d + "/sub_volumes.bin", nvol);
  wr(d + "/sub_criteria.bin", crit);
  wr(d + "/sub_zorder.bin", zo);
  for (int ranks = 2; ranks <= 3; ranks++)
    partition(d, "sub_", ranks, n_new, S, out, nvol,
              [&](int* rk, t8_locidx_t* ix, Restricted nv, std::array<FT* const*, 5> all, FT* ovol, FT* const* vptr, int nq) {
                const auto old = MM::all(all);
                launch(nq, cell, [&] { partition_variable_data<VariableList, SG>(rk, ix, nv, old); }, false);
                launch(blocks(nq), line, [&] { partition_volume_data<VariableList>(rk, ix, ovol, vptr, nq); }, false);
              });
}

int main(int, char** argv) {
  const std::string d = argv[1];
  const int rank = std::atoi(argv[2]);          // 0: no Subgrid run
  auto sz = rd<int32_t>(d + "/sizes.bin");      // n_old, n_new, F
  const int n_old = sz[0], n_new = sz[1], F = sz[2];
  auto ad = rd<int32_t>(d + "/adapt_data.bin"), fn = rd<int32_t>(d + "/fn.bin");
  auto st = rd<FT>(d + "/state.bin"), vol = rd<FT>(d + "/volume.bin");
  using MM = MemoryManager<VariableList, int>;
  std::array<FT*, 5> sp;
  for (int k = 0; k < 5; k++) sp[k] = st.data() + (size_t)k * n_old;
  {   // MeshManager::adapt (mesh_manager.inl:258-281)
    std::vector<FT> out(5 * (size_t)n_new, FT(-1)), nvol(n_new, FT(-1));
    Restricted op;
    for (int k = 0; k < 5; k++) op[k] = out.data() + (size_t)k * n_new;
    const auto v = MM::own(sp);
    launch(blocks(n_new), line, [&] { adapt_variables_and_volume<VariableList>(v, op, vol.data(), nvol.data(), ad.data(), n_new); }, false);
    wr(d + "/variables.bin", out);
    wr(d + "/volumes.bin", nvol);
    for (int ranks = 2; ranks <= 3; ranks++)
      partition(d, "", ranks, n_new, 1, out, nvol,
                [&](int* rk, t8_locidx_t* ix, Restricted nv, std::array<FT* const*, 5> all, FT* ovol, FT* const* vptr, int nq) {
                  const auto old = MM::all(all);
                  launch(blocks(nq), line, [&] { partition_data<VariableList>(rk, ix, nv, old, ovol, vptr, nq); }, false);
                });
  }
  {   // CompressibleEulerSolver::adapt (solver.cu:243-263): the gradient into the (zeroed) Fluxes planes, then the criteria
    std::vector<int> ranks(n_old, 0);
    std::vector<int32_t> idx(n_old);
    for (int i = 0; i < n_old; i++) idx[i] = i;
    std::vector<FT> flux(5 * (size_t)n_old, FT(0)), crit(n_old, FT(-1));
    std::array<FT*, 5> fp;
    std::array<FT* const*, 5> spp, fpp;
    for (int k = 0; k < 5; k++) { fp[k] = flux.data() + (size_t)k * n_old; spp[k] = &sp[k]; fpp[k] = &fp[k]; }
    const auto conn = MeshManager<VariableList, int, 3>::conn(ranks.data(), idx.data(), fn.data(), nullptr, nullptr, F, 0);
    const auto next = MM::all(spp), fluxes = MM::all(fpp);
    launch(blocks(F), line, [&] { estimate_gradient(conn, next, fluxes); }, false);
    launch(blocks(n_old), line, [&] { compute_refinement_criteria(fp[0], vol.data(), crit.data(), n_old); }, false);
    for (size_t i = n_old; i < flux.size(); i++) if (flux[i] != FT(0)) return 4;      // only the rho plane is written
    wr(d + "/gradient.bin", std::vector<FT>(flux.begin(), flux.begin() + n_old));
    wr(d + "/criteria.bin", crit);
  }
  if (rank == 3) subgrid<Subgrid<4, 4, 4>>(d, n_old, n_new, ad, vol);
  if (rank == 2) subgrid<Subgrid<4, 4>>(d, n_old, n_new, ad, vol);
  return 0;
}
"""


def forests():
    """name -> (old mesh, marks, Subgrid rank or 0)"""
    from t8gpu_amd.synth import SynthMesh
    out = {}
    for dim in (2, 3):
        mesh = SynthMesh(dim, 2, 4 if dim == 2 else 3, band=0.2)
        x = mesh.partition().centres[:mesh.num_elements, 0]
        rng = np.random.default_rng(7 + dim)
        marks = np.where(x < 0.5, -1, np.where(x > 0.75, rng.integers(0, 2, mesh.num_elements), 0)).astype(np.int8)
        marks[-1] = 1
        out[f"mixed{dim}d"] = (mesh, marks, 2 if dim == 2 else 0)

        coarse = SynthMesh(dim, 1, 2, band=0.0)
        mesh = coarse.adapt(np.ones(coarse.num_elements, np.int8))[0]
        marks = np.zeros(mesh.num_elements, np.int8)
        marks[:2 ** dim] = -1
        marks[-2:] = 1
        out[f"ends{dim}d"] = (mesh, marks, dim)

        out[f"one{dim}d"] = (coarse, -np.ones(coarse.num_elements, np.int8), dim)

        mesh = SynthMesh(dim, 2, 3, band=0.2)
        marks = np.random.default_rng(7 + dim).integers(-1, 2, mesh.num_elements).astype(np.int8)
        marks[:2 ** dim] = 1
        marks[-1] = 1
        out[f"refined_ends{dim}d"] = (mesh, marks, 0)
    return out


def partition_plan(old_mesh, new_mesh, adapt_data, R):
    """Where the adapt leaves the new elements (rank p: those made from its old elements) and where the equal split of the new
    curve wants them. Returns have_off, new_off [R + 1], ranks, indices [n_new] (old owner and position in its buffers, per new
    element in curve order) and runs [nruns, 5] = (old owner, first there, new owner, first there, count)."""
    n_new = new_mesh.num_elements
    have = np.searchsorted(adapt_data[:-1], old_mesh.partition_offsets(R), side="left").astype(np.int64)
    have[-1] = n_new
    noff = new_mesh.partition_offsets(R)
    g = np.arange(n_new)
    ranks = (np.searchsorted(have, g, side="right") - 1).astype(np.int32)
    indices = (g - have[ranks]).astype(np.int32)
    runs = []
    for p in range(R):
        for q in range(R):
            s0, s1 = max(int(have[p]), int(noff[q])), min(int(have[p + 1]), int(noff[q + 1]))
            if s1 > s0:
                runs.append((p, s0 - int(have[p]), q, s0 - int(noff[q]), s1 - s0))
    runs = np.array(runs, np.int32).reshape(-1, 5)
    assert int(runs[:, 4].sum()) == n_new
    return have.astype(np.int32), noff.astype(np.int32), ranks, indices, runs


def write_npz(path, arrays):
    """an .npz that np.load reads, with fixed member dates: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    if not os.path.isdir(REF):
        sys.exit(f"this generator needs the reference tree at {REF} (build container only)")
    cases = {}
    for cname, (mesh, marks, rank) in forests().items():
        new_mesh, ad = mesh.adapt(marks)
        steps = np.diff(ad)
        census = {int(k): int((steps == k).sum()) for k in np.unique(steps)}
        n_old, n_new, want = CENSUS[cname]
        assert (mesh.num_elements, new_mesh.num_elements, census) == (n_old, n_new, want), (cname, mesh.num_elements, new_mesh.num_elements, census)
        if cname.startswith("refined_ends"):
            assert list(ad[:2 ** mesh.dim + 1]) == [0] * 2 ** mesh.dim + [1], (cname, ad[:9])   # a refined family at e = 0
        if cname.startswith("ends"):
            assert ad[1] == 2 ** mesh.dim and list(ad[-2 ** mesh.dim - 1:]) == [mesh.num_elements - 1] * 2 ** mesh.dim + [mesh.num_elements]
        cases[cname] = (mesh, marks, rank, new_mesh, ad.astype(np.int32), census)
    res = {}
    with tempfile.TemporaryDirectory(prefix="t8gpu_refamr_") as tmp:
        w = lambda name, text: open(os.path.join(tmp, name), "w").write(text)
        w("ref_meta.inl", between("t8gpu/utils/meta.h", "namespace t8gpu::meta {", "#endif  // UTILS_META_H"))
        mem = between("t8gpu/memory/memory_manager.h", "// Type traits are necessary", "  class MemoryManager {")
        mem = mem[:mem.rindex("  template<typename VariableType, typename StepType>")]
        sub = between("t8gpu/memory/subgrid_memory_manager.h", "// Forward declarations.", "  class SubgridMemoryManager {")
        sub = sub[:sub.rindex("  template<typename VariableType, typename StepType, typename SubgridType>")]
        w("ref_submem.inl", sub)
        w("ref_conn.inl", between("t8gpu/mesh/mesh_manager.h", "/// Forward declaration of MeshManager class", "/// @brief class that represents a distributed mesh"))
        w("ref_kernels_h.inl", between("examples/compressible_euler/kernels.h", "__global__ void kepes_compute_fluxes", "}  // namespace t8gpu"))
        w("ref_adapt_plain.inl", lines("t8gpu/mesh/mesh_manager.inl", 164, 193))
        w("ref_partition_plain.inl", lines("t8gpu/mesh/mesh_manager.inl", 625, 643))
        w("ref_estimate_gradient.inl", lines("examples/compressible_euler/kernels.cu", 471, 501))
        w("ref_criteria_plain.inl", lines("examples/compressible_euler/solver.cu", 231, 241))
        w("ref_adapt_subgrid.inl", lines("t8gpu/mesh/subgrid_mesh_manager.inl", 245, 425))
        w("ref_zorder.inl", lines("t8gpu/mesh/subgrid_mesh_manager.inl", 1007, 1049))
        w("ref_partition_subgrid.inl", lines("t8gpu/mesh/subgrid_mesh_manager.inl", 1216, 1280))
        w("ref_criteria_subgrid.inl", lines("examples/subgrid/kernels.inl", 1109, 1168))
        w("amr.cpp", DRIVER)
        for ft, npdt, tag in (("double", np.float64, "f64"), ("float", np.float32, "f32")):
            text = mem
            if ft == "double":
                assert text.count("= float;") == 2
                text = text.replace("= float;", "= double;")
            w("ref_mem.inl", text)
            exe = os.path.join(tmp, "amr_" + tag)
            subprocess.check_call(["g++", "-std=c++17", "-O0", "-ffp-contract=off", "-pthread", "-w", "-I", tmp, os.path.join(tmp, "amr.cpp"),
                                   "-o", exe])
            for cname, (mesh, marks, rank, new_mesh, ad, census) in cases.items():
                part = mesh.partition()
                n_old, n_new, F, S = part.N, new_mesh.num_elements, part.F, 4 ** rank if rank else 0
                seed = sum(ord(c) for c in cname)
                d = os.path.join(tmp, f"{cname}_{tag}")
                os.makedirs(d)
                ins = {"sizes": np.array([n_old, n_new, F, mesh.dim, rank], np.int32),
                       "adapt_data": ad, "marks": marks.astype(np.int8),
                       "fn": np.ascontiguousarray(part.face_neighbors[:2 * F], np.int32),
                       "state": np.ascontiguousarray(perturbed(n_old, seed), npdt),
                       "volume": np.ascontiguousarray(part.volumes[:n_old], npdt)}
                if rank:
                    ins["sub_state"] = np.ascontiguousarray(perturbed(n_old * S, seed + 1), npdt)
                for R in PART_RANKS:
                    have, noff, ranks, indices, runs = partition_plan(mesh, new_mesh, ad, R)
                    ins.update({f"part{R}_have_off": have, f"part{R}_new_off": noff, f"part{R}_ranks": ranks, f"part{R}_indices": indices,
                                f"part{R}_runs": runs})
                for k, v in ins.items():
                    v.tofile(os.path.join(d, k + ".bin"))
                subprocess.check_call([exe, d, str(rank)])
                out = lambda k: np.fromfile(os.path.join(d, k + ".bin"), npdt)
                outs = ["variables", "volumes", "gradient", "criteria"] + (["sub_variables", "sub_volumes", "sub_criteria", "sub_zorder"] if rank else [])
                for pre in ("", "sub_") if rank else ("",):       # the partition kernels copy: their output is the stored transfer
                    for R in PART_RANKS:
                        assert np.array_equal(out(f"{pre}part{R}_variables"), out(pre + "variables")), (cname, tag, pre, R)
                        assert np.array_equal(out(f"{pre}part{R}_volumes"), out(pre + "volumes")), (cname, tag, pre, R)
                for k, v in ins.items():
                    res[f"{cname}|{tag}|in|{k}"] = v
                for k in outs:
                    res[f"{cname}|{tag}|out|{k}"] = out(k)
    res["meta"] = np.array([
        "reference AMR kernel bodies (t8gpu/mesh/mesh_manager.inl:164-193, 625-643; t8gpu/mesh/subgrid_mesh_manager.inl:245-425, "
        "1007-1049, 1216-1280; examples/subgrid/kernels.inl:1109-1168; examples/compressible_euler/kernels.cu:471-501, "
        "solver.cu:231-241) executed on the host through the reference's own accessor classes; CUDA built-ins, the accessor-owning "
        "friend classes and the example solver structs are stand-ins; a launch is a loop over blocks and threads, atomicAdd a "
        "sequential read-modify-write (estimate_gradient adds in face order). The executed partition kernels reproduced "
        "variables / volumes (sub_variables / sub_volumes) bit for bit with 2 and 3 ranks and are not stored again. "
        "Parity stays 'unpinned' (DESIGN.md section 2). Forests: SynthMesh.adapt; states seeded per case name."])
    # two files, each below the size limit of a committed file: the Subgrid arrays of the rank-3 cases travel apart
    rank3 = {k for k in res if k != "meta" and cases[k.split("|")[0]][2] == 3 and k.split("|")[3].startswith("sub_")}
    bad = [k for k, v in res.items() if k != "meta" and v.dtype.kind == "f" and not np.isfinite(v).all()]
    for name, keys in (("reference_amr_vectors.npz", [k for k in res if k not in rank3]),
                       ("reference_amr_vectors_rank3.npz", ["meta"] + sorted(rank3))):
        path = os.path.join(HERE, name)
        write_npz(path, {k: res[k] for k in keys})
        assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
        print(f"wrote {path}: {len(keys) - 1} arrays ({os.path.getsize(path) / 1024:.0f} KiB)")
    print(f"non-finite: {bad}")
    for cname, (mesh, marks, rank, new_mesh, ad, census) in cases.items():
        print(f"  {cname}: {mesh.num_elements} -> {new_mesh.num_elements} elements, steps of adapt_data {census}, Subgrid rank {rank}, "
              f"adapt_data starts {ad[:6]}")


if __name__ == "__main__":
    main()
