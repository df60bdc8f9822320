// fields.hip -- derived output fields on the device: pressure, velocity, Mach number, entropy (pointwise) and vorticity,
// dilatation, schlieren (gradient fields) from the five planes of one step. The reference writes conserved variables
// only (MeshManager::save_variables_to_vtk, t8gpu/mesh/mesh_manager.inl:588-623); what a run shows of itself beyond them
// needs the face lists, the 2:1 sub-face map of Subgrid blocks and the ghost layer, which all sit on the device already.
//
// Not a stage kernel: an output pass between steps, self-contained like kernels_monitor.hip. Everything it needs is in
// this file, the sub-face -> cell map of the Subgrid outer faces included (restated from kernels_compat.hip:
// sg_face_cells, in both directions), so no kernel header changes with it.
//
// Slot table and definitions: t8gpu_hip.h, DESIGN.md §10. Arithmetic in double for both float types, gamma = 1.4.
// Gradient fields: (1 / 2 V_c) sum over the interior (sub-)faces s of cell c of A_s n_s (q_o - q_c) -- a GATHER, one sum
// per cell in a fixed order (CSR order = ascending face id; inside a hanging face j-major, i-minor), no atomics: two
// calls give the same bits. A uniform state gives q_o - q_c = 0 exactly, hence +-0 everywhere.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "t8gpu_hip.h"

namespace t8gpu_hip {

template <class T>
using field_vars_t = std::conditional_t<std::is_same<T, float>::value, T8gpuVars_f32, T8gpuVars_f64>;

// the sums of one cell: curl (cx, cy, cz) and divergence of u, gradient of rho -- each still times 2 V_c
struct FieldSums {
  double cx, cy, cz, div, gx, gy, gz;
};

// rho and u = m / rho of cell i
template <class T>
__device__ __forceinline__ void load_rho_u(const field_vars_t<T>& st, size_t i, double& rho, double& u, double& v, double& w) {
  rho = (double)st.p[0][i];
  u   = (double)st.p[1][i] / rho;
  v   = (double)st.p[2][i] / rho;
  w   = (double)st.p[3][i] / rho;
}

// one face term A n (q_o - q_c), n outward from c
__device__ __forceinline__ void field_term(FieldSums& g, double A, double nx, double ny, double nz, double drho, double du,
                                           double dv, double dw) {
  g.cx += A * (ny * dw - nz * dv);
  g.cy += A * (nz * du - nx * dw);
  g.cz += A * (nx * dv - ny * du);
  g.div += A * (nx * du + ny * dv + nz * dw);
  g.gx += A * nx * drho;
  g.gy += A * ny * drho;
  g.gz += A * nz * drho;
}

__device__ __forceinline__ bool any_pointwise(const T8gpuFieldPlanes& out) {
  return out.p[0] || out.p[1] || out.p[2] || out.p[3] || out.p[4] || out.p[5];
}

// planes 0-5 of cell i (a NULL plane: nothing computed, nothing stored; the branches are uniform over the launch)
__device__ __forceinline__ void store_pointwise(const T8gpuFieldPlanes& out, size_t i, double rho, double mx, double my, double mz,
                                                double E, double u, double v, double w) {
  if (out.p[1]) out.p[1][i] = u;
  if (out.p[2]) out.p[2][i] = v;
  if (out.p[3]) out.p[3][i] = w;
  if (out.p[0] || out.p[4] || out.p[5]) {
    const double p = 0.4 * (E - 0.5 * (mx * mx + my * my + mz * mz) / rho);
    if (out.p[0]) out.p[0][i] = p;
    if (out.p[4]) out.p[4][i] = sqrt(u * u + v * v + w * w) / sqrt(1.4 * p / rho);
    if (out.p[5]) out.p[5][i] = log(p) - 1.4 * log(rho);
  }
}

// planes 6-10 of cell i; s = 1 / (2 V_c)
__device__ __forceinline__ void store_gradient(const T8gpuFieldPlanes& out, size_t i, double s, const FieldSums& g) {
  if (out.p[6]) out.p[6][i] = s * g.cx;
  if (out.p[7]) out.p[7][i] = s * g.cy;
  if (out.p[8]) out.p[8][i] = s * g.cz;
  if (out.p[9]) out.p[9][i] = s * g.div;
  if (out.p[10]) {
    const double x = s * g.gx, y = s * g.gy, z = s * g.gz;
    out.p[10][i] = sqrt(x * x + y * y + z * z);
  }
}

// ---- plain elements: one lane per owned element, which walks its CSR row ---------------------------------------------
template <class T, bool GRAD>
__global__ __launch_bounds__(256) void k_plain_fields(int n, int ndim, field_vars_t<T> st, const T* __restrict__ volume,
                                                      const int32_t* __restrict__ fn, const T* __restrict__ normals,
                                                      const T* __restrict__ areas, const int32_t* __restrict__ csr_off,
                                                      const int32_t* __restrict__ csr_ent, T8gpuFieldPlanes out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  double rho, u, v, w;
  load_rho_u<T>(st, c, rho, u, v, w);
  if (any_pointwise(out))
    store_pointwise(out, c, rho, (double)st.p[1][c], (double)st.p[2][c], (double)st.p[3][c], (double)st.p[4][c], u, v, w);
  if constexpr (GRAD) {
    FieldSums g   = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int end = csr_off[c + 1];
    for (int k = csr_off[c]; k < end; k++) {
      const int    ent  = csr_ent[k];              // 2 f + side: side 0, c is l of face f and the stored normal is outward
      const size_t f    = (size_t)(ent >> 1);
      const int    o    = fn[ent ^ 1];             // the cell across: the other half of the face's pair (may be a ghost slot)
      const double sign = (ent & 1) ? -1.0 : 1.0;
      const double nx   = sign * (double)normals[ndim * f];
      const double ny   = sign * (double)normals[ndim * f + 1];
      const double nz   = ndim == 3 ? sign * (double)normals[ndim * f + 2] : 0.0;
      double       ro, uo, vo, wo;
      load_rho_u<T>(st, o, ro, uo, vo, wo);
      field_term(g, (double)areas[f], nx, ny, nz, ro - rho, uo - u, vo - v, wo - w);
    }
    store_gradient(out, c, 0.5 / (double)volume[c], g);
  }
}

// ---- Subgrid blocks: one wavefront per Subgrid<4,4,4> block, four Subgrid<4,4> blocks per wavefront -------------------
// Subcell c = i + 4 j + 16 k of block e sits in lane c (2D: lane 16 * (e % 4) + c). The block's rho, u, v, w are read once
// and passed through LDS for the in-block neighbours; the subcells on the block's surface then walk the block's CSR row
// and take, from every face, the sub-faces on their own side.
//
// The sub-face map (kernels_compat.hip: sg_face_cells), for face f with unit normal +-e_a outward from block l, tangential
// axes t1 < t2 (2D: t1 only), sub-face (i, j), level difference 0 (ds = 2) or hanging (ds = 1, l the finer block):
//   l-subcell: coordinate 3 (normal +) or 0 (normal -) along a, i along t1, j along t2
//   r-subcell: face_neighbor_offset + (0 along a, ds i / 2 along t1, ds j / 2 along t2)
// Forward (the block is l): the subcell on the l side of the face owns sub-face (i, j) = its tangential coordinates.
// Inverse (the block is r): the subcell whose coordinates are offset + (0, k1, k2) owns sub-face (k1, k2) of a same-level
// face and the 2^(rank-1) sub-faces (2 k1 + {0, 1}, 2 k2 + {0, 1}) of a hanging one.
template <class T, int RANK, bool GRAD>
__global__ __launch_bounds__(64) void k_subgrid_fields(int N, field_vars_t<T> st, const T* __restrict__ volumes,
                                                       const int32_t* __restrict__ fn, const int32_t* __restrict__ level_diff,
                                                       const int32_t* __restrict__ nb_off, const T* __restrict__ normals,
                                                       const T* __restrict__ areas, const int32_t* __restrict__ csr_off,
                                                       const int32_t* __restrict__ csr_ent, T8gpuFieldPlanes out) {
  constexpr int S   = RANK == 3 ? 64 : 16;
  constexpr int SF  = RANK == 3 ? 16 : 4;
  constexpr int EPB = 64 / S;                  // blocks per wavefront
  const int     lane = threadIdx.x;
  const int     c    = lane % S;
  const int     e    = blockIdx.x * EPB + lane / S;
  const bool    live = e < N;
  const size_t  cell = (size_t)(live ? e : 0) * S + c;
  double        rho, u, v, w;
  load_rho_u<T>(st, cell, rho, u, v, w);
  if (live && any_pointwise(out))
    store_pointwise(out, cell, rho, (double)st.p[1][cell], (double)st.p[2][cell], (double)st.p[3][cell], (double)st.p[4][cell], u, v,
                    w);
  if constexpr (GRAD) {
    __shared__ double sh[4][64];
    sh[0][lane] = rho;
    sh[1][lane] = u;
    sh[2][lane] = v;
    sh[3][lane] = w;
    __syncthreads();
    if (!live) return;                         // (behind the kernel's only barrier)
    const double vol = (double)volumes[e];
    const double h   = (RANK == 3 ? cbrt(vol) : sqrt(vol)) * 0.25;
    const double Ain = RANK == 3 ? h * h : h;
    FieldSums    g   = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // in-block faces: -x +x -y +y (-z +z)
#pragma unroll
    for (int d = 0; d < RANK; d++) {
      const int    str = 1 << (2 * d);
      const int    cd  = (c >> (2 * d)) & 3;
      const double ex = d == 0 ? 1.0 : 0.0, ey = d == 1 ? 1.0 : 0.0, ez = d == 2 ? 1.0 : 0.0;
      if (cd > 0) {
        const int j = lane - str;
        field_term(g, Ain, -ex, -ey, -ez, sh[0][j] - rho, sh[1][j] - u, sh[2][j] - v, sh[3][j] - w);
      }
      if (cd < 3) {
        const int j = lane + str;
        field_term(g, Ain, ex, ey, ez, sh[0][j] - rho, sh[1][j] - u, sh[2][j] - v, sh[3][j] - w);
      }
    }
    // outer faces: the block's CSR row, for the subcells on its surface
    const int  c0 = c & 3, c1 = (c >> 2) & 3, c2 = c >> 4;
    const bool surface = c0 == 0 || c0 == 3 || c1 == 0 || c1 == 3 || (RANK == 3 && (c2 == 0 || c2 == 3));
    if (surface) {
      const int end = csr_off[e + 1];
      for (int k = csr_off[e]; k < end; k++) {
        const int    ent  = csr_ent[k];            // 2 f + side: side 0, this block is l of face f
        const size_t f    = (size_t)(ent >> 1);
        const int    side = ent & 1;
        const double nx = (double)normals[RANK * f], ny = (double)normals[RANK * f + 1];
        const double nz = RANK == 3 ? (double)normals[RANK * f + 2] : 0.0;
        const int    a  = nx != 0.0 ? 0 : (ny != 0.0 ? 1 : 2);           // the face's axis (exact +-1 normals)
        const int    t1 = a == 0 ? 1 : 0, t2 = a == 2 ? 1 : 2;           // tangential axes (2D: t2 = 2, coordinate 0)
        const double na = a == 0 ? nx : (a == 1 ? ny : nz);
        const int    al = na > 0.0 ? 3 : 0;                              // the l-subcells' coordinate along a
        const bool   hanging = level_diff[f] != 0;
        const int    o0 = nb_off[RANK * f], o1 = nb_off[RANK * f + 1], o2 = RANK == 3 ? nb_off[RANK * f + 2] : 0;
        const int    oa  = a == 0 ? o0 : (a == 1 ? o1 : o2);
        const int    ot1 = t1 == 0 ? o0 : o1;
        const int    ot2 = t2 == 1 ? o1 : o2;
        const int    ca  = (c >> (2 * a)) & 3, ct1 = (c >> (2 * t1)) & 3, ct2 = (c >> (2 * t2)) & 3;
        int          nterm, b1, b2, fixed;       // terms; the first neighbour's tangential coordinates; its coordinate along a
        if (side == 0) {
          if (ca != al) continue;
          nterm = 1;
          fixed = oa;
          b1    = ot1 + (hanging ? ct1 / 2 : ct1);
          b2    = ot2 + (hanging ? ct2 / 2 : ct2);
        } else {
          if (ca != oa) continue;
          const int k1 = ct1 - ot1, k2 = ct2 - ot2, span = hanging ? 2 : 4;
          if (k1 < 0 || k1 >= span || k2 < 0 || k2 >= span) continue;
          nterm = hanging ? (RANK == 3 ? 4 : 2) : 1;
          fixed = al;
          b1    = hanging ? 2 * k1 : k1;
          b2    = hanging ? 2 * k2 : k2;
        }
        const size_t other = (size_t)fn[ent ^ 1] * S;                    // the block across (may be a ghost block)
        const double sign  = side ? -1.0 : 1.0;
        const double A     = (double)areas[f] / SF;
        for (int t = 0; t < nterm; t++) {        // a hanging face from its coarse side: j-major, i-minor
          const int    flat = (fixed << (2 * a)) + ((b1 + (t & 1)) << (2 * t1)) + ((b2 + (t >> 1)) << (2 * t2));
          double       ro, uo, vo, wo;
          load_rho_u<T>(st, other + flat, ro, uo, vo, wo);
          field_term(g, A, sign * nx, sign * ny, sign * nz, ro - rho, uo - u, vo - v, wo - w);
        }
      }
    }
    store_gradient(out, cell, 0.5 * S / vol, g);
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
inline bool any_gradient(const T8gpuFieldPlanes& out) {
  return out.p[6] || out.p[7] || out.p[8] || out.p[9] || out.p[10];
}

template <class T>
int plain_fields(int n, int ndim, field_vars_t<T> st, const T* volume, const int32_t* fn, const T* normals, const T* areas,
                 const int32_t* csr_off, const int32_t* csr_ent, T8gpuFieldPlanes out, void* stream) {
  if (n <= 0) return 0;
  if (ndim != 2 && ndim != 3) return static_cast<int>(hipErrorInvalidValue);
  const bool grad = any_gradient(out);
  if (grad && (!volume || !fn || !normals || !areas || !csr_off || !csr_ent)) return static_cast<int>(hipErrorInvalidValue);
  for (int k = 0; k < 5; k++)
    if (!st.p[k]) return static_cast<int>(hipErrorInvalidValue);
  const dim3  grid((n + 255) / 256), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (grad)
    hipLaunchKernelGGL((k_plain_fields<T, true>), grid, block, 0, s, n, ndim, st, volume, fn, normals, areas, csr_off, csr_ent, out);
  else
    hipLaunchKernelGGL((k_plain_fields<T, false>), grid, block, 0, s, n, ndim, st, volume, fn, normals, areas, csr_off, csr_ent, out);
  return static_cast<int>(hipGetLastError());
}

template <class T, int RANK>
int subgrid_fields_rank(int N, bool grad, field_vars_t<T> st, const T* volumes, const int32_t* fn, const int32_t* level_diff,
                        const int32_t* nb_off, const T* normals, const T* areas, const int32_t* csr_off, const int32_t* csr_ent,
                        T8gpuFieldPlanes out, hipStream_t s) {
  constexpr int EPB = RANK == 3 ? 1 : 4;
  const dim3    grid((N + EPB - 1) / EPB), block(64);
  if (grad)
    hipLaunchKernelGGL((k_subgrid_fields<T, RANK, true>), grid, block, 0, s, N, st, volumes, fn, level_diff, nb_off, normals, areas,
                       csr_off, csr_ent, out);
  else
    hipLaunchKernelGGL((k_subgrid_fields<T, RANK, false>), grid, block, 0, s, N, st, volumes, fn, level_diff, nb_off, normals, areas,
                       csr_off, csr_ent, out);
  return static_cast<int>(hipGetLastError());
}

template <class T>
int subgrid_fields(int rank, int N, field_vars_t<T> st, const T* volumes, const int32_t* fn, const int32_t* level_diff,
                   const int32_t* nb_off, const T* normals, const T* areas, const int32_t* csr_off, const int32_t* csr_ent,
                   T8gpuFieldPlanes out, void* stream) {
  if (N <= 0) return 0;
  if (rank != 2 && rank != 3) return static_cast<int>(hipErrorInvalidValue);
  const bool grad = any_gradient(out);
  if (grad && (!volumes || !fn || !level_diff || !nb_off || !normals || !areas || !csr_off || !csr_ent))
    return static_cast<int>(hipErrorInvalidValue);
  for (int k = 0; k < 5; k++)
    if (!st.p[k]) return static_cast<int>(hipErrorInvalidValue);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return rank == 3 ? subgrid_fields_rank<T, 3>(N, grad, st, volumes, fn, level_diff, nb_off, normals, areas, csr_off, csr_ent, out, s)
                   : subgrid_fields_rank<T, 2>(N, grad, st, volumes, fn, level_diff, nb_off, normals, areas, csr_off, csr_ent, out, s);
}

}  // namespace t8gpu_hip

extern "C" {
int t8gpu_hip_plain_fields_f32(int num_elements, int normal_dim, T8gpuVars_f32 state, const float* volume,
                               const int32_t* face_neighbors, const float* face_normals, const float* face_surfaces,
                               const int32_t* csr_offsets, const int32_t* csr_entries, T8gpuFieldPlanes out, void* stream) {
  return t8gpu_hip::plain_fields<float>(num_elements, normal_dim, state, volume, face_neighbors, face_normals, face_surfaces,
                                        csr_offsets, csr_entries, out, stream);
}
int t8gpu_hip_plain_fields_f64(int num_elements, int normal_dim, T8gpuVars_f64 state, const double* volume,
                               const int32_t* face_neighbors, const double* face_normals, const double* face_surfaces,
                               const int32_t* csr_offsets, const int32_t* csr_entries, T8gpuFieldPlanes out, void* stream) {
  return t8gpu_hip::plain_fields<double>(num_elements, normal_dim, state, volume, face_neighbors, face_normals, face_surfaces,
                                         csr_offsets, csr_entries, out, stream);
}
int t8gpu_hip_subgrid_fields_f32(int rank, int num_blocks, T8gpuVars_f32 state, const float* volumes,
                                 const int32_t* face_neighbors, const int32_t* face_level_difference,
                                 const int32_t* face_neighbor_offset, const float* face_normals, const float* face_surfaces,
                                 const int32_t* csr_offsets, const int32_t* csr_entries, T8gpuFieldPlanes out, void* stream) {
  return t8gpu_hip::subgrid_fields<float>(rank, num_blocks, state, volumes, face_neighbors, face_level_difference,
                                          face_neighbor_offset, face_normals, face_surfaces, csr_offsets, csr_entries, out, stream);
}
int t8gpu_hip_subgrid_fields_f64(int rank, int num_blocks, T8gpuVars_f64 state, const double* volumes,
                                 const int32_t* face_neighbors, const int32_t* face_level_difference,
                                 const int32_t* face_neighbor_offset, const double* face_normals, const double* face_surfaces,
                                 const int32_t* csr_offsets, const int32_t* csr_entries, T8gpuFieldPlanes out, void* stream) {
  return t8gpu_hip::subgrid_fields<double>(rank, num_blocks, state, volumes, face_neighbors, face_level_difference,
                                           face_neighbor_offset, face_normals, face_surfaces, csr_offsets, csr_entries, out, stream);
}
}
