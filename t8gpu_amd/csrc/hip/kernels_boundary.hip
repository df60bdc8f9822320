// kernels_boundary.hip -- what crosses the boundary: the boundary faces' numerical fluxes and wall pressure forces of one
// state, summed per face group (a side, a boundary kind, any labelling of the caller) instead of scattered into cells.
// monitor() says how the five integrals change; on a domain with open sides they are meant to change, and these sums
// are the other half of the budget: change of the integral + dt * boundary flux = 0, stage by stage. The reference has
// nothing of the kind.
//
// Per face the arithmetic is the compat tier's by construction: the routines its boundary kernels call (compat_faces.hpp:
// boundary_face_flux, sg_inside_cell) in the state's float type with contraction off. Products with the area
// and every sum are double. Scheme of kernels_monitor.hip: the faces arrive sorted by group (face_order, group_offsets);
// pass one reduces a contiguous chunk of ONE group's faces per workgroup (wavefront shuffles, then LDS), pass two folds a
// group's chunk partials in a fixed tree. No atomics: the same data gives the same bits. Slot table: t8gpu_hip.h, DESIGN §13.
#include <hip/hip_runtime.h>

// the compat tier's rounding sequence: no mul+add contraction
#pragma clang fp contract(off)

#include <type_traits>

#include "compat_faces.hpp"
#include "flux_math.hpp"
#include "fused_common.hpp"
#include "t8gpu_hip.h"
#include "t8gpu_host.h"

namespace t8gpu_hip {
namespace {

constexpr int kBndSlots = T8GPU_BOUNDARY_SLOTS;
constexpr int kBndLive  = 13;                        // slots 13-15 are reserved (0)
constexpr int kBndMax   = T8GPU_BOUNDARY_GROUPS_MAX;
constexpr int kBndLanes = 256;                       // lanes of a pass-one workgroup: one face (Subgrid: sub-face) each

template <class T>
using bvars_t = std::conditional_t<std::is_same<T, float>::value, T8gpuVars_f32, T8gpuVars_f64>;

// first face of every group in face_order (and B behind the last), by value in the kernel arguments
struct GroupOffsets {
  int32_t off[kBndMax + 1];
};

// chunk c of the launch -> (group, first position in face_order, end of the group); chunks of a group are consecutive
__device__ __forceinline__ bool chunk_of(const GroupOffsets& go, int num_groups, int per_chunk, int c, int& lo, int& hi) {
  for (int g = 0; g < num_groups; g++) {
    const int n = go.off[g + 1] - go.off[g], nc = (n + per_chunk - 1) / per_chunk;
    if (c < nc) {
      lo = go.off[g] + c * per_chunk;
      hi = go.off[g + 1];
      return true;
    }
    c -= nc;
  }
  return false;
}

// one face / sub-face into the 13 accumulators: area A, flux g (float type, per unit area, outward), inside state s, normal n
template <class T>
__device__ __forceinline__ void boundary_face(double (&a)[kBndLive], double A, const T g[5], const T s[5], const T n[3]) {
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 5; k++) fin = fin && __builtin_isfinite(g[k]);
  const double rho = (double)s[0], mx = (double)s[1], my = (double)s[2], mz = (double)s[3];
  const double p    = 0.4 * ((double)s[4] - 0.5 * (mx * mx + my * my + mz * mz) / rho);
  const bool   finp = fin && __builtin_isfinite(p);
  a[0] += A;
#pragma unroll
  for (int k = 0; k < 5; k++) a[1 + k] += fin ? A * (double)g[k] : 0.0;
#pragma unroll
  for (int d = 0; d < 3; d++) a[6 + d] += finp ? A * p * (double)n[d] : 0.0;
  a[9] += finp ? A * p : 0.0;
  a[10] += (fin && g[0] > T(0)) ? A * (double)g[0] : 0.0;
  a[11] += 1.0;
  a[12] += fin ? 0.0 : 1.0;
}

// wavefront shuffles, then the four wavefronts through LDS; thread k < 13 leaves with slot k of the workgroup
__device__ __forceinline__ double boundary_block_reduce(double (&a)[kBndLive]) {
  __shared__ double part[kBndLive][4];
#pragma unroll
  for (int k = 0; k < kBndLive; k++) {
    double v = a[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x < kBndLive) {
    const int k = threadIdx.x;
    r = (part[k][0] + part[k][1]) + (part[k][2] + part[k][3]);
  }
  return r;
}

// ---- pass one, plain elements: one lane per boundary face ------------------------------------------------------------
template <class T, int KIND>
__global__ __launch_bounds__(kBndLanes) void k_boundary_partial(int F, int ndim, GroupOffsets go, int num_groups,
                                                                const int32_t* __restrict__ order, const int32_t* __restrict__ fn,
                                                                const uint8_t* __restrict__ kinds, const T* __restrict__ inflow,
                                                                const T* __restrict__ normals, const T* __restrict__ areas,
                                                                bvars_t<T> st, double* __restrict__ partial) {
  double a[kBndLive];
#pragma unroll
  for (int k = 0; k < kBndLive; k++) a[k] = 0.0;
  int lo = 0, hi = 0;
  chunk_of(go, num_groups, kBndLanes, blockIdx.x, lo, hi);      // (the launch has exactly the chunks of the groups)
  const int j = lo + threadIdx.x;
  if (j < hi) {
    const int    i    = order[j];
    const size_t slot = (size_t)F + i;
    const int    e    = fn[2 * (size_t)F + i];
    const int    kind = kinds ? kinds[i] : 0;
    T            n[3] = {T(0), T(0), T(0)};
    for (int k = 0; k < ndim; k++) n[k] = normals[(size_t)ndim * slot + k];
    T s[5];
#pragma unroll
    for (int k = 0; k < 5; k++) s[k] = st.p[k][e];
    T t1[3], t2[3], Ff[5], g[5], spd;
    boundary_face_flux<T, KIND, true>(n, s, kind, inflow, t1, t2, Ff, spd);
    from_face_frame<T>(n, t1, t2, Ff, g);
    boundary_face<T>(a, (double)areas[slot], g, s, n);
  }
  const double r = boundary_block_reduce(a);
  if (threadIdx.x < kBndLive) partial[(size_t)blockIdx.x * kBndSlots + threadIdx.x] = r;
}

// ---- pass one, Subgrid blocks: one lane per sub-face, 256 / SF block faces per workgroup ------------------------------
template <class T, int KIND, int RANK>
__global__ __launch_bounds__(kBndLanes) void k_subgrid_boundary_partial(int F, GroupOffsets go, int num_groups,
                                                                        const int32_t* __restrict__ order,
                                                                        const int32_t* __restrict__ fn,
                                                                        const uint8_t* __restrict__ kinds, const T* __restrict__ inflow,
                                                                        const T* __restrict__ normals, const T* __restrict__ areas,
                                                                        bvars_t<T> st, double* __restrict__ partial) {
  constexpr int S  = RANK == 3 ? 64 : 16;
  constexpr int SF = RANK == 3 ? 16 : 4;
  double a[kBndLive];
#pragma unroll
  for (int k = 0; k < kBndLive; k++) a[k] = 0.0;
  int lo = 0, hi = 0;
  chunk_of(go, num_groups, kBndLanes / SF, blockIdx.x, lo, hi);
  const int jf = lo + threadIdx.x / SF;
  if (jf < hi) {
    const int    f    = order[jf];
    const int    t    = threadIdx.x % SF;
    const int    i    = t % 4, j = t / 4;
    const size_t slot = (size_t)F + f;
    const int    l    = fn[2 * (size_t)F + f];
    const int    kind = kinds ? kinds[f] : 0;
    T n[3] = {T(0), T(0), T(0.0)};
    for (int d = 0; d < RANK; d++) n[d] = normals[(size_t)RANK * slot + d];
    int          si[3], sj[3];
    const size_t li = (size_t)l * S + sg_inside_cell<T, RANK>(n, i, j, si, sj);
    T            sl[5], t1[3], t2[3], Ff[5], g[5], spd;
#pragma unroll
    for (int k = 0; k < 5; k++) sl[k] = st.p[k][li];
    boundary_face_flux<T, KIND, true>(n, sl, kind, inflow, t1, t2, Ff, spd);
    from_face_frame<T>(n, t1, t2, Ff, g);
    boundary_face<T>(a, (double)areas[slot] / SF, g, sl, n);
  }
  const double r = boundary_block_reduce(a);
  if (threadIdx.x < kBndLive) partial[(size_t)blockIdx.x * kBndSlots + threadIdx.x] = r;
}

// ---- pass two: one workgroup per group. Thread t folds slot t % 16 of the chunks t / 16, t / 16 + 16, ... in index order,
// then thread k < 16 adds the sixteen strands in order. result = value, or result + weight * value (slots 0-10) ----------
__global__ __launch_bounds__(256) void k_boundary_final(GroupOffsets go, int per_chunk, const double* __restrict__ partial,
                                                        double* __restrict__ result, int accumulate, double weight) {
  __shared__ double strand[16][kBndSlots];
  const int g = blockIdx.x;
  int       first = 0;
  for (int h = 0; h < g; h++) first += (go.off[h + 1] - go.off[h] + per_chunk - 1) / per_chunk;
  const int nc = (go.off[g + 1] - go.off[g] + per_chunk - 1) / per_chunk;
  const int k = threadIdx.x & 15, w = threadIdx.x >> 4;
  double    v = 0.0;
  if (k < kBndLive)
    for (int c = w; c < nc; c += 16) v += partial[(size_t)(first + c) * kBndSlots + k];
  strand[w][k] = v;
  __syncthreads();
  if (threadIdx.x < kBndSlots) {
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < 16; q++) sum += strand[q][k];
    double* out = result + (size_t)g * kBndSlots + k;
    if (accumulate && k <= 10) sum = *out + weight * sum;
    *out = sum;
  }
}

// arguments shared by both launchers; nchunks = the chunks of all groups
int check_groups(int B, int num_groups, const int32_t* group_offsets, int per_chunk, GroupOffsets& go, int& nchunks) {
  if (B < 0 || num_groups < 1 || num_groups > kBndMax || !group_offsets || group_offsets[0] != 0 || group_offsets[num_groups] != B)
    return static_cast<int>(hipErrorInvalidValue);
  nchunks = 0;
  for (int g = 0; g <= kBndMax; g++) go.off[g] = group_offsets[g < num_groups ? g : num_groups];
  for (int g = 0; g < num_groups; g++) {
    if (go.off[g + 1] < go.off[g]) return static_cast<int>(hipErrorInvalidValue);
    nchunks += (go.off[g + 1] - go.off[g] + per_chunk - 1) / per_chunk;
  }
  return 0;
}

template <class T>
int boundary_fluxes(int kind, int F, int B, int ndim, const int32_t* fn, const uint8_t* kinds, const T* inflow, const T* normals,
                    const T* areas, bvars_t<T> st, int num_groups, const int32_t* order, const int32_t* group_offsets,
                    void* workspace, double* result, int accumulate, double weight, void* stream) {
  GroupOffsets go;
  int          nchunks = 0;
  if (check_groups(B, num_groups, group_offsets, kBndLanes, go, nchunks) != 0 || F < 0 || ndim < 2 || ndim > 3 || kind < 0 ||
      kind > 2 || !result || (B > 0 && (!workspace || !order || !fn || !normals || !areas)))
    return static_cast<int>(hipErrorInvalidValue);
  hipStream_t s  = static_cast<hipStream_t>(stream);
  double*     ws = static_cast<double*>(workspace);
  int         rc = 0;
  if (nchunks > 0)
    rc = dispatch_kind(
        [&](auto K) {
          return launch(&k_boundary_partial<T, K>, dim3(nchunks), dim3(kBndLanes), 0, s, F, ndim, go, num_groups, order, fn, kinds,
                        inflow, normals, areas, st, ws);
        },
        kind);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(k_boundary_final, dim3(num_groups), dim3(256), 0, s, go, kBndLanes, static_cast<const double*>(ws), result,
                     accumulate, weight);
  return static_cast<int>(hipGetLastError());
}

template <class T>
int subgrid_boundary_fluxes(int kind, int rank, int F, int B, const int32_t* fn, const uint8_t* kinds, const T* inflow,
                            const T* normals, const T* areas, bvars_t<T> st, int num_groups, const int32_t* order,
                            const int32_t* group_offsets, void* workspace, double* result, int accumulate, double weight,
                            void* stream) {
  if (rank != 2 && rank != 3) return static_cast<int>(hipErrorInvalidValue);
  const int    per_chunk = kBndLanes / (rank == 3 ? 16 : 4);
  GroupOffsets go;
  int          nchunks = 0;
  if (check_groups(B, num_groups, group_offsets, per_chunk, go, nchunks) != 0 || F < 0 || kind < 0 || kind > 2 || !result ||
      (B > 0 && (!workspace || !order || !fn || !normals || !areas)))
    return static_cast<int>(hipErrorInvalidValue);
  hipStream_t s  = static_cast<hipStream_t>(stream);
  double*     ws = static_cast<double*>(workspace);
  int         rc = 0;
  if (nchunks > 0)
    rc = dispatch_kind(
        [&](auto K, auto RANK3) {
          return launch(&k_subgrid_boundary_partial<T, K, RANK3 ? 3 : 2>, dim3(nchunks), dim3(kBndLanes), 0, s, F, go, num_groups,
                        order, fn, kinds, inflow, normals, areas, st, ws);
        },
        kind, rank == 3);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(k_boundary_final, dim3(num_groups), dim3(256), 0, s, go, per_chunk, static_cast<const double*>(ws), result,
                     accumulate, weight);
  return static_cast<int>(hipGetLastError());
}

}  // namespace
}  // namespace t8gpu_hip

using namespace t8gpu_hip;

extern "C" {
size_t t8gpu_hip_boundary_fluxes_workspace_bytes(int num_boundary_faces, int num_groups) {
  // one partial per chunk; the smallest chunk is the 16 block faces of a Subgrid<4,4,4> workgroup, and every group may end
  // with a chunk that is not full
  const size_t B = num_boundary_faces > 0 ? (size_t)num_boundary_faces : 0, G = num_groups > 0 ? (size_t)num_groups : 0;
  return sizeof(double) * kBndSlots * ((B + 15) / 16 + G + 1);
}
int t8gpu_hip_boundary_fluxes_f32(int flux_kind, int num_faces, int num_boundary_faces, int normal_dim, const int32_t* face_neighbors,
                                  const uint8_t* boundary_kinds, const float* inflow_table, const float* face_normals,
                                  const float* face_surfaces, T8gpuVars_f32 state, int num_groups, const int32_t* face_order,
                                  const int32_t* group_offsets, void* workspace, double* result, int accumulate, double weight,
                                  void* stream) {
  return boundary_fluxes<float>(flux_kind, num_faces, num_boundary_faces, normal_dim, face_neighbors, boundary_kinds, inflow_table,
                                face_normals, face_surfaces, state, num_groups, face_order, group_offsets, workspace, result,
                                accumulate, weight, stream);
}
int t8gpu_hip_boundary_fluxes_f64(int flux_kind, int num_faces, int num_boundary_faces, int normal_dim, const int32_t* face_neighbors,
                                  const uint8_t* boundary_kinds, const double* inflow_table, const double* face_normals,
                                  const double* face_surfaces, T8gpuVars_f64 state, int num_groups, const int32_t* face_order,
                                  const int32_t* group_offsets, void* workspace, double* result, int accumulate, double weight,
                                  void* stream) {
  return boundary_fluxes<double>(flux_kind, num_faces, num_boundary_faces, normal_dim, face_neighbors, boundary_kinds, inflow_table,
                                 face_normals, face_surfaces, state, num_groups, face_order, group_offsets, workspace, result,
                                 accumulate, weight, stream);
}
int t8gpu_hip_subgrid_boundary_fluxes_f32(int flux_kind, int rank, int num_faces, int num_boundary_faces,
                                          const int32_t* face_neighbors, const uint8_t* boundary_kinds, const float* inflow_table,
                                          const float* face_normals, const float* face_surfaces, T8gpuVars_f32 state, int num_groups,
                                          const int32_t* face_order, const int32_t* group_offsets, void* workspace, double* result,
                                          int accumulate, double weight, void* stream) {
  return subgrid_boundary_fluxes<float>(flux_kind, rank, num_faces, num_boundary_faces, face_neighbors, boundary_kinds, inflow_table,
                                        face_normals, face_surfaces, state, num_groups, face_order, group_offsets, workspace, result,
                                        accumulate, weight, stream);
}
int t8gpu_hip_subgrid_boundary_fluxes_f64(int flux_kind, int rank, int num_faces, int num_boundary_faces,
                                          const int32_t* face_neighbors, const uint8_t* boundary_kinds, const double* inflow_table,
                                          const double* face_normals, const double* face_surfaces, T8gpuVars_f64 state, int num_groups,
                                          const int32_t* face_order, const int32_t* group_offsets, void* workspace, double* result,
                                          int accumulate, double weight, void* stream) {
  return subgrid_boundary_fluxes<double>(flux_kind, rank, num_faces, num_boundary_faces, face_neighbors, boundary_kinds, inflow_table,
                                         face_normals, face_surfaces, state, num_groups, face_order, group_offsets, workspace, result,
                                         accumulate, weight, stream);
}
}
