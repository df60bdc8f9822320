// kernels_compat.hip -- reference-dataflow kernels (face -> atomic scatter, separate RK pass).
//
// Same data flow as the reference's CUDA kernels (one lane per face / sub-face, float atomics into
// the flux planes, a streaming RK pass that also zeroes the flux planes) written directly for gfx950:
// 64-lane waves, flat local slots instead of the [rank][index] pointer-table double indirection,
// several small faces/blocks packed per wavefront. These are the kernels the accessor-level C++ API
// (include/t8gpu/) launches, and the baseline the fused tile kernels are measured against.
#include <hip/hip_runtime.h>

// Keep the reference's rounding sequence in this tier: no mul+add contraction.
#pragma clang fp contract(off)

#include "compat_faces.hpp"
#include "flux_math.hpp"
#include "fused_common.hpp"
#include "stage_kernel_note.hpp"
#include "t8gpu_hip.h"
#include "t8gpu_host.h"

namespace t8gpu_hip {

template <class T>
struct Vars {
  T* p[5];
};

template <class T>
T8_DEV void load5(const Vars<T>& v, size_t i, T s[5]) {
#pragma unroll
  for (int k = 0; k < 5; k++) s[k] = v.p[k][i];
}

// float/double atomic add to global memory; hipcc lowers this to global_atomic_add_f32 /
// global_atomic_add_f64 on gfx950 (no CAS loop; checked in the .s).
template <class T>
T8_DEV void gadd(T* addr, T v) {
  unsafeAtomicAdd(addr, v);
}

// ---- a4: interior faces, kernels.cu:135-309 ----------------------------------------------------
template <class T, int KIND>
__global__ __launch_bounds__(256) void k_flux_faces(int F, int ndim, const int32_t* __restrict__ fn,
                                                    const int32_t* __restrict__ idx, const T* __restrict__ normals,
                                                    const T* __restrict__ areas, Vars<T> st, Vars<T> fl,
                                                    T* __restrict__ speed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F) return;
  const T area = areas[i];
  int     l = fn[2 * (size_t)i], r = fn[2 * (size_t)i + 1];
  if (idx) {
    l = idx[l];
    r = idx[r];
  }
  T n[3] = {T(0), T(0), T(0)};
  for (int k = 0; k < ndim; k++) n[k] = normals[(size_t)ndim * i + k];
  T sl[5], sr[5];
  load5(st, l, sl);
  load5(st, r, sr);
  T t1[3], t2[3], Ff[5], g[5], spd;
  face_basis<T>(n, t1, t2);
  face_frame_flux_ref<T, KIND>(n, t1, t2, sl, sr, false, Ff, spd);
  if (speed) speed[i] = spd;
#pragma unroll
  for (int k = 0; k < 5; k++) Ff[k] = area * Ff[k];
  from_face_frame<T>(n, t1, t2, Ff, g);
#pragma unroll
  for (int k = 0; k < 5; k++) {
    gadd(&fl.p[k][l], -g[k]);
    gadd(&fl.p[k][r], g[k]);
  }
}

// ---- a5: boundary faces, kernels.cu:311-469 (reflective walls) ------------------------------------
// MODE (compat_faces.hpp: BoundaryMode) = kBndWalls: the reference's kernel, every face a wall, no kinds list or table read;
// kBndFar: the faces' kinds 0..15 (open boundaries and far field; not in the reference), the same flux against the outside
// state of the kind (boundary_face_flux).
template <class T, int KIND, int MODE>
__global__ __launch_bounds__(256) void k_flux_boundary(int F, int B, int ndim, const int32_t* __restrict__ fn,
                                                       const uint8_t* __restrict__ kinds, const T* __restrict__ inflow,
                                                       const T* __restrict__ normals, const T* __restrict__ areas,
                                                       Vars<T> st, Vars<T> fl, T* __restrict__ speed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const T   area = areas[F + i];
  const int e    = fn[2 * (size_t)F + i];
  const int kind = MODE == kBndWalls ? 0 : kinds[i];
  T         n[3] = {T(0), T(0), T(0)};
  for (int k = 0; k < ndim; k++) n[k] = normals[(size_t)ndim * (F + i) + k];
  T s[5];
  load5(st, e, s);
  T t1[3], t2[3], Ff[5], g[5], spd;
  boundary_face_flux<T, KIND, MODE == kBndFar>(n, s, kind, inflow, t1, t2, Ff, spd);
  if (speed) speed[F + i] = spd;
#pragma unroll
  for (int k = 0; k < 5; k++) Ff[k] = area * Ff[k];
  from_face_frame<T>(n, t1, t2, Ff, g);
#pragma unroll
  for (int k = 0; k < 5; k++) gadd(&fl.p[k][e], -g[k]);
}

// ---- a6: SSP-RK3 stages, ssp_runge_kutta.inl:30-99 (S = 1) and :101-221 (S = Subgrid::size) -------
// One lane per cell; `volume[i / S] / S` for subgrids. Grid-stride, coalesced, fluxes zeroed.
template <class T, int STAGE, int S>
__global__ __launch_bounds__(256) void k_rk_stage(size_t ncells, Vars<T> prev, Vars<T> mid, Vars<T> out, Vars<T> fl,
                                                  const T* __restrict__ volume, T dt) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ncells; i += (size_t)gridDim.x * blockDim.x) {
    const T vol = (S == 1) ? volume[i] : volume[i / S] / static_cast<T>(S);
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const T f = fl.p[k][i];
      T       o;
      if (STAGE == 1) {
        o = prev.p[k][i] + dt / vol * f;
      } else if (STAGE == 2) {
        o = rk3c<T>::c21 * prev.p[k][i] + rk3c<T>::c22 * mid.p[k][i] + rk3c<T>::c23 * dt / vol * f;
      } else {
        o = rk3c<T>::c31 * prev.p[k][i] + rk3c<T>::c32 * mid.p[k][i] + rk3c<T>::c33 * dt / vol * f;
      }
      out.p[k][i] = o;
      fl.p[k][i]  = T(0.0);
    }
  }
}

// ---- a13: inner fluxes of a block, kernels.inl:335-662 -------------------------------------------
// One 64-lane wavefront per workgroup: a whole Subgrid<4,4,4> block, or four Subgrid<4,4> blocks.
// The wave runs in lock-step, so the reference's latent LDS race cannot occur.
template <class T, int KIND, int RANK>
__global__ __launch_bounds__(64) void k_subgrid_inner(int N, Vars<T> st, Vars<T> fl, const T* __restrict__ volumes) {
  constexpr int S   = RANK == 3 ? 64 : 16;
  constexpr int EPB = 64 / S;  // elements per workgroup
  const int     c   = threadIdx.x % S;
  const int     sub = threadIdx.x / S;
  const int     e   = blockIdx.x * EPB + sub;
  __shared__ T  sh[5][64];
  const bool    live = e < N;
  const size_t  o    = (size_t)(live ? e : 0) * S;
  T             own[5];
  load5(st, o + c, own);
  const T vol     = volumes[live ? e : 0];
  const T edge    = (RANK == 3 ? t8_cbrt(vol) : t8_sqrt(vol)) / static_cast<T>(4);
  const T surface = RANK == 3 ? edge * edge : edge;
  T       acc[5];
#pragma unroll
  for (int k = 0; k < 5; k++) acc[k] = fl.p[k][o + c];
#pragma unroll
  for (int d = 0; d < RANK; d++) {
    const int str = d == 0 ? 1 : (d == 1 ? 4 : 16);
    const int cd  = (c / str) % 4;
    T         n[3] = {T(0.0), T(0.0), T(0.0)};
    n[d]           = T(1.0);
    T t1[3], t2[3];
    face_basis<T>(n, t1, t2);
    T g[5] = {T(0.0), T(0.0), T(0.0), T(0.0), T(0.0)};
    if (cd < 3) {
      T nb[5], Ff[5], spd;
      load5(st, o + c + str, nb);
      face_frame_flux_ref<T, KIND>(n, t1, t2, own, nb, false, Ff, spd);
      from_face_frame<T>(n, t1, t2, Ff, g);
#pragma unroll
      for (int k = 0; k < 5; k++) g[k] = g[k] * surface;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 5; k++) sh[k][threadIdx.x] = g[k];
    __syncthreads();
    if (cd < 3) {
#pragma unroll
      for (int k = 0; k < 5; k++) acc[k] -= g[k];
    }
    if (cd > 0) {
#pragma unroll
      for (int k = 0; k < 5; k++) acc[k] += sh[k][threadIdx.x - str];
    }
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < 5; k++) fl.p[k][o + c] = acc[k];
  }
}

// ---- a14: outer faces of blocks, kernels.inl:664-911 ---------------------------------------------
// SF = sub-faces per coarse face (16 or 4); 64/SF coarse faces share one wavefront.
template <class T, int KIND, int RANK>
__global__ __launch_bounds__(64) void k_subgrid_faces(int F, const int32_t* __restrict__ fn, const int32_t* __restrict__ idx,
                                                      const int32_t* __restrict__ level_diff,
                                                      const int32_t* __restrict__ nb_off,
                                                      const T* __restrict__ normals, const T* __restrict__ areas,
                                                      Vars<T> st, Vars<T> fl) {
  constexpr int S  = RANK == 3 ? 64 : 16;
  constexpr int SF = RANK == 3 ? 16 : 4;
  const int     f  = blockIdx.x * (64 / SF) + threadIdx.x / SF;
  if (f >= F) return;
  const int t = threadIdx.x % SF;
  const int i = t % 4, j = t / 4;
  int       l = fn[2 * (size_t)f], r = fn[2 * (size_t)f + 1], off[3] = {0, 0, 0};
  if (idx) {
    l = idx[l];
    r = idx[r];
  }
  const int ds = (level_diff[f] == 0) ? 2 : 1;
  for (int d = 0; d < RANK; d++) off[d] = nb_off[(size_t)RANK * f + d];
  T n[3] = {T(0), T(0), T(0.0)};
  for (int d = 0; d < RANK; d++) n[d] = normals[(size_t)RANK * f + d];
  T t1[3], t2[3];
  face_basis<T>(n, t1, t2);
  int lflat, rflat;
  sg_face_cells<T, RANK>(n, off, ds, i, j, lflat, rflat);
  const size_t li = (size_t)l * S + lflat;
  const size_t ri = (size_t)r * S + rflat;
  T            sl[5], sr[5], Ff[5], g[5], spd;
  load5(st, li, sl);
  load5(st, ri, sr);
  face_frame_flux_ref<T, KIND>(n, t1, t2, sl, sr, false, Ff, spd);
  from_face_frame<T>(n, t1, t2, Ff, g);
  const T surface = areas[f] / static_cast<T>(SF);
#pragma unroll
  for (int k = 0; k < 5; k++) {
    gadd(&fl.p[k][li], -g[k] * surface);
    gadd(&fl.p[k][ri], g[k] * surface);
  }
}

// ---- a15: boundary faces of blocks, kernels.inl:913-1107 (reflective walls) ------------------------
// The boundary slices start after the F interior entries. MODE (compat_faces.hpp: BoundaryMode) = kBndWalls: the reference's
// kernel; kBndOpen: the faces' kinds 0..9 (not in the reference), for plans without far-field faces -- no far-field code;
// kBndFar: kinds 0..15, the outside state of every sub-face from its inside subcell and the block face's outward normal.
template <class T, int KIND, int RANK, int MODE>
__global__ __launch_bounds__(64) void k_subgrid_boundary(int F, int B, const int32_t* __restrict__ fn,
                                                         const uint8_t* __restrict__ kinds, const T* __restrict__ inflow,
                                                         const T* __restrict__ normals, const T* __restrict__ areas,
                                                         Vars<T> st, Vars<T> fl) {
  constexpr int S  = RANK == 3 ? 64 : 16;
  constexpr int SF = RANK == 3 ? 16 : 4;
  const int     f  = blockIdx.x * (64 / SF) + threadIdx.x / SF;
  if (f >= B) return;
  const int    t    = threadIdx.x % SF;
  const int    i    = t % 4, j = t / 4;
  const size_t slot = (size_t)F + f;
  const int    l    = fn[2 * (size_t)F + f];
  const int    kind = MODE == kBndWalls ? 0 : kinds[f];
  T n[3] = {T(0), T(0), T(0.0)};
  for (int d = 0; d < RANK; d++) n[d] = normals[(size_t)RANK * slot + d];
  int          si[3], sj[3];
  const size_t li = (size_t)l * S + sg_inside_cell<T, RANK>(n, i, j, si, sj);
  T            sl[5], t1[3], t2[3], Ff[5], g[5], spd;
  load5(st, li, sl);
  boundary_face_flux<T, KIND, MODE == kBndFar>(n, sl, kind, inflow, t1, t2, Ff, spd);
  from_face_frame<T>(n, t1, t2, Ff, g);
  const T surface = areas[slot] / static_cast<T>(SF);
#pragma unroll
  for (int k = 0; k < 5; k++) gadd(&fl.p[k][li], -g[k] * surface);
}

// ---- launchers ------------------------------------------------------------------------------------
template <class T, class V>
Vars<T> mk(const V& v) {
  Vars<T> o;
  for (int k = 0; k < 5; k++) o.p[k] = v.p[k];
  return o;
}

// Every launcher: 0 for an empty launch, hipErrorInvalidValue for a dimension or flux kind it has no kernel for, else the
// launch's status. dispatch_kind (fused_common.hpp) turns the flux kind (and the rank, as a flag) into template arguments.
inline bool bad_kind(int kind) { return kind < 0 || kind > 2; }

template <class T, class V>
int flux_faces(int kind, int F, int ndim, const int32_t* fn, const int32_t* idx, const T* normals, const T* areas,
               V st, V fl, T* speed, void* stream) {
  if (F <= 0) return 0;
  if (ndim < 2 || ndim > 3 || bad_kind(kind)) return static_cast<int>(hipErrorInvalidValue);
  const dim3 grid((F + 255) / 256), block(256);
  return dispatch_kind(
      [&](auto K) {
        return launch(&k_flux_faces<T, K>, grid, block, 0, static_cast<hipStream_t>(stream), F, ndim, fn, idx, normals, areas,
                      mk<T>(st), mk<T>(fl), speed);
      },
      kind);
}

// MODE = kBndWalls: kinds and inflow are not read
template <class T, int MODE, class V>
int flux_boundary(int kind, int F, int B, int ndim, const int32_t* fn, const uint8_t* kinds, const T* inflow, const T* normals,
                  const T* areas, V st, V fl, T* speed, void* stream) {
  if (B <= 0) return 0;
  if (ndim < 2 || ndim > 3 || bad_kind(kind)) return static_cast<int>(hipErrorInvalidValue);
  const dim3 grid((B + 255) / 256), block(256);
  return dispatch_kind(
      [&](auto K) {
        return launch(&k_flux_boundary<T, K, MODE>, grid, block, 0, static_cast<hipStream_t>(stream), F, B, ndim, fn, kinds,
                      inflow, normals, areas, mk<T>(st), mk<T>(fl), speed);
      },
      kind);
}

// STAGE = stage: dispatch_kind's three values 0..2 are stage - 1
template <class T, int S, class V>
int rk_stage(int stage, size_t ncells, V prev, V mid, V out, V fl, const T* volume, T dt, void* stream) {
  if (ncells == 0) return 0;
  if (stage < 1 || stage > 3) return static_cast<int>(hipErrorInvalidValue);
  size_t blocks = (ncells + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  const dim3 grid(static_cast<unsigned>(blocks)), block(256);
  return dispatch_kind(
      [&](auto S0) {
        return launch(&k_rk_stage<T, S0 + 1, S>, grid, block, 0, static_cast<hipStream_t>(stream), ncells, mk<T>(prev),
                      stage == 1 ? mk<T>(prev) : mk<T>(mid), mk<T>(out), mk<T>(fl), volume, dt);
      },
      stage - 1);
}

template <class T, class V>
int subgrid_inner(int kind, int rank, int N, V st, V fl, const T* volumes, void* stream) {
  if (N <= 0) return 0;
  if ((rank != 2 && rank != 3) || bad_kind(kind)) return static_cast<int>(hipErrorInvalidValue);
  const dim3 block(64), grid(rank == 3 ? N : (N + 3) / 4);
  return dispatch_kind(
      [&](auto K, auto RANK3) {
        return launch(&k_subgrid_inner<T, K, RANK3 ? 3 : 2>, grid, block, 0, static_cast<hipStream_t>(stream), N, mk<T>(st),
                      mk<T>(fl), volumes);
      },
      kind, rank == 3);
}

template <class T, class V>
int subgrid_faces(int kind, int rank, int F, const int32_t* fn, const int32_t* idx, const int32_t* ld, const int32_t* off,
                  const T* normals, const T* areas, V st, V fl, void* stream) {
  if (F <= 0) return 0;
  if ((rank != 2 && rank != 3) || bad_kind(kind)) return static_cast<int>(hipErrorInvalidValue);
  const int  fpb = rank == 3 ? 4 : 16;
  const dim3 block(64), grid((F + fpb - 1) / fpb);
  return dispatch_kind(
      [&](auto K, auto RANK3) {
        return launch(&k_subgrid_faces<T, K, RANK3 ? 3 : 2>, grid, block, 0, static_cast<hipStream_t>(stream), F, fn, idx, ld,
                      off, normals, areas, mk<T>(st), mk<T>(fl));
      },
      kind, rank == 3);
}

// MODE = kBndWalls: kinds and inflow are not read
template <class T, int MODE, class V>
int subgrid_boundary(int kind, int rank, int F, int B, const int32_t* fn, const uint8_t* kinds, const T* inflow, const T* normals,
                     const T* areas, V st, V fl, void* stream) {
  if (B <= 0) return 0;
  if ((rank != 2 && rank != 3) || bad_kind(kind)) return static_cast<int>(hipErrorInvalidValue);
  const int  fpb = rank == 3 ? 4 : 16;
  const dim3 block(64), grid((B + fpb - 1) / fpb);
  return dispatch_kind(
      [&](auto K, auto RANK3) {
        return launch(&k_subgrid_boundary<T, K, RANK3 ? 3 : 2, MODE>, grid, block, 0, static_cast<hipStream_t>(stream), F, B, fn,
                      kinds, inflow, normals, areas, mk<T>(st), mk<T>(fl));
      },
      kind, rank == 3);
}

}  // namespace t8gpu_hip

namespace t8gpu_hip {
StageKernelNote& stage_kernel_note() {
  // per host thread: the step driver's two lanes enqueue from two threads (stepper.hip); the caller's thread -- the one that asks
  // t8gpu_hip_last_stage_kernel -- launches the interior tiles, the bulk of a stage
  static thread_local StageKernelNote note = {{0}, -1, 0, 0, {}};
  return note;
}
}  // namespace t8gpu_hip

using namespace t8gpu_hip;

extern "C" {

const char* t8gpu_hip_last_stage_kernel(void) { return stage_kernel_note().name; }
int t8gpu_hip_last_stage_workgroups(void) { return stage_kernel_note().weight < 0 ? 0 : stage_kernel_note().workgroups; }
const char* t8gpu_hip_last_stage_launch(int index, int* workgroups) {
  const StageKernelNote& n = stage_kernel_note();
  if (index < 0 || index >= n.n_launches || index >= kStageLaunchesNoted) return nullptr;
  if (workgroups) *workgroups = n.launches[index].workgroups;
  return n.launches[index].name;
}
int t8gpu_hip_set_resident_limit(int workgroups) { return resident_limit().exchange(workgroups > 0 ? workgroups : 0); }
int t8gpu_hip_abi_version(void) { return 16; }   // 2: T8gpuPlainPlan.tile_desc; 3: T8gpuSubgridPlan row format (far-cell recipes), n_blocks_addressed, family records; 4: T8gpuPlainPlan.n_patch_tiles; 5: T8gpuPlainPlan.ell holds rows for generic tiles only (tile_desc word 6), patch_dim; 6: T8gpuPlainPlan.n_irregular_tiles; 7: T8gpuPlainPlan ghost window (ghost_buf, send_map, send_list, send_buf, n_owned); 8: t8gpu_hip_plain_geo_frames_* (plan builders must call it); 9: T8gpuPlainPlan open boundaries (inflow, has_open_faces), t8gpu_hip_flux_boundary_bc_*, t8gpu_hip_plain_inflow_table_*; 10: T8gpuSubgridPlan open boundaries (inflow, has_open_faces), t8gpu_hip_subgrid_boundary_bc_*; 11: far-field boundary kinds (T8gpuPlainPlan.has_farfield_faces, face_lr codes 0xFFF8 + k, t8gpu_hip_flux_boundary_bc_* kinds 10..15); 12: far-field kinds on Subgrid blocks (T8gpuSubgridPlan.has_farfield_faces, code bits 23-26 hold 10 + k, t8gpu_hip_subgrid_boundary_far_*); 13: planar 2D stage (t8gpu_hip_plain_fused_stage_planar_*, t8gpu_hip_stepper_set_planar / _planar, t8gpu_hip_planes_or_bits_*); 14: t8gpu_hip_plain_patch_lds_bytes; 15: iterate_steps writes the speed estimates in its last step only (t8gpu_hip_stepper_set_speed_every_step / _speed_stages); 16: t8gpu_hip_set_resident_limit, t8gpu_hip_last_stage_workgroups, t8gpu_hip_last_stage_launch
int t8gpu_hip_device_count(int* count) { return static_cast<int>(hipGetDeviceCount(count)); }
int t8gpu_hip_set_device(int device) { return static_cast<int>(hipSetDevice(device)); }
const char* t8gpu_hip_error_string(int code) {
  if (code >= 10000) return "RCCL error (code - 10000 is the ncclResult_t)";
  return hipGetErrorString(static_cast<hipError_t>(code));
}

// (a _bc / _far call without a kinds list is the walls-only launch)
#define T8_DEFINE_COMPAT(SUF, T, V)                                                                                  \
  int t8gpu_hip_flux_faces_##SUF(int kind, int F, int ndim, const int32_t* fn, const int32_t* idx, const T* normals, \
                                 const T* areas, V st, V fl, T* speed, void* stream) {                               \
    return flux_faces<T, V>(kind, F, ndim, fn, idx, normals, areas, st, fl, speed, stream);                          \
  }                                                                                                                  \
  int t8gpu_hip_flux_boundary_##SUF(int kind, int F, int B, int ndim, const int32_t* fn, const T* normals,           \
                                    const T* areas, V st, V fl, T* speed, void* stream) {                            \
    return flux_boundary<T, kBndWalls, V>(kind, F, B, ndim, fn, nullptr, nullptr, normals, areas, st, fl, speed,     \
                                          stream);                                                                   \
  }                                                                                                                  \
  int t8gpu_hip_flux_boundary_bc_##SUF(int kind, int F, int B, int ndim, const int32_t* fn, const uint8_t* kinds,    \
                                       const T* inflow, const T* normals, const T* areas, V st, V fl, T* speed,      \
                                       void* stream) {                                                               \
    return kinds ? flux_boundary<T, kBndFar, V>(kind, F, B, ndim, fn, kinds, inflow, normals, areas, st, fl, speed,  \
                                                stream)                                                              \
                 : t8gpu_hip_flux_boundary_##SUF(kind, F, B, ndim, fn, normals, areas, st, fl, speed, stream);       \
  }                                                                                                                  \
  int t8gpu_hip_rk3_stage_##SUF(int stage, int N, V prev, V mid, V out, V fl, const T* volume, T dt, void* stream) { \
    return rk_stage<T, 1, V>(stage, N < 0 ? 0 : (size_t)N, prev, mid, out, fl, volume, dt, stream);                  \
  }                                                                                                                  \
  int t8gpu_hip_subgrid_inner_##SUF(int kind, int rank, int N, V st, V fl, const T* volumes, void* stream) {         \
    return subgrid_inner<T, V>(kind, rank, N, st, fl, volumes, stream);                                              \
  }                                                                                                                  \
  int t8gpu_hip_subgrid_outer_##SUF(int kind, int rank, int F, const int32_t* fn, const int32_t* idx,                \
                                    const int32_t* ld, const int32_t* off, const T* normals, const T* areas, V st,   \
                                    V fl, void* stream) {                                                            \
    return subgrid_faces<T, V>(kind, rank, F, fn, idx, ld, off, normals, areas, st, fl, stream);                     \
  }                                                                                                                  \
  int t8gpu_hip_subgrid_boundary_##SUF(int kind, int rank, int F, int B, const int32_t* fn, const T* normals,        \
                                       const T* areas, V st, V fl, void* stream) {                                   \
    return subgrid_boundary<T, kBndWalls, V>(kind, rank, F, B, fn, nullptr, nullptr, normals, areas, st, fl, stream); \
  }                                                                                                                  \
  int t8gpu_hip_subgrid_boundary_bc_##SUF(int kind, int rank, int F, int B, const int32_t* fn, const uint8_t* kinds, \
                                          const T* inflow, const T* normals, const T* areas, V st, V fl,             \
                                          void* stream) {                                                            \
    return kinds ? subgrid_boundary<T, kBndOpen, V>(kind, rank, F, B, fn, kinds, inflow, normals, areas, st, fl, stream) \
                 : t8gpu_hip_subgrid_boundary_##SUF(kind, rank, F, B, fn, normals, areas, st, fl, stream);           \
  }                                                                                                                  \
  int t8gpu_hip_subgrid_boundary_far_##SUF(int kind, int rank, int F, int B, const int32_t* fn, const uint8_t* kinds, \
                                           const T* inflow, const T* normals, const T* areas, V st, V fl,            \
                                           void* stream) {                                                           \
    return kinds ? subgrid_boundary<T, kBndFar, V>(kind, rank, F, B, fn, kinds, inflow, normals, areas, st, fl, stream) \
                 : t8gpu_hip_subgrid_boundary_##SUF(kind, rank, F, B, fn, normals, areas, st, fl, stream);           \
  }                                                                                                                  \
  int t8gpu_hip_subgrid_rk3_stage_##SUF(int stage, int rank, int N, V prev, V mid, V out, V fl, const T* volumes,    \
                                        T dt, void* stream) {                                                        \
    if (rank == 3) return rk_stage<T, 64, V>(stage, (size_t)(N < 0 ? 0 : N) * 64, prev, mid, out, fl, volumes, dt, stream); \
    if (rank == 2) return rk_stage<T, 16, V>(stage, (size_t)(N < 0 ? 0 : N) * 16, prev, mid, out, fl, volumes, dt, stream); \
    return static_cast<int>(hipErrorInvalidValue);                                                                   \
  }

T8_DEFINE_COMPAT(f32, float, T8gpuVars_f32)
T8_DEFINE_COMPAT(f64, double, T8gpuVars_f64)

}  // extern "C"
