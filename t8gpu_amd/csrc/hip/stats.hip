// stats.hip -- time-averaged flow statistics on the device: weighted running sums of fifteen per-cell quantities of the
// state (first moments, the raw second moments behind the rms values and the Reynolds stresses, the Mach number) and the
// pass that turns the sums into means, rms values, stresses and turbulent kinetic energy. The reference has nothing of
// the kind: its runs write instantaneous conserved variables only (MeshManager::save_variables_to_vtk,
// t8gpu/mesh/mesh_manager.inl:588-623).
//
// Not a stage kernel: passes between steps, self-contained like fields.hip and kernels_monitor.hip, so no kernel header
// changes with them. Slot tables and definitions: t8gpu_hip.h, DESIGN.md §14. All arithmetic in double for both float
// types, gamma = 1.4 as in flux_math.hpp.
//
// Accumulate is a streaming read-modify-write: per cell 5 state values in, 15 doubles in, 15 doubles out, no reuse, no
// atomics (one lane owns a cell's fifteen sums), nothing filtered. WIDE: two cells per lane and trip -- 16-byte accesses of
// the accumulator rows (240 of the 260 / 280 bytes a cell moves) and of fp64 state planes, 8-byte ones of fp32 state planes;
// the scalar form takes any alignment. Four fp32 cells per lane (16-byte state loads) put the accumulator accesses of
// neighbouring lanes 32 bytes apart and measured 1.73 times the time of this form on the c3 mesh. The grid
// is capped and strides over the rest. Two calls on the same data give the same bits.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "t8gpu_hip.h"

// The rms values and stresses are differences of two nearly equal terms: every product and sum in this file is rounded on
// its own, as the formulas of t8gpu_hip.h are written, so the results do not depend on what the compiler chooses to fuse.
#pragma clang fp contract(off)

namespace t8gpu_hip {

constexpr int kStatsPlanes = T8GPU_STATS_PLANES;
constexpr int kStatsBlocks = 2048;                   // grid cap: 8 workgroups of 256 per CU

template <class T>
using stats_vars_t = std::conditional_t<std::is_same<T, float>::value, T8gpuVars_f32, T8gpuVars_f64>;
typedef float  stats_f32x2 __attribute__((ext_vector_type(2)));
typedef double stats_f64x2 __attribute__((ext_vector_type(2)));
template <class T>
using stats_pair_t = std::conditional_t<std::is_same<T, float>::value, stats_f32x2, stats_f64x2>;   // two cells of a state plane

// the fifteen quantities of one cell (all indices compile-time constants: the array stays in registers)
__device__ __forceinline__ void stats_cell(double (&q)[kStatsPlanes], double rho, double mx, double my, double mz, double E) {
  const double m2 = mx * mx + my * my + mz * mz;
  const double p  = 0.4 * (E - 0.5 * m2 / rho);
  q[0]  = rho;
  q[1]  = mx;
  q[2]  = my;
  q[3]  = mz;
  q[4]  = E;
  q[5]  = p;
  q[6]  = rho * rho;
  q[7]  = p * p;
  q[8]  = mx * mx / rho;
  q[9]  = my * my / rho;
  q[10] = mz * mz / rho;
  q[11] = mx * my / rho;
  q[12] = mx * mz / rho;
  q[13] = my * mz / rho;
  q[14] = (sqrt(m2) / rho) / sqrt(1.4 * p / rho);
}

template <class T, bool WIDE>
__global__ __launch_bounds__(256) void k_stats_accumulate(size_t n, stats_vars_t<T> st, double weight, double* __restrict__ sums,
                                                          size_t stride) {
  constexpr int V = 2;
  using W         = stats_pair_t<T>;
  const T* __restrict__ p0 = st.p[0];
  const T* __restrict__ p1 = st.p[1];
  const T* __restrict__ p2 = st.p[2];
  const T* __restrict__ p3 = st.p[3];
  const T* __restrict__ p4 = st.p[4];
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, gstride = (size_t)gridDim.x * 256;

  auto scalar_cell = [&](size_t i) {
    double q[kStatsPlanes], a[kStatsPlanes];
#pragma unroll
    for (int k = 0; k < kStatsPlanes; k++) a[k] = sums[(size_t)k * stride + i];
    stats_cell(q, (double)p0[i], (double)p1[i], (double)p2[i], (double)p3[i], (double)p4[i]);
#pragma unroll
    for (int k = 0; k < kStatsPlanes; k++) sums[(size_t)k * stride + i] = a[k] + weight * q[k];
  };

  // cells i and i + 1 (i even, the rows 16-byte aligned): fifteen 16-byte loads, fifteen 16-byte stores
  auto cell_pair = [&](size_t i, double r0, double x0, double y0, double z0, double e0, double r1, double x1, double y1, double z1,
                       double e1) {
    stats_f64x2 a[kStatsPlanes];
#pragma unroll
    for (int k = 0; k < kStatsPlanes; k++) a[k] = *reinterpret_cast<const stats_f64x2*>(sums + (size_t)k * stride + i);
    double qa[kStatsPlanes], qb[kStatsPlanes];
    stats_cell(qa, r0, x0, y0, z0, e0);
    stats_cell(qb, r1, x1, y1, z1, e1);
#pragma unroll
    for (int k = 0; k < kStatsPlanes; k++) {
      stats_f64x2 v;
      v[0] = a[k][0] + weight * qa[k];
      v[1] = a[k][1] + weight * qb[k];
      *reinterpret_cast<stats_f64x2*>(sums + (size_t)k * stride + i) = v;
    }
  };

  if constexpr (!WIDE) {
    for (size_t i = gid; i < n; i += gstride) scalar_cell(i);
  } else {
    const size_t nvec = n / V;
    for (size_t v = gid; v < nvec; v += gstride) {
      const size_t i  = v * V;
      const W      u0 = *reinterpret_cast<const W*>(p0 + i);
      const W      u1 = *reinterpret_cast<const W*>(p1 + i);
      const W      u2 = *reinterpret_cast<const W*>(p2 + i);
      const W      u3 = *reinterpret_cast<const W*>(p3 + i);
      const W      u4 = *reinterpret_cast<const W*>(p4 + i);
      cell_pair(i, (double)u0[0], (double)u1[0], (double)u2[0], (double)u3[0], (double)u4[0], (double)u0[1], (double)u1[1],
                (double)u2[1], (double)u3[1], (double)u4[1]);
    }
    if (gid < n - nvec * V) scalar_cell(nvec * V + gid);   // the cell behind the last whole pair
  }
}

// one lane per cell; the branches on the output pointers are uniform over the launch
__global__ __launch_bounds__(256) void k_stats_results(size_t n, const double* __restrict__ sums, size_t stride, double W,
                                                       T8gpuStatsPlanes out) {
  const size_t gstride = (size_t)gridDim.x * 256;
  const bool   stress  = out.p[12] || out.p[13] || out.p[14] || out.p[15] || out.p[16] || out.p[17] || out.p[18];
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gstride) {
    auto A = [&](int k) { return sums[(size_t)k * stride + i]; };
    const double a0 = A(0);
    if (out.p[0]) out.p[0][i] = a0 / W;
    if (out.p[4]) out.p[4][i] = A(4) / W;
    if (out.p[6]) out.p[6][i] = A(14) / W;
    if (out.p[1] || out.p[2] || out.p[3] || out.p[7] || out.p[8] || out.p[9] || stress) {
      const double m[3] = {A(1), A(2), A(3)};
#pragma unroll
      for (int c = 0; c < 3; c++) {
        if (out.p[1 + c]) out.p[1 + c][i] = m[c] / W;
        if (out.p[7 + c]) out.p[7 + c][i] = m[c] / a0;
      }
      if (stress) {
        const double d = a0 * W;
        const double rxx = A(8) / W - m[0] * m[0] / d, ryy = A(9) / W - m[1] * m[1] / d, rzz = A(10) / W - m[2] * m[2] / d;
        if (out.p[12]) out.p[12][i] = rxx;
        if (out.p[13]) out.p[13][i] = ryy;
        if (out.p[14]) out.p[14][i] = rzz;
        if (out.p[15]) out.p[15][i] = A(11) / W - m[0] * m[1] / d;
        if (out.p[16]) out.p[16][i] = A(12) / W - m[0] * m[2] / d;
        if (out.p[17]) out.p[17][i] = A(13) / W - m[1] * m[2] / d;
        if (out.p[18]) out.p[18][i] = 0.5 * (rxx + ryy + rzz) / (a0 / W);
      }
    }
    if (out.p[5] || out.p[11]) {
      const double mp = A(5) / W;
      if (out.p[5]) out.p[5][i] = mp;
      if (out.p[11]) out.p[11][i] = sqrt(fmax(0.0, A(7) / W - mp * mp));
    }
    if (out.p[10]) {
      const double mr = a0 / W;
      out.p[10][i]    = sqrt(fmax(0.0, A(6) / W - mr * mr));
    }
  }
}

inline int stats_grid(size_t work) {
  const size_t b = (work + 255) / 256;
  return static_cast<int>(b < 1 ? 1 : (b > (size_t)kStatsBlocks ? (size_t)kStatsBlocks : b));
}

template <class T>
int stats_accumulate(size_t n, stats_vars_t<T> st, double weight, double* sums, size_t stride, void* stream) {
  if (n == 0) return 0;
  if (!sums || stride < n) return static_cast<int>(hipErrorInvalidValue);
  for (int k = 0; k < 5; k++)
    if (!st.p[k]) return static_cast<int>(hipErrorInvalidValue);
  constexpr size_t V = 2;
  auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  bool wide = n >= V && aligned(sums) && stride % 2 == 0;      // every accumulator row starts on 16 bytes
  for (int k = 0; k < 5; k++) wide = wide && aligned(st.p[k]); // (fp32 planes would do with 8: one rule for both types)
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (wide)
    hipLaunchKernelGGL((k_stats_accumulate<T, true>), dim3(stats_grid(n / V)), dim3(256), 0, s, n, st, weight, sums, stride);
  else
    hipLaunchKernelGGL((k_stats_accumulate<T, false>), dim3(stats_grid(n)), dim3(256), 0, s, n, st, weight, sums, stride);
  return static_cast<int>(hipGetLastError());
}

}  // namespace t8gpu_hip

extern "C" {
int t8gpu_hip_stats_accumulate_f32(size_t num_cells, T8gpuVars_f32 state, double weight, double* sums, size_t plane_stride,
                                   void* stream) {
  return t8gpu_hip::stats_accumulate<float>(num_cells, state, weight, sums, plane_stride, stream);
}
int t8gpu_hip_stats_accumulate_f64(size_t num_cells, T8gpuVars_f64 state, double weight, double* sums, size_t plane_stride,
                                   void* stream) {
  return t8gpu_hip::stats_accumulate<double>(num_cells, state, weight, sums, plane_stride, stream);
}
int t8gpu_hip_stats_results(size_t num_cells, const double* sums, size_t plane_stride, double total_weight, T8gpuStatsPlanes out,
                            void* stream) {
  if (num_cells == 0) return 0;
  if (!sums || plane_stride < num_cells || !(total_weight > 0.0) || !__builtin_isfinite(total_weight))
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(t8gpu_hip::k_stats_results, dim3(t8gpu_hip::stats_grid(num_cells)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), num_cells, sums, plane_stride, total_weight, out);
  return static_cast<int>(hipGetLastError());
}
}
