// kernels_monitor.hip -- one streaming pass over the state between steps that answers what a run loop asks of it:
// how large the next step may be (max (|v| + c) / h), whether mass, momentum and energy are conserved (the five
// integrals), which way the entropy moves, and whether the state is still physical (min rho, min p, counts of
// non-finite and of non-physical cells). The reference has none of this on the device: compute_integral copies to the
// host (examples/compressible_euler/solver.cu:190-211, examples/subgrid/solver.inl:281-305) and the Subgrid
// compute_timestep is not implemented (solver.inl:309-325).
//
// Scheme of kernels_reduce.hip: grid-stride partials per workgroup -> one final kernel, no atomics, a fixed tree, so
// two calls on the same data give the same bits. Per-cell arithmetic and all accumulation in double whatever
// float_type is; gamma = 1.4 as in flux_math.hpp. Every state value is read once. Slot table: t8gpu_hip.h, DESIGN.md.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "t8gpu_hip.h"

namespace t8gpu_hip {

constexpr int kMonitorBlocks = 1024;                 // grid cap: 4 workgroups of 256 per CU
constexpr int kMonitorSlots  = T8GPU_MONITOR_SLOTS;
constexpr int kMonitorLive   = 13;                   // slots 13-15 are reserved (0)

// slot classes: 0-6 and 11-12 sums, 7-8 maxima (identity 0: speeds are >= 0), 9-10 minima (identity +inf)
enum { kSum = 0, kMax = 1, kMin = 2 };
__host__ __device__ constexpr int slot_class(int k) { return (k == 7 || k == 8) ? kMax : (k == 9 || k == 10) ? kMin : kSum; }
__device__ __forceinline__ double slot_identity(int cls) { return cls == kMin ? __builtin_huge_val() : 0.0; }
__device__ __forceinline__ double slot_combine(int cls, double a, double b) {
  return cls == kSum ? a + b : cls == kMax ? (b > a ? b : a) : (b < a ? b : a);
}

template <class T>
using vars_t = std::conditional_t<std::is_same<T, float>::value, T8gpuVars_f32, T8gpuVars_f64>;
typedef float  f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
template <class T>
using wide_t = std::conditional_t<std::is_same<T, float>::value, f32x4, f64x2>;   // 16 bytes per lane

// 1 / h, h = vol^(1/DIM): the edge of a Cartesian cell; on curved cells the cbrt(volume) length of the reference's
// refinement criterion (examples/compressible_euler/solver.cu:240), not an inradius
template <int DIM>
__device__ __forceinline__ double inv_length(double vol) {
  return DIM == 2 ? rsqrt(vol) : rcbrt(vol);
}

// one cell into the 13 accumulators (all indices compile-time constants: the array stays in registers)
__device__ __forceinline__ void monitor_cell(double (&a)[kMonitorLive], double rho, double mx, double my, double mz, double E,
                                             double vol, double inv_h) {
  const bool   fin  = __builtin_isfinite(rho) && __builtin_isfinite(mx) && __builtin_isfinite(my) && __builtin_isfinite(mz) &&
                    __builtin_isfinite(E);
  const bool   pos  = fin && rho > 0.0;
  const double m2   = mx * mx + my * my + mz * mz;
  const double ke   = 0.5 * m2 / rho;
  const double p    = 0.4 * (E - ke);
  const bool   phys = pos && p > 0.0;
  a[0] += fin ? vol * rho : 0.0;
  a[1] += fin ? vol * mx : 0.0;
  a[2] += fin ? vol * my : 0.0;
  a[3] += fin ? vol * mz : 0.0;
  a[4] += fin ? vol * E : 0.0;
  a[5] += pos ? vol * ke : 0.0;
  const double ent = vol * rho * (log(p) - 1.4 * log(rho));
  a[6] += phys ? ent : 0.0;
  const double s = sqrt(m2) / rho + sqrt(1.4 * p / rho);
  const double r = s * inv_h;
  a[7]  = (phys && s > a[7]) ? s : a[7];
  a[8]  = (phys && r > a[8]) ? r : a[8];
  a[9]  = (fin && rho < a[9]) ? rho : a[9];
  a[10] = (pos && p < a[10]) ? p : a[10];
  a[11] += fin ? 0.0 : 1.0;
  a[12] += (fin && !phys) ? 1.0 : 0.0;
}

// wavefront shuffles, then the four wavefronts through LDS; thread k < 13 leaves with slot k of the workgroup
__device__ __forceinline__ double monitor_block_reduce(double (&a)[kMonitorLive]) {
  __shared__ double part[kMonitorLive][4];
#pragma unroll
  for (int k = 0; k < kMonitorLive; k++) {
    double v = a[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = slot_combine(slot_class(k), v, __shfl_down(v, off, 64));
    if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x < kMonitorLive) {
    const int k = threadIdx.x, cls = slot_class(k);
    r = slot_combine(cls, slot_combine(cls, part[k][0], part[k][1]), slot_combine(cls, part[k][2], part[k][3]));
  }
  return r;
}

// MODE 0: one cell per lane and trip, any alignment, any cells_per_element (shift >= 0: a power of two);
// MODE 1: 16-byte loads of the five planes and of the volumes, cells_per_element = 1;
// MODE 2: 16-byte loads of the planes, cells_per_element = 2^shift a multiple of the vector: one volume per vector.
// partial[slot * kMonitorBlocks + workgroup]
template <class T, int DIM, int MODE>
__global__ __launch_bounds__(256) void k_monitor_partial(size_t n, int cpe, int shift, vars_t<T> st, const T* __restrict__ volume,
                                                         double* __restrict__ partial) {
  constexpr int V = 16 / sizeof(T);
  using W         = wide_t<T>;
  const T* __restrict__ p0 = st.p[0];
  const T* __restrict__ p1 = st.p[1];
  const T* __restrict__ p2 = st.p[2];
  const T* __restrict__ p3 = st.p[3];
  const T* __restrict__ p4 = st.p[4];
  double a[kMonitorLive];
#pragma unroll
  for (int k = 0; k < kMonitorLive; k++) a[k] = slot_identity(slot_class(k));
  const double inv_cpe = 1.0 / cpe;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, gstride = (size_t)gridDim.x * 256;

  auto scalar_cell = [&](size_t i) {
    const size_t e   = shift >= 0 ? (i >> shift) : i / (size_t)cpe;
    const double vol = (double)volume[e] * inv_cpe;
    monitor_cell(a, (double)p0[i], (double)p1[i], (double)p2[i], (double)p3[i], (double)p4[i], vol, inv_length<DIM>(vol));
  };

  if constexpr (MODE == 0) {
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
      if constexpr (MODE == 1) {
        const W vv = *reinterpret_cast<const W*>(volume + i);
#pragma unroll
        for (int j = 0; j < V; j++) {
          const double vol = (double)vv[j];
          monitor_cell(a, (double)u0[j], (double)u1[j], (double)u2[j], (double)u3[j], (double)u4[j], vol, inv_length<DIM>(vol));
        }
      } else {
        const double vol = (double)volume[i >> shift] * inv_cpe, inv_h = inv_length<DIM>(vol);
#pragma unroll
        for (int j = 0; j < V; j++) monitor_cell(a, (double)u0[j], (double)u1[j], (double)u2[j], (double)u3[j], (double)u4[j], vol, inv_h);
      }
    }
    if (gid < n - nvec * V) scalar_cell(nvec * V + gid);   // the cells behind the last whole vector (fewer than V)
  }
  const double r = monitor_block_reduce(a);
  if (threadIdx.x < kMonitorLive) partial[(size_t)threadIdx.x * kMonitorBlocks + blockIdx.x] = r;
}

// one workgroup per slot
__global__ __launch_bounds__(256) void k_monitor_final(int nparts, const double* __restrict__ partial, double* __restrict__ result) {
  __shared__ double part[4];
  const int k = blockIdx.x;
  if (k >= kMonitorLive) {
    if (threadIdx.x == 0) result[k] = 0.0;
    return;
  }
  const int cls = slot_class(k);
  double    v   = slot_identity(cls);
  for (int i = threadIdx.x; i < nparts; i += 256) v = slot_combine(cls, v, partial[(size_t)k * kMonitorBlocks + i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = slot_combine(cls, v, __shfl_down(v, off, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) result[k] = slot_combine(cls, slot_combine(cls, part[0], part[1]), slot_combine(cls, part[2], part[3]));
}

template <class T, int DIM>
int state_monitor_dim(size_t n, int cpe, vars_t<T> st, const T* volume, void* workspace, double* result, hipStream_t s) {
  constexpr size_t V = 16 / sizeof(T);
  int shift = -1;
  if ((cpe & (cpe - 1)) == 0)
    for (shift = 0; (1 << shift) < cpe; shift++) {}
  auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  bool wide = n >= V;
  for (int k = 0; k < 5; k++) wide = wide && aligned(st.p[k]);
  const int mode = !wide ? 0 : (cpe == 1 && aligned(volume)) ? 1 : (shift >= 0 && (size_t)cpe % V == 0) ? 2 : 0;
  const size_t work = mode == 0 ? n : n / V;           // lanes' worth of trips
  const size_t b    = (work + 255) / 256;
  const int    nb   = static_cast<int>(b < 1 ? 1 : (b > (size_t)kMonitorBlocks ? (size_t)kMonitorBlocks : b));
  double*      ws   = static_cast<double*>(workspace);
  if (mode == 0)
    hipLaunchKernelGGL((k_monitor_partial<T, DIM, 0>), dim3(nb), dim3(256), 0, s, n, cpe, shift, st, volume, ws);
  else if (mode == 1)
    hipLaunchKernelGGL((k_monitor_partial<T, DIM, 1>), dim3(nb), dim3(256), 0, s, n, cpe, shift, st, volume, ws);
  else
    hipLaunchKernelGGL((k_monitor_partial<T, DIM, 2>), dim3(nb), dim3(256), 0, s, n, cpe, shift, st, volume, ws);
  hipLaunchKernelGGL(k_monitor_final, dim3(kMonitorSlots), dim3(256), 0, s, nb, static_cast<const double*>(ws), result);
  return static_cast<int>(hipGetLastError());
}

template <class T>
int state_monitor(size_t n, int cpe, int dim, vars_t<T> st, const T* volume, void* workspace, double* result, void* stream) {
  if (!workspace || !result || cpe < 1 || (dim != 2 && dim != 3)) return static_cast<int>(hipErrorInvalidValue);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dim == 2 ? state_monitor_dim<T, 2>(n, cpe, st, volume, workspace, result, s)
                  : state_monitor_dim<T, 3>(n, cpe, st, volume, workspace, result, s);
}

}  // namespace t8gpu_hip

extern "C" {
size_t t8gpu_hip_state_monitor_workspace_bytes(void) {
  return sizeof(double) * t8gpu_hip::kMonitorSlots * t8gpu_hip::kMonitorBlocks;
}
int t8gpu_hip_state_monitor_f32(size_t num_cells, int cells_per_element, int dim, T8gpuVars_f32 state, const float* volume,
                                void* workspace, double* result, void* stream) {
  return t8gpu_hip::state_monitor<float>(num_cells, cells_per_element, dim, state, volume, workspace, result, stream);
}
int t8gpu_hip_state_monitor_f64(size_t num_cells, int cells_per_element, int dim, T8gpuVars_f64 state, const double* volume,
                                void* workspace, double* result, void* stream) {
  return t8gpu_hip::state_monitor<double>(num_cells, cells_per_element, dim, state, volume, workspace, result, stream);
}
}
