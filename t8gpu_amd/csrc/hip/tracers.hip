// tracers.hip -- passive tracer particles on Cartesian forests, advected by Heun's method (DESIGN.md §15, t8gpu_hip.h:
// t8gpu_hip_tracers_*, t8gpu_amd/tracers.py, whose numpy functions are the definition). The reference has nothing of the kind.
//
// Not a stage kernel: two passes around a flow step, on the locate of forest/locate.hpp. A particle is a coordinate, not a
// member of a cell: the velocity at a point is that of the cell that holds it, m / rho in double, never interpolated.
//   predict  k1 = u^n(x),  xs = map(x + dt k1)                      (before the flow step)
//   correct  k2 = u^(n+1)(xs),  x = map(x + (dt / 2) (k1 + k2))     (after it)
// One lane per particle, 256-lane workgroups, no atomics, no LDS; every particle reads and writes its own entries only, so the
// result does not depend on the launch shape. All arithmetic in double, every operation rounded on its own.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "t8gpu_hip.h"

// x + dt k must come out as the numpy form: the product rounded, then the sum. No contraction into fused multiply-adds.
#pragma clang fp contract(off)

#include "forest/locate.hpp"

namespace t8gpu_hip {

template <class T>
using vars_t = std::conditional_t<std::is_same<T, float>::value, T8gpuVars_f32, T8gpuVars_f64>;

struct TracerForest {
  const uint64_t* keys;
  const int32_t*  levels;
  int             n, sub;
  int32_t         cells;        // owned cells: n, or n 4^dim
};

// ---- velocity at a point --------------------------------------------------------------------------------------------------
// u[a] = double(m_a[c]) / double(rho[c]) of the holding cell c and true, or +0 and false when no owned cell holds p. `hint`
// (may be NULL) is the particle's own in/out guess of the element.
template <class T, int DIM>
__device__ __forceinline__ bool point_velocity(const double* __restrict__ p, const TracerForest& f, const vars_t<T>& state,
                                               int32_t* __restrict__ hint, double* u) {
  int32_t       elem;
  const int32_t c = locate_cell_hinted<DIM>(p[0], p[1], DIM == 3 ? p[2] : 0.0, f.keys, f.levels, f.n, f.sub, hint ? *hint : -1, elem);
  if (hint) *hint = elem;
  const bool held = c >= 0 && c < f.cells;                  // (the index is an address from here on)
  const double rho = held ? (double)state.p[0][c] : 1.0;
  for (int a = 0; a < DIM; a++) u[a] = held ? (double)state.p[1 + a][c] / rho : 0.0;
  return held;
}

// ---- map: back into the domain, or out of it ---------------------------------------------------------------------------------
constexpr int    MAP_OK = 0, MAP_LEFT = 1, MAP_LOST = 2;
constexpr double BELOW_ONE = 0x1.fffffffffffffp-1;          // the largest double below 1

// raw[DIM] -> y[DIM]. Non-finite: lost. An open side crossed on any axis: left, y = raw. Periodic axis: y = p - floor(p), 0
// when that rounds to 1. Wall: mirrored once, exactly 1 becomes BELOW_ONE; still outside [0, 1): lost.
template <int DIM>
__device__ __forceinline__ int map_point(const double* raw, const T8gpuTracerSides& sides, double* y) {
  bool finite = true, left = false, lost = false;
  for (int a = 0; a < DIM; a++) {
    const double p = raw[a];
    finite = finite && __builtin_isfinite(p);
    const int lo = sides.kind[2 * a], hi = sides.kind[2 * a + 1];
    double    q = p;
    if (lo == T8GPU_TRACER_PERIODIC) {
      q = p - floor(p);
      if (q >= 1.0) q = 0.0;
    } else if (p < 0.0) {
      if (lo == T8GPU_TRACER_WALL) q = -p; else left = true;
    } else if (p >= 1.0) {
      if (hi == T8GPU_TRACER_WALL) q = 2.0 - p; else left = true;
    }
    if (q == 1.0) q = BELOW_ONE;
    lost = lost || !(q >= 0.0 && q < 1.0);
    y[a] = q;
  }
  if (!finite) return MAP_LOST;
  if (left) {
    for (int a = 0; a < DIM; a++) y[a] = raw[a];
    return MAP_LEFT;
  }
  return lost ? MAP_LOST : MAP_OK;
}

// ---- move: one phase of one particle, on a velocity that is already there -------------------------------------------------------
struct TracerArrays {
  double*  x;
  double*  xs;
  double*  k1;
  uint8_t* flag;
  uint8_t* status;
};

template <int DIM>
__device__ __forceinline__ void move_point(int phase, size_t i, double dt, const T8gpuTracerSides& sides, const double* k, bool held,
                                           const TracerArrays& t) {
  double x[DIM], raw[DIM], y[DIM];
  for (int a = 0; a < DIM; a++) x[a] = t.x[DIM * i + a];
  if (phase == T8GPU_TRACER_PREDICT) {
    for (int a = 0; a < DIM; a++) t.k1[DIM * i + a] = k[a];
    int out = MAP_LOST;
    if (held) {
      for (int a = 0; a < DIM; a++) {
        const double d = dt * k[a];
        raw[a] = x[a] + d;
      }
      out = map_point<DIM>(raw, sides, y);
    }
    if (out == MAP_LOST) {
      t.status[i] = T8GPU_TRACER_LOST;
      for (int a = 0; a < DIM; a++) y[a] = x[a];
    }
    for (int a = 0; a < DIM; a++) t.xs[DIM * i + a] = y[a];
    t.flag[i] = out == MAP_LEFT ? 1 : 0;
    return;
  }
  const bool   left = t.flag[i] != 0;
  const double h = 0.5 * dt;
  int          out = MAP_LOST;
  if (left || held) {
    for (int a = 0; a < DIM; a++) {
      const double k1 = t.k1[DIM * i + a];
      const double s = k1 + (left ? k1 : k[a]);
      const double d = h * s;
      raw[a] = x[a] + d;
    }
    out = map_point<DIM>(raw, sides, y);
  }
  if (out == MAP_LOST) {
    t.status[i] = T8GPU_TRACER_LOST;
    return;
  }
  if (out == MAP_LEFT) t.status[i] = T8GPU_TRACER_LEFT;
  for (int a = 0; a < DIM; a++) t.x[DIM * i + a] = y[a];
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
template <class T, int DIM>
__global__ __launch_bounds__(256) void k_tracers_velocity(size_t m, const double* __restrict__ points, TracerForest f, vars_t<T> state,
                                                          int32_t* __restrict__ hint, double* __restrict__ k,
                                                          int32_t* __restrict__ held) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  double p[DIM], u[DIM];
  for (int a = 0; a < DIM; a++) p[a] = points[DIM * i + a];
  const bool h = point_velocity<T, DIM>(p, f, state, hint ? hint + i : nullptr, u);
  for (int a = 0; a < DIM; a++) k[DIM * i + a] = u[a];
  held[i] = h ? 1 : 0;
}

template <int DIM>
__global__ __launch_bounds__(256) void k_tracers_move(int phase, size_t m, double dt, T8gpuTracerSides sides,
                                                      const double* __restrict__ k, const int32_t* __restrict__ held, TracerArrays t) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m || t.status[i] != T8GPU_TRACER_ACTIVE) return;
  double u[DIM];
  for (int a = 0; a < DIM; a++) u[a] = k[DIM * i + a];
  move_point<DIM>(phase, i, dt, sides, u, held[i] != 0, t);
}

template <class T, int DIM>
__global__ __launch_bounds__(256) void k_tracers_step(int phase, size_t m, double dt, T8gpuTracerSides sides, TracerForest f,
                                                      vars_t<T> state, int32_t* __restrict__ hint, TracerArrays t) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m || t.status[i] != T8GPU_TRACER_ACTIVE) return;
  const double* points = phase == T8GPU_TRACER_PREDICT ? t.x : t.xs;
  double        p[DIM], u[DIM];
  for (int a = 0; a < DIM; a++) p[a] = points[DIM * i + a];
  const bool h = point_velocity<T, DIM>(p, f, state, hint ? hint + i : nullptr, u);
  move_point<DIM>(phase, i, dt, sides, u, h, t);
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
constexpr size_t MAX_PARTICLES = (size_t)1 << 31;

template <class T>
bool bad_state(int dim, const vars_t<T>& state) {
  for (int a = 0; a <= dim; a++)
    if (!state.p[a]) return true;
  return false;
}

inline bool bad_move(int dim, int phase, double dt, const T8gpuTracerSides& sides) {
  if ((dim != 2 && dim != 3) || (phase != T8GPU_TRACER_PREDICT && phase != T8GPU_TRACER_CORRECT) || !(dt - dt == 0.0)) return true;
  for (int a = 0; a < dim; a++) {
    const int lo = sides.kind[2 * a], hi = sides.kind[2 * a + 1];
    if (lo < T8GPU_TRACER_PERIODIC || lo > T8GPU_TRACER_OPEN || hi < T8GPU_TRACER_PERIODIC || hi > T8GPU_TRACER_OPEN) return true;
    if ((lo == T8GPU_TRACER_PERIODIC) != (hi == T8GPU_TRACER_PERIODIC)) return true;
  }
  return false;
}

inline TracerForest forest_of(int dim, const uint64_t* keys, const int32_t* levels, int n, int sub) {
  return TracerForest{keys, levels, n, sub, (int32_t)(n * (sub == 1 ? 1 : (dim == 3 ? 64 : 16)))};
}

template <class T>
int tracers_velocity(int dim, size_t m, const double* points, const uint64_t* keys, const int32_t* levels, int n, int sub,
                     vars_t<T> state, int32_t* hint, double* k, int32_t* held, void* stream) {
  if (bad_forest(dim, n, keys, levels, sub) || m > MAX_PARTICLES) return static_cast<int>(hipErrorInvalidValue);
  if (m == 0) return 0;
  if (!points || !k || !held || (n > 0 && bad_state<T>(dim, state))) return static_cast<int>(hipErrorInvalidValue);
  const dim3         grid((unsigned)((m + 255) / 256)), block(256);
  hipStream_t        s = static_cast<hipStream_t>(stream);
  const TracerForest f = forest_of(dim, keys, levels, n, sub);
  if (dim == 3)
    hipLaunchKernelGGL((k_tracers_velocity<T, 3>), grid, block, 0, s, m, points, f, state, hint, k, held);
  else
    hipLaunchKernelGGL((k_tracers_velocity<T, 2>), grid, block, 0, s, m, points, f, state, hint, k, held);
  return static_cast<int>(hipGetLastError());
}

inline bool bad_arrays(const TracerArrays& t) { return !t.x || !t.xs || !t.k1 || !t.flag || !t.status; }

inline int tracers_move(int dim, int phase, size_t m, double dt, T8gpuTracerSides sides, const double* k, const int32_t* held,
                        TracerArrays t, void* stream) {
  if (bad_move(dim, phase, dt, sides) || m > MAX_PARTICLES) return static_cast<int>(hipErrorInvalidValue);
  if (m == 0) return 0;
  if (!k || !held || bad_arrays(t)) return static_cast<int>(hipErrorInvalidValue);
  const dim3  grid((unsigned)((m + 255) / 256)), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dim == 3)
    hipLaunchKernelGGL((k_tracers_move<3>), grid, block, 0, s, phase, m, dt, sides, k, held, t);
  else
    hipLaunchKernelGGL((k_tracers_move<2>), grid, block, 0, s, phase, m, dt, sides, k, held, t);
  return static_cast<int>(hipGetLastError());
}

template <class T>
int tracers_step(int dim, int phase, size_t m, double dt, T8gpuTracerSides sides, const uint64_t* keys, const int32_t* levels, int n,
                 int sub, vars_t<T> state, int32_t* hint, TracerArrays t, void* stream) {
  if (bad_forest(dim, n, keys, levels, sub) || bad_move(dim, phase, dt, sides) || m > MAX_PARTICLES)
    return static_cast<int>(hipErrorInvalidValue);
  if (m == 0) return 0;
  if (bad_arrays(t) || (n > 0 && bad_state<T>(dim, state))) return static_cast<int>(hipErrorInvalidValue);
  const dim3         grid((unsigned)((m + 255) / 256)), block(256);
  hipStream_t        s = static_cast<hipStream_t>(stream);
  const TracerForest f = forest_of(dim, keys, levels, n, sub);
  if (dim == 3)
    hipLaunchKernelGGL((k_tracers_step<T, 3>), grid, block, 0, s, phase, m, dt, sides, f, state, hint, t);
  else
    hipLaunchKernelGGL((k_tracers_step<T, 2>), grid, block, 0, s, phase, m, dt, sides, f, state, hint, t);
  return static_cast<int>(hipGetLastError());
}

}  // namespace t8gpu_hip

extern "C" {
int t8gpu_hip_tracers_velocity_f32(int dim, size_t num_points, const double* points, const uint64_t* keys, const int32_t* levels,
                                   int num_elements, int cells_per_axis, T8gpuVars_f32 state, int32_t* hint, double* k, int32_t* held,
                                   void* stream) {
  return t8gpu_hip::tracers_velocity<float>(dim, num_points, points, keys, levels, num_elements, cells_per_axis, state, hint, k, held,
                                            stream);
}
int t8gpu_hip_tracers_velocity_f64(int dim, size_t num_points, const double* points, const uint64_t* keys, const int32_t* levels,
                                   int num_elements, int cells_per_axis, T8gpuVars_f64 state, int32_t* hint, double* k, int32_t* held,
                                   void* stream) {
  return t8gpu_hip::tracers_velocity<double>(dim, num_points, points, keys, levels, num_elements, cells_per_axis, state, hint, k, held,
                                             stream);
}
int t8gpu_hip_tracers_move(int dim, int phase, size_t num_points, double dt, T8gpuTracerSides sides, const double* k,
                           const int32_t* held, double* x, double* xs, double* k1, uint8_t* flag, uint8_t* status, void* stream) {
  return t8gpu_hip::tracers_move(dim, phase, num_points, dt, sides, k, held, t8gpu_hip::TracerArrays{x, xs, k1, flag, status}, stream);
}
int t8gpu_hip_tracers_step_f32(int dim, int phase, size_t num_points, double dt, T8gpuTracerSides sides, const uint64_t* keys,
                               const int32_t* levels, int num_elements, int cells_per_axis, T8gpuVars_f32 state, int32_t* hint,
                               double* x, double* xs, double* k1, uint8_t* flag, uint8_t* status, void* stream) {
  return t8gpu_hip::tracers_step<float>(dim, phase, num_points, dt, sides, keys, levels, num_elements, cells_per_axis, state, hint,
                                        t8gpu_hip::TracerArrays{x, xs, k1, flag, status}, stream);
}
int t8gpu_hip_tracers_step_f64(int dim, int phase, size_t num_points, double dt, T8gpuTracerSides sides, const uint64_t* keys,
                               const int32_t* levels, int num_elements, int cells_per_axis, T8gpuVars_f64 state, int32_t* hint,
                               double* x, double* xs, double* k1, uint8_t* flag, uint8_t* status, void* stream) {
  return t8gpu_hip::tracers_step<double>(dim, phase, num_points, dt, sides, keys, levels, num_elements, cells_per_axis, state, hint,
                                         t8gpu_hip::TracerArrays{x, xs, k1, flag, status}, stream);
}
}
