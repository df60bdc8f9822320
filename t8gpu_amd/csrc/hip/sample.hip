// sample.hip -- sampling of cell data on Cartesian forests: probe points, image grids and slices, conservative resampling
// onto a uniform level. The reference has nothing of the kind; the arrays a run describes itself with come in storage
// order (Morton order of the leaves, column-major inside a Subgrid block), and this file is the way from a coordinate to
// a storage index on the device.
//
// Not a stage kernel: an output pass between steps, self-contained like fields.hip. Definitions: t8gpu_hip.h,
// DESIGN.md §12. In short, with D = T8GPU_SAMPLE_DEPTH = 20: the key of a point is the bit-interleave of
// floor(x 2^D) per axis, x in the lowest bit; keys[e] is the key of element e's lower corner. In storage order the keys
// ascend strictly and element e covers the keys [keys[e], keys[e] + 2^(dim (D - level[e]))). So the element of a point
// is upper_bound(keys, key) - 1 plus one containment check (which also tells a point of another rank), and the
// elements inside a dyadic pixel are one contiguous index range between two lower bounds.
//
// Everything is a gather: no atomics, no LDS, sums in ascending storage order by one lane, so two calls give the same
// bits whatever the launch shape. Values are cast to double and never interpolated.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "t8gpu_hip.h"

// pixel centres must come out as numpy forms lo + (i + 0.5) (hi - lo) / n: no contraction into fused multiply-adds
#pragma clang fp contract(off)

#include "forest/locate.hpp"      // keys, searches, locate_cell, bad_forest: shared with tracers.hip

namespace t8gpu_hip {

template <class T>
using sample_planes_t = std::conditional_t<std::is_same<T, float>::value, T8gpuSamplePlanes_f32, T8gpuSamplePlanes_f64>;

template <class T>
__device__ __forceinline__ double plane_value(const sample_planes_t<T>& src, int k, size_t cell) {
  return src.q[k] ? (double)src.q[k][cell] : src.d[k][cell];
}

// ---- locate, gather: one lane per point -----------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void k_sample_locate(size_t m, const double* __restrict__ points,
                                                       const uint64_t* __restrict__ keys, const int32_t* __restrict__ levels,
                                                       int n, int sub, int32_t* __restrict__ cells) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const double x = points[DIM * i], y = points[DIM * i + 1], z = DIM == 3 ? points[DIM * i + 2] : 0.0;
  cells[i] = locate_cell<DIM>(x, y, z, keys, levels, n, sub);
}

template <class T>
__global__ __launch_bounds__(256) void k_sample_gather(size_t m, const int32_t* __restrict__ cells, int n_planes,
                                                       sample_planes_t<T> src, double fill, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const int32_t c = cells[i];
  for (int k = 0; k < n_planes; k++) out[(size_t)k * m + i] = c >= 0 ? plane_value<T>(src, k, (size_t)c) : fill;
}

// ---- grid: locate and gather fused, one wavefront per 8 x 8 tile of pixels -------------------------------------------------
// block b: tile (b % tx, (b / tx) % ty) of layer b / (tx ty); lane: pixel (lane % 8, lane / 8) of the tile
__device__ __forceinline__ bool tile_pixel(int nx, int ny, int& px, int& py, int& pz) {
  const int tx = (nx + 7) >> 3, ty = (ny + 7) >> 3;
  const int b  = blockIdx.x;
  px = ((b % tx) << 3) + (threadIdx.x & 7);
  py = (((b / tx) % ty) << 3) + (threadIdx.x >> 3);
  pz = b / (tx * ty);
  return px < nx && py < ny;
}

template <class T, int DIM>
__global__ __launch_bounds__(64) void k_sample_grid(T8gpuSampleGrid g, const uint64_t* __restrict__ keys,
                                                    const int32_t* __restrict__ levels, int n, int sub, int n_planes,
                                                    sample_planes_t<T> src, double fill, double* __restrict__ out,
                                                    int32_t* __restrict__ cells) {
  int px, py, pz;
  if (!tile_pixel(g.n[0], g.n[1], px, py, pz)) return;       // (ragged tiles: masked)
  const double x = g.lo[0] + ((double)px + 0.5) * (g.hi[0] - g.lo[0]) / (double)g.n[0];
  const double y = g.lo[1] + ((double)py + 0.5) * (g.hi[1] - g.lo[1]) / (double)g.n[1];
  const double z = DIM == 3 ? g.lo[2] + ((double)pz + 0.5) * (g.hi[2] - g.lo[2]) / (double)g.n[2] : 0.0;
  const int32_t c = locate_cell<DIM>(x, y, z, keys, levels, n, sub);
  const size_t  pixels = (size_t)g.n[0] * g.n[1] * (DIM == 3 ? g.n[2] : 1);
  const size_t  i      = (size_t)px + (size_t)g.n[0] * ((size_t)py + (size_t)g.n[1] * pz);
  if (cells) cells[i] = c;
  for (int k = 0; k < n_planes; k++) out[(size_t)k * pixels + i] = c >= 0 ? plane_value<T>(src, k, (size_t)c) : fill;
}

// ---- uniform: sums of w q and of w over pixel P of level L, w = 2^(-dim level of the overlap) --------------------------------
// With kp the key of P's lower corner and P covering [kp, kp + sp): the elements that START inside P are [a, b) between two
// lower bounds. Either they are as fine as P or finer and tile the owned part of P (the range case), or one element as
// coarse as P or coarser holds P (it starts at kp: a itself; or before it: a - 1), or this rank owns nothing of P.
// For blocks of level l the cells have level l + 2: L <= l is the range case over whole blocks, L = l + 1 takes the 2^dim
// subcells of P's corner of the block, L >= l + 2 the one subcell that holds P.
template <class T, int DIM>
__global__ __launch_bounds__(64) void k_sample_uniform(int L, const uint64_t* __restrict__ keys, const int32_t* __restrict__ levels,
                                                       int n, int sub, int n_planes, sample_planes_t<T> src, double fill,
                                                       double* __restrict__ sums, double* __restrict__ weights) {
  const int side = 1 << L;
  int       px, py, pz;
  if (!tile_pixel(side, side, px, py, pz)) return;
  const size_t pixels = (size_t)1 << (DIM * L);
  const size_t i      = (size_t)px + (size_t)side * ((size_t)py + (size_t)side * pz);
  const int    up     = SAMPLE_D - L;
  const uint64_t kp = key_of<DIM>((uint32_t)px << up, (uint32_t)py << up, DIM == 3 ? (uint32_t)pz << up : 0u);
  const uint64_t sp = span_of<DIM>(L);
  const int    S = sub == 1 ? 1 : (DIM == 3 ? 64 : 16);
  const int    a = count_before<true>(keys, n, kp), b = count_before<true>(keys, n, kp + sp);
  const bool   range = b > a && levels[a] >= L;
  // the one element that may hold P, the subcells of it that P covers (first index, counts per axis), their common weight
  int    e = -1, first = 0, cnt = 1;
  double w = 0.0;
  if (!range) {
    e = b > a ? a : a - 1;
    if (e >= 0 && kp - keys[e] >= span_of<DIM>(levels[e])) e = -1;
    if (e >= 0) {
      const int l = levels[e];
      if (sub == 1 || L >= l + 2) {
        w = ldexp(1.0, -DIM * L);
        if (sub != 1) {
          const int sh = L - l - 2;
          first = ((px >> sh) & 3) + 4 * ((py >> sh) & 3) + (DIM == 3 ? 16 * ((pz >> sh) & 3) : 0);
        }
      } else {                                   // L = l + 1: half a block per axis
        w     = ldexp(1.0, -DIM * (l + 2));
        cnt   = 2;
        first = 2 * (px & 1) + 8 * (py & 1) + (DIM == 3 ? 32 * (pz & 1) : 0);
      }
    }
  }
  double wsum = 0.0;
  for (int k = 0; k < n_planes; k++) {
    double s = 0.0, ws = 0.0;
    if (range) {
      for (int el = a; el < b; el++) {
        const double wl = ldexp(1.0, -DIM * (levels[el] + (sub == 1 ? 0 : 2)));
        for (int c = 0; c < S; c++) {
          s += wl * plane_value<T>(src, k, (size_t)el * S + c);
          ws += wl;
        }
      }
    } else if (e >= 0) {
      for (int kk = 0; kk < (DIM == 3 ? cnt : 1); kk++)
        for (int jj = 0; jj < cnt; jj++)
          for (int ii = 0; ii < cnt; ii++) {
            s += w * plane_value<T>(src, k, (size_t)e * S + first + ii + 4 * jj + 16 * kk);
            ws += w;
          }
    }
    wsum = ws;
    sums[(size_t)k * pixels + i] = weights ? s : (ws > 0.0 ? s / ws : fill);
  }
  if (weights) weights[i] = wsum;                // (the same sum of w for every plane)
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
template <class T>
bool bad_planes(int n_planes, const sample_planes_t<T>& src) {
  if (n_planes < 0 || n_planes > T8GPU_SAMPLE_PLANES) return true;
  for (int k = 0; k < n_planes; k++)
    if (!src.q[k] && !src.d[k]) return true;
  return false;
}

inline int sample_locate(int dim, size_t m, const double* points, const uint64_t* keys, const int32_t* levels, int n, int sub,
                         int32_t* cells, void* stream) {
  if (bad_forest(dim, n, keys, levels, sub) || m > ((size_t)1 << 39)) return static_cast<int>(hipErrorInvalidValue);
  if (m == 0) return 0;
  if (!points || !cells) return static_cast<int>(hipErrorInvalidValue);
  const dim3  grid((unsigned)((m + 255) / 256)), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dim == 3)
    hipLaunchKernelGGL((k_sample_locate<3>), grid, block, 0, s, m, points, keys, levels, n, sub, cells);
  else
    hipLaunchKernelGGL((k_sample_locate<2>), grid, block, 0, s, m, points, keys, levels, n, sub, cells);
  return static_cast<int>(hipGetLastError());
}

template <class T>
int sample_gather(size_t m, const int32_t* cells, int n_planes, sample_planes_t<T> src, double fill, double* out, void* stream) {
  if (bad_planes<T>(n_planes, src) || m > ((size_t)1 << 39)) return static_cast<int>(hipErrorInvalidValue);
  if (m == 0 || n_planes == 0) return 0;
  if (!cells || !out) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL((k_sample_gather<T>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), m, cells,
                     n_planes, src, fill, out);
  return static_cast<int>(hipGetLastError());
}

// blocks of a launch over nx x ny x nz pixels in 8 x 8 x 1 tiles, or 0 when they do not fit a grid
inline size_t tile_blocks(size_t nx, size_t ny, size_t nz) {
  const size_t blocks = ((nx + 7) / 8) * ((ny + 7) / 8) * nz;
  return blocks < ((size_t)1 << 31) ? blocks : 0;
}

template <class T>
int sample_grid(int dim, T8gpuSampleGrid g, const uint64_t* keys, const int32_t* levels, int n, int sub, int n_planes,
                sample_planes_t<T> src, double fill, double* out, int32_t* cells, void* stream) {
  if (bad_forest(dim, n, keys, levels, sub) || bad_planes<T>(n_planes, src)) return static_cast<int>(hipErrorInvalidValue);
  for (int a = 0; a < dim; a++)
    if (g.n[a] <= 0 || g.n[a] > (1 << 24)) return static_cast<int>(hipErrorInvalidValue);      // (a grid of size 0: an error)
  if ((n_planes > 0 && !out) || (n_planes == 0 && !cells)) return static_cast<int>(hipErrorInvalidValue);
  const size_t blocks = tile_blocks(g.n[0], g.n[1], dim == 3 ? g.n[2] : 1);
  if (blocks == 0) return static_cast<int>(hipErrorInvalidValue);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dim == 3)
    hipLaunchKernelGGL((k_sample_grid<T, 3>), dim3((unsigned)blocks), dim3(64), 0, s, g, keys, levels, n, sub, n_planes, src, fill, out,
                       cells);
  else
    hipLaunchKernelGGL((k_sample_grid<T, 2>), dim3((unsigned)blocks), dim3(64), 0, s, g, keys, levels, n, sub, n_planes, src, fill, out,
                       cells);
  return static_cast<int>(hipGetLastError());
}

template <class T>
int sample_uniform(int dim, int level, const uint64_t* keys, const int32_t* levels, int n, int sub, int n_planes,
                   sample_planes_t<T> src, double fill, double* sums, double* weights, void* stream) {
  if (bad_forest(dim, n, keys, levels, sub) || bad_planes<T>(n_planes, src)) return static_cast<int>(hipErrorInvalidValue);
  if (level < 0 || level > SAMPLE_D || dim * level > 36) return static_cast<int>(hipErrorInvalidValue);
  if (n_planes == 0 || !sums) return static_cast<int>(hipErrorInvalidValue);
  const size_t side   = (size_t)1 << level;
  const size_t blocks = tile_blocks(side, side, dim == 3 ? side : 1);
  if (blocks == 0) return static_cast<int>(hipErrorInvalidValue);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dim == 3)
    hipLaunchKernelGGL((k_sample_uniform<T, 3>), dim3((unsigned)blocks), dim3(64), 0, s, level, keys, levels, n, sub, n_planes, src, fill,
                       sums, weights);
  else
    hipLaunchKernelGGL((k_sample_uniform<T, 2>), dim3((unsigned)blocks), dim3(64), 0, s, level, keys, levels, n, sub, n_planes, src, fill,
                       sums, weights);
  return static_cast<int>(hipGetLastError());
}

}  // namespace t8gpu_hip

extern "C" {
int t8gpu_hip_sample_locate(int dim, size_t num_points, const double* points, const uint64_t* keys, const int32_t* levels,
                            int num_elements, int cells_per_axis, int32_t* cells, void* stream) {
  return t8gpu_hip::sample_locate(dim, num_points, points, keys, levels, num_elements, cells_per_axis, cells, stream);
}
int t8gpu_hip_sample_gather_f32(size_t num_points, const int32_t* cells, int num_planes, T8gpuSamplePlanes_f32 planes, double fill,
                                double* out, void* stream) {
  return t8gpu_hip::sample_gather<float>(num_points, cells, num_planes, planes, fill, out, stream);
}
int t8gpu_hip_sample_gather_f64(size_t num_points, const int32_t* cells, int num_planes, T8gpuSamplePlanes_f64 planes, double fill,
                                double* out, void* stream) {
  return t8gpu_hip::sample_gather<double>(num_points, cells, num_planes, planes, fill, out, stream);
}
int t8gpu_hip_sample_grid_f32(int dim, T8gpuSampleGrid grid, const uint64_t* keys, const int32_t* levels, int num_elements,
                              int cells_per_axis, int num_planes, T8gpuSamplePlanes_f32 planes, double fill, double* out,
                              int32_t* cells, void* stream) {
  return t8gpu_hip::sample_grid<float>(dim, grid, keys, levels, num_elements, cells_per_axis, num_planes, planes, fill, out, cells,
                                       stream);
}
int t8gpu_hip_sample_grid_f64(int dim, T8gpuSampleGrid grid, const uint64_t* keys, const int32_t* levels, int num_elements,
                              int cells_per_axis, int num_planes, T8gpuSamplePlanes_f64 planes, double fill, double* out,
                              int32_t* cells, void* stream) {
  return t8gpu_hip::sample_grid<double>(dim, grid, keys, levels, num_elements, cells_per_axis, num_planes, planes, fill, out, cells,
                                        stream);
}
int t8gpu_hip_sample_uniform_f32(int dim, int level, const uint64_t* keys, const int32_t* levels, int num_elements,
                                 int cells_per_axis, int num_planes, T8gpuSamplePlanes_f32 planes, double fill, double* sums,
                                 double* weights, void* stream) {
  return t8gpu_hip::sample_uniform<float>(dim, level, keys, levels, num_elements, cells_per_axis, num_planes, planes, fill, sums,
                                          weights, stream);
}
int t8gpu_hip_sample_uniform_f64(int dim, int level, const uint64_t* keys, const int32_t* levels, int num_elements,
                                 int cells_per_axis, int num_planes, T8gpuSamplePlanes_f64 planes, double fill, double* sums,
                                 double* weights, void* stream) {
  return t8gpu_hip::sample_uniform<double>(dim, level, keys, levels, num_elements, cells_per_axis, num_planes, planes, fill, sums,
                                           weights, stream);
}
}
