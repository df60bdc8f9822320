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
// bits whatever the launch shape. Values are cast to double and never interpolated. The averages along homogeneous axes
//  add such per-pixel sums across a wavefront, in an order that is part of their definition.
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
// What a pixel takes from the forest, found once per pixel: the range [a, b) of the range case, or the one element e that
// holds P (-1: none), the subcells of it that P covers (first index, count per axis) and their common weight w.
struct PixelCover {
  int    a, b, e, first, cnt;
  bool   range;
  double w;
};

template <int DIM>
__device__ __forceinline__ PixelCover pixel_cover(int L, int px, int py, int pz, const uint64_t* __restrict__ keys,
                                                  const int32_t* __restrict__ levels, int n, int sub) {
  const int      up = SAMPLE_D - L;
  const uint64_t kp = key_of<DIM>((uint32_t)px << up, (uint32_t)py << up, DIM == 3 ? (uint32_t)pz << up : 0u);
  const uint64_t sp = span_of<DIM>(L);
  PixelCover     c;
  c.a = count_before<true>(keys, n, kp), c.b = count_before<true>(keys, n, kp + sp);
  c.range = c.b > c.a && levels[c.a] >= L;
  c.e = -1, c.first = 0, c.cnt = 1;
  c.w = 0.0;
  if (!c.range) {
    int e = c.b > c.a ? c.a : c.a - 1;
    if (e >= 0 && kp - keys[e] >= span_of<DIM>(levels[e])) e = -1;
    if (e >= 0) {
      const int l = levels[e];
      if (sub == 1 || L >= l + 2) {
        c.w = ldexp(1.0, -DIM * L);
        if (sub != 1) {
          const int sh = L - l - 2;
          c.first = ((px >> sh) & 3) + 4 * ((py >> sh) & 3) + (DIM == 3 ? 16 * ((pz >> sh) & 3) : 0);
        }
      } else {                                   // L = l + 1: half a block per axis
        c.w     = ldexp(1.0, -DIM * (l + 2));
        c.cnt   = 2;
        c.first = 2 * (px & 1) + 8 * (py & 1) + (DIM == 3 ? 32 * (pz & 1) : 0);
      }
    }
    c.e = e;
  }
  return c;
}

// sum of w q of plane k over the cells of a cover, in ascending storage order; ws receives the sum of w (the same for every k)
template <class T, int DIM>
__device__ __forceinline__ double pixel_sum(const PixelCover& c, const int32_t* __restrict__ levels, int sub,
                                            const sample_planes_t<T>& src, int k, double& ws) {
  const int S = sub == 1 ? 1 : (DIM == 3 ? 64 : 16);
  double    s = 0.0;
  ws = 0.0;
  if (c.range) {
    for (int el = c.a; el < c.b; el++) {
      const double wl = ldexp(1.0, -DIM * (levels[el] + (sub == 1 ? 0 : 2)));
      for (int i = 0; i < S; i++) {
        s += wl * plane_value<T>(src, k, (size_t)el * S + i);
        ws += wl;
      }
    }
  } else if (c.e >= 0) {
    for (int kk = 0; kk < (DIM == 3 ? c.cnt : 1); kk++)
      for (int jj = 0; jj < c.cnt; jj++)
        for (int ii = 0; ii < c.cnt; ii++) {
          s += c.w * plane_value<T>(src, k, (size_t)c.e * S + c.first + ii + 4 * jj + 16 * kk);
          ws += c.w;
        }
  }
  return s;
}

template <class T, int DIM>
__global__ __launch_bounds__(64) void k_sample_uniform(int L, const uint64_t* __restrict__ keys, const int32_t* __restrict__ levels,
                                                       int n, int sub, int n_planes, sample_planes_t<T> src, double fill,
                                                       double* __restrict__ sums, double* __restrict__ weights) {
  const int side = 1 << L;
  int       px, py, pz;
  if (!tile_pixel(side, side, px, py, pz)) return;
  const size_t pixels = (size_t)1 << (DIM * L);
  const size_t i      = (size_t)px + (size_t)side * ((size_t)py + (size_t)side * pz);
  const PixelCover c = pixel_cover<DIM>(L, px, py, pz, keys, levels, n, sub);
  double wsum = 0.0;
  for (int k = 0; k < n_planes; k++) {
    double       ws;
    const double s = pixel_sum<T, DIM>(c, levels, sub, src, k, ws);
    wsum = ws;
    sums[(size_t)k * pixels + i] = weights ? s : (ws > 0.0 ? s / ws : fill);
  }
  if (weights) weights[i] = wsum;                // (the same sum of w for every plane)
}

// ---- average: the uniform sums of level L added along the mesh axes of `mask`, one wavefront per (bin, chunk) -----------------
// A bin is a pixel of the kept axes, index sum p_K[i] side^i over the kept axes K ascending; a reduced pixel of it has index
// r = sum p_A[i] side^i over the averaged axes A ascending, r < R = side^|A|. Chunk c of a bin holds r in [4096 c, 4096 c + 4096):
// lane j adds to +0 the pixels r = 4096 c + 64 t + j for t = 0 .. 63 ascending (r >= R: skipped), the 64 lane values meet in the
// xor butterfly s = 32 .. 1, and the chunk values of a bin are added to +0 in ascending c (here when there is one chunk, else by
// k_sample_average_finish from `scratch`). host_average of sample.py is this in numpy. The sums sit in registers: the plane loop
// is unrolled over T8GPU_SAMPLE_PLANES with constant indices.
constexpr int AVG_CHUNK = T8GPU_SAMPLE_AVERAGE_CHUNK;
static_assert(AVG_CHUNK == 64 * 64, "a chunk is 64 rounds of one wavefront");

__device__ __forceinline__ double wave_butterfly(double v) {
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
  return v;
}

template <class T, int DIM>
__global__ __launch_bounds__(64) void k_sample_average(int L, int mask, uint64_t R, unsigned chunks, const uint64_t* __restrict__ keys,
                                                       const int32_t* __restrict__ levels, int n, int sub, int n_planes,
                                                       sample_planes_t<T> src, double fill, size_t bins, double* __restrict__ sums,
                                                       double* __restrict__ weights, double* __restrict__ scratch) {
  const unsigned chunk = blockIdx.x % chunks;
  const uint64_t bin   = blockIdx.x / chunks;
  const int      lane  = threadIdx.x;
  const uint32_t low   = (1u << L) - 1u;
  double         acc[T8GPU_SAMPLE_PLANES];
  double         wacc = 0.0;
#pragma unroll
  for (int k = 0; k < T8GPU_SAMPLE_PLANES; k++) acc[k] = 0.0;
  for (int t = 0; t < 64; t++) {
    const uint64_t r = (uint64_t)chunk * AVG_CHUNK + (uint64_t)(64 * t + lane);
    if (r < R) {
      uint64_t rr = r, bb = bin;
      int      p[3] = {0, 0, 0};
#pragma unroll
      for (int a = 0; a < DIM; a++) {
        if ((mask >> a) & 1) {
          p[a] = (int)(rr & low);
          rr >>= L;
        } else {
          p[a] = (int)(bb & low);
          bb >>= L;
        }
      }
      const PixelCover c = pixel_cover<DIM>(L, p[0], p[1], p[2], keys, levels, n, sub);
      double           ws = 0.0;
#pragma unroll
      for (int k = 0; k < T8GPU_SAMPLE_PLANES; k++)
        if (k < n_planes) acc[k] = acc[k] + pixel_sum<T, DIM>(c, levels, sub, src, k, ws);
      wacc = wacc + ws;
    }
  }
  wacc = wave_butterfly(wacc);
#pragma unroll
  for (int k = 0; k < T8GPU_SAMPLE_PLANES; k++)
    if (k < n_planes) acc[k] = wave_butterfly(acc[k]);
  if (lane != 0) return;
  if (chunks > 1) {                              // scratch[bin][chunk][planes + 1], the weight last
    double* out = scratch + ((size_t)bin * chunks + chunk) * (size_t)(n_planes + 1);
#pragma unroll
    for (int k = 0; k < T8GPU_SAMPLE_PLANES; k++)
      if (k < n_planes) out[k] = acc[k];
    out[n_planes] = wacc;
    return;
  }
  wacc = 0.0 + wacc;                             // (one chunk added to +0: the same bits, written for the definition's sake)
#pragma unroll
  for (int k = 0; k < T8GPU_SAMPLE_PLANES; k++)
    if (k < n_planes) sums[(size_t)k * bins + bin] = weights ? acc[k] : (wacc > 0.0 ? acc[k] / wacc : fill);
  if (weights) weights[bin] = wacc;
}

// one lane per (bin, plane): the chunk values of the plane and of the weight added to +0 in ascending chunk order
__global__ __launch_bounds__(256) void k_sample_average_finish(size_t bins, unsigned chunks, int n_planes, const double* __restrict__ scratch,
                                                               double fill, double* __restrict__ sums, double* __restrict__ weights) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= bins * (size_t)n_planes) return;
  const size_t  bin = i / n_planes;
  const int     k   = (int)(i % n_planes);
  const double* in  = scratch + bin * chunks * (size_t)(n_planes + 1);
  double        s = 0.0, w = 0.0;
  for (unsigned c = 0; c < chunks; c++) {
    s = s + in[(size_t)c * (n_planes + 1) + k];
    w = w + in[(size_t)c * (n_planes + 1) + n_planes];
  }
  sums[(size_t)k * bins + bin] = weights ? s : (w > 0.0 ? s / w : fill);
  if (weights && k == 0) weights[bin] = w;
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

template <class T>
int sample_average(int dim, int level, int mask, const uint64_t* keys, const int32_t* levels, int n, int sub, int n_planes,
                   sample_planes_t<T> src, double fill, double* sums, double* weights, double* scratch, void* stream) {
  if (bad_forest(dim, n, keys, levels, sub) || bad_planes<T>(n_planes, src)) return static_cast<int>(hipErrorInvalidValue);
  if (level < 0 || level > SAMPLE_D || dim * level > 36) return static_cast<int>(hipErrorInvalidValue);
  if (n_planes == 0 || !sums) return static_cast<int>(hipErrorInvalidValue);
  const int full = (1 << dim) - 1;
  if (mask <= 0 || mask >= full) return static_cast<int>(hipErrorInvalidValue);      // a non-empty proper subset of the axes
  const int      averaged = __builtin_popcount((unsigned)mask);
  const uint64_t R        = (uint64_t)1 << (level * averaged);
  const size_t   bins     = (size_t)1 << (level * (dim - averaged));
  const uint64_t chunks   = (R + AVG_CHUNK - 1) / AVG_CHUNK;
  const uint64_t blocks   = bins * chunks;
  if (blocks >= ((uint64_t)1 << 31) || (chunks > 1 && !scratch)) return static_cast<int>(hipErrorInvalidValue);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dim == 3)
    hipLaunchKernelGGL((k_sample_average<T, 3>), dim3((unsigned)blocks), dim3(64), 0, s, level, mask, R, (unsigned)chunks, keys, levels, n,
                       sub, n_planes, src, fill, bins, sums, weights, scratch);
  else
    hipLaunchKernelGGL((k_sample_average<T, 2>), dim3((unsigned)blocks), dim3(64), 0, s, level, mask, R, (unsigned)chunks, keys, levels, n,
                       sub, n_planes, src, fill, bins, sums, weights, scratch);
  int err = static_cast<int>(hipGetLastError());
  if (err != 0 || chunks == 1) return err;
  const size_t lanes = bins * (size_t)n_planes;
  hipLaunchKernelGGL(k_sample_average_finish, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, bins, (unsigned)chunks, n_planes,
                     scratch, fill, sums, weights);
  return static_cast<int>(hipGetLastError());
}

}  // namespace t8gpu_hip

extern "C" {
int t8gpu_hip_sample_average_f32(int dim, int level, int axes_mask, const uint64_t* keys, const int32_t* levels, int num_elements,
                                 int cells_per_axis, int num_planes, T8gpuSamplePlanes_f32 planes, double fill, double* sums,
                                 double* weights, double* scratch, void* stream) {
  return t8gpu_hip::sample_average<float>(dim, level, axes_mask, keys, levels, num_elements, cells_per_axis, num_planes, planes, fill,
                                          sums, weights, scratch, stream);
}
int t8gpu_hip_sample_average_f64(int dim, int level, int axes_mask, const uint64_t* keys, const int32_t* levels, int num_elements,
                                 int cells_per_axis, int num_planes, T8gpuSamplePlanes_f64 planes, double fill, double* sums,
                                 double* weights, double* scratch, void* stream) {
  return t8gpu_hip::sample_average<double>(dim, level, axes_mask, keys, levels, num_elements, cells_per_axis, num_planes, planes, fill,
                                           sums, weights, scratch, stream);
}
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
