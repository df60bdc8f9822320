// forest/locate.hpp -- from a coordinate of the unit square / cube to a storage index on a Cartesian forest: Morton keys, the
// searches on them and locate_cell. Shared by sample.hip (probe points, image grids, resampling) and tracers.hip (the velocity
// at a particle). Definitions: t8gpu_hip.h, DESIGN.md §12. In short, with D = T8GPU_SAMPLE_DEPTH = 20: the key of a point is the
// bit-interleave of floor(x 2^D) per axis, x in the lowest bit; keys[e] is the key of element e's lower corner. In storage order
// the keys ascend strictly and element e covers the keys [keys[e], keys[e] + 2^(dim (D - level[e]))). So the element of a point
// is upper_bound(keys, key) - 1 plus one containment check (which also tells a point of another rank).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "t8gpu_hip.h"

namespace t8gpu_hip {

constexpr int SAMPLE_D = T8GPU_SAMPLE_DEPTH;

// ---- keys ---------------------------------------------------------------------------------------------------------------
// bit b of v (b < 21) to bit 2 b / 3 b
__device__ __forceinline__ uint64_t spread2(uint32_t v) {
  uint64_t x = v;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}
__device__ __forceinline__ uint64_t spread3(uint32_t v) {
  uint64_t x = v & 0x1FFFFFu;
  x = (x | (x << 32)) & 0x001F00000000FFFFull;
  x = (x | (x << 16)) & 0x001F0000FF0000FFull;
  x = (x | (x << 8)) & 0x100F00F00F00F00Full;
  x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}
template <int DIM>
__device__ __forceinline__ uint64_t key_of(uint32_t ix, uint32_t iy, uint32_t iz) {
  if constexpr (DIM == 2)
    return spread2(ix) | (spread2(iy) << 1);
  else
    return spread3(ix) | (spread3(iy) << 1) | (spread3(iz) << 2);
}

// keys a cell of level l covers
template <int DIM>
__device__ __forceinline__ uint64_t span_of(int level) {
  return 1ull << (DIM * (SAMPLE_D - level));
}

// number of keys[0, n) that are <= key (STRICT = false: upper bound) or < key (STRICT = true: lower bound). Branch-free: every
// lane runs the same ceil(log2 n) rounds, and every read is inside [0, n).
template <bool STRICT>
__device__ __forceinline__ int count_before(const uint64_t* __restrict__ keys, int n, uint64_t key) {
  if (n <= 0) return 0;
  int base = 0, len = n;
  while (len > 1) {
    const int      half = len >> 1;
    const uint64_t k    = keys[base + half];
    base = (STRICT ? k < key : k <= key) ? base + half : base;
    len -= half;
  }
  const uint64_t k = keys[base];
  return base + ((STRICT ? k < key : k <= key) ? 1 : 0);
}

// the in-range test on the doubles themselves: NaN, +-inf, 1e300 and -1e-300 all fail it, and only what passes is converted
__device__ __forceinline__ bool inside_unit(double x) { return x >= 0.0 && x < 1.0; }

// storage index of the owned cell that holds (x, y, z) under the half-open rule, or -1. SUB: cells per block axis (1 or 4).
template <int DIM>
__device__ __forceinline__ int32_t locate_cell(double x, double y, double z, const uint64_t* __restrict__ keys,
                                               const int32_t* __restrict__ levels, int n, int sub) {
  if (!(inside_unit(x) && inside_unit(y) && (DIM == 2 || inside_unit(z)))) return -1;
  const double   scale = (double)(1u << SAMPLE_D);
  const uint32_t ix = (uint32_t)(x * scale), iy = (uint32_t)(y * scale), iz = DIM == 3 ? (uint32_t)(z * scale) : 0u;
  const uint64_t key = key_of<DIM>(ix, iy, iz);
  const int      e   = count_before<false>(keys, n, key) - 1;
  if (e < 0) return -1;
  const int l = levels[e];
  if (key - keys[e] >= span_of<DIM>(l)) return -1;          // (past this rank's last element, or in a gap of its range)
  if (sub == 1) return e;
  const int sh = SAMPLE_D - l - 2;
  int       c  = (int)((ix >> sh) & 3u) + 4 * (int)((iy >> sh) & 3u);
  if constexpr (DIM == 3) c += 16 * (int)((iz >> sh) & 3u);
  return e * (DIM == 3 ? 64 : 16) + c;
}

// locate_cell with a guess: when `hint` lies in [0, n) and that element covers the point's key, the search is skipped; the
// result is that of locate_cell whatever `hint` holds (an element covers a key or it does not, and at most one does).
// `elem` receives the element found, or -1. Nothing is read through `hint` before it is range-checked.
template <int DIM>
__device__ __forceinline__ int32_t locate_cell_hinted(double x, double y, double z, const uint64_t* __restrict__ keys,
                                                      const int32_t* __restrict__ levels, int n, int sub, int32_t hint,
                                                      int32_t& elem) {
  elem = -1;
  if (n <= 0 || !(inside_unit(x) && inside_unit(y) && (DIM == 2 || inside_unit(z)))) return -1;
  const double   scale = (double)(1u << SAMPLE_D);
  const uint32_t ix = (uint32_t)(x * scale), iy = (uint32_t)(y * scale), iz = DIM == 3 ? (uint32_t)(z * scale) : 0u;
  const uint64_t key = key_of<DIM>(ix, iy, iz);
  int            e = -1, l = 0;
  if (hint >= 0 && hint < n) {
    const uint64_t kh = keys[hint];
    const int      lh = levels[hint];
    if (key >= kh && key - kh < span_of<DIM>(lh)) e = hint, l = lh;
  }
  if (e < 0) {
    e = count_before<false>(keys, n, key) - 1;
    if (e < 0) return -1;
    l = levels[e];
    if (key - keys[e] >= span_of<DIM>(l)) return -1;
  }
  elem = e;
  if (sub == 1) return e;
  const int sh = SAMPLE_D - l - 2;
  int       c  = (int)((ix >> sh) & 3u) + 4 * (int)((iy >> sh) & 3u);
  if constexpr (DIM == 3) c += 16 * (int)((iz >> sh) & 3u);
  return e * (DIM == 3 ? 64 : 16) + c;
}

// what every launcher on a forest refuses
inline bool bad_forest(int dim, int n, const uint64_t* keys, const int32_t* levels, int sub) {
  return (dim != 2 && dim != 3) || n < 0 || (sub != 1 && sub != 4) || (n > 0 && (!keys || !levels)) ||
         (double)n * (sub == 1 ? 1.0 : (dim == 3 ? 64.0 : 16.0)) >= 2147483648.0;
}

}  // namespace t8gpu_hip
