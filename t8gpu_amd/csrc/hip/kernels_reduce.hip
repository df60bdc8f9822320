// kernels_reduce.hip -- the two scalar reductions that sit right after the hot path.
//
//   max wave speed : compute_timestep() reduces the per-face speed estimates with thrust::reduce(max)
//                    and MPI_Allreduce (examples/compressible_euler/solver.cu:213-229);
//   integral       : compute_integral() copies a variable and the volumes to the host and sums
//                    vol * u there (solver.cu:190-211; subgrid: examples/subgrid/solver.inl:281-305).
// Both become a two-level device reduction (grid-stride partials per workgroup -> one workgroup) that
// writes a device scalar, stays on the stream and is bitwise reproducible (fixed tree, no atomics).
// The integral accumulates in double whatever float_type is. The maximum starts from 0 and PROPAGATES NaN: one NaN speed
// estimate (a blown-up state) gives a NaN result wherever in the array it sits, so compute_timestep never turns such a
// state into a finite step on one layout and NaN on another.
// A third one serves the step driver: the OR of the raw bits of four planes (is a plane all +0?).
#include <hip/hip_runtime.h>

#include "t8gpu_hip.h"

namespace t8gpu_hip {

constexpr int kReduceBlocks = 1024;

struct OpMax {
  static __device__ double identity() { return 0.0; }  // speeds are >= 0; the reference starts from 0 too
  // a NaN on either side comes out (`a > b ? a : b` alone keeps or drops one depending on which side it arrives)
  static __device__ double apply(double a, double b) { return (a > b || a != a) ? a : b; }
};
struct OpSum {
  static __device__ double identity() { return 0.0; }
  static __device__ double apply(double a, double b) { return a + b; }
};

template <class Op>
__device__ double block_reduce(double v) {
  __shared__ double part[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = Op::apply(v, __shfl_down(v, off, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = Op::identity();
  if (threadIdx.x == 0) r = Op::apply(Op::apply(part[0], part[1]), Op::apply(part[2], part[3]));
  __syncthreads();
  return r;  // valid in thread 0
}

template <class T>
__global__ __launch_bounds__(256) void k_max_partial(size_t n, const T* __restrict__ x, double* __restrict__ partial) {
  double v = OpMax::identity();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) v = OpMax::apply(v, (double)x[i]);
  v = block_reduce<OpMax>(v);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

template <class T>
__global__ __launch_bounds__(256) void k_integral_partial(size_t ncells, int cells_per_element, const T* __restrict__ u,
                                                          const T* __restrict__ volume, double* __restrict__ partial) {
  double       v   = 0.0;
  const double inv = 1.0 / cells_per_element;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < ncells; i += (size_t)gridDim.x * 256)
    v += (double)volume[i / cells_per_element] * inv * (double)u[i];
  v = block_reduce<OpSum>(v);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

template <class Op>
__global__ __launch_bounds__(256) void k_final(int nparts, const double* __restrict__ partial, double* __restrict__ result) {
  double v = Op::identity();
  for (int i = threadIdx.x; i < nparts; i += 256) v = Op::apply(v, partial[i]);
  v = block_reduce<Op>(v);
  if (threadIdx.x == 0) *result = v;
}

inline int blocks_for(size_t n) {
  size_t b = (n + 255) / 256;
  return static_cast<int>(b < 1 ? 1 : (b > kReduceBlocks ? kReduceBlocks : b));
}

template <class T>
int max_speed(size_t n, const T* speed, void* workspace, double* result, void* stream) {
  if (!workspace || !result) return static_cast<int>(hipErrorInvalidValue);
  hipStream_t s  = static_cast<hipStream_t>(stream);
  const int   nb = blocks_for(n);
  hipLaunchKernelGGL((k_max_partial<T>), dim3(nb), dim3(256), 0, s, n, speed, static_cast<double*>(workspace));
  hipLaunchKernelGGL((k_final<OpMax>), dim3(1), dim3(256), 0, s, nb, static_cast<const double*>(workspace), result);
  return static_cast<int>(hipGetLastError());
}

template <class T>
int integral(size_t ncells, int cpe, const T* u, const T* volume, void* workspace, double* result, void* stream) {
  if (!workspace || !result || cpe < 1) return static_cast<int>(hipErrorInvalidValue);
  hipStream_t s  = static_cast<hipStream_t>(stream);
  const int   nb = blocks_for(ncells);
  hipLaunchKernelGGL((k_integral_partial<T>), dim3(nb), dim3(256), 0, s, ncells, cpe, u, volume, static_cast<double*>(workspace));
  hipLaunchKernelGGL((k_final<OpSum>), dim3(1), dim3(256), 0, s, nb, static_cast<const double*>(workspace), result);
  return static_cast<int>(hipGetLastError());
}

// ---- are these planes all +0? (stepper.hip: the planar decision of a 2D run) --------------------------------------------------
// OR of the raw 32-bit words of four planes of `nwords` words each, one plane per blockIdx.y: 16-byte loads over the aligned
// body (four in flight per lane), the at most three words before and after it by workgroup 0, a wavefront OR by shuffles and
// ONE atomic OR per workgroup into out[plane] (skipped where the workgroup saw only zero bits). -0.0 has a bit set, +0 has none.
struct OrPlanes {
  const uint32_t* p[4];
};
__global__ __launch_bounds__(256) void k_planes_or_bits(OrPlanes P, size_t nwords, uint32_t* __restrict__ out) {
  const uint32_t* const p = P.p[blockIdx.y];
  size_t head = ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2;   // words before the first 16-byte boundary
  if (head > nwords) head = nwords;
  const size_t       nvec = (nwords - head) >> 2;
  const size_t       tail = nwords - head - 4 * nvec;                       // < 4
  const uint4* const v    = reinterpret_cast<const uint4*>(p + head);
  const size_t       step = static_cast<size_t>(gridDim.x) * 256;
  uint32_t           acc  = 0;
  size_t             i    = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  for (; i + 3 * step < nvec; i += 4 * step) {
    const uint4 a = v[i], b = v[i + step], c = v[i + 2 * step], d = v[i + 3 * step];
    acc |= (a.x | a.y | a.z | a.w) | (b.x | b.y | b.z | b.w) | (c.x | c.y | c.z | c.w) | (d.x | d.y | d.z | d.w);
  }
  for (; i < nvec; i += step) {
    const uint4 a = v[i];
    acc |= a.x | a.y | a.z | a.w;
  }
  if (blockIdx.x == 0) {
    if (threadIdx.x < head) acc |= p[threadIdx.x];
    if (threadIdx.x < tail) acc |= p[head + 4 * nvec + threadIdx.x];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc |= __shfl_xor(acc, off, 64);
  __shared__ uint32_t part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t r = part[0] | part[1] | part[2] | part[3];
    if (r) atomicOr(out + blockIdx.y, r);
  }
}

template <class T>
int planes_or_bits(size_t n, const T* const planes[4], uint32_t* out4, void* stream) {
  if (!planes || !out4) return static_cast<int>(hipErrorInvalidValue);
  if (n == 0) return 0;
  OrPlanes P;
  for (int j = 0; j < 4; j++) {
    if (!planes[j]) return static_cast<int>(hipErrorInvalidValue);
    P.p[j] = reinterpret_cast<const uint32_t*>(planes[j]);
  }
  const size_t nwords = n * (sizeof(T) / 4);
  const size_t per    = 256 * 4 * 4;   // words a workgroup takes per round of its loop
  size_t       nb     = (nwords + per - 1) / per;
  nb                  = nb < 1 ? 1 : (nb > 2048 ? 2048 : nb);
  hipLaunchKernelGGL(k_planes_or_bits, dim3(static_cast<unsigned>(nb), 4), dim3(256), 0, static_cast<hipStream_t>(stream), P, nwords, out4);
  return static_cast<int>(hipGetLastError());
}

}  // namespace t8gpu_hip

extern "C" {
int t8gpu_hip_planes_or_bits_f32(size_t n, const float* const planes[4], uint32_t* out4, void* stream) {
  return t8gpu_hip::planes_or_bits<float>(n, planes, out4, stream);
}
int t8gpu_hip_planes_or_bits_f64(size_t n, const double* const planes[4], uint32_t* out4, void* stream) {
  return t8gpu_hip::planes_or_bits<double>(n, planes, out4, stream);
}
size_t t8gpu_hip_reduce_workspace_bytes(void) { return sizeof(double) * t8gpu_hip::kReduceBlocks; }
int t8gpu_hip_max_speed_f32(size_t n, const float* speed, void* workspace, double* result, void* stream) {
  return t8gpu_hip::max_speed<float>(n, speed, workspace, result, stream);
}
int t8gpu_hip_max_speed_f64(size_t n, const double* speed, void* workspace, double* result, void* stream) {
  return t8gpu_hip::max_speed<double>(n, speed, workspace, result, stream);
}
int t8gpu_hip_integral_f32(size_t num_cells, int cells_per_element, const float* variable, const float* volume,
                           void* workspace, double* result, void* stream) {
  return t8gpu_hip::integral<float>(num_cells, cells_per_element, variable, volume, workspace, result, stream);
}
int t8gpu_hip_integral_f64(size_t num_cells, int cells_per_element, const double* variable, const double* volume,
                           void* workspace, double* result, void* stream) {
  return t8gpu_hip::integral<double>(num_cells, cells_per_element, variable, volume, workspace, result, stream);
}
}
