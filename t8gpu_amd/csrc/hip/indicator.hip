// indicator.hip -- the scale-free refinement indicator: Loehner's estimator without cross terms, per axis, on density,
// pressure, Mach number or entropy, with the usual noise filter and a closure for cells at a boundary. The reference steers
// its AMR by a dimensional density jump (estimate_gradient, examples/compressible_euler/kernels.cu:471-501, summed with float
// atomics; in-block H1 seminorm for Subgrid); this one is dimensionless, lies in [0, 1], does not depend on the level, looks
// across block faces and is a GATHER: one sum per cell in a fixed order, no atomics, two calls give the same bits.
//
// Not a stage kernel: a pass of the adapt cycle, self-contained like fields.hip, whose formulas for the quantities and whose
// sub-face walk it restates (so no kernel header changes with it). Definition: t8gpu_hip.h, DESIGN.md §11.
//
// For cell c and quantity q, over the interior (sub-)faces s of c, o the cell across, n outward from c, everything in double:
//   h = V^(1/dim);  d_s = (h_c + h_o) / 2;  w_s,a = A_s |n_s,a|
//   N_a = sum_s w_s,a (q_o - q_c) / d_s           D_a = sum_s w_s,a (|q_o - q_c| + eps (|q_o| + |q_c|)) / d_s
//   b_a = sum_s A_s n_s,a    W_a = sum_s w_s,a    k_a = W_a > 0 ? max(0, 1 - |b_a| / W_a) : 0
//   E_q = sqrt(sum_a (k_a N_a)^2) / sqrt(sum_a D_a^2)   (0 where the denominator is 0);   E = max over the quantities asked for
// Summation order: CSR order = ascending face id; inside a hanging face j-major, i-minor; a subcell's in-block faces first,
// -x +x -y +y (-z +z).
//
// No contraction into fused multiply-adds in this file: the two opposite faces of a Cartesian cell must give terms that are
// exact negatives of each other, so that a linear field leaves N_a = 0 exactly; a fused multiply-add would leave the rounding
// error of the first product behind.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "t8gpu_hip.h"

#pragma clang fp contract(off)

namespace t8gpu_hip {

template <class T>
using ind_vars_t = std::conditional_t<std::is_same<T, float>::value, T8gpuVars_f32, T8gpuVars_f64>;

constexpr unsigned IND_MASK_ALL   = 15u;       // bit 0 density, 1 pressure, 2 mach, 3 entropy
constexpr unsigned IND_MASK_STATE = 14u;       // the quantities that need all five planes

// the sums of one cell
struct IndSums {
  double N[4][3], D[4][3], b[3], W[3];
};

// V^(1/dim). cbrt may be an ulp off; one Newton step makes it exact for the volumes 2^(-3 L) of Cartesian cells (with r =
// 2^-L (1 + e), r^3 - V = 3 e V exactly and the correction is e r), so that a block's in-block face area h^2 and the sub-face
// area of its outer faces agree bit for bit.
__device__ __forceinline__ double cell_length(double v, int dim) {
  if (dim == 2) return sqrt(v);
  const double r = cbrt(v);
  return r - (r * r * r - v) / (3.0 * r * r);
}

// the quantities of cell i that `mask` asks for (fields.hip: store_pointwise); the others 0
template <class T>
__device__ __forceinline__ void load_quantities(const ind_vars_t<T>& st, size_t i, unsigned mask, double q[4]) {
  const double rho = (double)st.p[0][i];
  q[0] = rho;
  q[1] = q[2] = q[3] = 0.0;
  if (mask & IND_MASK_STATE) {
    const double mx = (double)st.p[1][i], my = (double)st.p[2][i], mz = (double)st.p[3][i], E = (double)st.p[4][i];
    const double p = 0.4 * (E - 0.5 * (mx * mx + my * my + mz * mz) / rho);
    q[1]           = p;
    if (mask & 4u) {
      const double u = mx / rho, v = my / rho, w = mz / rho;
      q[2]           = sqrt(u * u + v * v + w * w) / sqrt(1.4 * p / rho);
    }
    if (mask & 8u) q[3] = log(p) - 1.4 * log(rho);
  }
}

// one face: area A, normal n outward from c, distance d of the two cell centres
__device__ __forceinline__ void ind_term(IndSums& g, unsigned mask, double eps, double A, double nx, double ny, double nz, double d,
                                         const double qc[4], const double qo[4]) {
  const double n[3] = {nx, ny, nz};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double w  = A * fabs(n[a]);
    const double wd = w / d;
    g.b[a] += A * n[a];
    g.W[a] += w;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if ((mask >> k) & 1u) {
        const double dq = qo[k] - qc[k];
        g.N[k][a] += wd * dq;
        g.D[k][a] += wd * (fabs(dq) + eps * (fabs(qo[k]) + fabs(qc[k])));
      }
  }
}

__device__ __forceinline__ double ind_value(const IndSums& g, unsigned mask) {
  double k[3];
#pragma unroll
  for (int a = 0; a < 3; a++) k[a] = g.W[a] > 0.0 ? fmax(0.0, 1.0 - fabs(g.b[a]) / g.W[a]) : 0.0;
  double E = 0.0;
#pragma unroll
  for (int q = 0; q < 4; q++)
    if ((mask >> q) & 1u) {
      double num = 0.0, den = 0.0;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const double kn = k[a] * g.N[q][a];
        num += kn * kn;
        den += g.D[q][a] * g.D[q][a];
      }
      if (den > 0.0) E = fmax(E, sqrt(num) / sqrt(den));
    }
  return E;
}

__device__ __forceinline__ void ind_clear(IndSums& g) {
#pragma unroll
  for (int a = 0; a < 3; a++) {
    g.b[a] = g.W[a] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) g.N[k][a] = g.D[k][a] = 0.0;
  }
}

// ---- plain elements: one lane per owned element, which walks its CSR row ---------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void k_plain_indicator(int n, int ndim, int dim, unsigned mask, double eps, ind_vars_t<T> st,
                                                         const T* __restrict__ volume, const int32_t* __restrict__ fn,
                                                         const T* __restrict__ normals, const T* __restrict__ areas,
                                                         const int32_t* __restrict__ csr_off, const int32_t* __restrict__ csr_ent,
                                                         double* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  double qc[4], qo[4];
  load_quantities<T>(st, c, mask, qc);
  const double hc = cell_length((double)volume[c], dim);
  IndSums      g;
  ind_clear(g);
  const int end = csr_off[c + 1];
  for (int k = csr_off[c]; k < end; k++) {
    const int    ent  = csr_ent[k];              // 2 f + side: side 0, c is l of face f and the stored normal is outward
    const size_t f    = (size_t)(ent >> 1);
    const int    o    = fn[ent ^ 1];             // the cell across (may be a ghost slot)
    const double sign = (ent & 1) ? -1.0 : 1.0;
    const double nx   = sign * (double)normals[ndim * f];
    const double ny   = sign * (double)normals[ndim * f + 1];
    const double nz   = ndim == 3 ? sign * (double)normals[ndim * f + 2] : 0.0;
    load_quantities<T>(st, o, mask, qo);
    const double d = 0.5 * (hc + cell_length((double)volume[o], dim));
    ind_term(g, mask, eps, (double)areas[f], nx, ny, nz, d, qc, qo);
  }
  out[c] = ind_value(g, mask);
}

// ---- Subgrid blocks: one wavefront per Subgrid<4,4,4> block, four Subgrid<4,4> blocks per wavefront -------------------
// Subcell c = i + 4 j + 16 k of block e sits in lane c (2D: lane 16 * (e % 4) + c). The selected quantities are formed once
// and passed through LDS for the in-block neighbours; the subcells on the block's surface then walk the block's CSR row and
// take, from every face, the sub-faces on their own side.
//
// The sub-face map (kernels_compat.hip: sg_face_cells), for face f with unit normal +-e_a outward from block l, tangential
// axes t1 < t2 (2D: t1 only), sub-face (i, j), level difference 0 (ds = 2) or hanging (ds = 1, l the finer block):
//   l-subcell: coordinate 3 (normal +) or 0 (normal -) along a, i along t1, j along t2
//   r-subcell: face_neighbor_offset + (0 along a, ds i / 2 along t1, ds j / 2 along t2)
// Forward (the block is l): the subcell on the l side of the face owns sub-face (i, j) = its tangential coordinates.
// Inverse (the block is r): the subcell whose coordinates are offset + (0, k1, k2) owns sub-face (k1, k2) of a same-level
// face and the 2^(rank-1) sub-faces (2 k1 + {0, 1}, 2 k2 + {0, 1}) of a hanging one.
//
// No lane leaves before the block maximum is formed: the lanes of a dead block in the ragged last wavefront (2D, N % 4 != 0)
// carry E = 0 through the shuffles, which in addition stay inside their own S-lane group (width S).
template <class T, int RANK>
__global__ __launch_bounds__(64) void k_subgrid_indicator(int N, unsigned mask, double eps, ind_vars_t<T> st,
                                                          const T* __restrict__ volumes, const int32_t* __restrict__ fn,
                                                          const int32_t* __restrict__ level_diff, const int32_t* __restrict__ nb_off,
                                                          const T* __restrict__ normals, const T* __restrict__ areas,
                                                          const int32_t* __restrict__ csr_off, const int32_t* __restrict__ csr_ent,
                                                          double* __restrict__ cell_out, double* __restrict__ block_out) {
  constexpr int S   = RANK == 3 ? 64 : 16;
  constexpr int SF  = RANK == 3 ? 16 : 4;
  constexpr int EPB = 64 / S;                  // blocks per wavefront
  const int     lane = threadIdx.x;
  const int     c    = lane % S;
  const int     e    = blockIdx.x * EPB + lane / S;
  const bool    live = e < N;
  const int     eb   = live ? e : 0;
  const size_t  cell = (size_t)eb * S + c;
  double        qc[4], qo[4];
  load_quantities<T>(st, cell, mask, qc);
  __shared__ double sh[4][64];
#pragma unroll
  for (int k = 0; k < 4; k++) sh[k][lane] = qc[k];
  __syncthreads();
  double E = 0.0;
  if (live) {
    const double vol = (double)volumes[e];
    const double h   = cell_length(vol, RANK) * 0.25;       // = (vol / S)^(1 / RANK)
    const double Ain = RANK == 3 ? h * h : h;
    IndSums      g;
    ind_clear(g);
    // in-block faces: -x +x -y +y (-z +z); both cells have length h
#pragma unroll
    for (int d = 0; d < RANK; d++) {
      const int    str = 1 << (2 * d);
      const int    cd  = (c >> (2 * d)) & 3;
      const double ex = d == 0 ? 1.0 : 0.0, ey = d == 1 ? 1.0 : 0.0, ez = d == 2 ? 1.0 : 0.0;
      if (cd > 0) {
        const int j = lane - str;
#pragma unroll
        for (int k = 0; k < 4; k++) qo[k] = sh[k][j];
        ind_term(g, mask, eps, Ain, -ex, -ey, -ez, 0.5 * (h + h), qc, qo);
      }
      if (cd < 3) {
        const int j = lane + str;
#pragma unroll
        for (int k = 0; k < 4; k++) qo[k] = sh[k][j];
        ind_term(g, mask, eps, Ain, ex, ey, ez, 0.5 * (h + h), qc, qo);
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
        const int    ob    = fn[ent ^ 1];                                // the block across (may be a ghost block)
        const size_t other = (size_t)ob * S;
        const double sign  = side ? -1.0 : 1.0;
        // A sub-face is a face of a subcell of the finer block: its area from that block's VOLUME, as the in-block faces', not
        // from areas[f] / SF. On dyadic geometry the two are the same bits (cell_length); where areas and volumes are rounded
        // separately (fp32 storage of a box that is not the unit cube) only one source of lengths keeps E scale-free.
        const double ho    = cell_length((double)volumes[ob], RANK) * 0.25;
        const double hf    = fmin(h, ho);
        const double A     = RANK == 3 ? hf * hf : hf;
        const double d     = 0.5 * (h + ho);
        for (int t = 0; t < nterm; t++) {        // a hanging face from its coarse side: j-major, i-minor
          const int flat = (fixed << (2 * a)) + ((b1 + (t & 1)) << (2 * t1)) + ((b2 + (t >> 1)) << (2 * t2));
          load_quantities<T>(st, other + flat, mask, qo);
          ind_term(g, mask, eps, A, sign * nx, sign * ny, sign * nz, d, qc, qo);
        }
      }
    }
    E = ind_value(g, mask);
    if (cell_out) cell_out[cell] = E;
  }
  if (block_out) {                               // (uniform over the launch)
#pragma unroll
    for (int m = S / 2; m >= 1; m >>= 1) E = fmax(E, __shfl_xor(E, m, S));
    if (live && c == 0) block_out[e] = E;
  }
}

// ---- one buffer layer: out[e] = max(in[e], in[o] over the face neighbours o); in has n + ghosts entries -----------------
__global__ __launch_bounds__(256) void k_indicator_spread(int n, const double* __restrict__ in, const int32_t* __restrict__ fn,
                                                          const int32_t* __restrict__ csr_off, const int32_t* __restrict__ csr_ent,
                                                          double* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double    m   = in[e];
  const int end = csr_off[e + 1];
  for (int k = csr_off[e]; k < end; k++) m = fmax(m, in[fn[csr_ent[k] ^ 1]]);
  out[e] = m;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
inline bool indicator_args_ok(unsigned mask, double eps) { return mask != 0u && (mask & ~IND_MASK_ALL) == 0u && eps >= 0.0; }

template <class T>
int plain_indicator(int n, int ndim, int dim, unsigned mask, double eps, ind_vars_t<T> st, const T* volume, const int32_t* fn,
                    const T* normals, const T* areas, const int32_t* csr_off, const int32_t* csr_ent, double* out, void* stream) {
  if (n <= 0) return 0;
  if ((ndim != 2 && ndim != 3) || (dim != 2 && dim != 3) || !indicator_args_ok(mask, eps)) return static_cast<int>(hipErrorInvalidValue);
  if (!volume || !fn || !normals || !areas || !csr_off || !csr_ent || !out) return static_cast<int>(hipErrorInvalidValue);
  for (int k = 0; k < 5; k++)
    if (!st.p[k]) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL((k_plain_indicator<T>), dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), n, ndim, dim, mask,
                     eps, st, volume, fn, normals, areas, csr_off, csr_ent, out);
  return static_cast<int>(hipGetLastError());
}

template <class T>
int subgrid_indicator(int rank, int N, unsigned mask, double eps, ind_vars_t<T> st, const T* volumes, const int32_t* fn,
                      const int32_t* level_diff, const int32_t* nb_off, const T* normals, const T* areas, const int32_t* csr_off,
                      const int32_t* csr_ent, double* cell_out, double* block_out, void* stream) {
  if (N <= 0) return 0;
  if ((rank != 2 && rank != 3) || !indicator_args_ok(mask, eps)) return static_cast<int>(hipErrorInvalidValue);
  if (!volumes || !fn || !level_diff || !nb_off || !normals || !areas || !csr_off || !csr_ent) return static_cast<int>(hipErrorInvalidValue);
  for (int k = 0; k < 5; k++)
    if (!st.p[k]) return static_cast<int>(hipErrorInvalidValue);
  if (!cell_out && !block_out) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rank == 3)
    hipLaunchKernelGGL((k_subgrid_indicator<T, 3>), dim3(N), dim3(64), 0, s, N, mask, eps, st, volumes, fn, level_diff, nb_off, normals,
                       areas, csr_off, csr_ent, cell_out, block_out);
  else
    hipLaunchKernelGGL((k_subgrid_indicator<T, 2>), dim3((N + 3) / 4), dim3(64), 0, s, N, mask, eps, st, volumes, fn, level_diff, nb_off,
                       normals, areas, csr_off, csr_ent, cell_out, block_out);
  return static_cast<int>(hipGetLastError());
}

}  // namespace t8gpu_hip

extern "C" {
int t8gpu_hip_plain_indicator_f32(int num_elements, int normal_dim, int dim, unsigned quantity_mask, double filter, T8gpuVars_f32 state,
                                  const float* volume, const int32_t* face_neighbors, const float* face_normals,
                                  const float* face_surfaces, const int32_t* csr_offsets, const int32_t* csr_entries, double* out,
                                  void* stream) {
  return t8gpu_hip::plain_indicator<float>(num_elements, normal_dim, dim, quantity_mask, filter, state, volume, face_neighbors,
                                           face_normals, face_surfaces, csr_offsets, csr_entries, out, stream);
}
int t8gpu_hip_plain_indicator_f64(int num_elements, int normal_dim, int dim, unsigned quantity_mask, double filter, T8gpuVars_f64 state,
                                  const double* volume, const int32_t* face_neighbors, const double* face_normals,
                                  const double* face_surfaces, const int32_t* csr_offsets, const int32_t* csr_entries, double* out,
                                  void* stream) {
  return t8gpu_hip::plain_indicator<double>(num_elements, normal_dim, dim, quantity_mask, filter, state, volume, face_neighbors,
                                            face_normals, face_surfaces, csr_offsets, csr_entries, out, stream);
}
int t8gpu_hip_subgrid_indicator_f32(int rank, int num_blocks, unsigned quantity_mask, double filter, T8gpuVars_f32 state,
                                    const float* volumes, const int32_t* face_neighbors, const int32_t* face_level_difference,
                                    const int32_t* face_neighbor_offset, const float* face_normals, const float* face_surfaces,
                                    const int32_t* csr_offsets, const int32_t* csr_entries, double* cell_out, double* block_out,
                                    void* stream) {
  return t8gpu_hip::subgrid_indicator<float>(rank, num_blocks, quantity_mask, filter, state, volumes, face_neighbors,
                                             face_level_difference, face_neighbor_offset, face_normals, face_surfaces, csr_offsets,
                                             csr_entries, cell_out, block_out, stream);
}
int t8gpu_hip_subgrid_indicator_f64(int rank, int num_blocks, unsigned quantity_mask, double filter, T8gpuVars_f64 state,
                                    const double* volumes, const int32_t* face_neighbors, const int32_t* face_level_difference,
                                    const int32_t* face_neighbor_offset, const double* face_normals, const double* face_surfaces,
                                    const int32_t* csr_offsets, const int32_t* csr_entries, double* cell_out, double* block_out,
                                    void* stream) {
  return t8gpu_hip::subgrid_indicator<double>(rank, num_blocks, quantity_mask, filter, state, volumes, face_neighbors,
                                              face_level_difference, face_neighbor_offset, face_normals, face_surfaces, csr_offsets,
                                              csr_entries, cell_out, block_out, stream);
}
int t8gpu_hip_indicator_spread(int num_elements, const double* in, const int32_t* face_neighbors, const int32_t* csr_offsets,
                               const int32_t* csr_entries, double* out, void* stream) {
  if (num_elements <= 0) return 0;
  if (!in || !face_neighbors || !csr_offsets || !csr_entries || !out || in == out) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(t8gpu_hip::k_indicator_spread, dim3((num_elements + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                     num_elements, in, face_neighbors, csr_offsets, csr_entries, out);
  return static_cast<int>(hipGetLastError());
}
}
