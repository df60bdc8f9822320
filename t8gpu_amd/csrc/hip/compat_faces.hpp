// compat_faces.hpp -- the boundary face of the reference-dataflow tier, stated once: the outside state of a face of kind k, the
// face-frame flux the face carries, and the sub-face -> subcell map of a block face. Shared by the stage kernels of
// kernels_compat.hip and the boundary budgets of kernels_boundary.hip, so that both do the same arithmetic by construction.
//
// ROUNDING-SENSITIVE: the code here is the reference's rounding sequence. Only translation units that switch contraction off
// (`#pragma clang fp contract(off)` before their includes) may include it -- those two files and no other. The fused tiers
// have routines of their own (fused_tile_body.hpp, kernels_subgrid_fused.hip).
#ifndef T8GPU_HIP_COMPAT_FACES_HPP
#define T8GPU_HIP_COMPAT_FACES_HPP

#include "flux_math.hpp"
#include "fused_common.hpp"
#include "t8gpu_hip.h"
#include "t8gpu_host.h"

namespace t8gpu_hip {

// The outside state o of a boundary face of kind `kind` with outward normal n and inside state s (t8gpu_host.h: T8GPU_BOUNDARY_*,
// t8gpu_hip.h: T8GPU_INFLOW_WORDS): wall (0, which the flux mirrors) and outflow (1) keep the inside state, inflow 2 + k takes the
// conservative state of table row k (words 0-4), far field 10 + k the characteristic state against row k
// (fused_common.hpp: farfield_state). FAR = false: kinds below 10 only.
template <class T, bool FAR>
T8_DEV void boundary_outside_state(int kind, const T* __restrict__ inflow, const T n[3], const T s[5], T o[5]) {
#pragma unroll
  for (int k = 0; k < 5; k++) o[k] = s[k];
  if (FAR && kind >= T8GPU_BOUNDARY_FARFIELD) {
    farfield_state<T>(inflow + T8GPU_INFLOW_WORDS * (kind - T8GPU_BOUNDARY_FARFIELD), n, o);
  } else if (kind >= 2) {
#pragma unroll
    for (int k = 0; k < 5; k++) o[k] = inflow[T8GPU_INFLOW_WORDS * (kind - 2) + k];
  }
}

// The face-frame flux Ff (per unit area) and speed estimate of a boundary face: builds the frame (t1, t2, left to the caller),
// forms the outside state and evaluates the flux. It stops there on purpose -- what follows differs between the callers, each
// as its reference kernel has it: the plain kernel scales Ff by the area and then rotates back, the Subgrid kernels rotate and
// then multiply by areas / SF, the budgets rotate the unit flux and multiply in double.
template <class T, int KIND, bool FAR>
T8_DEV void boundary_face_flux(const T n[3], const T s[5], int kind, const T* __restrict__ inflow, T t1[3], T t2[3], T Ff[5],
                               T& spd) {
  T o[5];
  face_basis<T>(n, t1, t2);
  boundary_outside_state<T, FAR>(kind, inflow, n, s, o);
  face_frame_flux_ref<T, KIND>(n, t1, t2, s, o, kind == 0, Ff, spd);
}

// sub-face -> cell map of compute_outer_fluxes, kernels.inl:710-758 / 837-866 (exact +-1.0 compares). The left half: the
// inside subcell (flat index in its block) of sub-face (i, j) of a block face with normal n; si / sj = the axes i and j run along.
template <class T, int RANK>
T8_DEV int sg_inside_cell(const T n[3], int i, int j, int si[3], int sj[3]) {
  int al[3] = {0, 0, 0};
#pragma unroll
  for (int d = 0; d < 3; d++) si[d] = sj[d] = 0;
  if (RANK == 3) {
    if (n[0] == T(1.0)) { al[0] = 3; si[1] = 1; sj[2] = 1; }
    if (n[0] == T(-1.0)) { si[1] = 1; sj[2] = 1; }
    if (n[1] == T(1.0)) { al[1] = 3; si[0] = 1; sj[2] = 1; }
    if (n[1] == T(-1.0)) { si[0] = 1; sj[2] = 1; }
    if (n[2] == T(1.0)) { al[2] = 3; si[0] = 1; sj[1] = 1; }
    if (n[2] == T(-1.0)) { si[0] = 1; sj[1] = 1; }
  } else {
    if (n[0] == T(1.0)) { al[0] = 3; si[1] = 1; }
    if (n[0] == T(-1.0)) { si[1] = 1; }
    if (n[1] == T(1.0)) { al[1] = 3; si[0] = 1; }
    if (n[1] == T(-1.0)) { si[0] = 1; }
  }
  int lc[3];
#pragma unroll
  for (int d = 0; d < 3; d++) lc[d] = al[d] + i * si[d] + j * sj[d];
  return lc[0] + 4 * lc[1] + 16 * lc[2];
}
// both halves: the right subcell lies at `off` in the neighbour block, two sub-faces per cell where the neighbour is coarser
template <class T, int RANK>
T8_DEV void sg_face_cells(const T n[3], const int off[3], int ds, int i, int j, int& lflat, int& rflat) {
  int si[3], sj[3], rc[3];
  lflat = sg_inside_cell<T, RANK>(n, i, j, si, sj);
#pragma unroll
  for (int d = 0; d < 3; d++) rc[d] = off[d] + ds * (i * si[d] + j * sj[d]) / 2;
  rflat = rc[0] + 4 * rc[1] + 16 * rc[2];
}

}  // namespace t8gpu_hip

#endif
