// kernels_fused.hip -- fused tile kernels for plain elements (flux + RK stage in one launch).
//
// Workgroup = 256 lanes = one tile of the plan (tile_plan.cpp). Three phases, two barriers:
//   1. lanes = tile elements + halo: gather the 5 conserved values (own range coalesced, halo through
//      the sorted id list), turn them into per-element primitives, keep them in LDS;
//   2. lanes = tile faces: packed (l, r), {n, area} streamed from the tile-ordered arrays (coalesced),
//      primitives of both sides from LDS, one KEPES/HLL evaluation, area-scaled xyz flux to LDS;
//   3. lanes = owned elements: sum the element's faces from LDS in CSR order (deterministic, no
//      atomics), apply the SSP-RK3 stage, store the new state coalesced.
// HBM sees: state in, state out, previous-step state, volume and the plan arrays -- the flux planes
// never leave the chip. blockIdx -> tile is XCD-aware: blocks b, b+8, ... share an XCD (and its L2),
// so each XCD gets one contiguous run of tiles and neighbouring tiles' halos hit the same L2.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "fused_common.hpp"
#include "stage_kernel_note.hpp"

namespace t8gpu_hip {

template <class T, int KIND, int STAGE, bool OPEN = false>
__global__ __launch_bounds__(256) void k_plain_fused(T8gpuPlainPlan P, int tile_begin, FVars<T> prev, FVars<T> src,
                                                     FVars<T> out, const T* __restrict__ vol, T dt,
                                                     T* __restrict__ speed) {
  // OPEN: the plan has outflow / inflow faces (fused_common.hpp: decode_face_side); OPEN = false is the wall-only kernel
  constexpr bool FAR = false;
#include "plain_fused_body.inc"
}
// plans with far-field faces (T8gpuPlainPlan::has_farfield_faces): the OPEN body with far-field faces decoded. A kernel of its own
// name, so that the instantiations of k_plain_fused keep their symbols.
template <class T, int KIND, int STAGE>
__global__ __launch_bounds__(256) void k_plain_fused_far(T8gpuPlainPlan P, int tile_begin, FVars<T> prev, FVars<T> src,
                                                         FVars<T> out, const T* __restrict__ vol, T dt,
                                                         T* __restrict__ speed) {
  constexpr bool OPEN = true, FAR = true;
#include "plain_fused_body.inc"
}

}  // namespace t8gpu_hip

#include "fused_tile_body.hpp"  // k_plain_fused_p: the one-tile-per-workgroup kernel, shared with kernels_fused_patch.hip

namespace t8gpu_hip {


// tiles [tile_begin, tile_begin + tile_count) of tile_order, none of them a patch tile. whole_plan: the caller's launch
// covers the whole plan (what the persistent kernel is for).
template <class T, class V>
int plain_generic_stage(int kind, int stage, const T8gpuPlainPlan* plan, int tile_begin, int tile_count, V prev, V mid,
                        V out, const T* volume, T dt, T* speed, bool whole_plan, void* stream) {
  if (tile_count == 0) return 0;
  const int   nw = kind == 0 ? kPrimWords : 5;
  hipStream_t s  = static_cast<hipStream_t>(stream);
  const dim3  grid(tile_count), block(256);
  const int   slots = plan_slots(*plan);
  const bool  pipelined = plain_tiles_pipelined(plan);
  const bool  four = plan->max_faces > 512;
  // (the generic kernel walks the CSR lists; callers that know their plan stays inside the pipelined kernels' limits need not
  //  upload them -- t8gpu_amd/fused.py does not)
  if (!pipelined && (!plan->csr_off || !plan->csr_ent)) return static_cast<int>(hipErrorInvalidValue);
  const bool  open = plan->has_open_faces != 0;   // outflow / inflow faces: the OPEN instantiations
  const bool  far  = open && plan->has_farfield_faces != 0;   // far-field faces too: the _far kernels
  if (open && !plan->inflow) return static_cast<int>(hipErrorInvalidValue);
  // The persistent, software-pipelined kernel (kernels_fused_persistent.hip) for launches that cover the whole plan.
  // A multi-rank stage is split into tile classes on three streams beside the pack / RCCL / unpack kernels
  // (stepper.hip): persistent workgroups would hold every register file and LDS slot of the chip until their class is
  // done and keep those small kernels -- the exchange the split exists to overlap -- from starting, so partial
  // ranges use the one-tile-per-workgroup kernels, whose slots free up continuously. Both give the same bits.
  static const bool persistent_always = std::getenv("T8GPU_PERSISTENT") && std::getenv("T8GPU_PERSISTENT")[0] == '2';
  // (the persistent kernel knows no ghost window -- t8gpu_hip.h: such launches run one tile per workgroup)
  if ((persistent_always || whole_plan) && !plan->ghost_buf && !plan->send_map) {
    const int rc = plain_persistent_stage<T>(kind, stage, plan, tile_begin, tile_count, fmk<T>(prev), fmk<T>(mid), fmk<T>(out), volume,
                                             dt, speed, s);
    if (rc >= 0) return rc;
  }
  const size_t tab       = lds_log_table<T>(kind);
  const size_t lds_table = tab ? tab + 16 : 0;
  size_t       lds       = sizeof(T) * ((size_t)nw * slots + (size_t)5 * (pipelined ? 256 : plan->max_faces)) + lds_table;
  if (lds > 160 * 1024) return static_cast<int>(hipErrorInvalidValue);
  const bool  dict  = pipelined && plan->geo_idx && plan->geo_table && plan->n_geo > 0;
  // the DENSE register budget (fused_tile_body.hpp) for fp64 KEPES tiles of <= 36 KB with a dictionary and <= 512 faces
  // (not for far-field plans: the _far body would spill under that budget -- their tiles take the default one)
  const bool  dense = !far && dict && !four && kind == 0 && sizeof(T) == 8 && lds - lds_table <= static_cast<size_t>(36) * 1024;
  if (dense) lds -= lds_table;   // (the DENSE kernel reads the logarithm table from global memory)
  return dispatch(
      [&](auto K, auto S, auto OPEN, auto FAR, auto PIPELINED, auto DICT, auto FOUR, auto DENSE) {
        if constexpr (FAR && !OPEN) {
          return static_cast<int>(hipErrorInvalidValue);   // (never: `far` implies `open`)
        } else if constexpr (!PIPELINED && FAR) {
          note_stage_kernel<T>(tile_count, grid.x, "k_plain_fused_far", K, S);
          return launch(&k_plain_fused_far<T, K, S>, grid, block, lds, s, *plan, tile_begin, fmk<T>(prev), fmk<T>(mid), fmk<T>(out),
                        volume, dt, speed);
        } else if constexpr (!PIPELINED) {
          note_stage_kernel<T>(tile_count, grid.x, "k_plain_fused", K, S, OPEN);
          return launch(&k_plain_fused<T, K, S, OPEN>, grid, block, lds, s, *plan, tile_begin, fmk<T>(prev), fmk<T>(mid), fmk<T>(out),
                        volume, dt, speed);
        } else if constexpr (FAR) {
          constexpr int  MAXP = FOUR ? 4 : 2;
          note_stage_kernel<T>(tile_count, grid.x, "k_plain_fused_p_far", K, S, DICT, MAXP);
          return launch(&k_plain_fused_p_far<T, K, S, DICT, MAXP>, grid, block, lds, s, *plan, tile_begin, fmk<T>(prev), fmk<T>(mid),
                        fmk<T>(out), volume, dt, speed);
        } else {
          constexpr int  MAXP = FOUR ? 4 : 2;
          constexpr bool D    = DENSE && DICT && !FOUR && K == 0 && sizeof(T) == 8;   // (`dense` is never set otherwise)
          note_stage_kernel<T>(tile_count, grid.x, "k_plain_fused_p", K, S, DICT, MAXP, D, OPEN);
          return launch(&k_plain_fused_p<T, K, S, DICT, MAXP, D, OPEN>, grid, block, lds, s, *plan, tile_begin, fmk<T>(prev), fmk<T>(mid),
                        fmk<T>(out), volume, dt, speed);
        }
      },
      kind, stage, open, far, pipelined, dict, four, dense);
}

// The C-ABI entry: splits the range of tile_order into its patch tiles (kernels_fused_patch.hip) and its generic tiles
// (the kernels above / the persistent kernel). Inside every class the patch tiles come first (T8gpuPlainPlan).
template <class T, class V>
int plain_fused_stage(int kind, int stage, const T8gpuPlainPlan* plan, int tile_begin, int tile_count, V prev, V mid,
                      V out, const T* volume, T dt, T* speed, int planar, void* stream) {
  if (!plan || kind < 0 || kind > 2 || stage < 1 || stage > 3) return static_cast<int>(hipErrorInvalidValue);
  if (tile_begin < 0 || tile_count < 0 || tile_begin + tile_count > plan->ntiles) return static_cast<int>(hipErrorInvalidValue);
  if (plan->max_elems > 256 * 4) return static_cast<int>(hipErrorInvalidValue);
  // stage 1 is u1 = u0 + dt/vol f(u0) (ssp_runge_kutta.inl:30-50: `prev` is both the flux source and the summand):
  // the pipelined kernel keeps the source state in registers and never reads `prev` at stage 1, the generic kernel
  // does -- so a caller passing prev != mid at stage 1 would get variant-dependent results. Refused instead.
  if (stage == 1)
    for (int k = 0; k < 5; k++)
      if (prev.p[k] != mid.p[k]) return static_cast<int>(hipErrorInvalidValue);
  if (tile_count == 0) return 0;
  if ((plan->ghost_buf || plan->send_map) && (plan->n_owned <= 0 || (plan->send_map && !plan->send_buf))) return static_cast<int>(hipErrorInvalidValue);
  if (plan->has_open_faces && !plan->inflow) return static_cast<int>(hipErrorInvalidValue);
  stage_kernel_note_reset();
  // The interior launch of a multi-rank stage -- exactly [0, n_interior) -- is a persistent grid like a whole-plan launch. In
  // the three-stream pipeline of rounds 1-3 resident workgroups that never leave kept the exchange kernels from starting
  // (profiles/r03_halo_overhead.md); the two-lane driver queues the RCCL kernel and the ghost-reading tiles a stage ahead of
  // their deadline and they slip in at the drain between two interior launches: rank 3 of the 8-way c4 split 0.168 -> 0.153
  // ms/step (profiles/r04_halo_overhead.md).
  const bool whole = tile_begin == 0 && (tile_count == plan->ntiles || tile_count == plan->n_interior_tiles);
  const int  np_total = plan->n_patch_tiles[0] + plan->n_patch_tiles[1] + plan->n_patch_tiles[2];
  if (np_total == 0) return plain_generic_stage<T, V>(kind, stage, plan, tile_begin, tile_count, prev, mid, out, volume, dt, speed, whole, stream);
  if (!plan->tile_desc) return static_cast<int>(hipErrorInvalidValue);
  const int nd = plan->n_deep_tiles > 0 && plan->n_deep_tiles <= plan->n_interior_tiles ? plan->n_deep_tiles : 0;
  // class segments of tile_order: [0, nd) deep, [nd, n_interior) near the boundary, [n_interior, ntiles) ghost-reading.
  // (a plan whose n_deep_tiles is 0 = "unknown" has classes 0 and 1 merged: the planner then reports no class-1 patches)
  const int seg[4] = {0, nd, plan->n_interior_tiles, plan->ntiles};
  const int b = tile_begin, e = tile_begin + tile_count;
  static const bool persistent_always = std::getenv("T8GPU_PERSISTENT") && std::getenv("T8GPU_PERSISTENT")[0] == '2';
  const bool        persistent        = whole || persistent_always;   // (patch launches: persistent grids)
  // the planar form of the 2D patch body (kernels_fused_patch.hip): whole-plan launches of a plan without a ghost window and
  // without open faces (their prescribed outside state may carry a z-momentum, which the general tiles would write), KEPES
  const bool planar_ok = planar != 0 && kind == 0 && tile_begin == 0 && tile_count == plan->ntiles && plan->patch_dim != 3 &&
                         !plan->ghost_buf && !plan->send_map && !plan->has_open_faces && !plan->has_farfield_faces;
  const hipStream_t s                 = static_cast<hipStream_t>(stream);
  // generic sub-ranges that touch are launched together (single rank: one patch launch + one generic launch)
  int gb = -1, ge = -1;
  auto flush = [&]() -> int {
    if (gb < 0 || ge <= gb) return 0;
    const int rc = plain_generic_stage<T, V>(kind, stage, plan, gb, ge - gb, prev, mid, out, volume, dt, speed, whole, stream);
    gb = ge = -1;
    return rc;
  };
  for (int c = 0; c < 3; c++) {
    const int s0 = seg[c], s1 = seg[c + 1], p1 = s0 + plan->n_patch_tiles[c];
    if (p1 > s1) return static_cast<int>(hipErrorInvalidValue);
    const int pb = b > s0 ? b : s0, pe = e < p1 ? e : p1;   // patch tiles of this class inside the range
    int       qb = b > p1 ? b : p1, qe = e < s1 ? e : s1;   // its generic tiles
    if (pe > pb && plan->patch_dim == 3) {   // 8 x 8 x 4 hexahedral patches: their own kernel, the generic tiles apart
      if (plan->ghost_buf || plan->send_map) return static_cast<int>(hipErrorInvalidValue);   // (no ghost window in k_plain_patch3)
      if (int rc = flush()) return rc;
      // (Measured and dropped: the generic tiles on a side stream forked from / joined to the caller's stream by events, so
      //  that they run BESIDE the patches -- c5 5 235 -> 5 078, c5u 5 070 -> 4 716 M/s: the fork / join events cost more than
      //  the overlap returns, as with the Subgrid leftover blocks of round 2.)
      // (the class's patch tiles are [regular | irregular]: one launch each)
      const int ni = plan->n_irregular_tiles[c];
      if (ni < 0 || ni > plan->n_patch_tiles[c]) return static_cast<int>(hipErrorInvalidValue);
      const int i0 = p1 - ni;   // first irregular patch of the class
      const int rb = pb, re = pe < i0 ? pe : i0, ib = pb > i0 ? pb : i0, ie = pe;
      const int both = re > rb && ie > ib && persistent   // both kinds in one launch (kernels_fused_patch3.hip; -1: not taken)
                           ? plain_patch3_both_stage<T>(kind, stage, plan, rb, re - rb, ib, ie - ib, fmk<T>(prev), fmk<T>(mid), fmk<T>(out),
                                                        volume, dt, speed, s)
                           : -1;
      if (both > 0) return both;
      if (both < 0) {
        if (re > rb)
          if (int rc = plain_patch3_stage<T>(kind, stage, plan, rb, re - rb, fmk<T>(prev), fmk<T>(mid), fmk<T>(out), volume, dt, speed,
                                             persistent, false, s))
            return rc;
        if (ie > ib)
          if (int rc = plain_patch3_stage<T>(kind, stage, plan, ib, ie - ib, fmk<T>(prev), fmk<T>(mid), fmk<T>(out), volume, dt, speed,
                                             persistent, true, s))
            return rc;
      }
    } else if (pe > pb) {
      if (int rc = flush()) return rc;
      // patches and generic tiles of the class in ONE launch where the patches carry most of it (the generic tiles then
      // run the one-tile body behind the persistent patch workgroups); otherwise the generic tiles keep their own launch
      // (the persistent tile kernel where the range covers the plan)
      const bool mixed = qe > qb && static_cast<long long>(pe - pb) * 256 >= static_cast<long long>(qe - qb) * 128;
      int rc = plain_patch_stage<T>(kind, stage, plan, pb, pe - pb, qb, mixed ? qe - qb : 0, fmk<T>(prev), fmk<T>(mid), fmk<T>(out), volume,
                                    dt, speed, persistent, planar_ok, s);
      if (rc == -1)   // (the mixed kernel does not take this plan's generic tiles)
        rc = plain_patch_stage<T>(kind, stage, plan, pb, pe - pb, qb, 0, fmk<T>(prev), fmk<T>(mid), fmk<T>(out), volume, dt, speed,
                                  persistent, planar_ok, s);
      else if (rc == 0 && mixed)
        qe = qb;   // done
      if (rc != 0) return rc;
    }
    if (qe > qb) {
      if (gb >= 0 && ge == qb) {
        ge = qe;
      } else {
        if (int rc = flush()) return rc;
        gb = qb;
        ge = qe;
      }
    }
  }
  return flush();
}

}  // namespace t8gpu_hip

namespace t8gpu_hip {
template <class T>
__global__ __launch_bounds__(128) void k_geo_frames(T* __restrict__ table, int n_geo) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_geo) return;
  T* const row  = table + 12 * static_cast<size_t>(i);
  const T  n[3] = {row[0], row[1], row[2]};
  T        t1[3], t2[3];
  face_basis_fast<T>(n, t1, t2);
  for (int k = 0; k < 3; k++) {
    row[4 + k] = t1[k];
    row[8 + k] = t2[k];
  }
}
template <class T>
int geo_frames(void* table, int n_geo, void* stream) {
  if (n_geo < 0 || (n_geo > 0 && !table)) return static_cast<int>(hipErrorInvalidValue);
  if (n_geo == 0) return 0;
  hipLaunchKernelGGL((k_geo_frames<T>), dim3((n_geo + 127) / 128), dim3(128), 0, static_cast<hipStream_t>(stream), static_cast<T*>(table), n_geo);
  return static_cast<int>(hipGetLastError());
}
}  // namespace t8gpu_hip

namespace t8gpu_hip {
// inflow table entries (t8gpu_hip.h: T8GPU_INFLOW_WORDS): the state and its KEPES record by the routine the tile kernels run
// for their cells (fp64: table-driven logarithms, the table read from global memory -- the same values as the LDS copy)
template <class T>
__global__ __launch_bounds__(64) void k_inflow_table(const T* __restrict__ states, int n, T* __restrict__ table) {
  const int i = threadIdx.x;
  if (i >= n) return;
  T s[5];
  for (int k = 0; k < 5; k++) s[k] = states[5 * i + k];
  const Prim<T> q = prim_from_state<T, sizeof(T) == 8>(s, kLogTab);
  T* const      w = table + T8GPU_INFLOW_WORDS * i;
  for (int k = 0; k < 5; k++) w[k] = s[k];
  w[5] = q.rho; w[6] = q.vx; w[7] = q.vy; w[8] = q.vz; w[9] = q.p; w[10] = q.beta; w[11] = q.lrho; w[12] = q.lbeta; w[13] = q.v0;
  w[14] = T(0);
  w[15] = T(0);
}
template <class T>
int inflow_table(const T* states, int n, T* table, void* stream) {
  if (n < 0 || n > 8 || (n > 0 && (!states || !table))) return static_cast<int>(hipErrorInvalidValue);
  if (n == 0) return 0;
  hipLaunchKernelGGL((k_inflow_table<T>), dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), states, n, table);
  return static_cast<int>(hipGetLastError());
}
}  // namespace t8gpu_hip

extern "C" {
int t8gpu_hip_plain_inflow_table_f32(const float* states, int n, float* table, void* stream) { return t8gpu_hip::inflow_table<float>(states, n, table, stream); }
int t8gpu_hip_plain_inflow_table_f64(const double* states, int n, double* table, void* stream) { return t8gpu_hip::inflow_table<double>(states, n, table, stream); }
int t8gpu_hip_plain_geo_frames_f32(void* geo_table, int n_geo, void* stream) { return t8gpu_hip::geo_frames<float>(geo_table, n_geo, stream); }
int t8gpu_hip_plain_geo_frames_f64(void* geo_table, int n_geo, void* stream) { return t8gpu_hip::geo_frames<double>(geo_table, n_geo, stream); }
int t8gpu_hip_plain_needs_csr(const T8gpuPlainPlan* plan) { return plan && t8gpu_hip::plain_tiles_pipelined(plan) ? 0 : 1; }
int t8gpu_hip_plain_fused_stage_f32(int kind, int stage, const T8gpuPlainPlan* plan, int tile_begin, int tile_count,
                                    T8gpuVars_f32 prev, T8gpuVars_f32 mid, T8gpuVars_f32 out, const float* volume,
                                    float dt, float* speed, void* stream) {
  return t8gpu_hip::plain_fused_stage<float>(kind, stage, plan, tile_begin, tile_count, prev, mid, out, volume, dt,
                                             speed, 0, stream);
}
int t8gpu_hip_plain_fused_stage_f64(int kind, int stage, const T8gpuPlainPlan* plan, int tile_begin, int tile_count,
                                    T8gpuVars_f64 prev, T8gpuVars_f64 mid, T8gpuVars_f64 out, const double* volume,
                                    double dt, double* speed, void* stream) {
  return t8gpu_hip::plain_fused_stage<double>(kind, stage, plan, tile_begin, tile_count, prev, mid, out, volume, dt,
                                              speed, 0, stream);
}
int t8gpu_hip_plain_fused_stage_planar_f32(int kind, int stage, const T8gpuPlainPlan* plan, int tile_begin, int tile_count,
                                           T8gpuVars_f32 prev, T8gpuVars_f32 mid, T8gpuVars_f32 out, const float* volume,
                                           float dt, float* speed, void* stream, int planar) {
  return t8gpu_hip::plain_fused_stage<float>(kind, stage, plan, tile_begin, tile_count, prev, mid, out, volume, dt,
                                             speed, planar, stream);
}
int t8gpu_hip_plain_fused_stage_planar_f64(int kind, int stage, const T8gpuPlainPlan* plan, int tile_begin, int tile_count,
                                           T8gpuVars_f64 prev, T8gpuVars_f64 mid, T8gpuVars_f64 out, const double* volume,
                                           double dt, double* speed, void* stream, int planar) {
  return t8gpu_hip::plain_fused_stage<double>(kind, stage, plan, tile_begin, tile_count, prev, mid, out, volume, dt,
                                              speed, planar, stream);
}
}
