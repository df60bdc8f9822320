// kernels_fused_patch.hip -- fused RK stage over STRUCTURED PATCHES of a plain-element mesh (round 3).
//
// Reference: examples/compressible_euler/kernels.cu:135-309 (kepes_compute_fluxes) + ssp_runge_kutta.inl:30-99, the same
// stage the tile kernels fuse (kernels_fused.hip, kernels_fused_persistent.hip).
//
// Adaptive quadrilateral meshes are locally structured: on the benchmark mesh (c4) 97 % of the elements lie in aligned
// 16 x 16 blocks of same-size squares, which are 256 CONSECUTIVE elements in Morton order. The host plan finds such
// patches from the reference-format arrays alone (csrc/host/tile_plan.cpp: find_patches) and hands them over as tiles
// WITHOUT face records. For those tiles everything the generic tile kernels fetch per face -- packed (l, r) indices,
// geometry index, original face id, the per-element face list -- follows from the lane index:
//
//   lane t = element e0 + t = cell (i, j) of the patch (t = Morton interleave of i and j, x in bit 0)
//   phase 1   primitives of the own cell -> registers and an LDS record; wave 3 also takes the 64 cells across the
//             patch's four sides (the plan lists them per patch: [-x | +x | -y | +y] x 16)
//   phase 2   the lane's OWN faces: +x against cell (i + 1, j), +y against (i, j + 1) (normals exactly +e_x, +e_y: no
//             rotation, no dictionary; left operand in registers); lanes 0-31 of wave 0 evaluate the 32 faces of the
//             -x / -y sides, which belong to the cells across (same orientation, same values as in their own tile)
//   phase 3   a cell adds its four fluxes in ascending original face id, which for a patch is: the -x and -y faces in
//             the order of the owning neighbours' indices (a function of (i, j), checked by the planner), then +x, +y;
//             RK stage
//
// Per 256 elements that is 5 + 9 wave-rounds of primitives / fluxes (the tile kernels: 8 + 8 for 234) and a quarter of
// the index traffic; speed estimates go to fbase + 2 t (+1) without an id list. Same flux functions, same operand order,
// same summation order as the tile kernels: results are bitwise theirs (tests/test_gpu_patch.py), and a face that a patch
// and a generic tile both evaluate gets the same value in both.
//
// Persistent and software-pipelined like k_plain_persistent: a workgroup walks patches j, j + n, ... of its XCD's
// contiguous share with the next patch's loads in flight; two barriers per patch.
#include "fused_common.hpp"
#include "fused_tile_body.hpp"
#include "patch_common.hpp"
#include "stage_kernel_note.hpp"

namespace t8gpu_hip {

// workgroup `wg` of the `nwg` that share the patch tiles [tile_begin, tile_begin + tile_count) of tile_order
// chunk = 0: persistent walk -- the XCD's workgroups stride through its share together (tiles j, j + n, ...); chunk = c > 0:
// workgroup j of the XCD takes the c CONSECUTIVE tiles [j c, j c + c) of the share and leaves (a grid of ~count / c
// workgroups that the hardware hands out as slots free up: what a launch beside other kernels wants, see plain_patch_stage)
//
// PLANAR (KEPES only): the launch's contract is that the z-momentum planes of `prev` and `src` are all +0 over the slots it reads
// and that of `out` is +0 already over the slots it writes (2D meshes; the native stepper proves it per call, stepper.hip). The
// body then carries four variables: no load of src.p[3] / prev.p[3] (own cells, side cells, prefetch), no store to out.p[3], no
// vz word in the LDS records, four flux planes in ff, no z primitive and no z RK update -- and stores the bits the general form
// stores (flux_math.hpp: kepes_core_planar has the argument term by term). FINITE states only: an infinity or NaN in another
// variable would reach the z plane in the general form and does not here.
// PLANAR in fp64 (SPLIT below) is built for FOUR workgroups per CU: a register budget of 128 VGPRs, which the patch body
// meets without a spill (113 / 123 / 123 in stages 1 / 2 / 3), 64-byte LDS records in chunk planes (fused_common.hpp: 39 936 bytes
// per workgroup against 45 056 with the padded records) and the state planes addressed as base + k x spacing.
template <class T, int KIND, int STAGE, bool NT, bool PLANAR = false>
T8_DEV void plain_patch_body(const T8gpuPlainPlan& P, int tile_begin, int tile_count, int wg, int nwg, int chunk, const FVars<T>& prev,
                             const FVars<T>& src, const FVars<T>& out, const T* __restrict__ vol, T dt, T* __restrict__ speed) {
  static_assert(!PLANAR || KIND == 0, "the planar form exists for KEPES");
  constexpr int NV  = PLANAR ? 4 : 5;                              // variables carried; variable c lives in plane pl(c)
  constexpr int NW  = KIND == 0 ? (PLANAR ? kPrimWordsPlanar : kPrimWords) : 5;
  constexpr bool SPLIT = PLANAR && sizeof(T) == 8;                   // 64-byte records in four chunk planes (fused_common.hpp)
  constexpr int  REC = SPLIT ? kPrimWordsPlanar : rec_words<T, NW>();
  auto pl = [](int c) { return PLANAR && c == 3 ? 4 : c; };
  extern __shared__ __attribute__((aligned(16))) double lds_raw[];
  T* const  ff = reinterpret_cast<T*>(lds_raw);               // [NV][kPatchFF] the patch's face fluxes
  T* const  pe = ff + NV * kPatchFF;                          // [320][REC] primitives (or states): 256 own, 64 across the sides
  constexpr bool kTab = sizeof(T) == 8 && KIND == 0;          // fp64 KEPES: the logarithm table, behind the records
  double* const lt = reinterpret_cast<double*>(pe + REC * 320);
  const int tid = threadIdx.x;
  // a record is named by its handle: the word offset of record r, or (SPLIT) the byte offset of its first chunk
  auto rec_at = [](int r) { return SPLIT ? kSplitChunkBytes * r : r * REC; };
  auto store_rec = [&](int h, const T* w) {
    if constexpr (SPLIT)
      rec_split_store<320>(reinterpret_cast<double*>(pe), h, reinterpret_cast<const double*>(w));
    else
      rec_store<T, NW>(pe + h, w);
  };
  auto load_rec = [&](int h, T* w) {
    if constexpr (SPLIT)
      rec_split_load<320>(reinterpret_cast<const double*>(pe), h, reinterpret_cast<double*>(w));
    else
      rec_load<T, NW>(pe + h, w);
  };

  // Plane k of a state. SPLIT: the launch's contract is that the planes of prev, src and out are EQUALLY SPACED, all by the
  // spacing of src (plain_patch_stage checks it; the step drivers' planes are rows of one array): a plane is p[0] + k x spacing,
  // two scalar instructions where it is used, instead of twelve pointers held in scalar registers through the loop -- with them
  // the stage kernel's loop reloaded 60 - 114 spilled scalars per patch (v_readlane: VALU work). The spacing is made opaque once
  // per iteration, so that the plane addresses are not hoisted out of the loop into as many register pairs again. (Measured on
  // c4, ms per step: pointers 0.681, this 0.666; each address opaque where it is formed -- scalar adds, but more scalar spills
  // in stages 2 and 3 -- 0.679.)
  using GT = __attribute__((address_space(1))) T;
  long pstride = 0;
  if constexpr (SPLIT) pstride = reinterpret_cast<const char*>(src.p[1]) - reinterpret_cast<const char*>(src.p[0]);
  auto plane = [&](const FVars<T>& v, int k) -> T* {
    if constexpr (SPLIT) {
      uintptr_t a = reinterpret_cast<uintptr_t>(v.p[0]) + static_cast<uintptr_t>(pl(k) * pstride);
      return (T*)reinterpret_cast<GT*>(a);
    } else {
      return v.p[pl(k)];
    }
  };

  // this workgroup's patches (same walk as k_plain_persistent: XCD x takes one contiguous eighth of the range, its
  // workgroups walk it together)
  const int G = nwg, xcd = wg & 7, jw = wg >> 3;
  const int nxcd = G < 8 ? G : 8, nx = (G - xcd + 7) >> 3;
  const int per = tile_count / nxcd, rem = tile_count % nxcd;
  const int x0   = tile_begin + xcd * per + (xcd < rem ? xcd : rem);
  int       tend = x0 + per + (xcd < rem ? 1 : 0);
  int       t    = x0 + (chunk > 0 ? jw * chunk : jw);
  if (chunk > 0 && t + chunk < tend) tend = t + chunk;
  if (xcd >= nxcd || t >= tend) return;
  if (kTab) {
    lt[tid] = kLogTab[tid];
    __syncthreads();
  }

  // ---- lane constants -------------------------------------------------------------------------------------------------
  int ci = 0, cj = 0;
#pragma unroll
  for (int b = 0; b < 4; b++) {
    ci |= ((tid >> (2 * b)) & 1) << b;
    cj |= ((tid >> (2 * b + 1)) & 1) << b;
  }
  // records of the right operands of the lane's faces; flux slots of its - faces (the + faces of the cells across)
  const int  rx   = rec_at(ci < 15 ? patch_morton(ci + 1, cj) : 272 + cj);
  const int  ry   = rec_at(cj < 15 ? patch_morton(ci, cj + 1) : 304 + ci);
  const int  rme  = rec_at(tid);
  const int  a_mx = ci > 0 ? patch_morton(ci - 1, cj) : 512 + cj;
  const int  a_my = cj > 0 ? 256 + patch_morton(ci, cj - 1) : 528 + ci;
  const bool yfirst_lane = patch_ctz4(cj) >= patch_ctz4(ci);   // (cell (0, 0): per patch, from the descriptor)
  // The two extra jobs of a patch -- the 64 cells across the sides (one round of primitives) and the 32 faces of the - sides
  // (one half-filled flux round) -- ROTATE over the four wavefronts from patch to patch: wavefront w has role (w + it) & 3 at
  // the workgroup's it-th patch, role 3 takes the side cells, role 0 the - faces. Fixed to wavefronts 3 and 0 (round 3) the
  // wavefronts of a workgroup carry 730 / 520 / 520 / 620 VALU instructions per patch, and a workgroup's wavefront i runs on
  // SIMD i of its CU: one SIMD of four does 22 % more than the average while the others wait at the barriers.
  // Measured (same box, against an experiment build with the fixed assignment, since removed): c4 fp64 11 640 -> 11 727 M/s,
  // fp32 and c2 unchanged -- the dispatcher does not pin wavefront i to SIMD i as strictly as feared.
  const int  wv = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63;
  auto role = [&](int it) { return (wv + it) & 3; };
  const int  hl      = ln;                                     // side-cell lane: cell hl of [-x | +x | -y | +y] x 16
  const bool minus_y = ln >= 16;                               // - face lanes 0-31 of the role-0 wavefront: -x side, then -y side
  const int  m_l = rec_at(256 + (minus_y ? 32 : 0) + (ln & 15));   // left operand: the cell across; right: the patch's cell
  const int  m_r = rec_at(minus_y ? patch_morton(ln & 15, 0) : patch_morton(0, ln & 15));

  typedef int int8v __attribute__((ext_vector_type(8)));
  struct Desc {
    int    e0, h0, fbase, flags;
    double area, vol;   // vol: the patch's uniform element volume where flags has 0x400 (tile_plan.cpp), else unused
  };
  auto load_desc = [&](int tt) {   // scalar load through the constant address space (see k_plain_persistent)
    const size_t k = static_cast<size_t>(tt < tend ? tt : tend - 1);
    const int8v  r = *reinterpret_cast<const __attribute__((address_space(4))) int8v*>(
        reinterpret_cast<const __attribute__((address_space(4))) char*>(reinterpret_cast<uintptr_t>(P.tile_desc)) + 32 * k);
    Desc d;
    d.e0 = r[0]; d.h0 = r[2]; d.fbase = r[4]; d.flags = r[5];
    d.area = __hiloint2double(r[7], r[6]);
    d.vol  = __hiloint2double(r[3], r[1]);
    return d;
  };
  struct Pre {
    T s0[NV], sh[NV];
  };
  // first: the prologue's request. A launch with a ghost window (t8gpu_hip.h; the multi-rank driver's ghost-reading class)
  // runs one patch per workgroup -- plain_patch_stage() sees to it -- so only that request can meet a ghost slot.
  auto prefetch = [&](const Desc& d, int hslot, bool first, bool halo_wave) {
    Pre p;
#pragma unroll
    for (int k = 0; k < NV; k++) p.s0[k] = at32<T>(plane(src, k), static_cast<unsigned>(d.e0 + tid));
    if (!PLANAR && halo_wave && first && P.ghost_buf) {   // (a planar launch has no ghost window: plain_patch_stage)
#pragma unroll
      for (int k = 0; k < NV; k++) p.sh[k] = ghost_window_load<T>(P, src, hslot, pl(k));
    } else if (halo_wave) {
#pragma unroll
      for (int k = 0; k < NV; k++) p.sh[k] = at32<T>(plane(src, k), static_cast<unsigned>(hslot));
    } else {
#pragma unroll
      for (int k = 0; k < NV; k++) p.sh[k] = T(0);
    }
    return p;
  };

  const int stride = chunk > 0 ? 1 : nx;
  Desc      d0 = load_desc(t), d1 = load_desc(t + stride);
  int       hs_a = role(0) == 3 ? P.halo_ids[d0.h0 + hl] : 0, hs_b = role(1) == 3 ? P.halo_ids[d1.h0 + hl] : 0;
  Pre       cur = prefetch(d0, hs_a, true, role(0) == 3);
  int       it  = 0;
  T         res[NV];
#pragma unroll
  for (int k = 0; k < NV; k++) res[k] = T(0);
  int       res_e  = -1;
  __builtin_amdgcn_s_waitcnt(0);   // (see k_plain_persistent: the prologue's loads must not become a wait inside the loop)

  for (; t < tend; t += stride, it++) {
    if constexpr (SPLIT) asm volatile("" : "+s"(pstride));
    const bool halo_wave = role(it) == 3, minus_lane = role(it) == 0 && ln < 32;
    const Desc d2   = load_desc(t + 2 * stride);
    const int  hs_c = role(it + 2) == 3 ? P.halo_ids[d2.h0 + hl] : 0;
    Pre        nxt;
    if (t + stride < tend) nxt = prefetch(d1, hs_b, false, role(it + 1) == 3);
    const int e = d0.e0 + tid;
    T         pv[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) pv[k] = T(0);
    if (STAGE > 1) {
#pragma unroll
      for (int k = 0; k < NV; k++) pv[k] = stream_load<NT>(&at32<T>(plane(prev, k), static_cast<unsigned>(e)));
    }
    // (patches of uniform volume carry it in their descriptor: 8 of ~130 bytes per element and stage less to load)
    const T volume = (d0.flags & 0x400) ? static_cast<T>(d0.vol) : at32<T>(vol, static_cast<unsigned>(e));
    const T area   = static_cast<T>(d0.area);

    // ---- phase 1: records of the own cell and (wave 3) of the cells across the sides ----------------------------------
    T mine[NW];
    if constexpr (PLANAR) {
      prim_words_planar<T>(cur.s0, mine, lt);
    } else if constexpr (KIND == 0) {
      prim_words<T>(cur.s0, mine, lt);
    } else {
#pragma unroll
      for (int k = 0; k < 5; k++) mine[k] = cur.s0[k];
    }
    store_rec(rme, mine);
    if (halo_wave) {
      T w[NW];
      if constexpr (PLANAR) {
        prim_words_planar<T>(cur.sh, w, lt);
      } else if constexpr (KIND == 0) {
        prim_words<T>(cur.sh, w, lt);
      } else {
#pragma unroll
        for (int k = 0; k < 5; k++) w[k] = cur.sh[k];
      }
      store_rec(rec_at(256 + hl), w);
    }
    if (res_e >= 0) {   // results of the previous patch: behind this iteration's first wait (vmcnt retires in order)
#pragma unroll
      for (int k = 0; k < NV; k++) stream_store<NT>(&at32<T>(plane(out, k), static_cast<unsigned>(res_e)), res[k]);
    }
    __syncthreads();

    // ---- phase 2: the lane's +x and +y faces; the - sides ------------------------------------------------------------
    auto face = [&](bool y, const T* wl, const T* wr, T* g, T& spd) {
      if constexpr (PLANAR)
        patch_face_planar<T>(y, wl, wr, area, g, spd);
      else
        patch_face<T, KIND, NW>(y, wl, wr, area, g, spd);
    };
    T gy[NV];
    {
      T wr[NW], g[NV], sx, sy;
      load_rec(rx, wr);
      face(false, mine, wr, g, sx);
#pragma unroll
      for (int k = 0; k < NV; k++) ff[k * kPatchFF + tid] = g[k];
      load_rec(ry, wr);
      face(true, mine, wr, gy, sy);
#pragma unroll
      for (int k = 0; k < NV; k++) ff[k * kPatchFF + 256 + tid] = gy[k];
      if (speed) {   // the patch's own faces: ids fbase + 2 t (+x) and fbase + 2 t + 1 (+y): one 16-byte store where aligned
        T* const sp = speed + d0.fbase + 2 * tid;
        if ((d0.fbase & 1) == 0 || sizeof(T) == 4) {   // (wave-uniform; fp32: an 8-byte store is aligned for every fbase)
          using V2 = typename vec2<T>::type;
          V2 v;
          v.x = sx;
          v.y = sy;
          *reinterpret_cast<V2*>(sp) = v;
        } else {
          sp[0] = sx;
          sp[1] = sy;
        }
      }
    }
    if (minus_lane) {
      T wl[NW], wr[NW], g[NV], sm;
      load_rec(m_l, wl);
      load_rec(m_r, wr);
      face(minus_y, wl, wr, g, sm);
#pragma unroll
      for (int k = 0; k < NV; k++) ff[k * kPatchFF + 512 + ln] = g[k];
    }
    __syncthreads();

    // ---- phase 3: the four fluxes in ascending face id, RK stage -------------------------------------------------------
    const bool yfirst = tid == 0 ? (d0.flags & 1) != 0 : yfirst_lane;
    const int  a1 = yfirst ? a_my : a_mx, a2 = yfirst ? a_mx : a_my;
    T          acc[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) {
      acc[k] = __builtin_fma(T(1), ff[k * kPatchFF + a1], T(0));
      acc[k] = __builtin_fma(T(1), ff[k * kPatchFF + a2], acc[k]);
      acc[k] = __builtin_fma(T(-1), ff[k * kPatchFF + tid], acc[k]);
      acc[k] = __builtin_fma(T(-1), gy[k], acc[k]);
    }
    // (a patch of uniform volume: its operands are wave-uniform -- the power-of-two test runs on scalar registers)
    const T scale = (d0.flags & 0x400) ? rk_scale(dt, static_cast<T>(d0.vol)) : dt / volume;
#pragma unroll
    for (int k = 0; k < NV; k++) res[k] = rk_stage_update<T, STAGE>(pv[k], cur.s0[k], scale, acc[k]);
    res_e = e;

    cur  = nxt;
    d0   = d1;
    d1   = d2;
    hs_b = hs_c;
  }
  if (res_e >= 0) {
#pragma unroll
    for (int k = 0; k < NV; k++) stream_store<NT>(&at32<T>(plane(out, k), static_cast<unsigned>(res_e)), res[k]);
    if constexpr (!PLANAR)
      if (P.send_map) ghost_window_send<T>(P, res_e, res);   // (one patch per workgroup there: this is its only store)
  }
}

// (second launch bound = waves per SIMD the register allocation must allow: 3 workgroups per CU in fp64, 5 in fp32 -- and 4 in
//  the planar fp64 form, whose body needs 113 / 123 / 123 VGPRs in stages 1 / 2 / 3 and whose LDS window is below a quarter CU's)
template <class T, bool PLANAR>
constexpr int patch_wgs_per_cu() {
  return sizeof(T) == 8 ? (PLANAR ? 4 : 3) : 5;
}

template <class T, int KIND, int STAGE, bool NT, bool PLANAR = false>
__global__ __launch_bounds__(256, (patch_wgs_per_cu<T, PLANAR>())) void k_plain_patch(T8gpuPlainPlan P, int tile_begin, int tile_count, int chunk, FVars<T> prev,
                                                                                FVars<T> src, FVars<T> out, const T* __restrict__ vol, T dt,
                                                                                T* __restrict__ speed) {
  plain_patch_body<T, KIND, STAGE, NT, PLANAR>(P, tile_begin, tile_count, blockIdx.x, gridDim.x, chunk, prev, src, out, vol, dt, speed);
}

// ONE launch per stage for a range of tile_order that holds patch tiles AND generic tiles: the first `patch_wgs`
// workgroups walk the patch tiles, every further workgroup takes one generic tile (fused_tile_body.hpp). As two launches
// the generic tiles of the benchmark mesh -- 3 % of its elements -- cost 9 % of the stage: a launch of their own, started
// when the patch launch has drained. Here they start as the persistent patch workgroups finish and fill the ragged end.
// OPEN: the plan has outflow / inflow faces -- only its generic tiles can see them (a cell with an open face is in no patch)
// PLANAR: the patch workgroups run the planar body; the generic tiles keep the general form (they read the zeros of the
// z-momentum plane and write +0, as the contract has it), so the kernel's register count is the larger of the two bodies'.
template <class T, int KIND, int STAGE, bool NT, bool OPEN = false, bool PLANAR = false>
__global__ __launch_bounds__(256, (patch_wgs_per_cu<T, PLANAR>())) void k_plain_stage(T8gpuPlainPlan P, int patch_begin, int patch_count, int patch_wgs, int chunk,
                                                                                int tile_begin, int tile_count, FVars<T> prev, FVars<T> src,
                                                                                FVars<T> out, const T* __restrict__ vol, T dt,
                                                                                T* __restrict__ speed) {
  const int b = blockIdx.x;
  if (b < patch_wgs) {
    plain_patch_body<T, KIND, STAGE, NT, PLANAR>(P, patch_begin, patch_count, b, patch_wgs, chunk, prev, src, out, vol, dt, speed);
  } else {
    const int pos = tile_begin + xcd_position(b - patch_wgs, tile_count);
    plain_tile_body<T, KIND, STAGE, true, 2, false, OPEN>(P, pos, prev, src, out, vol, dt, speed);
  }
}

// are the five planes of v spaced like the first two of `ref`?
template <class T>
bool planes_equally_spaced(const FVars<T>& v, const FVars<T>& ref) {
  const ptrdiff_t d = reinterpret_cast<const char*>(ref.p[1]) - reinterpret_cast<const char*>(ref.p[0]);
  for (int k = 0; k < 4; k++)
    if (reinterpret_cast<const char*>(v.p[k + 1]) - reinterpret_cast<const char*>(v.p[k]) != d) return false;
  return true;
}

// LDS window of a generic tile in the mixed launch: what plain_tile_body<T, K, S, true, 2> takes (kernels_fused.hip: the pipelined
// kernel with a geometry dictionary, two passes of 256 faces). fp64 KEPES: 8 x (9 x slots + 1 280) + 2 064 bytes.
template <class T>
size_t mixed_tile_lds(int kind, const T8gpuPlainPlan* plan) {
  const int    nw  = kind == 0 ? kPrimWords : 5;
  const size_t tab = lds_log_table<T>(kind);
  return sizeof(T) * (static_cast<size_t>(nw) * plan_slots(*plan) + static_cast<size_t>(5) * 256) + (tab ? tab + 16 : 0);
}

// Patch tiles [patch_begin, patch_begin + patch_count) of tile_order, and -- in the same launch -- the generic tiles
// [tile_begin, tile_begin + tile_count) (tile_count = 0: none). persistent = false: one patch per workgroup (class-split
// multi-rank launches: slots free up continuously, see plain_fused_stage). Returns -1 when generic tiles were handed in
// that the mixed kernel does not take (the caller then launches the two parts separately), else 0 or a hipError_t.
template <class T>
int plain_patch_stage(int kind, int stage, const T8gpuPlainPlan* plan, int patch_begin, int patch_count, int tile_begin, int tile_count,
                      FVars<T> prev, FVars<T> mid, FVars<T> out, const T* volume, T dt, T* speed, bool persistent, bool planar,
                      hipStream_t stream) {
  if (patch_count <= 0) return tile_count > 0 ? -1 : 0;
  // (does this launch run beside another lane's kernels? a plan with ghost-reading tiles, launched in part)
  const bool shared_gpu = plan->n_interior_tiles < plan->ntiles && patch_count + (tile_count > 0 ? tile_count : 0) < plan->ntiles;
  if (!plan->tile_desc) return static_cast<int>(hipErrorInvalidValue);
  if (!plan_planes_fit_32bit<T>(plan)) return static_cast<int>(hipErrorInvalidValue);
  if (plan->ghost_buf || plan->send_map || !persistent || kind != 0) planar = false;   // (the general form, silently)
  // (the planar fp64 body addresses plane k as p[0] + k x spacing: planes not so spaced run the general form as well)
  if (planar && sizeof(T) == 8 && !(planes_equally_spaced(mid, mid) && planes_equally_spaced(out, mid) && (stage == 1 || planes_equally_spaced(prev, mid))))
    planar = false;
  size_t lds = patch_lds<T>(kind, planar);
  // the planar fp64 kernels are built for four workgroups per CU; a launch has four where its LDS window allows them
  const bool planar64 = planar && sizeof(T) == 8;
  // (far-field faces: the generic tiles run k_plain_fused_p_far in a launch of their own -- under the mixed kernel's register
  //  budget of 3 / 5 workgroups per CU their far-field state spills)
  if (tile_count > 0 && plan->has_farfield_faces) return -1;
  if (tile_count > 0) {
    // what plain_tile_body<T, K, S, true, 2> takes, and its LDS window
    if (!plain_tiles_pipelined(plan) || plan->max_faces > 512 || !plan->geo_idx || !plan->geo_table || plan->n_geo <= 0) return -1;
    const size_t lds_tile = mixed_tile_lds<T>(kind, plan);
    if (lds_tile > lds) lds = lds_tile;
    if (sizeof(T) == 8 && 3 * lds > static_cast<size_t>(156) * 1024) return -1;   // (the kernel lives on three workgroups per CU)
  }
  // (else three, under the guard above: generic tiles of more than 398 slots; T8GPU_PATCH_WGS=3: three, for A/B runs)
  static const int per_cu_env = env_per_cu("T8GPU_PATCH_WGS");
  const bool       four       = planar64 && lds <= kLdsQuarterCU && per_cu_env != 3;
  const int cus = device_cu_count();
  if (cus == 0) return static_cast<int>(hipErrorInvalidDevice);
  // persistent = true: the launch covers the whole plan -- as many patch workgroups as stay resident (3 per CU in fp64, 4 in
  // the planar form).
  // persistent = false: a class of a multi-rank stage, launched beside the pack / RCCL / unpack kernels of the exchange: one
  // patch per workgroup, so that slots free up continuously. That costs the patch kernel its software pipeline (13 % at c2
  // size, 19 % at c4 size, measured on one rank), but a "polite" persistent grid of two workgroups per CU for the class
  // launches -- measured in round 3 -- is worse where it matters: rank 3 of the 8-way c4 split with an RCCL
  // self-exchange 0.173 -> 0.205 ms/step (profiles/r03_halo_overhead.md); the exchange kernels wait behind resident
  // workgroups that never leave.
  // a ghost window (t8gpu_hip.h) is honoured by a workgroup's FIRST patch only (plain_patch_body): one patch per workgroup
  if (plan->ghost_buf || plan->send_map) persistent = false;
  const int  per_cu    = sizeof(T) == 8 ? (four ? 4 : 3) : 5;
  const int  resident  = resident_workgroups(cus, per_cu);
  // A persistent launch that shares the GPU with the other lane's kernels (the interior launch of a multi-rank stage: the plan
  // has ghost-reading tiles and the range is not the whole plan) must not count on all its workgroups being resident from
  // the start: whatever slots the RCCL kernel and the ghost-reading tiles hold when it is dispatched, that many of its
  // workgroups start when the FIRST of the others retire and then walk their whole share -- the launch takes up to twice
  // as long (rank 0 of the 2-way c4 split: interior kernel 180 instead of 150 us, profiles/r04_halo_overhead.md). Such
  // launches hand out CHUNKS instead: workgroup j takes `chunk` consecutive patches, with the software pipeline inside the
  // chunk, and the hardware dispatches the chunks as slots free up.
  int chunk = 0;
  // (measured, rank of the c4 mesh split 2 / 4 / 8 ways with a self-exchange, ms per step: persistent walk 0.549 / 0.313 / 0.151,
  //  chunks of 2: 0.497 / 0.280 / 0.153, of 3: 0.483 / 0.268 / 0.151, of 4: 0.481 / 0.264 / 0.156, of 6: 0.469 / 0.288 / 0.157)
  if (persistent && shared_gpu && patch_count >= resident) chunk = 3;
  int patch_wgs = (!persistent || patch_count < resident) ? patch_count : resident;
  if (chunk > 0) {   // 8 XCD shares of ceil(count / 8) patches, ceil(share / chunk) workgroups each
    const int share = (patch_count + 7) / 8;
    patch_wgs       = 8 * ((share + chunk - 1) / chunk);
  }
  const dim3 grid(patch_wgs + (tile_count > 0 ? tile_count : 0)), block(256);
  // non-temporal stage results / previous-state loads where the stage's planes are a stream for the caches (flux_math.hpp)
  const bool nt = stream_hint(plan->n_slots_addressed, sizeof(T));
  return dispatch(
      [&](auto K, auto S, auto NT, auto MIXED, auto OPEN, auto PLANAR) {
        constexpr bool PL = PLANAR && K == 0;   // (HLL / HLLC: nothing new is instantiated)
        if constexpr (MIXED) {
          note_stage_kernel<T>(patch_count + tile_count, grid.x, "k_plain_stage", K, S, NT, OPEN, PL);
          return launch(&k_plain_stage<T, K, S, NT, OPEN, PL>, grid, block, lds, stream, *plan, patch_begin, patch_count, patch_wgs, chunk,
                        tile_begin, tile_count, prev, mid, out, volume, dt, speed);
        } else {
          note_stage_kernel<T>(patch_count, grid.x, "k_plain_patch", K, S, NT, PL);
          return launch(&k_plain_patch<T, K, S, NT, PL>, grid, block, lds, stream, *plan, patch_begin, patch_count, chunk, prev, mid, out, volume,
                        dt, speed);
        }
      },
      kind, stage, nt, tile_count > 0, tile_count > 0 && plan->has_open_faces, planar);
}

// (t8gpu_hip_plain_patch_lds_bytes: the windows above, for the host)
size_t plain_patch_window(int kind, int float_size, bool planar, const T8gpuPlainPlan* tiles) {
  if (kind != 0) planar = false;
  const size_t lds  = float_size == 8 ? patch_lds<double>(kind, planar) : patch_lds<float>(kind, planar);
  const size_t tile = !tiles ? 0 : float_size == 8 ? mixed_tile_lds<double>(kind, tiles) : mixed_tile_lds<float>(kind, tiles);
  return tile > lds ? tile : lds;
}

template int plain_patch_stage<float>(int, int, const T8gpuPlainPlan*, int, int, int, int, FVars<float>, FVars<float>, FVars<float>,
                                      const float*, float, float*, bool, bool, hipStream_t);
template int plain_patch_stage<double>(int, int, const T8gpuPlainPlan*, int, int, int, int, FVars<double>, FVars<double>, FVars<double>,
                                       const double*, double, double*, bool, bool, hipStream_t);

}  // namespace t8gpu_hip

extern "C" int t8gpu_hip_plain_patch_lds_bytes(const T8gpuPlainPlan* plan, int flux_kind, int float_size, int planar) {
  if (flux_kind < 0 || flux_kind > 2 || (float_size != 4 && float_size != 8)) return -1;
  return static_cast<int>(t8gpu_hip::plain_patch_window(flux_kind, float_size, planar != 0, plan));
}
