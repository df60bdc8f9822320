// fused_common.hpp -- small pieces shared by the fused tile kernels (kernels_fused.hip, kernels_fused_persistent.hip).
#ifndef T8GPU_HIP_FUSED_COMMON_HPP
#define T8GPU_HIP_FUSED_COMMON_HPP

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "flux_math.hpp"
#include "t8gpu_hip.h"

namespace t8gpu_hip {

// Compute units of the current device, asked once (0: no device). Function-local statics: the launchers are called from two
// host threads of a rank (stepper.hip: the step driver's lanes), so their lazily initialised settings must be race-free.
inline int device_cu_count() {
  static const int n = [] {
    int             dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    return prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }();
  return n;
}
// a tuning variable holding workgroups per CU: 1 .. 8, anything else (or unset) = 0 = "the kernel's own default"
inline int env_per_cu(const char* name) {
  const char* env = std::getenv(name);
  const int   v   = env ? std::atoi(env) : 0;
  return (v < 0 || v > 8) ? 0 : v;
}

// Resident workgroups of a persistent launch: `per_cu` on each of `cus` compute units, or the limit a test has set
// (t8gpu_hip.h: t8gpu_hip_set_resident_limit; 0 = none) where that is smaller. Every persistent launcher sizes its grid -- and
// takes its decisions that compare a tile count with the resident workgroups -- through this one function. An atomic, read at
// launch time: the step driver launches from two host threads.
inline std::atomic<int>& resident_limit() {
  static std::atomic<int> limit{0};
  return limit;
}
inline int resident_workgroups(int cus, int per_cu) {
  const int full = cus * per_cu, limit = resident_limit().load(std::memory_order_relaxed);
  return limit > 0 && limit < full ? limit : full;
}

// ---- host side of the fused-stage launchers ---------------------------------------------------------------------
// Runtime launch choices -> compile-time constants: dispatch(f, kind, stage, b...) calls f(int_c<kind>, int_c<stage>,
// bool_c<b>...) for kind 0..2 (KEPES, HLL, HLLC) and stage 1..3. The generic lambda f names its kernel with these constants
// as template arguments (and `if constexpr` keeps combinations it never launches from instantiating a kernel).
template <int V>
using int_c = std::integral_constant<int, V>;
template <bool V>
using bool_c = std::integral_constant<bool, V>;

template <class F>
int dispatch_flags(F&& f) {
  return f();
}
template <class F, class... B>
int dispatch_flags(F&& f, bool b, B... rest) {
  if (b) return dispatch_flags([&](auto... c) { return f(bool_c<true>{}, c...); }, rest...);
  return dispatch_flags([&](auto... c) { return f(bool_c<false>{}, c...); }, rest...);
}
template <class F, class... B>
int dispatch(F&& f, int kind, int stage, B... flags) {
  auto with_kind = [&](auto K) {
    auto with_stage = [&](auto S) { return dispatch_flags([&](auto... c) { return f(K, S, c...); }, flags...); };
    return stage == 1 ? with_stage(int_c<1>{}) : stage == 2 ? with_stage(int_c<2>{}) : with_stage(int_c<3>{});
  };
  return kind == 0 ? with_kind(int_c<0>{}) : kind == 1 ? with_kind(int_c<1>{}) : with_kind(int_c<2>{});
}
// its sibling for launchers without a stage (kernels_compat.hip, kernels_boundary.hip): f(int_c<kind>, bool_c<b>...), kind 0..2
template <class F, class... B>
int dispatch_kind(F&& f, int kind, B... flags) {
  auto with_kind = [&](auto K) { return dispatch_flags([&](auto... c) { return f(K, c...); }, flags...); };
  return kind == 0 ? with_kind(int_c<0>{}) : kind == 1 ? with_kind(int_c<1>{}) : with_kind(int_c<2>{});
}

// Launches `kernel` with `lds` bytes of dynamic LDS; a kernel is granted more than the default 64 KiB first. Returns 0 or a
// hipError_t.
template <class... P, class... A>
int launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, A&&... args) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(lds));
    if (e != hipSuccess) return static_cast<int>(e);
  }
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, std::forward<A>(args)...);
  return static_cast<int>(hipGetLastError());
}

// element slots per LDS plane of a generic tile: the plan's max_slots, or (0) the element and halo caps together
__host__ __device__ __forceinline__ int plan_slots(const T8gpuPlainPlan& P) {
  return P.max_slots > 0 ? P.max_slots : P.max_elems + P.max_halo;
}

// Do the generic tiles of this plan run the pipelined one-tile kernels (ELL rows + tile descriptors: no CSR lists read), or the
// generic kernel, which walks csr_off / csr_ent? One definition for the launchers (kernels_fused.hip, kernels_fused_patch.hip)
// and for t8gpu_hip_plain_needs_csr, which the host asks before it decides what to upload.
inline bool plain_tiles_pipelined(const T8gpuPlainPlan* plan) {
  return plan->ell && plan->tile_desc && plan->ell_width >= 8 && plan->ell_width % 8 == 0 && plan->max_elems <= 256 &&
         plan_slots(*plan) <= 512 && plan->max_faces <= 1024;
}

// LDS bytes of the fp64 KEPES logarithm table (flux_math.hpp: kLogTab), 0 where the kernel has none
template <class T>
size_t lds_log_table(int kind) {
  return (sizeof(T) == 8 && kind == 0) ? 2 * kLogTabEntries * sizeof(double) : 0;
}

template <class T>
struct FVars {
  T* p[5];
};

template <class T>
struct vec4;
template <>
struct vec4<float> {
  using type = float4;
};
template <>
struct vec4<double> {
  using type = double4;
};

template <class T>
struct vec2;
template <>
struct vec2<float> {
  using type = float2;
};
template <>
struct vec2<double> {
  using type = double2;
};

// XCD-aware bijection block -> position in [0, nb): XCD x (= b % 8) owns a contiguous run.
T8_DEV int xcd_position(int b, int nb) {
  const int q = nb >> 3, rem = nb & 7, x = b & 7, k = b >> 3;
  return x * q + (x < rem ? x : rem) + k;
}

template <class T, class V>
FVars<T> fmk(const V& v) {
  FVars<T> o;
  for (int k = 0; k < 5; k++) o.p[k] = v.p[k];
  return o;
}

// ---- ghost window (T8gpuPlainPlan::ghost_buf / send_map: the multi-rank step driver's zero-copy exchange) -------------
// State value `k` of slot `slot`: ghosts (slot >= n_owned) come from the exchange's receive buffer in its wire format.
template <class T>
T8_DEV T ghost_window_load(const T8gpuPlainPlan& P, const FVars<T>& src, int slot, int k) {
  const T* gb = static_cast<const T*>(P.ghost_buf);
  const T* p  = slot >= P.n_owned ? gb + (5 * static_cast<size_t>(slot - P.n_owned) + k) : src.p[k] + slot;
  return *p;
}
// The five new values of owned element e also go to its send slots (a no-op for the elements no peer mirrors).
template <class T>
T8_DEV void ghost_window_send(const T8gpuPlainPlan& P, int e, const T v[5]) {
  const int m = P.send_map[e];
  if (m == -1) return;
  T* const sb = static_cast<T*>(P.send_buf);
  if (m >= 0) {
#pragma unroll
    for (int k = 0; k < 5; k++) sb[5 * static_cast<size_t>(m) + k] = v[k];
    return;
  }
  const int32_t* l = P.send_list + (-m - 2);
  for (;;) {
    const int ent = *l++;
    const size_t t = static_cast<size_t>(ent & 0x7FFFFFFF);
#pragma unroll
    for (int k = 0; k < 5; k++) sb[5 * t + k] = v[k];
    if (ent < 0) break;
  }
}

// Which boundary kinds a kernel decodes (compile time): walls only (no kinds list and no inflow table is read), kinds 0..9
// (wall, outflow, inflow k), or kinds 0..15 (far field k as well). A kernel below kBndFar holds no far-field code. The MODE of
// the compat tier (compat_faces.hpp, kernels_compat.hip, kernels_boundary.hip) and of the Subgrid stage kernels
// (kernels_subgrid_fused.hip); the plain tile kernels spell the same choice as the bools OPEN, FAR (below).
enum BoundaryMode { kBndWalls = 0, kBndOpen = 1, kBndFar = 2 };

// ---- boundary faces of the tile plan (ABI 9) ------------------------------------------------------------------------
// The r half of a face_lr entry (tile_plan.cpp: boundary_code): a tile-local slot below 0xFFF0, else 0xFFFF reflective wall,
// 0xFFFE outflow, 0xFFF0 + k inflow state k. The one place that spells the codes; only the OPEN instantiations of the tile
// kernels decode the open ones (the others see walls only, as before ABI 9).
// FAR (ABI 11): the plan also has far-field faces, 0xFFF8 + k far-field state k (k < 6); inflow codes are then 0xFFF0..0xFFF7.
// FAR = false decodes exactly as before ABI 11 (those plans have no far-field codes).
struct FaceSide {
  int  r;        // slot of the right state in LDS: the neighbour, or l itself at a boundary face
  bool wall;     // reflective wall: the right state is the mirror image of the left one
  bool open;     // outflow, inflow or far field: no right element to update
  int  inflow;   // inflow state index, -1 otherwise
  int  far;      // far-field state index, -1 otherwise (FAR only)
};
template <bool FAR = false>
T8_DEV FaceSide decode_face_side(int l, unsigned r16) {
  FaceSide f;
  f.wall   = r16 == 0xFFFFu;
  f.open   = r16 >= 0xFFF0u && r16 < 0xFFFFu;
  if constexpr (FAR) {
    f.inflow = r16 >= 0xFFF0u && r16 < 0xFFF8u ? static_cast<int>(r16 - 0xFFF0u) : -1;
    f.far    = r16 >= 0xFFF8u && r16 < 0xFFFEu ? static_cast<int>(r16 - 0xFFF8u) : -1;
  } else {
    f.inflow = r16 >= 0xFFF0u && r16 < 0xFFFEu ? static_cast<int>(r16 - 0xFFF0u) : -1;
    f.far    = -1;
  }
  f.r      = r16 >= 0xFFF0u ? l : static_cast<int>(r16);
  return f;
}

// ---- far-field faces (ABI 11): the Riemann-invariant condition ----------------------------------------
// The outside state of a far-field face from the inside primitives (ri, vi, pi), the face's outward unit normal n and the
// far-field state of inflow-table row `row` (its primitives rho, v, p: words 5-9). gamma = 1.4, 2 / (gamma - 1) = 5.
// Returns what the face takes as its outside state:
//   kFarTable   supersonic inflow (qi <= -ci): the table row itself -- the bits of an inflow face with that state;
//   kFarInside  supersonic outflow (qi >= ci), or the guard cb <= 0: the inside state itself -- the bits of an outflow face;
//   kFarBuilt   subsonic: (rb, vb, pb) from the outgoing invariant qi + 5 ci and the incoming one qf - 5 cf, with the
//               entropy and tangential velocity of the side the flow comes from (inside if qb > 0, else the far field).
// Shared by the fused tiers (kernels_fused.hip, fused_tile_body.hpp) and the compat tier (kernels_compat.hip).
enum FarSide { kFarTable = 0, kFarInside = 1, kFarBuilt = 2 };
template <class T>
T8_DEV int farfield_outside(T ri, const T vi[3], T pi, const T n[3], const T* __restrict__ row, T& rb, T vb[3], T& pb) {
  const T* w  = row + 5;
  const T  rf = w[0], pf = w[4];
  const T  vf[3] = {w[1], w[2], w[3]};
  const T  ci = sqrt(T(1.4) * pi / ri);
  const T  qi = vi[0] * n[0] + vi[1] * n[1] + vi[2] * n[2];
  if (qi <= -ci) return kFarTable;
  if (qi >= ci) return kFarInside;
  const T cf = sqrt(T(1.4) * pf / rf);
  const T qf = vf[0] * n[0] + vf[1] * n[1] + vf[2] * n[2];
  const T rp = qi + T(5) * ci, rm = qf - T(5) * cf;
  const T qb = T(0.5) * (rp + rm), cb = (rp - rm) / T(10);
  if (!(cb > T(0))) return kFarInside;
  const bool in = qb > T(0);
  const T    rr = in ? ri : rf, cr = in ? ci : cf, dq = qb - (in ? qi : qf);
  const T    x = cb / cr, x2 = x * x;
  rb = rr * (x2 * x2 * x);   // isentropic with the reference side's entropy: rho_r (cb / cr)^5
  pb = rb * cb * cb / T(1.4);
#pragma unroll
  for (int k = 0; k < 3; k++) vb[k] = (in ? vi[k] : vf[k]) + dq * n[k];
  return kFarBuilt;
}
// conservative state of the primitives (rho, v, p)
template <class T>
T8_DEV void state_from_prim(T rho, const T v[3], T p, T s[5]) {
  s[0] = rho;
  s[1] = rho * v[0];
  s[2] = rho * v[1];
  s[3] = rho * v[2];
  s[4] = p / T(0.4) + T(0.5) * rho * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}
// The KEPES side: R holds the inside record on entry (a boundary face's right slot is its left one) and the outside record on
// return -- the table's record, the inside one, or the built state's record by the routine cells use (prim_from_state).
template <class T, bool TAB>
T8_DEV void farfield_prim(const T* __restrict__ row, const T n[3], const double* logtab, Prim<T>& R) {
  const T   vi[3] = {R.vx, R.vy, R.vz};
  T         rb, vb[3], pb;
  const int side = farfield_outside<T>(R.rho, vi, R.p, n, row, rb, vb, pb);
  if (side == kFarTable) {
    const T* w = row + 5;
    R.rho = w[0]; R.vx = w[1]; R.vy = w[2]; R.vz = w[3]; R.p = w[4]; R.beta = w[5]; R.lrho = w[6]; R.lbeta = w[7]; R.v0 = w[8];
  } else if (side == kFarBuilt) {
    T s[5];
    state_from_prim<T>(rb, vb, pb, s);
    R = prim_from_state<T, TAB>(s, logtab);
  }
}
// The conservative side (HLL / HLLC, compat tier, Subgrid blocks): s holds the inside state on entry and the outside state on
// return. Returns the FarSide (kFarInside: s is untouched -- a caller that holds the inside cell's record keeps that).
template <class T>
T8_DEV int farfield_state(const T* __restrict__ row, const T n[3], T s[5]) {
  const Prim<T> q     = prim_from_state<T>(s);   // (only rho, v, p are used)
  const T       vi[3] = {q.vx, q.vy, q.vz};
  T             rb, vb[3], pb;
  const int     side = farfield_outside<T>(q.rho, vi, q.p, n, row, rb, vb, pb);
  if (side == kFarTable) {
#pragma unroll
    for (int k = 0; k < 5; k++) s[k] = row[k];
  } else if (side == kFarBuilt) {
    state_from_prim<T>(rb, vb, pb, s);
  }
  return side;
}
// the conservative state (words 0-4) and the KEPES per-element record (words 5-13) of inflow state k
template <class T>
T8_DEV const T* inflow_entry(const T8gpuPlainPlan& P, int k) {
  return static_cast<const T*>(P.inflow) + T8GPU_INFLOW_WORDS * k;
}
template <class T>
T8_DEV void inflow_prim(const T8gpuPlainPlan& P, int k, Prim<T>& q) {
  const T* w = inflow_entry<T>(P, k) + 5;
  q.rho = w[0]; q.vx = w[1]; q.vy = w[2]; q.vz = w[3]; q.p = w[4]; q.beta = w[5]; q.lrho = w[6]; q.lbeta = w[7]; q.v0 = w[8];
}

// ---- LDS records of the persistent kernels (kernels_fused_persistent.hip, kernels_fused_patch.hip) ---------------
template <class T>
struct vec16;
template <>
struct vec16<double> {
  using type = double2;
  static constexpr int lanes = 2;
};
template <>
struct vec16<float> {
  using type = float4;
  static constexpr int lanes = 4;
};

// words per LDS record: NW payload words padded so that (a) 16-byte pieces stay aligned and (b) consecutive slots
// start in different bank groups (record size / 16 B is odd: 5 or 3)
template <class T, int NW>
constexpr int rec_words() {
  return sizeof(T) == 8 ? (NW > 5 ? 10 : 6) : 12;
}

// dynamic LDS of a patch or persistent launch: `words` words of flux buffers and tables, `records` LDS records, the logarithm table
template <class T>
size_t record_lds(int kind, size_t words, size_t records) {
  const size_t rec = kind == 0 ? rec_words<T, kPrimWords>() : rec_words<T, 5>();
  return sizeof(T) * (words + rec * records) + lds_log_table<T>(kind);
}

template <class T, int NW>
T8_DEV void rec_store(T* rec, const T* w) {
  using V         = typename vec16<T>::type;
  constexpr int L = vec16<T>::lanes;
#pragma unroll
  for (int c = 0; c + L <= NW; c += L) {
    V v;
    T* vv = reinterpret_cast<T*>(&v);
#pragma unroll
    for (int j = 0; j < L; j++) vv[j] = w[c + j];
    *reinterpret_cast<V*>(rec + c) = v;
  }
#pragma unroll
  for (int c = NW / L * L; c < NW; c++) rec[c] = w[c];
}

template <class T, int NW>
T8_DEV void rec_load(const T* rec, T* w) {
  using V         = typename vec16<T>::type;
  constexpr int L = vec16<T>::lanes;
#pragma unroll
  for (int c = 0; c + L <= NW; c += L) {
    const V  v  = *reinterpret_cast<const V*>(rec + c);
    const T* vv = reinterpret_cast<const T*>(&v);
#pragma unroll
    for (int j = 0; j < L; j++) w[c + j] = vv[j];
  }
#pragma unroll
  for (int c = NW / L * L; c < NW; c++) w[c] = rec[c];
}

template <class T>
T8_DEV void prim_words(const T s[5], T w[kPrimWords], const double* logtab) {
  const Prim<T> q = prim_from_state<T, sizeof(T) == 8>(s, logtab);   // fp64: table-driven logarithms (flux_math.hpp)
  w[0] = q.rho; w[1] = q.vx; w[2] = q.vy; w[3] = q.vz; w[4] = q.p; w[5] = q.beta; w[6] = q.lrho; w[7] = q.lbeta; w[8] = q.v0;
}
template <class T>
T8_DEV void words_prim(const T w[kPrimWords], Prim<T>& q) {
  q.rho = w[0]; q.vx = w[1]; q.vy = w[2]; q.vz = w[3]; q.p = w[4]; q.beta = w[5]; q.lrho = w[6]; q.lbeta = w[7]; q.v0 = w[8];
}

// PLANAR records (kernels_fused_patch.hip): no vz word. fp32: eight payload words in a record of the SAME stride as the nine-word
// one (rec_words: 12 floats), so consecutive records keep starting in different bank groups. fp64: 64 bytes per record, in
// chunk planes (rec_split_store / rec_split_load below) -- eight doubles side by side would put the 16-byte record reads of
// neighbouring cells on four bank groups.
constexpr int kPrimWordsPlanar = 8;
template <class T>
T8_DEV void prim_words_planar(const T s[4], T w[kPrimWordsPlanar], const double* logtab) {
  const Prim<T> q = prim_from_state_planar<T, sizeof(T) == 8>(s, logtab);
  w[0] = q.rho; w[1] = q.vx; w[2] = q.vy; w[3] = q.p; w[4] = q.beta; w[5] = q.lrho; w[6] = q.lbeta; w[7] = q.v0;
}
template <class T>
T8_DEV void words_prim_planar(const T w[kPrimWordsPlanar], Prim<T>& q) {
  q.rho = w[0]; q.vx = w[1]; q.vy = w[2]; q.p = w[3]; q.beta = w[4]; q.lrho = w[5]; q.lbeta = w[6]; q.v0 = w[7];
}

// PLANAR fp64 records (kernels_fused_patch.hip): the eight payload doubles take 64 bytes -- 320 records 20 480 bytes instead of
// 25 600, which is what lets a fourth workgroup per CU fit the LDS -- stored as FOUR PLANES OF 16-BYTE CHUNKS: chunk c (words 2 c,
// 2 c + 1) of record r lies at 16 r + c x (16 x records). A wavefront reads chunk c of its lanes' records with one ds_read_b128,
// and records r, r' meet in a bank group only where r = r' (mod 16): the behaviour of the padded records (80 bytes = 5 bank
// groups, 5 odd), where 64-byte records side by side would put neighbouring cells on four bank groups. A record is named by
// the byte offset 16 r of its first chunk; the plane stride is a compile-time constant and rides in the instruction's offset.
constexpr int kSplitChunkBytes = 16;
template <int RECORDS>
T8_DEV void rec_split_store(double* recs, int off0, const double w[kPrimWordsPlanar]) {
#pragma unroll
  for (int c = 0; c < 4; c++) {
    double2 v;
    v.x = w[2 * c];
    v.y = w[2 * c + 1];
    *reinterpret_cast<double2*>(reinterpret_cast<char*>(recs) + off0 + c * (kSplitChunkBytes * RECORDS)) = v;
  }
}
template <int RECORDS>
T8_DEV void rec_split_load(const double* recs, int off0, double w[kPrimWordsPlanar]) {
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const double2 v = *reinterpret_cast<const double2*>(reinterpret_cast<const char*>(recs) + off0 + c * (kSplitChunkBytes * RECORDS));
    w[2 * c]     = v.x;
    w[2 * c + 1] = v.y;
  }
}

// persistent, software-pipelined tile kernel (kernels_fused_persistent.hip). Returns -1 when the plan is outside what
// that kernel takes (the caller then uses the one-tile-per-workgroup kernels), otherwise 0 or a hipError_t.
template <class T>
int plain_persistent_stage(int kind, int stage, const T8gpuPlainPlan* plan, int tile_begin, int tile_count, FVars<T> prev,
                           FVars<T> mid, FVars<T> out, const T* volume, T dt, T* speed, hipStream_t stream);

// structured-patch kernel (kernels_fused_patch.hip): [patch_begin, +patch_count) of tile_order are patch tiles; the generic
// tiles [tile_begin, +tile_count) ride in the same launch where the mixed kernel takes them (-1: it does not; launch apart).
// planar: the caller vouches for the planar contract (t8gpu_hip.h: t8gpu_hip_plain_fused_stage_planar_*); honoured for KEPES
// in a persistent launch without a ghost window, otherwise the general form runs.
template <class T>
int plain_patch_stage(int kind, int stage, const T8gpuPlainPlan* plan, int patch_begin, int patch_count, int tile_begin, int tile_count,
                      FVars<T> prev, FVars<T> mid, FVars<T> out, const T* volume, T dt, T* speed, bool persistent, bool planar,
                      hipStream_t stream);

// 3D structured patches (kernels_fused_patch3.hip): [tile_begin, +tile_count) of tile_order are 8 x 8 x 4 patch tiles, all
// regular or (irregular = true) all irregular ones
template <class T>
int plain_patch3_stage(int kind, int stage, const T8gpuPlainPlan* plan, int tile_begin, int tile_count, FVars<T> prev, FVars<T> mid,
                       FVars<T> out, const T* volume, T dt, T* speed, bool persistent, bool irregular, hipStream_t stream);

// regular + irregular 3D patches of one class in one persistent launch (-1: launch them one after the other)
template <class T>
int plain_patch3_both_stage(int kind, int stage, const T8gpuPlainPlan* plan, int reg_begin, int reg_count, int irr_begin, int irr_count,
                            FVars<T> prev, FVars<T> mid, FVars<T> out, const T* volume, T dt, T* speed, hipStream_t stream);

}  // namespace t8gpu_hip

#endif  // T8GPU_HIP_FUSED_COMMON_HPP
