// oracle/oracle.hpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
//
// Host-side restatement of the t8gpu finite-volume hot path (KEPES / HLL face
// flux + SSP-RK3 stages, plain elements and Subgrid<4,4>/<4,4,4>), used by
// tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg as the
// checker. Every function cites the reference lines (relative to
// /root/reference) whose floating-point sequence it follows. Operation order
// and association are kept as written there, so that a host compilation with
// `-ffp-contract=off` reproduces the reference arithmetic.
//
// PINNING STATUS: the reference ships no tests, fixtures or golden vectors
//  and cannot be built here (needs nvcc + t8code/libsc).
// What pins this file to it (tests/golden/README.md):
//  * the three known answers of SURVEY.md section 8c (KEPES f64/f32, HLL f32)
//    and the 10 240 flux vectors per float type made from the reference's own
//    flux functions compiled for the host: tests/test_oracle_golden.py, bit for
//    bit;
//  * the executed kernel vectors -- inputs and outputs of the reference's
//    kernel BODIES (plain and Subgrid flux kernels with the 2:1 hanging map,
//    walls, the six RK stages) run on tiny AMR meshes:
//    tests/test_oracle_reference_kernels.py, bit for bit;
//  * the executed AMR vectors -- the plain and Subgrid transfer kernels of
//    adapt(), both refinement criteria and estimate_gradient, run on real
//    forests (a coarsened and a refined family at element 0, a new mesh of one
//    element): tests/test_oracle_reference_amr_kernels.py, bit for bit;
//  * the HIP tiers meet those same arrays directly, not only through this file:
//    tests/test_gpu_reference_kernels.py (compat kernels one by one, the
//    element -> slot map, one fused stage per kernel form) and
//    tests/test_gpu_reference_amr_kernels.py (transfer, criteria, gradient,
//    z-order, gather / scatter / repartition, amr.adapt and amr.adapt_subgrid).
// All three fixtures come from host compilations behind stand-ins for the CUDA
// qualifiers and built-ins, so by the project's rules
// parity formally stays "unpinned".
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#if defined(_OPENMP)
#include <omp.h>

#include <vector>
#endif

namespace oracle {

// ---------------------------------------------------------------------------
// constants: t8gpu/timestepping/ssp_runge_kutta.inl:3-26 (truncated decimals,
// SURVEY quirk Q1) and examples/compressible_euler/kernels.cu:5-20.
// ---------------------------------------------------------------------------
template <class T>
struct rk3;
template <>
struct rk3<float> {
  static constexpr float c21 = 0.75f, c22 = 0.25f, c23 = 0.25f;
  static constexpr float c31 = 0.33333333333333f, c32 = 0.66666666666666f, c33 = 0.66666666666666f;
};
template <>
struct rk3<double> {
  static constexpr double c21 = 0.75, c22 = 0.25, c23 = 0.25;
  static constexpr double c31 = 0.33333333333333, c32 = 0.66666666666666, c33 = 0.66666666666666;
};

// ---------------------------------------------------------------------------
// a1: logarithmic mean, examples/compressible_euler/kernels.cu:24-36
// (duplicate at examples/subgrid/kernels.inl:21-33).
// ---------------------------------------------------------------------------
template <class T>
inline T ln_mean(T aL, T aR) {
  const T xi = aR / aL;
  const T u  = (xi * (xi - T(2.0)) + T(1.0)) / (xi * (xi + T(2.0)) + T(1.0));
  if (u < T(1.0e-4)) {
    return (aL + aR) * T(52.50) / (T(105.0) + u * (T(35.0) + u * (T(21.0) + u * T(15.0))));
  }
  return (aR - aL) / std::log(xi);
}

template <class T>
struct Means {
  T u, v, w, a, rho, h, p1;
};

// ---------------------------------------------------------------------------
// a2: entropy-conservative two-point flux in the face frame,
// kernels.cu:38-93 (dup kernels.inl:35-90). gamma = 1.4 literal.
// ---------------------------------------------------------------------------
template <class T>
inline void kepes_ec_flux(const T uL[5], const T uR[5], T Fs[5], Means<T>& m) {
  const T one = T(1), half = T(0.5);
  const T kappa = T(1.4);
  const T km1   = kappa - one;
  const T skm1  = one / km1;

  const T irL = one / uL[0];
  const T vxL = irL * uL[1], vyL = irL * uL[2], vzL = irL * uL[3];
  const T irR = one / uR[0];
  const T vxR = irR * uR[1], vyR = irR * uR[2], vzR = irR * uR[3];

  const T qL = half * (vxL * vxL + vyL * vyL + vzL * vzL);
  const T qR = half * (vxR * vxR + vyR * vyR + vzR * vzR);

  const T pL = km1 * (uL[4] - uL[0] * qL);
  const T pR = km1 * (uR[4] - uR[0] * qR);

  const T bL = half * uL[0] / pL;
  const T bR = half * uR[0] / pR;

  const T rho_mean  = half * (uL[0] + uR[0]);
  m.rho             = ln_mean<T>(uL[0], uR[0]);
  const T beta_mean = half * (bL + bR);
  const T beta_hat  = ln_mean<T>(bL, bR);

  m.u  = half * (vxL + vxR);
  m.v  = half * (vyL + vyR);
  m.w  = half * (vzL + vzR);
  m.a  = std::sqrt(kappa * half * (pL + pR) / m.rho);
  m.h  = kappa / (T(2.0f) * km1 * beta_hat) + half * (vxL * vxR + vyL * vyR + vzL * vzR);
  m.p1 = half * rho_mean / beta_mean;
  const T q2 = qL + qR;

  Fs[0] = m.rho * m.u;
  Fs[1] = Fs[0] * m.u + m.p1;
  Fs[2] = Fs[0] * m.v;
  Fs[3] = Fs[0] * m.w;
  Fs[4] = Fs[0] * half * (skm1 / beta_hat - q2) + m.u * Fs[1] + m.v * Fs[2] + m.w * Fs[3];
}

// ---------------------------------------------------------------------------
// a3 + dissipation: kernels.cu:95-133 (eigenvector matrix, eigenvalue scaling)
// and kernels.cu:224-279 (entropy variables, jump, R D R^T [v], F = F* - D/2);
// the same sequence is kernels.inl:92-130 + 189-261 (compute_total_kepes_flux).
// `speed` (may be null) receives |uHat| + aHat as in kernels.cu:222.
// ---------------------------------------------------------------------------
template <class T>
inline void kepes_total_flux(const T uL[5], const T uR[5], T F[5], T* speed) {
  const T zero = T(0), one = T(1), half = T(0.5);
  T        Fs[5];
  Means<T> m;
  kepes_ec_flux<T>(uL, uR, Fs, m);

  const T kappa = T(1.4);
  const T km1   = kappa - one;

  const T R[5][5] = {
      {one, one, zero, zero, one},
      {m.u - m.a, m.u, zero, zero, m.u + m.a},
      {m.v, m.v, one, zero, m.v},
      {m.w, m.w, zero, one, m.w},
      {m.h - m.u * m.a, static_cast<T>(0.5) * (m.u * m.u + m.v * m.v + m.w * m.w), m.v, m.w, m.h + m.u * m.a}};
  T D[5];
  D[0] = half * std::abs(m.u - m.a) * m.rho / kappa;
  D[1] = std::abs(m.u) * (km1 / kappa) * m.rho;
  D[2] = std::abs(m.u) * m.p1;
  D[3] = D[2];
  D[4] = half * std::abs(m.u + m.a) * m.rho / kappa;

  if (speed) *speed = std::abs(m.u) + m.a;

  const T irL = one / uL[0], irR = one / uR[0];
  const T VL[3] = {uL[1] * irL, uL[2] * irL, uL[3] * irL};
  const T VR[3] = {uR[1] * irR, uR[2] * irR, uR[3] * irR};
  const T pL = km1 * (uL[4] - half * (uL[1] * VL[0] + uL[2] * VL[1] + uL[3] * VL[2]));
  const T pR = km1 * (uR[4] - half * (uR[1] * VR[0] + uR[2] * VR[1] + uR[3] * VR[2]));
  const T sL = std::log(pL) - kappa * std::log(uL[0]);
  const T sR = std::log(pR) - kappa * std::log(uR[0]);
  const T rpL = uL[0] / pL, rpR = uR[0] / pR;

  T vL[5], vR[5], jump[5], d[5];
  vL[0] = (kappa - sL) / (km1)-half * rpL * (VL[0] * VL[0] + VL[1] * VL[1] + VL[2] * VL[2]);
  vR[0] = (kappa - sR) / (km1)-half * rpR * (VR[0] * VR[0] + VR[1] * VR[1] + VR[2] * VR[2]);
  for (int c = 0; c < 3; c++) {
    vL[1 + c] = rpL * VL[c];
    vR[1 + c] = rpR * VR[c];
  }
  vR[4] = -rpR;
  vL[4] = -rpL;

  for (int k = 0; k < 5; k++) jump[k] = vR[k] - vL[k];
  for (int k = 0; k < 5; k++)
    d[k] = D[k] * (R[0][k] * jump[0] + R[1][k] * jump[1] + R[2][k] * jump[2] + R[3][k] * jump[3] + R[4][k] * jump[4]);
  for (int k = 0; k < 5; k++) {
    const T dk = R[k][0] * d[0] + R[k][1] * d[1] + R[k][2] * d[2] + R[k][3] * d[3] + R[k][4] * d[4];
    F[k]       = Fs[k] - half * dk;
  }
}

// ---------------------------------------------------------------------------
// a12: HLL flux (dead code in the reference), kernels.inl:263-332.
// `speed` (may be null; NOT in the reference, whose HLL writes no estimate): max(|S_l|, |S_r|) of the wave-speed
// bounds before the clamp to zero -- the CFL-relevant signal speed of this solver, so that compute_timestep works
// with flux_kind HLL / HLLC as it does with KEPES (kernels.cu:222).
// ---------------------------------------------------------------------------
template <class T>
inline void hll_total_flux(const T uL[5], const T uR[5], T F[5], T* speed = nullptr) {
  const T zero = T(0), one = T(1), half = T(0.5);
  const T g = T(1.4);

  const T v1l = uL[1] / uL[0], v2l = uL[2] / uL[0], v3l = uL[3] / uL[0];
  const T pl  = (g - 1) * (uL[4] - half * uL[0] * (v1l * v1l + v2l * v2l + v3l * v3l));
  const T Hl  = (uL[4] + pl) / uL[0];
  const T cl  = std::sqrt((g - 1) * (Hl - half * (v1l * v1l + v2l * v2l + v3l * v3l)));

  const T v1r = uR[1] / uR[0], v2r = uR[2] / uR[0], v3r = uR[3] / uR[0];
  const T pr  = (g - one) * (uR[4] - half * uR[0] * (v1r * v1r + v2r * v2r + v3r * v3r));
  const T Hr  = (uR[4] + pr) / uR[0];
  const T cr  = std::sqrt((g - one) * (Hr - half * (v1r * v1r + v2r * v2r + v3r * v3r)));

  const T wl = std::sqrt(uL[0]), wr = std::sqrt(uR[0]);
  const T ws = wl + wr;
  const T v1 = (wl * v1l + wr * v1r) / ws;
  const T v2 = (wl * v2l + wr * v2r) / ws;
  const T v3 = (wl * v3l + wr * v3r) / ws;
  const T H  = (wl * Hl + wr * Hr) / ws;
  const T c  = std::sqrt((g - one) * (H - half * (v1 * v1 + v2 * v2 + v3 * v3)));

  const T Sl = std::min(v1 - c, v1l - cl);
  const T Sr = std::max(v1 + c, v1r + cr);
  if (speed) *speed = std::max(std::abs(Sl), std::abs(Sr));

  const T Fl[5] = {uL[1], uL[1] * uL[1] / uL[0] + pl, uL[1] * v2l, uL[1] * v3l, uL[1] * Hl};
  const T Fr[5] = {uR[1], uR[1] * uR[1] / uR[0] + pr, uR[1] * v2r, uR[1] * v3r, uR[1] * Hr};

  const T sl = std::min(Sl, zero);
  const T sr = std::max(Sr, zero);
  for (int k = 0; k < 5; k++) F[k] = ((sr * Fl[k] - sl * Fr[k]) + sr * sl * (uR[k] - uL[k])) / (sr - sl);
}

// ---------------------------------------------------------------------------
// a11: face frame. Basis kernels.cu:174-193 == kernels.inl:133-156; rotation
// kernels.cu:196-206 / kernels.inl:159-166; wall mirror kernels.cu:371-375 /
// kernels.inl:169-176; back-rotation kernels.cu:288-290 / kernels.inl:179-186.
// ---------------------------------------------------------------------------
// ONE DEPARTURE from the reference: its seed (ny, nz, -nx) is antiparallel to n at n = +-(1, -1, 1) / sqrt 3, where the
// projection leaves nothing (t1 = -n, t2 = 0 or NaN) and near which the frame loses orthonormality as eps / |r|. Where the
// squared length before normalisation is below 2^-6 (4.2 degrees around that direction, 0.27 % of all directions) the frame
// is built from the second seed (nz, -nx, ny) in the same way. Every other normal keeps the reference's arithmetic and bits.
template <class T>
inline T frame_project(const T n[3], T s0, T s1, T s2, T t1[3]) {
  t1[0] = s0;
  t1[1] = s1;
  t1[2] = s2;
  const T dp = n[0] * t1[0] + n[1] * t1[1] + n[2] * t1[2];
  t1[0] -= dp * n[0];
  t1[1] -= dp * n[1];
  t1[2] -= dp * n[2];
  return t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2];
}
template <class T>
inline void face_basis(const T n[3], T t1[3], T t2[3]) {
  T r2 = frame_project<T>(n, n[1], n[2], -n[0], t1);
  if (r2 < T(0.015625)) r2 = frame_project<T>(n, n[2], -n[0], n[1], t1);
  const T nrm = std::sqrt(r2);
  t1[0] /= nrm;
  t1[1] /= nrm;
  t1[2] /= nrm;
  t2[0] = n[1] * t1[2] - n[2] * t1[1];
  t2[1] = n[2] * t1[0] - n[0] * t1[2];
  t2[2] = n[0] * t1[1] - n[1] * t1[0];
}

template <class T>
inline void to_face_frame(const T n[3], const T t1[3], const T t2[3], const T s[5], T r[5], bool mirror) {
  r[0]       = s[0];
  const T mn = s[1] * n[0] + s[2] * n[1] + s[3] * n[2];
  r[1]       = mirror ? -(mn) : mn;
  r[2]       = s[1] * t1[0] + s[2] * t1[1] + s[3] * t1[2];
  r[3]       = s[1] * t2[0] + s[2] * t2[1] + s[3] * t2[2];
  r[4]       = s[4];
}

// ---------------------------------------------------------------------------
// HLLC (Toro, Spruce & Speares 1994; Toro, "Riemann Solvers ...", 3rd ed., eqs. 10.37-10.39, 10.71-10.73).
// NOT in the reference (its only approximate Riemann solver is the dead HLL above); the project brief
// names it, so it is offered as a third flux with the wave-speed estimates of that HLL (Roe averages and
// one-sided bounds, kernels.inl:296-304) and the contact restored. Checked by its defining properties
// (consistency, exact stationary / moving contacts, upwinding) in tests/test_oracle_golden.py.
// ---------------------------------------------------------------------------
template <class T>
inline void hllc_total_flux(const T uL[5], const T uR[5], T F[5], T* speed = nullptr) {
  const T zero = T(0), one = T(1), half = T(0.5);
  const T g = T(1.4);
  const T v1l = uL[1] / uL[0], v2l = uL[2] / uL[0], v3l = uL[3] / uL[0];
  const T kl  = half * (v1l * v1l + v2l * v2l + v3l * v3l);
  const T pl  = (g - one) * (uL[4] - uL[0] * kl);
  const T Hl  = (uL[4] + pl) / uL[0];
  const T cl  = std::sqrt((g - one) * (Hl - kl));
  const T v1r = uR[1] / uR[0], v2r = uR[2] / uR[0], v3r = uR[3] / uR[0];
  const T kr  = half * (v1r * v1r + v2r * v2r + v3r * v3r);
  const T pr  = (g - one) * (uR[4] - uR[0] * kr);
  const T Hr  = (uR[4] + pr) / uR[0];
  const T cr  = std::sqrt((g - one) * (Hr - kr));
  const T wl = std::sqrt(uL[0]), wr = std::sqrt(uR[0]);
  const T ws = wl + wr;
  const T v1 = (wl * v1l + wr * v1r) / ws, v2 = (wl * v2l + wr * v2r) / ws, v3 = (wl * v3l + wr * v3r) / ws;
  const T H  = (wl * Hl + wr * Hr) / ws;
  const T c  = std::sqrt((g - one) * (H - half * (v1 * v1 + v2 * v2 + v3 * v3)));
  const T Sl = std::min(v1 - c, v1l - cl), Sr = std::max(v1 + c, v1r + cr);
  if (speed) *speed = std::max(std::abs(Sl), std::abs(Sr));
  const T ml = uL[0] * (Sl - v1l), mr = uR[0] * (Sr - v1r);           // rho_K (S_K - u_K)
  const T Ss = ((pr - pl) + (uL[1] * (Sl - v1l) - uR[1] * (Sr - v1r))) / (ml - mr);
  const bool left = Ss >= zero;
  const T*   u  = left ? uL : uR;
  const T    S  = left ? std::min(Sl, zero) : std::max(Sr, zero);     // S_K, or 0 when that side is fully upwind
  const T    SK = left ? Sl : Sr, vn = left ? v1l : v1r, vt1 = left ? v2l : v2r, vt2 = left ? v3l : v3r;
  const T    p = left ? pl : pr, Hk = left ? Hl : Hr, m = left ? ml : mr;
  const T    fac = m / (SK - Ss);                                      // rho*_K
  const T    Us[5] = {fac, fac * Ss, fac * vt1, fac * vt2, fac * (u[4] / u[0] + (Ss - vn) * (Ss + p / m))};
  const T    Fk[5] = {u[1], u[1] * vn + p, u[1] * vt1, u[1] * vt2, u[1] * Hk};
  for (int k = 0; k < 5; k++) F[k] = Fk[k] + S * (Us[k] - u[k]);
}

enum FluxKind { KEPES = 0, HLL = 1, HLLC = 2 };

template <class T>
inline void face_frame_flux(int kind, const T a[5], const T b[5], T F[5], T* speed) {
  if (kind == HLL) {
    hll_total_flux<T>(a, b, F, speed);
  } else if (kind == HLLC) {
    hllc_total_flux<T>(a, b, F, speed);
  } else {
    kepes_total_flux<T>(a, b, F, speed);
  }
}

// ---------------------------------------------------------------------------
// SoA plane view: plane(step, var) = base + (step*5 + var) * stride
// (t8gpu/memory/shared_device_vector.inl:193-197, memory_manager.inl:73-80).
// ---------------------------------------------------------------------------
template <class T>
struct Planes {
  T*     base;
  size_t stride;
  T*     at(int step, int var) const { return base + (static_cast<size_t>(step) * 5 + var) * stride; }
};

#if defined(_OPENMP)
// ---------------------------------------------------------------------------
// OpenMP build only (liboracle_omp.so: the TIMED cpu_baseline of bench.py, never a parity reference). The face loops
// scatter +-F into two elements; instead of `omp atomic` on every addition (10 per face) each thread owns a range
// of elements -- the range its static chunk of faces lists as LEFT elements, which is contiguous because faces are
// listed by ascending left element (mesh_manager.inl:411-424) -- adds to its own elements directly and parks the few
// contributions to other threads' elements (faces next to a chunk boundary) in per-destination buckets that the
// owners add after a barrier. No atomics, deterministic for a given thread count; correct for any face order
// (a non-monotone list just parks more).
// ---------------------------------------------------------------------------
template <class T>
struct OwnerScatter {
  struct Parked {
    size_t idx;
    T      v[5];
  };
  int                                           nt;
  std::vector<int64_t>                          first;   // first[t] = first element owned by thread t; first[nt] = +inf
  std::vector<std::vector<std::vector<Parked>>> parked;  // [source thread][destination thread]

  // left(f) = left element of face f; F faces are split into nt static chunks
  template <class Left>
  OwnerScatter(int F, Left left) : nt(omp_get_max_threads()), first(nt + 1), parked(nt, std::vector<std::vector<Parked>>(nt)) {
    for (int t = 0; t < nt; t++) {
      const int64_t f0 = static_cast<int64_t>(F) * t / nt;
      first[t]         = (t == 0 || f0 >= F) ? (t == 0 ? INT64_MIN : INT64_MAX) : left(static_cast<int>(f0));
    }
    first[nt] = INT64_MAX;
    for (int t = nt - 1; t > 0; t--) first[t] = std::min(first[t], first[t + 1]);   // keep the bounds monotone
  }
  int owner(int64_t elem) const { return static_cast<int>(std::upper_bound(first.begin() + 1, first.end(), elem) - first.begin()) - 1; }
  void add(int t, int64_t elem, size_t idx, const T v[5], T sign, T* const flux[5]) {
    const int o = std::min(owner(elem), nt - 1);
    if (o == t) {
      for (int k = 0; k < 5; k++) flux[k][idx] += sign * v[k];
    } else {
      Parked p;
      p.idx = idx;
      for (int k = 0; k < 5; k++) p.v[k] = sign * v[k];
      parked[t][o].push_back(p);
    }
  }
  void drain(int t, T* const flux[5]) {   // call after `#pragma omp barrier`
    for (int src = 0; src < nt; src++)
      for (const Parked& p : parked[src][t])
        for (int k = 0; k < 5; k++) flux[k][p.idx] += p.v[k];
  }
};
#endif

// ---------------------------------------------------------------------------
// a4: interior faces of plain elements, kernels.cu:135-309. One iteration ==
// one CUDA thread. `indices` (nullable) is the element->slot map
// (get_element_owner_remote_index); the owner rank is ignored because the new
// backend resolves ghosts to local mirror slots. dim = number of
// stored normal components (2 or 3; missing ones are 0).
// plain order: scale by area BEFORE rotating back (kernels.cu:281-290).
// ---------------------------------------------------------------------------
template <class T>
void plain_interior_faces(int kind, int F, int dim, const int32_t* face_neighbors, const int32_t* indices,
                          const T* normals, const T* areas, const T* const state[5], T* const flux[5], T* speed) {
  // one face: gather, rotate, flux, scale by the area, rotate back (kernels.cu:160-290); returns l, r and the xyz flux
  auto face = [&](int i, int& l, int& r, T out[5]) {
    const T area = areas[i];
    l = face_neighbors[2 * i];
    r = face_neighbors[2 * i + 1];
    if (indices) {
      l = indices[l];
      r = indices[r];
    }
    T n[3] = {T(0), T(0), T(0)};
    for (int k = 0; k < dim; k++) n[k] = normals[static_cast<size_t>(dim) * i + k];
    T sl[5], sr[5];
    for (int k = 0; k < 5; k++) {
      sl[k] = state[k][l];
      sr[k] = state[k][r];
    }
    T t1[3], t2[3];
    face_basis<T>(n, t1, t2);
    T a[5], b[5], Ff[5];
    to_face_frame<T>(n, t1, t2, sl, a, false);
    to_face_frame<T>(n, t1, t2, sr, b, false);
    T spd = T(0);
    face_frame_flux<T>(kind, a, b, Ff, &spd);
    if (speed) speed[i] = spd;
    const T f0 = area * Ff[0], f1 = area * Ff[1], f2 = area * Ff[2], f3 = area * Ff[3], f4 = area * Ff[4];
    out[0] = f0;
    out[1] = f1 * n[0] + f2 * t1[0] + f3 * t2[0];
    out[2] = f1 * n[1] + f2 * t1[1] + f3 * t2[1];
    out[3] = f1 * n[2] + f2 * t1[2] + f3 * t2[2];
    out[4] = f4;
  };
#if defined(_OPENMP)
  OwnerScatter<T> scatter(F, [&](int f) { return static_cast<int64_t>(indices ? indices[face_neighbors[2 * f]] : face_neighbors[2 * f]); });
#pragma omp parallel
  {
    // chunk c of the faces (and the elements it owns) is handled by exactly one thread, whatever team size we got
    for (int c = omp_get_thread_num(); c < scatter.nt; c += omp_get_num_threads()) {
      const int f0 = static_cast<int>(static_cast<int64_t>(F) * c / scatter.nt), f1 = static_cast<int>(static_cast<int64_t>(F) * (c + 1) / scatter.nt);
      for (int i = f0; i < f1; i++) {
        int l, r;
        T   out[5];
        face(i, l, r, out);
        scatter.add(c, l, static_cast<size_t>(l), out, T(-1), flux);
        scatter.add(c, r, static_cast<size_t>(r), out, T(1), flux);
      }
    }
#pragma omp barrier
    for (int c = omp_get_thread_num(); c < scatter.nt; c += omp_get_num_threads()) scatter.drain(c, flux);
  }
#else
  for (int i = 0; i < F; i++) {
    int l, r;
    T   out[5];
    face(i, l, r, out);
    for (int k = 0; k < 5; k++) {
      flux[k][l] += -out[k];
      flux[k][r] += out[k];
    }
  }
#endif
}

// ---------------------------------------------------------------------------
// a5: reflective wall faces, kernels.cu:311-469. Boundary slices start after
// the F interior entries (t8gpu/mesh/mesh_manager.h:68-70,92-98,132-134).
// ---------------------------------------------------------------------------
template <class T>
void plain_boundary_faces(int kind, int F, int B, int dim, const int32_t* face_neighbors, const T* normals,
                          const T* areas, const T* const state[5], T* const flux[5], T* speed) {
  for (int i = 0; i < B; i++) {
    const T   area = areas[F + i];
    const int e    = face_neighbors[2 * static_cast<size_t>(F) + i];
    T         n[3] = {T(0), T(0), T(0)};
    for (int k = 0; k < dim; k++) n[k] = normals[static_cast<size_t>(dim) * (F + i) + k];
    T s[5];
    for (int k = 0; k < 5; k++) s[k] = state[k][e];
    T t1[3], t2[3];
    face_basis<T>(n, t1, t2);
    T a[5], b[5], Ff[5];
    to_face_frame<T>(n, t1, t2, s, a, false);
    to_face_frame<T>(n, t1, t2, s, b, true);
    T spd = T(0);
    face_frame_flux<T>(kind, a, b, Ff, &spd);
    if (speed) speed[F + i] = spd;
    const T f0 = area * Ff[0], f1 = area * Ff[1], f2 = area * Ff[2], f3 = area * Ff[3], f4 = area * Ff[4];
    const T fx = f1 * n[0] + f2 * t1[0] + f3 * t2[0];
    const T fy = f1 * n[1] + f2 * t1[1] + f3 * t2[1];
    const T fz = f1 * n[2] + f2 * t1[2] + f3 * t2[2];
    flux[0][e] += -f0;
    flux[1][e] += -fx;
    flux[2][e] += -fy;
    flux[3][e] += -fz;
    flux[4][e] += -f4;
  }
}

// ---------------------------------------------------------------------------
// a6: SSP-RK3 stage kernels for plain elements,
// t8gpu/timestepping/ssp_runge_kutta.inl:30-99. stage in {1,2,3}; `mid` is
// Step1 (stage 2) / Step2 (stage 3), unused for stage 1. Fluxes are zeroed.
// ---------------------------------------------------------------------------
template <class T>
void plain_rk_stage(int stage, int N, const T* const prev[5], const T* const mid[5], T* const out[5], T* const flux[5],
                    const T* volume, T dt) {
#if defined(_OPENMP)
#pragma omp parallel for schedule(static)
#endif
  for (int i = 0; i < N; i++) {
    for (int k = 0; k < 5; k++) {
      if (stage == 1) {
        out[k][i] = prev[k][i] + dt / volume[i] * flux[k][i];
      } else if (stage == 2) {
        out[k][i] = rk3<T>::c21 * prev[k][i] + rk3<T>::c22 * mid[k][i] + rk3<T>::c23 * dt / volume[i] * flux[k][i];
      } else {
        out[k][i] = rk3<T>::c31 * prev[k][i] + rk3<T>::c32 * mid[k][i] + rk3<T>::c33 * dt / volume[i] * flux[k][i];
      }
    }
    for (int k = 0; k < 5; k++) flux[k][i] = T(0.0);
  }
}

// ---------------------------------------------------------------------------
// a7: CompressibleEulerSolver::iterate, examples/compressible_euler/
// solver.cu:75-175. The caller has already swapped next/prev (solver.cu:76):
// `prev` holds the current solution, `next` receives the new one. Steps:
// 0..3 = Step0..Step3, 4 = Fluxes (solver.h:24-31); volume = plane 25.
// ---------------------------------------------------------------------------
template <class T>
void plain_iterate(int kind, int N, int F, int B, int dim, const int32_t* face_neighbors, const int32_t* indices,
                   const T* normals, const T* areas, Planes<T> P, int prev, int next, T dt, T* speed) {
  const int Step1 = 1, Step2 = 2, Fluxes = 4;
  const T*  vol   = P.base + static_cast<size_t>(25) * P.stride;
  const int src[3] = {prev, Step1, Step2};
  const int dst[3] = {Step1, Step2, next};
  for (int s = 0; s < 3; s++) {
    const T* st[5];
    T*       fl[5];
    for (int k = 0; k < 5; k++) {
      st[k] = P.at(src[s], k);
      fl[k] = P.at(Fluxes, k);
    }
    plain_interior_faces<T>(kind, F, dim, face_neighbors, indices, normals, areas, st, fl, speed);
    if (B > 0) plain_boundary_faces<T>(kind, F, B, dim, face_neighbors, normals, areas, st, fl, speed);
    const T* pv[5];
    const T* md[5];
    T*       ot[5];
    for (int k = 0; k < 5; k++) {
      pv[k] = P.at(prev, k);
      md[k] = P.at(src[s], k);
      ot[k] = P.at(dst[s], k);
    }
    plain_rk_stage<T>(s + 1, N, pv, md, ot, fl, vol, dt);
  }
}

// ===========================================================================
// Subgrid<4,4> / Subgrid<4,4,4>. In-block index flat = i + 4 j + 16 k
// (t8gpu/memory/subgrid_memory_manager.h:55-64), element-major e*S + flat
// (:88-90). E = 4 (cubic subgrids).
// ===========================================================================
constexpr int E = 4;

inline int sg_size(int rank) { return rank == 3 ? 64 : 16; }

// a13: compute_inner_fluxes, kernels.inl:335-662. Per direction the reference
// does `flux(c) -= sh[c]` (lanes with coord < 3) then `flux(c) += sh[c - 1]`
// (lanes with coord > 0) directly on the global flux planes; x, then y, then z.
// inner order: rotate back FIRST, then scale by surface (kernels.inl:395-401).
template <class T>
void subgrid_inner(int kind, int rank, int N, const T* const state[5], T* const flux[5], const T* volumes) {
  const int S = sg_size(rank);
#if defined(_OPENMP)
#pragma omp parallel for schedule(static)
#endif
  for (int e = 0; e < N; e++) {
    const T vol     = volumes[e];
    const T edge    = (rank == 3 ? std::cbrt(vol) : std::sqrt(vol)) / static_cast<T>(E);
    const T surface = rank == 3 ? edge * edge : edge;
    const size_t o  = static_cast<size_t>(e) * S;
    T            sh[5][64];
    for (int d = 0; d < rank; d++) {
      const int str = d == 0 ? 1 : (d == 1 ? 4 : 16);
      T         n[3] = {T(0.0), T(0.0), T(0.0)};
      n[d]           = T(1.0);
      T t1[3], t2[3];
      face_basis<T>(n, t1, t2);
      for (int c = 0; c < S; c++) {
        const int cd = (c / str) % E;
        for (int k = 0; k < 5; k++) sh[k][c] = T(0.0);
        if (cd < E - 1) {
          T sl[5], sr[5], a[5], b[5], Ff[5];
          for (int k = 0; k < 5; k++) {
            sl[k] = state[k][o + c];
            sr[k] = state[k][o + c + str];
          }
          to_face_frame<T>(n, t1, t2, sl, a, false);
          to_face_frame<T>(n, t1, t2, sr, b, false);
          face_frame_flux<T>(kind, a, b, Ff, nullptr);
          const T g[5] = {Ff[0], Ff[1] * n[0] + Ff[2] * t1[0] + Ff[3] * t2[0], Ff[1] * n[1] + Ff[2] * t1[1] + Ff[3] * t2[1],
                          Ff[1] * n[2] + Ff[2] * t1[2] + Ff[3] * t2[2], Ff[4]};
          for (int k = 0; k < 5; k++) sh[k][c] = g[k] * surface;
        }
      }
      for (int c = 0; c < S; c++) {
        const int cd = (c / str) % E;
        if (cd < E - 1)
          for (int k = 0; k < 5; k++) flux[k][o + c] -= sh[k][c];
        if (cd > 0)
          for (int k = 0; k < 5; k++) flux[k][o + c] += sh[k][c - str];
      }
    }
  }
}

// Sub-face -> cell maps of compute_outer_fluxes / compute_boundary_fluxes,
// kernels.inl:710-758 (3D) and :837-866 (2D). Anchors are selected by EXACT
// comparison of the stored normal against +-1.0.
template <class T>
inline void sg_face_cells(int rank, const T n[3], const int off[3], int double_stride, int i, int j, int lc[3],
                          int rc[3]) {
  int al[3] = {0, 0, 0}, si[3] = {0, 0, 0}, sj[3] = {0, 0, 0};
  if (rank == 3) {
    if (n[0] == 1.0) { al[0] = E - 1; si[1] = 1; sj[2] = 1; }
    if (n[0] == -1.0) { si[1] = 1; sj[2] = 1; }
    if (n[1] == 1.0) { al[1] = E - 1; si[0] = 1; sj[2] = 1; }
    if (n[1] == -1.0) { si[0] = 1; sj[2] = 1; }
    if (n[2] == 1.0) { al[2] = E - 1; si[0] = 1; sj[1] = 1; }
    if (n[2] == -1.0) { si[0] = 1; sj[1] = 1; }
  } else {
    if (n[0] == 1.0) { al[0] = E - 1; si[1] = 1; }
    if (n[0] == -1.0) { si[1] = 1; }
    if (n[1] == 1.0) { al[1] = E - 1; si[0] = 1; }
    if (n[1] == -1.0) { si[0] = 1; }
  }
  for (int d = 0; d < 3; d++) {
    lc[d] = al[d] + i * si[d] + j * sj[d];
    rc[d] = off[d] + double_stride * (i * si[d] + j * sj[d]) / 2;
  }
}

// a14: compute_outer_fluxes, kernels.inl:664-911. One outer iteration == one
// CUDA block (coarse face), inner (j, i) == threads. `indices` as for plain.
template <class T>
void subgrid_outer(int kind, int rank, int F, const int32_t* face_neighbors, const int32_t* indices,
                   const int32_t* level_diff, const int32_t* nb_offset, const T* normals, const T* areas,
                   const T* const state[5], T* const flux[5]) {
  const int S  = sg_size(rank);
  const int nj = rank == 3 ? E : 1;
  auto left_of = [&](int f) { return static_cast<int64_t>(indices ? indices[face_neighbors[2 * static_cast<size_t>(f)]] : face_neighbors[2 * static_cast<size_t>(f)]); };
  // one coarse face = one CUDA block of the reference; emit(block, cell index, flux, sign) receives every contribution
  auto coarse_face = [&](int f, auto&& emit) {
    const int ds     = (level_diff[f] == 0) ? 2 : 1;
    int       off[3] = {0, 0, 0};
    for (int d = 0; d < rank; d++) off[d] = nb_offset[static_cast<size_t>(rank) * f + d];
    int l = face_neighbors[2 * static_cast<size_t>(f)], r = face_neighbors[2 * static_cast<size_t>(f) + 1];
    if (indices) {
      l = indices[l];
      r = indices[r];
    }
    T n[3] = {T(0), T(0), T(0.0)};
    for (int d = 0; d < rank; d++) n[d] = normals[static_cast<size_t>(rank) * f + d];
    T t1[3], t2[3];
    face_basis<T>(n, t1, t2);
    const T surface = areas[f] / static_cast<T>(rank == 3 ? E * E : E);
    for (int j = 0; j < nj; j++)
      for (int i = 0; i < E; i++) {
        int lc[3], rc[3];
        sg_face_cells<T>(rank, n, off, ds, i, j, lc, rc);
        const size_t li = static_cast<size_t>(l) * S + lc[0] + 4 * lc[1] + 16 * lc[2];
        const size_t ri = static_cast<size_t>(r) * S + rc[0] + 4 * rc[1] + 16 * rc[2];
        T            sl[5], sr[5], a[5], b[5], Ff[5];
        for (int k = 0; k < 5; k++) {
          sl[k] = state[k][li];
          sr[k] = state[k][ri];
        }
        to_face_frame<T>(n, t1, t2, sl, a, false);
        to_face_frame<T>(n, t1, t2, sr, b, false);
        face_frame_flux<T>(kind, a, b, Ff, nullptr);
        const T g[5] = {Ff[0], Ff[1] * n[0] + Ff[2] * t1[0] + Ff[3] * t2[0], Ff[1] * n[1] + Ff[2] * t1[1] + Ff[3] * t2[1],
                        Ff[1] * n[2] + Ff[2] * t1[2] + Ff[3] * t2[2], Ff[4]};
        const T gs[5] = {g[0] * surface, g[1] * surface, g[2] * surface, g[3] * surface, g[4] * surface};
        emit(l, li, gs, T(-1));
        emit(r, ri, gs, T(1));
      }
  };
#if defined(_OPENMP)
  OwnerScatter<T> scatter(F, left_of);
#pragma omp parallel
  {
    for (int c = omp_get_thread_num(); c < scatter.nt; c += omp_get_num_threads()) {
      const int f0 = static_cast<int>(static_cast<int64_t>(F) * c / scatter.nt), f1 = static_cast<int>(static_cast<int64_t>(F) * (c + 1) / scatter.nt);
      for (int f = f0; f < f1; f++)
        coarse_face(f, [&](int block, size_t idx, const T v[5], T sign) { scatter.add(c, block, idx, v, sign, flux); });
    }
#pragma omp barrier
    for (int c = omp_get_thread_num(); c < scatter.nt; c += omp_get_num_threads()) scatter.drain(c, flux);
  }
#else
  (void)left_of;
  for (int f = 0; f < F; f++)
    coarse_face(f, [&](int, size_t idx, const T v[5], T sign) {
      for (int k = 0; k < 5; k++) flux[k][idx] += sign * v[k];
    });
#endif
}

// a15: compute_boundary_fluxes, kernels.inl:913-1107 (reflect_state on the right).
template <class T>
void subgrid_boundary(int kind, int rank, int F, int B, const int32_t* face_neighbors, const T* normals,
                      const T* areas, const T* const state[5], T* const flux[5]) {
  const int S  = sg_size(rank);
  const int nj = rank == 3 ? E : 1;
  for (int f = 0; f < B; f++) {
    const int e    = face_neighbors[2 * static_cast<size_t>(F) + f];
    T         n[3] = {T(0), T(0), T(0.0)};
    for (int d = 0; d < rank; d++) n[d] = normals[static_cast<size_t>(rank) * (F + f) + d];
    T t1[3], t2[3];
    face_basis<T>(n, t1, t2);
    const T   surface = areas[F + f] / static_cast<T>(rank == 3 ? E * E : E);
    const int off[3]  = {0, 0, 0};
    for (int j = 0; j < nj; j++)
      for (int i = 0; i < E; i++) {
        int lc[3], rc[3];
        sg_face_cells<T>(rank, n, off, 2, i, j, lc, rc);
        const size_t li = static_cast<size_t>(e) * S + lc[0] + 4 * lc[1] + 16 * lc[2];
        T            s[5], a[5], b[5], Ff[5];
        for (int k = 0; k < 5; k++) s[k] = state[k][li];
        to_face_frame<T>(n, t1, t2, s, a, false);
        to_face_frame<T>(n, t1, t2, s, b, true);
        face_frame_flux<T>(kind, a, b, Ff, nullptr);
        const T g[5] = {Ff[0], Ff[1] * n[0] + Ff[2] * t1[0] + Ff[3] * t2[0], Ff[1] * n[1] + Ff[2] * t1[1] + Ff[3] * t2[1],
                        Ff[1] * n[2] + Ff[2] * t1[2] + Ff[3] * t2[2], Ff[4]};
        for (int k = 0; k < 5; k++) flux[k][li] += -g[k] * surface;
      }
  }
}

// a16: subgrid RK stages, ssp_runge_kutta.inl:101-221 (volume = volumes[e] / S).
template <class T>
void subgrid_rk_stage(int stage, int rank, int N, const T* const prev[5], const T* const mid[5], T* const out[5],
                      T* const flux[5], const T* volumes, T dt) {
  const int S = sg_size(rank);
#if defined(_OPENMP)
#pragma omp parallel for schedule(static)
#endif
  for (int e = 0; e < N; e++) {
    const T volume = volumes[e] / static_cast<T>(S);
    for (int c = 0; c < S; c++) {
      const size_t i = static_cast<size_t>(e) * S + c;
      for (int k = 0; k < 5; k++) {
        if (stage == 1) {
          out[k][i] = prev[k][i] + dt / volume * flux[k][i];
        } else if (stage == 2) {
          out[k][i] = rk3<T>::c21 * prev[k][i] + rk3<T>::c22 * mid[k][i] + rk3<T>::c23 * dt / volume * flux[k][i];
        } else {
          out[k][i] = rk3<T>::c31 * prev[k][i] + rk3<T>::c32 * mid[k][i] + rk3<T>::c33 * dt / volume * flux[k][i];
        }
        flux[k][i] = T(0.0);
      }
    }
  }
}

// a17: SubgridCompressibleEulerSolver::iterate, examples/subgrid/solver.inl:152-266
// (inner -> boundary -> outer -> RK, three times). Caller swapped prev/next (:154).
// Variable planes have stride `P.stride` in SUBCELLS; volumes is a separate
// per-block vector (subgrid_memory_manager.h:553-554).
template <class T>
void subgrid_iterate(int kind, int rank, int N, int F, int B, const int32_t* face_neighbors, const int32_t* indices,
                     const int32_t* level_diff, const int32_t* nb_offset, const T* normals, const T* areas,
                     Planes<T> P, const T* volumes, int prev, int next, T dt) {
  const int Step1 = 1, Step2 = 2, Fluxes = 4;
  const int src[3] = {prev, Step1, Step2};
  const int dst[3] = {Step1, Step2, next};
  for (int s = 0; s < 3; s++) {
    const T* st[5];
    T*       fl[5];
    const T* pv[5];
    T*       ot[5];
    for (int k = 0; k < 5; k++) {
      st[k] = P.at(src[s], k);
      fl[k] = P.at(Fluxes, k);
      pv[k] = P.at(prev, k);
      ot[k] = P.at(dst[s], k);
    }
    subgrid_inner<T>(kind, rank, N, st, fl, volumes);
    if (B > 0) subgrid_boundary<T>(kind, rank, F, B, face_neighbors, normals, areas, st, fl);
    subgrid_outer<T>(kind, rank, F, face_neighbors, indices, level_diff, nb_offset, normals, areas, st, fl);
    subgrid_rk_stage<T>(s + 1, rank, N, pv, st, ot, fl, volumes, dt);
  }
}

// ===========================================================================
// AMR indicator and data transfer (plain elements).
// ===========================================================================
// estimate_gradient, examples/compressible_euler/kernels.cu:471-501.
template <class T>
void estimate_gradient(int F, const int32_t* fn, const int32_t* indices, const T* rho, T* gradient) {
  for (int i = 0; i < F; i++) {
    int l = fn[2 * static_cast<size_t>(i)], r = fn[2 * static_cast<size_t>(i) + 1];
    if (indices) {
      l = indices[l];
      r = indices[r];
    }
    const T g = std::abs(rho[r] - rho[l]);
    gradient[l] += g;
    gradient[r] += g;
  }
}

// compute_refinement_criteria, examples/compressible_euler/solver.cu:231-241.
template <class T>
void refinement_criteria(int N, const T* gradient, const T* volume, T* criteria) {
  for (int i = 0; i < N; i++) criteria[i] = gradient[i] / std::cbrt(volume[i]);
}

// adapt_variables_and_volume, t8gpu/mesh/mesh_manager.inl:165-193. The reference's factors are
// 0.125 / 8.0 whatever the dimension (dim = 3 here); dim = 2 uses 0.25 / 4.0.
template <class T>
void adapt_variables_and_volume(int n_new, int dim, const int32_t* adapt_data, const T* const old_v[5], T* const new_v[5],
                                const T* vol_old, T* vol_new) {
  const T down = dim == 3 ? T(0.125) : T(0.25), up = dim == 3 ? T(8.0) : T(4.0);
  for (int i = 0; i < n_new; i++) {
    const int diff = adapt_data[i + 1] - adapt_data[i];
    const int nsum = std::max(1, diff);
    vol_new[i]     = vol_old[adapt_data[i]] * (diff == 0 ? down : (diff == 1 ? T(1.0) : up));
    if (i > 0 && adapt_data[i - 1] == adapt_data[i]) vol_new[i] = vol_old[adapt_data[i]] * down;
    for (int k = 0; k < 5; k++) {
      new_v[k][i] = T(0.0);
      for (int j = 0; j < nsum; j++) new_v[k][i] += old_v[k][adapt_data[i] + j] / static_cast<T>(nsum);
    }
  }
}

// compute_refinement_criteria<Subgrid>, examples/subgrid/kernels.inl:1110-1168.
template <class T>
void subgrid_refinement_criteria(int rank, int N, const T* rho, const T* volumes, T* criteria) {
  const int S = sg_size(rank), nz = rank == 3 ? E : 1;
  for (int e = 0; e < N; e++) {
    const T* d   = rho + static_cast<size_t>(e) * S;
    const T  h   = (rank == 3 ? std::cbrt(volumes[e]) : std::sqrt(volumes[e])) / static_cast<T>(E);
    T        acc = T{0.0};
    for (int p = 0; p < E - 1; p++)
      for (int q = 0; q < E; q++)
        for (int r = 0; r < nz; r++) acc += (d[p + 1 + 4 * q + 16 * r] - d[p + 4 * q + 16 * r]) * (d[p + 1 + 4 * q + 16 * r] - d[p + 4 * q + 16 * r]) * h;
    for (int p = 0; p < E; p++)
      for (int q = 0; q < E - 1; q++)
        for (int r = 0; r < nz; r++) acc += (d[p + 4 * (q + 1) + 16 * r] - d[p + 4 * q + 16 * r]) * (d[p + 4 * (q + 1) + 16 * r] - d[p + 4 * q + 16 * r]) * h;
    if (rank == 3)
      for (int p = 0; p < E; p++)
        for (int q = 0; q < E; q++)
          for (int r = 0; r < E - 1; r++) acc += (d[p + 4 * q + 16 * (r + 1)] - d[p + 4 * q + 16 * r]) * (d[p + 4 * q + 16 * (r + 1)] - d[p + 4 * q + 16 * r]) * h;
    criteria[e] = acc / volumes[e];
  }
}

// adapt_volume + adapt_variables for subgrids, t8gpu/mesh/subgrid_mesh_manager.inl:246-425.
template <class T>
void subgrid_adapt_variables_and_volume(int rank, int n_new, const int32_t* adapt_data, const T* const old_v[5], T* const new_v[5],
                                        const T* vol_old, T* vol_new) {
  const int S = sg_size(rank);
  const T   down = rank == 3 ? T(0.125) : T(0.25), up = rank == 3 ? T(8.0) : T(4.0);
  for (int e = 0; e < n_new; e++) {
    const int diff = adapt_data[e + 1] - adapt_data[e];
    vol_new[e]     = vol_old[adapt_data[e]] * (diff == 0 ? down : (diff == 1 ? T(1.0) : up));
    if (e > 0 && adapt_data[e - 1] == adapt_data[e]) vol_new[e] = vol_old[adapt_data[e]] * down;
    for (int c = 0; c < S; c++) {
      const int    i = c & 3, j = (c >> 2) & 3, k = rank == 3 ? c >> 4 : 0;
      const size_t dst = static_cast<size_t>(e) * S + c;
      if (diff == 0 || (e > 0 && adapt_data[e] == adapt_data[e - 1])) {
        int refinement_index = 0;
        while (e - refinement_index >= 0 && adapt_data[e - refinement_index] == adapt_data[e]) refinement_index++;
        const int I = (refinement_index - 1) & 1, J = ((refinement_index - 1) >> 1) & 1, K = ((refinement_index - 1) >> 2) & 1;
        const size_t src = static_cast<size_t>(adapt_data[e]) * S + (I * 2 + i / 2) + 4 * (J * 2 + j / 2) + (rank == 3 ? 16 * (K * 2 + k / 2) : 0);
        for (int l = 0; l < 5; l++) new_v[l][dst] = old_v[l][src];
      } else if (diff > 1) {
        const int    z   = (i >> 1) | ((j >> 1) << 1) | (rank == 3 ? (k >> 1) << 2 : 0);
        const size_t blk = static_cast<size_t>(adapt_data[e] + z) * S;
        for (int l = 0; l < 5; l++) {
          new_v[l][dst] = T(0.0);
          for (int ii = 0; ii < 2; ii++)
            for (int jj = 0; jj < 2; jj++)
              for (int kk = 0; kk < (rank == 3 ? 2 : 1); kk++)
                new_v[l][dst] += old_v[l][blk + (2 * (i & 1) + ii) + 4 * (2 * (j & 1) + jj) + (rank == 3 ? 16 * (2 * (k & 1) + kk) : 0)];
          new_v[l][dst] /= static_cast<T>(1 << rank);
        }
      } else {
        for (int l = 0; l < 5; l++) new_v[l][dst] = old_v[l][static_cast<size_t>(adapt_data[e]) * S + c];
      }
    }
  }
}

}  // namespace oracle
