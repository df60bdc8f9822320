// plain_fused_body.inc -- the body of the generic fused tile kernels k_plain_fused and k_plain_fused_far (kernels_fused.hip),
// included inside both. Not a device function: a kernel that hands its parameters to one gets different code (more SGPRs)
// than the same statements in its own body, and k_plain_fused keeps the code it has always had.
// In scope: the kernel parameters (P, tile_begin, prev, src, out, vol, dt, speed) and the compile-time T, KIND, STAGE, OPEN
// (the plan has outflow / inflow faces: fused_common.hpp: decode_face_side) and FAR (with OPEN: far-field faces too,
// fused_common.hpp: farfield_prim / farfield_state).
  extern __shared__ double lds_raw[];
  T* const      lds = reinterpret_cast<T*>(lds_raw);
  constexpr int NW  = KIND == 0 ? kPrimWords : 5;  // words per element kept in LDS
  const int     LE  = plan_slots(P);                 // element slots per LDS plane
  const int     LF  = P.max_faces;
  T* const      pe  = lds;                         // [NW][LE]
  T* const      ff  = lds + (size_t)NW * LE;       // [5][LF]
  constexpr bool kTab = sizeof(T) == 8 && KIND == 0;   // fp64 KEPES: table-driven logarithms (flux_math.hpp: t8_log_tab)
  double* const lt  = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(ff + (size_t)5 * LF) + 15) & ~uintptr_t(15));   // 16-byte rows
  if (kTab) {
    lt[threadIdx.x] = kLogTab[threadIdx.x];
    __syncthreads();
  }

  const int tile = P.tile_order[tile_begin + xcd_position(blockIdx.x, gridDim.x)];
  const int e0 = P.elem_off[tile], ne = P.elem_off[tile + 1] - e0;
  const int h0 = P.halo_off[tile], nh = P.halo_off[tile + 1] - h0;
  const int f0 = P.face_off[tile], nf = P.face_off[tile + 1] - f0;
  const int tid = threadIdx.x;

  // ---- phase 1: elements -> LDS --------------------------------------------------------------
  for (int i = tid; i < ne + nh; i += 256) {
    const int slot = i < ne ? e0 + i : P.halo_ids[h0 + (i - ne)];
    T         s[5];
    if (P.ghost_buf) {
#pragma unroll
      for (int k = 0; k < 5; k++) s[k] = ghost_window_load<T>(P, src, slot, k);
    } else {
#pragma unroll
      for (int k = 0; k < 5; k++) s[k] = src.p[k][slot];
    }
    if (KIND == 0) {
      const Prim<T> q = prim_from_state<T, kTab>(s, lt);
      pe[0 * LE + i]  = q.rho;
      pe[1 * LE + i]  = q.vx;
      pe[2 * LE + i]  = q.vy;
      pe[3 * LE + i]  = q.vz;
      pe[4 * LE + i]  = q.p;
      pe[5 * LE + i]  = q.beta;
      pe[6 * LE + i]  = q.lrho;
      pe[7 * LE + i]  = q.lbeta;
      pe[8 * LE + i]  = q.v0;
    } else {
#pragma unroll
      for (int k = 0; k < 5; k++) pe[k * LE + i] = s[k];
    }
  }
  __syncthreads();

  // ---- phase 2: faces -----------------------------------------------------------------------
  using V4 = typename vec4<T>::type;
  const V4* __restrict__ geo = reinterpret_cast<const V4*>(P.face_geo) + f0;
  for (int f = tid; f < nf; f += 256) {
    const uint32_t lr = P.face_lr[f0 + f];
    const V4       gm = geo[f];
    const int      l = lr & 0xFFFFu, r16 = lr >> 16;
    bool           wall;
    int            r, inflow = -1, far = -1;
    if constexpr (OPEN) {
      const FaceSide fs = decode_face_side<FAR>(l, r16);
      wall   = fs.wall;
      r      = fs.r;
      inflow = fs.inflow;
      far    = fs.far;
    } else {
      wall = r16 == 0xFFFFu;
      r    = wall ? l : r16;
    }
    const T        n[3] = {gm.x, gm.y, gm.z};
    T              t1[3], t2[3], g[5], spd = T(0);
    face_basis_fast<T>(n, t1, t2);
    if (KIND == 0) {
      Prim<T> L, R;
      L.rho = pe[0 * LE + l]; L.vx = pe[1 * LE + l]; L.vy = pe[2 * LE + l]; L.vz = pe[3 * LE + l]; L.p = pe[4 * LE + l];
      L.beta = pe[5 * LE + l]; L.lrho = pe[6 * LE + l]; L.lbeta = pe[7 * LE + l]; L.v0 = pe[8 * LE + l];
      R.rho = pe[0 * LE + r]; R.vx = pe[1 * LE + r]; R.vy = pe[2 * LE + r]; R.vz = pe[3 * LE + r]; R.p = pe[4 * LE + r];
      R.beta = pe[5 * LE + r]; R.lrho = pe[6 * LE + r]; R.lbeta = pe[7 * LE + r]; R.v0 = pe[8 * LE + r];
      if (OPEN && inflow >= 0) inflow_prim<T>(P, inflow, R);
      if (FAR && far >= 0) farfield_prim<T, kTab>(inflow_entry<T>(P, far), n, lt, R);
      kepes_prim<T>(L, R, wall, n, t1, t2, gm.w, g, spd);
    } else {
      T sl[5], sr[5];
#pragma unroll
      for (int k = 0; k < 5; k++) {
        sl[k] = pe[k * LE + l];
        sr[k] = pe[k * LE + r];
      }
      if (OPEN && inflow >= 0) {
        const T* q = inflow_entry<T>(P, inflow);
#pragma unroll
        for (int k = 0; k < 5; k++) sr[k] = q[k];
      }
      if (FAR && far >= 0) farfield_state<T>(inflow_entry<T>(P, far), n, sr);
      hll_face<T>(sl, sr, wall, n, t1, t2, gm.w, g, spd, KIND == 2);
    }
    if (speed) {
      const int orig = P.face_orig[f0 + f];
      if (orig >= 0) speed[orig] = spd;
    }
#pragma unroll
    for (int k = 0; k < 5; k++) ff[k * LF + f] = g[k];
  }
  __syncthreads();

  // ---- phase 3: per-element sum + RK stage (ssp_runge_kutta.inl:30-99) ---------------------------
  for (int i = tid; i < ne; i += 256) {
    const int e  = e0 + i;
    const int c0 = P.csr_off[e], c1 = P.csr_off[e + 1];
    T         acc[5] = {T(0), T(0), T(0), T(0), T(0)};
    for (int c = c0; c < c1; c++) {
      const unsigned ent = P.csr_ent[c];
      const int      f   = ent & 0x7FFFu;
      if (ent & 0x8000u) {
#pragma unroll
        for (int k = 0; k < 5; k++) acc[k] += ff[k * LF + f];
      } else {
#pragma unroll
        for (int k = 0; k < 5; k++) acc[k] -= ff[k * LF + f];
      }
    }
    const T scale = dt / vol[e];
    T       res[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
      // (stage 1: prev is the stage's source state, plain_fused_stage() checks it)
      res[k] = rk_stage_update<T, STAGE>(prev.p[k][e], STAGE == 1 ? prev.p[k][e] : src.p[k][e], scale, acc[k]);
      out.p[k][e] = res[k];
    }
    if (P.send_map) ghost_window_send<T>(P, e, res);
  }
