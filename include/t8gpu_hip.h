/* t8gpu_hip.h -- C ABI of the MI355X (gfx950) backend for t8gpu's finite-volume hot path.
 *
 * t8gpu itself has no FFI: its boundary is the C++ template API of t8gpu/ (see include/t8gpu/ for
 * the HIP-backed mirror of those headers). This C ABI is what those headers -- or any other host
 * language -- bind to reach the hand-written HIP kernels. Every entry point names the reference
 * kernel / function it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - suffix _f32 / _f64 selects float_type (reference: t8gpu/memory/memory_manager.h:29, float only).
 *   - all pointers are DEVICE pointers unless the name says host; `stream` is a hipStream_t (NULL =
 *     default stream). Calls are asynchronous on that stream and safe to capture in a hipGraph.
 *   - T8gpuVars_*: the 5 variable planes of one step, exactly the pointers a
 *     MemoryAccessorOwn<VariableList> holds (memory_manager.h:173): Rho, Rho_v1, Rho_v2, Rho_v3, Rho_e.
 *   - ghosts: element indices refer to local slots; ghost elements live in mirror slots [N, N+G)
 *     of the same planes. `indices` (nullable) is the element->slot map of
 *     MeshConnectivityAccessor::get_element_owner_remote_index (mesh_manager.h:155-157).
 *   - return value: 0 on success, otherwise the hipError_t (or ncclResult_t + 10000) code; the C++
 *     wrappers turn non-zero into the reference's print-and-abort (t8gpu/utils/cuda.h:7-15).
 *   - flux_kind: 0 = KEPES (the flux the reference runs), 1 = HLL (reference dead code,
 *     examples/subgrid/kernels.inl:263-332), 2 = HLLC (NOT in the reference: the project brief names it; the HLL
 *     above with the contact wave restored, same wave-speed estimates; oracle/oracle.hpp states the formulas).
 */
#ifndef T8GPU_HIP_H
#define T8GPU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T8GPU_FLUX_KEPES 0
#define T8GPU_FLUX_HLL 1
#define T8GPU_FLUX_HLLC 2

typedef struct T8gpuVars_f32 { float* p[5]; } T8gpuVars_f32;
typedef struct T8gpuVars_f64 { double* p[5]; } T8gpuVars_f64;

/* ---- library / device ------------------------------------------------------------------------ */
int         t8gpu_hip_abi_version(void);
int         t8gpu_hip_device_count(int* count);
int         t8gpu_hip_set_device(int device);
const char* t8gpu_hip_error_string(int code);
/* roctx ranges for `rocprofv3 --marker-trace`: active only with T8GPU_ROCTX=1 in the environment
 * (the roctx library is dlopen'ed then); both return 1 when a range was pushed / popped, 0 when ranges are off. The
 * step drivers mark iterate_steps and every RK stage themselves. */
int         t8gpu_hip_range_push(const char* name);
int         t8gpu_hip_range_pop(void);
/* Name of the kernel the most recent t8gpu_hip_*_fused_stage_* call launched for the bulk of its tiles / blocks, spelled as
 * rocprofv3 prints it (e.g. "k_plain_stage<double, 0, 3>"); "" before the first call. bench.py compares it with the kernels
 * named by the committed profile before it reports that profile's PMC figures. Not thread-safe (one host thread per rank). */
const char* t8gpu_hip_last_stage_kernel(void);
/* The grid of that launch in workgroups (ABI 16; 0 before the first call), and launch `index` (0, 1, ... in launch order; at
 * most the first 8) of the same call: its kernel name and, through `workgroups` (nullable), its grid; NULL past the call's
 * last launch. Per host thread, like the name. */
int         t8gpu_hip_last_stage_workgroups(void);
const char* t8gpu_hip_last_stage_launch(int index, int* workgroups);
/* A limit on the resident workgroups of the persistent launches, FOR TESTS (ABI 16): the persistent kernels (k_plain_persistent,
 * k_plain_patch / k_plain_stage, k_plain_patch3 / k_plain_patch3_both) size their grid as min(tiles, resident) with resident =
 * compute units x workgroups per CU -- hundreds -- so only meshes of benchmark size make a workgroup walk several tiles. With a
 * limit of `workgroups` > 0 every launcher takes resident = min(compute units x workgroups per CU, workgroups), in its grid and
 * in every decision that compares a tile count with the resident workgroups (the persistent tile kernel's size rule: a plan of
 * at least 8 x limit generic tiles takes it; the chunked patch walk; k_plain_patch3_both, which needs a limit >= 16 that is a
 * multiple of 8 and declines any other). 0 (the default): none -- no launch changes. Returns the previous value. Process-wide
 * and atomic, read at launch time: it holds for the launches enqueued after the call, from any host thread. A captured graph
 * keeps the grid it was captured with. t8gpu_hip_plain_persistent_accepts answers under the limit as well: plan while it is 0. */
int         t8gpu_hip_set_resident_limit(int workgroups);

/* ---- plain elements, reference-dataflow kernels ("compat" tier) ------------------------------- */

/* kepes_compute_fluxes<<<ceil(F/256),256>>>, examples/compressible_euler/kernels.cu:135-309
 * (declared kernels.h:22-27). face_neighbors = [2F] (l,r) pairs, face_normals = [normal_dim*F] AoS,
 * face_surfaces = [F]; scatter-adds -F to l and +F to r; speed_estimates[F] may be NULL. */
int t8gpu_hip_flux_faces_f32(int flux_kind, int num_faces, int normal_dim, const int32_t* face_neighbors,
                             const int32_t* indices, const float* face_normals, const float* face_surfaces,
                             T8gpuVars_f32 state, T8gpuVars_f32 fluxes, float* speed_estimates, void* stream);
int t8gpu_hip_flux_faces_f64(int flux_kind, int num_faces, int normal_dim, const int32_t* face_neighbors,
                             const int32_t* indices, const double* face_normals, const double* face_surfaces,
                             T8gpuVars_f64 state, T8gpuVars_f64 fluxes, double* speed_estimates, void* stream);

/* reflective_boundary_condition<<<ceil(B/256),256>>>, kernels.cu:311-469 (kernels.h:39-44). The
 * arrays are the SAME arrays as above; boundary entries start after the F interior ones
 * (t8gpu/mesh/mesh_manager.h:68-70,92-98,132-134). speed_estimates[F + i] written if non-NULL. */
int t8gpu_hip_flux_boundary_f32(int flux_kind, int num_faces, int num_boundary_faces, int normal_dim,
                                const int32_t* face_neighbors, const float* face_normals,
                                const float* face_surfaces, T8gpuVars_f32 state, T8gpuVars_f32 fluxes,
                                float* speed_estimates, void* stream);
int t8gpu_hip_flux_boundary_f64(int flux_kind, int num_faces, int num_boundary_faces, int normal_dim,
                                const int32_t* face_neighbors, const double* face_normals,
                                const double* face_surfaces, T8gpuVars_f64 state, T8gpuVars_f64 fluxes,
                                double* speed_estimates, void* stream);
/* The boundary faces with their kinds (t8gpu_host.h: boundary_kinds[B], device copy): walls as above; outflow faces evaluate
 * the interior face flux with the outside state = the inside one; inflow faces with the outside state = the conservative
 * state k of `inflow_table` (t8gpu_hip_plain_inflow_table_*; may be NULL when no face is an inflow or far-field face);
 * far-field faces (ABI 11) with the outside state of the characteristic condition against state k.
 * boundary_kinds = NULL is t8gpu_hip_flux_boundary_*. */
int t8gpu_hip_flux_boundary_bc_f32(int flux_kind, int num_faces, int num_boundary_faces, int normal_dim,
                                   const int32_t* face_neighbors, const uint8_t* boundary_kinds, const float* inflow_table,
                                   const float* face_normals, const float* face_surfaces, T8gpuVars_f32 state,
                                   T8gpuVars_f32 fluxes, float* speed_estimates, void* stream);
int t8gpu_hip_flux_boundary_bc_f64(int flux_kind, int num_faces, int num_boundary_faces, int normal_dim,
                                   const int32_t* face_neighbors, const uint8_t* boundary_kinds, const double* inflow_table,
                                   const double* face_normals, const double* face_surfaces, T8gpuVars_f64 state,
                                   T8gpuVars_f64 fluxes, double* speed_estimates, void* stream);

/* timestepping::SSP_3RK_step{1,2,3}<V><<<ceil(N/256),256>>>, t8gpu/timestepping/ssp_runge_kutta.inl:30-99.
 * stage 1: out = prev + dt/vol*f;  stage 2: out = .75 prev + .25 mid + .25 dt/vol*f;
 * stage 3: out = c31 prev + c32 mid + c33 dt/vol*f (truncated literals, :12-14,23-25); f := 0. */
int t8gpu_hip_rk3_stage_f32(int stage, int num_elements, T8gpuVars_f32 prev, T8gpuVars_f32 mid, T8gpuVars_f32 out,
                            T8gpuVars_f32 fluxes, const float* volume, float delta_t, void* stream);
int t8gpu_hip_rk3_stage_f64(int stage, int num_elements, T8gpuVars_f64 prev, T8gpuVars_f64 mid, T8gpuVars_f64 out,
                            T8gpuVars_f64 fluxes, const double* volume, double delta_t, void* stream);

/* ---- Subgrid<4,4> (rank 2) and Subgrid<4,4,4> (rank 3), reference-dataflow kernels ------------- */

/* compute_inner_fluxes<Subgrid><<<N, block_size>>>, examples/subgrid/kernels.inl:335-662. */
int t8gpu_hip_subgrid_inner_f32(int flux_kind, int rank, int num_elements, T8gpuVars_f32 state, T8gpuVars_f32 fluxes,
                                const float* volumes, void* stream);
int t8gpu_hip_subgrid_inner_f64(int flux_kind, int rank, int num_elements, T8gpuVars_f64 state, T8gpuVars_f64 fluxes,
                                const double* volumes, void* stream);

/* compute_outer_fluxes<Subgrid><<<F, (4,4)|(4)>>>, kernels.inl:664-911. face_level_difference[F],
 * face_neighbor_offset[rank*F] as in t8gpu/mesh/subgrid_mesh_manager.h:108-126. */
int t8gpu_hip_subgrid_outer_f32(int flux_kind, int rank, int num_faces, const int32_t* face_neighbors,
                                const int32_t* indices, const int32_t* face_level_difference,
                                const int32_t* face_neighbor_offset, const float* face_normals,
                                const float* face_surfaces, T8gpuVars_f32 state, T8gpuVars_f32 fluxes, void* stream);
int t8gpu_hip_subgrid_outer_f64(int flux_kind, int rank, int num_faces, const int32_t* face_neighbors,
                                const int32_t* indices, const int32_t* face_level_difference,
                                const int32_t* face_neighbor_offset, const double* face_normals,
                                const double* face_surfaces, T8gpuVars_f64 state, T8gpuVars_f64 fluxes, void* stream);

/* compute_boundary_fluxes<Subgrid><<<B, (4,4)|(4)>>>, kernels.inl:913-1107. */
int t8gpu_hip_subgrid_boundary_f32(int flux_kind, int rank, int num_faces, int num_boundary_faces,
                                   const int32_t* face_neighbors, const float* face_normals,
                                   const float* face_surfaces, T8gpuVars_f32 state, T8gpuVars_f32 fluxes,
                                   void* stream);
int t8gpu_hip_subgrid_boundary_f64(int flux_kind, int rank, int num_faces, int num_boundary_faces,
                                   const int32_t* face_neighbors, const double* face_normals,
                                   const double* face_surfaces, T8gpuVars_f64 state, T8gpuVars_f64 fluxes,
                                   void* stream);
/* The boundary faces with their kinds (t8gpu_host.h: boundary_kinds[B], device copy): walls as above; on an outflow face
 * every sub-face evaluates the interior face flux with the outside state = the inside subcell's, on an inflow face with the
 * outside state = the conservative state k of `inflow_table` (t8gpu_hip_plain_inflow_table_*, words 0-4 of a row; may be
 * NULL when no face is an inflow face); outward normal, area face_surfaces / sub-faces. boundary_kinds = NULL is
 * t8gpu_hip_subgrid_boundary_*. */
int t8gpu_hip_subgrid_boundary_bc_f32(int flux_kind, int rank, int num_faces, int num_boundary_faces,
                                      const int32_t* face_neighbors, const uint8_t* boundary_kinds, const float* inflow_table,
                                      const float* face_normals, const float* face_surfaces, T8gpuVars_f32 state,
                                      T8gpuVars_f32 fluxes, void* stream);
int t8gpu_hip_subgrid_boundary_bc_f64(int flux_kind, int rank, int num_faces, int num_boundary_faces,
                                      const int32_t* face_neighbors, const uint8_t* boundary_kinds, const double* inflow_table,
                                      const double* face_normals, const double* face_surfaces, T8gpuVars_f64 state,
                                      T8gpuVars_f64 fluxes, void* stream);
/* The same with far-field faces as well (ABI 12): kinds 10 + k take the outside state of the characteristic condition against
 * state k of `inflow_table`, per sub-face from the inside subcell and the block face's outward normal. Kinds of 9
 * and below as t8gpu_hip_subgrid_boundary_bc_* (bit for bit: one kernel template, whose instantiation behind _bc holds no
 * far-field code, for plans without far-field faces). */
int t8gpu_hip_subgrid_boundary_far_f32(int flux_kind, int rank, int num_faces, int num_boundary_faces,
                                       const int32_t* face_neighbors, const uint8_t* boundary_kinds, const float* inflow_table,
                                       const float* face_normals, const float* face_surfaces, T8gpuVars_f32 state,
                                       T8gpuVars_f32 fluxes, void* stream);
int t8gpu_hip_subgrid_boundary_far_f64(int flux_kind, int rank, int num_faces, int num_boundary_faces,
                                       const int32_t* face_neighbors, const uint8_t* boundary_kinds, const double* inflow_table,
                                       const double* face_normals, const double* face_surfaces, T8gpuVars_f64 state,
                                       T8gpuVars_f64 fluxes, void* stream);

/* timestepping::subgrid::SSP_3RK_step{1,2,3}<V,Subgrid><<<N, block_size>>>, ssp_runge_kutta.inl:101-221
 * (per-subcell volume = volumes[e] / Subgrid::size). */
int t8gpu_hip_subgrid_rk3_stage_f32(int stage, int rank, int num_elements, T8gpuVars_f32 prev, T8gpuVars_f32 mid,
                                    T8gpuVars_f32 out, T8gpuVars_f32 fluxes, const float* volumes, float delta_t,
                                    void* stream);
int t8gpu_hip_subgrid_rk3_stage_f64(int stage, int rank, int num_elements, T8gpuVars_f64 prev, T8gpuVars_f64 mid,
                                    T8gpuVars_f64 out, T8gpuVars_f64 fluxes, const double* volumes, double delta_t,
                                    void* stream);

/* ---- plain elements, fused tile kernels ("fast" tier) ------------------------------------------
 * One launch per RK stage replaces kepes_compute_fluxes + reflective_boundary_condition +
 * SSP_3RK_stepK of that stage (solver.cu:81-110 / 115-142 / 147-174): every tile (compact window of
 * owned elements) stages per-element primitives in LDS, evaluates each of its faces once, sums the
 * fluxes per element in a fixed order and applies the RK stage. The Fluxes planes are neither read
 * nor written (the reference leaves them zero after every stage); speed_estimates is written as the
 * reference does (may be NULL). The plan is built on the host by t8gpu_plan_plain_create()
 * (t8gpu_amd/csrc/host/tile_plan.cpp) at every connectivity rebuild and uploaded by the caller. */
typedef struct T8gpuPlainPlan {
  const int32_t*  elem_off;   /* [ntiles+1] first owned element of each tile                      */
  const int32_t*  halo_off;   /* [ntiles+1] into halo_ids                                         */
  const int32_t*  face_off;   /* [ntiles+1] into face_*                                           */
  const int32_t*  halo_ids;   /* slots of outside elements (other tiles / ghost mirrors)          */
  const uint32_t* face_lr;    /* tile-local l | r << 16 (r = 0xFFFF: reflective wall; 0xFFFE, 0xFFF0 + k: open, ABI 9) */
  const void*     face_geo;   /* float_type [n_faces][4] = nx, ny, nz, area                       */
  const int32_t*  face_orig;  /* original face index if this tile reports the speed, else -1      */
  const int32_t*  csr_off;    /* [N+1] into csr_ent. The two CSR arrays are read by the generic kernel only: may be NULL where `ell`
                               * and `tile_desc` are given and max_elems <= 256, max_slots <= 512, max_faces <= 1024 (the pipelined kernels) */
  const uint16_t* csr_ent;    /* tile-local face | 0x8000 when the element is the face's right side */
  const int32_t*  tile_order; /* [ntiles] deep-interior tiles, then interior tiles that read an element
                               * owned by a ghost-reading tile, then the tiles reading ghost slots */
  int32_t ntiles, n_interior_tiles, max_elems, max_halo, max_faces, ell_width;
  /* optional compressed forms (NULL = absent); with them and tiles of <= 256 elements, <= 512 own+halo
   * elements and <= 1024 faces the software-pipelined kernel variant is used (two passes of 256 faces up
   * to 512 faces per tile, up to four above) */
  const uint16_t* ell;        /* [rows][ell_width] copy of the CSR lists, 0xFFFF-padded, 16-byte rows. ABI 5: rows exist for the
                               * elements of GENERIC tiles only; a tile's first row is word 6 of its tile_desc record, element e
                               * of the tile is row (word 6) + (e - first element)                                  */
  const uint16_t* geo_idx;    /* per tile face: row of geo_table (bits 0-12) | direction code << 13: 2 * axis + (normal
                               * along +axis) for an exact axis normal, 6 otherwise. Inside every block of 256 tile
                               * faces the faces are ordered by that code                                  */
  const void*     geo_table;  /* float_type [n_geo][12]: distinct {nx,ny,nz,area, t1x,t1y,t1z,0, t2x,t2y,t2z,0} */
  int32_t n_geo;
  int32_t max_slots;          /* max over tiles of own + halo elements (0: unknown, max_elems + max_halo is used) */
  int32_t n_deep_tiles;       /* leading tiles of tile_order that read nothing a ghost-reading tile owns (0: unknown) */
  int32_t n_slots_addressed;  /* owned + ghost elements of the planes the plan indexes (ABI 5; was reserved). The patch kernels
                               * address a plane by a 32-bit byte offset and refuse plans whose planes reach 4 GiB (or that
                               * leave this 0): build the plan without patches for such meshes */
  const int32_t* tile_desc;   /* [ntiles][8], in tile_order order: {first element, elements, first halo entry, halo entries,
                               * first face, faces, first ELL row, 0} of tile_order[k] -- one 32-byte record per tile for the persistent
                               * kernel, which reads it several tiles ahead (NULL: that kernel is not used) */
  /* STRUCTURED PATCHES (ABI 4; t8gpu_plan_plain_create_ex flag 1, csrc/host/tile_plan.cpp: find_patches): tiles of 256
   * consecutive elements that form an aligned 16 x 16 block of same-size quadrilaterals with the canonical face listing.
   * They have no face records; their tile_desc is {first element, 256, first halo entry, 64, id of the first own face,
   * 0x100 | flags, area as a double}, their 64 halo entries the elements across the -x | +x | -y | +y sides. The first
   * n_patch_tiles[c] tiles of class c of tile_order (c = 0: [0, n_deep_tiles), 1: [n_deep_tiles, n_interior_tiles),
   * 2: the rest) are patch tiles; they run through kernels_fused_patch.hip. All zero: no patches.
   * Flag 0x400 in word 5 of a patch descriptor: every element of the patch has one volume, carried as a double in words
   * 1 and 3 (the planner checked the volumes it was given, t8gpu_plan_plain_patch_volumes); the kernels then do not read
   * `volume[]` for that patch -- rebuild the plan if the volumes change. */
  int32_t n_patch_tiles[3];
  int32_t patch_dim;          /* 2: the 16 x 16 patches above; 3: 8 x 8 x 4 blocks of same-size hexahedra (256 halo entries:
                               * -x 32 | +x 32 | -y 32 | +y 32 | -z 64 | +z 64; own faces fbase + 3 t + {0, 1, 2}; flags bits 0-2:
                               * -y before -x, -z before -x, -z before -y where both coordinates of the pair are 0); 0: no patches */
  int32_t n_irregular_tiles[3]; /* ABI 6: the LAST so many of the n_patch_tiles[c] patch tiles of class c are IRREGULAR 3D patches
                               * (t8gpu_host.h: t8gpu_plan_plain_create_ex flag 8): descriptor word 5 has 0x800, word 4 is the
                               * first of 512 face_lr / face_orig entries with the per-cell words. They run through the
                               * irregular instantiation of k_plain_patch3 in a launch of their own */
  /* GHOST WINDOW (ABI 7). Run-time attachments of the multi-rank step driver (csrc/hip/stepper.hip), all NULL / 0 in a plan
   * that comes from the planner -- callers of t8gpu_hip_plain_fused_stage_* leave them so unless they do what the driver does.
   * With them a launch of the ghost-reading tiles needs no pack and no unpack kernel around the RCCL exchange:
   *   ghost_buf != NULL: a slot s >= n_owned is read from ghost_buf[5 * (s - n_owned) + var] -- the receive buffer of the
   *     exchange in its wire format -- instead of the mirror slot s of the planes (which is then neither read nor written);
   *   send_map != NULL: after the RK update of owned element e the five new values also go to send_buf[5 * t + var] for every
   *     send slot t of e: send_map[e] = -1 (not sent), t >= 0 (one slot), or -(2 + i) (several: send_list[i], send_list[i+1],
   *     ... up to and including the first entry with bit 31 set; slot = entry & 0x7FFFFFFF).
   * Taken by the 2D patch kernel and the one-tile kernels (launches with either pointer set run one tile per workgroup); the
   * launchers refuse them for 3D patch tiles (hipErrorInvalidValue). */
  const void*    ghost_buf;   /* DEVICE float_type [5 * G], element-major                                   */
  const int32_t* send_map;    /* DEVICE [n_owned]                                                           */
  const int32_t* send_list;   /* DEVICE, may be NULL when no element has more than one send slot            */
  void*          send_buf;    /* DEVICE float_type [5 * n_send], element-major                              */
  int32_t        n_owned;     /* N: first ghost slot                                                        */
  int32_t        reserved7;
  /* OPEN BOUNDARIES (ABI 9). A plan built with boundary_kinds (t8gpu_host.h: t8gpu_plan_plain_create_bc) encodes the r half of
   * a boundary face's face_lr as 0xFFFF (reflective wall), 0xFFFE (outflow: the outside state is the inside one) or
   * 0xFFF0 + k (inflow with prescribed state k). has_open_faces = 1 selects the kernels that decode the two open codes; 0 (a
   * zeroed tail) is the behaviour of earlier ABIs: every boundary face a wall. `inflow` is the table of the prescribed
   * states, filled once by t8gpu_hip_plain_inflow_table_*; it must be given (at least one entry, hipErrorInvalidValue
   * otherwise) whenever has_open_faces is set, and holds an entry for every inflow code of the plan. No launch writes it. The persistent tile kernel does not take plans with open faces (t8gpu_hip_plain_persistent_accepts says 0):
   * their launches run the one-tile kernels, which give the same bits. */
  const void*    inflow;      /* DEVICE float_type [K][T8GPU_INFLOW_WORDS]                                  */
  int32_t        has_open_faces;
  /* FAR-FIELD FACES (ABI 11): 0xFFF8 + k in face_lr is a far-field face against state k of `inflow` (k < 6; the inflow codes are
   * then 0xFFF0 .. 0xFFF7). has_farfield_faces = 1 (with has_open_faces = 1) selects the _far kernels, which build the outside
   * state of such a face from the inside state, the face normal and the table row (Riemann invariants); the
   * table must then hold an entry for every far-field code too. 0 (a zeroed tail): no far-field faces, as before ABI 11. */
  int32_t        has_farfield_faces;
} T8gpuPlainPlan;

/* One inflow-table entry: the conservative state (5 values), the 9 per-element KEPES quantities the tile kernels derive from a
 * state (rho, v, p, beta, log rho, log beta, entropy term: the same device routine the tiles run for their cells, so an inflow
 * state equal to a cell's state gives that cell's bits), 2 words of padding. */
#define T8GPU_INFLOW_WORDS 16
/* table[K][T8GPU_INFLOW_WORDS] (DEVICE, float_type) from states[K][5] (DEVICE, float_type, conservative), K <= 8. */
int t8gpu_hip_plain_inflow_table_f32(const float* states, int num_states, float* table, void* stream);
int t8gpu_hip_plain_inflow_table_f64(const double* states, int num_states, double* table, void* stream);

/* tile_begin/tile_count select a range of tile_order (0, ntiles = everything; [0, n_interior) can run
 * while the halo exchange of `src` is still in flight, [n_interior, ntiles) after it). mid = state
 * the fluxes are evaluated on (prev for stage 1, Step1, Step2); ghost slots of `mid` must be current.
 * Stage 1 is u1 = u0 + dt/vol f(u0) (ssp_runge_kutta.inl:30-50): prev and mid MUST be the same planes there,
 * anything else returns hipErrorInvalidValue. speed_estimates (may be NULL) gets one value per face for EVERY
 * flux_kind: |uHat| + aHat for KEPES (kernels.cu:222), max(|S_l|, |S_r|) of the wave-speed bounds for HLL / HLLC. */
int t8gpu_hip_plain_fused_stage_f32(int flux_kind, int stage, const T8gpuPlainPlan* plan, int tile_begin,
                                    int tile_count, T8gpuVars_f32 prev, T8gpuVars_f32 mid, T8gpuVars_f32 out,
                                    const float* volume, float delta_t, float* speed_estimates, void* stream);
int t8gpu_hip_plain_fused_stage_f64(int flux_kind, int stage, const T8gpuPlainPlan* plan, int tile_begin,
                                    int tile_count, T8gpuVars_f64 prev, T8gpuVars_f64 mid, T8gpuVars_f64 out,
                                    const double* volume, double delta_t, double* speed_estimates, void* stream);

/* The same with a PLANAR request (ABI 13; planar = 0: exactly the entry points above). planar != 0 is the caller's word that,
 * over the slots this launch reads and writes, the z-momentum planes (variable 3) of `prev` and `mid` hold the +0 bit pattern
 * everywhere and that of `out` holds +0 already -- what a 2D run keeps true from step to step. The 2D patch tiles then run a
 * form of the stage that neither loads nor stores that plane and carries no z terms through the flux; the results are the
 * general form's bit for bit, signed zeros included, for FINITE states (an infinity or NaN in another variable reaches the
 * z-momentum in the general form and does not in the planar one). Honoured for KEPES in a whole-plan launch (tile_begin = 0,
 * tile_count = ntiles) of a plan with 2D patches, no ghost window and no open faces -- and, in fp64 (ABI 14), with the five planes of `prev` (stages 2, 3), `mid` and `out` equally
 * spaced, all by the spacing of `mid` (rows of one array, as the step drivers pass them: the kernel addresses plane k as
 * p[0] + k x spacing); anything else runs the general form, silently. The generic tiles of the launch always run the general
 * form. */
int t8gpu_hip_plain_fused_stage_planar_f32(int flux_kind, int stage, const T8gpuPlainPlan* plan, int tile_begin,
                                           int tile_count, T8gpuVars_f32 prev, T8gpuVars_f32 mid, T8gpuVars_f32 out,
                                           const float* volume, float delta_t, float* speed_estimates, void* stream, int planar);
int t8gpu_hip_plain_fused_stage_planar_f64(int flux_kind, int stage, const T8gpuPlainPlan* plan, int tile_begin,
                                           int tile_count, T8gpuVars_f64 prev, T8gpuVars_f64 mid, T8gpuVars_f64 out,
                                           const double* volume, double delta_t, double* speed_estimates, void* stream, int planar);

/* 1 if a whole-plan launch of `tile_count` tiles (flux_kind, float_size = 4 | 8) would run the persistent, software-
 * pipelined tile kernel (kernels_fused_persistent.hip), 0 if it goes to the one-tile-per-workgroup kernels: the launcher's
 * own test, for host code that picks tile caps (t8gpu_amd/fused.py). Only the plan's integer fields and the NULL-ness of
 * tile_desc / ell / geo_idx / geo_table are looked at; no GPU is needed. */
int t8gpu_hip_plain_persistent_accepts(const T8gpuPlainPlan* plan, int flux_kind, int float_size, int tile_count);
/* 1 if a launch of this plan's generic tiles reads csr_off / csr_ent (the generic kernel), 0 if it runs the pipelined kernels
 * (ELL rows + tile descriptors), whose callers need not upload the CSR lists: the launcher's own test, from the plan's
 * integer fields and the NULL-ness of ell / tile_desc alone; no GPU is needed. */
int t8gpu_hip_plain_needs_csr(const T8gpuPlainPlan* plan);
/* Bytes of dynamic LDS of a workgroup of the 2D patch launch (kernels_fused_patch.hip) for flux_kind and float_size = 4 | 8, in
 * the planar form if `planar` (honoured for KEPES, as by the launcher): the patch body's window, or -- `plan` not NULL: its generic
 * tiles ride in the same launch -- the larger of that and the tile body's window for the plan's max_slots. The launcher's own
 * sizes; a planar fp64 launch holds four workgroups per CU where this is at most 40 960. -1: bad arguments. No GPU is needed. */
int t8gpu_hip_plain_patch_lds_bytes(const T8gpuPlainPlan* plan, int flux_kind, int float_size, int planar);
/* The tangent rows of a geometry dictionary ALREADY ON THE DEVICE (`geo_table`: n_geo rows {n, area} {t1, .} {t2, .} of the
 * plan's float type), recomputed from its normals by the routine the per-face kernels use (flux_math.hpp: face_basis_fast --
 * the frame of kernels.cu:174-193 with one reciprocal square root instead of a square root and three divisions). Plan builders
 * call it once after the upload, so that a tile evaluated with the dictionary and the same face evaluated with per-face
 * geometry rows (a partition of the mesh, another tile cap) see the same bits; the host planner's own frames
 * (t8gpu_plan_plain_compressed) differ from these in the last bit on oblique normals. */
int t8gpu_hip_plain_geo_frames_f32(void* geo_table, int n_geo, void* stream);
int t8gpu_hip_plain_geo_frames_f64(void* geo_table, int n_geo, void* stream);

/* ---- ghost-layer exchange (device side) ----------------------------------------------------------
 * Replaces the reference's cross-rank pointer sharing (cudaIpc*, t8gpu/memory/shared_device_vector.inl:
 * 15-30,159-199) and remote atomics (kernels.cu:295-308): ghosts are mirror slots [N, N+G) of the same
 * planes, refreshed once per RK stage by  pack -> RCCL send/recv per neighbour rank -> unpack.
 * Wire format: 5 values per element, element-major (sendbuf[5*t + var]); each peer's elements are a
 * contiguous run of send_idx / of the ghost slots, so one message per peer and direction. The
 * transport (ncclSend/ncclRecv in one group, on the stream of these kernels) is issued by the host
 * side (t8gpu_amd/halo.py through torch.distributed's RCCL communicator) or natively (T8gpuHalo below).
 * cells_per_element = 1 for plain elements, Subgrid::size (16 / 64) for blocks (a ghost block mirrors all
 * its subcells; wire format (element, cell, variable)). */
int t8gpu_hip_halo_pack_f32(int n_send, int cells_per_element, const int32_t* send_idx, T8gpuVars_f32 state,
                            float* sendbuf, void* stream);
int t8gpu_hip_halo_pack_f64(int n_send, int cells_per_element, const int32_t* send_idx, T8gpuVars_f64 state,
                            double* sendbuf, void* stream);
int t8gpu_hip_halo_unpack_f32(int num_ghosts, int first_ghost_slot, int cells_per_element, const float* recvbuf,
                              T8gpuVars_f32 state, void* stream);
int t8gpu_hip_halo_unpack_f64(int num_ghosts, int first_ghost_slot, int cells_per_element, const double* recvbuf,
                              T8gpuVars_f64 state, void* stream);

/* ---- native RCCL transport + whole-step driver ----------------------------------------------------
 * One communicator per process (one rank per GPU); the 128-byte id is created on one rank and
 * distributed by the caller (MPI_Bcast, torch.distributed, ...). Replaces the MPI_Allgather of CUDA-IPC
 * handles at construction and at EVERY resize (shared_device_vector.inl:21-22,95-96,179-185,270-276). */
int t8gpu_hip_comm_unique_id(char* id128);
int t8gpu_hip_comm_create(const char* id128, int rank, int nranks, void** comm);
int t8gpu_hip_comm_destroy(void* comm);
int t8gpu_hip_comm_abort(void* comm);
int t8gpu_hip_stream_wait(void* stream, double timeout_s); /* 0 idle, 1 timed out, else hipError_t */
/* out4 = {RCCL version of the headers this library was compiled with (NCCL_VERSION_CODE), RCCL version of the library the
 * process bound (ncclGetVersion), HIP_VERSION of the headers, hipRuntimeGetVersion}. A process may bind another build than
 * the headers came from (the torch wheel's librccl / libamdhip64 against /opt/rocm's headers): t8gpu_hip_comm_create checks
 * the pairs -- same major versions, RCCL >= 2.7 (the send / recv API this library uses, unchanged since) -- and returns
 * hipErrorNotSupported otherwise; bench.py reports both pairs. */
int t8gpu_hip_runtime_versions(int out4[4]);

typedef struct T8gpuHalo {
  int32_t num_elements, num_ghosts, n_peers, n_send;
  int32_t cells_per_element, reserved; /* 1 (plain elements) or Subgrid::size                            */
  const int32_t* peers;     /* HOST [n_peers] neighbour ranks, ascending                               */
  const int32_t* send_off;  /* HOST [n_peers+1] ranges of send_idx per peer                            */
  const int32_t* recv_off;  /* HOST [n_peers+1] ranges of the ghost slots (relative to N) per peer     */
  const int32_t* send_idx;  /* DEVICE [n_send] owned elements mirrored on a peer                       */
  void* sendbuf;            /* DEVICE 5*n_send*cells_per_element float_type                            */
  void* recvbuf;            /* DEVICE 5*num_ghosts*cells_per_element float_type                        */
  void* comm;               /* from t8gpu_hip_comm_create                                              */
} T8gpuHalo;

/* pack -> ncclGroupStart, ncclRecv/ncclSend per peer, ncclGroupEnd -> unpack, all on `stream`. */
int t8gpu_hip_halo_exchange_f32(const T8gpuHalo* halo, T8gpuVars_f32 state, void* stream);
int t8gpu_hip_halo_exchange_f64(const T8gpuHalo* halo, T8gpuVars_f64 state, void* stream);

/* CompressibleEulerSolver::iterate (solver.cu:75-175) as one call: `planes` is the MemoryManager
 * allocation (26 planes of `stride`, plane = step*5+var, volume = plane 25; memory_manager.h:460), prev /
 * next the step ids AFTER the caller's std::swap (solver.cu:76). Enqueues, per stage, the exchange and the
 * ghost-reading tiles on an internal second stream beside the interior tiles on `stream` (two lanes, each waiting
 * only for the other lane's PREVIOUS stage; the caller's thread enqueues both lanes, stage by stage;
 * csrc/hip/stepper.hip, with the exchange itself in csrc/hip/transport.hip) and returns; no host sync. Work queued on
 * `stream` before the call is seen by it, work queued after the call sees its result. For plain 2D / tile plans
 * the ghost-reading tiles read the receive buffer and fill the send buffer themselves (T8gpuPlainPlan "ghost
 * window"): the ghost mirror slots [N, N+G) of the planes are then NOT refreshed by this driver -- code that reads
 * them between steps calls t8gpu_hip_halo_exchange_* (T8GPU_GHOST_WINDOW=0: pack / unpack kernels, slots refreshed).
 * iterate_steps: n_steps consecutive steps in one call, prev / next given for the FIRST step and swapped
 * from step to step (after an odd n_steps the caller's roles are swapped once more); the two streams then
 * meet only at the entry and the exit of the call instead of once per step.
 * speed_estimates (ABI 15): when the call's work is done the array holds the estimates of the call's LAST step, one value
 * for every face, exactly what n_steps calls of one step leave there (what compute_timestep reads: "computed at the last
 * step of the last timestepping", solver.h:88-91). The estimates of the steps before are NOT materialised: nothing can
 * read them before the next step overwrites them, so only the third stage of the last step is handed the array
 * (t8gpu_hip_stepper_set_speed_every_step below). A caller that wants them per step calls with n_steps = 1. */
int t8gpu_hip_plain_stepper_create(const T8gpuPlainPlan* plan, const T8gpuHalo* halo_or_null, void** stepper);
int t8gpu_hip_plain_stepper_destroy(void* stepper);
int t8gpu_hip_plain_stepper_iterate_f32(void* stepper, int flux_kind, float* planes, size_t stride, int prev, int next,
                                        float delta_t, float* speed_estimates, void* stream);
int t8gpu_hip_plain_stepper_iterate_f64(void* stepper, int flux_kind, double* planes, size_t stride, int prev, int next,
                                        double delta_t, double* speed_estimates, void* stream);
int t8gpu_hip_plain_stepper_iterate_steps_f32(void* stepper, int flux_kind, float* planes, size_t stride, int prev, int next,
                                              float delta_t, float* speed_estimates, int n_steps, void* stream);
int t8gpu_hip_plain_stepper_iterate_steps_f64(void* stepper, int flux_kind, double* planes, size_t stride, int prev, int next,
                                              double delta_t, double* speed_estimates, int n_steps, void* stream);
/* optional HIP-event timing of the stage kernels (for roofline accounting): enable = 0 off, n > 0 = the stage
 * kernels of every n-th step of a call are bracketed by events (n > 1 keeps the host-side cost of the
 * events out of latency-bound multi-rank runs); elapsed() sums what has been recorded since. */
/* hipGraph replay ("hipGraph capture of the 3-stage step"): enable = 1 -> an iterate_steps() call is captured
 * once per argument set (the four most recent sets are kept: a step loop alternates between two) and replayed with ONE
 * hipGraphLaunch afterwards; enable = 0 -> direct enqueue (default); enable < 0 -> query only. counts (may be NULL)
 * receives {captures, replays}. A capture the runtime refuses returns its error code. delta_t is part of the argument set
 * (a CFL-adaptive step size re-captures per value: use the direct enqueue there).
 * A stepper WITH a halo always enqueues directly (the two-lane driver), whatever this switch says. */
int t8gpu_hip_plain_stepper_graph(void* stepper, int enable, int* counts);
int t8gpu_hip_plain_stepper_timing(void* stepper, int enable);
/* The planar 2D stage in the step driver (ABI 13). A single-rank stepper over a plain plan with 2D patches, KEPES: at the start
 * of an iterate / iterate_steps call ONE device reduction ORs the raw bits of the z-momentum planes of the four step slots the
 * call touches (prev, Step1, Step2, next; the slots the plan addresses) and the host reads the four words after the only
 * stream synchronisation this adds. prev not all +0: the call runs in the general form. Otherwise the other planes that are
 * not all +0 are zeroed (hipMemsetAsync; none in steady state) and every stage of the call runs planar
 * (t8gpu_hip_plain_fused_stage_planar_*). Nothing is remembered from call to call: the caller may write the planes in between.
 * mode 0 = never, 1 = where the check is amortised (n_steps x elements >= 2^25; the default),
 * 2 = whenever the check proves it. A plan with open faces (has_open_faces / has_farfield_faces) never runs planar: a
 * prescribed outside state may carry a z-momentum. A call that checks SYNCHRONISES the stream once, also when the stepper
 * replays a graph (the check runs before the replay): the host cannot enqueue the next call ahead of the GPU then.
 * _planar: what the last call DECIDED (1 planar, 0 general); the kernel a stage then launched is named by
 * t8gpu_hip_last_stage_kernel (the launcher runs the general kernel for launches that are not whole-plan persistent ones). */
int t8gpu_hip_stepper_set_planar(void* stepper, int mode);
int t8gpu_hip_stepper_planar(void* stepper);
/* Which stages of an iterate_steps call write the speed estimates (ABI 15): on = 0, the third stage of the call's last step
 * only (the default); on = 1, the third stage of every step (the behaviour before ABI 15; for A/B measurements). The array
 * holds the same bits on return either way. A new stepper starts with on = 1 if T8GPU_SPEED_EVERY_STEP is set to anything
 * but "" or "0..." in the environment. The mode is part of the argument set of a captured graph.
 * _speed_stages: how many RK stages of the last call were handed a non-NULL speed_estimates (a stage counts once, however
 * many lanes or tile classes it is launched in; 0 for Subgrid steppers, which have no such array). */
int t8gpu_hip_stepper_set_speed_every_step(void* stepper, int on);
int t8gpu_hip_stepper_speed_stages(void* stepper);
/* Diagnostics (scripts/halo_overhead.py): with T8GPU_STEPPER_PROFILE=1 in the environment the step drivers time their own
 * host calls; ns4 / calls4 (may be NULL) receive nanoseconds and counts for {kernel launches, RCCL groups, event records,
 * stream waits} since the last reset. Returns 1 when the profile is on, 0 when off (all zeros). */
int t8gpu_hip_stepper_host_profile(int reset, double* ns4, long long* calls4);
int t8gpu_hip_plain_stepper_elapsed(void* stepper, double* total_ms, int* launches);
int t8gpu_hip_plain_stepper_timed_stages(void* stepper); /* RK stages covered by elapsed() */
/* host time the multi-rank driver spent enqueueing (wall time of its iterate calls) and the steps that covers, since
 * creation or the last reset; 0 / 0 for single-rank steppers */
int t8gpu_hip_plain_stepper_host_time(void* stepper, int reset, double* total_ms, long long* steps);

/* ---- Subgrid<4,4,4> and Subgrid<4,4>, fused block kernels ("fast" tier) -----------------------------
 * One launch per RK stage replaces compute_inner_fluxes + compute_boundary_fluxes + compute_outer_fluxes
 * + subgrid::SSP_3RK_stepK of that stage (examples/subgrid/solver.inl:166-195): one 64-lane wavefront per
 * 4x4x4 block (or per four 4x4 blocks) evaluates every flux its subcells need (an outer sub-face is evaluated by both blocks that
 * share it) and applies the RK stage; the Fluxes planes are neither read nor written. The plan is the
 * per-block face list built by t8gpu_plan_subgrid_create() (csrc/host/subgrid_plan.cpp). */
typedef struct T8gpuSubgridPlan {
  /* joined records, t8gpu_plan_subgrid_records(): one dependent load level between a wavefront's position
   * and all of its far-cell loads */
  const int32_t* block_rec;     /* [num_elements][32], blocks that touch no ghost block first: {block, n generic
                                   faces, first bf_rec entry, 0, 3 x the +d face {other block (-1 wall, -2 none / in
                                   the generic list), code, area (2 words)}, 3 x the -d face likewise, 4 spare words}
                                   (128-byte rows) */
  const int32_t* bf_rec;        /* [n_entries][4] generic faces (towards finer blocks) in the same order: {other block,
                                   code (bit 12: the block is the face's RIGHT side), area (2 words)} */
  int32_t num_elements, rank, max_faces_per_block, n_interior_blocks;
  int32_t n_deep_blocks;        /* leading blocks that have no neighbour touching a ghost block (0: unknown) */
  int32_t n_blocks_addressed;   /* 1 + the largest block index any record refers to (owned and ghost blocks; sizes[5] of
                                   t8gpu_plan_subgrid_sizes): lets the kernel use 32-bit byte offsets into the state planes
                                   when a plane is shorter than 4 GiB. 0 = unknown (64-bit addressing) */
  /* optional (t8gpu_plan_subgrid_family_records()): 2x2x2 cubes (RANK 3) / 2x2 squares (RANK 2) of consecutive same-level
   * deep interior blocks take the family kernels (one workgroup of 8 wavefronts per cube / one wavefront per square) when a
   * launch covers the whole plan or exactly its first class [0, n_deep_blocks); the blocks outside every family then run
   * through rest_rec (launches inside the later classes read rest_rec too). n_families = 0: every block through block_rec. */
  const int32_t* fam_rec;       /* RANK 3: [n_families][160] = {first block, 0, 0, 0, 36 rows {far, code, area (2 words)}}: the 12
                                   outward + faces, the 12 outward - faces, the 12 inner faces; RANK 2: [n_families][64] with
                                   4 + 4 + 4 rows (layout: subgrid_plan.cpp) */
  const int32_t* rest_rec;      /* [n_rest][32]: block_rec rows of the blocks outside every family, in block_order order */
  int32_t n_families, n_rest;
  /* OPEN BOUNDARIES (ABI 10). A plan built with boundary_kinds (t8gpu_host.h: t8gpu_plan_subgrid_create_bc) keeps far = -1 for
   * every boundary face and carries the face's kind in bits 23-26 of its code word: 0 reflective wall, 1 outflow (the outside
   * state is the inside subcell's), 2 + k inflow with prescribed state k. has_open_faces = 1 selects the kernels that decode
   * the kind; 0 (a zeroed tail) is the behaviour of earlier ABIs: every boundary face a wall. `inflow` is the table of the
   * prescribed states filled by t8gpu_hip_plain_inflow_table_* (the Subgrid kernels read words 0-4 of a row, the conservative
   * state); it must be given whenever has_open_faces is set (hipErrorInvalidValue otherwise) and holds an entry for every
   * inflow code of the plan. No launch writes it. No family holds a block with an open face. */
  const void*    inflow;        /* DEVICE float_type [K][T8GPU_INFLOW_WORDS] */
  int32_t        has_open_faces;
  /* FAR-FIELD FACES (ABI 12): a plan built by t8gpu_plan_subgrid_create_far may hold kinds 10 + k in the same bits: a far-field
   * face against state k of `inflow` (k < 6). has_farfield_faces = 1 (with has_open_faces = 1) selects the kernels of MODE kBndFar, whose
   * block algorithm builds the outside state of every such sub-face from the inside subcell, the outward normal +-e_axis and
   * the table row (Riemann invariants); the table must then hold an entry for every far-field code too. 0 (a
   * zeroed tail): no far-field faces, as before ABI 12. */
  int32_t        has_farfield_faces;
} T8gpuSubgridPlan;

/* block_begin/block_count select a range of block_order (0, num_elements = everything; [0, n_interior_blocks)
 * can run while the halo exchange of `mid` is in flight). */
int t8gpu_hip_subgrid_fused_stage_f32(int flux_kind, int stage, const T8gpuSubgridPlan* plan, int block_begin,
                                      int block_count, T8gpuVars_f32 prev, T8gpuVars_f32 mid, T8gpuVars_f32 out,
                                      const float* volumes, float delta_t, void* stream);
int t8gpu_hip_subgrid_fused_stage_f64(int flux_kind, int stage, const T8gpuSubgridPlan* plan, int block_begin,
                                      int block_count, T8gpuVars_f64 prev, T8gpuVars_f64 mid, T8gpuVars_f64 out,
                                      const double* volumes, double delta_t, void* stream);

/* Native step driver for Subgrid blocks: SubgridCompressibleEulerSolver::iterate (examples/subgrid/solver.inl:152-266)
 * in one host call, the pipeline of t8gpu_hip_plain_stepper_* over the block classes of the plan (deep interior /
 * near-boundary / ghost-touching blocks on the two lanes, one RCCL exchange of whole ghost blocks per stage;
 * halo->cells_per_element = 4^rank). `planes` = 25 variable planes of `stride` values (stride >= (N + G) * 4^rank),
 * `volumes` the per-block volume array. The handle is destroyed / timed with the t8gpu_hip_plain_stepper_destroy,
 * _timing, _elapsed and _timed_stages entry points above. */
int t8gpu_hip_subgrid_stepper_create(const T8gpuSubgridPlan* plan, const T8gpuHalo* halo_or_null, void** stepper);
int t8gpu_hip_subgrid_stepper_iterate_steps_f32(void* stepper, int flux_kind, float* planes, size_t stride, const float* volumes,
                                                int prev, int next, float delta_t, int n_steps, void* stream);
int t8gpu_hip_subgrid_stepper_iterate_steps_f64(void* stepper, int flux_kind, double* planes, size_t stride, const double* volumes,
                                                int prev, int next, double delta_t, int n_steps, void* stream);

/* ---- scalar reductions next to the hot path -------------------------------------------
 * Device-side replacements of the two host round trips of the reference solvers; results are device
 * scalars (double) written on `stream`; `workspace` = t8gpu_hip_reduce_workspace_bytes() device bytes.
 * Fixed reduction tree, no atomics: bitwise reproducible. */
size_t t8gpu_hip_reduce_workspace_bytes(void);
/* out4[j] |= OR of the raw bits of planes[j][0 .. n) for j < 4 (float_type planes; out4: DEVICE uint32_t[4], zeroed by the
 * caller; for 64-bit values the two halves are ORed together). 0 means: every value is +0. One atomic OR per workgroup. */
int t8gpu_hip_planes_or_bits_f32(size_t n, const float* const planes[4], uint32_t* out4, void* stream);
int t8gpu_hip_planes_or_bits_f64(size_t n, const double* const planes[4], uint32_t* out4, void* stream);
/* max over the per-face speed estimates: thrust::reduce(..., maximum) in compute_timestep,
 * examples/compressible_euler/solver.cu:213-217 (the caller all-reduces the scalar across ranks, :218-223,
 * and forms dt = cfl * 0.5^max_level / speed, :225-228). Starts from 0 (the result for n = 0 and for data that is all
 * negative). A NaN among the estimates propagates: the result is NaN wherever in the array it sits. */
int t8gpu_hip_max_speed_f32(size_t n, const float* speed_estimates, void* workspace, double* result, void* stream);
int t8gpu_hip_max_speed_f64(size_t n, const double* speed_estimates, void* workspace, double* result, void* stream);
/* sum of volume * variable over the owned cells: compute_integral, solver.cu:190-211; with
 * cells_per_element = Subgrid::size the per-cell volume is volume[e] / size (examples/subgrid/solver.inl:295-297). */
int t8gpu_hip_integral_f32(size_t num_cells, int cells_per_element, const float* variable, const float* volume,
                           void* workspace, double* result, void* stream);
int t8gpu_hip_integral_f64(size_t num_cells, int cells_per_element, const double* variable, const double* volume,
                           void* workspace, double* result, void* stream);

/* ---- state monitor: CFL rate, integrals, entropy, positivity in one pass ------------------------------
 * What a run loop asks of the state between steps, from one streaming read of the five planes and the volumes (the
 * reference answers none of it on the device: compute_integral copies to the host, solver.cu:190-211 and
 * examples/subgrid/solver.inl:281-305; the Subgrid compute_timestep is unimplemented, solver.inl:309-325).
 * num_cells = owned cells (Subgrid: subcells); volume per ELEMENT, indexed by i / cells_per_element; the cell volume is
 * vol = volume[e] / cells_per_element and the cell length h = vol^(1/dim), dim = 2 | 3: the edge of a Cartesian cell, and on
 * curved cells the cbrt(volume) length of the reference's refinement criterion (solver.cu:240) -- NOT a safe inradius
 * for prisms and tetrahedra. Arithmetic and accumulation in double for both float types; gamma = 1.4. Per cell
 *   m2 = mx^2 + my^2 + mz^2,  p = 0.4 (E - m2 / (2 rho)),  c = sqrt(1.4 p / rho),  s = |m| / rho + c;
 * a cell is FINITE when its five values are, PHYSICAL when finite with rho > 0 and p > 0. result[16] (doubles):
 *   0-4  sum vol * u_k (rho, mx, my, mz, E)            finite cells
 *   5    sum vol * m2 / (2 rho)  (kinetic energy)      finite, rho > 0
 *   6    sum vol * rho * (log p - 1.4 log rho)         physical
 *   7    max s                                         physical
 *   8    max s / h  (the CFL step is cfl / this)       physical
 *   9    min rho                                       finite
 *   10   min p                                         finite, rho > 0
 *   11   number of non-finite cells
 *   12   number of finite, non-physical cells
 *   13-15  0 (reserved)
 * Sums and counts 0, maxima 0, minima +inf where no cell qualifies (num_cells = 0). Ranks combine blocks by sum
 * (0-6, 11, 12), max (7, 8) and min (9, 10). Two launches on `stream` (grid-stride partials, then one workgroup per
 * slot), no atomics: the same data gives the same bits. 16-byte loads when the five plane pointers are 16-byte
 * aligned (and the volume pointer, for cells_per_element = 1), one value per lane otherwise.
 * workspace = t8gpu_hip_state_monitor_workspace_bytes() device bytes. hipErrorInvalidValue for a null workspace or
 * result, cells_per_element < 1 or dim outside {2, 3}. */
#define T8GPU_MONITOR_SLOTS 16
size_t t8gpu_hip_state_monitor_workspace_bytes(void);
int t8gpu_hip_state_monitor_f32(size_t num_cells, int cells_per_element, int dim, T8gpuVars_f32 state, const float* volume,
                                void* workspace, double* result /* [16] */, void* stream);
int t8gpu_hip_state_monitor_f64(size_t num_cells, int cells_per_element, int dim, T8gpuVars_f64 state, const double* volume,
                                void* workspace, double* result /* [16] */, void* stream);

/* ---- boundary budgets: the boundary faces' fluxes and wall pressure forces, summed per face group ------
 * The other half of the monitor's conservation check on a domain with open sides: change of the integral + dt * boundary
 * flux = 0, stage by stage (the reference has nothing of the kind). `state` is read through the arrays the
 * boundary kernels above take (face_neighbors, face_normals, face_surfaces with the boundary entries after the num_faces
 * interior ones; boundary_kinds, NULL = every face a wall; inflow_table, NULL allowed when no face is an inflow or
 * far-field face). The caller labels every boundary face with a group < num_groups <= T8GPU_BOUNDARY_GROUPS_MAX and hands
 * the faces over sorted by group: face_order[B] (DEVICE, int32: indices 0 .. B - 1 of the boundary faces, a stable sort by
 * group) and group_offsets[num_groups + 1] (HOST, int32: the first position of every group in face_order, [0] = 0,
 * [num_groups] = B; read during the call). result[num_groups][T8GPU_BOUNDARY_SLOTS] (DEVICE, doubles), every slot a sum over
 * the faces of the group (Subgrid blocks: over the sub-faces, each with the area face_surfaces / sub-faces):
 *   0      A
 *   1-5    A * g_k   g = the scheme's numerical flux through the face along the OUTWARD normal, in xyz (rho, mx, my, mz, E):
 *                    the vector t8gpu_hip_flux_boundary_bc_* / t8gpu_hip_subgrid_boundary_far_* subtract from the inside cell,
 *                    from the same routines in float_type; outside state by kind (wall: mirrored; outflow: the inside state;
 *                    inflow k: row k; far field k: the characteristic state against row k)
 *   6-8    A * p * n   p = 0.4 (E - |m|^2 / (2 rho)) of the inside cell
 *   9      A * p
 *   10     A * max(g_0, 0)   mass leaving; mass entering is slot 10 - slot 1
 *   11     number of faces / sub-faces
 *   12     number of them whose flux has a non-finite component; these add nothing to slots 1-10
 *   13-15  0 (reserved)
 * Products with A and all accumulation in double for both float types. Ranks combine blocks with one SUM. A group without
 * faces, and num_boundary_faces = 0, give zeros. accumulate = 0: result is overwritten. accumulate != 0: slots 0-10 become
 * result + weight * value (one thread per slot; a loop integrates in time on the device), slots 11-15 are overwritten.
 * Two launches on `stream` (one workgroup per contiguous chunk of one group's faces, then one workgroup per group folding
 * the chunk partials in a fixed tree), no atomics: the same data gives the same bits. Nothing is allocated, nothing waits.
 * workspace = t8gpu_hip_boundary_fluxes_workspace_bytes(B, num_groups) device bytes. hipErrorInvalidValue for a flux_kind
 * outside 0..2, normal_dim / rank outside {2, 3}, num_groups outside 1..32, offsets that do not run from 0 to B in
 * ascending order, or a null result (with B > 0: a null workspace, face_order or face array). */
#define T8GPU_BOUNDARY_SLOTS 16
#define T8GPU_BOUNDARY_GROUPS_MAX 32
size_t t8gpu_hip_boundary_fluxes_workspace_bytes(int num_boundary_faces, int num_groups);
int t8gpu_hip_boundary_fluxes_f32(int flux_kind, int num_faces, int num_boundary_faces, int normal_dim, const int32_t* face_neighbors,
                                  const uint8_t* boundary_kinds, const float* inflow_table, const float* face_normals,
                                  const float* face_surfaces, T8gpuVars_f32 state, int num_groups, const int32_t* face_order,
                                  const int32_t* group_offsets, void* workspace, double* result /* [num_groups][16] */,
                                  int accumulate, double weight, void* stream);
int t8gpu_hip_boundary_fluxes_f64(int flux_kind, int num_faces, int num_boundary_faces, int normal_dim, const int32_t* face_neighbors,
                                  const uint8_t* boundary_kinds, const double* inflow_table, const double* face_normals,
                                  const double* face_surfaces, T8gpuVars_f64 state, int num_groups, const int32_t* face_order,
                                  const int32_t* group_offsets, void* workspace, double* result /* [num_groups][16] */,
                                  int accumulate, double weight, void* stream);
/* Subgrid<4,4> (rank 2) and Subgrid<4,4,4> (rank 3) blocks: one lane per sub-face with the indexing of
 * t8gpu_hip_subgrid_boundary_far_* (the inside subcell of the sub-face map, the block face's outward normal). */
int t8gpu_hip_subgrid_boundary_fluxes_f32(int flux_kind, int rank, int num_faces, int num_boundary_faces,
                                          const int32_t* face_neighbors, const uint8_t* boundary_kinds, const float* inflow_table,
                                          const float* face_normals, const float* face_surfaces, T8gpuVars_f32 state, int num_groups,
                                          const int32_t* face_order, const int32_t* group_offsets, void* workspace,
                                          double* result /* [num_groups][16] */, int accumulate, double weight, void* stream);
int t8gpu_hip_subgrid_boundary_fluxes_f64(int flux_kind, int rank, int num_faces, int num_boundary_faces,
                                          const int32_t* face_neighbors, const uint8_t* boundary_kinds, const double* inflow_table,
                                          const double* face_normals, const double* face_surfaces, T8gpuVars_f64 state, int num_groups,
                                          const int32_t* face_order, const int32_t* group_offsets, void* workspace,
                                          double* result /* [num_groups][16] */, int accumulate, double weight, void* stream);

/* ---- derived output fields: pressure, velocity, Mach, entropy, vorticity, dilatation, schlieren ---------
 * What a run writes to look at itself, formed on the device from the five planes of one step (csrc/hip/fields.hip; the
 * reference writes conserved variables only). All arithmetic in double whatever float_type is, gamma = 1.4,
 * u = (m_x, m_y, m_z) / rho. Output planes (doubles, one value per owned cell in storage order; a vector is three planes):
 *    0      pressure    0.4 (E - |m|^2 / (2 rho))
 *    1-3    velocity    m / rho
 *    4      mach        |u| / sqrt(1.4 p / rho)
 *    5      entropy     log p - 1.4 log rho                    (the per-cell integrand of monitor slot 6 without rho vol)
 *    6-8    vorticity   (1 / 2 V_c) sum_s A_s n_s x (u_o - u_c)
 *    9      dilatation  (1 / 2 V_c) sum_s A_s n_s . (u_o - u_c)
 *    10     schlieren   | (1 / 2 V_c) sum_s A_s n_s (rho_o - rho_c) |
 * The sums run over the INTERIOR faces (sub-faces) s of cell c: n_s the unit normal outward from c, A_s the area, o the cell
 * across s -- the jump form of the Green-Gauss gradient, the central difference on uniform Cartesian cells, exactly +-0 for
 * a uniform state. Boundary faces of every kind contribute no term (a zero-jump closure); at a 2:1 face the arithmetic face
 * mean is first-order consistent only. Non-physical cells get their IEEE results. A 2-component normal
 * has z = 0.
 * A NULL plane is not computed and nothing is stored for it. When planes 6-10 are all NULL the connectivity pointers
 * (volume, face arrays, CSR) may be NULL and no neighbour is read. csr_offsets[n + 1] / csr_entries: the element -> faces
 * lists of t8gpu_host_cell_faces (t8gpu_host.h), device copies. The neighbour's slot may be a ghost slot: its state must be
 * current. Gathers without atomics: a cell sums its terms in CSR order (inside a hanging Subgrid face j-major, i-minor; the
 * in-block faces of a subcell first, -x +x -y +y -z +z), so two calls give the same bits. One launch on `stream`.
 * Plain elements: one lane per owned element; V_c = volume[c]; face f has normals[normal_dim f ..] outward from
 * l = face_neighbors[2 f] and face_surfaces[f], as t8gpu_hip_flux_faces_* reads them.
 * Subgrid blocks: one wavefront per Subgrid<4,4,4> block, four Subgrid<4,4> blocks per wavefront; V_c = volumes[e] / S;
 * in-block faces have area h^(rank-1), h = volumes[e]^(1/rank) / 4; an outer sub-face has face_surfaces[f] / SF and the
 * cell pair of t8gpu_hip_subgrid_outer_* (a hanging face is listed by the finer block).
 * Returns 0 for n <= 0; hipErrorInvalidValue, before any launch, for normal_dim / rank outside {2, 3} or a requested
 * gradient plane with a NULL connectivity pointer. */
typedef struct T8gpuFieldPlanes { double* p[11]; } T8gpuFieldPlanes;
#define T8GPU_FIELD_PLANES 11
int t8gpu_hip_plain_fields_f32(int num_elements, int normal_dim, T8gpuVars_f32 state, const float* volume,
                               const int32_t* face_neighbors, const float* face_normals, const float* face_surfaces,
                               const int32_t* csr_offsets, const int32_t* csr_entries, T8gpuFieldPlanes out, void* stream);
int t8gpu_hip_plain_fields_f64(int num_elements, int normal_dim, T8gpuVars_f64 state, const double* volume,
                               const int32_t* face_neighbors, const double* face_normals, const double* face_surfaces,
                               const int32_t* csr_offsets, const int32_t* csr_entries, T8gpuFieldPlanes out, void* stream);
int t8gpu_hip_subgrid_fields_f32(int rank, int num_blocks, T8gpuVars_f32 state, const float* volumes,
                                 const int32_t* face_neighbors, const int32_t* face_level_difference,
                                 const int32_t* face_neighbor_offset, const float* face_normals, const float* face_surfaces,
                                 const int32_t* csr_offsets, const int32_t* csr_entries, T8gpuFieldPlanes out, void* stream);
int t8gpu_hip_subgrid_fields_f64(int rank, int num_blocks, T8gpuVars_f64 state, const double* volumes,
                                 const int32_t* face_neighbors, const int32_t* face_level_difference,
                                 const int32_t* face_neighbor_offset, const double* face_normals, const double* face_surfaces,
                                 const int32_t* csr_offsets, const int32_t* csr_entries, T8gpuFieldPlanes out, void* stream);

/* ---- sampling on Cartesian forests: probe points, image grids, conservative resampling (csrc/hip/sample.hip)
 * From a coordinate of the unit square / cube to the storage index of the cell that holds it, and from there to values. With
 * D = T8GPU_SAMPLE_DEPTH: the integer coordinate of x in [0, 1) is floor(x 2^D), the key of a point the bit-interleave of its
 * integer coordinates with x in the lowest bit. keys[num_elements] holds the key of every owned element's lower corner and
 * levels[num_elements] its level, both in storage order (device arrays; t8gpu_amd/sample.py builds them): the keys ascend
 * strictly and element e covers [keys[e], keys[e] + 2^(dim (D - levels[e]))). cells_per_axis is 1 for plain elements and 4
 * for Subgrid blocks, whose cells have level levels[e] + 2; levels up to D (blocks: D - 2).
 * Ownership: a point belongs to the cell with lo <= x < hi on every axis, so a point on a shared face or corner goes to the
 * cell on the higher side. The cell index is the storage index among the owned cells: e, or e S + i + 4 j (+ 16 k) with
 * (i, j, k) the two bits of the integer coordinates below the block's level. It is -1 for a point with a coordinate < 0 or
 * >= 1, NaN or infinite (tested on the doubles, before any conversion), and for a point in no owned element (another rank's).
 * Values are those of the holding cell cast to double, `fill` for cell -1; nothing is interpolated. Plane k of a
 * T8gpuSamplePlanes is read from q[k] (the state's float type) when that is not NULL, else from d[k] (doubles, e.g. the
 * planes of t8gpu_hip_*_fields_*); outputs are [num_planes][points or pixels], doubles.
 * t8gpu_hip_sample_locate: cells[i] for points[i dim .. i dim + dim), one lane per point.
 * t8gpu_hip_sample_gather: out[k][i] = plane k at cells[i], or fill.
 * t8gpu_hip_sample_grid: both fused over a grid of n[0] x n[1] (x n[2]) pixels, x fastest, pixel centre
 * lo + (i + 0.5) (hi - lo) / n per axis, evaluated in exactly this order without contraction (an axis with lo == hi is a slice
 * plane at that coordinate); one wavefront per 8 x 8 tile of pixels, ragged tiles masked. `cells` may be NULL; with
 * num_planes = 0 only the cells are written.
 * t8gpu_hip_sample_uniform: conservative resampling onto the 2^level pixels per axis of a uniform level. For pixel P
 * sums[k][P] = sum of w q over the owned cells that meet P and weights[P] = sum of w, w = 2^(-dim level of the smaller of
 * pixel and cell): a pixel inside a cell takes w q of that cell, a pixel covering several cells sums them in ascending
 * storage order in double. With weights = NULL sums[k][P] holds sum / weight instead, `fill` where the weight is 0. The order
 * of a sum does not depend on the launch: two calls give the same bits. Ranks combine by adding sums and weights.
 * t8gpu_hip_sample_average: those per-pixel sums and weights of level `level` added along the mesh axes whose bits are set in
 * axes_mask (bit a: axis a; a non-empty proper subset of the axes), without the image ever being written.
 * With n = 2^level, A the averaged and K the kept axes in ascending order: a bin is a pixel of the kept axes, index
 * sum p_K[i] n^i, and sums[k][bin], weights[bin] are [num_planes][n^|K|] and [n^|K|]. A reduced pixel of a bin has index
 * r = sum p_A[i] n^i < R = n^|A|. Chunks hold T8GPU_SAMPLE_AVERAGE_CHUNK consecutive r; in chunk c lane j of one wavefront adds
 * to +0 the pixels r = 4096 c + 64 t + j for t = 0 .. 63 in ascending order (r >= R skipped), the 64 lane values are combined
 * by the xor butterfly v[j] = v[j] + v[j ^ s], s = 32, 16, 8, 4, 2, 1, and the chunk values of a bin are added to +0 in
 * ascending chunk order; the same for the weights. With weights = NULL sums[k][bin] holds sum / weight, `fill` where the weight
 * is 0. For R > 4096 `scratch` must hold n^|K| ceil(R / 4096) (num_planes + 1) doubles (a second small kernel adds the chunks);
 * otherwise it may be NULL. host_average of t8gpu_amd/sample.py is the definition in numpy.
 * No atomics, no LDS. Return 0 without a launch for num_points = 0 (gather: or num_planes = 0); hipErrorInvalidValue, before any
 * launch, for dim outside {2, 3}, cells_per_axis outside {1, 4}, 2^31 or more owned cells, more than T8GPU_SAMPLE_PLANES
 * planes or a plane with q and d both NULL, a grid extent <= 0, level outside [0, D], uniform without a plane, a NULL array that would be used;
 * average also for dim level > 36, an axes_mask that is empty, full or names an axis >= dim, 2^31 or more wavefronts. */
#define T8GPU_SAMPLE_DEPTH 20
#define T8GPU_SAMPLE_PLANES 16
#define T8GPU_SAMPLE_AVERAGE_CHUNK 4096
typedef struct T8gpuSamplePlanes_f32 { const float* q[16]; const double* d[16]; } T8gpuSamplePlanes_f32;
typedef struct T8gpuSamplePlanes_f64 { const double* q[16]; const double* d[16]; } T8gpuSamplePlanes_f64;
typedef struct T8gpuSampleGrid { double lo[3]; double hi[3]; int32_t n[3]; int32_t pad; } T8gpuSampleGrid;
int t8gpu_hip_sample_locate(int dim, size_t num_points, const double* points, const uint64_t* keys, const int32_t* levels,
                            int num_elements, int cells_per_axis, int32_t* cells, void* stream);
int t8gpu_hip_sample_gather_f32(size_t num_points, const int32_t* cells, int num_planes, T8gpuSamplePlanes_f32 planes, double fill,
                                double* out, void* stream);
int t8gpu_hip_sample_gather_f64(size_t num_points, const int32_t* cells, int num_planes, T8gpuSamplePlanes_f64 planes, double fill,
                                double* out, void* stream);
int t8gpu_hip_sample_grid_f32(int dim, T8gpuSampleGrid grid, const uint64_t* keys, const int32_t* levels, int num_elements,
                              int cells_per_axis, int num_planes, T8gpuSamplePlanes_f32 planes, double fill, double* out,
                              int32_t* cells, void* stream);
int t8gpu_hip_sample_grid_f64(int dim, T8gpuSampleGrid grid, const uint64_t* keys, const int32_t* levels, int num_elements,
                              int cells_per_axis, int num_planes, T8gpuSamplePlanes_f64 planes, double fill, double* out,
                              int32_t* cells, void* stream);
int t8gpu_hip_sample_uniform_f32(int dim, int level, const uint64_t* keys, const int32_t* levels, int num_elements,
                                 int cells_per_axis, int num_planes, T8gpuSamplePlanes_f32 planes, double fill, double* sums,
                                 double* weights, void* stream);
int t8gpu_hip_sample_uniform_f64(int dim, int level, const uint64_t* keys, const int32_t* levels, int num_elements,
                                 int cells_per_axis, int num_planes, T8gpuSamplePlanes_f64 planes, double fill, double* sums,
                                 double* weights, void* stream);
int t8gpu_hip_sample_average_f32(int dim, int level, int axes_mask, const uint64_t* keys, const int32_t* levels, int num_elements,
                                 int cells_per_axis, int num_planes, T8gpuSamplePlanes_f32 planes, double fill, double* sums,
                                 double* weights, double* scratch, void* stream);
int t8gpu_hip_sample_average_f64(int dim, int level, int axes_mask, const uint64_t* keys, const int32_t* levels, int num_elements,
                                 int cells_per_axis, int num_planes, T8gpuSamplePlanes_f64 planes, double fill, double* sums,
                                 double* weights, double* scratch, void* stream);

/* ---- tracer particles on Cartesian forests, advected by Heun's method (csrc/hip/tracers.hip) ---------------
 * A particle is a coordinate x[dim] in double, not a member of a cell. The forest arguments (keys, levels, num_elements,
 * cells_per_axis) and the holding cell c of a point are those of the sampling section above. All arithmetic in double, every
 * operation rounded on its own (no fused multiply-add); the numpy functions host_velocity / host_map / host_predict /
 * host_correct of t8gpu_amd/tracers.py state the same arithmetic and are the definition.
 * Velocity at a point p: u_a = double(state.p[1 + a][c]) / double(state.p[0][c]) for a < dim and held = 1, or u = +0 and
 * held = 0 when no owned cell holds p. Never interpolated.
 * map(p), per axis a with the kinds sides.kind[2 a] (lower side) and sides.kind[2 a + 1] (upper side):
 *    periodic   y = p - floor(p), and y = 0 when that is >= 1
 *    wall       p < 0: y = -p (lower side);  p >= 1: y = 2 - p (upper side);  a result of exactly 1 becomes the largest double
 *               below 1
 *    open       p < 0 or p >= 1 on any axis: the particle has LEFT, y = p on every axis
 * and the particle is LOST when p is non-finite on any axis (this first), or, not having left, when some y is outside [0, 1).
 * Phases, for the particles with status ACTIVE only -- a LEFT or LOST particle is neither read nor written again:
 *    PREDICT  k1 = k.  held = 0: LOST, xs = x.  Else raw = x + dt k1 and xs = map(raw), flag = 0;  left: xs = raw, flag = 1
 *             (the status changes in CORRECT);  lost: status = LOST, xs = x, flag = 0.
 *    CORRECT  k2 = flag ? k1 : k.  flag = 0 and held = 0: LOST (x stays).  Else x = map(x + (0.5 dt) (k1 + k2)), the sum first;
 *             left: status = LEFT, x = the raw point;  lost: status = LOST, x stays.
 * t8gpu_hip_tracers_velocity: k[i dim + a], held[i] for points[i dim ..), every point whatever its status. hint[num_points]
 * (may be NULL) is one in/out element index per point: when it lies in [0, num_elements) and that element covers the point,
 * the binary search is skipped; it is range-checked before it is used, the result does not depend on what it held, and the
 * element found (-1: none) is written back.
 * t8gpu_hip_tracers_move: one phase from given k and held (e.g. summed over the ranks of a partitioned run: one rank holds a
 * point and contributes, the others contribute +0).
 * t8gpu_hip_tracers_step: both in one launch, from the same device functions: velocity at x (PREDICT) or xs (CORRECT) of the
 * ACTIVE particles, then the phase. `hint` as above, one array per phase.
 * One lane per particle, 256-lane workgroups, no atomics, no LDS. Return 0 without a launch for num_points = 0;
 * hipErrorInvalidValue, before any launch, for what the sampling calls refuse, a phase or side kind outside the codes below, a
 * periodic side whose opposite side is not periodic, a non-finite dt, a NULL array that would be used. */
#define T8GPU_TRACER_ACTIVE 0
#define T8GPU_TRACER_LEFT 1
#define T8GPU_TRACER_LOST 2
#define T8GPU_TRACER_PERIODIC 0
#define T8GPU_TRACER_WALL 1
#define T8GPU_TRACER_OPEN 2
#define T8GPU_TRACER_PREDICT 0
#define T8GPU_TRACER_CORRECT 1
typedef struct T8gpuTracerSides { int32_t kind[6]; } T8gpuTracerSides;
int t8gpu_hip_tracers_velocity_f32(int dim, size_t num_points, const double* points, const uint64_t* keys, const int32_t* levels,
                                   int num_elements, int cells_per_axis, T8gpuVars_f32 state, int32_t* hint, double* k, int32_t* held,
                                   void* stream);
int t8gpu_hip_tracers_velocity_f64(int dim, size_t num_points, const double* points, const uint64_t* keys, const int32_t* levels,
                                   int num_elements, int cells_per_axis, T8gpuVars_f64 state, int32_t* hint, double* k, int32_t* held,
                                   void* stream);
int t8gpu_hip_tracers_move(int dim, int phase, size_t num_points, double dt, T8gpuTracerSides sides, const double* k,
                           const int32_t* held, double* x, double* xs, double* k1, uint8_t* flag, uint8_t* status, void* stream);
int t8gpu_hip_tracers_step_f32(int dim, int phase, size_t num_points, double dt, T8gpuTracerSides sides, const uint64_t* keys,
                               const int32_t* levels, int num_elements, int cells_per_axis, T8gpuVars_f32 state, int32_t* hint,
                               double* x, double* xs, double* k1, uint8_t* flag, uint8_t* status, void* stream);
int t8gpu_hip_tracers_step_f64(int dim, int phase, size_t num_points, double dt, T8gpuTracerSides sides, const uint64_t* keys,
                               const int32_t* levels, int num_elements, int cells_per_axis, T8gpuVars_f64 state, int32_t* hint,
                               double* x, double* xs, double* k1, uint8_t* flag, uint8_t* status, void* stream);

/* ---- time-averaged flow statistics: running sums and what they give (csrc/hip/stats.hip) -------------
 * t8gpu_hip_stats_accumulate: for every owned cell i and slot k, sums[k plane_stride + i] += weight q_k(i), all arithmetic in
 * double whatever float_type is, gamma = 1.4, with m = (m_x, m_y, m_z):
 *    0      rho                          6      rho^2
 *    1-3    m_x, m_y, m_z                7      p^2
 *    4      E                            8-10   m_x m_x / rho, m_y m_y / rho, m_z m_z / rho
 *    5      p = 0.4 (E - |m|^2 / (2 rho))   11-13  m_x m_y / rho, m_x m_z / rho, m_y m_z / rho
 *                                        14     Mach = (|m| / rho) / sqrt(1.4 p / rho)
 * One launch on `stream`: no host sync, no allocation, no atomics; every state value is read once, every accumulator value
 * read once and written once. Cells [0, num_cells) only: ghost slots and spare capacity are neither read nor written.
 * Nothing is filtered: a non-finite or non-physical cell makes that cell's sums non-finite (the state monitor is the guard).
 * Two cells per lane -- 16-byte accesses of the accumulator rows and of fp64 state planes, 8-byte ones of fp32 state planes --
 * when the five state planes and sums are 16-byte aligned and plane_stride is even, a scalar form otherwise; both give the
 * same bits. The usual weight is the step size; the sums are time integrals of per-volume quantities, so the
 * AMR transfer (child = parent, coarsened = mean of the family) carries them exactly.
 * t8gpu_hip_stats_results: with W = total_weight and A_k = sums[k plane_stride + i], one launch that writes the planes of
 * `out` that are not NULL (doubles, one value per owned cell) and nothing else:
 *    0      mean_density     A0 / W                  10     density_rms   sqrt(max(0, A6 / W - (A0 / W)^2))
 *    1-3    mean_momentum    A1..3 / W               11     pressure_rms  sqrt(max(0, A7 / W - (A5 / W)^2))
 *    4      mean_energy      A4 / W                  12-17  reynolds_stress xx yy zz xy xz yz:
 *    5      mean_pressure    A5 / W                         A_(8+k) / W - A_i A_j / (A0 W), the mean of rho u_i'' u_j''
 *    6      mean_mach        A14 / W                 18     tke           0.5 (R_xx + R_yy + R_zz) / (A0 / W)
 *    7-9    mean_velocity    A1..3 / A0 (the Favre mean)
 * The second moments are raw sums: an rms far below about 1e-7 of the mean is rounding.
 * Return 0 without a launch for num_cells = 0; hipErrorInvalidValue, before any launch, for a NULL state plane or sums,
 * plane_stride < num_cells, or a total_weight that is not finite and > 0. */
#define T8GPU_STATS_PLANES 15
#define T8GPU_STATS_RESULT_PLANES 19
typedef struct T8gpuStatsPlanes { double* p[19]; } T8gpuStatsPlanes;
int t8gpu_hip_stats_accumulate_f32(size_t num_cells, T8gpuVars_f32 state, double weight, double* sums, size_t plane_stride,
                                   void* stream);
int t8gpu_hip_stats_accumulate_f64(size_t num_cells, T8gpuVars_f64 state, double weight, double* sums, size_t plane_stride,
                                   void* stream);
int t8gpu_hip_stats_results(size_t num_cells, const double* sums, size_t plane_stride, double total_weight, T8gpuStatsPlanes out,
                            void* stream);

/* ---- scale-free refinement indicator (csrc/hip/indicator.hip) ------------------------------
 * Loehner's estimator without cross terms, per axis, with a noise filter and a boundary closure. For cell c (an element, or a
 * subcell of a Subgrid block) and a scalar q, over the INTERIOR (sub-)faces s of c -- o the cell across, n_s the unit normal
 * outward from c, A_s the area, everything in double whatever float_type is:
 *    h = V^(1/dim)   (subcell: (V_block / S)^(1/rank));   d_s = (h_c + h_o) / 2;   w_s,a = A_s |n_s,a|,  a = x, y, z
 *    N_a = sum_s w_s,a (q_o - q_c) / d_s        D_a = sum_s w_s,a (|q_o - q_c| + filter (|q_o| + |q_c|)) / d_s
 *    b_a = sum_s A_s n_s,a    W_a = sum_s w_s,a    k_a = W_a > 0 ? max(0, 1 - |b_a| / W_a) : 0
 *    E_q = sqrt(sum_a (k_a N_a)^2) / sqrt(sum_a D_a^2)    (0 where the denominator is 0)
 * and E = the maximum of E_q over the quantities of quantity_mask: bit 0 density, 1 pressure, 2 mach, 3 entropy (the formulas
 * of the output fields above, gamma = 1.4). E is dimensionless, lies in [0, 1] and does not depend on the level. Boundary
 * faces add no term; k_a closes the cell: b_a is what its interior faces leave open, so a Cartesian cell at a wall has k_a = 0
 * along the wall normal, a cell with all faces interior k_a = 1. A face to a ghost slot is an interior face: the ghost state
 * (and, for the plain kernel, volume[ghost]) must be current. A uniform state gives exactly +0; a linear q on a uniform
 * Cartesian mesh gives exactly 0 when its differences are exact (the file is compiled without contraction into fused
 * multiply-adds for that). Non-finite or non-physical states: not specified. Gathers without atomics, summed in the order of
 * the output fields above (CSR order; inside a hanging face j-major, i-minor; in-block faces first): two calls, same bits.
 * Plain: one lane per owned element, writes out[num_elements]; dim is the mesh dimension of h (2 for a 2D mesh stored with
 * normal_dim = 3). Subgrid: writes cell_out[num_blocks S] (per subcell, storage order) and block_out[num_blocks] (the maximum
 * over the block's subcells); either may be NULL and is then left alone. Subgrid: A_s of a sub-face is min(h_c, h_o)^(rank - 1),
 * from the block volumes like the faces inside a block (on dyadic geometry the bits of face_surfaces / sub-faces; one source
 * of lengths keeps E scale-free where areas and volumes are rounded separately); face_surfaces must be given and is not read.
 * Returns 0 for n <= 0; hipErrorInvalidValue, before any launch, for a NULL state plane or connectivity pointer, an empty
 * mask, a bit above 3, filter < 0, normal_dim / dim / rank outside {2, 3}.
 * t8gpu_hip_indicator_spread: one buffer layer, out[e] = max(in[e], in[o] over the face neighbours o of e) for the owned
 * elements or blocks e; `in` has num_elements + ghosts entries, ghost entries are read; in != out. max is exact. */
#define T8GPU_INDICATOR_DENSITY 1u
#define T8GPU_INDICATOR_PRESSURE 2u
#define T8GPU_INDICATOR_MACH 4u
#define T8GPU_INDICATOR_ENTROPY 8u
int t8gpu_hip_plain_indicator_f32(int num_elements, int normal_dim, int dim, unsigned quantity_mask, double filter, T8gpuVars_f32 state,
                                  const float* volume, const int32_t* face_neighbors, const float* face_normals,
                                  const float* face_surfaces, const int32_t* csr_offsets, const int32_t* csr_entries, double* out,
                                  void* stream);
int t8gpu_hip_plain_indicator_f64(int num_elements, int normal_dim, int dim, unsigned quantity_mask, double filter, T8gpuVars_f64 state,
                                  const double* volume, const int32_t* face_neighbors, const double* face_normals,
                                  const double* face_surfaces, const int32_t* csr_offsets, const int32_t* csr_entries, double* out,
                                  void* stream);
int t8gpu_hip_subgrid_indicator_f32(int rank, int num_blocks, unsigned quantity_mask, double filter, T8gpuVars_f32 state,
                                    const float* volumes, const int32_t* face_neighbors, const int32_t* face_level_difference,
                                    const int32_t* face_neighbor_offset, const float* face_normals, const float* face_surfaces,
                                    const int32_t* csr_offsets, const int32_t* csr_entries, double* cell_out, double* block_out,
                                    void* stream);
int t8gpu_hip_subgrid_indicator_f64(int rank, int num_blocks, unsigned quantity_mask, double filter, T8gpuVars_f64 state,
                                    const double* volumes, const int32_t* face_neighbors, const int32_t* face_level_difference,
                                    const int32_t* face_neighbor_offset, const double* face_normals, const double* face_surfaces,
                                    const int32_t* csr_offsets, const int32_t* csr_entries, double* cell_out, double* block_out,
                                    void* stream);
int t8gpu_hip_indicator_spread(int num_elements, const double* in, const int32_t* face_neighbors, const int32_t* csr_offsets,
                               const int32_t* csr_entries, double* out, void* stream);

/* ---- AMR indicator and data transfer for plain elements---------------------------------
 * estimate_gradient<<<>>>: examples/compressible_euler/kernels.cu:471-501 (|rho_r - rho_l| added to both
 * neighbours; the reference accumulates into its Fluxes/Rho plane, any zeroed plane works). */
int t8gpu_hip_estimate_gradient_f32(int num_faces, const int32_t* face_neighbors, const int32_t* indices,
                                    const float* rho, float* gradient, void* stream);
int t8gpu_hip_estimate_gradient_f64(int num_faces, const int32_t* face_neighbors, const int32_t* indices,
                                    const double* rho, double* gradient, void* stream);
/* compute_refinement_criteria<<<>>>: examples/compressible_euler/solver.cu:231-241 (gradient / cbrt(volume)). */
int t8gpu_hip_refinement_criteria_f32(int num_elements, const float* gradient, const float* volume, float* criteria,
                                      void* stream);
int t8gpu_hip_refinement_criteria_f64(int num_elements, const double* gradient, const double* volume, double* criteria,
                                      void* stream);
/* adapt_variables_and_volume<<<>>>: t8gpu/mesh/mesh_manager.inl:165-193. adapt_data[n_new+1] = first old element of
 * each new element (mesh_manager.inl:258-281): equal neighbours = children of a refined element (injection, volume
 * / 2^dim), difference 2^dim = coarsened family (mean, volume * 2^dim). dim = 3 reproduces the reference's
 * hard-coded factors 0.125 / 8.0; pass 2 for quad forests. */
int t8gpu_hip_adapt_variables_and_volume_f32(int num_new_elements, int dim, const int32_t* adapt_data,
                                             T8gpuVars_f32 old_variables, T8gpuVars_f32 new_variables,
                                             const float* volume_old, float* volume_new, void* stream);
int t8gpu_hip_adapt_variables_and_volume_f64(int num_new_elements, int dim, const int32_t* adapt_data,
                                             T8gpuVars_f64 old_variables, T8gpuVars_f64 new_variables,
                                             const double* volume_old, double* volume_new, void* stream);
/* device half of partition_data<<<>>> (mesh_manager.inl:626-643): a contiguous run of elements <-> one message of
 * 6 planes (5 variables + volume) of n values. */
int t8gpu_hip_gather_elements_f32(int n, int first, T8gpuVars_f32 variables, const float* volume, float* out, void* stream);
int t8gpu_hip_gather_elements_f64(int n, int first, T8gpuVars_f64 variables, const double* volume, double* out, void* stream);
int t8gpu_hip_scatter_elements_f32(int n, int first, const float* in, T8gpuVars_f32 variables, float* volume, void* stream);
int t8gpu_hip_scatter_elements_f64(int n, int first, const double* in, T8gpuVars_f64 variables, double* volume, void* stream);

/* MeshManager::partition / SubgridMeshManager::partition, device half, over RCCL (mesh_manager.inl:626-723,
 * subgrid_mesh_manager.inl:1217-1369): the reference's new owner PULLS an element's variables through CUDA-IPC pointers
 * (partition_data<<<>>>), here the old owner SENDS. Elements move in contiguous runs of the space-filling curve; run j of the
 * send list = elements [send_first[j], + send_count[j]) of the five `src` planes and of `src_volume` (cells_per_element
 * values per element and variable, one volume per element) to rank send_peer[j]; the receive list likewise into `dst` /
 * `dst_volume`. Six messages per run straight between the planes, one RCCL group per call; runs whose peer is `my_rank` are
 * device copies (the i-th such send pairs with the i-th such receive) and `comm` may be NULL if there are no others.
 * All index arrays on the HOST. Collective over the ranks that exchange runs. */
int t8gpu_hip_repartition_f32(void* comm, int my_rank, int n_send, const int32_t* send_peer, const int32_t* send_first,
                              const int32_t* send_count, int n_recv, const int32_t* recv_peer, const int32_t* recv_first,
                              const int32_t* recv_count, T8gpuVars_f32 src, const float* src_volume, T8gpuVars_f32 dst,
                              float* dst_volume, int cells_per_element, void* stream);
int t8gpu_hip_repartition_f64(void* comm, int my_rank, int n_send, const int32_t* send_peer, const int32_t* send_first,
                              const int32_t* send_count, int n_recv, const int32_t* recv_peer, const int32_t* recv_first,
                              const int32_t* recv_count, T8gpuVars_f64 src, const double* src_volume, T8gpuVars_f64 dst,
                              double* dst_volume, int cells_per_element, void* stream);
/* every rank's chunk mine[offsets[rank + 1] - offsets[rank]] of a distributed array of doubles to every rank's
 * all[offsets[nranks]] (device pointers, offsets on the host): how the refinement criteria of a partitioned adapt travel
 * (the reference's adapt callback reads per-element criteria of its own rank; with a replicated forest description every
 * rank evaluates it on the whole array). Collective. */
int t8gpu_hip_comm_allgatherv_f64(void* comm, int rank, int nranks, const double* mine, double* all, const int64_t* offsets,
                                  void* stream);

/* ---- AMR indicator and data transfer for Subgrid<4,4> / Subgrid<4,4,4> blocks -------------
 * compute_refinement_criteria<Subgrid><<<>>>: examples/subgrid/kernels.inl:1110-1168 (discrete H1 seminorm of the
 * density inside a block / block volume). */
int t8gpu_hip_subgrid_refinement_criteria_f32(int rank, int num_elements, const float* rho, const float* volumes,
                                              float* criteria, void* stream);
int t8gpu_hip_subgrid_refinement_criteria_f64(int rank, int num_elements, const double* rho, const double* volumes,
                                              double* criteria, void* stream);
/* adapt_variables<Subgrid><<<>>> + adapt_volume<Subgrid><<<>>>: t8gpu/mesh/subgrid_mesh_manager.inl:246-425
 * (refined block: injection from the parent's octant; coarsened block: mean of the 2^rank fine cells). */
int t8gpu_hip_subgrid_adapt_variables_and_volume_f32(int rank, int num_new_elements, const int32_t* adapt_data,
                                                     T8gpuVars_f32 old_variables, T8gpuVars_f32 new_variables,
                                                     const float* volume_old, float* volume_new, void* stream);
int t8gpu_hip_subgrid_adapt_variables_and_volume_f64(int rank, int num_new_elements, const int32_t* adapt_data,
                                                     T8gpuVars_f64 old_variables, T8gpuVars_f64 new_variables,
                                                     const double* volume_old, double* volume_new, void* stream);

/* ---- read-back for the VTK writers ---------------------------------------------------------
 * column_major_to_z_order<Subgrid><<<>>>: subgrid_mesh_manager.inl:1008-1049 -- cell (i,j,k) of every block to
 * the z-order position it has once the block is refined uniformly twice (how the reference hands Subgrid
 * data to t8_forest_write_vtk_ext). from != to; both [num_elements * 4^rank]. */
int t8gpu_hip_column_major_to_z_order_f32(int rank, int num_elements, const float* from, float* to, void* stream);
int t8gpu_hip_column_major_to_z_order_f64(int rank, int num_elements, const double* from, double* to, void* stream);
/* get_host_scalar_variable / get_host_vector_variable (mesh_manager.inl:516-586, subgrid_mesh_manager.inl:
 * 1140-1183): the device-side half -- cast to double, vectors interleaved xyz -- so that the host needs one
 * copy of `out` (device memory, n resp. 3 n doubles). */
int t8gpu_hip_host_scalar_variable_f32(size_t n, const float* variable, double* out, void* stream);
int t8gpu_hip_host_scalar_variable_f64(size_t n, const double* variable, double* out, void* stream);
int t8gpu_hip_host_vector_variable_f32(size_t n, const float* v0, const float* v1, const float* v2, double* out, void* stream);
int t8gpu_hip_host_vector_variable_f64(size_t n, const double* v0, const double* v1, const double* v2, double* out, void* stream);

/* ---- diagnostics -----------------------------------------------------------------------------------------
 * Element-wise evaluation of the fast-tier scalar helpers (reciprocal / division / sqrt / log without the
 * IEEE special-case handling, and the logarithmic mean built on them: kernels.cu:24-36) so that their
 * accuracy can be pinned against a host libm. out[i] = op(a[i], b[i]); b may be null for unary ops. */
enum {
  T8GPU_PROBE_RCP = 0,
  T8GPU_PROBE_DIV = 1,
  T8GPU_PROBE_SQRT = 2,
  T8GPU_PROBE_LOG = 3,
  T8GPU_PROBE_LN_MEAN = 4,    /* fast tier: from the two values and the difference of their logs */
  T8GPU_PROBE_LN_MEAN_REF = 5, /* compat tier: the reference formula, IEEE division and library log */
  T8GPU_PROBE_LOG_TAB = 6,     /* the table-driven fp64 log of the plain tile kernels (fp32: same as LOG) */
  T8GPU_PROBE_SQRT_RATIO = 7,  /* sqrt(a / b) through one reciprocal square root (the sound speed of the KEPES flux) */
  T8GPU_PROBE_DIV_SHARED = 8,  /* a / b from a reciprocal that several quotients share */
  T8GPU_PROBE_RSQRT = 9,       /* 1 / sqrt(a): the normalisation of the per-face frames of curved meshes */
  T8GPU_PROBE_RK_SCALE = 10,   /* a / b = dt / vol of the RK update (exact exponent arithmetic where vol is a power of two) */
  T8GPU_PROBE_LN_MEAN_RS = 11, /* LN_MEAN with s = b + a and its shared reciprocal handed in (no kernel calls this form: probe only) */
  T8GPU_PROBE_LN_MEAN_INV_RS = 12 /* 1 / (logarithmic mean), same arguments: the form the KEPES flux takes for beta */
};
int t8gpu_hip_math_probe_f32(int op, int n, const float* a, const float* b, float* out, void* stream);
int t8gpu_hip_math_probe_f64(int op, int n, const double* a, const double* b, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* T8GPU_HIP_H */
