// stepper.hip -- native driver of one SSP-RK3 step: iterate() without any host language in the loop.
//
// Mirrors CompressibleEulerSolver::iterate (examples/compressible_euler/solver.cu:75-175) for the fused
// tier: 3 x [ghost exchange || interior tiles -> ghost-reading tiles]. Where the reference brackets
// every kernel with cudaDeviceSynchronize + MPI_Barrier (5 pairs per step) this driver only enqueues:
// ordering is carried by two HIP streams and their events, the ghost exchange is one RCCL group of
// ncclSend/ncclRecv per neighbour rank over xGMI, and the host returns immediately.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "ranges.hpp"
#include "t8gpu_hip.h"

namespace {

inline int nccl_code(ncclResult_t r) { return r == ncclSuccess ? 0 : 10000 + static_cast<int>(r); }

#define T8_HIP_TRY(expr)                                  \
  do {                                                    \
    hipError_t e__ = (expr);                              \
    if (e__ != hipSuccess) return static_cast<int>(e__);  \
  } while (0)
#define T8_TRY(expr)            \
  do {                          \
    int c__ = (expr);           \
    if (c__ != 0) return c__;   \
  } while (0)

// Host cost of the enqueue by category (T8GPU_STEPPER_PROFILE=1; printed when the stepper is destroyed): where the time of a
// multi-rank stage goes on the host -- kernel launches, the RCCL group, event records / waits.
struct HostProfile {
  bool   on = std::getenv("T8GPU_STEPPER_PROFILE") != nullptr;
  double ns[4] = {0, 0, 0, 0};
  long   calls[4] = {0, 0, 0, 0};
};
HostProfile& host_profile() {
  static HostProfile p;
  return p;
}
struct HostTimer {   // cat: 0 kernel launch, 1 RCCL group, 2 event record, 3 stream wait
  int cat;
  std::chrono::steady_clock::time_point t0;
  explicit HostTimer(int c) : cat(c) {
    if (host_profile().on) t0 = std::chrono::steady_clock::now();
  }
  ~HostTimer() {
    if (!host_profile().on) return;
    static std::mutex m;   // (two host threads enqueue: stepper lanes)
    std::lock_guard<std::mutex> lk(m);
    host_profile().ns[cat] += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
    host_profile().calls[cat]++;
  }
};

inline bool env_on(const char* name) {   // set, not empty and not "0..."
  const char* v = std::getenv(name);
  return v && v[0] != '\0' && v[0] != '0';
}

struct Stepper {
  T8gpuPlainPlan   plan{};      // plain elements: units = tiles of the plan
  T8gpuSubgridPlan splan{};     // Subgrid blocks: units = blocks in block_order position order
  bool             subgrid = false;
  bool           has_halo = false;  // the stepper has peers: iterate() runs the two-lane driver
  T8gpuHalo      halo{};
  std::vector<int32_t> peers, send_off, recv_off;
  hipStream_t    comm_stream = nullptr;   // the comm lane's stream
  hipEvent_t     ev_state = nullptr;      // step entry
  int            timing = 0;        // 0 = off, n = time the stage kernels of every n-th step
  int            stages_timed = 0;
  // hipGraph replay of a whole single-rank iterate_steps() call (t8gpu_hip_plain_stepper_graph): the enqueue sequence is
  // captured once per distinct argument set on an internal origin stream and replayed with one hipGraphLaunch
  int             graph_mode = 0;       // 0 off, 1 on
  hipStream_t     graph_stream = nullptr;
  hipEvent_t      ev_graph_in = nullptr, ev_graph_out = nullptr;
  struct GraphEntry {               // one executable per argument set; a step loop alternates between two (the roles of
    hipGraphExec_t exec = nullptr;  // prev / next swap with every odd n_steps), so the cache holds a few
    unsigned char  key[96] = {0};
    unsigned long  used = 0;
    int            speed_stages = 0;   // stages of the captured sequence that write the speed estimates
  };
  GraphEntry      graph_cache[4];
  unsigned long   graph_clock = 0;
  int             graph_captures = 0, graph_replays = 0;
  // the planar 2D stage (t8gpu_hip.h: t8gpu_hip_stepper_set_planar; planar_decide below)
  int             planar_mode = 1;      // 0 never, 1 where the check is amortised, 2 whenever proven
  bool            planar_now  = false;  // the current call runs planar
  int             planar_last = 0;      // what the last call did
  uint32_t*       d_bits = nullptr;     // device: OR of the bits of the four z-momentum planes
  uint32_t*       h_bits = nullptr;     // pinned host copy
  // the per-face speed estimates (t8gpu_hip.h: t8gpu_hip_stepper_set_speed_every_step; stage_args below)
  // 0 the third stage of a call's last step writes them, 1 the third stage of every step; T8GPU_SPEED_EVERY_STEP in the
  // environment sets the mode a new stepper starts in
  int             speed_every_step = env_on("T8GPU_SPEED_EVERY_STEP") ? 1 : 0;
  int             speed_stages = 0;     // stages of the last call that were handed the array

  // ---- lanes: the two-lane driver (iterate_lanes); a single rank launches on the deep lane ---------------------------------
  static constexpr int kRing = 4;
  struct Lane {
    hipStream_t        stream = nullptr;
    hipEvent_t         ring[kRing] = {nullptr, nullptr, nullptr, nullptr};   // the record of stage g uses ring[g % kRing]
    std::atomic<long>  recorded{0};     // stages of the current call whose record has been issued
    std::vector<hipEvent_t> pool;       // timing events of this lane: start / stop pairs of the stage-kernel launches
    size_t             used = 0;
  };
  Lane            deep_lane, comm_lane;     // C tiles | RCCL, A tiles, B tiles
  bool            zero_copy = false;        // ghost window: A tiles read the receive buffer and fill the send buffer themselves
  T8gpuPlainPlan  plan_a{};                 // `plan` + the ghost window (launches of the A class)
  void*           d_send_map = nullptr;
  void*           d_send_list = nullptr;
  std::atomic<bool> lane_abort{false};
  // the comm lane's host thread (enqueues its lane while the caller's thread enqueues the deep lane)
  std::thread               worker;
  std::mutex                mu;
  std::condition_variable   cv;
  std::function<int()>      job;            // guarded by mu
  std::atomic<int>          job_state{0};   // 0 idle, 1 posted, 2 done
  int                       job_rc = 0;
  bool                      worker_exit = false;
  int                       device = 0;
  bool                      threads = true;
  double                    host_ns = 0;    // host time inside iterate_lanes (both threads overlap: wall time of the call)
  long                      host_steps = 0;
};

template <class T>
ncclDataType_t nccl_type();
template <>
ncclDataType_t nccl_type<float>() { return ncclFloat; }
template <>
ncclDataType_t nccl_type<double>() { return ncclDouble; }

template <class T, class V>
int halo_pack(const T8gpuHalo& h, V state, hipStream_t s) {
  HostTimer ht(0);
  const int cells = h.cells_per_element < 1 ? 1 : h.cells_per_element;
  if constexpr (sizeof(T) == 4)
    return t8gpu_hip_halo_pack_f32(h.n_send, cells, h.send_idx, state, static_cast<T*>(h.sendbuf), s);
  else
    return t8gpu_hip_halo_pack_f64(h.n_send, cells, h.send_idx, state, static_cast<T*>(h.sendbuf), s);
}

template <class T, class V>
int halo_unpack(const T8gpuHalo& h, V state, hipStream_t s) {
  HostTimer ht(0);
  const int cells = h.cells_per_element < 1 ? 1 : h.cells_per_element;
  if constexpr (sizeof(T) == 4)
    return t8gpu_hip_halo_unpack_f32(h.num_ghosts, h.num_elements, cells, static_cast<const T*>(h.recvbuf), state, s);
  else
    return t8gpu_hip_halo_unpack_f64(h.num_ghosts, h.num_elements, cells, static_cast<const T*>(h.recvbuf), state, s);
}

// The RCCL group of one exchange: per peer, its ghosts into the receive buffer and what it mirrors out of the send buffer.
template <class T>
int exchange_wire(const T8gpuHalo& h, const int32_t* peers, const int32_t* send_off, const int32_t* recv_off, hipStream_t s) {
  HostTimer   ht(1);
  T*          sb    = static_cast<T*>(h.sendbuf);
  T*          rb    = static_cast<T*>(h.recvbuf);
  const int   cells = h.cells_per_element < 1 ? 1 : h.cells_per_element;
  ncclComm_t  comm  = static_cast<ncclComm_t>(h.comm);
  T8_TRY(nccl_code(ncclGroupStart()));
  for (int j = 0; j < h.n_peers; j++) {
    const size_t w  = 5 * static_cast<size_t>(cells);   // values per element on the wire
    const size_t rc = w * static_cast<size_t>(recv_off[j + 1] - recv_off[j]);
    const size_t sc = w * static_cast<size_t>(send_off[j + 1] - send_off[j]);
    if (rc) T8_TRY(nccl_code(ncclRecv(rb + w * static_cast<size_t>(recv_off[j]), rc, nccl_type<T>(), peers[j], comm, s)));
    if (sc) T8_TRY(nccl_code(ncclSend(sb + w * static_cast<size_t>(send_off[j]), sc, nccl_type<T>(), peers[j], comm, s)));
  }
  T8_TRY(nccl_code(ncclGroupEnd()));
  return 0;
}

// t8gpu_hip_halo_exchange_*: pack -> RCCL group -> unpack, all on s
template <class T, class V>
int exchange(const T8gpuHalo& h, V state, hipStream_t s) {
  if (h.n_peers <= 0) return 0;
  T8_TRY((halo_pack<T, V>(h, state, s)));
  T8_TRY(exchange_wire<T>(h, h.peers, h.send_off, h.recv_off, s));
  return halo_unpack<T, V>(h, state, s);
}

template <class V, class T>
V step_vars(T* planes, size_t stride, int step) {
  V v;
  for (int k = 0; k < 5; k++) v.p[k] = planes + (static_cast<size_t>(step) * 5 + k) * stride;
  return v;
}

// Stage g of an iterate_steps() call: stage k = g % 3 of its step, the planes it reads (previous state, stage source) and writes.
template <class T, class V>
struct StageArgs {
  int k;
  V   pv, sv, ov;
  T*  stage_speed;
};
template <class T, class V>
StageArgs<T, V> stage_args(T* planes, size_t stride, int prev, int next, T* speed, int g, int n_steps, bool every_step) {
  StageArgs<T, V> a;
  a.k          = g % 3;
  const int pr = (g / 3) % 2 == 0 ? prev : next, nx = (g / 3) % 2 == 0 ? next : prev;
  const int src = a.k == 0 ? pr : a.k, dst = a.k == 2 ? nx : a.k + 1;   // Step1 = 1, Step2 = 2 (solver.h:24-31)
  a.pv = step_vars<V>(planes, stride, pr);
  a.sv = step_vars<V>(planes, stride, src);
  a.ov = step_vars<V>(planes, stride, dst);
  // The per-face speed estimates are rewritten by every stage and read only between CALLS (compute_timestep uses
  // those "computed at the last step of the last timestepping", solver.h:88-91): only the third stage of the call's
  // last step writes them. Every third stage would store the whole array (one value per face) and the next step
  // overwrite it before anyone can look: same contents on return, F + B stores less per intermediate step.
  // every_step (t8gpu_hip_stepper_set_speed_every_step): the third stage of every step, for A/B runs.
  a.stage_speed = a.k == 2 && (every_step || g == 3 * n_steps - 1) ? speed : nullptr;
  return a;
}

int lane_tick(Stepper::Lane& L) {
  if (L.used == L.pool.size()) {
    hipEvent_t e;
    T8_HIP_TRY(hipEventCreate(&e));
    L.pool.push_back(e);
  }
  T8_HIP_TRY(hipEventRecord(L.pool[L.used++], L.stream));
  return 0;
}

// units [b, b + n) of stage a on lane L; `sample`: bracketed by the lane's timing events
template <class T, class V>
int launch_stage(Stepper* S, Stepper::Lane& L, int kind, const T8gpuPlainPlan* plan, const StageArgs<T, V>& a, int b, int n,
                 const T* vol, T dt, bool sample) {
  if (n <= 0) return 0;
  HostTimer ht(0);
  if (sample) T8_TRY(lane_tick(L));
  const int planar = S->planar_now ? 1 : 0;   // (0: exactly t8gpu_hip_plain_fused_stage_*)
  if constexpr (sizeof(T) == 4) {
    if (S->subgrid)
      T8_TRY(t8gpu_hip_subgrid_fused_stage_f32(kind, a.k + 1, &S->splan, b, n, a.pv, a.sv, a.ov, vol, dt, L.stream));
    else
      T8_TRY(t8gpu_hip_plain_fused_stage_planar_f32(kind, a.k + 1, plan, b, n, a.pv, a.sv, a.ov, vol, dt, a.stage_speed, L.stream, planar));
  } else {
    if (S->subgrid)
      T8_TRY(t8gpu_hip_subgrid_fused_stage_f64(kind, a.k + 1, &S->splan, b, n, a.pv, a.sv, a.ov, vol, dt, L.stream));
    else
      T8_TRY(t8gpu_hip_plain_fused_stage_planar_f64(kind, a.k + 1, plan, b, n, a.pv, a.sv, a.ov, vol, dt, a.stage_speed, L.stream, planar));
  }
  if (sample) T8_TRY(lane_tick(L));
  return 0;
}


// ---- the two-lane driver: a stepper with peers ------------------------------------------------------------------------
// At 8 ranks the exchange chain of a stage is its critical path (the RCCL kernel alone takes ~50 us beside the tile kernels),
// and the host needs about as long to enqueue a stage as the GPU to run it (profiles/r04_halo_*.md). This driver shortens both:
//   * GHOST WINDOW (plain 2D / tile plans): the A tiles (the tiles that read ghost slots) read their ghosts straight from the
//     receive buffer of the exchange, in its wire format, and write the elements a peer mirrors into the send buffer in their
//     RK epilogue (T8gpuPlainPlan::ghost_buf / send_map, fused_common.hpp). No pack kernel (except for the first stage of a
//     call, whose source state comes from outside) and no unpack kernel: the chain is RCCL -> A tiles.
//   * TWO LANES, each depending only on the OTHER lane's PREVIOUS stage:
//       deep lane (caller's stream)  : [A_(g-1)] -> I_g          I = all interior tiles [0, n_interior): one launch
//       comm lane                    : RCCL_g -> [I_(g-1)] -> A_g
//     I_g reads what I- and A-tiles of stage g-1 wrote; A_g reads the ghosts of stage g and what A- and I-tiles of stage
//     g-1 wrote; RCCL_g sends what A_(g-1) put into the send buffer. Both waits refer to work that ended most of a stage
//     earlier (the chain RCCL + A, ~35 us, is shorter than I, ~45 us, beside it), so neither lane ever stalls on the
//     other and the long launches run back to back.
//     The RCCL kernel needs 264 VGPRs per lane (rcclGenericKernel<1, false> of RCCL 2.26.6 for gfx950): beside tile kernels
//     that hold 3 x 160 of a SIMD's 512 it is not dispatched before the tile launch has handed out its last workgroup.
//     Here it is queued a whole stage ahead of its deadline and slips in at the drain between two interior launches.
//     (A plan WITH a deep / near-boundary split of its interior tiles -- Subgrid plans, plain plans built without flag 32 -- runs
//     C_g on the deep lane behind [B_(g-1)] and B_g on the comm lane behind A_g and [C_(g-1)].)
//   * The comm lane is enqueued by a HOST THREAD of its own while the caller's thread enqueues the deep lane; the threads
//     meet through two counters (a wait on stage g's event may only be issued once the other thread has recorded it).
// Plans the ghost window does not cover (Subgrid blocks, 3D patch tiles) run the same two lanes with the pack / unpack
// kernels around the group.
// (Rounds 1-3 ran a three-stream pipeline instead -- C, B and pack -> RCCL -> unpack -> A on a stream each; its deep tiles
//  waited across queues for the exchange chain, ~10 us of idle GPU per stage. Replaced in round 4: DESIGN.md section 6.)
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#endif
}

// wait until the other lane's host thread has RECORDED stage g (only then may a wait on that event be issued)
inline bool lane_wait_recorded(Stepper* S, Stepper::Lane& other, long g) {
  while (other.recorded.load(std::memory_order_acquire) <= g) {
    if (S->lane_abort.load(std::memory_order_relaxed)) return false;
    cpu_relax();
  }
  return true;
}

void worker_main(Stepper* S) {
  (void)hipSetDevice(S->device);
  std::unique_lock<std::mutex> lk(S->mu);
  for (;;) {
    // spin briefly for the next call (a step loop calls again within microseconds), then sleep
    lk.unlock();
    const auto t0 = std::chrono::steady_clock::now();
    while (S->job_state.load(std::memory_order_acquire) != 1 &&
           std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() < 300.0)
      cpu_relax();
    lk.lock();
    S->cv.wait(lk, [&] { return S->job_state.load(std::memory_order_acquire) == 1 || S->worker_exit; });
    if (S->worker_exit) return;
    std::function<int()> job = std::move(S->job);
    lk.unlock();
    const int rc = job();
    lk.lock();
    S->job_rc = rc;
    S->job_state.store(2, std::memory_order_release);
  }
}

template <class T, class V>
int iterate_lanes(Stepper* S, int kind, T* planes, size_t stride, const T* vol, int prev, int next, T dt, T* speed, int n_steps,
                  hipStream_t s) {
  if (n_steps <= 0) return 0;
  const auto host_t0 = std::chrono::steady_clock::now();
  const int  nt = S->subgrid ? S->splan.num_elements : S->plan.ntiles;
  const int  ni = S->subgrid ? S->splan.n_interior_blocks : S->plan.n_interior_tiles;
  const int  ndeep = S->subgrid ? S->splan.n_deep_blocks : S->plan.n_deep_tiles;
  // The plan decides: one interior class (n_deep = n_interior; t8gpu_plan_plain_create_ex flag 32, what partitioned meshes get)
  // -> the interior tiles are ONE launch per stage on the deep lane; a deep / near-boundary split in the plan (Subgrid plans,
  // plain plans built without the flag) -> C_g on the deep lane, B_g behind A_g on the comm lane. n_deep = 0 ("unknown"):
  // every interior tile counts as near-boundary.
  const int  nd = (ndeep > 0 && ndeep <= ni) ? ndeep : 0;
  const int  G  = 3 * n_steps;
  t8gpu_hip::Range whole("t8gpu.iterate_steps (exchange -> ghost-reading tiles || interior tiles, two lanes)");
  Stepper::Lane& DL = S->deep_lane;
  Stepper::Lane& XL = S->comm_lane;
  DL.stream = s;
  XL.stream = S->comm_stream;
  DL.recorded.store(0, std::memory_order_relaxed);
  XL.recorded.store(0, std::memory_order_relaxed);
  S->lane_abort.store(false, std::memory_order_relaxed);
  const int timing = S->timing;
  if (timing > 0) S->stages_timed += 3 * ((n_steps + timing - 1) / timing);
  const bool every_step = S->speed_every_step != 0;
  S->speed_stages = 0;

  // entry: the lanes see everything the caller queued on s
  T8_HIP_TRY(hipEventRecord(S->ev_state, s));
  T8_HIP_TRY(hipStreamWaitEvent(XL.stream, S->ev_state, 0));
  if (DL.stream != s) T8_HIP_TRY(hipStreamWaitEvent(DL.stream, S->ev_state, 0));

  auto launch = [=](Stepper::Lane& L, const T8gpuPlainPlan* plan, const StageArgs<T, V>& a, int b, int n, bool sample) -> int {
    return launch_stage<T, V>(S, L, kind, plan, a, b, n, vol, dt, sample);
  };

  // ---- comm lane, stage g: RCCL_g -> A_g -> [C_(g-1)] -> B_g --------------------------------------------------------------
  auto comm_stage = [=, &DL, &XL](int g) -> int {
    const T8gpuHalo&      h      = S->halo;
    const StageArgs<T, V> a      = stage_args<T, V>(planes, stride, prev, next, speed, g, n_steps, every_step);
    const bool            sample = timing > 0 && (g / 3) % timing == 0;
    if (!S->zero_copy || g == 0)   // (ghost window: the A tiles of stage g-1 have filled the send buffer)
      T8_TRY((halo_pack<T, V>(h, a.sv, XL.stream)));
    T8_TRY(exchange_wire<T>(h, S->peers.data(), S->send_off.data(), S->recv_off.data(), XL.stream));
    if (!S->zero_copy) T8_TRY((halo_unpack<T, V>(h, a.sv, XL.stream)));
    auto wait_deep = [&]() -> int {   // the deep lane's stage g-1
      if (g == 0 || nd == 0) return 0;
      if (!lane_wait_recorded(S, DL, g - 1)) return 0;
      HostTimer ht(3);
      T8_HIP_TRY(hipStreamWaitEvent(XL.stream, DL.ring[(g - 1) % Stepper::kRing], 0));
      return 0;
    };
    if (nd == ni) T8_TRY(wait_deep());                                                   // A_g <- interior_(g-1)
    T8_TRY(launch(XL, S->zero_copy ? &S->plan_a : &S->plan, a, ni, nt - ni, sample));   // A_g
    if (nd < ni) {
      T8_TRY(wait_deep());                                                               // B_g <- C_(g-1)
      T8_TRY(launch(XL, &S->plan, a, nd, ni - nd, sample));                              // B_g
    }
    {
      HostTimer ht(2);
      T8_HIP_TRY(hipEventRecord(XL.ring[g % Stepper::kRing], XL.stream));
    }
    XL.recorded.store(g + 1, std::memory_order_release);
    return 0;
  };
  // ---- deep lane, stage g: [B_(g-1)] -> C_g --------------------------------------------------------------------------------
  auto deep_stage = [=, &DL, &XL](int g) -> int {
    const StageArgs<T, V> a      = stage_args<T, V>(planes, stride, prev, next, speed, g, n_steps, every_step);
    const bool            sample = timing > 0 && (g / 3) % timing == 0;
    if (a.stage_speed) S->speed_stages++;   // (counted on this lane only: the comm lane runs the same stage's other tiles)
    if (nd > 0) {
      if (g > 0) {
        if (!lane_wait_recorded(S, XL, g - 1)) return 0;
        HostTimer ht(3);
        T8_HIP_TRY(hipStreamWaitEvent(DL.stream, XL.ring[(g - 1) % Stepper::kRing], 0));
      }
      T8_TRY(launch(DL, &S->plan, a, 0, nd, sample));                                    // C_g
      HostTimer ht(2);
      T8_HIP_TRY(hipEventRecord(DL.ring[g % Stepper::kRing], DL.stream));
    }
    DL.recorded.store(g + 1, std::memory_order_release);
    return 0;
  };
  // (a lane that fails must not leave the other one's host thread waiting for its records)
  auto run_lane = [S, G](const std::function<int(int)>& stage) -> int {
    for (int g = 0; g < G; g++) {
      const int rc = stage(g);
      if (rc != 0) {
        S->lane_abort.store(true, std::memory_order_relaxed);
        return rc;
      }
      if (S->lane_abort.load(std::memory_order_relaxed)) return 0;
    }
    return 0;
  };

  int rc_comm = 0, rc_deep = 0;
  if (S->threads) {
    if (!S->worker.joinable()) {
      (void)hipGetDevice(&S->device);
      S->worker = std::thread(worker_main, S);
    }
    {
      std::lock_guard<std::mutex> lk(S->mu);
      S->job = [&]() { return run_lane(comm_stage); };
      S->job_state.store(1, std::memory_order_release);
    }
    S->cv.notify_one();
    rc_deep = run_lane(deep_stage);
    while (S->job_state.load(std::memory_order_acquire) != 2) cpu_relax();
    {
      std::lock_guard<std::mutex> lk(S->mu);
      rc_comm = S->job_rc;
      S->job_state.store(0, std::memory_order_release);
    }
  } else {
    // one host thread: stage by stage, the deep lane first (every wait for a record is then satisfied when it is reached)
    for (int g = 0; g < G && rc_deep == 0 && rc_comm == 0; g++) {
      rc_deep = deep_stage(g);
      if (rc_deep == 0) rc_comm = comm_stage(g);
    }
  }
  // exit: everything is ordered on s again
  T8_HIP_TRY(hipStreamWaitEvent(s, XL.ring[(G - 1) % Stepper::kRing], 0));
  if (DL.stream != s && nd > 0) T8_HIP_TRY(hipStreamWaitEvent(s, DL.ring[(G - 1) % Stepper::kRing], 0));
  S->host_ns += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - host_t0).count();
  S->host_steps += n_steps;
  return rc_deep != 0 ? rc_deep : rc_comm;
}

// n_steps SSP-RK3 steps; (prev, next) are the roles of the FIRST step, they swap from step to step (solver.cu:76).
// A stepper with peers runs the two-lane driver above. A single rank launches all its units [0, nt) once per stage on the
// caller's stream (the deep lane's stream for the call, whose events time the sampled steps).
// Subgrid blocks run through the same drivers (SubgridCompressibleEulerSolver::iterate, examples/subgrid/solver.inl:
// 152-266): units are blocks in the plan's position order (deep interior, near-boundary, ghost-touching), a ghost
// block mirrors all 4^rank subcells, `vol` is the separate per-block volume array of SubgridMemoryManager.
template <class T, class V>
int iterate(Stepper* S, int kind, T* planes, size_t stride, const T* vol, int prev, int next, T dt, T* speed, int n_steps,
            hipStream_t s) {
  if (S->has_halo) return iterate_lanes<T, V>(S, kind, planes, stride, vol, prev, next, dt, speed, n_steps, s);
  const int nt = S->subgrid ? S->splan.num_elements : S->plan.ntiles;
  t8gpu_hip::Range whole("t8gpu.iterate_steps");
  static const char* const stage_name[3] = {"t8gpu.rk_stage1", "t8gpu.rk_stage2", "t8gpu.rk_stage3"};
  Stepper::Lane& L = S->deep_lane;
  L.stream = s;
  const bool every_step = S->speed_every_step != 0;
  S->speed_stages = 0;
  for (int g = 0; g < 3 * n_steps; g++) {
    const StageArgs<T, V> a = stage_args<T, V>(planes, stride, prev, next, speed, g, n_steps, every_step);
    t8gpu_hip::Range stage_range(stage_name[a.k]);
    const bool sample = S->timing > 0 && (g / 3) % S->timing == 0;
    if (sample) S->stages_timed++;
    if (a.stage_speed) S->speed_stages++;
    T8_TRY((launch_stage<T, V>(S, L, kind, &S->plan, a, 0, nt, vol, dt, sample)));
  }
  return 0;
}

// ---- the planar decision (single rank, plain plan with 2D patches, KEPES) ------------------------------------------------------
// On a 2D mesh the z-momentum is +0 in every cell and stays +0, and the patch kernels have a form that neither moves nor computes
// it (kernels_fused_patch.hip: PLANAR). Its contract -- the z-momentum planes of everything a stage reads are all +0 bit patterns,
// that of what it writes is +0 already -- is PROVEN here at the start of every call, never assumed: one reduction ORs the raw bits
// of that plane in the four step slots the call touches (prev, Step1, Step2, next) over the slots the plan addresses; the host
// reads the four words through pinned memory after the one stream synchronisation this costs.
//   prev not all +0 (a 3D-like state, a -0.0 somewhere): the whole call runs the general form;
//   else: whichever of the other three is not all +0 (stale stage values, NaN of a fresh allocation) is zeroed -- the general form
//   would store +0 there anyway (flux_math.hpp: kepes_core_planar) -- and every stage of the call runs planar. Between the check
//   and the end of the call only this call's kernels write those planes. That they keep them +0 holds for interior, periodic and
//   wall faces (the outside state of a wall mirrors the inside one: no z-momentum comes in). It does NOT hold for open boundaries:
//   the generic tiles of the launch evaluate inflow and far-field faces against a prescribed state (inflow_entry), which may carry
//   a z-momentum (a 2.5D setup), and stage 1 would then write a non-zero z-momentum that the planar stages 2 and 3 never read.
//   A plan with open faces of any kind (outflow included: no argument is made for it) therefore always runs the general form;
//   the launcher refuses the planar request for such plans too (kernels_fused.hip).
// Nothing is remembered across calls: callers write the planes in between (a restored initial state, an adapted mesh).
// Auto mode asks for n_steps x elements >= kPlanarAutoWork, where the check is amortised (DESIGN.md section 4 has the measured
// costs); a call on a capturing stream cannot synchronise and runs the general form. In graph mode the check runs before the
// replay, so a call that checks synchronises the caller's stream once: the host cannot enqueue the next call ahead of the GPU.
// planar_last is the DECISION of the last call; what the launcher then ran is t8gpu_hip_last_stage_kernel's to say (it takes the
// general kernel for launches that are not whole-plan persistent ones).
constexpr long long kPlanarAutoWork = 1ll << 25;
template <class T>
int planar_decide(Stepper* S, int kind, T* planes, size_t stride, int prev, int next, int n_steps, hipStream_t s) {
  S->planar_now  = false;
  S->planar_last = 0;
  const T8gpuPlainPlan& P = S->plan;
  if (S->planar_mode == 0 || S->has_halo || S->subgrid || kind != T8GPU_FLUX_KEPES || n_steps <= 0 || !planes) return 0;
  if (P.patch_dim == 3 || P.n_patch_tiles[0] + P.n_patch_tiles[1] + P.n_patch_tiles[2] <= 0 || P.ghost_buf || P.send_map) return 0;
  if (P.has_open_faces || P.has_farfield_faces) return 0;   // (a prescribed outside state may carry a z-momentum: see above)
  const size_t n = P.n_slots_addressed > 0 ? static_cast<size_t>(P.n_slots_addressed) : 0;
  if (n == 0 || n > stride) return 0;
  if (S->planar_mode == 1 && static_cast<long long>(n_steps) * static_cast<long long>(n) < kPlanarAutoWork) return 0;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return 0;
  }
  if (!S->d_bits) T8_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&S->d_bits), 4 * sizeof(uint32_t)));
  if (!S->h_bits) T8_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S->h_bits), 4 * sizeof(uint32_t), hipHostMallocDefault));
  const int slot[4] = {prev, 1, 2, next};   // Step1 = 1, Step2 = 2 (stage_args)
  T*        zp[4];
  for (int j = 0; j < 4; j++) zp[j] = planes + (static_cast<size_t>(slot[j]) * 5 + 3) * stride;
  T8_HIP_TRY(hipMemsetAsync(S->d_bits, 0, 4 * sizeof(uint32_t), s));
  if constexpr (sizeof(T) == 4)
    T8_TRY(t8gpu_hip_planes_or_bits_f32(n, zp, S->d_bits, s));
  else
    T8_TRY(t8gpu_hip_planes_or_bits_f64(n, zp, S->d_bits, s));
  T8_HIP_TRY(hipMemcpyAsync(S->h_bits, S->d_bits, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  T8_HIP_TRY(hipStreamSynchronize(s));
  if (S->h_bits[0] != 0) return 0;
  for (int j = 1; j < 4; j++)
    if (S->h_bits[j] != 0) T8_HIP_TRY(hipMemsetAsync(zp[j], 0, n * sizeof(T), s));
  S->planar_now  = true;
  S->planar_last = 1;
  return 0;
}

// iterate() of a single-rank stepper through a hipGraph: capture the enqueue sequence once per argument set, then replay
// it. The capture runs on the stepper's own origin stream (the caller's stream may be the legacy default stream, which
// cannot capture). Timing events are off in graph mode, and a stepper with peers always enqueues directly (the two-lane
// driver). If the runtime refuses the capture the error is returned and the caller falls back.
// (Round 3 could capture the RCCL groups of a multi-rank stepper too, opt-in; never run across xGMI, more host time than the
//  lanes, and a crash inside the HIP runtime's hipStreamEndCapture for some layouts: removed)
template <class T, class V>
int iterate_graph(Stepper* S, int kind, T* planes, size_t stride, const T* vol, int prev, int next, T dt, T* speed, int n_steps,
                  hipStream_t s) {
  S->speed_stages = 0;
  if (!S->graph_mode || S->timing > 0 || n_steps <= 0 || S->has_halo)
    return iterate<T, V>(S, kind, planes, stride, vol, prev, next, dt, speed, n_steps, s);
  struct Key {
    int kind, prev, next, n_steps, tsize, subgrid, planar, every_step;   // (planar: the call's decision picks other kernels;
                                                                         //  every_step: which stages write the speed estimates)
    const void *planes, *vol, *speed;
    size_t stride;
    double dt;
  } key{kind, prev, next, n_steps, static_cast<int>(sizeof(T)), S->subgrid ? 1 : 0, S->planar_now ? 1 : 0,
        S->speed_every_step ? 1 : 0, planes, vol, speed, stride, static_cast<double>(dt)};
  static_assert(sizeof(Key) <= sizeof(S->graph_cache[0].key), "graph key");
  if (!S->graph_stream) {
    T8_HIP_TRY(hipStreamCreateWithFlags(&S->graph_stream, hipStreamNonBlocking));
    T8_HIP_TRY(hipEventCreateWithFlags(&S->ev_graph_in, hipEventDisableTiming));
    T8_HIP_TRY(hipEventCreateWithFlags(&S->ev_graph_out, hipEventDisableTiming));
  }
  // look the argument set up; on a miss the least recently used entry is replaced. (delta_t is part of the key: a
  // CFL-adaptive step size re-captures per value -- use the direct enqueue for such loops.)
  Stepper::GraphEntry* hit = nullptr;
  Stepper::GraphEntry* lru = &S->graph_cache[0];
  for (auto& ge : S->graph_cache) {
    if (ge.exec && std::memcmp(&key, ge.key, sizeof(Key)) == 0) hit = &ge;
    if (!ge.exec || (lru->exec && ge.used < lru->used)) lru = &ge;
  }
  if (!hit) {
    if (lru->exec) {
      (void)hipGraphExecDestroy(lru->exec);
      lru->exec = nullptr;
    }
    hipGraph_t g = nullptr;
    T8_HIP_TRY(hipStreamBeginCapture(S->graph_stream, hipStreamCaptureModeRelaxed));
    const int  rc = iterate<T, V>(S, kind, planes, stride, vol, prev, next, dt, speed, n_steps, S->graph_stream);
    hipError_t e  = hipStreamEndCapture(S->graph_stream, &g);
    if (rc != 0 || e != hipSuccess || !g) {
      if (g) (void)hipGraphDestroy(g);
      return rc != 0 ? rc : static_cast<int>(e != hipSuccess ? e : hipErrorStreamCaptureInvalidated);
    }
    e = hipGraphInstantiate(&lru->exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) {
      lru->exec = nullptr;
      return static_cast<int>(e);
    }
    std::memset(lru->key, 0, sizeof(lru->key));
    std::memcpy(lru->key, &key, sizeof(Key));
    lru->speed_stages = S->speed_stages;
    S->graph_captures++;
    hit = lru;
  }
  hit->used = ++S->graph_clock;
  S->speed_stages = hit->speed_stages;   // (a replay runs what was captured)
  T8_HIP_TRY(hipEventRecord(S->ev_graph_in, s));                         // the graph starts behind the caller's work ...
  T8_HIP_TRY(hipStreamWaitEvent(S->graph_stream, S->ev_graph_in, 0));
  T8_HIP_TRY(hipGraphLaunch(hit->exec, S->graph_stream));
  T8_HIP_TRY(hipEventRecord(S->ev_graph_out, S->graph_stream));
  T8_HIP_TRY(hipStreamWaitEvent(s, S->ev_graph_out, 0));                 // ... and the caller's stream continues behind it
  S->graph_replays++;
  return 0;
}


// ---- MeshManager::partition over RCCL ------------------------------------------------------------------------
// The device half of the reference's partition() (t8gpu/mesh/mesh_manager.inl:626-723, subgrid_mesh_manager.inl:1217-1369):
// there the new owner of an element PULLS its variables through CUDA-IPC pointers into the old owner's memory
// (partition_data<<<>>>); here the old owner SENDS. Elements move in contiguous runs of the space-filling curve, and a run is
// contiguous in every variable plane and in the volume array, so a run is six messages straight from the source planes into
// the destination planes -- no gather kernel, no staging buffer. One RCCL group for all runs of a call; a run whose peer is
// this rank is a device copy.
template <class T, class V>
int repartition(void* comm, int my_rank, int n_send, const int32_t* send_peer, const int32_t* send_first, const int32_t* send_count,
                int n_recv, const int32_t* recv_peer, const int32_t* recv_first, const int32_t* recv_count, V src, const T* src_vol, V dst,
                T* dst_vol, int cells, hipStream_t s) {
  if (cells < 1 || n_send < 0 || n_recv < 0) return static_cast<int>(hipErrorInvalidValue);
  const size_t w = static_cast<size_t>(cells);
  // runs that stay on this rank: the i-th local send pairs with the i-th local receive (both lists are in curve order)
  int js = 0;
  for (int jr = 0; jr < n_recv; jr++) {
    if (recv_peer[jr] != my_rank) continue;
    while (js < n_send && send_peer[js] != my_rank) js++;
    if (js >= n_send || send_count[js] != recv_count[jr]) return static_cast<int>(hipErrorInvalidValue);
    const size_t n = static_cast<size_t>(recv_count[jr]);
    for (int k = 0; k < 5; k++)
      T8_HIP_TRY(hipMemcpyAsync(dst.p[k] + w * recv_first[jr], src.p[k] + w * send_first[js], sizeof(T) * w * n, hipMemcpyDeviceToDevice, s));
    T8_HIP_TRY(hipMemcpyAsync(dst_vol + recv_first[jr], src_vol + send_first[js], sizeof(T) * n, hipMemcpyDeviceToDevice, s));
    js++;
  }
  bool remote = false;
  for (int j = 0; j < n_send; j++) remote = remote || send_peer[j] != my_rank;
  for (int j = 0; j < n_recv; j++) remote = remote || recv_peer[j] != my_rank;
  if (!remote) return 0;
  if (!comm) return static_cast<int>(hipErrorInvalidValue);
  ncclComm_t c = static_cast<ncclComm_t>(comm);
  T8_TRY(nccl_code(ncclGroupStart()));
  for (int j = 0; j < n_recv; j++) {
    if (recv_peer[j] == my_rank || recv_count[j] <= 0) continue;
    const size_t n = static_cast<size_t>(recv_count[j]);
    for (int k = 0; k < 5; k++) T8_TRY(nccl_code(ncclRecv(dst.p[k] + w * recv_first[j], w * n, nccl_type<T>(), recv_peer[j], c, s)));
    T8_TRY(nccl_code(ncclRecv(dst_vol + recv_first[j], n, nccl_type<T>(), recv_peer[j], c, s)));
  }
  for (int j = 0; j < n_send; j++) {
    if (send_peer[j] == my_rank || send_count[j] <= 0) continue;
    const size_t n = static_cast<size_t>(send_count[j]);
    for (int k = 0; k < 5; k++) T8_TRY(nccl_code(ncclSend(src.p[k] + w * send_first[j], w * n, nccl_type<T>(), send_peer[j], c, s)));
    T8_TRY(nccl_code(ncclSend(src_vol + send_first[j], n, nccl_type<T>(), send_peer[j], c, s)));
  }
  T8_TRY(nccl_code(ncclGroupEnd()));
  return 0;
}
}  // namespace

extern "C" {

// roctx ranges for host code above the C-ABI (bench.py marks pre-warm / warm-up / timed repetitions with them)
int t8gpu_hip_range_push(const char* name) {
  if (!t8gpu_hip::roctx().on) return 0;
  t8gpu_hip::roctx().push(name ? name : "t8gpu");
  return 1;
}
int t8gpu_hip_range_pop(void) {
  if (!t8gpu_hip::roctx().on) return 0;
  t8gpu_hip::roctx().pop();
  return 1;
}

int t8gpu_hip_comm_unique_id(char* id128) {
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) return nccl_code(r);
  static_assert(sizeof(id) == 128, "ncclUniqueId layout");
  std::memcpy(id128, &id, 128);
  return 0;
}

int t8gpu_hip_comm_create(const char* id128, int rank, int nranks, void** comm) {
  {   // header / runtime skew (t8gpu_hip_runtime_versions): same major version, at least 2.7
    int v[4];
    (void)t8gpu_hip_runtime_versions(v);
    if (v[1] < 20700 || v[1] / 10000 != NCCL_VERSION_CODE / 10000 || v[3] / 10000000 != HIP_VERSION / 10000000) {
      std::fprintf(stderr, "[t8gpu] RCCL %d / HIP %d at run time do not match the headers this library was built with (RCCL %d, HIP %d)\n",
                   v[1], v[3], v[0], v[2]);
      return static_cast<int>(hipErrorNotSupported);
    }
  }
  ncclUniqueId id;
  std::memcpy(&id, id128, 128);
  ncclComm_t c = nullptr;
  ncclResult_t r = ncclCommInitRank(&c, nranks, id, rank);
  if (r != ncclSuccess) return nccl_code(r);
  *comm = c;
  return 0;
}

int t8gpu_hip_comm_destroy(void* comm) { return comm ? nccl_code(ncclCommDestroy(static_cast<ncclComm_t>(comm))) : 0; }
int t8gpu_hip_comm_abort(void* comm) { return comm ? nccl_code(ncclCommAbort(static_cast<ncclComm_t>(comm))) : 0; }

int t8gpu_hip_halo_exchange_f32(const T8gpuHalo* h, T8gpuVars_f32 state, void* stream) {
  if (!h) return static_cast<int>(hipErrorInvalidValue);
  return exchange<float, T8gpuVars_f32>(*h, state, static_cast<hipStream_t>(stream));
}
int t8gpu_hip_halo_exchange_f64(const T8gpuHalo* h, T8gpuVars_f64 state, void* stream) {
  if (!h) return static_cast<int>(hipErrorInvalidValue);
  return exchange<double, T8gpuVars_f64>(*h, state, static_cast<hipStream_t>(stream));
}

int t8gpu_hip_repartition_f32(void* comm, int my_rank, int n_send, const int32_t* send_peer, const int32_t* send_first,
                              const int32_t* send_count, int n_recv, const int32_t* recv_peer, const int32_t* recv_first,
                              const int32_t* recv_count, T8gpuVars_f32 src, const float* src_volume, T8gpuVars_f32 dst, float* dst_volume,
                              int cells_per_element, void* stream) {
  return repartition<float, T8gpuVars_f32>(comm, my_rank, n_send, send_peer, send_first, send_count, n_recv, recv_peer, recv_first, recv_count,
                                           src, src_volume, dst, dst_volume, cells_per_element, static_cast<hipStream_t>(stream));
}
int t8gpu_hip_repartition_f64(void* comm, int my_rank, int n_send, const int32_t* send_peer, const int32_t* send_first,
                              const int32_t* send_count, int n_recv, const int32_t* recv_peer, const int32_t* recv_first,
                              const int32_t* recv_count, T8gpuVars_f64 src, const double* src_volume, T8gpuVars_f64 dst, double* dst_volume,
                              int cells_per_element, void* stream) {
  return repartition<double, T8gpuVars_f64>(comm, my_rank, n_send, send_peer, send_first, send_count, n_recv, recv_peer, recv_first, recv_count,
                                            src, src_volume, dst, dst_volume, cells_per_element, static_cast<hipStream_t>(stream));
}

// Every rank's chunk of a distributed double array to every rank: mine[offsets[rank + 1] - offsets[rank]] -> all[offsets[nranks]]
// (device pointers; offsets on the host). The refinement criteria of a partitioned adapt travel this way (the forest is
// replicated, so every rank evaluates the adapt callback on the whole array).
int t8gpu_hip_comm_allgatherv_f64(void* comm, int rank, int nranks, const double* mine, double* all, const int64_t* offsets, void* stream) {
  if (!mine || !all || !offsets || rank < 0 || rank >= nranks) return static_cast<int>(hipErrorInvalidValue);
  hipStream_t  s = static_cast<hipStream_t>(stream);
  const size_t n = static_cast<size_t>(offsets[rank + 1] - offsets[rank]);
  if (n) T8_HIP_TRY(hipMemcpyAsync(all + offsets[rank], mine, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  if (nranks == 1) return 0;
  if (!comm) return static_cast<int>(hipErrorInvalidValue);
  ncclComm_t c = static_cast<ncclComm_t>(comm);
  T8_TRY(nccl_code(ncclGroupStart()));
  for (int q = 0; q < nranks; q++) {
    if (q == rank) continue;
    const size_t m = static_cast<size_t>(offsets[q + 1] - offsets[q]);
    if (m) T8_TRY(nccl_code(ncclRecv(all + offsets[q], m, ncclDouble, q, c, s)));
    if (n) T8_TRY(nccl_code(ncclSend(mine, n, ncclDouble, q, c, s)));
  }
  T8_TRY(nccl_code(ncclGroupEnd()));
  return 0;
}

// Polls a stream until it is idle or `timeout_s` elapsed (1 = timed out). Lets a caller bound the
// first exchange on a new communicator and fall back (t8gpu_hip_comm_abort) instead of hanging.
int t8gpu_hip_stream_wait(void* stream, double timeout_s) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    hipError_t e = hipStreamQuery(static_cast<hipStream_t>(stream));
    if (e == hipSuccess) return 0;
    if (e != hipErrorNotReady) return static_cast<int>(e);
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) return 1;
    std::this_thread::sleep_for(std::chrono::milliseconds(1));
  }
}

static int stepper_halo_setup(Stepper* S, const T8gpuHalo* halo) {
  if (halo && halo->n_peers > 0) {
    S->has_halo = true;
    S->halo     = *halo;
    S->peers.assign(halo->peers, halo->peers + halo->n_peers);
    S->send_off.assign(halo->send_off, halo->send_off + halo->n_peers + 1);
    S->recv_off.assign(halo->recv_off, halo->recv_off + halo->n_peers + 1);
    // Normal priority on purpose: a high-priority comm stream was measured (rocprofv3 kernel trace, one rank
    // of the 8-way c4 split) to make everything slower -- tile kernels 49 -> 90-150 us, the 5 us pack / unpack
    // kernels up to 90 us, 50 us gaps -- the queue preempts the running tile waves instead of waiting for a slot.
    // (round 4, two-lane driver: the highest stream priority for the comm lane changes nothing -- 0.1521 / 0.1522 ms per step on
    //  rank 3 of the 8-way c4 split)
    hipError_t e = hipStreamCreateWithFlags(&S->comm_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&S->ev_state, hipEventDisableTiming);
    // the lanes' events order two queues of ONE device: a device-scope release is all they need (the default is a
    // system-scope fence per record)
    const unsigned flags = hipEventDisableTiming | hipEventReleaseToDevice;
    for (int i = 0; i < Stepper::kRing && e == hipSuccess; i++) {
      e = hipEventCreateWithFlags(&S->deep_lane.ring[i], flags);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&S->comm_lane.ring[i], flags);
    }
    if (e != hipSuccess) return static_cast<int>(e);
    const char* th = std::getenv("T8GPU_STEPPER_THREADS");
    S->threads     = !(th && th[0] == '0');
    // (Measured and dropped: the interior tiles on a stream whose CU mask leaves 8 or 16 compute units to the comm lane
    //  (hipExtStreamCreateWithCUMask) -- 0.200 instead of 0.168 ms per step with the three-class lanes; such a stream is also a
    //  blocking one, which serialises it with the legacy default stream most callers use.)
    // the ghost window (t8gpu_hip.h): plain elements through the tile / 2D patch kernels
    const char* gw = std::getenv("T8GPU_GHOST_WINDOW");
    if (!S->subgrid && halo->cells_per_element <= 1 && S->plan.patch_dim != 3 && halo->n_send > 0 && halo->num_elements > 0 &&
        halo->sendbuf && halo->recvbuf && !(gw && gw[0] == '0')) {
      // send slots per owned element, from the rank's send list: -1 none, t >= 0 one slot, -(2 + i) a run of send_list
      const int            N = halo->num_elements, ns = halo->n_send;
      std::vector<int32_t> idx(ns), map(N, -1), cnt(N, 0), list;
      e = hipMemcpy(idx.data(), halo->send_idx, sizeof(int32_t) * ns, hipMemcpyDeviceToHost);
      if (e != hipSuccess) return static_cast<int>(e);
      for (int t = 0; t < ns; t++) {
        if (idx[t] < 0 || idx[t] >= N) return static_cast<int>(hipErrorInvalidValue);
        cnt[idx[t]]++;
      }
      std::vector<int32_t> first(N, -1);
      for (int t = 0; t < ns; t++) {
        const int el = idx[t];
        if (cnt[el] == 1) {
          map[el] = t;
        } else {
          if (first[el] < 0) {   // reserve the element's run
            first[el] = static_cast<int32_t>(list.size());
            list.resize(list.size() + cnt[el], -1);
            map[el] = -(2 + first[el]);
          }
          int32_t* run = list.data() + first[el];
          int      k   = 0;
          while (run[k] != -1) k++;
          run[k] = (k == cnt[el] - 1) ? static_cast<int32_t>(static_cast<uint32_t>(t) | 0x80000000u) : t;
        }
      }
      e = hipMalloc(&S->d_send_map, sizeof(int32_t) * N);
      if (e == hipSuccess) e = hipMemcpy(S->d_send_map, map.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice);
      if (e == hipSuccess && !list.empty()) {
        e = hipMalloc(&S->d_send_list, sizeof(int32_t) * list.size());
        if (e == hipSuccess) e = hipMemcpy(S->d_send_list, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice);
      }
      if (e != hipSuccess) return static_cast<int>(e);
      S->plan_a           = S->plan;
      S->plan_a.ghost_buf = halo->recvbuf;
      S->plan_a.send_map  = static_cast<const int32_t*>(S->d_send_map);
      S->plan_a.send_list = static_cast<const int32_t*>(S->d_send_list);
      S->plan_a.send_buf  = halo->sendbuf;
      S->plan_a.n_owned   = N;
      S->zero_copy        = true;
    }
  }
  return 0;
}

int t8gpu_hip_plain_stepper_create(const T8gpuPlainPlan* plan, const T8gpuHalo* halo, void** out) {
  if (!plan || !out) return static_cast<int>(hipErrorInvalidValue);
  Stepper* S = new Stepper;
  S->plan = *plan;
  const int rc = stepper_halo_setup(S, halo);
  if (rc != 0) {
    t8gpu_hip_plain_stepper_destroy(S);
    return rc;
  }
  *out = S;
  return 0;
}

// Subgrid blocks: the same driver over a T8gpuSubgridPlan (halo->cells_per_element = 4^rank). The handle is used
// with t8gpu_hip_subgrid_stepper_iterate_steps_* and the generic destroy / timing / elapsed entry points above.
int t8gpu_hip_subgrid_stepper_create(const T8gpuSubgridPlan* plan, const T8gpuHalo* halo, void** out) {
  if (!plan || !out) return static_cast<int>(hipErrorInvalidValue);
  if (halo && halo->n_peers > 0 && halo->cells_per_element != (plan->rank == 3 ? 64 : 16)) return static_cast<int>(hipErrorInvalidValue);
  Stepper* S = new Stepper;
  S->subgrid = true;
  S->splan   = *plan;
  const int rc = stepper_halo_setup(S, halo);
  if (rc != 0) {
    t8gpu_hip_plain_stepper_destroy(S);
    return rc;
  }
  *out = S;
  return 0;
}

int t8gpu_hip_plain_stepper_destroy(void* h) {
  Stepper* S = static_cast<Stepper*>(h);
  if (!S) return 0;
  if (S->worker.joinable()) {
    {
      std::lock_guard<std::mutex> lk(S->mu);
      S->worker_exit = true;
    }
    S->cv.notify_one();
    S->worker.join();
  }
  for (Stepper::Lane* L : {&S->deep_lane, &S->comm_lane}) {
    for (hipEvent_t e : L->pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : L->ring)
      if (e) (void)hipEventDestroy(e);
  }
  if (S->d_bits) (void)hipFree(S->d_bits);
  if (S->h_bits) (void)hipHostFree(S->h_bits);
  if (S->d_send_map) (void)hipFree(S->d_send_map);
  if (S->d_send_list) (void)hipFree(S->d_send_list);
  if (S->ev_state) (void)hipEventDestroy(S->ev_state);
  if (S->comm_stream) (void)hipStreamDestroy(S->comm_stream);
  for (auto& ge : S->graph_cache)
    if (ge.exec) (void)hipGraphExecDestroy(ge.exec);
  if (S->ev_graph_in) (void)hipEventDestroy(S->ev_graph_in);
  if (S->ev_graph_out) (void)hipEventDestroy(S->ev_graph_out);
  if (S->graph_stream) (void)hipStreamDestroy(S->graph_stream);
  delete S;
  return 0;
}

int t8gpu_hip_plain_stepper_iterate_f32(void* h, int flux_kind, float* planes, size_t stride, int prev, int next,
                                        float delta_t, float* speed, void* stream) {
  return t8gpu_hip_plain_stepper_iterate_steps_f32(h, flux_kind, planes, stride, prev, next, delta_t, speed, 1, stream);
}
int t8gpu_hip_plain_stepper_iterate_f64(void* h, int flux_kind, double* planes, size_t stride, int prev, int next,
                                        double delta_t, double* speed, void* stream) {
  return t8gpu_hip_plain_stepper_iterate_steps_f64(h, flux_kind, planes, stride, prev, next, delta_t, speed, 1, stream);
}
int t8gpu_hip_plain_stepper_iterate_steps_f32(void* h, int flux_kind, float* planes, size_t stride, int prev, int next,
                                              float delta_t, float* speed, int n_steps, void* stream) {
  if (!h || prev < 0 || prev > 3 || next < 0 || next > 3 || prev == next || n_steps < 0) return static_cast<int>(hipErrorInvalidValue);
  if (static_cast<Stepper*>(h)->subgrid) return static_cast<int>(hipErrorInvalidValue);
  T8_TRY(planar_decide<float>(static_cast<Stepper*>(h), flux_kind, planes, stride, prev, next, n_steps, static_cast<hipStream_t>(stream)));
  return iterate_graph<float, T8gpuVars_f32>(static_cast<Stepper*>(h), flux_kind, planes, stride, planes + 25 * stride, prev, next,
                                             delta_t, speed, n_steps, static_cast<hipStream_t>(stream));
}
int t8gpu_hip_plain_stepper_iterate_steps_f64(void* h, int flux_kind, double* planes, size_t stride, int prev, int next,
                                              double delta_t, double* speed, int n_steps, void* stream) {
  if (!h || prev < 0 || prev > 3 || next < 0 || next > 3 || prev == next || n_steps < 0) return static_cast<int>(hipErrorInvalidValue);
  if (static_cast<Stepper*>(h)->subgrid) return static_cast<int>(hipErrorInvalidValue);
  T8_TRY(planar_decide<double>(static_cast<Stepper*>(h), flux_kind, planes, stride, prev, next, n_steps, static_cast<hipStream_t>(stream)));
  return iterate_graph<double, T8gpuVars_f64>(static_cast<Stepper*>(h), flux_kind, planes, stride, planes + 25 * stride, prev, next,
                                              delta_t, speed, n_steps, static_cast<hipStream_t>(stream));
}

int t8gpu_hip_subgrid_stepper_iterate_steps_f32(void* h, int flux_kind, float* planes, size_t stride, const float* volumes, int prev,
                                                int next, float delta_t, int n_steps, void* stream) {
  if (!h || !static_cast<Stepper*>(h)->subgrid || prev < 0 || prev > 3 || next < 0 || next > 3 || prev == next || n_steps < 0)
    return static_cast<int>(hipErrorInvalidValue);
  return iterate_graph<float, T8gpuVars_f32>(static_cast<Stepper*>(h), flux_kind, planes, stride, volumes, prev, next, delta_t, nullptr,
                                             n_steps, static_cast<hipStream_t>(stream));
}
int t8gpu_hip_subgrid_stepper_iterate_steps_f64(void* h, int flux_kind, double* planes, size_t stride, const double* volumes, int prev,
                                                int next, double delta_t, int n_steps, void* stream) {
  if (!h || !static_cast<Stepper*>(h)->subgrid || prev < 0 || prev > 3 || next < 0 || next > 3 || prev == next || n_steps < 0)
    return static_cast<int>(hipErrorInvalidValue);
  return iterate_graph<double, T8gpuVars_f64>(static_cast<Stepper*>(h), flux_kind, planes, stride, volumes, prev, next, delta_t, nullptr,
                                              n_steps, static_cast<hipStream_t>(stream));
}

// hipGraph replay of a single-rank stepper's iterate_steps(): enable = 1 captures the whole call once per argument set and
// replays it with one hipGraphLaunch; 0 enqueues directly. A stepper with peers always enqueues directly. counts (may be
// NULL) = {captures, replays} so far.
int t8gpu_hip_plain_stepper_graph(void* h, int enable, int* counts) {
  Stepper* S = static_cast<Stepper*>(h);
  if (!S) return static_cast<int>(hipErrorInvalidValue);
  if (enable >= 0) S->graph_mode = enable ? 1 : 0;
  if (counts) {
    counts[0] = S->graph_captures;
    counts[1] = S->graph_replays;
  }
  return 0;
}

// Diagnostics (T8GPU_STEPPER_PROFILE=1 in the environment, else all zeros): host time the step drivers of this process spent
// in {kernel launches, RCCL groups, event records, stream waits} since the last reset. ns4 / calls4 may be NULL.
int t8gpu_hip_stepper_host_profile(int reset, double* ns4, long long* calls4) {
  for (int c = 0; c < 4; c++) {
    if (ns4) ns4[c] = host_profile().ns[c];
    if (calls4) calls4[c] = host_profile().calls[c];
    if (reset) {
      host_profile().ns[c]    = 0;
      host_profile().calls[c] = 0;
    }
  }
  return host_profile().on ? 1 : 0;
}

// Host time the step driver spent enqueueing (wall time of the multi-rank iterate calls; both host threads of the two-lane
// driver overlap inside it) and the steps that covers, since the stepper was created or last reset. 0 / 0 for single-rank
// steppers (their enqueue is a handful of launches).
int t8gpu_hip_plain_stepper_host_time(void* h, int reset, double* total_ms, long long* steps) {
  Stepper* S = static_cast<Stepper*>(h);
  if (!S) return static_cast<int>(hipErrorInvalidValue);
  if (total_ms) *total_ms = S->host_ns * 1e-6;
  if (steps) *steps = S->host_steps;
  if (reset) {
    S->host_ns    = 0;
    S->host_steps = 0;
  }
  return 0;
}

// {RCCL version this library was compiled against (NCCL_VERSION_CODE), RCCL version of the library the process bound,
//  HIP version compiled against (HIP_VERSION), HIP runtime version}. The process may bind another build than the headers
// came from (here: the torch wheel's librccl / libamdhip64 against /opt/rocm's headers): the entry points this library
// uses -- ncclGetUniqueId, ncclCommInitRank, ncclGroupStart / End, ncclSend, ncclRecv, ncclCommDestroy / Abort, all with
// their NCCL 2.7 signatures, no ncclConfig_t -- exist unchanged in every 2.x since 2.7. t8gpu_hip_comm_create refuses a
// runtime with another major version or older than 2.7 (hipErrorNotSupported).
int t8gpu_hip_runtime_versions(int out4[4]) {
  if (!out4) return static_cast<int>(hipErrorInvalidValue);
  int nv = 0, hv = 0;
  out4[0] = NCCL_VERSION_CODE;
  out4[1] = ncclGetVersion(&nv) == ncclSuccess ? nv : -1;
  out4[2] = HIP_VERSION;
  out4[3] = hipRuntimeGetVersion(&hv) == hipSuccess ? hv : -1;
  return 0;
}

int t8gpu_hip_stepper_set_planar(void* h, int mode) {
  Stepper* S = static_cast<Stepper*>(h);
  if (!S || mode < 0 || mode > 2) return static_cast<int>(hipErrorInvalidValue);
  S->planar_mode = mode;
  return 0;
}
int t8gpu_hip_stepper_planar(void* h) {
  Stepper* S = static_cast<Stepper*>(h);
  return S ? S->planar_last : 0;
}

int t8gpu_hip_stepper_set_speed_every_step(void* h, int on) {
  Stepper* S = static_cast<Stepper*>(h);
  if (!S || on < 0 || on > 1) return static_cast<int>(hipErrorInvalidValue);
  S->speed_every_step = on;
  return 0;
}
int t8gpu_hip_stepper_speed_stages(void* h) {
  Stepper* S = static_cast<Stepper*>(h);
  return S ? S->speed_stages : 0;
}

int t8gpu_hip_plain_stepper_timing(void* h, int enable) {
  Stepper* S = static_cast<Stepper*>(h);
  if (!S) return static_cast<int>(hipErrorInvalidValue);
  S->timing = enable < 0 ? 0 : enable;
  S->stages_timed = 0;
  S->deep_lane.used = S->comm_lane.used = 0;
  return 0;
}

// Sum of the stage-kernel durations recorded since timing was enabled (call after a device sync).
int t8gpu_hip_plain_stepper_elapsed(void* h, double* total_ms, int* launches) {
  Stepper* S = static_cast<Stepper*>(h);
  if (!S || !total_ms || !launches) return static_cast<int>(hipErrorInvalidValue);
  double sum = 0;
  int    n   = 0;
  auto   add = [&](const std::vector<hipEvent_t>& pool, size_t used) -> int {
    for (size_t i = 0; i + 1 < used; i += 2) {
      float ms = 0;
      T8_HIP_TRY(hipEventElapsedTime(&ms, pool[i], pool[i + 1]));
      sum += ms;
      n++;
    }
    return 0;
  };
  T8_TRY(add(S->deep_lane.pool, S->deep_lane.used));   // (a single rank's launches are all on the deep lane)
  T8_TRY(add(S->comm_lane.pool, S->comm_lane.used));
  *total_ms = sum;
  *launches = n;
  return 0;
}


// Number of RK stages whose kernels were bracketed by events since timing was enabled (elapsed() / this = the
// average duration of one stage's kernels, however many tile ranges a stage is split into).
int t8gpu_hip_plain_stepper_timed_stages(void* h) {
  Stepper* S = static_cast<Stepper*>(h);
  return S ? S->stages_timed : 0;
}

}  // extern "C"
