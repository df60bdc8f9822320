// stepper.hip -- native driver of one SSP-RK3 step: iterate() without any host language in the loop.
//
// Mirrors CompressibleEulerSolver::iterate (examples/compressible_euler/solver.cu:75-175) for the fused
// tier: 3 x [ghost exchange || interior tiles -> ghost-reading tiles]. Where the reference brackets
// every kernel with cudaDeviceSynchronize + MPI_Barrier (5 pairs per step) this driver only enqueues:
// ordering is carried by two HIP streams and their events, the ghost exchange is one RCCL group of
// ncclSend/ncclRecv per neighbour rank over xGMI (transport.hip), and the host returns immediately.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "driver/transport.hpp"
#include "ranges.hpp"
#include "t8gpu_hip.h"

namespace {
using namespace t8gpu_hip;

inline bool env_on(const char* name) {   // set, not empty and not "0..."
  const char* v = std::getenv(name);
  return v && v[0] != '\0' && v[0] != '0';
}

// Move-only owner of one HIP handle: released when its owner goes, whichever way.
template <class H, hipError_t (*Release)(H)>
struct Owned {
  H h = nullptr;
  Owned() = default;
  Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
  Owned(const Owned&)            = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }
  void reset() {
    if (h) (void)Release(h);
    h = nullptr;
  }
  H* put() {   // for the create / malloc call that fills it
    reset();
    return &h;
  }
  operator H() const { return h; }
};
using Stream    = Owned<hipStream_t, hipStreamDestroy>;
using Event     = Owned<hipEvent_t, hipEventDestroy>;
using GraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;
using DeviceMem = Owned<void*, hipFree>;
using PinnedMem = Owned<void*, hipHostFree>;

template <class T>
struct VarsOf { using type = T8gpuVars_f64; };
template <>
struct VarsOf<float> { using type = T8gpuVars_f32; };
template <class T>
using Vars = typename VarsOf<T>::type;

// The arguments of one iterate_steps() call; (prev, next) are the roles of the FIRST step.
template <class T>
struct Call {
  int      kind;
  T*       planes;
  size_t   stride;
  const T* vol;
  int      prev, next;
  T        dt;
  T*       speed;
  int      n_steps;
};

// Stage g of an iterate_steps() call: stage k = g % 3 of its step, the planes it reads (previous state, stage source) and
// writes, whether it writes the speed estimates and whether its kernels are bracketed by timing events.
template <class T>
struct StageArgs {
  int     k;
  Vars<T> pv, sv, ov;
  T*      stage_speed;
  bool    sample;
};

// What the drivers step: the tiles of a plain plan or the blocks of a Subgrid plan in block_order position order
// (deep interior, near-boundary, ghost-touching). Units [0, nd) are deep, [nd, ni) near-boundary, [ni, nt) read ghosts.
struct Units {
  T8gpuPlainPlan   plan{};
  T8gpuSubgridPlan splan{};
  bool             subgrid = false;
  explicit Units(const T8gpuPlainPlan& p) : plan(p) {}
  explicit Units(const T8gpuSubgridPlan& p) : splan(p), subgrid(true) {}
  int nt() const { return subgrid ? splan.num_elements : plan.ntiles; }
  int ni() const { return subgrid ? splan.n_interior_blocks : plan.n_interior_tiles; }
  // The plan decides: one interior class (n_deep = n_interior; t8gpu_plan_plain_create_ex flag 32, what partitioned meshes get)
  // -> the interior tiles are ONE launch per stage on the deep lane; a deep / near-boundary split in the plan (Subgrid plans,
  // plain plans built without the flag) -> C_g on the deep lane, B_g behind A_g on the comm lane. n_deep = 0 ("unknown"):
  // every interior tile counts as near-boundary.
  int nd() const {
    const int ndeep = subgrid ? splan.n_deep_blocks : plan.n_deep_tiles;
    return (ndeep > 0 && ndeep <= ni()) ? ndeep : 0;
  }
  // units [b, b + n) of stage a on s; `window`: the plain plan with the ghost window for the A class, else NULL
  template <class T>
  int launch(int kind, const StageArgs<T>& a, int b, int n, const T* vol, T dt, hipStream_t s, bool planar,
             const T8gpuPlainPlan* window) const {
    const T8gpuPlainPlan* p  = window ? window : &plan;
    const int             pl = planar ? 1 : 0;   // (0: exactly t8gpu_hip_plain_fused_stage_*)
    if constexpr (sizeof(T) == 4)
      return subgrid ? t8gpu_hip_subgrid_fused_stage_f32(kind, a.k + 1, &splan, b, n, a.pv, a.sv, a.ov, vol, dt, s)
                     : t8gpu_hip_plain_fused_stage_planar_f32(kind, a.k + 1, p, b, n, a.pv, a.sv, a.ov, vol, dt, a.stage_speed, s, pl);
    else
      return subgrid ? t8gpu_hip_subgrid_fused_stage_f64(kind, a.k + 1, &splan, b, n, a.pv, a.sv, a.ov, vol, dt, s)
                     : t8gpu_hip_plain_fused_stage_planar_f64(kind, a.k + 1, p, b, n, a.pv, a.sv, a.ov, vol, dt, a.stage_speed, s, pl);
  }
};

// Timing events of one lane: start / stop pairs of its stage-kernel launches.
struct EventPool {
  std::vector<Event> pool;
  size_t             used = 0;
  int tick(hipStream_t s) {
    if (used == pool.size()) {
      Event e;
      T8_HIP_TRY(hipEventCreate(e.put()));
      pool.push_back(std::move(e));
    }
    T8_HIP_TRY(hipEventRecord(pool[used++], s));
    return 0;
  }
};
struct Timing {
  int       every = 0;   // 0 = off, n = time the stage kernels of every n-th step
  int       stages_timed = 0;
  EventPool deep, comm;   // (a single rank's launches are all on the deep lane)
};

// hipGraph replay of a whole single-rank iterate_steps() call (t8gpu_hip_plain_stepper_graph): the enqueue sequence is
// captured once per distinct argument set on an internal origin stream and replayed with one hipGraphLaunch
struct GraphCache {
  int    mode = 0;   // 0 off, 1 on
  Stream stream;
  Event  ev_in, ev_out;
  struct Entry {        // one executable per argument set; a step loop alternates between two (the roles of
    GraphExec     exec;   // prev / next swap with every odd n_steps), so the cache holds a few
    unsigned char key[96] = {0};
    unsigned long used = 0;
    int           speed_stages = 0;   // stages of the captured sequence that write the speed estimates
  };
  Entry         entries[4];
  unsigned long clock = 0;
  int           captures = 0, replays = 0;

  // Look the argument set up; on a miss the least recently used entry is replaced by a capture of what `enqueue(stream)`
  // queues (*fresh = true). (delta_t is part of the key: a CFL-adaptive step size re-captures per value -- use the direct
  // enqueue for such loops.)
  template <class Key, class F>
  int find_or_capture(const Key& key, F&& enqueue, Entry** out, bool* fresh) {
    static_assert(sizeof(Key) <= sizeof(Entry::key), "graph key");
    if (!stream) {
      T8_HIP_TRY(hipStreamCreateWithFlags(stream.put(), hipStreamNonBlocking));
      T8_HIP_TRY(hipEventCreateWithFlags(ev_in.put(), hipEventDisableTiming));
      T8_HIP_TRY(hipEventCreateWithFlags(ev_out.put(), hipEventDisableTiming));
    }
    Entry* hit = nullptr;
    Entry* lru = &entries[0];
    for (auto& ge : entries) {
      if (ge.exec && std::memcmp(&key, ge.key, sizeof(Key)) == 0) hit = &ge;
      if (!ge.exec || (lru->exec && ge.used < lru->used)) lru = &ge;
    }
    *fresh = !hit;
    if (!hit) {
      lru->exec.reset();
      hipGraph_t g = nullptr;
      T8_HIP_TRY(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
      const int  rc = enqueue(static_cast<hipStream_t>(stream));
      hipError_t e  = hipStreamEndCapture(stream, &g);
      if (rc != 0 || e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        return rc != 0 ? rc : static_cast<int>(e != hipSuccess ? e : hipErrorStreamCaptureInvalidated);
      }
      e = hipGraphInstantiate(lru->exec.put(), g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      if (e != hipSuccess) {
        lru->exec.h = nullptr;
        return static_cast<int>(e);
      }
      std::memset(lru->key, 0, sizeof(lru->key));
      std::memcpy(lru->key, &key, sizeof(Key));
      captures++;
      hit = lru;
    }
    hit->used = ++clock;
    *out      = hit;
    return 0;
  }
  int replay(const Entry& e, hipStream_t s) {
    T8_HIP_TRY(hipEventRecord(ev_in, s));                      // the graph starts behind the caller's work ...
    T8_HIP_TRY(hipStreamWaitEvent(stream, ev_in, 0));
    T8_HIP_TRY(hipGraphLaunch(e.exec, stream));
    T8_HIP_TRY(hipEventRecord(ev_out, stream));
    T8_HIP_TRY(hipStreamWaitEvent(s, ev_out, 0));              // ... and the caller's stream continues behind it
    replays++;
    return 0;
  }
};

// the planar 2D stage (t8gpu_hip.h: t8gpu_hip_stepper_set_planar; planar_decide below)
struct PlanarCheck {
  int       mode = 1;      // 0 never, 1 where the check is amortised, 2 whenever proven
  bool      now  = false;  // the current call runs planar
  int       last = 0;      // what the last call did
  DeviceMem d_bits;        // device: OR of the bits of the four z-momentum planes
  PinnedMem h_bits;        // pinned host copy
};

// Send slots per owned element from a rank's send list (T8gpuPlainPlan::send_map / send_list): map[e] = -1 none, t >= 0 the
// one slot, -(2 + i) a run of `list` starting at i, in send-list order, its last slot flagged in bit 31.
// false: an index outside [0, n_owned).
bool build_send_map(const std::vector<int32_t>& send_idx, int n_owned, std::vector<int32_t>& map, std::vector<int32_t>& list) {
  map.assign(n_owned, -1);
  list.clear();
  std::vector<int32_t> cnt(n_owned, 0), filled(n_owned, 0);
  for (const int32_t el : send_idx) {
    if (el < 0 || el >= n_owned) return false;
    cnt[el]++;
  }
  for (size_t t = 0; t < send_idx.size(); t++) {
    const int32_t el = send_idx[t], slot = static_cast<int32_t>(t);
    if (cnt[el] == 1) {
      map[el] = slot;
      continue;
    }
    if (filled[el] == 0) {   // reserve the element's run
      map[el] = -(2 + static_cast<int32_t>(list.size()));
      list.resize(list.size() + cnt[el], -1);
    }
    const bool last = ++filled[el] == cnt[el];
    list[-(map[el] + 2) + filled[el] - 1] = last ? static_cast<int32_t>(static_cast<uint32_t>(slot) | 0x80000000u) : slot;
  }
  return true;
}

// ---- lanes: what only a stepper with peers has (iterate_lanes below) ---------------------------------------------------------
struct Lanes {
  static constexpr int kRing = 4;
  T8gpuHalo            halo{};
  std::vector<int32_t> peers, send_off, recv_off;
  Stream               comm_stream;                    // the comm lane's stream; the deep lane is the caller's
  Event                ev_state;                       // step entry
  Event                deep_ring[kRing], comm_ring[kRing];   // the record of stage g uses ring[g % kRing]
  bool                 zero_copy = false;   // ghost window: A tiles read the receive buffer and fill the send buffer themselves
  T8gpuPlainPlan       plan_a{};            // the plan + the ghost window (launches of the A class)
  DeviceMem            d_send_map, d_send_list;
  double               host_ns    = 0;      // host time inside iterate_lanes
  long                 host_steps = 0;

  int setup(const Units& U, const T8gpuHalo& h) {
    halo = h;
    peers.assign(h.peers, h.peers + h.n_peers);
    send_off.assign(h.send_off, h.send_off + h.n_peers + 1);
    recv_off.assign(h.recv_off, h.recv_off + h.n_peers + 1);
    // Normal priority on purpose: a high-priority comm stream was measured (rocprofv3 kernel trace, one rank
    // of the 8-way c4 split) to make everything slower -- tile kernels 49 -> 90-150 us, the 5 us pack / unpack
    // kernels up to 90 us, 50 us gaps -- the queue preempts the running tile waves instead of waiting for a slot.
    // (round 4, two-lane driver: the highest stream priority for the comm lane changes nothing -- 0.1521 / 0.1522 ms per step on
    //  rank 3 of the 8-way c4 split)
    T8_HIP_TRY(hipStreamCreateWithFlags(comm_stream.put(), hipStreamNonBlocking));
    T8_HIP_TRY(hipEventCreateWithFlags(ev_state.put(), hipEventDisableTiming));
    // the lanes' events order two queues of ONE device: a device-scope release is all they need (the default is a
    // system-scope fence per record)
    const unsigned flags = hipEventDisableTiming | hipEventReleaseToDevice;
    for (int i = 0; i < kRing; i++) {
      T8_HIP_TRY(hipEventCreateWithFlags(deep_ring[i].put(), flags));
      T8_HIP_TRY(hipEventCreateWithFlags(comm_ring[i].put(), flags));
    }
    // (Measured and dropped: the interior tiles on a stream whose CU mask leaves 8 or 16 compute units to the comm lane
    //  (hipExtStreamCreateWithCUMask) -- 0.200 instead of 0.168 ms per step with the three-class lanes; such a stream is also a
    //  blocking one, which serialises it with the legacy default stream most callers use.)
    // the ghost window (t8gpu_hip.h): plain elements through the tile / 2D patch kernels
    const char* gw = std::getenv("T8GPU_GHOST_WINDOW");
    if (U.subgrid || h.cells_per_element > 1 || U.plan.patch_dim == 3 || h.n_send <= 0 || h.num_elements <= 0 || !h.sendbuf ||
        !h.recvbuf || (gw && gw[0] == '0'))
      return 0;
    const int            N = h.num_elements;
    std::vector<int32_t> idx(h.n_send), map, list;
    T8_HIP_TRY(hipMemcpy(idx.data(), h.send_idx, sizeof(int32_t) * idx.size(), hipMemcpyDeviceToHost));
    if (!build_send_map(idx, N, map, list)) return static_cast<int>(hipErrorInvalidValue);
    T8_HIP_TRY(hipMalloc(d_send_map.put(), sizeof(int32_t) * N));
    T8_HIP_TRY(hipMemcpy(d_send_map, map.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice));
    if (!list.empty()) {
      T8_HIP_TRY(hipMalloc(d_send_list.put(), sizeof(int32_t) * list.size()));
      T8_HIP_TRY(hipMemcpy(d_send_list, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice));
    }
    plan_a           = U.plan;
    plan_a.ghost_buf = h.recvbuf;
    plan_a.send_map  = static_cast<const int32_t*>(d_send_map.h);
    plan_a.send_list = static_cast<const int32_t*>(d_send_list.h);
    plan_a.send_buf  = h.sendbuf;
    plan_a.n_owned   = N;
    zero_copy        = true;
    return 0;
  }
  // stage g of a lane is over / the other lane waits for it
  int record(const Event (&ring)[kRing], int g, hipStream_t lane) const {
    HostTimer ht(2);
    T8_HIP_TRY(hipEventRecord(ring[g % kRing], lane));
    return 0;
  }
  int wait(hipStream_t lane, const Event (&ring)[kRing], int g) const {
    HostTimer ht(3);
    T8_HIP_TRY(hipStreamWaitEvent(lane, ring[g % kRing], 0));
    return 0;
  }
};

struct Stepper {
  template <class Plan>
  explicit Stepper(const Plan& plan) : units(plan) {}
  Units       units;
  Timing      timing;
  GraphCache  graph;
  PlanarCheck planar;
  // the per-face speed estimates (t8gpu_hip.h: t8gpu_hip_stepper_set_speed_every_step; stage_args below)
  // 0 the third stage of a call's last step writes them, 1 the third stage of every step; T8GPU_SPEED_EVERY_STEP in the
  // environment sets the mode a new stepper starts in
  int speed_every_step = env_on("T8GPU_SPEED_EVERY_STEP") ? 1 : 0;
  int speed_stages     = 0;   // stages of the last call that were handed the array
  std::unique_ptr<Lanes> lanes;   // the stepper has peers: iterate() runs the two-lane driver
};

template <class T>
Vars<T> step_vars(T* planes, size_t stride, int step) {
  Vars<T> v;
  for (int k = 0; k < 5; k++) v.p[k] = planes + (static_cast<size_t>(step) * 5 + k) * stride;
  return v;
}

// The arguments of stage g, and the stepper's per-stage accounting (once per stage, however many launches it takes)
template <class T>
StageArgs<T> stage_args(Stepper* S, const Call<T>& c, int g) {
  StageArgs<T> a;
  a.k          = g % 3;
  const int pr = (g / 3) % 2 == 0 ? c.prev : c.next, nx = (g / 3) % 2 == 0 ? c.next : c.prev;
  const int src = a.k == 0 ? pr : a.k, dst = a.k == 2 ? nx : a.k + 1;   // Step1 = 1, Step2 = 2 (solver.h:24-31)
  a.pv = step_vars(c.planes, c.stride, pr);
  a.sv = step_vars(c.planes, c.stride, src);
  a.ov = step_vars(c.planes, c.stride, dst);
  // The per-face speed estimates are rewritten by every stage and read only between CALLS (compute_timestep uses
  // those "computed at the last step of the last timestepping", solver.h:88-91): only the third stage of the call's
  // last step writes them. Every third stage would store the whole array (one value per face) and the next step
  // overwrite it before anyone can look: same contents on return, F + B stores less per intermediate step.
  // speed_every_step (t8gpu_hip_stepper_set_speed_every_step): the third stage of every step, for A/B runs.
  a.stage_speed = a.k == 2 && (S->speed_every_step || g == 3 * c.n_steps - 1) ? c.speed : nullptr;
  a.sample      = S->timing.every > 0 && (g / 3) % S->timing.every == 0;
  if (a.stage_speed) S->speed_stages++;
  if (a.sample) S->timing.stages_timed++;
  return a;
}

// units [b, b + n) of stage a on stream s; a sampled stage is bracketed by events of `pool`
template <class T>
int launch_stage(Stepper* S, hipStream_t s, EventPool& pool, const T8gpuPlainPlan* window, const Call<T>& c, const StageArgs<T>& a, int b,
                 int n) {
  if (n <= 0) return 0;
  HostTimer ht(0);
  if (a.sample) T8_TRY(pool.tick(s));
  T8_TRY(S->units.launch(c.kind, a, b, n, c.vol, c.dt, s, S->planar.now, window));
  if (a.sample) T8_TRY(pool.tick(s));
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
//   * ONE HOST THREAD enqueues both lanes, stage by stage, the deep lane first: every event a lane waits for has been
//     recorded when the wait is issued. (A host thread per lane was measured and dropped: DESIGN.md section 6.)
// Plans the ghost window does not cover (Subgrid blocks, 3D patch tiles) run the same two lanes with the pack / unpack
// kernels around the group.
template <class T>
int iterate_lanes(Stepper* S, const Call<T>& c, hipStream_t s) {
  if (c.n_steps <= 0) return 0;
  const auto   host_t0 = std::chrono::steady_clock::now();
  Lanes&       L  = *S->lanes;
  const Units& U  = S->units;
  const int    nt = U.nt(), ni = U.ni(), nd = U.nd(), G = 3 * c.n_steps;
  const hipStream_t xs = L.comm_stream;
  t8gpu_hip::Range  whole("t8gpu.iterate_steps (exchange -> ghost-reading tiles || interior tiles, two lanes)");

  // entry: the lanes see everything the caller queued on s
  T8_HIP_TRY(hipEventRecord(L.ev_state, s));
  T8_HIP_TRY(hipStreamWaitEvent(xs, L.ev_state, 0));

  auto stage = [&](int g) -> int {
    const StageArgs<T> a = stage_args(S, c, g);
    // ---- deep lane: [B_(g-1)] -> C_g ----------------------------------------------------------------------------------------
    if (nd > 0) {
      if (g > 0) T8_TRY(L.wait(s, L.comm_ring, g - 1));
      T8_TRY(launch_stage(S, s, S->timing.deep, nullptr, c, a, 0, nd));                       // C_g
      T8_TRY(L.record(L.deep_ring, g, s));
    }
    // ---- comm lane: RCCL_g -> A_g -> [C_(g-1)] -> B_g -----------------------------------------------------------------------
    if (!L.zero_copy || g == 0)   // (ghost window: the A tiles of stage g-1 have filled the send buffer)
      T8_TRY((halo_pack<T, Vars<T>>(L.halo, a.sv, xs)));
    T8_TRY(exchange_wire<T>(L.halo, L.peers.data(), L.send_off.data(), L.recv_off.data(), xs));
    if (!L.zero_copy) T8_TRY((halo_unpack<T, Vars<T>>(L.halo, a.sv, xs)));
    const bool after_deep = g > 0 && nd > 0;   // the deep lane's stage g-1 has work this lane reads
    if (nd == ni && after_deep) T8_TRY(L.wait(xs, L.deep_ring, g - 1));                       // A_g <- interior_(g-1)
    T8_TRY(launch_stage(S, xs, S->timing.comm, L.zero_copy ? &L.plan_a : nullptr, c, a, ni, nt - ni));   // A_g
    if (nd < ni) {
      if (after_deep) T8_TRY(L.wait(xs, L.deep_ring, g - 1));                                 // B_g <- C_(g-1)
      T8_TRY(launch_stage(S, xs, S->timing.comm, nullptr, c, a, nd, ni - nd));                // B_g
    }
    return L.record(L.comm_ring, g, xs);
  };
  int rc = 0;
  for (int g = 0; g < G && rc == 0; g++) rc = stage(g);
  // exit: everything is ordered on s again
  T8_HIP_TRY(hipStreamWaitEvent(s, L.comm_ring[(G - 1) % Lanes::kRing], 0));
  L.host_ns += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - host_t0).count();
  L.host_steps += c.n_steps;
  return rc;
}

// n_steps SSP-RK3 steps; (prev, next) are the roles of the FIRST step, they swap from step to step (solver.cu:76).
// A stepper with peers runs the two-lane driver above. A single rank launches all its units [0, nt) once per stage on the
// caller's stream (the deep lane's stream for the call, whose events time the sampled steps).
// Subgrid blocks run through the same drivers (SubgridCompressibleEulerSolver::iterate, examples/subgrid/solver.inl:
// 152-266): units are blocks in the plan's position order (deep interior, near-boundary, ghost-touching), a ghost
// block mirrors all 4^rank subcells, `vol` is the separate per-block volume array of SubgridMemoryManager.
template <class T>
int iterate(Stepper* S, const Call<T>& c, hipStream_t s) {
  if (S->lanes) return iterate_lanes(S, c, s);
  t8gpu_hip::Range whole("t8gpu.iterate_steps");
  static const char* const stage_name[3] = {"t8gpu.rk_stage1", "t8gpu.rk_stage2", "t8gpu.rk_stage3"};
  for (int g = 0; g < 3 * c.n_steps; g++) {
    const StageArgs<T> a = stage_args(S, c, g);
    t8gpu_hip::Range   stage_range(stage_name[a.k]);
    T8_TRY(launch_stage(S, s, S->timing.deep, nullptr, c, a, 0, S->units.nt()));
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
// planar.last is the DECISION of the last call; what the launcher then ran is t8gpu_hip_last_stage_kernel's to say (it takes the
// general kernel for launches that are not whole-plan persistent ones).
constexpr long long kPlanarAutoWork = 1ll << 25;
template <class T>
int planar_decide(Stepper* S, const Call<T>& c, hipStream_t s) {
  PlanarCheck& C = S->planar;
  C.now  = false;
  C.last = 0;
  const T8gpuPlainPlan& P = S->units.plan;
  if (C.mode == 0 || S->lanes || S->units.subgrid || c.kind != T8GPU_FLUX_KEPES || c.n_steps <= 0 || !c.planes) return 0;
  if (P.patch_dim == 3 || P.n_patch_tiles[0] + P.n_patch_tiles[1] + P.n_patch_tiles[2] <= 0 || P.ghost_buf || P.send_map) return 0;
  if (P.has_open_faces || P.has_farfield_faces) return 0;   // (a prescribed outside state may carry a z-momentum: see above)
  const size_t n = P.n_slots_addressed > 0 ? static_cast<size_t>(P.n_slots_addressed) : 0;
  if (n == 0 || n > c.stride) return 0;
  if (C.mode == 1 && static_cast<long long>(c.n_steps) * static_cast<long long>(n) < kPlanarAutoWork) return 0;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return 0;
  }
  if (!C.d_bits) T8_HIP_TRY(hipMalloc(C.d_bits.put(), 4 * sizeof(uint32_t)));
  if (!C.h_bits) T8_HIP_TRY(hipHostMalloc(C.h_bits.put(), 4 * sizeof(uint32_t), hipHostMallocDefault));
  uint32_t* const d_bits  = static_cast<uint32_t*>(C.d_bits.h);
  uint32_t* const h_bits  = static_cast<uint32_t*>(C.h_bits.h);
  const int       slot[4] = {c.prev, 1, 2, c.next};   // Step1 = 1, Step2 = 2 (stage_args)
  T*              zp[4];
  for (int j = 0; j < 4; j++) zp[j] = c.planes + (static_cast<size_t>(slot[j]) * 5 + 3) * c.stride;
  T8_HIP_TRY(hipMemsetAsync(d_bits, 0, 4 * sizeof(uint32_t), s));
  if constexpr (sizeof(T) == 4)
    T8_TRY(t8gpu_hip_planes_or_bits_f32(n, zp, d_bits, s));
  else
    T8_TRY(t8gpu_hip_planes_or_bits_f64(n, zp, d_bits, s));
  T8_HIP_TRY(hipMemcpyAsync(h_bits, d_bits, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  T8_HIP_TRY(hipStreamSynchronize(s));
  if (h_bits[0] != 0) return 0;
  for (int j = 1; j < 4; j++)
    if (h_bits[j] != 0) T8_HIP_TRY(hipMemsetAsync(zp[j], 0, n * sizeof(T), s));
  C.now  = true;
  C.last = 1;
  return 0;
}

// iterate() of a single-rank stepper through a hipGraph: capture the enqueue sequence once per argument set, then replay
// it. The capture runs on the stepper's own origin stream (the caller's stream may be the legacy default stream, which
// cannot capture). Timing events are off in graph mode, and a stepper with peers always enqueues directly (the two-lane
// driver). If the runtime refuses the capture the error is returned and the caller falls back.
template <class T>
int iterate_graph(Stepper* S, const Call<T>& c, hipStream_t s) {
  S->speed_stages = 0;
  if (!S->graph.mode || S->timing.every > 0 || c.n_steps <= 0 || S->lanes) return iterate(S, c, s);
  struct Key {
    int kind, prev, next, n_steps, tsize, subgrid, planar, every_step;   // (planar: the call's decision picks other kernels;
                                                                         //  every_step: which stages write the speed estimates)
    const void *planes, *vol, *speed;
    size_t stride;
    double dt;
  } key{c.kind, c.prev, c.next, c.n_steps, static_cast<int>(sizeof(T)), S->units.subgrid ? 1 : 0, S->planar.now ? 1 : 0,
        S->speed_every_step ? 1 : 0, c.planes, c.vol, c.speed, c.stride, static_cast<double>(c.dt)};
  GraphCache::Entry* hit   = nullptr;
  bool               fresh = false;
  T8_TRY(S->graph.find_or_capture(key, [&](hipStream_t origin) { return iterate(S, c, origin); }, &hit, &fresh));
  if (fresh) hit->speed_stages = S->speed_stages;
  S->speed_stages = hit->speed_stages;   // (a replay runs what was captured)
  return S->graph.replay(*hit, s);
}

// The iterate_steps entries: one validation for both precisions; a plain handle is refused by a Subgrid entry and the reverse.
template <class T>
int iterate_steps(void* h, bool subgrid, int kind, T* planes, size_t stride, const T* vol, int prev, int next, T dt, T* speed,
                  int n_steps, void* stream) {
  Stepper* S = static_cast<Stepper*>(h);
  if (!S || S->units.subgrid != subgrid || prev < 0 || prev > 3 || next < 0 || next > 3 || prev == next || n_steps < 0)
    return static_cast<int>(hipErrorInvalidValue);
  const Call<T>     c{kind, planes, stride, vol, prev, next, dt, speed, n_steps};
  const hipStream_t s = static_cast<hipStream_t>(stream);
  T8_TRY(planar_decide(S, c, s));   // (never planar for Subgrid blocks)
  return iterate_graph(S, c, s);
}

template <class Plan>
int create(const Plan& plan, const T8gpuHalo* halo, void** out) {
  std::unique_ptr<Stepper> S(new Stepper(plan));
  if (halo && halo->n_peers > 0) {
    S->lanes.reset(new Lanes);
    T8_TRY(S->lanes->setup(S->units, *halo));   // (a failure releases what was made: the parts own their handles)
  }
  *out = S.release();
  return 0;
}
}  // namespace

extern "C" {

int t8gpu_hip_plain_stepper_create(const T8gpuPlainPlan* plan, const T8gpuHalo* halo, void** out) {
  if (!plan || !out) return static_cast<int>(hipErrorInvalidValue);
  return create(*plan, halo, out);
}

// Subgrid blocks: the same driver over a T8gpuSubgridPlan (halo->cells_per_element = 4^rank). The handle is used
// with t8gpu_hip_subgrid_stepper_iterate_steps_* and the generic destroy / timing / elapsed entry points.
int t8gpu_hip_subgrid_stepper_create(const T8gpuSubgridPlan* plan, const T8gpuHalo* halo, void** out) {
  if (!plan || !out) return static_cast<int>(hipErrorInvalidValue);
  if (halo && halo->n_peers > 0 && halo->cells_per_element != (plan->rank == 3 ? 64 : 16)) return static_cast<int>(hipErrorInvalidValue);
  return create(*plan, halo, out);
}

int t8gpu_hip_plain_stepper_destroy(void* h) {
  delete static_cast<Stepper*>(h);
  return 0;
}

int t8gpu_hip_plain_stepper_iterate_f32(void* h, int flux_kind, float* planes, size_t stride, int prev, int next,
                                        float delta_t, float* speed, void* stream) {
  return iterate_steps<float>(h, false, flux_kind, planes, stride, planes + 25 * stride, prev, next, delta_t, speed, 1, stream);
}
int t8gpu_hip_plain_stepper_iterate_f64(void* h, int flux_kind, double* planes, size_t stride, int prev, int next,
                                        double delta_t, double* speed, void* stream) {
  return iterate_steps<double>(h, false, flux_kind, planes, stride, planes + 25 * stride, prev, next, delta_t, speed, 1, stream);
}
int t8gpu_hip_plain_stepper_iterate_steps_f32(void* h, int flux_kind, float* planes, size_t stride, int prev, int next,
                                              float delta_t, float* speed, int n_steps, void* stream) {
  return iterate_steps<float>(h, false, flux_kind, planes, stride, planes + 25 * stride, prev, next, delta_t, speed, n_steps, stream);
}
int t8gpu_hip_plain_stepper_iterate_steps_f64(void* h, int flux_kind, double* planes, size_t stride, int prev, int next,
                                              double delta_t, double* speed, int n_steps, void* stream) {
  return iterate_steps<double>(h, false, flux_kind, planes, stride, planes + 25 * stride, prev, next, delta_t, speed, n_steps, stream);
}
int t8gpu_hip_subgrid_stepper_iterate_steps_f32(void* h, int flux_kind, float* planes, size_t stride, const float* volumes, int prev,
                                                int next, float delta_t, int n_steps, void* stream) {
  return iterate_steps<float>(h, true, flux_kind, planes, stride, volumes, prev, next, delta_t, nullptr, n_steps, stream);
}
int t8gpu_hip_subgrid_stepper_iterate_steps_f64(void* h, int flux_kind, double* planes, size_t stride, const double* volumes, int prev,
                                                int next, double delta_t, int n_steps, void* stream) {
  return iterate_steps<double>(h, true, flux_kind, planes, stride, volumes, prev, next, delta_t, nullptr, n_steps, stream);
}

// hipGraph replay of a single-rank stepper's iterate_steps(): enable = 1 captures the whole call once per argument set and
// replays it with one hipGraphLaunch; 0 enqueues directly. A stepper with peers always enqueues directly. counts (may be
// NULL) = {captures, replays} so far.
int t8gpu_hip_plain_stepper_graph(void* h, int enable, int* counts) {
  Stepper* S = static_cast<Stepper*>(h);
  if (!S) return static_cast<int>(hipErrorInvalidValue);
  if (enable >= 0) S->graph.mode = enable ? 1 : 0;
  if (counts) {
    counts[0] = S->graph.captures;
    counts[1] = S->graph.replays;
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

// Host time the step driver spent enqueueing (wall time of the multi-rank iterate calls) and the steps that covers, since
// the stepper was created or last reset. 0 / 0 for single-rank steppers (their enqueue is a handful of launches).
int t8gpu_hip_plain_stepper_host_time(void* h, int reset, double* total_ms, long long* steps) {
  Stepper* S = static_cast<Stepper*>(h);
  if (!S) return static_cast<int>(hipErrorInvalidValue);
  Lanes* L = S->lanes.get();
  if (total_ms) *total_ms = L ? L->host_ns * 1e-6 : 0.0;
  if (steps) *steps = L ? L->host_steps : 0;
  if (reset && L) {
    L->host_ns    = 0;
    L->host_steps = 0;
  }
  return 0;
}

int t8gpu_hip_stepper_set_planar(void* h, int mode) {
  Stepper* S = static_cast<Stepper*>(h);
  if (!S || mode < 0 || mode > 2) return static_cast<int>(hipErrorInvalidValue);
  S->planar.mode = mode;
  return 0;
}
int t8gpu_hip_stepper_planar(void* h) {
  Stepper* S = static_cast<Stepper*>(h);
  return S ? S->planar.last : 0;
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
  S->timing.every        = enable < 0 ? 0 : enable;
  S->timing.stages_timed = 0;
  S->timing.deep.used = S->timing.comm.used = 0;
  return 0;
}

// Sum of the stage-kernel durations recorded since timing was enabled (call after a device sync).
int t8gpu_hip_plain_stepper_elapsed(void* h, double* total_ms, int* launches) {
  Stepper* S = static_cast<Stepper*>(h);
  if (!S || !total_ms || !launches) return static_cast<int>(hipErrorInvalidValue);
  double sum = 0;
  int    n   = 0;
  for (const EventPool* p : {&S->timing.deep, &S->timing.comm})
    for (size_t i = 0; i + 1 < p->used; i += 2) {
      float ms = 0;
      T8_HIP_TRY(hipEventElapsedTime(&ms, p->pool[i], p->pool[i + 1]));
      sum += ms;
      n++;
    }
  *total_ms = sum;
  *launches = n;
  return 0;
}

// Number of RK stages whose kernels were bracketed by events since timing was enabled (elapsed() / this = the
// average duration of one stage's kernels, however many tile ranges a stage is split into).
int t8gpu_hip_plain_stepper_timed_stages(void* h) {
  Stepper* S = static_cast<Stepper*>(h);
  return S ? S->timing.stages_timed : 0;
}

}  // extern "C"
