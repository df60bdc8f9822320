// driver/transport.hpp -- what the step driver (stepper.hip) uses of the RCCL transport (transport.hip): the pieces of one
// ghost exchange, the error-code conventions of the C-ABI and the host-cost profile of the enqueue.
#ifndef T8GPU_HIP_DRIVER_TRANSPORT_HPP
#define T8GPU_HIP_DRIVER_TRANSPORT_HPP

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>

#include "t8gpu_hip.h"

namespace t8gpu_hip {

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

// Host cost of the enqueue by category (T8GPU_STEPPER_PROFILE=1; read and reset through t8gpu_hip_stepper_host_profile): where
// the time of a multi-rank stage goes on the host -- kernel launches, the RCCL group, event records / waits. One per process.
struct HostProfile {
  bool   on;
  double ns[4]    = {0, 0, 0, 0};
  long   calls[4] = {0, 0, 0, 0};
};
HostProfile& host_profile();

struct HostTimer {   // cat: 0 kernel launch, 1 RCCL group, 2 event record, 3 stream wait
  int cat;
  std::chrono::steady_clock::time_point t0;
  explicit HostTimer(int c) : cat(c) {
    if (host_profile().on) t0 = std::chrono::steady_clock::now();
  }
  ~HostTimer() {
    if (!host_profile().on) return;
    host_profile().ns[cat] += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
    host_profile().calls[cat]++;
  }
};

// The pieces of one exchange, each enqueued on s (T = float with V = T8gpuVars_f32, double with T8gpuVars_f64):
// state -> send buffer; the RCCL group (per peer, its ghosts into the receive buffer and what it mirrors out of the send
// buffer); receive buffer -> the ghost slots of state.
template <class T, class V>
int halo_pack(const T8gpuHalo& h, V state, hipStream_t s);
template <class T, class V>
int halo_unpack(const T8gpuHalo& h, V state, hipStream_t s);
template <class T>
int exchange_wire(const T8gpuHalo& h, const int32_t* peers, const int32_t* send_off, const int32_t* recv_off, hipStream_t s);

}  // namespace t8gpu_hip

#endif  // T8GPU_HIP_DRIVER_TRANSPORT_HPP
