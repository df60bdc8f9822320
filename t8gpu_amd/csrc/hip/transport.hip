// transport.hip -- the RCCL transport below the step driver and the mesh managers: the communicator, the ghost exchange
// (pack -> one group of ncclSend / ncclRecv per neighbour rank -> unpack), repartition, allgatherv, a bounded stream wait --
// and the roctx ranges for host code above the C-ABI. The step driver (stepper.hip) uses the pieces of the exchange through
// driver/transport.hpp.
#include "driver/transport.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "ranges.hpp"

namespace t8gpu_hip {

HostProfile& host_profile() {
  static HostProfile p{std::getenv("T8GPU_STEPPER_PROFILE") != nullptr};
  return p;
}

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

template int halo_pack<float, T8gpuVars_f32>(const T8gpuHalo&, T8gpuVars_f32, hipStream_t);
template int halo_pack<double, T8gpuVars_f64>(const T8gpuHalo&, T8gpuVars_f64, hipStream_t);
template int halo_unpack<float, T8gpuVars_f32>(const T8gpuHalo&, T8gpuVars_f32, hipStream_t);
template int halo_unpack<double, T8gpuVars_f64>(const T8gpuHalo&, T8gpuVars_f64, hipStream_t);
template int exchange_wire<float>(const T8gpuHalo&, const int32_t*, const int32_t*, const int32_t*, hipStream_t);
template int exchange_wire<double>(const T8gpuHalo&, const int32_t*, const int32_t*, const int32_t*, hipStream_t);

}  // namespace t8gpu_hip

namespace {
using namespace t8gpu_hip;

// t8gpu_hip_halo_exchange_*: pack -> RCCL group -> unpack, all on s
template <class T, class V>
int exchange(const T8gpuHalo* h, V state, void* stream) {
  if (!h) return static_cast<int>(hipErrorInvalidValue);
  if (h->n_peers <= 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  T8_TRY((halo_pack<T, V>(*h, state, s)));
  T8_TRY(exchange_wire<T>(*h, h->peers, h->send_off, h->recv_off, s));
  return halo_unpack<T, V>(*h, state, s);
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
                T* dst_vol, int cells, void* stream) {
  if (cells < 1 || n_send < 0 || n_recv < 0) return static_cast<int>(hipErrorInvalidValue);
  hipStream_t  s = static_cast<hipStream_t>(stream);
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

int t8gpu_hip_halo_exchange_f32(const T8gpuHalo* h, T8gpuVars_f32 state, void* stream) { return exchange<float>(h, state, stream); }
int t8gpu_hip_halo_exchange_f64(const T8gpuHalo* h, T8gpuVars_f64 state, void* stream) { return exchange<double>(h, state, stream); }

int t8gpu_hip_repartition_f32(void* comm, int my_rank, int n_send, const int32_t* send_peer, const int32_t* send_first,
                              const int32_t* send_count, int n_recv, const int32_t* recv_peer, const int32_t* recv_first,
                              const int32_t* recv_count, T8gpuVars_f32 src, const float* src_volume, T8gpuVars_f32 dst, float* dst_volume,
                              int cells_per_element, void* stream) {
  return repartition(comm, my_rank, n_send, send_peer, send_first, send_count, n_recv, recv_peer, recv_first, recv_count, src, src_volume,
                     dst, dst_volume, cells_per_element, stream);
}
int t8gpu_hip_repartition_f64(void* comm, int my_rank, int n_send, const int32_t* send_peer, const int32_t* send_first,
                              const int32_t* send_count, int n_recv, const int32_t* recv_peer, const int32_t* recv_first,
                              const int32_t* recv_count, T8gpuVars_f64 src, const double* src_volume, T8gpuVars_f64 dst, double* dst_volume,
                              int cells_per_element, void* stream) {
  return repartition(comm, my_rank, n_send, send_peer, send_first, send_count, n_recv, recv_peer, recv_first, recv_count, src, src_volume,
                     dst, dst_volume, cells_per_element, stream);
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

}  // extern "C"
