// t8gpu/mesh/forest_core.h (MI355X backend)
//
// What MeshManager (mesh_manager.h) and SubgridMeshManager (subgrid_mesh_manager.h) have in common, written once. The two
// classes differ in their memory-manager base, in "element" vs "block of SubgridType::size cells" and in the data-transfer
// kernel of adapt(); everything else about a forest that is adapted, repartitioned and read through a ghost layer is here:
//   * hip::vars_t / to_vars and the f32 / f64 faces of the C-ABI calls the managers make (one mechanism: T8GPU_DISPATCH);
//   * DeviceBuffer<T>: an owning device array (the managers' connectivity, halo, scratch and staging arrays);
//   * read_host_connectivity: connectivity handle -> counts, face lists, xyz normals, areas, volumes, ghost lists;
//   * ForestCore<float_type>: forest handle, levels, rank layout, Transport, ghost lists + their device buffers, the common
//     device connectivity arrays, and adapt() / partition() / refresh_ghost_layer() on them. Each manager holds one as a
//     member and passes the cells per element (1 | SubgridType::size) and its data-transfer call.
#ifndef T8GPU_HIP_MESH_FOREST_CORE_H
#define T8GPU_HIP_MESH_FOREST_CORE_H

#include <t8gpu/backend/transport.h>
#include <t8gpu/memory/subgrid_memory_manager.h>

#include <t8gpu_hip.h>
#include <t8gpu_host.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace t8gpu {

  namespace hip {

    template<typename ft>
    using vars_t = std::conditional_t<std::is_same_v<ft, float>, T8gpuVars_f32, T8gpuVars_f64>;

    template<typename VariableType>
    auto to_vars(MemoryAccessorOwn<VariableType> acc) {
      using ft = typename variable_traits<VariableType>::float_type;
      static_assert(variable_traits<VariableType>::nb_variables == 5, "the Euler kernels expect Rho, Rho_v1..3, Rho_e");
      vars_t<ft> v;
      for (int k = 0; k < 5; k++) v.p[k] = acc.get(k);
      return v;
    }
    // Subgrid<4,4> / Subgrid<4,4,4>
    template<typename VariableType, typename SubgridType>
    auto to_vars(SubgridMemoryAccessorOwn<VariableType, SubgridType> acc) {
      using ft = typename variable_traits<VariableType>::float_type;
      static_assert(variable_traits<VariableType>::nb_variables == 5, "the Euler kernels expect Rho, Rho_v1..3, Rho_e");
      vars_t<ft> v;
      for (int k = 0; k < 5; k++) v.p[k] = acc.data(static_cast<typename variable_traits<VariableType>::index_type>(k));
      return v;
    }
    /// five planes `stride` values apart in one allocation
    template<typename ft>
    vars_t<ft> to_vars(ft* base, size_t stride) {
      vars_t<ft> v;
      for (int k = 0; k < 5; k++) v.p[k] = base + static_cast<size_t>(k) * stride;
      return v;
    }

// (hip_fast.h, which includes this header through the managers, uses the macro for its own calls and removes it)
#define T8GPU_DISPATCH(ft, name, ...)                                \
  do {                                                               \
    if constexpr (std::is_same_v<ft, float>) {                       \
      T8GPU_HIP_CHECK_ABI(name##_f32(__VA_ARGS__));                  \
    } else {                                                         \
      T8GPU_HIP_CHECK_ABI(name##_f64(__VA_ARGS__));                  \
    }                                                                \
  } while (0)

    /// adapt_variables_and_volume<<<>>> (mesh_manager.inl:165-193)
    template<typename ft>
    void adapt_variables_and_volume(int num_new_elements, int dim, int32_t const* adapt_data, vars_t<ft> old_variables,
                                    vars_t<ft> new_variables, ft const* volume_old, ft* volume_new) {
      T8GPU_DISPATCH(ft, t8gpu_hip_adapt_variables_and_volume, num_new_elements, dim, adapt_data, old_variables, new_variables,
                     volume_old, volume_new, nullptr);
    }
    /// adapt_variables + adapt_volume, block-wise (subgrid_mesh_manager.inl:246-425)
    template<typename ft>
    void subgrid_adapt_variables_and_volume(int rank, int num_new_elements, int32_t const* adapt_data, vars_t<ft> old_variables,
                                            vars_t<ft> new_variables, ft const* volume_old, ft* volume_new) {
      T8GPU_DISPATCH(ft, t8gpu_hip_subgrid_adapt_variables_and_volume, rank, num_new_elements, adapt_data, old_variables,
                     new_variables, volume_old, volume_new, nullptr);
    }
    template<typename ft>
    void host_scalar_variable(size_t n, ft const* variable, double* out) {
      T8GPU_DISPATCH(ft, t8gpu_hip_host_scalar_variable, n, variable, out, nullptr);
    }
    template<typename ft>
    void host_vector_variable(size_t n, ft const* v0, ft const* v1, ft const* v2, double* out) {
      T8GPU_DISPATCH(ft, t8gpu_hip_host_vector_variable, n, v0, v1, v2, out, nullptr);
    }
    template<typename ft>
    void column_major_to_z_order(int rank, int num_elements, ft const* from, ft* to) {
      T8GPU_DISPATCH(ft, t8gpu_hip_column_major_to_z_order, rank, num_elements, from, to, nullptr);
    }

  }  // namespace hip

  /// Owning device array: hipMalloc on construction (at least one element, so that get() is never null), hipFree on
  /// destruction, move-only. Not SharedDeviceVector, which mirrors the reference's per-rank pointer tables.
  template<typename T>
  class DeviceBuffer {
   public:
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t count) { T8GPU_CUDA_CHECK_ERROR(hipMalloc(&m_data, sizeof(T) * std::max<size_t>(count, 1))); }
    explicit DeviceBuffer(std::vector<T> const& host) : DeviceBuffer(host.size()) {
      if (!host.empty()) T8GPU_CUDA_CHECK_ERROR(hipMemcpy(m_data, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice));
    }
    ~DeviceBuffer() { reset(); }
    DeviceBuffer(DeviceBuffer&& o) noexcept : m_data{std::exchange(o.m_data, nullptr)} {}
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
      if (this != &o) {
        reset();
        m_data = std::exchange(o.m_data, nullptr);
      }
      return *this;
    }
    void reset() {
      (void)hipFree(m_data);
      m_data = nullptr;
    }
    [[nodiscard]] T* get() const { return m_data; }
    explicit         operator bool() const { return m_data != nullptr; }

   private:
    T* m_data = nullptr;
  };

  /// What the ghost layer needs besides the host mesh arrays (peers ascending; offsets have n_peers + 1 entries; send_idx = owned
  /// elements mirrored on a peer; the ghosts of peer j are the mirror slots N + [recv_off[j], recv_off[j + 1])).
  struct HostHaloArrays {
    std::vector<int32_t> peers, recv_off, send_off, send_idx;
  };

  /// T8_VTK_SCALAR / T8_VTK_VECTOR of t8code's t8_vtk_data_field_t: values per cell
  enum : int { T8GPU_VTK_SCALAR = 1, T8GPU_VTK_VECTOR = 3 };

  /// Named host array of doubles ready for the writer (mesh_manager.h / subgrid_mesh_manager.h:387-423: HostVariableInfo)
  struct HostVariableInfo {
    int                       m_type = T8GPU_VTK_SCALAR;  // T8GPU_VTK_SCALAR | T8GPU_VTK_VECTOR
    std::unique_ptr<double[]> m_data;
    std::string               m_name;
  };
  /// the three parallel arrays t8gpu_host_write_vtu takes for a list of fields
  struct VtkFields {
    std::vector<char const*>   names;
    std::vector<int32_t>       comps;
    std::vector<double const*> data;
    explicit VtkFields(std::vector<HostVariableInfo> const& host_variables) {
      for (auto const& h : host_variables) {
        names.push_back(h.m_name.c_str());
        comps.push_back(h.m_type);
        data.push_back(h.m_data.get());
      }
    }
    [[nodiscard]] int size() const { return static_cast<int>(names.size()); }
  };

  /// One rank's connectivity (t8gpu_host_connectivity_create[_subgrid]) into the fields HostMeshArrays and HostSubgridMeshArrays
  /// share: counts, face_neighbors[2F + B], face_surfaces[F + B], volumes[N + G] and face_normals with the adapter's THREE
  /// components per face (the caller keeps `dim` of them: keep_normal_components); `halo` (nullable) receives the ghost lists.
  template<typename HostArrays>
  void read_host_connectivity(void const* connectivity, HostArrays& m, HostHaloArrays* halo) {
    int64_t c[6];
    t8gpu_host_connectivity_counts(connectivity, c);
    m.num_local_elements = static_cast<int32_t>(c[0]); m.num_ghost_elements = static_cast<int32_t>(c[1]);
    m.num_local_faces = static_cast<int32_t>(c[2]); m.num_local_boundary_faces = static_cast<int32_t>(c[3]);
    m.face_neighbors.resize(2 * c[2] + c[3]);
    m.face_normals.resize(3 * (c[2] + c[3]));
    m.face_surfaces.resize(c[2] + c[3]);
    m.volumes.resize(c[0] + c[1]);
    HostHaloArrays hh;
    hh.peers.resize(c[4]); hh.recv_off.resize(c[4] + 1); hh.send_off.resize(c[4] + 1); hh.send_idx.resize(c[5]);
    t8gpu_host_connectivity_arrays(connectivity, m.face_neighbors.data(), m.face_normals.data(), m.face_surfaces.data(), m.volumes.data(),
                                   hh.peers.data(), hh.recv_off.data(), hh.send_off.data(), hh.send_idx.data());
    if (halo) *halo = std::move(hh);
  }
  /// xyz normals -> the first `dim` components of each, in place (the accessors stride by `dim`)
  inline void keep_normal_components(std::vector<double>& normals, size_t dim) {
    const size_t nf = normals.size() / 3;
    for (size_t i = 0; i < nf; i++)
      for (size_t k = 0; k < dim; k++) normals[dim * i + k] = normals[3 * i + k];
    normals.resize(dim * nf);
  }

  template<typename float_type>
  class ForestCore {
   public:
    using vars = hip::vars_t<float_type>;
    struct ForestDeleter {
      void operator()(void* f) const { t8gpu_synth_mesh_destroy(f); }
    };
    using ForestHandle = std::unique_ptr<void, ForestDeleter>;

    /// `owner`: the manager's class name, for the abort messages; `cells_per_element`: values per variable and element
    ForestCore(char const* owner, size_t cells_per_element, int lowest_level, int highest_level, sc_MPI_Comm comm)
        : min_level{lowest_level}, max_level{highest_level}, m_owner{owner}, m_cells{cells_per_element} {
      detail::comm_layout(comm, rank, nb_ranks);
    }
    static int rank_of(sc_MPI_Comm comm) {
      int r = 0, n = 1;
      detail::comm_layout(comm, r, n);
      return r;
    }
    static int size_of(sc_MPI_Comm comm) {
      int r = 0, n = 1;
      detail::comm_layout(comm, r, n);
      return n;
    }

    ForestHandle   forest;                // synthetic forest (owned) when the manager was constructed from one
    int            min_level, max_level;   // bounds of adapt()
    int            rank = 0, nb_ranks = 1;
    // several ranks: the channel (not owned), the ghost lists of the current share and the device side of refresh_ghost_layer()
    Transport*               transport = nullptr;
    HostHaloArrays           halo;
    DeviceBuffer<int32_t>    send_idx;
    DeviceBuffer<float_type> sendbuf, recvbuf;
    // device connectivity both accessors read: ranks[N + G], indices[N + G], face_neighbors[2F + B], normals, areas
    int32_t                  num_local_elements = 0, num_ghost_elements = 0;
    DeviceBuffer<int>        ranks;
    DeviceBuffer<int32_t>    indices, face_neighbors;
    DeviceBuffer<float_type> face_normals, face_surfaces;
    /// what adapt() leaves for partition()
    struct Pending {
      ForestHandle             forest;           // the adapted forest (replicated)
      DeviceBuffer<float_type> planes, volume;   // this rank's n = have_off[r + 1] - have_off[r] adapted elements: 5 planes of cells x n values, n volumes
      std::vector<int64_t>     have_off;         // new elements made from rank q's old ones: [have_off[q], have_off[q + 1])
    } pending;

    void require_transport(char const* what) const {
      if (transport) return;
      std::fprintf(stderr, "t8gpu: %s on %d ranks needs a transport (%s::set_transport)\n", what, nb_ranks, m_owner);
      std::abort();
    }

    /// compute_connectivity_information (mesh_manager.inl:333-481): device copies of the face arrays of `m` (HostMeshArrays |
    /// HostSubgridMeshArrays) and, on several ranks, the buffers of the ghost exchange for the current `halo`
    template<typename HostArrays>
    void upload_connectivity(HostArrays const& m, int owner_rank) {
      num_local_elements = m.num_local_elements;
      num_ghost_elements = m.num_ghost_elements;
      const size_t         tot = static_cast<size_t>(m.num_local_elements) + m.num_ghost_elements;
      std::vector<int32_t> idx(tot);
      for (size_t i = 0; i < tot; i++) idx[i] = static_cast<int32_t>(i);
      ranks          = DeviceBuffer<int>(std::vector<int>(tot, owner_rank));
      indices        = DeviceBuffer<int32_t>(idx);
      face_neighbors = DeviceBuffer<int32_t>(m.face_neighbors);
      face_normals   = DeviceBuffer<float_type>(std::vector<float_type>(m.face_normals.begin(), m.face_normals.end()));
      face_surfaces  = DeviceBuffer<float_type>(std::vector<float_type>(m.face_surfaces.begin(), m.face_surfaces.end()));
      send_idx.reset();
      sendbuf.reset();
      recvbuf.reset();
      if (nb_ranks > 1 && !halo.peers.empty()) {   // device side of refresh_ghost_layer(): whole elements on the wire
        send_idx = DeviceBuffer<int32_t>(halo.send_idx);
        sendbuf  = DeviceBuffer<float_type>(5 * m_cells * halo.send_idx.size() + 1);
        recvbuf  = DeviceBuffer<float_type>(5 * m_cells * static_cast<size_t>(m.num_ghost_elements) + 1);
      }
    }

    /// Refresh the ghost mirror slots [N, N + G) of the five planes `state` from their owners; a no-op on one rank
    void refresh_ghost_layer(vars state) {
      if (nb_ranks <= 1 || halo.peers.empty()) return;
      require_transport("refresh_ghost_layer()");
      T8gpuHalo h{};
      h.num_elements = num_local_elements; h.num_ghosts = num_ghost_elements;
      h.n_peers = static_cast<int32_t>(halo.peers.size()); h.n_send = static_cast<int32_t>(halo.send_idx.size());
      h.cells_per_element = static_cast<int32_t>(m_cells);
      h.peers = halo.peers.data(); h.send_off = halo.send_off.data(); h.recv_off = halo.recv_off.data();
      h.send_idx = send_idx.get(); h.sendbuf = sendbuf.get(); h.recvbuf = recvbuf.get();
      transport->halo_exchange(h, state);
    }

    /// The forest half of adapt() and the data transfer into temporary planes (`pending`). The reference's adapt callback on the
    /// criteria (refine above `threshold`, coarsen a family whose first four members are below it), 2:1 balance, then
    /// `transfer(n, adapt_data, new_variables, new_volume)` -- the manager's data-transfer kernel from the planes it holds --
    /// for this rank's n adapted elements. On several ranks (t8gpu_amd/amr.py: PartitionedAdapt, the same scheme in C++) the
    /// forest description is replicated: the criteria of all ranks are gathered, every rank evaluates the callback on the whole
    /// array, and families cut by a rank boundary are not coarsened (their members' data live on two ranks). The result is
    /// what the reference holds after its adapt(): adapted elements on their old owners.
    template<typename Transfer>
    void adapt(std::vector<float_type> const& refinement_criteria, double threshold, Transfer&& transfer) {
      if (!forest) {
        std::fprintf(stderr, "t8gpu: adapt() needs a manager constructed from a forest\n");
        std::abort();
      }
      const int R = nb_ranks, r = rank;
      if (R > 1) require_transport("adapt()");
      pending = Pending{};   // adapt() twice without partition(): drop the first
      const int64_t        n_glob = t8gpu_synth_mesh_num_elements(forest.get());
      std::vector<int64_t> old_off(static_cast<size_t>(R) + 1);
      for (int q = 0; q <= R; q++) old_off[q] = n_glob * q / R;
      const int64_t n_mine = old_off[r + 1] - old_off[r];
      if (static_cast<int64_t>(refinement_criteria.size()) < n_mine) std::abort();
      // 1. all criteria on every rank
      std::vector<double> all(refinement_criteria.begin(), refinement_criteria.begin() + n_mine);
      if (R > 1) {
        DeviceBuffer<double> d_mine(all), d_all(static_cast<size_t>(n_glob));
        all.resize(static_cast<size_t>(n_glob));
        transport->allgatherv(d_mine.get(), d_all.get(), old_off.data());
        T8GPU_CUDA_CHECK_ERROR(hipMemcpy(all.data(), d_all.get(), sizeof(double) * n_glob, hipMemcpyDeviceToHost));
      }
      // 2. the adapt callback on the whole forest, families split by a rank boundary left alone; the new forest
      std::vector<int8_t> marks(static_cast<size_t>(n_glob));
      t8gpu_synth_mesh_marks(forest.get(), all.data(), threshold, min_level, max_level, 4, marks.data());
      if (R > 1) t8gpu_synth_mesh_unmark_split_families(forest.get(), marks.data(), old_off.data() + 1, R - 1);
      ForestHandle new_forest{t8gpu_synth_mesh_adapt(forest.get(), marks.data())};
      if (!new_forest) {
        std::fprintf(stderr, "t8gpu: forest adaptation failed\n");
        std::abort();
      }
      const int64_t        n_new = t8gpu_synth_mesh_num_elements(new_forest.get());
      std::vector<int32_t> adapt_data(static_cast<size_t>(n_new) + 1);
      if (t8gpu_synth_mesh_adapt_data(forest.get(), new_forest.get(), adapt_data.data()) != 0) std::abort();
      pending.have_off.assign(static_cast<size_t>(R) + 1, n_new);
      for (int q = 0; q < R; q++)
        pending.have_off[q] = std::lower_bound(adapt_data.begin(), adapt_data.begin() + n_new, static_cast<int32_t>(old_off[q])) - adapt_data.begin();
      // 3. this rank's elements through the data-transfer kernel into 5 temporary planes + their volumes
      const int64_t        a  = pending.have_off[r];
      const int32_t        nh = pending_count();
      std::vector<int32_t> local(static_cast<size_t>(nh) + 1);
      for (int32_t i = 0; i <= nh; i++) local[i] = adapt_data[a + i] - static_cast<int32_t>(old_off[r]);
      DeviceBuffer<int32_t> d_ad(local);
      pending.planes = DeviceBuffer<float_type>(5 * pending_stride());
      pending.volume = DeviceBuffer<float_type>(static_cast<size_t>(nh));
      if (nh > 0) transfer(nh, d_ad.get(), pending_vars(), pending.volume.get());
      T8GPU_CUDA_CHECK_ERROR(hipDeviceSynchronize());
      pending.forest = std::move(new_forest);
    }
    /// this rank's adapted elements waiting in `pending`
    [[nodiscard]] int32_t pending_count() const { return static_cast<int32_t>(pending.have_off[rank + 1] - pending.have_off[rank]); }

    /// One rank: the adapted elements are where they belong. Copies them into `dst` / `dst_volume` (the manager's planes,
    /// resized to pending_count() elements) and installs the new forest.
    void install_pending(vars dst, float_type* dst_volume) {
      const size_t n   = static_cast<size_t>(pending_count());
      const vars   src = pending_vars();
      for (int k = 0; k < 5; k++) T8GPU_CUDA_CHECK_ERROR(hipMemcpy(dst.p[k], src.p[k], sizeof(float_type) * m_cells * n, hipMemcpyDeviceToDevice));
      T8GPU_CUDA_CHECK_ERROR(hipMemcpy(dst_volume, pending.volume.get(), sizeof(float_type) * n, hipMemcpyDeviceToDevice));
      forest  = std::move(pending.forest);
      pending = Pending{};
    }

    /// false when partition() is the identity: one rank, or no adapt() pending (t8_forest_partition moves nothing)
    [[nodiscard]] bool partition_pending() const {
      if (!pending.forest) return false;
      require_transport("partition()");
      return true;
    }
    /// partition() after adapt() on several ranks: every run of adapted elements goes to its owner in the equal split of the NEW
    /// curve (t8gpu_hip_repartition_*: the old owner sends, where the reference's new owner pulls through CUDA-IPC pointers,
    /// partition_data<<<>>> mesh_manager.inl:626-643), into `dst` / `dst_volume` -- the manager's planes, already resized for
    /// `m`, the new share's connectivity, whose ghost lists are `new_halo`. Installs the new forest; the caller uploads `m`.
    template<typename HostArrays>
    void partition(HostArrays const& m, HostHaloArrays new_halo, vars dst, float_type* dst_volume) {
      const int     R = nb_ranks, r = rank;
      const int64_t n_new = t8gpu_synth_mesh_num_elements(pending.forest.get());
      auto off = [&](int q) { return n_new * q / R; };
      const int64_t a = pending.have_off[r], b = pending.have_off[r + 1], lo = off(r), hi = off(r + 1);
      std::vector<int32_t> sp, sf, sc, rp, rf, rc;
      for (int q = 0; q < R; q++) {
        const int64_t s0 = std::max(a, off(q)), s1 = std::min(b, off(q + 1));
        if (s1 > s0) { sp.push_back(q); sf.push_back(static_cast<int32_t>(s0 - a)); sc.push_back(static_cast<int32_t>(s1 - s0)); }
        const int64_t r0 = std::max(pending.have_off[q], lo), r1 = std::min(pending.have_off[q + 1], hi);
        if (r1 > r0) { rp.push_back(q); rf.push_back(static_cast<int32_t>(r0 - lo)); rc.push_back(static_cast<int32_t>(r1 - r0)); }
      }
      transport->repartition(static_cast<int>(sp.size()), sp.data(), sf.data(), sc.data(), static_cast<int>(rp.size()), rp.data(), rf.data(),
                             rc.data(), pending_vars(), pending.volume.get(), dst, dst_volume, static_cast<int>(m_cells));
      forest  = std::move(pending.forest);
      pending = Pending{};
      halo    = std::move(new_halo);
      // the volumes of the ghost slots come with the connectivity (the owned ones arrived with the elements)
      if (m.num_ghost_elements > 0) {
        std::vector<float_type> gv(m.volumes.begin() + m.num_local_elements, m.volumes.end());
        T8GPU_CUDA_CHECK_ERROR(hipMemcpy(dst_volume + m.num_local_elements, gv.data(), sizeof(float_type) * gv.size(), hipMemcpyHostToDevice));
      }
    }

   private:
    char const* m_owner;
    size_t      m_cells;

    [[nodiscard]] size_t pending_stride() const { return m_cells * static_cast<size_t>(std::max(pending_count(), 1)); }
    [[nodiscard]] vars   pending_vars() const { return hip::to_vars(pending.planes.get(), pending_stride()); }
  };

}  // namespace t8gpu

#endif  // T8GPU_HIP_MESH_FOREST_CORE_H
