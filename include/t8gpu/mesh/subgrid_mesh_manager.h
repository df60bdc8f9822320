// t8gpu/mesh/subgrid_mesh_manager.h (MI355X backend)
//
// SubgridMeshConnectivityAccessor<float_type, SubgridType>: device view of the coarse-face lists of a
// Subgrid mesh with the getters of the reference (t8gpu/mesh/subgrid_mesh_manager.h:29-216): the plain
// arrays plus face_level_difference[F] (level(right) - level(left) <= 0) and face_neighbor_offset[rank*F]
// (anchor inside the right block; subgrid_mesh_manager.inl:587-680). Normals have SubgridType::rank
// components. SubgridMeshManager<V, S, Subgrid>: the class of the reference (subgrid_mesh_manager.h:266-509) with
// the same public members (constructor (comm, scheme, cmesh, forest), initialize_variables, adapt, partition,
// compute_connectivity_information, save_variable_to_vtk, save_mesh_to_vtk, HostVariableInfo, get_host_*,
// save_variables_to_vtk, get_connectivity_information, get_num_*, min_level / max_level) on top of
// SubgridMemoryManager. As for MeshManager (mesh_manager.h) the t8code constructor is declared for every build and
// defined by the t8code adapter only; the synthetic forest / host arrays constructors make the class usable here,
// and SyntheticSubgridMeshManager is an alias kept for the earlier name. What it shares with MeshManager (forest, adapt,
// partition, ghost layer, common device arrays) is a ForestCore member (forest_core.h) with SubgridType::size cells per element.
#ifndef T8GPU_HIP_MESH_SUBGRID_MESH_MANAGER_H
#define T8GPU_HIP_MESH_SUBGRID_MESH_MANAGER_H

#include <t8gpu/memory/subgrid_memory_manager.h>
#include <t8gpu/mesh/mesh_manager.h>

#include <algorithm>
#include <string>
#include <vector>

namespace t8gpu {

  template<typename float_type, typename SubgridType>
  class SubgridMeshConnectivityAccessor {
    template<typename VT, typename ST, typename SG>
    friend class SubgridMeshManager;
    static constexpr int dim = SubgridType::rank;

   public:
    SubgridMeshConnectivityAccessor(SubgridMeshConnectivityAccessor const&)            = default;
    SubgridMeshConnectivityAccessor& operator=(SubgridMeshConnectivityAccessor const&) = default;

    /// public constructor: the arrays come from any provider of the reference's formats
    __host__ __device__ SubgridMeshConnectivityAccessor(int const* ranks, t8_locidx_t const* indices, t8_locidx_t const* fn,
                                                        t8_locidx_t const* level_difference, t8_locidx_t const* neighbor_offset,
                                                        float_type const* normals, float_type const* surfaces, t8_locidx_t F,
                                                        t8_locidx_t B)
        : m_ranks{ranks}, m_indices{indices}, m_face_neighbors{fn}, m_face_level_difference{level_difference},
          m_face_neighbor_offset{neighbor_offset}, m_face_normals{normals}, m_face_surfaces{surfaces},
          m_num_local_faces{F}, m_num_local_boundary_faces{B} {}

    [[nodiscard]] __host__ __device__ inline t8_locidx_t get_num_local_faces() const { return m_num_local_faces; }
    [[nodiscard]] __host__ __device__ inline t8_locidx_t get_num_local_boundary_faces() const { return m_num_local_boundary_faces; }
    [[nodiscard]] __device__ inline float_type get_face_surface(int f) const { return m_face_surfaces[f]; }
    [[nodiscard]] __device__ inline float_type get_boundary_face_surface(int f) const { return m_face_surfaces[m_num_local_faces + f]; }
    [[nodiscard]] __device__ inline std::array<float_type, dim> get_face_normal(int f) const { return normal_at(f); }
    [[nodiscard]] __device__ inline std::array<float_type, dim> get_boundary_face_normal(int f) const { return normal_at(m_num_local_faces + f); }
    [[nodiscard]] __device__ inline t8_locidx_t get_face_level_difference(int f) const { return m_face_level_difference[f]; }
    [[nodiscard]] __device__ inline std::array<t8_locidx_t, SubgridType::rank> get_face_neighbor_offset(int f) const {
      std::array<t8_locidx_t, SubgridType::rank> o{};
      for (int k = 0; k < dim; k++) o[k] = m_face_neighbor_offset[dim * f + k];
      return o;
    }
    [[nodiscard]] __device__ inline std::array<t8_locidx_t, 2> get_face_neighbor_indices(int f) const {
      return {m_face_neighbors[2 * f], m_face_neighbors[2 * f + 1]};
    }
    [[nodiscard]] __device__ inline t8_locidx_t get_boundary_face_neighbor_index(int f) const { return m_face_neighbors[2 * m_num_local_faces + f]; }
    [[nodiscard]] __device__ inline t8_locidx_t get_element_owner_rank(int e) const { return m_ranks[e]; }
    [[nodiscard]] __device__ inline t8_locidx_t get_element_owner_remote_index(int e) const { return m_indices[e]; }

   private:
    int const*         m_ranks;
    t8_locidx_t const* m_indices;
    t8_locidx_t const* m_face_neighbors;
    t8_locidx_t const* m_face_level_difference;
    t8_locidx_t const* m_face_neighbor_offset;
    float_type const*  m_face_normals;
    float_type const*  m_face_surfaces;
    t8_locidx_t        m_num_local_faces;
    t8_locidx_t        m_num_local_boundary_faces;

    __device__ inline std::array<float_type, dim> normal_at(int slot) const {
      std::array<float_type, dim> n{};
      for (int k = 0; k < dim; k++) n[k] = m_face_normals[dim * slot + k];
      return n;
    }
  };

  /// One rank's Subgrid mesh in the reference's array formats (subgrid_mesh_manager.h:29-216); normals have
  /// `rank` components, level differences are level(right) - level(left) <= 0.
  struct HostSubgridMeshArrays {
    int32_t num_local_elements = 0, num_ghost_elements = 0, num_local_faces = 0, num_local_boundary_faces = 0, rank = 3;
    int     mpirank = 0;
    std::vector<int32_t> face_neighbors, face_level_difference, face_neighbor_offset;
    std::vector<double>  face_normals, face_surfaces, volumes;
    // only needed by the VTK members: geometry of the owned blocks on the unit domain
    int64_t              first_global_element = 0;
    std::vector<double>  centres;   // [N][3]
    std::vector<int32_t> levels;    // [N]
  };

  template<typename VariableType, typename StepType, typename SubgridType>
  class SubgridMeshManager : public SubgridMemoryManager<VariableType, StepType, SubgridType> {
   public:
    using float_type                  = typename variable_traits<VariableType>::float_type;
    using variable_index_type         = typename variable_traits<VariableType>::index_type;
    static constexpr int nb_variables = variable_traits<VariableType>::nb_variables;
    static constexpr int dim          = SubgridType::rank;

    using step_index_type            = typename step_traits<StepType>::index_type;
    static constexpr size_t nb_steps = step_traits<StepType>::nb_steps;

    static constexpr t8_locidx_t min_level = 1;   // subgrid_mesh_manager.h:276-277
    static constexpr t8_locidx_t max_level = 6;

    /// subgrid_mesh_manager.h:288 / .inl:20-75: takes ownership of cmesh and forest. Declared for every build, DEFINED
    /// by the t8code adapter only; see MeshManager.
    SubgridMeshManager(sc_MPI_Comm comm, t8_scheme_cxx_t* scheme, t8_cmesh_t cmesh, t8_forest_t forest);

    explicit SubgridMeshManager(HostSubgridMeshArrays const& m, sc_MPI_Comm comm = sc_MPI_COMM_WORLD)
        : SubgridMemoryManager<VariableType, StepType, SubgridType>(static_cast<size_t>(m.num_local_elements) + m.num_ghost_elements, comm),
          m_core{"SubgridMeshManager", SubgridType::size, min_level, max_level, comm} {
      rebuild_connectivity(m);
      const size_t            tot = static_cast<size_t>(m.num_local_elements) + m.num_ghost_elements;
      std::vector<float_type> vol(m.volumes.begin(), m.volumes.end());
      vol.resize(tot, float_type(1));
      this->set_volume(vol);
    }
    /// From a synthetic forest (owned afterwards): stands for SubgridMeshManager(comm, scheme, cmesh, forest)
    /// (subgrid_mesh_manager.inl:3-60); connectivity through the forest-query adapter. On several ranks every rank passes
    /// its own handle of the same forest and owns an equal share of the curve; set_transport() must follow (see MeshManager).
    explicit SubgridMeshManager(void* synth_mesh, int lowest_level = min_level, int highest_level = max_level,
                                sc_MPI_Comm comm = sc_MPI_COMM_WORLD)
        : SubgridMeshManager(arrays_of(synth_mesh, Core::rank_of(comm), Core::size_of(comm), nullptr), comm) {
      m_core.forest.reset(synth_mesh);
      m_core.min_level = lowest_level;
      m_core.max_level = highest_level;
      if (m_core.nb_ranks > 1) rebuild_connectivity(arrays_of(synth_mesh, m_core.rank, m_core.nb_ranks, &m_core.halo));   // (+ the halo lists)
    }
    /// The channel adapt() / partition() / refresh_ghost_layer() use on several ranks (not owned). See backend/transport.h.
    void set_transport(Transport* transport) { m_core.transport = transport; }

    /// subgrid_mesh_manager.inl:144-194: `func(accessor, forest, tree_idx, element, e_idx)` fills ONE value per
    /// variable and block in a host MemoryAccessorOwn; every subcell of the block gets that value in Step 0
    /// (copy_variables_coarse_mesh_to_fine). With the synthetic provider `element` is a SyntheticElement.
    template<typename Func>
    void initialize_variables(Func func) {
      constexpr size_t S = SubgridType::size;
      const size_t     n = static_cast<size_t>(m_host.num_local_elements), tot = n + static_cast<size_t>(m_host.num_ghost_elements);
      std::array<std::vector<float_type>, nb_variables> coarse{};
      std::array<float_type*, nb_variables>             array{};
      for (size_t k = 0; k < static_cast<size_t>(nb_variables); k++) {
        coarse[k].resize(n);
        array[k] = coarse[k].data();
      }
      MemoryAccessorOwn<VariableType> host_variable_memory{array};
      for (size_t e = 0; e < n; e++) {
        SyntheticElement el{{m_host.centres[3 * e], m_host.centres[3 * e + 1], m_host.centres[3 * e + 2]}, m_host.levels[e],
                            m_host.volumes[e]};
        func(host_variable_memory, reinterpret_cast<t8_forest_t>(m_core.forest.get()), t8_locidx_t{0},
             reinterpret_cast<t8_element_t const*>(&el), static_cast<t8_locidx_t>(e));
      }
      std::vector<float_type> fine(tot * S, float_type(0));
      for (size_t k = 0; k < static_cast<size_t>(nb_variables); k++) {
        for (size_t e = 0; e < n; e++) std::fill(fine.begin() + e * S, fine.begin() + (e + 1) * S, coarse[k][e]);
        this->set_variable(static_cast<step_index_type>(0), static_cast<variable_index_type>(k), fine);
      }
    }

    /// subgrid_mesh_manager.h:327 (the reference's signature)
    void adapt(thrust::host_vector<float_type> const& refinement_criteria, step_index_type step) {
      adapt(std::vector<float_type>(refinement_criteria.begin(), refinement_criteria.end()), step);
    }

    /// subgrid_mesh_manager.inl:1217-1369. As MeshManager::partition with whole blocks for elements: every run of adapted
    /// blocks goes to its owner in the new equal split (ForestCore::partition with cells_per_element = 4^rank; the reference's
    /// new owner pulls through CUDA-IPC pointers, partition_data<<<>>> :1217-1250), the new forest is installed and the
    /// connectivity rebuilt. Only `step` and the volumes are valid afterwards. The identity on one rank or when no adapt()
    /// is pending.
    void partition(step_index_type step) {
      if (!m_core.partition_pending()) return;
      HostHaloArrays        halo;
      HostSubgridMeshArrays m = arrays_of(m_core.pending.forest.get(), m_core.rank, m_core.nb_ranks, &halo);   // first: it says how many ghost blocks the planes need
      this->resize(static_cast<size_t>(m.num_local_elements) + m.num_ghost_elements);
      m_core.partition(m, std::move(halo), hip::to_vars(this->get_own_variables(step)), this->get_own_volume());
      rebuild_connectivity(m);
    }

    /// Refresh the ghost BLOCKS [N, N + G) of the five planes of `step` from their owners (several ranks only; see
    /// MeshManager::refresh_ghost_layer). The step drivers refresh what they read themselves.
    void refresh_ghost_layer(step_index_type step) { m_core.refresh_ghost_layer(hip::to_vars(this->get_own_variables(step))); }
    [[nodiscard]] HostHaloArrays const& host_halo() const { return m_core.halo; }
    [[nodiscard]] int comm_rank() const { return m_core.rank; }
    [[nodiscard]] int comm_size() const { return m_core.nb_ranks; }

    /// subgrid_mesh_manager.inl:560-961: coarse-face lists, level differences, neighbour offsets -> device arrays
    void compute_connectivity_information() {
      if (m_core.forest)
        rebuild_connectivity(arrays_of(m_core.forest.get(), m_core.rank, m_core.nb_ranks, m_core.nb_ranks > 1 ? &m_core.halo : nullptr));
    }

    /// SubgridMeshManager::adapt (subgrid_mesh_manager.inl:428-558): adapt callback on the per-block criteria, 2:1
    /// balance, block-wise transfer adapt_variables + adapt_volume (:246-425) from `step` into temporary planes
    /// (ForestCore::adapt, the scheme of MeshManager::adapt with blocks for elements). One rank: copied back, new
    /// connectivity; several ranks: partition() ships them. Only `step` and the volumes are valid afterwards.
    void adapt(std::vector<float_type> const& refinement_criteria, step_index_type step, double threshold = 0.02) {
      m_core.adapt(refinement_criteria, threshold, [&](int32_t n, int32_t const* adapt_data, typename Core::vars new_variables, float_type* new_volume) {
        hip::subgrid_adapt_variables_and_volume<float_type>(SubgridType::rank, n, adapt_data, hip::to_vars(this->get_own_variables(step)),
                                                            new_variables, this->get_own_volume(), new_volume);
      });
      if (m_core.nb_ranks > 1) return;
      this->resize(static_cast<size_t>(m_core.pending_count()));
      m_core.install_pending(hip::to_vars(this->get_own_variables(step)), this->get_own_volume());
      rebuild_connectivity(arrays_of(m_core.forest.get(), 0, 1, nullptr));
    }

    [[nodiscard]] void const* forest() const { return m_core.forest.get(); }

    SubgridMeshManager(SubgridMeshManager const&)            = delete;
    SubgridMeshManager& operator=(SubgridMeshManager const&) = delete;

    [[nodiscard]] SubgridMeshConnectivityAccessor<float_type, SubgridType> get_connectivity_information() const {
      return {m_core.ranks.get(), m_core.indices.get(), m_core.face_neighbors.get(), m_level_difference.get(), m_neighbor_offset.get(),
              m_core.face_normals.get(), m_core.face_surfaces.get(), m_host.num_local_faces, m_host.num_local_boundary_faces};
    }
    [[nodiscard]] t8_locidx_t get_num_local_elements() const { return m_host.num_local_elements; }
    [[nodiscard]] t8_locidx_t get_num_ghost_elements() const { return m_host.num_ghost_elements; }
    [[nodiscard]] t8_locidx_t get_num_local_faces() const { return m_host.num_local_faces; }
    [[nodiscard]] t8_locidx_t get_num_local_boundary_faces() const { return m_host.num_local_boundary_faces; }
    [[nodiscard]] HostSubgridMeshArrays const& host_arrays() const { return m_host; }

    /// Named host array of doubles ready for the writer (subgrid_mesh_manager.h:387-423: HostVariableInfo)
    using HostVariableInfo = t8gpu::HostVariableInfo;

    /// subgrid_mesh_manager.h:426. One variable of one step on the host: every subcell, in the z-order of the forest
    /// refined log2(extent) times, as doubles (z-order + cast on the device, one D2H copy). The reference copies the
    /// first num_local_elements values of the block-major array only (subgrid_mesh_manager.inl:1138-1157) and its
    /// save_variables_to_vtk is commented out (:1181-1206); this is the field those two were written to deliver.
    [[nodiscard]] HostVariableInfo get_host_scalar_variable(step_index_type step, variable_index_type variable,
                                                            std::string const& name) const {
      const size_t n = static_cast<size_t>(m_host.num_local_elements) * SubgridType::size;
      std::unique_ptr<double[]> h = std::make_unique<double[]>(n ? n : 1);
      z_order_doubles(step, variable);
      T8GPU_CUDA_CHECK_ERROR(hipMemcpy(h.get(), m_scratch64.get(), sizeof(double) * n, hipMemcpyDeviceToHost));
      return {T8GPU_VTK_SCALAR, std::move(h), name};
    }
    /// subgrid_mesh_manager.h:438: three variables as interleaved xyz doubles per subcell (same ordering as above)
    [[nodiscard]] HostVariableInfo get_host_vector_variable(step_index_type step, std::array<variable_index_type, 3> variables,
                                                            std::string const& name) const {
      const size_t n = static_cast<size_t>(m_host.num_local_elements) * SubgridType::size;
      std::unique_ptr<double[]> h = std::make_unique<double[]>(3 * n ? 3 * n : 1);
      std::vector<double>       one(n);
      for (int c = 0; c < 3; c++) {
        z_order_doubles(step, variables[c]);
        T8GPU_CUDA_CHECK_ERROR(hipMemcpy(one.data(), m_scratch64.get(), sizeof(double) * n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) h[3 * i + c] = one[i];
      }
      return {T8GPU_VTK_VECTOR, std::move(h), name};
    }
    /// subgrid_mesh_manager.h:446: all fields in one file, on the forest refined down to the subcells
    void save_variables_to_vtk(std::vector<HostVariableInfo> host_variables, std::string const& prefix) const {
      const VtkFields fields(host_variables);
      write(prefix, SubgridType::template extent<0>, fields.size(), fields.names.data(), fields.comps.data(), fields.data.data());
    }

    /// subgrid_mesh_manager.inl:1051-1138: the variable on the forest refined uniformly twice (z-order), field "variables"
    void save_variable_to_vtk(step_index_type step, variable_index_type variable, std::string const& prefix) const {
      std::vector<HostVariableInfo> v;
      v.push_back(get_host_scalar_variable(step, variable, "variables"));
      save_variables_to_vtk(std::move(v), prefix);
    }
    /// subgrid_mesh_manager.inl:1185-1206: the forest itself, no data
    void save_mesh_to_vtk(std::string const& prefix) const { write(prefix, 1, 0, nullptr, nullptr, nullptr); }

   private:
    using SubgridMemoryManager<VariableType, StepType, SubgridType>::resize;   // subgrid_mesh_manager.h:466
    using Core = ForestCore<float_type>;

    Core                             m_core;   // forest, rank layout, transport, ghost lists, common device connectivity (forest_core.h)
    HostSubgridMeshArrays            m_host;
    DeviceBuffer<t8_locidx_t>        m_level_difference, m_neighbor_offset;
    mutable DeviceBuffer<float_type> m_scratch;   // z-ordered copy of one variable (float_type / double)
    mutable DeviceBuffer<double>     m_scratch64;

    /// rank `rank` of `nranks`' share of the forest; `halo` (nullable) receives the ghost lists
    static HostSubgridMeshArrays arrays_of(void* forest, int rank, int nranks, HostHaloArrays* halo) {
      constexpr int     R = SubgridType::rank;
      T8gpuForestQuery* q = t8gpu_synth_query_create(forest, rank, nranks);
      void*             h = q ? t8gpu_host_connectivity_create_subgrid(q, R) : nullptr;
      if (!h) {
        std::fprintf(stderr, "t8gpu: connectivity of the synthetic forest could not be built\n");
        std::abort();
      }
      HostSubgridMeshArrays m;
      read_host_connectivity(h, m, halo);
      m.rank = R;
      m.mpirank = rank;
      m.first_global_element = t8gpu_synth_mesh_num_elements(forest) * rank / nranks;
      m.face_level_difference.resize(static_cast<size_t>(m.num_local_faces));
      m.face_neighbor_offset.resize(static_cast<size_t>(R) * m.num_local_faces);
      t8gpu_host_connectivity_subgrid_arrays(h, m.face_level_difference.data(), m.face_neighbor_offset.data());
      t8gpu_host_connectivity_destroy(h);
      t8gpu_synth_query_destroy(q);
      keep_normal_components(m.face_normals, R);   // the Subgrid accessors carry `rank` components
      const size_t tot = static_cast<size_t>(m.num_local_elements) + m.num_ghost_elements;
      void*        part = t8gpu_synth_part_create(forest, rank, nranks, 1, R);
      m.levels.resize(tot);           // (the provider lists owned + ghost blocks; the manager keeps the owned ones)
      m.centres.resize(3 * tot);
      t8gpu_synth_part_elements(part, m.levels.data(), nullptr, m.centres.data());
      m.levels.resize(m.num_local_elements);
      m.centres.resize(3 * static_cast<size_t>(m.num_local_elements));
      t8gpu_synth_part_destroy(part);
      return m;
    }
    void rebuild_connectivity(HostSubgridMeshArrays const& m) {
      m_host = m;
      m_core.upload_connectivity(m, m.mpirank);
      m_level_difference = DeviceBuffer<t8_locidx_t>(m.face_level_difference);
      m_neighbor_offset  = DeviceBuffer<t8_locidx_t>(m.face_neighbor_offset);
      m_scratch.reset();   // sized for the old mesh
      m_scratch64.reset();
    }

    /// column_major_to_z_order (subgrid_mesh_manager.inl:1008-1049) + cast: `variable` of `step` -> m_scratch64
    void z_order_doubles(step_index_type step, variable_index_type variable) const {
      const size_t n = static_cast<size_t>(m_host.num_local_elements) * SubgridType::size;
      if (!m_scratch) m_scratch = DeviceBuffer<float_type>(n);
      if (!m_scratch64) m_scratch64 = DeviceBuffer<double>(n);
      float_type const* src = static_cast<float_type const*>(this->get_own_variable(step, variable));
      hip::column_major_to_z_order<float_type>(SubgridType::rank, m_host.num_local_elements, src, m_scratch.get());
      hip::host_scalar_variable<float_type>(n, m_scratch.get(), m_scratch64.get());
      T8GPU_CUDA_CHECK_ERROR(hipDeviceSynchronize());
    }

    void write(std::string const& prefix, int cells_per_dim, int nf, char const* const* names, int32_t const* comps,
               double const* const* data) const {
      const std::string path = prefix + ".vtu";
      const int rc = t8gpu_host_write_vtu(path.c_str(), SubgridType::rank, m_host.num_local_elements, m_host.centres.data(),
                                          m_host.levels.data(), cells_per_dim, m_host.mpirank, m_host.first_global_element, nf, names, comps,
                                          data, 0);
      if (rc != 0) {
        std::fprintf(stderr, "t8gpu: writing %s failed (code %d)\n", path.c_str(), rc);
        std::abort();
      }
    }
  };

  /// earlier name of the class when it is built from the synthetic provider or from host arrays
  template<typename VariableType, typename StepType, typename SubgridType>
  using SyntheticSubgridMeshManager = SubgridMeshManager<VariableType, StepType, SubgridType>;

}  // namespace t8gpu

#endif  // T8GPU_HIP_MESH_SUBGRID_MESH_MANAGER_H
