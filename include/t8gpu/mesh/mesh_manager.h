// t8gpu/mesh/mesh_manager.h (MI355X backend)
//
// MeshConnectivityAccessor<float_type, dim>: the device-side view of the face lists, with the getters
// of the reference (t8gpu/mesh/mesh_manager.h:30-182) over the same arrays:
//   ranks[N+G], indices[N+G], face_neighbors[2F + B], face_normals[dim * (F + B)], face_surfaces[F + B].
// MeshManager<V, S, dim>: the class of the reference (t8gpu/mesh/mesh_manager.h:232-465) with the same public
// members -- constructor (comm, scheme, cmesh, forest), initialize_variables(Func), adapt(criteria, step),
// partition(step), compute_connectivity_information(), save_variable(s)_to_vtk, HostVariableInfo,
// get_host_{scalar,vector}_variable, get_connectivity_information(), get_num_local_{elements,faces,
// boundary_faces}(), get_num_ghost_elements(), min_level / max_level -- on top of MemoryManager. Where the mesh
// comes from is a provider behind the class:
//   * a t8code forest: the (comm, scheme, cmesh, forest) constructor. It is DECLARED here and defined only in a
//     build that has t8code (it fills a T8gpuForestQuery from t8code calls); this image
//     has no t8code, so example TUs compile against it and link once that adapter is compiled in.
//   * the t8code-free synthetic forest of include/t8gpu_host.h, or plain host arrays (HostMeshArrays): the two
//     extra constructors below. `SyntheticMeshManager<V,S,dim>` is an alias of MeshManager kept for code written
//     against the earlier name.
// The forest, its adaptation and repartition, the ghost layer and the device connectivity arrays are a ForestCore
// (forest_core.h) held as a member: SubgridMeshManager holds the same one with blocks for elements.
// Read-back / VTK members (mesh_manager.inl:516-623): device half in csrc/hip/kernels_readback.hip, the file is
// written by t8gpu_host_write_vtu where the reference calls t8_forest_write_vtk_ext.
#ifndef T8GPU_HIP_MESH_MESH_MANAGER_H
#define T8GPU_HIP_MESH_MESH_MANAGER_H

#include <t8gpu/memory/memory_manager.h>
#include <t8gpu/mesh/forest_core.h>

#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include <thrust/host_vector.h>

#if __has_include(<t8.h>)
#include <t8.h>
#else
// no t8code on the include path: the handle types of the constructor's signature, opaque
using t8_locidx_t = int32_t;
typedef struct t8_forest* t8_forest_t;
typedef struct t8_cmesh*  t8_cmesh_t;
struct t8_scheme_cxx;
typedef struct t8_scheme_cxx t8_scheme_cxx_t;
struct t8_element;
typedef struct t8_element t8_element_t;
#endif

namespace t8gpu {

  template<typename float_type, size_t dim>
  class MeshConnectivityAccessor {
    template<typename VT, typename ST, size_t dim_>
    friend class MeshManager;

   public:
    MeshConnectivityAccessor(MeshConnectivityAccessor const&)            = default;
    MeshConnectivityAccessor& operator=(MeshConnectivityAccessor const&) = default;

    [[nodiscard]] __host__ __device__ inline t8_locidx_t get_num_local_faces() const { return m_num_local_faces; }
    [[nodiscard]] __host__ __device__ inline t8_locidx_t get_num_local_boundary_faces() const { return m_num_local_boundary_faces; }

    [[nodiscard]] __device__ inline float_type get_face_surface(int f) const { return m_face_surfaces[f]; }
    [[nodiscard]] __device__ inline float_type get_boundary_face_surface(int f) const { return m_face_surfaces[m_num_local_faces + f]; }

    [[nodiscard]] __device__ inline std::array<float_type, dim> get_face_normal(int f) const { return normal_at(f); }
    [[nodiscard]] __device__ inline std::array<float_type, dim> get_boundary_face_normal(int f) const { return normal_at(m_num_local_faces + f); }

    /// (left, right) LOCAL element indices; >= num_local_elements means a ghost (mirror slot)
    [[nodiscard]] __device__ inline std::array<t8_locidx_t, 2> get_face_neighbor_indices(int f) const {
      return {m_face_neighbors[2 * f], m_face_neighbors[2 * f + 1]};
    }
    [[nodiscard]] __device__ inline t8_locidx_t get_boundary_face_neighbor_index(int f) const {
      return m_face_neighbors[2 * m_num_local_faces + f];
    }
    /// owner rank / slot of a local element index. In this backend every element (ghosts included)
    /// resolves to a slot of THIS rank's planes, so `var[rank][index]` never leaves the device.
    [[nodiscard]] __device__ inline t8_locidx_t get_element_owner_rank(int e) const { return m_ranks[e]; }
    [[nodiscard]] __device__ inline t8_locidx_t get_element_owner_remote_index(int e) const { return m_indices[e]; }

    // raw arrays, for the C-ABI (t8gpu_hip_flux_faces_* takes exactly these)
    [[nodiscard]] __host__ __device__ t8_locidx_t const* face_neighbors() const { return m_face_neighbors; }
    [[nodiscard]] __host__ __device__ t8_locidx_t const* indices() const { return m_indices; }
    [[nodiscard]] __host__ __device__ float_type const*  face_normals() const { return m_face_normals; }
    [[nodiscard]] __host__ __device__ float_type const*  face_surfaces() const { return m_face_surfaces; }

   private:
    int const*         m_ranks;
    t8_locidx_t const* m_indices;
    t8_locidx_t const* m_face_neighbors;
    float_type const*  m_face_normals;
    float_type const*  m_face_surfaces;
    t8_locidx_t        m_num_local_faces;
    t8_locidx_t        m_num_local_boundary_faces;

    __device__ inline std::array<float_type, dim> normal_at(int slot) const {
      std::array<float_type, dim> n{};
      for (size_t k = 0; k < dim; k++) n[k] = m_face_normals[dim * slot + k];
      return n;
    }
    MeshConnectivityAccessor(int const* ranks, t8_locidx_t const* indices, t8_locidx_t const* fn, float_type const* normals,
                             float_type const* surfaces, t8_locidx_t F, t8_locidx_t B)
        : m_ranks{ranks}, m_indices{indices}, m_face_neighbors{fn}, m_face_normals{normals}, m_face_surfaces{surfaces},
          m_num_local_faces{F}, m_num_local_boundary_faces{B} {}
  };

  /// Host description of one rank's mesh in the reference's array formats (doubles are converted to
  /// float_type the way the reference casts t8code's doubles, mesh_manager.inl:400-407).
  struct HostMeshArrays {
    int32_t num_local_elements = 0, num_ghost_elements = 0, num_local_faces = 0, num_local_boundary_faces = 0;
    int     rank = 0;
    std::vector<int32_t> face_neighbors;  // [2F + B]
    std::vector<double>  face_normals;    // [dim * (F + B)]
    std::vector<double>  face_surfaces;   // [F + B]
    std::vector<double>  volumes;         // [N + G]
    // only needed by save_variables_to_vtk: geometry of the owned leaves on the unit domain
    int                  mesh_dim = 2;
    int64_t              first_global_element = 0;
    std::vector<double>  centres;         // [N][3]
    std::vector<int32_t> levels;          // [N]
  };

  /// What initialize_variables hands to the user function as `t8_element_t const*` when the forest is the synthetic
  /// provider's (there is no t8code element behind it): centre, level and volume of the leaf on the unit domain.
  /// `t8gpu::synthetic_element(element)` turns the opaque pointer back into this record.
  struct SyntheticElement {
    double  centre[3];
    int32_t level;
    double  volume;
  };
  [[nodiscard]] inline SyntheticElement const& synthetic_element(t8_element_t const* element) {
    return *reinterpret_cast<SyntheticElement const*>(element);
  }

  template<typename VariableType, typename StepType, size_t dim>
  class MeshManager : public MemoryManager<VariableType, StepType> {
   public:
    using float_type                  = typename variable_traits<VariableType>::float_type;
    using variable_index_type         = typename variable_traits<VariableType>::index_type;
    static constexpr int nb_variables = variable_traits<VariableType>::nb_variables;

    using step_index_type            = typename step_traits<StepType>::index_type;
    static constexpr size_t nb_steps = step_traits<StepType>::nb_steps;

    static constexpr t8_locidx_t min_level = 1;   // mesh_manager.h:240-241 (adapt() of a t8code forest uses them)
    static constexpr t8_locidx_t max_level = 4;

    /// mesh_manager.h:253 / mesh_manager.inl:20-64: takes ownership of cmesh and forest. Declared for every build;
    /// DEFINED by the t8code adapter only (fills a T8gpuForestQuery from t8_forest_leaf_face_neighbors & co.,
    /// INTEGRATION.md section 4) -- a build without t8code cannot call it and gets a link error if it tries.
    MeshManager(sc_MPI_Comm comm, t8_scheme_cxx_t* scheme, t8_cmesh_t cmesh, t8_forest_t forest);

    /// From host arrays in the reference's formats (one rank's share; ghosts resolved to mirror slots).
    explicit MeshManager(HostMeshArrays const& m, sc_MPI_Comm comm = sc_MPI_COMM_WORLD)
        : MemoryManager<VariableType, StepType>(static_cast<size_t>(m.num_local_elements) + m.num_ghost_elements, comm),
          m_core{"MeshManager", 1, min_level, max_level, comm} {
      rebuild_connectivity(m);
      this->set_volume(std::vector<float_type>(m.volumes.begin(), m.volumes.end()));
    }
    /// From a synthetic forest (t8gpu_synth_mesh_create; the manager takes ownership): stands for
    /// MeshManager(comm, scheme, cmesh, forest) (mesh_manager.inl:3-44). The connectivity comes through the
    /// forest-query adapter (csrc/host/connectivity.cpp), i.e. the way a t8code build would provide it.
    /// `lowest_level` / `highest_level` bound adapt() (the class constants min_level / max_level by default).
    /// On several ranks (comm.size > 1) every rank passes ITS OWN handle of the same forest (the description is replicated,
    /// as in t8gpu_amd/amr.py) and owns the contiguous share [n r / size, n (r + 1) / size) of the space-filling curve;
    /// set_transport() must follow before adapt() / partition() / refresh_ghost_layer() are called.
    explicit MeshManager(void* synth_mesh, int lowest_level = min_level, int highest_level = max_level,
                         sc_MPI_Comm comm = sc_MPI_COMM_WORLD)
        : MeshManager(arrays_of(synth_mesh, Core::rank_of(comm), Core::size_of(comm), nullptr), comm) {
      m_core.forest.reset(synth_mesh);
      m_core.min_level = lowest_level;
      m_core.max_level = highest_level;
      if (m_core.nb_ranks > 1) rebuild_connectivity(arrays_of(synth_mesh, m_core.rank, m_core.nb_ranks, &m_core.halo));   // (+ the halo lists)
    }
    /// The channel adapt() / partition() / refresh_ghost_layer() use on several ranks (not owned). See backend/transport.h.
    void set_transport(Transport* transport) { m_core.transport = transport; }

    /// mesh_manager.inl:76-122: `func(accessor, forest, tree_idx, element, e_idx)` fills the variables of element
    /// e_idx in a HOST accessor; all 26 planes are zeroed, Step 0 and the volume uploaded. With the synthetic provider
    /// `forest` is its handle, tree_idx 0 and `element` a SyntheticElement (see synthetic_element()).
    template<typename Func>
    void initialize_variables(Func func) {
      const size_t n = static_cast<size_t>(m_host.num_local_elements), tot = n + static_cast<size_t>(m_host.num_ghost_elements);
      std::array<std::vector<float_type>, nb_variables> host_variables{};
      std::array<float_type*, nb_variables>             array{};
      for (size_t k = 0; k < static_cast<size_t>(nb_variables); k++) {
        host_variables[k].resize(n);
        array[k] = host_variables[k].data();
      }
      MemoryAccessorOwn<VariableType> host_variable_memory{array};
      std::vector<float_type>         element_volume(tot, float_type(1));
      for (size_t e = 0; e < n; e++) {
        SyntheticElement el{{m_host.centres[3 * e], m_host.centres[3 * e + 1], m_host.centres[3 * e + 2]}, m_host.levels[e], m_host.volumes[e]};
        element_volume[e] = static_cast<float_type>(el.volume);
        func(host_variable_memory, reinterpret_cast<t8_forest_t>(m_core.forest.get()), t8_locidx_t{0},
             reinterpret_cast<t8_element_t const*>(&el), static_cast<t8_locidx_t>(e));
      }
      for (size_t g = n; g < tot; g++) element_volume[g] = static_cast<float_type>(m_host.volumes[g]);
      // every plane of every step zeroed one by one (the reference memsets 26*N values from plane 0, valid only while
      // capacity == size: SURVEY quirk Q10)
      std::vector<float_type> zeros(tot, float_type(0));
      for (size_t st = 0; st < nb_steps; st++)
        for (size_t k = 0; k < static_cast<size_t>(nb_variables); k++)
          this->set_variable(static_cast<step_index_type>(st), static_cast<variable_index_type>(k), zeros);
      for (size_t k = 0; k < static_cast<size_t>(nb_variables); k++) {
        host_variables[k].resize(tot, float_type(0));
        this->set_variable(static_cast<step_index_type>(0), static_cast<variable_index_type>(k), host_variables[k]);
      }
      this->set_volume(element_volume);
    }

    /// mesh_manager.h:297 (the reference's signature); criteria above 10 refine, families below it coarsen
    void adapt(thrust::host_vector<float_type> const& refinement_criteria, step_index_type step) {
      adapt(std::vector<float_type>(refinement_criteria.begin(), refinement_criteria.end()), step);
    }

    /// mesh_manager.inl:626-723. After adapt() the elements a rank holds are no longer its equal share of the curve;
    /// partition() ships every run of adapted elements to its owner in the new equal split (ForestCore::partition),
    /// installs the new forest and rebuilds the connectivity. Only `step` and the volume are valid afterwards, as in the
    /// reference. On one rank, or when no adapt() is pending, it is the identity (t8_forest_partition moves nothing).
    void partition(step_index_type step) {
      if (!m_core.partition_pending()) return;
      // the new share's connectivity first: it says how many ghost slots the planes need
      HostHaloArrays halo;
      HostMeshArrays m = arrays_of(m_core.pending.forest.get(), m_core.rank, m_core.nb_ranks, &halo);
      this->resize(static_cast<size_t>(m.num_local_elements) + m.num_ghost_elements);
      m_core.partition(m, std::move(halo), hip::to_vars(this->get_own_variables(step)), this->get_own_volume());
      rebuild_connectivity(m);
    }

    /// Refresh the ghost mirror slots [N, N + G) of the five planes of `step` from their owners (several ranks only; a
    /// no-op on one). The reference needs no such call: a ghost is read through the owner's CUDA-IPC pointer
    /// (kernels.cu:164-168). Kernels that read ghost values outside iterate() -- estimate_gradient of the adapt criterion,
    /// solver.cu:245-263 -- call it first; the step drivers refresh what they read themselves.
    void refresh_ghost_layer(step_index_type step) { m_core.refresh_ghost_layer(hip::to_vars(this->get_own_variables(step))); }
    [[nodiscard]] HostHaloArrays const& host_halo() const { return m_core.halo; }
    [[nodiscard]] int comm_rank() const { return m_core.rank; }
    [[nodiscard]] int comm_size() const { return m_core.nb_ranks; }

    /// mesh_manager.inl:333-481: face lists, normals, areas, ghost slots of the current forest -> device arrays.
    /// adapt() already leaves them current; calling this again is harmless (the reference requires the call).
    void compute_connectivity_information() {
      if (m_core.forest)
        rebuild_connectivity(arrays_of(m_core.forest.get(), m_core.rank, m_core.nb_ranks, m_core.nb_ranks > 1 ? &m_core.halo : nullptr));
    }

    /// MeshManager::adapt (mesh_manager.inl:196-330): the reference's adapt callback on the criteria (refine above
    /// `threshold`, coarsen a family whose first four members are below it; :125-162), 2:1 balance, the data-transfer
    /// kernel adapt_variables_and_volume (:165-193) from `step` into temporary planes (ForestCore::adapt). On one rank
    /// they are copied into the (possibly re-allocated) manager and the connectivity is rebuilt; on several ranks the
    /// adapted elements wait on their old owners for partition(). Only `step` and the volume are valid afterwards, as
    /// in the reference.
    void adapt(std::vector<float_type> const& refinement_criteria, step_index_type step, double threshold = 10.0) {
      m_core.adapt(refinement_criteria, threshold, [&](int32_t n, int32_t const* adapt_data, typename Core::vars new_variables, float_type* new_volume) {
        hip::adapt_variables_and_volume<float_type>(n, m_host.mesh_dim, adapt_data, hip::to_vars(this->get_own_variables(step)), new_variables,
                                                    this->get_own_volume(), new_volume);
      });
      if (m_core.nb_ranks > 1) return;
      this->resize(static_cast<size_t>(m_core.pending_count()));
      m_core.install_pending(hip::to_vars(this->get_own_variables(step)), this->get_own_volume());
      rebuild_connectivity(arrays_of(m_core.forest.get(), 0, 1, nullptr));
    }

    [[nodiscard]] void const* forest() const { return m_core.forest.get(); }
    [[nodiscard]] HostMeshArrays const& host_arrays() const { return m_host; }

    MeshManager(MeshManager const&)            = delete;
    MeshManager& operator=(MeshManager const&) = delete;

    [[nodiscard]] MeshConnectivityAccessor<float_type, dim> get_connectivity_information() const {
      return {m_core.ranks.get(), m_core.indices.get(), m_core.face_neighbors.get(), m_core.face_normals.get(), m_core.face_surfaces.get(),
              m_host.num_local_faces, m_host.num_local_boundary_faces};
    }
    [[nodiscard]] t8_locidx_t get_num_local_elements() const { return m_host.num_local_elements; }
    [[nodiscard]] t8_locidx_t get_num_ghost_elements() const { return m_host.num_ghost_elements; }
    [[nodiscard]] t8_locidx_t get_num_local_faces() const { return m_host.num_local_faces; }
    [[nodiscard]] t8_locidx_t get_num_local_boundary_faces() const { return m_host.num_local_boundary_faces; }

    /// Named host array of doubles ready for the writer (mesh_manager.h: HostVariableInfo).
    using HostVariableInfo = t8gpu::HostVariableInfo;

    /// mesh_manager.h:326: one variable in one file
    void save_variable_to_vtk(step_index_type step, variable_index_type variable, std::string const& prefix) const {
      std::vector<HostVariableInfo> v;
      v.push_back(get_host_scalar_variable(step, variable, "variable"));
      save_variables_to_vtk(std::move(v), prefix);
    }

    /// mesh_manager.inl:516-545: one variable of one step, cast to double (on the device), on the host.
    [[nodiscard]] HostVariableInfo get_host_scalar_variable(step_index_type step, variable_index_type variable,
                                                            std::string const& name) const {
      const size_t n = static_cast<size_t>(m_host.num_local_elements);
      double*      d = staging(n);
      hip::host_scalar_variable(n, this->get_own_variable(step, variable), d);
      return {T8GPU_VTK_SCALAR, fetch(d, n), name};
    }
    /// mesh_manager.inl:547-586: three variables as interleaved xyz doubles.
    [[nodiscard]] HostVariableInfo get_host_vector_variable(step_index_type step, std::array<variable_index_type, 3> variables,
                                                            std::string const& name) const {
      const size_t      n = static_cast<size_t>(m_host.num_local_elements);
      double*           d = staging(3 * n);
      float_type const* v[3];
      for (int k = 0; k < 3; k++) v[k] = this->get_own_variable(step, variables[k]);
      hip::host_vector_variable(n, v[0], v[1], v[2], d);
      return {T8GPU_VTK_VECTOR, fetch(d, 3 * n), name};
    }
    /// mesh_manager.inl:588-623: this rank's piece `<prefix>.vtu` (`<prefix>_RRRR.vtu` in a multi-rank run).
    void save_variables_to_vtk(std::vector<HostVariableInfo> host_variables, std::string const& prefix, int num_ranks = 1,
                               bool ascii = false) const {
      const VtkFields fields(host_variables);
      char            suffix[16] = "";
      if (num_ranks > 1) std::snprintf(suffix, sizeof suffix, "_%04d", m_host.rank);
      const std::string path = prefix + suffix + ".vtu";
      const int rc = t8gpu_host_write_vtu(path.c_str(), m_host.mesh_dim, m_host.num_local_elements, m_host.centres.data(), m_host.levels.data(), 1,
                                          m_host.rank, m_host.first_global_element, fields.size(), fields.names.data(), fields.comps.data(),
                                          fields.data.data(), ascii);
      if (rc != 0) {
        std::fprintf(stderr, "t8gpu: writing %s failed (code %d)\n", path.c_str(), rc);
        std::abort();
      }
    }

   private:
    using MemoryManager<VariableType, StepType>::resize;   // private here, as in the reference (mesh_manager.h:425)
    using Core = ForestCore<float_type>;

    Core                         m_core;   // forest, rank layout, transport, ghost lists, device connectivity (forest_core.h)
    HostMeshArrays               m_host;
    mutable DeviceBuffer<double> m_staging;
    mutable size_t               m_staging_count = 0;

    /// rank `rank` of `nranks`' share of the forest in the reference's array formats, through the forest-query adapter
    /// (csrc/host/connectivity.cpp) -- the way a t8code build would provide it; `halo` (nullable) receives the ghost lists.
    /// Plus the leaf geometry the VTK members need.
    static HostMeshArrays arrays_of(void* forest, int rank, int nranks, HostHaloArrays* halo) {
      T8gpuForestQuery* q = t8gpu_synth_query_create(forest, rank, nranks);
      void*             h = q ? t8gpu_host_connectivity_create(q) : nullptr;
      if (!h) {
        std::fprintf(stderr, "t8gpu: connectivity of the synthetic forest could not be built\n");
        std::abort();
      }
      HostMeshArrays m;
      read_host_connectivity(h, m, halo);
      m.rank = rank;
      t8gpu_host_connectivity_destroy(h);
      t8gpu_synth_query_destroy(q);
      static_assert(dim == 2 || dim == 3, "face normals have 2 or 3 components");
      keep_normal_components(m.face_normals, dim);   // the adapter hands out xyz; MeshConnectivityAccessor<ft, dim> strides by `dim`
      const size_t tot = static_cast<size_t>(m.num_local_elements) + m.num_ghost_elements;
      void*        part = t8gpu_synth_part_create(forest, rank, nranks, 0, 3);
      m.mesh_dim = t8gpu_synth_mesh_dim(forest);
      m.first_global_element = t8gpu_synth_mesh_num_elements(forest) * rank / nranks;
      m.levels.resize(tot);           // (the provider lists owned + ghost elements; the manager keeps the owned ones)
      m.centres.resize(3 * tot);
      t8gpu_synth_part_elements(part, m.levels.data(), nullptr, m.centres.data());
      m.levels.resize(m.num_local_elements);
      m.centres.resize(3 * static_cast<size_t>(m.num_local_elements));
      t8gpu_synth_part_destroy(part);
      return m;
    }
    /// compute_connectivity_information (mesh_manager.inl:333-481): device copies of the face arrays
    void rebuild_connectivity(HostMeshArrays const& m) {
      m_host = m;
      m_core.upload_connectivity(m, m.rank);
    }

    double* staging(size_t n) const {
      if (n > m_staging_count) {
        m_staging       = DeviceBuffer<double>(n);
        m_staging_count = n;
      }
      return m_staging.get();
    }
    static std::unique_ptr<double[]> fetch(double const* d, size_t n) {
      std::unique_ptr<double[]> h = std::make_unique<double[]>(n);
      T8GPU_CUDA_CHECK_ERROR(hipMemcpy(h.get(), d, sizeof(double) * n, hipMemcpyDeviceToHost));
      return h;
    }
  };

  /// earlier name of the class when it is built from the synthetic provider or from host arrays
  template<typename VariableType, typename StepType, size_t dim>
  using SyntheticMeshManager = MeshManager<VariableType, StepType, dim>;

}  // namespace t8gpu

#endif  // T8GPU_HIP_MESH_MESH_MANAGER_H
