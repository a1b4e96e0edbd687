// wavehip.hpp -- header-only C++17 wrappers over the C ABI (wavehip.h) that keep
// the reference's class names, constructor arguments and apply semantics, so
// that reference-side code (common/LinearGLL.hpp, the demo mains) can switch by
// changing an include.  Exceptions: the C ABI never throws; these wrappers
// re-throw std::runtime_error exactly where the reference does
// (common/cuda/array.hpp:15-17,33-35; mass.hpp:91-92; utils.hpp:30-34).
//
// The operator classes are templated on a Vector concept satisfied by
// dolfinx::la::Vector<T, Alloc> (x.array().data(), y.mutable_array().data());
// the vectors must live in device memory (hipMalloc; see wavehip::allocator).
// The function-space argument of the reference is replaced by a plain
// `wavehip::Space` aggregate; INTEGRATION.md shows how to fill it from a
// dolfinx::fem::FunctionSpace.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "wavehip.h"

namespace wavehip {

inline void check(int rc)
{
  if (rc != WF_OK) throw std::runtime_error(std::string("wavehip: ") + wf_last_error());
}

/// demo/cpu_planar3d/main.cpp:48-66: the time step CFL h / (c0 P^2) for the smallest cell diameter h (mesh::h,
/// wf_fs_min_cell_diameter), rounded down to a whole number of steps per source period: (time step, steps per period)
inline std::pair<double, int> cfl_time_step(std::int64_t nverts, const double* x, std::int64_t ncells, const std::int32_t* cells,
                                            int degree, double c0, double freq, double CFL)
{
  double h = 0.0;
  check(wf_fs_min_cell_diameter(nverts, x, ncells, cells, &h));
  const double dt = CFL * h / (c0 * degree * degree), period = 1.0 / freq;
  const int spp = (int)(period / dt + 1);
  return {period / spp, spp};
}

// ---- utils::set_device (common/cuda/utils.hpp:22-38) ----------------------
inline int set_device(int rank)
{
  check(wf_set_device(rank));
  return rank;
}

// ---- cuda::array<T> (common/cuda/array.hpp:8-51) ---------------------------
template <class T>
class array {
public:
  array() = default;
  explicit array(std::size_t size) : _size(size) { check(wf_malloc(reinterpret_cast<void**>(&_data), size * sizeof(T))); }
  array(const array&) = delete;
  array& operator=(const array&) = delete;
  array(array&& o) noexcept : _data(o._data), _size(o._size) { o._data = nullptr; o._size = 0; }
  ~array() { wf_free(_data); }
  std::size_t size() const { return _size; }
  const T* data() const { return _data; }
  T* data() { return _data; }
  template <class Container>
  void set(const Container& source)
  {
    if (source.size() != _size) throw std::runtime_error("wavehip::array::set: size mismatch");
    check(wf_memcpy_h2d(_data, source.data(), _size * sizeof(T)));
  }
  std::vector<T> copy_to_host() const
  {
    std::vector<T> h(_size);
    check(wf_memcpy_d2h(h.data(), _data, _size * sizeof(T)));
    return h;
  }

private:
  T* _data = nullptr;
  std::size_t _size = 0;
};

// ---- CUDA::allocator<T> (common/cuda/allocator.hpp:9-40) -------------------
// std-allocator over device memory for dolfinx::la::Vector<T, Alloc>.  The
// reference uses managed memory; MI355X-native code uses explicit device buffers,
// so host code must not dereference vectors allocated with it.
template <class T>
struct allocator {
  using value_type = T;
  allocator() = default;
  template <class U>
  allocator(const allocator<U>&) noexcept {}
  T* allocate(std::size_t n)
  {
    void* p = nullptr;
    check(wf_malloc(&p, n * sizeof(T)));
    return static_cast<T*>(p);
  }
  void deallocate(T* p, std::size_t) noexcept { wf_free(p); }
  template <class U>
  bool operator==(const allocator<U>&) const noexcept { return true; }
  template <class U>
  bool operator!=(const allocator<U>&) const noexcept { return false; }
};

// ---- free kernels (common/cuda/scatter.hpp:7-14, transform.hpp:7-8) --------
template <typename T>
void gather(std::int32_t N, const std::int32_t* indices, const T* in, T* out, int /*block_size*/ = 512, void* stream = nullptr)
{
  check(wf_gather(N, indices, in, out, stream));
}
template <typename T>
void scatter(std::int32_t N, const std::int32_t* indices, const T* in, T* out, int /*block_size*/ = 512, void* stream = nullptr)
{
  check(wf_scatter_add(N, indices, in, out, stream));
}
/// The plan of the order-fixed accumulation (WF_FLAG_ORDERED): stable counting sort of a flattened dofmap, host only.
inline void ordered_slots(std::int64_t ncells, int nd, std::int32_t ndofs, const std::int32_t* dofmap, std::int32_t* row_off,
                          std::int32_t* slot)
{
  check(wf_ordered_slots(ncells, nd, ndofs, dofmap, row_off, slot));
}
/// y[d] += vals[row_off[d]] + ... + vals[row_off[d+1]-1], summed front to back by one thread per row (no atomics).
inline void segment_sum_add(std::int32_t n, const std::int32_t* row_off, const double* vals, double* y, void* stream = nullptr)
{
  check(wf_segment_sum_add(n, row_off, vals, y, stream));
}
template <typename T>
void transform1(std::int32_t N, const T* in, const T* detJ, T* out, int /*block_size*/ = 512, void* stream = nullptr)
{
  check(wf_transform1(N, in, detJ, out, stream));
}

// What the operators need from a dolfinx::fem::FunctionSpace (host arrays).
struct Space {
  int degree = 0;
  std::int32_t ncells = 0;                  // mesh->topology().index_map(tdim)->size_local()
  std::int32_t ndofs = 0;                   // index_map->size_local() + num_ghosts()
  const std::int32_t* dofmap = nullptr;     // V->dofmap()->list().array().data(), [ncells][nd]
  const std::int32_t* perm = nullptr;       // element.get_tensor_product_representation()[0] perm, or nullptr
  int tensor_flags = 0;                     // WF_FLAG_TENSOR_X_SLOWEST when perm (or the dofmap, or handed-over
                                            // G / detJ) is in Basix' tensor order l' = (i n + j) n + k
  std::int32_t nverts = 0;
  const double* x = nullptr;                // mesh->geometry().x().data(), [nverts][3]
  const std::int32_t* geom_dofmap = nullptr;// mesh->geometry().dofmap().array().data(), [ncells][8]
};

namespace detail {
/// the descriptor of wf_op_create and wf_cell_form_create on the space V: sizes, dofmap, tensor frame and mesh
inline wf_op_desc hex_desc(const Space& V, int kind, int degree)
{
  wf_op_desc d{};
  d.kind = kind;
  d.degree = degree;
  d.ncells = V.ncells;
  d.ndofs = V.ndofs;
  d.h_dofmap = V.dofmap;
  d.h_perm = V.perm;
  d.flags = V.tensor_flags;
  d.nverts = V.nverts;
  d.h_xverts = V.x;
  d.h_geom_dofmap = V.geom_dofmap;
  return d;
}

class OpBase {
public:
  OpBase() = default;
  OpBase(const OpBase&) = delete;
  OpBase& operator=(const OpBase&) = delete;
  virtual ~OpBase() { wf_op_destroy(_op); }
  std::size_t num_quads() const { return info().num_quads; }
  std::size_t num_cells() const { return info().num_cells; }
  std::size_t num_dofs() const { return info().num_dofs_cell; }
  double flops() const { return info().flops; }
  /// whether the operator was created with a cell coefficient array (wf_op_info_t.cell_coeff)
  bool cell_coeff() const { return info().cell_coeff != 0; }

  /// y += A x   (common/operators.hpp:183, common/cuda/mass.hpp:76)
  template <typename Vector>
  void apply(const Vector& x, Vector& y, void* stream = nullptr)
  {
    check(wf_op_apply(_op, x.array().data(), y.mutable_array().data(), stream));
  }
  template <typename Vector>
  void operator()(const Vector& x, Vector& y) { apply(x, y); }
  void apply(const double* d_x, double* d_y, void* stream = nullptr) { check(wf_op_apply(_op, d_x, d_y, stream)); }
  wf_op* handle() const { return _op; }

protected:
  wf_op_info_t info() const
  {
    wf_op_info_t i{};
    check(wf_op_info(_op, &i));
    return i;
  }
  wf_op* _op = nullptr;
};
}  // namespace detail

/// Every operator wrapper takes an optional cell_coeff: one double per cell in the order of the dofmap's rows (on a box
/// cx + nx (cy + ny cz)), copied during construction; the operator is then sum_c a_c P_c^T A_c P_c (wavehip.h, "Cell
/// coefficients").  nullptr is the operator without one.  It is the last argument of every wrapper, behind tuning / flags.
///
/// StiffnessOperator(V, bdegree, params) -- common/operators.hpp:137-201.  tuning: the kernel selection of wf_tuning
/// (read during construction only), e.g. geometry = WF_GEOMETRY_PER_CELL for a mesh of affine cells at degrees 1 to 4.
template <typename T>
class StiffnessOperator : public detail::OpBase {
  static_assert(sizeof(T) == sizeof(double), "fp64 only");

public:
  StiffnessOperator(const Space& V, int bdegree, std::map<std::string, double>& params, const wf_tuning* tuning = nullptr,
                    const double* cell_coeff = nullptr)
  {
    wf_op_desc d = detail::hex_desc(V, WF_OP_STIFFNESS, bdegree);
    auto it = params.find("c0");
    d.c0 = it == params.end() ? 1500.0 : it->second;   // operators.hpp:114
    d.tuning = tuning;
    d.h_cell_coeff = cell_coeff;
    check(wf_op_create(&d, &_op));
  }
};

/// MassOperatorCPU(V, bdegree) -- common/operators.hpp:44-109 (the `MassOperator`
/// that common/LinearGLL.hpp:63,105 instantiates)
template <typename T>
class MassOperatorLumped : public detail::OpBase {
public:
  MassOperatorLumped(const Space& V, int bdegree, int flags = WF_FLAG_NONE, const double* cell_coeff = nullptr)
  {
    wf_op_desc d = detail::hex_desc(V, WF_OP_MASS_LUMPED, bdegree);
    d.flags |= flags;
    d.h_cell_coeff = cell_coeff;
    check(wf_op_create(&d, &_op));
  }
};

/// SpectralMassOperator(V, bdegree) -- common/cuda/spectral_mass.hpp:24-100
template <typename T>
class SpectralMassOperator : public MassOperatorLumped<T> {
public:
  SpectralMassOperator(const Space& V, int bdegree, const double* cell_coeff = nullptr)
      : MassOperatorLumped<T>(check_degree(V, bdegree), bdegree, WF_FLAG_NO_FABS, cell_coeff)
  {
  }

private:
  static const Space& check_degree(const Space& V, int bdegree)
  {
    if (bdegree < 2 || bdegree > 7) throw std::runtime_error("SpectralMassOperator: degree must be 2..7");
    return V;
  }
};

/// MassOperator(V, element, quad_type, qd) -- common/cuda/mass.hpp:18-107.
/// phi1: 1-D interpolation matrix [nq1][degree+1]; detJ: [ncells][nq1^3] (host).  tuning: the kernel selection of
/// wf_tuning (read during construction only), e.g. kernel = WF_KERNEL_FORCE_MASS_MARCH for a rectangular table.
template <typename T>
class MassOperator : public detail::OpBase {
public:
  MassOperator(const Space& V, int degree, int nq1, const double* phi1, const double* detJ, const wf_tuning* tuning = nullptr,
               const double* cell_coeff = nullptr)
  {
    wf_op_desc d = detail::hex_desc(V, WF_OP_MASS_DENSE, degree);
    d.nq1 = nq1;
    d.h_phi1 = phi1;
    d.h_detJ = detJ;
    d.tuning = tuning;
    d.h_cell_coeff = cell_coeff;
    check(wf_op_create(&d, &_op));
  }
  /// The reference's argument list (mass.hpp:20-21): element = degree + Lagrange variant
  /// (WF_VARIANT_GLL_WARPED / WF_VARIANT_EQUISPACED), quad_type (WF_QUAD_GLL /
  /// WF_QUAD_GAUSS_JACOBI) and quadrature degree qd.  Builds the 1-D table (tabulate_1d,
  /// precompute.hpp:179-189) on the host and det J * w at the rule's points on the device.
  MassOperator(const Space& V, int degree, int variant, int quad_type, int qd, const wf_tuning* tuning = nullptr,
               const double* cell_coeff = nullptr)
  {
    int nq1 = 0;
    double pts[WF_MAX_QUAD_POINTS], wts[WF_MAX_QUAD_POINTS];
    check(wf_quadrature_1d(quad_type, qd, &nq1, pts, wts));
    std::vector<double> phi1((std::size_t)nq1 * (degree + 1));
    check(wf_tabulate_1d(degree, variant, nq1, pts, 0, phi1.data()));
    wf_op_desc d = detail::hex_desc(V, WF_OP_MASS_DENSE, degree);
    d.nq1 = nq1;
    d.h_phi1 = phi1.data();
    d.h_qpts1 = pts;
    d.h_qwts1 = wts;
    d.flags |= WF_FLAG_NO_FABS;   // mass.hpp:35-39: det J * w keeps its sign (compute_jacobian_determinant)
    d.tuning = tuning;
    d.h_cell_coeff = cell_coeff;
    check(wf_op_create(&d, &_op));
  }
};

/// Structured box operators (mesh::create_box with this engine's numbering).
template <typename T>
class BoxStiffnessOperator : public detail::OpBase {
public:
  BoxStiffnessOperator(int degree, int nx, int ny, int nz, const double* xverts, double c0, const wf_tuning* tuning = nullptr,
                       const double* cell_coeff = nullptr)
  {
    check(wf_op_create_box_coeff(WF_OP_STIFFNESS, degree, nx, ny, nz, xverts, c0, cell_coeff, WF_FLAG_NONE, tuning, &_op));
  }
};
/// The lumped mass on the same box: the pre-assembled diagonal.
template <typename T>
class BoxMassOperatorLumped : public detail::OpBase {
public:
  BoxMassOperatorLumped(int degree, int nx, int ny, int nz, const double* xverts, int flags = WF_FLAG_NONE,
                        const double* cell_coeff = nullptr)
  {
    check(wf_op_create_box_coeff(WF_OP_MASS_LUMPED, degree, nx, ny, nz, xverts, 0.0, cell_coeff, flags, nullptr, &_op));
  }
};

/// Cell form of an operator: e_c(lambda, u) = (P_c lambda)^T A_c (P_c u), one number per cell in the order of the
/// dofmap's rows (wavehip.h, "cell forms").  kind: WF_OP_STIFFNESS (params["c0"], default 1500) or WF_OP_MASS_LUMPED.
/// tuning may set geometry only.  The box constructor is the form on mesh::create_box with this engine's numbering.
/// eval holds no scratch state: evaluations of one form may be in flight on different streams.
template <typename T>
class CellForm {
  static_assert(sizeof(T) == sizeof(double), "fp64 only");

public:
  CellForm(const Space& V, int degree, int kind, std::map<std::string, double>& params, const wf_tuning* tuning = nullptr,
           const double* cell_coeff = nullptr, int flags = WF_FLAG_NONE)
  {
    wf_op_desc d = detail::hex_desc(V, kind, degree);
    d.flags |= flags;
    auto it = params.find("c0");
    d.c0 = it == params.end() ? 1500.0 : it->second;
    d.tuning = tuning;
    d.h_cell_coeff = cell_coeff;
    check(wf_cell_form_create(&d, &_f));
  }
  CellForm(int kind, int degree, int nx, int ny, int nz, const double* xverts, double c0, const wf_tuning* tuning = nullptr,
           const double* cell_coeff = nullptr, int flags = WF_FLAG_NONE)
  {
    check(wf_cell_form_create_box(kind, degree, nx, ny, nz, xverts, c0, cell_coeff, flags, tuning, &_f));
  }
  CellForm(const CellForm&) = delete;
  CellForm& operator=(const CellForm&) = delete;
  ~CellForm() { wf_cell_form_destroy(_f); }

  /// out[c] = (accumulate ? out[c] : 0) + alpha e_c(lambda, u); lambda may be u
  void eval(const double* d_lambda, const double* d_u, double* d_out, double alpha = 1.0, bool accumulate = false,
            void* stream = nullptr) const
  {
    check(wf_cell_form_eval(_f, d_lambda, d_u, alpha, accumulate ? 1 : 0, d_out, stream));
  }
  wf_cell_form_info_t info() const
  {
    wf_cell_form_info_t i{};
    check(wf_cell_form_info(_f, &i));
    return i;
  }
  std::size_t num_cells() const { return info().num_cells; }
  int geometry() const { return info().geometry; }
  bool cell_coeff() const { return info().cell_coeff != 0; }
  wf_cell_form* handle() const { return _f; }

private:
  wf_cell_form* _f = nullptr;
};

// ---- communicator + VectorUpdater (demo/gpu_scatter_mpi/VectorUpdater.hpp) ----
/// RCCL communicator behind the C ABI.  The reference's launcher is mpirun; a
/// launcher that exports RANK / WORLD_SIZE / LOCAL_RANK (torchrun --no-python,
/// a shell loop, SLURM) works with from_env(), which meets through a file.
class Comm {
public:
  Comm(const char* id, int rank, int nranks) { check(wf_comm_create(id, rank, nranks, &_c)); }
  Comm(const std::string& rendezvous_file, int rank, int nranks, double timeout_s = 120.0)
  {
    check(wf_comm_create_from_file(rendezvous_file.c_str(), rank, nranks, timeout_s, &_c));
  }
  Comm(const Comm&) = delete;
  Comm& operator=(const Comm&) = delete;
  ~Comm() { wf_comm_destroy(_c); }

  static int env_int(const char* name, int dflt)
  {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
  }
  /// One rank per process: device LOCAL_RANK, rendezvous file $WF_COMM_FILE or
  /// /tmp/wavehip_comm_$MASTER_PORT.  Calls set_device.
  static std::unique_ptr<Comm> from_env()
  {
    const int rank = env_int("RANK", 0), size = env_int("WORLD_SIZE", 1);
    set_device(env_int("LOCAL_RANK", rank));
    const char* f = std::getenv("WF_COMM_FILE");
    std::string path = f ? f : std::string("/tmp/wavehip_comm_") + std::to_string(env_int("MASTER_PORT", 29500));
    return std::make_unique<Comm>(path, rank, size);
  }
  int rank() const
  {
    int r = 0;
    check(wf_comm_info(_c, &r, nullptr, nullptr));
    return r;
  }
  int size() const
  {
    int n = 1;
    check(wf_comm_info(_c, nullptr, &n, nullptr));
    return n;
  }
  /// MPI_Allreduce on device data (demo/gpu_cg/CUDA/cg.hpp:21)
  void allreduce(const double* d_in, double* d_out, std::int64_t count, int op = WF_SUM, void* stream = nullptr)
  {
    check(wf_comm_allreduce(_c, op, count, d_in, d_out, stream));
  }
  void barrier(void* stream = nullptr) { check(wf_comm_barrier(_c, stream)); }
  wf_comm* handle() const { return _c; }

private:
  wf_comm* _c = nullptr;
};

/// The IndexMap data the reference's VectorUpdater constructor extracts
/// (VectorUpdater.hpp:31-98): neighbours, displacements, scatter_fwd_indices and
/// ghost positions.  A DOLFINx caller fills it from
/// index_map->scatter_fwd_indices() / scatter_fwd_ghost_positions().
struct GhostLists {
  std::int32_t ndofs = 0;                       // size_local + num_ghosts
  std::vector<int> send_neighbors, recv_neighbors;
  std::vector<std::int32_t> send_offsets{0}, recv_offsets{0};
  std::vector<std::int32_t> send_indices;       // owned local dofs, per send neighbour
  std::vector<std::int32_t> ghost_positions;    // local positions of the ghosts, per recv neighbour
  bool empty() const { return send_neighbors.empty() && recv_neighbors.empty(); }
};

/// VectorUpdater<T, AllocatorT> -- demo/gpu_scatter_mpi/VectorUpdater.hpp:21-230.
/// Same method names; vectors are anything with array()/mutable_array() or raw
/// device pointers.  All calls are stream-ordered (no host synchronisation).
template <typename T>
class VectorUpdater {
  static_assert(sizeof(T) == sizeof(double), "fp64 only");

public:
  VectorUpdater(Comm* comm, const GhostLists& g, int flags = WF_UPDATER_DEFAULT)
  {
    wf_updater_desc d{};
    d.ndofs = g.ndofs;
    d.num_send_neighbors = (int)g.send_neighbors.size();
    d.send_neighbors = g.send_neighbors.data();
    d.send_offsets = g.send_offsets.data();
    d.send_indices = g.send_indices.data();
    d.num_recv_neighbors = (int)g.recv_neighbors.size();
    d.recv_neighbors = g.recv_neighbors.data();
    d.recv_offsets = g.recv_offsets.data();
    d.ghost_positions = g.ghost_positions.data();
    d.flags = flags;
    check(wf_updater_create(comm ? comm->handle() : nullptr, &d, &_u));
  }
  VectorUpdater(const VectorUpdater&) = delete;
  VectorUpdater& operator=(const VectorUpdater&) = delete;
  ~VectorUpdater() { wf_updater_destroy(_u); }

  void update_fwd_begin(const T* x, void* stream = nullptr) { check(wf_updater_fwd_begin(_u, x, stream)); }
  void update_fwd_begin(T* x, void* stream = nullptr) { update_fwd_begin(static_cast<const T*>(x), stream); }
  void update_rev_begin(T* x, void* stream = nullptr) { update_rev_begin(static_cast<const T*>(x), stream); }
  void update_fwd_end(T* x, void* stream = nullptr) { check(wf_updater_fwd_end(_u, x, stream)); }
  void update_fwd(T* x, void* stream = nullptr) { check(wf_updater_fwd(_u, x, stream)); }
  void update_rev_begin(const T* x, void* stream = nullptr) { check(wf_updater_rev_begin(_u, x, stream)); }
  void update_rev_end(T* x, void* stream = nullptr) { check(wf_updater_rev_end(_u, x, stream)); }
  void update_rev(T* x, void* stream = nullptr) { check(wf_updater_rev(_u, x, stream)); }
  template <typename Vector>
  void update_fwd_begin(const Vector& x) { update_fwd_begin(static_cast<const T*>(x.array().data())); }
  template <typename Vector>
  void update_fwd_end(Vector& x) { update_fwd_end(static_cast<T*>(x.mutable_array().data())); }
  template <typename Vector>
  void update_fwd(Vector& x) { update_fwd(static_cast<T*>(x.mutable_array().data())); }
  template <typename Vector>
  void update_rev_begin(const Vector& x) { update_rev_begin(static_cast<const T*>(x.array().data())); }
  template <typename Vector>
  void update_rev_end(Vector& x) { update_rev_end(static_cast<T*>(x.mutable_array().data())); }
  template <typename Vector>
  void update_rev(Vector& x) { update_rev(static_cast<T*>(x.mutable_array().data())); }
  wf_updater* handle() const { return _u; }

private:
  wf_updater* _u = nullptr;
};

// ---- device::cg (demo/gpu_cg/CUDA/cg.hpp:38-121) -------------------------------
namespace device {
/// Solve A x = b with the conjugate gradient method; returns the iteration count.
/// matvec(p, y) must ACCUMULATE y += A p on raw device pointers (cg zeroes y first),
/// e.g. [&](const double* p, double* y, void* s) { op.apply(p, y, s); }.  x holds the
/// initial guess.  On a partitioned mesh pass the VectorUpdater and its Comm.
/// Textbook CG with the reference's stopping rule (cg.hpp:103); see wf_cg.
template <typename T>
int cg(T* x, const T* b, std::int64_t n, std::function<void(const T*, T*, void*)> matvec, int kmax = 50,
       double rtol = 1e-8, VectorUpdater<T>* updater = nullptr, Comm* comm = nullptr, double* rel_residual = nullptr)
{
  static_assert(sizeof(T) == sizeof(double), "fp64 only");
  struct Ctx {
    std::function<void(const T*, T*, void*)>* f;
    std::string what;
  } ctx{&matvec, {}};
  wf_cg_desc d{};
  d.n = n;
  d.user = &ctx;
  d.matvec = [](void* user, const double* v, double* y, void* stream) -> int {
    auto* c = static_cast<Ctx*>(user);
    try {
      (*c->f)(v, y, stream);
      return 0;
    } catch (const std::exception& e) {   // exceptions must not cross the C boundary
      c->what = e.what();
      return -1;
    }
  };
  d.updater = updater ? updater->handle() : nullptr;
  d.comm = comm ? comm->handle() : nullptr;
  d.kmax = kmax;
  d.rtol = rtol;
  int its = 0;
  const int rc = wf_cg(&d, x, b, &its, rel_residual, nullptr);
  if (rc != WF_OK && !ctx.what.empty()) throw std::runtime_error("wavehip::device::cg: matvec threw: " + ctx.what);
  check(rc);
  return its;
}
/// Vector-concept overload with the reference's argument order.
template <typename Vector>
int cg(Vector& x, const Vector& b, std::function<void(const double*, double*, void*)> matvec, int kmax = 50,
       double rtol = 1e-8)
{
  return cg<double>(x.mutable_array().data(), b.array().data(), (std::int64_t)x.array().size(), std::move(matvec), kmax, rtol);
}
}  // namespace device

// ---- linalg:: (common/cuda/la.hpp:31-138) and kernels:: (LinearGLL.hpp:15-35)
namespace linalg {
template <typename Vector>
void copy(const Vector& x, Vector& y, void* stream = nullptr)
{
  check(wf_copy((std::int64_t)x.array().size(), x.array().data(), y.mutable_array().data(), stream));
}
template <typename Scalar, typename Vector>
void axpy(Scalar alpha, const Vector& x, Vector& y, void* stream = nullptr)   // y = alpha x + y over size_local
{
  check(wf_axpy((std::int64_t)x.map()->size_local(), (double)alpha, x.array().data(), y.array().data(),
                y.mutable_array().data(), stream));
}
template <typename Scalar, typename Vector>
void scale(Scalar alpha, Vector& x, void* stream = nullptr)
{
  check(wf_scale((std::int64_t)x.map()->size_local(), (double)alpha, x.mutable_array().data(), stream));
}
}  // namespace linalg

/// p += lam * ((up - 2 u) + um) over n entries, evaluated as written (wf_leapfrog_correlate): the per-step term of the
/// lumped-mass sensitivity of the leapfrog loop's discrete adjoint.  p must not overlap an input.
inline void leapfrog_correlate(std::int64_t n, const double* d_lam, const double* d_up, const double* d_u, const double* d_um,
                               double* d_p, void* stream = nullptr)
{
  check(wf_leapfrog_correlate(n, d_lam, d_up, d_u, d_um, d_p, stream));
}

/// p = (p + lam * ((up - 2 u) + um)) + 12 (om * w) and, with d_z, z = u + w over n entries, evaluated as written
/// (wf_leapfrog4_correlate): the per-step terms of the fourth-order leapfrog loop's discrete adjoint.
/// p and z must not overlap an input or each other.
inline void leapfrog4_correlate(std::int64_t n, const double* d_lam, const double* d_om, const double* d_up, const double* d_u,
                                const double* d_um, const double* d_w, double* d_p, double* d_z = nullptr, void* stream = nullptr)
{
  check(wf_leapfrog4_correlate(n, d_lam, d_om, d_up, d_u, d_um, d_w, d_p, d_z, stream));
}

// ---- point sources and receivers (wf_points_*, wf_sources_*; not in the reference) ----
/// Physical points located in the mesh of a Space (wf_points_locate, reference coordinates in [0, 1]^3) with their
/// dofmap rows and interpolation weights on the device.  Throws naming the first point that lies in no cell.
class Points {
public:
  Points(const Space& V, const std::vector<std::array<double, 3>>& xyz, double tol = 1e-10) : _n((int)xyz.size())
  {
    const int n1 = V.degree + 1, nd = n1 * n1 * n1;
    std::vector<double> p(3 * xyz.size()), ref(3 * xyz.size()), w(3 * xyz.size() * n1);
    std::vector<std::int32_t> cell(xyz.size()), dofs(xyz.size() * nd);
    for (std::size_t i = 0; i < xyz.size(); ++i) std::copy(xyz[i].begin(), xyz[i].end(), p.begin() + 3 * i);
    check(wf_points_locate(V.nverts, V.x, V.ncells, V.geom_dofmap, _n, p.data(), tol, cell.data(), ref.data()));
    for (std::size_t i = 0; i < xyz.size(); ++i) {
      if (cell[i] < 0) throw std::runtime_error("wavehip::Points: point " + std::to_string(i) + " lies in no cell of the mesh");
      std::copy(V.dofmap + (std::size_t)cell[i] * nd, V.dofmap + (std::size_t)(cell[i] + 1) * nd, dofs.begin() + i * nd);
    }
    check(wf_points_weights(V.degree, _n, ref.data(), w.data()));
    check(wf_points_create(V.degree, V.ndofs, _n, dofs.data(), w.data(), &_p));
  }
  Points(const Points&) = delete;
  Points& operator=(const Points&) = delete;
  ~Points() { wf_points_destroy(_p); }
  int size() const { return _n; }
  const wf_points* handle() const { return _p; }

private:
  wf_points* _p = nullptr;
  int _n = 0;
};

/// s(t) = amplitude (1 - 2a) e^{-a}, a = (pi frequency (t - delay))^2
inline wf_wavelet ricker(double frequency, double delay, double amplitude = 1.0)
{
  wf_wavelet w{};
  w.kind = WF_WAVELET_RICKER, w.amplitude = amplitude, w.frequency = frequency, w.delay = delay;
  return w;
}

/// Point sources f = s_i(t) delta(x - x_i), the right-hand side of the equation as the model states it
/// (u_tt - c0^2 Lap u = f): add(t, b) does b[d] += sum_i s_i(t) phi_d(x_i) in one launch, one writer per dof.
class Sources {
public:
  Sources(const Space& V, const std::vector<std::array<double, 3>>& xyz, const std::vector<wf_wavelet>& wavelets)
  {
    if (xyz.size() != wavelets.size()) throw std::runtime_error("wavehip::Sources: one wavelet per point");
    Points pts(V, xyz);
    std::vector<std::int32_t> point_of(xyz.size());
    for (std::size_t i = 0; i < xyz.size(); ++i) point_of[i] = (std::int32_t)i;
    check(wf_sources_create(pts.handle(), (int)xyz.size(), point_of.data(), wavelets.data(), &_s));
  }
  Sources(const Sources&) = delete;
  Sources& operator=(const Sources&) = delete;
  ~Sources() { wf_sources_destroy(_s); }
  void add(double t, double* d_b, void* stream = nullptr) const { check(wf_sources_add(_s, t, d_b, stream)); }
  /// b[d] += scale * sum_i d_values[i] phi_d(x_i): device values in the place of the wavelets (wf_sources_add_values),
  /// the transpose of Receivers::sample on the same points
  void add_values(const double* d_values, double* d_b, double scale = 1.0, void* stream = nullptr) const
  {
    check(wf_sources_add_values(_s, d_values, scale, d_b, stream));
  }
  const wf_sources* handle() const { return _s; }

private:
  wf_sources* _s = nullptr;
};

/// Receivers: sample(x, out) evaluates a device vector at the points; record(x, t) appends a row to a device buffer that
/// doubles when full; traces() copies the recorded rows [rows][size()] to the host, times() are their times.
class Receivers {
public:
  Receivers(const Space& V, const std::vector<std::array<double, 3>>& xyz) : _pts(V, xyz) {}
  int size() const { return _pts.size(); }
  const wf_points* points() const { return _pts.handle(); }
  void sample(const double* d_x, double* d_out, void* stream = nullptr) const { check(wf_points_sample(_pts.handle(), d_x, d_out, stream)); }
  /// Room for `rows` more rows and the device pointer of the next one, for a writer that fills them itself (the time
  /// loops of the library; advance() then counts them).  Without receivers there is no buffer: nullptr.
  double* reserve(std::size_t rows)
  {
    const std::size_t R = (std::size_t)size();
    if (!R) return nullptr;
    std::size_t need = _buf ? _buf->size() : 64 * R;   // 64 rows at first, then twice as many
    while (need < (_rows + rows) * R) need *= 2;
    if (!_buf || need > _buf->size()) {
      auto grown = std::make_unique<array<double>>(need);
      if (_buf && _rows) check(wf_copy((std::int64_t)(_rows * R), _buf->data(), grown->data(), nullptr));
      check(wf_sync(nullptr));
      _buf = std::move(grown);
    }
    return _buf->data() + _rows * R;
  }
  /// count `n` rows written behind reserve(), with their times
  void advance(const double* times, std::size_t n)
  {
    _rows += n;
    _times.insert(_times.end(), times, times + n);
  }
  void record(const double* d_x, double t)
  {
    double* row = reserve(1);
    if (row) sample(d_x, row);   // without receivers only the times are kept
    advance(&t, 1);
  }
  std::size_t rows() const { return _rows; }
  const std::vector<double>& times() const { return _times; }
  std::vector<double> traces() const
  {
    std::vector<double> out(_rows * (std::size_t)size());
    check(wf_sync(nullptr));
    if (!out.empty()) check(wf_memcpy_d2h(out.data(), _buf->data(), out.size() * sizeof(double)));
    return out;
  }
  void reset()
  {
    _rows = 0;
    _times.clear();
  }

private:
  Points _pts;
  std::unique_ptr<array<double>> _buf;
  std::size_t _rows = 0;
  std::vector<double> _times;
};

}  // namespace wavehip
