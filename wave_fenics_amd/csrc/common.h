// Internal declarations shared by the libwavehip translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "box_items.h"
#include "march_plan.h"
#include "wavehip.h"

// Diagnostic ablation flags (WF_ABLATE environment variable: skip the scatter, serve geometry from
// L2, ...) are compiled in only with -DWF_DIAG (tools/diag_build.sh).  In the product build the
// kernels see the constant 0 and every diagnostic branch folds away: as run-time branches they
// split the hot loops into basic blocks, and at each join the compiler's s_waitcnt bookkeeping
// turns conservative (measured +13 % on the tetrahedral MFMA kernel).
#ifdef WF_DIAG
#define WF_ABLATE_FLAGS(arg) (arg)
#else
#define WF_ABLATE_FLAGS(arg) 0
#endif

namespace wf {

constexpr int kMaxDegree = 7;
constexpr int kMaxN = kMaxDegree + 1;

void set_error(const std::string& msg);

// roctx range markers (markers.cpp); no-ops unless wf_markers_enable(1)
bool markers_on();
void marker_push(const char* name);
void marker_pop();
struct MarkerScope {
  explicit MarkerScope(const char* name) { marker_push(name); }
  ~MarkerScope() { marker_pop(); }
};

#define WF_HIP_CHECK(expr)                                                          \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess) {                                                         \
      ::wf::set_error(std::string(#expr) + " failed: " + hipGetErrorString(_e));     \
      return WF_ERR_HIP;                                                            \
    }                                                                               \
  } while (0)

#define WF_REQUIRE(cond, msg)                    \
  do {                                           \
    if (!(cond)) {                               \
      ::wf::set_error(msg);                      \
      return WF_ERR_INVALID;                     \
    }                                            \
  } while (0)

// After a kernel launch: WF_ERR_HIP with "<what> launch failed: ..." if it did not go out.
inline int launch_status(const char* what)
{
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return WF_OK;
  set_error(std::string(what) + " launch failed: " + hipGetErrorString(e));
  return WF_ERR_HIP;
}
#define WF_LAUNCH_CHECK()                                       \
  do {                                                          \
    if (int _rc = ::wf::launch_status("kernel")) return _rc;    \
  } while (0)
// workgroups of `block` threads for n work items, one each
inline unsigned grid_for(size_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }
// Grid of the streaming kernels (vector_kernels.hip, time_step.hip): one entry per thread up to 2^22 workgroups (their
// loops are grid-stride, so any n is covered).  A grid capped
// at 8 workgroups per CU, every thread looping ~10 times, measured 10 % slower on the streaming kernels in the
// sustained RK4 loop (stage kernel 0.152 -> 0.136 ms, step 1.372 -> 1.308 ms): fresh waves keep more independent
// requests in flight than the iterations of a resident one.
inline unsigned capped_grid(size_t n, unsigned block)
{
  size_t g = (n + block - 1) / block;
  const size_t cap = (size_t)1 << 22;
  return (unsigned)(g < cap ? (g ? g : 1) : cap);
}
// every pointer 16-byte aligned (a null pointer counts as aligned): what the 16-byte forms of the streaming kernels ask
template <class... T>
inline bool aligned16(const T*... p)
{
  return ((reinterpret_cast<uintptr_t>(p) | ... | (uintptr_t)0) & 15) == 0;
}

// Diagnostic ablation mask (profiling only; WF_ABLATE unset or 0 in production):
// 1 = no scatter, 2 = geometry served from L2, 4 = no x gather, 8 = no contractions.
// 16 = owner stiffness kernel: every run ends after its prologue (what a run costs before its first layer).
inline int ablate_flags()
{
#ifdef WF_DIAG
  const char* e = std::getenv("WF_ABLATE");
  return e ? std::atoi(e) : 0;
#else
  return 0;
#endif
}

// Workgroups of a 256-thread kernel without dynamic LDS resident on the device at once (occupancy query x CUs; the z
// segmentation of wf_op_create_box runs its work items in rounds of this many).  0 if the query fails.
template <class Kernel>
int resident_workgroups(Kernel kernel)
{
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) == hipSuccess ? per_cu * cus : 0;
}

// 1-D collocation derivative matrix, passed by value as a kernel argument so
// that compile-time-indexed entries become scalar (SGPR) operands.
struct DMat {
  double v[kMaxN * kMaxN];
};

// ---- host tabulation (tables.cpp) ----
void gll_points_weights(int n, double* pts, double* wts);
void gll_derivative_matrix(int P, double* D);  // clamped, D[q*n + a]

// ---- collocated facet masses (function_space.cpp, host only) ----
// The loop behind wf_fs_facet_mass_weighted and wf_box_facet_mass: acc[dof] += w_a w_b |dx/ds x dx/dt| (times
// cell_weight[cell] if given) over the GLL points of every listed facet (cell, axis, side), facets in list order.
// vertex(c, v): row of xverts of vertex v = a + 2b + 4c of cell c, -1 if the mesh names none; dof(c, l): the dof at
// element-local (l[0], l[1], l[2]) of cell c.
struct FacetList {
  int64_t count;
  const int32_t *cell, *axis, *side;
};
int facet_mass(int P, const FacetList& facets, int64_t ncells, const double* xverts,
               const std::function<int64_t(int64_t, int)>& vertex, const std::function<int32_t(int64_t, const int*)>& dof,
               const double* cell_weight, std::map<int32_t, double>& acc);

// cells per workgroup batch of the column-thread kernels: floor(256 / n^2).  For host code with a run-time P; the
// kernels and their launchers take it from CellBatch<P> (cell_batch.h), which asserts that the two agree.
constexpr int cells_per_batch(int P) { return 256 / ((P + 1) * (P + 1)); }

// ---- geometry set-up (hex_geometry.hip) ----
// d_cell_coeff (every geometry launcher; null: none): the cell coefficient a_c per cell in the order of the cells the
// kernel is given; every entry written, det J w included, is then the entry without it times a_c
int launch_geometry_hex(int P, int ncells, const double* d_xverts, const int32_t* d_geom_dofmap,
                        const double* d_pts, const double* d_wts, int use_fabs, int clamp,
                        double* d_G9, double* d_G6blk, double* d_detJ, const double* d_cell_coeff, hipStream_t s);
int launch_geometry_box(int P, int nx, int ny, int nz, int bx, int by, int bz, const double* d_xverts,
                        const double* d_pts, const double* d_wts, int use_fabs, int clamp,
                        double* d_G6blk, double* d_detJ_lattice, const double* d_cell_coeff, hipStream_t s);
int launch_geometry_hex_slots(int P, int CB, int ncells, const double* d_xverts, const int32_t* d_geom_dofmap,
                              const int32_t* d_slot_of, const uint8_t* d_orient, const double* d_pts, const double* d_wts,
                              int use_fabs, int clamp, double* d_G6blk, const double* d_cell_coeff, hipStream_t s);
int launch_pack_G6(int P, int CB, int ncells, const double* d_G9, double* d_G6blk, hipStream_t s);

// ---- cell-batch stiffness kernels (stiffness_batch.hip) ----
int launch_stiffness_generic(int P, int ncells, const int32_t* d_dofmap, const double* d_G6blk,
                             const double* d_D, const DMat& dm, double coeff, const double* d_x,
                             double* d_y, hipStream_t s);
int launch_stiffness_generic_u(int P, int ncells, const int32_t* d_uoff, const int32_t* d_uniq, const uint16_t* d_loc,
                               const double* d_G6blk, const double* d_D, const DMat& dm, double coeff,
                               const double* d_x, double* d_y, hipStream_t s);
int launch_stiffness_box(int P, int nx, int ny, int nz, int bx, int by, int bz, const double* d_G6blk,
                         const double* d_D, const DMat& dm, double coeff, const double* d_x, double* d_y,
                         hipStream_t s);

// ---- cell-batch mass kernels (mass_batch.hip) ----
int launch_mass_lumped(int64_t nentries, const int32_t* d_dofmap, const double* d_detJ, const double* d_x,
                       double* d_y, hipStream_t s);
// y[d] += m[d] x[d] where m[d] != 0: the pre-assembled diagonal on vectors that hold dofs no cell names (m = 0 there)
int launch_diagonal_named(int64_t n, const double* d_m, const double* d_x, double* d_y, hipStream_t s);
int launch_mass_lumped_u(int ncells, int nd, int CB, const int32_t* d_uoff, const int32_t* d_uniq,
                         const uint16_t* d_loc, const double* d_detJ, const double* d_x, double* d_y, hipStream_t s);
int mass_dense_cells_per_batch(int mx);
int launch_mass_dense_col(int P, int ncells, const int32_t* d_uoff, const int32_t* d_uniq, const uint16_t* d_loc,
                          const double* d_phi1, const double* d_detJ, const double* d_x, double* d_y, hipStream_t s);
int launch_mass_dense(int P, int nq1, int ncells, const int32_t* d_dofmap, const int32_t* d_uoff,
                      const int32_t* d_uniq, const uint16_t* d_loc, int CBu, const double* d_phi1,
                      const double* d_detJ, const double* d_x, double* d_y, hipStream_t s);
// pass 1 of the order-fixed accumulation (ordered.hip): the kernel above it with v[slot[c][l]] = element-local value
int launch_mass_dense_ordered(int P, int nq1, int ncells, const int32_t* d_dofmap, const int32_t* d_slot, const double* d_phi1,
                              const double* d_detJ, const double* d_x, double* d_v, hipStream_t s);
int launch_mass_lumped_ordered(int64_t nentries, const int32_t* d_dofmap, const int32_t* d_slot, const double* d_detJ,
                               const double* d_x, double* d_v, hipStream_t s);

// ---- order-fixed accumulation (ordered.hip): the plan and the stiffness pass 1; pass 2 is wf_segment_sum_add ----
// ordered_slots: the stable counting sort of a flattened dofmap (wf_ordered_slots)
int ordered_slots(int64_t nentries, int32_t ndofs, const int32_t* dofmap, int32_t* row_off, int32_t* slot);
// pass 1, stiffness: k_stiffness_generic (stiffness_elementwise.h) with v[slot[c][l]] = element-local value
int launch_stiffness_ordered(int P, int ncells, const int32_t* d_dofmap, const int32_t* d_slot, const double* d_G6blk,
                             const double* d_D, const DMat& dm, double coeff, const double* d_x, double* d_v, hipStream_t s);

// ---- marching kernels (stiffness_march*.hip, mass_march.hip) ----
// lattice plans with a fill (cells per cell slot) below this keep the batch kernel: the marching kernels
// read geometry for every slot of a column, empty or not
constexpr double kMinPlanFill = 0.55;
bool march_variant(int P, int variant, int* bx, int* by);
// Geometry form of the box marching kernel (stiffness_march.hip): G at every point, one full G_c per affine cell, or
// one diagonal G_c per rectilinear affine cell (the separable operator: one 1-D operator A = D^T diag(w) D per axis).
enum class MarchGeom : int { point = 0, cell = 1, cell_axes = 2 };
// geom != point: d_Gcell is the per-cell geometry of affine cells (d_G6blk unused); d_D then carries the 1-D weights
// at [2 n^2, 2 n^2 + n) and, for cell_axes, A at [2 n^2 + n, 3 n^2 + n); dm is A instead of D for cell_axes
int launch_stiffness_march(int P, int variant, MarchGeom geom, int nx, int ny, int nz, int lz, int lz0,
                           const double* d_G6blk, const double* d_Gcell, const double* d_D, const DMat& dm, double coeff,
                           const double* d_x, double* d_y, const int32_t* d_items, int nitems, hipStream_t s);
int march_resident(int P, int variant, MarchGeom geom);   // workgroups resident on the device (occupancy query)
// Owner-computes form of cell_axes (stiffness_march_owner.hip): every y entry read and written once by its owning thread,
// no atomics.  Its own cross-section table (march_owner_variant); columns = lattice lines in pieces of P*BX x P*BY.
bool march_owner_variant(int P, int variant, int* bx, int* by);
// d_Gcell blocked by gbx x gby: the atomic form's cross-section at P <= 4, the owner cross-section itself at P >= 5
// lz < 0: d_items is a run table of nitems entries (column, z0, z1), one per workgroup (box_run_plan.h)
int launch_stiffness_march_owner(int P, int variant, int nx, int ny, int nz, int lz, int lz0, int gbx, int gby,
                                 const double* d_Gcell,
                                 const double* d_D, const DMat& am, double coeff, const double* d_x, double* d_y,
                                 const int32_t* d_items, int nitems, hipStream_t s);
int march_owner_resident(int P, int variant);   // workgroups resident on the device (occupancy query)
// work items of the box marching kernels (columns x z segments), for host and kernels alike: box_items.h
// indexed marching kernels for arbitrary dofmaps (stiffness_march_idx.hip, stiffness_march_ks.hip): the plan is
// MarchPlan of march_plan.h, this is the view of its device arrays the launchers take
struct MarchPlanDev {
  int nitems = 0, lz = 0, tile_size = 0, bx = 0, by = 0;
  int32_t *d_item_base = nullptr, *d_item_pattern = nullptr, *d_item_layers = nullptr, *d_pat_off = nullptr;
};
constexpr int OP_KIND_STIFFNESS = 0, OP_KIND_MASS = 1;
// column cross-section, LDS need and LDS budget (per workgroup) of the indexed marching kernel of (kind, P); the
// needs of the k-split and the dense-mass kernel themselves: march_ks_lds_bytes, mass_march_lds_bytes (march_column.h)
void march_idx_shape(int kind, int P, int* bx, int* by);   // stiffness: keeps a compiled (*bx, *by) of the k-split kernel
// geom: the geometry form of the stiffness kernel at P <= 4 (the per-cell forms have less static LDS and run more
// workgroups per CU)
size_t march_idx_lds_bytes(int kind, int P, int BX, int BY, int lz, MarchGeom geom = MarchGeom::point);
size_t march_idx_lds_budget(int kind, int P, int BX, int BY, MarchGeom geom = MarchGeom::point);
// dense mass on the lattice columns (mass_march.hip), 1-D table phi1[M][P + 1].  mass_march_shape: whether the pair
// (P, M) is compiled; then keeps a compiled (*bx, *by) of the pair, else sets the pair's default
bool mass_march_shape(int P, int M, int* bx, int* by);
int launch_mass_march(int P, int M, const MarchPlanDev& pd, const double* d_detJblk, const double* d_phi1, const double* d_x,
                      double* d_y, hipStream_t s);
// geom != point (P <= 4): d_geom is the per-cell geometry Gc[(item lz + layer) BX BY + cell][6] of affine cells and d_D
// carries the weights and A as for launch_stiffness_march; dm is A instead of D for cell_axes
int launch_stiffness_march_idx(int P, MarchGeom geom, const MarchPlanDev& pd, const double* d_geom, const double* d_D,
                               const DMat& dm, double coeff, const double* d_x, double* d_y, const int32_t* d_items,
                               int nitems, hipStream_t s);
// k-split marching kernel (stiffness_march_ks.hip): the stiffness kernel of every degree
bool march_ks_shape(int P, int* bx, int* by);   // keeps a compiled (*bx, *by), else sets the degree's default
int march_ks_resident(int P, int bx, int by);   // workgroups resident on the chip
int launch_stiffness_march_ks_box(int P, int bx, int by, int nx, int ny, int nz, int lz, int lz0, const double* d_G6blk,
                                  const double* d_D, const DMat& dm, double coeff, const double* d_x, double* d_y,
                                  const int32_t* d_items, int nitems, hipStream_t s);
int launch_stiffness_march_ks_idx(int P, int bx, int by, const MarchPlanDev& pd, const double* d_G6blk, const double* d_D,
                                  const DMat& dm, double coeff, const double* d_x, double* d_y, const int32_t* d_items,
                                  int nitems, hipStream_t s);
// a cell coefficient array (may be null): WF_ERR_INVALID naming the first cell whose entry is not finite
inline int check_cell_coeff(const double* a, size_t ncells, const char* who)
{
  for (size_t c = 0; a && c < ncells; ++c)
    if (!std::isfinite(a[c])) {
      set_error(std::string(who) + ": h_cell_coeff[" + std::to_string(c) + "] is not finite (cell " + std::to_string(c) + ")");
      return WF_ERR_INVALID;
    }
  return WF_OK;
}
// host-side validation of indices a kernel will dereference: WF_ERR_INVALID with `message` unless every
// idx[e], e < count, lies in [0, bound)
inline int check_index_range(const int32_t* idx, size_t count, int64_t bound, const std::string& message)
{
  for (size_t e = 0; e < count; ++e) WF_REQUIRE(idx[e] >= 0 && idx[e] < bound, message);
  return WF_OK;
}

}  // namespace wf
