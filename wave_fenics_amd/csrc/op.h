// The operator handle (wf_op) and the set-up steps its creation paths share.
//   op_setup.hip       the shared steps          op_create.hip   wf_op_create and its three paths
//   op_create_box.hip  the box creation path     op_apply.hip    launch, interior / interface splits, info, destroy
//   box_mesh.h         the box as a dofmap mesh (box_space.cpp)
// The index lists the kernels trust are computed in files without HIP that take no wf_op: box_items.h (work items and
// their split), box_run_plan.h (run tables), unique_lists.h (batch-unique lists), march_plan.h (lattice columns).
#pragma once
#include <functional>
#include <memory>

#include "box_mesh.h"
#include "box_run_plan.h"
#include "device_array.h"

namespace wf { struct DenseOpData; struct DenseMassData; }   // the dense simplex operators own their arrays (dense_simplex.h)

// What wf_op_apply launches.  Creation sets it once; apply, the interior / interface splits and wf_op_info switch on it.
enum class OpKernel : int {
  none = 0,
  box_march,             // box, one thread per column, P <= 4 (stiffness_march.hip); geometry form: wf_op.geom
  box_ksplit,            // box, the k-split kernel (stiffness_march_ks.hip)
  box_owner,             // box, owner-computes separable form (stiffness_march_owner.hip)
  box_block,             // box, single-pass block kernel (stiffness_batch.hip)
  idx_march,             // lattice columns found in a caller's dofmap (stiffness_march_idx.hip); geometry form: wf_op.geom
  generic_unique,        // batch stiffness with batch-unique dof lists
  generic_elementwise,   // batch stiffness, element-wise atomics
  lumped_unique,         // lumped mass in the reference's sequence, batch-unique dof lists
  lumped_elementwise,    // lumped mass in the reference's sequence, one thread per element-local dof
  diagonal,              // pre-assembled diagonal, y += m .* x
  mass_march,            // dense mass on lattice columns (mass_march.hip)
  mass_column,           // dense mass, square table, column threads on batch-unique dof lists
  mass_any,              // dense mass, any tensor rule
  dense_simplex,         // dense simplex operator (stiffness_dense.hip)
  dense_simplex_mass,    // dense simplex mass (mass_dense_simplex.hip)
  ordered_stiffness,     // WF_FLAG_ORDERED (ordered.hip): cell batches store to v[slot], one thread per y entry sums its run
  ordered_mass,          // the same for the dense mass, any tensor rule
  ordered_lumped,        // the same for the lumped mass in the reference's sequence
};

// what wf_op_create_box_tuned decides about a box operator before it touches device memory (choose_box_stiffness)
struct BoxChoice {
  int variant = 0;              // marching kernels: index of the compiled cross-section
  int bx = 1, by = 1, bz = 1;   // cells per column (block kernel: per block); also the blocking of the geometry
  int obx = 0, oby = 0;         // owner form: its own cross-section
  int lz = 1;                   // marching kernels: layers per z segment
};

// Every device array is owned here (or by dense / dense_mass) and freed with the handle; wf::op_device_bytes sums them.
struct wf_op {
  OpKernel kernel = OpKernel::none;
  int kind = 0, P = 0, n = 0, nd = 0, nq = 0, ncells = 0, ndofs = 0;
  int structured = 0, nx = 0, ny = 0, nz = 0;
  BoxChoice box{};
  // geometry form of the marching stiffness kernels (box_march, idx_march; box_owner is cell_axes by construction):
  // set by whichever creation path chose it, point for every other kernel
  wf::MarchGeom geom = wf::MarchGeom::point;
  int nq1 = 0;
  int lz0_split = 1;   // length of the first z segment of the interior / interface parts
  double coeff = 0.0;
  int cell_coeff = 0;   // created with a cell coefficient array: folded into the stored geometry (dense simplex: own array)
  wf::DMat dm{};
  wf::DMat am{};   // A = D^T diag(w) D: the 1-D operator of the separable box form (MarchGeom::cell_axes)
  wf::DevArray<int32_t> d_dofmap;
  wf::DevArray<double> d_G6blk;
  wf::DevArray<double> d_Gcell;   // affine cells: G_c per cell, blocked like G6blk (box) or in the plan's slot order
  wf::DevArray<double> d_detJ;
  wf::DevArray<double> d_D;
  wf::DevArray<double> d_phi1;
  wf::DevArray<double> d_mdiag;
  bool diag_named_only = false;   // the vectors hold dofs no cell names: the diagonal apply leaves them alone
  // batch-unique gather/scatter lists of the batch kernels (empty: the kernel scatters element-wise)
  wf::DevArray<int32_t> d_uoff, d_uniq;
  wf::DevArray<uint16_t> d_loc;
  int unique_cb = 0;
  // order-fixed accumulation (WF_FLAG_ORDERED): slot of every element-local entry (internal cell order, tensor order),
  // row offsets per dof and the scratch v[ncells * nd] that pass 1 writes and pass 2 reads
  int ordered = 0;
  wf::DevArray<int32_t> d_slot, d_row_off;
  wf::DevArray<double> d_v;
  // work-item lists of the marching kernel: [0] interior, [1] interface, [2]/[3] the two halves of the interior
  wf::DevArray<int32_t> d_items[4];
  int nitems[4] = {0, 0, 0, 0};
  int have_parts = 0;
  // run table of the owner form's whole apply (box_run_plan.h): [runs][3] = (column, z0, z1) in launch order, on the
  // device and as planned on the host; empty when the uniform z segments of box.lz run
  wf::DevArray<int32_t> d_runs;
  std::vector<int32_t> h_runs;
  int runs_longest = 0;   // layers of the longest run
  // lattice columns of idx_march and mass_march: the arrays, and the view of them the launchers take
  wf::DevArray<int32_t> d_item_base, d_item_pattern, d_item_layers, d_pat_off;
  wf::MarchPlanDev plan{};
  int plan_patterns = 0;
  wf::DenseOpData* dense = nullptr;   // dense simplex operator (stiffness_dense.hip)
  int dense_clamp = 1;
  wf::DenseMassData* dense_mass = nullptr;   // dense simplex mass (mass_dense_simplex.hip)
  int plan_reoriented = 0;
  double plan_fill = 0.0;
  wf_tuning tun{};
  ~wf_op();
};

namespace wf {

using OpPtr = std::unique_ptr<wf_op>;
// the common header of a new operator
OpPtr new_op(int kind, int P, int nd, int nq, int ncells, int ndofs, double c0, const wf_tuning* tuning);

// what the geometry kernels take from the WF_FLAG_* bits
inline int fabs_flag(int flags) { return (flags & WF_FLAG_NO_FABS) ? 0 : 1; }
inline int clamp_flag(int flags) { return (flags & WF_FLAG_NO_CLAMP) ? 0 : 1; }

// the 1-D table a marching stiffness launch takes by value: A for the separable form, else D
inline const DMat& march_table(const wf_op* op) { return op->geom == MarchGeom::cell_axes ? op->am : op->dm; }

// ---- what every entry point on a hexahedral wf_op_desc checks (wf_op_create, wf_cell_form_create and the box entry
// points in front of them); `who` names the entry point in the message ----
// WF_ERR_UNSUPPORTED unless the degree is one the kernels are compiled for
inline int check_hex_degree(int P, const char* who)
{
  if (P >= 1 && P <= kMaxDegree) return WF_OK;
  set_error(std::string(who) + ": degree must be 1..7 (hexahedron)");   // mass.hpp:91-92 "Not implemented"
  return WF_ERR_UNSUPPORTED;
}
// The arrays of a descriptor whose degree holds, every index a kernel will dereference included.  In this order: the
// sizes, a missing dofmap, the dofmap's range, h_perm a permutation, the vertex range, the cell coefficients
// (op_setup.hip).
int check_hex_arrays(const wf_op_desc* desc, const char* who);
// WF_GEOMETRY_PER_CELL asked of a mesh that does not allow it: hex_cell_geometry's first bad cell and its reason
int per_cell_refusal(const char* who, int64_t bad, int reason);
// ... and of a descriptor that hands over geometry of its own
int per_cell_refuses_G(const char* who);

// ---- per-cell geometry of affine hexahedra (hex_cell_geometry.cpp, host only) ----
// geom_dofmap[ncells][8] names the vertices of every cell.  Returns the first cell that does not qualify (*reason says
// why; Gc is then complete only below it), -1 when all do.
int64_t hex_cell_geometry(int P, size_t ncells, const double* xv, const int32_t* geom_dofmap, int use_fabs, int clamp,
                          double* Gc, int* reason);
// the same rule on a box's implicit vertex lattice: false unless every cell qualifies
bool box_cell_geometry(int P, int nx, int ny, int nz, const double* xv, int use_fabs, int clamp, std::vector<double>& Gc);
// metric of per-cell geometry Gc[ncells][6]: the first cell whose G_c has a non-zero off-diagonal (exactly 0, either
// sign, counts as zero), -1 when every G_c is diagonal and the separable (axes) form applies
int64_t first_offdiagonal_cell(const std::vector<double>& Gc);

// ---- set-up steps shared by the creation paths (op_setup.hip) ----
struct HexMesh {
  size_t ncells;
  int nverts;
  const double* xverts;
  const int32_t* geom_dofmap;
};

// the GLL points and weights of degree P on the device
int upload_tables(int P, DevArray<double>& d_pts, DevArray<double>& d_wts);
// batch-unique gather/scatter lists of h_dofmap (what d_dofmap holds), batches of CB cells: built on the host, uploaded
int upload_unique_lists(wf_op* op, const int32_t* h_dofmap, size_t ncells, int nd, int CB);
// h_cell_coeff (may be null): the cell coefficient per cell of `mesh`, folded into every array written
int mesh_geometry_rule(int n1, const double* h_pts, const double* h_wts, const HexMesh& mesh, int use_fabs, int clamp,
                       const double* h_cell_coeff, double* d_G9, double* d_G6blk, double* d_detJ);
int host_detJ(const wf_op_desc* desc, std::vector<double>& hd, const double** hsrc, bool* raw_points);
int upload_derivative_tables(wf_op* op, bool box);
// per-cell geometry h_Gc [ncells][6] times the cell coefficient a_c (h_cell_coeff may be null: nothing to do)
void scale_cell_geometry(std::vector<double>& h_Gc, const double* h_cell_coeff);
int stage_G9(int P, int CB, size_t nslots, const double* direct, const std::function<void(size_t, double*)>& fill_slot,
             double* d_G6blk);

// Axis order of the caller's tensor indices.  The engine's is x-FASTEST: l = i + n (j + n k),
// i along x.  With WF_FLAG_TENSOR_X_SLOWEST the caller's tensor index (the domain of h_perm
// -- or of the dofmap itself when h_perm is NULL -- and the point index of h_G / h_detJ) is
// l' = (i n + j) n + k, the order of Basix' tensor-product factorisation.  Both are folded
// into one element permutation and one point permutation here; the 3x3 axes of G keep
// their meaning (reference axes 0, 1, 2 = x, y, z in both conventions).
struct CallerFrame {
  bool xslow;
  const int32_t* h_perm;
  std::vector<int32_t> eff_perm;
  CallerFrame(const wf_op_desc* desc, int n);
  // engine tensor position -> the caller's element-local index; null: the identity
  const int32_t* perm() const { return xslow ? eff_perm.data() : h_perm; }
  // point permutation of per-point input arrays of an m^3 rule: engine point q <- caller point qmap[q]
  std::vector<int32_t> qmap(int m) const;
};
// tensor-ordered dofmap in the caller's cell order (permute.hpp:10-27 when the caller's element ordering differs):
// *tdm is h_dofmap itself, or store
int tensor_dofmap(const wf_op_desc* desc, const CallerFrame& fr, int nd, std::vector<int32_t>& store, const int32_t** tdm);

// engine point index (lattice frame of the cell, x fastest) -> the caller's point index, per orientation
struct PointMaps {
  const CallerFrame& fr;
  int n;
  std::vector<std::vector<int32_t>> maps = std::vector<std::vector<int32_t>>(48);
  const std::vector<int32_t>& operator()(int code);
};

// ---- op_create_box.hip ----
// Plans the whole apply of a box owner operator for `resident` workgroups by the model of box_run_plan.h: builds or drops
// the run table.  box.lz, and with it the interior / interface parts, stay as they are.
int plan_owner_runs(wf_op* op, int resident);
// what creation does: the cut of the whole apply chosen by timing the uniform plan and aligned cuts on the device (P4,
// more than one round, no wf_tuning.lz; every other operator: no table)
int tune_owner_runs(wf_op* op);

// ---- op_apply.hip ----
size_t op_device_bytes(const wf_op* op);   // wf_op_info_t.device_bytes: what the handle holds now

}  // namespace wf
