// Set-up steps shared by the operator creation paths and the cell forms (op.h): the checks of a hexahedral descriptor
// and the per-cell refusals, tables, geometry staging, the upload of the batch-unique lists (unique_lists.cpp builds
// them, also for the batch plan of the dense simplex operators), the caller's tensor frame.
#include <cmath>
#include <cstring>

#include "dense_simplex.h"
#include "op.h"
#include "unique_lists.h"

namespace wf {

OpPtr new_op(int kind, int P, int nd, int nq, int ncells, int ndofs, double c0, const wf_tuning* tuning)
{
  OpPtr op(new wf_op);
  op->kind = kind;
  op->P = P;
  op->n = P + 1;
  op->nd = nd;
  op->nq = nq;
  op->ncells = ncells;
  op->ndofs = ndofs;
  op->coeff = -1.0 * c0 * c0;   // operators.hpp:115
  op->tun = tuning ? *tuning : wf_tuning{};
  return op;
}

int check_hex_arrays(const wf_op_desc* desc, const char* who)
{
  const std::string w = std::string(who) + ": ";
  WF_REQUIRE(desc->ncells >= 0 && desc->ndofs >= 0, w + "negative size");
  WF_REQUIRE(desc->h_dofmap || desc->ncells == 0, w + "dofmap missing");
  const int n = desc->degree + 1, nd = n * n * n;
  const size_t ncells = (size_t)desc->ncells;
  int rc;
  if ((rc = check_index_range(desc->h_dofmap, ncells * nd, desc->ndofs, w + "dofmap entry out of range")) != WF_OK) return rc;
  if (desc->h_perm) {
    std::vector<char> seen(nd, 0);
    for (int k = 0; k < nd; ++k) {
      WF_REQUIRE(desc->h_perm[k] >= 0 && desc->h_perm[k] < nd && !seen[desc->h_perm[k]], w + "perm is not a permutation");
      seen[desc->h_perm[k]] = 1;
    }
  }
  if (desc->h_xverts && desc->h_geom_dofmap
      && (rc = check_index_range(desc->h_geom_dofmap, ncells * 8, desc->nverts, w + "vertex index out of range")) != WF_OK)
    return rc;
  return check_cell_coeff(desc->h_cell_coeff, ncells, who);
}

int per_cell_refusal(const char* who, int64_t bad, int reason)
{
  static const char* kWhy[4] = {"", "is not affine (its edge vectors along a reference axis differ)",
                                "is degenerate (det J zero or not finite)",
                                "has geometry on which the -1/0/1 clamp takes effect (WF_FLAG_NO_CLAMP turns it off)"};
  set_error(std::string(who) + ": WF_GEOMETRY_PER_CELL: cell " + std::to_string(bad) + " " + kWhy[reason]);
  return WF_ERR_INVALID;
}

int per_cell_refuses_G(const char* who)
{
  set_error(std::string(who) + ": WF_GEOMETRY_PER_CELL: per-cell geometry is derived from the mesh; h_G must be NULL");
  return WF_ERR_UNSUPPORTED;
}

int tensor_dofmap(const wf_op_desc* desc, const CallerFrame& fr, int nd, std::vector<int32_t>& store, const int32_t** tdm)
{
  *tdm = desc->h_dofmap;
  if (!fr.perm() || desc->ncells == 0) return WF_OK;
  store.resize((size_t)desc->ncells * nd);
  int rc = wf_reorder_dofmap(desc->ncells, nd, fr.perm(), desc->h_dofmap, store.data());
  *tdm = store.data();
  return rc;
}

void scale_cell_geometry(std::vector<double>& h_Gc, const double* h_cell_coeff)
{
  if (h_cell_coeff)
    for (size_t e = 0; e < h_Gc.size(); ++e) h_Gc[e] *= h_cell_coeff[e / 6];
}

int upload_tables(int P, DevArray<double>& d_pts, DevArray<double>& d_wts)
{
  const int n = P + 1;
  std::vector<double> pts(n), wts(n);
  gll_points_weights(n, pts.data(), wts.data());
  int rc = d_pts.upload(pts);
  if (rc != WF_OK) return rc;
  return d_wts.upload(wts);
}

// The batch-unique lists (unique_lists.h) of the batch kernels, for batches of CB cells of h_dofmap: the dofmap that
// d_dofmap holds, tensor order and internal cell order.
int upload_unique_lists(wf_op* op, const int32_t* h_dofmap, size_t ncells, int nd, int CB)
{
  if (ncells == 0) return WF_OK;
  UniqueLists lists;
  if ((size_t)CB * nd > 65535 || !build_unique_lists(h_dofmap, ncells, nd, CB, &lists)) {
    set_error("build_unique_lists: batch too large for 16-bit local indices");
    return WF_ERR_UNSUPPORTED;
  }
  int rc;
  if ((rc = op->d_uoff.upload(lists.uoff)) != WF_OK) return rc;
  if ((rc = op->d_uniq.upload(lists.uniq)) != WF_OK) return rc;
  if ((rc = op->d_loc.upload(lists.loc)) != WF_OK) return rc;
  op->unique_cb = CB;
  return WF_OK;
}

// The same for the 64-cell batches of the dense simplex kernels (dense_simplex.h), with the local indices packed two to
// a word in the kernels' operand order (pack_dense_loc).
int DenseBatchPlanDev::build(int nd, int KT, int ncells, const int32_t* dofmap)
{
  UniqueLists lists;
  if (!build_unique_lists(dofmap, (size_t)ncells, nd, kDenseBatchCells, &lists)) {
    set_error("dense_setup: more than 65535 unique dofs in a batch");
    return WF_ERR_UNSUPPORTED;
  }
  nbatch = (int)lists.uoff.size() - 1;
  numax = std::max(1, lists.largest());
  int rc;
  if ((rc = locP.upload(pack_dense_loc(lists.loc, (size_t)ncells, nd, KT, kDenseBatchCells))) != WF_OK) return rc;
  if ((rc = uoff.upload(lists.uoff)) != WF_OK) return rc;
  return uniq.upload(lists.uniq);
}

// Geometry of every cell at the n1^3 points of a 1-D rule, computed from the mesh into whichever of the device arrays
// d_G9[ncells][n1^3][9], d_G6blk (blocked by cells_per_batch(n1 - 1)) and d_detJ[ncells][n1^3] (det J * w) are given.
// The kernel is generic in the number of points per direction.
int mesh_geometry_rule(int n1, const double* h_pts, const double* h_wts, const HexMesh& mesh, int use_fabs, int clamp,
                       const double* h_cell_coeff, double* d_G9, double* d_G6blk, double* d_detJ)
{
  DevArray<double> d_x, d_pts, d_wts, d_coeff;
  DevArray<int32_t> d_gd;
  int rc;
  if ((rc = d_x.upload(mesh.xverts, (size_t)mesh.nverts * 3)) != WF_OK) return rc;
  if ((rc = d_gd.upload(mesh.geom_dofmap, mesh.ncells * 8)) != WF_OK) return rc;
  if ((rc = d_pts.upload(h_pts, (size_t)n1)) != WF_OK) return rc;
  if ((rc = d_wts.upload(h_wts, (size_t)n1)) != WF_OK) return rc;
  if (h_cell_coeff && (rc = d_coeff.upload(h_cell_coeff, mesh.ncells)) != WF_OK) return rc;
  if ((rc = launch_geometry_hex(n1 - 1, (int)mesh.ncells, d_x.data(), d_gd.data(), d_pts.data(), d_wts.data(), use_fabs,
                                clamp, d_G9, d_G6blk, d_detJ, d_coeff.data(), nullptr)) != WF_OK)
    return rc;
  WF_HIP_CHECK(hipDeviceSynchronize());
  return WF_OK;
}

// det J * w per cell and point of a dense mass with a square table, on the host: the caller's h_detJ (caller's point
// order), else computed from the mesh at the caller's rule into hd (*raw_points: the engine's point order).  With a cell
// coefficient every entry is det J w times a_c (a scaled copy of h_detJ in hd)
int host_detJ(const wf_op_desc* desc, std::vector<double>& hd, const double** hsrc, bool* raw_points)
{
  *hsrc = desc->h_detJ;
  *raw_points = !desc->h_detJ;
  const int n = desc->nq1;
  if (desc->h_detJ && desc->h_cell_coeff) {
    const size_t nq = (size_t)n * n * n;
    hd.resize((size_t)desc->ncells * nq);
    for (size_t c = 0; c < (size_t)desc->ncells; ++c)
      for (size_t q = 0; q < nq; ++q) hd[c * nq + q] = desc->h_detJ[c * nq + q] * desc->h_cell_coeff[c];
    *hsrc = hd.data();
  }
  if (desc->h_detJ) return WF_OK;
  DevArray<double> d_det;
  hd.resize((size_t)desc->ncells * n * n * n);
  int rc;
  if ((rc = d_det.alloc(hd.size())) != WF_OK) return rc;
  const HexMesh mesh{(size_t)desc->ncells, desc->nverts, desc->h_xverts, desc->h_geom_dofmap};
  if ((rc = mesh_geometry_rule(n, desc->h_qpts1, desc->h_qwts1, mesh, fabs_flag(desc->flags), 0, desc->h_cell_coeff, nullptr, nullptr,
                               d_det.data())) != WF_OK)
    return rc;
  WF_HIP_CHECK(hipMemcpy(hd.data(), d_det.data(), hd.size() * sizeof(double), hipMemcpyDeviceToHost));
  *hsrc = hd.data();
  return WF_OK;
}

// Uploads the 1-D tables to op->d_D: D, then its transpose (scalar-loaded by the k-split kernel); op->dm = D.
// box: then the 1-D weights (per-cell marching kernel), then A = D^T diag(w) D (axes form: A[i][a] = sum_q D[q][i] w_q
// D[q][a], summed in long double and rounded once); op->am = A.
int upload_derivative_tables(wf_op* op, bool box)
{
  const int P = op->P, n = op->n;
  std::vector<double> D(box ? 3 * n * n + n : 2 * n * n);
  gll_derivative_matrix(P, D.data());
  for (int q = 0; q < n; ++q)
    for (int a2 = 0; a2 < n; ++a2) D[n * n + a2 * n + q] = D[q * n + a2];
  for (int q = 0; q < n * n; ++q) op->dm.v[q] = D[q];
  if (box) {
    std::vector<double> pts(n);
    double* w = D.data() + 2 * n * n;
    gll_points_weights(n, pts.data(), w);
    double* A = w + n;
    for (int i = 0; i < n; ++i)
      for (int a2 = i; a2 < n; ++a2) {
        long double s = 0.0L;
        for (int q = 0; q < n; ++q) s += (long double)D[q * n + i] * (long double)w[q] * (long double)D[q * n + a2];
        A[i * n + a2] = A[a2 * n + i] = (double)s;
      }
    for (int q = 0; q < n * n; ++q) op->am.v[q] = A[q];
  }
  return op->d_D.upload(D);
}

// Stages geometry given as G[slot][nd][3][3] (the reference layout, precomputation.hpp:46) into the blocked upper
// triangle d_G6blk, in slabs of 64 MiB to bound the temporary.  direct: the caller's array when it is in slot order
// already; otherwise fill_slot(slot, dst) writes the nd * 9 values of a slot (zeros for an empty one).
int stage_G9(int P, int CB, size_t nslots, const double* direct, const std::function<void(size_t, double*)>& fill_slot,
             double* d_G6blk)
{
  const int n = P + 1, nd = n * n * n;
  const size_t slab_slots = std::max<size_t>(CB, (((size_t)64 << 20) / (nd * 9 * sizeof(double))) / CB * CB);
  DevArray<double> d_G9;
  int rc;
  if ((rc = d_G9.alloc(std::min(slab_slots, nslots) * nd * 9)) != WF_OK) return rc;
  std::vector<double> slab;
  for (size_t s0 = 0; s0 < nslots; s0 += slab_slots) {
    const size_t ns = std::min(slab_slots, nslots - s0);
    const double* hsrc = direct ? direct + s0 * nd * 9 : nullptr;
    if (!hsrc) {
      slab.resize(ns * nd * 9);
      for (size_t q = 0; q < ns; ++q) fill_slot(s0 + q, &slab[q * nd * 9]);
      hsrc = slab.data();
    }
    WF_HIP_CHECK(hipMemcpy(d_G9.data(), hsrc, ns * nd * 9 * sizeof(double), hipMemcpyHostToDevice));
    // slabs start on a batch boundary, so the packed destination is offset by whole batches
    if ((rc = launch_pack_G6(P, CB, (int)ns, d_G9.data(), d_G6blk + (s0 / CB) * CB * nd * 6, nullptr)) != WF_OK) return rc;
    WF_HIP_CHECK(hipDeviceSynchronize());
  }
  return WF_OK;
}

CallerFrame::CallerFrame(const wf_op_desc* desc, int n) : xslow((desc->flags & WF_FLAG_TENSOR_X_SLOWEST) != 0), h_perm(desc->h_perm)
{
  if (!xslow) return;
  eff_perm.resize((size_t)n * n * n);
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) {
        const int lp = (i * n + j) * n + k;
        eff_perm[i + n * (j + n * k)] = h_perm ? h_perm[lp] : lp;
      }
}

std::vector<int32_t> CallerFrame::qmap(int m) const
{
  std::vector<int32_t> q((size_t)m * m * m);
  for (int k = 0; k < m; ++k)
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < m; ++i) q[i + m * (j + m * k)] = xslow ? (i * m + j) * m + k : i + m * (j + m * k);
  return q;
}

const std::vector<int32_t>& PointMaps::operator()(int code)
{
  auto& m = maps[code];
  if (m.empty()) {
    const std::vector<int32_t> qm = fr.qmap(n), om = orient_node_map(code, n);
    m.resize(om.size());
    for (size_t l = 0; l < om.size(); ++l) m[l] = qm[om[l]];
  }
  return m;
}

}  // namespace wf

// The dof numbering that follows the lattice plan of the stiffness operator (plan_numbering, march_plan.h).
// h_dofmap: tensor-ordered (x fastest) [ncells][(P+1)^3]; h_new_of_old[ndofs]: new index of every old dof.
extern "C" int wf_lattice_numbering(int degree, int64_t ncells, int32_t ndofs, const int32_t* h_dofmap, int32_t* h_new_of_old)
{
  using namespace wf;
  WF_REQUIRE(degree >= 1 && degree <= 7, "wf_lattice_numbering: degree must be 1..7");
  WF_REQUIRE(ncells >= 0 && ndofs >= 0 && (ncells == 0 || h_dofmap) && (ndofs == 0 || h_new_of_old), "wf_lattice_numbering: bad arguments");
  const int P = degree, n = P + 1, nd = n * n * n;
  for (int64_t e = 0; e < ncells * nd; ++e)
    WF_REQUIRE(h_dofmap[e] >= 0 && h_dofmap[e] < ndofs, "wf_lattice_numbering: dofmap entry out of range");
  int BX = 0, BY = 0;
  march_idx_shape(OP_KIND_STIFFNESS, P, &BX, &BY);
  MarchPlan plan;
  int rc = build_march_plan(P, (size_t)ncells, h_dofmap, BX, BY, 8, 8, true, &plan);
  if (rc != WF_OK) return rc;
  plan_numbering(plan, (size_t)ncells, nd, h_dofmap, ndofs, h_new_of_old);
  return WF_OK;
}
