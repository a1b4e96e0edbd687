// C ABI of libwavehip: device shims, geometry setup, operator handles.
// See include/wavehip.h for the reference interface each entry point replaces.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "march_column.h"

using namespace wf;

// What wf_op_apply launches.  Creation sets it once; apply, the interior / interface splits and wf_op_info switch on it.
enum class OpKernel : int {
  none = 0,
  box_march,             // box, one thread per column, P <= 4 (stiffness_march.hip); geometry form: wf_op.geom
  box_ksplit,            // box, the k-split kernel (stiffness_march_ks.hip)
  box_owner,             // box, owner-computes separable form (stiffness_march_owner.hip)
  box_block,             // box, single-pass block kernel (kernels.hip)
  idx_march,             // lattice columns found in a caller's dofmap (stiffness_march_idx.hip)
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
  MarchGeom geom = MarchGeom::point;   // geometry form of box_march (box_owner is cell_axes by construction)
  int lz = 1;                   // marching kernels: layers per z segment
};

struct wf_op {
  OpKernel kernel = OpKernel::none;
  int kind = 0, P = 0, n = 0, nd = 0, nq = 0, ncells = 0, ndofs = 0;
  int structured = 0, nx = 0, ny = 0, nz = 0;
  BoxChoice box{};
  int nq1 = 0;
  int lz0_split = 1;   // length of the first z segment of the interior / interface parts
  double coeff = 0.0;
  DMat dm{};
  DMat am{};   // A = D^T diag(w) D: the 1-D operator of the separable box form (MarchGeom::cell_axes)
  int32_t* d_dofmap = nullptr;
  double* d_G6blk = nullptr;
  double* d_Gcell = nullptr;   // box of affine cells: G_c per cell, blocked like G6blk (stiffness_march.hip)
  double* d_detJ = nullptr;
  double* d_D = nullptr;
  double* d_phi1 = nullptr;
  double* d_mdiag = nullptr;
  bool diag_named_only = false;   // the vectors hold dofs no cell names: the diagonal apply leaves them alone
  // batch-unique gather/scatter lists of the batch kernels (null: the kernel scatters element-wise)
  int32_t* d_uoff = nullptr;
  int32_t* d_uniq = nullptr;
  uint16_t* d_loc = nullptr;
  int unique_cb = 0;
  // order-fixed accumulation (WF_FLAG_ORDERED): slot of every element-local entry (internal cell order, tensor order),
  // row offsets per dof and the scratch v[ncells * nd] that pass 1 writes and pass 2 reads
  int ordered = 0;
  int32_t* d_slot = nullptr;
  int32_t* d_row_off = nullptr;
  double* d_v = nullptr;
  // work-item lists of the marching kernel: [0] interior, [1] interface, [2]/[3] the two halves of the interior
  int32_t* d_items[4] = {nullptr, nullptr, nullptr, nullptr};
  int nitems[4] = {0, 0, 0, 0};
  int have_parts = 0;
  MarchPlanDev plan{};            // lattice columns of idx_march and mass_march
  MarchGeom idx_geom = MarchGeom::point;   // geometry form of idx_march (per cell: d_Gcell in the plan's slot order)
  int plan_patterns = 0;
  DenseOpData* dense = nullptr;   // dense simplex operator (stiffness_dense.hip)
  int dense_clamp = 1;
  DenseMassData* dense_mass = nullptr;   // dense simplex mass (mass_dense_simplex.hip)
  size_t device_bytes = 0;
  int plan_reoriented = 0;
  double plan_fill = 0.0;
  wf_tuning tun{};
};

namespace {

template <typename T>
int dev_alloc(T** p, size_t count, size_t* total)
{
  *p = nullptr;
  if (count == 0) return WF_OK;
  WF_HIP_CHECK(hipMalloc((void**)p, count * sizeof(T)));
  if (total) *total += count * sizeof(T);
  return WF_OK;
}

template <typename T>
int dev_upload(T** p, const T* host, size_t count, size_t* total)
{
  int rc = dev_alloc(p, count, total);
  if (rc != WF_OK) return rc;
  if (count) WF_HIP_CHECK(hipMemcpy(*p, host, count * sizeof(T), hipMemcpyHostToDevice));
  return WF_OK;
}

// temporary device buffer freed at scope exit
template <typename T>
struct Scratch {
  T* p = nullptr;
  ~Scratch()
  {
    if (p) (void)hipFree(p);
  }
};

void free_op(wf_op* op)
{
  if (!op) return;
  (void)hipFree(op->d_dofmap);
  (void)hipFree(op->d_G6blk);
  (void)hipFree(op->d_Gcell);
  (void)hipFree(op->d_detJ);
  (void)hipFree(op->d_D);
  (void)hipFree(op->d_phi1);
  (void)hipFree(op->d_mdiag);
  (void)hipFree(op->d_uoff);
  (void)hipFree(op->d_uniq);
  (void)hipFree(op->d_loc);
  (void)hipFree(op->d_slot);
  (void)hipFree(op->d_row_off);
  (void)hipFree(op->d_v);
  for (int k = 0; k < 4; ++k) (void)hipFree(op->d_items[k]);
  (void)hipFree(op->plan.d_item_base);
  (void)hipFree(op->plan.d_item_pattern);
  (void)hipFree(op->plan.d_item_layers);
  (void)hipFree(op->plan.d_pat_off);
  dense_free(op->dense);
  dense_mass_free(op->dense_mass);
  delete op;
}

int upload_tables(int P, Scratch<double>& d_pts, Scratch<double>& d_wts)
{
  const int n = P + 1;
  std::vector<double> pts(n), wts(n);
  gll_points_weights(n, pts.data(), wts.data());
  int rc = dev_upload(&d_pts.p, pts.data(), n, nullptr);
  if (rc != WF_OK) return rc;
  return dev_upload(&d_wts.p, wts.data(), n, nullptr);
}

// Batch-unique gather/scatter lists: for every batch of CB consecutive cells the
// sorted list of its distinct dofs (uniq, offsets uoff) and the position of each
// element-local dof in that list (loc).  Kernels read x once per unique dof, sum
// the batch in LDS and issue one global atomic per unique dof.
int build_unique_lists(wf_op* op, size_t ncells, int nd, int CB)
{
  if (ncells == 0) return WF_OK;
  if ((size_t)CB * nd > 65535) {
    set_error("build_unique_lists: batch too large for 16-bit local indices");
    return WF_ERR_UNSUPPORTED;
  }
  const size_t nbatch = (ncells + CB - 1) / CB;
  std::vector<int32_t> tdm(ncells * nd);
  WF_HIP_CHECK(hipMemcpy(tdm.data(), op->d_dofmap, tdm.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<int32_t> uoff(nbatch + 1, 0), uniq, tmp;
  std::vector<uint16_t> loc(ncells * nd);
  uniq.reserve(ncells * nd / 2);
  for (size_t b = 0; b < nbatch; ++b) {
    const size_t c0 = b * CB, nc = std::min<size_t>(CB, ncells - c0);
    tmp.assign(tdm.begin() + c0 * nd, tdm.begin() + (c0 + nc) * nd);
    std::sort(tmp.begin(), tmp.end());
    tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
    for (size_t e = c0 * nd; e < (c0 + nc) * nd; ++e)
      loc[e] = (uint16_t)(std::lower_bound(tmp.begin(), tmp.end(), tdm[e]) - tmp.begin());
    uniq.insert(uniq.end(), tmp.begin(), tmp.end());
    uoff[b + 1] = (int32_t)uniq.size();
  }
  int rc;
  if ((rc = dev_upload(&op->d_uoff, uoff.data(), uoff.size(), &op->device_bytes)) != WF_OK) return rc;
  if ((rc = dev_upload(&op->d_uniq, uniq.data(), uniq.size(), &op->device_bytes)) != WF_OK) return rc;
  if ((rc = dev_upload(&op->d_loc, loc.data(), loc.size(), &op->device_bytes)) != WF_OK) return rc;
  op->unique_cb = CB;
  return WF_OK;
}

// Per-cell geometry of hexahedral cells whose eight vertices vert(c, v) names (v = a + 2 b + 4 c', the tensor order of
// h_geom_dofmap).  The trilinear map of a cell is affine when its edge vectors along each reference axis are bitwise
// equal; J is then [x1-x0 | x2-x0 | x4-x0] everywhere and G(q) = J^-1 J^-T |det J| w_q = G_c w_i w_j w_k.
// A cell qualifies when
//  * it is affine (else reason 1) with det J != 0, finite (else reason 2);
//  * with the reference's -1/0/1 clamp on: the clamp changes neither a cmap derivative at the rule's points nor a
//    component of any G(q) (it maps |v| <= 1e-8 to 0 and v within 1e-5 of +-1 to +-1: per point that would
//    be a change per-cell G_c w_i w_j w_k cannot express; else reason 3).  Components that are exactly 0 stay 0 either way.
// Computing G_c from the edge vectors avoids the cancellation of the sum over vertices x_v dphi_v.
// Gc (may be null): [ncells][6] in cell order, components G00 G01 G02 G11 G12 G22 (the blocked layout's order).
// Returns the first cell that does not qualify (Gc is then complete only below it), -1 when all do.
template <class VertexOf>
int64_t hex_cell_geometry(int P, size_t ncells, const double* xv, VertexOf&& vert, int use_fabs, int clamp, double* Gc,
                          int* reason)
{
  const int n = P + 1;
  std::vector<double> pts(n), wts(n);
  gll_points_weights(n, pts.data(), wts.data());
  auto clamp101 = [](double v) {   // as kernels.hip
    if (std::fabs(v + 1.0) <= 1e-8 + 1e-5) v = -1.0;
    if (std::fabs(v) <= 1e-8) v = 0.0;
    if (std::fabs(v - 1.0) <= 1e-8 + 1e-5) v = 1.0;
    return v;
  };
  std::vector<double> W;   // w_i w_j w_k as the per-point geometry forms them
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) W.push_back(wts[i] * wts[j] * wts[k]);
  const double wmin = *std::min_element(W.begin(), W.end()), wmax = *std::max_element(W.begin(), W.end());
  bool cmap_clamped = false;   // the same for every cell
  if (clamp) {
    for (int k = 0; k < n; ++k)
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
          const double f0[2] = {1.0 - pts[i], pts[i]}, f1[2] = {1.0 - pts[j], pts[j]}, f2[2] = {1.0 - pts[k], pts[k]};
          const double g[2] = {-1.0, 1.0};
          for (int v = 0; v < 8; ++v) {
            const int a = v & 1, b = (v >> 1) & 1, c = (v >> 2) & 1;
            const double d[3] = {g[a] * f1[b] * f2[c], f0[a] * g[b] * f2[c], f0[a] * f1[b] * g[c]};
            for (double dv : d)
              if (clamp101(dv) != dv) cmap_clamped = true;
          }
        }
  }
  // does clamp101 leave every value |v| * W alone?  (relative slack for the rounding of the per-point form)
  constexpr double slack = 1e-6, lo1 = 1.0 - (1e-8 + 1e-5), hi1 = 1.0 + (1e-8 + 1e-5);
  auto clamp_free = [&](double v) {
    v = std::fabs(v);
    if (v == 0.0) return true;
    if (v * wmin * (1.0 - slack) <= 1e-8) return false;
    if (v * wmax * (1.0 + slack) < lo1 || v * wmin * (1.0 - slack) > hi1) return true;
    for (double w : W)
      if (v * w * (1.0 + slack) >= lo1 && v * w * (1.0 - slack) <= hi1) return false;
    return true;
  };
  *reason = 0;
  for (size_t cell = 0; cell < ncells; ++cell) {
    const double* x[8];
    for (int v = 0; v < 8; ++v) x[v] = xv + 3 * (size_t)vert(cell, v);
    double J[9];   // J[i * 3 + d]: component i of the edge along reference axis d
    for (int i = 0; i < 3; ++i) {
      const double e[3] = {x[1][i] - x[0][i], x[2][i] - x[0][i], x[4][i] - x[0][i]};
      // x1-x0 == x3-x2 == x5-x4 == x7-x6, x2-x0 == x3-x1 == x6-x4 == x7-x5, x4-x0 == x5-x1 == x6-x2 == x7-x3
      if (!(x[3][i] - x[2][i] == e[0] && x[5][i] - x[4][i] == e[0] && x[7][i] - x[6][i] == e[0] &&
            x[3][i] - x[1][i] == e[1] && x[6][i] - x[4][i] == e[1] && x[7][i] - x[5][i] == e[1] &&
            x[5][i] - x[1][i] == e[2] && x[6][i] - x[2][i] == e[2] && x[7][i] - x[3][i] == e[2]))
        return *reason = 1, (int64_t)cell;
      for (int d = 0; d < 3; ++d) J[i * 3 + d] = e[d];
    }
    double det = J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
    if (!(det != 0.0) || !std::isfinite(det)) return *reason = 2, (int64_t)cell;
    const double idet = 1.0 / det;
    double Ji[9];
    Ji[0] = (J[4] * J[8] - J[5] * J[7]) * idet;
    Ji[1] = (J[2] * J[7] - J[1] * J[8]) * idet;
    Ji[2] = (J[1] * J[5] - J[2] * J[4]) * idet;
    Ji[3] = (J[5] * J[6] - J[3] * J[8]) * idet;
    Ji[4] = (J[0] * J[8] - J[2] * J[6]) * idet;
    Ji[5] = (J[2] * J[3] - J[0] * J[5]) * idet;
    Ji[6] = (J[3] * J[7] - J[4] * J[6]) * idet;
    Ji[7] = (J[1] * J[6] - J[0] * J[7]) * idet;
    Ji[8] = (J[0] * J[4] - J[1] * J[3]) * idet;
    if (use_fabs) det = std::fabs(det);
    static const int comp[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
    for (int m = 0; m < 6; ++m) {
      const int a = comp[m][0], b = comp[m][1];
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += (Ji[a * 3 + k] * det) * Ji[b * 3 + k];
      if (!std::isfinite(s)) return *reason = 2, (int64_t)cell;
      if (clamp && (cmap_clamped || !clamp_free(s))) return *reason = 3, (int64_t)cell;
      if (Gc) Gc[cell * 6 + m] = s;
    }
  }
  return -1;
}

// Per-cell geometry of a box (wf_op_create_box): the rule above on the box's implicit vertex lattice.  Returns false --
// the operator keeps per-point geometry -- unless every cell qualifies.
bool box_cell_geometry(int P, int nx, int ny, int nz, const double* xv, int use_fabs, int clamp, std::vector<double>& Gc)
{
  const size_t ncells = (size_t)nx * ny * nz;
  Gc.assign(ncells * 6, 0.0);
  auto vert = [&](size_t c, int v) {
    const size_t cx = c % nx, cy = (c / nx) % ny, cz = c / ((size_t)nx * ny);
    return (cx + (v & 1)) + (size_t)(nx + 1) * ((cy + ((v >> 1) & 1)) + (size_t)(ny + 1) * (cz + ((v >> 2) & 1)));
  };
  int reason;
  return hex_cell_geometry(P, ncells, xv, vert, use_fabs, clamp, Gc.data(), &reason) < 0;
}

void default_box_block(int P, const wf_tuning& tun, int* bx, int* by, int* bz)
{
  switch (P) {
    case 1: *bx = 4; *by = 4; *bz = 4; break;
    case 2: *bx = 3; *by = 3; *bz = 3; break;
    case 3: *bx = 4; *by = 2; *bz = 2; break;
    case 4: *bx = 5; *by = 2; *bz = 1; break;
    case 5: *bx = 7; *by = 1; *bz = 1; break;
    case 6: *bx = 5; *by = 1; *bz = 1; break;
    default: *bx = 4; *by = 1; *bz = 1; break;
  }
  if (tun.bx > 0 && tun.by > 0 && tun.bz > 0 && tun.bx * tun.by * tun.bz * (P + 1) * (P + 1) <= 256) {
    *bx = tun.bx;
    *by = tun.by;
    *bz = tun.bz;
  }
}

using OpPtr = std::unique_ptr<wf_op, void (*)(wf_op*)>;

// the common header of a new operator
OpPtr new_op(int kind, int P, int nd, int nq, int ncells, int ndofs, double c0, const wf_tuning* tuning)
{
  OpPtr op(new wf_op, free_op);
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

// what the geometry kernels take from the WF_FLAG_* bits
int fabs_flag(int flags) { return (flags & WF_FLAG_NO_FABS) ? 0 : 1; }
int clamp_flag(int flags) { return (flags & WF_FLAG_NO_CLAMP) ? 0 : 1; }

struct HexMesh {
  size_t ncells;
  int nverts;
  const double* xverts;
  const int32_t* geom_dofmap;
};

// Geometry of every cell at the n1^3 points of a 1-D rule, computed from the mesh into whichever of the device arrays
// d_G9[ncells][n1^3][9], d_G6blk (blocked by cells_per_batch(n1 - 1)) and d_detJ[ncells][n1^3] (det J * w) are given.
// The kernel is generic in the number of points per direction.
int mesh_geometry_rule(int n1, const double* h_pts, const double* h_wts, const HexMesh& mesh, int use_fabs, int clamp,
                       double* d_G9, double* d_G6blk, double* d_detJ)
{
  Scratch<double> d_x, d_pts, d_wts;
  Scratch<int32_t> d_gd;
  int rc;
  if ((rc = dev_upload(&d_x.p, mesh.xverts, (size_t)mesh.nverts * 3, nullptr)) != WF_OK) return rc;
  if ((rc = dev_upload(&d_gd.p, mesh.geom_dofmap, mesh.ncells * 8, nullptr)) != WF_OK) return rc;
  if ((rc = dev_upload(&d_pts.p, h_pts, (size_t)n1, nullptr)) != WF_OK) return rc;
  if ((rc = dev_upload(&d_wts.p, h_wts, (size_t)n1, nullptr)) != WF_OK) return rc;
  if ((rc = launch_geometry_hex(n1 - 1, (int)mesh.ncells, d_x.p, d_gd.p, d_pts.p, d_wts.p, use_fabs, clamp, d_G9, d_G6blk,
                                d_detJ, nullptr)) != WF_OK)
    return rc;
  WF_HIP_CHECK(hipDeviceSynchronize());
  return WF_OK;
}

// det J * w per cell and point of a dense mass with a square table, on the host: the caller's h_detJ (caller's point
// order), else computed from the mesh at the caller's rule into hd (*raw_points: the engine's point order)
int host_detJ(const wf_op_desc* desc, std::vector<double>& hd, const double** hsrc, bool* raw_points)
{
  *hsrc = desc->h_detJ;
  *raw_points = !desc->h_detJ;
  if (desc->h_detJ) return WF_OK;
  const int n = desc->nq1;
  Scratch<double> d_det;
  hd.resize((size_t)desc->ncells * n * n * n);
  int rc;
  if ((rc = dev_alloc(&d_det.p, hd.size(), nullptr)) != WF_OK) return rc;
  const HexMesh mesh{(size_t)desc->ncells, desc->nverts, desc->h_xverts, desc->h_geom_dofmap};
  if ((rc = mesh_geometry_rule(n, desc->h_qpts1, desc->h_qwts1, mesh, fabs_flag(desc->flags), 0, nullptr, nullptr, d_det.p)) != WF_OK)
    return rc;
  WF_HIP_CHECK(hipMemcpy(hd.data(), d_det.p, hd.size() * sizeof(double), hipMemcpyDeviceToHost));
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
  return dev_upload(&op->d_D, D.data(), D.size(), &op->device_bytes);
}

// Stages geometry given as G[slot][nd][3][3] (the reference layout, precomputation.hpp:46) into the blocked upper
// triangle d_G6blk, in slabs of 64 MiB to bound the temporary.  direct: the caller's array when it is in slot order
// already; otherwise fill_slot(slot, dst) writes the nd * 9 values of a slot (zeros for an empty one).
template <class FillSlot>
int stage_G9(int P, int CB, size_t nslots, const double* direct, FillSlot&& fill_slot, double* d_G6blk)
{
  const int n = P + 1, nd = n * n * n;
  const size_t slab_slots = std::max<size_t>(CB, (((size_t)64 << 20) / (nd * 9 * sizeof(double))) / CB * CB);
  Scratch<double> d_G9;
  int rc;
  if ((rc = dev_alloc(&d_G9.p, std::min(slab_slots, nslots) * nd * 9, nullptr)) != WF_OK) return rc;
  std::vector<double> slab;
  for (size_t s0 = 0; s0 < nslots; s0 += slab_slots) {
    const size_t ns = std::min(slab_slots, nslots - s0);
    const double* hsrc = direct ? direct + s0 * nd * 9 : nullptr;
    if (!hsrc) {
      slab.resize(ns * nd * 9);
      for (size_t q = 0; q < ns; ++q) fill_slot(s0 + q, &slab[q * nd * 9]);
      hsrc = slab.data();
    }
    WF_HIP_CHECK(hipMemcpy(d_G9.p, hsrc, ns * nd * 9 * sizeof(double), hipMemcpyHostToDevice));
    // slabs start on a batch boundary, so the packed destination is offset by whole batches
    if ((rc = launch_pack_G6(P, CB, (int)ns, d_G9.p, d_G6blk + (s0 / CB) * CB * nd * 6, nullptr)) != WF_OK) return rc;
    WF_HIP_CHECK(hipDeviceSynchronize());
  }
  return WF_OK;
}

// the three box marching kernels: work items = columns x z segments (common.h), which split into interior / interface
bool is_box_march(OpKernel k)
{
  return k == OpKernel::box_march || k == OpKernel::box_ksplit || k == OpKernel::box_owner;
}

// columns of a box marching operator: cells in pieces of bx x by, or the owner form's pieces of lattice lines
BoxColumns op_columns(const wf_op* op)
{
  return op->kernel == OpKernel::box_owner ? box_owner_columns(op->P, op->nx, op->ny, op->box.obx, op->box.oby)
                                           : box_columns(op->nx, op->ny, op->box.bx, op->box.by);
}

}  // namespace

extern "C" {

// ---- device runtime shims ------------------------------------------------
int wf_device_count(int* count)
{
  WF_REQUIRE(count != nullptr, "wf_device_count: null output");
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) {
    *count = 0;
    set_error(std::string("hipGetDeviceCount failed: ") + hipGetErrorString(e));
    return WF_ERR_NODEVICE;
  }
  return WF_OK;
}

int wf_set_device(int device)
{
  int count = 0;
  int rc = wf_device_count(&count);
  if (rc != WF_OK) return rc;
  if (device < 0 || device >= count) {
    // utils.hpp:30-34: "The number of MPI processes should be less or equal the number of available devices"
    set_error("wf_set_device: device " + std::to_string(device) + " not available (" + std::to_string(count)
              + " devices)");
    return WF_ERR_NODEVICE;
  }
  WF_HIP_CHECK(hipSetDevice(device));
  return WF_OK;
}

int wf_device_info(int device, char* name, size_t name_len, size_t* total_mem, int* num_cu)
{
  hipDeviceProp_t prop;
  WF_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  if (name && name_len) {
    std::strncpy(name, prop.name, name_len - 1);
    name[name_len - 1] = 0;
  }
  if (total_mem) *total_mem = prop.totalGlobalMem;
  if (num_cu) *num_cu = prop.multiProcessorCount;
  return WF_OK;
}

int wf_malloc(void** d_ptr, size_t bytes)
{
  WF_REQUIRE(d_ptr != nullptr, "wf_malloc: null output");
  *d_ptr = nullptr;
  if (bytes == 0) return WF_OK;
  WF_HIP_CHECK(hipMalloc(d_ptr, bytes));
  return WF_OK;
}
int wf_free(void* d_ptr)
{
  if (d_ptr) WF_HIP_CHECK(hipFree(d_ptr));
  return WF_OK;
}
int wf_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes)
{
  if (bytes) WF_HIP_CHECK(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
  return WF_OK;
}
int wf_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes)
{
  if (bytes) WF_HIP_CHECK(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
  return WF_OK;
}
int wf_memset(void* d_dst, int value, size_t bytes, void* stream)
{
  if (bytes) WF_HIP_CHECK(hipMemsetAsync(d_dst, value, bytes, (hipStream_t)stream));
  return WF_OK;
}
int wf_sync(void* stream)
{
  if (stream)
    WF_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  else
    WF_HIP_CHECK(hipDeviceSynchronize());
  return WF_OK;
}

// ---- geometry --------------------------------------------------------------
static int geometry_hex_rule(int n, const double* h_pts, const double* h_wts, int ncells, int nverts,
                             const double* h_xverts, const int32_t* h_geom_dofmap, int use_fabs, int clamp, double* h_G,
                             double* h_detJ, const char* who)
{
  if (!(ncells >= 0 && nverts >= 0 && h_xverts && h_geom_dofmap)) {
    set_error(std::string(who) + ": bad arguments");
    return WF_ERR_INVALID;
  }
  for (size_t e = 0; e < (size_t)ncells * 8; ++e)
    if (h_geom_dofmap[e] < 0 || h_geom_dofmap[e] >= nverts) {
      set_error(std::string(who) + ": vertex index out of range");
      return WF_ERR_INVALID;
    }
  const size_t nq = (size_t)n * n * n;
  Scratch<double> d_G, d_det;
  int rc;
  if (h_G && (rc = dev_alloc(&d_G.p, (size_t)ncells * nq * 9, nullptr)) != WF_OK) return rc;
  if (h_detJ && (rc = dev_alloc(&d_det.p, (size_t)ncells * nq, nullptr)) != WF_OK) return rc;
  if ((rc = mesh_geometry_rule(n, h_pts, h_wts, {(size_t)ncells, nverts, h_xverts, h_geom_dofmap}, use_fabs, clamp, d_G.p,
                               nullptr, d_det.p)) != WF_OK)
    return rc;
  if (h_G) WF_HIP_CHECK(hipMemcpy(h_G, d_G.p, (size_t)ncells * nq * 9 * sizeof(double), hipMemcpyDeviceToHost));
  if (h_detJ) WF_HIP_CHECK(hipMemcpy(h_detJ, d_det.p, (size_t)ncells * nq * sizeof(double), hipMemcpyDeviceToHost));
  return WF_OK;
}

int wf_geometry_hex(int P, int ncells, int nverts, const double* h_xverts, const int32_t* h_geom_dofmap,
                    int use_fabs, int clamp, double* h_G, double* h_detJ)
{
  if (P < 1 || P > kMaxDegree) {
    set_error("wf_geometry_hex: degree must be 1..7");
    return WF_ERR_UNSUPPORTED;
  }
  const int n = P + 1;
  std::vector<double> pts(n), wts(n);
  gll_points_weights(n, pts.data(), wts.data());
  return geometry_hex_rule(n, pts.data(), wts.data(), ncells, nverts, h_xverts, h_geom_dofmap, use_fabs, clamp, h_G,
                           h_detJ, "wf_geometry_hex");
}

int wf_geometry_hex_rule(int ncells, int nverts, const double* h_xverts, const int32_t* h_geom_dofmap, int nq1,
                         const double* h_points1, const double* h_weights1, int use_fabs, int clamp, double* h_G,
                         double* h_detJ)
{
  WF_REQUIRE(nq1 >= 1 && nq1 <= WF_MAX_QUAD_POINTS && h_points1 && h_weights1, "wf_geometry_hex_rule: bad rule");
  return geometry_hex_rule(nq1, h_points1, h_weights1, ncells, nverts, h_xverts, h_geom_dofmap, use_fabs, clamp, h_G,
                           h_detJ, "wf_geometry_hex_rule");
}

int wf_geometry_hex_cell(int P, int64_t ncells, int64_t nverts, const double* h_xverts, const int32_t* h_geom_dofmap,
                         int use_fabs, int clamp, double* h_Gc, int64_t* first_bad, int* reason)
{
  if (P < 1 || P > kMaxDegree) {
    set_error("wf_geometry_hex_cell: degree must be 1..7");
    return WF_ERR_UNSUPPORTED;
  }
  WF_REQUIRE(ncells >= 0 && nverts >= 0 && first_bad && reason && (ncells == 0 || (h_xverts && h_geom_dofmap)),
             "wf_geometry_hex_cell: bad arguments");
  for (size_t e = 0; e < (size_t)ncells * 8; ++e)
    WF_REQUIRE(h_geom_dofmap[e] >= 0 && h_geom_dofmap[e] < nverts, "wf_geometry_hex_cell: vertex index out of range");
  *first_bad = hex_cell_geometry(P, (size_t)ncells, h_xverts, [&](size_t c, int v) { return h_geom_dofmap[c * 8 + v]; },
                                 use_fabs, clamp, h_Gc, reason);
  return WF_OK;
}

}  // extern "C"

// ---- operators -------------------------------------------------------------
namespace {

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
  CallerFrame(const wf_op_desc* desc, int n) : xslow((desc->flags & WF_FLAG_TENSOR_X_SLOWEST) != 0), h_perm(desc->h_perm)
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
  // engine tensor position -> the caller's element-local index; null: the identity
  const int32_t* perm() const { return xslow ? eff_perm.data() : h_perm; }
  // point permutation of per-point input arrays of an m^3 rule: engine point q <- caller point qmap[q]
  std::vector<int32_t> qmap(int m) const
  {
    std::vector<int32_t> q((size_t)m * m * m);
    for (int k = 0; k < m; ++k)
      for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) q[i + m * (j + m * k)] = xslow ? (i * m + j) * m + k : i + m * (j + m * k);
    return q;
  }
};

// tensor-ordered dofmap in the caller's cell order (permute.hpp:10-27 when the caller's element ordering differs):
// *tdm is h_dofmap itself, or store
int tensor_dofmap(const wf_op_desc* desc, const CallerFrame& fr, int nd, std::vector<int32_t>& store, const int32_t** tdm)
{
  *tdm = desc->h_dofmap;
  if (!fr.perm() || desc->ncells == 0) return WF_OK;
  store.resize((size_t)desc->ncells * nd);
  int rc = wf_reorder_dofmap(desc->ncells, nd, fr.perm(), desc->h_dofmap, store.data());
  *tdm = store.data();
  return rc;
}

// ---- path 1: dense mass with a COLLOCATED rule (the quadrature points are the nodes, phi1 = identity: the GLL rule of
// demo/gpu_operator_monolithic/main.cpp:94-96 and of LinearGLL): Phi^T D Phi is the diagonal sum_cells det J w.
// It is assembled once and applied as y += m .* x (24 B/dof) -- the result of the dense evaluation up to the
// rounding of the six identity contractions.
bool mass_collocated(const wf_op_desc* desc, int n)
{
  for (int q = 0; q < n; ++q)
    for (int a2 = 0; a2 < n; ++a2)
      if (std::abs(desc->h_phi1[q * n + a2] - (q == a2 ? 1.0 : 0.0)) > 1e-14) return false;
  return true;
}

// Does the caller keep dofs in its vectors that no cell names (the dofs of deleted cells, padding)?  The gather /
// scatter kernels never touch them; the pre-assembled diagonal has m = 0 there, and y += m .* x would still turn
// whatever x holds in such an entry -- uninitialised memory, NaN -- into y.
bool has_unnamed_dofs(const wf_op_desc* desc, int nd)
{
  std::vector<char> named((size_t)desc->ndofs, 0);
  for (size_t e = 0; e < (size_t)desc->ncells * nd; ++e) named[desc->h_dofmap[e]] = 1;
  return std::find(named.begin(), named.end(), 0) != named.end();
}

int create_mass_diagonal(const wf_op_desc* desc, const CallerFrame& fr, wf_op* op)
{
  const int n = op->n, nd = op->nd;
  const size_t ncells = (size_t)desc->ncells;
  std::vector<double> hd;
  const double* hsrc;
  bool raw_points;
  int rc;
  if ((rc = host_detJ(desc, hd, &hsrc, &raw_points)) != WF_OK) return rc;
  std::vector<int32_t> qm = fr.qmap(n);
  if (raw_points)
    for (int q = 0; q < nd; ++q) qm[q] = q;
  const int32_t* perm = fr.perm();
  std::vector<double> md((size_t)desc->ndofs, 0.0);
  for (size_t c = 0; c < ncells; ++c)
    for (int l = 0; l < nd; ++l) {
      const int32_t dof = desc->h_dofmap[c * nd + (perm ? perm[l] : l)];   // tensor position l of cell c
      md[dof] += hsrc[c * nd + qm[l]];
    }
  if ((rc = dev_upload(&op->d_mdiag, md.data(), md.size(), &op->device_bytes)) != WF_OK) return rc;
  op->nq1 = n;
  op->diag_named_only = has_unnamed_dofs(desc, nd);
  op->kernel = OpKernel::diagonal;
  return WF_OK;
}

// ---- path 2: marching over lattice columns found in the caller's mesh (generic_plan.cpp): the default of the
// stiffness operator and of the dense mass with a square 1-D table ----

// engine point index (lattice frame of the cell, x fastest) -> the caller's point index, per orientation
struct PointMaps {
  const CallerFrame& fr;
  int n;
  std::vector<std::vector<int32_t>> maps = std::vector<std::vector<int32_t>>(48);
  const std::vector<int32_t>& operator()(int code)
  {
    auto& m = maps[code];
    if (m.empty()) {
      const std::vector<int32_t> qm = fr.qmap(n);
      m.resize((size_t)n * n * n);
      for (int k = 0; k < n; ++k)
        for (int j = 0; j < n; ++j)
          for (int i = 0; i < n; ++i) m[i + n * (j + n * k)] = qm[orient_local_index(code, n, i, j, k)];
    }
    return m;
  }
};

// stiffness geometry in slot order [item][layer][ly][lx]; missing cells stay zero (they contribute nothing)
// h_Gc: per-cell geometry on request (wf_tuning.geometry), [ncells][6] in the cells' own frames; uploaded as
// Gc[(item lz + layer) CB + cell][6] in the plan's frame, op->idx_geom already says which form reads it
int plan_stiffness_geometry(const wf_op_desc* desc, const CallerFrame& fr, const MarchPlan& plan, const double* h_Gc, wf_op* op)
{
  const int P = op->P, n = op->n, nd = op->nd, CB = op->plan.bx * op->plan.by;
  const size_t nslots = (size_t)plan.nitems * plan.lz * CB;
  int rc;
  if (h_Gc) {
    // G_c of a cell seen in the lattice frame, as h_G below: G'[a][b] = s_a s_b G[r_a][r_b].  Without fabs G_c carries
    // the sign of the cell's own det J, which is what the per-point path restores with orient_sign.
    if ((rc = upload_derivative_tables(op, true)) != WF_OK) return rc;
    static const int comp[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
    static const int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    std::vector<double> blk(nslots * 6, 0.0);
    for (size_t q = 0; q < nslots; ++q) {
      const int32_t c = plan.slot_cell[q];
      if (c < 0) continue;
      int ra[3], fl[3];
      orient_decode(plan.cell_orient[c], ra, fl);
      for (int m = 0; m < 6; ++m) {
        const int a = comp[m][0], b2 = comp[m][1];
        const double g = h_Gc[(size_t)c * 6 + sym[ra[a]][ra[b2]]];
        blk[q * 6 + m] = (fl[a] ^ fl[b2]) ? -g : g;
      }
    }
    if ((rc = dev_upload(&op->d_Gcell, blk.data(), blk.size(), &op->device_bytes)) != WF_OK) return rc;
    op->kernel = OpKernel::idx_march;
    return WF_OK;
  }
  if ((rc = upload_derivative_tables(op, false)) != WF_OK) return rc;
  const size_t g6 = nslots * nd * 6;
  if ((rc = dev_alloc(&op->d_G6blk, g6, &op->device_bytes)) != WF_OK) return rc;
  WF_HIP_CHECK(hipMemset(op->d_G6blk, 0, g6 * sizeof(double)));
  if (desc->h_G) {
    // G of a cell seen in the lattice frame: G'[a][b] = s_a s_b G[r_a][r_b] (r = the cell's own axis
    // along lattice axis a, s = -1 when reversed) at the relabelled point -- the operator
    // D^T G D is the same in every frame
    PointMaps point_map{fr, n};
    auto fill_slot = [&](size_t slot, double* dst) {
      const int32_t c = plan.slot_cell[slot];
      if (c < 0) {
        std::fill(dst, dst + (size_t)nd * 9, 0.0);
        return;
      }
      const int code = plan.cell_orient[c];
      const std::vector<int32_t>& pm = point_map(code);
      const double* gsrc = desc->h_G + (size_t)c * nd * 9;
      if (code == 0) {
        for (int pt = 0; pt < nd; ++pt) std::memcpy(dst + (size_t)pt * 9, gsrc + (size_t)pm[pt] * 9, 9 * sizeof(double));
        return;
      }
      int ra[3], fl[3];
      orient_decode(code, ra, fl);
      for (int pt = 0; pt < nd; ++pt) {
        const double* g9 = gsrc + (size_t)pm[pt] * 9;
        for (int a = 0; a < 3; ++a)
          for (int b2 = 0; b2 < 3; ++b2) dst[pt * 9 + a * 3 + b2] = ((fl[a] ^ fl[b2]) ? -1.0 : 1.0) * g9[ra[a] * 3 + ra[b2]];
      }
    };
    if ((rc = stage_G9(P, CB, nslots, nullptr, fill_slot, op->d_G6blk)) != WF_OK) return rc;
  } else {
    // one geometry thread per (present cell, point), written to the cell's slot; a cell is handed
    // over with its vertices relabelled into the lattice frame
    const size_t ncells = (size_t)desc->ncells;
    std::vector<int32_t> gd, slot_of;
    std::vector<uint8_t> sign;
    gd.reserve(ncells * 8);
    slot_of.reserve(ncells);
    sign.reserve(ncells);
    for (size_t q = 0; q < nslots; ++q) {
      const int32_t c = plan.slot_cell[q];
      if (c < 0) continue;
      const int code = plan.cell_orient[c];
      const int32_t* gsrc = desc->h_geom_dofmap + (size_t)c * 8;
      for (int v = 0; v < 8; ++v) gd.push_back(gsrc[orient_local_index(code, 2, v & 1, (v >> 1) & 1, (v >> 2) & 1)]);
      slot_of.push_back((int32_t)q);
      sign.push_back((uint8_t)(int8_t)orient_sign(code));
    }
    Scratch<double> d_x, d_pts, d_wts;
    Scratch<int32_t> d_gd, d_slot;
    Scratch<uint8_t> d_sign;
    if ((rc = dev_upload(&d_x.p, desc->h_xverts, (size_t)desc->nverts * 3, nullptr)) != WF_OK) return rc;
    if ((rc = dev_upload(&d_gd.p, gd.data(), gd.size(), nullptr)) != WF_OK) return rc;
    if ((rc = dev_upload(&d_slot.p, slot_of.data(), slot_of.size(), nullptr)) != WF_OK) return rc;
    if ((rc = dev_upload(&d_sign.p, sign.data(), sign.size(), nullptr)) != WF_OK) return rc;
    if ((rc = upload_tables(P, d_pts, d_wts)) != WF_OK) return rc;
    if ((rc = launch_geometry_hex_slots(P, CB, (int)slot_of.size(), d_x.p, d_gd.p, d_slot.p, d_sign.p, d_pts.p, d_wts.p,
                                        fabs_flag(desc->flags), clamp_flag(desc->flags), op->d_G6blk, nullptr)) != WF_OK)
      return rc;
  }
  op->kernel = OpKernel::idx_march;
  return WF_OK;
}

// dense mass: det J * w at the M^3 points of the rule (M = nq1) in the blocked slot layout [item * lz + layer][qk][t],
// t = slot_in_layer * M^2 + qj M + qi; empty slots zero
int plan_mass_detJ(const wf_op_desc* desc, const CallerFrame& fr, const MarchPlan& plan, wf_op* op)
{
  const int n = op->n, M = desc->nq1, nq = M * M * M, CB = op->plan.bx * op->plan.by, NTq = CB * M * M;
  const size_t nslots = (size_t)plan.nitems * plan.lz * CB;
  // det J * w per cell and point, host copy in the caller's cell order and point order
  std::vector<double> hd;
  const double* hsrc;
  bool raw_points;   // hd is in the engine's (raw cell frame) point order already
  int rc;
  if ((rc = host_detJ(desc, hd, &hsrc, &raw_points)) != WF_OK) return rc;
  PointMaps point_map{fr, M};
  std::vector<double> blk(nslots * nq, 0.0);
  for (size_t q = 0; q < nslots; ++q) {
    const int32_t c = plan.slot_cell[q];
    if (c < 0) continue;
    const int code = plan.cell_orient[c];
    const size_t sub = q / CB, sl = q % CB;
    const double* src = hsrc + (size_t)c * nq;
    for (int k = 0; k < M; ++k)
      for (int ji = 0; ji < M * M; ++ji) {
        const int l = ji + M * M * k;
        const int rp = raw_points ? orient_local_index(code, M, l % M, (l / M) % M, l / (M * M)) : point_map(code)[l];
        blk[(sub * M + k) * NTq + sl * M * M + ji] = src[rp];
      }
  }
  // A non-symmetric 1-D table kept the caller's frames (normalise in create_on_plan).
  if ((rc = dev_upload(&op->d_detJ, blk.data(), blk.size(), &op->device_bytes)) != WF_OK) return rc;
  if ((rc = dev_upload(&op->d_phi1, desc->h_phi1, (size_t)M * n, &op->device_bytes)) != WF_OK) return rc;
  for (int q = 0; q < M * n; ++q) op->dm.v[q] = desc->h_phi1[q];
  op->nq1 = M;
  op->nq = nq;
  op->kernel = OpKernel::mass_march;
  return WF_OK;
}

// leaves op untouched (no kernel) when the mesh does not tile into lattice columns: the batch kernels take it
// h_Gc: the stiffness operator with per-cell geometry (on request; op->idx_geom is set): any fill is adopted, and a mesh
// that does not tile is an error
int create_on_plan(const wf_op_desc* desc, const CallerFrame& fr, const int32_t* tdm, bool mass, const double* h_Gc, wf_op* op)
{
  const int P = op->P, n = op->n;
  const wf_tuning& tun = op->tun;
  const int pkind = mass ? OP_KIND_MASS : OP_KIND_STIFFNESS;
  const int M = mass ? desc->nq1 : n;   // points of the 1-D table
  int BX = tun.bx, BY = tun.by;   // a compiled cross-section of the k-split / the dense-mass kernel, else the default
  if (!mass) {
    march_idx_shape(pkind, P, &BX, &BY);
  } else if (!mass_march_shape(P, M, &BX, &BY)) {
    set_error("wf_op_create: WF_KERNEL_FORCE_MASS_MARCH: no marching kernel is compiled for (P, nq1) = (" + std::to_string(P)
              + ", " + std::to_string(M) + ")");
    return WF_ERR_UNSUPPORTED;
  }
  // layers per work item: as many as the kernel's LDS budget per workgroup allows, at most 16
  int lz_max = mass ? 32 : 16;   // (the dense-mass kernel streams its index table: no LDS limit)
  while (!mass && lz_max > 1 && march_idx_lds_bytes(pkind, P, BX, BY, lz_max, op->idx_geom) > march_idx_lds_budget(pkind, P, BX, BY, op->idx_geom))
    --lz_max;
  // A cell may be looked at with an axis reversed only if the 1-D table reads the same backwards,
  // phi1[M-1-q][n-1-a] == phi1[q][a] (true for every symmetric node / point set; the GLL derivative
  // matrix of the stiffness operator has the matching antisymmetry by construction).
  bool normalise = tun.orient == 0;
  if (mass)
    for (int q = 0; q < M && normalise; ++q)
      for (int a2 = 0; a2 < n; ++a2)
        if (std::abs(desc->h_phi1[q * n + a2] - desc->h_phi1[(M - 1 - q) * n + (n - 1 - a2)]) > 1e-13) normalise = false;
  MarchPlan plan;
  int rc;
  if ((rc = build_march_plan(P, (size_t)desc->ncells, tdm, BX, BY, lz_max, std::max(0, tun.lz), normalise, &plan)) != WF_OK) return rc;
  // mostly empty columns (a mesh one cell wide, a mesh shattered into tiny lattice components): the
  // marching kernel would read geometry for every slot -- batch kernel instead (per-cell geometry is 48 B per slot)
  const bool forced = tun.kernel == WF_KERNEL_FORCE_MARCH || tun.kernel == WF_KERNEL_FORCE_MASS_MARCH || h_Gc;
  if (plan.ok && plan.fill < kMinPlanFill && !forced) plan.ok = false;
  if (!plan.ok && mass && M != n) {   // a rectangular table is here on request only
    set_error("wf_op_create: WF_KERNEL_FORCE_MASS_MARCH: the mesh does not tile into lattice columns ((P, nq1) = ("
              + std::to_string(P) + ", " + std::to_string(M) + "))");
    return WF_ERR_UNSUPPORTED;
  }
  if (!plan.ok && h_Gc) {
    set_error("wf_op_create: WF_GEOMETRY_PER_CELL: the mesh does not tile into lattice columns");
    return WF_ERR_UNSUPPORTED;
  }
  if (!plan.ok) return WF_OK;

  op->plan = MarchPlanDev{plan.nitems, plan.lz, plan.tile_size, BX, BY};
  op->plan_patterns = plan.npatterns;
  op->plan_reoriented = plan.reoriented;
  op->plan_fill = plan.fill;
  if ((rc = dev_upload(&op->plan.d_item_base, plan.item_base.data(), plan.item_base.size(), &op->device_bytes)) != WF_OK) return rc;
  if ((rc = dev_upload(&op->plan.d_item_pattern, plan.item_pattern.data(), plan.item_pattern.size(), &op->device_bytes)) != WF_OK) return rc;
  if ((rc = dev_upload(&op->plan.d_item_layers, plan.item_layers.data(), plan.item_layers.size(), &op->device_bytes)) != WF_OK) return rc;
  if ((rc = dev_upload(&op->plan.d_pat_off, plan.pat_off.data(), plan.pat_off.size(), &op->device_bytes)) != WF_OK) return rc;
  if ((rc = mass ? plan_mass_detJ(desc, fr, plan, op) : plan_stiffness_geometry(desc, fr, plan, h_Gc, op)) != WF_OK) return rc;
  WF_HIP_CHECK(hipDeviceSynchronize());
  return WF_OK;
}

// wf_tuning.geometry = WF_GEOMETRY_PER_CELL on wf_op_create (stiffness, ncells > 0): what else the request allows, the
// per-cell geometry h_Gc [ncells][6] in the cells' own frames and the form that will read it (op->idx_geom).  Host only;
// the order of the checks decides which error a bad request reports.
int choose_idx_cell_geometry(const wf_op_desc* desc, bool have_mesh, wf_op* op, std::vector<double>& h_Gc)
{
  const wf_tuning& tun = op->tun;
  const int P = op->P;
  if (P > 4) {
    set_error("wf_op_create: WF_GEOMETRY_PER_CELL: the dofmap kernel has per-cell forms at degrees 1..4 (degree "
              + std::to_string(P) + " runs the k-split kernel, per-point geometry only)");
    return WF_ERR_UNSUPPORTED;
  }
  if (desc->h_G) {
    set_error("wf_op_create: WF_GEOMETRY_PER_CELL: per-cell geometry is derived from the mesh; h_G must be NULL");
    return WF_ERR_UNSUPPORTED;
  }
  WF_REQUIRE(have_mesh, "wf_op_create: WF_GEOMETRY_PER_CELL needs the mesh (h_xverts, h_geom_dofmap)");
  WF_REQUIRE(tun.kernel == WF_KERNEL_AUTO || tun.kernel == WF_KERNEL_FORCE_MARCH,
             "wf_op_create: WF_GEOMETRY_PER_CELL: wf_tuning.kernel must be AUTO or FORCE_MARCH (only the marching kernel on "
             "lattice columns reads per-cell geometry)");
  WF_REQUIRE(tun.update >= WF_UPDATE_AUTO && tun.update <= WF_UPDATE_OWNER, "wf_op_create: wf_tuning.update out of range");
  if (tun.update == WF_UPDATE_OWNER) {
    set_error("wf_op_create: WF_GEOMETRY_PER_CELL: the owner update needs the box's implicit lattice (wf_op_create_box)");
    return WF_ERR_UNSUPPORTED;
  }
  WF_REQUIRE(tun.metric >= WF_METRIC_AUTO && tun.metric <= WF_METRIC_AXES, "wf_op_create: wf_tuning.metric out of range");
  h_Gc.assign((size_t)desc->ncells * 6, 0.0);
  int reason = 0;
  const int32_t* gd = desc->h_geom_dofmap;
  const int64_t bad = hex_cell_geometry(P, (size_t)desc->ncells, desc->h_xverts, [&](size_t c, int v) { return gd[c * 8 + v]; },
                                        fabs_flag(desc->flags), clamp_flag(desc->flags), h_Gc.data(), &reason);
  if (bad >= 0) {
    static const char* kWhy[4] = {"", "is not affine (its edge vectors along a reference axis differ)",
                                  "is degenerate (det J zero or not finite)",
                                  "has geometry on which the -1/0/1 clamp takes effect (WF_FLAG_NO_CLAMP turns it off)"};
    set_error("wf_op_create: WF_GEOMETRY_PER_CELL: cell " + std::to_string(bad) + " " + kWhy[reason]);
    return WF_ERR_INVALID;
  }
  // metric: the separable (axes) form when every G_c is diagonal -- off-diagonals exactly 0, either sign.  Taking a cell
  // into the plan's frame permutes and negates components, so the cells' own frames decide.
  bool diagonal = true;
  size_t c = 0;
  for (; c < h_Gc.size() && diagonal; c += 6) diagonal = h_Gc[c + 1] == 0.0 && h_Gc[c + 2] == 0.0 && h_Gc[c + 4] == 0.0;
  if (tun.metric == WF_METRIC_AXES && !diagonal) {
    set_error("wf_op_create: axes metric requested but the G_c of cell " + std::to_string(c / 6 - 1)
              + " has a non-zero off-diagonal");
    return WF_ERR_INVALID;
  }
  op->idx_geom = diagonal && tun.metric != WF_METRIC_FULL ? MarchGeom::cell_axes : MarchGeom::cell;
  return WF_OK;
}

// ---- path 3: the batch kernels ----

// Internal cell order: cells are summed independently, so the operator may visit
// them in any order.  Sorting by the smallest dof of each cell puts cells that
// share dofs into the same workgroup batch whatever order the caller's mesh has
// (a randomly ordered cfg2 mesh: 0.46 ms unsorted -> the 0.31 ms of the
// lexicographic order).  wf_tuning.keep_cell_order keeps the caller's order.
// Returns whether the order is the caller's.
bool batch_cell_order(const wf_op_desc* desc, int nd, bool keep, std::vector<int32_t>& cperm)
{
  const size_t ncells = (size_t)desc->ncells;
  cperm.resize(ncells);
  for (size_t c = 0; c < ncells; ++c) cperm[c] = (int32_t)c;
  if (!keep && ncells > 1) {
    std::vector<int32_t> key(ncells);
    for (size_t c = 0; c < ncells; ++c) key[c] = *std::min_element(desc->h_dofmap + c * nd, desc->h_dofmap + (c + 1) * nd);
    std::stable_sort(cperm.begin(), cperm.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
  }
  for (size_t c = 0; c < ncells; ++c)
    if (cperm[c] != (int32_t)c) return false;
  return true;
}

// the caller's per-cell arrays in the internal cell order and the engine's point order (copies only where they differ)
struct BatchInputs {
  std::vector<int32_t> cperm, p_geom;
  std::vector<double> p_detJ;
  bool identity_cells = true;
  bool have_mesh = false;
  HexMesh mesh{};
  const double* h_detJ = nullptr;
};

// Order-fixed accumulation: the plan of the order contract (wf_ordered_slots on the CALLER's dofmap, so neither the
// internal cell order nor the tensor permutation enters the summation order), the slot table carried into the internal
// cell order and the engine's tensor order, and the scratch v.
int build_ordered_plan(const wf_op_desc* desc, const CallerFrame& fr, const std::vector<int32_t>& cperm, wf_op* op)
{
  const int nd = op->nd;
  const size_t ncells = (size_t)desc->ncells;
  std::vector<int32_t> row_off((size_t)desc->ndofs + 1), slot(ncells * nd), tslot(ncells * nd);
  int rc;
  if ((rc = wf_ordered_slots((int64_t)ncells, nd, desc->ndofs, desc->h_dofmap, row_off.data(), slot.data())) != WF_OK) return rc;
  const int32_t* perm = fr.perm();
  for (size_t c = 0; c < ncells; ++c)
    for (int l = 0; l < nd; ++l) tslot[c * nd + l] = slot[(size_t)cperm[c] * nd + (perm ? perm[l] : l)];
  if ((rc = dev_upload(&op->d_slot, tslot.data(), tslot.size(), &op->device_bytes)) != WF_OK) return rc;
  if ((rc = dev_upload(&op->d_row_off, row_off.data(), row_off.size(), &op->device_bytes)) != WF_OK) return rc;
  return dev_alloc(&op->d_v, ncells * nd, &op->device_bytes);
}

void free_ordered_plan(wf_op* op)
{
  const size_t entries = (size_t)op->ncells * op->nd;
  op->device_bytes -= entries * (sizeof(int32_t) + sizeof(double)) + ((size_t)op->ndofs + 1) * sizeof(int32_t);
  (void)hipFree(op->d_slot);
  (void)hipFree(op->d_row_off);
  (void)hipFree(op->d_v);
  op->d_slot = op->d_row_off = nullptr;
  op->d_v = nullptr;
}

int batch_stiffness(const wf_op_desc* desc, const CallerFrame& fr, const BatchInputs& in, bool no_unique, wf_op* op)
{
  const int P = op->P, n = op->n, nd = op->nd, CB = cells_per_batch(P);
  const size_t ncells = (size_t)desc->ncells, nbatch = (ncells + CB - 1) / CB;
  int rc;
  // batch-unique dof lists (WF_KERNEL_FORCE_ELEMENTWISE keeps the element-wise scatter for comparison)
  const bool unique = !no_unique && ncells > 0 && !op->ordered;
  if (unique && (rc = build_unique_lists(op, ncells, nd, CB)) != WF_OK) return rc;
  op->kernel = op->ordered ? OpKernel::ordered_stiffness : unique ? OpKernel::generic_unique : OpKernel::generic_elementwise;
  const size_t g6 = nbatch * CB * nd * 6;
  if ((rc = dev_alloc(&op->d_G6blk, g6, &op->device_bytes)) != WF_OK) return rc;
  if (g6) WF_HIP_CHECK(hipMemset(op->d_G6blk, 0, g6 * sizeof(double)));
  if (desc->h_G) {
    const bool direct = in.identity_cells && !fr.xslow;
    const std::vector<int32_t> qm = fr.qmap(n);
    auto fill_cell = [&](size_t c, double* dst) {
      const double* gsrc = desc->h_G + (size_t)in.cperm[c] * nd * 9;
      for (int q = 0; q < nd; ++q) std::memcpy(dst + (size_t)q * 9, gsrc + (size_t)qm[q] * 9, 9 * sizeof(double));
    };
    return stage_G9(P, CB, ncells, direct ? desc->h_G : nullptr, fill_cell, op->d_G6blk);
  }
  if (in.have_mesh) {
    std::vector<double> pts(n), wts(n);
    gll_points_weights(n, pts.data(), wts.data());
    return mesh_geometry_rule(n, pts.data(), wts.data(), in.mesh, fabs_flag(desc->flags), clamp_flag(desc->flags), nullptr, op->d_G6blk, nullptr);
  }
  if (ncells) {
    set_error("wf_op_create: stiffness needs h_G or the mesh (h_xverts, h_geom_dofmap)");
    return WF_ERR_INVALID;
  }
  return WF_OK;
}

// mass operators: detJ[ncells][nq]
int batch_mass(const wf_op_desc* desc, const BatchInputs& in, bool no_unique, wf_op* op)
{
  const int P = op->P, n = op->n, nd = op->nd;
  const size_t ncells = (size_t)desc->ncells;
  const wf_tuning& tun = op->tun;
  const bool dense = desc->kind == WF_OP_MASS_DENSE;
  int rc, nq1 = n;
  if (dense) {
    WF_REQUIRE(desc->h_phi1 && desc->nq1 >= 1 && desc->nq1 <= 16, "wf_op_create: dense mass needs phi1[nq1][P+1]");
    WF_REQUIRE(desc->h_detJ || (in.have_mesh && desc->h_qpts1 && desc->h_qwts1),
               "wf_op_create: dense mass needs h_detJ[ncells][nq1^3] or the mesh and the 1-D rule (h_qpts1, h_qwts1)");
    nq1 = desc->nq1;
    if ((rc = dev_upload(&op->d_phi1, desc->h_phi1, (size_t)nq1 * n, &op->device_bytes)) != WF_OK) return rc;
  }
  op->nq1 = nq1;
  op->nq = nq1 * nq1 * nq1;
  // square tables (nq1 == P+1): column-thread kernel, batches of cells_per_batch(P)
  const bool square = dense && nq1 == n && tun.kernel != WF_KERNEL_FORCE_MASS_ANY && !op->ordered;
  const int CBm = (dense && !square) ? mass_dense_cells_per_batch(std::max(n, nq1)) : cells_per_batch(P);
  // dense mass: the unique-dof tile pays off only for small elements (measured at 10 M dofs:
  // P2 0.80 -> 0.68 ms, P4 0.43 -> 0.46 ms, P6 0.34 -> 0.41 ms)
  // lumped mass: the diagonal is pre-assembled below unless the caller asks for the
  // reference's element-wise sequence
  const bool elementwise = !dense && (desc->flags & WF_FLAG_MASS_ELEMENTWISE);
  const bool want = elementwise || (dense && (P <= 3 || square));
  const bool unique = want && !no_unique && ncells > 0 && !op->ordered;
  if (unique && (rc = build_unique_lists(op, ncells, nd, CBm)) != WF_OK) return rc;

  if (desc->h_detJ) {
    if ((rc = dev_upload(&op->d_detJ, in.h_detJ, ncells * op->nq, &op->device_bytes)) != WF_OK) return rc;
  } else if (in.have_mesh) {
    // det J * w at the caller's tensor rule (precompute.hpp:49-116, mass.hpp:35-39); lumped mass: at the GLL nodes
    std::vector<double> pts(n), wts(n);
    if (!dense) gll_points_weights(n, pts.data(), wts.data());
    if ((rc = dev_alloc(&op->d_detJ, ncells * op->nq, &op->device_bytes)) != WF_OK) return rc;
    if ((rc = mesh_geometry_rule(nq1, dense ? desc->h_qpts1 : pts.data(), dense ? desc->h_qwts1 : wts.data(), in.mesh,
                                 fabs_flag(desc->flags), 0, nullptr, nullptr, op->d_detJ)) != WF_OK)
      return rc;
  } else if (ncells) {
    set_error("wf_op_create: mass needs h_detJ or the mesh (h_xverts, h_geom_dofmap)");
    return WF_ERR_INVALID;
  }
  if (dense) {
    op->kernel = op->ordered ? OpKernel::ordered_mass : square && unique ? OpKernel::mass_column : OpKernel::mass_any;
    return WF_OK;
  }
  if (elementwise) {
    op->kernel = op->ordered ? OpKernel::ordered_lumped : unique ? OpKernel::lumped_unique : OpKernel::lumped_elementwise;
    return WF_OK;
  }
  // A lumped mass is a diagonal: assemble m = M 1 once with the reference's own
  // sequence (gather 1, * detJ, scatter-add; spectral_mass.hpp:84-89) and apply it as
  // y += m .* x -- 24 B/dof instead of 8 nq + 4 nd per cell + 16 per dof.
  Scratch<double> d_ones;
  if ((rc = dev_alloc(&d_ones.p, (size_t)op->ndofs, nullptr)) != WF_OK) return rc;
  if ((rc = dev_alloc(&op->d_mdiag, (size_t)op->ndofs, &op->device_bytes)) != WF_OK) return rc;
  if (op->ndofs) {
    if ((rc = wf_fill(op->ndofs, 1.0, d_ones.p, nullptr)) != WF_OK) return rc;
    WF_HIP_CHECK(hipMemset(op->d_mdiag, 0, (size_t)op->ndofs * sizeof(double)));
    // WF_FLAG_ORDERED: the same sequence through the two ordered passes, so that m is bitwise reproducible
    if (ncells && op->ordered) {
      if ((rc = launch_mass_lumped_ordered((int64_t)ncells * nd, op->d_dofmap, op->d_slot, op->d_detJ, d_ones.p, op->d_v, nullptr)) != WF_OK)
        return rc;
      if ((rc = wf_segment_sum_add(op->ndofs, op->d_row_off, op->d_v, op->d_mdiag, nullptr)) != WF_OK) return rc;
    } else if (ncells && (rc = launch_mass_lumped((int64_t)ncells * nd, op->d_dofmap, op->d_detJ, d_ones.p, op->d_mdiag, nullptr)) != WF_OK) {
      return rc;
    }
    WF_HIP_CHECK(hipDeviceSynchronize());
  }
  if (op->ordered) free_ordered_plan(op);
  op->device_bytes -= ncells * nd * sizeof(double);
  (void)hipFree(op->d_detJ);
  op->d_detJ = nullptr;
  op->diag_named_only = has_unnamed_dofs(desc, nd);
  op->kernel = OpKernel::diagonal;
  return WF_OK;
}

int create_batch(const wf_op_desc* desc, const CallerFrame& fr, const int32_t* tdm, wf_op* op)
{
  const int n = op->n, nd = op->nd;
  const size_t ncells = (size_t)desc->ncells;
  const bool no_unique = op->tun.kernel == WF_KERNEL_FORCE_ELEMENTWISE;
  BatchInputs in;
  in.identity_cells = batch_cell_order(desc, nd, op->tun.keep_cell_order != 0, in.cperm);
  in.have_mesh = desc->h_xverts && desc->h_geom_dofmap;
  in.mesh = {ncells, desc->nverts, desc->h_xverts, desc->h_geom_dofmap};
  in.h_detJ = desc->h_detJ;
  if (!in.identity_cells && in.have_mesh) {
    in.p_geom.resize(ncells * 8);
    for (size_t c = 0; c < ncells; ++c)
      std::memcpy(&in.p_geom[c * 8], desc->h_geom_dofmap + (size_t)in.cperm[c] * 8, 8 * sizeof(int32_t));
    in.mesh.geom_dofmap = in.p_geom.data();
  }
  if (desc->h_detJ && (!in.identity_cells || fr.xslow)) {
    const int mq = desc->kind == WF_OP_MASS_DENSE ? desc->nq1 : n;
    WF_REQUIRE(mq >= 1 && mq <= 16, "wf_op_create: bad nq1");
    const size_t nqm = (size_t)mq * mq * mq;
    const std::vector<int32_t> qm = fr.qmap(mq);
    in.p_detJ.resize(ncells * nqm);
    for (size_t c = 0; c < ncells; ++c) {
      const double* src = desc->h_detJ + (size_t)in.cperm[c] * nqm;
      for (size_t q = 0; q < nqm; ++q) in.p_detJ[c * nqm + q] = src[qm[q]];
    }
    in.h_detJ = in.p_detJ.data();
  }
  int rc;
  {
    std::vector<int32_t> sorted;
    const int32_t* src = tdm;
    if (!in.identity_cells) {
      sorted.resize(ncells * nd);
      for (size_t c = 0; c < ncells; ++c) std::memcpy(&sorted[c * nd], tdm + (size_t)in.cperm[c] * nd, nd * sizeof(int32_t));
      src = sorted.data();
    }
    if ((rc = dev_upload(&op->d_dofmap, src, ncells * nd, &op->device_bytes)) != WF_OK) return rc;
  }
  if ((rc = upload_derivative_tables(op, false)) != WF_OK) return rc;
  if (op->ordered && (rc = build_ordered_plan(desc, fr, in.cperm, op)) != WF_OK) return rc;
  rc = desc->kind == WF_OP_STIFFNESS ? batch_stiffness(desc, fr, in, no_unique, op) : batch_mass(desc, in, no_unique, op);
  if (rc != WF_OK) return rc;
  WF_HIP_CHECK(hipDeviceSynchronize());
  return WF_OK;
}

}  // namespace

extern "C" {

int wf_op_create(const wf_op_desc* desc, wf_op** out)
{
  WF_REQUIRE(desc && out, "wf_op_create: null argument");
  *out = nullptr;
  const int P = desc->degree;
  if (P < 1 || P > kMaxDegree) {
    set_error("wf_op_create: degree must be 1..7 (hexahedron)");   // mass.hpp:91-92 "Not implemented"
    return WF_ERR_UNSUPPORTED;
  }
  WF_REQUIRE(desc->kind == WF_OP_STIFFNESS || desc->kind == WF_OP_MASS_LUMPED || desc->kind == WF_OP_MASS_DENSE,
             "wf_op_create: unknown operator kind");
  WF_REQUIRE(desc->ncells >= 0 && desc->ndofs >= 0, "wf_op_create: negative size");
  WF_REQUIRE(desc->h_dofmap || desc->ncells == 0, "wf_op_create: dofmap missing");
  const int n = P + 1, nd = n * n * n;
  const size_t ncells = (size_t)desc->ncells;
  const bool have_mesh = desc->h_xverts && desc->h_geom_dofmap;

  // host-side validation of every index the kernels will dereference
  for (size_t e = 0; e < ncells * nd; ++e)
    WF_REQUIRE(desc->h_dofmap[e] >= 0 && desc->h_dofmap[e] < desc->ndofs, "wf_op_create: dofmap entry out of range");
  if (desc->h_perm) {
    std::vector<char> seen(nd, 0);
    for (int k = 0; k < nd; ++k) {
      WF_REQUIRE(desc->h_perm[k] >= 0 && desc->h_perm[k] < nd && !seen[desc->h_perm[k]],
                 "wf_op_create: perm is not a permutation");
      seen[desc->h_perm[k]] = 1;
    }
  }
  if (have_mesh)
    for (size_t e = 0; e < ncells * 8; ++e)
      WF_REQUIRE(desc->h_geom_dofmap[e] >= 0 && desc->h_geom_dofmap[e] < desc->nverts,
                 "wf_op_create: vertex index out of range");

  const CallerFrame fr(desc, n);
  OpPtr op = new_op(desc->kind, P, nd, nd, desc->ncells, desc->ndofs, desc->c0, desc->tuning);
  const wf_tuning& tun = op->tun;
  // order-fixed accumulation: one form per operator kind, always on the cell batches -- there is no kernel to choose
  op->ordered = (desc->flags & WF_FLAG_ORDERED) != 0;
  if (op->ordered) {
    wf_tuning rest = tun;
    rest.keep_cell_order = 0;
    const wf_tuning none{};
    WF_REQUIRE(std::memcmp(&rest, &none, sizeof(wf_tuning)) == 0,
               "wf_op_create: WF_FLAG_ORDERED takes no wf_tuning field other than keep_cell_order");
  }

  WF_REQUIRE(tun.kernel != WF_KERNEL_FORCE_MASS_MARCH || desc->kind == WF_OP_MASS_DENSE,
             "wf_op_create: WF_KERNEL_FORCE_MASS_MARCH applies to the dense mass only");
  // the lattice-column plan serves the stiffness operator and the dense mass: with a square 1-D table by default, with
  // a rectangular one on request (WF_KERNEL_FORCE_MASS_MARCH)
  const bool plan_stiffness = desc->kind == WF_OP_STIFFNESS;
  const bool mass_table = desc->kind == WF_OP_MASS_DENSE && desc->nq1 >= 1 && desc->h_phi1
                          && (desc->h_detJ || (have_mesh && desc->h_qpts1 && desc->h_qwts1));
  const bool plan_mass = mass_table && (desc->nq1 == n || tun.kernel == WF_KERNEL_FORCE_MASS_MARCH);
  const bool force_batch = tun.kernel == WF_KERNEL_FORCE_BATCH || tun.kernel == WF_KERNEL_FORCE_ELEMENTWISE
                           || tun.kernel == WF_KERNEL_FORCE_MASS_ANY;
  int rc;
  // a collocated dense mass is a diagonal; a wf_tuning kernel hint keeps the dense kernels
  if (plan_mass && tun.kernel == WF_KERNEL_AUTO && ncells > 0 && !op->ordered && mass_collocated(desc, n)) {
    rc = create_mass_diagonal(desc, fr, op.get());
  } else {
    std::vector<int32_t> tdm_store;
    const int32_t* tdm = nullptr;
    rc = tensor_dofmap(desc, fr, nd, tdm_store, &tdm);
    // per-cell geometry of the stiffness operator, on request: decided on the host before the first device allocation
    std::vector<double> h_Gc;
    const bool per_cell = plan_stiffness && tun.geometry == WF_GEOMETRY_PER_CELL && ncells > 0 && !op->ordered;
    if (rc == WF_OK && per_cell) rc = choose_idx_cell_geometry(desc, have_mesh, op.get(), h_Gc);
    if (rc == WF_OK && (plan_stiffness || plan_mass) && !force_batch && !op->ordered && ncells > 0) {
      if (plan_stiffness)
        WF_REQUIRE(desc->h_G || have_mesh, "wf_op_create: stiffness needs h_G or the mesh (h_xverts, h_geom_dofmap)");
      rc = create_on_plan(desc, fr, tdm, plan_mass, per_cell ? h_Gc.data() : nullptr, op.get());
    }
    // no kernel yet: the mesh does not tile into lattice columns, or the plan was not asked for
    if (rc == WF_OK && op->kernel == OpKernel::none) rc = create_batch(desc, fr, tdm, op.get());
  }
  if (rc != WF_OK) return rc;
  *out = op.release();
  return WF_OK;
}

int wf_op_create_box(int kind, int degree, int nx, int ny, int nz, const double* h_xverts, double c0, int flags,
                     wf_op** out)
{
  return wf_op_create_box_tuned(kind, degree, nx, ny, nz, h_xverts, c0, flags, nullptr, out);
}

}  // extern "C"

namespace {

// Kernel, cross-section, geometry form, metric, update and z segmentation of a box stiffness operator.  h_Gc: the per-cell
// geometry [ncells][6] when geom != point.  The order of the checks decides which error a bad tuning reports.
int choose_box_stiffness(int P, int nx, int ny, int nz, const double* h_xverts, int flags, const wf_tuning& tun,
                         OpKernel* kernel, BoxChoice* ch, std::vector<double>& h_Gc)
{
  // production kernel: marching columns (stiffness_march.hip; P >= 5: the k-split form,
  // stiffness_march_ks.hip).  wf_tuning: kernel = WF_KERNEL_FORCE_BOX_BLOCK selects the single-pass
  // block kernel, variant the compiled column cross-section, lz the layers per z segment.
  const bool march = tun.kernel != WF_KERNEL_FORCE_BOX_BLOCK;
  *kernel = march ? OpKernel::box_march : OpKernel::box_block;
  if (march) {
    // P <= 4: the one-thread-per-column kernel (stiffness_march.hip), cross-section wf_tuning.variant - 1;
    // P >= 5: the k-split kernel (stiffness_march_ks.hip), cross-section wf_tuning.bx x by when compiled
    // (wf_tuning.variant = 4 selects it at P4 as well, for comparisons).  P >= 5 with wf_tuning.update = OWNER: the
    // owner form (stiffness_march_owner.hip) when the mesh allows it; wf_tuning.variant indexes its cross-sections and
    // the per-cell geometry is blocked by that cross-section (there is no atomic per-cell kernel at these degrees).
    static const int kDefaultVariant[5] = {0, 0, 0, 0, 1};                // P4: 5x2 columns
    static const int kOwnerDefaultHi[8] = {0, 0, 0, 0, 0, 1, 2, 0};   // P5 5x2, P6 2x3, P7 2x2: the measured best
    if (P >= 5 && tun.update == WF_UPDATE_OWNER) {
      // stays box_march until the geometry below allows the owner form: it is per-cell capable
      ch->variant = tun.variant > 0 ? tun.variant - 1 : kOwnerDefaultHi[P];
      if (!march_owner_variant(P, ch->variant, &ch->bx, &ch->by)) {
        set_error("wf_op_create_box: wf_tuning.variant out of range");
        return WF_ERR_INVALID;
      }
    } else if (P >= 5 || tun.variant == 4) {
      *kernel = OpKernel::box_ksplit;
      ch->bx = tun.bx;
      ch->by = tun.by;
      if (!march_ks_shape(P, &ch->bx, &ch->by)) {
        set_error("wf_op_create_box: the k-split kernel is compiled for degrees 4..7");
        return WF_ERR_UNSUPPORTED;
      }
    } else {
      ch->variant = tun.variant > 0 ? tun.variant - 1 : kDefaultVariant[P];
      if (!march_variant(P, ch->variant, &ch->bx, &ch->by)) {
        set_error("wf_op_create_box: wf_tuning.variant out of range");
        return WF_ERR_INVALID;
      }
    }
    ch->bz = 1;
  }
  // geometry: per cell when every cell is affine and the P <= 4 marching kernel or the owner form runs (the k-split
  // and the single-pass block kernels read per-point geometry only)
  WF_REQUIRE(tun.geometry >= WF_GEOMETRY_AUTO && tun.geometry <= WF_GEOMETRY_PER_CELL,
             "wf_op_create_box: wf_tuning.geometry out of range");
  WF_REQUIRE(tun.metric >= WF_METRIC_AUTO && tun.metric <= WF_METRIC_AXES, "wf_op_create_box: wf_tuning.metric out of range");
  const bool cell_capable = *kernel == OpKernel::box_march;
  if (tun.geometry == WF_GEOMETRY_PER_CELL && !cell_capable) {
    set_error("wf_op_create_box: per-cell geometry needs the marching kernel of degree <= 4");
    return WF_ERR_UNSUPPORTED;
  }
  bool per_cell = false;
  if (cell_capable && tun.geometry != WF_GEOMETRY_PER_POINT) {
    if (box_cell_geometry(P, nx, ny, nz, h_xverts, fabs_flag(flags), clamp_flag(flags), h_Gc))
      per_cell = true;
    else if (tun.geometry == WF_GEOMETRY_PER_CELL) {
      set_error("wf_op_create_box: per-cell geometry requested but the mesh is not affine (or the -1/0/1 clamp "
                "takes effect)");
      return WF_ERR_INVALID;
    }
  }
  // metric: the separable (axes) form when every G_c is diagonal -- off-diagonals exactly 0, either sign; the
  // clamp checks above already hold (they leave an exact 0 alone)
  if (tun.metric == WF_METRIC_AXES && !per_cell) {
    set_error("wf_op_create_box: the axes metric needs per-cell geometry");
    return WF_ERR_UNSUPPORTED;
  }
  if (per_cell) {
    bool diagonal = true;
    for (size_t c = 0; c < h_Gc.size() && diagonal; c += 6)
      diagonal = h_Gc[c + 1] == 0.0 && h_Gc[c + 2] == 0.0 && h_Gc[c + 4] == 0.0;
    if (tun.metric == WF_METRIC_AXES && !diagonal) {
      set_error("wf_op_create_box: axes metric requested but a cell's G_c has a non-zero off-diagonal");
      return WF_ERR_INVALID;
    }
    ch->geom = diagonal && tun.metric != WF_METRIC_FULL ? MarchGeom::cell_axes : MarchGeom::cell;
  }
  // update: the owner-computes form of the separable kernel (no atomics) where it measured faster -- P4 -- or on
  // request (P1 to P7); wf_tuning.variant then indexes its own cross-section table.  The per-cell geometry keeps the
  // blocking of the atomic form's cross-section of the same index (P >= 5: of the owner cross-section).
  WF_REQUIRE(tun.update >= WF_UPDATE_AUTO && tun.update <= WF_UPDATE_OWNER, "wf_op_create_box: wf_tuning.update out of range");
  if (ch->geom == MarchGeom::cell_axes) {
    if (tun.update == WF_UPDATE_OWNER || (tun.update == WF_UPDATE_AUTO && P == 4)) {
      if (!march_owner_variant(P, ch->variant, &ch->obx, &ch->oby)) {
        set_error("wf_op_create_box: wf_tuning.variant out of range");
        return WF_ERR_INVALID;
      }
      *kernel = OpKernel::box_owner;
    }
  } else if (tun.update == WF_UPDATE_OWNER) {
    set_error("wf_op_create_box: the owner update needs the separable (axes) form of the marching kernel");
    return WF_ERR_UNSUPPORTED;
  }
  if (!march) return WF_OK;
  // z segmentation: work items = columns x segments run in rounds of the resident workgroups (occupancy
  // query of the kernel that launches: 2 per CU for the per-point P4 kernel, 3 for the full per-cell one and 3 for
  // the axes one); each item pays ~1.5 layers of
  // pipeline fill.  Pick the segment length that minimises rounds * (lz + 1.5).
  const bool owner = *kernel == OpKernel::box_owner;
  const int ncols = owner ? box_owner_columns(P, nx, ny, ch->obx, ch->oby).count() : box_columns(nx, ny, ch->bx, ch->by).count();
  long resident = owner                                 ? march_owner_resident(P, ch->variant)
                  : *kernel == OpKernel::box_march ? march_resident(P, ch->variant, ch->geom)
                                                        : march_ks_resident(P, ch->bx, ch->by);
  if (resident <= 0) resident = 512;
  double best = 1e300;
  ch->lz = nz;
  for (int nseg = 1; nseg <= nz; ++nseg) {
    const int lz = (nz + nseg - 1) / nseg;
    if (lz < 3 && nseg > 1) break;
    const long items = (long)ncols * box_segments(nz, lz, lz);
    const double cost = (double)((items + resident - 1) / resident) * (lz + 1.5);
    if (cost < best - 1e-9) {
      best = cost;
      ch->lz = lz;
    }
  }
  if (tun.lz > 0) ch->lz = tun.lz;
  return WF_OK;
}

// G_c blocked like G6blk: [column-layer block][cell of the layer][6], padding cells zero
int upload_box_cell_geometry(wf_op* op, const std::vector<double>& h_Gc)
{
  const int nx = op->nx, ny = op->ny, nz = op->nz, CB = op->box.bx * op->box.by;
  const BoxColumns cols = box_columns(nx, ny, op->box.bx, op->box.by);
  std::vector<double> blk((size_t)cols.count() * nz * CB * 6, 0.0);
  for (int cz = 0; cz < nz; ++cz)
    for (int cy = 0; cy < ny; ++cy)
      for (int cx = 0; cx < nx; ++cx) {
        const size_t b = (size_t)(cx / op->box.bx) + (size_t)cols.nbx * ((cy / op->box.by) + (size_t)cols.nby * cz);
        const int cl = cx % op->box.bx + op->box.bx * (cy % op->box.by);
        std::memcpy(&blk[(b * CB + cl) * 6], &h_Gc[((size_t)cx + (size_t)nx * (cy + (size_t)ny * cz)) * 6], 6 * sizeof(double));
      }
  return dev_upload(&op->d_Gcell, blk.data(), blk.size(), &op->device_bytes);
}

// WF_FLAG_ORDERED on a box: the box's lexicographic dofmap (dof (I, J, K) -> I + NX (J + NY K), tensor order) and vertex
// map (vertex (a, b, c) -> a + (nx+1)(b + (ny+1) c)) built on the host, then the dofmap operator of wf_op_create -- a box
// operator with the flag IS that dofmap operator, bit for bit.
int create_box_ordered(int kind, int P, int nx, int ny, int nz, const double* h_xverts, double c0, int flags,
                       const wf_tuning* tuning, wf_op** out)
{
  const int n = P + 1, nd = n * n * n;
  const size_t NX = (size_t)P * nx + 1, NY = (size_t)P * ny + 1, NZ = (size_t)P * nz + 1;
  const size_t ncells = (size_t)nx * ny * nz;
  std::vector<int32_t> dm(ncells * nd), gd(ncells * 8);
  for (int cz = 0; cz < nz; ++cz)
    for (int cy = 0; cy < ny; ++cy)
      for (int cx = 0; cx < nx; ++cx) {
        const size_t c = (size_t)cx + (size_t)nx * (cy + (size_t)ny * cz);
        const size_t base = (size_t)P * cx + NX * ((size_t)P * cy + NY * ((size_t)P * cz));
        for (int k = 0; k < n; ++k)
          for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) dm[c * nd + i + n * (j + n * k)] = (int32_t)(base + i + NX * (j + NY * k));
        for (int v = 0; v < 8; ++v)
          gd[c * 8 + v] = (int32_t)((cx + (v & 1)) + (size_t)(nx + 1) * ((cy + ((v >> 1) & 1)) + (size_t)(ny + 1) * (cz + ((v >> 2) & 1))));
      }
  wf_op_desc d{};
  d.kind = kind;
  d.degree = P;
  d.ncells = (int)ncells;
  d.ndofs = (int)(NX * NY * NZ);
  d.h_dofmap = dm.data();
  d.nverts = (nx + 1) * (ny + 1) * (nz + 1);
  d.h_xverts = h_xverts;
  d.h_geom_dofmap = gd.data();
  d.c0 = c0;
  d.flags = flags;
  d.tuning = tuning;
  int rc = wf_op_create(&d, out);
  if (rc != WF_OK) return rc;
  (*out)->structured = 1;
  (*out)->nx = nx;
  (*out)->ny = ny;
  (*out)->nz = nz;
  return WF_OK;
}

// uploads the interior / interface work-item lists (and the two interior halves)
int set_item_lists(wf_op* op, std::vector<int32_t> (&items)[4])
{
  // the interior halves let a caller hide BOTH halo directions: forward update under
  // half A, reverse update under half B (alternate items so both halves span the mesh)
  items[2].clear();
  items[3].clear();
  for (size_t q = 0; q < items[0].size(); ++q) items[2 + (q & 1)].push_back(items[0][q]);
  for (int k = 0; k < 4; ++k) {
    if (op->d_items[k]) op->device_bytes -= (size_t)op->nitems[k] * sizeof(int32_t);
    (void)hipFree(op->d_items[k]);
    op->d_items[k] = nullptr;
    op->nitems[k] = (int)items[k].size();
    if (op->nitems[k]) {
      int rc = dev_upload(&op->d_items[k], items[k].data(), items[k].size(), &op->device_bytes);
      if (rc != WF_OK) return rc;
    }
  }
  op->have_parts = 1;
  return WF_OK;
}

// Splits the work items of a box marching operator (item = column + columns * z segment): interface(Bx, By, seg, z0, z1)
// says whether the item of column (Bx, By) and layers [z0, z1) reads a ghost value of x or adds into one of y.
// With a ghost plane below, the first z segment is kept short (wf_tuning.lz0, default 3 layers):
// only its first layer reads the ghost plane, but the whole segment has to wait for the halo, and
// the less interface work there is the earlier the reverse exchange can start under the interior.
template <class Interface>
int split_box_items(wf_op* op, bool ghost_below, Interface&& interface)
{
  const int lz = op->box.lz;
  op->lz0_split = ghost_below ? std::max(1, std::min(op->tun.lz0 > 0 ? op->tun.lz0 : 3, lz)) : lz;
  const BoxColumns cols = op_columns(op);
  const int ncols = cols.count(), nseg = box_segments(op->nz, lz, op->lz0_split);
  std::vector<int32_t> items[4];
  for (int seg = 0; seg < nseg; ++seg) {
    const BoxSegment zs = box_segment(seg, op->nz, lz, op->lz0_split);
    for (int col = 0; col < ncols; ++col)
      items[interface(col % cols.nbx, col / cols.nbx, seg, zs.z0, zs.z1) ? 1 : 0].push_back(col + ncols * seg);
  }
  return set_item_lists(op, items);
}

}  // namespace

extern "C" {

int wf_op_create_box_tuned(int kind, int degree, int nx, int ny, int nz, const double* h_xverts, double c0, int flags,
                           const wf_tuning* tuning, wf_op** out)
{
  WF_REQUIRE(out != nullptr, "wf_op_create_box: null output");
  *out = nullptr;
  const int P = degree;
  if (P < 1 || P > kMaxDegree) {
    set_error("wf_op_create_box: degree must be 1..7 (hexahedron)");
    return WF_ERR_UNSUPPORTED;
  }
  WF_REQUIRE(kind == WF_OP_STIFFNESS || kind == WF_OP_MASS_LUMPED, "wf_op_create_box: kind must be stiffness or lumped mass");
  WF_REQUIRE(!tuning || tuning->kernel != WF_KERNEL_FORCE_MASS_MARCH,
             "wf_op_create_box: WF_KERNEL_FORCE_MASS_MARCH applies to the dense mass only");
  WF_REQUIRE(nx > 0 && ny > 0 && nz > 0 && h_xverts, "wf_op_create_box: bad mesh");
  const size_t NX = (size_t)P * nx + 1, NY = (size_t)P * ny + 1, NZ = (size_t)P * nz + 1;
  WF_REQUIRE(NX * NY * NZ < ((size_t)1 << 31), "wf_op_create_box: dof lattice exceeds int32");
  const int n = P + 1, nd = n * n * n;
  if (flags & WF_FLAG_ORDERED) return create_box_ordered(kind, P, nx, ny, nz, h_xverts, c0, flags, tuning, out);

  OpPtr op = new_op(kind, P, nd, nd, nx * ny * nz, (int)(NX * NY * NZ), c0, tuning);
  op->nq1 = n;
  op->structured = 1;
  op->nx = nx;
  op->ny = ny;
  op->nz = nz;

  op->kernel = OpKernel::diagonal;   // lumped mass: the pre-assembled diagonal
  std::vector<double> h_Gc;          // per-cell geometry, [ncells][6]
  default_box_block(P, op->tun, &op->box.bx, &op->box.by, &op->box.bz);
  int rc;
  if (kind == WF_OP_STIFFNESS
      && (rc = choose_box_stiffness(P, nx, ny, nz, h_xverts, flags, op->tun, &op->kernel, &op->box, h_Gc)) != WF_OK)
    return rc;

  if ((rc = upload_derivative_tables(op.get(), true)) != WF_OK) return rc;
  Scratch<double> d_x, d_pts, d_wts;
  const size_t nverts = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
  if ((rc = dev_upload(&d_x.p, h_xverts, nverts * 3, nullptr)) != WF_OK) return rc;
  if ((rc = upload_tables(P, d_pts, d_wts)) != WF_OK) return rc;

  if (kind == WF_OP_STIFFNESS && op->box.geom != MarchGeom::point) {
    if ((rc = upload_box_cell_geometry(op.get(), h_Gc)) != WF_OK) return rc;
  } else if (kind == WF_OP_STIFFNESS) {
    const size_t nblk = (size_t)box_columns(nx, ny, op->box.bx, op->box.by).count() * ((nz + op->box.bz - 1) / op->box.bz);
    const size_t g6 = nblk * op->box.bx * op->box.by * op->box.bz * nd * 6;
    if ((rc = dev_alloc(&op->d_G6blk, g6, &op->device_bytes)) != WF_OK) return rc;
    WF_HIP_CHECK(hipMemset(op->d_G6blk, 0, g6 * sizeof(double)));
    if ((rc = launch_geometry_box(P, nx, ny, nz, op->box.bx, op->box.by, op->box.bz, d_x.p, d_pts.p, d_wts.p, fabs_flag(flags), clamp_flag(flags),
                                  op->d_G6blk, nullptr, nullptr)) != WF_OK)
      return rc;
  } else {
    // pre-assembled lumped mass diagonal: y += m .* x is 24 B/dof instead of the
    // 34.8 B/dof gather/transform/scatter of spectral_mass.hpp:84-89
    if ((rc = dev_alloc(&op->d_mdiag, (size_t)op->ndofs, &op->device_bytes)) != WF_OK) return rc;
    WF_HIP_CHECK(hipMemset(op->d_mdiag, 0, (size_t)op->ndofs * sizeof(double)));
    if ((rc = launch_geometry_box(P, nx, ny, nz, 1, 1, 1, d_x.p, d_pts.p, d_wts.p, fabs_flag(flags), clamp_flag(flags), nullptr,
                                  op->d_mdiag, nullptr)) != WF_OK)
      return rc;
  }
  WF_HIP_CHECK(hipDeviceSynchronize());
  *out = op.release();
  return WF_OK;
}

int wf_op_create_dense_simplex(const wf_dense_desc* desc, wf_op** out)
{
  WF_REQUIRE(desc && out, "wf_op_create_dense_simplex: null argument");
  *out = nullptr;
  WF_REQUIRE(desc->nd > 0 && desc->nq > 0 && desc->ncells >= 0 && desc->ndofs >= 0, "wf_op_create_dense_simplex: bad sizes");
  if (desc->flags & WF_FLAG_ORDERED) {
    set_error("wf_op_create_dense_simplex: WF_FLAG_ORDERED is not implemented for the dense simplex operator (its "
              "persistent MFMA kernel adds with atomics)");
    return WF_ERR_UNSUPPORTED;
  }
  WF_REQUIRE(desc->h_dofmap && desc->h_dphi && desc->h_weights && desc->h_xverts && desc->h_geom_dofmap,
             "wf_op_create_dense_simplex: null array");
  for (size_t e = 0; e < (size_t)desc->ncells * desc->nd; ++e)
    WF_REQUIRE(desc->h_dofmap[e] >= 0 && desc->h_dofmap[e] < desc->ndofs, "wf_op_create_dense_simplex: dofmap entry out of range");
  for (size_t e = 0; e < (size_t)desc->ncells * 4; ++e)
    WF_REQUIRE(desc->h_geom_dofmap[e] >= 0 && desc->h_geom_dofmap[e] < desc->nverts,
               "wf_op_create_dense_simplex: vertex index out of range");
  OpPtr op = new_op(WF_OP_STIFFNESS, 0, desc->nd, desc->nq, desc->ncells, desc->ndofs, desc->c0, nullptr);
  op->kernel = OpKernel::dense_simplex;
  op->dense_clamp = clamp_flag(desc->flags);
  int rc = dense_setup(desc->nd, desc->nq, desc->ncells, desc->ndofs, desc->h_dofmap, desc->h_dphi, desc->h_weights,
                       desc->h_xverts, desc->h_geom_dofmap, &op->dense);
  if (rc != WF_OK) return rc;
  op->device_bytes = dense_bytes(op->dense);
  *out = op.release();
  return WF_OK;
}

int wf_op_create_dense_simplex_mass(const wf_dense_mass_desc* desc, wf_op** out)
{
  // every check, dense_mass_setup's included, precedes the first HIP call
  WF_REQUIRE(desc && out, "wf_op_create_dense_simplex_mass: null argument");
  *out = nullptr;
  WF_REQUIRE(desc->nd > 0 && desc->nq > 0 && desc->ncells >= 0 && desc->ndofs >= 0 && desc->nverts >= 0,
             "wf_op_create_dense_simplex_mass: bad sizes (nd, nq, ncells, ndofs, nverts)");
  if (desc->flags & WF_FLAG_ORDERED) {
    set_error("wf_op_create_dense_simplex_mass: WF_FLAG_ORDERED is not implemented for the dense simplex mass (its "
              "persistent MFMA kernel adds with atomics)");
    return WF_ERR_UNSUPPORTED;
  }
  if (desc->flags & ~(WF_FLAG_NO_FABS | WF_FLAG_ORDERED)) {
    set_error("wf_op_create_dense_simplex_mass: unknown flag bit in flags = " + std::to_string(desc->flags)
              + " (the operator takes WF_FLAG_NO_FABS only)");
    return WF_ERR_INVALID;
  }
  WF_REQUIRE(desc->h_dofmap && desc->h_phi && desc->h_weights && desc->h_xverts && desc->h_geom_dofmap,
             "wf_op_create_dense_simplex_mass: null array (h_dofmap, h_phi, h_weights, h_xverts, h_geom_dofmap)");
  for (size_t e = 0; e < (size_t)desc->ncells * desc->nd; ++e)
    WF_REQUIRE(desc->h_dofmap[e] >= 0 && desc->h_dofmap[e] < desc->ndofs, "wf_op_create_dense_simplex_mass: dofmap entry out of range");
  for (size_t e = 0; e < (size_t)desc->ncells * 4; ++e)
    WF_REQUIRE(desc->h_geom_dofmap[e] >= 0 && desc->h_geom_dofmap[e] < desc->nverts,
               "wf_op_create_dense_simplex_mass: vertex index out of range");
  OpPtr op = new_op(WF_OP_MASS_DENSE, 0, desc->nd, desc->nq, desc->ncells, desc->ndofs, 0.0, nullptr);
  op->kernel = OpKernel::dense_simplex_mass;
  int rc = dense_mass_setup(desc->nd, desc->nq, desc->ncells, desc->h_dofmap, desc->h_phi, desc->h_weights, desc->h_xverts,
                            desc->h_geom_dofmap, fabs_flag(desc->flags), &op->dense_mass);
  if (rc != WF_OK) return rc;
  op->device_bytes = dense_mass_bytes(op->dense_mass);
  *out = op.release();
  return WF_OK;
}

// The one place that maps the kernel choice to a launch.  wf_op_apply runs every work item (d_items null, lz0 = lz);
// wf_op_apply_part the items of one part of a marching operator, whose first z segment has lz0 layers.
static int launch_op(const wf_op* op, int lz0, const int32_t* d_items, int nitems, const double* d_x, double* d_y, hipStream_t s)
{
  switch (op->kernel) {
    case OpKernel::box_march:
      return launch_stiffness_march(op->P, op->box.variant, op->box.geom, op->nx, op->ny, op->nz, op->box.lz, lz0, op->d_G6blk,
                                    op->d_Gcell, op->d_D, op->box.geom == MarchGeom::cell_axes ? op->am : op->dm, op->coeff, d_x,
                                    d_y, d_items, nitems, s);
    case OpKernel::box_ksplit:
      return launch_stiffness_march_ks_box(op->P, op->box.bx, op->box.by, op->nx, op->ny, op->nz, op->box.lz, lz0, op->d_G6blk, op->d_D,
                                           op->dm, op->coeff, d_x, d_y, d_items, nitems, s);
    case OpKernel::box_owner:
      return launch_stiffness_march_owner(op->P, op->box.variant, op->nx, op->ny, op->nz, op->box.lz, lz0, op->box.bx, op->box.by,
                                          op->d_Gcell, op->d_D, op->am, op->coeff, d_x, d_y, d_items, nitems, s);
    case OpKernel::box_block:
      return launch_stiffness_box(op->P, op->nx, op->ny, op->nz, op->box.bx, op->box.by, op->box.bz, op->d_G6blk, op->d_D, op->dm,
                                  op->coeff, d_x, d_y, s);
    case OpKernel::idx_march:
      return launch_stiffness_march_idx(op->P, op->idx_geom, op->plan, op->idx_geom == MarchGeom::point ? op->d_G6blk : op->d_Gcell,
                                        op->d_D, op->idx_geom == MarchGeom::cell_axes ? op->am : op->dm, op->coeff, d_x, d_y,
                                        d_items, nitems, s);
    case OpKernel::generic_unique:
      return launch_stiffness_generic_u(op->P, op->ncells, op->d_uoff, op->d_uniq, op->d_loc, op->d_G6blk, op->d_D,
                                        op->dm, op->coeff, d_x, d_y, s);
    case OpKernel::generic_elementwise:
      return launch_stiffness_generic(op->P, op->ncells, op->d_dofmap, op->d_G6blk, op->d_D, op->dm, op->coeff, d_x, d_y, s);
    case OpKernel::lumped_unique:
      return launch_mass_lumped_u(op->ncells, op->nd, op->unique_cb, op->d_uoff, op->d_uniq, op->d_loc, op->d_detJ, d_x, d_y, s);
    case OpKernel::lumped_elementwise:
      return launch_mass_lumped((int64_t)op->ncells * op->nd, op->d_dofmap, op->d_detJ, d_x, d_y, s);
    case OpKernel::diagonal:
      if (op->diag_named_only) return launch_diagonal_named(op->ndofs, op->d_mdiag, d_x, d_y, s);
      return wf_pointwise_mult_add(op->ndofs, op->d_mdiag, d_x, d_y, s);
    case OpKernel::mass_march: return launch_mass_march(op->P, op->nq1, op->plan, op->d_detJ, op->d_phi1, d_x, d_y, s);
    case OpKernel::mass_column:
      return launch_mass_dense_col(op->P, op->ncells, op->d_uoff, op->d_uniq, op->d_loc, op->d_phi1, op->d_detJ, d_x, d_y, s);
    case OpKernel::mass_any:   // with the unique-dof tile when creation built the lists (d_uoff)
      return launch_mass_dense(op->P, op->nq1, op->ncells, op->d_dofmap, op->d_uoff, op->d_uniq, op->d_loc, op->unique_cb,
                               op->d_phi1, op->d_detJ, d_x, d_y, s);
    case OpKernel::dense_simplex: return launch_stiffness_dense(op->dense, op->coeff, op->dense_clamp, d_x, d_y, s);
    case OpKernel::dense_simplex_mass: return launch_mass_dense_simplex(op->dense_mass, d_x, d_y, s);
    case OpKernel::ordered_stiffness:
    case OpKernel::ordered_mass:
    case OpKernel::ordered_lumped: {
      // pass 1 into the operator's scratch v, pass 2 behind it on the same stream
      int rc = op->kernel == OpKernel::ordered_stiffness
                   ? launch_stiffness_ordered(op->P, op->ncells, op->d_dofmap, op->d_slot, op->d_G6blk, op->d_D, op->dm, op->coeff, d_x, op->d_v, s)
               : op->kernel == OpKernel::ordered_mass
                   ? launch_mass_dense_ordered(op->P, op->nq1, op->ncells, op->d_dofmap, op->d_slot, op->d_phi1, op->d_detJ, d_x, op->d_v, s)
                   : launch_mass_lumped_ordered((int64_t)op->ncells * op->nd, op->d_dofmap, op->d_slot, op->d_detJ, d_x, op->d_v, s);
      if (rc != WF_OK || op->ncells == 0) return rc;
      return wf_segment_sum_add(op->ndofs, op->d_row_off, op->d_v, d_y, s);
    }
    case OpKernel::none: break;
  }
  set_error("wf_op_apply: corrupt handle");
  return WF_ERR_INVALID;
}

int wf_op_apply(wf_op* op, const double* d_x, double* d_y, void* stream)
{
  WF_REQUIRE(op && d_x && d_y, "wf_op_apply: null argument");
  MarkerScope mk("wf_op_apply");
  return launch_op(op, op->box.lz, nullptr, 0, d_x, d_y, (hipStream_t)stream);
}

int wf_op_set_ghost_faces(wf_op* op, int ghost_x0, int ghost_y0, int ghost_z0)
{
  WF_REQUIRE(op != nullptr, "wf_op_set_ghost_faces: null handle");
  if (!is_box_march(op->kernel)) {
    set_error("wf_op_set_ghost_faces: only the marching box stiffness operator has lattice faces (wf_op_set_ghost_dofs "
              "splits any marching operator)");
    return WF_ERR_UNSUPPORTED;
  }
  // A work item is "interface" when it reads a ghost plane of x / adds into a ghost plane of y.  The owner form's columns
  // are lattice lines in pieces of P*obx x P*oby and it reads P lattice lines / planes below what it owns:
  // [I0 - P, ..] x [J0 - P, ..] x [P z0 - P, ..]
  const bool owner = op->kernel == OpKernel::box_owner;
  const int P = op->P, obx = op->box.obx, oby = op->box.oby;
  return split_box_items(op, ghost_z0 != 0, [&](int Bx, int By, int seg, int z0, int) {
    return owner ? (ghost_x0 && P * obx * Bx <= P) || (ghost_y0 && P * oby * By <= P) || (ghost_z0 && z0 <= 1)
                 : (ghost_x0 && Bx == 0) || (ghost_y0 && By == 0) || (ghost_z0 && seg == 0);
  });
}

int wf_op_set_ghost_dofs(wf_op* op, const int32_t* h_ghost_positions, int32_t nghosts)
{
  WF_REQUIRE(op != nullptr && nghosts >= 0 && (nghosts == 0 || h_ghost_positions), "wf_op_set_ghost_dofs: bad argument");
  const bool box = is_box_march(op->kernel);
  if (!box && op->kernel != OpKernel::idx_march) {
    set_error("wf_op_set_ghost_dofs: only the marching stiffness operators split into interior / interface work items "
              "(this operator runs a batch kernel)");
    return WF_ERR_UNSUPPORTED;
  }
  std::vector<char> ghost((size_t)op->ndofs, 0);
  for (int32_t g = 0; g < nghosts; ++g) {
    WF_REQUIRE(h_ghost_positions[g] >= 0 && h_ghost_positions[g] < op->ndofs, "wf_op_set_ghost_dofs: ghost position out of range");
    ghost[h_ghost_positions[g]] = 1;
  }
  const int P = op->P;
  if (box) {
    const int NX = P * op->nx + 1, NY = P * op->ny + 1;
    const size_t plane = (size_t)NX * NY;
    bool gz = false;   // a z ghost plane below
    for (size_t g = 0; g < plane && !gz; ++g) gz = ghost[g] != 0;
    // the owner form's columns are pieces of P*obx x P*oby lattice lines; its footprint reaches P lines / planes below
    // what it owns: [I0 - P, I0 + P obx] x [J0 - P, J0 + P oby] x [P z0 - P, P z1]
    const bool owner = op->kernel == OpKernel::box_owner;
    const int cbx = owner ? op->box.obx : op->box.bx, cby = owner ? op->box.oby : op->box.by;   // cells per column
    const int halo = owner ? P : 0;
    return split_box_items(op, gz, [&](int Bx, int By, int, int z0, int z1) {
      const int I0 = std::max(0, P * Bx * cbx - halo), J0 = std::max(0, P * By * cby - halo);
      const int I1 = std::min(NX - 1, P * Bx * cbx + P * cbx), J1 = std::min(NY - 1, P * By * cby + P * cby);
      for (int K = std::max(0, P * z0 - halo); K <= P * z1; ++K)
        for (int J = J0; J <= J1; ++J) {
          const char* row = &ghost[(size_t)I0 + (size_t)NX * J + plane * K];
          for (int I = 0; I <= I1 - I0; ++I)
            if (row[I]) return true;
        }
      return false;
    });
  }
  // an item is interface iff its dof tile (base + pattern offsets) contains a ghost position
  std::vector<int32_t> items[4];
  const int nit = op->plan.nitems;
  const size_t tsize = (size_t)op->plan.tile_size;
  std::vector<int32_t> base(nit), pat(nit), pat_off((size_t)op->plan_patterns * tsize);
  WF_HIP_CHECK(hipMemcpy(base.data(), op->plan.d_item_base, (size_t)nit * sizeof(int32_t), hipMemcpyDeviceToHost));
  WF_HIP_CHECK(hipMemcpy(pat.data(), op->plan.d_item_pattern, (size_t)nit * sizeof(int32_t), hipMemcpyDeviceToHost));
  WF_HIP_CHECK(hipMemcpy(pat_off.data(), op->plan.d_pat_off, pat_off.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int it = 0; it < nit; ++it) {
    const int32_t* off = &pat_off[(size_t)pat[it] * tsize];
    bool iface = false;
    for (size_t e = 0; e < tsize; ++e)
      if (off[e] >= 0 && ghost[(size_t)base[it] + off[e]]) {
        iface = true;
        break;
      }
    items[iface ? 1 : 0].push_back(it);
  }
  return set_item_lists(op, items);
}

int wf_op_apply_part(wf_op* op, const double* d_x, double* d_y, int part, void* stream)
{
  WF_REQUIRE(op && d_x && d_y, "wf_op_apply_part: null argument");
  if (part == WF_PART_ALL) return wf_op_apply(op, d_x, d_y, stream);
  WF_REQUIRE(part >= WF_PART_INTERIOR && part <= WF_PART_INTERIOR_B, "wf_op_apply_part: unknown part");
  if (op->kernel == OpKernel::dense_simplex_mass) {
    set_error("wf_op_apply_part: the dense simplex mass runs a batch kernel (no work items to split)");
    return WF_ERR_UNSUPPORTED;
  }
  if (!op->have_parts) {
    set_error("wf_op_apply_part: call wf_op_set_ghost_dofs / wf_op_set_ghost_faces first");
    return WF_ERR_INVALID;
  }
  const int k = part - 1;   // WF_PART_INTERIOR, _INTERFACE, _INTERIOR_A, _INTERIOR_B
  if (op->nitems[k] == 0) return WF_OK;
  static const char* kPartName[4] = {"wf_op_apply_part interior", "wf_op_apply_part interface", "wf_op_apply_part interior A",
                                     "wf_op_apply_part interior B"};
  MarkerScope mk(kPartName[k]);
  return launch_op(op, op->lz0_split, op->d_items[k], op->nitems[k], d_x, d_y, (hipStream_t)stream);
}

int wf_op_info(const wf_op* op, wf_op_info_t* info)
{
  WF_REQUIRE(op && info, "wf_op_info: null argument");
  // the public description of the kernel choice
  int kernel = WF_KERNEL_NONE, geometry = WF_GEOMETRY_AUTO, metric = WF_METRIC_NONE, update = WF_UPDATE_NONE;
  bool plan = false;
  switch (op->kernel) {
    case OpKernel::box_march:
      kernel = WF_KERNEL_MARCH_BOX;
      geometry = op->box.geom == MarchGeom::point ? WF_GEOMETRY_PER_POINT : WF_GEOMETRY_PER_CELL;
      metric = op->box.geom == MarchGeom::cell ? WF_METRIC_FULL : op->box.geom == MarchGeom::cell_axes ? WF_METRIC_AXES : WF_METRIC_NONE;
      update = op->box.geom == MarchGeom::cell_axes ? WF_UPDATE_ATOMIC : WF_UPDATE_NONE;
      break;
    case OpKernel::box_ksplit: kernel = WF_KERNEL_MARCH_BOX, geometry = WF_GEOMETRY_PER_POINT; break;
    case OpKernel::box_owner:
      kernel = WF_KERNEL_MARCH_BOX, geometry = WF_GEOMETRY_PER_CELL, metric = WF_METRIC_AXES, update = WF_UPDATE_OWNER;
      break;
    case OpKernel::box_block: kernel = WF_KERNEL_BOX_BLOCK, geometry = WF_GEOMETRY_PER_POINT; break;
    case OpKernel::idx_march:
      kernel = WF_KERNEL_MARCH_IDX, plan = true;
      geometry = op->idx_geom == MarchGeom::point ? WF_GEOMETRY_PER_POINT : WF_GEOMETRY_PER_CELL;
      metric = op->idx_geom == MarchGeom::cell ? WF_METRIC_FULL : op->idx_geom == MarchGeom::cell_axes ? WF_METRIC_AXES : WF_METRIC_NONE;
      update = op->idx_geom == MarchGeom::cell_axes ? WF_UPDATE_ATOMIC : WF_UPDATE_NONE;
      break;
    case OpKernel::generic_unique: kernel = WF_KERNEL_BATCH_UNIQUE, geometry = WF_GEOMETRY_PER_POINT; break;
    case OpKernel::generic_elementwise: kernel = WF_KERNEL_ELEMENTWISE, geometry = WF_GEOMETRY_PER_POINT; break;
    case OpKernel::lumped_unique: kernel = WF_KERNEL_BATCH_UNIQUE; break;
    case OpKernel::lumped_elementwise: kernel = WF_KERNEL_ELEMENTWISE; break;
    case OpKernel::diagonal: kernel = WF_KERNEL_DIAGONAL; break;
    case OpKernel::mass_march: kernel = WF_KERNEL_MARCH_IDX, plan = true; break;
    case OpKernel::mass_column: kernel = WF_KERNEL_BATCH_UNIQUE; break;
    case OpKernel::mass_any: kernel = WF_KERNEL_MASS_DENSE_ANY; break;
    case OpKernel::dense_simplex: kernel = WF_KERNEL_DENSE_SIMPLEX, geometry = WF_GEOMETRY_PER_CELL; break;
    case OpKernel::dense_simplex_mass: kernel = WF_KERNEL_DENSE_SIMPLEX_MASS; break;
    case OpKernel::ordered_stiffness: kernel = WF_KERNEL_CELLS_ORDERED, geometry = WF_GEOMETRY_PER_POINT, update = WF_UPDATE_ORDERED; break;
    case OpKernel::ordered_mass:
    case OpKernel::ordered_lumped: kernel = WF_KERNEL_CELLS_ORDERED, update = WF_UPDATE_ORDERED; break;
    case OpKernel::none: break;
  }
  const bool dense = op->kernel == OpKernel::dense_simplex;
  info->kind = op->kind;
  info->degree = op->P;
  info->num_cells = op->ncells;
  info->num_dofs_cell = op->nd;
  info->num_quads = op->nq;
  info->ndofs = op->ndofs;
  info->structured = op->structured;
  // mass.hpp:71; dense skernel: SURVEY 8a3.  (The dense simplex mass is reported by the reference's model too; its
  // collapsed kernel executes 2 nd^2 per cell, whatever nq.)
  info->flops = (dense ? 12.0 : 4.0) * op->ncells * (double)op->nq * op->nd;
  if (geometry == WF_GEOMETRY_PER_CELL)
    info->alg_bytes = (double)op->ncells * (48.0 + 4.0 * op->nd) + 16.0 * op->ndofs;   // one G per cell
  else if (geometry == WF_GEOMETRY_PER_POINT)
    info->alg_bytes = (double)op->ncells * (48.0 * op->nq + 4.0 * op->nd) + 16.0 * op->ndofs;
  else if (op->kernel == OpKernel::dense_simplex_mass)
    info->alg_bytes = (double)op->ncells * (8.0 + 4.0 * op->nd) + 16.0 * op->ndofs;   // one scale per affine cell
  else if (op->kernel == OpKernel::diagonal)
    info->alg_bytes = 24.0 * op->ndofs;   // pre-assembled diagonal: read m, x, y + write y (SURVEY 8d counts 24)
  else
    info->alg_bytes = (double)op->ncells * (8.0 * op->nq + 4.0 * op->nd) + 16.0 * op->ndofs;
  // order-fixed accumulation: per element-local entry the slot (4), the store and the load of v (8 + 8); the row offsets
  if (kernel == WF_KERNEL_CELLS_ORDERED) info->alg_bytes += 20.0 * op->ncells * op->nd + 4.0 * (op->ndofs + 1.0);
  info->device_bytes = op->device_bytes;
  info->items_interior = op->nitems[0];
  info->items_interface = op->nitems[1];
  info->kernel = kernel;
  info->plan_items = plan ? op->plan.nitems : 0;
  info->plan_patterns = plan ? op->plan_patterns : 0;
  info->plan_lz = plan ? op->plan.lz : is_box_march(op->kernel) ? op->box.lz : 0;
  info->plan_reoriented = op->plan_reoriented;
  info->plan_fill = op->plan_fill;
  info->geometry = geometry;
  info->metric = metric;
  info->update = update;
  return WF_OK;
}

int wf_op_destroy(wf_op* op)
{
  free_op(op);
  return WF_OK;
}

}  // extern "C"
