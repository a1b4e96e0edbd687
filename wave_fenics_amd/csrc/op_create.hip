// wf_op_create: an operator on a caller's hexahedral dofmap.  Three paths: the collocated dense mass as a diagonal, the
// marching kernels on lattice columns found in the mesh, the batch kernels.
#include <cmath>
#include <cstring>

#include "op.h"

using namespace wf;

namespace {

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
  if ((rc = op->d_mdiag.upload(md)) != WF_OK) return rc;
  op->nq1 = n;
  op->diag_named_only = has_unnamed_dofs(desc, nd);
  op->kernel = OpKernel::diagonal;
  return WF_OK;
}

// ---- path 2: marching over lattice columns found in the caller's mesh (march_plan.cpp): the default of the
// stiffness operator and of the dense mass with a square 1-D table ----

// stiffness geometry in slot order [item][layer][ly][lx]; missing cells stay zero (they contribute nothing)
// h_Gc: per-cell geometry on request (wf_tuning.geometry), [ncells][6] in the cells' own frames; uploaded as
// Gc[(item lz + layer) CB + cell][6] in the plan's frame, op->geom already says which form reads it
int plan_stiffness_geometry(const wf_op_desc* desc, const CallerFrame& fr, const MarchPlan& plan, const double* h_Gc, wf_op* op)
{
  const int P = op->P, n = op->n, nd = op->nd, CB = op->plan.bx * op->plan.by;
  const size_t nslots = (size_t)plan.nitems * plan.lz * CB;
  int rc;
  if (h_Gc) {
    // G_c of a cell seen in the lattice frame, as h_G below (orient_tensor).  Without fabs G_c carries
    // the sign of the cell's own det J, which is what the per-point path restores with orient_sign.
    if ((rc = upload_derivative_tables(op, true)) != WF_OK) return rc;
    std::vector<double> blk(nslots * 6, 0.0);
    for (size_t q = 0; q < nslots; ++q) {
      const int32_t c = plan.slot_cell[q];
      if (c < 0) continue;
      orient_tensor(plan.cell_orient[c], kSym6, h_Gc + (size_t)c * 6, &blk[q * 6]);
      if (desc->h_cell_coeff)   // the cell coefficient follows the cell into its slot
        for (int m = 0; m < 6; ++m) blk[q * 6 + m] *= desc->h_cell_coeff[c];
    }
    if ((rc = op->d_Gcell.upload(blk)) != WF_OK) return rc;
    op->kernel = OpKernel::idx_march;
    return WF_OK;
  }
  if ((rc = upload_derivative_tables(op, false)) != WF_OK) return rc;
  const size_t g6 = nslots * nd * 6;
  if ((rc = op->d_G6blk.alloc(g6)) != WF_OK) return rc;
  WF_HIP_CHECK(hipMemset(op->d_G6blk.data(), 0, g6 * sizeof(double)));
  if (desc->h_G) {
    // G of a cell seen in the lattice frame (orient_tensor) at the relabelled point
    PointMaps point_map{fr, n};
    auto fill_slot_plain = [&](size_t slot, double* dst) {
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
      for (int pt = 0; pt < nd; ++pt) orient_tensor(code, kFull9, gsrc + (size_t)pm[pt] * 9, dst + (size_t)pt * 9);
    };
    auto fill_slot = [&](size_t slot, double* dst) {
      fill_slot_plain(slot, dst);
      const int32_t c = plan.slot_cell[slot];
      if (desc->h_cell_coeff && c >= 0)   // the cell coefficient follows the cell into its slot
        for (int e = 0; e < nd * 9; ++e) dst[e] *= desc->h_cell_coeff[c];
    };
    if ((rc = stage_G9(P, CB, nslots, nullptr, fill_slot, op->d_G6blk.data())) != WF_OK) return rc;
  } else {
    // one geometry thread per (present cell, point), written to the cell's slot; a cell is handed
    // over with its vertices relabelled into the lattice frame
    const size_t ncells = (size_t)desc->ncells;
    std::vector<int32_t> gd, slot_of;
    std::vector<uint8_t> sign;
    std::vector<double> coeff;   // the cell coefficient of every listed cell (empty: none)
    gd.reserve(ncells * 8);
    slot_of.reserve(ncells);
    sign.reserve(ncells);
    for (size_t q = 0; q < nslots; ++q) {
      const int32_t c = plan.slot_cell[q];
      if (c < 0) continue;
      const int code = plan.cell_orient[c];
      gd.resize(gd.size() + 8);
      orient_vertices(code, desc->h_geom_dofmap + (size_t)c * 8, &gd[gd.size() - 8]);
      slot_of.push_back((int32_t)q);
      sign.push_back((uint8_t)(int8_t)orient_sign(code));
      if (desc->h_cell_coeff) coeff.push_back(desc->h_cell_coeff[c]);
    }
    DevArray<double> d_x, d_pts, d_wts, d_coeff;
    DevArray<int32_t> d_gd, d_slot;
    DevArray<uint8_t> d_sign;
    if ((rc = d_x.upload(desc->h_xverts, (size_t)desc->nverts * 3)) != WF_OK) return rc;
    if ((rc = d_gd.upload(gd)) != WF_OK) return rc;
    if ((rc = d_slot.upload(slot_of)) != WF_OK) return rc;
    if ((rc = d_sign.upload(sign)) != WF_OK) return rc;
    if ((rc = d_coeff.upload(coeff)) != WF_OK) return rc;   // no coefficient: no array
    if ((rc = upload_tables(P, d_pts, d_wts)) != WF_OK) return rc;
    if ((rc = launch_geometry_hex_slots(P, CB, (int)slot_of.size(), d_x.data(), d_gd.data(), d_slot.data(), d_sign.data(),
                                        d_pts.data(), d_wts.data(), fabs_flag(desc->flags), clamp_flag(desc->flags),
                                        op->d_G6blk.data(), d_coeff.data(), nullptr)) != WF_OK)
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
  OrientMaps raw_map{M};   // hd is in the cells' own frames: the orientation alone
  std::vector<double> blk(nslots * nq, 0.0);
  for (size_t q = 0; q < nslots; ++q) {
    const int32_t c = plan.slot_cell[q];
    if (c < 0) continue;
    const int code = plan.cell_orient[c];
    const size_t sub = q / CB, sl = q % CB;
    const double* src = hsrc + (size_t)c * nq;
    const std::vector<int32_t>& pm = raw_points ? raw_map(code) : point_map(code);
    for (int k = 0; k < M; ++k)
      for (int ji = 0; ji < M * M; ++ji) blk[(sub * M + k) * NTq + sl * M * M + ji] = src[pm[ji + M * M * k]];
  }
  // A non-symmetric 1-D table kept the caller's frames (normalise in create_on_plan).
  if ((rc = op->d_detJ.upload(blk)) != WF_OK) return rc;
  if ((rc = op->d_phi1.upload(desc->h_phi1, (size_t)M * n)) != WF_OK) return rc;
  for (int q = 0; q < M * n; ++q) op->dm.v[q] = desc->h_phi1[q];
  op->nq1 = M;
  op->nq = nq;
  op->kernel = OpKernel::mass_march;
  return WF_OK;
}

// leaves op untouched (no kernel) when the mesh does not tile into lattice columns: the batch kernels take it
// h_Gc: the stiffness operator with per-cell geometry (on request; op->geom is set): any fill is adopted, and a mesh
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
  while (!mass && lz_max > 1 && march_idx_lds_bytes(pkind, P, BX, BY, lz_max, op->geom) > march_idx_lds_budget(pkind, P, BX, BY, op->geom))
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
  const std::string why = std::string(": ") + plan_reason_text(plan.reason);
  if (!plan.ok && mass && M != n) {   // a rectangular table is here on request only
    set_error("wf_op_create: WF_KERNEL_FORCE_MASS_MARCH: the mesh does not tile into lattice columns ((P, nq1) = ("
              + std::to_string(P) + ", " + std::to_string(M) + "))" + why);
    return WF_ERR_UNSUPPORTED;
  }
  if (!plan.ok && h_Gc) {
    set_error("wf_op_create: WF_GEOMETRY_PER_CELL: the mesh does not tile into lattice columns" + why);
    return WF_ERR_UNSUPPORTED;
  }
  if (!plan.ok) return WF_OK;

  if ((rc = op->d_item_base.upload(plan.item_base)) != WF_OK) return rc;
  if ((rc = op->d_item_pattern.upload(plan.item_pattern)) != WF_OK) return rc;
  if ((rc = op->d_item_layers.upload(plan.item_layers)) != WF_OK) return rc;
  if ((rc = op->d_pat_off.upload(plan.pat_off)) != WF_OK) return rc;
  op->plan = MarchPlanDev{plan.nitems, plan.lz, plan.tile_size, BX, BY, op->d_item_base.data(), op->d_item_pattern.data(),
                          op->d_item_layers.data(), op->d_pat_off.data()};
  op->plan_patterns = plan.npatterns;
  op->plan_reoriented = plan.reoriented;
  op->plan_fill = plan.fill;
  if ((rc = mass ? plan_mass_detJ(desc, fr, plan, op) : plan_stiffness_geometry(desc, fr, plan, h_Gc, op)) != WF_OK) return rc;
  WF_HIP_CHECK(hipDeviceSynchronize());
  return WF_OK;
}

// wf_tuning.geometry = WF_GEOMETRY_PER_CELL on wf_op_create (stiffness, ncells > 0): what else the request allows, the
// per-cell geometry h_Gc [ncells][6] in the cells' own frames and the form that will read it (op->geom).  Host only;
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
  if (desc->h_G) return per_cell_refuses_G("wf_op_create");
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
  const int64_t bad = hex_cell_geometry(P, (size_t)desc->ncells, desc->h_xverts, desc->h_geom_dofmap, fabs_flag(desc->flags),
                                        clamp_flag(desc->flags), h_Gc.data(), &reason);
  if (bad >= 0) return per_cell_refusal("wf_op_create", bad, reason);
  // metric: the separable (axes) form when every G_c is diagonal -- off-diagonals exactly 0, either sign.  Taking a cell
  // into the plan's frame permutes and negates components, so the cells' own frames decide.
  const int64_t offdiag = first_offdiagonal_cell(h_Gc);
  if (tun.metric == WF_METRIC_AXES && offdiag >= 0) {
    set_error("wf_op_create: axes metric requested but the G_c of cell " + std::to_string(offdiag)
              + " has a non-zero off-diagonal");
    return WF_ERR_INVALID;
  }
  op->geom = offdiag < 0 && tun.metric != WF_METRIC_FULL ? MarchGeom::cell_axes : MarchGeom::cell;
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
  std::vector<double> p_detJ, p_coeff;
  const double* cell_coeff = nullptr;   // the cell coefficient in the internal cell order (null: none)
  bool identity_cells = true;
  bool have_mesh = false;
  HexMesh mesh{};
  const double* h_detJ = nullptr;
  std::vector<int32_t> p_dofmap;
  const int32_t* dofmap = nullptr;   // the tensor-ordered dofmap in the internal cell order: what d_dofmap holds
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
  if ((rc = op->d_slot.upload(tslot)) != WF_OK) return rc;
  if ((rc = op->d_row_off.upload(row_off)) != WF_OK) return rc;
  return op->d_v.alloc(ncells * nd);
}

int batch_stiffness(const wf_op_desc* desc, const CallerFrame& fr, const BatchInputs& in, bool no_unique, wf_op* op)
{
  const int P = op->P, n = op->n, nd = op->nd, CB = cells_per_batch(P);
  const size_t ncells = (size_t)desc->ncells, nbatch = (ncells + CB - 1) / CB;
  int rc;
  // batch-unique dof lists (WF_KERNEL_FORCE_ELEMENTWISE keeps the element-wise scatter for comparison)
  const bool unique = !no_unique && ncells > 0 && !op->ordered;
  if (unique && (rc = upload_unique_lists(op, in.dofmap, ncells, nd, CB)) != WF_OK) return rc;
  op->kernel = op->ordered ? OpKernel::ordered_stiffness : unique ? OpKernel::generic_unique : OpKernel::generic_elementwise;
  const size_t g6 = nbatch * CB * nd * 6;
  if ((rc = op->d_G6blk.alloc(g6)) != WF_OK) return rc;
  if (g6) WF_HIP_CHECK(hipMemset(op->d_G6blk.data(), 0, g6 * sizeof(double)));
  if (desc->h_G) {
    const bool direct = in.identity_cells && !fr.xslow && !in.cell_coeff;
    const std::vector<int32_t> qm = fr.qmap(n);
    auto fill_cell = [&](size_t c, double* dst) {
      const double* gsrc = desc->h_G + (size_t)in.cperm[c] * nd * 9;
      for (int q = 0; q < nd; ++q) std::memcpy(dst + (size_t)q * 9, gsrc + (size_t)qm[q] * 9, 9 * sizeof(double));
      if (in.cell_coeff)
        for (int e = 0; e < nd * 9; ++e) dst[e] *= in.cell_coeff[c];
    };
    return stage_G9(P, CB, ncells, direct ? desc->h_G : nullptr, fill_cell, op->d_G6blk.data());
  }
  if (in.have_mesh) {
    std::vector<double> pts(n), wts(n);
    gll_points_weights(n, pts.data(), wts.data());
    return mesh_geometry_rule(n, pts.data(), wts.data(), in.mesh, fabs_flag(desc->flags), clamp_flag(desc->flags), in.cell_coeff,
                              nullptr, op->d_G6blk.data(), nullptr);
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
    if ((rc = op->d_phi1.upload(desc->h_phi1, (size_t)nq1 * n)) != WF_OK) return rc;
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
  if (unique && (rc = upload_unique_lists(op, in.dofmap, ncells, nd, CBm)) != WF_OK) return rc;

  if (desc->h_detJ) {
    if ((rc = op->d_detJ.upload(in.h_detJ, ncells * op->nq)) != WF_OK) return rc;
  } else if (in.have_mesh) {
    // det J * w at the caller's tensor rule (precompute.hpp:49-116, mass.hpp:35-39); lumped mass: at the GLL nodes
    std::vector<double> pts(n), wts(n);
    if (!dense) gll_points_weights(n, pts.data(), wts.data());
    if ((rc = op->d_detJ.alloc(ncells * op->nq)) != WF_OK) return rc;
    if ((rc = mesh_geometry_rule(nq1, dense ? desc->h_qpts1 : pts.data(), dense ? desc->h_qwts1 : wts.data(), in.mesh,
                                 fabs_flag(desc->flags), 0, in.cell_coeff, nullptr, nullptr, op->d_detJ.data())) != WF_OK)
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
  DevArray<double> d_ones;
  if ((rc = d_ones.alloc((size_t)op->ndofs)) != WF_OK) return rc;
  if ((rc = op->d_mdiag.alloc((size_t)op->ndofs)) != WF_OK) return rc;
  if (op->ndofs) {
    if ((rc = wf_fill(op->ndofs, 1.0, d_ones.data(), nullptr)) != WF_OK) return rc;
    WF_HIP_CHECK(hipMemset(op->d_mdiag.data(), 0, op->d_mdiag.bytes()));
    // WF_FLAG_ORDERED: the same sequence through the two ordered passes, so that m is bitwise reproducible
    if (ncells && op->ordered) {
      if ((rc = launch_mass_lumped_ordered((int64_t)ncells * nd, op->d_dofmap.data(), op->d_slot.data(), op->d_detJ.data(),
                                           d_ones.data(), op->d_v.data(), nullptr)) != WF_OK)
        return rc;
      if ((rc = wf_segment_sum_add(op->ndofs, op->d_row_off.data(), op->d_v.data(), op->d_mdiag.data(), nullptr)) != WF_OK) return rc;
    } else if (ncells && (rc = launch_mass_lumped((int64_t)ncells * nd, op->d_dofmap.data(), op->d_detJ.data(), d_ones.data(),
                                                  op->d_mdiag.data(), nullptr)) != WF_OK) {
      return rc;
    }
    WF_HIP_CHECK(hipDeviceSynchronize());
  }
  // the diagonal is all the apply reads: det J and the ordered plan go (empty already without WF_FLAG_ORDERED)
  op->d_detJ.reset();
  op->d_slot.reset();
  op->d_row_off.reset();
  op->d_v.reset();
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
  if (desc->h_cell_coeff) {
    in.cell_coeff = desc->h_cell_coeff;
    if (!in.identity_cells) {
      in.p_coeff.resize(ncells);
      for (size_t c = 0; c < ncells; ++c) in.p_coeff[c] = desc->h_cell_coeff[in.cperm[c]];
      in.cell_coeff = in.p_coeff.data();
    }
  }
  if (desc->h_detJ && (!in.identity_cells || fr.xslow || in.cell_coeff)) {
    const int mq = desc->kind == WF_OP_MASS_DENSE ? desc->nq1 : n;
    WF_REQUIRE(mq >= 1 && mq <= 16, "wf_op_create: bad nq1");
    const size_t nqm = (size_t)mq * mq * mq;
    const std::vector<int32_t> qm = fr.qmap(mq);
    in.p_detJ.resize(ncells * nqm);
    for (size_t c = 0; c < ncells; ++c) {
      const double* src = desc->h_detJ + (size_t)in.cperm[c] * nqm;
      for (size_t q = 0; q < nqm; ++q) in.p_detJ[c * nqm + q] = in.cell_coeff ? src[qm[q]] * in.cell_coeff[c] : src[qm[q]];
    }
    in.h_detJ = in.p_detJ.data();
  }
  in.dofmap = tdm;
  if (!in.identity_cells) {
    in.p_dofmap.resize(ncells * nd);
    for (size_t c = 0; c < ncells; ++c) std::memcpy(&in.p_dofmap[c * nd], tdm + (size_t)in.cperm[c] * nd, nd * sizeof(int32_t));
    in.dofmap = in.p_dofmap.data();
  }
  int rc;
  if ((rc = op->d_dofmap.upload(in.dofmap, ncells * nd)) != WF_OK) return rc;
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
  int rc;
  if ((rc = check_hex_degree(P, "wf_op_create")) != WF_OK) return rc;
  WF_REQUIRE(desc->kind == WF_OP_STIFFNESS || desc->kind == WF_OP_MASS_LUMPED || desc->kind == WF_OP_MASS_DENSE,
             "wf_op_create: unknown operator kind");
  if ((rc = check_hex_arrays(desc, "wf_op_create")) != WF_OK) return rc;
  const int n = P + 1, nd = n * n * n;
  const size_t ncells = (size_t)desc->ncells;
  const bool have_mesh = desc->h_xverts && desc->h_geom_dofmap;

  const CallerFrame fr(desc, n);
  OpPtr op = new_op(desc->kind, P, nd, nd, desc->ncells, desc->ndofs, desc->c0, desc->tuning);
  op->cell_coeff = desc->h_cell_coeff != nullptr;
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

}  // extern "C"
