// wf_op_create_box: an operator on a structured box, whose dofmap and vertex lattice are implicit.
#include <cstring>

#include "op.h"

using namespace wf;

namespace {

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

// Kernel, cross-section, geometry form (*geom), metric, update and z segmentation of a box stiffness operator.  h_Gc: the
// per-cell geometry [ncells][6] when *geom != point.  The order of the checks decides which error a bad tuning reports.
int choose_box_stiffness(int P, int nx, int ny, int nz, const double* h_xverts, int flags, const wf_tuning& tun,
                         OpKernel* kernel, BoxChoice* ch, MarchGeom* geom, std::vector<double>& h_Gc)
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
    const bool diagonal = first_offdiagonal_cell(h_Gc) < 0;
    if (tun.metric == WF_METRIC_AXES && !diagonal) {
      set_error("wf_op_create_box: axes metric requested but a cell's G_c has a non-zero off-diagonal");
      return WF_ERR_INVALID;
    }
    *geom = diagonal && tun.metric != WF_METRIC_FULL ? MarchGeom::cell_axes : MarchGeom::cell;
  }
  // update: the owner-computes form of the separable kernel (no atomics) where it measured faster -- P4 -- or on
  // request (P1 to P7); wf_tuning.variant then indexes its own cross-section table.  The per-cell geometry keeps the
  // blocking of the atomic form's cross-section of the same index (P >= 5: of the owner cross-section).
  WF_REQUIRE(tun.update >= WF_UPDATE_AUTO && tun.update <= WF_UPDATE_OWNER, "wf_op_create_box: wf_tuning.update out of range");
  if (*geom == MarchGeom::cell_axes) {
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
  // the axes one); each item pays a prologue of pipeline fill, counted in layers (box_run_plan.h).  Pick the segment
  // length that minimises rounds * (lz + prologue).
  const bool owner = *kernel == OpKernel::box_owner;
  const int ncols = owner ? box_owner_columns(P, nx, ny, ch->obx, ch->oby).count() : box_columns(nx, ny, ch->bx, ch->by).count();
  long resident = owner                                 ? march_owner_resident(P, ch->variant)
                  : *kernel == OpKernel::box_march ? march_resident(P, ch->variant, *geom)
                                                        : march_ks_resident(P, ch->bx, ch->by);
  if (resident <= 0) resident = 512;
  ch->lz = box_uniform_lz(ncols, nz, resident, kMarchPrologue, nullptr, nullptr);
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
  return op->d_Gcell.upload(blk);
}

// WF_FLAG_ORDERED on a box: the box written out as a dofmap mesh (BoxDesc, box_mesh.h), then the dofmap operator of
// wf_op_create -- a box operator with the flag IS that dofmap operator, bit for bit.
int create_box_ordered(int kind, int P, int nx, int ny, int nz, const double* h_xverts, double c0, const double* h_cell_coeff,
                       int flags, const wf_tuning* tuning, wf_op** out)
{
  const BoxDesc box(kind, P, nx, ny, nz, h_xverts, c0, h_cell_coeff, flags, tuning);
  int rc = wf_op_create(&box.desc, out);
  if (rc != WF_OK) return rc;
  (*out)->structured = 1;
  (*out)->nx = nx;
  (*out)->ny = ny;
  (*out)->nz = nz;
  return WF_OK;
}

}  // namespace

int wf::plan_owner_runs(wf_op* op, int resident)
{
  // the plan's column sequence is the kernel's column index: x fastest, as the uniform order (y fastest measured slower)
  const BoxColumns cols = box_owner_columns(op->P, op->nx, op->ny, op->box.obx, op->box.oby);
  const BoxRunPlan plan = box_run_plan(cols.count(), op->nz, resident, kXcds, kOwnerPrologue, op->tun.lz);
  op->h_runs.clear();
  op->runs_longest = plan.longest;
  for (const BoxRun& r : plan.runs) op->h_runs.insert(op->h_runs.end(), {r.col, r.z0, r.z1});
  return op->d_runs.upload(op->h_runs);   // no runs: no array
}

namespace {

// a run table (box_run_plan.h) on the handle and the device; the empty table: the uniform z segments of box.lz run
int install_runs(wf_op* op, std::vector<int32_t> table)
{
  op->h_runs = std::move(table);
  op->runs_longest = op->h_runs.empty() ? op->box.lz : longest_run(op->h_runs);
  return op->d_runs.upload(op->h_runs);   // no runs: no array
}

// shortest of `reps` applies in microseconds
int time_apply(wf_op* op, const double* d_x, double* d_y, hipEvent_t e0, hipEvent_t e1, int reps, float* us)
{
  for (int r = 0; r < reps + 2; ++r) {   // two untimed
    WF_HIP_CHECK(hipEventRecord(e0, nullptr));
    int rc = wf_op_apply(op, d_x, d_y, nullptr);
    if (rc != WF_OK) return rc;
    WF_HIP_CHECK(hipEventRecord(e1, nullptr));
    WF_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.0f;
    WF_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 2) *us = std::min(*us, ms * 1e3f);
  }
  return WF_OK;
}

struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EventPair()
  {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

}  // namespace

// The cut of the whole apply, chosen by timing it ("r19"): the uniform plan against aligned cuts of 4 to 12
// layers per run.  Only at P4, where the bits of y do not depend on the cut, without wf_tuning.lz, and where the uniform
// plan needs more than one round of the resident workgroups: every other operator stays what it was.
int wf::tune_owner_runs(wf_op* op)
{
  int rc = install_runs(op, {});
  const int ncols = box_owner_columns(op->P, op->nx, op->ny, op->box.obx, op->box.oby).count(), nz = op->nz;
  long resident = march_owner_resident(op->P, op->box.variant);
  if (resident <= 0) resident = 512;
  if (rc != WF_OK || !owner_cut_is_timed(op->P, op->tun.lz, ncols, nz, op->box.lz, resident)) return rc;
  DevArray<double> vectors;   // x | y of the timing; no room for them: the uniform plan stays
  if (vectors.alloc(2 * (size_t)op->ndofs) != WF_OK) return (void)hipGetLastError(), WF_OK;
  const double* d_x = vectors.data();
  double* d_y = vectors.data() + op->ndofs;
  WF_HIP_CHECK(hipMemset(vectors.data(), 0, vectors.bytes()));
  EventPair ev;
  WF_HIP_CHECK(hipEventCreate(&ev.e0));
  WF_HIP_CHECK(hipEventCreate(&ev.e1));
  std::vector<int> nsegs = {0};   // 0: the uniform plan
  for (int nseg : owner_cut_candidates(nz)) nsegs.push_back(nseg);
  std::vector<float> us(nsegs.size(), 1e30f);
  for (int pass = 0; pass < 3; ++pass)   // interleaved, so that a clock ramp after idle does not favour a candidate
    for (size_t c = 0; c < nsegs.size(); ++c) {
      if ((rc = install_runs(op, nsegs[c] ? aligned_runs(ncols, nz, nsegs[c]) : std::vector<int32_t>())) != WF_OK) return rc;
      if ((rc = time_apply(op, d_x, d_y, ev.e0, ev.e1, 6, &us[c])) != WF_OK) return rc;
    }
  size_t best = 0;
  for (size_t c = 1; c < nsegs.size(); ++c)
    if (us[c] < us[best] && us[c] < 0.99f * us[0]) best = c;   // a table has to win by more than the timing's noise
  return install_runs(op, nsegs[best] ? aligned_runs(ncols, nz, nsegs[best]) : std::vector<int32_t>());
}

extern "C" {

int wf_box_run_plan(int ncols, int nz, int resident, int nxcd, double prologue, int lz, int32_t* h_runs, int32_t capacity,
                    int32_t* nruns, double* cost, double* uniform_cost, int32_t* uniform_lz)
{
  WF_REQUIRE(ncols > 0 && nz > 0 && resident > 0 && nxcd > 0 && prologue >= 0.0 && nruns, "wf_box_run_plan: bad argument");
  const BoxRunPlan plan = box_run_plan(ncols, nz, resident, nxcd, prologue, lz);
  *nruns = (int32_t)plan.runs.size();
  if (cost) *cost = plan.cost;
  if (uniform_cost) *uniform_cost = plan.uniform_cost;
  if (uniform_lz) *uniform_lz = plan.uniform_lz;
  if (plan.runs.empty()) return WF_OK;
  WF_REQUIRE(h_runs && (size_t)capacity >= plan.runs.size(), "wf_box_run_plan: h_runs holds fewer than *nruns runs");
  static_assert(sizeof(BoxRun) == 3 * sizeof(int32_t), "BoxRun is the table's entry");
  std::memcpy(h_runs, plan.runs.data(), plan.runs.size() * sizeof(BoxRun));
  return WF_OK;
}

int wf_op_replan_runs(wf_op* op, int resident)
{
  WF_REQUIRE(op != nullptr && resident >= 0, "wf_op_replan_runs: bad argument");
  if (op->kernel != OpKernel::box_owner) {
    set_error("wf_op_replan_runs: only the owner form of the box stiffness operator runs by a run table");
    return WF_ERR_UNSUPPORTED;
  }
  WF_HIP_CHECK(hipDeviceSynchronize());   // an apply in flight may still read the table this replaces
  return resident > 0 ? plan_owner_runs(op, resident) : tune_owner_runs(op);
}

int wf_op_set_runs(wf_op* op, const int32_t* h_runs, int32_t nruns)
{
  WF_REQUIRE(op != nullptr && nruns >= 0 && (nruns == 0 || h_runs), "wf_op_set_runs: bad argument");
  if (op->kernel != OpKernel::box_owner) {
    set_error("wf_op_set_runs: only the owner form of the box stiffness operator runs by a run table");
    return WF_ERR_UNSUPPORTED;
  }
  static const char* kFault[4] = {nullptr, "wf_op_set_runs: run outside the mesh or empty",
                                 "wf_op_set_runs: a layer of a column is covered twice",
                                 "wf_op_set_runs: the runs do not cover every layer of every column"};
  const int ncols = box_owner_columns(op->P, op->nx, op->ny, op->box.obx, op->box.oby).count();
  const RunTableFault fault = check_run_table(h_runs, nruns, ncols, op->nz);
  WF_REQUIRE(fault == RunTableFault::none, kFault[(int)fault]);
  WF_HIP_CHECK(hipDeviceSynchronize());   // an apply in flight may still read the table this replaces
  return install_runs(op, std::vector<int32_t>(h_runs, h_runs + 3 * (size_t)nruns));
}

int wf_op_get_runs(const wf_op* op, int32_t* h_runs, int32_t capacity, int32_t* nruns)
{
  WF_REQUIRE(op && nruns, "wf_op_get_runs: null argument");
  *nruns = (int32_t)(op->h_runs.size() / 3);
  if (op->h_runs.empty() || !h_runs) return WF_OK;
  WF_REQUIRE((size_t)capacity >= op->h_runs.size() / 3, "wf_op_get_runs: h_runs holds fewer than *nruns runs");
  std::memcpy(h_runs, op->h_runs.data(), op->h_runs.size() * sizeof(int32_t));
  return WF_OK;
}

int wf_op_create_box(int kind, int degree, int nx, int ny, int nz, const double* h_xverts, double c0, int flags,
                     wf_op** out)
{
  return wf_op_create_box_coeff(kind, degree, nx, ny, nz, h_xverts, c0, nullptr, flags, nullptr, out);
}

int wf_op_create_box_tuned(int kind, int degree, int nx, int ny, int nz, const double* h_xverts, double c0, int flags,
                           const wf_tuning* tuning, wf_op** out)
{
  return wf_op_create_box_coeff(kind, degree, nx, ny, nz, h_xverts, c0, nullptr, flags, tuning, out);
}

int wf_op_create_box_coeff(int kind, int degree, int nx, int ny, int nz, const double* h_xverts, double c0,
                           const double* h_cell_coeff, int flags, const wf_tuning* tuning, wf_op** out)
{
  WF_REQUIRE(out != nullptr, "wf_op_create_box: null output");
  *out = nullptr;
  const int P = degree;
  int rc;
  // the degree is reported ahead of the kind and the tuning, the mesh behind them
  if ((rc = check_hex_degree(P, "wf_op_create_box")) != WF_OK) return rc;
  WF_REQUIRE(kind == WF_OP_STIFFNESS || kind == WF_OP_MASS_LUMPED, "wf_op_create_box: kind must be stiffness or lumped mass");
  WF_REQUIRE(!tuning || tuning->kernel != WF_KERNEL_FORCE_MASS_MARCH,
             "wf_op_create_box: WF_KERNEL_FORCE_MASS_MARCH applies to the dense mass only");
  if ((rc = check_box_args("wf_op_create_box", P, nx, ny, nz, h_xverts)) != WF_OK) return rc;
  const size_t NX = (size_t)P * nx + 1, NY = (size_t)P * ny + 1, NZ = (size_t)P * nz + 1;
  const int n = P + 1, nd = n * n * n;
  const size_t ncells = (size_t)nx * ny * nz;
  if (int bad = check_cell_coeff(h_cell_coeff, ncells, "wf_op_create_box")) return bad;
  if (flags & WF_FLAG_ORDERED) return create_box_ordered(kind, P, nx, ny, nz, h_xverts, c0, h_cell_coeff, flags, tuning, out);

  OpPtr op = new_op(kind, P, nd, nd, nx * ny * nz, (int)(NX * NY * NZ), c0, tuning);
  op->cell_coeff = h_cell_coeff != nullptr;
  op->nq1 = n;
  op->structured = 1;
  op->nx = nx;
  op->ny = ny;
  op->nz = nz;

  op->kernel = OpKernel::diagonal;   // lumped mass: the pre-assembled diagonal
  std::vector<double> h_Gc;          // per-cell geometry, [ncells][6]
  default_box_block(P, op->tun, &op->box.bx, &op->box.by, &op->box.bz);
  if (kind == WF_OP_STIFFNESS
      && (rc = choose_box_stiffness(P, nx, ny, nz, h_xverts, flags, op->tun, &op->kernel, &op->box, &op->geom, h_Gc)) != WF_OK)
    return rc;
  // The cell coefficient enters behind every choice: the affine-cell test, the axes test and the z segmentation have
  // seen the geometry without it.  Per-cell geometry takes it here, in the caller's cell order; the device-built arrays
  // take it in the geometry kernel.
  if (kind == WF_OP_STIFFNESS && op->geom != MarchGeom::point) scale_cell_geometry(h_Gc, h_cell_coeff);

  if ((rc = upload_derivative_tables(op.get(), true)) != WF_OK) return rc;
  DevArray<double> d_x, d_pts, d_wts, d_coeff;
  if (h_cell_coeff && (kind != WF_OP_STIFFNESS || op->geom == MarchGeom::point)
      && (rc = d_coeff.upload(h_cell_coeff, ncells)) != WF_OK)
    return rc;
  const size_t nverts = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
  if ((rc = d_x.upload(h_xverts, nverts * 3)) != WF_OK) return rc;
  if ((rc = upload_tables(P, d_pts, d_wts)) != WF_OK) return rc;

  if (kind == WF_OP_STIFFNESS && op->geom != MarchGeom::point) {
    if ((rc = upload_box_cell_geometry(op.get(), h_Gc)) != WF_OK) return rc;
  } else if (kind == WF_OP_STIFFNESS) {
    const size_t nblk = (size_t)box_columns(nx, ny, op->box.bx, op->box.by).count() * ((nz + op->box.bz - 1) / op->box.bz);
    const size_t g6 = nblk * op->box.bx * op->box.by * op->box.bz * nd * 6;
    if ((rc = op->d_G6blk.alloc(g6)) != WF_OK) return rc;
    WF_HIP_CHECK(hipMemset(op->d_G6blk.data(), 0, g6 * sizeof(double)));
    if ((rc = launch_geometry_box(P, nx, ny, nz, op->box.bx, op->box.by, op->box.bz, d_x.data(), d_pts.data(), d_wts.data(),
                                  fabs_flag(flags), clamp_flag(flags), op->d_G6blk.data(), nullptr, d_coeff.data(), nullptr)) != WF_OK)
      return rc;
  } else {
    // pre-assembled lumped mass diagonal: y += m .* x is 24 B/dof instead of the
    // 34.8 B/dof gather/transform/scatter of spectral_mass.hpp:84-89
    if ((rc = op->d_mdiag.alloc((size_t)op->ndofs)) != WF_OK) return rc;
    WF_HIP_CHECK(hipMemset(op->d_mdiag.data(), 0, (size_t)op->ndofs * sizeof(double)));
    if ((rc = launch_geometry_box(P, nx, ny, nz, 1, 1, 1, d_x.data(), d_pts.data(), d_wts.data(), fabs_flag(flags),
                                  clamp_flag(flags), nullptr, op->d_mdiag.data(), d_coeff.data(), nullptr)) != WF_OK)
      return rc;
  }
  WF_HIP_CHECK(hipDeviceSynchronize());
  if (op->kernel == OpKernel::box_owner && (rc = tune_owner_runs(op.get())) != WF_OK) return rc;
  *out = op.release();
  return WF_OK;
}

}  // extern "C"
