// What is done with an operator handle once it exists: the launch switch, the entry points of the interior / interface
// splits of the marching operators (the split itself: box_items.cpp, march_plan.cpp), wf_op_info and wf_op_destroy --
// and the two dense simplex creators, whose set-up lives with their kernels (stiffness_dense.hip, mass_dense_simplex.hip).
#include "dense_simplex.h"
#include "march_column.h"
#include "op.h"

using namespace wf;

wf_op::~wf_op()
{
  dense_free(dense);
  dense_mass_free(dense_mass);
}

size_t wf::op_device_bytes(const wf_op* op)
{
  size_t total = dense_bytes(op->dense) + dense_mass_bytes(op->dense_mass);
  for (const DevArray<int32_t>* a : {&op->d_dofmap, &op->d_uoff, &op->d_uniq, &op->d_slot, &op->d_row_off, &op->d_items[0],
                                     &op->d_items[1], &op->d_items[2], &op->d_items[3], &op->d_runs, &op->d_item_base, &op->d_item_pattern,
                                     &op->d_item_layers, &op->d_pat_off})
    total += a->bytes();
  for (const DevArray<double>* a : {&op->d_G6blk, &op->d_Gcell, &op->d_detJ, &op->d_D, &op->d_phi1, &op->d_mdiag, &op->d_v})
    total += a->bytes();
  return total + op->d_loc.bytes();
}

namespace {

// the three box marching kernels: work items = columns x z segments (box_items.h), which split into interior / interface
bool is_box_march(OpKernel k)
{
  return k == OpKernel::box_march || k == OpKernel::box_ksplit || k == OpKernel::box_owner;
}

// what the split (box_items.h) takes of a box marching operator: its columns are cells in pieces of bx x by, or the
// owner form's pieces of P*obx x P*oby lattice lines
BoxItemShape item_shape(const wf_op* op)
{
  const bool owner = op->kernel == OpKernel::box_owner;
  return {op->P, op->nx, op->ny, op->nz, owner, owner ? op->box.obx : op->box.bx, owner ? op->box.oby : op->box.by,
          op->box.lz, op->tun.lz0};
}

// the public (geometry, metric, update) of wf_op_info_t for the geometry form of a marching stiffness kernel
void geom_info(MarchGeom geom, int* geometry, int* metric, int* update)
{
  *geometry = geom == MarchGeom::point ? WF_GEOMETRY_PER_POINT : WF_GEOMETRY_PER_CELL;
  *metric = geom == MarchGeom::cell ? WF_METRIC_FULL : geom == MarchGeom::cell_axes ? WF_METRIC_AXES : WF_METRIC_NONE;
  *update = geom == MarchGeom::cell_axes ? WF_UPDATE_ATOMIC : WF_UPDATE_NONE;
}

// uploads the interior / interface work-item lists and the two interior halves
int set_item_lists(wf_op* op, const std::vector<int32_t> (&items)[4])
{
  for (int k = 0; k < 4; ++k) {
    op->nitems[k] = (int)items[k].size();
    int rc = op->d_items[k].upload(items[k]);   // replaces the list of an earlier split
    if (rc != WF_OK) return rc;
  }
  op->have_parts = 1;
  return WF_OK;
}

int set_box_item_lists(wf_op* op, const BoxItemLists& split)
{
  op->lz0_split = split.lz0_split;
  return set_item_lists(op, split.items);
}

}  // namespace

extern "C" {

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
  int rc;
  if ((rc = check_index_range(desc->h_dofmap, (size_t)desc->ncells * desc->nd, desc->ndofs,
                              "wf_op_create_dense_simplex: dofmap entry out of range")) != WF_OK)
    return rc;
  if ((rc = check_index_range(desc->h_geom_dofmap, (size_t)desc->ncells * 4, desc->nverts,
                              "wf_op_create_dense_simplex: vertex index out of range")) != WF_OK)
    return rc;
  if ((rc = check_cell_coeff(desc->h_cell_coeff, (size_t)desc->ncells, "wf_op_create_dense_simplex")) != WF_OK) return rc;
  OpPtr op = new_op(WF_OP_STIFFNESS, 0, desc->nd, desc->nq, desc->ncells, desc->ndofs, desc->c0, nullptr);
  op->cell_coeff = desc->h_cell_coeff != nullptr;
  op->kernel = OpKernel::dense_simplex;
  op->dense_clamp = clamp_flag(desc->flags);
  rc = dense_setup(desc->nd, desc->nq, desc->ncells, desc->ndofs, desc->h_dofmap, desc->h_dphi, desc->h_weights,
                   desc->h_xverts, desc->h_geom_dofmap, desc->h_cell_coeff, &op->dense);
  if (rc != WF_OK) return rc;
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
  int rc;
  if ((rc = check_index_range(desc->h_dofmap, (size_t)desc->ncells * desc->nd, desc->ndofs,
                              "wf_op_create_dense_simplex_mass: dofmap entry out of range")) != WF_OK)
    return rc;
  if ((rc = check_index_range(desc->h_geom_dofmap, (size_t)desc->ncells * 4, desc->nverts,
                              "wf_op_create_dense_simplex_mass: vertex index out of range")) != WF_OK)
    return rc;
  if ((rc = check_cell_coeff(desc->h_cell_coeff, (size_t)desc->ncells, "wf_op_create_dense_simplex_mass")) != WF_OK) return rc;
  OpPtr op = new_op(WF_OP_MASS_DENSE, 0, desc->nd, desc->nq, desc->ncells, desc->ndofs, 0.0, nullptr);
  op->cell_coeff = desc->h_cell_coeff != nullptr;
  op->kernel = OpKernel::dense_simplex_mass;
  rc = dense_mass_setup(desc->nd, desc->nq, desc->ncells, desc->h_dofmap, desc->h_phi, desc->h_weights, desc->h_xverts,
                        desc->h_geom_dofmap, fabs_flag(desc->flags), desc->h_cell_coeff, &op->dense_mass);
  if (rc != WF_OK) return rc;
  *out = op.release();
  return WF_OK;
}

// The one place that maps the kernel choice to a launch.  wf_op_apply runs every work item (d_items null, lz0 = lz);
// wf_op_apply_part the items of one part of a marching operator, whose first z segment has lz0 layers.
static int launch_op(const wf_op* op, int lz0, const int32_t* d_items, int nitems, const double* d_x, double* d_y, hipStream_t s)
{
  // the launchers take plain pointers (null for an array the operator does not have)
  const double *G6blk = op->d_G6blk.data(), *Gcell = op->d_Gcell.data(), *D = op->d_D.data(), *detJ = op->d_detJ.data(),
               *phi1 = op->d_phi1.data(), *mdiag = op->d_mdiag.data();
  const int32_t *dofmap = op->d_dofmap.data(), *uoff = op->d_uoff.data(), *uniq = op->d_uniq.data(), *slot = op->d_slot.data();
  const uint16_t* loc = op->d_loc.data();
  double* v = op->d_v.data();
  switch (op->kernel) {
    case OpKernel::box_march:
      return launch_stiffness_march(op->P, op->box.variant, op->geom, op->nx, op->ny, op->nz, op->box.lz, lz0, G6blk, Gcell, D,
                                    march_table(op), op->coeff, d_x, d_y, d_items, nitems, s);
    case OpKernel::box_ksplit:
      return launch_stiffness_march_ks_box(op->P, op->box.bx, op->box.by, op->nx, op->ny, op->nz, op->box.lz, lz0, G6blk, D,
                                           op->dm, op->coeff, d_x, d_y, d_items, nitems, s);
    case OpKernel::box_owner:
      // the whole apply by the run table when the operator has one (lz < 0 says so to the launcher)
      if (!d_items && op->d_runs.size())
        return launch_stiffness_march_owner(op->P, op->box.variant, op->nx, op->ny, op->nz, -1, -1, op->box.bx, op->box.by, Gcell,
                                            D, op->am, op->coeff, d_x, d_y, op->d_runs.data(), (int)(op->d_runs.size() / 3), s);
      return launch_stiffness_march_owner(op->P, op->box.variant, op->nx, op->ny, op->nz, op->box.lz, lz0, op->box.bx, op->box.by,
                                          Gcell, D, op->am, op->coeff, d_x, d_y, d_items, nitems, s);
    case OpKernel::box_block:
      return launch_stiffness_box(op->P, op->nx, op->ny, op->nz, op->box.bx, op->box.by, op->box.bz, G6blk, D, op->dm,
                                  op->coeff, d_x, d_y, s);
    case OpKernel::idx_march:
      return launch_stiffness_march_idx(op->P, op->geom, op->plan, op->geom == MarchGeom::point ? G6blk : Gcell, D,
                                        march_table(op), op->coeff, d_x, d_y, d_items, nitems, s);
    case OpKernel::generic_unique:
      return launch_stiffness_generic_u(op->P, op->ncells, uoff, uniq, loc, G6blk, D, op->dm, op->coeff, d_x, d_y, s);
    case OpKernel::generic_elementwise:
      return launch_stiffness_generic(op->P, op->ncells, dofmap, G6blk, D, op->dm, op->coeff, d_x, d_y, s);
    case OpKernel::lumped_unique:
      return launch_mass_lumped_u(op->ncells, op->nd, op->unique_cb, uoff, uniq, loc, detJ, d_x, d_y, s);
    case OpKernel::lumped_elementwise: return launch_mass_lumped((int64_t)op->ncells * op->nd, dofmap, detJ, d_x, d_y, s);
    case OpKernel::diagonal:
      if (op->diag_named_only) return launch_diagonal_named(op->ndofs, mdiag, d_x, d_y, s);
      return wf_pointwise_mult_add(op->ndofs, mdiag, d_x, d_y, s);
    case OpKernel::mass_march: return launch_mass_march(op->P, op->nq1, op->plan, detJ, phi1, d_x, d_y, s);
    case OpKernel::mass_column: return launch_mass_dense_col(op->P, op->ncells, uoff, uniq, loc, phi1, detJ, d_x, d_y, s);
    case OpKernel::mass_any:   // with the unique-dof tile when creation built the lists (d_uoff)
      return launch_mass_dense(op->P, op->nq1, op->ncells, dofmap, uoff, uniq, loc, op->unique_cb, phi1, detJ, d_x, d_y, s);
    case OpKernel::dense_simplex: return launch_stiffness_dense(op->dense, op->coeff, op->dense_clamp, d_x, d_y, s);
    case OpKernel::dense_simplex_mass: return launch_mass_dense_simplex(op->dense_mass, d_x, d_y, s);
    case OpKernel::ordered_stiffness:
    case OpKernel::ordered_mass:
    case OpKernel::ordered_lumped: {
      // pass 1 into the operator's scratch v, pass 2 behind it on the same stream
      int rc = op->kernel == OpKernel::ordered_stiffness
                   ? launch_stiffness_ordered(op->P, op->ncells, dofmap, slot, G6blk, D, op->dm, op->coeff, d_x, v, s)
               : op->kernel == OpKernel::ordered_mass
                   ? launch_mass_dense_ordered(op->P, op->nq1, op->ncells, dofmap, slot, phi1, detJ, d_x, v, s)
                   : launch_mass_lumped_ordered((int64_t)op->ncells * op->nd, dofmap, slot, detJ, d_x, v, s);
      if (rc != WF_OK || op->ncells == 0) return rc;
      return wf_segment_sum_add(op->ndofs, op->d_row_off.data(), v, d_y, s);
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
  return set_box_item_lists(op, split_box_items_by_faces(item_shape(op), ghost_x0 != 0, ghost_y0 != 0, ghost_z0 != 0));
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
  if (box) return set_box_item_lists(op, split_box_items_by_ghosts(item_shape(op), ghost));
  // the plan's item arrays are read back from the handle's device copies: the handle keeps no host copy
  std::vector<int32_t> items[4], base, pat, pat_off;
  int rc;
  if ((rc = op->d_item_base.download(base)) != WF_OK) return rc;
  if ((rc = op->d_item_pattern.download(pat)) != WF_OK) return rc;
  if ((rc = op->d_pat_off.download(pat_off)) != WF_OK) return rc;
  split_items_by_ghost(base, pat, pat_off, op->plan.tile_size, ghost, items[0], items[1]);
  alternate_interior(items);
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
  return launch_op(op, op->lz0_split, op->d_items[k].data(), op->nitems[k], d_x, d_y, (hipStream_t)stream);
}

int wf_op_info(const wf_op* op, wf_op_info_t* info)
{
  WF_REQUIRE(op && info, "wf_op_info: null argument");
  // the public description of the kernel choice
  int kernel = WF_KERNEL_NONE, geometry = WF_GEOMETRY_AUTO, metric = WF_METRIC_NONE, update = WF_UPDATE_NONE;
  bool plan = false;
  switch (op->kernel) {
    case OpKernel::box_march: kernel = WF_KERNEL_MARCH_BOX, geom_info(op->geom, &geometry, &metric, &update); break;
    case OpKernel::box_ksplit: kernel = WF_KERNEL_MARCH_BOX, geometry = WF_GEOMETRY_PER_POINT; break;
    case OpKernel::box_owner:
      kernel = WF_KERNEL_MARCH_BOX, geometry = WF_GEOMETRY_PER_CELL, metric = WF_METRIC_AXES, update = WF_UPDATE_OWNER;
      break;
    case OpKernel::box_block: kernel = WF_KERNEL_BOX_BLOCK, geometry = WF_GEOMETRY_PER_POINT; break;
    case OpKernel::idx_march: kernel = WF_KERNEL_MARCH_IDX, plan = true, geom_info(op->geom, &geometry, &metric, &update); break;
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
  if (dense && op->cell_coeff) info->alg_bytes += 8.0 * op->ncells;   // the one per-cell array the coefficient adds
  // order-fixed accumulation: per element-local entry the slot (4), the store and the load of v (8 + 8); the row offsets
  if (kernel == WF_KERNEL_CELLS_ORDERED) info->alg_bytes += 20.0 * op->ncells * op->nd + 4.0 * (op->ndofs + 1.0);
  info->device_bytes = op_device_bytes(op);
  info->items_interior = op->nitems[0];
  info->items_interface = op->nitems[1];
  info->kernel = kernel;
  info->plan_items = plan ? op->plan.nitems : 0;
  info->plan_patterns = plan ? op->plan_patterns : 0;
  info->plan_lz = plan ? op->plan.lz : op->d_runs.size() ? op->runs_longest : is_box_march(op->kernel) ? op->box.lz : 0;
  info->plan_reoriented = op->plan_reoriented;
  info->plan_fill = op->plan_fill;
  info->geometry = geometry;
  info->metric = metric;
  info->update = update;
  info->cell_coeff = op->cell_coeff;
  return WF_OK;
}

int wf_op_destroy(wf_op* op)
{
  delete op;
  return WF_OK;
}

}  // extern "C"
