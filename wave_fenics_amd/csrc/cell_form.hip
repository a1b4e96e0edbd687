// Cell forms: e_c(lambda, u) = (P_c lambda)^T A_c (P_c u), one number per cell (wf_cell_form).
//   k_cell_form_stiffness<P, false>  G at every point, the geometry stream of the element-wise batch kernel
//   k_cell_form_stiffness<P, true>   one G_c per affine cell
//   k_cell_form_lumped<P>            the stored det J w
// The batch shape is CellBatch<P>'s and the body that of stiffness_elementwise.h up to out[k] = (A_c u_c)[i, j, k]; the
// scatter is replaced by the products with lambda and a reduction whose order is fixed: a thread sums its column with k
// ascending, the first thread of a cell sums the cell's n^2 columns with ji ascending, and that thread alone stores
// out[c].  No atomics; e_c depends neither on the cell's place in its batch, nor on the batch's other cells, nor on the
// grid.  The kernels have a translation unit of their own: which other kernels a translation unit holds decides how the
// compiler forms their LDS addresses.
#include <cstring>

#include "cell_batch.h"
#include "op.h"
#include "stiffness_core.h"

using namespace wf;

struct wf_cell_form {
  int kind = 0, P = 0, ncells = 0, ndofs = 0;
  int geometry = WF_GEOMETRY_AUTO;   // stiffness: the form that was built; lumped mass: none
  int cell_coeff = 0;
  // the state of the operator set-up (op.h): d_dofmap in tensor order and the caller's cell order, d_D, dm, coeff, and
  // d_G6blk in the batch-blocked layout | d_Gcell [ncells][6] | d_detJ [ncells][nd].  Never applied.
  OpPtr op;
};

namespace wf {

// the column sums of a batch are in part[t]; the first thread of every cell adds its cell's in ascending ji and stores
template <int P>
__device__ __forceinline__ void cell_form_store(const double* part, int cell, bool valid, int ji, int cl, double alpha,
                                                int accumulate, double* __restrict__ out)
{
  constexpr int n2 = CellBatch<P>::n2;
  if (valid && ji == 0) {
    double e = part[cl * n2];
#pragma unroll
    for (int m = 1; m < n2; ++m) e += part[cl * n2 + m];
    const double v = alpha * e;
    out[cell] = accumulate ? out[cell] + v : v;
  }
}

template <int P, bool CELLGEOM>
__global__ __launch_bounds__(256) void k_cell_form_stiffness(int ncells, const int32_t* __restrict__ dofmap,
                                                             const double2* __restrict__ G, const double* __restrict__ dD,
                                                             DMat dm, double coeff, const double* __restrict__ lam,
                                                             const double* __restrict__ u, double alpha, int accumulate,
                                                             double* __restrict__ out)
{
  constexpr int n = CellBatch<P>::n, n2 = CellBatch<P>::n2, nd = CellBatch<P>::nd;
  constexpr int CB = CellBatch<P>::CB, NT = CellBatch<P>::NT, NFLAT = CellBatch<P>::NFLAT;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* U = smem;                 // [CB][nd]
  double* Fr = U + CB * nd;         // [CB][nd]
  double* Fs = Fr + CB * nd;        // [CB][nd]
  double* sD = Fs + CB * nd;        // [n][n]

  const int t = threadIdx.x;
  const size_t batch = blockIdx.x;
  const int cell0 = (int)batch * CB;
  const bool active = t < NT;
  const int cl = t / n2, ji = t % n2, j = ji / n, i = ji % n;
  const bool valid = active && cell0 + cl < ncells;   // padded cells of the last batch: zeros in, nothing out

  // 1. geometry first: the stream of the batch (padded cells read zeros), or the cell's G_c
  [[maybe_unused]] double2 g[n][3];
  [[maybe_unused]] double2 gcw[3];
  [[maybe_unused]] double wk[n];
  if constexpr (CELLGEOM) {
    const double cw = coeff * dD[2 * n2 + i] * dD[2 * n2 + j];
#pragma unroll
    for (int k = 0; k < n; ++k) wk[k] = dD[2 * n2 + k];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const double2 gc = valid ? G[(size_t)(cell0 + cl) * 3 + p] : make_double2(0.0, 0.0);
      gcw[p] = make_double2(cw * gc.x, cw * gc.y);
    }
  } else if (active) {
    const double2* gp = G + (batch * n * 3) * (size_t)NT + t;
#pragma unroll
    for (int k = 0; k < n; ++k)
#pragma unroll
      for (int p = 0; p < 3; ++p) g[k][p] = load_stream(gp + (size_t)(k * 3 + p) * NT);
  }
  if (t < n * n) sD[t] = dD[t];

  // 2. u: flat, coalesced gather into the tile; lambda: the thread's own column straight into registers
  const int nvalid = min(CB, ncells - cell0) * nd;
#pragma unroll
  for (int m = 0; m < NFLAT; ++m) {
    const int pos = t + 256 * m;
    if (pos < nvalid)
      U[pos] = u[dofmap[(size_t)cell0 * nd + pos]];
    else if (pos < CB * nd)
      U[pos] = 0.0;
  }
  double lk[n];
#pragma unroll
  for (int k = 0; k < n; ++k) lk[k] = valid ? lam[dofmap[(size_t)(cell0 + cl) * nd + k * n2 + ji]] : 0.0;
  __syncthreads();

  double o[n];
  if constexpr (CELLGEOM) {
    double ft[n];
    stiffness_phase1_cell<P>(U + cl * nd, n2, n, Fr + cl * nd, Fs + cl * nd, sD, dm, gcw, wk, i, j, active, ft);
    __syncthreads();
    stiffness_phase2<P>(Fr + cl * nd, Fs + cl * nd, sD, dm, ft, i, j, active, o);
  } else {
    stiffness_column<P>(U + cl * nd, n2, n, Fr + cl * nd, Fs + cl * nd, sD, dm, g, coeff, i, j, active, o);
  }

  // 3. the column's share, k ascending; through U, whose reads all precede the barrier between the two phases
  if (active) {
    double s = lk[0] * o[0];
#pragma unroll
    for (int k = 1; k < n; ++k) s += lk[k] * o[k];
    U[t] = s;
  }
  __syncthreads();
  cell_form_store<P>(U, cell0 + cl, valid, ji, cl, alpha, accumulate, out);
}

template <int P>
__global__ __launch_bounds__(256) void k_cell_form_lumped(int ncells, const int32_t* __restrict__ dofmap,
                                                          const double* __restrict__ detJ, const double* __restrict__ lam,
                                                          const double* __restrict__ u, double alpha, int accumulate,
                                                          double* __restrict__ out)
{
  constexpr int n = CellBatch<P>::n, n2 = CellBatch<P>::n2, nd = CellBatch<P>::nd;
  constexpr int CB = CellBatch<P>::CB, NT = CellBatch<P>::NT;
  __shared__ double part[256];
  const int t = threadIdx.x;
  const int cell0 = (int)blockIdx.x * CB;
  const int cl = t / n2, ji = t % n2;
  const bool valid = t < NT && cell0 + cl < ncells;
  if (valid) {
    const size_t e0 = (size_t)(cell0 + cl) * nd + ji;
    int32_t d[n];
    double w[n];
#pragma unroll
    for (int k = 0; k < n; ++k) {
      d[k] = dofmap[e0 + k * n2];
      w[k] = detJ[e0 + k * n2];
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < n; ++k) {
      const double mu = u[d[k]] * w[k];   // the lumped apply's own product (spectral_mass.hpp:84-89)
      s = k ? s + lam[d[k]] * mu : lam[d[k]] * mu;
    }
    part[t] = s;
  }
  __syncthreads();
  cell_form_store<P>(part, cell0 + cl, valid, ji, cl, alpha, accumulate, out);
}

}  // namespace wf

namespace {

template <int P>
int launch_cell_form(const wf_cell_form* f, const double* d_lam, const double* d_u, double alpha, int accumulate, double* d_out,
                     hipStream_t s)
{
  const wf_op* op = f->op.get();
  const dim3 grid(CellBatch<P>::batches(f->ncells)), block(256);
  constexpr size_t lds = CellBatch<P>::stiffness_lds_bytes;
  if (f->kind == WF_OP_MASS_LUMPED)
    hipLaunchKernelGGL(k_cell_form_lumped<P>, grid, block, 0, s, f->ncells, op->d_dofmap.data(), op->d_detJ.data(), d_lam, d_u,
                       alpha, accumulate, d_out);
  else if (f->geometry == WF_GEOMETRY_PER_CELL)
    hipLaunchKernelGGL((k_cell_form_stiffness<P, true>), grid, block, lds, s, f->ncells, op->d_dofmap.data(),
                       reinterpret_cast<const double2*>(op->d_Gcell.data()), op->d_D.data(), op->dm, op->coeff, d_lam, d_u, alpha,
                       accumulate, d_out);
  else
    hipLaunchKernelGGL((k_cell_form_stiffness<P, false>), grid, block, lds, s, f->ncells, op->d_dofmap.data(),
                       reinterpret_cast<const double2*>(op->d_G6blk.data()), op->d_D.data(), op->dm, op->coeff, d_lam, d_u, alpha,
                       accumulate, d_out);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

// The per-cell stiffness form: G_c [ncells][6] as hex_cell_geometry left it, times a_c, beside the tensor-ordered dofmap
// and the tables of the box set-up (D, D^T, the 1-D weights).  The per-point arrays are never allocated.
int create_per_cell(const wf_op_desc* desc, std::vector<double>& h_Gc, wf_op* op)
{
  const CallerFrame fr(desc, op->n);
  std::vector<int32_t> store;
  const int32_t* tdm = nullptr;
  int rc;
  if ((rc = tensor_dofmap(desc, fr, op->nd, store, &tdm)) != WF_OK) return rc;
  scale_cell_geometry(h_Gc, desc->h_cell_coeff);
  if ((rc = op->d_dofmap.upload(tdm, (size_t)desc->ncells * op->nd)) != WF_OK) return rc;
  if ((rc = upload_derivative_tables(op, true)) != WF_OK) return rc;
  return op->d_Gcell.upload(h_Gc);
}

}  // namespace

extern "C" {

int wf_cell_form_create(const wf_op_desc* desc, wf_cell_form** out)
{
  WF_REQUIRE(desc && out, "wf_cell_form_create: null argument");
  *out = nullptr;
  if (desc->kind == WF_OP_MASS_DENSE) {
    set_error("wf_cell_form_create: the dense mass has no cell form (kinds: stiffness, lumped mass)");
    return WF_ERR_UNSUPPORTED;
  }
  WF_REQUIRE(desc->kind == WF_OP_STIFFNESS || desc->kind == WF_OP_MASS_LUMPED, "wf_cell_form_create: unknown operator kind");
  const int P = desc->degree;
  int rc;
  if ((rc = check_hex_degree(P, "wf_cell_form_create")) != WF_OK) return rc;
  WF_REQUIRE(!(desc->flags & WF_FLAG_ORDERED),
             "wf_cell_form_create: WF_FLAG_ORDERED does not apply (the form is order-fixed by construction)");
  WF_REQUIRE(!(desc->flags & WF_FLAG_MASS_ELEMENTWISE),
             "wf_cell_form_create: WF_FLAG_MASS_ELEMENTWISE does not apply (the form is element-wise by construction)");
  wf_tuning tun = desc->tuning ? *desc->tuning : wf_tuning{};
  const int geometry = tun.geometry;
  tun.geometry = 0;
  const wf_tuning none{};
  WF_REQUIRE(std::memcmp(&tun, &none, sizeof(wf_tuning)) == 0, "wf_cell_form_create: takes no wf_tuning field other than geometry");
  WF_REQUIRE(geometry >= WF_GEOMETRY_AUTO && geometry <= WF_GEOMETRY_PER_CELL, "wf_cell_form_create: wf_tuning.geometry out of range");
  if ((rc = check_hex_arrays(desc, "wf_cell_form_create")) != WF_OK) return rc;
  const int n = P + 1, nd = n * n * n;
  const size_t ncells = (size_t)desc->ncells;
  const bool have_mesh = desc->h_xverts && desc->h_geom_dofmap;
  const bool stiffness = desc->kind == WF_OP_STIFFNESS;
  if (stiffness)
    WF_REQUIRE(desc->h_G || have_mesh || ncells == 0, "wf_cell_form_create: stiffness needs h_G or the mesh (h_xverts, h_geom_dofmap)");
  else
    WF_REQUIRE(desc->h_detJ || have_mesh || ncells == 0, "wf_cell_form_create: mass needs h_detJ or the mesh (h_xverts, h_geom_dofmap)");

  // geometry of the stiffness form, decided on the host: per cell where the mesh allows it or on request
  std::vector<double> h_Gc;
  bool per_cell = false;
  if (stiffness && geometry == WF_GEOMETRY_PER_CELL && desc->h_G) return per_cell_refuses_G("wf_cell_form_create");
  if (stiffness && geometry != WF_GEOMETRY_PER_POINT && !desc->h_G && have_mesh && ncells > 0) {
    h_Gc.assign(ncells * 6, 0.0);
    int reason = 0;
    const int64_t bad = hex_cell_geometry(P, ncells, desc->h_xverts, desc->h_geom_dofmap, fabs_flag(desc->flags),
                                          clamp_flag(desc->flags), h_Gc.data(), &reason);
    per_cell = bad < 0;
    if (bad >= 0 && geometry == WF_GEOMETRY_PER_CELL) return per_cell_refusal("wf_cell_form_create", bad, reason);
  }

  std::unique_ptr<wf_cell_form> f(new wf_cell_form);
  f->kind = desc->kind;
  f->P = P;
  f->ncells = desc->ncells;
  f->ndofs = desc->ndofs;
  f->cell_coeff = desc->h_cell_coeff != nullptr;
  f->geometry = !stiffness ? WF_GEOMETRY_AUTO : per_cell ? WF_GEOMETRY_PER_CELL : WF_GEOMETRY_PER_POINT;
  if (per_cell) {
    f->op = new_op(desc->kind, P, nd, nd, desc->ncells, desc->ndofs, desc->c0, nullptr);
    f->op->cell_coeff = f->cell_coeff;
    if ((rc = create_per_cell(desc, h_Gc, f->op.get())) != WF_OK) return rc;
  } else {
    // the element-wise batch operator in the caller's cell order is the state the kernels read
    wf_tuning keep{};
    keep.kernel = WF_KERNEL_FORCE_ELEMENTWISE;
    keep.keep_cell_order = 1;
    wf_op_desc d = *desc;
    d.tuning = &keep;
    if (!stiffness) d.flags |= WF_FLAG_MASS_ELEMENTWISE;
    wf_op* op = nullptr;
    if ((rc = wf_op_create(&d, &op)) != WF_OK) return rc;
    f->op.reset(op);
  }
  *out = f.release();
  return WF_OK;
}

int wf_cell_form_create_box(int kind, int degree, int nx, int ny, int nz, const double* h_xverts, double c0,
                            const double* h_cell_coeff, int flags, const wf_tuning* tuning, wf_cell_form** out)
{
  WF_REQUIRE(out != nullptr, "wf_cell_form_create_box: null output");
  *out = nullptr;
  if (int rc = check_box_args("wf_cell_form_create_box", degree, nx, ny, nz, h_xverts)) return rc;
  // the box written out as a dofmap mesh, as for WF_FLAG_ORDERED box operators
  const BoxDesc box(kind, degree, nx, ny, nz, h_xverts, c0, h_cell_coeff, flags, tuning);
  return wf_cell_form_create(&box.desc, out);
}

int wf_cell_form_eval(const wf_cell_form* f, const double* d_lambda, const double* d_u, double alpha, int accumulate,
                      double* d_out, void* stream)
{
  WF_REQUIRE(f && d_lambda && d_u && d_out, "wf_cell_form_eval: null argument");
  if (f->ncells == 0) return WF_OK;
  return dispatch_degree(f->P, "wf_cell_form_eval: degree must be 1..7", [&](auto p) {
    return launch_cell_form<decltype(p)::value>(f, d_lambda, d_u, alpha, accumulate != 0, d_out, (hipStream_t)stream);
  });
}

int wf_cell_form_info(const wf_cell_form* f, wf_cell_form_info_t* info)
{
  WF_REQUIRE(f && info, "wf_cell_form_info: null argument");
  const double nd = (double)f->op->nd, nc = (double)f->ncells;
  info->kind = f->kind;
  info->degree = f->P;
  info->num_cells = f->ncells;
  info->ndofs = f->ndofs;
  info->geometry = f->geometry;
  info->cell_coeff = f->cell_coeff;
  if (f->kind == WF_OP_STIFFNESS)
    info->alg_bytes = nc * (f->geometry == WF_GEOMETRY_PER_CELL ? 48.0 : 48.0 * nd) + 4.0 * nd * nc + 8.0 * nc + 16.0 * f->ndofs;
  else
    info->alg_bytes = nc * (12.0 * nd + 8.0) + 16.0 * f->ndofs;
  info->device_bytes = op_device_bytes(f->op.get());
  return WF_OK;
}

int wf_cell_form_destroy(wf_cell_form* f)
{
  delete f;
  return WF_OK;
}

}  // extern "C"
