// Dense mass operator for affine simplex cells: the reference's MassOperator (common/cuda/mass.hpp:18-107,
// y_e = Phi^T (det J w .* (Phi x_e))) with an arbitrary dense table phi[nq][nd].  On an affine cell det J is one
// number, so the two products collapse into one matrix per operator and one scale per cell:
//
//   A[nd][nd]      = Phi^T diag(w) Phi                      (host, long double, rounded once)
//   Y[nd][cells]   = A . U[nd][cells]                       (MFMA, f64 16x16x4, k = nd)
//   y[dof]        += s_c Y[.][c],  s_c = |det J_c| (det J_c with WF_FLAG_NO_FABS, mass.hpp:35-39)
//
// The cost does not depend on nq.  The decomposition is that of k_stiffness_dense (stiffness_dense.hip), and what the
// two kernels share -- batch shape, LDS layout of the matrix, prefetch pieces and the rules of the batch pipeline, the
// device plan -- is dense_simplex.h.  DT KT MFMAs per batch (27 at P4, against 288 in the stiffness kernel): the kernel
// is not bound by the matrix pipe.
//
// Measured (P4 Kuhn box of 54^3 cubes, 944 784 cells, 10.2 M dofs, 125-point rule; five rounds alternating with the
// stiffness apply and with every variant below in one process): 0.135 ms against 0.493 ms for k_stiffness_dense,
// 0.28 of 8 TB/s on alg_bytes.  What bounds it is the rate of the global fp64 atomics: a batch leaves with ~1154
// of them (18 wave-instructions of 512 B), 17 M per apply, and every variant of the pipeline in front of them landed
// within 3 % of the others:
//   workgroups per CU      2: 0.1349 ms (0.1347-0.1351)   3: 0.1380 (0.1372-0.1389)   4: 0.1393 (0.1386-0.1398)
//   x gather one batch later (issued behind the MFMAs for batch b + G, as k_stiffness_dense does), 3 and 4
//   workgroups per CU: 0.1371 / 0.1371 -- no gain over issuing it a whole iteration ahead (0.1380 / 0.1393)
//   without the MFMAs of the third tile at P4 (wrong results; the most the stiffness kernel's XR rows could save):
//   0.1398 / 0.1400 at 3 / 4 workgroups per CU -- nothing, so XR is not built.
// Fewer atomics (larger batches, or an owner form) is what would make it faster, not the gather pipeline.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "dense_simplex.h"

namespace wf {

typedef double double4_t __attribute__((ext_vector_type(4)));

// Workgroups per CU of the persistent grid: the grid is min(nbatch, 256 kMassWgsPerCU) workgroups of one wave per SIMD.
// The registers are capped so that this many are resident (amdgpu_waves_per_eu); LDS is 35 KB at P4 with NU = 5 and
// 51 KB with NU = 9, so up to three would fit in every case.  Two measured fastest (above); -DWF_MASS_WGS_PER_CU=n
// builds another count (tools/variant_lib.sh).
#ifndef WF_MASS_WGS_PER_CU
#define WF_MASS_WGS_PER_CU 2
#endif
constexpr int kMassWgsPerCU = WF_MASS_WGS_PER_CU;
constexpr int kMassGridBound = 256 * kMassWgsPerCU;

// KT = ceil(nd/4) k-steps, DT = ceil(nd/16) output tiles; A lives in LDS as [16 DT][KP], KP = dense_pitch(KT), with
// output row 16 dt + m stored at row 16 dt + dense_row_perm(m): the A operand of tile dt and k-step ks is
// A[16 dt + lc][4 ks + lg], and with that pitch and row order the 32 lanes an LDS read serves at a time touch 32
// distinct 8-byte banks (dense_simplex.h).
// The B operand of k-step ks is dof 4 ks + lg of cell lc; accumulator register r of tile dt is dof 4 (4 dt + r) + lg of
// the same cell, so the packed local indices loc serve the gather and the scatter.
// NU: unique dofs of a batch per thread (DenseBatchShape).
template <int KT, int DT, int NW, int NU>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(kMassWgsPerCU))) void k_mass_dense_simplex(
    int nd, int ncells, int nbatch, int numax,
    const double* __restrict__ Ag,      // [16 DT][KP] padded matrix, rows permuted
    const double* __restrict__ sg,      // [nbatch * 16 NW] scale per cell slot (0 in the padded slots)
    const uint32_t* __restrict__ locP,  // [nbatch][ceil(KT/2)][4][16 NW]: local index of dof 4(2j)+lg | that of dof 4(2j+1)+lg << 16
    const int32_t* __restrict__ uoff,   // [nbatch+1]
    const int32_t* __restrict__ uniq,   // unique dofs of all batches
    const double* __restrict__ x, double* __restrict__ y)
{
  using Shape = DenseBatchShape<KT, NW, NU>;
  constexpr int KP = Shape::KP, NT = Shape::NT, NCB = Shape::NCB, KT2 = Shape::KT2;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* A = smem;              // [16 DT][KP]
  double* Xu = A + 16 * DT * KP; // [numax]  x at the unique dofs of the batch
  double* Yu = Xu + numax;       // [numax]  sum of the cell results per unique dof

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lc = lane & 15, lg = lane >> 4;
  for (int p = t; p < 16 * DT * KP; p += NT) A[p] = Ag[p];

  // Software pipeline over the batches of this (persistent) workgroup, all in registers: while batch b is computed the
  // x values of batch b + G, the indices and scales of batch b + G and the unique-dof lists of batches b + G and b + 2G
  // are held or in flight.  The x gather of batch b + 2G goes out at the END of iteration b (its index list arrived
  // during the iteration) and is consumed at the end of iteration b + G: a whole iteration covers its latency, and no
  // load ever waits on an index that was fetched behind a global atomic.
  const int G = gridDim.x;
  // the prefetch pieces and their rules: dense_simplex.h
  auto load_range = [&](int b) { return dense_load_range(uoff, nbatch, b); };
  auto load_uq = [&](int32_t (&uq)[NU], const DenseRange& rg) { dense_load_uq<NT>(uq, uniq, rg, t); };
  // count_of and the locP load of load_cell are the same lines as in k_stiffness_dense: as shared functions they changed
  // the code (profiles/r23_summary.md)
  auto count_of = [&](const DenseRange& rg) { return rg.live ? rg.hi - rg.lo : 0; };
  auto load_x = [&](double (&xr)[NU], const int32_t (&uq)[NU]) { dense_load_x(xr, x, uq); };
  auto load_cell = [&](uint32_t (&loc)[KT2], double& s, int b) {
    const int bb = b < nbatch ? b : nbatch - 1;
#pragma unroll
    for (int j = 0; j < KT2; ++j) loc[j] = locP[(((size_t)bb * KT2 + j) * 4 + lg) * NCB + wave * 16 + lc];
    s = sg[(size_t)bb * NCB + wave * 16 + lc];
  };
  int32_t uq_cur[NU], uq_nxt[NU];   // unique dofs (this thread's share) of the batch being computed / of the next one
  double xr[NU];                    // x at uq_nxt
  uint32_t loc[KT2], locn[KT2];
  auto loc_of = [&](int ks) { return dense_loc_of(loc, ks); };
  double sc, scn;
  int nu_cur, nu_nxt;   // live entries of uq_cur / uq_nxt
  // prologue: first batch straight into LDS, list and x values of the second
  {
    const DenseRange r0 = load_range(blockIdx.x), r1 = load_range(blockIdx.x + G);
    load_uq(uq_cur, r0);
    nu_cur = count_of(r0);
    load_x(xr, uq_cur);
    load_cell(loc, sc, blockIdx.x);
    load_uq(uq_nxt, r1);
    nu_nxt = count_of(r1);
#pragma unroll
    for (int m = 0; m < NU; ++m) {
      const int u = t + NT * m;
      if (u < numax) {
        Xu[u] = xr[m];
        Yu[u] = 0.0;
      }
    }
    load_x(xr, uq_nxt);
  }
  DenseRange rg2 = load_range(blockIdx.x + 2 * G);   // range of the batch whose unique-dof list is fetched next

  for (int batch = blockIdx.x; batch < nbatch; batch += G) {
    __syncthreads();   // Xu holds this batch's x values, Yu is zero (first round: A is staged)

    // B operands: this lane's dof values, one per k-step
    double ub[KT];
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) {
      const double v = Xu[loc_of(ks)];   // padded k: local index 0, a valid entry
      ub[ks] = (4 * ks + lg) < nd ? v : 0.0;
    }
    // indices and scales of the next batch, index list of the one after it
    int32_t uq_nn[NU];
    load_cell(locn, scn, batch + G);
    load_uq(uq_nn, rg2);
    const int nu_nn = count_of(rg2);
    const DenseRange rg3 = load_range(batch + 3 * G);

    // ---- Y = A . U.  The A operands come from LDS two k-steps ahead in rotating registers: written as "read, then
    // MFMA" every k-step pays the LDS latency.  (The rotation of the first product of k_stiffness_dense, with DT row
    // sets 16 KP apart: stiffness_dense.hip explains it.)
    double4_t Y[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) Y[dt] = double4_t{0.0, 0.0, 0.0, 0.0};
    const double* Aa = A + dense_row_perm(lc) * KP + lg;   // + 16 dt KP + 4 ks
    double a3[3][DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) a3[0][dt] = Aa[16 * dt * KP];
    if (KT > 1) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) a3[1][dt] = Aa[16 * dt * KP + 4];
    }
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) {
      if (ks + 2 < KT) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) a3[(ks + 2) % 3][dt] = Aa[16 * dt * KP + 4 * (ks + 2)];
      }
      __builtin_amdgcn_sched_barrier(0);   // keep the reads above the MFMAs
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) Y[dt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a3[ks % 3][dt], ub[ks], Y[dt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- scale by s_c (every accumulator entry of a lane belongs to cell lc), sum per unique dof in LDS.  A padded
    // cell slot of the last batch must not scatter: its operands are those of local index 0, and 0 * inf is not 0.
    const bool cell_live = (size_t)batch * NCB + wave * 16 + lc < (size_t)ncells;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ks = 4 * dt + r;   // d = 16 dt + lg + 4 r = 4 ks + lg
        if (ks < KT && cell_live && 4 * ks + lg < nd) atomicAdd(&Yu[loc_of(ks < KT ? ks : 0)], sc * Y[dt][r]);
      }
    __syncthreads();   // Yu complete; every wave has taken its operands out of Xu
    // End-of-batch stage, the same lines as in k_stiffness_dense (stiffness_dense.hip) but for the x gather, which is
    // issued here for batch + 2G; written out in both, see rule 3 of dense_simplex.h: every consumer of a prefetched
    // register (xr, uq_nn, locn, scn, the next ranges) and that gather come BEFORE the first global atomic.
    double yv[NU];
    int32_t uq_old[NU];
#pragma unroll
    for (int m = 0; m < NU; ++m) {
      const int u = t + NT * m;
      yv[m] = u < numax ? Yu[u] : 0.0;
      uq_old[m] = uq_cur[m];
    }
#pragma unroll
    for (int m = 0; m < NU; ++m) {
      const int u = t + NT * m;
      if (u < numax) {   // same thread, same entries: next batch's x values in, sums back to zero
        Xu[u] = xr[m];
        Yu[u] = 0.0;
      }
      uq_cur[m] = uq_nxt[m];
      uq_nxt[m] = uq_nn[m];
    }
    load_x(xr, uq_nxt);   // x of batch + 2G
#pragma unroll
    for (int j = 0; j < KT2; ++j) loc[j] = locn[j];
    sc = scn;
    rg2 = rg3;
    const int nu_old = nu_cur;
    nu_cur = nu_nxt;
    nu_nxt = nu_nn;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int m = 0; m < NU; ++m) {
      if (t + NT * m < nu_old) unsafeAtomicAdd(&y[uq_old[m]], yv[m]);
    }
  }
}

struct DenseMassData {
  int nd = 0, nq = 0, KT = 0, DT = 0, ncells = 0;
  DevArray<double> d_A, d_s;
  DenseBatchPlanDev plan;
};

void dense_mass_free(DenseMassData* d) { delete d; }

size_t dense_mass_bytes(const DenseMassData* d)
{
  return d ? d->d_A.bytes() + d->d_s.bytes() + d->plan.bytes() : 0;
}

// Compiled tile pairs (KT, DT): Lagrange P1..P4 on the tetrahedron, nd = 4, 10, 20, 35.  Any nd with the same tile
// counts runs on them; nq does not enter the kernel.
#define WF_MASS_SIMPLEX_SHAPES(F) F(1, 1) F(3, 1) F(5, 2) F(9, 3)

#define WF_MASS_HAS(K, D) || (KT == K && DT == D)
static bool mass_simplex_shape_compiled(int KT, int DT) { return false WF_MASS_SIMPLEX_SHAPES(WF_MASS_HAS); }
#undef WF_MASS_HAS

// Host setup: A = Phi^T diag(w) Phi in the padded LDS layout, s_c per cell slot, the batch plan of the dense simplex
// kernels.  Nothing touches the device before every check on the caller's data has passed.
int dense_mass_setup(int nd, int nq, int ncells, const int32_t* dofmap, const double* phi, const double* weights,
                     const double* xverts, const int32_t* geom_dofmap, int use_fabs, const double* cell_coeff,
                     DenseMassData** out)
{
  std::unique_ptr<DenseMassData, void (*)(DenseMassData*)> d(new DenseMassData, dense_mass_free);
  d->nd = nd;
  d->nq = nq;
  d->KT = (nd + 3) / 4;
  d->DT = (nd + 15) / 16;
  d->ncells = ncells;
  if (!mass_simplex_shape_compiled(d->KT, d->DT)) {
    set_error("wf_op_create_dense_simplex_mass: nd = " + std::to_string(nd) + " (ceil(nd/4) = " + std::to_string(d->KT)
              + ", ceil(nd/16) = " + std::to_string(d->DT) + ") is a shape not compiled (supported: the tile counts of "
              "tetrahedron P1..P4, nd = 1..4, 9..12, 17..20, 33..36)");
    return WF_ERR_UNSUPPORTED;
  }
  constexpr int NCB = kDenseBatchCells;
  const int KP = dense_pitch(d->KT);
  std::vector<double> A((size_t)16 * d->DT * KP, 0.0);
  for (int a = 0; a < nd; ++a)
    for (int b = 0; b < nd; ++b) {
      long double s = 0.0L;
      for (int q = 0; q < nq; ++q) s += (long double)weights[q] * phi[(size_t)q * nd + a] * phi[(size_t)q * nd + b];
      A[(size_t)(16 * (a / 16) + dense_row_perm(a % 16)) * KP + b] = (double)s;
    }
  const int nbatch = (ncells + NCB - 1) / NCB;
  std::vector<double> sc((size_t)nbatch * NCB, 0.0);
  for (int c = 0; c < ncells; ++c) {
    long double J[9];
    const double det = (double)tet_jacobian(xverts, geom_dofmap + (size_t)c * 4, J);
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) {   // det J = 0, NaN, infinite
      set_error("wf_op_create_dense_simplex_mass: cell " + std::to_string(c) + " is degenerate (det J is zero or not finite)");
      return WF_ERR_INVALID;
    }
    sc[c] = use_fabs ? std::fabs(det) : det;
    if (cell_coeff) sc[c] *= cell_coeff[c];   // the cell coefficient: folded into s_c, rounded once
  }
  int rc;
  if ((rc = d->plan.build(nd, d->KT, ncells, dofmap)) != WF_OK) return rc;
  if (d->plan.numax > dense_nu(d->plan.numax) * kDenseThreads) {   // cannot happen: 64 cells of nd <= 36 dofs
    set_error("mass_dense_simplex: more unique dofs in a batch than the kernel holds");
    return WF_ERR_UNSUPPORTED;
  }
  if ((rc = d->d_A.upload(A)) != WF_OK) return rc;
  if ((rc = d->d_s.upload(sc)) != WF_OK) return rc;
  *out = d.release();
  return WF_OK;
}

template <int KT, int DT, int NW, int NU>
static int launch_mass_simplex_t(const DenseMassData* d, const double* d_x, double* d_y, hipStream_t s)
{
  const DenseBatchPlanDev& pl = d->plan;
  // at most (16 * 3 * 38 + 2 * 2304) * 8 = 51456 B: below the 64 KB a kernel may take without an attribute
  const size_t lds = ((size_t)16 * DT * dense_pitch(KT) + 2 * pl.numax) * sizeof(double);
  const unsigned nb = (unsigned)std::min(pl.nbatch, kMassGridBound);   // persistent: A is staged into LDS once per workgroup
  hipLaunchKernelGGL((k_mass_dense_simplex<KT, DT, NW, NU>), dim3(nb), dim3(64 * NW), lds, s, d->nd, d->ncells, pl.nbatch,
                     pl.numax, d->d_A.data(), d->d_s.data(), pl.locP.data(), pl.uoff.data(), pl.uniq.data(), d_x, d_y);
  return launch_status("mass_dense_simplex");
}

#define WF_MASS_CASE(K, D)                                                                                                          \
  if (d->KT == K && d->DT == D)                                                                                                     \
    return dense_nu(d->plan.numax) == kDenseNuSmall ? launch_mass_simplex_t<K, D, kDenseWaves, kDenseNuSmall>(d, d_x, d_y, s)       \
                                                    : launch_mass_simplex_t<K, D, kDenseWaves, kDenseNuLarge>(d, d_x, d_y, s);

// (dense_mass_setup has refused every shape that is not in WF_MASS_SIMPLEX_SHAPES)
int launch_mass_dense_simplex(const DenseMassData* d, const double* d_x, double* d_y, hipStream_t s)
{
  if (d->plan.nbatch == 0) return WF_OK;
  WF_MASS_SIMPLEX_SHAPES(WF_MASS_CASE)
  set_error("mass_dense_simplex: shape not compiled");
  return WF_ERR_UNSUPPORTED;
}

}  // namespace wf
