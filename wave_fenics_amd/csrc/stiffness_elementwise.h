// Element-wise cell-batch stiffness: arbitrary tensor-ordered dofmap, one batch of CellBatch<P>::CB cells per workgroup.
// One body, two output stages:
//   k_stiffness_generic  (ORDERED = false)  atomic scatter y[dof] += value; carries the ablation masks; launched by
//                                           stiffness_batch.hip under the hint {"kernel": "elementwise"};
//   k_stiffness_ordered  (ORDERED = true)   pass 1 of the order-fixed accumulation: plain store v[slot] = value;
//                                           launched by ordered.hip.
// Every thread of a batch runs the same instruction sequence on its cell, so a cell's arithmetic does not depend on
// where the cell sits.  The two kernels are instantiated in different translation units on purpose: which other
// kernels a translation unit holds decides how the compiler forms their LDS addresses.
#pragma once
#include "cell_batch.h"
#include "stiffness_core.h"  // stiffness_column<P>, load_stream

namespace wf {

template <int P, bool ORDERED>
__device__ __forceinline__ void stiffness_elementwise(int ncells, const int32_t* __restrict__ dofmap,
                                                      const int32_t* __restrict__ slot,
                                                      const double2* __restrict__ G6blk,
                                                      const double* __restrict__ dD, const DMat& dm, double coeff,
                                                      const double* __restrict__ x, double* __restrict__ y,
                                                      [[maybe_unused]] const int ablate)
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

  // 1. issue the whole geometry stream of this batch first (16 B per lane,
  //    contiguous across the wave); padded cells read zeros.
  double2 g[n][3];
  if (active) {
    const double2* gp = G6blk + (batch * n * 3) * (size_t)NT + t;
    if (ablate & 2) gp = G6blk + t;   // diagnostic: every workgroup re-reads batch 0 (L2-resident)
    // batch_load_geometry (stiffness_batch.hip), written out: the call compiles to other code in this kernel
#pragma unroll
    for (int k = 0; k < n; ++k)
#pragma unroll
      for (int p = 0; p < 3; ++p) g[k][p] = load_stream(gp + (size_t)(k * 3 + p) * NT);
  }
  if (t < n * n) sD[t] = dD[t];

  // 2. gather: flat, coalesced dofmap (and slot) reads; the output addresses stay in registers
  int32_t idx[NFLAT];
  const int nvalid = min(CB, ncells - cell0) * nd;
#pragma unroll
  for (int m = 0; m < NFLAT; ++m) {
    const int pos = t + 256 * m;
    idx[m] = -1;
    if (pos < nvalid) {
      if constexpr (ORDERED) {
        idx[m] = slot[(size_t)cell0 * nd + pos];
        U[pos] = x[dofmap[(size_t)cell0 * nd + pos]];
      } else {
        idx[m] = dofmap[(size_t)cell0 * nd + pos];
        U[pos] = (ablate & 4) ? 1.0 + idx[m] : x[idx[m]];
      }
    } else if (pos < CB * nd) {
      U[pos] = 0.0;
    }
  }
  __syncthreads();

  double out[n];
  stiffness_column<P>(U + cl * nd, n2, n, Fr + cl * nd, Fs + cl * nd, sD, dm, g, coeff, i, j, active, out, ablate);

  // 3. element results back through LDS (Fr is free after the second barrier
  //    only for this thread's own entries -> use U, whose reads all precede the
  //    first barrier inside stiffness_column), then the flat output stage: one atomic
  //    scatter-add, or one plain store, per element-local entry.
  if (active) {
#pragma unroll
    for (int k = 0; k < n; ++k) U[cl * nd + k * n2 + ji] = out[k];
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < NFLAT; ++m) {
    const int pos = t + 256 * m;
    if (idx[m] >= 0) {
      if constexpr (ORDERED) {
        y[idx[m]] = U[pos];
      } else if (ablate & 1) {   // diagnostic: no scatter (store kept live, never taken)
        if (U[pos] == 1.2345e300) y[idx[m]] = U[pos];
      } else {
        unsafeAtomicAdd(&y[idx[m]], U[pos]);
      }
    }
  }
}

template <int P>
__global__ __launch_bounds__(256) void k_stiffness_generic(int ncells, const int32_t* __restrict__ dofmap,
                                                           const double2* __restrict__ G6blk,
                                                           const double* __restrict__ dD, DMat dm,
                                                           double coeff, const double* __restrict__ x,
                                                           double* __restrict__ y, int ablate_arg)
{
  stiffness_elementwise<P, false>(ncells, dofmap, nullptr, G6blk, dD, dm, coeff, x, y, WF_ABLATE_FLAGS(ablate_arg));
}

template <int P>
__global__ __launch_bounds__(256) void k_stiffness_ordered(int ncells, const int32_t* __restrict__ dofmap,
                                                           const int32_t* __restrict__ slot,
                                                           const double2* __restrict__ G6blk, const double* __restrict__ dD,
                                                           DMat dm, double coeff, const double* __restrict__ x,
                                                           double* __restrict__ v)
{
  stiffness_elementwise<P, true>(ncells, dofmap, slot, G6blk, dD, dm, coeff, x, v, 0);
}

}  // namespace wf
