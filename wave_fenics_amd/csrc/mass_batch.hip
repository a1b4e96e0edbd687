// Cell-batch mass kernels for hexahedra: the lumped (spectral) mass, element-wise and batch-unique, and the dense mass
// Phi^T D Phi with a tensor-product rule -- the any-rule kernel k_mass_dense (the fall-back for rectangular tables and
// meshes that do not tile; mass_march.hip takes the rest) and the column-thread kernel for square tables.  The
// *_ordered kernels are pass 1 of the order-fixed accumulation (ordered.hip): the same arithmetic per cell, with
// v[slot] = value in place of the atomic add.
#include "cell_batch.h"

namespace wf {

// --------------------------------------------------------------------------
// lumped (spectral) mass: fused gather * detJ -> scatter-add
// replaces the three launches of common/cuda/spectral_mass.hpp:84-89
// --------------------------------------------------------------------------
__global__ void k_mass_lumped(int64_t nentries, const int32_t* __restrict__ dofmap,
                              const double* __restrict__ detJ, const double* __restrict__ x,
                              double* __restrict__ y)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nentries) {
    const int32_t d = dofmap[e];
    unsafeAtomicAdd(&y[d], x[d] * detJ[e]);
  }
}

// pass 1 of the ordered form (spectral_mass.hpp:84-89 without the scatter): v[slot] = x[dof] * detJ
__global__ void k_mass_lumped_ordered(int64_t nentries, const int32_t* __restrict__ dofmap, const int32_t* __restrict__ slot,
                                      const double* __restrict__ detJ, const double* __restrict__ x, double* __restrict__ v)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nentries) v[slot[e]] = x[dofmap[e]] * detJ[e];
}

// the pre-assembled diagonal on vectors with entries that no cell names: m = 0 there, and those entries of x must not
// reach y (0 * NaN) -- the gather / scatter sequence above does nothing with them.  The test is m != 0, not "named": a
// named dof whose contributions cancel exactly (possible only without the fabs of det J) is skipped as well, which
// leaves y as a finite x would.  One entry per thread: it runs on dofmaps with unnamed dofs only.
__global__ void k_diagonal_named(int64_t n, const double* __restrict__ m, const double* __restrict__ x, double* __restrict__ y)
{
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d < n && m[d] != 0.0) y[d] += m[d] * x[d];
}

// batch-unique form of the lumped mass (default): x once per unique dof, the
// batch summed in LDS, one global atomic per unique dof
__global__ __launch_bounds__(256) void k_mass_lumped_u(int ncells, int nd, int CB, const int32_t* __restrict__ uoff,
                                                       const int32_t* __restrict__ uniq,
                                                       const uint16_t* __restrict__ loc,
                                                       const double* __restrict__ detJ,
                                                       const double* __restrict__ x, double* __restrict__ y)
{
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = threadIdx.x;
  const int nbatch = (ncells + CB - 1) / CB;
  for (int batch = blockIdx.x; batch < nbatch; batch += gridDim.x) {
    const int u0 = uoff[batch], nu = uoff[batch + 1] - u0;
    double* Xu = smem;
    double* Yu = smem + nu;
    __syncthreads();
    for (int u = t; u < nu; u += 256) {
      Xu[u] = x[uniq[u0 + u]];
      Yu[u] = 0.0;
    }
    __syncthreads();
    const size_t e0 = (size_t)batch * CB * nd;
    const int ne = min(CB, ncells - batch * CB) * nd;
    for (int p = t; p < ne; p += 256) {
      const int l = loc[e0 + p];
      atomicAdd(&Yu[l], Xu[l] * detJ[e0 + p]);
    }
    __syncthreads();
    for (int u = t; u < nu; u += 256) unsafeAtomicAdd(&y[uniq[u0 + u]], Yu[u]);
  }
}

// --------------------------------------------------------------------------
// dense mass Phi^T D Phi with a tensor-product rule, sum-factorised:
// replaces common/cuda/mass_kernel.cu:5-46 and the DGEMM pair of
// demo/gpu_operator/main.cpp:149-155 / demo/gpu_tsmm (k >> m ~ n).  A workgroup
// processes CB cells at once (P2: 32 cells) so that all 256 lanes work in each of
// the six 1-D contraction passes; the passes ping-pong between two LDS tiles.
// phi1: [m][n] row-major (m 1-D quadrature points, n = P+1 1-D nodes).
// One body, two output stages:
//   k_mass_dense          (ORDERED = false)  y[dof] += value, element-wise or through the unique-dof tile (uoff non-null);
//   k_mass_dense_ordered  (ORDERED = true)   pass 1 of the order-fixed accumulation, no unique-dof tile: out[slot] = value.
// --------------------------------------------------------------------------
template <bool ORDERED>
__device__ __forceinline__ void mass_dense_batches(int n, int m, int CB, int ncells, const int32_t* __restrict__ dofmap,
                                                   const int32_t* __restrict__ slot,
                                                   const int32_t* __restrict__ uoff,   // batch-unique lists or null
                                                   const int32_t* __restrict__ uniq, const uint16_t* __restrict__ loc,
                                                   const double* __restrict__ phi1, const double* __restrict__ detJ,
                                                   const double* __restrict__ x, double* __restrict__ y)
{
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int mx = max(n, m), mx3 = mx * mx * mx;
  double* A = smem;                  // ping  [CB][mx^3]
  double* B = A + CB * mx3;          // pong  [CB][mx^3]
  double* sphi = B + CB * mx3;       // [m][n]
  double* Xu = sphi + m * n;         // [CB * nd] unique-dof tile (batch-unique form)
  const bool unique = !ORDERED && uoff;
  const int t = threadIdx.x;
  const int nd = n * n * n, nq = m * m * m;
  for (int p = t; p < m * n; p += 256) sphi[p] = phi1[p];
  const int nbatch = (ncells + CB - 1) / CB;
  for (int batch = blockIdx.x; batch < nbatch; batch += gridDim.x) {
    const int c0 = batch * CB;
    const int nc = min(CB, ncells - c0);
    __syncthreads();
    int u0 = 0, nu = 0;
    if (unique) {
      u0 = uoff[batch];
      nu = uoff[batch + 1] - u0;
      for (int u = t; u < nu; u += 256) Xu[u] = x[uniq[u0 + u]];
      __syncthreads();
      for (int p = t; p < nc * nd; p += 256) {
        const int c = p / nd, l = p - c * nd;
        A[c * mx3 + l] = Xu[loc[(size_t)c0 * nd + p]];
      }
      __syncthreads();
      for (int u = t; u < nu; u += 256) Xu[u] = 0.0;
    } else {
      for (int p = t; p < nc * nd; p += 256) {
        const int c = p / nd, l = p - c * nd;
        A[c * mx3 + l] = x[dofmap[(size_t)c0 * nd + p]];
      }
    }
    __syncthreads();
    // forward x: B[c][k][j][qi] = sum_i phi[qi][i] A[c][k][j][i]
    for (int p = t; p < nc * n * n * m; p += 256) {
      const int c = p / (n * n * m), r = p - c * (n * n * m);
      const int qi = r % m, kj = r / m;
      double s = 0.0;
      for (int a = 0; a < n; ++a) s += sphi[qi * n + a] * A[c * mx3 + kj * n + a];
      B[c * mx3 + r] = s;
    }
    __syncthreads();
    // forward y: A[c][k][qj][qi] = sum_j phi[qj][j] B[c][k][j][qi]
    for (int p = t; p < nc * n * m * m; p += 256) {
      const int c = p / (n * m * m), r = p - c * (n * m * m);
      const int qi = r % m, qj = (r / m) % m, k = r / (m * m);
      double s = 0.0;
      for (int a = 0; a < n; ++a) s += sphi[qj * n + a] * B[c * mx3 + (k * n + a) * m + qi];
      A[c * mx3 + r] = s;
    }
    __syncthreads();
    // forward z and D: B[c][qk][qj][qi] = detJ * sum_k phi[qk][k] A[c][k][qj][qi]
    for (int p = t; p < nc * nq; p += 256) {
      const int c = p / nq, r = p - c * nq;
      const int qji = r % (m * m), qk = r / (m * m);
      double s = 0.0;
      for (int a = 0; a < n; ++a) s += sphi[qk * n + a] * A[c * mx3 + a * m * m + qji];
      B[c * mx3 + r] = s * detJ[(size_t)(c0 + c) * nq + r];
    }
    __syncthreads();
    // backward z: A[c][k][qj][qi] = sum_qk phi[qk][k] B[c][qk][qj][qi]
    for (int p = t; p < nc * n * m * m; p += 256) {
      const int c = p / (n * m * m), r = p - c * (n * m * m);
      const int qji = r % (m * m), k = r / (m * m);
      double s = 0.0;
      for (int a = 0; a < m; ++a) s += sphi[a * n + k] * B[c * mx3 + a * m * m + qji];
      A[c * mx3 + r] = s;
    }
    __syncthreads();
    // backward y: B[c][k][j][qi] = sum_qj phi[qj][j] A[c][k][qj][qi]
    for (int p = t; p < nc * n * n * m; p += 256) {
      const int c = p / (n * n * m), r = p - c * (n * n * m);
      const int qi = r % m, j = (r / m) % n, k = r / (m * n);
      double s = 0.0;
      for (int a = 0; a < m; ++a) s += sphi[a * n + j] * A[c * mx3 + (k * m + a) * m + qi];
      B[c * mx3 + r] = s;
    }
    __syncthreads();
    // backward x and the output stage: sum_qi phi[qi][i] B[c][k][j][qi] -> y[dof] +=, or out[slot] =
    for (int p = t; p < nc * nd; p += 256) {
      const int c = p / nd, l = p - c * nd;
      const int i = l % n, kj = l / n;
      double s = 0.0;
      for (int a = 0; a < m; ++a) s += sphi[a * n + i] * B[c * mx3 + kj * m + a];
      if constexpr (ORDERED)
        y[slot[(size_t)c0 * nd + p]] = s;
      else if (unique)
        atomicAdd(&Xu[loc[(size_t)c0 * nd + p]], s);
      else
        unsafeAtomicAdd(&y[dofmap[(size_t)c0 * nd + p]], s);
    }
    if (unique) {
      __syncthreads();
      for (int u = t; u < nu; u += 256) unsafeAtomicAdd(&y[uniq[u0 + u]], Xu[u]);
    }
  }
}

__global__ __launch_bounds__(256) void k_mass_dense(int n, int m, int CB, int ncells,
                                                    const int32_t* __restrict__ dofmap,
                                                    const int32_t* __restrict__ uoff,   // batch-unique lists or null
                                                    const int32_t* __restrict__ uniq,
                                                    const uint16_t* __restrict__ loc,
                                                    const double* __restrict__ phi1,
                                                    const double* __restrict__ detJ,
                                                    const double* __restrict__ x, double* __restrict__ y)
{
  mass_dense_batches<false>(n, m, CB, ncells, dofmap, nullptr, uoff, uniq, loc, phi1, detJ, x, y);
}

__global__ __launch_bounds__(256) void k_mass_dense_ordered(int n, int m, int CB, int ncells, const int32_t* __restrict__ dofmap,
                                                            const int32_t* __restrict__ slot, const double* __restrict__ phi1,
                                                            const double* __restrict__ detJ, const double* __restrict__ x,
                                                            double* __restrict__ v)
{
  mass_dense_batches<true>(n, m, CB, ncells, dofmap, slot, nullptr, nullptr, nullptr, phi1, detJ, x, v);
}

// --------------------------------------------------------------------------
// dense mass, column-thread form for square tables (nq1 == P+1: the GLL-collocated
// rule of demo/gpu_operator_monolithic and the Gauss rule of degree 2P of
// demo/gpu_operator): compile-time sizes, one thread per (i, j) column, the z
// contractions in registers, x/y contractions through LDS, batch-unique
// gather/scatter.  y += Phi^T (detJ .* (Phi x)),  Phi = phi1 (x) phi1 (x) phi1.
// --------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(256) void k_mass_dense_col(int ncells, const int32_t* __restrict__ uoff,
                                                        const int32_t* __restrict__ uniq,
                                                        const uint16_t* __restrict__ loc,
                                                        const double* __restrict__ phi1,   // [n][n]: phi1[q][a]
                                                        const double* __restrict__ detJ,   // [ncells][n^3]
                                                        const double* __restrict__ x, double* __restrict__ y)
{
  constexpr int n = CellBatch<P>::n, n2 = CellBatch<P>::n2, nd = CellBatch<P>::nd;
  constexpr int CB = CellBatch<P>::CB, NT = CellBatch<P>::NT, NFLAT = CellBatch<P>::NFLAT;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* U = smem;               // [CB][nd]
  double* A = U + CB * nd;        // [CB][nd]; also the unique-dof tile before/after the contractions
  double* sP = A + CB * nd;       // [n][n]
  const int t = threadIdx.x;
  const size_t batch = blockIdx.x;
  const int cell0 = (int)batch * CB;
  const bool active = t < NT;
  const int cl = t / n2, ji = t % n2, j = ji / n, i = ji % n;
  if (t < n * n) sP[t] = phi1[t];
  const int u0 = uoff[batch], nu = uoff[batch + 1] - u0;
  for (int u = t; u < nu; u += 256) A[u] = x[uniq[u0 + u]];
  uint16_t lc[NFLAT];
  const int nvalid = min(CB, ncells - cell0) * nd;
#pragma unroll
  for (int m = 0; m < NFLAT; ++m) {
    const int pos = t + 256 * m;
    lc[m] = pos < nvalid ? loc[(size_t)cell0 * nd + pos] : (uint16_t)0xFFFF;
  }
  double dj_[n];   // detJ of this thread's column (quadrature points (i, j, *)); zero for padded cells
#pragma unroll
  for (int k = 0; k < n; ++k) dj_[k] = (active && cell0 + cl < ncells) ? detJ[(size_t)(cell0 + cl) * nd + k * n2 + ji] : 0.0;
  __syncthreads();
#pragma unroll
  for (int m = 0; m < NFLAT; ++m) {
    const int pos = t + 256 * m;
    if (pos < CB * nd) U[pos] = lc[m] != 0xFFFF ? A[lc[m]] : 0.0;
  }
  __syncthreads();
  double* Uc = U + cl * nd;
  double* Ac = A + cl * nd;
  double v[n];
  // forward x: A[k][j][qi = i] = sum_a phi[i][a] U[k][j][a]
  if (active) {
#pragma unroll
    for (int k = 0; k < n; ++k) {
      double s_ = 0.0;
#pragma unroll
      for (int a = 0; a < n; ++a) s_ += sP[i * n + a] * Uc[k * n2 + j * n + a];
      v[k] = s_;
    }
#pragma unroll
    for (int k = 0; k < n; ++k) Ac[k * n2 + ji] = v[k];
  }
  __syncthreads();
  // forward y (thread = (qi = i, qj = j)), then z, detJ, backward z in registers
  if (active) {
    double vy[n];
#pragma unroll
    for (int k = 0; k < n; ++k) {
      double s_ = 0.0;
#pragma unroll
      for (int a = 0; a < n; ++a) s_ += sP[j * n + a] * Ac[k * n2 + a * n + i];
      vy[k] = s_;
    }
    double w[n];
#pragma unroll
    for (int q = 0; q < n; ++q) {
      double s_ = 0.0;
#pragma unroll
      for (int k = 0; k < n; ++k) s_ += sP[q * n + k] * vy[k];
      w[q] = s_ * dj_[q];
    }
#pragma unroll
    for (int k = 0; k < n; ++k) {
      double s_ = 0.0;
#pragma unroll
      for (int q = 0; q < n; ++q) s_ += sP[q * n + k] * w[q];
      v[k] = s_;
    }
  }
  __syncthreads();   // all reads of A (forward y) done
  if (active) {
#pragma unroll
    for (int k = 0; k < n; ++k) Uc[k * n2 + ji] = v[k];   // B1[k][qj][qi]
  }
  __syncthreads();
  // backward y: B2[k][j][qi = i] = sum_qj phi[qj][j] B1[k][qj][i]
  if (active) {
#pragma unroll
    for (int k = 0; k < n; ++k) {
      double s_ = 0.0;
#pragma unroll
      for (int q = 0; q < n; ++q) s_ += sP[q * n + j] * Uc[k * n2 + q * n + i];
      v[k] = s_;
    }
#pragma unroll
    for (int k = 0; k < n; ++k) Ac[k * n2 + ji] = v[k];
  }
  __syncthreads();
  // backward x: out[k][j][i] = sum_qi phi[qi][i] B2[k][j][qi]
  if (active) {
#pragma unroll
    for (int k = 0; k < n; ++k) {
      double s_ = 0.0;
#pragma unroll
      for (int q = 0; q < n; ++q) s_ += sP[q * n + i] * Ac[k * n2 + j * n + q];
      v[k] = s_;
    }
  }
  __syncthreads();   // all reads of A done: A becomes the unique-dof sum tile, U the element results
  if (active) {
#pragma unroll
    for (int k = 0; k < n; ++k) Uc[k * n2 + ji] = v[k];
  }
  for (int u = t; u < nu; u += 256) A[u] = 0.0;
  __syncthreads();
#pragma unroll
  for (int m = 0; m < NFLAT; ++m) {
    const int pos = t + 256 * m;
    if (lc[m] != 0xFFFF) atomicAdd(&A[lc[m]], U[pos]);
  }
  __syncthreads();
  for (int u = t; u < nu; u += 256) unsafeAtomicAdd(&y[uniq[u0 + u]], A[u]);
}

// --------------------------------------------------------------------------
// launchers
// --------------------------------------------------------------------------
int launch_mass_lumped(int64_t nentries, const int32_t* d_dofmap, const double* d_detJ, const double* d_x,
                       double* d_y, hipStream_t s)
{
  if (nentries == 0) return WF_OK;
  hipLaunchKernelGGL(k_mass_lumped, dim3(grid_for((size_t)nentries, 256)), dim3(256), 0, s, nentries, d_dofmap,
                     d_detJ, d_x, d_y);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int launch_mass_lumped_ordered(int64_t nentries, const int32_t* d_dofmap, const int32_t* d_slot, const double* d_detJ,
                               const double* d_x, double* d_v, hipStream_t s)
{
  if (nentries == 0) return WF_OK;
  hipLaunchKernelGGL(k_mass_lumped_ordered, dim3(grid_for((size_t)nentries, 256)), dim3(256), 0, s, nentries, d_dofmap,
                     d_slot, d_detJ, d_x, d_v);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int launch_diagonal_named(int64_t n, const double* d_m, const double* d_x, double* d_y, hipStream_t s)
{
  if (n <= 0) return WF_OK;
  hipLaunchKernelGGL(k_diagonal_named, dim3(grid_for((size_t)n, 256)), dim3(256), 0, s, n, d_m, d_x, d_y);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int launch_mass_lumped_u(int ncells, int nd, int CB, const int32_t* d_uoff, const int32_t* d_uniq,
                         const uint16_t* d_loc, const double* d_detJ, const double* d_x, double* d_y, hipStream_t s)
{
  if (ncells == 0) return WF_OK;
  const int nbatch = (ncells + CB - 1) / CB;
  const size_t lds = (size_t)2 * CB * nd * sizeof(double);
  hipLaunchKernelGGL(k_mass_lumped_u, dim3((unsigned)std::min(nbatch, 256 * 8)), dim3(256), lds, s, ncells, nd, CB,
                     d_uoff, d_uniq, d_loc, d_detJ, d_x, d_y);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

template <int P>
static int launch_mass_dense_col_t(int ncells, const int32_t* d_uoff, const int32_t* d_uniq, const uint16_t* d_loc,
                                   const double* d_phi1, const double* d_detJ, const double* d_x, double* d_y,
                                   hipStream_t s)
{
  constexpr int n = CellBatch<P>::n, nd = CellBatch<P>::nd, CB = CellBatch<P>::CB;
  const unsigned nb = CellBatch<P>::batches(ncells);
  const size_t lds = (size_t)(2 * CB * nd + n * n) * sizeof(double);
  hipLaunchKernelGGL(k_mass_dense_col<P>, dim3(nb), dim3(256), lds, s, ncells, d_uoff, d_uniq, d_loc, d_phi1, d_detJ,
                     d_x, d_y);
  return launch_status("mass_dense_col");
}

int launch_mass_dense_col(int P, int ncells, const int32_t* d_uoff, const int32_t* d_uniq, const uint16_t* d_loc,
                          const double* d_phi1, const double* d_detJ, const double* d_x, double* d_y, hipStream_t s)
{
  if (ncells == 0) return WF_OK;
  return dispatch_degree(P, "mass_dense_col: degree must be 1..7", [&](auto p) {
    return launch_mass_dense_col_t<decltype(p)::value>(ncells, d_uoff, d_uniq, d_loc, d_phi1, d_detJ, d_x, d_y, s);
  });
}

// cells per workgroup of k_mass_dense: enough that every contraction pass fills 256
// lanes (measured: P2 >= 8, P4 2..8, P6 4)
int mass_dense_cells_per_batch(int mx)
{
  return std::max(1, std::min(1400 / (mx * mx * mx), 32));
}

// What the two launchers of mass_dense_batches share: the dynamic LDS of a workgroup of CB cells (ping, pong, the table,
// the unique-dof tile where there is one), the refusal above 160 KB ("<who>: tables do not fit LDS"), the attribute a
// kernel needs above 64 KB, and the grid of the persistent loop.
struct MassDenseShape {
  size_t lds = 0;    // dynamic LDS bytes
  unsigned nb = 0;   // workgroups
};
template <class Kernel>
static int mass_dense_launch_shape(Kernel kernel, const char* who, int n, int nq1, int CB, bool unique_tile, int ncells,
                                   MassDenseShape* shape)
{
  const int mx = n > nq1 ? n : nq1, mx3 = mx * mx * mx;
  shape->lds = (size_t)(2 * CB * mx3 + nq1 * n + (unique_tile ? CB * n * n * n : 0)) * sizeof(double);
  if (shape->lds > 160 * 1024) {
    set_error(std::string(who) + ": tables do not fit LDS");
    return WF_ERR_UNSUPPORTED;
  }
  shape->nb = (unsigned)std::min<int64_t>((ncells + CB - 1) / CB, 256 * 8);
  if (shape->lds > 64 * 1024)
    WF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)shape->lds));
  return WF_OK;
}

int launch_mass_dense(int P, int nq1, int ncells, const int32_t* d_dofmap, const int32_t* d_uoff,
                      const int32_t* d_uniq, const uint16_t* d_loc, int CBu, const double* d_phi1,
                      const double* d_detJ, const double* d_x, double* d_y, hipStream_t s)
{
  if (ncells == 0) return WF_OK;
  const int n = P + 1;
  // cells per workgroup: enough that every contraction pass fills 256 lanes, within ~32 KB of LDS
  const int CB = d_uoff ? CBu : mass_dense_cells_per_batch(std::max(n, nq1));   // the unique lists fix the batch size
  MassDenseShape sh;
  if (int rc = mass_dense_launch_shape(k_mass_dense, "mass_dense", n, nq1, CB, d_uoff != nullptr, ncells, &sh)) return rc;
  hipLaunchKernelGGL(k_mass_dense, dim3(sh.nb), dim3(256), sh.lds, s, n, nq1, CB, ncells, d_dofmap, d_uoff, d_uniq, d_loc,
                     d_phi1, d_detJ, d_x, d_y);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int launch_mass_dense_ordered(int P, int nq1, int ncells, const int32_t* d_dofmap, const int32_t* d_slot, const double* d_phi1,
                              const double* d_detJ, const double* d_x, double* d_v, hipStream_t s)
{
  if (ncells == 0) return WF_OK;
  const int n = P + 1, CB = mass_dense_cells_per_batch(std::max(n, nq1));
  MassDenseShape sh;
  if (int rc = mass_dense_launch_shape(k_mass_dense_ordered, "ordered mass_dense", n, nq1, CB, false, ncells, &sh)) return rc;
  hipLaunchKernelGGL(k_mass_dense_ordered, dim3(sh.nb), dim3(256), sh.lds, s, n, nq1, CB, ncells, d_dofmap, d_slot, d_phi1, d_detJ,
                     d_x, d_v);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

}  // namespace wf
