// Order-fixed accumulation (WF_FLAG_ORDERED): y as a pure function of the inputs on any mesh.
//
// Two passes, no atomics in LDS or in global memory:
//   pass 1  every cell's element-local result, written with plain stores to v[slot[c][l]];
//   pass 2  one thread per y entry d sums v[row_off[d] .. row_off[d+1]) front to back and reads and writes y[d] once.
// slot is the stable counting sort of the caller's flattened dofmap (wf_ordered_slots): the contributions of dof d lie
// in the order in which the caller's h_dofmap lists d, whatever the internal cell order or the batch a cell sits in.
//
// Layout: pass 1 stores slot-ordered, so that pass 2 streams contiguous runs and needs no source index (20 B per
// element-local entry: 4 slot + 8 store + 8 load).  The other layout -- v[cell][local] with plain coalesced stores and a
// source index per entry in pass 2 (4 + 8 + 8 B as well, but one gathered 8-byte load per entry) -- is not measured.
//
// The pass-1 kernels are the cell-batch kernels of kernels.hip with the output stage replaced; every thread of a batch
// runs the same instruction sequence on its cell, so a cell's arithmetic does not depend on where the cell sits.
#include "stiffness_core.h"

namespace wf {

// --------------------------------------------------------------------------
// pass 1, stiffness: k_stiffness_generic (kernels.hip) with v[slot] = value in place of the atomic add
// --------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(256) void k_stiffness_ordered(int ncells, const int32_t* __restrict__ dofmap,
                                                           const int32_t* __restrict__ slot,
                                                           const double2* __restrict__ G6blk, const double* __restrict__ dD,
                                                           DMat dm, double coeff, const double* __restrict__ x,
                                                           double* __restrict__ v)
{
  constexpr int n = P + 1, n2 = n * n, nd = n * n2;
  constexpr int CB = 256 / n2, NT = CB * n2;
  constexpr int NFLAT = (CB * nd + 255) / 256;
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

  // 1. the whole geometry stream of this batch first (16 B per lane, contiguous across the wave); padded cells read zeros
  double2 g[n][3];
  if (active) {
    const double2* gp = G6blk + (batch * n * 3) * (size_t)NT + t;
#pragma unroll
    for (int k = 0; k < n; ++k)
#pragma unroll
      for (int p = 0; p < 3; ++p) g[k][p] = load_stream(gp + (size_t)(k * 3 + p) * NT);
  }
  if (t < n * n) sD[t] = dD[t];

  // 2. gather: flat, coalesced dofmap and slot reads; the slots stay in registers for the store
  int32_t sl[NFLAT];
  const int nvalid = min(CB, ncells - cell0) * nd;
#pragma unroll
  for (int m = 0; m < NFLAT; ++m) {
    const int pos = t + 256 * m;
    sl[m] = -1;
    if (pos < nvalid) {
      sl[m] = slot[(size_t)cell0 * nd + pos];
      U[pos] = x[dofmap[(size_t)cell0 * nd + pos]];
    } else if (pos < CB * nd) {
      U[pos] = 0.0;
    }
  }
  __syncthreads();

  double out[n];
  stiffness_column<P>(U + cl * nd, n2, n, Fr + cl * nd, Fs + cl * nd, sD, dm, g, coeff, i, j, active, out);

  // 3. element results back through LDS (U: all its reads precede the barrier inside stiffness_column), then one plain
  //    store per element-local entry
  if (active) {
#pragma unroll
    for (int k = 0; k < n; ++k) U[cl * nd + k * n2 + ji] = out[k];
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < NFLAT; ++m)
    if (sl[m] >= 0) v[sl[m]] = U[t + 256 * m];
}

// --------------------------------------------------------------------------
// pass 1, dense mass: the sum-factorised passes of k_mass_dense (kernels.hip) without the unique-dof tile; the last loop
// stores.  phi1: [m][n] row-major.
// --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mass_dense_ordered(int n, int m, int CB, int ncells, const int32_t* __restrict__ dofmap,
                                                            const int32_t* __restrict__ slot, const double* __restrict__ phi1,
                                                            const double* __restrict__ detJ, const double* __restrict__ x,
                                                            double* __restrict__ v)
{
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int mx = max(n, m), mx3 = mx * mx * mx;
  double* A = smem;                  // ping  [CB][mx^3]
  double* B = A + CB * mx3;          // pong  [CB][mx^3]
  double* sphi = B + CB * mx3;       // [m][n]
  const int t = threadIdx.x;
  const int nd = n * n * n, nq = m * m * m;
  for (int p = t; p < m * n; p += 256) sphi[p] = phi1[p];
  const int nbatch = (ncells + CB - 1) / CB;
  for (int batch = blockIdx.x; batch < nbatch; batch += gridDim.x) {
    const int c0 = batch * CB;
    const int nc = min(CB, ncells - c0);
    __syncthreads();
    for (int p = t; p < nc * nd; p += 256) {
      const int c = p / nd, l = p - c * nd;
      A[c * mx3 + l] = x[dofmap[(size_t)c0 * nd + p]];
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
    // backward x and store: v[slot] = sum_qi phi[qi][i] B[c][k][j][qi]
    for (int p = t; p < nc * nd; p += 256) {
      const int c = p / nd, l = p - c * nd;
      const int i = l % n, kj = l / n;
      double s = 0.0;
      for (int a = 0; a < m; ++a) s += sphi[a * n + i] * B[c * mx3 + kj * m + a];
      v[slot[(size_t)c0 * nd + p]] = s;
    }
  }
}

// --------------------------------------------------------------------------
// pass 1, element-wise lumped mass (spectral_mass.hpp:84-89 without the scatter): v[slot] = x[dof] * detJ
// --------------------------------------------------------------------------
__global__ void k_mass_lumped_ordered(int64_t nentries, const int32_t* __restrict__ dofmap, const int32_t* __restrict__ slot,
                                      const double* __restrict__ detJ, const double* __restrict__ x, double* __restrict__ v)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nentries) v[slot[e]] = x[dofmap[e]] * detJ[e];
}

// --------------------------------------------------------------------------
// pass 2: y[d] += v[row_off[d]] + v[row_off[d] + 1] + ... in that order; an empty row leaves y[d] untouched.
// One thread per row; neighbouring threads read neighbouring runs of v, so every cache line fetched is used in full.  v is
// read exactly once: non-temporal loads, 16 bytes wide from the first even entry of the run on (hipMalloc'd arrays are
// 16-byte aligned; v_aligned = 0 takes 8-byte loads throughout), a scalar entry before and after.
// --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_segment_sum_add(int32_t n, int v_aligned, const int32_t* __restrict__ row_off,
                                                         const double* __restrict__ v, double* __restrict__ y)
{
  typedef double d2v __attribute__((ext_vector_type(2)));
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= n) return;
  int32_t b = row_off[d];
  const int32_t e = row_off[d + 1];   // the pair row_off[d], row_off[d + 1]: adjacent loads, merged where aligned
  if (b >= e) return;
  double s = __builtin_nontemporal_load(v + b);
  ++b;
  if (v_aligned) {
    if ((b & 1) && b < e) {
      s = s + __builtin_nontemporal_load(v + b);
      ++b;
    }
    for (; b + 1 < e; b += 2) {
      const d2v w = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(v + b));
      s = s + w.x;
      s = s + w.y;
    }
  }
  for (; b < e; ++b) s = s + __builtin_nontemporal_load(v + b);
  y[d] = y[d] + s;
}

// --------------------------------------------------------------------------
// launchers
// --------------------------------------------------------------------------
template <int P>
static int launch_stiffness_ordered_t(int ncells, const int32_t* d_dofmap, const int32_t* d_slot, const double* d_G6blk,
                                      const double* d_D, const DMat& dm, double coeff, const double* d_x, double* d_v,
                                      hipStream_t s)
{
  constexpr int n = P + 1, nd = n * n * n, CB = 256 / (n * n);
  const unsigned nb = (unsigned)((ncells + CB - 1) / CB);
  const size_t lds = (size_t)(3 * CB * nd + n * n) * sizeof(double);
  hipLaunchKernelGGL(k_stiffness_ordered<P>, dim3(nb), dim3(256), lds, s, ncells, d_dofmap, d_slot,
                     reinterpret_cast<const double2*>(d_G6blk), d_D, dm, coeff, d_x, d_v);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int launch_stiffness_ordered(int P, int ncells, const int32_t* d_dofmap, const int32_t* d_slot, const double* d_G6blk,
                             const double* d_D, const DMat& dm, double coeff, const double* d_x, double* d_v, hipStream_t s)
{
  if (ncells == 0) return WF_OK;
#define WF_ORDERED_CASE(PP) \
  case PP: return launch_stiffness_ordered_t<PP>(ncells, d_dofmap, d_slot, d_G6blk, d_D, dm, coeff, d_x, d_v, s)
  switch (P) {
    WF_ORDERED_CASE(1);
    WF_ORDERED_CASE(2);
    WF_ORDERED_CASE(3);
    WF_ORDERED_CASE(4);
    WF_ORDERED_CASE(5);
    WF_ORDERED_CASE(6);
    WF_ORDERED_CASE(7);
  }
#undef WF_ORDERED_CASE
  set_error("ordered stiffness: degree must be 1..7");
  return WF_ERR_UNSUPPORTED;
}

int launch_mass_dense_ordered(int P, int nq1, int ncells, const int32_t* d_dofmap, const int32_t* d_slot, const double* d_phi1,
                              const double* d_detJ, const double* d_x, double* d_v, hipStream_t s)
{
  if (ncells == 0) return WF_OK;
  const int n = P + 1, mx = n > nq1 ? n : nq1, mx3 = mx * mx * mx;
  const int CB = mass_dense_cells_per_batch(mx);
  const size_t lds = (size_t)(2 * CB * mx3 + nq1 * n) * sizeof(double);
  if (lds > 160 * 1024) {
    set_error("ordered mass_dense: tables do not fit LDS");
    return WF_ERR_UNSUPPORTED;
  }
  const unsigned nb = (unsigned)std::min<int64_t>((ncells + CB - 1) / CB, 256 * 8);
  if (lds > 64 * 1024)
    WF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_mass_dense_ordered),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_mass_dense_ordered, dim3(nb), dim3(256), lds, s, n, nq1, CB, ncells, d_dofmap, d_slot, d_phi1, d_detJ,
                     d_x, d_v);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int launch_mass_lumped_ordered(int64_t nentries, const int32_t* d_dofmap, const int32_t* d_slot, const double* d_detJ,
                               const double* d_x, double* d_v, hipStream_t s)
{
  if (nentries == 0) return WF_OK;
  hipLaunchKernelGGL(k_mass_lumped_ordered, dim3((unsigned)((nentries + 255) / 256)), dim3(256), 0, s, nentries, d_dofmap,
                     d_slot, d_detJ, d_x, d_v);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

// The plan of the order contract: a stable counting sort of the flattened dofmap.  row_off[ndofs + 1], slot[nentries].
int ordered_slots(int64_t nentries, int32_t ndofs, const int32_t* dofmap, int32_t* row_off, int32_t* slot)
{
  std::fill(row_off, row_off + (size_t)ndofs + 1, 0);
  for (int64_t e = 0; e < nentries; ++e) {
    if (dofmap[e] < 0 || dofmap[e] >= ndofs) {
      set_error("wf_ordered_slots: dofmap entry out of range");
      return WF_ERR_INVALID;
    }
    ++row_off[dofmap[e] + 1];
  }
  for (int32_t d = 0; d < ndofs; ++d) row_off[d + 1] += row_off[d];
  std::vector<int32_t> next(row_off, row_off + ndofs);
  for (int64_t e = 0; e < nentries; ++e) slot[e] = next[dofmap[e]]++;
  return WF_OK;
}

}  // namespace wf

using namespace wf;

extern "C" {

int wf_ordered_slots(int64_t ncells, int nd, int32_t ndofs, const int32_t* h_dofmap, int32_t* h_row_off, int32_t* h_slot)
{
  WF_REQUIRE(ncells >= 0 && nd > 0 && ndofs >= 0 && h_row_off, "wf_ordered_slots: bad argument");
  if (ncells > (int64_t)INT32_MAX / nd) {
    set_error("wf_ordered_slots: ncells * nd exceeds int32");
    return WF_ERR_UNSUPPORTED;
  }
  WF_REQUIRE(ncells == 0 || (h_dofmap && h_slot), "wf_ordered_slots: null array");
  return ordered_slots(ncells * nd, ndofs, h_dofmap, h_row_off, h_slot);
}

int wf_segment_sum_add(int32_t n, const int32_t* d_row_off, const double* d_vals, double* d_y, void* stream)
{
  WF_REQUIRE(n >= 0, "wf_segment_sum_add: negative size");
  if (n == 0) return WF_OK;
  WF_REQUIRE(d_row_off && d_y, "wf_segment_sum_add: null argument");   // d_vals may be null when every row is empty
  const int aligned = (reinterpret_cast<uintptr_t>(d_vals) & 15) == 0;
  hipLaunchKernelGGL(k_segment_sum_add, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                     aligned, d_row_off, d_vals, d_y);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

}  // extern "C"
