// Cell-batch stiffness kernels for hexahedra: the sum-factorised operator
//     y += -c0^2 * sum_cells  P_c^T  D^T (G .* (D P_c x))
// on batches of CB cells per 256-thread workgroup (cell_batch.h), in place of the dense per-cell loop of
// common/operators.hpp:113-133 (skernel) and the gather/kernel/scatter launch triple of common/cuda/mass.hpp:76-95.
//
// What runs them today: the batch-unique kernels (k_stiffness_generic_up2 / _up) are the fall-back for dofmap meshes
// that do not tile into lattice columns (the marching kernels take the ones that do); the element-wise kernel
// (k_stiffness_generic, stiffness_elementwise.h) and the box block kernel (k_stiffness_box) are reachable by a tuning
// hint only.  None of this is the hot path of the benchmark.
//
// Thread mapping ("column threads", 64-wide waves): one thread owns the column (i, j, *) of one cell and keeps its
// n = P+1 values along z in registers.  x- and y-direction contractions go through an LDS tile of the cell's dofs, the
// z-direction contraction stays in registers (stiffness_core.h).  The per-point symmetric geometry tensor (6 doubles)
// is the dominant HBM stream; it is stored pre-blocked per workgroup (hex_geometry.hip) so that every lane issues
// 16-byte loads that are contiguous across the wave, and all loads of a batch are issued before any arithmetic.
#include "cell_batch.h"
#include "stiffness_core.h"  // stiffness_column<P>, load_stream
#include "stiffness_elementwise.h"  // k_stiffness_generic<P>

namespace wf {

// the whole geometry of one thread's column (i, j, *) of a batch, from its first entry gp = G6blk[batch][0][0][t]:
// 3 n non-temporal 16-byte loads, contiguous across the wave, issued together (NT: threads of the batch)
template <int P>
__device__ __forceinline__ void batch_load_geometry(double2 (&g)[P + 1][3], const double2* gp, int NT)
{
#pragma unroll
  for (int k = 0; k < P + 1; ++k)
#pragma unroll
    for (int p = 0; p < 3; ++p) g[k][p] = load_stream(gp + (size_t)(k * 3 + p) * NT);
}

// --------------------------------------------------------------------------
// generic stiffness, batch-unique form (default for arbitrary dofmaps): the host
// lists the unique dofs of every batch of CB cells once (uniq, sorted) and the
// position of every element-local dof in that list (loc, uint16).  x is read once
// per unique dof, the cells of the batch are summed per unique dof in LDS
// (ds_add_f64) and y receives ONE atomic per unique dof, in ascending address
// order -- fewer and better-shaped atomic requests than the element-wise scatter
// (P4, lexicographic numbering: 1025 instead of 1250 per batch, runs of 41
// contiguous doubles instead of 5).
// The product library launches the pipelined forms below (k_stiffness_generic_up2 / _up).  This plain one-batch-per-
// workgroup form carries the ablation masks, so it is compiled for the diagnostic build only (-DWF_DIAG, where a
// non-zero WF_ABLATE selects it) or as the only form with -DWF_GENERIC_PIPELINED=0.
// --------------------------------------------------------------------------
#ifndef WF_GENERIC_PIPELINED
#define WF_GENERIC_PIPELINED 1
#endif
#if defined(WF_DIAG) || !WF_GENERIC_PIPELINED
#define WF_GENERIC_U_PLAIN 1
template <int P>
__global__ __launch_bounds__(256) void k_stiffness_generic_u(int ncells, const int32_t* __restrict__ uoff,
                                                             const int32_t* __restrict__ uniq,
                                                             const uint16_t* __restrict__ loc,
                                                             const double2* __restrict__ G6blk,
                                                             const double* __restrict__ dD, DMat dm,
                                                             double coeff, const double* __restrict__ x,
                                                             double* __restrict__ y, int ablate_arg)
{
  [[maybe_unused]] const int ablate = WF_ABLATE_FLAGS(ablate_arg);
  constexpr int n = CellBatch<P>::n, n2 = CellBatch<P>::n2, nd = CellBatch<P>::nd;
  constexpr int CB = CellBatch<P>::CB, NT = CellBatch<P>::NT, NFLAT = CellBatch<P>::NFLAT;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* U = smem;                 // [CB][nd]
  double* Fr = U + CB * nd;         // [CB][nd]; also the unique-dof tile before phase 1 and after phase 2
  double* Fs = Fr + CB * nd;        // [CB][nd]
  double* sD = Fs + CB * nd;        // [n][n]

  const int t = threadIdx.x;
  const size_t batch = blockIdx.x;
  const int cell0 = (int)batch * CB;
  const bool active = t < NT;
  const int cl = t / n2, ji = t % n2, j = ji / n, i = ji % n;

  double2 g[n][3];
  if (active) {
    const double2* gp = G6blk + (batch * n * 3) * (size_t)NT + t;
    if (ablate & 2) gp = G6blk + t;
    batch_load_geometry<P>(g, gp, NT);
  }
  if (t < n * n) sD[t] = dD[t];

  const int u0 = uoff[batch], nu = uoff[batch + 1] - u0;
  for (int u = t; u < nu; u += 256) Fr[u] = (ablate & 4) ? 1.0 + u : x[uniq[u0 + u]];
  uint16_t lc[NFLAT];
  const int nvalid = min(CB, ncells - cell0) * nd;
#pragma unroll
  for (int m = 0; m < NFLAT; ++m) {
    const int pos = t + 256 * m;
    lc[m] = pos < nvalid ? loc[(size_t)cell0 * nd + pos] : (uint16_t)0xFFFF;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < NFLAT; ++m) {
    const int pos = t + 256 * m;
    if (pos < CB * nd) U[pos] = lc[m] != 0xFFFF ? Fr[lc[m]] : 0.0;
  }
  __syncthreads();

  double out[n];
  stiffness_column<P>(U + cl * nd, n2, n, Fr + cl * nd, Fs + cl * nd, sD, dm, g, coeff, i, j, active, out, ablate);

  if (active) {
#pragma unroll
    for (int k = 0; k < n; ++k) U[cl * nd + k * n2 + ji] = out[k];
  }
  __syncthreads();   // phase 2 has read Fr/Fs, U holds the element results
  for (int u = t; u < nu; u += 256) Fr[u] = 0.0;
  __syncthreads();
#pragma unroll
  for (int m = 0; m < NFLAT; ++m) {
    const int pos = t + 256 * m;
    if (lc[m] != 0xFFFF) atomicAdd(&Fr[lc[m]], U[pos]);
  }
  __syncthreads();
  for (int u = t; u < nu; u += 256) {
    if (ablate & 1) {
      if (Fr[u] == 1.2345e300) y[uniq[u0 + u]] = Fr[u];
    } else {
      unsafeAtomicAdd(&y[uniq[u0 + u]], Fr[u]);
    }
  }
}
#endif

// The same kernel as a persistent workgroup that walks batches and carries the NEXT batch's unique-dof indices in
// registers: the x gather of a batch is a chain of three dependent loads (uoff -> uniq -> x), and the ablation masks
// showed it costs as much as the whole geometry stream (P4, 10 M dofs: 0.261 ms; without the x loads 0.202, with the
// geometry served from L2 0.204).  With the indices fetched one batch ahead the x loads are issued at the top of a
// batch together with its geometry: one memory latency per batch instead of two and a half.  All loads of the loop
// are unconditional on clamped addresses (a guard is a branch; at its join the compiler waits for every pending
// load), the indices double as the scatter addresses of the batch.
// The phase loops of this kernel and the next stay written out: as helper functions they compile to other code.
template <int P>
__global__ __launch_bounds__(256) void k_stiffness_generic_up(int ncells, int nbatch, const int32_t* __restrict__ uoff,
                                                              const int32_t* __restrict__ uniq, const uint16_t* __restrict__ loc,
                                                              const double2* __restrict__ G6blk, const double* __restrict__ dD,
                                                              DMat dm, double coeff, const double* __restrict__ x,
                                                              double* __restrict__ y)
{
  constexpr int n = CellBatch<P>::n, n2 = CellBatch<P>::n2, nd = CellBatch<P>::nd;
  constexpr int CB = CellBatch<P>::CB, NT = CellBatch<P>::NT;
  constexpr int NFLAT = CellBatch<P>::NFLAT;   // element-local dofs per thread; also bounds the unique dofs per thread
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* U = smem;                 // [CB][nd]
  double* Fr = U + CB * nd;         // [CB][nd]; also the unique-dof tile before phase 1 and after phase 2
  double* Fs = Fr + CB * nd;        // [CB][nd]
  double* sD = Fs + CB * nd;        // [n][n]

  const int t = threadIdx.x;
  const bool active = t < NT;
  const int cl = t / n2, ji = t % n2, j = ji / n, i = ji % n;
  if (t < n * n) sD[t] = dD[t];

  // unique-dof indices of a batch -> registers (entry u = t + 256 m; past the list: its last entry)
  auto load_uniq = [&](int32_t (&uq)[NFLAT], int& nu, int b) {
    const int u0 = uoff[b];
    nu = uoff[b + 1] - u0;
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int u = t + 256 * m;
      uq[m] = uniq[u0 + (u < nu ? u : nu - 1)];
    }
  };
  int32_t uqa[NFLAT], uqb[NFLAT];
  int nua = 0, nub = 0;
  int batch = blockIdx.x;
  if (batch < nbatch) load_uniq(uqa, nua, batch);

  auto one = [&](int32_t (&uq)[NFLAT], int nu, int32_t (&uqn)[NFLAT], int& nun, int b) {
    const int cell0 = b * CB;
    // (a) this batch's x values, geometry and local positions; the next batch's indices
    double xr[NFLAT];
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) xr[m] = x[uq[m]];
    double2 g[n][3];
    batch_load_geometry<P>(g, G6blk + ((size_t)b * n * 3) * (size_t)NT + (active ? t : NT - 1), NT);
    uint16_t lc[NFLAT];
    const int nvalid = min(CB, ncells - cell0) * nd;
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int pos = t + 256 * m;
      const uint16_t v = loc[(size_t)cell0 * nd + (pos < nvalid ? pos : 0)];
      lc[m] = pos < nvalid ? v : (uint16_t)0xFFFF;
    }
    const int bn = b + (int)gridDim.x;
    load_uniq(uqn, nun, bn < nbatch ? bn : b);
    // (b) unique tile -> LDS -> element-local layout
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int u = t + 256 * m;
      if (u < nu) Fr[u] = xr[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int pos = t + 256 * m;
      if (pos < CB * nd) U[pos] = lc[m] != 0xFFFF ? Fr[lc[m]] : 0.0;
    }
    __syncthreads();
    double out[n];
    stiffness_column<P>(U + cl * nd, n2, n, Fr + cl * nd, Fs + cl * nd, sD, dm, g, coeff, i, j, active, out, 0);
    if (active) {
#pragma unroll
      for (int k = 0; k < n; ++k) U[cl * nd + k * n2 + ji] = out[k];
    }
    __syncthreads();   // phase 2 has read Fr/Fs, U holds the element results
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int u = t + 256 * m;
      if (u < nu) Fr[u] = 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int pos = t + 256 * m;
      if (lc[m] != 0xFFFF) atomicAdd(&Fr[lc[m]], U[pos]);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int u = t + 256 * m;
      if (u < nu) unsafeAtomicAdd(&y[uq[m]], Fr[u]);
    }
    __syncthreads();   // Fr is the next batch's unique tile
  };
  while (batch < nbatch) {
    one(uqa, nua, uqb, nub, batch);
    batch += gridDim.x;
    if (batch >= nbatch) break;
    one(uqb, nub, uqa, nua, batch);
    batch += gridDim.x;
  }
}

// Fully pipelined form (P <= 4: two geometry register sets fit at two workgroups per CU): everything batch b + s needs (s = the grid size) --
// geometry, x values, local positions -- is requested while batch b computes, its unique-dof indices one batch
// earlier, the two scalars that locate them one batch earlier still.  There is no `has_next` anywhere: a batch past
// the end is the last batch again (redundant reads, never stored), so the wait counts the compiler derives stay
// exact (stiffness_march.hip on what a uniform branch around a prefetch costs).
template <int P>
__global__ __launch_bounds__(256) void k_stiffness_generic_up2(int ncells, int nbatch, const int32_t* __restrict__ uoff,
                                                               const int32_t* __restrict__ uniq, const uint16_t* __restrict__ loc,
                                                               const double2* __restrict__ G6blk, const double* __restrict__ dD,
                                                               DMat dm, double coeff, const double* __restrict__ x,
                                                               double* __restrict__ y)
{
  constexpr int n = CellBatch<P>::n, n2 = CellBatch<P>::n2, nd = CellBatch<P>::nd;
  constexpr int CB = CellBatch<P>::CB, NT = CellBatch<P>::NT, NFLAT = CellBatch<P>::NFLAT;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* U = smem;
  double* Fr = U + CB * nd;
  double* Fs = Fr + CB * nd;
  double* sD = Fs + CB * nd;

  const int t = threadIdx.x;
  const bool active = t < NT;
  const int cl = t / n2, ji = t % n2, j = ji / n, i = ji % n;
  if (t < n * n) sD[t] = dD[t];
  const int stride = (int)gridDim.x;
  auto clampb = [&](int b) { return b < nbatch ? b : nbatch - 1; };

  // unique-dof indices of the batch whose list is uniq[u0 .. u0 + nu) -> registers (past the list: its last entry)
  auto load_uniq = [&](int32_t (&uq)[NFLAT], int u0, int nu) {
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int u = t + 256 * m;
      uq[m] = uniq[u0 + (u < nu ? u : nu - 1)];
    }
  };
  auto load_batch = [&](double (&xr)[NFLAT], double2 (&g)[n][3], uint16_t (&lc)[NFLAT], const int32_t (&uq)[NFLAT], int b) {
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) xr[m] = x[uq[m]];
    batch_load_geometry<P>(g, G6blk + ((size_t)b * n * 3) * (size_t)NT + (active ? t : NT - 1), NT);
    const int cell0 = b * CB, nvalid = min(CB, ncells - cell0) * nd;
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int pos = t + 256 * m;
      const uint16_t v = loc[(size_t)cell0 * nd + (pos < nvalid ? pos : 0)];
      lc[m] = pos < nvalid ? v : (uint16_t)0xFFFF;
    }
  };

  int batch = blockIdx.x;
  if (batch >= nbatch) return;
  // list locations (scalars) of batches b, b + s, b + 2 s; vectors in two sets that swap roles (loop unrolled by two)
  int b1 = clampb(batch + stride), b2 = clampb(batch + 2 * stride);
  int u0c = uoff[batch], nuc = uoff[batch + 1] - u0c;
  int u0n = uoff[b1], nun = uoff[b1 + 1] - u0n;
  int u0nn = uoff[b2], nunn = uoff[b2 + 1] - u0nn;
  int32_t uqA[NFLAT], uqB[NFLAT];
  double xA[NFLAT], xB[NFLAT];
  double2 gA[n][3], gB[n][3];
  uint16_t lcA[NFLAT], lcB[NFLAT];
  load_uniq(uqA, u0c, nuc);
  load_uniq(uqB, u0n, nun);
  load_batch(xA, gA, lcA, uqA, batch);

  // batch b sits in (xr, g, lc); uqn holds the indices of batch b + s, into which (xn, gn, lcn) are loaded; uq (the
  // indices of batch b, no longer needed: its scatter re-reads them from L2) is refilled with those of batch b + 2 s
  auto one = [&](int32_t (&uq)[NFLAT], double (&xr)[NFLAT], double2 (&g)[n][3], uint16_t (&lc)[NFLAT], int32_t (&uqn)[NFLAT],
                 double (&xn)[NFLAT], double2 (&gn)[n][3], uint16_t (&lcn)[NFLAT], int b) {
    const int nu = nuc, u0 = u0c;
    // (a) unique tile -> LDS (consumes xr) -> element-local layout
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int u = t + 256 * m;
      if (u < nu) Fr[u] = xr[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int pos = t + 256 * m;
      if (pos < CB * nd) U[pos] = lc[m] != 0xFFFF ? Fr[lc[m]] : 0.0;
    }
    __syncthreads();
    // (b) this batch's scatter addresses again (L2), then the requests for batch b + s and the indices of b + 2 s,
    //     then the list location of b + 3 s: all in flight during the phases
    int32_t us[NFLAT];
    load_uniq(us, u0, nu);
    load_batch(xn, gn, lcn, uqn, clampb(b + stride));
    load_uniq(uq, u0nn, nunn);
    const int b3 = clampb(b + 3 * stride);
    const int u0n3 = uoff[b3], nun3 = uoff[b3 + 1] - u0n3;
    // (c) element kernel
    double out[n];
    stiffness_column<P>(U + cl * nd, n2, n, Fr + cl * nd, Fs + cl * nd, sD, dm, g, coeff, i, j, active, out, 0);
    if (active) {
#pragma unroll
      for (int k = 0; k < n; ++k) U[cl * nd + k * n2 + ji] = out[k];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int u = t + 256 * m;
      if (u < nu) Fr[u] = 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int pos = t + 256 * m;
      if (lc[m] != 0xFFFF) atomicAdd(&Fr[lc[m]], U[pos]);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NFLAT; ++m) {
      const int u = t + 256 * m;
      if (u < nu) unsafeAtomicAdd(&y[us[m]], Fr[u]);
    }
    __syncthreads();
    u0c = u0n;
    nuc = nun;
    u0n = u0nn;
    nun = nunn;
    u0nn = u0n3;
    nunn = nun3;
  };
  while (true) {
    one(uqA, xA, gA, lcA, uqB, xB, gB, lcB, batch);
    batch += stride;
    if (batch >= nbatch) break;
    one(uqB, xB, gB, lcB, uqA, xA, gA, lcA, batch);
    batch += stride;
    if (batch >= nbatch) break;
  }
}

// --------------------------------------------------------------------------
// structured box stiffness: implicit dofmap, block dof tile in LDS, atomics only
// on dofs shared with a neighbouring block
// --------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(256) void k_stiffness_box(int nx, int ny, int nz, int bx, int by, int bz,
                                                       const double2* __restrict__ G6blk,
                                                       const double* __restrict__ dD, DMat dm,
                                                       double coeff, const double* __restrict__ x,
                                                       double* __restrict__ y, int ablate_arg)
{
  [[maybe_unused]] const int ablate = WF_ABLATE_FLAGS(ablate_arg);
  constexpr int n = CellBatch<P>::n, n2 = CellBatch<P>::n2, nd = CellBatch<P>::nd;
  const int CB = bx * by * bz, NT = CB * n2;   // the block of the caller, not CellBatch<P>::CB
  const int TX = P * bx + 1, TY = P * by + 1, TZ = P * bz + 1;
  const int tile = TX * TY * TZ;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* Ut = smem;                         // [TZ][TY][TX] x tile, later the y tile
  double* Fr = Ut + ((tile + 1) & ~1);       // [CB][nd]
  double* Fs = Fr + CB * nd;                 // [CB][nd]
  double* sD = Fs + CB * nd;                 // [n][n]

  const int t = threadIdx.x;
  const int nbx = (nx + bx - 1) / bx, nby = (ny + by - 1) / by;
  const int Bx = blockIdx.x % nbx, By = (blockIdx.x / nbx) % nby, Bz = blockIdx.x / (nbx * nby);
  const bool inrange = t < NT;
  const int cl = t / n2, ji = t % n2, j = ji / n, i = ji % n;
  const int lx = cl % bx, ly = (cl / bx) % by, lz = cl / (bx * by);
  const int cx = Bx * bx + lx, cy = By * by + ly, cz = Bz * bz + lz;
  const bool active = inrange && cx < nx && cy < ny && cz < nz;

  double2 g[n][3];
  if (inrange) {
    const double2* gp = G6blk + ((size_t)blockIdx.x * n * 3) * (size_t)NT + t;
    if (ablate & 2) gp = G6blk + t;
    // batch_load_geometry, written out: the call compiles to other code in this kernel
#pragma unroll
    for (int k = 0; k < n; ++k)
#pragma unroll
      for (int p = 0; p < 3; ++p) g[k][p] = load_stream(gp + (size_t)(k * 3 + p) * NT);
  }
  if (t < n * n) sD[t] = dD[t];

  // dof tile of this block inside the global lattice (clipped at the mesh end)
  const int NX = P * nx + 1, NY = P * ny + 1, NZ = P * nz + 1;
  const int I0 = P * Bx * bx, J0 = P * By * by, K0 = P * Bz * bz;
  const int EX = min(TX, NX - I0), EY = min(TY, NY - J0), EZ = min(TZ, NZ - K0);
  for (int pos = t; pos < tile; pos += 256) {
    const int I = pos % TX, J = (pos / TX) % TY, K = pos / (TX * TY);
    double v = 0.0;
    if (I < EX && J < EY && K < EZ)
      v = (ablate & 4) ? 1.0 + pos : x[(size_t)(I0 + I) + (size_t)NX * ((size_t)(J0 + J) + (size_t)NY * (K0 + K))];
    Ut[pos] = v;
  }
  __syncthreads();

  double out[n];
  const double* Uc = Ut + (P * lz) * TX * TY + (P * ly) * TX + P * lx;
  stiffness_column<P>(Uc, TX * TY, TX, Fr + cl * nd, Fs + cl * nd, sD, dm, g, coeff, i, j, active, out, ablate);

  // y tile: zero, accumulate the cells of the block with LDS atomics
  __syncthreads();
  for (int pos = t; pos < tile; pos += 256) Ut[pos] = 0.0;
  __syncthreads();
  if (active) {
    double* Yc = Ut + (P * lz) * TX * TY + (P * ly) * TX + P * lx;
#pragma unroll
    for (int k = 0; k < n; ++k) atomicAdd(&Yc[k * TX * TY + j * TX + i], out[k]);
  }
  __syncthreads();
  // flush: dofs interior to the block (or on the mesh boundary) are exclusive to
  // this workgroup -> plain read-modify-write; faces shared with a neighbouring
  // block -> global atomic add.
  const bool sx0 = Bx > 0, sy0 = By > 0, sz0 = Bz > 0;
  const bool sx1 = I0 + TX < NX, sy1 = J0 + TY < NY, sz1 = K0 + TZ < NZ;
  for (int pos = t; pos < tile; pos += 256) {
    const int I = pos % TX, J = (pos / TX) % TY, K = pos / (TX * TY);
    if (I < EX && J < EY && K < EZ) {
      const size_t gidx = (size_t)(I0 + I) + (size_t)NX * ((size_t)(J0 + J) + (size_t)NY * (K0 + K));
      const bool shared = (sx0 && I == 0) || (sx1 && I == TX - 1) || (sy0 && J == 0) || (sy1 && J == TY - 1)
                          || (sz0 && K == 0) || (sz1 && K == TZ - 1);
      const double v = Ut[pos];
      if (ablate & 1) {
        if (v == 1.2345e300) y[gidx] = v;
      } else if (shared)
        unsafeAtomicAdd(&y[gidx], v);
      else
        y[gidx] += v;
    }
  }
}

// --------------------------------------------------------------------------
// launchers
// --------------------------------------------------------------------------
template <int P>
static int launch_stiffness_generic_t(int ncells, const int32_t* d_dofmap, const double* d_G6blk,
                                      const double* d_D, const DMat& dm, double coeff, const double* d_x,
                                      double* d_y, hipStream_t s)
{
  hipLaunchKernelGGL(k_stiffness_generic<P>, dim3(CellBatch<P>::batches(ncells)), dim3(256), CellBatch<P>::stiffness_lds_bytes, s,
                     ncells, d_dofmap, reinterpret_cast<const double2*>(d_G6blk), d_D, dm, coeff, d_x, d_y, ablate_flags());
  WF_LAUNCH_CHECK();
  return WF_OK;
}

#ifndef WF_GENERIC_UP2_MAXP
#define WF_GENERIC_UP2_MAXP 4   // degrees that use the fully pipelined kernel (two geometry register sets; P5, P6 need 256 VGPRs + AGPRs: one wave per SIMD)
#endif
template <int P>
static int launch_stiffness_generic_u_t(int ncells, const int32_t* d_uoff, const int32_t* d_uniq,
                                        const uint16_t* d_loc, const double* d_G6blk, const double* d_D,
                                        const DMat& dm, double coeff, const double* d_x, double* d_y, hipStream_t s)
{
  const unsigned nb = CellBatch<P>::batches(ncells);
  constexpr size_t lds = CellBatch<P>::stiffness_lds_bytes;
#ifdef WF_GENERIC_U_PLAIN
  if (!WF_GENERIC_PIPELINED || ablate_flags() != 0) {
    hipLaunchKernelGGL(k_stiffness_generic_u<P>, dim3(nb), dim3(256), lds, s, ncells, d_uoff, d_uniq, d_loc,
                       reinterpret_cast<const double2*>(d_G6blk), d_D, dm, coeff, d_x, d_y, ablate_flags());
    WF_LAUNCH_CHECK();
    return WF_OK;
  }
#endif
  // persistent workgroups, as many as fit the chip at this kernel's register / LDS use (4 per CU at P <= 4)
  int per_cu = 0;
  if constexpr (P <= WF_GENERIC_UP2_MAXP) {
    WF_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_stiffness_generic_up2<P>, 256, lds));
    const unsigned grid = std::min<unsigned>(nb, (unsigned)std::max(1, per_cu) * 256u);
    hipLaunchKernelGGL(k_stiffness_generic_up2<P>, dim3(grid), dim3(256), lds, s, ncells, (int)nb, d_uoff, d_uniq, d_loc,
                       reinterpret_cast<const double2*>(d_G6blk), d_D, dm, coeff, d_x, d_y);
  } else {
    WF_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_stiffness_generic_up<P>, 256, lds));
    const unsigned grid = std::min<unsigned>(nb, (unsigned)std::max(1, per_cu) * 256u);
    hipLaunchKernelGGL(k_stiffness_generic_up<P>, dim3(grid), dim3(256), lds, s, ncells, (int)nb, d_uoff, d_uniq, d_loc,
                       reinterpret_cast<const double2*>(d_G6blk), d_D, dm, coeff, d_x, d_y);
  }
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int launch_stiffness_generic_u(int P, int ncells, const int32_t* d_uoff, const int32_t* d_uniq, const uint16_t* d_loc,
                               const double* d_G6blk, const double* d_D, const DMat& dm, double coeff,
                               const double* d_x, double* d_y, hipStream_t s)
{
  if (ncells == 0) return WF_OK;
  return dispatch_degree(P, "stiffness: degree must be 1..7", [&](auto p) {
    return launch_stiffness_generic_u_t<decltype(p)::value>(ncells, d_uoff, d_uniq, d_loc, d_G6blk, d_D, dm, coeff, d_x, d_y, s);
  });
}

int launch_stiffness_generic(int P, int ncells, const int32_t* d_dofmap, const double* d_G6blk,
                             const double* d_D, const DMat& dm, double coeff, const double* d_x, double* d_y,
                             hipStream_t s)
{
  if (ncells == 0) return WF_OK;
  return dispatch_degree(P, "stiffness: degree must be 1..7", [&](auto p) {
    return launch_stiffness_generic_t<decltype(p)::value>(ncells, d_dofmap, d_G6blk, d_D, dm, coeff, d_x, d_y, s);
  });
}

template <int P>
static int launch_stiffness_box_t(int nx, int ny, int nz, int bx, int by, int bz, const double* d_G6blk,
                                  const double* d_D, const DMat& dm, double coeff, const double* d_x,
                                  double* d_y, hipStream_t s)
{
  constexpr int n = CellBatch<P>::n, nd = CellBatch<P>::nd;
  const int CB = bx * by * bz;
  const int tile = (P * bx + 1) * (P * by + 1) * (P * bz + 1);
  const unsigned nb = (unsigned)(((nx + bx - 1) / bx) * ((ny + by - 1) / by) * ((nz + bz - 1) / bz));
  const size_t lds = (size_t)(((tile + 1) & ~1) + 2 * CB * nd + n * n) * sizeof(double);
  hipLaunchKernelGGL(k_stiffness_box<P>, dim3(nb), dim3(256), lds, s, nx, ny, nz, bx, by, bz,
                     reinterpret_cast<const double2*>(d_G6blk), d_D, dm, coeff, d_x, d_y, ablate_flags());
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int launch_stiffness_box(int P, int nx, int ny, int nz, int bx, int by, int bz, const double* d_G6blk,
                         const double* d_D, const DMat& dm, double coeff, const double* d_x, double* d_y,
                         hipStream_t s)
{
  if ((size_t)nx * ny * nz == 0) return WF_OK;
  if (bx * by * bz * (P + 1) * (P + 1) > 256) {
    set_error("stiffness_box: block does not fit a 256-thread workgroup");
    return WF_ERR_INVALID;
  }
  return dispatch_degree(P, "stiffness_box: degree must be 1..7", [&](auto p) {
    return launch_stiffness_box_t<decltype(p)::value>(nx, ny, nz, bx, by, bz, d_G6blk, d_D, dm, coeff, d_x, d_y, s);
  });
}

}  // namespace wf
