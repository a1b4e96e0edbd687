// Dense (non-tensor-product) stiffness operator for affine simplex cells:
// the reference's skernel (common/operators.hpp:113-133) with arbitrary dense
// tables dphi[3][nq][nd], i.e. the "non-tensor-product operator path" of
// BASELINE.json configs[4] (P4 tetrahedra, nd = 35, nq = 64).
//
//   W[3 nq][cells] = T[3 nq][nd] . U[nd][cells]            (MFMA, f64 16x16x4)
//   F[dir][q][c]   = -c0^2 * sum_e clamp(w_q C_c)[dir][e] W[e][q][c]   (lane-local)
//   Y[nd][cells]   = T^T . F                                (MFMA, f64 16x16x4)
//
// This is the one place of the engine where the contraction is GEMM-shaped with a
// k-dimension worth a matrix core (k = nd = 35 and k = 3 nq = 192), so it runs on
// v_mfma_f64_16x16x4_f64.  One wave owns 16 cells (the N dimension); W stays in
// registers between the two products: the f64 accumulator layout
// (row = (lane>>4) + 4*reg, col = lane&15) is exactly the B-operand layout of
// k-step `reg`, so F feeds the second product with no LDS round trip.
// The table T lives in LDS; geometry is 6 doubles per affine cell.
// Gather/scatter ("permute/scatter stress"): per batch of 64 cells the host
// computes the list of unique dofs; x is read once per unique dof into LDS, the
// cell results are summed per unique dof in LDS (ds_add_f64) and leave with one
// global atomic per unique dof.  What this kernel shares with k_mass_dense_simplex (mass_dense_simplex.hip) -- batch
// shape, LDS layout of the table, prefetch pieces and the rules of the batch pipeline, the device plan -- is
// dense_simplex.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "dense_simplex.h"

namespace wf {

typedef double double4_t __attribute__((ext_vector_type(4)));

// Diagnostic build (tools/dense_trace.sh): per-wave timestamps of the phases of the first batches
// of every workgroup, 100 MHz constant clock.
#ifdef WF_DENSE_TRACE
constexpr int kDenseTraceIters = 12, kDenseTraceSlots = 6;
__device__ unsigned long long g_dense_trace[512 * 4 * kDenseTraceIters * kDenseTraceSlots + 512 * 4];   // + HW_ID | XCC_ID << 32 per wave
#define WF_DTR(slot)                                                                                         \
  if ((threadIdx.x & 63) == 0 && trace_it < kDenseTraceIters && blockIdx.x < 512)                             \
  g_dense_trace[((blockIdx.x * 4 + (threadIdx.x >> 6)) * kDenseTraceIters + trace_it) * kDenseTraceSlots + (slot)] = wall_clock64()
#else
#define WF_DTR(slot)
#endif

// xt::isclose clamp to -1/0/1 (precomputation.hpp:105-107); the common case
// (no clamp zone hit) costs two compares.
__device__ __forceinline__ double clamp101d(double v)
{
  const double a = fabs(v);
  if (a <= 1e-8) return 0.0;
  if (fabs(a - 1.0) <= 1e-8 + 1e-5) return v < 0.0 ? -1.0 : 1.0;
  return v;
}

// QT = ceil(nq/16), KT = ceil(nd/4), DT = ceil(nd/16); KP = row pitch of T in LDS.
// The table's rows are stored in the order dense_row_perm at the pitch dense_pitch(KT): the first product reads
// T[row(lc)][4 ks + lg], the second T[row(lg)][16 dt + lc], both without bank conflicts (dense_simplex.h).
// NU: unique dofs of a batch per thread (DenseBatchShape).
// XR: output rows past the last whole 16-row tile that are NOT given an MFMA tile of their own
// (nd = 16 (DT - 1) + XR, XR <= 4; 0 = pad nd to 16 DT as before).  P4 tetrahedra have nd = 35:
// a third tile would spend 16 rows of matrix-core time on 3 rows of result, a fifth of the
// kernel's MFMA cycles.  Those rows are instead accumulated lane-locally with VALU FMAs in the
// shadow of the MFMAs (each lane owns the quadrature points q = lg mod 4 of its cell) and summed
// over the four lane groups once per batch.
// AC: the operator has a cell coefficient a_c (wavehip.h, "Cell coefficients"): Ag holds one per cell slot, loaded and
// prefetched with the lane's C_c, and the factor of F is coeff * a_c.  It cannot be folded into C_c: the clamp windows
// are windows of w_q C_c.  The AC = false instantiations never touch Ag and are the kernel without the parameter.
template <int QT, int KT, int DT, int NW, int NU, int XR, bool AC>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_stiffness_dense(int nd, int nq, int nbatch, int numax,
                                                         const double* __restrict__ Tg,      // [3*16*QT][KP] padded table
                                                         const double* __restrict__ wq,      // [16*QT] weights (0 beyond nq)
                                                         const double* __restrict__ Cg,      // [nbatch*16*NW][6]
                                                         const double* __restrict__ Ag,      // AC: [nbatch*16*NW] cell coefficients (padding 0)
                                                         const uint32_t* __restrict__ locP,  // [nbatch][ceil(KT/2)][4][16*NW]: local index of dof 4(2j)+lg | that of dof 4(2j+1)+lg << 16
                                                         const int32_t* __restrict__ uoff,   // [nbatch+1]
                                                         const int32_t* __restrict__ uniq,   // unique dofs of all batches
                                                         const uint8_t* __restrict__ clampb, // [nbatch] 1: some w_q C_c of the batch lies in a clamp window
                                                         double coeff, int do_clamp, const double* __restrict__ x,
                                                         double* __restrict__ y, int ablate_arg, int stagger)
{
  [[maybe_unused]] const int ablate = WF_ABLATE_FLAGS(ablate_arg);
  using Shape = DenseBatchShape<KT, NW, NU>;
  constexpr int NQP = 16 * QT, KP = Shape::KP, NT = Shape::NT, NCB = Shape::NCB, KT2 = Shape::KT2;
  constexpr int DTM = XR > 0 ? DT - 1 : DT, XN = XR > 0 ? XR : 1;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* T = smem;                 // [3*NQP][KP]
  double* sw = T + 3 * NQP * KP;    // [NQP]
  double* Xu = sw + NQP;            // [numax]  x at the unique dofs of the batch
  double* Yu = Xu + numax;          // [numax]  sum of the cell results per unique dof

  (void)nq;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lc = lane & 15, lg = lane >> 4;
  // Two workgroups share a CU (one wave of each per SIMD; workgroups b and b + 256, per HW_ID in
  // tools/dense_trace.py).  Experiment knob WF_DENSE_STAGGER (default 0 = off): start the second
  // resident workgroup half a batch late so that its gather / scatter phases fall under the other's
  // MFMA section.  It gains nothing (0.600 / 0.607 / 0.614 ms at 0 / 1 / 2 sleeps before the other
  // changes of the round): the phase offset persists, but a lone wave keeps the MFMA pipe only 57 %
  // busy -- barely more than half of the saturated pipe two overlapping MFMA sections share.
  if (stagger > 0 && ((blockIdx.x / 256) & 1)) {
    for (int i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(127);   // 127 * 64 cycles each
  }
  for (int p = t; p < 3 * NQP * KP; p += NT) T[p] = Tg[p];
  for (int p = t; p < NQP; p += NT) sw[p] = wq[p];

  // Software pipeline over the batches of this (persistent) workgroup: while batch b is in its
  // MFMA section, the gather of batch b + G is in flight in registers (x values xr, local
  // indices and geometry) and the unique-dof list of batch b + 2G is being fetched (uq), so the
  // only memory latency left on the critical path is the scatter's.  Inside the MFMA section no
  // global load is consumed (loads retire in order).
  const int G = gridDim.x;
  // the prefetch pieces and their rules: dense_simplex.h
  auto load_range = [&](int b) { return dense_load_range(uoff, nbatch, b); };
  auto load_uq = [&](int32_t (&uq)[NU], const DenseRange& rg) { dense_load_uq<NT>(uq, uniq, rg, t); };
  // count_of and the locP load of load_cell are the same lines as in k_mass_dense_simplex: as shared functions they changed
  // the code (profiles/r23_summary.md)
  auto count_of = [&](const DenseRange& rg) { return rg.live ? rg.hi - rg.lo : 0; };
  auto load_clamp = [&](int b) -> int {   // a per-batch scalar: a vector load
    return clampb[(b < nbatch ? b : nbatch - 1) + dense_vgpr_zero()];
  };
  auto load_x = [&](double (&xr)[NU], const int32_t (&uq)[NU]) {   // dense_load_x, but for the ablation
#pragma unroll
    for (int m = 0; m < NU; ++m) xr[m] = (ablate & 4) ? 1.0 + m : x[uq[m]];
  };
  auto load_cell = [&](uint32_t (&loc)[KT2], double (&C)[6], double& ac, int b) {
    const int bb = b < nbatch ? b : nbatch - 1;
    if constexpr (AC) ac = Ag[(size_t)bb * NCB + wave * 16 + lc];
#pragma unroll
    for (int j = 0; j < KT2; ++j) loc[j] = locP[(((size_t)bb * KT2 + j) * 4 + lg) * NCB + wave * 16 + lc];
    const double* cp = Cg + ((size_t)bb * NCB + wave * 16 + lc) * 6;
#pragma unroll
    for (int e = 0; e < 6; ++e) C[e] = cp[e];
  };
  int32_t uq_cur[NU], uq_nxt[NU];     // unique dofs (this thread's share) of the batch being computed / of the next one
  double xr[NU];
  uint32_t loc[KT2], locn[KT2];
  auto loc_of = [&](int ks) { return dense_loc_of(loc, ks); };
  double C[6], Cn[6];
  [[maybe_unused]] double ac = 1.0, acn = 1.0;   // AC: the lane's cell coefficient, this batch's and the next one's
  // prologue: first batch straight into LDS, indices of the second
  int nu_cur, nu_nxt;   // live entries of uq_cur / uq_nxt
  {
    const DenseRange r0 = load_range(blockIdx.x), r1 = load_range(blockIdx.x + G);
    load_uq(uq_cur, r0);
    nu_cur = count_of(r0);
    load_x(xr, uq_cur);
    load_cell(loc, C, ac, blockIdx.x);
    load_uq(uq_nxt, r1);
    nu_nxt = count_of(r1);
  }
  DenseRange rg2 = load_range(blockIdx.x + 2 * G);   // range of the batch whose unique-dof list is fetched next
  int clamp_cur = load_clamp(blockIdx.x);
#pragma unroll
  for (int m = 0; m < NU; ++m) {
    const int u = t + NT * m;
    if (u < numax) {
      Xu[u] = xr[m];
      Yu[u] = 0.0;
    }
  }

  [[maybe_unused]] int trace_it = 0;
#ifdef WF_DENSE_TRACE
  if ((threadIdx.x & 63) == 0 && blockIdx.x < 512)
    g_dense_trace[512 * 4 * kDenseTraceIters * kDenseTraceSlots + blockIdx.x * 4 + (threadIdx.x >> 6)] =
        (unsigned long long)__builtin_amdgcn_s_getreg(63492) | ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32);
#endif
  for (int batch = blockIdx.x; batch < nbatch; batch += G) {
    // the -1/0/1 clamp of G (precomputation.hpp:105-107) is the identity unless a product w_q C_c
    // falls into one of its windows; the host marks the batches where that happens (same
    // double-precision products), every other batch skips ~200 VALU instructions per slab
    const bool clamp_here = do_clamp && clamp_cur;
    double coeff_c = coeff;   // the factor of F: -c0^2, times the cell's coefficient
    if constexpr (AC) coeff_c = coeff * ac;
    __syncthreads();   // Xu holds this batch's x values, Yu is zero
    WF_DTR(0);

    // B operands of the first product: this lane's dof values, one per k-step
    double ub[KT];
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) {
      const double v = (ablate & 32) ? 1.0 + ks : Xu[loc_of(ks)];   // padded k: local index 0, a valid entry
      ub[ks] = (4 * ks + lg) < nd ? v : 0.0;
    }
    WF_DTR(1);
    // gather of the next batch (registers) and index list of the one after it
    int32_t uq_nn[NU];
    load_cell(locn, Cn, acn, batch + G);
    load_uq(uq_nn, rg2);
    const int nu_nn = count_of(rg2);
    const DenseRange rg3 = load_range(batch + 3 * G);
    const int clamp_nxt = load_clamp(batch + G);

    double4_t Y[DTM];
#pragma unroll
    for (int dt = 0; dt < DTM; ++dt) Y[dt] = double4_t{0.0, 0.0, 0.0, 0.0};
    double yx[XN];
#pragma unroll
    for (int i = 0; i < XN; ++i) yx[i] = 0.0;

    // one 16-point slab of quadrature points at a time keeps the register
    // footprint small (3 accumulator tiles instead of 3*QT) -> more waves per SIMD
#pragma unroll 1
    for (int qt = 0; qt < ((ablate & 8) ? 0 : QT); ++qt) {
      // ---- W = T . U for the rows (dir, 16 qt .. 16 qt + 15) ---------------------
      // The A operands come from LDS.  Written as "read, then MFMA" the compiler waits for each
      // read right before the MFMA that uses it (ds_read -> s_waitcnt lgkmcnt(0) -> v_mfma), so
      // every k-step pays the LDS latency; explicit register double buffers keep the reads of
      // step s + 1 in flight behind the MFMAs of step s.
      double4_t W[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) W[e] = double4_t{0.0, 0.0, 0.0, 0.0};
      const double* Ta = T + (16 * qt + dense_row_perm(lc)) * KP + lg;   // + e NQP KP + 4 ks
      // (k_mass_dense_simplex rotates its DT row sets, 16 KP apart, in the same way: written out in both)
      double a3[3][3];   // rotating operand sets, reads two k-steps ahead (no copies: a copy waits for the read just issued)
#pragma unroll
      for (int e = 0; e < 3; ++e) a3[0][e] = Ta[e * NQP * KP];
      if (KT > 1) {
#pragma unroll
        for (int e = 0; e < 3; ++e) a3[1][e] = Ta[e * NQP * KP + 4];
      }
#pragma unroll
      for (int ks = 0; ks < KT; ++ks) {
        if (ks + 2 < KT) {
#pragma unroll
          for (int e = 0; e < 3; ++e) a3[(ks + 2) % 3][e] = Ta[e * NQP * KP + 4 * (ks + 2)];
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the reads above the MFMAs (the scheduler sinks them otherwise)
#pragma unroll
        for (int e = 0; e < 3; ++e) W[e] = __builtin_amdgcn_mfma_f64_16x16x4f64(a3[ks % 3][e], ub[ks], W[e], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // the x gather of the next batch (NU scattered 8-byte loads per thread, up to 64 cache lines per
      // wave instruction) goes out behind the first product of the first slab, not in front of the
      // MFMA section: a wave blocks in the issue of such a burst (the CU's outstanding-request
      // capacity), and here its 27 queued MFMAs cover that
      if (qt == 0) load_x(xr, uq_nxt);
      // first A operands of the second product: in flight during the lane-local geometry product
      // (row = e NQP + 16 qt + pi(4 r + lg), column d = 16 dt + lc; columns >= 4 KT are never stored: pad = 0)
      // accumulator register r of lane group lg is quadrature point pi(4 r + lg) = 2 r + pi(lg) of the slab
      const double* Tb = T + (16 * qt + dense_row_perm(lg)) * KP + lc;   // + (e NQP + 2 r) KP + 16 dt
      const double* Tx = T + (16 * qt + dense_row_perm(lg)) * KP + 16 * DTM;   // extra rows: + (e NQP + 2 r) KP + i (no lc: broadcast reads)
      double b3[3][DTM], x3[3][XN];   // operands of steps st, st + 1, st + 2 of the second product
      auto load_b = [&](int st) {
        const int e = st / 4, r = st % 4;
#pragma unroll
        for (int dt = 0; dt < DTM; ++dt)
          b3[st % 3][dt] = (XR > 0 || (16 * dt + lc) < 4 * KT) ? Tb[(e * NQP + 2 * r) * KP + 16 * dt] : 0.0;
        if (XR > 0) {
#pragma unroll
          for (int i = 0; i < XN; ++i) x3[st % 3][i] = Tx[(e * NQP + 2 * r) * KP + i];
        }
      };
      load_b(0);
      load_b(1);
      // ---- F = coeff * G W (lane-local: the three directions of one (q, cell) share lane and register)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 16 * qt + 2 * r + dense_row_perm(lg);
        const double w = sw[q];
        double g00 = w * C[0], g01 = w * C[1], g02 = w * C[2], g11 = w * C[3], g12 = w * C[4], g22 = w * C[5];
        if (clamp_here) {   // precomputation.hpp:105-107
          g00 = clamp101d(g00); g01 = clamp101d(g01); g02 = clamp101d(g02);
          g11 = clamp101d(g11); g12 = clamp101d(g12); g22 = clamp101d(g22);
        }
        const double w0 = W[0][r], w1 = W[1][r], w2 = W[2][r];
        W[0][r] = coeff_c * (g00 * w0 + g01 * w1 + g02 * w2);
        W[1][r] = coeff_c * (g01 * w0 + g11 * w1 + g12 * w2);
        W[2][r] = coeff_c * (g02 * w0 + g12 * w1 + g22 * w2);
      }
      // ---- Y += T^T . F : accumulator register r of a tile is the B operand of k-step r
#pragma unroll
      for (int st = 0; st < 12; ++st) {
        const int e = st / 4, r = st % 4;
        if (st + 2 < 12) load_b(st + 2);
        const double b = W[e][r];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int dt = 0; dt < DTM; ++dt) Y[dt] = __builtin_amdgcn_mfma_f64_16x16x4f64(b3[st % 3][dt], b, Y[dt], 0, 0, 0);
        if (XR > 0) {
#pragma unroll
          for (int i = 0; i < XN; ++i) yx[i] = fma(x3[st % 3][i], b, yx[i]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    WF_DTR(2);
    // ---- per-batch accumulation over unique dofs, then one atomic per unique dof
#pragma unroll
    for (int dt = 0; dt < DTM; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ks = 4 * dt + r;   // d = 16 dt + lg + 4 r = 4 ks + lg
        if (!(ablate & 2) && ks < KT && 4 * ks + lg < nd) atomicAdd(&Yu[loc_of(ks < KT ? ks : 0)], Y[dt][r]);
      }
    if (XR > 0) {
      // row 16 DTM + i of cell lc: sum of the four lane groups' partial sums; lane group i scatters it
      // (its loc[4 DTM] is the local index of dof 16 DTM + lg)
      double mine = 0.0;
#pragma unroll
      for (int i = 0; i < XN; ++i) {
        double v = yx[i];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (lg == i) mine = v;
      }
      if (!(ablate & 2) && lg < XR) atomicAdd(&Yu[loc_of(4 * DTM < KT ? 4 * DTM : 0)], mine);
    }
    WF_DTR(3);
    __syncthreads();   // Yu complete; every wave has taken its operands out of Xu
    WF_DTR(4);
    // End-of-batch stage, the same lines as in k_mass_dense_simplex (mass_dense_simplex.hip), which also issues its
    // x gather here; written out in both, see rule 3 of dense_simplex.h: every consumer of a prefetched register (xr,
    // uq_nn, locn, Cn, the next ranges) comes BEFORE the first global atomic.
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
#pragma unroll
    for (int j = 0; j < KT2; ++j) loc[j] = locn[j];
#pragma unroll
    for (int e = 0; e < 6; ++e) C[e] = Cn[e];
    if constexpr (AC) ac = acn;
    rg2 = rg3;
    clamp_cur = clamp_nxt;
    const int nu_old = nu_cur;
    nu_cur = nu_nxt;
    nu_nxt = nu_nn;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int m = 0; m < NU; ++m) {
      if (t + NT * m < nu_old) {
        if (ablate & 1) {
          if (yv[m] == 1.2345e300) y[uq_old[m]] = yv[m];
        } else {
          unsafeAtomicAdd(&y[uq_old[m]], yv[m]);
        }
      }
    }
    WF_DTR(5);
    ++trace_it;
  }
}

struct DenseOpData {
  int nd = 0, nq = 0, QT = 0, KT = 0, DT = 0;
  DevArray<double> d_T, d_w, d_C;
  DevArray<double> d_a;   // cell coefficients per cell slot of the batches; empty: none, the AC = false kernel runs
  DenseBatchPlanDev plan;
  DevArray<uint8_t> d_clampb;
};

void dense_free(DenseOpData* d) { delete d; }

// Compiled shapes (QT, KT, DT, XR): Lagrange P1..P4 on the tetrahedron with the m = p Gauss-Jacobi
// rule, (nd, nq) = (4,1) (10,8) (20,27) (35,64), plus P4 with the m = 3 rule.  The XR = 0 form of a
// shape serves every other (nd, nq) with the same tile counts.
#define WF_DENSE_SHAPES(F) \
  F(1, 1, 1, 0)            \
  F(1, 3, 1, 0)            \
  F(2, 5, 2, 4) /* P3: nd = 20 = 16 + 4 */ \
  F(2, 5, 2, 0)            \
  F(4, 9, 3, 3) /* P4: nd = 35 = 32 + 3 */ \
  F(4, 9, 3, 0)            \
  F(2, 9, 3, 3)            \
  F(2, 9, 3, 0)

#define WF_DENSE_HAS(Q, K, D, X) || (QT == Q && KT == K && DT == D)
static bool dense_shape_compiled(int QT, int KT, int DT) { return false WF_DENSE_SHAPES(WF_DENSE_HAS); }
#undef WF_DENSE_HAS

// Host setup: padded table, per-cell affine geometry C = |det J| K K^T, per-batch
// unique-dof lists and local indices.
int dense_setup(int nd, int nq, int ncells, int ndofs, const int32_t* dofmap, const double* dphi,
                const double* weights, const double* xverts, const int32_t* geom_dofmap, const double* cell_coeff,
                DenseOpData** out)
{
  std::unique_ptr<DenseOpData, void (*)(DenseOpData*)> d(new DenseOpData, dense_free);
  d->nd = nd;
  d->nq = nq;
  d->QT = (nq + 15) / 16;
  d->KT = (nd + 3) / 4;
  d->DT = (nd + 15) / 16;
  if (!dense_shape_compiled(d->QT, d->KT, d->DT)) {
    set_error("stiffness_dense: (nd, nq) shape not compiled (supported: tetrahedron P1..P4)");
    return WF_ERR_UNSUPPORTED;
  }

  constexpr int NCB = kDenseBatchCells;
  const int NQP = 16 * d->QT, KP = dense_pitch(d->KT);
  std::vector<double> T((size_t)3 * NQP * KP, 0.0), w(NQP, 0.0);
  for (int dir = 0; dir < 3; ++dir)
    for (int q = 0; q < nq; ++q)
      for (int k = 0; k < nd; ++k) T[((size_t)dir * NQP + q) * KP + k] = dphi[((size_t)dir * nq + q) * nd + k];
  for (int q = 0; q < nq; ++q) w[q] = weights[q];
  const int nbatch = (ncells + NCB - 1) / NCB;
  std::vector<double> C((size_t)nbatch * NCB * 6, 0.0);
  for (int c = 0; c < ncells; ++c) {
    double J[9];
    const double det = tet_jacobian(xverts, geom_dofmap + (size_t)c * 4, J);
    const double id = 1.0 / det;
    double K[9];
    K[0] = (J[4] * J[8] - J[5] * J[7]) * id;
    K[1] = (J[2] * J[7] - J[1] * J[8]) * id;
    K[2] = (J[1] * J[5] - J[2] * J[4]) * id;
    K[3] = (J[5] * J[6] - J[3] * J[8]) * id;
    K[4] = (J[0] * J[8] - J[2] * J[6]) * id;
    K[5] = (J[2] * J[3] - J[0] * J[5]) * id;
    K[6] = (J[3] * J[7] - J[4] * J[6]) * id;
    K[7] = (J[1] * J[6] - J[0] * J[7]) * id;
    K[8] = (J[0] * J[4] - J[1] * J[3]) * id;
    const double ad = std::fabs(det);
    auto kk = [&](int a, int b) {
      double s = 0.0;
      for (int m = 0; m < 3; ++m) s += (K[a * 3 + m] * ad) * K[b * 3 + m];
      return s;
    };
    double* cc = &C[(size_t)c * 6];
    cc[0] = kk(0, 0); cc[1] = kk(0, 1); cc[2] = kk(0, 2); cc[3] = kk(1, 1); cc[4] = kk(1, 2); cc[5] = kk(2, 2);
    bool finite = ad > 0.0;   // false for det J = 0 and for NaN
    for (int e = 0; e < 6; ++e) finite = finite && std::isfinite(cc[e]);
    if (!finite) {
      set_error("wf_op_create_dense_simplex: cell " + std::to_string(c) + " is degenerate (det J is zero or not finite)");
      return WF_ERR_INVALID;
    }
  }
  (void)ndofs;
  // batches in which the clamp is not the identity
  std::vector<uint8_t> clampb(nbatch, 0);
  for (int c = 0; c < ncells; ++c) {
    bool hit = false;
    for (int q = 0; q < nq && !hit; ++q)
      for (int e = 0; e < 6 && !hit; ++e) {
        const double a = std::fabs(weights[q] * C[(size_t)c * 6 + e]);
        hit = (a > 0.0 && a <= 1e-8) || (a != 1.0 && std::fabs(a - 1.0) <= 1e-8 + 1e-5);
      }
    if (hit) clampb[c / NCB] = 1;
  }
  int rc;
  if ((rc = d->plan.build(nd, d->KT, ncells, dofmap)) != WF_OK) return rc;
  if ((rc = d->d_T.upload(T)) != WF_OK) return rc;
  if ((rc = d->d_w.upload(w)) != WF_OK) return rc;
  if ((rc = d->d_C.upload(C)) != WF_OK) return rc;
  if (cell_coeff) {   // in the batches' cell order, which is the caller's; padding slots 0
    std::vector<double> a((size_t)nbatch * NCB, 0.0);
    std::copy(cell_coeff, cell_coeff + ncells, a.begin());
    if ((rc = d->d_a.upload(a)) != WF_OK) return rc;
  }
  if ((rc = d->d_clampb.upload(clampb)) != WF_OK) return rc;
  *out = d.release();
  return WF_OK;
}

size_t dense_bytes(const DenseOpData* d)
{
  return d ? d->d_T.bytes() + d->d_w.bytes() + d->d_C.bytes() + d->d_a.bytes() + d->plan.bytes() + d->d_clampb.bytes()
           : 0;
}

template <int QT, int KT, int DT, int NW, int NU, int XR, bool AC>
static int launch_dense_t(const DenseOpData* d, double coeff, int do_clamp, const double* d_x, double* d_y,
                          hipStream_t s)
{
  constexpr int NQP = 16 * QT, KP = dense_pitch(KT);
  const DenseBatchPlanDev& pl = d->plan;
  const size_t lds = ((size_t)3 * NQP * KP + NQP + 2 * pl.numax) * sizeof(double);
  if (lds > 160 * 1024) {
    set_error("stiffness_dense: tables do not fit LDS");
    return WF_ERR_UNSUPPORTED;
  }
  auto kern = k_stiffness_dense<QT, KT, DT, NW, NU, XR, AC>;
  if (lds > 64 * 1024)
    WF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
#ifdef WF_DIAG   // diagnostic overrides, compiled in by tools/diag_build.sh only
  const int wgs_per_cu = std::getenv("WF_DENSE_WGS") ? std::atoi(std::getenv("WF_DENSE_WGS")) : 2;
  const int ablate = std::getenv("WF_ABLATE") ? std::atoi(std::getenv("WF_ABLATE")) : 0;
  const int stagger = std::getenv("WF_DENSE_STAGGER") ? std::atoi(std::getenv("WF_DENSE_STAGGER")) : 0;
#else
  const int wgs_per_cu = 2, ablate = 0, stagger = 0;
#endif
  const unsigned nb = (unsigned)std::min(pl.nbatch, 256 * wgs_per_cu);   // persistent: the table is staged into LDS once per workgroup
  hipLaunchKernelGGL(kern, dim3(nb), dim3(64 * NW), lds, s, d->nd, d->nq, pl.nbatch, pl.numax, d->d_T.data(),
                     d->d_w.data(), d->d_C.data(), d->d_a.data(), pl.locP.data(), pl.uoff.data(), pl.uniq.data(), d->d_clampb.data(),
                     coeff, do_clamp, d_x, d_y, ablate, stagger);
  return launch_status("stiffness_dense");
}

// the XR form of a shape where nd fits it, with the coefficient variant where the operator has one
#define WF_DENSE_LAUNCH(Q, K, D, X, NU)                                                                                        \
  (d->d_a.size() ? launch_dense_t<Q, K, D, kDenseWaves, NU, X, true>(d, coeff, do_clamp, d_x, d_y, s)                          \
                 : launch_dense_t<Q, K, D, kDenseWaves, NU, X, false>(d, coeff, do_clamp, d_x, d_y, s))
#define WF_DENSE_CASE(Q, K, D, X)                                                                                              \
  if (d->QT == Q && d->KT == K && d->DT == D && (X == 0 || d->nd == 16 * (D - 1) + X))                                          \
    return dense_nu(d->plan.numax) == kDenseNuSmall ? WF_DENSE_LAUNCH(Q, K, D, X, kDenseNuSmall) : WF_DENSE_LAUNCH(Q, K, D, X, kDenseNuLarge);

// (dense_setup has refused every shape that is not in WF_DENSE_SHAPES)
int launch_stiffness_dense(const DenseOpData* d, double coeff, int do_clamp, const double* d_x, double* d_y,
                           hipStream_t s)
{
  if (d->plan.nbatch == 0) return WF_OK;
  WF_DENSE_SHAPES(WF_DENSE_CASE)
  set_error("stiffness_dense: (nd, nq) shape not compiled (supported: tetrahedron P1..P4)");
  return WF_ERR_UNSUPPORTED;
}

}  // namespace wf

#ifdef WF_DENSE_TRACE
extern "C" int wf_debug_dense_trace(unsigned long long* host, size_t n)
{
  void* sym = nullptr;
  if (hipGetSymbolAddress(&sym, HIP_SYMBOL(wf::g_dense_trace)) != hipSuccess) return -1;
  if (n > sizeof(wf::g_dense_trace) / 8) n = sizeof(wf::g_dense_trace) / 8;
  return hipMemcpy(host, sym, n * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
