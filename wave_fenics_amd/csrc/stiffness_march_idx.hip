// k_march_idx<P, BX, BY, G>: the marching stiffness kernel (stiffness_march.hip) for
// an ARBITRARY dofmap -- StiffnessOperator::operator(), common/operators.hpp:183-200, on any
// conforming hexahedral mesh whose cells link up like a lattice (generic_plan.cpp), whatever
// the cell order and dof numbering.
//
// Same structure as the box kernel: a 256-thread workgroup owns a column of BX x BY cells and
// marches through <= lz layers; the next layer's geometry (48 B per point) and x planes are in
// flight while the current layer is computed; the z-shared plane is carried in a register; the
// finished planes go to y with one fp64 atomic per tile dof.  The only difference is where
// ADDRESSES come from: the column's dof tile [P lz + 1][P BY + 1][P BX + 1] is a table of dof
// offsets (PATTERN, shared by all work items with the same relative numbering) that is staged
// in LDS once per work item -- inside the layer loop the only global loads are then the
// prefetches (vmcnt retires loads in order: an index load consumed inside a layer would have to
// wait for the geometry prefetch issued before it).
// HBM-bound; algorithmic bytes ncells (48 nq + 4 nd) + 16 ndofs; the index
// table costs 4 P (P BX + 1)(P BY + 1) / (BX BY) bytes per cell when it is not L2-resident.
//
// Compiled for the stiffness operator at P <= 4 (P >= 5: stiffness_march_ks.hip; the dense mass
// operator on the same columns: mass_march.hip).
//
// Per-cell geometry (G != MarchGeom::point; every cell affine, on request: wf_tuning.geometry): geom is then
// Gc[(item lz + layer) CB + cell][3] (double2: G00 G01 | G02 G11 | G12 G22, weights left out, in the plan's frame, zeros
// in empty slots) and the element pass is the box kernel's (stiffness_march.hip): stiffness_phase1_cell + phase 2 for
// G = cell, stiffness_axes_cell for G = cell_axes (every G_c diagonal; dm = A = D^T diag(w) D, no Fr / Fs / sD and no
// barrier inside the element pass).  Each thread loads the 48 B of its cell one layer ahead.  Index tile, x prefetch, tile
// add, rotate, flush and epilogue are those of the per-point form.
#include "march_column.h"
#include "stiffness_core.h"

namespace wf {

// Diagnostic build (tools/march_trace.sh -DWF_IDX_TRACE): per-wave timestamps of the phases of the
// first layers of the first 512 workgroups, 100 MHz constant clock.
#ifdef WF_IDX_TRACE
WF_COLUMN_TRACE(g_idx_trace, wf_debug_idx_trace, 12, 6)
#define WF_ITR(slot) WF_TRACE_STAMP(g_idx_trace, trace_it, slot)
#else
#define WF_ITR(slot)
#endif

// static LDS of the kernel in doubles (every array starts on 16 bytes)
template <int P, int BX, int BY, MarchGeom G = MarchGeom::point>
struct IdxLayout : ColumnTile<P, BX, BY> {
  using T = ColumnTile<P, BX, BY>;
  static constexpr bool AX = G == MarchGeom::cell_axes;   // the axes form has no phase scratch and reads A from dm and dD
  static constexpr int nUx = (P + 1) * T::TP, nO = P * T::TP > T::CB * T::n2 ? P * T::TP : T::CB * T::n2,
                       nF = AX ? 1 : T::CB * T::nd, nD = AX ? 1 : T::n2;
  static constexpr int ndoubles = (nUx + 1) / 2 * 2 + (nO + 1) / 2 * 2 + 2 * ((nF + 1) / 2 * 2) + (nD + 1) / 2 * 2;
};

// Workgroups per CU (= waves per SIMD) of the forms.  Per point: two geometry register sets, 2.  Per cell: as the box
// kernel's forms, 4 at P <= 3 (128 VGPRs) and 3 at P4; the LDS budget of a work item's index tile follows
// (march_idx_lds_budget), so these forms march through fewer layers per item than the per-point one.
#ifndef WF_IDX_CELL_WAVES_P4
#define WF_IDX_CELL_WAVES_P4 3
#endif
#ifndef WF_IDX_AXES_WAVES_P4
#define WF_IDX_AXES_WAVES_P4 3
#endif
constexpr int march_idx_waves(MarchGeom G, int P)
{
  return G == MarchGeom::point ? 2 : P < 4 ? 4 : G == MarchGeom::cell ? WF_IDX_CELL_WAVES_P4 : WF_IDX_AXES_WAVES_P4;
}

template <int P, int BX, int BY, MarchGeom G>
__global__ __launch_bounds__(256, march_idx_waves(G, P)) void k_march_idx(int lz, int tile_size, const int32_t* __restrict__ item_base,
                                                      const int32_t* __restrict__ item_pattern,
                                                      const int32_t* __restrict__ item_layers,
                                                      const int32_t* __restrict__ pat_off,
                                                      const void* __restrict__ geom,
                                                      const double* __restrict__ dD, DMat dm, double coeff,
                                                      const double* __restrict__ x, double* __restrict__ y,
                                                      const int32_t* __restrict__ items)
{
  using L = IdxLayout<P, BX, BY, G>;
  constexpr bool PC = G != MarchGeom::point, AX = G == MarchGeom::cell_axes;
  constexpr int n = L::n, n2 = L::n2, nd = L::nd, CB = L::CB, NT = CB * n2, TX = L::TX, TP = L::TP;
  constexpr int NPOS = (P * TP + 255) / 256;        // flush / x-prefetch positions per thread
  constexpr int NPOS0 = ((P + 1) * TP + 255) / 256; // prologue x positions per thread
  constexpr int NCP = (TP + 255) / 256;             // positions of one plane per thread
  static_assert(NT <= 256, "column does not fit a 256-thread workgroup");

  __shared__ __attribute__((aligned(16))) double Ux[L::nUx];   // x planes of the layer
  // results of the layer's cells, summed where they share a face (ds_add_f64): planes 0..P-1 of the tile
  // (see stiffness_march.hip); reused for the carried plane in the epilogue
  __shared__ __attribute__((aligned(16))) double O[L::nO];
  __shared__ __attribute__((aligned(16))) double Fr[L::nF];
  __shared__ __attribute__((aligned(16))) double Fs[L::nF];
  __shared__ __attribute__((aligned(16))) double sD[L::nD];
  extern __shared__ __attribute__((aligned(16))) int32_t sIdx[];     // [(P lz + 1)][TP] dof offsets of the column, -1 = none

  const int t = threadIdx.x;
  // work item; an optional item list selects a subset (interior / interface split of the ghost exchange)
  const size_t item = items ? (size_t)items[blockIdx.x] : (size_t)blockIdx.x;
  const int nl = item_layers[item];
  const size_t gbase = (size_t)item_base[item];
  const int32_t* __restrict__ pat = pat_off + (size_t)item_pattern[item] * tile_size;
  const bool active = t < NT;
  const int cl = t / n2, ji = t % n2, j = ji / n, i = ji % n;
  const int lx = cl % BX, ly = cl / BX;

  // geometry registers: 3 x double2 per point (G upper triangle), in
  // two register sets that swap roles from layer to layer (the layer loop is unrolled by two): a
  // copy gcur = gnext ends up at the loop's back edge, behind the flush, and waits for the atomics
  // (per cell: the 3 x double2 of the thread's cell; axes form: the three scales of stiffness_axes_cell)
  using GReg = std::conditional_t<AX, double[3], std::conditional_t<PC, double2[3], double2[n][3]>>;
  GReg gA, gB;
  // per-cell forms: coeff * w_i w_j, the weights w_k (held in VGPRs for the whole item) and the thread's cell clamped
  // into the column (idle threads read the last one); axes form: the thread's rows A[i][.], A[j][.] and the per-axis
  // scales without G_c (coeff w_j, coeff w_i, coeff w_i w_j) -- dD carries the weights and A behind D and D^T
  [[maybe_unused]] double cw = 0.0, sx0 = 0.0, sy0 = 0.0, wk[n], ai[n], aj[n];
  [[maybe_unused]] const int clc = cl < CB ? cl : CB - 1;
  if constexpr (PC) {
    cw = coeff * dD[2 * n2 + i] * dD[2 * n2 + j];
#pragma unroll
    for (int k = 0; k < n; ++k) wk[k] = dD[2 * n2 + k];
  }
  if constexpr (AX) {
    sx0 = coeff * dD[2 * n2 + j], sy0 = coeff * dD[2 * n2 + i];
#pragma unroll
    for (int a = 0; a < n; ++a) {
      ai[a] = dD[2 * n2 + n + i * n + a];
      aj[a] = dD[2 * n2 + n + j * n + a];
    }
  }
  auto load_gc = [&](double2 (&g)[3], int l) {
    const double2* gp = static_cast<const double2*>(geom) + ((item * lz + l) * CB + clc) * 3;
#pragma unroll
    for (int p = 0; p < 3; ++p) g[p] = gp[p];
  };
  auto axes_scales = [&](double (&sc)[3], const double2 (&g)[3]) {
    sc[0] = sx0 * g[0].x;   // coeff G00 w_j
    sc[1] = sy0 * g[1].y;   // coeff G11 w_i
    sc[2] = cw * g[2].y;    // coeff G22 w_i w_j
  };
  auto load_g = [&](double2 (&g)[n][3], int l, int k0 = 0, int k1 = P + 1) {
    const double2* gp = static_cast<const double2*>(geom) + ((item * lz + l) * n * 3) * (size_t)NT + (t < NT ? t : NT - 1);
#pragma unroll
    for (int k = 0; k < n; ++k)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        if (k >= k0 && k < k1) g[k][p] = load_stream(gp + (size_t)(k * 3 + p) * NT);
  };
  // P >= 4: the next layer's geometry is requested in three instalments over the layer
  // (see stiffness_march.hip)
  constexpr bool kSpread = P >= 4 && !PC;
  constexpr int G1 = kSpread ? (n + 1) / 3 : n, G2 = kSpread ? (2 * n + 1) / 3 : n;
  // index table first (L2-resident for regular numberings), then the first layer's geometry and
  // x planes together: one HBM latency in the prologue, not two (loads retire in order)
  if constexpr (!AX)
    if (t < n * n) sD[t] = dD[t];
  for (int e = t; e < P * TP; e += 256) O[e] = 0.0;
  for (int e = t; e < (P * nl + 1) * TP; e += 256) sIdx[e] = pat[e];
  __syncthreads();
  if constexpr (AX) {
    double2 g0[3];
    load_gc(g0, 0);
    axes_scales(gA, g0);
  } else if constexpr (PC)
    load_gc(gA, 0);
  else
    load_g(gA, 0);
  // ---- prologue: x planes 0..P of the first layer -> LDS ------------------------
#pragma unroll
  for (int m = 0; m < NPOS0; ++m) {
    const int pos = t + 256 * m;
    if (pos < (P + 1) * TP) {
      const int32_t off = sIdx[pos];
      Ux[pos] = off >= 0 ? x[gbase + off] : 0.0;
    }
  }
  __syncthreads();

  double carry = 0.0;
  const double* Uc = Ux + (P * ly) * TX + P * lx;

  [[maybe_unused]] int trace_it = 0;
  // (idle threads load the last thread's geometry instead of branching around the loads; `has_next` is a compile-time
  // constant of the layer body at P4, a run-time flag below: stiffness_march.hip)
  auto layer = [&](auto hn_tag, GReg& gcur, GReg& gnext, int l) {
    const bool has_next = hn_tag;
    WF_ITR(0);
    // (a) next layer's x planes and geometry: in flight during this layer's arithmetic
    // (unconditional loads on clamped addresses -- dead entries and positions past the tile read the item's first
    // dof, the last layer its own planes again: a guard around a load is a branch, and behind it the compiler waits
    // for every memory operation still pending; what is live is decided where the registers are consumed)
    double xn[NPOS];
    const int ln = has_next ? l + 1 : l;
#pragma unroll
    for (int m = 0; m < NPOS; ++m) {
      const int pos = t + 256 * m;
      const int32_t off = pos < P * TP ? sIdx[(P * ln + 1) * TP + pos] : -1;
      xn[m] = x[gbase + (off >= 0 ? off : 0)];
    }
    // (per cell: 48 B on the clamped layer, unconditional like the x loads -- the last layer re-reads its own)
    [[maybe_unused]] double2 gl[3];
    if constexpr (AX)
      load_gc(gl, ln);      // turned into the scales gnext in (c)
    else if constexpr (PC)
      load_gc(gnext, ln);
    else if (has_next)
      load_g(gnext, l + 1, 0, G1);

    WF_ITR(1);
    // (b) element kernels of the layer
    double out[n];
    if constexpr (AX) {
      stiffness_axes_cell<P>(Uc, TP, TX, dm, ai, aj, wk, gcur[0], gcur[1], gcur[2], i, j, active, out);
    } else if constexpr (PC) {
      double ft[n];
      double2 gcw[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) gcw[p] = make_double2(cw * gcur[p].x, cw * gcur[p].y);
      stiffness_phase1_cell<P>(Uc, TP, TX, Fr + cl * nd, Fs + cl * nd, sD, dm, gcw, wk, i, j, active, ft);
      __syncthreads();
      stiffness_phase2<P>(Fr + cl * nd, Fs + cl * nd, sD, dm, ft, i, j, active, out);
    } else {
      double ft[n];
      stiffness_phase1<P>(Uc, TP, TX, Fr + cl * nd, Fs + cl * nd, sD, dm, gcur, coeff, i, j, active, ft);
      __syncthreads();
      if (kSpread && has_next) load_g(gnext, l + 1, G1, G2);
      stiffness_phase2<P>(Fr + cl * nd, Fs + cl * nd, sD, dm, ft, i, j, active, out);
    }
    WF_ITR(2);
    double xcp[NCP];
#pragma unroll
    for (int m = 0; m < NCP; ++m) {
      const int pos = t + 256 * m;
      xcp[m] = pos < TP ? Ux[P * TP + pos] : 0.0;
    }
    if (active) {
      out[0] += carry;        // z-shared plane: partial sum of the layer below
      carry = out[P];
      double* To = O + (P * ly + j) * TX + P * lx + i;
#pragma unroll
      for (int k = 0; k < P; ++k) __hip_atomic_fetch_add(To + k * TP, out[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    WF_ITR(3);

    // (c) rotate the x planes.  The rotation -- the consumers of the prefetched registers -- comes before the
    // flush, so that its wait does not include this layer's atomics (loads and atomics share vmcnt; see
    // stiffness_march.hip).  Measured both ways (cfg-size meshes): P4 0.245 -> 0.239 ms with the rotation first; the
    // dense mass, a third of the geometry bytes and shorter layers, is faster with the flush first (mass_march.hip).
    // (The two steps stay lambdas: written out in place they compile to other code.)
    auto rotate = [&]() {
    if (has_next) {
#pragma unroll
      for (int m = 0; m < NCP; ++m) {
        const int pos = t + 256 * m;
        if (pos < TP) Ux[pos] = xcp[m];
      }
#pragma unroll
      for (int m = 0; m < NPOS; ++m) {
        const int pos = t + 256 * m;
        if (pos < P * TP) Ux[TP + pos] = sIdx[(P * ln + 1) * TP + pos] >= 0 ? xn[m] : 0.0;
      }
    }
    };
    // (d) the finished planes, the cells of the layer already summed in O, go to y
    auto flush = [&]() {
#pragma unroll
    for (int m = 0; m < NPOS; ++m) {
      const int pos = t + 256 * m;
      if (pos >= P * TP) continue;
      const int32_t off = sIdx[(P * l) * TP + pos];
      const double v = O[pos];
      O[pos] = 0.0;
      if (off < 0) continue;
      unsafeAtomicAdd(y + gbase + off, v);
    }
    };
    rotate();
    // axes form: the G_c loads are consumed here too, before the layer's atomics (loads and atomics share vmcnt; consumed
    // in the next layer's element pass their wait would cover this layer's atomics).  The empty asm pins the products
    // here (stiffness_march.hip, (c)).
    if constexpr (AX) {
      axes_scales(gnext, gl);
      __asm__ volatile("" : "+v"(gnext[0]), "+v"(gnext[1]), "+v"(gnext[2]));
    }
    __builtin_amdgcn_sched_barrier(0);
    WF_ITR(4);
    if constexpr (!PC)
      if (kSpread && has_next) load_g(gnext, l + 1, G2, n);
    flush();
    WF_ITR(5);
    ++trace_it;

    __syncthreads();
  };
  for (int l = 0; l < nl; l += 2) {
    if constexpr (P < 4) {
      layer(l + 1 < nl, gA, gB, l);
      if (l + 1 < nl) layer(l + 2 < nl, gB, gA, l + 1);
    } else if (l + 1 < nl) {
      layer(On{}, gA, gB, l);
      if (l + 2 < nl)
        layer(On{}, gB, gA, l + 1);
      else
        layer(Off{}, gB, gA, l + 1);
    } else {
      layer(Off{}, gA, gB, l);
    }
  }

  // ---- epilogue: the last (carried) plane ------------------------------------
  if (active) O[cl * n2 + ji] = carry;
  __syncthreads();
#pragma unroll
  for (int m = 0; m < NCP; ++m) {
    const int pos = t + 256 * m;
    if (pos >= TP) continue;
    const int32_t off = sIdx[(P * nl) * TP + pos];
    if (off < 0) continue;
    const int J = pos / TX, I = pos % TX;
    const double v = column_plane_sum<P, BX, BY>(O, I, J);
    unsafeAtomicAdd(y + gbase + off, v);
  }
}

template <int P, int BX, int BY, MarchGeom G>
static int launch_g(const MarchPlanDev& pd, const double* d_G6blk, const double* d_D, const DMat& dm, double coeff,
                    const double* d_x, double* d_y, const int32_t* d_items, int nitems, hipStream_t s)
{
  const int nwg = d_items ? nitems : pd.nitems;
  if (nwg == 0) return WF_OK;
  const size_t dyn = (size_t)pd.tile_size * sizeof(int32_t);
  // static + dynamic LDS may exceed the 64 KB default limit.  The attribute is per device; it is set on
  // every launch (a cheap host call) instead of being cached in a process-wide static, which a second
  // device or a concurrent first launch from another host thread would not see.
  WF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_march_idx<P, BX, BY, G>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  hipLaunchKernelGGL((k_march_idx<P, BX, BY, G>), dim3((unsigned)nwg), dim3(256), dyn, s, pd.lz, pd.tile_size,
                     pd.d_item_base, pd.d_item_pattern, pd.d_item_layers, pd.d_pat_off,
                     static_cast<const void*>(d_G6blk), d_D, dm, coeff, d_x, d_y, d_items);
  return launch_status("stiffness_march_idx");
}

template <int P, int BX, int BY>
static int launch_t(MarchGeom geom, const MarchPlanDev& pd, const double* d_geom, const double* d_D, const DMat& dm, double coeff,
                    const double* d_x, double* d_y, const int32_t* d_items, int nitems, hipStream_t s)
{
  if (geom == MarchGeom::cell_axes) return launch_g<P, BX, BY, MarchGeom::cell_axes>(pd, d_geom, d_D, dm, coeff, d_x, d_y, d_items, nitems, s);
  if (geom == MarchGeom::cell) return launch_g<P, BX, BY, MarchGeom::cell>(pd, d_geom, d_D, dm, coeff, d_x, d_y, d_items, nitems, s);
  return launch_g<P, BX, BY, MarchGeom::point>(pd, d_geom, d_D, dm, coeff, d_x, d_y, d_items, nitems, s);
}

// the stiffness operator runs the k-split kernel (stiffness_march_ks.hip) at P >= 5
// P >= 5 runs the k-split kernel.  P4, any dofmap, cfg2: k_march_idx<4,5,2> 0.204 ms, k_march_ks<4,5,1,true> 0.208 ms
// (-DWF_IDX_KS_MINP=4 selects the latter)
#ifndef WF_IDX_KS_MINP
#define WF_IDX_KS_MINP 5
#endif
static bool march_idx_uses_ks(int P) { return P >= WF_IDX_KS_MINP; }

// the one cross-section per degree, with BX * BY == floor(256 / n^2) cells (geometry batch layout)
// (tests/nonbox_helpers.py STIFFNESS_BLOCK copies these: it predicts plan_fill from them)
#define WF_IDX_SHAPES(X) X(1, 8, 8) X(2, 7, 4) X(3, 4, 4) X(4, 5, 2)

void march_idx_shape(int kind, int P, int* bx, int* by)
{
  if (kind == OP_KIND_MASS) {
    mass_march_shape(P, P + 1, bx, by);   // (square table; a rectangular one: mass_march_shape itself)
    return;
  }
  if (march_idx_uses_ks(P)) {
    march_ks_shape(P, bx, by);   // keeps a compiled (*bx, *by), else the degree's default
    return;
  }
#define X(PP, BXX, BYY) \
  if (P == PP) *bx = BXX, *by = BYY;
  WF_IDX_SHAPES(X)
#undef X
}

// LDS of one workgroup: the kernel's static arrays (O counted as P planes per cell, which covers the tile) + the index tile
// (the axes form: Fr, Fs and sD are one padded double each)
constexpr size_t march_idx_static_lds_bytes(int P, int BX, int BY, MarchGeom geom = MarchGeom::point)
{
  const ColumnDims c = column_dims(P, BX, BY);
  if (geom == MarchGeom::cell_axes) return (size_t)((P + 1) * c.TP + c.CB * P * c.n2 + 8) * sizeof(double);
  return (size_t)((P + 1) * c.TP + c.CB * P * c.n2 + 2 * c.CB * c.nd + c.n2) * sizeof(double);
}
#define X(PP, BXX, BYY)                                                                                            \
  static_assert(march_idx_static_lds_bytes(PP, BXX, BYY) >= IdxLayout<PP, BXX, BYY>::ndoubles * sizeof(double), \
                "march_idx_lds_bytes does not cover the static arrays of k_march_idx");                         \
  static_assert(march_idx_static_lds_bytes(PP, BXX, BYY, MarchGeom::cell)                                          \
                    >= IdxLayout<PP, BXX, BYY, MarchGeom::cell>::ndoubles * sizeof(double),                        \
                "march_idx_lds_bytes does not cover the static arrays of k_march_idx (per cell)");              \
  static_assert(march_idx_static_lds_bytes(PP, BXX, BYY, MarchGeom::cell_axes)                                     \
                    >= IdxLayout<PP, BXX, BYY, MarchGeom::cell_axes>::ndoubles * sizeof(double),                   \
                "march_idx_lds_bytes does not cover the static arrays of k_march_idx (axes)");
WF_IDX_SHAPES(X)
#undef X

size_t march_idx_lds_bytes(int kind, int P, int BX, int BY, int lz, MarchGeom geom)
{
  if (kind == OP_KIND_MASS) return mass_march_lds_bytes(P, P + 1, BX, BY, lz);
  if (march_idx_uses_ks(P)) return march_ks_lds_bytes(P, BX, BY, lz, true);
  return march_idx_static_lds_bytes(P, BX, BY, geom) + (size_t)(P * lz + 1) * column_dims(P, BX, BY).TP * sizeof(int32_t);
}

// LDS a workgroup may use so that as many fit a CU as the kernel's registers allow: the dense-mass kernel runs two
// 256-thread workgroups per CU; the k-split stiffness kernel one 512-thread, two (P >= 5) or three 256-thread ones
// (the per-cell stiffness forms: march_idx_waves workgroups per CU)
size_t march_idx_lds_budget(int kind, int P, int BX, int BY, MarchGeom geom)
{
  if (kind == OP_KIND_STIFFNESS && !march_idx_uses_ks(P) && geom != MarchGeom::point)
    return (size_t)158 * 1024 / march_idx_waves(geom, P);
  if (kind != OP_KIND_STIFFNESS || !march_idx_uses_ks(P)) return (size_t)80 * 1024;
  return (size_t)158 * 1024 / ks_workgroups_per_cu(P, BX, BY);
}

int launch_stiffness_march_idx(int P, MarchGeom geom, const MarchPlanDev& pd, const double* d_G6blk, const double* d_D,
                               const DMat& dm, double coeff, const double* d_x, double* d_y, const int32_t* d_items,
                               int nitems, hipStream_t s)
{
  if (march_idx_uses_ks(P) && geom != MarchGeom::point) {
    set_error("stiffness_march_idx: the k-split kernel reads per-point geometry only");
    return WF_ERR_UNSUPPORTED;
  }
  if (march_idx_uses_ks(P))
    return launch_stiffness_march_ks_idx(P, pd.bx, pd.by, pd, d_G6blk, d_D, dm, coeff, d_x, d_y, d_items, nitems, s);
#define X(PP, BXX, BYY) \
  if (P == PP) return launch_t<PP, BXX, BYY>(geom, pd, d_G6blk, d_D, dm, coeff, d_x, d_y, d_items, nitems, s);
  WF_IDX_SHAPES(X)
#undef X
  set_error("stiffness_march_idx: degree must be 1..7");
  return WF_ERR_UNSUPPORTED;
}

}  // namespace wf
