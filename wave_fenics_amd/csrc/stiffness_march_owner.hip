// Box stiffness, separable (cell_axes) form, owner-computes update: y += -c0^2 K x without atomics.
//
// Every lattice dof of y is owned by exactly one thread, which reads it once and writes it once, with
// plain loads and stores.  The result at node (I, J, K) is gathered from the (at most 8) cells that
// contain it ("r06"); with the GLL rule at the nodes and a diagonal G_c per cell:
//   y(I,J,K) += sum_{cx ∋ I} (A[i_cx] . x(cx-line along x)) coeff w_j w_k sum_{cy ∋ J, cz ∋ K} G00(cx,cy,cz)
//             + sum_{cy ∋ J} (A[j_cy] . x(cy-line along y)) coeff w_i w_k sum_{cx ∋ I, cz ∋ K} G11(cx,cy,cz)
//             + sum_{cz ∋ K} (A[k_cz] . x(cz-line along z)) coeff w_i w_j sum_{cx ∋ I, cy ∋ J} G22(cx,cy,cz)
// with A = D^T diag(w) D and w_0 = w_P (symmetric rule), so the weight of a face node is the same in both cells.
//
// One 256-thread workgroup owns the lattice lines I in [I0, I0 + P BX), J in [J0, J0 + P BY) of a z segment
// (a column of BX x BY cells; the lattice is cut into such pieces from I = 0, so the closing line I = NX - 1 of a
// mesh whose nx is a multiple of BX falls into a column of its own) and marches in z, one thread per (I, J) line:
//   * z term: the thread's own x line, in a register window of 2P + 1 planes that rotates by P per layer;
//   * x and y terms: the layer's P + 1 x planes staged in LDS with a halo of P lattice lines on the -x / -y sides
//     and the closing line on the +x / +y sides (a (P BX + P + 1) x (P BY + P + 1) rectangle);
//   * scales: the G_c of the (BX + 1) x (BY + 1) cells around the column (halo cells included) staged in LDS per
//     layer; each thread sums the ones its node touches into five scales per layer and carries the previous layer's
//     for the shared plane k = 0;
//   * x, y and G_c of the next layer are prefetched one layer ahead as unconditional loads on clamped addresses, and
//     the layer body exists as two compile-time copies (has_next), as in k_stiffness_march;
//   * the rows of A indexed by the plane (row k of the z term, row P of the -x / -y / -z cells) are scalar operands from
//     the by-value DMat at P <= 4; at P >= 5 they would be up to 128 SGPRs, so only row P stays a scalar operand there
//     and the rows k < P are broadcast reads from LDS (as the z rows of D in k_march_ks), and the kernel is built for
//     two workgroups per CU instead of three (-DWF_OWNER_A_CONST: every such row a constant load from d_D instead).
// The summation order of every y entry is fixed, so the apply is bitwise reproducible.
//
// Work of a workgroup: a z segment of the uniform cut (item = column + columns * segment, lz layers each), or, with
// lz < 0, one run (column, z0, z1) of the operator's run table, which the host planned for this launch order.
//
// P = 4, lane exchange ("r18"; -DWF_OWNER_LANE_EXCHANGE=0: the form above): a cell's 4 x 4 lines are one
// 16-lane DPP row of a wave (lane = 16 c' + 4 j + i), so the in-cell operands of the +x / +y terms are the own x
// values xz[P + k] of other lanes of the row and come by v_mov_b32_dpp (quad_perm for the x line, row_ror for the
// y line) instead of from LDS; only the closing node of each line is read from the rectangle, and the -x / -y cell
// lines are read by the lanes with i = 0 / j = 0 alone.
//
// P = 4, 4x4 and 8x2, direct-to-LDS x planes ("r25"; -DWF_OWNER_DMA=0: the form above): the rectangle's
// rows are padded to an even length and a plane is cut into 16-byte pieces (owner_pieces.h), piece t of every plane owned
// by thread t.  A wave fills its 64 pieces of a plane with one global_load_lds_dwordx4 (lane-linear LDS image, per-lane
// source, 8-byte aligned); pieces outside the mesh are zeroed once per run and never loaded, pieces that straddle the
// mesh's last line in x take the register path, 8 bytes wide.  There are two buffers of P + 1 plane slots (and of G_c):
// layer kz reads one while planes 1..P of layer kz + 1 land in the other, plane P is copied across before the layer's
// only barrier, whose wait for the loads is the one the planes need, and the unroll by two keeps every LDS offset a
// compile-time constant.  No floating-point sum changes, so y keeps the bits of the register form.
#include <cstdlib>

#include "march_column.h"
#include "owner_pieces.h"
#include "stiffness_core.h"

namespace wf {

// workgroups per CU the register allocation must allow: three at P4 (<= 168 VGPRs, no scratch); P1-P3 fit more
#ifndef WF_OWNER_WAVES
#define WF_OWNER_WAVES 3
#endif
// P >= 5: at three per CU every cross-section spills to scratch (36 to 280 B/lane); two (<= 256 VGPRs) do not
#ifndef WF_OWNER_WAVES_HI
#define WF_OWNER_WAVES_HI 2
#endif

template <int P>
constexpr int owner_waves() { return P >= 5 ? WF_OWNER_WAVES_HI : WF_OWNER_WAVES; }

// P = 4: in-cell contraction operands from the registers of other lanes (1) or from LDS as at every other degree (0)
#ifndef WF_OWNER_LANE_EXCHANGE
#define WF_OWNER_LANE_EXCHANGE 1
#endif

template <int P>
constexpr bool owner_lane_exchange() { return WF_OWNER_LANE_EXCHANGE != 0 && P == 4; }

// P = 4: the x planes by direct-to-LDS loads into two buffers, one barrier per layer (1; DESIGN §4.2, "r25") or through
// registers into one buffer as at every other degree (0).  A cross-section whose plane has more than 256 pieces (2 x 8:
// 259) stays on the register form.
#ifndef WF_OWNER_DMA
#define WF_OWNER_DMA 1
#endif

template <int P, int BX, int BY>
constexpr bool owner_dma() { return WF_OWNER_DMA != 0 && P == 4 && owner_rect(P, BX, BY).NPC <= 256; }

// 16 bytes per lane from src (per lane, 8-byte aligned) to the LDS image that starts at dst (the same in every lane
// of the wave): lane l's bytes land at dst + 16 l.  Lanes that are masked off neither read nor write.
__device__ __forceinline__ void load_to_lds16(const double* src, double* dst)
{
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// Lane-exchange thread map: the BX BY = 16 cells of the column x-fastest, four per wave; lane = 16 c' + 4 j + i.
// Returns the owned line ti + P BX tj of thread t.
template <int P, int BX, int BY>
constexpr int owner_lane_line(int t)
{
  const int c = 4 * (t / 64) + (t % 64) / 16, j = (t % 16) / 4, i = t % 4;
  return P * (c % BX) + i + P * BX * (P * (c / BX) + j);
}

template <int P, int BX, int BY>
constexpr bool owner_lane_map_is_bijection()
{
  if (P != 4 || BX * BY != 16) return false;
  bool seen[256] = {};
  for (int t = 0; t < 256; ++t) {
    const int l = owner_lane_line<P, BX, BY>(t);
    if (l < 0 || l >= P * BX * P * BY || seen[l]) return false;
    seen[l] = true;
  }
  return true;
}

// v from another lane of the wave: CTRL = quad_perm (a | a << 2 | a << 4 | a << 6) or row_ror:n (0x120 + n).  Every
// lane of the wave must be active; both controls have a source lane for every lane, so no bound or mask applies.
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v)
{
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// a + b rounded on its own, never contracted with the product that made a or b
__device__ __forceinline__ double add_rounded(double a, double b)
{
#pragma clang fp contract(off)
  return a + b;
}
constexpr int dpp_quad(int a) { return a | a << 2 | a << 4 | a << 6; }
constexpr int dpp_row_ror(int n) { return 0x120 + n; }

template <int P, int BX, int BY>
__global__ __launch_bounds__(256, (owner_waves<P>())) void k_stiffness_owner(
    int nx, int ny, int nz, int lz, int lz0, int gbx, int gby, const double* __restrict__ Gc, const double* __restrict__ dD, DMat am,
    double coeff, const double* __restrict__ x, double* __restrict__ y, const int32_t* __restrict__ items,
    int ablate_arg)
{
  [[maybe_unused]] const int ablate = WF_ABLATE_FLAGS(ablate_arg);
  constexpr int n = P + 1;
  constexpr int LX = P * BX, LY = P * BY, NL = LX * LY;   // owned lines
  // direct-to-LDS form: the rectangle's rows padded to an even length, a plane in 16-byte pieces (owner_pieces.h),
  // two buffers of P + 1 plane slots and of the staged G_c
  constexpr bool dma = owner_dma<P, BX, BY>();
  constexpr int NB = dma ? 2 : 1;
  constexpr int RX = dma ? owner_rect(P, BX, BY).RX : LX + P + 1, RY = LY + P + 1, RP = RX * RY;   // staged rectangle of one plane
  constexpr int NPC = RP / 2, UB = (P + 1) * RP;   // pieces of a plane, doubles of a buffer
  constexpr int NPF = (P * RP + 255) / 256;          // x prefetch positions per thread (planes 1..P)
  constexpr int NCP = (RP + 255) / 256;              // positions of one plane
  constexpr int GCX = BX + 1, GC = GCX * (BY + 1), NG = 3 * GC;   // staged G00 | G11 | G22 of the cells
  constexpr int NGL = (NG + 255) / 256;
  static_assert(NL <= 256, "column does not fit a 256-thread workgroup");
  static_assert(!dma || (RP % 2 == 0 && NPC <= 256), "a plane is not one 16-byte piece per thread");
  constexpr bool lx = owner_lane_exchange<P>();
  static_assert(!lx || owner_lane_map_is_bijection<P, BX, BY>(), "lane-exchange map is not onto the owned lines");

  // x planes 0..P of the layer + a dump row for positions past the rectangle (branchless rotate, see (c))
  __shared__ __attribute__((aligned(16))) double Ux[dma ? NB * UB : UB + 256];
  __shared__ __attribute__((aligned(16))) double Gs[NB * NGL * 256];
  // A[k][a] for the rows indexed by the plane (k, a compile-time after unrolling).  P >= 5: rows k < P from LDS (filled
  // before the prologue's first barrier), row P from am.v; P <= 4: am.v
#ifdef WF_OWNER_A_CONST
  constexpr bool a_lds = false, a_const = P >= 5;
#else
  constexpr bool a_lds = P >= 5, a_const = false;
#endif
  __shared__ __attribute__((aligned(16))) double As[a_lds ? P * n : 1];
  auto arow = [&](int k, int a) {
    if (a_const) return dD[2 * n * n + n + k * n + a];
    if (a_lds && k < P) return As[k * n + a];
    return am.v[k * n + a];
  };

  const int t = threadIdx.x;
  const int NX = P * nx + 1, NY = P * ny + 1;
  const size_t plane = (size_t)NX * NY;
  const int nbxo = (NX + LX - 1) / LX, nbyo = (NY + LY - 1) / LY, ncols = nbxo * nbyo;
  // XCD-aware order: consecutive workgroups go round-robin to the 8 XCDs, so each XCD is given a contiguous run of
  // items instead; the halo lines a column reads then mostly belong to columns on the same XCD, and its L2 serves them
  // lz < 0: `items` is the operator's run table instead ("r19"; box_run_plan.h), entry blockIdx.x =
  // (column, z0, z1) of this workgroup, already in the order of its XCD.  Selects, not two branches that meet: the
  // uniform cut is turned into the same three values, and the kernels at the register limit keep their allocation.
  const bool table = lz < 0;
  const int nwg = (int)gridDim.x, xq = nwg / 8, xr = nwg % 8, xcd = (int)blockIdx.x % 8;
  const int b = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (int)blockIdx.x / 8;
  const int e = table ? 3 * (int)blockIdx.x : b;
  const int w0 = items ? items[e] : b;   // the item, or the run's column
  const int w1 = table ? items[e + 1] : 0, w2 = table ? items[e + 2] : 0;
  const BoxSegment zs = box_segment(w0 / ncols, nz, lz, lz0);
  const int col = table ? w0 : w0 % ncols, z0 = table ? w1 : zs.z0, z1 = table ? w2 : zs.z1;
  const int Bx = col % nbxo, By = col / nbxo;
  const int I0 = LX * Bx, J0 = LY * By, cx0 = BX * Bx, cy0 = BY * By;

  // ---- the thread's line ---------------------------------------------------
  const int tt = lx ? owner_lane_line<P, BX, BY>(t) : t < NL ? t : NL - 1;
  const int ti = tt % LX, tj = tt / LX, i = ti % P, j = tj % P;
  const int I = I0 + ti, J = J0 + tj;
  const bool own = t < NL && I < NX && J < NY;
  const int32_t yoff = own ? (int32_t)((size_t)I + (size_t)NX * J) : (int32_t)((size_t)I0 + (size_t)NX * J0);
  // LDS: own position, first node of the +x cell in the thread's row, first node of the +y cell in its column
  const int rown = (tj + P) * RX, cown = ti + P;
  const int cR = P + ti - i, rA = P + tj - j;

  // rows of A (the thread's i and j), 1-D weights, coefficient products
  double ai[n], aj[n], wk[n];
#pragma unroll
  for (int a = 0; a < n; ++a) {
    wk[a] = dD[2 * n * n + a];
    ai[a] = dD[2 * n * n + n + i * n + a];
    aj[a] = dD[2 * n * n + n + j * n + a];
  }
  const double cwj = coeff * wk[j], cwi = coeff * wk[i], cwij = coeff * wk[i] * wk[j];
  if constexpr (a_lds)
    if (t < P * n) As[t] = dD[2 * n * n + n + t];
  // lane exchange: row_ror:4m hands the lane the own value of another j of its i; which j is read off the rotate
  // itself, and ajr[m] is the entry of row j of A for it (ajr[0]: the lane's own node, ajr[P]: the closing node)
  [[maybe_unused]] double ajr[n];
  if constexpr (lx) {
    const int js[P] = {j, __builtin_amdgcn_mov_dpp(j, dpp_row_ror(4), 0xf, 0xf, false),
                       __builtin_amdgcn_mov_dpp(j, dpp_row_ror(8), 0xf, 0xf, false),
                       __builtin_amdgcn_mov_dpp(j, dpp_row_ror(12), 0xf, 0xf, false)};
#pragma unroll
    for (int m = 0; m < P; ++m) ajr[m] = dD[2 * n * n + n + j * n + js[m]];
    ajr[P] = aj[P];
  }

  // ---- staged positions (identical in every layer) -------------------------
  // position m: (I0 - P + c, J0 - P + r, pl); prefetch of the next layer: plane P*(kz+1) + pl + 1 -> LDS slot pl + 1
  int32_t poff[NPF];   // lattice offset relative to plane P*kz' + 1; -1 = outside the mesh or past the rectangle
#pragma unroll
  for (int m = 0; m < NPF; ++m) {
    const int pos = t + 256 * m;
    const int pl = pos / RP, r = pos % RP, II = I0 - P + r % RX, JJ = J0 - P + r / RX;
    poff[m] = -1;
    if (pos < P * RP && II >= 0 && II < NX && JJ >= 0 && JJ < NY)
      poff[m] = (int32_t)((size_t)II + (size_t)NX * JJ + plane * pl);
  }
  const int32_t pclamp = (int32_t)((size_t)I0 + (size_t)NX * J0);   // first owned position: always inside the mesh
  // direct-to-LDS form: the thread's piece of every plane (threads NPC.. have none), and where a wave's 64 pieces of
  // plane slot 0 of buffer 0 start in LDS
  [[maybe_unused]] const OwnerPiece pc = dma ? owner_piece(P, BX, BY, NX, NY, I0, J0, t) : OwnerPiece{PIECE_NONE, 0, 0};
  [[maybe_unused]] const bool pc_in = pc.kind == PIECE_INSIDE, pc_edge = pc.kind == PIECE_STRADDLING;
  [[maybe_unused]] double* const wave_img = dma ? Ux + 128 * __builtin_amdgcn_readfirstlane(t >> 6) : Ux;

  // G_c entries staged by this thread: entry e = comp * GC + cell, cell (lcx, lcy) = (cx0 - 1 + lcx, cy0 - 1 + lcy).
  // Gc is blocked by gbx x gby: the atomic form's cross-section at P <= 4 (the operator's geometry does not depend on the
  // update there), the owner cross-section at P >= 5 (no atomic per-cell kernel).
  const int nbx = (nx + gbx - 1) / gbx, nby = (ny + gby - 1) / gby;
  const size_t gstride = (size_t)nbx * nby * (gbx * gby) * 6;   // one cell layer of the blocked layout
  size_t gbase[NGL];
  bool gval[NGL];
#pragma unroll
  for (int q = 0; q < NGL; ++q) {
    const int e = t + 256 * q, comp = e / GC, c = e % GC;
    const int cx = cx0 - 1 + c % GCX, cy = cy0 - 1 + c / GCX;
    gval[q] = e < NG && cx >= 0 && cx < nx && cy >= 0 && cy < ny;
    const int cxc = gval[q] ? cx : 0, cyc = gval[q] ? cy : 0;
    gbase[q] = (((size_t)(cxc / gbx) + (size_t)nbx * (cyc / gby)) * (gbx * gby) + cxc % gbx + gbx * (cyc % gby)) * 6 +
               (comp == 0 ? 0 : comp == 1 ? 3 : 5);
  }
  auto load_g = [&](double (&g)[NGL], int kz) {
#pragma unroll
    for (int q = 0; q < NGL; ++q) g[q] = Gc[gbase[q] + gstride * kz];
  };
  auto store_g = [&](const double (&g)[NGL], int gb = 0) {   // gb: buffer of the direct-to-LDS form
#pragma unroll
    for (int q = 0; q < NGL; ++q)
      if constexpr (dma)
        Gs[gb * (NGL * 256) + t + 256 * q] = gval[q] ? g[q] : 0.0;
      else
        Gs[t + 256 * q] = gval[q] ? g[q] : 0.0;
  };
  // the thread's five scales of one layer from the staged G_c: x term (+x cell, -x cell), y term (+y, -y), z term
  const bool mi = i == 0, mj = j == 0;
  const int lR = (ti - i) / P + 1, lA = (tj - j) / P + 1;   // staged cell of the +x / +y cell
  auto scales = [&](double (&s)[5], int gb = 0) {
    const double* g0 = Gs;
    const double* g1 = Gs + GC;
    const double* g2 = Gs + 2 * GC;
    if constexpr (dma) g0 += gb * (NGL * 256), g1 += gb * (NGL * 256), g2 += gb * (NGL * 256);
    const int AR = lA * GCX + lR, AL = AR - 1, BR = AR - GCX, BL = BR - 1;
    const double x_ar = g0[AR], x_br = g0[BR], x_al = g0[AL], x_bl = g0[BL];
    const double y_ar = g1[AR], y_al = g1[AL], y_br = g1[BR], y_bl = g1[BL];
    const double z_ar = g2[AR], z_al = g2[AL], z_br = g2[BR], z_bl = g2[BL];
    s[0] = cwj * (mj ? x_ar + x_br : x_ar);
    s[1] = mi ? cwj * (mj ? x_al + x_bl : x_al) : 0.0;
    s[2] = cwi * (mi ? y_ar + y_al : y_ar);
    s[3] = mj ? cwi * (mi ? y_br + y_bl : y_br) : 0.0;
    const double za = mi ? z_ar + z_al : z_ar, zb = mi ? z_br + z_bl : z_br;
    s[4] = cwij * (mj ? za + zb : za);
  };

  // ---- prologue: x planes 0..P of layer z0 -> LDS, the scales of layers z0 - 1 and z0, y of layer z0 ------------
  double xz[2 * P + 1];   // x(I, J, P*kz - P + m)
  double sc[5], sf[4], spz;   // scales of the layer; the shared plane's x / y scales (this + previous layer); previous z
  double yA[P], yB[P];
  {
    double gp[NGL], gcur[NGL];
    load_g(gp, z0 > 0 ? z0 - 1 : z0);
    load_g(gcur, z0);
#pragma unroll
    for (int m = 0; m < P; ++m) {
      const long K = (long)P * z0 - P + m;
      const double v = x[plane * (size_t)(K >= 0 ? K : 0) + yoff];
      xz[m] = K >= 0 ? v : 0.0;
    }
#pragma unroll
    for (int k = 0; k < P; ++k) yA[k] = (ablate & 1) ? 0.0 : y[plane * (size_t)(P * z0 + k) + yoff];
    if constexpr (dma) {
      // direct-to-LDS form: what lies outside the mesh is set to +0.0 once, in both buffers, and never loaded; every
      // other piece of planes 0..P goes to buffer 0, a wave's 64 pieces by one load per plane, the straddling pieces'
      // positions in the mesh by 8-byte loads.  Nothing has read this LDS before, and the barriers below come after
      // the wait for all of these loads.
      if (pc.kind == PIECE_OUTSIDE || pc_edge)
#pragma unroll
        for (int m = 0; m < NB * (P + 1); ++m) Ux[m * RP + 2 * t] = Ux[m * RP + 2 * t + 1] = 0.0;
      const double* xb = x + plane * (size_t)(P * z0) + pc.off;
      if (pc_in)
#pragma unroll
        for (int m = 0; m <= P; ++m) load_to_lds16(xb + plane * m, wave_img + m * RP);
      if (pc_edge) {
        double xe[P + 1];
#pragma unroll
        for (int m = 0; m <= P; ++m) xe[m] = xb[plane * m];
#pragma unroll
        for (int m = 0; m <= P; ++m) Ux[m * RP + 2 * t + pc.half] = xe[m];
      }
    } else {
      // every plane load is in flight before the first is consumed: unconditional loads on clamped addresses, then
      // the LDS stores (positions past the rectangle go to the dump row), as in the rotate (c).  One decomposition of
      // the staged positions serves both ("r20"): planes 1..P through poff, exactly as the rotate loads
      // them, and plane 0 through the first NCP entries of poff from its own base (a position t + 256 m < RP of the
      // P RP staged ones lies in the first plane of its block, so its offset is the one within any plane).
      const double* xb = x + plane * (size_t)(P * z0) + plane;
      double xp0[NCP], xp[NPF];
#pragma unroll
      for (int m = 0; m < NCP; ++m) xp0[m] = (xb - plane)[t + 256 * m < RP && poff[m] >= 0 ? poff[m] : pclamp];
#pragma unroll
      for (int m = 0; m < NPF; ++m) xp[m] = xb[poff[m] >= 0 ? poff[m] : pclamp];
#pragma unroll
      for (int m = 0; m < NCP; ++m) {
        const int pos = t + 256 * m;
        Ux[tile_or_dump<RP>(m, pos, 0, (P + 1) * RP, t)] = (pos < RP && poff[m] >= 0) ? xp0[m] : 0.0;
      }
#pragma unroll
      for (int m = 0; m < NPF; ++m) {
        const int pos = t + 256 * m;
        Ux[tile_or_dump<P * RP>(m, pos, RP, (P + 1) * RP, t)] = poff[m] >= 0 ? xp[m] : 0.0;
      }
    }
    store_g(gp);
    __syncthreads();
    double sp[5];
    scales(sp);
    if (z0 == 0)
#pragma unroll
      for (int q = 0; q < 5; ++q) sp[q] = 0.0;
    __syncthreads();
    store_g(gcur);
    __syncthreads();
    scales(sc);
    // lane exchange: the shared plane's scales are the sum of two rounded products here and in the rotate, so a plane
    // gets the same bits whether a z segment starts at it or runs through it (parts with lz0 against the whole apply)
#pragma unroll
    for (int q = 0; q < 4; ++q) sf[q] = lx ? add_rounded(sc[q], sp[q]) : sc[q] + sp[q];
    spz = sp[4];
#pragma unroll
    for (int m = 0; m <= P; ++m) xz[P + m] = Ux[m * RP + rown + cown];
  }
  // lane exchange: the z term of the cell below the shared plane is formed once its P + 1 values are there (here, and
  // at the end of every layer for the next), in the order a = 0..P of the sum in (b); the lower half of the window
  // is then dead in the loop, which frees the registers that the lane moves need
  [[maybe_unused]] double zpc = 0.0;
  if constexpr (lx) {
#pragma unroll
    for (int a = 0; a < n; ++a) zpc += arow(P, a) * xz[a];
  }

  // diagnostic (WF_ABLATE bit 16, tools/ablate.py): the run ends after its prologue.  Everything the prologue forms
  // goes into a store that never happens, so that none of it is removed.
  if (ablate & 16) {
    double u = zpc + spz;
#pragma unroll
    for (int m = 0; m <= 2 * P; ++m) u += xz[m];
#pragma unroll
    for (int q = 0; q < 5; ++q) u += sc[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) u += sf[q];
#pragma unroll
    for (int k = 0; k < P; ++k) u += yA[k];
    if (u == 1.2345e300) y[yoff] = u;
    return;
  }

  // the x / y terms of one plane (LDS slot k of buffer cb): sx, sy = the scales of the +x / -x / +y / -y cells
  auto xy_terms = [&](int k, double s0, double s1, double s2, double s3, int cb = 0) {
    const double* L = Ux + k * RP;
    if constexpr (dma) L += cb * UB;
    double xr = 0.0, xl = 0.0, ya = 0.0, yb = 0.0;
    if constexpr (lx) {
      const double xo = xz[P + k];
      // -x / -y cells: only a lane on the cell's first line has them (its own node closes their line), so only
      // those lanes read them; in the others, which had the scale 0.0, the term stays +0.0.  Only the reads are under
      // the lane mask: the products are not, so that no wait for LDS falls inside a divergent branch.
      const double xc = L[rown + cR + P], yc = L[(rA + P) * RX + cown];   // closing nodes of the +x / +y lines
      double vl[P], vb[P];
#pragma unroll
      for (int a = 0; a < P; ++a) vl[a] = vb[a] = 0.0;
      if (mi)
#pragma unroll
        for (int a = 0; a < P; ++a) vl[a] = L[rown + cR - P + a];
      if (mj)
#pragma unroll
        for (int a = 0; a < P; ++a) vb[a] = L[(rA - P + a) * RX + cown];
#pragma unroll
      for (int a = 0; a < P; ++a) {
        xl += arow(P, a) * vl[a];
        yb += arow(P, a) * vb[a];
      }
      xl += arow(P, P) * (mi ? xo : 0.0);
      yb += arow(P, P) * (mj ? xo : 0.0);
      // the two sums are formed here, before the lane moves, and not where the compiler would sink them to (the `own`
      // branch of the store, after the moves): the eight operands would stay live beside the moved values, which
      // costs more than the 168 registers of three workgroups per CU
      asm volatile("" : "+v"(xl), "+v"(yb));
      // +x / +y cells: nodes 0..P-1 of the line from the lanes of the cell, the closing node from the rectangle.
      // xr in the order a = 0..P as below; ya own node first, then in the order of the rotate (fixed per lane).
      xr += ai[0] * dpp_move<dpp_quad(0)>(xo);
      xr += ai[1] * dpp_move<dpp_quad(1)>(xo);
      xr += ai[2] * dpp_move<dpp_quad(2)>(xo);
      xr += ai[3] * dpp_move<dpp_quad(3)>(xo);
      xr += ai[P] * xc;
      ya += ajr[0] * xo;
      ya += ajr[1] * dpp_move<dpp_row_ror(4)>(xo);
      ya += ajr[2] * dpp_move<dpp_row_ror(8)>(xo);
      ya += ajr[3] * dpp_move<dpp_row_ror(12)>(xo);
      ya += ajr[P] * yc;
    } else {
#pragma unroll
      for (int a = 0; a < n; ++a) {
        xr += ai[a] * L[rown + cR + a];
        xl += arow(P, a) * L[rown + cR - P + a];
        ya += aj[a] * L[(rA + a) * RX + cown];
        yb += arow(P, a) * L[(rA - P + a) * RX + cown];
      }
    }
    return xr * s0 + xl * s1 + ya * s2 + yb * s3;
  };
  auto store_y = [&](size_t K, double v) {
    double* dst = y + plane * K + yoff;
    if (ablate & 1) {
      if (v == 1.2345e300) *dst = v;
    } else if (own) {
      *dst = v;
    }
  };

  // One layer: owned planes P*kz .. P*kz + P - 1.  ycur holds their y (prefetched), ynext receives the next layer's.
  // Direct-to-LDS form: the layer reads buffer cb and fills the other one (a compile-time value at every call).
  auto layer = [&](auto hn_tag, double (&ycur)[P], double (&ynext)[P], int kz, int cb = 0) {
    constexpr bool has_next = decltype(hn_tag)::value;
    [[maybe_unused]] const int nb = 1 - cb;
    // (a) next layer's x planes, G_c and y: in flight during this layer's arithmetic.  Unconditional loads on
    // clamped addresses; what is live is decided where the registers are consumed, in (c).
    [[maybe_unused]] double xn[NPF], gn[NGL], xe[P];
    if constexpr (has_next) {
      const double* xb = x + plane * (size_t)(P * (kz + 1) + 1);
      if constexpr (dma) {
        // planes 1..P of the next layer straight into the other buffer, which nobody reads during this layer (its
        // last readers passed the previous layer's barrier); the straddling pieces' positions through registers
        if (pc_in)
#pragma unroll
          for (int m = 0; m < P; ++m) load_to_lds16(xb + plane * m + pc.off, wave_img + nb * UB + (m + 1) * RP);
        if (pc_edge)
#pragma unroll
          for (int m = 0; m < P; ++m) xe[m] = xb[plane * m + pc.off];
      } else {
#pragma unroll
        for (int m = 0; m < NPF; ++m) xn[m] = xb[poff[m] >= 0 ? poff[m] : pclamp];
      }
      load_g(gn, kz + 1);
#pragma unroll
      for (int k = 0; k < P; ++k) ynext[k] = (ablate & 1) ? 0.0 : y[plane * (size_t)(P * (kz + 1) + k) + yoff];
    }

    // (b) the P owned planes.  Plane 0 is shared with the layer below: x / y scales of both layers, two z terms.
#pragma unroll
    for (int k = 0; k < P; ++k) {
      double zc = 0.0;
#pragma unroll
      for (int a = 0; a < n; ++a) zc += arow(k, a) * xz[P + a];
      double v;
      if (k == 0) {
        double zp = 0.0;
        if constexpr (lx) {
          zp = zpc;
        } else {
#pragma unroll
          for (int a = 0; a < n; ++a) zp += arow(P, a) * xz[a];
        }
        v = wk[0] * xy_terms(0, sf[0], sf[1], sf[2], sf[3], cb) + zc * sc[4] + zp * spz;
      } else {
        v = wk[k] * xy_terms(k, sc[0], sc[1], sc[2], sc[3], cb) + zc * sc[4];
      }
      store_y((size_t)(P * kz + k), ycur[k] + v);
    }

    if constexpr (has_next) {
      if constexpr (lx) {
        zpc = 0.0;
#pragma unroll
        for (int a = 0; a < n; ++a) zpc += arow(P, a) * xz[P + a];
      }
      if constexpr (dma) {
        // (c) plane P of this buffer -> slot 0 of the other (its zeros with it), the straddling pieces' positions and
        // the next G_c; then the layer's one barrier.  Its wait for every load of (a) is the wait the planes need: a
        // wave's direct loads are ordered for the readers by that wait followed by the barrier.
        if (t < NPC) {
          const double c0 = Ux[cb * UB + P * RP + 2 * t], c1 = Ux[cb * UB + P * RP + 2 * t + 1];
          Ux[nb * UB + 2 * t] = c0;
          Ux[nb * UB + 2 * t + 1] = c1;
        }
        if (pc_edge)
#pragma unroll
          for (int m = 0; m < P; ++m) Ux[nb * UB + (m + 1) * RP + 2 * t + pc.half] = xe[m];
      } else {
        double xcp[NCP];
#pragma unroll
        for (int m = 0; m < NCP; ++m) {
          const int pos = t + 256 * m;
          xcp[m] = pos < RP ? Ux[P * RP + pos] : 0.0;
        }
        __syncthreads();
        // (c) rotate: plane P -> slot 0, the prefetched planes -> slots 1..P, G_c of the next layer.  No per-lane
        // branch between the loads and these stores: a thread's last position past the rectangle goes to the dump row.
#pragma unroll
        for (int m = 0; m < NCP; ++m) {
          const int pos = t + 256 * m;
          Ux[tile_or_dump<RP>(m, pos, 0, (P + 1) * RP, t)] = xcp[m];
        }
#pragma unroll
        for (int m = 0; m < NPF; ++m) {
          const int pos = t + 256 * m;
          Ux[tile_or_dump<P * RP>(m, pos, RP, (P + 1) * RP, t)] = poff[m] >= 0 ? xn[m] : 0.0;
        }
      }
      store_g(gn, nb);
      __syncthreads();
      // the z window rotates by P; the new scales, the shared plane's sums
#pragma unroll
      for (int m = 0; m <= P; ++m) xz[m] = xz[m + P];
#pragma unroll
      for (int m = 1; m <= P; ++m)
        if constexpr (dma)
          xz[P + m] = Ux[nb * UB + m * RP + rown + cown];
        else
          xz[P + m] = Ux[m * RP + rown + cown];
      double sn[5];
      scales(sn, nb);
#pragma unroll
      for (int q = 0; q < 4; ++q) sf[q] = lx ? add_rounded(sn[q], sc[q]) : sn[q] + sc[q];
      spz = sc[4];
#pragma unroll
      for (int q = 0; q < 5; ++q) sc[q] = sn[q];
    }
  };

  // unrolled by two: the y registers swap roles instead of being copied (a copy would wait for the prefetch), and the
  // direct-to-LDS form's two buffers swap with them
  for (int kz = z0; kz < z1; kz += 2) {
    if (kz + 1 < z1) {
      layer(On{}, yA, yB, kz, 0);
      if (kz + 2 < z1)
        layer(On{}, yB, yA, kz + 1, dma ? 1 : 0);
      else
        layer(Off{}, yB, yA, kz + 1, dma ? 1 : 0);
    } else {
      layer(Off{}, yA, yB, kz, 0);
    }
  }

  // ---- epilogue: the mesh's top plane P*nz (LDS slot P), owned by the last segment: the last layer's cells only --
  // Direct-to-LDS form: a run of an odd number of layers ends in buffer 0, of an even number in buffer 1.
  if (z1 == nz) {
    double zp = 0.0;
#pragma unroll
    for (int a = 0; a < n; ++a) zp += arow(P, a) * xz[P + a];
    double xy;
    if constexpr (dma)
      xy = ((z1 - z0) & 1) ? xy_terms(P, sc[0], sc[1], sc[2], sc[3], 0) : xy_terms(P, sc[0], sc[1], sc[2], sc[3], 1);
    else
      xy = xy_terms(P, sc[0], sc[1], sc[2], sc[3]);
    const double v = wk[0] * xy + zp * sc[4];
    const size_t K = (size_t)P * nz;
    const double y0 = (ablate & 1) ? 0.0 : y[plane * K + yoff];
    store_y(K, y0 + v);
  }
}

template <int P, int BX, int BY>
static int launch_owner_t(int nx, int ny, int nz, int lz, int lz0, int gbx, int gby, const double* d_Gcell, const double* d_D,
                          const DMat& am, double coeff, const double* d_x, double* d_y, const int32_t* d_items, int nitems,
                          hipStream_t s)
{
  const int nwg = d_items ? nitems : box_owner_columns(P, nx, ny, BX, BY).count() * box_segments(nz, lz, lz0);
  if (nwg == 0) return WF_OK;
  hipLaunchKernelGGL((k_stiffness_owner<P, BX, BY>), dim3((unsigned)nwg), dim3(256), 0, s, nx, ny, nz, lz, lz0, gbx, gby, d_Gcell,
                     d_D, am, coeff, d_x, d_y, d_items, ablate_flags());
  return launch_status("stiffness_march (owner)");
}

// The (P, variant, BX, BY) column cross-sections of the owner form (variant = wf_tuning.variant - 1 when the owner
// form runs; WF_MARCH_SHAPES is the table of the atomic forms).  P*BX x P*BY owned lines, at most 256: square, wide, tall.
#define WF_OWNER_SHAPES(X)                                                                                \
  X(1, 0, 16, 16) X(1, 1, 32, 8) X(1, 2, 8, 32) /* P1: 256 lines */                                         \
  X(2, 0, 8, 8) X(2, 1, 16, 4) X(2, 2, 4, 16)   /* P2: 256 lines */                                         \
  X(3, 0, 5, 5) X(3, 1, 7, 3) X(3, 2, 3, 7)     /* P3: 225 / 189 / 189 lines */                             \
  X(4, 0, 4, 4) X(4, 1, 8, 2) X(4, 2, 2, 8)     /* P4: 256 lines; default index 1 (8x2), as the atomic 5x2 */ \
  X(5, 0, 3, 3) X(5, 1, 5, 2) X(5, 2, 2, 5)     /* P5: 225 / 250 / 250 lines; default index 1 (5x2) */      \
  X(6, 0, 3, 2) X(6, 1, 7, 1) X(6, 2, 2, 3)     /* P6: 216 / 252 / 216 lines; default index 2 (2x3) */      \
  X(7, 0, 2, 2) X(7, 1, 5, 1) X(7, 2, 1, 5)     /* P7: 196 / 245 / 245 lines; default index 0 (2x2) */

bool march_owner_variant(int P, int variant, int* bx, int* by)
{
#define X(PP, V, BXX, BYY) \
  if (P == PP && variant == V) return *bx = BXX, *by = BYY, true;
  WF_OWNER_SHAPES(X)
#undef X
  return false;
}

int launch_stiffness_march_owner(int P, int variant, int nx, int ny, int nz, int lz, int lz0, int gbx, int gby,
                                 const double* d_Gcell,
                                 const double* d_D, const DMat& am, double coeff, const double* d_x, double* d_y,
                                 const int32_t* d_items, int nitems, hipStream_t s)
{
  if ((size_t)nx * ny * nz == 0) return WF_OK;
#define X(PP, V, BXX, BYY) \
  if (P == PP && variant == V) return launch_owner_t<PP, BXX, BYY>(nx, ny, nz, lz, lz0, gbx, gby, d_Gcell, d_D, am, coeff, d_x, d_y, d_items, nitems, s);
  WF_OWNER_SHAPES(X)
#undef X
  set_error("stiffness_march (owner): unsupported degree/variant");
  return WF_ERR_UNSUPPORTED;
}

int march_owner_resident(int P, int variant)
{
#define X(PP, V, BXX, BYY) \
  if (P == PP && variant == V) return resident_workgroups(k_stiffness_owner<PP, BXX, BYY>);
  WF_OWNER_SHAPES(X)
#undef X
  return 0;
}

}  // namespace wf
