// What the five marching kernels (stiffness_march, _idx, _ks, _owner, mass_march) share: a workgroup owns a column of
// BX x BY cells and marches through its z layers.  One copy each of the column's sizes, the steps that do not depend on
// the element kernel, the LDS sizes the host plans with, and the diagnostic trace.
#pragma once
#include <type_traits>

#include "box_items.h"
#include "common.h"

namespace wf {

// ---- sizes of a column: cells CB, dof tile TX x TY (TP positions per lattice plane) ----------------------------------
struct ColumnDims {
  int n, n2, nd, CB, TX, TY, TP;
};
constexpr ColumnDims column_dims(int P, int BX, int BY)
{
  const int n = P + 1, TX = P * BX + 1, TY = P * BY + 1;
  return {n, n * n, n * n * n, BX * BY, TX, TY, TX * TY};
}
template <int P, int BX, int BY>
struct ColumnTile {
  static constexpr ColumnDims dims = column_dims(P, BX, BY);
  static constexpr int n = dims.n, n2 = dims.n2, nd = dims.nd, CB = dims.CB, TX = dims.TX, TY = dims.TY, TP = dims.TP;
};

// Compile-time flags of a layer body (has_next, has_next2): the kernels keep one copy of the body per value, chosen by
// a uniform branch per layer, so that no prefetch sits behind a run-time `if` (stiffness_march.hip on what that costs).
using On = std::true_type;
using Off = std::false_type;

// ---- steps ----------------------------------------------------------------------------------------------------------
// The carried (z-shared) plane of a column at tile position (I, J): the sum over the up to four cells that share it.
// C holds the cells' private planes, C[cell][j][i] with cell = cb * BX + ca.  (The terms with cb > 0 exist only for BY >= 2.)
template <int P, int BX, int BY>
__device__ __forceinline__ double column_plane_sum(const double* C, int I, int J)
{
  constexpr int n = P + 1, n2 = n * n;
  const int ca = I / P, ia = I % P, cb = J / P, jb = J % P;
  double v = 0.0;
  if (cb < BY) {
    if (ca < BX) v += C[(cb * BX + ca) * n2 + jb * n + ia];
    if (ia == 0 && ca > 0) v += C[(cb * BX + ca - 1) * n2 + jb * n + P];
  }
  if (jb == 0 && cb > 0) {
    if (ca < BX) v += C[((cb - 1) * BX + ca) * n2 + P * n + ia];
    if (ia == 0 && ca > 0) v += C[((cb - 1) * BX + ca - 1) * n2 + P * n + P];
  }
  return v;
}

// LDS index of a 256-thread workgroup's store number m, position pos = t + 256 m of LIMIT: base + pos, or the thread's
// slot of the dump row when pos lies past LIMIT (only a thread's last position can).  Keeps the stores that consume
// prefetched registers in straight-line code.
template <int LIMIT>
__device__ __forceinline__ int tile_or_dump(int m, int pos, int base, int dump, int t)
{
  return (256 * (m + 1) <= LIMIT || pos < LIMIT) ? base + pos : dump + t;
}

// The layers of a z segment of a box: box_segment (box_items.h).

// ---- LDS of one workgroup, as the host plans with it (lz is chosen from these values; the kernel files assert, for
// every compiled cross-section, that they cover what the kernel's layout needs) -----------------------------------------
// k-split kernel (stiffness_march_ks.hip): two halves of whole waves, one thread per cell column (i, j) each
constexpr int ks_workgroup_size(int P, int BX, int BY)
{
  const ColumnDims c = column_dims(P, BX, BY);
  return 2 * (((c.CB * c.n2 + 63) / 64) * 64);
}
// workgroups of it per CU that the register file allows: one 512-thread, two (P >= 5) or three 256-thread ones
constexpr int ks_workgroups_per_cu(int P, int BX, int BY)
{
  const int WG = ks_workgroup_size(P, BX, BY);
  return WG >= 512 ? (P <= 3 ? 2 : 1) : (P <= 4 ? 768 / WG : 512 / WG);
}
constexpr size_t march_ks_lds_bytes(int P, int BX, int BY, int lz, bool idx)
{
  const ColumnDims c = column_dims(P, BX, BY);
  const size_t d = (size_t)2 * (P + 1) * c.TP + (size_t)2 * P * c.TP + (size_t)2 * c.CB * c.n2 + (size_t)3 * c.CB * c.nd + 2 * c.n2 + 2;
  return d * sizeof(double) + (idx ? (size_t)(P * lz + 1) * c.TP * sizeof(int32_t) : 0);
}
// dense mass (mass_march.hip), 1-D table of M points: whole cells per wave (a cell takes max(P + 1, M)^2 lanes); the
// index table streams through a ring of 4 P + 1 planes, so the footprint does not depend on the segment length
constexpr int mass_workgroup_size(int P, int M, int BX, int BY)
{
  const ColumnDims c = column_dims(P, BX, BY);
  const int MX = M > c.n ? M : c.n, CW = 64 / (MX * MX);
  return 64 * ((c.CB + CW - 1) / CW);
}
constexpr size_t mass_march_lds_bytes(int P, int M, int BX, int BY, int /*lz*/)
{
  const ColumnDims c = column_dims(P, BX, BY);
  const size_t WG = (size_t)mass_workgroup_size(P, M, BX, BY), MX = M > c.n ? M : c.n;
  const size_t d = (size_t)2 * (P + 1) * c.TP + (size_t)2 * P * c.TP + (size_t)2 * c.CB * c.n2 + (size_t)c.CB * c.n * MX * M + WG + 2;
  return d * sizeof(double) + ((size_t)(4 * P + 1) * c.TP + WG) * sizeof(int32_t);
}

// ---- diagnostic trace (tools/march_trace.sh, tools/mass_trace.sh): per-wave timestamps of `slots` phases of the first
// `iters` layers of the first 512 workgroups (first four waves), 100 MHz constant clock.  WF_COLUMN_TRACE declares the
// buffer and the extern "C" function that copies it to the host; WF_TRACE_STAMP(buf, it, slot) records one stamp.
#define WF_COLUMN_TRACE(buf, export_name, iters, slots)                                            \
  constexpr int buf##_iters = iters, buf##_slots = slots;                                          \
  __device__ unsigned long long buf[512 * 4 * iters * slots];                                      \
  extern "C" int export_name(unsigned long long* host, size_t n)                                   \
  {                                                                                                \
    void* sym = nullptr;                                                                           \
    if (hipGetSymbolAddress(&sym, HIP_SYMBOL(buf)) != hipSuccess) return -1;                       \
    if (n > sizeof(buf) / 8) n = sizeof(buf) / 8;                                                  \
    return hipMemcpy(host, sym, n * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;              \
  }
#define WF_TRACE_STAMP(buf, it, slot)                                                                        \
  if ((threadIdx.x & 63) == 0 && (it) < buf##_iters && blockIdx.x < 512 && (threadIdx.x >> 6) < 4)            \
  buf[((blockIdx.x * 4 + (threadIdx.x >> 6)) * buf##_iters + (it)) * buf##_slots + (slot)] = wall_clock64()

}  // namespace wf
