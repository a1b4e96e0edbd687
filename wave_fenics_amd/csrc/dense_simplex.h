// What the two MFMA kernels for affine tetrahedra share: k_stiffness_dense (stiffness_dense.hip) and
// k_mass_dense_simplex (mass_dense_simplex.hip).  The batch shape, the LDS layout of an A-operand table, the prefetch
// pieces of the batch pipeline with the rules they obey, the device plan of the batches and the Jacobian of a cell; the
// host entry points of both operators are declared at the end.
#pragma once
#include "device_array.h"

namespace wf {

// ---- the batch shape ----
// One wave owns 16 cells (the N dimension of v_mfma_f64_16x16x4_f64), the four waves of a workgroup a batch of 64
// consecutive cells.  x enters through the batch's unique-dof tile in LDS, the cell results are summed per unique dof
// in LDS and leave with one global atomic per unique dof; workgroups are persistent and stage their table once.
constexpr int kDenseWaves = 4;

// LDS layout of an A-operand table of KT = ceil(nd/4) k-steps: row pitch KP = dense_pitch(KT), and the 16 rows of an
// MFMA tile stored in the order pi(j) = dense_row_perm(j).
// LDS has 64 banks x 4 B and serves a ds_read_b64 32 lanes at a time.  An A operand is read as T[row(lc)][4 ks + lg]
// (16 rows x 2 columns per half wave: the first stiffness product, the mass product), the B-side table of the second
// stiffness product as T[row(lg)][16 dt + lc] (2 rows x 16 columns).  With KP = 4 KT + 2 (twice an odd number) and rows
// in the order pi(j) = (j >> 1) + 8 (j & 1) both patterns touch 32 distinct 8-byte banks: rows pi(.) KP cover all even
// bank pairs, and the two rows of a half wave in the second pattern are 8 KP = 16 (mod 32) doubles apart.  (KP = 4 KT + 1
// with rows in natural order had 2-way conflicts on a third of the lanes in both.)
__host__ __device__ constexpr int dense_pitch(int KT) { return 4 * KT + 2; }
__host__ __device__ constexpr int dense_row_perm(int j) { return (j >> 1) + 8 * (j & 1); }

// KT k-steps, NW waves, NU unique dofs of a batch per thread (numax <= NU NT: a compile-time bound for the
// register-staged gather of the next batch)
template <int KT, int NW, int NU>
struct DenseBatchShape {
  static constexpr int NT = 64 * NW;       // threads of a workgroup
  static constexpr int NCB = 16 * NW;      // cells of a batch
  static constexpr int KT2 = (KT + 1) / 2; // packed pairs of local indices per lane
  static constexpr int KP = dense_pitch(KT);
};
// the same two numbers for host code: cells of a batch, threads of a workgroup
constexpr int kDenseBatchCells = DenseBatchShape<1, kDenseWaves, 1>::NCB, kDenseThreads = DenseBatchShape<1, kDenseWaves, 1>::NT;

// NU of a plan: 5 covers the unique dofs of 64 well-numbered P4 cells (1154 on the Kuhn box), 9 the worst case of 64
// cells with 36 dofs each and none shared.  More than dense_nu(numax) kDenseThreads unique dofs no kernel holds.
constexpr int kDenseNuSmall = 5, kDenseNuLarge = 9;
constexpr int dense_nu(int numax) { return numax <= kDenseNuSmall * kDenseThreads ? kDenseNuSmall : kDenseNuLarge; }

// ---- the prefetch pieces of the batch pipeline ----
// A persistent workgroup of a grid of G runs batches b, b + G, ...  While batch b is computed, the cell payload (local
// indices, geometry or scale) of batch b + G, its x values and the unique-dof lists of the batches behind it are held in
// registers or in flight; the end-of-batch stage moves them up.  Three rules make that work, and both kernels obey them:
//  1. Every prefetch load is unconditional, on clamped indices: a thread past the end of a batch's unique-dof list
//     re-reads the last entry, a batch past the end re-reads the last batch.  Guards around loads become branches, and
//     at every join the compiler's vmcnt bookkeeping falls back to waiting for loads it has just issued.  Whether an
//     entry is live is decided where it is consumed (DenseRange::live, the kernels' count_of).
//  2. Per-batch scalars (the unique-dof range; the stiffness kernel's clamp flag) are fetched with VECTOR loads: as
//     scalar loads their (cold, ~1 us) latency sat in front of the MFMA section, and a pending s_load turns every LDS
//     wait into lgkmcnt(0).
//  3. In the end-of-batch stage every consumer of a prefetched register (the x values, the next lists, the next cell
//     payload, the next ranges) and the issue of the next x gather come BEFORE the first global atomic.  On gfx9 loads
//     and atomics share vmcnt and the compiler waits for vmcnt(0) once both kinds are pending, so an atomic issued
//     earlier puts its whole round trip (~0.5 us, NU times per batch) in front of the next consumer.
// The pieces are free functions; the stage loops that use them are written out in both kernels (cut into helpers they
// compile to another exec-mask structure: profiles/r23_summary.md).  The one deliberate difference between the two
// pipelines is the depth of the x gather: the stiffness kernel issues the gather of batch b + G behind the first
// product of batch b (its queued MFMAs cover the issue of the burst), the mass kernel that of batch b + 2G at the end of
// batch b (it has no MFMA section to speak of, and a whole iteration covers the latency).

// an opaque per-lane 0: pointer + this stays a global pointer but lives in VGPRs (rule 2)
__device__ __forceinline__ int dense_vgpr_zero()
{
  int z = 0;
  asm volatile("" : "+v"(z));
  return z;
}

__device__ __forceinline__ int32_t dense_vload_i32(const int32_t* p) { return p[dense_vgpr_zero()]; }

struct DenseRange {
  int32_t lo, hi;   // uoff[b], uoff[b + 1]  (b clamped to a valid batch; `live` says whether b < nbatch)
  bool live;
};
__device__ __forceinline__ DenseRange dense_load_range(const int32_t* uoff, int nbatch, int b)
{
  const int bb = b < nbatch ? b : nbatch - 1;
  return DenseRange{dense_vload_i32(uoff + bb), dense_vload_i32(uoff + bb + 1), b < nbatch};
}
// thread t's share of a batch's unique-dof list: entries t, t + NT, ...
template <int NT, int NU>
__device__ __forceinline__ void dense_load_uq(int32_t (&uq)[NU], const int32_t* uniq, const DenseRange& rg, int t)
{
#pragma unroll
  for (int m = 0; m < NU; ++m) uq[m] = uniq[min(rg.lo + t + NT * m, rg.hi - 1)];
}
template <int NU>
__device__ __forceinline__ void dense_load_x(double (&xr)[NU], const double* x, const int32_t (&uq)[NU])
{
#pragma unroll
  for (int m = 0; m < NU; ++m) xr[m] = x[uq[m]];
}
// Local indices, locP[b][KT2][4][NCB]: the position of dof 4 ks + lg of cell slot c in the batch's unique list sits in
// bits 16 (ks & 1) .. 16 (ks & 1) + 15 of word [b][ks / 2][lg][c].  They travel as packed pairs: loaded as 16-bit values
// the compiler packs them two to a register right after the load, i.e. waits for the prefetch it has just issued.  Each
// kernel loads its lane's KT2 words in its load_cell, next to its own payload (C_c and a_c, or s_c).
template <int KT2>
__device__ __forceinline__ uint32_t dense_loc_of(const uint32_t (&loc)[KT2], int ks)
{
  return (loc[ks >> 1] >> (16 * (ks & 1))) & 0xffffu;
}

// ---- host side ----
// The gather/scatter plan of the batches on the device: for every batch of kDenseBatchCells consecutive cells the sorted
// list of its distinct dofs (uniq, offsets uoff) and the packed local indices locP (dense_loc_of).
struct DenseBatchPlanDev {
  int nbatch = 0;
  int numax = 0;               // most unique dofs of a batch (at least 1)
  DevArray<uint32_t> locP;     // [nbatch][ceil(KT/2)][4][kDenseBatchCells]
  DevArray<int32_t> uoff;      // [nbatch + 1]
  DevArray<int32_t> uniq;      // unique dofs of all batches
  // plans on the host, then uploads; refuses a batch with more than 65535 unique dofs before it touches the device
  int build(int nd, int KT, int ncells, const int32_t* dofmap);   // op_setup.hip
  size_t bytes() const { return locP.bytes() + uoff.bytes() + uniq.bytes(); }
};

// Jacobian of the affine tetrahedron with vertices v[0..3]: J[i][j] = x_{v[j+1]}[i] - x_{v[0]}[i]; returns det J, expanded
// along the first row.  T = double for the stiffness operator, long double for the mass.
template <class T>
T tet_jacobian(const double* xverts, const int32_t* v, T (&J)[9])
{
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) J[i * 3 + j] = (T)xverts[(size_t)v[j + 1] * 3 + i] - xverts[(size_t)v[0] * 3 + i];
  return J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
}

// dense simplex stiffness (stiffness_dense.hip)
struct DenseOpData;
int dense_setup(int nd, int nq, int ncells, int ndofs, const int32_t* dofmap, const double* dphi,
                const double* weights, const double* xverts, const int32_t* geom_dofmap, const double* cell_coeff,
                DenseOpData** out);
void dense_free(DenseOpData* d);
size_t dense_bytes(const DenseOpData* d);
int launch_stiffness_dense(const DenseOpData* d, double coeff, int do_clamp, const double* d_x, double* d_y,
                           hipStream_t s);
// dense simplex mass (mass_dense_simplex.hip): y += s_c A x per cell, A = Phi^T diag(w) Phi, s_c = |det J_c|
struct DenseMassData;
int dense_mass_setup(int nd, int nq, int ncells, const int32_t* dofmap, const double* phi, const double* weights,
                     const double* xverts, const int32_t* geom_dofmap, int use_fabs, const double* cell_coeff,
                     DenseMassData** out);
void dense_mass_free(DenseMassData* d);
size_t dense_mass_bytes(const DenseMassData* d);
int launch_mass_dense_simplex(const DenseMassData* d, const double* d_x, double* d_y, hipStream_t s);

}  // namespace wf
