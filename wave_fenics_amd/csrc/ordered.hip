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
// The pass-1 kernels are written next to their atomic twins and share their bodies: k_stiffness_ordered
// (stiffness_elementwise.h), k_mass_dense_ordered and k_mass_lumped_ordered (mass_batch.hip).  Every thread of a batch
// runs the same instruction sequence on its cell, so a cell's arithmetic does not depend on where the cell sits.  This
// file holds the plan, pass 2, and the launcher of k_stiffness_ordered, which is compiled here.
#include "stiffness_elementwise.h"  // k_stiffness_ordered<P>

namespace wf {

// --------------------------------------------------------------------------
// pass 1, stiffness
// --------------------------------------------------------------------------
template <int P>
static int launch_stiffness_ordered_t(int ncells, const int32_t* d_dofmap, const int32_t* d_slot, const double* d_G6blk,
                                      const double* d_D, const DMat& dm, double coeff, const double* d_x, double* d_v,
                                      hipStream_t s)
{
  hipLaunchKernelGGL(k_stiffness_ordered<P>, dim3(CellBatch<P>::batches(ncells)), dim3(256), CellBatch<P>::stiffness_lds_bytes, s,
                     ncells, d_dofmap, d_slot, reinterpret_cast<const double2*>(d_G6blk), d_D, dm, coeff, d_x, d_v);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int launch_stiffness_ordered(int P, int ncells, const int32_t* d_dofmap, const int32_t* d_slot, const double* d_G6blk,
                             const double* d_D, const DMat& dm, double coeff, const double* d_x, double* d_v, hipStream_t s)
{
  if (ncells == 0) return WF_OK;
  return dispatch_degree(P, "ordered stiffness: degree must be 1..7", [&](auto p) {
    return launch_stiffness_ordered_t<decltype(p)::value>(ncells, d_dofmap, d_slot, d_G6blk, d_D, dm, coeff, d_x, d_v, s);
  });
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
