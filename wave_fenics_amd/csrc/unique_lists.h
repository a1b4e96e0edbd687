// Batch-unique gather/scatter lists (unique_lists.cpp; no HIP): for every batch of CB consecutive cells the sorted list of
// its distinct dofs (uniq, offsets uoff) and the position of each element-local dof in that list (loc).  Kernels read x
// once per unique dof, sum the batch in LDS and issue one global atomic per unique dof: uniq becomes global addresses
// and loc 16-bit LDS indices, neither checked again.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace wf {

struct UniqueLists {
  std::vector<int32_t> uoff;   // [nbatch + 1]
  std::vector<int32_t> uniq;   // the batches' unique dofs, each batch ascending
  std::vector<uint16_t> loc;   // [ncells * nd]: uniq[uoff[b] + loc[e]] == dofmap[e] for entry e of batch b
  int largest() const;         // most unique dofs of a batch
};

// dofmap[ncells * nd], batches of CB cells (the last one what is left).  false: a batch holds more than 65535 unique
// dofs (out is then incomplete).
bool build_unique_lists(const int32_t* dofmap, size_t ncells, int nd, int CB, UniqueLists* out);

// The local indices of the dense simplex kernels' batches of NCB cells, two to a word in the kernels' operand order:
// locP[b][ks / 2][lg][cell] holds the local index of dof 4 ks + lg in bits 16 (ks & 1) .. 16 (ks & 1) + 15
// (dense_loc_of, dense_simplex.h); KT = ceil(nd / 4) k-steps.  Lanes past nd or past the last cell hold zero.
std::vector<uint32_t> pack_dense_loc(const std::vector<uint16_t>& loc, size_t ncells, int nd, int KT, int NCB);

}  // namespace wf
