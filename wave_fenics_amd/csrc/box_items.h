// Work items of the box marching kernels, and their split into interior / interface lists (box_items.cpp; no HIP).
//
// item = column + columns * z segment.  Columns of the atomic forms are pieces of bx x by cells; the owner form cuts the
// lattice lines 0 .. P nx into pieces of P*bx x P*by from (0, 0).  Segment 0 has lz0 layers, every later one lz (the last
// one what is left of nz).  Plain inline functions: the kernels, the launchers, the host split and the host program
// tests/cxx/op_lists_walk.cpp all use these.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WF_BOX_FN __host__ __device__ inline
#else
#define WF_BOX_FN inline
#endif

namespace wf {

struct BoxColumns {
  int nbx, nby;
  int count() const { return nbx * nby; }
};
inline BoxColumns box_columns(int nx, int ny, int bx, int by) { return {(nx + bx - 1) / bx, (ny + by - 1) / by}; }
inline BoxColumns box_owner_columns(int P, int nx, int ny, int bx, int by)
{
  return box_columns(P * nx + 1, P * ny + 1, P * bx, P * by);
}
inline int box_segments(int nz, int lz, int lz0) { return 1 + (std::max(nz - lz0, 0) + lz - 1) / lz; }

// Layers [z0, z1) of z segment seg of a box (lz0 = lz unless the operator is split for the ghost exchange: a short first
// segment keeps the work that reads the z ghost plane small).  box_segments counts them.
struct BoxSegment {
  int z0, z1;
};
WF_BOX_FN BoxSegment box_segment(int seg, int nz, int lz, int lz0)
{
  const int z0 = seg == 0 ? 0 : lz0 + (seg - 1) * lz, e = seg == 0 ? lz0 : z0 + lz;
  return {z0, nz < e ? nz : e};
}

// ---- the split (box_items.cpp) ----
// What the split needs to know of a box marching operator.
struct BoxItemShape {
  int P, nx, ny, nz;
  bool owner;     // the columns are the owner form's
  int cbx, cby;   // cells per column
  int lz, lz0;    // layers per z segment; wf_tuning.lz0 (0: the default of 3) for the first one under a z ghost plane
};
struct BoxItemLists {
  int lz0_split = 0;                // layers of the first z segment
  std::vector<int32_t> items[4];    // interior, interface, interior A, interior B
};

// The two halves of the interior, which let a caller hide BOTH halo directions: forward update under half A, reverse
// update under half B (alternate items, so that both halves span the mesh).
void alternate_interior(std::vector<int32_t> (&items)[4]);

// An item is "interface" when it reads a ghost value of x or adds into one of y: when its footprint holds a ghost.
// Atomic forms: the closed lattice box of the column's cells over planes [P z0, P z1].  Owner form: that box and P
// lattice lines / planes below it, [I0 - P, I0 + P cbx] x [J0 - P, J0 + P cby] x [P z0 - P, P z1].
// With a ghost plane below, the first z segment is kept short (lz0, default 3 layers): only its first layer reads the
// ghost plane, but the whole segment has to wait for the halo, and the less interface work there is the earlier the
// reverse exchange can start under the interior.
// by_faces: the ghosts are whole lower lattice planes I = 0, J = 0, K = 0.
BoxItemLists split_box_items_by_faces(const BoxItemShape& s, bool ghost_x0, bool ghost_y0, bool ghost_z0);
// by_ghosts: ghost[ndofs] marks the ghost positions of the lattice, x fastest.  There is a z ghost plane below when
// every position of plane K = 0 is a ghost, which is what ghost_z0 says.  (A ghost anywhere in the plane is not enough:
// an x or y ghost plane alone holds the plane's edge, and the same planes then gave another segmentation than by_faces.)
BoxItemLists split_box_items_by_ghosts(const BoxItemShape& s, const std::vector<char>& ghost);

}  // namespace wf
