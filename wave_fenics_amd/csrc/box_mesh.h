// The box written out as a dofmap mesh (box_space.cpp, host only, no HIP): the lexicographic dofmap, the vertex map and
// the wf_op_desc over them.  wf_box_dofmap, wf_box_mesh and the box entry points that ARE the dofmap entry point
// (wf_op_create_box with WF_FLAG_ORDERED, wf_cell_form_create_box) share these.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "wavehip.h"

namespace wf {

// vertex v = a + 2 b + 4 c of cell `cell` (x fastest) on the implicit vertex lattice of an nx x ny x nz box
inline size_t box_vertex(int nx, int ny, size_t cell, int v)
{
  const size_t cx = cell % nx, cy = (cell / nx) % ny, cz = cell / ((size_t)nx * ny);
  return (cx + (v & 1)) + (size_t)(nx + 1) * ((cy + ((v >> 1) & 1)) + (size_t)(ny + 1) * (cz + ((v >> 2) & 1)));
}

// dofmap[cell][i + n (j + n k)] = dof (P cx + i, P cy + j, P cz + k) -> I + NX (J + NY K), cells x fastest
void fill_box_dofmap(int P, int nx, int ny, int nz, int32_t* dofmap);
// geom_dofmap[cell][v] = box_vertex(cell, v)
void fill_box_vertex_map(int nx, int ny, int nz, int32_t* geom_dofmap);

// what a box entry point asks of its mesh arguments, in this order: the degree (WF_ERR_UNSUPPORTED), "bad mesh", a dof
// lattice of fewer than 2^31 points
int check_box_args(const char* who, int degree, int nx, int ny, int nz, const double* h_xverts);

// The descriptor of the dofmap entry points for a box that passed check_box_args: it points into the two arrays held
// here, its rows are the box's cells in lexicographic order.
struct BoxDesc {
  std::vector<int32_t> dofmap, geom_dofmap;
  wf_op_desc desc{};
  BoxDesc(int kind, int P, int nx, int ny, int nz, const double* h_xverts, double c0, const double* h_cell_coeff, int flags,
          const wf_tuning* tuning);
  BoxDesc(const BoxDesc&) = delete;
  BoxDesc& operator=(const BoxDesc&) = delete;
};

}  // namespace wf
