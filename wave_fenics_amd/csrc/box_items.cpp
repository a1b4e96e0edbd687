// The interior / interface split of the box marching operators' work items (box_items.h), as plain host arithmetic.
#include "box_items.h"

namespace wf {

void alternate_interior(std::vector<int32_t> (&items)[4])
{
  items[2].clear();
  items[3].clear();
  for (size_t q = 0; q < items[0].size(); ++q) items[2 + (q & 1)].push_back(items[0][q]);
}

namespace {

// interface(Bx, By, seg, z0, z1): whether the item of column (Bx, By) and layers [z0, z1) is an interface item
template <class Interface>
BoxItemLists split(const BoxItemShape& s, bool ghost_below, Interface&& interface)
{
  BoxItemLists out;
  out.lz0_split = ghost_below ? std::max(1, std::min(s.lz0 > 0 ? s.lz0 : 3, s.lz)) : s.lz;
  const BoxColumns cols = s.owner ? box_owner_columns(s.P, s.nx, s.ny, s.cbx, s.cby) : box_columns(s.nx, s.ny, s.cbx, s.cby);
  const int ncols = cols.count(), nseg = box_segments(s.nz, s.lz, out.lz0_split);
  for (int seg = 0; seg < nseg; ++seg) {
    const BoxSegment zs = box_segment(seg, s.nz, s.lz, out.lz0_split);
    for (int col = 0; col < ncols; ++col)
      out.items[interface(col % cols.nbx, col / cols.nbx, seg, zs.z0, zs.z1) ? 1 : 0].push_back(col + ncols * seg);
  }
  alternate_interior(out.items);
  return out;
}

}  // namespace

BoxItemLists split_box_items_by_faces(const BoxItemShape& s, bool ghost_x0, bool ghost_y0, bool ghost_z0)
{
  const int P = s.P;
  return split(s, ghost_z0, [&](int Bx, int By, int seg, int z0, int) {
    return s.owner ? (ghost_x0 && P * s.cbx * Bx <= P) || (ghost_y0 && P * s.cby * By <= P) || (ghost_z0 && z0 <= 1)
                   : (ghost_x0 && Bx == 0) || (ghost_y0 && By == 0) || (ghost_z0 && seg == 0);
  });
}

BoxItemLists split_box_items_by_ghosts(const BoxItemShape& s, const std::vector<char>& ghost)
{
  const int P = s.P, NX = P * s.nx + 1, NY = P * s.ny + 1;
  const size_t plane = (size_t)NX * NY;
  bool gz = true;
  for (size_t g = 0; g < plane && gz; ++g) gz = ghost[g] != 0;
  const int halo = s.owner ? P : 0;
  return split(s, gz, [&](int Bx, int By, int, int z0, int z1) {
    const int I0 = std::max(0, P * Bx * s.cbx - halo), J0 = std::max(0, P * By * s.cby - halo);
    const int I1 = std::min(NX - 1, P * Bx * s.cbx + P * s.cbx), J1 = std::min(NY - 1, P * By * s.cby + P * s.cby);
    for (int K = std::max(0, P * z0 - halo); K <= P * z1; ++K)
      for (int J = J0; J <= J1; ++J) {
        const char* row = &ghost[(size_t)I0 + (size_t)NX * J + plane * K];
        for (int I = 0; I <= I1 - I0; ++I)
          if (row[I]) return true;
      }
    return false;
  });
}

}  // namespace wf
