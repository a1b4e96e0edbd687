// Lattice-column plan of the indexed marching kernels (stiffness_march_idx.hip, stiffness_march_ks.hip, mass_march.hip)
// and what its consumers need to know about it: cell orientations, the plan itself, the interior / interface test and
// the numbering that follows the plan.  Host only: no device code, no HIP (march_plan.cpp links into a program alone;
// tests/cxx/march_plan_walk.cpp walks it under the sanitizers).
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace wf {

// ---- cell orientations: the 48 signed permutations of a cell's local axes ----
// code = 8 * perm + flips: lattice axis m of a cell runs along its own ("raw") axis raw_axis[m], reversed when flip[m]
void orient_decode(int code, int raw_axis[3], int flip[3]);
int orient_local_index(int code, int n, int i, int j, int k);   // raw tensor index of lattice-frame node (i, j, k)
int orient_sign(int code);                                       // +1 rotation, -1 reflection
// raw tensor index (x fastest) of every lattice-frame node / point of an n^3 tensor: map[i + n (j + n k)]
std::vector<int32_t> orient_node_map(int code, int n);
// orient_node_map per code, made when first asked for
struct OrientMaps {
  int n;
  std::vector<std::vector<int32_t>> maps = std::vector<std::vector<int32_t>>(48);
  const std::vector<int32_t>& operator()(int code);
};
// the 8 vertices (or corner dofs) of a cell relabelled into the lattice frame: out[v] = raw[corner of v], v = a + 2b + 4c
void orient_vertices(int code, const int32_t raw[8], int32_t out[8]);
// A symmetric tensor of a cell seen in the lattice frame: G'[a][b] = s_a s_b G[r_a][r_b] (r = the cell's own axis along
// lattice axis a, s = -1 when reversed) -- the operator D^T G D is the same in every frame.  at[a][b] is where entry
// (a, b) is stored, in g and out alike: kSym6 for the 6 components of the upper triangle, kFull9 for all 9.  The sign
// is applied as a negation.
constexpr int kSym6[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
constexpr int kFull9[3][3] = {{0, 1, 2}, {3, 4, 5}, {6, 7, 8}};
void orient_tensor(int code, const int (&at)[3][3], const double* g, double* out);

// ---- the plan ----
// why a mesh does not tile into lattice columns: one value per early exit of build_march_plan
enum class PlanReason : int {
  ok = 0,
  nonmanifold_face,     // three cells name the four corner dofs of one face
  position_taken,       // two cells of a component at one lattice position (placement is injective: not expected)
  nonconforming_tile,   // two cells of a work item name different dofs at one position of its dof tile
};
const char* plan_reason_text(PlanReason r);

struct MarchPlan {
  bool ok = false;                      // false: the mesh does not tile into lattice columns
  PlanReason reason = PlanReason::ok;   // why not
  int BX = 0, BY = 0, lz = 0, nitems = 0, npatterns = 0, tile_size = 0;
  int reoriented = 0, ncomponents = 0;  // cells looked at in a rotated / reflected frame; lattice components
  double fill = 0.0;                    // cells / cell slots
  std::vector<int32_t> slot_cell;       // [nitems * lz * BX * BY] cell index or -1, slot order [layer][ly][lx]
  std::vector<uint8_t> cell_orient;     // [ncells] orientation code (orient_decode)
  std::vector<int32_t> item_base;       // [nitems] smallest dof of the item
  std::vector<int32_t> item_pattern;    // [nitems]
  std::vector<int32_t> item_layers;     // [nitems] 1 + the last non-empty layer (<= lz)
  std::vector<std::array<int32_t, 4>> item_key;   // [nitems] (lattice component, column x, column y, z segment)
  std::vector<int32_t> pat_off;         // [npatterns][tile_size] dof - base per tile position, -1 = uncovered
};

// Work items run in rounds of this many resident workgroups (2 per CU on 256 CUs) and each pays kMarchPrologue layers of
// pipeline fill (box_run_plan.h): the segment length of a plan minimises rounds * (lz + kMarchPrologue).
constexpr long kPlanResidentWorkgroups = 512;

// tdm: tensor-ordered dofmap [ncells][(P+1)^3] (the caller's cell frames).  Returns WF_OK and plan->ok = true when the
// mesh tiles into columns of BX x BY cells cut into segments of <= lz_max layers (lz_fixed > 0: of min(lz_max, lz_fixed)
// layers); plan->ok = false (still WF_OK) with plan->reason when it does not.  normalise = false requires the cells'
// local axes to agree as given (orientation code 0 everywhere).
int build_march_plan(int P, size_t ncells, const int32_t* tdm, int BX, int BY, int lz_max, int lz_fixed, bool normalise,
                     MarchPlan* plan);

// ---- consumers ----
// An item is interface iff its dof tile (base + pattern offsets) contains a ghost position (ghost[dof] != 0); the items
// of each list in ascending order.
void split_items_by_ghost(const std::vector<int32_t>& item_base, const std::vector<int32_t>& item_pattern,
                          const std::vector<int32_t>& pat_off, int tile_size, const std::vector<char>& ghost,
                          std::vector<int32_t>& interior, std::vector<int32_t>& interface);
// The dof numbering that follows a plan (wf_lattice_numbering): work items in (component, z segment, column y, column x)
// order, inside an item plane by plane, row by row; a plan that is not ok gives the first-touch numbering of the cell
// order.  Dofs no cell names keep their relative order behind the others.  new_of_old[ndofs].
void plan_numbering(const MarchPlan& plan, size_t ncells, int nd, const int32_t* tdm, int32_t ndofs, int32_t* new_of_old);

}  // namespace wf
