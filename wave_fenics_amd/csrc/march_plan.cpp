// Host-side work plan of the indexed marching kernels k_march_idx / k_march_idx_ks
// (stiffness_march_idx.hip, stiffness_march_ks.hip): the production kernels for an ARBITRARY
// dofmap.  StiffnessOperator(V, ...) of common/operators.hpp:137-201 visits its cells in dofmap
// order; cells are summed independently (operators.hpp:188-199), so the operator may regroup
// them freely -- and may look at every cell in whichever of the 48 orientations of the reference
// cube suits it, as long as dofs and geometry are relabelled together.
//
// The marching box kernel (stiffness_march.hip) owes its speed to columns of BX x BY x lz
// cells: the dof planes between the layers never leave the workgroup.  Nothing in that
// needs the lexicographic numbering -- only the ADDRESSES of the column's dofs do.  The
// plan therefore finds such columns in any conforming hexahedral mesh, whatever its cell order,
// dof numbering and local cell orientations (a DOLFINx box mesh, a gmsh multi-block mesh).
// build_march_plan is a driver over four steps:
//   1. link_cells: two cells are linked when they share the four corner dofs of a face;
//   2. place_cells: a breadth-first walk over the links gives every cell integer
//      coordinates (cx, cy, cz) and an ORIENTATION (signed permutation of its local axes) under
//      which its axes agree with the lattice.  A cell is only placed where every already placed
//      cell among its 26 lattice neighbours shares exactly the corner dofs the lattice says it
//      should (so irregular vertices -- three or five cells around an edge, O-grids -- and
//      periodic wrap-arounds cut the lattice into COMPONENTS instead of breaking the plan);
//   3. segment_length, cut_items: columns of BX x BY cells are cut into segments of <= lz layers
//      = work items;
//   4. build_tiles: per item, the dof of every position of the column's dof tile
//      [P lz + 1][P BY + 1][P BX + 1] is recorded (as an offset from the item's smallest
//      dof, -1 where no cell covers the position) and checked for conformity: all cells
//      covering a position must name the same dof.  Identical tables are stored once
//      (PATTERNS), so a regularly numbered mesh keeps its index data in L2.
// The plan reports its fill (cells per cell slot); the caller falls back to the batch kernel
// k_stiffness_generic_u when the columns are mostly empty.
#include "march_plan.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <queue>
#include <unordered_map>

#include "box_run_plan.h"
#include "wavehip.h"

namespace wf {

// ---- cell orientations ---------------------------------------------------------------
static const int kAxisPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

void orient_decode(int code, int raw_axis[3], int flip[3])
{
  for (int m = 0; m < 3; ++m) {
    raw_axis[m] = kAxisPerm[code >> 3][m];
    flip[m] = (code >> m) & 1;
  }
}

int orient_local_index(int code, int n, int i, int j, int k)
{
  int ra[3], fl[3];
  orient_decode(code, ra, fl);
  const int l[3] = {i, j, k};
  int r[3] = {0, 0, 0};
  for (int m = 0; m < 3; ++m) r[ra[m]] = fl[m] ? n - 1 - l[m] : l[m];
  return r[0] + n * (r[1] + n * r[2]);
}

int orient_sign(int code)
{
  static const int perm_sign[6] = {1, -1, -1, 1, 1, -1};
  int s = perm_sign[code >> 3];
  for (int m = 0; m < 3; ++m)
    if ((code >> m) & 1) s = -s;
  return s;
}

std::vector<int32_t> orient_node_map(int code, int n)
{
  std::vector<int32_t> m((size_t)n * n * n);
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) m[i + n * (j + n * k)] = orient_local_index(code, n, i, j, k);
  return m;
}

const std::vector<int32_t>& OrientMaps::operator()(int code)
{
  auto& m = maps[code];
  if (m.empty()) m = orient_node_map(code, n);
  return m;
}

// corner q (bits = lattice-frame position) of a cell under orientation `code`: index 0..7 of the raw corner
static inline int oriented_corner(int code, int q) { return orient_local_index(code, 2, q & 1, (q >> 1) & 1, (q >> 2) & 1); }

void orient_vertices(int code, const int32_t raw[8], int32_t out[8])
{
  for (int v = 0; v < 8; ++v) out[v] = raw[oriented_corner(code, v)];
}

void orient_tensor(int code, const int (&at)[3][3], const double* g, double* out)
{
  int ra[3], fl[3];
  orient_decode(code, ra, fl);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double v = g[at[ra[a]][ra[b]]];
      out[at[a][b]] = (fl[a] ^ fl[b]) ? -v : v;
    }
}

const char* plan_reason_text(PlanReason r)
{
  switch (r) {
    case PlanReason::ok: return "ok";
    case PlanReason::nonmanifold_face: return "three cells share one face";
    case PlanReason::position_taken: return "two cells at one lattice position";
    case PlanReason::nonconforming_tile: return "the cells of a column name different dofs at one position";
  }
  return "?";
}

namespace {

uint64_t fnv(const void* data, size_t bytes, uint64_t h = 1469598103934665603ull)
{
  const unsigned char* p = static_cast<const unsigned char*>(data);
  for (size_t i = 0; i < bytes; ++i) {
    h ^= p[i];
    h *= 1099511628211ull;
  }
  return h;
}

using Key4 = std::array<int32_t, 4>;
using Pos = std::array<int32_t, 3>;
struct KeyHash {
  size_t operator()(const Key4& k) const { return (size_t)fnv(k.data(), sizeof(k)); }
};
using CellAt = std::unordered_map<Key4, int32_t, KeyHash>;   // (component, x, y, z) -> cell

// the two lattice axes in the face across axis a, ascending
inline void face_axes(int a, int* b, int* c)
{
  *b = (a + 1) % 3 < (a + 2) % 3 ? (a + 1) % 3 : (a + 2) % 3;
  *c = 3 - a - *b;
}

// ---- step 1: cell corners and face links ------------------------------------------------
struct CellLinks {
  std::vector<std::array<int32_t, 8>> corner;   // corner dofs of every cell in its own frame, corner q = a + 2b + 4c
  std::vector<std::array<int32_t, 6>> nb;       // nb[c][raw face = 2 * raw axis + side] = the cell across it, or -1
  std::vector<int32_t> key, by_key;             // smallest dof of every cell; the cells ordered by it (stable)
};

struct FaceRec {
  std::array<int32_t, 4> key;   // sorted corner dofs
  int32_t cell;
  int8_t face;                  // 2 * raw axis + side
  bool operator<(const FaceRec& o) const { return key < o.key; }
};

PlanReason link_cells(int P, size_t ncells, const int32_t* tdm, CellLinks* out)
{
  const int n = P + 1, nd = n * n * n;
  auto& corner = out->corner;
  corner.resize(ncells);
  for (size_t c = 0; c < ncells; ++c) {
    const int32_t* d = tdm + c * nd;
    for (int q = 0; q < 8; ++q)
      corner[c][q] = d[((q & 1) ? P : 0) + n * (((q >> 1) & 1 ? P : 0) + n * ((q >> 2) & 1 ? P : 0))];
  }
  out->nb.resize(ncells);
  for (auto& a : out->nb) a.fill(-1);
  std::vector<FaceRec> faces;
  faces.reserve(ncells * 6);
  for (size_t c = 0; c < ncells; ++c)
    for (int axis = 0; axis < 3; ++axis)
      for (int side = 0; side < 2; ++side) {
        FaceRec f;
        int m = 0;
        for (int q = 0; q < 8; ++q)
          if (((q >> axis) & 1) == side) f.key[m++] = corner[c][q];
        std::sort(f.key.begin(), f.key.end());
        f.cell = (int32_t)c;
        f.face = (int8_t)(2 * axis + side);
        faces.push_back(f);
      }
  std::sort(faces.begin(), faces.end());
  for (size_t a = 0; a + 1 < faces.size(); ++a) {
    const FaceRec &f = faces[a], &g = faces[a + 1];
    if (f.key != g.key || f.cell == g.cell) continue;
    if (a + 2 < faces.size() && faces[a + 2].key == f.key) return PlanReason::nonmanifold_face;
    if (f.key[0] == f.key[1] || f.key[1] == f.key[2] || f.key[2] == f.key[3]) continue;   // degenerate face
    out->nb[f.cell][f.face] = g.cell;
    out->nb[g.cell][g.face] = f.cell;
  }
  out->key.resize(ncells);
  out->by_key.resize(ncells);
  for (size_t c = 0; c < ncells; ++c) {
    out->key[c] = *std::min_element(tdm + c * nd, tdm + (c + 1) * nd);
    out->by_key[c] = (int32_t)c;
  }
  std::stable_sort(out->by_key.begin(), out->by_key.end(), [&](int32_t a, int32_t b) { return out->key[a] < out->key[b]; });
  return PlanReason::ok;
}

// ---- step 2: lattice placement -------------------------------------------------------------
struct Placement {
  std::vector<int32_t> comp;     // [ncells] lattice component
  std::vector<Pos> xyz;          // [ncells] integer coordinates in the component
  std::vector<uint8_t> orient;   // [ncells] orientation code under which the cell's axes agree with the lattice
  std::vector<Pos> cmin;         // [components] smallest coordinate per axis
  // coordinates counted from the component's minimum
  Pos rel(size_t c) const
  {
    const Pos& lo = cmin[comp[c]];
    return {xyz[c][0] - lo[0], xyz[c][1] - lo[1], xyz[c][2] - lo[2]};
  }
};

// orientation of a cell with corner dofs `corner` such that its lattice-frame face (axis a, side 1 - s) carries, corner
// by corner, the dofs `want[4]` (in-face positions (beta, gamma) over the other two lattice axes, beta fastest);
// -1 if there is none
int orientation_from_face(const std::array<int32_t, 8>& corner, int a, int s, const int32_t want[4])
{
  int r[4];
  for (int m = 0; m < 4; ++m) {
    r[m] = -1;
    for (int q = 0; q < 8; ++q)
      if (corner[q] == want[m]) {
        if (r[m] >= 0) return -1;   // a dof twice among the corners (periodic cell one cell wide)
        r[m] = q;
      }
    if (r[m] < 0) return -1;
  }
  int b, c;
  face_axes(a, &b, &c);
  const int db = r[1] ^ r[0], dc = r[2] ^ r[0];
  if ((db != 1 && db != 2 && db != 4) || (dc != 1 && dc != 2 && dc != 4) || db == dc || (r[3] ^ r[0]) != (db | dc)) return -1;
  const int rb = db == 1 ? 0 : db == 2 ? 1 : 2, rc = dc == 1 ? 0 : dc == 2 ? 1 : 2, ra = 3 - rb - rc;
  int raw_axis[3], flip[3];
  raw_axis[a] = ra;
  raw_axis[b] = rb;
  raw_axis[c] = rc;
  flip[b] = (r[0] >> rb) & 1;
  flip[c] = (r[0] >> rc) & 1;
  flip[a] = ((r[0] >> ra) & 1) ^ (1 - s);   // the shared face sits at lattice side 1 - s of the neighbour
  for (int pi = 0; pi < 6; ++pi)
    if (kAxisPerm[pi][0] == raw_axis[0] && kAxisPerm[pi][1] == raw_axis[1] && kAxisPerm[pi][2] == raw_axis[2])
      return 8 * pi + flip[0] + 2 * flip[1] + 4 * flip[2];
  return -1;
}

// may cell c (with orientation oc) sit at p of component ci?  Every placed cell among the 26
// lattice neighbours must share exactly the corner dofs the lattice prescribes.
bool fits(const CellLinks& links, const Placement& pl, const CellAt& at, int32_t c, int oc, int32_t ci, const Pos& p)
{
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (!dx && !dy && !dz) continue;
        auto it = at.find({ci, p[0] + dx, p[1] + dy, p[2] + dz});
        if (it == at.end()) continue;
        const int32_t o = it->second;
        const int d[3] = {dx, dy, dz};
        for (int q = 0; q < 8; ++q) {   // corners of c that lie on the side(s) facing o
          bool shared = true;
          int qo = 0;
          for (int m = 0; m < 3; ++m) {
            const int bit = (q >> m) & 1;
            if (d[m] == 1 && !bit) shared = false;
            if (d[m] == -1 && bit) shared = false;
            qo |= (d[m] == 0 ? bit : 1 - bit) << m;
          }
          if (!shared) continue;
          if (links.corner[c][oriented_corner(oc, q)] != links.corner[o][oriented_corner(pl.orient[o], qo)]) return false;
        }
      }
  return true;
}

// breadth-first from the unplaced cell with the smallest key, component by component
void place_cells(const CellLinks& links, bool normalise, Placement* pl)
{
  const size_t ncells = links.corner.size();
  pl->xyz.resize(ncells);
  pl->comp.assign(ncells, -1);
  pl->orient.assign(ncells, 0);
  CellAt at;
  at.reserve(ncells * 2);
  for (size_t s0 = 0; s0 < ncells; ++s0) {
    const int32_t seed = links.by_key[s0];
    if (pl->comp[seed] >= 0) continue;
    const int32_t ci = (int32_t)pl->cmin.size();
    Pos lo{0, 0, 0};
    std::queue<int32_t> q;
    pl->comp[seed] = ci;
    pl->xyz[seed] = {0, 0, 0};
    pl->orient[seed] = 0;
    at[{ci, 0, 0, 0}] = seed;
    q.push(seed);
    while (!q.empty()) {
      const int32_t c = q.front();
      q.pop();
      for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], pl->xyz[c][a]);
      int ra[3], fl[3];
      orient_decode(pl->orient[c], ra, fl);
      for (int a = 0; a < 3; ++a)
        for (int s = 0; s < 2; ++s) {
          // lattice face (a, s) of c is its raw face (ra[a], s ^ fl[a])
          const int32_t o = links.nb[c][2 * ra[a] + (s ^ fl[a])];
          if (o < 0 || pl->comp[o] >= 0) continue;   // placed cells were checked when they were placed
          Pos want = pl->xyz[c];
          want[a] += s ? 1 : -1;
          if (at.count({ci, want[0], want[1], want[2]})) continue;   // position taken: o starts another component later
          int b, cc;
          face_axes(a, &b, &cc);
          int32_t fd[4];   // lattice-frame corner dofs of c on the face
          for (int m = 0; m < 4; ++m)
            fd[m] = links.corner[c][oriented_corner(pl->orient[c], (s << a) | ((m & 1) << b) | ((m >> 1) << cc))];
          const int oc = orientation_from_face(links.corner[o], a, s, fd);
          if (oc < 0 || (!normalise && oc != 0)) continue;
          if (!fits(links, *pl, at, o, oc, ci, want)) continue;
          pl->comp[o] = ci;
          pl->xyz[o] = want;
          pl->orient[o] = (uint8_t)oc;
          at[{ci, want[0], want[1], want[2]}] = o;
          q.push(o);
        }
    }
    pl->cmin.push_back(lo);
  }
}

// ---- step 3: segment length, work items ----------------------------------------------------
// The lz <= lz_max that minimises rounds * (lz + kMarchPrologue), rounds of kPlanResidentWorkgroups items; of equal
// costs the larger lz.  Not box_uniform_lz (box_run_plan.h) on purpose: that rule cuts one box into equal segments of at
// least 3 layers and keeps the smaller lz of a tie; this one counts the segments of columns that start and end anywhere.
int segment_length(const Placement& pl, int BX, int BY, int lz_max)
{
  std::unordered_map<Key4, std::array<int32_t, 2>, KeyHash> cols;   // column -> z range
  for (size_t c = 0; c < pl.comp.size(); ++c) {
    const Pos r = pl.rel(c);
    const Key4 ck{pl.comp[c], r[0] / BX, r[1] / BY, 0};
    auto it = cols.find(ck);
    if (it == cols.end())
      cols.emplace(ck, std::array<int32_t, 2>{r[2], r[2]});
    else {
      it->second[0] = std::min(it->second[0], r[2]);
      it->second[1] = std::max(it->second[1], r[2]);
    }
  }
  int lz = lz_max;
  double best = 1e300;
  for (int cand = 1; cand <= lz_max; ++cand) {
    long nitems = 0;
    for (const auto& kv : cols) nitems += kv.second[1] / cand - kv.second[0] / cand + 1;
    const double cost = (double)((nitems + kPlanResidentWorkgroups - 1) / kPlanResidentWorkgroups) * (cand + kMarchPrologue);
    if (cost <= best + 1e-9) {
      best = cost;
      lz = cand;
    }
  }
  return lz;
}

struct Items {
  std::vector<std::vector<int32_t>> cells;   // per item its cells in slot order [layer][ly][lx], -1 = missing
  std::vector<Key4> keys;                    // per item (component, column x, column y, z segment)
  std::vector<int32_t> item_min;             // per item its smallest dof
  std::vector<int32_t> order;                // launch order: the items by item_min (stable)
};

// items are numbered as the cells, taken by key, first reach them
PlanReason cut_items(const CellLinks& links, const Placement& pl, int BX, int BY, int lz, Items* out)
{
  const int CB = BX * BY, slots = lz * CB;
  std::unordered_map<Key4, int32_t, KeyHash> item_of;
  for (int32_t c : links.by_key) {
    const Pos r = pl.rel(c);
    const Key4 ik{pl.comp[c], r[0] / BX, r[1] / BY, r[2] / lz};
    auto it = item_of.find(ik);
    int32_t id;
    if (it == item_of.end()) {
      id = (int32_t)out->cells.size();
      item_of.emplace(ik, id);
      out->cells.emplace_back(slots, -1);
      out->keys.push_back(ik);
    } else
      id = it->second;
    const int slot = (r[2] % lz) * CB + (r[1] % BY) * BX + (r[0] % BX);
    if (out->cells[id][slot] >= 0) return PlanReason::position_taken;
    out->cells[id][slot] = c;
  }
  const size_t nit = out->cells.size();
  out->item_min.assign(nit, INT32_MAX);
  out->order.resize(nit);
  for (size_t b = 0; b < nit; ++b) {
    for (int32_t c : out->cells[b])
      if (c >= 0) out->item_min[b] = std::min(out->item_min[b], links.key[c]);
    out->order[b] = (int32_t)b;
  }
  std::stable_sort(out->order.begin(), out->order.end(), [&](int32_t a, int32_t b) { return out->item_min[a] < out->item_min[b]; });
  return PlanReason::ok;
}

// ---- step 4: dof tiles, conformity check, patterns ----------------------------------------
// fills the per-item arrays of the plan (plan->BX, BY, lz and cell_orient are set) in launch order
PlanReason build_tiles(int P, const int32_t* tdm, const Items& items, MarchPlan* plan)
{
  const int n = P + 1, nd = n * n * n, BX = plan->BX, BY = plan->BY, lz = plan->lz, CB = BX * BY, slots = lz * CB;
  const int TX = P * BX + 1, TY = P * BY + 1, TP = TX * TY;
  const size_t nit = items.cells.size(), tsize = (size_t)(P * lz + 1) * TP;
  OrientMaps local_map{n};
  plan->tile_size = (int)tsize;
  plan->slot_cell.assign(nit * slots, -1);
  plan->item_base.resize(nit);
  plan->item_pattern.resize(nit);
  plan->item_layers.resize(nit);
  plan->item_key.resize(nit);
  plan->pat_off.clear();
  std::unordered_map<uint64_t, std::vector<int32_t>> seen;   // tile hash -> patterns with it
  std::vector<int32_t> tile(tsize);
  int npat = 0;
  for (size_t ob = 0; ob < nit; ++ob) {
    const std::vector<int32_t>& cells = items.cells[items.order[ob]];
    std::copy(cells.begin(), cells.end(), plan->slot_cell.begin() + ob * slots);
    std::fill(tile.begin(), tile.end(), -1);
    int layers = 0;
    for (int l = 0; l < lz; ++l)
      for (int ly = 0; ly < BY; ++ly)
        for (int lx = 0; lx < BX; ++lx) {
          const int32_t c = cells[l * CB + ly * BX + lx];
          if (c < 0) continue;
          layers = l + 1;
          const int32_t* d = tdm + (size_t)c * nd;
          const std::vector<int32_t>& lm = local_map(plan->cell_orient[c]);
          for (int k = 0; k < n; ++k)
            for (int j = 0; j < n; ++j)
              for (int i = 0; i < n; ++i) {
                int32_t& slot = tile[(size_t)(P * l + k) * TP + (P * ly + j) * TX + (P * lx + i)];
                const int32_t dof = d[lm[i + n * (j + n * k)]];
                if (slot >= 0 && slot != dof) return PlanReason::nonconforming_tile;
                slot = dof;
              }
        }
    // (a dof may sit at two positions of the tile -- around an irregular edge, or on a periodic mesh
    // one column wide: its x value is read twice and its contributions reach y in two atomics)
    const int32_t base = items.item_min[items.order[ob]];
    for (auto& v : tile)
      if (v >= 0) v -= base;
    const uint64_t h = fnv(tile.data(), tsize * sizeof(int32_t));
    int32_t pid = -1;
    auto& cand = seen[h];
    for (int32_t p : cand)
      if (std::memcmp(&plan->pat_off[(size_t)p * tsize], tile.data(), tsize * sizeof(int32_t)) == 0) {
        pid = p;
        break;
      }
    if (pid < 0) {
      pid = npat++;
      cand.push_back(pid);
      plan->pat_off.insert(plan->pat_off.end(), tile.begin(), tile.end());
    }
    plan->item_base[ob] = base;
    plan->item_pattern[ob] = pid;
    plan->item_layers[ob] = layers;
    plan->item_key[ob] = items.keys[items.order[ob]];
  }
  plan->nitems = (int)nit;
  plan->npatterns = npat;
  return PlanReason::ok;
}

}  // namespace

int build_march_plan(int P, size_t ncells, const int32_t* tdm, int BX, int BY, int lz_max, int lz_fixed, bool normalise,
                     MarchPlan* plan)
{
  *plan = MarchPlan{};
  plan->BX = BX;
  plan->BY = BY;
  plan->lz = lz_max;
  plan->cell_orient.assign(ncells, 0);
  if (ncells == 0) {
    plan->ok = true;
    plan->fill = 1.0;
    return WF_OK;
  }
  CellLinks links;
  if ((plan->reason = link_cells(P, ncells, tdm, &links)) != PlanReason::ok) return WF_OK;

  Placement pl;
  place_cells(links, normalise, &pl);
  plan->ncomponents = (int)pl.cmin.size();
  plan->cell_orient = pl.orient;
  for (size_t c = 0; c < ncells; ++c)
    if (pl.orient[c] != 0) ++plan->reoriented;

  plan->lz = lz_fixed > 0 ? std::min(lz_max, lz_fixed) : segment_length(pl, BX, BY, lz_max);
  Items items;
  if ((plan->reason = cut_items(links, pl, BX, BY, plan->lz, &items)) != PlanReason::ok) return WF_OK;
  plan->fill = (double)ncells / ((double)items.cells.size() * plan->lz * BX * BY);

  if ((plan->reason = build_tiles(P, tdm, items, plan)) != PlanReason::ok) return WF_OK;
  plan->ok = true;
  return WF_OK;
}

// ---- consumers ---------------------------------------------------------------------------------
void split_items_by_ghost(const std::vector<int32_t>& item_base, const std::vector<int32_t>& item_pattern,
                          const std::vector<int32_t>& pat_off, int tile_size, const std::vector<char>& ghost,
                          std::vector<int32_t>& interior, std::vector<int32_t>& interface)
{
  const size_t tsize = (size_t)tile_size;
  for (size_t it = 0; it < item_base.size(); ++it) {
    const int32_t* off = &pat_off[(size_t)item_pattern[it] * tsize];
    bool iface = false;
    for (size_t e = 0; e < tsize; ++e)
      if (off[e] >= 0 && ghost[(size_t)item_base[it] + off[e]]) {
        iface = true;
        break;
      }
    (iface ? interface : interior).push_back((int32_t)it);
  }
}

// SURVEY section 7's "setup-time renumbering option": the rows the marching kernels read and add to become contiguous
// in memory whatever numbering the caller's space came with (a uniformly random numbering costs 2.8x in the stiffness
// apply: every access its own cache line).
void plan_numbering(const MarchPlan& plan, size_t ncells, int nd, const int32_t* tdm, int32_t ndofs, int32_t* new_of_old)
{
  std::fill(new_of_old, new_of_old + ndofs, -1);
  int32_t next = 0;
  auto touch = [&](int32_t d) {
    if (new_of_old[d] < 0) new_of_old[d] = next++;
  };
  if (plan.ok && ncells > 0) {
    std::vector<int32_t> order(plan.nitems);
    for (int i = 0; i < plan.nitems; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
      const auto &ka = plan.item_key[a], &kb = plan.item_key[b];
      if (ka[0] != kb[0]) return ka[0] < kb[0];
      if (ka[3] != kb[3]) return ka[3] < kb[3];
      if (ka[2] != kb[2]) return ka[2] < kb[2];
      return ka[1] < kb[1];
    });
    for (int32_t it : order) {
      const int32_t* pat = &plan.pat_off[(size_t)plan.item_pattern[it] * plan.tile_size];
      for (int e = 0; e < plan.tile_size; ++e)
        if (pat[e] >= 0) touch(plan.item_base[it] + pat[e]);
    }
  } else {
    for (size_t e = 0; e < ncells * nd; ++e) touch(tdm[e]);
  }
  for (int32_t d = 0; d < ndofs; ++d) touch(d);
}

}  // namespace wf
