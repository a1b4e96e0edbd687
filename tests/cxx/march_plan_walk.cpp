// Walks the lattice-column planner (csrc/march_plan.cpp) over small meshes generated from the implicit box dofmap --
// shuffled, reoriented, renumbered, holed, periodic, irregular, non-manifold, non-conforming -- and checks every plan
// against the dofmap it was made from, then the orientation helpers, the interior / interface test and the numbering.
// Built as a stand-alone program with -fsanitize=address,undefined by tests/test_march_plan_host.py: the sanitizers
// see every read and write of the planner.  Prints one "case" line per plan (counts and an FNV-1a hash of its arrays
// and of the numbering made from it), which the test compares with tests/golden/march_plan_walk.txt, and a last line
// with the number of failed checks; exit status 0 when there is none.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "march_plan.h"
#include "wavehip.h"

using namespace wf;

static int failures = 0;
static std::string current;
#define EXPECT(cond)                                                              \
  do {                                                                            \
    if (!(cond)) {                                                                \
      if (++failures <= 50) std::printf("%s: line %d: %s\n", current.c_str(), __LINE__, #cond); \
    }                                                                             \
  } while (0)

// ---- a small generator of its own: the cases must be the same wherever the program runs ----
struct Rng {
  uint64_t s;
  uint32_t next()
  {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return (uint32_t)(s >> 32);
  }
  int below(int n) { return (int)(next() % (uint32_t)n); }
  std::vector<int32_t> permutation(int n)
  {
    std::vector<int32_t> p(n);
    for (int i = 0; i < n; ++i) p[i] = i;
    for (int i = n - 1; i > 0; --i) std::swap(p[i], p[below(i + 1)]);
    return p;
  }
};

static uint64_t fnv(const void* data, size_t bytes, uint64_t h)
{
  const unsigned char* p = static_cast<const unsigned char*>(data);
  for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}
template <class T>
static uint64_t fnv(const std::vector<T>& v, uint64_t h) { return v.empty() ? h : fnv(v.data(), v.size() * sizeof(T), h); }

// ---- meshes ----
struct Mesh {
  int P = 1, n = 2, nd = 8;
  int32_t ndofs = 0;
  std::vector<int32_t> tdm;   // [ncells][nd], tensor order, x fastest
  size_t ncells() const { return tdm.size() / nd; }
};

// the nx x ny x nz box in lexicographic cell and dof order; per[a]: the dofs of the two faces across axis a are one
static Mesh box(int P, int nx, int ny, int nz, bool px = false, bool py = false, bool pz = false)
{
  Mesh m;
  m.P = P, m.n = P + 1, m.nd = m.n * m.n * m.n;
  const int NX = P * nx + 1, NY = P * ny + 1, NZ = P * nz + 1;
  m.ndofs = NX * NY * NZ;
  for (int cz = 0; cz < nz; ++cz)
    for (int cy = 0; cy < ny; ++cy)
      for (int cx = 0; cx < nx; ++cx)
        for (int k = 0; k < m.n; ++k)
          for (int j = 0; j < m.n; ++j)
            for (int i = 0; i < m.n; ++i) {
              int I = P * cx + i, J = P * cy + j, K = P * cz + k;
              if (px) I %= P * nx;
              if (py) J %= P * ny;
              if (pz) K %= P * nz;
              m.tdm.push_back(I + NX * (J + NY * K));
            }
  return m;
}

static Mesh keep_cells(const Mesh& m, const std::vector<char>& keep)
{
  Mesh o = m;
  o.tdm.clear();
  for (size_t c = 0; c < m.ncells(); ++c)
    if (keep[c]) o.tdm.insert(o.tdm.end(), m.tdm.begin() + c * m.nd, m.tdm.begin() + (c + 1) * m.nd);
  return o;
}

// the masks of tests/nonbox_helpers.py on an nx x ny x nz box
static Mesh holed(const Mesh& m, int nx, int ny, const char* mask)
{
  std::vector<char> keep(m.ncells());
  for (size_t c = 0; c < m.ncells(); ++c) {
    const int cx = (int)(c % nx), cy = (int)((c / nx) % ny), cz = (int)(c / ((size_t)nx * ny));
    const std::string k = mask;
    if (k == "L") keep[c] = !(cx >= 3 && cz >= 3);
    if (k == "cavity") keep[c] = !(cx >= 2 && cx <= 3 && cy == 2 && cz >= 2 && cz <= 4);
    if (k == "stair") keep[c] = cz >= cx;
    if (k == "pillar") keep[c] = !((cz == 2 || cz == 3) && cx != 0);
  }
  return keep_cells(m, keep);
}

static Mesh shuffled(const Mesh& m, Rng& rng)
{
  Mesh o = m;
  const std::vector<int32_t> p = rng.permutation((int)m.ncells());
  for (size_t c = 0; c < m.ncells(); ++c) std::copy_n(m.tdm.begin() + (size_t)p[c] * m.nd, m.nd, o.tdm.begin() + c * m.nd);
  return o;
}

static Mesh renumbered(const Mesh& m, Rng& rng)
{
  Mesh o = m;
  const std::vector<int32_t> p = rng.permutation(m.ndofs);
  for (auto& d : o.tdm) d = p[d];
  return o;
}

// every cell stored in a frame of its own: all 48 orientation codes occur when the mesh has 48 cells
static Mesh reoriented(const Mesh& m, Rng& rng)
{
  Mesh o = m;
  const std::vector<int32_t> who = rng.permutation((int)m.ncells());
  bool seen[48] = {};
  for (size_t c = 0; c < m.ncells(); ++c) {
    const int code = who[c] < 48 ? who[c] : rng.below(48);
    seen[code] = true;
    for (int k = 0; k < m.n; ++k)
      for (int j = 0; j < m.n; ++j)
        for (int i = 0; i < m.n; ++i)
          o.tdm[c * m.nd + orient_local_index(code, m.n, i, j, k)] = m.tdm[c * m.nd + i + m.n * (j + m.n * k)];
  }
  for (int code = 0; code < 48; ++code) EXPECT(seen[code] || m.ncells() < 48);
  return o;
}

// Three blocks of b x b x nz cells in an L around the edge x = y = b, bent until the +y face of the block at (1, 0)
// meets the +x face of the block at (0, 1): three cells around every edge of that line.
static Mesh bent_L(int P, int b, int nz)
{
  Mesh full = box(P, 2 * b, 2 * b, nz);
  const int NX = P * 2 * b + 1, NY = NX, e = P * b;
  std::vector<char> keep(full.ncells());
  for (size_t c = 0; c < full.ncells(); ++c) keep[c] = !((int)(c % (2 * b)) >= b && (int)((c / (2 * b)) % (2 * b)) >= b);
  Mesh m = keep_cells(full, keep);
  for (auto& d : m.tdm) {
    const int I = d % NX, J = (d / NX) % NY, K = d / (NX * NY);
    if (I == e && J > e) d = (e + (J - e)) + NX * (e + NY * K);   // (e, e + t) is (e + t, e)
  }
  return m;
}

// m stacks of nz cells around one line of edges: cell k has the line at its local i = j = 0, its face i = 0 is the
// face j = 0 of cell k + 1.  Three cells fit one lattice; five do not, and the lattice has to split.
static Mesh around_edge(int P, int m, int nz)
{
  Mesh o;
  o.P = P, o.n = P + 1, o.nd = o.n * o.n * o.n;
  const int NZ = P * nz + 1, spoke0 = NZ, inner0 = spoke0 + m * P * NZ;
  o.ndofs = inner0 + m * P * P * NZ;
  for (int cell = 0; cell < m; ++cell)
    for (int cz = 0; cz < nz; ++cz)
      for (int k = 0; k < o.n; ++k)
        for (int j = 0; j < o.n; ++j)
          for (int i = 0; i < o.n; ++i) {
            const int z = P * cz + k;
            int d = z;                                                               // on the line
            if (i > 0 && j == 0) d = spoke0 + (cell * P + i - 1) * NZ + z;           // the cell's own spoke
            if (i == 0 && j > 0) d = spoke0 + ((cell + 1) % m * P + j - 1) * NZ + z;   // the next cell's
            if (i > 0 && j > 0) d = inner0 + ((cell * P + i - 1) * P + j - 1) * NZ + z;
            o.tdm.push_back(d);
          }
  return o;
}

// the 2 x 1 x 1 box with a third cell on the face the two share
static Mesh three_on_a_face(int P)
{
  Mesh m = box(P, 2, 1, 1);
  std::vector<int32_t> third(m.tdm.begin() + m.nd, m.tdm.end());
  for (int l = 0; l < m.nd; ++l)
    if (l % m.n != 0) third[l] = m.ndofs++;   // off the shared face: dofs of its own
  m.tdm.insert(m.tdm.end(), third.begin(), third.end());
  return m;
}

// the 2 x 2 x 2 box at P >= 2 with one face-interior node of cell 1 named by that cell alone
static Mesh nonconforming(int P)
{
  Mesh m = box(P, 2, 2, 2);
  m.tdm[1 * m.nd + 0 + m.n * (1 + m.n * 1)] = m.ndofs++;
  return m;
}

// ---- what every plan must satisfy ----
struct Expect {
  bool one_pattern_one_component = false;
};

static void check_plan(const Mesh& m, int BX, int BY, int lz_max, int lz_fixed, bool normalise, const MarchPlan& plan, const Expect& ex)
{
  const int P = m.P, n = m.n, nd = m.nd, CB = BX * BY, lz = plan.lz;
  const size_t ncells = m.ncells();
  const int before = failures;
  EXPECT(plan.BX == BX && plan.BY == BY && plan.cell_orient.size() == ncells);
  EXPECT(lz >= 1 && lz <= lz_max);
  if (lz_fixed > 0) EXPECT(lz == std::min(lz_max, lz_fixed));
  int reoriented = 0;
  for (uint8_t o : plan.cell_orient) {
    EXPECT(o < 48);
    reoriented += o != 0;
  }
  EXPECT(plan.ok == (plan.reason == PlanReason::ok));
  if (!plan.ok) return;
  EXPECT(reoriented == plan.reoriented && (normalise || reoriented == 0));
  if (ncells == 0) {
    EXPECT(plan.nitems == 0 && plan.fill == 1.0 && plan.slot_cell.empty());
    return;
  }
  const int TX = P * BX + 1, TY = P * BY + 1, TP = TX * TY, slots = lz * CB;
  const size_t tsize = (size_t)(P * lz + 1) * TP, nit = (size_t)plan.nitems;
  EXPECT(plan.tile_size == (int)tsize);
  EXPECT(plan.slot_cell.size() == nit * slots && plan.item_base.size() == nit && plan.item_pattern.size() == nit);
  EXPECT(plan.item_layers.size() == nit && plan.item_key.size() == nit);
  EXPECT(plan.pat_off.size() == (size_t)plan.npatterns * tsize);
  EXPECT(plan.fill == (double)ncells / ((double)nit * slots));
  EXPECT(plan.ncomponents >= 1);
  if (ex.one_pattern_one_component) EXPECT(plan.ncomponents == 1 && plan.npatterns == 1 && plan.fill == 1.0);
  if (failures != before) return;   // the sizes are what the loops below rely on
  std::vector<int> times(ncells, 0);
  std::vector<char> covered(tsize);
  for (size_t it = 0; it < nit; ++it) {
    EXPECT(plan.item_pattern[it] >= 0 && plan.item_pattern[it] < plan.npatterns);
    if (plan.item_pattern[it] < 0 || plan.item_pattern[it] >= plan.npatterns) continue;
    const int32_t* off = &plan.pat_off[(size_t)plan.item_pattern[it] * tsize];
    const int32_t base = plan.item_base[it];
    std::fill(covered.begin(), covered.end(), 0);
    int layers = 0;
    int32_t smallest = INT32_MAX;
    for (int l = 0; l < lz; ++l)
      for (int ly = 0; ly < BY; ++ly)
        for (int lx = 0; lx < BX; ++lx) {
          const int32_t c = plan.slot_cell[it * slots + l * CB + ly * BX + lx];
          EXPECT(c >= -1 && c < (int32_t)ncells);
          if (c < 0 || c >= (int32_t)ncells) continue;
          ++times[c];
          layers = l + 1;
          for (int k = 0; k < n; ++k)
            for (int j = 0; j < n; ++j)
              for (int i = 0; i < n; ++i) {
                const size_t e = (size_t)(P * l + k) * TP + (P * ly + j) * TX + (P * lx + i);
                const int32_t dof = m.tdm[(size_t)c * nd + orient_local_index(plan.cell_orient[c], n, i, j, k)];
                EXPECT(off[e] >= 0 && base + off[e] == dof);
                covered[e] = 1;
                smallest = std::min(smallest, dof);
              }
        }
    EXPECT(plan.item_layers[it] == layers && layers >= 1);
    EXPECT(base == smallest);
    for (size_t e = 0; e < tsize; ++e) EXPECT(covered[e] ? off[e] >= 0 : off[e] == -1);
  }
  for (size_t c = 0; c < ncells; ++c) EXPECT(times[c] == 1);
  for (int p = 0; p < plan.npatterns; ++p)
    for (int q = 0; q < p; ++q)
      EXPECT(std::memcmp(&plan.pat_off[(size_t)p * tsize], &plan.pat_off[(size_t)q * tsize], tsize * sizeof(int32_t)) != 0);
}

// the interior / interface test on random ghost masks against a scan of the dofs of every item's cells
static void check_ghost_split(const Mesh& m, const MarchPlan& plan, Rng& rng)
{
  const int slots = plan.lz * plan.BX * plan.BY;
  for (int density : {0, 1, 40, 400}) {   // ghosts per 1000 dofs
    std::vector<char> ghost((size_t)m.ndofs, 0);
    for (auto& g : ghost) g = rng.below(1000) < density;
    std::vector<int32_t> interior, iface, want_interior, want_iface;
    split_items_by_ghost(plan.item_base, plan.item_pattern, plan.pat_off, plan.tile_size, ghost, interior, iface);
    for (int it = 0; it < plan.nitems; ++it) {
      bool any = false;
      for (int s = 0; s < slots; ++s) {
        const int32_t c = plan.slot_cell[(size_t)it * slots + s];
        for (int l = 0; c >= 0 && l < m.nd; ++l) any = any || ghost[m.tdm[(size_t)c * m.nd + l]];
      }
      (any ? want_iface : want_interior).push_back(it);
    }
    EXPECT(interior == want_interior && iface == want_iface);
  }
}

static uint64_t numbering_hash(const Mesh& m, const MarchPlan& plan)
{
  std::vector<int32_t> new_of_old((size_t)m.ndofs, -7);
  plan_numbering(plan, m.ncells(), m.nd, m.tdm.data(), m.ndofs, new_of_old.data());
  std::vector<char> hit((size_t)m.ndofs, 0);
  for (int32_t v : new_of_old) {
    EXPECT(v >= 0 && v < m.ndofs && !hit[v]);
    if (v >= 0 && v < m.ndofs) hit[v] = 1;
  }
  return fnv(new_of_old, 1469598103934665603ull);
}

static int ncases = 0;
static void run(const std::string& name, const Mesh& m, int BX, int BY, int lz_max, int lz_fixed, bool normalise, Rng& rng,
                const Expect& ex = Expect{})
{
  current = name + " P" + std::to_string(m.P) + " " + std::to_string(BX) + "x" + std::to_string(BY) + " lz_max " + std::to_string(lz_max)
            + " lz_fixed " + std::to_string(lz_fixed) + (normalise ? "" : " as given");
  MarchPlan plan;
  EXPECT(build_march_plan(m.P, m.ncells(), m.tdm.data(), BX, BY, lz_max, lz_fixed, normalise, &plan) == WF_OK);
  check_plan(m, BX, BY, lz_max, lz_fixed, normalise, plan, ex);
  uint64_t h = 1469598103934665603ull, hn = 0;
  if (plan.ok) {
    h = fnv(&plan.lz, sizeof(int), h);
    h = fnv(&plan.tile_size, sizeof(int), h);
    h = fnv(plan.slot_cell, h);
    h = fnv(plan.cell_orient, h);
    h = fnv(plan.item_base, h);
    h = fnv(plan.item_pattern, h);
    h = fnv(plan.item_layers, h);
    h = fnv(plan.item_key, h);
    h = fnv(plan.pat_off, h);
    if (m.ncells()) check_ghost_split(m, plan, rng);
  }
  // the numbering as wf_lattice_numbering makes it: from the plan of the same cross-section with 8 layers, fixed
  MarchPlan nplan;
  EXPECT(build_march_plan(m.P, m.ncells(), m.tdm.data(), BX, BY, 8, 8, true, &nplan) == WF_OK);
  hn = numbering_hash(m, nplan);
  std::printf("case %s: cells %zu ok %d reason %d items %d patterns %d lz %d components %d reoriented %d fill %.17g plan %016llx numbering %016llx\n",
              current.c_str(), m.ncells(), (int)plan.ok, (int)plan.reason, plan.ok ? plan.nitems : 0, plan.ok ? plan.npatterns : 0,
              plan.lz, plan.ncomponents, plan.reoriented, plan.ok ? plan.fill : 0.0, (unsigned long long)h, (unsigned long long)hn);
  ++ncases;
}

// ---- the orientation helpers, all 48 codes ----
static void check_orientations()
{
  current = "orientations";
  Rng rng{0x9e3779b97f4a7c15ull};
  for (int code = 0; code < 48; ++code) {
    int ra[3], fl[3];
    orient_decode(code, ra, fl);
    // R[a][r_a] = s_a: the signed permutation that takes the cell's own axes to the lattice's
    double R[3][3] = {};
    for (int a = 0; a < 3; ++a) R[a][ra[a]] = fl[a] ? -1.0 : 1.0;
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0])
                       + R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    EXPECT(orient_sign(code) == (int)det && (det == 1.0 || det == -1.0));
    for (int n : {2, 3, 5}) {
      const std::vector<int32_t> map = orient_node_map(code, n);
      OrientMaps maps{n};
      EXPECT(maps(code) == map && map.size() == (size_t)n * n * n);
      std::vector<char> hit(map.size(), 0);
      for (int k = 0; k < n; ++k)
        for (int j = 0; j < n; ++j)
          for (int i = 0; i < n; ++i) {
            const int r = orient_local_index(code, n, i, j, k);
            EXPECT(r >= 0 && r < (int)map.size() && map[i + n * (j + n * k)] == r);
            if (r >= 0 && r < (int)map.size()) {
              EXPECT(!hit[r]);
              hit[r] = 1;
            }
          }
    }
    const int32_t raw[8] = {10, 11, 12, 13, 14, 15, 16, 17};
    int32_t out[8];
    orient_vertices(code, raw, out);
    for (int v = 0; v < 8; ++v) EXPECT(out[v] == raw[orient_local_index(code, 2, v & 1, (v >> 1) & 1, (v >> 2) & 1)]);
    // G' = R G R^T, on all 9 entries and on the 6 of the upper triangle
    double G[3][3], g9[9], g6[6], o9[9], o6[6];
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b) G[a][b] = G[b][a] = (double)(rng.below(2001) - 1000) / 64.0;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) g9[kFull9[a][b]] = g6[kSym6[a][b]] = G[a][b];
    orient_tensor(code, kFull9, g9, o9);
    orient_tensor(code, kSym6, g6, o6);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        double s = 0.0;
        for (int c = 0; c < 3; ++c)
          for (int d = 0; d < 3; ++d) s += R[a][c] * G[c][d] * R[b][d];
        EXPECT(o9[kFull9[a][b]] == s && o6[kSym6[a][b]] == s);
      }
  }
}

int main()
{
  Rng rng{20250101ull};
  // cross-sections of the stiffness kernels per degree (march_idx_shape; degree 6: march_ks_shape)
  const int shapes[][3] = {{1, 8, 8}, {2, 7, 4}, {4, 5, 2}, {6, 2, 1}};
  for (const auto& s : shapes) {
    const int P = s[0], BX = s[1], BY = s[2];
    for (int lz_max : {8, 16}) {
      // lexicographic boxes: multiples of the column, and not
      Expect whole;
      whole.one_pattern_one_component = true;
      const int lzw = lz_max == 8 ? 4 : 2;
      run("box whole columns", box(P, BX, P >= 4 ? 2 * BY : BY, 2 * lzw), BX, BY, lz_max, lzw, true, rng, whole);
      const Mesh b = box(P, 7, 5, 7);
      run("box 7x5x7", b, BX, BY, lz_max, 0, true, rng);
      run("box 7x5x7 shuffled", shuffled(b, rng), BX, BY, lz_max, 0, true, rng);
      run("box 5x3x7 lz below", box(P, 5, 3, 7), BX, BY, lz_max, 3, true, rng);
      run("box 5x3x7 lz above", box(P, 5, 3, 7), BX, BY, lz_max, lz_max + 4, true, rng);
    }
    const int lz_max = P == 2 ? 16 : 8;
    const Mesh b = box(P, 7, 5, 7), small = box(P, 4, 4, 3);
    const Mesh turned = reoriented(shuffled(b, rng), rng);
    run("box 7x5x7 reoriented", turned, BX, BY, lz_max, 0, true, rng);
    run("box 7x5x7 reoriented", turned, BX, BY, lz_max, 0, false, rng);
    run("box 4x4x3 reoriented", reoriented(small, rng), BX, BY, lz_max, 0, true, rng);
    run("box 7x5x7 renumbered", renumbered(b, rng), BX, BY, lz_max, 0, true, rng);
    run("box 4x4x3 shuffled reoriented renumbered", renumbered(reoriented(shuffled(small, rng), rng), rng), BX, BY, lz_max, 0, true, rng);
    const Mesh h = box(P, 6, 5, 7);
    for (const char* mask : {"L", "cavity", "stair", "pillar"}) {
      run(std::string("holed ") + mask, holed(h, 6, 5, mask), BX, BY, lz_max, 0, true, rng);
      if (P == 2) run(std::string("holed shuffled ") + mask, shuffled(holed(h, 6, 5, mask), rng), BX, BY, lz_max, 0, true, rng);
    }
    for (int w = 1; w <= 3; ++w) {
      run("periodic x " + std::to_string(w) + " wide", box(P, w, 3, 4, true, false, false), BX, BY, lz_max, 0, true, rng);
      run("periodic z " + std::to_string(w) + " wide", box(P, 3, 2, w, false, false, true), BX, BY, lz_max, 0, true, rng);
      run("periodic xyz " + std::to_string(w) + " wide", box(P, w, w, w, true, true, true), BX, BY, lz_max, 0, true, rng);
    }
    run("periodic xy 4x3x5", box(P, 4, 3, 5, true, true, false), BX, BY, lz_max, 0, true, rng);
    run("bent L 1x1x3", bent_L(P, 1, 3), BX, BY, lz_max, 0, true, rng);
    run("bent L 2x2x3", bent_L(P, 2, 3), BX, BY, lz_max, 0, true, rng);
    run("bent L 2x2x3 shuffled reoriented", reoriented(shuffled(bent_L(P, 2, 3), rng), rng), BX, BY, lz_max, 0, true, rng);
    run("three cells around an edge", around_edge(P, 3, 3), BX, BY, lz_max, 0, true, rng);
    run("five cells around an edge", around_edge(P, 5, 3), BX, BY, lz_max, 0, true, rng);
    run("five cells around an edge shuffled", shuffled(around_edge(P, 5, 3), rng), BX, BY, lz_max, 2, true, rng);
    run("three cells on a face", three_on_a_face(P), BX, BY, lz_max, 0, true, rng);
    if (P >= 2) run("non-conforming face node", nonconforming(P), BX, BY, lz_max, 0, true, rng);
    run("no cells", keep_cells(box(P, 1, 1, 1), {0}), BX, BY, lz_max, 0, true, rng);
    run("one cell", box(P, 1, 1, 1), BX, BY, lz_max, 0, true, rng);
    run("one cell wide 1x1x7", box(P, 1, 1, 7), BX, BY, lz_max, 0, true, rng);
    run("one cell wide 7x1x1", box(P, 7, 1, 1), BX, BY, lz_max, 0, true, rng);
    run("box 6x5x7 shuffled renumbered", renumbered(shuffled(h, rng), rng), BX, BY, 8, 8, true, rng);
  }
  // more work items than workgroups in a round: the segment-length search settles above one layer
  run("segment search 16x8x5", box(1, 16, 8, 5), 1, 1, 16, 0, true, rng);
  run("segment search 16x8x9 L", holed(box(1, 16, 8, 9), 16, 8, "L"), 1, 1, 16, 0, true, rng);
  check_orientations();
  std::printf("%d cases, %d failures\n", ncases, failures);
  return failures ? 1 : 0;
}
