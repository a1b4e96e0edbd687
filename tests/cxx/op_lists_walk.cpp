// The index lists that operator set-up computes on the host and the kernels dereference unchecked, walked without a GPU:
//   work items   the interior / interface split of the box marching operators (wave_fenics_amd/csrc/box_items.{h,cpp});
//   run tables   the owner kernel's (column, z0, z1) tables (csrc/box_run_plan.{h,cpp}: aligned_runs, check_run_table),
//                and which of them creation times (owner_cut_is_timed, owner_cut_candidates);
//   unique lists the batch-unique gather/scatter lists and their packed dense form (csrc/unique_lists.{h,cpp}).
// Every expectation is written out here from the contract (include/wavehip.h, DESIGN "Interior / interface split"), not
// taken from the code under test: the columns, the z segments, the footprint of an item, the first-segment rule.
// Builds with a plain C++17 compiler and no HIP include path.  Prints one line per case and "<n> failures".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "box_items.h"
#include "box_run_plan.h"
#include "unique_lists.h"

namespace {

long failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (++failures <= 30) {                             \
        std::printf("FAILED %s: ", #cond);                \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                                \
      }                                                   \
    }                                                     \
  } while (0)

int ceil_div(int a, int b) { return (a + b - 1) / b; }

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd(uint32_t bound)   // splitmix64, reduced
{
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) % bound);
}

// ---- work items ------------------------------------------------------------------------------------------------------
struct Section {
  int P, BX, BY;
  bool owner;
};
struct Lattice {
  int NX, NY, NZ;
  long at(int I, int J, int K) const { return I + (long)NX * (J + (long)NY * K); }
  long size() const { return (long)NX * NY * NZ; }
};
struct GhostSet {
  std::string name;
  std::vector<long> pos;
  int faces[3];   // the same planes as wf_op_set_ghost_faces flags; faces[0] < 0: no such description
};

// z segments under the contract: the first has lz0s layers, every later one lz, the last one what is left
std::vector<std::pair<int, int>> segments_of(int nz, int lz, int lz0s)
{
  std::vector<std::pair<int, int>> segs = {{0, std::min(lz0s, nz)}};
  for (int z = lz0s; z < nz; z += lz) segs.push_back({z, std::min(z + lz, nz)});
  return segs;
}

struct ItemCase {
  Section sec;
  int nx, ny, nz, lz, lz0;
  Lattice lat() const { return {sec.P * nx + 1, sec.P * ny + 1, sec.P * nz + 1}; }
  wf::BoxItemShape shape() const { return {sec.P, nx, ny, nz, sec.owner, sec.BX, sec.BY, lz, lz0}; }
};

bool same(const wf::BoxItemLists& a, const wf::BoxItemLists& b)
{
  bool eq = a.lz0_split == b.lz0_split;
  for (int k = 0; k < 4; ++k) eq = eq && a.items[k] == b.items[k];
  return eq;
}

// every assertion on one split; gz: the ghosts hold the whole plane K = 0
void check_split(const ItemCase& c, const GhostSet& g, const wf::BoxItemLists& got, const char* api)
{
  const int P = c.sec.P, BX = c.sec.BX, BY = c.sec.BY;
  const Lattice L = c.lat();
  const std::string tag_s = std::string(c.sec.owner ? "owner" : "atomic") + " P" + std::to_string(P) + " " + std::to_string(BX) + "x"
                            + std::to_string(BY) + " box " + std::to_string(c.nx) + "x" + std::to_string(c.ny) + "x"
                            + std::to_string(c.nz) + " lz " + std::to_string(c.lz) + " lz0 " + std::to_string(c.lz0) + " ghosts '"
                            + g.name + "' by " + api;
  const char* tag = tag_s.c_str();
  std::vector<char> on_plane0((size_t)L.NX * L.NY, 0);
  for (long p : g.pos)
    if (p < (long)on_plane0.size()) on_plane0[p] = 1;
  const bool gz = std::count(on_plane0.begin(), on_plane0.end(), 1) == (long)on_plane0.size();
  const int lz0s = gz ? std::max(1, std::min(c.lz0 > 0 ? c.lz0 : 3, c.lz)) : c.lz;
  CHECK(got.lz0_split == lz0s, "%s: first segment of %d layers, contract %d", tag, got.lz0_split, lz0s);
  const std::vector<std::pair<int, int>> segs = segments_of(c.nz, c.lz, lz0s);
  const int nseg = (int)segs.size();
  CHECK(wf::box_segments(c.nz, c.lz, lz0s) == nseg, "%s: box_segments %d, contract %d", tag, wf::box_segments(c.nz, c.lz, lz0s), nseg);
  for (int s = 0; s < nseg; ++s) {
    const wf::BoxSegment zs = wf::box_segment(s, c.nz, c.lz, lz0s);
    CHECK(zs.z0 == segs[s].first && zs.z1 == segs[s].second, "%s: box_segment %d = [%d, %d)", tag, s, zs.z0, zs.z1);
  }
  const int nbx = c.sec.owner ? ceil_div(L.NX, P * BX) : ceil_div(c.nx, BX), nby = c.sec.owner ? ceil_div(L.NY, P * BY) : ceil_div(c.ny, BY);
  const int ncols = nbx * nby;
  const std::vector<int32_t>&interior = got.items[0], &interface = got.items[1];
  // interior + interface: every (column, segment) exactly once
  CHECK((long)interior.size() + (long)interface.size() == (long)ncols * nseg, "%s: %zu + %zu items, %d columns x %d segments", tag,
        interior.size(), interface.size(), ncols, nseg);
  std::vector<int> part((size_t)ncols * nseg, -1);
  for (int k = 0; k < 2; ++k)
    for (int32_t item : got.items[k]) {
      CHECK(item >= 0 && item < ncols * nseg, "%s: item %d of %d", tag, item, ncols * nseg);
      if (item < 0 || item >= ncols * nseg) continue;
      CHECK(part[item] < 0, "%s: item %d listed twice", tag, item);
      part[item] = k;
    }
  // the halves partition the interior alternately
  CHECK(got.items[2].size() == (interior.size() + 1) / 2 && got.items[3].size() == interior.size() / 2, "%s: halves of %zu + %zu", tag,
        got.items[2].size(), got.items[3].size());
  for (size_t q = 0; q < interior.size(); ++q) {
    const std::vector<int32_t>& half = got.items[2 + (q & 1)];
    CHECK(q / 2 < half.size() && half[q / 2] == interior[q], "%s: interior item %zu is not item %zu of half %c", tag, q, q / 2,
          "AB"[q & 1]);
  }
  // interface if and only if the footprint holds a ghost
  const int halo = c.sec.owner ? P : 0;
  for (int item = 0; item < ncols * nseg; ++item) {
    const int col = item % ncols, seg = item / ncols, Bx = col % nbx, By = col / nbx;
    const int I0 = std::max(0, P * BX * Bx - halo), I1 = std::min(L.NX - 1, P * BX * Bx + P * BX);
    const int J0 = std::max(0, P * BY * By - halo), J1 = std::min(L.NY - 1, P * BY * By + P * BY);
    const int K0 = std::max(0, P * segs[seg].first - halo), K1 = P * segs[seg].second;
    bool holds = false;
    for (long p : g.pos) {
      const int I = (int)(p % L.NX), J = (int)(p / L.NX % L.NY), K = (int)(p / ((long)L.NX * L.NY));
      if (I >= I0 && I <= I1 && J >= J0 && J <= J1 && K >= K0 && K <= K1) {
        holds = true;
        break;
      }
    }
    CHECK(part[item] == (holds ? 1 : 0), "%s: item %d (column %d,%d layers [%d, %d)) is in list %d, its footprint %s a ghost", tag, item,
          Bx, By, segs[seg].first, segs[seg].second, part[item], holds ? "holds" : "holds no");
  }
}

std::vector<char> mask_of(const Lattice& L, const std::vector<long>& pos)
{
  std::vector<char> m((size_t)L.size(), 0);   // exactly ndofs entries: AddressSanitizer watches the scan
  for (long p : pos) m[p] = 1;
  return m;
}

long walk_item_case(const ItemCase& c)
{
  const int P = c.sec.P, BX = c.sec.BX;
  const Lattice L = c.lat();
  std::vector<GhostSet> sets;
  auto plane = [&](int axis, int at) {
    std::vector<long> pos;
    for (int K = 0; K < L.NZ; ++K)
      for (int J = 0; J < L.NY; ++J)
        for (int I = 0; I < L.NX; ++I)
          if ((axis == 0 ? I : axis == 1 ? J : K) == at) pos.push_back(L.at(I, J, K));
    return pos;
  };
  auto join = [](std::vector<long> a, const std::vector<long>& b) {
    a.insert(a.end(), b.begin(), b.end());
    std::sort(a.begin(), a.end());
    a.erase(std::unique(a.begin(), a.end()), a.end());
    return a;
  };
  const std::vector<long> lower[3] = {plane(0, 0), plane(1, 0), plane(2, 0)};
  sets.push_back({"none", {}, {0, 0, 0}});
  // the lower planes alone and together
  for (int m = 1; m < 8; ++m) {
    GhostSet g{"", {}, {m & 1, (m >> 1) & 1, (m >> 2) & 1}};
    for (int a = 0; a < 3; ++a)
      if (g.faces[a]) g.pos = join(g.pos, lower[a]), g.name += a == 0 ? "x0 " : a == 1 ? "y0 " : "z0 ";
    g.name.pop_back();
    sets.push_back(g);
  }
  sets.push_back({"x1", plane(0, L.NX - 1), {-1, 0, 0}});
  sets.push_back({"y1", plane(1, L.NY - 1), {-1, 0, 0}});
  sets.push_back({"z1", plane(2, L.NZ - 1), {-1, 0, 0}});
  sets.push_back({"z0 x1", join(lower[2], plane(0, L.NX - 1)), {-1, 0, 0}});
  // single dofs (where the box has them): on a column boundary, on the boundary plane of segment 1 (no z ghost plane: it
  // starts at layer lz), P lines below a column (the owner form's halo)
  const int J1 = std::min(1, L.NY - 1), K1 = std::min(1, L.NZ - 1);
  if (P * BX < L.NX) sets.push_back({"column boundary", {L.at(P * BX, J1, K1)}, {-1, 0, 0}});
  if (c.lz < c.nz) sets.push_back({"segment boundary", {L.at(1, J1, P * c.lz)}, {-1, 0, 0}});
  if (P * BX - P < L.NX) sets.push_back({"below a column", {L.at(P * BX - P, J1, K1)}, {-1, 0, 0}});

  for (const GhostSet& g : sets) {
    const wf::BoxItemLists by_dofs = wf::split_box_items_by_ghosts(c.shape(), mask_of(L, g.pos));
    check_split(c, g, by_dofs, "dofs");
    CHECK((by_dofs.items[1].empty()) == g.pos.empty(), "%s: %zu interface items", g.name.c_str(), by_dofs.items[1].size());
    if (g.faces[0] >= 0) {
      const wf::BoxItemLists by_faces = wf::split_box_items_by_faces(c.shape(), g.faces[0], g.faces[1], g.faces[2]);
      check_split(c, g, by_faces, "faces");
      CHECK(same(by_faces, by_dofs), "P%d %dx%d %s box %dx%dx%d lz %d lz0 %d ghosts '%s': the two entry points differ", P, BX, c.sec.BY,
            c.sec.owner ? "owner" : "atomic", c.nx, c.ny, c.nz, c.lz, c.lz0, g.name.c_str());
    }
  }
  return (long)sets.size();
}

// every single dof of the lattice as the only ghost
long walk_single_dofs(const ItemCase& c)
{
  const Lattice L = c.lat();
  std::vector<char> mask((size_t)L.size(), 0);
  for (long p = 0; p < L.size(); ++p) {
    mask[p] = 1;
    check_split(c, {"dof " + std::to_string(p), {p}, {-1, 0, 0}}, wf::split_box_items_by_ghosts(c.shape(), mask), "dofs");
    mask[p] = 0;
  }
  return L.size();
}

void walk_items()
{
  const Section sections[] = {{1, 8, 8, false}, {2, 5, 5, false}, {4, 5, 2, false}, {5, 3, 1, false}, {7, 2, 1, false},
                              {4, 8, 2, true},  {6, 2, 3, true},  {7, 2, 2, true}};
  const int segmentations[3][2] = {{2, 1}, {3, 2}, {2, 0}};   // lz0 = 0: wf_tuning's default
  for (const Section& s : sections) {
    const int boxes[3][3] = {{s.BX + 1, s.BY + 1, 5}, {s.BX, s.BY, 4}, {1, 1, 1}};
    for (const auto& b : boxes)
      for (const auto& z : segmentations) {
        const ItemCase c{s, b[0], b[1], b[2], z[0], z[1]};
        const long before = failures, nsets = walk_item_case(c);
        std::printf("items %s P%d %dx%d box %dx%dx%d lz %d lz0 %d: %ld ghost sets, %ld failures\n", s.owner ? "owner" : "atomic", s.P,
                    s.BX, s.BY, b[0], b[1], b[2], z[0], z[1], nsets, failures - before);
      }
  }
  // exhaustive single-dof ghosts on the smallest boxes of P2 and of the P4 owner form: the one-cell box, and the
  // smallest box with more than one column and segment (the exact multiple)
  for (const Section& s : {sections[1], sections[5]}) {
    const int boxes[2][3] = {{1, 1, 1}, {s.BX, s.BY, 4}};
    for (const auto& b : boxes)
      for (const auto& z : segmentations) {
        const ItemCase c{s, b[0], b[1], b[2], z[0], z[1]};
        const long before = failures, ndofs = walk_single_dofs(c);
        std::printf("items %s P%d %dx%d box %dx%dx%d lz %d lz0 %d: each of %ld dofs as the only ghost, %ld failures\n",
                    s.owner ? "owner" : "atomic", s.P, s.BX, s.BY, b[0], b[1], b[2], z[0], z[1], ndofs, failures - before);
      }
  }
}

// ---- run tables ------------------------------------------------------------------------------------------------------
const char* fault_name(wf::RunTableFault f)
{
  static const char* names[4] = {"none", "outside_or_empty", "covered_twice", "not_covered"};
  return names[(int)f];
}

void walk_aligned(int ncols, int nz, int nseg)
{
  const std::vector<int32_t> t = wf::aligned_runs(ncols, nz, nseg);
  const size_t n = (size_t)ncols * nseg;
  CHECK(t.size() == 3 * n, "aligned_runs(%d, %d, %d): %zu entries", ncols, nz, nseg, t.size());
  if (t.size() != 3 * n) return;
  const wf::RunTableFault f = wf::check_run_table(t.data(), (int32_t)n, ncols, nz);
  CHECK(f == wf::RunTableFault::none, "aligned_runs(%d, %d, %d): %s", ncols, nz, nseg, fault_name(f));
  int shortest = nz, longest = 0;
  for (size_t r = 0; r < n; ++r) shortest = std::min(shortest, t[3 * r + 2] - t[3 * r + 1]), longest = std::max(longest, t[3 * r + 2] - t[3 * r + 1]);
  CHECK(longest - shortest <= 1 && shortest >= 1, "aligned_runs(%d, %d, %d): runs of %d to %d layers", ncols, nz, nseg, shortest, longest);
  CHECK(wf::longest_run(t) == longest && longest == ceil_div(nz, nseg), "aligned_runs(%d, %d, %d): longest_run %d, %d", ncols, nz, nseg,
        wf::longest_run(t), longest);
  // entry e runs on XCD e mod 8: each XCD a contiguous chunk of the segment-major sequence, the chunks in XCD order
  std::vector<int> seg_of_z0(nz + 1, -1);
  for (int s = 0; s < nseg; ++s) seg_of_z0[(long)nz * s / nseg] = s;
  long next = 0;
  for (int k = 0; k < wf::kXcds; ++k)
    for (size_t e = k; e < n; e += wf::kXcds) {
      const int s = t[3 * e + 1] >= 0 && t[3 * e + 1] <= nz ? seg_of_z0[t[3 * e + 1]] : -1;
      const long at = s < 0 ? -1 : (long)s * ncols + t[3 * e];
      CHECK(at == next, "aligned_runs(%d, %d, %d): entry %zu of XCD %d is position %ld of the sequence, not %ld", ncols, nz, nseg, e, k, at,
            next);
      ++next;
    }
}

void expect_fault(const char* what, std::vector<int32_t> t, int ncols, int nz, wf::RunTableFault want)
{
  const wf::RunTableFault got = wf::check_run_table(t.data(), (int32_t)(t.size() / 3), ncols, nz);
  CHECK(got == want, "%s: %s, expected %s", what, fault_name(got), fault_name(want));
  std::printf("runs mutant '%s': %s\n", what, fault_name(got));
}

// What creation decides before it times the owner apply (owner_cut_candidates, owner_cut_is_timed): the lists written
// out, every table a candidate stands for, and the predicate at its edges.
void walk_timed_cuts()
{
  const struct {
    int nz;
    std::vector<int> nsegs;
  } lists[] = {{7, {}},
               {8, {2}},
               {13, {2, 3}},
               {27, {3, 4, 5, 6}},
               {54, {5, 6, 7, 8, 9, 10, 11, 12, 13}},
               {200, {17, 20, 23, 26, 29, 32, 35, 38, 41, 44, 47, 50}}};
  long before = failures;
  for (const auto& l : lists) {
    const std::vector<int> got = wf::owner_cut_candidates(l.nz);
    CHECK(got == l.nsegs, "owner_cut_candidates(%d): %zu candidates from %d to %d, expected %zu from %d to %d", l.nz, got.size(),
          got.empty() ? 0 : got.front(), got.empty() ? 0 : got.back(), l.nsegs.size(), l.nsegs.empty() ? 0 : l.nsegs.front(),
          l.nsegs.empty() ? 0 : l.nsegs.back());
  }
  for (int nz = 0; nz < 8; ++nz) CHECK(wf::owner_cut_candidates(nz).empty(), "owner_cut_candidates(%d) is not empty", nz);
  std::printf("runs timed cuts, candidate lists of nz 0..8, 13, 27, 54, 200: %ld failures\n", failures - before);

  // every candidate of nz = 8 .. 256: an exact cover (walk_aligned) by runs of 4 to 12 layers, the list ascending, of
  // at most 17 entries and never empty; 33 columns leave the XCDs unequal shares at every nseg that 8 does not divide
  before = failures;
  int tables = 0;
  for (int nz = 8; nz <= 256; ++nz) {
    const std::vector<int> nsegs = wf::owner_cut_candidates(nz);
    CHECK(!nsegs.empty() && nsegs.size() <= 17, "owner_cut_candidates(%d): %zu candidates", nz, nsegs.size());
    for (size_t c = 0; c < nsegs.size(); ++c, ++tables) {
      const int ncols = 33, nseg = nsegs[c];
      CHECK(nseg >= 2 && (c == 0 || nseg > nsegs[c - 1]), "owner_cut_candidates(%d): entry %zu is %d", nz, c, nseg);
      if (nseg < 1 || nseg > nz) continue;
      walk_aligned(ncols, nz, nseg);
      const std::vector<int32_t> t = wf::aligned_runs(ncols, nz, nseg);
      for (size_t r = 0; 3 * r + 2 < t.size(); ++r) {
        const int len = t[3 * r + 2] - t[3 * r + 1];
        CHECK(len >= 4 && len <= 12, "aligned_runs(%d, %d, %d): run %zu of %d layers", ncols, nz, nseg, r, len);
      }
    }
  }
  std::printf("runs timed cuts, nz 8..256: %d tables of 4 to 12 layers a run, %ld failures\n", tables, failures - before);

  // the tuner runs: P4 only, without wf_tuning.lz, and with more items than resident workgroups.  33 columns of 27
  // layers in segments of 7: 4 segments, 132 items.
  before = failures;
  const int ncols = 33, nz = 27, lz = 7, items = 132;
  CHECK(ncols * wf::box_segments(nz, lz, lz) == items, "%d items", ncols * wf::box_segments(nz, lz, lz));
  CHECK(wf::owner_cut_is_timed(4, 0, ncols, nz, lz, items - 1), "one item above one round: not timed");
  CHECK(!wf::owner_cut_is_timed(4, 0, ncols, nz, lz, items), "items == resident: timed");
  CHECK(!wf::owner_cut_is_timed(4, 0, ncols, nz, lz, items + 1), "fewer items than resident workgroups: timed");
  CHECK(!wf::owner_cut_is_timed(4, 0, ncols, nz, lz, 768), "one round of 768: timed");
  for (int P : {1, 2, 3, 5, 6, 7}) CHECK(!wf::owner_cut_is_timed(P, 0, ncols, nz, lz, 1), "P%d: timed", P);
  for (int tuning_lz : {1, 7, 27}) CHECK(!wf::owner_cut_is_timed(4, tuning_lz, ncols, nz, lz, 1), "wf_tuning.lz = %d: timed", tuning_lz);
  // whole columns (lz = nz) are one segment each: 33 items; the count does not wrap where int would (2^16 columns of
  // 2^16 single layers against 2^31 resident)
  CHECK(wf::owner_cut_is_timed(4, 0, ncols, nz, nz, 32) && !wf::owner_cut_is_timed(4, 0, ncols, nz, nz, 33), "whole columns");
  CHECK(wf::owner_cut_is_timed(4, 0, 1 << 16, 1 << 16, 1, 1L << 31), "2^32 items against 2^31 resident: not timed");
  std::printf("runs timed cuts, predicate: %ld failures\n", failures - before);
}

void walk_runs()
{
  for (int ncols : {1, 7, 8, 9, 63}) {
    const long before = failures;
    int tables = 0;
    for (int nz = 4; nz <= 13; ++nz)
      // what tune_owner_runs asks for is nseg in [max(2, ceil(nz / 12)), nz / 4]; every cut into non-empty runs holds too
      for (int nseg = 1; nseg <= nz; ++nseg, ++tables) walk_aligned(ncols, nz, nseg);
    std::printf("runs aligned, %d columns: %d tables, %ld failures\n", ncols, tables, failures - before);
  }
  const int ncols = 7, nz = 9, nseg = 3;
  const std::vector<int32_t> valid = wf::aligned_runs(ncols, nz, nseg);
  expect_fault("valid", valid, ncols, nz, wf::RunTableFault::none);
  CHECK(wf::check_run_table(nullptr, 0, ncols, nz) == wf::RunTableFault::none, "the empty table");
  CHECK(wf::longest_run({}) == 0, "longest run of the empty table");
  std::vector<int32_t> t = valid;
  t[3 * 5 + 0] = t[0], t[3 * 5 + 1] = t[1], t[3 * 5 + 2] = t[2];   // run 5 repeats run 0
  expect_fault("a duplicated layer", t, ncols, nz, wf::RunTableFault::covered_twice);
  t = valid;
  t.resize(t.size() - 3);
  expect_fault("a gap", t, ncols, nz, wf::RunTableFault::not_covered);
  t = valid;
  t[3 * 2 + 2] -= 1;   // one layer short, nothing twice
  expect_fault("a gap inside a column", t, ncols, nz, wf::RunTableFault::not_covered);
  t = valid;
  t[3 * 4] = ncols;
  expect_fault("a column out of range", t, ncols, nz, wf::RunTableFault::outside_or_empty);
  t = valid;
  t[3 * 4] = -1;
  expect_fault("a negative column", t, ncols, nz, wf::RunTableFault::outside_or_empty);
  t = valid;
  t[3 * 3 + 2] = t[3 * 3 + 1];
  expect_fault("an empty run", t, ncols, nz, wf::RunTableFault::outside_or_empty);
  t = valid;
  for (size_t r = 0; r < t.size() / 3; ++r)
    if (t[3 * r + 2] == nz) {
      t[3 * r + 2] = nz + 1;
      break;
    }
  expect_fault("z1 > nz", t, ncols, nz, wf::RunTableFault::outside_or_empty);
}

// ---- unique lists ----------------------------------------------------------------------------------------------------
void check_lists(const char* what, const std::vector<int32_t>& dm, size_t ncells, int nd, int CB, bool dense)
{
  const long before = failures;
  wf::UniqueLists u;
  const bool ok = wf::build_unique_lists(dm.data(), ncells, nd, CB, &u);
  CHECK(ok, "%s: refused", what);
  if (!ok) return;
  const size_t nbatch = (ncells + CB - 1) / CB;
  CHECK(u.uoff.size() == nbatch + 1 && u.uoff[0] == 0 && (size_t)u.uoff[nbatch] == u.uniq.size() && u.loc.size() == ncells * nd,
        "%s: sizes", what);
  if (u.uoff.size() != nbatch + 1 || u.loc.size() != ncells * nd) return;
  int largest = 0;
  for (size_t b = 0; b < nbatch; ++b) {
    CHECK(u.uoff[b] <= u.uoff[b + 1] && (size_t)u.uoff[b + 1] <= u.uniq.size(), "%s: uoff[%zu] = %d, uoff[%zu] = %d", what, b, u.uoff[b],
          b + 1, u.uoff[b + 1]);
    if (u.uoff[b] > u.uoff[b + 1] || (size_t)u.uoff[b + 1] > u.uniq.size()) return;
    for (int32_t q = u.uoff[b] + 1; q < u.uoff[b + 1]; ++q)
      CHECK(u.uniq[q - 1] < u.uniq[q], "%s: batch %zu is not strictly ascending at %d", what, b, q - u.uoff[b]);
    const size_t c0 = b * CB, c1 = std::min(ncells, c0 + CB);
    const std::set<int32_t> distinct(dm.begin() + c0 * nd, dm.begin() + c1 * nd);
    CHECK((size_t)(u.uoff[b + 1] - u.uoff[b]) == distinct.size(), "%s: batch %zu lists %d dofs, it names %zu", what, b,
          u.uoff[b + 1] - u.uoff[b], distinct.size());
    largest = std::max(largest, (int)distinct.size());
    for (size_t e = c0 * nd; e < c1 * nd; ++e) {
      const int32_t at = u.uoff[b] + u.loc[e];
      CHECK(at < u.uoff[b + 1] && u.uniq[at] == dm[e], "%s: entry %zu (dof %d) has local index %d of %d", what, e, dm[e], (int)u.loc[e],
            u.uoff[b + 1] - u.uoff[b]);
    }
  }
  CHECK(u.largest() == largest, "%s: largest batch %d, counted %d", what, u.largest(), largest);
  if (dense) {
    // the kernels' view: lane (lg, cell slot c) of batch b holds words j < KT2 and reads the local index of dof 4 ks + lg
    // as dense_loc_of does (csrc/dense_simplex.h)
    const int KT = (nd + 3) / 4, KT2 = (KT + 1) / 2;
    const std::vector<uint32_t> locP = wf::pack_dense_loc(u.loc, ncells, nd, KT, CB);
    CHECK(locP.size() == nbatch * KT2 * 4 * CB, "%s: locP of %zu words", what, locP.size());
    if (locP.size() != nbatch * KT2 * 4 * CB) return;
    for (size_t b = 0; b < nbatch; ++b)
      for (int c = 0; c < CB; ++c)
        for (int lg = 0; lg < 4; ++lg)
          for (int ks = 0; ks < 2 * KT2; ++ks) {
            const uint32_t word = locP[((b * KT2 + (ks >> 1)) * 4 + lg) * CB + c], got = (word >> (16 * (ks & 1))) & 0xffffu;
            const size_t cell = b * CB + c;
            const int k = 4 * ks + lg;
            const uint32_t want = cell < ncells && k < nd ? u.loc[cell * nd + k] : 0u;
            CHECK(got == want, "%s: locP of batch %zu cell %d dof %d unpacks to %u, not %u", what, b, c, k, got, want);
          }
  }
  std::printf("lists %s: %zu cells of %d dofs in batches of %d, largest batch %d, %ld failures\n", what, ncells, nd, CB, u.largest(),
              failures - before);
}

std::vector<int32_t> shuffled_cells(const std::vector<int32_t>& dm, size_t ncells, int nd)
{
  std::vector<size_t> order(ncells);
  for (size_t c = 0; c < ncells; ++c) order[c] = c;
  for (size_t c = ncells; c > 1; --c) std::swap(order[c - 1], order[rnd((uint32_t)c)]);
  std::vector<int32_t> out(dm.size());
  for (size_t c = 0; c < ncells; ++c) std::copy(dm.begin() + order[c] * nd, dm.begin() + (order[c] + 1) * nd, out.begin() + c * nd);
  return out;
}

void walk_lists()
{
  // hexahedra: the box of ncells x 1 x 1 cells as a dofmap, tensor order, in lexicographic and in shuffled cell order
  for (int P : {1, 2, 3, 7}) {
    const int n = P + 1, nd = n * n * n, CB = 256 / (n * n);
    const size_t ncells = 2 * (size_t)CB + 1;
    const long NX = P * (long)ncells + 1, NY = n;
    std::vector<int32_t> dm(ncells * nd);
    for (size_t c = 0; c < ncells; ++c)
      for (int k = 0; k < n; ++k)
        for (int j = 0; j < n; ++j)
          for (int i = 0; i < n; ++i) dm[c * nd + i + n * (j + n * k)] = (int32_t)(P * (long)c + i + NX * (j + NY * k));
    check_lists(("hex P" + std::to_string(P) + " lexicographic").c_str(), dm, ncells, nd, CB, false);
    check_lists(("hex P" + std::to_string(P) + " shuffled").c_str(), shuffled_cells(dm, ncells, nd), ncells, nd, CB, false);
  }
  check_lists("hex P1 one periodic cell", {0, 1, 2, 3, 0, 1, 2, 3}, 1, 8, 64, false);
  // dense simplex batches of 64 cells: every cell nd distinct dofs of a pool it shares with the others
  for (int nd : {10, 35})
    for (size_t ncells : {1, 63, 64, 65, 129}) {
      const uint32_t pool = (uint32_t)(nd + 4 * ncells);
      std::vector<int32_t> dm(ncells * nd);
      for (size_t c = 0; c < ncells; ++c) {
        std::set<int32_t> mine;
        while ((int)mine.size() < nd) mine.insert((int32_t)rnd(pool));
        std::vector<int32_t> cell(mine.begin(), mine.end());
        for (int k = nd; k > 1; --k) std::swap(cell[k - 1], cell[rnd((uint32_t)k)]);
        std::copy(cell.begin(), cell.end(), dm.begin() + c * nd);
      }
      check_lists(("dense nd " + std::to_string(nd)).c_str(), dm, ncells, nd, 64, true);
    }
  // 16-bit local indices: 65535 unique dofs in a batch are the most one holds
  auto distinct = [](size_t ncells, int nd) {
    std::vector<int32_t> dm(ncells * nd);
    for (size_t e = 0; e < dm.size(); ++e) dm[e] = (int32_t)e;
    return dm;
  };
  wf::UniqueLists u;
  CHECK(!wf::build_unique_lists(distinct(64, 1100).data(), 64, 1100, 64, &u), "64 cells of 1100 distinct dofs accepted");
  CHECK(!wf::build_unique_lists(distinct(64, 1024).data(), 64, 1024, 64, &u), "65536 unique dofs in a batch accepted");
  CHECK(wf::build_unique_lists(distinct(51, 1285).data(), 51, 1285, 64, &u) && u.largest() == 65535, "65535 unique dofs in a batch refused");
  std::printf("lists refusals: 70400 and 65536 unique dofs in a batch refused, 65535 accepted\n");
}

}  // namespace

int main()
{
  walk_items();
  walk_runs();
  walk_timed_cuts();
  walk_lists();
  std::printf("%ld failures\n", failures);
  return failures ? 1 : 0;
}
