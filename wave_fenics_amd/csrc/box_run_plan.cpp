// z segmentation of the box marching kernels: the uniform plan, and the run table of the owner form (box_run_plan.h).
#include "box_run_plan.h"

#include <algorithm>
#include <functional>
#include <queue>

#include "box_items.h"

namespace wf {

int box_uniform_lz(int ncols, int nz, long resident, double prologue, double* cost, long* items)
{
  double best = 1e300;
  long best_items = ncols;
  int best_lz = nz;
  for (int nseg = 1; nseg <= nz; ++nseg) {
    const int lz = (nz + nseg - 1) / nseg;
    if (lz < 3 && nseg > 1) break;
    const long it = (long)ncols * ((nz + lz - 1) / lz);
    const double c = (double)((it + resident - 1) / resident) * (lz + prologue);
    if (c < best - 1e-9) {
      best = c;
      best_lz = lz;
      best_items = it;
    }
  }
  if (cost) *cost = best;
  if (items) *items = best_items;
  return best_lz;
}

double box_runs_makespan(const std::vector<BoxRun>& runs, int xcd, int nxcd, int slots, double prologue)
{
  if (slots <= 0) return 1e300;
  std::priority_queue<double, std::vector<double>, std::greater<double>> free_at;
  for (int s = 0; s < slots; ++s) free_at.push(0.0);
  double end = 0.0;
  for (size_t e = (size_t)xcd; e < runs.size(); e += (size_t)nxcd) {
    const double t = free_at.top() + (runs[e].z1 - runs[e].z0) + prologue;
    free_at.pop();
    free_at.push(t);
    end = std::max(end, t);
  }
  return end;
}

namespace {

// Positions [a, b) of the column-major (column, layer) sequence in `shares` equal shares, cut at column ends as well.
void cut_runs(long a, long b, int nz, int shares, std::vector<BoxRun>& out)
{
  out.clear();
  long p = a;
  for (int s = 1; s <= shares; ++s) {
    const long q = a + (b - a) * s / shares;
    while (p < q) {
      const long col_end = (p / nz + 1) * nz, e = std::min(q, col_end);
      out.push_back({(int32_t)(p / nz), (int32_t)(p % nz), (int32_t)(p % nz + (e - p))});
      p = e;
    }
  }
}

// Brings `out` to exactly `count` runs by halving its longest run again and again, then orders it longest first (equal
// lengths stay in sequence order, so that neighbouring columns start together).  false: too few layers.
bool pad_and_order(std::vector<BoxRun>& out, size_t count)
{
  while (out.size() < count) {
    size_t l = 0;
    for (size_t r = 1; r < out.size(); ++r)
      if (out[r].z1 - out[r].z0 > out[l].z1 - out[l].z0) l = r;
    const int len = out[l].z1 - out[l].z0;
    if (len < 2) return false;
    const BoxRun upper = {out[l].col, out[l].z0 + (len + 1) / 2, out[l].z1};
    out[l].z1 = upper.z0;
    out.insert(out.begin() + (long)l + 1, upper);
  }
  std::stable_sort(out.begin(), out.end(), [](const BoxRun& x, const BoxRun& y) { return x.z1 - x.z0 > y.z1 - y.z0; });
  return true;
}

}  // namespace

BoxRunPlan box_run_plan(int ncols, int nz, int resident, int nxcd, double prologue, int lz_tuning)
{
  BoxRunPlan plan;
  long items = 0;
  const long slots = std::max(resident, 1);
  // the uniform cut is chosen as it always was, with the guessed prologue: the interior / interface parts run by it,
  // and an operator without a table is what it was before there were tables.  `prologue` prices both plans.
  plan.uniform_lz = box_uniform_lz(ncols, nz, slots, kMarchPrologue, nullptr, &items);
  if (lz_tuning > 0) {
    plan.uniform_lz = lz_tuning;
    items = (long)ncols * ((nz + lz_tuning - 1) / lz_tuning);
  }
  plan.uniform_cost = (double)((items + slots - 1) / slots) * (std::min(plan.uniform_lz, nz) + prologue);
  plan.cost = plan.uniform_cost;
  plan.longest = std::min(plan.uniform_lz, nz);
  // One round of cut columns is balanced already, and columns of fewer than 6 layers cannot be cut into segments of 3.
  // A single round that leaves longer columns whole does so only because two segments would need a second round.
  const bool one_round = items <= resident;
  if (lz_tuning > 0 || nxcd < 1 || resident < nxcd || (one_round && (plan.uniform_lz < nz || nz < 6))) return plan;

  // XCD k: a contiguous share of the sequence, resident / nxcd slots, and as many runs as every other XCD (entry e of
  // the table belongs to XCD e mod nxcd)
  const long total = (long)ncols * nz;
  std::vector<long> lo(nxcd + 1);
  for (int k = 0; k <= nxcd; ++k) lo[k] = total * k / nxcd;
  int slots_max = 0;
  long shares_max = total;
  for (int k = 0; k < nxcd; ++k) {
    if (lo[k + 1] <= lo[k]) return plan;
    shares_max = std::min(shares_max, lo[k + 1] - lo[k]);
    slots_max = std::max(slots_max, resident / nxcd + (k < resident % nxcd ? 1 : 0));
  }
  shares_max = std::min<long>(shares_max, 4L * slots_max);
  std::vector<std::vector<BoxRun>> xr(nxcd), best_xr;
  double best = plan.uniform_cost;
  for (int shares = 1; shares <= shares_max; ++shares) {
    size_t count = 0;
    for (int k = 0; k < nxcd; ++k) {
      cut_runs(lo[k], lo[k + 1], nz, shares, xr[k]);
      count = std::max(count, xr[k].size());
    }
    double c = 0.0;
    bool ok = true;
    for (int k = 0; k < nxcd && ok; ++k) {
      if (!(ok = pad_and_order(xr[k], count))) break;
      c = std::max(c, box_runs_makespan(xr[k], 0, 1, resident / nxcd + (k < resident % nxcd ? 1 : 0), prologue));
      ok = c < best - 1e-9;   // strictly better than the uniform plan and than every plan of fewer shares
    }
    if (!ok) continue;
    best = c;
    best_xr = xr;
  }
  if (best_xr.empty()) return plan;
  const size_t count = best_xr[0].size();
  plan.runs.resize(count * nxcd);
  plan.longest = 0;
  for (int k = 0; k < nxcd; ++k)
    for (size_t r = 0; r < count; ++r) {
      plan.runs[r * nxcd + k] = best_xr[k][r];
      plan.longest = std::max(plan.longest, best_xr[k][r].z1 - best_xr[k][r].z0);
    }
  plan.cost = best;
  return plan;
}

std::vector<int32_t> aligned_runs(int ncols, int nz, int nseg)
{
  const size_t n = (size_t)ncols * nseg, q = n / kXcds, r = n % kXcds;
  std::vector<int32_t> table(3 * n);
  size_t xcd = 0, i = 0;   // run i of XCD xcd is entry kXcds * i + xcd
  for (int s = 0; s < nseg; ++s)
    for (int col = 0; col < ncols; ++col) {
      int32_t* e = &table[3 * (kXcds * i + xcd)];
      e[0] = col, e[1] = (int32_t)((long)nz * s / nseg), e[2] = (int32_t)((long)nz * (s + 1) / nseg);
      if (++i == q + (xcd < r ? 1 : 0)) i = 0, ++xcd;
    }
  return table;
}

bool owner_cut_is_timed(int P, int tuning_lz, int ncols, int nz, int lz, long resident)
{
  return P == 4 && tuning_lz <= 0 && (long)ncols * box_segments(nz, lz, lz) > resident;
}

std::vector<int> owner_cut_candidates(int nz)
{
  const int lo = std::max(2, (nz + 11) / 12), hi = nz / 4, step = std::max(1, (hi - lo + 16) / 16);
  std::vector<int> nsegs;
  for (int nseg = lo; nseg <= hi; nseg += step) nsegs.push_back(nseg);
  return nsegs;
}

int longest_run(const std::vector<int32_t>& table)
{
  int longest = 0;
  for (size_t r = 0; r + 2 < table.size(); r += 3) longest = std::max(longest, table[r + 2] - table[r + 1]);
  return longest;
}

RunTableFault check_run_table(const int32_t* runs, int32_t nruns, int ncols, int nz)
{
  std::vector<char> seen((size_t)ncols * nz, 0);
  size_t covered = 0;
  for (int32_t r = 0; r < nruns; ++r) {
    const int32_t col = runs[3 * r], z0 = runs[3 * r + 1], z1 = runs[3 * r + 2];
    if (!(col >= 0 && col < ncols && z0 >= 0 && z0 < z1 && z1 <= nz)) return RunTableFault::outside_or_empty;
    for (int z = z0; z < z1; ++z) {
      if (seen[(size_t)col * nz + z]) return RunTableFault::covered_twice;
      seen[(size_t)col * nz + z] = 1;
    }
    covered += (size_t)(z1 - z0);
  }
  return nruns == 0 || covered == seen.size() ? RunTableFault::none : RunTableFault::not_covered;
}

}  // namespace wf
