// Walk of csrc/point_locate.cpp on the host (built beside tables.cpp with the sanitizers, tests/test_points_host.py):
// wf_points_locate on boxes 1x1x1, 2x3x2 and 4x4x4 -- uniform and graded/anisotropic, perturbed by 0, 0.1 and 0.25 of
// the local spacing, with a hole, with shuffled cells, at an offset of 1e6 -- for random interior points, every
// vertex, edge midpoint and face centre of every cell, points outside the mesh and points inside the hole.
//
// Expected cells come from three independent sources:
//   * a random interior point is the image of a known (cell, xi): that cell must come back, and that xi to 1e-9 where
//     the image is exact enough to say (meshes that are not offset);
//   * a vertex, an edge midpoint or a face centre lies in exactly the cells that name all of its vertices, so the tie
//     rule makes the expected cell the smallest such index (combinatorial; checked where the point is exact in double:
//     vertices always, midpoints and centres on meshes that are not offset);
//   * a brute-force search over ALL cells with Newton in long double, lowest accepting index: every point, -1 included.
// The residual |x(xi) - p| is evaluated in long double against a few ulp of the cell's coordinate magnitude,
//   32 eps diam + 4 eps |x|max
// (eight products summed per coordinate in the cell's frame; one rounding each for the vertex and the point when they
// are moved into that frame), for every probe the clamp cannot have moved: the random interior points and the cell
// centres.  The probes on vertices, edges and faces may be accepted up to tol/2 outside [0, 1] and clamped, which moves
// x by at most tol/2 |dx/dxi_d| <= tol/2 diam per coordinate: they, and only they, get 1.5 tol diam on top.  The worst
// ratio of each group is printed and must not exceed 1.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "wavehip.h"

namespace {

typedef long double LD;
constexpr double kTol = 1e-10;
constexpr double kEps = 2.220446049250313e-16;
int g_failures = 0, g_checks = 0;
double g_worst_interior = 0.0, g_worst_boundary = 0.0;   // residual in units of its bound, per group of probes

void expect(bool ok, const std::string& what)
{
  ++g_checks;
  if (!ok) {
    ++g_failures;
    if (g_failures <= 40) std::printf("FAIL %s\n", what.c_str());
  }
}

struct Mesh {
  std::vector<double> x;
  std::vector<int32_t> cells;
  int64_t nverts() const { return (int64_t)x.size() / 3; }
  int64_t ncells() const { return (int64_t)cells.size() / 8; }
};

Mesh make_box(const int n[3], const double lo[3], const double hi[3], double grade, double perturb, unsigned seed)
{
  Mesh m;
  std::vector<double> ax[3];
  for (int d = 0; d < 3; ++d)
    for (int i = 0; i <= n[d]; ++i) ax[d].push_back(i == n[d] ? hi[d] : lo[d] + (hi[d] - lo[d]) * std::pow((double)i / n[d], grade));
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  auto spacing = [&](int d, int i) { return std::min(ax[d][i] - ax[d][i - 1], ax[d][i + 1] - ax[d][i]); };
  for (int c = 0; c <= n[2]; ++c)
    for (int b = 0; b <= n[1]; ++b)
      for (int a = 0; a <= n[0]; ++a) {
        double p[3] = {ax[0][a], ax[1][b], ax[2][c]};
        const bool interior = a > 0 && a < n[0] && b > 0 && b < n[1] && c > 0 && c < n[2];
        if (interior && perturb > 0.0) {
          p[0] += perturb * spacing(0, a) * U(rng);
          p[1] += perturb * spacing(1, b) * U(rng);
          p[2] += perturb * spacing(2, c) * U(rng);
        }
        m.x.insert(m.x.end(), p, p + 3);
      }
  for (int cz = 0; cz < n[2]; ++cz)
    for (int cy = 0; cy < n[1]; ++cy)
      for (int cx = 0; cx < n[0]; ++cx)
        for (int v = 0; v < 8; ++v)
          m.cells.push_back((cx + (v & 1)) + (n[0] + 1) * ((cy + ((v >> 1) & 1)) + (n[1] + 1) * (cz + (v >> 2))));
  return m;
}

template <class T>
void map_point(const Mesh& m, int64_t c, const T xi[3], T out[3])
{
  for (int d = 0; d < 3; ++d) out[d] = 0;
  for (int v = 0; v < 8; ++v) {
    const T N = ((v & 1) ? xi[0] : 1 - xi[0]) * ((v & 2) ? xi[1] : 1 - xi[1]) * ((v & 4) ? xi[2] : 1 - xi[2]);
    for (int d = 0; d < 3; ++d) out[d] += N * (T)m.x[3 * (size_t)m.cells[8 * c + v] + d];
  }
}

// long double Newton in one cell: accepted?  In the frame of the cell's vertex 0 (differences of doubles are exact in
// long double), so that the iteration converges to long double precision on a mesh far from the origin too.
bool brute_cell(const Mesh& full, int64_t cell, const double p0[3])
{
  LD p[3];
  for (int d = 0; d < 3; ++d) p[d] = (LD)p0[d] - (LD)full.x[3 * (size_t)full.cells[8 * cell] + d];
  if (!std::isfinite((double)p[0]) || !std::isfinite((double)p[1]) || !std::isfinite((double)p[2])) return false;
  LD y[8][3];
  for (int v = 0; v < 8; ++v)
    for (int d = 0; d < 3; ++d) y[v][d] = (LD)full.x[3 * (size_t)full.cells[8 * cell + v] + d] - (LD)full.x[3 * (size_t)full.cells[8 * cell] + d];
  LD xi[3] = {0.5L, 0.5L, 0.5L};
  bool conv = false;
  for (int it = 0; it < 50 && !conv; ++it) {
    LD x[3] = {0, 0, 0}, J[3][3] = {{0}};
    for (int v = 0; v < 8; ++v) {
      const LD f[3] = {(v & 1) ? xi[0] : 1 - xi[0], (v & 2) ? xi[1] : 1 - xi[1], (v & 4) ? xi[2] : 1 - xi[2]};
      const LD s[3] = {(v & 1) ? 1.0L : -1.0L, (v & 2) ? 1.0L : -1.0L, (v & 4) ? 1.0L : -1.0L};
      for (int d = 0; d < 3; ++d) {
        const LD xv = y[v][d];
        x[d] += f[0] * f[1] * f[2] * xv;
        J[d][0] += s[0] * f[1] * f[2] * xv, J[d][1] += f[0] * s[1] * f[2] * xv, J[d][2] += f[0] * f[1] * s[2] * xv;
      }
    }
    const LD r[3] = {x[0] - p[0], x[1] - p[1], x[2] - p[2]};
    const LD det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0])
                   + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
    if (det == 0 || !std::isfinite((double)det)) return false;
    LD dx[3];
    for (int k = 0; k < 3; ++k) {   // Cramer: column k replaced by r
      LD A[3][3];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = j == k ? r[i] : J[i][j];
      dx[k] = (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0])
               + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0])) / det;
      xi[k] -= dx[k];
    }
    LD far = 0, step = 0;
    for (int k = 0; k < 3; ++k) far = std::max(far, std::fabs(xi[k] - 0.5L)), step = std::max(step, std::fabs(dx[k]));
    if (!(far <= 8.0L)) return false;
    conv = step <= 1e-17L;
  }
  if (!conv) return false;
  for (int k = 0; k < 3; ++k)
    if (!(std::fabs(2 * xi[k] - 1) <= 1 + (LD)kTol)) return false;
  return true;
}

int64_t brute(const Mesh& m, const double p[3])
{
  for (int64_t c = 0; c < m.ncells(); ++c)
    if (brute_cell(m, c, p)) return c;
  return -1;
}

// smallest cell that names every one of the given vertices
int64_t lowest_cell_with(const Mesh& m, const std::vector<int32_t>& verts)
{
  for (int64_t c = 0; c < m.ncells(); ++c) {
    bool all = true;
    for (int32_t v : verts) all = all && std::find(m.cells.begin() + 8 * c, m.cells.begin() + 8 * c + 8, v) != m.cells.begin() + 8 * c + 8;
    if (all) return c;
  }
  return -1;
}

struct Probe {
  double p[3];
  int64_t expect_cell;   // -2: no independent expectation
  double xi[3];
  bool has_xi;
  bool boundary;   // on a vertex, edge or face of its cell: the clamp may have moved xi
};

void walk(const char* name, const Mesh& m, bool exact_midpoints, const std::vector<Probe>& extra, unsigned seed)
{
  std::vector<Probe> probes = extra;
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.02, 0.98);
  for (int64_t c = 0; c < m.ncells(); ++c) {
    for (int r = 0; r < 3; ++r) {   // random interior points of a known cell
      Probe q{};
      q.xi[0] = U(rng), q.xi[1] = U(rng), q.xi[2] = U(rng);
      map_point<double>(m, c, q.xi, q.p);
      q.expect_cell = c, q.has_xi = exact_midpoints;   // at 1e6 the image of xi is rounded by more than xi resolves
      probes.push_back(q);
    }
    // the 27 points of the cell with every xi in {0, 1/2, 1}: vertices (8), edge midpoints (12), face centres (6), centre
    for (int t = 0; t < 27; ++t) {
      const int s[3] = {t % 3, (t / 3) % 3, t / 9};
      Probe q{};
      for (int d = 0; d < 3; ++d) q.xi[d] = 0.5 * s[d];
      map_point<double>(m, c, q.xi, q.p);
      std::vector<int32_t> verts;
      for (int v = 0; v < 8; ++v) {
        bool on = true;
        for (int d = 0; d < 3; ++d) on = on && (s[d] == 1 || ((v >> d) & 1) == s[d] / 2);
        if (on) verts.push_back(m.cells[8 * c + v]);
      }
      const bool vertex = verts.size() == 1;
      if (vertex)
        for (int d = 0; d < 3; ++d) q.p[d] = m.x[3 * (size_t)verts[0] + d];   // the vertex itself, bit for bit
      q.expect_cell = (vertex || exact_midpoints) ? lowest_cell_with(m, verts) : -2;
      q.has_xi = false;
      q.boundary = t != 13;   // all but the cell centre
      probes.push_back(q);
    }
  }
  const int64_t np = (int64_t)probes.size();
  std::vector<double> xyz((size_t)np * 3), ref((size_t)np * 3);
  std::vector<int32_t> cell((size_t)np);
  for (int64_t i = 0; i < np; ++i) std::copy(probes[i].p, probes[i].p + 3, xyz.begin() + 3 * i);
  const int rc = wf_points_locate(m.nverts(), m.x.data(), m.ncells(), m.cells.data(), np, xyz.data(), kTol, cell.data(), ref.data());
  expect(rc == 0, std::string(name) + ": wf_points_locate returned " + std::to_string(rc));
  int found = 0, missing = 0;
  for (int64_t i = 0; i < np && rc == 0; ++i) {
    const Probe& q = probes[i];
    const std::string at = std::string(name) + " point " + std::to_string(i);
    const int64_t b = brute(m, q.p);
    expect(cell[i] == b, at + ": cell " + std::to_string(cell[i]) + ", brute force " + std::to_string(b));
    if (q.expect_cell != -2) {
      expect(b == q.expect_cell, at + ": brute force " + std::to_string(b) + ", expected " + std::to_string(q.expect_cell));
      expect(cell[i] == q.expect_cell, at + ": cell " + std::to_string(cell[i]) + ", expected " + std::to_string(q.expect_cell));
    }
    if (cell[i] < 0) {
      ++missing;
      continue;
    }
    ++found;
    const int64_t c = cell[i];
    bool in01 = true;
    for (int d = 0; d < 3; ++d) in01 = in01 && ref[3 * i + d] >= 0.0 && ref[3 * i + d] <= 1.0;
    expect(in01, at + ": xi outside [0, 1]");
    LD xi[3] = {ref[3 * i], ref[3 * i + 1], ref[3 * i + 2]}, x[3], res = 0, diam = 0, amax = 0;
    map_point<LD>(m, c, xi, x);
    for (int d = 0; d < 3; ++d) res = std::max(res, std::fabs(x[d] - (LD)q.p[d]));
    for (int v = 0; v < 8; ++v)
      for (int u = 0; u < 8; ++u) {
        LD s = 0;
        for (int d = 0; d < 3; ++d) {
          const LD a = m.x[3 * (size_t)m.cells[8 * c + v] + d], bb = m.x[3 * (size_t)m.cells[8 * c + u] + d];
          s += (a - bb) * (a - bb), amax = std::max(amax, std::fabs(a));
        }
        diam = std::max(diam, std::sqrt(s));
      }
    const LD bound = (q.boundary ? 1.5L * kTol * diam : 0.0L) + 32 * kEps * diam + 4 * kEps * amax;
    double& worst = q.boundary ? g_worst_boundary : g_worst_interior;
    worst = std::max(worst, (double)(res / bound));
    expect(res <= bound, at + ": residual " + std::to_string((double)res) + " above " + std::to_string((double)bound));
    if (q.has_xi)
      for (int d = 0; d < 3; ++d)
        expect(std::fabs(ref[3 * i + d] - q.xi[d]) <= 1e-9, at + ": xi differs from the one the point was made from");
  }
  std::printf("case %s: %lld cells, %lld points, %d found, %d in no cell\n", name, (long long)m.ncells(), (long long)np, found, missing);
}

Mesh without_cells(const Mesh& m, const std::vector<int64_t>& drop)
{
  Mesh o;
  o.x = m.x;
  for (int64_t c = 0; c < m.ncells(); ++c)
    if (std::find(drop.begin(), drop.end(), c) == drop.end()) o.cells.insert(o.cells.end(), m.cells.begin() + 8 * c, m.cells.begin() + 8 * c + 8);
  return o;
}

Mesh shuffled(const Mesh& m, unsigned seed)
{
  std::vector<int64_t> order((size_t)m.ncells());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int64_t)i;
  std::mt19937_64 rng(seed);
  std::shuffle(order.begin(), order.end(), rng);
  Mesh o;
  o.x = m.x;
  for (int64_t c : order) o.cells.insert(o.cells.end(), m.cells.begin() + 8 * c, m.cells.begin() + 8 * c + 8);
  return o;
}

std::vector<Probe> outside_probes(const double lo[3], const double hi[3])
{
  std::vector<Probe> out;
  for (int d = 0; d < 3; ++d)
    for (int side = 0; side < 2; ++side)
      for (double far : {1e-6, 0.3, 50.0}) {
        Probe q{};
        for (int e = 0; e < 3; ++e) q.p[e] = lo[e] + 0.37 * (hi[e] - lo[e]);
        q.p[d] = side ? hi[d] + far * (hi[d] - lo[d]) : lo[d] - far * (hi[d] - lo[d]);
        q.expect_cell = -1;
        out.push_back(q);
      }
  Probe nan{};
  nan.p[0] = nan.p[1] = nan.p[2] = NAN;
  nan.expect_cell = -1;
  out.push_back(nan);
  return out;
}

}  // namespace

int main()
{
  const int sizes[3][3] = {{1, 1, 1}, {2, 3, 2}, {4, 4, 4}};
  const double unit_lo[3] = {0, 0, 0}, unit_hi[3] = {1, 1, 1}, ani_lo[3] = {-0.3, 0.1, 2.0}, ani_hi[3] = {1.7, 0.35, 2.9};
  const double far_lo[3] = {1e6, 1e6 + 3, -1e6}, far_hi[3] = {1e6 + 1, 1e6 + 4, -1e6 + 1};
  unsigned seed = 1;
  // every seed is drawn in a statement of its own, so that the meshes and probes do not depend on the compiler's order
  // of evaluating arguments
  auto draw = [&seed]() { return ++seed; };
  for (const auto& n : sizes)
    for (double perturb : {0.0, 0.1, 0.25}) {
      char name[128];
      {
        std::snprintf(name, sizeof name, "box %dx%dx%d perturb %.2f", n[0], n[1], n[2], perturb);
        const unsigned mesh_seed = draw();
        const unsigned probe_seed = draw();
        walk(name, make_box(n, unit_lo, unit_hi, 1.0, perturb, mesh_seed), true, outside_probes(unit_lo, unit_hi), probe_seed);
      }
      {
        std::snprintf(name, sizeof name, "graded anisotropic box %dx%dx%d perturb %.2f", n[0], n[1], n[2], perturb);
        const unsigned mesh_seed = draw();
        const unsigned probe_seed = draw();
        walk(name, make_box(n, ani_lo, ani_hi, 1.6, perturb, mesh_seed), true, outside_probes(ani_lo, ani_hi), probe_seed);
      }
      {
        std::snprintf(name, sizeof name, "shuffled box %dx%dx%d perturb %.2f", n[0], n[1], n[2], perturb);
        const unsigned mesh_seed = draw();
        const unsigned order_seed = draw();
        const unsigned probe_seed = draw();
        walk(name, shuffled(make_box(n, unit_lo, unit_hi, 1.0, perturb, mesh_seed), order_seed), true, outside_probes(unit_lo, unit_hi),
             probe_seed);
      }
      {
        std::snprintf(name, sizeof name, "box at 1e6 %dx%dx%d perturb %.2f", n[0], n[1], n[2], perturb);
        const unsigned mesh_seed = draw();
        const unsigned probe_seed = draw();
        walk(name, make_box(n, far_lo, far_hi, 1.0, perturb, mesh_seed), false, outside_probes(far_lo, far_hi), probe_seed);
      }
    }
  // a hole: the 2x2x2 cells in the middle of the 4x4x4 box, uniform and perturbed; points inside it are in no cell
  for (double perturb : {0.0, 0.25}) {
    const int n[3] = {4, 4, 4};
    const Mesh full = make_box(n, unit_lo, unit_hi, 1.0, perturb, draw());
    std::vector<int64_t> drop;
    for (int cz = 1; cz <= 2; ++cz)
      for (int cy = 1; cy <= 2; ++cy)
        for (int cx = 1; cx <= 2; ++cx) drop.push_back(cx + 4 * (cy + 4 * cz));
    std::vector<Probe> probes = outside_probes(unit_lo, unit_hi);
    std::mt19937_64 rng(draw());
    std::uniform_real_distribution<double> U(0.1, 0.9);
    for (int64_t c : drop)
      for (int r = 0; r < 4; ++r) {
        Probe q{};
        const double xi[3] = {U(rng), U(rng), U(rng)};
        map_point<double>(full, c, xi, q.p);
        q.expect_cell = -1;
        probes.push_back(q);
      }
    char name[128];
    std::snprintf(name, sizeof name, "holed box 4x4x4 perturb %.2f", perturb);
    const Mesh holed = without_cells(full, drop);
    walk(name, holed, true, probes, draw());
    std::snprintf(name, sizeof name, "holed shuffled box 4x4x4 perturb %.2f", perturb);
    const unsigned order_seed = draw();
    const unsigned probe_seed = draw();
    walk(name, shuffled(holed, order_seed), true, probes, probe_seed);
  }
  // refusals and edge cases of the calls
  {
    const int n[3] = {1, 1, 1};
    Mesh m = make_box(n, unit_lo, unit_hi, 1.0, 0.0, 1);
    double p[3] = {0.5, 0.5, 0.5}, ref[3], w[3 * 9];
    int32_t cell = 7;
    expect(wf_points_locate(m.nverts(), m.x.data(), 1, m.cells.data(), 1, p, -1.0, &cell, ref) == WF_ERR_INVALID, "negative tol refused");
    m.cells[3] = 8;
    expect(wf_points_locate(m.nverts(), m.x.data(), 1, m.cells.data(), 1, p, kTol, &cell, ref) == WF_ERR_INVALID, "vertex out of range refused");
    expect(wf_points_locate(0, nullptr, 0, nullptr, 1, p, kTol, &cell, ref) == WF_OK && cell == -1, "empty mesh: in no cell");
    expect(wf_points_weights(0, 1, p, w) == WF_ERR_UNSUPPORTED && wf_points_weights(8, 1, p, w) == WF_ERR_UNSUPPORTED, "degree 0 and 8 refused");
    for (int P = 1; P <= 7; ++P) {
      expect(wf_points_weights(P, 1, p, w) == WF_OK, "weights");
      for (int d = 0; d < 3; ++d) {
        double s = 0.0;
        for (int a = 0; a <= P; ++a) s += w[d * (P + 1) + a];
        expect(std::fabs(s - 1.0) <= (P + 1) * kEps, "a weight row sums to 1");
      }
    }
    // two sources in one cell of a P1 space sharing all 8 dofs, one of them on a node
    const int32_t dofs[16] = {4, 5, 6, 7, 0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3};
    const double pts[6] = {0.25, 0.5, 0.75, 1.0, 0.0, 1.0};
    double w2[2 * 3 * 2];
    expect(wf_points_weights(1, 2, pts, w2) == WF_OK, "weights of two points");
    int32_t nu = 0, ne = 0, dof[8], off[9], src[16];
    double wt[16];
    expect(wf_sources_merge(1, 2, dofs, w2, &nu, &ne, dof, off, src, wt) == WF_OK && nu == 8 && ne == 9, "merge: 8 dofs, 8 + 1 entries");
    bool ascending = true;
    for (int u = 1; u < nu; ++u) ascending = ascending && dof[u] > dof[u - 1];
    expect(ascending && off[0] == 0 && off[nu] == ne, "merge: dofs ascend, offsets close");
  }
  std::printf("worst residual / bound, probes the clamp cannot move %.3e\n", g_worst_interior);
  std::printf("worst residual / bound, probes on vertices, edges and faces %.3e\n", g_worst_boundary);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
