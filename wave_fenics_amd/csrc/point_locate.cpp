// Host side of the point sources and receivers (points.hip): where a physical point lies in a hexahedral mesh, the
// 1-D Lagrange weights of the degree-P field there, and the merge of several point sources into one CSR over the dofs
// they load.  No HIP header and no device call: the file builds and runs on its own beside tables.cpp
// (tests/cxx/point_locate_walk.cpp walks it under the sanitizers).
//
// wf_points_locate: the cell of a point is found by inverting the trilinear map of the cell's 8 vertices
// (vertex v = a + 2b + 4c, the order of wf_geometry_hex) with Newton's method from the cell centre.  Reference
// coordinates are those of wf_tabulate_gll and wf_geometry_hex: [0, 1]^3.  The map is evaluated on coordinates relative
// to the cell's vertex 0, so a mesh far from the origin loses nothing to cancellation.  Candidate cells come from a
// uniform bin grid over the bounding box of the mesh; every cell is listed, ascending, in each bin its (slightly
// inflated) bounding box touches, and a point takes the LOWEST cell that accepts it -- the answer does not depend on
// the bins.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "points_plan.h"
#include "wavehip.h"

namespace wf {

void set_error(const std::string& msg);                     // tables.cpp
void gll_points_weights(int n, double* pts, double* wts);   // tables.cpp

namespace {

constexpr int kNewtonMax = 20;
constexpr double kNewtonStep = 1e-14;   // converged: the last correction, in reference units
constexpr double kBoxSlack = 1e-6;      // bounding boxes grow by (tol + this) diagonals

struct CellFrame {
  double y[8][3];   // vertices relative to vertex 0
};

// x(xi) - q and its Jacobian, in the cell's frame
inline void trilinear(const CellFrame& c, const double xi[3], double x[3], double J[3][3])
{
  const double a0 = 1.0 - xi[0], a1 = xi[0], b0 = 1.0 - xi[1], b1 = xi[1], c0 = 1.0 - xi[2], c1 = xi[2];
  for (int d = 0; d < 3; ++d) {
    x[d] = 0.0;
    J[d][0] = J[d][1] = J[d][2] = 0.0;
  }
  for (int v = 0; v < 8; ++v) {
    const double fa = (v & 1) ? a1 : a0, fb = (v & 2) ? b1 : b0, fc = (v & 4) ? c1 : c0;
    const double da = (v & 1) ? 1.0 : -1.0, db = (v & 2) ? 1.0 : -1.0, dc = (v & 4) ? 1.0 : -1.0;
    const double N = fa * fb * fc, Na = da * fb * fc, Nb = fa * db * fc, Nc = fa * fb * dc;
    for (int d = 0; d < 3; ++d) {
      x[d] += N * c.y[v][d];
      J[d][0] += Na * c.y[v][d];
      J[d][1] += Nb * c.y[v][d];
      J[d][2] += Nc * c.y[v][d];
    }
  }
}

// Newton from the centre; true when it converged to a point with every coordinate in [-tol/2, 1 + tol/2]
// (max |2 xi - 1| <= 1 + tol), xi then clamped to [0, 1]
bool invert(const CellFrame& c, const double q[3], double tol, double xi[3])
{
  xi[0] = xi[1] = xi[2] = 0.5;
  bool converged = false;
  for (int it = 0; it < kNewtonMax && !converged; ++it) {
    double x[3], J[3][3];
    trilinear(c, xi, x, J);
    const double r[3] = {x[0] - q[0], x[1] - q[1], x[2] - q[2]};
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2],
                 c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
    const double inv = 1.0 / det;
    // J^{-1} r by the adjugate
    const double d0 = (c00 * r[0] + (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * r[1] + (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * r[2]) * inv;
    const double d1 = (c01 * r[0] + (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * r[1] + (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * r[2]) * inv;
    const double d2 = (c02 * r[0] + (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * r[1] + (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * r[2]) * inv;
    xi[0] -= d0, xi[1] -= d1, xi[2] -= d2;
    if (!std::isfinite(xi[0]) || !std::isfinite(xi[1]) || !std::isfinite(xi[2])) return false;
    // a point this far out is in another cell; stopping here keeps a diverging iteration from wandering
    if (std::fmax(std::fabs(xi[0] - 0.5), std::fmax(std::fabs(xi[1] - 0.5), std::fabs(xi[2] - 0.5))) > 8.0) return false;
    converged = std::fmax(std::fabs(d0), std::fmax(std::fabs(d1), std::fabs(d2))) <= kNewtonStep;
  }
  if (!converged) return false;
  for (int d = 0; d < 3; ++d)
    if (!(std::fabs(2.0 * xi[d] - 1.0) <= 1.0 + tol)) return false;
  for (int d = 0; d < 3; ++d) xi[d] = std::fmin(1.0, std::fmax(0.0, xi[d]));
  return true;
}

}  // namespace

void sources_merge(int P, int nsrc, const int32_t* dofs, const double* w, SourceCsr& out)
{
  const int n = P + 1, nd = n * n * n;
  struct Entry {
    int32_t dof, src;
    double weight;
  };
  std::vector<Entry> e;
  e.reserve((size_t)nsrc * nd);
  for (int s = 0; s < nsrc; ++s) {
    const double *wx = w + (size_t)s * 3 * n, *wy = wx + n, *wz = wy + n;
    for (int l = 0; l < nd; ++l) {
      const double wt = (wx[l % n] * wy[(l / n) % n]) * wz[l / (n * n)];
      if (wt != 0.0) e.push_back({dofs[(size_t)s * nd + l], s, wt});
    }
  }
  std::stable_sort(e.begin(), e.end(), [](const Entry& a, const Entry& b) { return a.dof != b.dof ? a.dof < b.dof : a.src < b.src; });
  out.dof.clear(), out.off.clear(), out.src.clear(), out.weight.clear();
  for (size_t i = 0; i < e.size(); ++i) {
    if (i == 0 || e[i].dof != e[i - 1].dof) {
      out.dof.push_back(e[i].dof);
      out.off.push_back((int32_t)i);
    }
    out.src.push_back(e[i].src);
    out.weight.push_back(e[i].weight);
  }
  out.off.push_back((int32_t)e.size());
}

}  // namespace wf

using namespace wf;

extern "C" {

int wf_points_locate(int64_t nverts, const double* h_xverts, int64_t ncells, const int32_t* h_cells, int64_t npoints,
                     const double* h_xyz, double tol, int32_t* h_cell, double* h_ref)
{
  if (nverts < 0 || ncells < 0 || npoints < 0 || ncells > INT32_MAX || !(tol >= 0.0) || !std::isfinite(tol)
      || (ncells > 0 && (!h_xverts || !h_cells)) || (npoints > 0 && (!h_xyz || !h_cell || !h_ref))) {
    set_error("wf_points_locate: bad argument");
    return WF_ERR_INVALID;
  }
  for (int64_t e = 0; e < ncells * 8; ++e)
    if (h_cells[e] < 0 || h_cells[e] >= nverts) {
      set_error("wf_points_locate: vertex index out of range in cell " + std::to_string(e / 8));
      return WF_ERR_INVALID;
    }
  for (int64_t p = 0; p < npoints; ++p) {
    h_cell[p] = -1;
    h_ref[3 * p] = h_ref[3 * p + 1] = h_ref[3 * p + 2] = 0.0;
  }
  if (ncells == 0 || npoints == 0) return WF_OK;

  // bounding boxes of the cells (a trilinear cell lies in the hull of its vertices), grown by the slack
  std::vector<double> blo((size_t)ncells * 3), bhi((size_t)ncells * 3);
  double mlo[3] = {INFINITY, INFINITY, INFINITY}, mhi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t c = 0; c < ncells; ++c) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, amax = 0.0;
    for (int v = 0; v < 8; ++v)
      for (int d = 0; d < 3; ++d) {
        const double x = h_xverts[3 * (size_t)h_cells[8 * c + v] + d];
        lo[d] = std::fmin(lo[d], x), hi[d] = std::fmax(hi[d], x), amax = std::fmax(amax, std::fabs(x));
      }
    const double diag = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
    const double grow = (2.0 * tol + kBoxSlack) * diag + 8.0 * 2.220446049250313e-16 * amax;
    for (int d = 0; d < 3; ++d) {
      blo[3 * c + d] = lo[d] - grow, bhi[3 * c + d] = hi[d] + grow;
      mlo[d] = std::fmin(mlo[d], blo[3 * c + d]), mhi[d] = std::fmax(mhi[d], bhi[3 * c + d]);
    }
  }
  // the bin grid: about one cell per bin
  const int nb = (int)std::min<int64_t>(64, std::max<int64_t>(1, (int64_t)std::llround(std::cbrt((double)ncells))));
  double scale[3];
  for (int d = 0; d < 3; ++d) scale[d] = mhi[d] > mlo[d] ? nb / (mhi[d] - mlo[d]) : 0.0;
  auto bin_of = [&](double x, int d) {
    const double f = std::floor((x - mlo[d]) * scale[d]);
    return (int)std::fmin((double)(nb - 1), std::fmax(0.0, f));
  };
  const size_t nbins = (size_t)nb * nb * nb;
  std::vector<int64_t> boff(nbins + 1, 0);   // two passes over the cells: count, then fill
  auto for_bins = [&](int64_t c, auto&& f) {
    const int i0 = bin_of(blo[3 * c], 0), i1 = bin_of(bhi[3 * c], 0), j0 = bin_of(blo[3 * c + 1], 1), j1 = bin_of(bhi[3 * c + 1], 1),
              k0 = bin_of(blo[3 * c + 2], 2), k1 = bin_of(bhi[3 * c + 2], 2);
    for (int k = k0; k <= k1; ++k)
      for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) f((size_t)i + (size_t)nb * (j + (size_t)nb * k));
  };
  for (int64_t c = 0; c < ncells; ++c) for_bins(c, [&](size_t b) { ++boff[b + 1]; });
  for (size_t b = 0; b < nbins; ++b) boff[b + 1] += boff[b];
  std::vector<int32_t> bcell((size_t)boff[nbins]);
  {
    std::vector<int64_t> at(boff.begin(), boff.end() - 1);
    for (int64_t c = 0; c < ncells; ++c) for_bins(c, [&](size_t b) { bcell[(size_t)at[b]++] = (int32_t)c; });   // ascending per bin
  }

  for (int64_t p = 0; p < npoints; ++p) {
    const double* x = h_xyz + 3 * p;
    bool inside = std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]);
    for (int d = 0; d < 3 && inside; ++d) inside = x[d] >= mlo[d] && x[d] <= mhi[d];
    if (!inside) continue;
    const size_t b = (size_t)bin_of(x[0], 0) + (size_t)nb * (bin_of(x[1], 1) + (size_t)nb * bin_of(x[2], 2));
    for (int64_t e = boff[b]; e < boff[b + 1]; ++e) {
      const int64_t c = bcell[(size_t)e];
      bool in_box = true;
      for (int d = 0; d < 3 && in_box; ++d) in_box = x[d] >= blo[3 * c + d] && x[d] <= bhi[3 * c + d];
      if (!in_box) continue;
      CellFrame f;
      const double* x0 = h_xverts + 3 * (size_t)h_cells[8 * c];
      for (int v = 0; v < 8; ++v)
        for (int d = 0; d < 3; ++d) f.y[v][d] = h_xverts[3 * (size_t)h_cells[8 * c + v] + d] - x0[d];
      const double q[3] = {x[0] - x0[0], x[1] - x0[1], x[2] - x0[2]};
      double xi[3];
      if (invert(f, q, tol, xi)) {
        h_cell[p] = (int32_t)c;   // candidates ascend: the first one is the lowest cell
        h_ref[3 * p] = xi[0], h_ref[3 * p + 1] = xi[1], h_ref[3 * p + 2] = xi[2];
        break;
      }
    }
  }
  return WF_OK;
}

int wf_points_weights(int P, int64_t npoints, const double* h_ref, double* h_w)
{
  if (P < 1 || P > 7) {
    set_error("wf_points_weights: degree must be 1..7");
    return WF_ERR_UNSUPPORTED;
  }
  if (npoints < 0 || (npoints > 0 && (!h_ref || !h_w))) {
    set_error("wf_points_weights: bad argument");
    return WF_ERR_INVALID;
  }
  const int n = P + 1;
  double node[8], lam[8];
  gll_points_weights(n, node, nullptr);
  for (int a = 0; a < n; ++a) {
    double prod = 1.0;
    for (int b = 0; b < n; ++b)
      if (b != a) prod *= node[a] - node[b];
    lam[a] = 1.0 / prod;
  }
  for (int64_t r = 0; r < npoints * 3; ++r) {
    const double x = h_ref[r];
    double* w = h_w + r * n;
    int hit = -1;
    for (int a = 0; a < n; ++a)
      if (x == node[a]) hit = a;
    if (hit >= 0) {
      for (int a = 0; a < n; ++a) w[a] = a == hit ? 1.0 : 0.0;
      continue;
    }
    // barycentric form: l_a(x) = (lam_a / (x - x_a)) / sum_b lam_b / (x - x_b)
    double sum = 0.0;
    int nearest = 0;
    for (int a = 0; a < n; ++a) {
      w[a] = lam[a] / (x - node[a]);
      sum += w[a];
      if (std::fabs(x - node[a]) < std::fabs(x - node[nearest])) nearest = a;
    }
    if (std::isfinite(sum)) {
      for (int a = 0; a < n; ++a) w[a] /= sum;
    } else {
      // x is so close to a node (only node 0 has neighbours that close) that the quotient overflowed: the node's row
      for (int a = 0; a < n; ++a) w[a] = a == nearest ? 1.0 : 0.0;
    }
  }
  return WF_OK;
}

int wf_sources_merge(int P, int nsrc, const int32_t* h_dofs, const double* h_w, int32_t* nunique, int32_t* nentries,
                     int32_t* h_dof, int32_t* h_off, int32_t* h_src, double* h_weight)
{
  if (P < 1 || P > 7) {
    set_error("wf_sources_merge: degree must be 1..7");
    return WF_ERR_UNSUPPORTED;
  }
  if (nsrc < 0 || (nsrc > 0 && (!h_dofs || !h_w)) || !nunique || !nentries) {
    set_error("wf_sources_merge: bad argument");
    return WF_ERR_INVALID;
  }
  SourceCsr csr;
  sources_merge(P, nsrc, h_dofs, h_w, csr);
  *nunique = (int32_t)csr.dof.size();
  *nentries = (int32_t)csr.src.size();
  if (h_dof) std::copy(csr.dof.begin(), csr.dof.end(), h_dof);
  if (h_off) std::copy(csr.off.begin(), csr.off.end(), h_off);
  if (h_src) std::copy(csr.src.begin(), csr.src.end(), h_src);
  if (h_weight) std::copy(csr.weight.begin(), csr.weight.end(), h_weight);
  return WF_OK;
}

}  // extern "C"
