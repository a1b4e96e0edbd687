// Per-cell geometry of affine hexahedral cells: the host-only rule that decides whether a marching stiffness operator
// may keep one G_c per cell, and the metric decision on its result.  No HIP call.
#include <cmath>

#include "op.h"

namespace wf {
namespace {

// Per-cell geometry of hexahedral cells whose eight vertices vert(c, v) names (v = a + 2 b + 4 c', the tensor order of
// h_geom_dofmap).  The trilinear map of a cell is affine when its edge vectors along each reference axis are bitwise
// equal; J is then [x1-x0 | x2-x0 | x4-x0] everywhere and G(q) = J^-1 J^-T |det J| w_q = G_c w_i w_j w_k.
// A cell qualifies when
//  * it is affine (else reason 1) with det J != 0, finite (else reason 2);
//  * with the reference's -1/0/1 clamp on: the clamp changes neither a cmap derivative at the rule's points nor a
//    component of any G(q) (it maps |v| <= 1e-8 to 0 and v within 1e-5 of +-1 to +-1: per point that would
//    be a change per-cell G_c w_i w_j w_k cannot express; else reason 3).  Components that are exactly 0 stay 0 either way.
// Computing G_c from the edge vectors avoids the cancellation of the sum over vertices x_v dphi_v.
// Gc (may be null): [ncells][6] in cell order, components G00 G01 G02 G11 G12 G22 (the blocked layout's order).
// Returns the first cell that does not qualify (Gc is then complete only below it), -1 when all do.
template <class VertexOf>
int64_t cell_geometry(int P, size_t ncells, const double* xv, VertexOf&& vert, int use_fabs, int clamp, double* Gc,
                      int* reason)
{
  const int n = P + 1;
  std::vector<double> pts(n), wts(n);
  gll_points_weights(n, pts.data(), wts.data());
  auto clamp101 = [](double v) {   // as hex_geometry.hip
    if (std::fabs(v + 1.0) <= 1e-8 + 1e-5) v = -1.0;
    if (std::fabs(v) <= 1e-8) v = 0.0;
    if (std::fabs(v - 1.0) <= 1e-8 + 1e-5) v = 1.0;
    return v;
  };
  std::vector<double> W;   // w_i w_j w_k as the per-point geometry forms them
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) W.push_back(wts[i] * wts[j] * wts[k]);
  const double wmin = *std::min_element(W.begin(), W.end()), wmax = *std::max_element(W.begin(), W.end());
  bool cmap_clamped = false;   // the same for every cell
  if (clamp) {
    for (int k = 0; k < n; ++k)
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
          const double f0[2] = {1.0 - pts[i], pts[i]}, f1[2] = {1.0 - pts[j], pts[j]}, f2[2] = {1.0 - pts[k], pts[k]};
          const double g[2] = {-1.0, 1.0};
          for (int v = 0; v < 8; ++v) {
            const int a = v & 1, b = (v >> 1) & 1, c = (v >> 2) & 1;
            const double d[3] = {g[a] * f1[b] * f2[c], f0[a] * g[b] * f2[c], f0[a] * f1[b] * g[c]};
            for (double dv : d)
              if (clamp101(dv) != dv) cmap_clamped = true;
          }
        }
  }
  // does clamp101 leave every value |v| * W alone?  (relative slack for the rounding of the per-point form)
  constexpr double slack = 1e-6, lo1 = 1.0 - (1e-8 + 1e-5), hi1 = 1.0 + (1e-8 + 1e-5);
  auto clamp_free = [&](double v) {
    v = std::fabs(v);
    if (v == 0.0) return true;
    if (v * wmin * (1.0 - slack) <= 1e-8) return false;
    if (v * wmax * (1.0 + slack) < lo1 || v * wmin * (1.0 - slack) > hi1) return true;
    for (double w : W)
      if (v * w * (1.0 + slack) >= lo1 && v * w * (1.0 - slack) <= hi1) return false;
    return true;
  };
  *reason = 0;
  for (size_t cell = 0; cell < ncells; ++cell) {
    const double* x[8];
    for (int v = 0; v < 8; ++v) x[v] = xv + 3 * (size_t)vert(cell, v);
    double J[9];   // J[i * 3 + d]: component i of the edge along reference axis d
    for (int i = 0; i < 3; ++i) {
      const double e[3] = {x[1][i] - x[0][i], x[2][i] - x[0][i], x[4][i] - x[0][i]};
      // x1-x0 == x3-x2 == x5-x4 == x7-x6, x2-x0 == x3-x1 == x6-x4 == x7-x5, x4-x0 == x5-x1 == x6-x2 == x7-x3
      if (!(x[3][i] - x[2][i] == e[0] && x[5][i] - x[4][i] == e[0] && x[7][i] - x[6][i] == e[0] &&
            x[3][i] - x[1][i] == e[1] && x[6][i] - x[4][i] == e[1] && x[7][i] - x[5][i] == e[1] &&
            x[5][i] - x[1][i] == e[2] && x[6][i] - x[2][i] == e[2] && x[7][i] - x[3][i] == e[2]))
        return *reason = 1, (int64_t)cell;
      for (int d = 0; d < 3; ++d) J[i * 3 + d] = e[d];
    }
    double det = J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
    if (!(det != 0.0) || !std::isfinite(det)) return *reason = 2, (int64_t)cell;
    const double idet = 1.0 / det;
    double Ji[9];
    Ji[0] = (J[4] * J[8] - J[5] * J[7]) * idet;
    Ji[1] = (J[2] * J[7] - J[1] * J[8]) * idet;
    Ji[2] = (J[1] * J[5] - J[2] * J[4]) * idet;
    Ji[3] = (J[5] * J[6] - J[3] * J[8]) * idet;
    Ji[4] = (J[0] * J[8] - J[2] * J[6]) * idet;
    Ji[5] = (J[2] * J[3] - J[0] * J[5]) * idet;
    Ji[6] = (J[3] * J[7] - J[4] * J[6]) * idet;
    Ji[7] = (J[1] * J[6] - J[0] * J[7]) * idet;
    Ji[8] = (J[0] * J[4] - J[1] * J[3]) * idet;
    if (use_fabs) det = std::fabs(det);
    static const int comp[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
    for (int m = 0; m < 6; ++m) {
      const int a = comp[m][0], b = comp[m][1];
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += (Ji[a * 3 + k] * det) * Ji[b * 3 + k];
      if (!std::isfinite(s)) return *reason = 2, (int64_t)cell;
      if (clamp && (cmap_clamped || !clamp_free(s))) return *reason = 3, (int64_t)cell;
      if (Gc) Gc[cell * 6 + m] = s;
    }
  }
  return -1;
}

}  // namespace

int64_t hex_cell_geometry(int P, size_t ncells, const double* xv, const int32_t* geom_dofmap, int use_fabs, int clamp,
                          double* Gc, int* reason)
{
  return cell_geometry(P, ncells, xv, [&](size_t c, int v) { return geom_dofmap[c * 8 + v]; }, use_fabs, clamp, Gc, reason);
}

// Per-cell geometry of a box (wf_op_create_box): the rule above on the box's implicit vertex lattice.  Returns false --
// the operator keeps per-point geometry -- unless every cell qualifies.
bool box_cell_geometry(int P, int nx, int ny, int nz, const double* xv, int use_fabs, int clamp, std::vector<double>& Gc)
{
  const size_t ncells = (size_t)nx * ny * nz;
  Gc.assign(ncells * 6, 0.0);
  int reason;
  return cell_geometry(P, ncells, xv, [&](size_t c, int v) { return box_vertex(nx, ny, c, v); }, use_fabs, clamp, Gc.data(),
                       &reason) < 0;
}

int64_t first_offdiagonal_cell(const std::vector<double>& Gc)
{
  for (size_t c = 0; c < Gc.size(); c += 6)
    if (!(Gc[c + 1] == 0.0 && Gc[c + 2] == 0.0 && Gc[c + 4] == 0.0)) return (int64_t)(c / 6);
  return -1;
}

}  // namespace wf

using namespace wf;

extern "C" int wf_geometry_hex_cell(int P, int64_t ncells, int64_t nverts, const double* h_xverts,
                                    const int32_t* h_geom_dofmap, int use_fabs, int clamp, double* h_Gc, int64_t* first_bad,
                                    int* reason)
{
  if (P < 1 || P > kMaxDegree) {
    set_error("wf_geometry_hex_cell: degree must be 1..7");
    return WF_ERR_UNSUPPORTED;
  }
  WF_REQUIRE(ncells >= 0 && nverts >= 0 && first_bad && reason && (ncells == 0 || (h_xverts && h_geom_dofmap)),
             "wf_geometry_hex_cell: bad arguments");
  if (int rc = check_index_range(h_geom_dofmap, (size_t)ncells * 8, nverts, "wf_geometry_hex_cell: vertex index out of range"))
    return rc;
  *first_bad = hex_cell_geometry(P, (size_t)ncells, h_xverts, h_geom_dofmap, use_fabs, clamp, h_Gc, reason);
  return WF_OK;
}
