// Host-side plans of the point kernels (points.hip), made by point_locate.cpp without any device call.
#pragma once
#include <cstdint>
#include <vector>

namespace wf {

// The CSR of wf_sources_add: the unique dofs the sources touch, ascending; within a dof the sources ascending.
// Entry weights are (wx[i] * wy[j]) * wz[k] of the source's point, the association of wf_points_sample; entries whose
// weight is exactly zero are dropped.
struct SourceCsr {
  std::vector<int32_t> dof, off, src;
  std::vector<double> weight;
};
// dofs [nsrc][(P+1)^3] and w [nsrc][3][P+1]: the rows of each source's point
void sources_merge(int P, int nsrc, const int32_t* dofs, const double* w, SourceCsr& out);

}  // namespace wf
