// The handles of the point layer (points.hip; adjoint.hip reads the sources' CSR).
#pragma once
#include <cstdint>
#include <vector>

#include "device_array.h"

struct wf_points {
  int P = 0, nd = 0, npoints = 0;
  int64_t ndofs = 0;
  std::vector<int32_t> h_dofs;   // [npoints][nd], kept for wf_sources_create
  std::vector<double> h_w;       // [npoints][3][P+1]
  wf::DevArray<int32_t> d_dofs;
  wf::DevArray<double> d_w;
};

struct wf_sources {
  int nsrc = 0, nunique = 0, nentries = 0;
  int64_t ndofs = 0;
  wf::DevArray<int32_t> d_dof, d_off, d_src;
  wf::DevArray<double> d_weight;
  // wavelets: kind, (amplitude, frequency, delay, t_start, dt) and the table [soff[s], soff[s+1]) per source
  wf::DevArray<int32_t> d_kind, d_soff;
  wf::DevArray<double> d_par, d_samples;
};
