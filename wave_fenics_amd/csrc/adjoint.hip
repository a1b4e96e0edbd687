// The two passes the discrete adjoint of the leapfrog loop adds to the existing kernels (LinearGLLOpt.misfit_gradient):
//
// k_leapfrog_correlate: p[i] = p[i] + lam[i] * ((up[i] - 2 u[i]) + um[i]), the pointwise product of the multiplier with
//   the second difference of the state, accumulated over the steps: with a lumped (diagonal) mass the whole mass
//   sensitivity is one cell form of p at the end.  The sweep of the step kernel (sweep.h): 16-byte entries where every
//   operand allows it, the odd last dof in the same launch, the scalar form otherwise.  lam, up, u, um, p read and p
//   written = 48 B/dof; up, um and p bypass the caches (nobody reads them next), lam and u were just written or read.
// k_sources_add_values: b[dof] += scale * sum_e weight[e] * values[src[e]] over the merged CSR of a wf_sources, one
//   thread per unique dof, CSR order, no atomics: the transpose of wf_points_sample, fed from device memory.
#include "common.h"
#include "points_handles.h"
#include "sweep.h"

namespace wf {

struct CorrelateArgs {
  const double* lam;
  const double* up;
  const double* u;
  const double* um;
  double* p;
};

// evaluated as written (no contraction: the 16-byte and the scalar form give the same bits)
__device__ __forceinline__ double correlate_value(double p, double lam, double up, double u, double um)
{
#pragma clang fp contract(off)
  return p + lam * ((up - 2.0 * u) + um);
}

template <int VEC, bool NT>
__device__ __forceinline__ void correlate_entry(const CorrelateArgs& a, Lanes<VEC, NT> io, int64_t g)
{
  using L = Lanes<VEC, NT>;
  using V = typename L::V;
  const V ll = io.ld(a.lam, g), pp = io.ldnt(a.up, g), uu = io.ld(a.u, g), mm = io.ldnt(a.um, g);
  V acc = io.ldnt(a.p, g);
  for (int l = 0; l < VEC; ++l) L::at(acc, l) = correlate_value(L::at(acc, l), L::at(ll, l), L::at(pp, l), L::at(uu, l), L::at(mm, l));
  io.stnt(a.p, g, acc);
}

template <int VEC, bool NT>
__global__ void __launch_bounds__(256) k_leapfrog_correlate(int64_t nvec, int ntail, CorrelateArgs a)
{
  sweep<VEC, NT>(nvec, ntail, WF_SWEEP_THREAD, [&](auto io, int64_t g) { correlate_entry(a, io, g); });
}

__global__ __launch_bounds__(256) void k_sources_add_values(int nunique, const int32_t* __restrict__ dof, const int32_t* __restrict__ off,
                                                             const int32_t* __restrict__ src, const double* __restrict__ weight,
                                                             const double* __restrict__ values, double scale, double* __restrict__ b)
{
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= nunique) return;
  double acc = 0.0;
  for (int e = off[u]; e < off[u + 1]; ++e) acc += weight[e] * values[src[e]];
  b[dof[u]] += scale * acc;
}

}  // namespace wf

extern "C" {

int wf_leapfrog_correlate(int64_t n, const double* d_lam, const double* d_up, const double* d_u, const double* d_um, double* d_p,
                          void* stream)
{
  if (n <= 0) return WF_OK;
  WF_REQUIRE(d_lam && d_up && d_u && d_um && d_p, "wf_leapfrog_correlate: null vector");
  auto overlap = [n](const double* p, const double* q) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), c = reinterpret_cast<uintptr_t>(q), len = (uintptr_t)n * sizeof(double);
    return a < c + len && c < a + len;
  };
  WF_REQUIRE(!overlap(d_p, d_lam) && !overlap(d_p, d_up) && !overlap(d_p, d_u) && !overlap(d_p, d_um),
             "wf_leapfrog_correlate: p must not overlap an input vector");
  wf::MarkerScope mk("wf_leapfrog_correlate");
  const wf::CorrelateArgs a{d_lam, d_up, d_u, d_um, d_p};
  const wf::SweepShape s = wf::sweep_shape(n, d_lam, d_up, d_u, d_um, d_p);
  if (s.vec)
    hipLaunchKernelGGL((wf::k_leapfrog_correlate<2, true>), dim3(s.grid), dim3(256), 0, (hipStream_t)stream, s.nvec, s.ntail, a);
  else
    hipLaunchKernelGGL((wf::k_leapfrog_correlate<1, false>), dim3(s.grid), dim3(256), 0, (hipStream_t)stream, s.nvec, s.ntail, a);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int wf_sources_add_values(const wf_sources* src, const double* d_values, double scale, double* d_b, void* stream)
{
  WF_REQUIRE(src != nullptr, "wf_sources_add_values: null handle");
  if (src->nunique == 0) return WF_OK;
  WF_REQUIRE(d_values != nullptr && d_b != nullptr && std::isfinite(scale), "wf_sources_add_values: null vector or scale not finite");
  hipLaunchKernelGGL(wf::k_sources_add_values, dim3(wf::grid_for((size_t)src->nunique, 256)), dim3(256), 0, (hipStream_t)stream,
                     src->nunique, src->d_dof.data(), src->d_off.data(), src->d_src.data(), src->d_weight.data(), d_values, scale, d_b);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

}  // extern "C"
