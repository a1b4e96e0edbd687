// The pass the discrete adjoint of the fourth-order leapfrog loop adds (LinearGLLOpt.misfit_gradient(scheme="leapfrog4"),
// wf_leapfrog4_correlate of include/wavehip.h), in a translation unit of its own: neighbours in a unit change code generation.
//
// k_leapfrog4_correlate: p[i] = (p[i] + lam[i] * ((up[i] - 2 u[i]) + um[i])) + 12 (om[i] * w[i]) and, if asked for,
//   z[i] = u[i] + w[i].  The first product is that of k_leapfrog_correlate (adjoint.hip); the second is the derivative
//   through the 1/m inside w = c12 b/m; z is the right operand of the step's first cell form, written here for 8 B/dof
//   instead of the 24 of an axpy.  The sweep of the step kernels (sweep.h): 16-byte entries where every operand allows
//   it, the odd last dof in the same launch, the scalar form otherwise.  Seven vectors read and p written = 64 B/dof, 72
//   with z.  up, um, w and p bypass the caches (nobody reads them next); om, u and z are read by the cell forms that
//   follow, lam by the corrector half of the adjoint step.
#include "common.h"
#include "sweep.h"
#include "wavehip.h"

namespace wf {

struct Correlate4Args {
  const double* lam;
  const double* om;
  const double* up;
  const double* u;
  const double* um;
  const double* w;
  double* p;
  double* z;
};

// evaluated as written (no contraction: the 16-byte and the scalar form give the same bits)
__device__ __forceinline__ double correlate4_value(double p, double lam, double om, double up, double u, double um, double w)
{
#pragma clang fp contract(off)
  return (p + lam * ((up - 2.0 * u) + um)) + 12.0 * (om * w);
}

__device__ __forceinline__ double correlate4_operand(double u, double w)
{
#pragma clang fp contract(off)
  return u + w;
}

template <bool Z, int VEC, bool NT>
__device__ __forceinline__ void correlate4_entry(const Correlate4Args& a, Lanes<VEC, NT> io, int64_t g)
{
  using L = Lanes<VEC, NT>;
  using V = typename L::V;
  const V ll = io.ld(a.lam, g), oo = io.ld(a.om, g), pp = io.ldnt(a.up, g), uu = io.ld(a.u, g), mm = io.ldnt(a.um, g),
          ww = io.ldnt(a.w, g);
  V acc = io.ldnt(a.p, g);
  for (int l = 0; l < VEC; ++l)
    L::at(acc, l) = correlate4_value(L::at(acc, l), L::at(ll, l), L::at(oo, l), L::at(pp, l), L::at(uu, l), L::at(mm, l), L::at(ww, l));
  io.stnt(a.p, g, acc);
  if constexpr (Z) {
    V zz = uu;
    for (int l = 0; l < VEC; ++l) L::at(zz, l) = correlate4_operand(L::at(uu, l), L::at(ww, l));
    io.st(a.z, g, zz);
  }
}

template <bool Z, int VEC, bool NT>
__global__ void __launch_bounds__(256) k_leapfrog4_correlate(int64_t nvec, int ntail, Correlate4Args a)
{
  sweep<VEC, NT>(nvec, ntail, WF_SWEEP_THREAD, [&](auto io, int64_t g) { correlate4_entry<Z>(a, io, g); });
}

template <bool Z>
void launch_correlate4(const SweepShape& s, const Correlate4Args& a, hipStream_t stream)
{
  if (s.vec)
    hipLaunchKernelGGL((k_leapfrog4_correlate<Z, 2, true>), dim3(s.grid), dim3(256), 0, stream, s.nvec, s.ntail, a);
  else
    hipLaunchKernelGGL((k_leapfrog4_correlate<Z, 1, false>), dim3(s.grid), dim3(256), 0, stream, s.nvec, s.ntail, a);
}

}  // namespace wf

extern "C" {

int wf_leapfrog4_correlate(int64_t n, const double* d_lam, const double* d_om, const double* d_up, const double* d_u,
                           const double* d_um, const double* d_w, double* d_p, double* d_z, void* stream)
{
  if (n <= 0) return WF_OK;
  WF_REQUIRE(d_lam && d_om && d_up && d_u && d_um && d_w && d_p, "wf_leapfrog4_correlate: null vector");
  auto overlap = [n](const double* p, const double* q) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), c = reinterpret_cast<uintptr_t>(q), len = (uintptr_t)n * sizeof(double);
    return a < c + len && c < a + len;
  };
  const double* const in[6] = {d_lam, d_om, d_up, d_u, d_um, d_w};
  for (const double* q : in) {
    WF_REQUIRE(!overlap(d_p, q), "wf_leapfrog4_correlate: p must not overlap an input vector");
    WF_REQUIRE(!d_z || !overlap(d_z, q), "wf_leapfrog4_correlate: z must not overlap an input vector");
  }
  WF_REQUIRE(!d_z || !overlap(d_z, d_p), "wf_leapfrog4_correlate: z must not overlap p");
  wf::MarkerScope mk("wf_leapfrog4_correlate");
  const wf::Correlate4Args a{d_lam, d_om, d_up, d_u, d_um, d_w, d_p, d_z};
  const wf::SweepShape s = wf::sweep_shape(n, d_lam, d_om, d_up, d_u, d_um, d_w, d_p, (const double*)d_z);
  if (d_z)
    wf::launch_correlate4<true>(s, a, (hipStream_t)stream);
  else
    wf::launch_correlate4<false>(s, a, (hipStream_t)stream);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

}  // extern "C"
