// Point receivers and point sources on the device (gfx950).
//
// A point in cell c with reference coordinates xi sees the degree-P field as
//   u(x) = sum_l (wx[i] wy[j]) wz[k] u[dofmap[c][l]],  l = i + n (j + n k),  n = P + 1,
// with the 1-D Lagrange weights of wf_points_weights.  A receiver samples that sum; a point source
// f = s(t) delta(x - x_s) loads the right-hand side with its transpose, b[d] += s(t) phi_d(x_s).
//
// k_points_sample: one wavefront per point, four points per 256-thread workgroup.  Lane L takes l = L, L + 64, ... in
//   ascending order (coalesced index reads), forms the weight product in that fixed association and accumulates in a
//   register; a fixed 64-lane butterfly of cross-lane moves sums the lanes, lane 0 stores.  No LDS, no atomics: out[r]
//   depends on the point alone, bit for bit, however many points share the launch.
// k_sources_add: one thread per unique dof of the merged CSR (points_plan.h).  The thread evaluates the wavelets of its
//   own entries at time t in fp64, sums w s(t) in CSR order and does one b[d] += acc: one writer per dof.
#include "common.h"
#include "device_array.h"
#include "points_handles.h"
#include "points_plan.h"
#include "wavehip.h"

namespace wf {

constexpr int kPointsPerGroup = 4;
constexpr int kWaveletPars = 5;

__global__ __launch_bounds__(256) void k_points_sample(int n, int nd, int npoints, const int32_t* __restrict__ dofs,
                                                        const double* __restrict__ w, const double* __restrict__ x,
                                                        double* __restrict__ out)
{
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * kPointsPerGroup + (threadIdx.x >> 6);
  if (r >= npoints) return;   // the whole wavefront leaves
  const int32_t* row = dofs + (size_t)r * nd;
  const double *wx = w + (size_t)r * 3 * n, *wy = wx + n, *wz = wy + n;
  const int n2 = n * n, iters = (nd + 63) >> 6;
  double acc = 0.0;
  for (int it = 0; it < iters; ++it) {   // a wave-uniform trip count: every lane reaches the butterfly
    const int l = lane + 64 * it;
    double term = 0.0;   // lanes past the row add an exact +0.0
    if (l < nd) {
      const int k = l / n2, j = (l - k * n2) / n, i = l - k * n2 - j * n;
      term = ((wx[i] * wy[j]) * wz[k]) * x[row[l]];
    }
    acc += term;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) out[r] = acc;
}

__device__ inline double wavelet_value(int kind, const double* __restrict__ par, const double* __restrict__ tab, int ns, double t)
{
  const double amp = par[0];
  if (kind == WF_WAVELET_RICKER) {
    const double arg = M_PI * par[1] * (t - par[2]);
    const double a = arg * arg;
    if (!(a < 800.0)) return 0.0;   // e^{-a} is below the smallest double: a clean zero, whatever 1 - 2a has grown to
    return amp * ((1.0 - 2.0 * a) * exp(-a));
  }
  // WF_WAVELET_SAMPLED: linear interpolation on t_start + k dt, zero outside the table
  const double u = (t - par[3]) / par[4];
  if (!(u >= 0.0) || !(u <= (double)(ns - 1))) return 0.0;
  int k = (int)u;
  if (k > ns - 2) k = ns - 2;
  const double th = u - (double)k;
  return amp * ((1.0 - th) * tab[k] + th * tab[k + 1]);
}

__global__ __launch_bounds__(256) void k_sources_add(int nunique, const int32_t* __restrict__ dof, const int32_t* __restrict__ off,
                                                      const int32_t* __restrict__ src, const double* __restrict__ weight,
                                                      const int32_t* __restrict__ kind, const int32_t* __restrict__ soff,
                                                      const double* __restrict__ par, const double* __restrict__ samples, double t,
                                                      double* __restrict__ b)
{
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= nunique) return;
  double acc = 0.0;
  for (int e = off[u]; e < off[u + 1]; ++e) {
    const int s = src[e];
    acc += weight[e] * wavelet_value(kind[s], par + (size_t)s * kWaveletPars, samples + soff[s], soff[s + 1] - soff[s], t);
  }
  b[dof[u]] += acc;
}

// k_sources_add with the wavelet of every entry replaced by ((a0 s(t0)) + a1 s(t1)) + a2 s(t2), the first nt terms, formed
// as written; times and weights travel with the launch.
struct SourceStencil {
  int nt;
  double t[3], a[3];
};

__device__ inline double stencil_sum(const SourceStencil& st, int kind, const double* __restrict__ par, const double* __restrict__ tab,
                                     int ns)
{
#pragma clang fp contract(off)
  double sum = st.a[0] * wavelet_value(kind, par, tab, ns, st.t[0]);
  if (st.nt > 1) sum = sum + st.a[1] * wavelet_value(kind, par, tab, ns, st.t[1]);
  if (st.nt > 2) sum = sum + st.a[2] * wavelet_value(kind, par, tab, ns, st.t[2]);
  return sum;
}

__global__ __launch_bounds__(256) void k_sources_add_stencil(int nunique, const int32_t* __restrict__ dof, const int32_t* __restrict__ off,
                                                              const int32_t* __restrict__ src, const double* __restrict__ weight,
                                                              const int32_t* __restrict__ kind, const int32_t* __restrict__ soff,
                                                              const double* __restrict__ par, const double* __restrict__ samples,
                                                              SourceStencil st, double* __restrict__ b)
{
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= nunique) return;
  double acc = 0.0;
  for (int e = off[u]; e < off[u + 1]; ++e) {
    const int s = src[e];
    acc += weight[e] * stencil_sum(st, kind[s], par + (size_t)s * kWaveletPars, samples + soff[s], soff[s + 1] - soff[s]);
  }
  b[dof[u]] += acc;
}

}  // namespace wf

extern "C" {

int wf_points_create(int P, int64_t ndofs, int npoints, const int32_t* h_dofs, const double* h_w, wf_points** out)
{
  WF_REQUIRE(out != nullptr, "wf_points_create: null output");
  *out = nullptr;
  if (P < 1 || P > wf::kMaxDegree) {
    wf::set_error("wf_points_create: degree must be 1..7");
    return WF_ERR_UNSUPPORTED;
  }
  WF_REQUIRE(ndofs >= 0 && ndofs <= INT32_MAX && npoints >= 0, "wf_points_create: bad argument");
  WF_REQUIRE(npoints == 0 || (h_dofs && h_w), "wf_points_create: null array");
  const int n = P + 1, nd = n * n * n;
  WF_REQUIRE((int64_t)npoints * nd <= INT32_MAX, "wf_points_create: npoints * (P+1)^3 exceeds int32");
  int rc = wf::check_index_range(h_dofs, (size_t)npoints * nd, ndofs, "wf_points_create: dof index out of range");
  if (rc != WF_OK) return rc;
  for (size_t e = 0; e < (size_t)npoints * 3 * n; ++e) WF_REQUIRE(std::isfinite(h_w[e]), "wf_points_create: weight is not finite");
  wf_points* p = new wf_points;
  p->P = P, p->nd = nd, p->npoints = npoints, p->ndofs = ndofs;
  p->h_dofs.assign(h_dofs, h_dofs + (size_t)npoints * nd);
  p->h_w.assign(h_w, h_w + (size_t)npoints * 3 * n);
  if ((rc = p->d_dofs.upload(p->h_dofs)) != WF_OK || (rc = p->d_w.upload(p->h_w)) != WF_OK) {
    delete p;
    return rc;
  }
  *out = p;
  return WF_OK;
}

int wf_points_destroy(wf_points* plan)
{
  delete plan;
  return WF_OK;
}

int wf_points_info(const wf_points* plan, int* npoints, int* nd, int* degree)
{
  WF_REQUIRE(plan != nullptr, "wf_points_info: null plan");
  if (npoints) *npoints = plan->npoints;
  if (nd) *nd = plan->nd;
  if (degree) *degree = plan->P;
  return WF_OK;
}

int wf_points_sample(const wf_points* plan, const double* d_x, double* d_out, void* stream)
{
  WF_REQUIRE(plan != nullptr, "wf_points_sample: null plan");
  if (plan->npoints == 0) return WF_OK;
  WF_REQUIRE(d_x && d_out, "wf_points_sample: null vector");
  hipLaunchKernelGGL(wf::k_points_sample, dim3(wf::grid_for((size_t)plan->npoints, wf::kPointsPerGroup)), dim3(256), 0,
                     (hipStream_t)stream, plan->P + 1, plan->nd, plan->npoints, plan->d_dofs.data(), plan->d_w.data(), d_x, d_out);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int wf_sources_create(const wf_points* plan, int nsrc, const int32_t* h_point_of_source, const wf_wavelet* h_wavelets,
                      wf_sources** out)
{
  WF_REQUIRE(out != nullptr, "wf_sources_create: null output");
  *out = nullptr;
  WF_REQUIRE(plan != nullptr && nsrc >= 0, "wf_sources_create: bad argument");
  WF_REQUIRE(nsrc == 0 || (h_point_of_source && h_wavelets), "wf_sources_create: null array");
  const int n = plan->P + 1, nd = plan->nd;
  std::vector<int32_t> dofs((size_t)nsrc * nd), kind(nsrc), soff(nsrc + 1, 0);
  std::vector<double> w((size_t)nsrc * 3 * n), par((size_t)nsrc * wf::kWaveletPars), samples;
  for (int s = 0; s < nsrc; ++s) {
    const int r = h_point_of_source[s];
    WF_REQUIRE(r >= 0 && r < plan->npoints, "wf_sources_create: point index out of range (source " + std::to_string(s) + ")");
    std::copy(plan->h_dofs.begin() + (size_t)r * nd, plan->h_dofs.begin() + (size_t)(r + 1) * nd, dofs.begin() + (size_t)s * nd);
    std::copy(plan->h_w.begin() + (size_t)r * 3 * n, plan->h_w.begin() + (size_t)(r + 1) * 3 * n, w.begin() + (size_t)s * 3 * n);
    const wf_wavelet& wl = h_wavelets[s];
    const std::string who = "wf_sources_create: source " + std::to_string(s) + ": ";
    WF_REQUIRE(wl.kind == WF_WAVELET_RICKER || wl.kind == WF_WAVELET_SAMPLED, who + "unknown wavelet kind");
    WF_REQUIRE(std::isfinite(wl.amplitude), who + "amplitude is not finite");
    double* q = par.data() + (size_t)s * wf::kWaveletPars;
    q[0] = wl.amplitude, q[1] = q[2] = q[3] = 0.0, q[4] = 1.0;
    kind[s] = wl.kind;
    if (wl.kind == WF_WAVELET_RICKER) {
      WF_REQUIRE(std::isfinite(wl.frequency) && wl.frequency > 0.0 && std::isfinite(wl.delay), who + "frequency must be positive, delay finite");
      q[1] = wl.frequency, q[2] = wl.delay;
    } else {
      WF_REQUIRE(wl.nsamples >= 2 && wl.h_samples, who + "a sampled wavelet needs nsamples >= 2");
      WF_REQUIRE(std::isfinite(wl.dt) && wl.dt > 0.0 && std::isfinite(wl.t_start), who + "dt must be positive, t_start finite");
      for (int k = 0; k < wl.nsamples; ++k) WF_REQUIRE(std::isfinite(wl.h_samples[k]), who + "sample is not finite");
      q[3] = wl.t_start, q[4] = wl.dt;
      samples.insert(samples.end(), wl.h_samples, wl.h_samples + wl.nsamples);
    }
    soff[s + 1] = (int32_t)samples.size();
  }
  wf::SourceCsr csr;
  wf::sources_merge(plan->P, nsrc, dofs.data(), w.data(), csr);
  wf_sources* src = new wf_sources;
  src->nsrc = nsrc, src->nunique = (int)csr.dof.size(), src->nentries = (int)csr.src.size(), src->ndofs = plan->ndofs;
  int rc;
  if ((rc = src->d_dof.upload(csr.dof)) != WF_OK || (rc = src->d_off.upload(csr.off)) != WF_OK || (rc = src->d_src.upload(csr.src)) != WF_OK
      || (rc = src->d_weight.upload(csr.weight)) != WF_OK || (rc = src->d_kind.upload(kind)) != WF_OK
      || (rc = src->d_soff.upload(soff)) != WF_OK || (rc = src->d_par.upload(par)) != WF_OK
      || (rc = src->d_samples.upload(samples)) != WF_OK) {
    delete src;
    return rc;
  }
  *out = src;
  return WF_OK;
}

int wf_sources_destroy(wf_sources* src)
{
  delete src;
  return WF_OK;
}

int wf_sources_info(const wf_sources* src, int* nsources, int* nunique, int* nentries)
{
  WF_REQUIRE(src != nullptr, "wf_sources_info: null handle");
  if (nsources) *nsources = src->nsrc;
  if (nunique) *nunique = src->nunique;
  if (nentries) *nentries = src->nentries;
  return WF_OK;
}

int wf_sources_add(const wf_sources* src, double t, double* d_b, void* stream)
{
  WF_REQUIRE(src != nullptr, "wf_sources_add: null handle");
  if (src->nunique == 0) return WF_OK;
  WF_REQUIRE(d_b != nullptr && std::isfinite(t), "wf_sources_add: null vector or time not finite");
  hipLaunchKernelGGL(wf::k_sources_add, dim3(wf::grid_for((size_t)src->nunique, 256)), dim3(256), 0, (hipStream_t)stream, src->nunique,
                     src->d_dof.data(), src->d_off.data(), src->d_src.data(), src->d_weight.data(), src->d_kind.data(),
                     src->d_soff.data(), src->d_par.data(), src->d_samples.data(), t, d_b);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int wf_sources_add_stencil(const wf_sources* src, int nt, const double* h_t, const double* h_a, double* d_b, void* stream)
{
  WF_REQUIRE(src != nullptr, "wf_sources_add_stencil: null handle");
  WF_REQUIRE(nt >= 1 && nt <= 3, "wf_sources_add_stencil: nt must be 1, 2 or 3");
  WF_REQUIRE(h_t && h_a, "wf_sources_add_stencil: null times or weights");
  wf::SourceStencil st{nt, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  for (int k = 0; k < nt; ++k) {
    WF_REQUIRE(std::isfinite(h_t[k]) && std::isfinite(h_a[k]), "wf_sources_add_stencil: time or weight not finite");
    st.t[k] = h_t[k], st.a[k] = h_a[k];
  }
  if (src->nunique == 0) return WF_OK;
  WF_REQUIRE(d_b != nullptr, "wf_sources_add_stencil: null vector");
  hipLaunchKernelGGL(wf::k_sources_add_stencil, dim3(wf::grid_for((size_t)src->nunique, 256)), dim3(256), 0, (hipStream_t)stream,
                     src->nunique, src->d_dof.data(), src->d_off.data(), src->d_src.data(), src->d_weight.data(), src->d_kind.data(),
                     src->d_soff.data(), src->d_par.data(), src->d_samples.data(), st, d_b);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

}  // extern "C"
