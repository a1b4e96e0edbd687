// Streaming kernels of the reference-order RK4 loop and the free gather/scatter/transform
// kernels (a8, a9, a15, a16); the fused passes of the time loops are in time_step.hip.  All are
// HBM-bound; every kernel is a grid-stride loop or one entry per thread on capped_grid (common.h), 16-byte accesses
// where the operands allow it (aligned16, common.h).
#include "common.h"

namespace wf {

// reductions (one atomic per workgroup): 8 workgroups per CU
static inline unsigned reduction_grid(size_t n, unsigned block)
{
  size_t g = (n + block - 1) / block;
  const size_t cap = 256u * 8u;
  return (unsigned)(g < cap ? (g ? g : 1) : cap);
}

// common/cuda/scatter.cu:5-11
__global__ void k_gather(int32_t N, const int32_t* __restrict__ idx, const double* __restrict__ in,
                         double* __restrict__ out)
{
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < N; g += (int64_t)gridDim.x * blockDim.x)
    out[g] = in[idx[g]];
}
// common/cuda/scatter.cu:39-45 (hardware global_atomic_add_f64, no CAS loop)
__global__ void k_scatter_add(int32_t N, const int32_t* __restrict__ idx, const double* __restrict__ in,
                              double* __restrict__ out)
{
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < N; g += (int64_t)gridDim.x * blockDim.x)
    unsafeAtomicAdd(&out[idx[g]], in[g]);
}
__global__ void k_scatter_set(int32_t N, const int32_t* __restrict__ idx, const double* __restrict__ in,
                              double* __restrict__ out)
{
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < N; g += (int64_t)gridDim.x * blockDim.x)
    out[idx[g]] = in[g];
}
// common/cuda/transform.cu:6-11
__global__ void k_transform1(int32_t N, const double* __restrict__ in, const double* __restrict__ detJ,
                             double* __restrict__ out)
{
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < N; g += (int64_t)gridDim.x * blockDim.x)
    out[g] = in[g] * detJ[g];
}

__global__ void k_fill(int64_t n, double v, double* __restrict__ out)
{
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x)
    out[g] = v;
}
// 16-byte forms of fill / axpy / scale (aligned arrays; the odd last entry by thread 0 of the last workgroup)
__global__ void k_fill2(int64_t npairs, int tail, double v, double* out)
{
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < npairs) reinterpret_cast<double2*>(out)[g] = make_double2(v, v);
  if (tail && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[2 * npairs] = v;
}
__global__ void k_axpy2(int64_t npairs, int tail, double alpha, const double* x, const double* y, double* r)
{
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < npairs) {   // r may alias y (or x): every thread reads its entry before it writes it
    const double2 xx = reinterpret_cast<const double2*>(x)[g], yy = reinterpret_cast<const double2*>(y)[g];
    reinterpret_cast<double2*>(r)[g] = make_double2(xx.x * alpha + yy.x, xx.y * alpha + yy.y);
  }
  if (tail && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) r[2 * npairs] = x[2 * npairs] * alpha + y[2 * npairs];
}
__global__ void k_scale2(int64_t npairs, int tail, double alpha, double* x)
{
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < npairs) {
    double2 v = reinterpret_cast<double2*>(x)[g];
    v.x *= alpha;
    v.y *= alpha;
    reinterpret_cast<double2*>(x)[g] = v;
  }
  if (tail && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) x[2 * npairs] *= alpha;
}
// kernels::axpy of common/LinearGLL.hpp:28-33: r = x*alpha + y (r may alias y)
__global__ void k_axpy(int64_t n, double alpha, const double* x, const double* y, double* r)
{
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x)
    r[g] = x[g] * alpha + y[g];
}
__global__ void k_scale(int64_t n, double alpha, double* x)
{
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x)
    x[g] *= alpha;
}
// common/LinearGLL.hpp:189-190: out = b / m
__global__ void k_div(int64_t n, const double* b, const double* m, double* out)
{
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x)
    out[g] = b[g] / m[g];
}
// The same with 16-byte accesses; the diagonal m and the result bypass the caches (non-temporal): inside the
// RK4 loop / the bench step they are streamed once per pass, while b (= y of the stiffness apply) and the
// apply's x are what the next stiffness apply touches again and should keep the Infinity Cache
// (cfg2: 4 x 82 MB of vectors do not fit its 256 MB, x + y do).
// `tail` (0 or 1): the odd last entry, done by the first thread of the last block in the same launch (as its own
// launch it cost 4 us of the 44 us the mass-inverse takes in the bench step).
__global__ void k_div2(int64_t npairs, int tail, const double* __restrict__ b, const double* __restrict__ m, double* __restrict__ out)
{
  typedef double d2v __attribute__((ext_vector_type(2)));
  if (tail && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[2 * npairs] = b[2 * npairs] / m[2 * npairs];
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < npairs; g += (int64_t)gridDim.x * blockDim.x) {
    const d2v bb = reinterpret_cast<const d2v*>(b)[g];
    const d2v mm = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(m) + g);
    d2v r;
    r.x = bb.x / mm.x;
    r.y = bb.y / mm.y;
    __builtin_nontemporal_store(r, reinterpret_cast<d2v*>(out) + g);
  }
}
__global__ void k_mult_add(int64_t n, const double* __restrict__ m, const double* __restrict__ x, double* y)
{
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x)
    y[g] += m[g] * x[g];
}
// y += m .* x with 16-byte accesses, the diagonal streamed past the caches
__global__ void k_mult_add2(int64_t npairs, int tail, const double* __restrict__ m, const double* __restrict__ x, double* __restrict__ y)
{
  typedef double d2v __attribute__((ext_vector_type(2)));
  if (tail && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) y[2 * npairs] += m[2 * npairs] * x[2 * npairs];
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < npairs; g += (int64_t)gridDim.x * blockDim.x) {
    const d2v mm = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(m) + g);
    const d2v xx = reinterpret_cast<const d2v*>(x)[g];
    d2v yy = reinterpret_cast<d2v*>(y)[g];
    yy.x += mm.x * xx.x;
    yy.y += mm.y * xx.y;
    reinterpret_cast<d2v*>(y)[g] = yy;
  }
}
// common/cuda/la.hpp:87-103 inner_product: wave shuffle -> LDS -> one atomic per workgroup
__global__ void k_dot(int64_t n, const double* __restrict__ x, const double* __restrict__ y,
                      double* __restrict__ result)
{
  __shared__ double part[4];
  double s = 0.0;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x)
    s += x[g] * y[g];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) unsafeAtomicAdd(result, part[0] + part[1] + part[2] + part[3]);
}

}  // namespace wf

using namespace wf;

extern "C" {

int wf_gather(int32_t N, const int32_t* d_indices, const double* d_in, double* d_out, void* stream)
{
  if (N <= 0) return WF_OK;
  hipLaunchKernelGGL(k_gather, dim3(capped_grid(N, 256)), dim3(256), 0, (hipStream_t)stream, N, d_indices, d_in,
                     d_out);
  WF_LAUNCH_CHECK();
  return WF_OK;
}
int wf_scatter_add(int32_t N, const int32_t* d_indices, const double* d_in, double* d_out, void* stream)
{
  if (N <= 0) return WF_OK;
  hipLaunchKernelGGL(k_scatter_add, dim3(capped_grid(N, 256)), dim3(256), 0, (hipStream_t)stream, N, d_indices,
                     d_in, d_out);
  WF_LAUNCH_CHECK();
  return WF_OK;
}
int wf_scatter_set(int32_t N, const int32_t* d_indices, const double* d_in, double* d_out, void* stream)
{
  if (N <= 0) return WF_OK;
  hipLaunchKernelGGL(k_scatter_set, dim3(capped_grid(N, 256)), dim3(256), 0, (hipStream_t)stream, N, d_indices,
                     d_in, d_out);
  WF_LAUNCH_CHECK();
  return WF_OK;
}
int wf_transform1(int32_t N, const double* d_in, const double* d_detJ, double* d_out, void* stream)
{
  if (N <= 0) return WF_OK;
  hipLaunchKernelGGL(k_transform1, dim3(capped_grid(N, 256)), dim3(256), 0, (hipStream_t)stream, N, d_in, d_detJ,
                     d_out);
  WF_LAUNCH_CHECK();
  return WF_OK;
}
int wf_copy(int64_t n, const double* d_in, double* d_out, void* stream)
{
  if (n <= 0) return WF_OK;
  WF_HIP_CHECK(hipMemcpyAsync(d_out, d_in, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice,
                              (hipStream_t)stream));
  return WF_OK;
}
int wf_fill(int64_t n, double value, double* d_out, void* stream)
{
  if (n <= 0) return WF_OK;
  const int64_t np2 = n / 2;
  if (aligned16(d_out) && np2 > 0 && np2 < ((int64_t)1 << 30))
    hipLaunchKernelGGL(k_fill2, dim3((unsigned)((np2 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, np2, (int)(n - 2 * np2), value, d_out);
  else
    hipLaunchKernelGGL(k_fill, dim3(capped_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, n, value, d_out);
  WF_LAUNCH_CHECK();
  return WF_OK;
}
int wf_axpy(int64_t n, double alpha, const double* d_x, const double* d_y, double* d_r, void* stream)
{
  if (n <= 0) return WF_OK;
  const int64_t np2 = n / 2;
  if (aligned16(d_x, d_y, d_r) && np2 > 0 && np2 < ((int64_t)1 << 30))
    hipLaunchKernelGGL(k_axpy2, dim3((unsigned)((np2 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, np2, (int)(n - 2 * np2), alpha, d_x,
                       d_y, d_r);
  else
    hipLaunchKernelGGL(k_axpy, dim3(capped_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, n, alpha, d_x, d_y, d_r);
  WF_LAUNCH_CHECK();
  return WF_OK;
}
int wf_scale(int64_t n, double alpha, double* d_x, void* stream)
{
  if (n <= 0) return WF_OK;
  const int64_t np2 = n / 2;
  if (aligned16(d_x) && np2 > 0 && np2 < ((int64_t)1 << 30))
    hipLaunchKernelGGL(k_scale2, dim3((unsigned)((np2 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, np2, (int)(n - 2 * np2), alpha, d_x);
  else
    hipLaunchKernelGGL(k_scale, dim3(capped_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, n, alpha, d_x);
  WF_LAUNCH_CHECK();
  return WF_OK;
}
int wf_pointwise_div(int64_t n, const double* d_b, const double* d_m, double* d_out, void* stream)
{
  if (n <= 0) return WF_OK;
  const bool vec = aligned16(d_b, d_m, d_out) && d_out != d_b && d_out != d_m;
  const int64_t nv = vec ? n / 2 : 0;
  if (nv)
    hipLaunchKernelGGL(k_div2, dim3(capped_grid(nv, 256)), dim3(256), 0, (hipStream_t)stream, nv, (int)(n - 2 * nv), d_b, d_m, d_out);
  else
    hipLaunchKernelGGL(k_div, dim3(capped_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, n, d_b, d_m, d_out);
  WF_LAUNCH_CHECK();
  return WF_OK;
}
int wf_pointwise_mult_add(int64_t n, const double* d_m, const double* d_x, double* d_y, void* stream)
{
  if (n <= 0) return WF_OK;
  const bool vec = aligned16(d_m, d_x, d_y) && d_y != d_x && d_y != d_m;
  const int64_t nv = vec ? n / 2 : 0;
  if (nv)
    hipLaunchKernelGGL(k_mult_add2, dim3(capped_grid(nv, 256)), dim3(256), 0, (hipStream_t)stream, nv, (int)(n - 2 * nv), d_m, d_x, d_y);
  else
    hipLaunchKernelGGL(k_mult_add, dim3(capped_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, n, d_m, d_x, d_y);
  WF_LAUNCH_CHECK();
  return WF_OK;
}
int wf_dot(int64_t n, const double* d_x, const double* d_y, double* d_result, void* stream)
{
  WF_HIP_CHECK(hipMemsetAsync(d_result, 0, sizeof(double), (hipStream_t)stream));
  if (n <= 0) return WF_OK;
  hipLaunchKernelGGL(k_dot, dim3(reduction_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, n, d_x, d_y, d_result);
  WF_LAUNCH_CHECK();
  return WF_OK;
}
}  // extern "C"
