// C ABI of libwavehip: the device shims and the per-point geometry entry points (wf_geometry_hex, wf_geometry_hex_rule).
// Operator handles: op.h.  See include/wavehip.h for the reference interface each entry point replaces.
#include <cstring>

#include "op.h"

using namespace wf;

extern "C" {

// ---- device runtime shims ------------------------------------------------
int wf_device_count(int* count)
{
  WF_REQUIRE(count != nullptr, "wf_device_count: null output");
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) {
    *count = 0;
    set_error(std::string("hipGetDeviceCount failed: ") + hipGetErrorString(e));
    return WF_ERR_NODEVICE;
  }
  return WF_OK;
}

int wf_set_device(int device)
{
  int count = 0;
  int rc = wf_device_count(&count);
  if (rc != WF_OK) return rc;
  if (device < 0 || device >= count) {
    // utils.hpp:30-34: "The number of MPI processes should be less or equal the number of available devices"
    set_error("wf_set_device: device " + std::to_string(device) + " not available (" + std::to_string(count)
              + " devices)");
    return WF_ERR_NODEVICE;
  }
  WF_HIP_CHECK(hipSetDevice(device));
  return WF_OK;
}

int wf_device_info(int device, char* name, size_t name_len, size_t* total_mem, int* num_cu)
{
  hipDeviceProp_t prop;
  WF_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  if (name && name_len) {
    std::strncpy(name, prop.name, name_len - 1);
    name[name_len - 1] = 0;
  }
  if (total_mem) *total_mem = prop.totalGlobalMem;
  if (num_cu) *num_cu = prop.multiProcessorCount;
  return WF_OK;
}

int wf_malloc(void** d_ptr, size_t bytes)
{
  WF_REQUIRE(d_ptr != nullptr, "wf_malloc: null output");
  *d_ptr = nullptr;
  if (bytes == 0) return WF_OK;
  WF_HIP_CHECK(hipMalloc(d_ptr, bytes));
  return WF_OK;
}
int wf_free(void* d_ptr)
{
  if (d_ptr) WF_HIP_CHECK(hipFree(d_ptr));
  return WF_OK;
}
int wf_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes)
{
  if (bytes) WF_HIP_CHECK(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
  return WF_OK;
}
int wf_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes)
{
  if (bytes) WF_HIP_CHECK(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
  return WF_OK;
}
int wf_memset(void* d_dst, int value, size_t bytes, void* stream)
{
  if (bytes) WF_HIP_CHECK(hipMemsetAsync(d_dst, value, bytes, (hipStream_t)stream));
  return WF_OK;
}
int wf_sync(void* stream)
{
  if (stream)
    WF_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  else
    WF_HIP_CHECK(hipDeviceSynchronize());
  return WF_OK;
}

// ---- geometry --------------------------------------------------------------
static int geometry_hex_rule(int n, const double* h_pts, const double* h_wts, int ncells, int nverts,
                             const double* h_xverts, const int32_t* h_geom_dofmap, int use_fabs, int clamp, double* h_G,
                             double* h_detJ, const char* who)
{
  if (!(ncells >= 0 && nverts >= 0 && h_xverts && h_geom_dofmap)) {
    set_error(std::string(who) + ": bad arguments");
    return WF_ERR_INVALID;
  }
  int rc;
  if ((rc = check_index_range(h_geom_dofmap, (size_t)ncells * 8, nverts, std::string(who) + ": vertex index out of range")) != WF_OK)
    return rc;
  const size_t nq = (size_t)n * n * n;
  DevArray<double> d_G, d_det;
  if (h_G && (rc = d_G.alloc((size_t)ncells * nq * 9)) != WF_OK) return rc;
  if (h_detJ && (rc = d_det.alloc((size_t)ncells * nq)) != WF_OK) return rc;
  if ((rc = mesh_geometry_rule(n, h_pts, h_wts, {(size_t)ncells, nverts, h_xverts, h_geom_dofmap}, use_fabs, clamp, nullptr,
                               d_G.data(), nullptr, d_det.data())) != WF_OK)
    return rc;
  if (h_G) WF_HIP_CHECK(hipMemcpy(h_G, d_G.data(), d_G.bytes(), hipMemcpyDeviceToHost));
  if (h_detJ) WF_HIP_CHECK(hipMemcpy(h_detJ, d_det.data(), d_det.bytes(), hipMemcpyDeviceToHost));
  return WF_OK;
}

int wf_geometry_hex(int P, int ncells, int nverts, const double* h_xverts, const int32_t* h_geom_dofmap,
                    int use_fabs, int clamp, double* h_G, double* h_detJ)
{
  if (P < 1 || P > kMaxDegree) {
    set_error("wf_geometry_hex: degree must be 1..7");
    return WF_ERR_UNSUPPORTED;
  }
  const int n = P + 1;
  std::vector<double> pts(n), wts(n);
  gll_points_weights(n, pts.data(), wts.data());
  return geometry_hex_rule(n, pts.data(), wts.data(), ncells, nverts, h_xverts, h_geom_dofmap, use_fabs, clamp, h_G,
                           h_detJ, "wf_geometry_hex");
}

int wf_geometry_hex_rule(int ncells, int nverts, const double* h_xverts, const int32_t* h_geom_dofmap, int nq1,
                         const double* h_points1, const double* h_weights1, int use_fabs, int clamp, double* h_G,
                         double* h_detJ)
{
  WF_REQUIRE(nq1 >= 1 && nq1 <= WF_MAX_QUAD_POINTS && h_points1 && h_weights1, "wf_geometry_hex_rule: bad rule");
  return geometry_hex_rule(nq1, h_points1, h_weights1, ncells, nverts, h_xverts, h_geom_dofmap, use_fabs, clamp, h_G,
                           h_detJ, "wf_geometry_hex_rule");
}

}  // extern "C"
