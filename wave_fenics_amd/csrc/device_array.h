// The one owner of device memory: every array a handle or a set-up step allocates is a DevArray.
#pragma once
#include "common.h"

namespace wf {

// Move-only device array, freed in its destructor.  An empty array is a null pointer of 0 bytes, which is what kernels
// and wf_op_info see for an array an operator does not have.  Never a kernel argument: launch sites pass data().
template <typename T>
class DevArray {
 public:
  DevArray() = default;
  DevArray(DevArray&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  DevArray& operator=(DevArray&& o) noexcept
  {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  DevArray(const DevArray&) = delete;
  DevArray& operator=(const DevArray&) = delete;
  ~DevArray() { reset(); }

  // a fresh, uninitialised array of count elements (what it held is freed first)
  int alloc(size_t count)
  {
    reset();
    if (count == 0) return WF_OK;
    WF_HIP_CHECK(hipMalloc((void**)&p_, count * sizeof(T)));
    n_ = count;
    return WF_OK;
  }
  int upload(const T* host, size_t count)
  {
    int rc = alloc(count);
    if (rc != WF_OK) return rc;
    if (count) WF_HIP_CHECK(hipMemcpy(p_, host, count * sizeof(T), hipMemcpyHostToDevice));
    return WF_OK;
  }
  int upload(const std::vector<T>& host) { return upload(host.data(), host.size()); }
  // the whole array back on the host
  int download(std::vector<T>& host) const
  {
    host.resize(n_);
    if (n_) WF_HIP_CHECK(hipMemcpy(host.data(), p_, n_ * sizeof(T), hipMemcpyDeviceToHost));
    return WF_OK;
  }
  void reset()
  {
    if (p_) (void)hipFree(p_);
    p_ = nullptr, n_ = 0;
  }
  T* data() const { return p_; }
  size_t size() const { return n_; }
  size_t bytes() const { return n_ * sizeof(T); }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

}  // namespace wf
