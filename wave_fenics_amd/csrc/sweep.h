// The sweep of the streaming passes (time_step.hip, adjoint.hip): the lane accessors of an entry, the grid-stride loop
// with the odd last dof in the same launch, and the launch shape chosen from the operands' alignment.
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace wf {

// Entry g, VEC doubles wide, of arrays that start at dof `off`: plain and non-temporal (cache-bypassing; NT, and only
// the 16-byte form) loads and stores, and the lanes of an entry by number.
template <int VEC, bool NT>
struct Lanes {
  using V = typename std::conditional<VEC == 2, double2, double>::type;
  typedef double d2v __attribute__((ext_vector_type(2)));
  int64_t off;

  __device__ __forceinline__ V ld(const double* p, int64_t g) const { return reinterpret_cast<const V*>(p + off)[g]; }
  __device__ __forceinline__ V ldnt(const double* p, int64_t g) const
  {
    if constexpr (NT && VEC == 2) {
      const d2v v = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p + off) + g);
      return make_double2(v.x, v.y);
    } else
      return ld(p, g);
  }
  __device__ __forceinline__ void st(double* p, int64_t g, V v) const { reinterpret_cast<V*>(p + off)[g] = v; }
  __device__ __forceinline__ void stnt(double* p, int64_t g, V v) const
  {
    if constexpr (NT && VEC == 2) {
      d2v w;
      w.x = v.x;
      w.y = v.y;
      __builtin_nontemporal_store(w, reinterpret_cast<d2v*>(p + off) + g);
    } else
      st(p, g, v);
  }
  static __device__ __forceinline__ double& at(V& v, int lane)
  {
    if constexpr (VEC == 2)
      return lane ? v.y : v.x;
    else
      return v;
  }
  static __device__ __forceinline__ double at(const V& v, int lane)
  {
    if constexpr (VEC == 2)
      return lane ? v.y : v.x;
    else
      return v;
  }
};

// The sweep of a pass: nvec entries of width VEC grid-stride, then `ntail` single entries (at most VEC - 1: the odd
// last dof of a 16-byte sweep) by the first threads of the last block -- one launch whatever the vector length.
// entry(Lanes, g) does entry g.  The thread's place in the grid (WF_SWEEP_THREAD: first entry, stride, whether its block
// is the last) is an argument and has to be spelled in the kernel's own body: read in a helper, blockDim.x is no longer
// folded to the launch bound, and every kernel gains the load and select of a non-uniform workgroup size.
template <int VEC, bool NT, class Entry>
__device__ __forceinline__ void sweep(int64_t nvec, int ntail, int64_t first, int64_t stride, bool last, Entry&& entry)
{
  for (int64_t g = first; g < nvec; g += stride) entry(Lanes<VEC, NT>{0}, g);
  if (VEC > 1 && last && (int)threadIdx.x < ntail) entry(Lanes<1, false>{(int64_t)VEC * nvec}, (int64_t)threadIdx.x);
}
#define WF_SWEEP_THREAD (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, blockIdx.x == gridDim.x - 1

// Launch shape of a sweep over n dofs: the 16-byte form (n / 2 pairs and the odd last dof) if every pointer is 16-byte
// aligned (a null pointer is), else the scalar form.
struct SweepShape {
  bool vec;
  int64_t nvec;
  int ntail;
  unsigned grid;
};
template <class... T>
inline SweepShape sweep_shape(int64_t n, const T*... p)
{
  SweepShape s;
  s.vec = aligned16(p...);
  s.nvec = s.vec ? n / 2 : n;
  s.ntail = s.vec ? (int)(n - 2 * s.nvec) : 0;
  s.grid = capped_grid((size_t)std::max<int64_t>(s.nvec, 1), 256);
  return s;
}

}  // namespace wf
