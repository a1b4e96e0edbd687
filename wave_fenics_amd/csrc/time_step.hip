// The fused passes of the time loops: the RK4 stage and the leapfrog step (one streaming pass between two stiffness
// applies each), and the diagonal boundary operator with its plan.  Both passes are the same sweep (16-byte entries
// where every operand allows it, the odd last dof in the same launch) over the same lane accessors, and both find the
// boundary dofs of an entry by the same plan lookup; a pass states its own arithmetic only.
#include <memory>
#include <type_traits>
#include <vector>

#include "device_array.h"
#include "sweep.h"
#include "wavehip.h"

namespace wf {

// diagonal boundary operator, LinearGLL.hpp:175 / forms.ufl:19-24
__global__ void k_boundary(int32_t n1, const int32_t* __restrict__ idx1, const double* __restrict__ m1,
                           double s1, int32_t n2, const int32_t* __restrict__ idx2,
                           const double* __restrict__ m2, double s2, const double* __restrict__ v,
                           double* __restrict__ b)
{
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < (int64_t)n1 + n2;
       g += (int64_t)gridDim.x * blockDim.x) {
    if (g < n1) {
      unsafeAtomicAdd(&b[idx1[g]], s1 * m1[g]);
    } else {
      const int64_t h = g - n1;
      const int32_t d = idx2[h];
      unsafeAtomicAdd(&b[d], s2 * m2[h] * v[d]);
    }
  }
}

// The boundary sets as the fused passes read them: a bitmap over the dofs (one 64-bit word per 64 dofs, L2-resident), a
// running count per word and the two coefficient arrays over the union set in dof order: 0.2 B/dof read instead of a
// further launch per pass.
struct BoundaryPlanDev {
  const unsigned long long* mask = nullptr;   // [ceil(n / 64)]
  const uint32_t* prefix = nullptr;           // [ceil(n / 64)] boundary dofs in front of the word
  const double* c1 = nullptr;                 // [nb] facet mass of Gamma_1 (0 for dofs only in Gamma_2)
  const double* c2 = nullptr;                 // [nb] facet mass of Gamma_2
  double s1 = 0.0, s2 = 0.0;
};

// f(lane, r) for every dof d0 + lane, lane < VEC, of the entry that starts at dof d0 and lies in the union set, r its row
// in c1 / c2.  VEC == 2: d0 is even, so both dofs lie in one mask word.
template <int VEC, class F>
__device__ __forceinline__ void for_boundary_dofs(const BoundaryPlanDev& bc, int64_t d0, F&& f)
{
  unsigned long long word;
  bool any = true;
  if constexpr (VEC == 2) {
    // a wave covers 128 consecutive dofs = two mask words (d0 / 2 is a multiple of 64 in lane 0): fetch
    // them with scalar loads and skip the whole block when the wave holds no boundary dof (97 % of the waves)
    const int64_t w0 = __builtin_amdgcn_readfirstlane((int)(d0 >> 6));
    const unsigned long long wa = bc.mask[w0], wb = bc.mask[w0 + 1];   // mask has one spare word at the end
    any = (wa | wb) != 0ull;
    word = (d0 >> 6) == w0 ? wa : wb;
  } else {
    word = bc.mask[d0 >> 6];
  }
  if (any) {
    const unsigned bits = (unsigned)(word >> (d0 & 63)) & (VEC == 2 ? 3u : 1u);
    if (bits) {
      const unsigned long long below = word & ((1ull << (d0 & 63)) - 1ull);
      int64_t r = (int64_t)bc.prefix[d0 >> 6] + __popcll(below);
      if constexpr (VEC == 2) {
        if (bits & 1u) {
          f(0, r);
          ++r;
        }
        if (bits & 2u) f(1, r);
      } else {
        f(0, r);
      }
    }
  }
}

// Fused tail of one RK4 stage (common/LinearGLL.hpp:182-191 divide, :260 f0,
// :264-265 solution update) plus the head of the next stage (:250-254) and the
// zeroing of b for the next stiffness apply (:173), so that the vector algebra
// between two stiffness applies is ONE pass:
//   kv = b / m ; ku = vn
//   u_ = ku*(dt*b_i) + u_read ; v_ = kv*(dt*b_i) + v_read ; b = 0
//   un = ku*(dt*a_next) + u0  ; vn_next = kv*(dt*a_next) + v0              (if has_next)
// HBM traffic per dof: stage 0 (u_read = u0, v_read = vn = v0) 4 reads + 5 writes = 72 B,
// stages 1-2 7 + 5 = 96 B, stage 3 5 + 3 = 64 B -- 82 B/stage on average against the
// 208 B/dof of the reference's separate copy/axpy/fill/transform passes.
// u_read/v_read may alias u_/v_ (stages 1..3) or be u0/v0 (stage 0).
// VEC = 2: 16-byte accesses (all pointers 16-byte aligned, n counted in pairs).
// NT: everything except the two vectors the next stiffness apply touches (un, b) bypasses the caches.
// BC: instead of zeroing b for the next stiffness apply, leave the NEXT right-hand side's diagonal boundary
// term in it (LinearGLL.hpp:175, forms.ufl:19-24): b[i] = s1 c1[r] + s2 c2[r] v'[i] for the dofs of the
// boundary sets, v' = the v argument of the next f1 (vn_next, or the updated solution after the last stage).
struct StageArgs {
  double bdt, adt_next;
  double* b;
  const double* m;
  const double* vn;
  const double* u_read;
  const double* v_read;
  double* u_;
  double* v_;
  const double* u0;
  const double* v0;
  double* un;
  double* vn_next;
  BoundaryPlanDev bc;
};

template <bool HAS_NEXT, bool BC, int VEC, bool NT>
__device__ __forceinline__ void stage_entry(const StageArgs& a, Lanes<VEC, NT> io, int64_t g)
{
  using L = Lanes<VEC, NT>;
  using V = typename L::V;
  const double bdt = a.bdt, adt_next = a.adt_next;
  const V bb = io.ldnt(a.b, g), mm = io.ldnt(a.m, g), ku = io.ldnt(a.vn, g), ur = io.ldnt(a.u_read, g), vr = io.ldnt(a.v_read, g);
  V kv, uo, vo, zero;
  // spelled per width, not as a loop over the lanes like leapfrog_entry: the loop form compiles to the same instructions
  // in another order in four of the eight kernels, this one in two
  if constexpr (VEC == 2) {
    kv = make_double2(bb.x / mm.x, bb.y / mm.y);
    uo = make_double2(ku.x * bdt + ur.x, ku.y * bdt + ur.y);
    vo = make_double2(kv.x * bdt + vr.x, kv.y * bdt + vr.y);
    zero = make_double2(0.0, 0.0);
  } else {
    kv = bb / mm;
    uo = ku * bdt + ur;
    vo = kv * bdt + vr;
    zero = 0.0;
  }
  V vnext = vo;   // the v the next right-hand side sees
  if constexpr (HAS_NEXT) {
    const V a0 = io.ldnt(a.u0, g), c0 = io.ldnt(a.v0, g);
    V un_, vn_;
    if constexpr (VEC == 2) {
      un_ = make_double2(ku.x * adt_next + a0.x, ku.y * adt_next + a0.y);
      vn_ = make_double2(kv.x * adt_next + c0.x, kv.y * adt_next + c0.y);
    } else {
      un_ = ku * adt_next + a0;
      vn_ = kv * adt_next + c0;
    }
    io.st(a.un, g, un_);
    io.stnt(a.vn_next, g, vn_);
    vnext = vn_;
  }
  io.stnt(a.u_, g, uo);
  io.stnt(a.v_, g, vo);
  if constexpr (BC) {
    const BoundaryPlanDev& bc = a.bc;
    for_boundary_dofs<VEC>(bc, io.off + (int64_t)VEC * g, [&](int lane, int64_t r) {
      L::at(zero, lane) = bc.s1 * bc.c1[r] + bc.s2 * bc.c2[r] * L::at(vnext, lane);
    });
  }
  io.st(a.b, g, zero);
}

template <int VEC, bool HAS_NEXT, bool NT = false, bool BC = false>
__global__ void __launch_bounds__(256) k_rk4_stage(int64_t nvec, int ntail, StageArgs a)
{
  sweep<VEC, NT>(nvec, ntail, WF_SWEEP_THREAD, [&](auto io, int64_t g) { stage_entry<HAS_NEXT, BC>(a, io, g); });
}

// One step of the central-difference (leapfrog, explicit Newmark beta = 0, gamma = 1/2) scheme on
// m u'' + d u' - K u = s1 c1 with the diagonal absorbing term d = -s2 c2 taken centred, in one pass after the
// stiffness apply that left K u in b:
//   dof outside the boundary sets:  a = b / m ; u_next = dt2 a + (2 u - u_prev)
//   dof r of the union set:         h = hdt c2[r] ; u_next = (dt2 (b + s1 c1[r]) + ((2 m) u - (m - h) u_prev)) / (m + h)
//   v = (u_next - u_prev) / (2 dt)  (HAS_V) ; b = +0.0
// dt2 = dt^2, hdt = -s2 dt / 2, tdt = 2 dt from the host.  u_next may alias u_prev (every thread reads its entry
// before it writes it).  HBM traffic per dof: b, m, u, u_prev read, u_next, b written = 48 B (56 B with v).
// u_next and b are what the next stiffness apply touches and are stored plainly, u is read plainly (the apply just
// read it); b, m, u_prev (and v) bypass the caches as in the stage kernel.
struct LeapfrogArgs {
  double dt2, hdt, tdt;
  double* b;
  const double* m;
  const double* u;
  const double* up;
  double* un;
  double* v;
  BoundaryPlanDev bc;   // s1 = the coefficient of the Gamma_1 term at the current time; s2 is folded into hdt
};

// the two update expressions, evaluated as written (no contraction: every compiled form gives the same bits)
__device__ __forceinline__ double leapfrog_plain(double b, double m, double u, double up, double dt2)
{
#pragma clang fp contract(off)
  const double a = b / m;
  return dt2 * a + (2.0 * u - up);
}
__device__ __forceinline__ double leapfrog_boundary(double b, double m, double u, double up, double dt2, double hdt, double s1,
                                                    double c1, double c2)
{
#pragma clang fp contract(off)
  const double h = hdt * c2;
  return (dt2 * (b + s1 * c1) + ((2.0 * m) * u - (m - h) * up)) / (m + h);
}

template <bool BC, bool HAS_V, int VEC, bool NT>
__device__ __forceinline__ void leapfrog_entry(const LeapfrogArgs& a, Lanes<VEC, NT> io, int64_t g)
{
  using L = Lanes<VEC, NT>;
  using V = typename L::V;
  const double dt2 = a.dt2;
  const V bb = io.ldnt(a.b, g), mm = io.ldnt(a.m, g), uu = io.ld(a.u, g), pp = io.ldnt(a.up, g);
  V nn, zero;
  for (int l = 0; l < VEC; ++l) {
    L::at(nn, l) = leapfrog_plain(L::at(bb, l), L::at(mm, l), L::at(uu, l), L::at(pp, l), dt2);
    L::at(zero, l) = 0.0;
  }
  if constexpr (BC) {
    const BoundaryPlanDev& bc = a.bc;
    for_boundary_dofs<VEC>(bc, io.off + (int64_t)VEC * g, [&](int lane, int64_t r) {
      L::at(nn, lane) = leapfrog_boundary(L::at(bb, lane), L::at(mm, lane), L::at(uu, lane), L::at(pp, lane), dt2, a.hdt, bc.s1,
                                          bc.c1[r], bc.c2[r]);
    });
  }
  io.st(a.un, g, nn);
  if constexpr (HAS_V) {
    V w;
    for (int l = 0; l < VEC; ++l) L::at(w, l) = (L::at(nn, l) - L::at(pp, l)) / a.tdt;
    io.stnt(a.v, g, w);
  }
  io.st(a.b, g, zero);
}

template <int VEC, bool NT, bool BC, bool HAS_V>
__global__ void __launch_bounds__(256) k_leapfrog_step(int64_t nvec, int ntail, LeapfrogArgs a)
{
  sweep<VEC, NT>(nvec, ntail, WF_SWEEP_THREAD, [&](auto io, int64_t g) { leapfrog_entry<BC, HAS_V>(a, io, g); });
}

// The two passes of one fourth-order (modified-equation) leapfrog step, (u+ - 2u + u-)/dt^2 = A u + (dt^2/12) A^2 u with
// A = M^-1 K: the predictor after the apply that left K u in b, the corrector after the apply that left K w in b.
//   predictor:  u* = the leapfrog update above (leapfrog_plain / leapfrog_boundary: the same bits)
//               w = c12 (b / m), on the union set c12 ((b + s1 c1[r]) / m) ; b = +0.0
//   corrector:  u_next = u* + dt2 (b / m), on the union set h = hdt c2[r] ; u_next = u* + (dt2 (b + s1c c1[r])) / (m + h)
//               v = (u_next - u_prev) / (2 dt)  (HAS_V) ; b = +0.0
// c12 = dt2 / 12 from the host, s1c the second difference of s1 over 12.  u* may alias u_prev and u_next may alias u*
// (every thread reads its entry before it writes it).  HBM traffic per dof: predictor b, m, u, u_prev read, u*, w, b
// written = 56 B; corrector b, m, u* read, u_next, b written = 40 B (56 B with u_prev and v).
// Plain accesses for what the next apply touches (w and b; u_next and b) and for u, which the last apply just read;
// everything else bypasses the caches as in k_leapfrog_step.
struct Leapfrog4PredictArgs {
  double dt2, hdt, c12;
  double* b;
  const double* m;
  const double* u;
  const double* up;
  double* us;
  double* w;
  BoundaryPlanDev bc;   // s1 = the coefficient of the Gamma_1 term at the current time; s2 is folded into hdt
};

__device__ __forceinline__ double leapfrog4_w_plain(double b, double m, double c12)
{
#pragma clang fp contract(off)
  return c12 * (b / m);
}
__device__ __forceinline__ double leapfrog4_w_boundary(double b, double m, double c12, double s1, double c1)
{
#pragma clang fp contract(off)
  return c12 * ((b + s1 * c1) / m);
}

template <bool BC, int VEC, bool NT>
__device__ __forceinline__ void leapfrog4_predict_entry(const Leapfrog4PredictArgs& a, Lanes<VEC, NT> io, int64_t g)
{
  using L = Lanes<VEC, NT>;
  using V = typename L::V;
  const double dt2 = a.dt2, c12 = a.c12;
  const V bb = io.ldnt(a.b, g), mm = io.ldnt(a.m, g), uu = io.ld(a.u, g), pp = io.ldnt(a.up, g);
  V ss, ww, zero;
  for (int l = 0; l < VEC; ++l) {
    L::at(ss, l) = leapfrog_plain(L::at(bb, l), L::at(mm, l), L::at(uu, l), L::at(pp, l), dt2);
    L::at(ww, l) = leapfrog4_w_plain(L::at(bb, l), L::at(mm, l), c12);
    L::at(zero, l) = 0.0;
  }
  if constexpr (BC) {
    const BoundaryPlanDev& bc = a.bc;
    for_boundary_dofs<VEC>(bc, io.off + (int64_t)VEC * g, [&](int lane, int64_t r) {
      const double c1 = bc.c1[r];
      L::at(ss, lane) = leapfrog_boundary(L::at(bb, lane), L::at(mm, lane), L::at(uu, lane), L::at(pp, lane), dt2, a.hdt, bc.s1, c1,
                                          bc.c2[r]);
      L::at(ww, lane) = leapfrog4_w_boundary(L::at(bb, lane), L::at(mm, lane), c12, bc.s1, c1);
    });
  }
  io.stnt(a.us, g, ss);
  io.st(a.w, g, ww);
  io.st(a.b, g, zero);
}

template <int VEC, bool NT, bool BC>
__global__ void __launch_bounds__(256) k_leapfrog4_predict(int64_t nvec, int ntail, Leapfrog4PredictArgs a)
{
  sweep<VEC, NT>(nvec, ntail, WF_SWEEP_THREAD, [&](auto io, int64_t g) { leapfrog4_predict_entry<BC>(a, io, g); });
}

struct Leapfrog4CorrectArgs {
  double dt2, hdt, tdt;
  double* b;
  const double* m;
  const double* us;
  const double* up;
  double* un;
  double* v;
  BoundaryPlanDev bc;   // s1 = s1c, the second difference of the Gamma_1 coefficient over 12; s2 is folded into hdt
};

__device__ __forceinline__ double leapfrog4_correct_plain(double b, double m, double us, double dt2)
{
#pragma clang fp contract(off)
  return us + dt2 * (b / m);
}
__device__ __forceinline__ double leapfrog4_correct_boundary(double b, double m, double us, double dt2, double hdt, double s1c, double c1,
                                                             double c2)
{
#pragma clang fp contract(off)
  const double h = hdt * c2;
  return us + (dt2 * (b + s1c * c1)) / (m + h);
}

template <bool BC, bool HAS_V, int VEC, bool NT>
__device__ __forceinline__ void leapfrog4_correct_entry(const Leapfrog4CorrectArgs& a, Lanes<VEC, NT> io, int64_t g)
{
  using L = Lanes<VEC, NT>;
  using V = typename L::V;
  const double dt2 = a.dt2;
  const V bb = io.ldnt(a.b, g), mm = io.ldnt(a.m, g), ss = io.ldnt(a.us, g);
  V nn, zero;
  for (int l = 0; l < VEC; ++l) {
    L::at(nn, l) = leapfrog4_correct_plain(L::at(bb, l), L::at(mm, l), L::at(ss, l), dt2);
    L::at(zero, l) = 0.0;
  }
  if constexpr (BC) {
    const BoundaryPlanDev& bc = a.bc;
    for_boundary_dofs<VEC>(bc, io.off + (int64_t)VEC * g, [&](int lane, int64_t r) {
      L::at(nn, lane) = leapfrog4_correct_boundary(L::at(bb, lane), L::at(mm, lane), L::at(ss, lane), dt2, a.hdt, bc.s1, bc.c1[r], bc.c2[r]);
    });
  }
  if constexpr (HAS_V) {
    const V pp = io.ldnt(a.up, g);
    V w;
    for (int l = 0; l < VEC; ++l) L::at(w, l) = (L::at(nn, l) - L::at(pp, l)) / a.tdt;
    io.stnt(a.v, g, w);
  }
  io.st(a.un, g, nn);
  io.st(a.b, g, zero);
}

template <int VEC, bool NT, bool BC, bool HAS_V>
__global__ void __launch_bounds__(256) k_leapfrog4_correct(int64_t nvec, int ntail, Leapfrog4CorrectArgs a)
{
  sweep<VEC, NT>(nvec, ntail, WF_SWEEP_THREAD, [&](auto io, int64_t g) { leapfrog4_correct_entry<BC, HAS_V>(a, io, g); });
}

}  // namespace wf

struct wf_boundary {
  int64_t n = 0;
  int32_t nb = 0, n1 = 0, n2 = 0;
  wf::DevArray<unsigned long long> d_mask;
  wf::DevArray<uint32_t> d_prefix;
  wf::DevArray<double> d_c1, d_c2;
  // the plain index form as well (first right-hand side of a run, reference-order loop)
  wf::DevArray<int32_t> d_idx1, d_idx2;
  wf::DevArray<double> d_m1, d_m2;
};

namespace {

// the plan as the kernels read it; null or empty plan: none (the pass is then launched without BC)
wf::BoundaryPlanDev plan_dev(const wf_boundary* bc, double s1, double s2)
{
  wf::BoundaryPlanDev d;
  if (bc && bc->nb > 0) {
    d.mask = bc->d_mask.data();
    d.prefix = bc->d_prefix.data();
    d.c1 = bc->d_c1.data();
    d.c2 = bc->d_c2.data();
    d.s1 = s1;
    d.s2 = s2;
  }
  return d;
}

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, std::bool_constant<b2>{}): three run-time booleans as template
// arguments, the eight forms of a kernel behind one call
template <class F>
void with_bools(bool b0, bool b1, bool b2, F&& f)
{
  auto pick = [](bool b, auto&& g) { b ? g(std::true_type{}) : g(std::false_type{}); };
  pick(b0, [&](auto c0) { pick(b1, [&](auto c1) { pick(b2, [&](auto c2) { f(c0, c1, c2); }); }); });
}

int rk4_stage_impl(int64_t n, double bdt, double adt_next, int has_next, double* d_b, const double* d_m, const double* d_vn,
                   const double* d_u_read, const double* d_v_read, double* d_u, double* d_v, const double* d_u0,
                   const double* d_v0, double* d_un, double* d_vn_next, const wf_boundary* bcp, double s1_next, double s2,
                   void* stream)
{
  if (n <= 0) return WF_OK;
  WF_REQUIRE(d_b && d_m && d_vn && d_u_read && d_v_read && d_u && d_v, "wf_rk4_stage: null vector");
  WF_REQUIRE(!has_next || (d_u0 && d_v0 && d_un && d_vn_next), "wf_rk4_stage: next-stage vectors missing");
  WF_REQUIRE(!has_next || d_vn_next != d_vn, "wf_rk4_stage: vn_next must not alias vn");
  WF_REQUIRE(!bcp || bcp->n == n, "wf_rk4_stage_bc: the boundary plan was built for another vector length");
  wf::MarkerScope mk("wf_rk4_stage");
  const wf::StageArgs a{bdt, adt_next, d_b, d_m, d_vn, d_u_read, d_v_read, d_u, d_v, d_u0, d_v0, d_un, d_vn_next,
                        plan_dev(bcp, s1_next, s2)};
  // 16-byte sweep (streaming accesses for everything but un and b: 0.155 -> 0.135 ms at cfg2) with the odd last dof
  // in the same launch, or the scalar kernel for unaligned vectors
  const wf::SweepShape s = has_next ? wf::sweep_shape(n, d_b, d_m, d_vn, d_u_read, d_v_read, d_u, d_v, d_u0, d_v0, d_un, d_vn_next)
                                : wf::sweep_shape(n, d_b, d_m, d_vn, d_u_read, d_v_read, d_u, d_v);
  with_bools(s.vec, has_next != 0, a.bc.mask != nullptr, [&](auto vec, auto next, auto bc) {
    hipLaunchKernelGGL((wf::k_rk4_stage<vec() ? 2 : 1, next(), vec(), bc()>), dim3(s.grid), dim3(256), 0, (hipStream_t)stream, s.nvec,
                       s.ntail, a);
  });
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int leapfrog_step_impl(int64_t n, double dt, double* d_b, const double* d_m, const double* d_u, const double* d_u_prev,
                       double* d_u_next, double* d_v, const wf_boundary* bcp, double s1, double s2, void* stream)
{
  if (n <= 0) return WF_OK;
  WF_REQUIRE(d_b && d_m && d_u && d_u_prev && d_u_next, "wf_leapfrog_step: null vector");
  WF_REQUIRE(dt > 0.0, "wf_leapfrog_step: the time step must be positive");
  WF_REQUIRE(!(s2 > 0.0), "wf_leapfrog_step_bc: s2 > 0 is a negative absorbing coefficient");
  // two vectors of n entries that share memory (u_next and u_prev may be the same vector, not shifted ones)
  auto overlap = [n](const double* p, const double* q) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), c = reinterpret_cast<uintptr_t>(q), len = (uintptr_t)n * sizeof(double);
    return a < c + len && c < a + len;
  };
  WF_REQUIRE(!overlap(d_u_next, d_u) && !overlap(d_u_next, d_b) && !overlap(d_u_next, d_m),
             "wf_leapfrog_step: u_next must not alias u, b or m");
  WF_REQUIRE(d_u_next == d_u_prev || !overlap(d_u_next, d_u_prev), "wf_leapfrog_step: u_next overlaps u_prev without being u_prev");
  WF_REQUIRE(!d_v || (!overlap(d_v, d_b) && !overlap(d_v, d_m) && !overlap(d_v, d_u) && !overlap(d_v, d_u_prev)
                      && !overlap(d_v, d_u_next)),
             "wf_leapfrog_step: v must not alias another vector of the call");
  WF_REQUIRE(!bcp || bcp->n == n, "wf_leapfrog_step_bc: the boundary plan was built for another vector length");
  wf::MarkerScope mk("wf_leapfrog_step");
  // s2 enters through hdt
  const wf::LeapfrogArgs a{dt * dt, (-s2) * (0.5 * dt), 2.0 * dt, d_b, d_m, d_u, d_u_prev, d_u_next, d_v, plan_dev(bcp, s1, 0.0)};
  const wf::SweepShape s = wf::sweep_shape(n, d_b, d_m, d_u, d_u_prev, d_u_next, d_v);
  with_bools(s.vec, a.bc.mask != nullptr, d_v != nullptr, [&](auto vec, auto bc, auto has_v) {
    hipLaunchKernelGGL((wf::k_leapfrog_step<vec() ? 2 : 1, vec(), bc(), has_v()>), dim3(s.grid), dim3(256), 0, (hipStream_t)stream,
                       s.nvec, s.ntail, a);
  });
  WF_LAUNCH_CHECK();
  return WF_OK;
}

// two vectors of n entries that share memory
bool vectors_overlap(int64_t n, const double* p, const double* q)
{
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), c = reinterpret_cast<uintptr_t>(q), len = (uintptr_t)n * sizeof(double);
  return a < c + len && c < a + len;
}

}  // namespace

extern "C" {

int wf_leapfrog4_predict(int64_t n, double dt, double* d_b, const double* d_m, const double* d_u, const double* d_u_prev,
                         double* d_u_star, double* d_w, const wf_boundary* bcp, double s1, double s2, void* stream)
{
  if (n <= 0) return WF_OK;
  WF_REQUIRE(d_b && d_m && d_u && d_u_prev && d_u_star && d_w, "wf_leapfrog4_predict: null vector");
  WF_REQUIRE(dt > 0.0, "wf_leapfrog4_predict: the time step must be positive");
  WF_REQUIRE(!(s2 > 0.0), "wf_leapfrog4_predict: s2 > 0 is a negative absorbing coefficient");
  auto overlap = [n](const double* p, const double* q) { return vectors_overlap(n, p, q); };
  WF_REQUIRE(!overlap(d_u_star, d_u) && !overlap(d_u_star, d_b) && !overlap(d_u_star, d_m),
             "wf_leapfrog4_predict: u_star must not alias u, b or m");
  WF_REQUIRE(d_u_star == d_u_prev || !overlap(d_u_star, d_u_prev), "wf_leapfrog4_predict: u_star overlaps u_prev without being u_prev");
  WF_REQUIRE(!overlap(d_w, d_b) && !overlap(d_w, d_m) && !overlap(d_w, d_u) && !overlap(d_w, d_u_prev) && !overlap(d_w, d_u_star),
             "wf_leapfrog4_predict: w must not alias another vector of the call");
  WF_REQUIRE(!bcp || bcp->n == n, "wf_leapfrog4_predict: the boundary plan was built for another vector length");
  wf::MarkerScope mk("wf_leapfrog4_predict");
  const double dt2 = dt * dt;
  const wf::Leapfrog4PredictArgs a{dt2, (-s2) * (0.5 * dt), dt2 / 12.0, d_b, d_m, d_u, d_u_prev, d_u_star, d_w, plan_dev(bcp, s1, 0.0)};
  const wf::SweepShape s = wf::sweep_shape(n, d_b, d_m, d_u, d_u_prev, d_u_star, d_w);
  with_bools(s.vec, a.bc.mask != nullptr, false, [&](auto vec, auto bc, auto) {
    hipLaunchKernelGGL((wf::k_leapfrog4_predict<vec() ? 2 : 1, vec(), bc()>), dim3(s.grid), dim3(256), 0, (hipStream_t)stream, s.nvec,
                       s.ntail, a);
  });
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int wf_leapfrog4_correct(int64_t n, double dt, double* d_b, const double* d_m, const double* d_u_star, const double* d_u_prev,
                         double* d_u_next, double* d_v, const wf_boundary* bcp, double s1c, double s2, void* stream)
{
  if (n <= 0) return WF_OK;
  WF_REQUIRE(d_b && d_m && d_u_star && d_u_next, "wf_leapfrog4_correct: null vector");
  WF_REQUIRE(!d_v || d_u_prev, "wf_leapfrog4_correct: v needs u_prev");
  WF_REQUIRE(dt > 0.0, "wf_leapfrog4_correct: the time step must be positive");
  WF_REQUIRE(!(s2 > 0.0), "wf_leapfrog4_correct: s2 > 0 is a negative absorbing coefficient");
  auto overlap = [n](const double* p, const double* q) { return vectors_overlap(n, p, q); };
  WF_REQUIRE(!overlap(d_u_next, d_b) && !overlap(d_u_next, d_m), "wf_leapfrog4_correct: u_next must not alias b or m");
  WF_REQUIRE(d_u_next == d_u_star || !overlap(d_u_next, d_u_star), "wf_leapfrog4_correct: u_next overlaps u_star without being u_star");
  WF_REQUIRE(!overlap(d_u_star, d_b) && !overlap(d_u_star, d_m), "wf_leapfrog4_correct: u_star must not alias b or m");
  WF_REQUIRE(!d_v || (!overlap(d_u_prev, d_u_next) && !overlap(d_u_prev, d_b) && !overlap(d_u_prev, d_u_star)),
             "wf_leapfrog4_correct: u_prev must not alias u_next, u_star or b");
  WF_REQUIRE(!d_v || (!overlap(d_v, d_b) && !overlap(d_v, d_m) && !overlap(d_v, d_u_star) && !overlap(d_v, d_u_prev)
                      && !overlap(d_v, d_u_next)),
             "wf_leapfrog4_correct: v must not alias another vector of the call");
  WF_REQUIRE(!bcp || bcp->n == n, "wf_leapfrog4_correct: the boundary plan was built for another vector length");
  wf::MarkerScope mk("wf_leapfrog4_correct");
  const double* const up = d_v ? d_u_prev : nullptr;          // not read without v, so not asked to be aligned either
  const wf::Leapfrog4CorrectArgs a{dt * dt, (-s2) * (0.5 * dt), 2.0 * dt, d_b, d_m, d_u_star, up, d_u_next, d_v, plan_dev(bcp, s1c, 0.0)};
  const wf::SweepShape s = wf::sweep_shape(n, d_b, d_m, d_u_star, up, d_u_next, d_v);
  with_bools(s.vec, a.bc.mask != nullptr, d_v != nullptr, [&](auto vec, auto bc, auto has_v) {
    hipLaunchKernelGGL((wf::k_leapfrog4_correct<vec() ? 2 : 1, vec(), bc(), has_v()>), dim3(s.grid), dim3(256), 0, (hipStream_t)stream,
                       s.nvec, s.ntail, a);
  });
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int wf_leapfrog_step(int64_t n, double dt, double* d_b, const double* d_m, const double* d_u, const double* d_u_prev,
                     double* d_u_next, double* d_v, void* stream)
{
  return leapfrog_step_impl(n, dt, d_b, d_m, d_u, d_u_prev, d_u_next, d_v, nullptr, 0.0, 0.0, stream);
}

int wf_leapfrog_step_bc(int64_t n, double dt, double* d_b, const double* d_m, const double* d_u, const double* d_u_prev,
                        double* d_u_next, double* d_v, const wf_boundary* bc, double s1, double s2, void* stream)
{
  WF_REQUIRE(bc != nullptr, "wf_leapfrog_step_bc: null boundary plan");
  return leapfrog_step_impl(n, dt, d_b, d_m, d_u, d_u_prev, d_u_next, d_v, bc, s1, s2, stream);
}

int wf_rk4_stage(int64_t n, double bdt, double adt_next, int has_next, double* d_b, const double* d_m,
                 const double* d_vn, const double* d_u_read, const double* d_v_read, double* d_u, double* d_v,
                 const double* d_u0, const double* d_v0, double* d_un, double* d_vn_next, void* stream)
{
  return rk4_stage_impl(n, bdt, adt_next, has_next, d_b, d_m, d_vn, d_u_read, d_v_read, d_u, d_v, d_u0, d_v0, d_un, d_vn_next,
                        nullptr, 0.0, 0.0, stream);
}

int wf_rk4_stage_bc(int64_t n, double bdt, double adt_next, int has_next, double* d_b, const double* d_m,
                    const double* d_vn, const double* d_u_read, const double* d_v_read, double* d_u, double* d_v,
                    const double* d_u0, const double* d_v0, double* d_un, double* d_vn_next, const wf_boundary* bc,
                    double s1_next, double s2, void* stream)
{
  WF_REQUIRE(bc != nullptr, "wf_rk4_stage_bc: null boundary plan");
  return rk4_stage_impl(n, bdt, adt_next, has_next, d_b, d_m, d_vn, d_u_read, d_v_read, d_u, d_v, d_u0, d_v0, d_un, d_vn_next, bc,
                        s1_next, s2, stream);
}

int wf_boundary_destroy(wf_boundary* bc)
{
  delete bc;
  return WF_OK;
}

int wf_boundary_create(int64_t n, int32_t n1, const int32_t* h_idx1, const double* h_m1, int32_t n2, const int32_t* h_idx2,
                       const double* h_m2, wf_boundary** out)
{
  WF_REQUIRE(out && n >= 0 && n1 >= 0 && n2 >= 0, "wf_boundary_create: bad argument");
  *out = nullptr;
  WF_REQUIRE((n1 == 0 || (h_idx1 && h_m1)) && (n2 == 0 || (h_idx2 && h_m2)), "wf_boundary_create: null array");
  int rc;
  if ((rc = wf::check_index_range(h_idx1, (size_t)n1, n, "wf_boundary_create: index out of range")) != WF_OK) return rc;
  if ((rc = wf::check_index_range(h_idx2, (size_t)n2, n, "wf_boundary_create: index out of range")) != WF_OK) return rc;
  const size_t nw = (size_t)((n + 63) / 64) + 1;   // + 1: the 16-byte sweeps read two words per wave
  std::vector<unsigned long long> mask(nw, 0ull);
  for (int32_t i = 0; i < n1; ++i) mask[h_idx1[i] >> 6] |= 1ull << (h_idx1[i] & 63);
  for (int32_t i = 0; i < n2; ++i) mask[h_idx2[i] >> 6] |= 1ull << (h_idx2[i] & 63);
  std::vector<uint32_t> prefix(nw, 0u);
  uint32_t run = 0;
  for (size_t w = 0; w < nw; ++w) {
    prefix[w] = run;
    run += (uint32_t)__builtin_popcountll(mask[w]);
  }
  const int32_t nb = (int32_t)run;
  auto rank = [&](int32_t d) {
    return (size_t)prefix[d >> 6] + (size_t)__builtin_popcountll(mask[d >> 6] & ((1ull << (d & 63)) - 1ull));
  };
  std::vector<double> c1((size_t)nb, 0.0), c2((size_t)nb, 0.0);
  for (int32_t i = 0; i < n1; ++i) c1[rank(h_idx1[i])] += h_m1[i];   // a repeated index accumulates, like wf_boundary_apply
  for (int32_t i = 0; i < n2; ++i) c2[rank(h_idx2[i])] += h_m2[i];
  auto bc = std::make_unique<wf_boundary>();
  bc->n = n;
  bc->nb = nb;
  bc->n1 = n1;
  bc->n2 = n2;
  if ((rc = bc->d_mask.upload(mask)) != WF_OK || (rc = bc->d_prefix.upload(prefix)) != WF_OK
      || (rc = bc->d_c1.upload(c1)) != WF_OK || (rc = bc->d_c2.upload(c2)) != WF_OK
      || (rc = bc->d_idx1.upload(h_idx1, (size_t)n1)) != WF_OK || (rc = bc->d_m1.upload(h_m1, (size_t)n1)) != WF_OK
      || (rc = bc->d_idx2.upload(h_idx2, (size_t)n2)) != WF_OK || (rc = bc->d_m2.upload(h_m2, (size_t)n2)) != WF_OK)
    return rc;
  *out = bc.release();
  return WF_OK;
}

// b[idx1[i]] += s1 m1[i]; b[idx2[i]] += s2 m2[i] v[idx2[i]] from a plan (the first right-hand side of a fused run)
int wf_boundary_apply_plan(const wf_boundary* bc, double s1, double s2, const double* d_v, double* d_b, void* stream)
{
  WF_REQUIRE(bc && d_v && d_b, "wf_boundary_apply_plan: null argument");
  return wf_boundary_apply(bc->n1, bc->d_idx1.data(), bc->d_m1.data(), s1, bc->n2, bc->d_idx2.data(), bc->d_m2.data(), s2, d_v, d_b,
                           stream);
}

int wf_boundary_apply(int32_t n1, const int32_t* d_idx1, const double* d_m1, double s1, int32_t n2,
                      const int32_t* d_idx2, const double* d_m2, double s2, const double* d_v, double* d_b,
                      void* stream)
{
  const int64_t n = (int64_t)n1 + n2;
  if (n <= 0) return WF_OK;
  hipLaunchKernelGGL(wf::k_boundary, dim3(wf::capped_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, n1, d_idx1, d_m1,
                     s1, n2, d_idx2, d_m2, s2, d_v, d_b);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

}  // extern "C"
