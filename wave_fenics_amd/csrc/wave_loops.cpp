// The time loops of the wave model, rk4_fused, leapfrog and leapfrog4, once: host code over the library's own entries (no HIP
// in here; wave_source.h holds the plane source).  The Python and the C++ LinearGLLOpt both call these.  Every launch
// goes to the caller's stream; nothing is allocated, freed or synchronised.
#include <algorithm>
#include <cstdint>
#include <string>

#include "wave_source.h"
#include "wavehip.h"

namespace wf {
void set_error(const std::string& msg);                     // tables.cpp
}

namespace {

// by scheme; WF_WAVE_LEAPFROG4: u^n, u^{n-1}, the corrector's operand, a scratch
constexpr int kWorkVectors[3] = {7, 3, 4};
constexpr double a_runge[4] = {0.0, 0.5, 0.5, 1.0};
constexpr double b_runge[4] = {1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0};
constexpr double c_runge[4] = {0.0, 0.5, 0.5, 1.0};

bool limit_reached(int64_t step, int64_t max_steps) { return max_steps >= 0 && step >= max_steps; }

// t + c dt as a product and then a sum, in two statements (two roundings: contracted to a fused multiply-add within one
// expression it would give other bits)
double stage_time(double t, double c, double dt)
{
  const double cdt = c * dt;
  return t + cdt;
}

#define WF_TRY(call)                     \
  do {                                   \
    if (int _rc = (call)) return _rc;    \
  } while (0)

#define WF_REFUSE_UNLESS(cond, msg)      \
  do {                                   \
    if (!(cond)) {                       \
      wf::set_error(msg);                \
      return WF_ERR_INVALID;             \
    }                                    \
  } while (0)

int check_call(const std::string& who, int scheme, const wf_wave_desc* d, double t0, double tf, double dt, int64_t max_steps,
               const double* d_u, const double* d_v)
{
  WF_REFUSE_UNLESS(d, who + ": null descriptor");
  WF_REFUSE_UNLESS(d->n >= 0, who + ": n < 0");
  WF_REFUSE_UNLESS(d_u && d_v, who + ": null state");
  WF_REFUSE_UNLESS(d->d_work, who + ": null work");
  for (int k = 0; k < kWorkVectors[scheme]; ++k) WF_REFUSE_UNLESS(d->d_work[k], who + ": null work");
  WF_REFUSE_UNLESS(d->d_m && d->d_b && d->bc, who + ": null m, b or boundary plan");
  WF_REFUSE_UNLESS(d->rhs || d->op, who + ": needs an operator handle or a right-hand-side callback");
  WF_REFUSE_UNLESS(d->rhs || !d->overlapped || d->updater, who + ": overlapped needs an updater");
  WF_REFUSE_UNLESS(dt > 0.0, who + ": the time step must be positive");
  WF_REFUSE_UNLESS(!d->receivers || d->d_traces, who + ": receivers without a trace buffer");
  WF_REFUSE_UNLESS(!(d->receivers || d->h_times) || d->trace_rows > wf_wave_step_count(scheme, t0, tf, dt, max_steps),
                   who + ": the trace buffer has fewer rows than steps + 1");
  return WF_OK;
}

// what a loop reads from its descriptor on every pass
struct Loop {
  const wf_wave_desc& d;
  void* s;
  int64_t npoints = 0;

  int init()
  {
    int np = 0;
    if (d.receivers) WF_TRY(wf_points_info(d.receivers, &np, nullptr, nullptr));
    npoints = np;
    return WF_OK;
  }
  // b += K x with the ghost exchange of a partitioned mesh around it: forward halo of x, reverse halo of b
  int rhs(double* x) const
  {
    if (d.rhs) {
      const int rc = d.rhs(d.rhs_user, x, d.d_b, s);
      if (rc != WF_OK) wf::set_error("wf_wave: right-hand-side callback failed");
      return rc;
    }
    // interior cells beside the halo of x, the interface cells and the reverse halo of b
    if (d.overlapped) return wf_op_apply_overlapped(d.op, d.updater, x, d.d_b, s);
    if (d.updater) WF_TRY(wf_updater_fwd(d.updater, x, s));
    WF_TRY(wf_op_apply(d.op, x, d.d_b, s));
    return d.updater ? wf_updater_rev(d.updater, d.d_b, s) : WF_OK;
  }
  int add_sources(double t) const { return d.sources ? wf_sources_add(d.sources, t, d.d_b, s) : WF_OK; }
  // b += the point sources' sum over nt times with weights (a difference quotient of the load)
  int add_stencil(int nt, const double* times, const double* weights) const
  {
    return d.sources ? wf_sources_add_stencil(d.sources, nt, times, weights, d.d_b, s) : WF_OK;
  }
  // row `row` of the traces: u at the receivers, at time t
  int record(const double* u, int64_t row, double t) const
  {
    if (d.h_times) d.h_times[row] = t;
    return d.receivers ? wf_points_sample(d.receivers, u, d.d_traces + row * npoints, s) : WF_OK;
  }
};

}  // namespace

extern "C" {

double wf_wave_window(const wf_wave_source* p, double t) { return wf::wave_window(*p, t); }
double wf_wave_g(const wf_wave_source* p, double t) { return wf::wave_g(*p, wf::wave_window(*p, t), t); }
double wf_wave_s1(const wf_wave_source* p, double t) { return wf::wave_s1(*p, t); }
double wf_wave_s1_left_to_right(const wf_wave_source* p, double t) { return wf::wave_s1_left_to_right(*p, t); }
double wf_wave_s2(const wf_wave_source* p) { return wf::wave_s2(*p); }

int wf_wave_work_vectors(int scheme) { return scheme >= WF_WAVE_RK4_FUSED && scheme <= WF_WAVE_LEAPFROG4 ? kWorkVectors[scheme] : -1; }

int64_t wf_wave_step_count(int scheme, double t0, double tf, double dt, int64_t max_steps)
{
  double t = t0;
  int64_t step = 0;
  while (t < tf) {
    if (scheme == WF_WAVE_RK4_FUSED) dt = std::min(dt, tf - t);
    t += dt;
    step += 1;
    if (limit_reached(step, max_steps) || !(dt > 0.0)) break;   // a step that does not advance would count for ever
  }
  return step;
}

int wf_wave_rk4_fused(const wf_wave_desc* desc, double t0, double tf, double dt, int64_t max_steps, double* d_u, double* d_v,
                      double* t_end, int64_t* steps, void* stream)
{
  WF_TRY(check_call("wf_wave_rk4_fused", WF_WAVE_RK4_FUSED, desc, t0, tf, dt, max_steps, d_u, d_v));
  const wf_wave_desc& d = *desc;
  Loop L{d, stream};
  WF_TRY(L.init());
  const int64_t n = d.n;
  double* const b = d.d_b;
  const double* const m = d.d_m;
  const bool fold = d.fold_boundary != 0;
  double *u0 = d.d_work[0], *v0 = d.d_work[1];                // solution at the start of the step
  double *u_ = d.d_work[2], *v_ = d.d_work[3];                // running solution of the step
  double *const un = d.d_work[4], *const vn_a = d.d_work[5], *const vn_b = d.d_work[6];
  const double s2 = wf::wave_s2(d.source);
  auto s1 = [&](double t) { return wf::wave_s1_left_to_right(d.source, t); };
  double t = t0;
  int64_t step = 0;
  WF_TRY(wf_copy(n, d_u, u0, stream));
  WF_TRY(wf_copy(n, d_v, v0, stream));
  WF_TRY(wf_fill(n, 0.0, b, stream));
  // boundary term of the first right-hand side; the stage kernels leave the others
  WF_TRY(wf_boundary_apply_plan(d.bc, s1(t), s2, v0, b, stream));
  WF_TRY(L.add_sources(t));                                   // likewise the point sources: a launch after each stage kernel
  WF_TRY(L.record(u0, 0, t));
  while (t < tf) {
    dt = std::min(dt, tf - t);
    // stage 0: un = u0, vn = v0 (a_0 = 0), read straight from u0 / v0
    double *x_u = u0, *x_v = v0, *vn_next = vn_a;
    for (int i = 0; i < 4; ++i) {
      WF_TRY(L.rhs(x_u));                                     // b holds the boundary term of this right-hand side on entry
      const bool last = i == 3;
      const double *ur = i == 0 ? u0 : u_, *vr = i == 0 ? v0 : v_;
      // the next right-hand side: the next stage, or stage 0 of the next step (v = the updated solution, time t + dt;
      // after the last step b is left holding a boundary term nobody reads)
      const double tn = last ? t + dt : stage_time(t, c_runge[i + 1], dt);
      const double adt = last ? 0.0 : dt * a_runge[i + 1];
      double* const v_next = last ? v_ : vn_next;
      if (fold) {
        WF_TRY(wf_rk4_stage_bc(n, dt * b_runge[i], adt, !last, b, m, x_v, ur, vr, u_, v_, last ? nullptr : u0, last ? nullptr : v0,
                               last ? nullptr : un, last ? nullptr : vn_next, d.bc, s1(tn), s2, stream));
      } else {
        WF_TRY(wf_rk4_stage(n, dt * b_runge[i], adt, !last, b, m, x_v, ur, vr, u_, v_, last ? nullptr : u0, last ? nullptr : v0,
                            last ? nullptr : un, last ? nullptr : vn_next, stream));
        WF_TRY(wf_boundary_apply_plan(d.bc, s1(tn), s2, v_next, b, stream));
      }
      WF_TRY(L.add_sources(tn));
      if (!last) {
        x_u = un, x_v = vn_next;
        vn_next = vn_next == vn_a ? vn_b : vn_a;
      }
    }
    std::swap(u0, u_);                                        // the new solution becomes the next step's u0
    std::swap(v0, v_);
    t += dt;
    step += 1;
    WF_TRY(L.record(u0, step, t));
    if (limit_reached(step, max_steps)) break;
  }
  WF_TRY(wf_copy(n, u0, d_u, stream));
  WF_TRY(wf_copy(n, v0, d_v, stream));
  if (t_end) *t_end = t;
  if (steps) *steps = step;
  return WF_OK;
}

int wf_wave_leapfrog(const wf_wave_desc* desc, double t0, double tf, double dt, int64_t max_steps, double* d_u, double* d_v,
                     wf_wave_step_fn before_step, void* before_step_user, double* t_end, int64_t* steps, void* stream)
{
  WF_TRY(check_call("wf_wave_leapfrog", WF_WAVE_LEAPFROG, desc, t0, tf, dt, max_steps, d_u, d_v));
  const wf_wave_desc& d = *desc;
  Loop L{d, stream};
  WF_TRY(L.init());
  const int64_t n = d.n;
  double* const b = d.d_b;
  const double* const m = d.d_m;
  double *u = d.d_work[0], *w = d.d_work[1];                  // u^n; u^{n-1}, overwritten in place by u^{n+1}
  double* const scratch = d.d_work[2];
  const double s2 = wf::wave_s2(d.source);
  auto s1 = [&](double t) { return wf::wave_s1(d.source, t); };
  double t = t0;
  int64_t step = 0;
  WF_TRY(wf_copy(n, d_u, u, stream));
  // start-up: scratch = a^0, w = u^{-1}
  WF_TRY(wf_fill(n, 0.0, b, stream));
  WF_TRY(L.rhs(u));
  WF_TRY(wf_boundary_apply_plan(d.bc, s1(t), s2, d_v, b, stream));
  WF_TRY(L.add_sources(t));
  WF_TRY(L.record(u, 0, t));
  WF_TRY(wf_pointwise_div(n, b, m, scratch, stream));
  WF_TRY(wf_axpy(n, -dt, d_v, u, w, stream));
  WF_TRY(wf_axpy(n, 0.5 * dt * dt, scratch, w, w, stream));
  WF_TRY(wf_fill(n, 0.0, b, stream));
  while (t < tf) {
    if (before_step && before_step(before_step_user, step, t, w, u, scratch, stream) != WF_OK) {
      wf::set_error("wf_wave_leapfrog: per-step callback failed");
      return WF_ERR_INVALID;
    }
    WF_TRY(L.rhs(u));                                         // b is zero on entry
    WF_TRY(L.add_sources(t));
    WF_TRY(wf_leapfrog_step_bc(n, dt, b, m, u, w, w, nullptr, d.bc, s1(t), s2, stream));
    std::swap(u, w);
    t += dt;
    step += 1;
    WF_TRY(L.record(u, step, t));
    if (limit_reached(step, max_steps)) break;
  }
  // finish: the step after the last one, into scratch, for the central velocity at t
  WF_TRY(L.rhs(u));
  WF_TRY(L.add_sources(t));
  WF_TRY(wf_leapfrog_step_bc(n, dt, b, m, u, w, scratch, d_v, d.bc, s1(t), s2, stream));
  WF_TRY(wf_copy(n, u, d_u, stream));
  if (t_end) *t_end = t;
  if (steps) *steps = step;
  return WF_OK;
}

int wf_wave_leapfrog4(const wf_wave_desc* desc, double t0, double tf, double dt, int64_t max_steps, double* d_u, double* d_v,
                      wf_wave_step_fn before_step, void* before_step_user, double* const* d_startup, double* t_end,
                      int64_t* steps, void* stream)
{
  WF_TRY(check_call("wf_wave_leapfrog4", WF_WAVE_LEAPFROG4, desc, t0, tf, dt, max_steps, d_u, d_v));
  for (int k = 0; d_startup && k < 3; ++k) WF_REFUSE_UNLESS(d_startup[k], "wf_wave_leapfrog4: null start-up vector");
  // the start-up derivative just formed in `from`, for the caller (the discrete adjoint reads a0, j0, q0)
  auto keep_startup = [&](int k, const double* from) { return d_startup ? wf_copy(desc->n, from, d_startup[k], stream) : WF_OK; };
  const wf_wave_desc& d = *desc;
  Loop L{d, stream};
  WF_TRY(L.init());
  const int64_t n = d.n;
  double* const b = d.d_b;
  const double* const m = d.d_m;
  double *u = d.d_work[0], *p = d.d_work[1];                  // u^n; u^{n-1}, overwritten in place by u* and then u^{n+1}
  double *const w = d.d_work[2], *const scratch = d.d_work[3];
  const double s2 = wf::wave_s2(d.source);
  const double dt2 = dt * dt;
  auto s1 = [&](double t) { return wf::wave_s1(d.source, t); };
  // central differences of the plane source's coefficient over t +- dt: first and second derivative, and the second
  // difference over 12 of the corrector
  auto s1_d1 = [&](double t) { return (s1(t + dt) - s1(t - dt)) / (2.0 * dt); };
  auto s1_dd = [&](double t) { return (s1(t + dt) - 2.0 * s1(t)) + s1(t - dt); };
  // the same differences of the point sources, onto b
  auto sources_d1 = [&](double t) {
    const double ts[2] = {t - dt, t + dt}, as[2] = {-1.0 / (2.0 * dt), 1.0 / (2.0 * dt)};
    return L.add_stencil(2, ts, as);
  };
  auto sources_dd = [&](double t, double scale) {
    const double ts[3] = {t - dt, t, t + dt}, as[3] = {scale, -2.0 * scale, scale};
    return L.add_stencil(3, ts, as);
  };
  // one step from (u, prev) at time t: u* and then u^{n+1} into `star` (prev itself, or another vector), v if asked for
  auto advance = [&](double t, const double* prev, double* star, double* v) {
    WF_TRY(L.rhs(u));                                         // b is zero on entry
    WF_TRY(L.add_sources(t));
    WF_TRY(wf_leapfrog4_predict(n, dt, b, m, u, prev, star, w, d.bc, s1(t), s2, stream));
    WF_TRY(L.rhs(w));
    WF_TRY(sources_dd(t, 1.0 / 12.0));
    return wf_leapfrog4_correct(n, dt, b, m, star, prev, star, v, d.bc, s1_dd(t) / 12.0, s2, stream);
  };
  double t = t0;
  int64_t step = 0;
  WF_TRY(wf_copy(n, d_u, u, stream));
  WF_TRY(L.record(u, 0, t));
  // start-up: a^0 in w, j^0 in scratch, q^0 in w; p = u^{-1} by its Taylor series to dt^4
  // (the boundary term goes onto the zeroed b in front of the apply, as in wf_wave_rk4_fused: wf_boundary_apply adds by
  // atomics, and a dof of both sets takes its two terms in either order -- onto zero that order cannot show)
  WF_TRY(wf_fill(n, 0.0, b, stream));
  WF_TRY(wf_boundary_apply_plan(d.bc, s1(t), s2, d_v, b, stream));
  WF_TRY(L.add_sources(t));
  WF_TRY(L.rhs(u));
  WF_TRY(wf_pointwise_div(n, b, m, w, stream));
  WF_TRY(keep_startup(0, w));
  WF_TRY(wf_axpy(n, -dt, d_v, u, p, stream));
  WF_TRY(wf_axpy(n, 0.5 * dt2, w, p, p, stream));
  WF_TRY(wf_fill(n, 0.0, b, stream));
  WF_TRY(wf_boundary_apply_plan(d.bc, s1_d1(t), s2, w, b, stream));
  WF_TRY(sources_d1(t));
  WF_TRY(L.rhs(d_v));
  WF_TRY(wf_pointwise_div(n, b, m, scratch, stream));
  WF_TRY(keep_startup(1, scratch));
  WF_TRY(wf_axpy(n, -(dt2 * dt) / 6.0, scratch, p, p, stream));
  WF_TRY(wf_fill(n, 0.0, b, stream));
  WF_TRY(wf_boundary_apply_plan(d.bc, s1_dd(t) / dt2, s2, scratch, b, stream));
  WF_TRY(sources_dd(t, 1.0 / dt2));
  WF_TRY(L.rhs(w));                                           // K a^0 accumulates onto the loads; a^0 is then free
  WF_TRY(wf_pointwise_div(n, b, m, w, stream));
  WF_TRY(keep_startup(2, w));
  WF_TRY(wf_axpy(n, (dt2 * dt2) / 24.0, w, p, p, stream));
  WF_TRY(wf_fill(n, 0.0, b, stream));
  while (t < tf) {
    if (before_step && before_step(before_step_user, step, t, p, u, d_startup ? d_startup[0] : nullptr, stream) != WF_OK) {
      wf::set_error("wf_wave_leapfrog4: per-step callback failed");
      return WF_ERR_INVALID;
    }
    WF_TRY(advance(t, p, p, nullptr));
    std::swap(u, p);
    t += dt;
    step += 1;
    WF_TRY(L.record(u, step, t));
    if (limit_reached(step, max_steps)) break;
  }
  // finish: the step after the last one out of place, u^{n+1} in scratch and the central velocity in d_v; then the
  // central acceleration in scratch, j = (K v + L'(t) - d a) / m in w and v -= dt^2/6 j
  WF_TRY(advance(t, p, scratch, d_v));
  WF_TRY(wf_axpy(n, -2.0, u, scratch, scratch, stream));
  WF_TRY(wf_axpy(n, 1.0, p, scratch, scratch, stream));
  WF_TRY(wf_scale(n, 1.0 / dt2, scratch, stream));
  WF_TRY(wf_boundary_apply_plan(d.bc, s1_d1(t), s2, scratch, b, stream));   // the corrector left b zero
  WF_TRY(sources_d1(t));
  WF_TRY(L.rhs(d_v));
  WF_TRY(wf_pointwise_div(n, b, m, w, stream));
  WF_TRY(wf_axpy(n, -dt2 / 6.0, w, d_v, d_v, stream));
  WF_TRY(wf_fill(n, 0.0, b, stream));
  WF_TRY(wf_copy(n, u, d_u, stream));
  if (t_end) *t_end = t;
  if (steps) *steps = step;
  return WF_OK;
}

}  // extern "C"
