// wavehip_linear_gll.hpp -- C++ host driver of the explicit RK4 wave model:
// class LinearGLLOpt with the reference's member names and call sequence
// (common/LinearGLL.hpp:37-288), every vector on the device, every operation a
// libwavehip call.  The mesh/meshtags constructor arguments of the reference are
// replaced by either a BoxSpace plus the facet tag map (tag 1 = Gamma_1 source,
// tag 2 = Gamma_2 absorbing), or -- the mesh-FILE path of demo/cpu_planar3d/main.cpp:39-45 --
// a general Space plus the two tagged boundary dof sets (wavehip_mesh.hpp: read_mesh,
// create_functionspace, boundary_set); the FFCx form L (demo/cpu_planar3d/forms.ufl:19-24)
// is applied in its diagonal GLL form by wf_boundary_apply.
//
// Domain-decomposed runs pass a VectorUpdater (and the BoxPartition it was built
// from): scatter_fwd / scatter_rev(add) of LinearGLL.hpp:110,127,164,176,284-285
// become update_fwd / update_rev over RCCL, overlapped with the interior cells
// (wf_op_apply_overlapped).  The boundary term is applied by the owner of each
// boundary dof with the fully assembled facet mass, so the forward update of v
// (LinearGLL.hpp:167) is not needed.
#pragma once

#include <cmath>
#include <memory>

#include "wavehip_box.hpp"

namespace wavehip {

namespace kernels {
// kernels::copy / kernels::axpy of common/LinearGLL.hpp:15-35 on device arrays
inline void copy(const array<double>& in, array<double>& out) { check(wf_copy((std::int64_t)in.size(), in.data(), out.data(), nullptr)); }
inline void axpy(array<double>& r, double alpha, const array<double>& x, const array<double>& y, std::int64_t size_local)
{
  check(wf_axpy(size_local, alpha, x.data(), y.data(), r.data(), nullptr));
}
}  // namespace kernels

class LinearGLLOpt {
public:
  using BoundarySet = std::pair<std::vector<std::int32_t>, std::vector<double>>;   // dofs and their collocated facet masses

protected:
  int k_;        // degree of basis function
  double c0_;     // speed of sound (m/s)
  double freq0_;  // source frequency (Hz)
  double p0_;     // pressure amplitude (Pa)
  double w0_;     // angular frequency (rad/s)
  double T_;      // period (s)
  double alpha_;

  std::int64_t N_;  // vector length (owned + ghost), size_local on one rank
  std::unique_ptr<array<double>> m, b;
  std::unique_ptr<array<std::int32_t>> idx1, idx2;
  std::unique_ptr<array<double>> mG1, mG2;
  std::unique_ptr<detail::OpBase> stiff_op;
  wf_boundary* bc_ = nullptr;                  // the boundary sets as the fused passes read them (setup)
  VectorUpdater<double>* updater_ = nullptr;   // nullptr on one rank
  bool split_ = false;                         // interior / interface overlap available
  const Sources* sources_ = nullptr;           // point sources added to every right-hand side (set_sources)
  Receivers* receivers_ = nullptr;             // records u at the start time and after every step (set_receivers)
  void add_sources(double t)
  {
    if (sources_) sources_->add(t, b->data());
  }
  void record(const array<double>& u, double t)
  {
    if (receivers_) receivers_->record(u.data(), t);
  }

  /// the plane source as the library evaluates it (csrc/wave_source.h); c0 * c0 is this front end's own c0^2
  wf_wave_source wave() const { return wf_wave_source{c0_, c0_ * c0_, p0_, w0_, freq0_, alpha_, T_, 0}; }
  /// g(t) of LinearGLL.hpp:153-162
  double source(double t) const
  {
    const wf_wave_source w = wave();
    return wf_wave_g(&w, t);
  }
  /// the two scalars of the boundary term b[idx1] += s1 mG1, b[idx2] += s2 mG2 v (LinearGLL.hpp:175) at time t
  double s1(double t) const
  {
    const wf_wave_source w = wave();
    return wf_wave_s1(&w, t);
  }
  double s2() const
  {
    const wf_wave_source w = wave();
    return wf_wave_s2(&w);
  }
  void boundary(double t, const double* v)
  {
    check(wf_boundary_apply((std::int32_t)idx1->size(), idx1->data(), mG1->data(), s1(t), (std::int32_t)idx2->size(), idx2->data(),
                            mG2->data(), s2(), v, b->data(), nullptr));
  }
  /// b += K u (+ ghost exchange on a partitioned mesh); b is zero on entry
  void stiffness(double* u)
  {
    if (split_) {
      check(wf_op_apply_overlapped(stiff_op->handle(), updater_->handle(), u, b->data(), nullptr));
      return;
    }
    if (updater_) updater_->update_fwd(u);
    stiff_op->apply(u, b->data());
    if (updater_) updater_->update_rev(b->data());
  }

  void set_parameters(int degreeOfBasis, double speedOfSound, double sourceFrequency, double pressureAmplitude)
  {
    k_ = degreeOfBasis;
    c0_ = speedOfSound;
    freq0_ = sourceFrequency;
    p0_ = pressureAmplitude;
    w0_ = 2.0 * M_PI * freq0_;
    T_ = 1.0 / freq0_;
    alpha_ = 4.0;
  }
  template <class C>
  static auto upload(const C& h)
  {
    auto a = std::make_unique<array<typename C::value_type>>(h.size());
    a->set(h);
    return a;
  }
  /// What both constructors end with, stiff_op in place: the vectors, m = M 1 with scatter_rev(add) (LinearGLL.hpp:102-110;
  /// the forward update keeps the ghost entries of m consistent: b / m runs over the whole array), the boundary sets on
  /// the device with their plan for the fused passes (built here from the host sets, not on a loop's first call:
  /// wf_boundary_create allocates and copies synchronously) and the first stiffness apply (LinearGLL.hpp:120-127).
  void setup(detail::OpBase&& mass, const BoundarySet& gamma1, const BoundarySet& gamma2)
  {
    auto filled = [&](double value) {
      auto a = std::make_unique<array<double>>((std::size_t)N_);
      check(wf_fill(N_, value, a->data(), nullptr));
      return a;
    };
    u_n = filled(0.0);
    v_n = filled(0.0);
    m = filled(0.0);
    b = filled(0.0);
    const auto ones = filled(1.0);
    mass.apply(ones->data(), m->data());
    if (updater_) {
      updater_->update_rev(m->data());
      updater_->update_fwd(m->data());
    }
    check(wf_sync(nullptr));
    idx1 = upload(gamma1.first);
    mG1 = upload(gamma1.second);
    idx2 = upload(gamma2.first);
    mG2 = upload(gamma2.second);
    check(wf_boundary_create(N_, (std::int32_t)gamma1.first.size(), gamma1.first.data(), gamma1.second.data(),
                             (std::int32_t)gamma2.first.size(), gamma2.first.data(), gamma2.second.data(), &bc_));
    stiffness(u_n->data());
  }

public:
  const BoxSpace* V = nullptr;   // the box constructor's space (nullptr for the general-Space constructor)
  std::unique_ptr<array<double>> u_n, v_n;
  /// the lumped mass the loops divide by (assembled by atomics at creation: two models' may differ in the last bit)
  const array<double>& lumped_mass() const { return *m; }

  /// The mesh-file path (demo/cpu_planar3d/main.cpp:39-45, common/LinearGLL.hpp:53-128): any conforming
  /// hexahedral space plus the dof sets of Gamma_1 (source) and Gamma_2 (absorbing) with their collocated
  /// facet masses (wavehip_mesh.hpp boundary_set).  One rank.  tuning: the wf_tuning of the stiffness operator (read
  /// during construction only).
  LinearGLLOpt(const Space& S, const BoundarySet& gamma1, const BoundarySet& gamma2, int degreeOfBasis, double speedOfSound,
               double sourceFrequency, double pressureAmplitude, const wf_tuning* tuning = nullptr)
  {
    set_parameters(degreeOfBasis, speedOfSound, sourceFrequency, pressureAmplitude);
    N_ = S.ndofs;
    std::map<std::string, double> params{{"c0", c0_}};
    stiff_op = std::make_unique<StiffnessOperator<double>>(S, k_, params, tuning);
    setup(MassOperatorLumped<double>(S, k_), gamma1, gamma2);
  }

  LinearGLLOpt(const BoxSpace& V_, const std::map<int, int>& facet_tags, int degreeOfBasis, double speedOfSound,
               double sourceFrequency, double pressureAmplitude, VectorUpdater<double>* updater = nullptr,
               const BoxPartition* part = nullptr)
      : updater_(updater), V(&V_)
  {
    if (updater && !part) throw std::runtime_error("LinearGLLOpt: a VectorUpdater needs its BoxPartition");
    set_parameters(degreeOfBasis, speedOfSound, sourceFrequency, pressureAmplitude);
    N_ = V->ndofs();
    // LinearGLL.hpp:113-115: boundary form L
    auto facet = [&](int tag) {
      auto f = facet_lumped_mass(*V, facet_tags, tag);
      if (!updater_) return f;
      // accumulate the rank-local facet masses to their owners, keep owned dofs only
      std::vector<double> dense((std::size_t)N_, 0.0);
      for (std::size_t i = 0; i < f.first.size(); ++i) dense[f.first[i]] = f.second[i];
      array<double> d((std::size_t)N_);
      d.set(dense);
      updater_->update_rev(d.data());
      check(wf_sync(nullptr));
      dense = d.copy_to_host();
      std::pair<std::vector<std::int32_t>, std::vector<double>> out;
      for (std::int32_t i = 0; i < (std::int32_t)N_; ++i)
        if (dense[i] != 0.0 && part->owned(i)) {
          out.first.push_back(i);
          out.second.push_back(dense[i]);
        }
      return out;
    };
    const auto f1 = facet(1), f2 = facet(2);
    const auto& n = V->mesh->n;
    stiff_op = std::make_unique<BoxStiffnessOperator<double>>(k_, n[0], n[1], n[2], V->mesh->x.data(), c0_);
    if (updater_) {
      const int rc = wf_op_set_ghost_faces(stiff_op->handle(), part->owned_lo[0], part->owned_lo[1], part->owned_lo[2]);
      if (rc != WF_OK && rc != WF_ERR_UNSUPPORTED) check(rc);
      split_ = rc == WF_OK;
    }
    setup(BoxMassOperatorLumped<double>(k_, n[0], n[1], n[2], V->mesh->x.data()), f1, f2);
  }

  ~LinearGLLOpt() { wf_boundary_destroy(bc_); }
  /// what the stiffness operator of the loop runs (kernel, geometry, metric, ...)
  wf_op_info_t stiffness_info() const
  {
    wf_op_info_t i{};
    check(wf_op_info(stiff_op->handle(), &i));
    return i;
  }
  LinearGLLOpt(const LinearGLLOpt&) = delete;
  LinearGLLOpt& operator=(const LinearGLLOpt&) = delete;

  /// Point sources f = s(t) delta(x - x_s), the right-hand side of u_tt - c0^2 Lap u = f: every loop adds
  /// b[d] += s(t) phi_d(x_s) at the time argument at which it evaluates the plane source (rk4: in f1 after the boundary
  /// term; rk4_fused: a launch after each stage kernel, and once before the loop; leapfrog: after K u, start-up and
  /// finish included).  Receivers record u at the start time and after every step (steps + 1 rows per call).  One rank;
  /// nullptr (the default) switches either off, and the loops then issue the launches they always did.  The objects
  /// must outlive the model's loops.
  void set_sources(const Sources* s)
  {
    if (s && updater_) throw std::runtime_error("LinearGLLOpt: point sources on a partitioned mesh are not implemented");
    sources_ = s;
  }
  void set_receivers(Receivers* r)
  {
    if (r && updater_) throw std::runtime_error("LinearGLLOpt: receivers on a partitioned mesh are not implemented");
    receivers_ = r;
  }

  /// Set the initial values of u and v (LinearGLL.hpp:131-134)
  void init()
  {
    check(wf_fill(N_, 0.0, u_n->data(), nullptr));
    check(wf_fill(N_, 0.0, v_n->data(), nullptr));
  }

  /// du/dt = f0(t, u, v)  (LinearGLL.hpp:141-144)
  void f0(double& /*t*/, array<double>& /*u*/, array<double>& v, array<double>& result) { kernels::copy(v, result); }

  /// dv/dt = f1(t, u, v)  (LinearGLL.hpp:151-192)
  void f1(double& t, array<double>& u, array<double>& v, array<double>& result)
  {
    check(wf_fill(N_, 0.0, b->data(), nullptr));
    stiffness(u.data());        // scatter_fwd(u); K; scatter_rev(b)
    kernels::copy(u, *u_n);
    kernels::copy(v, *v_n);
    boundary(t, v_n->data());
    add_sources(t);
    check(wf_pointwise_div(N_, b->data(), m->data(), result.data(), nullptr));
  }

  /// Runge-Kutta 4th order solver (LinearGLL.hpp:198-287), the reference's sequence of
  /// vector operations; returns the number of steps taken.  rk4, f0 and f1 are the line-by-line transcription of
  /// common/LinearGLL.hpp:141-287 and stay readable as such; the loops the product runs are the library's (below).
  int rk4(double& startTime, double& finalTime, double& timeStep)
  {
    double t = startTime, tf = finalTime, dt = timeStep;
    int step = 0;
    auto mk = [&]() { return std::make_unique<array<double>>((std::size_t)N_); };
    auto u_ = mk(), v_ = mk(), un = mk(), vn = mk(), u0 = mk(), v0 = mk(), ku = mk(), kv = mk();
    kernels::copy(*u_n, *u_);
    kernels::copy(*v_n, *v_);
    kernels::copy(*u_, *ku);
    kernels::copy(*v_, *kv);
    const int n_RK = 4;
    const double a_runge[4] = {0.0, 0.5, 0.5, 1.0};
    const double b_runge[4] = {1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0};
    const double c_runge[4] = {0.0, 0.5, 0.5, 1.0};
    double tn;
    record(*u_, t);
    while (t < tf) {
      dt = std::min(dt, tf - t);
      kernels::copy(*u_, *u0);
      kernels::copy(*v_, *v0);
      for (int i = 0; i < n_RK; i++) {
        kernels::copy(*u0, *un);
        kernels::copy(*v0, *vn);
        kernels::axpy(*un, dt * a_runge[i], *ku, *un, N_);
        kernels::axpy(*vn, dt * a_runge[i], *kv, *vn, N_);
        tn = t + c_runge[i] * dt;
        f0(tn, *un, *vn, *ku);
        f1(tn, *un, *vn, *kv);
        kernels::axpy(*u_, dt * b_runge[i], *ku, *u_, N_);
        kernels::axpy(*v_, dt * b_runge[i], *kv, *v_, N_);
      }
      t += dt;
      step += 1;
      record(*u_, t);
    }
    kernels::copy(*u_, *u_n);
    kernels::copy(*v_, *v_n);
    finish();
    return step;
  }

  /// The same integration with the vector algebra between two stiffness applies fused
  /// into ONE pass (wf_rk4_stage: divide, f0, both solution updates, the next stage's
  /// un / vn and the zeroing of b) and the stage-0 copies removed by pointer rotation.
  /// Same arithmetic expressions as rk4(); 72-96 B/dof of vector traffic per stage
  /// instead of 208.  The boundary term of each right-hand side is left in b by the stage kernel in front of it
  /// (wf_rk4_stage_bc), the first one by a plain launch: a stage is two launches, stiffness + vector algebra.
  /// The loop is wf_wave_rk4_fused, the one the Python model runs.  max_steps < 0: no limit.
  int rk4_fused(double& startTime, double& finalTime, double& timeStep, std::int64_t max_steps = -1)
  {
    return run(WF_WAVE_RK4_FUSED, startTime, finalTime, timeStep, max_steps);
  }

  /// Second-order central-difference (leapfrog, explicit Newmark beta = 0, gamma = 1/2) integration from the state
  /// (u_n, v_n) to the state (u_n, v_n): ONE stiffness apply and one streaming pass (wf_leapfrog_step_bc, 48 B/dof)
  /// per step.  The absorbing term is taken centred (implicit; diagonal, so a division), which keeps the stability
  /// limit at 2 / sqrt(lambda_max) whatever the boundary.  Start-up u^{-1} = u^0 - dt v^0 + dt^2/2 a^0 with
  /// a^0 = (K u^0 + boundary term) / m; finish: one more apply and update into a scratch vector for the central
  /// velocity v_n at the final time, u not advanced, so that a split run equals a continuous one.  The step is constant:
  /// steps are counted while t < finalTime and the last one is not shortened.  Returns the number of steps taken.
  /// The loop is wf_wave_leapfrog, the one the Python model runs.
  int leapfrog(double& startTime, double& finalTime, double& timeStep, std::int64_t max_steps = -1)
  {
    return run(WF_WAVE_LEAPFROG, startTime, finalTime, timeStep, max_steps);
  }

  /// Fourth-order leapfrog (the modified-equation scheme) from the state (u_n, v_n) to the state (u_n, v_n):
  /// (u+ - 2u + u-)/dt^2 = A u + (dt^2/12) A^2 u, A = M^-1 K: TWO stiffness applies and two streaming passes
  /// (wf_leapfrog4_predict, wf_leapfrog4_correct) per step, fourth order in time, stable for dt <= sqrt(12/lambda_max),
  /// sqrt(3) times leapfrog's limit.  The centred absorbing term stays second order.  Constant step, counted as
  /// leapfrog() counts; a split run equals a continuous one to truncation order, not to rounding.
  /// The loop is wf_wave_leapfrog4, the one the Python model runs.
  int leapfrog4(double& startTime, double& finalTime, double& timeStep, std::int64_t max_steps = -1)
  {
    return run(WF_WAVE_LEAPFROG4, startTime, finalTime, timeStep, max_steps);
  }

protected:
  /// one call of a loop of the library on (u_n, v_n): the descriptor, the work vectors and the trace rows
  int run(int scheme, double t0, double tf, double dt, std::int64_t max_steps)
  {
    wf_wave_desc d{};
    d.n = N_;
    d.d_m = m->data();
    d.d_b = b->data();
    d.bc = bc_;
    d.source = wave();
    d.fold_boundary = 1;
    d.op = stiff_op->handle();
    d.updater = updater_ ? updater_->handle() : nullptr;
    d.overlapped = split_;
    d.sources = sources_ ? sources_->handle() : nullptr;
    std::vector<double> times;
    if (receivers_) {
      times.resize((std::size_t)wf_wave_step_count(scheme, t0, tf, dt, max_steps) + 1);
      d.h_times = times.data();
      d.trace_rows = (std::int64_t)times.size();
      d.d_traces = receivers_->reserve(times.size());
      if (d.d_traces) d.receivers = receivers_->points();
    }
    std::vector<std::unique_ptr<array<double>>> work;
    std::vector<double*> work_ptr;
    for (int k = 0; k < wf_wave_work_vectors(scheme); ++k) {
      work.push_back(std::make_unique<array<double>>((std::size_t)N_));
      work_ptr.push_back(work.back()->data());
    }
    d.d_work = work_ptr.data();
    std::int64_t steps = 0;
    if (scheme == WF_WAVE_LEAPFROG4)
      check(wf_wave_leapfrog4(&d, t0, tf, dt, max_steps, u_n->data(), v_n->data(), nullptr, nullptr, nullptr, nullptr, &steps, nullptr));
    else if (scheme == WF_WAVE_LEAPFROG)
      check(wf_wave_leapfrog(&d, t0, tf, dt, max_steps, u_n->data(), v_n->data(), nullptr, nullptr, nullptr, &steps, nullptr));
    else
      check(wf_wave_rk4_fused(&d, t0, tf, dt, max_steps, u_n->data(), v_n->data(), nullptr, &steps, nullptr));
    if (receivers_) receivers_->advance(times.data(), (std::size_t)steps + 1);
    finish();   // synchronises: the work vectors go out of scope behind it
    return (int)steps;
  }

  void finish()
  {
    if (updater_) {   // LinearGLL.hpp:284-285
      updater_->update_fwd(u_n->data());
      updater_->update_fwd(v_n->data());
    }
    check(wf_sync(nullptr));
  }
};

}  // namespace wavehip
