// The plane source of the wave model (LinearGLL.hpp:153-162): the scalars of the boundary term
// b[idx1] += s1 mG1, b[idx2] += s2 mG2 v as both front ends and both time loops evaluate them.  Plain C++17, no HIP.
//
// s1 has two spellings.  Without a medium rk4_fused has always taken the product from left to right,
// ((c0^2 window) p0 w0 / c0) cos(w0 t), where the boundary term of f1 and of leapfrog forms
// c0^2 (window p0 w0 / c0 cos(w0 t)): equal up to the last bit only.  Both stay, so that neither loop's results change.
// With a medium the facet masses carry the admittance 1 / (rho c) and both are window p0 w0 cos(w0 t).
// c0^2 is the caller's (wf_wave_source.c0_squared): a compiler folds pow(x, 2.0) to x * x, which is not libm's pow in
// the last bit, so it is not formed here.
#pragma once
#include <cmath>

#include "wavehip.h"

namespace wf {

// the source's start-up ramp over alpha periods
inline double wave_window(const wf_wave_source& p, double t)
{
  if (t < p.period * p.alpha) return 0.5 * (1.0 - std::cos(p.freq0 * M_PI * t / p.alpha));
  return 1.0;
}

// g(t) of LinearGLL.hpp:153-162 (no medium: with one g = s1 / c differs from cell to cell and only s1 exists)
inline double wave_g(const wf_wave_source& p, double window, double t) { return window * p.p0 * p.w0 / p.c0 * std::cos(p.w0 * t); }

inline double wave_s1_medium(const wf_wave_source& p, double t) { return wave_window(p, t) * p.p0 * p.w0 * std::cos(p.w0 * t); }

// c0^2 g(t): f1 and leapfrog
inline double wave_s1(const wf_wave_source& p, double t)
{
  if (p.medium) return wave_s1_medium(p, t);
  return p.c0_squared * wave_g(p, wave_window(p, t), t);
}

// the same product from left to right: rk4_fused
inline double wave_s1_left_to_right(const wf_wave_source& p, double t)
{
  if (p.medium) return wave_s1_medium(p, t);
  return p.c0_squared * wave_window(p, t) * p.p0 * p.w0 / p.c0 * std::cos(p.w0 * t);
}

// coefficient of the Gamma_2 term: -c0 (LinearGLL.hpp:175); -1 with a medium (admittance-weighted facet masses)
inline double wave_s2(const wf_wave_source& p) { return p.medium ? -1.0 : -p.c0; }

}  // namespace wf
