/*
 * wavehip_leapfrog4.h -- the fourth-order leapfrog (modified-equation, "ME4") time stepping of libwavehip: the two fused
 * passes of a step, the weighted point-source load and the time loop.  Conventions, handles and wf_wave_desc are those
 * of wavehip.h.
 *
 * The scheme.  With A = M^-1 K (lumped mass m, sign convention of f1: u'' = b / m) one step is
 *       (u+ - 2u + u-) / dt^2 = A u + (dt^2/12) A^2 u   (+ loads and their second difference),
 * fourth order in time, two stiffness applies and two passes per step, stable for dt <= sqrt(12) / sqrt(lambda_max(-A)):
 * sqrt(3) times the limit of wf_leapfrog_step.  The diagonal absorbing term d u', d = -s2 c2, is taken centred exactly
 * as wf_leapfrog_step_bc takes it and stays second order.
 *
 * One step, b = +0.0 on entry, dt2 = dt*dt, hdt = (-s2)*(0.5*dt), tdt = 2*dt, c12 = dt2/12 computed by the host:
 *   1. b += K u (the apply); wf_sources_add(t)
 *   2. wf_leapfrog4_predict, with s1 = s1(t):
 *        u_star = what wf_leapfrog_step_bc stores in u_next (the same expressions, the same bits)
 *        outside the plan's union set (and every dof without a plan):   w = c12*(b/m)
 *        dof r of the union set:                                         w = c12*((b + s1*c1[r])/m)
 *        b = +0.0
 *      d_u_star may be d_u_prev (in place); it must not overlap d_u, d_b, d_m or d_w; d_w overlaps no other vector.
 *      56 B/dof of HBM traffic.
 *   3. b += K w (the apply, ghost exchange as in 1)
 *   4. wf_sources_add_stencil at t - dt, t, t + dt with the weights 1/12, -2/12, 1/12 (the Numerov weighting of the load)
 *   5. wf_leapfrog4_correct, with s1c = (s1(t+dt) - 2*s1(t) + s1(t-dt))/12 from the host:
 *        outside the union set:   u_next = u_star + dt2*(b/m)
 *        dof r of the union set:  h = hdt*c2[r];  u_next = u_star + (dt2*(b + s1c*c1[r]))/(m + h)
 *        d_v non-null:            v = (u_next - u_prev)/tdt   (d_u_prev must then still hold u^{n-1}: step 2 out of place)
 *        b = +0.0
 *      d_u_next may be d_u_star (in place); it must not overlap d_b or d_m, nor d_u_prev when d_v is given; d_v overlaps
 *      no other vector.  d_u_prev is not read without d_v and may then be NULL.  40 B/dof, 56 with d_v.
 * The expressions are evaluated as written (no fused multiply-add), so every compiled form -- 16-byte and scalar sweep,
 * with and without a plan, with and without v -- gives the same bits.  bc may be NULL: no boundary sets (s1, s2 are then
 * not used, s2 is still checked).  Refused (WF_ERR_INVALID, nothing written): a forbidden overlap, s2 > 0, dt <= 0 or
 * NaN, a plan built for another n, a null vector.  n <= 0 is a no-op.
 *
 * wf_sources_add_stencil: d_b[d] += sum over the sources at dof d, in source order, of weight * S,
 *   S = ((h_a[0] s(h_t[0])) + h_a[1] s(h_t[1])) + h_a[2] s(h_t[2])  (the first nt terms, 1 <= nt <= 3), one thread and one
 *   writer per dof like wf_sources_add; nt = 1 with h_a[0] = 1 gives the bits of wf_sources_add.  h_t and h_a are host
 *   arrays of nt doubles read during the call (they travel by value with the launch).  Refused: a null handle, nt outside
 *   1..3, a null array or vector, a time or weight that is not finite.
 *
 * wf_wave_leapfrog4: the loop, state (u, v) in and out as wf_wave_leapfrog, constant step, the last step not shortened,
 *   steps counted as wf_wave_step_count(WF_WAVE_LEAPFROG4, ...) counts them, which is as it counts WF_WAVE_LEAPFROG;
 *   receivers record u at t0 and after every step.  d_work holds wf_wave_leapfrog4_work_vectors() vectors.  Derivatives of the loads are central differences at
 *   t +- dt: the plane source through wf_boundary_apply_plan with the differenced s1 (wf_wave_s1), the point sources
 *   through wf_sources_add_stencil.
 *   Start-up (three applies): a0 = (K u0 + L(t0) - d v0)/m, j0 = (K v0 + L'(t0) - d a0)/m, q0 = (K a0 + L''(t0) - d j0)/m,
 *     u^{-1} = u0 - dt v0 + dt^2/2 a0 - dt^3/6 j0 + dt^4/24 q0.
 *   Finish (three applies): one more full step out of place gives vt = (u^{n+1} - u^{n-1})/(2 dt) and
 *     at = (u^{n+1} - 2 u^n + u^{n-1})/dt^2; then j = (K vt + L'(t) - d at)/m and v = vt - dt^2/6 j.  u is not advanced.
 *   A run split in two equals the continuous run to truncation order (the start-up is a Taylor series, not the inverse
 *   of the finish), not to rounding.
 *   Refusals before the first launch are those of wf_wave_leapfrog.
 */
#ifndef WAVEHIP_LEAPFROG4_H
#define WAVEHIP_LEAPFROG4_H

#include "wavehip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The loop's scheme number, beside WF_WAVE_RK4_FUSED and WF_WAVE_LEAPFROG of wavehip.h: wf_wave_step_count counts it as it
 * counts WF_WAVE_LEAPFROG (a constant step, the last one not shortened); wf_wave_work_vectors does not know it and
 * returns -1 -- wf_wave_leapfrog4_work_vectors is this loop's count. */
enum { WF_WAVE_LEAPFROG4 = 2 };

int wf_leapfrog4_predict(int64_t n, double dt, double* d_b, const double* d_m, const double* d_u, const double* d_u_prev,
                         double* d_u_star, double* d_w, const wf_boundary* bc, double s1, double s2, void* stream);
int wf_leapfrog4_correct(int64_t n, double dt, double* d_b, const double* d_m, const double* d_u_star, const double* d_u_prev,
                         double* d_u_next, double* d_v, const wf_boundary* bc, double s1c, double s2, void* stream);
int wf_sources_add_stencil(const wf_sources* src, int nt, const double* h_t, const double* h_a, double* d_b, void* stream);
int wf_wave_leapfrog4_work_vectors(void);
int wf_wave_leapfrog4(const wf_wave_desc* desc, double t0, double tf, double dt, int64_t max_steps, double* d_u, double* d_v,
                      double* t_end, int64_t* steps, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WAVEHIP_LEAPFROG4_H */
