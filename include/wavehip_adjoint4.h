/*
 * wavehip_adjoint4.h -- what the discrete adjoint of the fourth-order leapfrog loop (wavehip_leapfrog4.h) adds to
 * libwavehip: one streaming pass and the loop with a per-step callback.  Conventions, handles and wf_wave_desc are those
 * of wavehip.h; the notation is that of wavehip_leapfrog4.h.
 *
 * The adjoint.  Step n of wf_wave_leapfrog4 is A+ u^{n+1} = dt2 K' u^n + 2 m u^n - A- u^{n-1} + loads with A+- = m +- h and
 * K' = K + c12 K m^-1 K symmetric, so the multipliers march backwards through the step itself:
 *       mu_N = mu_{N+1} = 0,   A+ mu_{k-1} = dt2 (K mu_k + K om_k + R^T r^k / dt) + 2 m mu_k - A- mu_{k+1},   om_k = c12 (K mu_k)/m,
 * wf_leapfrog4_predict on b = K mu_k with s1 = 0 (it leaves om_k in its w), the residual load onto b = K om_k AFTER the
 * predictor (before it, it would flow into om), wf_leapfrog4_correct with s1c = 0.  Per step n < N the sensitivities are
 *       stiffness cells:  dt2 (e_c(mu_n, u^n + w^n) + e_c(om_n, u^n))
 *       pointwise:        p += mu_n (u^{n+1} - 2 u^n + u^{n-1}) + 12 om_n w^n       (the second term: through the 1/m inside w)
 * with w^n the predictor's w of the forward step, and the mass sensitivity is the lumped-mass form of -p at the end.
 *
 * wf_leapfrog4_correlate: for i < n
 *       p[i] = (p[i] + lam[i] * ((up[i] - 2.0*u[i]) + um[i])) + 12.0 * (om[i] * w[i])
 *       z[i] = u[i] + w[i]                                        (d_z may be NULL: no store)
 *   evaluated as written (no fused multiply-add), so the 16-byte and the scalar form of the sweep give the same bits.
 *   z is the right operand of the step's first cell form.  64 B/dof of HBM traffic, 72 with z.  Refused (WF_ERR_INVALID,
 *   nothing written): a null vector other than d_z; p or z overlapping an input or each other.  The inputs may overlap
 *   each other.  n <= 0 is a no-op.
 *
 * wf_wave_leapfrog4_steps: wf_wave_leapfrog4 with a callback and the start-up derivatives.
 *   before_step(user, n, t, u^{n-1}, u^n, d_startup ? d_startup[0] : NULL, stream) is called before step n = 0, 1, ... as
 *   wf_wave_leapfrog calls its own (not before the finishing step); it may copy the vectors, a non-zero return ends the
 *   loop with WF_ERR_INVALID.  d_startup, if not NULL, holds three vectors of n doubles that receive a0, j0 and q0 of the
 *   start-up (a copy after each is formed: the loop overwrites a0 with q0).  With before_step and d_startup NULL it
 *   launches exactly what wf_wave_leapfrog4 launches -- wf_wave_leapfrog4 is that call.  Refusals before the first
 *   launch: those of wf_wave_leapfrog4, and a null entry of d_startup.
 */
#ifndef WAVEHIP_ADJOINT4_H
#define WAVEHIP_ADJOINT4_H

#include "wavehip_leapfrog4.h"

#ifdef __cplusplus
extern "C" {
#endif

int wf_leapfrog4_correlate(int64_t n, const double* d_lam, const double* d_om, const double* d_up, const double* d_u,
                           const double* d_um, const double* d_w, double* d_p, double* d_z, void* stream);
int wf_wave_leapfrog4_steps(const wf_wave_desc* desc, double t0, double tf, double dt, int64_t max_steps, double* d_u, double* d_v,
                            wf_wave_step_fn before_step, void* before_step_user, double* const* d_startup, double* t_end,
                            int64_t* steps, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WAVEHIP_ADJOINT4_H */
