"""The numpy reference of LinearGLLOpt.misfit_gradient(scheme="leapfrog4") and the scenario its tests share
(tests/test_adjoint4_host.py, tests/test_gpu_adjoint4_model.py, tests/test_gpu_adjoint4_streams.py).  No GPU and no torch.

The model is that of adjoint_helpers (dense symmetric cell matrices K_c, lumped cell masses, fixed facet masses c1, c2)
and the scenario is adjoint_helpers.scenario with two things of its own: the time step, 0.9 of leapfrog4's stability
limit sqrt(12 / lambda_max(-M^-1 K)) so that the dt^4 terms weigh, and `observed`, the traces of the perturbed medium
under THIS loop.  The loop is leapfrog4_helpers.leapfrog4 restated so that it keeps what the adjoint reads (u^n, w^n,
a0, j0, q0, the traces); `forward` equals that stepper bit for bit in float64 (asserted by the host test).

Notation (wf_leapfrog4_predict in include/wavehip.h): A+- = m +- h, h = hdt c2, d = -s2 c2, c12 = dt2/12.  Step n:
    b1 = K u^n + F1^n,  u* = the leapfrog update,  w^n = c12 b1/m,  u^{n+1} = u* + dt2 (K w^n + F2^n)/A+
The adjoint, r^k = traces[k] - observed[k], J = 1/2 dt sum_{n <= N} |r^n|^2:
    mu_N = mu_{N+1} = 0,   om_k = c12 (K mu_k)/m,
    A+ mu_{k-1} = dt2 (K mu_k + K om_k + R^T r^k / dt) + 2 m mu_k - A- mu_{k+1}
    per step n < N:   gK_c += dt2 (e_c(mu_n, u^n + w^n) + e_c(om_n, u^n)),   p += mu_n (u^{n+1} - 2 u^n + u^{n-1}) + 12 om_n w^n
    start-up, nu = -A- mu_0:   qh = (dt^4/24 nu)/m,  jh = (-dt^3/6 nu - d qh)/m,  ah = (dt^2/2 nu + K qh - d jh)/m
                     gK_c += e_c(qh, a0) + e_c(jh, v0) + e_c(ah, u0),   p += qh q0 + jh j0 + ah a0
    dJ/da^M_c = m_c . (-p)
The residual load goes onto b AFTER the predictor half: it is no part of om.

What the method reaches (measured by tests/test_adjoint4_host.py, which asserts them again):
  FD_REACHED_4  |adjoint - FD| / max|g| over all cells and both arrays in long double at adjoint_helpers.FD_H
  D64_4         |g_float64 - g_longdouble| / max|g_longdouble|
  MUTANTS       the six wrong adjoints; each misses the differences by adjoint_helpers.MUTANT_MIN times the correct error"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import adjoint_helpers as ah
import leapfrog4_helpers as l4
import points_helpers as ph
from support import LD

STEPS = ah.STEPS
HOST_CASES = ah.HOST_CASES
SAFETY = 0.9

FD_REACHED_4 = 7e-11      # measured 1.9e-11 (P2: 2.4e-12 stiffness, 1.9e-11 mass) and 1.0e-11 (P3: 8.7e-12, 1.0e-11)
D64_4 = 1e-14             # measured 1.2e-15 (P2: 7.8e-16 stiffness, 1.2e-15 mass) and 2.6e-15 (P3: 8.5e-16, 2.6e-15); J 2.7e-15, 3.4e-15
#                           the mutants, of max|g|, P2 / P3: no_omega_form 1.3e-1 / 8.0e-2, no_w 3.5e-2 / 4.8e-2, no_12 5.6e-2 / 9.2e-2,
#                           startup2 1.4e-3 / 9.4e-3, no_Kq 1.1e-4 / 1.9e-3 (6.0e6 times the correct form's error on P2, the
#                           smallest factor), load_before 8.4e-2 / 4.9e-2
#                           the float64 directional derivative at adjoint_helpers.DIR_H: 3.2e-9 (P2), 6.8e-10 (P3) of sum |g||delta a|
MUTANTS = ("no_omega_form", "no_w", "no_12", "startup2", "no_Kq", "load_before")


def stable_dt(sc):
    """SAFETY * sqrt(12 / lambda_max(-M^-1 K)) of the scenario's medium, rounded to three digits so that every LAPACK
    gives the same number"""
    K = ah.stiffness_matrix(sc, sc.aK, np.float64)
    m = np.asarray(sc.aM) @ sc.Mc
    s = 1.0 / np.sqrt(m)
    lmax = float(np.linalg.eigvalsh(-(s[:, None] * K) * s[None, :]).max())
    return float(f"{SAFETY * np.sqrt(12.0 / lmax):.3g}")


@functools.lru_cache(maxsize=None)
def scenario(p: int, n=(2, 2, 2), perturb: float = 0.0, medium: bool = True):
    """adjoint_helpers.scenario with leapfrog4's time step and the observed traces of leapfrog4 (a namespace of its own:
    the shared one stays unchanged)"""
    base = ah.scenario(p, n, perturb, medium)
    sc = SimpleNamespace(**vars(base))
    sc.dt = stable_dt(base)
    sc.observed = None
    sc.observed = forward(sc, sc.aK_obs, sc.aM_obs, np.float64).traces
    sc.observed.setflags(write=False)
    return sc


def tf(sc):
    return ah.tf(sc)


def forward(sc, aK, aM, dtype, t0=0.0):
    """The leapfrog4 run in `dtype`: u^{-1} .. u^N (states[n + 1] = u^n), w^0 .. w^{N-1}, a0, j0, q0, the traces, J"""
    from wave_fenics_amd import points
    K = ah.stiffness_matrix(sc, aK, dtype)
    m = np.asarray(aM, dtype=dtype) @ sc.Mc.astype(dtype)
    c1, c2 = sc.c1.astype(dtype), sc.c2.astype(dtype)
    SW = ph.source_vector(sc.ndofs, sc.sd, sc.sw, [1.0], dtype)
    RW = ph.tensor_weights(sc.rw, dtype)
    g = lambda t: dtype(points.wavelet_value(sc.wavelet, t)) * SW    # noqa: E731
    s1, s2, dt = sc.s1, sc.s2, sc.dt
    dt2, hdt, _, c12 = l4.host_scalars(dt, s2)
    on = (c1 != 0.0) | (c2 != 0.0)
    h = hdt * c2
    d1 = lambda f, t: (f(t + dt) - f(t - dt)) / (2.0 * dt)           # noqa: E731
    dd = lambda f, t: (f(t + dt) - 2.0 * f(t)) + f(t - dt)           # noqa: E731

    def step(u, up, t):
        b = K @ u + g(t)
        s = s1(t)
        plain = dt2 * (b / m) + (2.0 * u - up)
        bnd = (dt2 * (b + s * c1) + ((2.0 * m) * u - (m - h) * up)) / (m + h)
        us = np.where(on, bnd, plain)
        w = c12 * ((b + s * c1) / m)
        b = K @ w
        b = b + dd(g, t) / 12.0
        s1c = dd(s1, t) / 12.0
        return np.where(on, us + (dt2 * (b + s1c * c1)) / (m + h), us + dt2 * (b / m)), w

    u, v0 = sc.u0.astype(dtype), sc.v0.astype(dtype)
    a0 = (K @ u + g(t0) + s1(t0) * c1 + s2 * c2 * v0) / m
    j0 = (K @ v0 + d1(g, t0) + d1(s1, t0) * c1 + s2 * c2 * a0) / m
    q0 = (K @ a0 + dd(g, t0) / dt2 + (dd(s1, t0) / dt2) * c1 + s2 * c2 * j0) / m
    up = (-dt) * v0 + u
    up = (0.5 * dt2) * a0 + up
    up = (-(dt2 * dt) / 6.0) * j0 + up
    up = ((dt2 * dt2) / 24.0) * q0 + up
    t, steps, end = t0, 0, tf(sc)
    states, ws, times = [up, u], [], [t]
    while t < end:
        un, w = step(u, up, t)
        up, u = u, un
        t += dt
        steps += 1
        states.append(u)
        ws.append(w)
        times.append(t)
    assert steps == STEPS
    traces = np.array([(RW * x[sc.rd]).sum(axis=1) for x in states[1:]])
    out = SimpleNamespace(K=K, m=m, h=h, c12=c12, states=states, ws=ws, a0=a0, j0=j0, q0=q0, traces=traces, times=times, RW=RW)
    if sc.observed is not None:
        out.resid = traces - sc.observed.astype(dtype)
        out.J = dtype(0.5) * dtype(dt) * (out.resid * out.resid).sum()
    return out


def misfit(sc, aK, aM, dtype):
    return forward(sc, aK, aM, dtype).J


def adjoint_gradient(sc, aK, aM, dtype, mutant=None):
    """(J, g_stiff, g_mass) of the module docstring in `dtype`.  mutant: None or one of MUTANTS --
    no_omega_form (no e_c(om_n, u^n)), no_w (u^n for u^n + w^n), no_12 (no 12 om w), startup2 (the second-order start-up:
    no jh, qh), no_Kq (ah without K qh), load_before (the residual load added before the predictor half)"""
    assert mutant is None or mutant in MUTANTS
    fw = forward(sc, aK, aM, dtype)
    N, dt = STEPS, sc.dt
    m, K, h, c12 = fw.m, fw.K, fw.h, fw.c12
    dt2 = l4.host_scalars(dt, sc.s2)[0]
    u = lambda n: fw.states[n + 1]                                   # noqa: E731
    Ap, Am = m + h, m - h
    d = dtype(-sc.s2) * sc.c2.astype(dtype)
    RT = np.zeros((sc.ndofs, fw.RW.shape[0]), dtype=dtype)
    for r in range(fw.RW.shape[0]):
        np.add.at(RT[:, r], sc.rd[r], fw.RW[r])
    zero = np.zeros(sc.ndofs, dtype=dtype)
    mu, om = [None] * (N + 2), [None] * (N + 1)
    mu[N] = mu[N + 1] = zero
    for k in range(N, -1, -1):
        b = K @ mu[k]
        load = (RT @ fw.resid[k]) / dtype(dt) if k > 0 else zero
        if mutant == "load_before":
            b = b + load
            load = zero
        om[k] = c12 * (b / m)
        if k > 0:
            mu[k - 1] = (dt2 * (b + (K @ om[k] + load)) + (dtype(2.0) * m) * mu[k] - Am * mu[k + 1]) / Ap
    Kc = sc.Kc.astype(dtype)
    eK = lambda lam, x: np.einsum("ci,cij,cj->c", lam[sc.dm], Kc, x[sc.dm])    # noqa: E731
    gK = np.zeros(sc.nc, dtype=dtype)
    p = np.zeros(sc.ndofs, dtype=dtype)
    for n in range(N - 1, -1, -1):
        w = fw.ws[n]
        gK += eK(mu[n], u(n) if mutant == "no_w" else u(n) + w)
        if mutant != "no_omega_form":
            gK += eK(om[n], u(n))
        p += mu[n] * ((u(n + 1) - dtype(2.0) * u(n)) + u(n - 1))
        if mutant != "no_12":
            p += dtype(12.0) * (om[n] * w)
    gK *= dt2
    nu = -(Am * mu[0])
    second = mutant == "startup2"
    qh = zero if second else (((dt2 * dt2) / 24.0) * nu) / m
    jh = zero if second else ((-(dt2 * dt) / 6.0) * nu - d * qh) / m
    kq = zero if mutant == "no_Kq" else K @ qh
    ahat = ((0.5 * dt2) * nu + kq - d * jh) / m
    gK += eK(qh, fw.a0) + eK(jh, sc.v0.astype(dtype)) + eK(ahat, u(0))
    p += qh * fw.q0 + jh * fw.j0 + ahat * fw.a0
    gM = sc.Mc.astype(dtype) @ (-p)
    return fw.J, gK, gM


def finite_differences(sc, dtype, h):
    """central differences of J in every cell of both arrays, a_c (1 +- h) (adjoint_helpers.finite_differences on this
    module's loop)"""
    out = np.zeros((2, sc.nc), dtype=dtype)
    for which in range(2):
        for c in range(sc.nc):
            J = []
            for sign in (1.0, -1.0):
                a = [np.array(sc.aK, dtype=dtype), np.array(sc.aM, dtype=dtype)]
                a[which][c] *= dtype(1.0) + dtype(sign) * dtype(h)
                J.append(misfit(sc, a[0], a[1], dtype))
            a0 = dtype([sc.aK, sc.aM][which][c])
            out[which, c] = (J[0] - J[1]) / (a0 * (dtype(1.0) + dtype(h)) - a0 * (dtype(1.0) - dtype(h)))
    return out


@functools.lru_cache(maxsize=None)
def reference(p: int, n=(2, 2, 2), perturb: float = 0.0, medium: bool = True):
    """(scenario, float64 adjoint (J, gK, gM), long-double adjoint, d64 per array) computed once"""
    sc = scenario(p, n, perturb, medium)
    g64 = adjoint_gradient(sc, sc.aK, sc.aM, np.float64)
    gld = adjoint_gradient(sc, sc.aK, sc.aM, LD)
    d64 = [float(np.abs(g64[i].astype(LD) - gld[i]).max() / np.abs(gld[i]).max()) for i in (1, 2)]
    return sc, g64, gld, d64
