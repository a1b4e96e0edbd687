"""References for the leapfrog (central-difference) time stepping: the per-entry expressions of wf_leapfrog_step(_bc) in
long double with their derived bounds, and a numpy stepper of LinearGLLOpt.leapfrog (start-up, steps, finish).

The expressions (include/wavehip.h), with dt2 = dt*dt and hdt = (-s2)*(0.5*dt) rounded once each in float64 by the host:

  plain dof:     a = b/m;  u_next = dt2*a + (2*u - u_prev)
  boundary dof:  h = hdt*c2;  u_next = (dt2*(b + s1*c1) + ((2*m)*u - (m - h)*u_prev)) / (m + h)
  velocity:      v = (u_next - u_prev) / (2*dt)

Bounds, eps = 2^-52, one rounding = eps/2 of the rounded value, the library evaluates the expressions as written
(no fused multiply-add; 2*u, 2*m and 2*dt are exact):

* plain: b/m, dt2*a, 2*u - u_prev and the sum round once each -- four roundings, each of a value no larger than
  S = |dt2 b/m| + 2|u| + |u_prev|, so |got - ref| <= 4 (eps/2) S (1 + O(eps)) <= 3 eps S.
* boundary: with D = m + h and T = dt2 (|b| + |s1 c1|) + 2 m |u| + (m + h) |u_prev| (h >= 0 because s2 <= 0 and c2 >= 0, so
  |m - h| <= m + h): the longest path is h -> m - h -> (m - h) u_prev -> difference -> sum -> quotient, plus the rounding
  of h and of m + h in the denominator; counted generously, at most seven roundings lie on any path from an input to the
  result, each relative to a partial result no larger than T / D: |got - ref| <= 7 (eps/2) T/D (1 + O(eps)) <= 5 eps T/D.
* velocity: the difference and the quotient, two roundings of at most (|u_next| + |u_prev|) / (2 dt) each:
  |got - ref| <= 2 eps (|u_next| + |u_prev|) / (2 dt), ref from the u_next the device wrote."""
import numpy as np

from support import EPS, LD  # noqa: F401

BOUND_PLAIN, BOUND_BOUNDARY, BOUND_V = 3.0, 5.0, 2.0      # in units of eps * magnitude


def host_scalars(dt, s2):
    """(dt2, hdt, 2 dt) as the host computes them, in float64"""
    dt, s2 = np.float64(dt), np.float64(s2)
    return dt * dt, (-s2) * (np.float64(0.5) * dt), np.float64(2.0) * dt


def plain_update(dtype, b, m, u, up, dt):
    """u_next of a dof outside the boundary sets, one operation at a time in `dtype`, and the magnitude of its bound"""
    c = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    dt2 = dtype(host_scalars(dt, 0.0)[0])
    a = c(b) / c(m)
    ref = dt2 * a + (dtype(2.0) * c(u) - c(up))
    L = lambda a: np.abs(np.asarray(a, dtype=LD))   # noqa: E731
    mag = LD(dt2) * L(b) / L(m) + LD(2.0) * L(u) + L(up)
    return ref, mag


def boundary_update(dtype, b, m, u, up, dt, s1, s2, c1, c2):
    """u_next of a dof of the union set and T / (m + h)"""
    c = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    dt2, hdt, _ = (dtype(x) for x in host_scalars(dt, s2))
    h = hdt * c(c2)
    ref = (dt2 * (c(b) + dtype(s1) * c(c1)) + ((dtype(2.0) * c(m)) * c(u) - (c(m) - h) * c(up))) / (c(m) + h)
    L = lambda a: np.abs(np.asarray(a, dtype=LD))   # noqa: E731
    hl = LD(hdt) * L(c2)
    T = LD(dt2) * (L(b) + LD(abs(s1)) * L(c1)) + LD(2.0) * L(m) * L(u) + (L(m) + hl) * L(up)
    return ref, T / (L(m) + hl)


def velocity(dtype, un, up, dt):
    c = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    tdt = dtype(host_scalars(dt, 0.0)[2])
    L = lambda a: np.abs(np.asarray(a, dtype=LD))   # noqa: E731
    return (c(un) - c(up)) / tdt, (L(un) + L(up)) / LD(tdt)


def step_reference(dtype, b, m, u, up, dt, plan=None, s1=0.0, s2=0.0):
    """u_next of every dof and the per-entry bound (already times its factor, in units of eps): plan = (dofs, c1, c2), the
    union set in dof order with the accumulated coefficients, or None"""
    ref, mag = plain_update(dtype, b, m, u, up, dt)
    bound = BOUND_PLAIN * mag
    if plan is not None and plan[0].size:
        d, c1, c2 = plan
        rb, mb = boundary_update(dtype, b[d], m[d], u[d], up[d], dt, s1, s2, c1, c2)
        ref = ref.copy()
        ref[d] = rb
        bound[d] = BOUND_BOUNDARY * mb
    return ref, bound


def worst_ratio(got, ref, bound):
    """max |got - ref| / (eps * bound) over the entries (<= 1 passes), whether every entry passes (the bound is absolute:
    a zero bound demands equality), and the first failing entry"""
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD))
    lim = LD(EPS) * np.asarray(bound, dtype=LD)
    ok = err <= lim
    pos = lim > 0
    worst = float(np.max(err[pos] / lim[pos])) if pos.any() else 0.0
    return worst, bool(ok.all()), int(np.argmin(ok)) if ok.size else -1


# the data of the kernel test (and of the headroom test of the float64 evaluation): dt2 b/m, u and u_prev of comparable
# size, h = hdt c2 between 0.14 and 4 around m in [0.5, 2], so that m - h passes through zero
KERNEL_DT, KERNEL_S1, KERNEL_S2 = 0.37, 0.8137, -7.3


def kernel_case(n, bc):
    """(host vectors b, m, u, up, boundary sets or None) of one kernel test case, seeded by its parameters; the sets by
    name as in test_gpu_vector_kernels.boundary_set ("none": no plan)"""
    import zlib

    import test_gpu_vector_kernels as vk
    rng = np.random.default_rng(zlib.crc32(f"{n} {bc}".encode()))
    host = {"b": vk.values(rng, n), "m": vk.divisors(rng, n), "u": vk.values(rng, n), "up": vk.values(rng, n)}
    return host, None if bc == "none" else vk.boundary_set(bc, n, rng)


# ---------------------------------------------------------------------------------------------------------------------
# the stepper
# ---------------------------------------------------------------------------------------------------------------------
def window(model, t):
    if t < model.T_ * model.alpha_:
        return 0.5 * (1.0 - np.cos(model.freq0_ * np.pi * t / model.alpha_))
    return 1.0


def oracle_parts(model):
    """(K, s1, s2) of oracle.LinearGLLOpt: K(u) = the stiffness apply onto zeros, s1(t) = c0^2 g(t), s2 = -c0"""
    def K(u):
        y = np.zeros_like(u)
        model.stiff_op(np.ascontiguousarray(u), y)
        return y

    def s1(t):
        return model.c0_ ** 2 * (window(model, t) * model.p0_ * model.w0_ / model.c0_ * np.cos(model.w0_ * t))
    return K, s1, -model.c0_


def medium_parts(model, K):
    """(K, s1, s2) of a model with admittance-weighted facet masses (LinearGLLOpt(medium=)): s1 = window p0 w0 cos(w0 t),
    s2 = -1"""
    return K, (lambda t: window(model, t) * model.p0_ * model.w0_ * np.cos(model.w0_ * t)), -1.0


def leapfrog(model, K, s1, s2, t0, tf, dt, max_steps=None, history=None):
    """LinearGLLOpt.leapfrog in numpy on any object with m, mG1, mG2 (dense dof vectors), u_n, v_n: start-up
    a0 = (K u0 + s1(t0) mG1 - d v0) / m, u_prev = u0 - dt v0 + dt^2/2 a0; steps with the kernel's two expressions while
    t < tf (constant step); finish: one more update for v_n = (u_next - u_prev) / (2 dt), u not advanced.
    history (a list): receives u^0, u^1, ... u^steps.  Returns (t, steps)."""
    m, c1, c2 = model.m, model.mG1, model.mG2
    dt2, hdt, tdt = host_scalars(dt, s2)
    on = (c1 != 0.0) | (c2 != 0.0)
    h = hdt * c2

    def update(b, u, up, s):
        plain = dt2 * (b / m) + (2.0 * u - up)
        bnd = (dt2 * (b + s * c1) + ((2.0 * m) * u - (m - h) * up)) / (m + h)
        return np.where(on, bnd, plain)

    u, v0 = model.u_n.copy(), model.v_n.copy()
    a0 = (K(u) + s1(t0) * c1 + s2 * c2 * v0) / m
    up = (-dt) * v0 + u
    up = (0.5 * dt * dt) * a0 + up
    t, steps = t0, 0
    if history is not None:
        history.append(u.copy())
    while t < tf:
        un = update(K(u), u, up, s1(t))
        up, u = u, un
        t += dt
        steps += 1
        if history is not None:
            history.append(u.copy())
        if max_steps is not None and steps >= max_steps:
            break
    un = update(K(u), u, up, s1(t))
    model.u_n[:] = u
    model.v_n[:] = (un - up) / tdt
    return t, steps


def dense_operator(K, m):
    """M^{-1/2} (-K) M^{-1/2} column by column (symmetrised: K is symmetric up to rounding)"""
    n = m.size
    A = np.empty((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        A[:, j] = -K(e)
        e[j] = 0.0
    s = 1.0 / np.sqrt(m)
    A = s[:, None] * A * s[None, :]
    return 0.5 * (A + A.T)


def energy(K, m, u0, u1, dt):
    """the conserved discrete energy of the scheme without boundary terms: 1/2 v^T m v - 1/2 u1^T K u0, v = (u1 - u0)/dt"""
    v = (u1 - u0) / dt
    return 0.5 * float(v @ (m * v)) - 0.5 * float(u1 @ K(u0))
