"""References for the fourth-order leapfrog (modified-equation) time stepping: the per-entry expressions of
wf_leapfrog4_predict / wf_leapfrog4_correct in long double with their derived bounds, and a numpy stepper of
LinearGLLOpt.leapfrog4 (start-up, steps, finish) over the parts of leapfrog_helpers.

The expressions (include/wavehip.h), with dt2 = dt*dt, hdt = (-s2)*(0.5*dt), tdt = 2*dt and c12 = dt2/12 rounded
once each in float64 by the host (the references take the host's float64 values as exact inputs):

  predictor   u_star:        the two expressions of leapfrog_helpers (plain_update, boundary_update)
              w, plain dof:  c12*(b/m)
              w, union set:  c12*((b + s1*c1)/m)
  corrector   plain dof:     u_next = u_star + dt2*(b/m)
              union set:     h = hdt*c2;  u_next = u_star + (dt2*(b + s1c*c1))/(m + h)
              velocity:      v = (u_next - u_prev)/tdt

Bounds B, in units of eps = 2^-52 times a magnitude; one rounding = eps/2 of the rounded value, the library evaluates the
expressions as written (no fused multiply-add).  k roundings, each of a partial result no larger than the magnitude S,
give |got - ref| <= k (eps/2) S (1 + O(eps)); B = k, so that a correct float64 evaluation stays within B/2
(test_leapfrog4_host.py holds numpy's to that):

* u_star: BOUND_PLAIN = 3 and BOUND_BOUNDARY = 5 of leapfrog_helpers, with their magnitudes, as they stand there.
* w plain: the quotient and the product, S = |c12 b/m|:                                                   B = 2
* w on the union set: s1*c1, the sum, the quotient, the product, S = c12 (|b| + |s1 c1|)/m:               B = 4
* u_next plain: the quotient, the product, the sum, S = |u_star| + dt2 |b|/m:                            B = 3
* u_next on the union set: h, m + h, s1c*c1, the sum, the product, the quotient, the last sum: seven roundings in all
  (at most five on one path), counted all, S = |u_star| + dt2 (|b| + |s1c c1|)/(m + h), h >= 0:           B = 7
* v: BOUND_V = 2 of leapfrog_helpers, from the u_next the device wrote."""
import numpy as np

import leapfrog_helpers as lh
from support import EPS, LD  # noqa: F401

BOUND_W_PLAIN, BOUND_W_BOUNDARY, BOUND_NEXT_PLAIN, BOUND_NEXT_BOUNDARY = 2.0, 4.0, 3.0, 7.0


def host_scalars(dt, s2):
    """(dt2, hdt, 2 dt, c12) as the host computes them, in float64"""
    dt2, hdt, tdt = lh.host_scalars(dt, s2)
    return dt2, hdt, tdt, dt2 / np.float64(12.0)


def _abs(a):
    return np.abs(np.asarray(a, dtype=LD))


def predict_reference(dtype, b, m, u, up, dt, plan=None, s1=0.0, s2=0.0):
    """(u_star, its bound, w, its bound) of every dof; plan = (dofs, c1, c2) as in leapfrog_helpers.step_reference"""
    c = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    us, us_bound = lh.step_reference(dtype, b, m, u, up, dt, plan, s1, s2)
    c12 = dtype(host_scalars(dt, s2)[3])
    w = c12 * (c(b) / c(m))
    w_bound = BOUND_W_PLAIN * (LD(c12) * _abs(b) / _abs(m))
    if plan is not None and plan[0].size:
        d, c1, _ = plan
        w = w.copy()
        w[d] = c12 * ((c(b[d]) + dtype(s1) * c(c1)) / c(m[d]))
        w_bound[d] = BOUND_W_BOUNDARY * (LD(c12) * (_abs(b[d]) + LD(abs(s1)) * _abs(c1)) / _abs(m[d]))
    return us, us_bound, w, w_bound


def correct_reference(dtype, b, m, us, dt, plan=None, s1c=0.0, s2=0.0):
    """(u_next, its bound) of every dof"""
    c = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    dt2, hdt = (dtype(x) for x in host_scalars(dt, s2)[:2])
    un = c(us) + dt2 * (c(b) / c(m))
    bound = BOUND_NEXT_PLAIN * (_abs(us) + LD(dt2) * _abs(b) / _abs(m))
    if plan is not None and plan[0].size:
        d, c1, c2 = plan
        h = hdt * c(c2)
        un = un.copy()
        un[d] = c(us[d]) + (dt2 * (c(b[d]) + dtype(s1c) * c(c1))) / (c(m[d]) + h)
        hl = LD(hdt) * _abs(c2)
        bound[d] = BOUND_NEXT_BOUNDARY * (_abs(us[d]) + LD(dt2) * (_abs(b[d]) + LD(abs(s1c)) * _abs(c1)) / (_abs(m[d]) + hl))
    return un, bound


# the data of the kernel test: that of leapfrog_helpers.kernel_case (h = hdt c2 around m), and a second difference of s1
KERNEL_DT, KERNEL_S1, KERNEL_S2, KERNEL_S1C = lh.KERNEL_DT, lh.KERNEL_S1, lh.KERNEL_S2, -0.0371


def kernel_case(n, bc):
    """leapfrog_helpers.kernel_case plus `us`, the u_star the corrector reads (values of its own: the corrector is tested
    apart from the predictor)"""
    import zlib

    import test_gpu_vector_kernels as vk
    host, sets = lh.kernel_case(n, bc)
    host["us"] = vk.values(np.random.default_rng(zlib.crc32(f"us {n} {bc}".encode())), n)
    return host, sets


def launch_cap():
    """the cap on workgroups of capped_grid (csrc/common.h), read from the source so that a retuned cap moves the test"""
    import os
    import re
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "wave_fenics_amd", "csrc", "common.h")) as f:
        text = f.read()
    body = text[text.index("inline unsigned capped_grid"):]
    return 1 << int(re.search(r"const size_t cap = \(size_t\)1 << (\d+);", body).group(1))


def entries_per_thread(n, vec, block=256):
    """the most entries one thread of the sweep takes at vector length n: sweep_shape (csrc/sweep.h) launches
    capped_grid(max(nvec, 1), 256) workgroups of 256 threads over nvec = n / 2 pairs (16-byte form) or n dofs (scalar
    form), grid-stride; the odd last dof of the 16-byte form goes to a thread of the last workgroup as a further entry of
    another width, not counted here"""
    nvec = n // 2 if vec else n
    groups = min(max((max(nvec, 1) + block - 1) // block, 1), launch_cap())
    return -(-nvec // (groups * block))


def two_entry_length():
    """the smallest n at which a thread takes two entries: the scalar form (an operand 8 bytes off) just past
    cap * 256 threads; the 16-byte form reaches it at twice that"""
    return launch_cap() * 256 + 1


# ---------------------------------------------------------------------------------------------------------------------
# the stepper
# ---------------------------------------------------------------------------------------------------------------------
def leapfrog4(model, K, s1, s2, t0, tf, dt, max_steps=None, history=None, load=None, numerov=True, correct_v=True):
    """LinearGLLOpt.leapfrog4 in numpy on any object with m, mG1, mG2 (dense dof vectors), u_n, v_n, as
    leapfrog_helpers.leapfrog is for leapfrog.  load(t) (optional): a dense load vector beside the plane source, the
    point sources of the device.  L' and L'' are central differences over t +- dt.
      start-up  a0 = (K u0 + L(t0) - d v0)/m, j0 = (K v0 + L'(t0) - d a0)/m, q0 = (K a0 + L''(t0) - d j0)/m,
                u_prev = u0 - dt v0 + dt^2/2 a0 - dt^3/6 j0 + dt^4/24 q0
      step      b = K u + load(t); u_star = the leapfrog update; w = c12 (b + s1 c1)/m;
                b = K w + (load(t-dt) - 2 load(t) + load(t+dt))/12; u_next = u_star + dt2 (b + s1c c1)/(m + h)
      finish    one more step for vt = (u_next - u_prev)/(2 dt), at = (u_next - 2 u + u_prev)/dt^2;
                j = (K vt + L'(t) - d at)/m; v_n = vt - dt^2/6 j; u not advanced
    For the tests of what each part is for: numerov=False drops the second-difference terms of the loads in the step,
    correct_v=False returns the plain central velocity vt.  history (a list): receives u^0 ... u^steps.
    Returns (t, steps)."""
    m, c1, c2 = model.m, model.mG1, model.mG2
    dt2, hdt, tdt, c12 = host_scalars(dt, s2)
    on = (c1 != 0.0) | (c2 != 0.0)
    h = hdt * c2
    zero = np.zeros_like(m)
    g = load if load is not None else (lambda t: zero)

    def d1(f, t):
        return (f(t + dt) - f(t - dt)) / (2.0 * dt)

    def dd(f, t):
        return (f(t + dt) - 2.0 * f(t)) + f(t - dt)

    def step(u, up, t):
        b = K(u) + g(t)
        s = s1(t)
        plain = dt2 * (b / m) + (2.0 * u - up)
        bnd = (dt2 * (b + s * c1) + ((2.0 * m) * u - (m - h) * up)) / (m + h)
        us = np.where(on, bnd, plain)
        w = c12 * ((b + s * c1) / m)
        b = K(w)
        s1c = 0.0
        if numerov:
            b = b + dd(g, t) / 12.0
            s1c = dd(s1, t) / 12.0
        return np.where(on, us + (dt2 * (b + s1c * c1)) / (m + h), us + dt2 * (b / m))

    u, v0 = model.u_n.copy(), model.v_n.copy()
    a0 = (K(u) + g(t0) + s1(t0) * c1 + s2 * c2 * v0) / m
    j0 = (K(v0) + d1(g, t0) + d1(s1, t0) * c1 + s2 * c2 * a0) / m
    q0 = (K(a0) + dd(g, t0) / dt2 + (dd(s1, t0) / dt2) * c1 + s2 * c2 * j0) / m
    up = (-dt) * v0 + u
    up = (0.5 * dt2) * a0 + up
    up = (-(dt2 * dt) / 6.0) * j0 + up
    up = ((dt2 * dt2) / 24.0) * q0 + up
    t, steps = t0, 0
    if history is not None:
        history.append(u.copy())
    while t < tf:
        un = step(u, up, t)
        up, u = u, un
        t += dt
        steps += 1
        if history is not None:
            history.append(u.copy())
        if max_steps is not None and steps >= max_steps:
            break
    un = step(u, up, t)
    vt = (un - up) / tdt
    at = ((-2.0) * u + un + up) * (1.0 / dt2)
    j = (K(vt) + d1(g, t) + d1(s1, t) * c1 + s2 * c2 * at) / m
    model.u_n[:] = u
    model.v_n[:] = (-dt2 / 6.0) * j + vt if correct_v else vt
    return t, steps


def modified_energy(K, m, u0, u1, dt):
    """the conserved discrete energy of the scheme without boundary terms: that of leapfrog_helpers.energy with K replaced
    by K' = K + (dt^2/12) K M^-1 K, which is symmetric: 1/2 v^T m v - 1/2 u1^T K' u0, v = (u1 - u0)/dt"""
    v = (u1 - u0) / dt
    k0 = K(u0)
    return 0.5 * (v @ (m * v)) - 0.5 * (u1 @ (k0 + (dt * dt / 12.0) * K(k0 / m)))      # in the precision of the states
