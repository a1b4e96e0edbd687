"""References for the point sources and receivers (wave_fenics_amd/points.py, csrc/point_locate.cpp, csrc/points.hip).

Weights.  wf_points_weights evaluates w_a = t_a / sum_b t_b, t_a = lam_a / (x - x_a), lam_a = 1 / prod_{b != a}(x_a - x_b),
n = P + 1 nodes, u = eps/2 per rounding: lam_a takes n - 1 differences, n - 2 products and a quotient, t_a one more
difference and quotient -- a relative error of at most 2n u.  The terms alternate in sign, so the sum of n of them has a
relative error of at most (2n + n - 1) u Lambda, Lambda = sum_a |w_a| (the Lebesgue function at x).  With the final
quotient |dw_a| <= (2n + 1 + 3n Lambda) u |w_a|.  A tensor weight is a product of three, so for nodal values q_l
    | sum_l W_l q_l - q(x) | <= WEIGHT_B(n, Lambda) eps sum_l |W_l| |q_l|,  WEIGHT_B = 3 (2n + 1 + 3n Lambda) / 2,
when the sum itself is taken in long double (the interpolant through the float64 nodes is exact for a polynomial of
degree <= P per variable, wherever the nodes lie).

Sampling.  wf_points_sample rounds the two weight products, the product with x and one addition per term, then six
butterfly additions: with nd terms, at most ceil(nd/64) + 6 additions lie on the path of a term, so
    | out - ref | <= SAMPLE_B(nd) eps sum_l |W_l| |x_l|,  SAMPLE_B = (3 + ceil(nd/64) + 6) / 2 rounded up.
wf_sources_add: per entry the weight product (2 roundings, done by the host merge), w * s and one addition per source
of the dof, then the addition onto b; the wavelet value s itself is compared separately."""
import math

import numpy as np

import leapfrog_helpers as lh
from support import EPS, LD  # noqa: F401


def WEIGHT_B(n, lebesgue):
    return 1.5 * (2 * n + 1 + 3 * n * lebesgue)


def SAMPLE_B(nd):
    return math.ceil((3 + -(-nd // 64) + 6) / 2)


def tensor_weights(w, dtype=np.float64):
    """[npoints][nd]: (wx[i] * wy[j]) * wz[k] at l = i + n (j + n k), the association of the kernels"""
    w = np.asarray(w, dtype=dtype)
    wx, wy, wz = w[:, 0, :], w[:, 1, :], w[:, 2, :]
    W = (wx[:, None, None, :] * wy[:, None, :, None]) * wz[:, :, None, None]      # [r][k][j][i]
    return W.reshape(w.shape[0], -1)


def sample_reference(dofs, w, x):
    """(ref, mag) of wf_points_sample in long double: sum_l W_l x[dofs_l] and sum_l |W_l| |x[dofs_l]|"""
    W = tensor_weights(w, LD)
    xv = np.asarray(x, dtype=LD)[dofs]
    return (W * xv).sum(axis=1), (np.abs(W) * np.abs(xv)).sum(axis=1)


def source_vector(ndofs, dofs, w, values, dtype=np.float64):
    """sum_i values[i] phi_d(x_i) as a dense vector, accumulated source by source (independent of the library's merge)"""
    W = tensor_weights(w, dtype)
    f = np.zeros(ndofs, dtype=dtype)
    for i in range(W.shape[0]):
        np.add.at(f, dofs[i], W[i] * dtype(values[i]))
    return f


def wavelet_ld(wl, t):
    """s(t) in long double, and whether float64 evaluation is expected to be exact (a clean zero)"""
    t = LD(t)
    if wl["kind"] == "ricker":
        a = (LD(np.pi) + LD(1.2246467991473532e-16)) * LD(wl["frequency"]) * (t - LD(wl["delay"]))
        a = a * a
        return LD(wl["amplitude"]) * (LD(1) - 2 * a) * np.exp(-a)
    v = np.asarray(wl["values"], dtype=LD)
    u = (t - LD(wl["t_start"])) / LD(wl["dt"])
    if not (0 <= u <= v.size - 1):
        return LD(0)
    k = min(int(u), v.size - 2)
    th = u - k
    return LD(wl["amplitude"]) * ((1 - th) * v[k] + th * v[k + 1])


class Parts:
    """What the steppers need of a model: m, c1 (plane-source facet mass), c2 (absorbing facet mass), K(u), s1(t), s2."""

    def __init__(self, m, c1, c2, K, s1, s2):
        self.m, self.c1, self.c2, self.K, self.s1, self.s2 = m, c1, c2, K, s1, s2
        self.u_n, self.v_n = np.zeros_like(m), np.zeros_like(m)


def oracle_parts(oracle, om, p, c0, freq, p0, absorbing_only=False):
    """Parts of oracle.LinearGLLOpt on the box om; absorbing_only: all six faces carry tag 2 (no plane source)"""
    ref = oracle.LinearGLLOpt(om, p, c0, freq, p0)
    K, s1, s2 = lh.oracle_parts(ref)
    if absorbing_only:
        return Parts(ref.m, np.zeros_like(ref.m), ref.mG1 + ref.mG2, K, lambda t: 0.0, s2)
    return Parts(ref.m, ref.mG1, ref.mG2, K, s1, s2)


def leapfrog(P, f, sample, t0, tf, dt, max_steps=None):
    """LinearGLLOpt.leapfrog with point sources in numpy: the stepper of leapfrog_helpers with f(t) (a dense load vector)
    added to K u wherever the device adds it -- start-up, every step, the finishing step -- and sample(u) recorded at t0
    and after every step.  Returns (t, steps, traces [steps + 1][R], times)."""
    m, c1, c2 = P.m, P.c1, P.c2
    dt2, hdt, tdt = lh.host_scalars(dt, P.s2)
    on = (c1 != 0.0) | (c2 != 0.0)
    h = hdt * c2

    def update(b, u, up, s):
        plain = dt2 * (b / m) + (2.0 * u - up)
        bnd = (dt2 * (b + s * c1) + ((2.0 * m) * u - (m - h) * up)) / (m + h)
        return np.where(on, bnd, plain)

    u, v0 = P.u_n.copy(), P.v_n.copy()
    a0 = (P.K(u) + P.s1(t0) * c1 + P.s2 * c2 * v0 + f(t0)) / m
    up = (-dt) * v0 + u
    up = (0.5 * dt * dt) * a0 + up
    t, steps = t0, 0
    rows, times = [sample(u)], [t]
    while t < tf:
        un = update(P.K(u) + f(t), u, up, P.s1(t))
        up, u = u, un
        t += dt
        steps += 1
        rows.append(sample(u))
        times.append(t)
        if max_steps is not None and steps >= max_steps:
            break
    un = update(P.K(u) + f(t), u, up, P.s1(t))
    P.u_n[:] = u
    P.v_n[:] = (un - up) / tdt
    return t, steps, np.array(rows), np.array(times)


def rk4(P, f, sample, t0, tf, dt, max_steps=None):
    """LinearGLLOpt.rk4 (oracle.LinearGLLOpt.rk4) with f(t) added to the right-hand side of f1"""
    def f1(t, u, v):
        return (P.K(u) + P.s1(t) * P.c1 + P.s2 * P.c2 * v + f(t)) / P.m

    t, steps = t0, 0
    u_, v_ = P.u_n.copy(), P.v_n.copy()
    ku, kv = u_.copy(), v_.copy()
    a_r, b_r, c_r = [0.0, 0.5, 0.5, 1.0], [1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0], [0.0, 0.5, 0.5, 1.0]
    rows, times = [sample(u_)], [t]
    while t < tf:
        dt = min(dt, tf - t)
        u0, v0 = u_.copy(), v_.copy()
        for i in range(4):
            un = ku * (dt * a_r[i]) + u0
            vn = kv * (dt * a_r[i]) + v0
            tn = t + c_r[i] * dt
            ku, kv = vn.copy(), f1(tn, un, vn)
            u_ = ku * (dt * b_r[i]) + u_
            v_ = kv * (dt * b_r[i]) + v_
        t += dt
        steps += 1
        rows.append(sample(u_))
        times.append(t)
        if max_steps is not None and steps >= max_steps:
            break
    P.u_n[:], P.v_n[:] = u_, v_
    return t, steps, np.array(rows), np.array(times)


def host_points(V, xyz):
    """(dofs [n][nd], w [n][3][P+1]) of physical points, through points.locate / points.weights (no device call)"""
    from wave_fenics_amd import points
    cell, ref = points.locate(V, xyz)
    assert (cell >= 0).all(), cell
    return np.asarray(V.dofmap)[cell].astype(np.int32), points.weights(V.degree, ref)


def load_and_sampler(V, src_xyz, wavelets, rec_xyz):
    """(f(t), sample(u)) of the numpy steppers for the given sources and receivers"""
    from wave_fenics_amd import points
    sd, sw = host_points(V, src_xyz)
    rd, rw = host_points(V, rec_xyz)
    RW = tensor_weights(rw)

    def f(t):
        return source_vector(V.ndofs, sd, sw, [points.wavelet_value(wl, t) for wl in wavelets])

    def sample(u):
        return (RW * u[rd]).sum(axis=1)
    return f, sample


def min_edge(mesh):
    """shortest cell edge of a hexahedral mesh"""
    xc = np.asarray(mesh.x)[np.asarray(mesh.geom_dofmap)]
    e = [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
    return min(float(np.linalg.norm(xc[:, a] - xc[:, b], axis=1).min()) for a, b in e)


# ---- the reciprocity pair and the free-space case, shared by the host and the GPU tests ----
RECIP_N, RECIP_P, RECIP_L, RECIP_C0, RECIP_F, RECIP_STEPS = (4, 4, 4), 4, 0.01, 1500.0, 1.0e6, 48
RECIP_A = (0.0031, 0.0042, 0.0036)      # cell (1, 1, 1)
RECIP_B = (0.0058, 0.0059, 0.0061)      # cell (2, 2, 2); |AB| = 4.05 mm, the Ricker peak arrives at step 42


def recip_dt():
    """0.70 of the leapfrog limit 2 / sqrt(lambda_max) = 1.4315e-7 s of this box (60 power iterations on the oracle)"""
    return 1.0e-7


def recip_wavelet():
    from wave_fenics_amd import points
    return points.ricker(RECIP_F, 1.5 / RECIP_F, 1.0e3)


def recip_space(oracle):
    import wave_fenics_amd as w
    om = oracle.create_box(RECIP_N, RECIP_P, hi=(RECIP_L,) * 3)
    mesh = w.BoxMesh(om.n, om.x.copy(), om.geom_dofmap.copy(), (0.0, 0.0, 0.0), (RECIP_L,) * 3)
    return om, w.create_functionspace(mesh, RECIP_P)


_RECIP = {}


def recip_host(oracle):
    """(trace A->B, trace B->A, relative difference) of the numpy leapfrog stepper with all faces absorbing, computed once"""
    if "r" not in _RECIP:
        om, V = recip_space(oracle)
        dt, out = recip_dt(), []
        for s, r in ((RECIP_A, RECIP_B), (RECIP_B, RECIP_A)):
            P = oracle_parts(oracle, om, RECIP_P, RECIP_C0, RECIP_F, 0.0, absorbing_only=True)
            f, sample = load_and_sampler(V, [s], [recip_wavelet()], [r])
            _, steps, rows, _ = leapfrog(P, f, sample, 0.0, RECIP_STEPS * dt - 1e-13, dt)
            assert steps == RECIP_STEPS
            out.append(rows[:, 0])
        _RECIP["r"] = (out[0], out[1], recip_diff(out[0], out[1]))
    return _RECIP["r"]


def recip_diff(ab, ba):
    return float(np.abs(ab - ba).max() / np.abs(ab).max())
