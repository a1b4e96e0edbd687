"""The numpy reference of LinearGLLOpt.misfit_gradient and the scenario its tests share (tests/test_adjoint_host.py,
tests/test_gpu_adjoint_kernels.py, tests/test_gpu_adjoint_model.py).  No GPU and no torch in here.

The model.  K = sum_c a^K_c P_c^T K_c P_c with dense cell matrices K_c from the oracle (oracle.StiffnessOperator fed one
cell at a time, symmetrised: K_c is symmetric up to rounding and the adjoint assumes K^T = K), m = sum_c a^M_c m_c with the
oracle's lumped cell masses, the facet masses c1 (plane term) and c2 (absorbing) FIXED, and the loop of
points_helpers.leapfrog (LinearGLLOpt.leapfrog in numpy) in float64 or long double.  The cell matrices, masses and the
host scalars dt2 = fl(dt dt), hdt = fl(-s2 dt / 2) are float64 numbers in both precisions, so both run the same recurrence.

The adjoint (see LinearGLLOpt.misfit_gradient): with A+- = m +- h, h = hdt c2, r^k = traces[k] - observed[k],
    mu_N = mu_{N+1} = 0,   A+ mu_{k-1} = dt2 (K mu_k + R^T r^k / dt) + 2 m mu_k - A- mu_{k+1},   k = N .. 1
    dJ/da^K_c = dt2 sum_n mu_n^T K_c u^n - dt2/2 ((A-/m) mu_0)^T K_c u^0
    dJ/da^M_c = m_c . (q - p),  p = sum_n mu_n (u^{n+1} - 2 u^n + u^{n-1}),  q = dt2/2 (A-/m) mu_0 a^0
J = 1/2 dt sum_{n <= N} |r^n|^2.  The second terms are the start-up: u^{-1} = u^0 - dt v^0 + dt2/2 a^0 and
a^0 = (K u^0 + ...) / m depend on both arrays.

The scenario: a box of cubes of 2.5 mm, a two-layer medium (c 1500 | 2800 m/s, rho 1000 | 1850 kg/m^3, the interface
normal to z), all six faces absorbing (h != 0) and the plane term on the face x = lo, one Ricker point source that is not
zero at t0 = 0, a smooth non-zero (u^0, v^0), four receivers -- two in cell 0, one exactly on a node -- and N = 23 steps.
`observed` is the traces of a medium perturbed by a few per cent, cell by cell.

What the method reaches (measured with the numpy reference by tests/test_adjoint_host.py, which asserts them again):
  FD_H        relative step of the central differences in long double, a_c (1 +- FD_H)
  FD_REACHED  |adjoint - FD| / max|g| over all cells and both arrays, long double: the truncation error of the
              differences, O(FD_H^2); the adjoint itself is exact for the loop
  D64         |g_float64 - g_longdouble| / max|g_longdouble|: what float64 rounding does to the gradient
  MUTANT_MIN  each of the three wrong adjoints (A+ <-> A-, no start-up terms, residual one row late) misses the
              differences by at least this factor more than the correct one
  DIR_H       relative step of the float64 directional derivative (the device's test), near eps^(1/3): the numpy float64
              stepper reaches |FD - g.delta| = 1.2e-9 .. 1.4e-9 of sum_c |g_c| |delta a_c| with it on the four
              configurations of the device test, all of it truncation (it scales with DIR_H^2)"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import leapfrog_helpers as lh
import points_helpers as ph
from support import LD, oracle_module

CELL = 0.0025
FREQ, P0 = 0.5e6, 6e4
SRC_F, SRC_AMP = 1.0e6, 0.05
STEPS = 23
HOST_CASES = {"P2": (2, (2, 2, 2)), "P3": (3, (3, 2, 2))}

FD_H = 1e-6
FD_REACHED = 5e-11        # measured 1.3e-11 (P2) and 1.1e-11 (P3); 1.3e-9 at h = 1e-5; at 1e-7 the rounding of J takes over (1e-11)
D64 = 4e-14               # measured 3.8e-14 (P2: 2.4e-14 stiffness, 3.8e-14 mass) and 2.0e-14 (P3)
MUTANT_MIN = 1e6          # measured: swap > 1e25 (the swapped recurrence amplifies), no start-up 3.6e9, late row 5.1e9
DIR_H = 1e-5              # float64: truncation 1.3e-9 of sum |g| |delta a|, above the rounding of J / DIR_H (1e-6: 2e-10 .. 7e-10)


def two_layer(mesh, hi):
    from wave_fenics_amd.medium import Medium
    return Medium.from_centroids(mesh, lambda xc: (np.where(xc[:, 2] < 0.5 * hi[2], 1500.0, 2800.0),
                                                   np.where(xc[:, 2] < 0.5 * hi[2], 1000.0, 1850.0)))


@functools.lru_cache(maxsize=None)
def scenario(p: int, n=(2, 2, 2), perturb: float = 0.0, medium: bool = True):
    """Everything of one configuration, computed once, shared and left unchanged."""
    import wave_fenics_amd as w
    from wave_fenics_amd import points
    from wave_fenics_amd.linear_gll import facet_lumped_mass
    o = oracle_module()
    hi = tuple(CELL * k for k in n)
    om = o.create_box(n, p, hi=hi, perturb=perturb)
    mesh = w.create_box(n, hi=hi, perturb=perturb)
    V = w.create_functionspace(mesh, p)
    assert np.array_equal(V.dofmap, om.dofmap) and np.array_equal(mesh.x, om.x)
    nc, nd, ndofs = om.ncells, (p + 1) ** 3, om.ndofs
    dm = np.asarray(om.dofmap)
    med = two_layer(mesh, hi) if medium else None
    c0 = 1.0 if medium else 1500.0
    # dense cell matrices, one cell's geometry at a time
    Kop = o.StiffnessOperator(om, p, {"c0": c0})
    Kc = np.zeros((nc, nd, nd))
    for c in range(nc):
        for l in range(nd):
            x, y = np.zeros(ndofs), np.zeros(ndofs)
            x[dm[c, l]] = 1.0
            Kop(x, y, cells=(c, c + 1))
            Kc[c, :, l] = y[dm[c]]
    Kc = 0.5 * (Kc + Kc.transpose(0, 2, 1))
    Mop = o.MassOperatorCPU(om, p)
    detJ = Mop.detJ.copy()
    Mc = np.zeros((nc, ndofs))
    for c in range(nc):
        Mop.detJ = np.zeros_like(detJ)
        Mop.detJ[c] = detJ[c]
        Mop(np.ones(ndofs), Mc[c])
    adm = None if med is None else med.admittance
    set1 = facet_lumped_mass(V, {0: 1}, 1, adm)
    set2 = facet_lumped_mass(V, {f: 2 for f in range(6)}, 2, adm)
    c1, c2 = np.zeros(ndofs), np.zeros(ndofs)
    np.add.at(c1, set1[0], set1[1])
    np.add.at(c2, set2[0], set2[1])
    aK = np.ones(nc) if med is None else med.stiff_coeff
    aM = np.ones(nc) if med is None else med.mass_coeff
    # the time step: 0.25 of the CFL figure of the fastest cell, as the cell-form model test runs leapfrog
    dt = 0.25 * np.sqrt(3.0) * CELL / (2800.0 * p ** 2) if medium else 0.25 * np.sqrt(3.0) * CELL / (1500.0 * p ** 2)
    # points by cell and reference coordinates: receivers 0 and 1 share cell 0, receiver 2 is a vertex of cell 3
    rec = (np.array([0, 0, 3, 5], dtype=np.int32), np.array([[0.3, 0.4, 0.6], [0.7, 0.2, 0.5], [1.0, 0.0, 1.0], [0.25, 0.75, 0.5]]))
    src = (np.array([6], dtype=np.int32), np.array([[0.4, 0.6, 0.3]]))
    wavelet = points.ricker(SRC_F, 1.0 / SRC_F, SRC_AMP)
    rd, rw = dm[rec[0]], points.weights(p, rec[1])
    sd, sw = dm[src[0]], points.weights(p, src[1])
    # a smooth non-zero state
    rng = np.random.default_rng(1000 * p + nc)
    xd = o.dof_coordinates(om) / CELL
    u0, v0 = np.zeros(ndofs), np.zeros(ndofs)
    for _ in range(3):
        k, ph_, amp = rng.uniform(0.5, 2.0, 3), rng.uniform(0, 2 * np.pi, 2), rng.uniform(0.5, 1.0, 2)
        u0 += 1e3 * amp[0] * np.cos(xd @ k + ph_[0])
        v0 += 1e3 * 2 * np.pi * FREQ * amp[1] * np.cos(xd @ k + ph_[1])
    pattern = np.sin(1.0 + 2.3 * np.arange(nc))
    delta = np.random.default_rng(7 + p).uniform(-1.0, 1.0, (2, nc))
    for a in (Kc, Mc, c1, c2, aK, aM, u0, v0, pattern, delta):
        a.setflags(write=False)
    model = SimpleNamespace(T_=1.0 / FREQ, alpha_=4.0, freq0_=FREQ, p0_=P0, w0_=2.0 * np.pi * FREQ, c0_=1500.0)
    if medium:
        s1, s2 = (lambda t: lh.window(model, t) * P0 * model.w0_ * np.cos(model.w0_ * t)), -1.0
    else:
        s1 = lambda t: 1500.0 ** 2 * (lh.window(model, t) * P0 * model.w0_ / 1500.0 * np.cos(model.w0_ * t))   # noqa: E731
        s2 = -1500.0
    sc = SimpleNamespace(p=p, n=n, hi=hi, om=om, mesh=mesh, V=V, med=med, nc=nc, nd=nd, ndofs=ndofs, dm=dm, Kc=Kc, Mc=Mc, c1=c1,
                         c2=c2, set1=set1, set2=set2, aK=aK, aM=aM, dt=float(dt), rec=rec, src=src, wavelet=wavelet, rd=rd, rw=rw,
                         sd=sd, sw=sw, u0=u0, v0=v0, s1=s1, s2=s2, delta=delta, medium=medium, perturb=perturb)
    # observed: the traces of the medium perturbed cell by cell (float64 stepper)
    sc.aK_obs, sc.aM_obs = aK * (1.0 + 0.04 * pattern), aM * (1.0 - 0.03 * pattern)
    sc.observed = forward(sc, sc.aK_obs, sc.aM_obs, np.float64).traces
    sc.observed.setflags(write=False)
    return sc


def tf(sc):
    """final time of the run: just short of STEPS steps, so that `while t < tf` takes exactly STEPS"""
    return STEPS * sc.dt - 1e-3 * sc.dt


def stiffness_matrix(sc, aK, dtype):
    K = np.zeros((sc.ndofs, sc.ndofs), dtype=dtype)
    for c in range(sc.nc):
        K[np.ix_(sc.dm[c], sc.dm[c])] += dtype(aK[c]) * sc.Kc[c].astype(dtype)
    return K


def forward(sc, aK, aM, dtype):
    """The run in `dtype`: states u^0 .. u^N, traces [N + 1][R], J against sc.observed (None while that is being made)"""
    from wave_fenics_amd import points
    K = stiffness_matrix(sc, aK, dtype)
    m = np.asarray(aM, dtype=dtype) @ sc.Mc.astype(dtype)
    P = ph.Parts(m, sc.c1.astype(dtype), sc.c2.astype(dtype), lambda u: K @ u, sc.s1, sc.s2)
    P.u_n[:], P.v_n[:] = sc.u0, sc.v0
    SW = ph.source_vector(sc.ndofs, sc.sd, sc.sw, [1.0], dtype)
    RW = ph.tensor_weights(sc.rw, dtype)
    states = []

    def sample(u):
        states.append(u.copy())
        return (RW * u[sc.rd]).sum(axis=1)

    f = lambda t: dtype(points.wavelet_value(sc.wavelet, t)) * SW    # noqa: E731
    _, steps, traces, times = ph.leapfrog(P, f, sample, 0.0, tf(sc), sc.dt)
    assert steps == STEPS
    out = SimpleNamespace(K=K, m=m, states=states, traces=traces, times=times, f=f, RW=RW, v_n=P.v_n.copy(), u_n=P.u_n.copy())
    if getattr(sc, "observed", None) is not None:
        out.resid = traces - sc.observed.astype(dtype)
        out.J = dtype(0.5) * dtype(sc.dt) * (out.resid * out.resid).sum()
    return out


def misfit(sc, aK, aM, dtype):
    return forward(sc, aK, aM, dtype).J


def adjoint_gradient(sc, aK, aM, dtype, mutant=None):
    """(J, g_stiff, g_mass) of the module docstring in `dtype`.  mutant: None, "swap" (A+ <-> A- in the backward
    recurrence), "no_startup" (the start-up terms dropped) or "late" (the residual row of step k - 1 loads step k)."""
    fw = forward(sc, aK, aM, dtype)
    N, dt = STEPS, sc.dt
    dt2, hdt, _ = (dtype(x) for x in lh.host_scalars(dt, sc.s2))
    m, K, u = fw.m, fw.K, fw.states
    h = hdt * sc.c2.astype(dtype)
    Ap, Am = m + h, m - h
    if mutant == "swap":
        Ap, Am = Am, Ap
    RT = np.zeros((sc.ndofs, fw.RW.shape[0]), dtype=dtype)
    for r in range(fw.RW.shape[0]):
        np.add.at(RT[:, r], sc.rd[r], fw.RW[r])
    # the start-up again, as the loop does it
    a0 = (K @ u[0] + dtype(sc.s1(0.0)) * sc.c1.astype(dtype) + dtype(sc.s2) * sc.c2.astype(dtype) * sc.v0.astype(dtype) + fw.f(0.0)) / m
    um1 = (-dt) * sc.v0.astype(dtype) + u[0]
    um1 = (0.5 * dt * dt) * a0 + um1
    mu = [None] * (N + 2)
    mu[N] = mu[N + 1] = np.zeros(sc.ndofs, dtype=dtype)
    for k in range(N, 0, -1):
        row = fw.resid[k - 1] if mutant == "late" else fw.resid[k]
        load = (RT @ row) / dtype(dt)
        mu[k - 1] = (dt2 * (K @ mu[k] + load) + (dtype(2.0) * m) * mu[k] - Am * mu[k + 1]) / Ap
    Kc = sc.Kc.astype(dtype)
    eK = lambda lam, x: np.einsum("ci,cij,cj->c", lam[sc.dm], Kc, x[sc.dm])    # noqa: E731
    gK = np.zeros(sc.nc, dtype=dtype)
    p = np.zeros(sc.ndofs, dtype=dtype)
    for n in range(N - 1, -1, -1):
        gK += eK(mu[n], u[n])
        p += mu[n] * ((u[n + 1] - dtype(2.0) * u[n]) + (u[n - 1] if n > 0 else um1))
    Am_true = m - h
    ratio = (Am_true / m) * mu[0]
    q = np.zeros(sc.ndofs, dtype=dtype)
    if mutant != "no_startup":
        gK += eK(dtype(-0.5) * ratio, u[0])
        q = (dtype(0.5) * dt2) * ratio * a0
    gK *= dt2
    gM = sc.Mc.astype(dtype) @ (q - p)
    return fw.J, gK, gM


def finite_differences(sc, dtype, h):
    """central differences of J in every cell of both arrays, a_c (1 +- h)"""
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


def directional(sc, h, run):
    """(J(a + h delta a) - J(a - h delta a)) / (2 h) along delta a = delta * a in both arrays at once; run(aK, aM) -> J"""
    dK, dM = sc.delta[0] * sc.aK, sc.delta[1] * sc.aM
    Jp = run(sc.aK + h * dK, sc.aM + h * dM)
    Jm = run(sc.aK - h * dK, sc.aM - h * dM)
    return (Jp - Jm) / (2.0 * h), dK, dM


@functools.lru_cache(maxsize=None)
def reference(p: int, n=(2, 2, 2), perturb: float = 0.0, medium: bool = True):
    """(scenario, float64 adjoint (J, gK, gM), long-double adjoint, d64 per array) computed once"""
    sc = scenario(p, n, perturb, medium)
    g64 = adjoint_gradient(sc, sc.aK, sc.aM, np.float64)
    gld = adjoint_gradient(sc, sc.aK, sc.aM, LD)
    d64 = [float(np.abs(g64[i].astype(LD) - gld[i]).max() / np.abs(gld[i]).max()) for i in (1, 2)]
    return sc, g64, gld, d64


class Coefficients:
    """What LinearGLLOpt reads of a medium, holding the two coefficient arrays themselves (no round trip through c and
    rho): for models at a +- h delta a whose boundary= sets stay those of the base medium."""

    def __init__(self, stiff_coeff, mass_coeff):
        self.stiff_coeff = np.ascontiguousarray(stiff_coeff, dtype=np.float64)
        self.mass_coeff = np.ascontiguousarray(mass_coeff, dtype=np.float64)
        self.admittance = None
        self.ncells = int(self.stiff_coeff.size)


def device_model(sc, gpu, structured=True, coefficients=None):
    """LinearGLLOpt of the scenario on the device at (u^0, v^0): explicit boundary sets, the source and the receivers by
    cell and reference coordinates; on the structured box the owner-computes stiffness kernel (no atomics)."""
    import torch
    import cell_form_helpers as cf
    from wave_fenics_amd import points
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    V = sc.V if structured else cf.unstructured(sc.V)
    medium = None
    if sc.medium:
        medium = sc.med if coefficients is None else Coefficients(*coefficients)
    eqn = LinearGLLOpt(V, sc.p, 1500.0, FREQ, P0, boundary=(sc.set1, sc.set2), structured=structured,
                       tuning={"update": "owner"} if structured else None, medium=medium,
                       sources=points.Sources(V, None, [sc.wavelet], located=sc.src),
                       receivers=points.Receivers(V, None, located=sc.rec))
    reset(eqn, sc, gpu)
    torch.cuda.synchronize()
    return eqn


def reset(eqn, sc, gpu):
    import torch
    eqn.u_n.copy_(torch.from_numpy(sc.u0.copy()).to(gpu))
    eqn.v_n.copy_(torch.from_numpy(sc.v0.copy()).to(gpu))
    eqn.receivers.reset()
