"""Leapfrog time stepping without a GPU: the headroom of the kernel test's bounds, the properties of the scheme on the
numpy stepper over the oracle (what LinearGLLOpt.leapfrog is compared against on the device), and the refusals of
wf_leapfrog_step that are decided before anything touches a device.

Cases: box 0.01^3, c0 = 1500, f = 0.5 MHz, P2 with 4^3 cells and P4 with 2^3 cells (729 dofs each)."""
import numpy as np
import pytest

import leapfrog_helpers as lh
import test_gpu_leapfrog_kernel as tk
import test_gpu_vector_kernels as vk
from leapfrog_helpers import LD

C0, FREQ, P0, L = 1500.0, 0.5e6, 6e4, 0.01
CASES = {"P2": (2, (4, 4, 4)), "P4": (4, (2, 2, 2))}
_CACHE = {}


def case(oracle, name):
    """(oracle mesh, model, K, s1, s2, lambda_max of -M^-1 K), computed once"""
    if name not in _CACHE:
        p, n = CASES[name]
        om = oracle.create_box(n, p, hi=(L, L, L))
        model = oracle.LinearGLLOpt(om, p, C0, FREQ, P0)
        K, s1, s2 = lh.oracle_parts(model)
        lam = float(np.linalg.eigvalsh(lh.dense_operator(K, model.m))[-1])
        _CACHE[name] = (om, model, K, s1, s2, lam)
    return _CACHE[name]


class State:
    """a model with the oracle's diagonals and optionally no boundary sets"""

    def __init__(self, model, boundary=True):
        self.m = model.m
        self.mG1 = model.mG1 if boundary else np.zeros_like(model.m)
        self.mG2 = model.mG2 if boundary else np.zeros_like(model.m)
        self.u_n, self.v_n = np.zeros_like(model.m), np.zeros_like(model.m)


def smooth_field(om, seed):
    """a few low Fourier modes at the dof coordinates: well inside the resolved spectrum"""
    import oracle.wave_oracle as o
    x = o.dof_coordinates(om) / L
    rng = np.random.default_rng(seed)
    f = np.zeros(x.shape[0])
    for _ in range(6):
        k = rng.integers(0, 3, 3)
        f += rng.uniform(-1, 1) * np.cos(np.pi * k[0] * x[:, 0]) * np.cos(np.pi * k[1] * x[:, 1]) * np.cos(np.pi * k[2] * x[:, 2])
    return f


def test_float64_evaluation_has_headroom():
    """The three expressions in plain float64 numpy (one rounding per operation, what the library's unfused evaluation
    does) against long double on every case of the kernel test: under the derived bounds, the worst ratio printed."""
    worst = {"plain": 0.0, "boundary": 0.0, "v": 0.0}
    for n in tk.LENGTHS:
        for bc in tk.BCS:
            host, sets = lh.kernel_case(n, bc)
            plan = None if sets is None else vk.plan_reference(*sets)
            args = (host["b"], host["m"], host["u"], host["up"], lh.KERNEL_DT, plan, lh.KERNEL_S1, lh.KERNEL_S2)
            lo, _ = lh.step_reference(np.float64, *args)
            hi, bound = lh.step_reference(LD, *args)
            on = np.zeros(n, dtype=bool)
            if plan is not None:
                on[plan[0]] = True
            for key, sel in (("plain", ~on), ("boundary", on)):
                if sel.any():
                    r, ok, where = lh.worst_ratio(lo[sel], hi[sel], bound[sel])
                    assert ok, (n, bc, key, where, r)
                    worst[key] = max(worst[key], r)
            v64, _ = lh.velocity(np.float64, lo, host["up"], lh.KERNEL_DT)
            vld, vmag = lh.velocity(LD, lo, host["up"], lh.KERNEL_DT)
            r, ok, where = lh.worst_ratio(v64, vld, lh.BOUND_V * vmag)
            assert ok, (n, bc, "v", where, r)
            worst["v"] = max(worst["v"], r)
    for key, r in worst.items():
        print(f"float64 numpy against long double, {key}: worst |error| = {r:.3f} of its bound")
        assert 0.0 < r <= 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_energy_is_conserved_without_boundary_sets(oracle, name):
    """1/2 v^T m v - 1/2 u^{n+1 T} K u^n drifts by <= 1e-13 (relative) over 400 steps at 0.9 of the critical step"""
    om, model, K, s1, s2, lam = case(oracle, name)
    dt = 0.9 * 2.0 / np.sqrt(lam)
    st = State(model, boundary=False)
    st.u_n[:] = smooth_field(om, 1)
    st.v_n[:] = smooth_field(om, 2) * np.sqrt(lam) * 0.05
    hist = []
    t, steps = lh.leapfrog(st, K, s1, s2, 0.0, 400 * dt - 1e-13, dt, history=hist)
    assert steps == 400 and len(hist) == 401
    E = np.array([lh.energy(K, st.m, hist[i], hist[i + 1], dt) for i in range(400)])
    drift = float(np.abs(E - E[0]).max() / abs(E[0]))
    print(f"{name}: energy drift over 400 steps at 0.9 of the critical step {drift:.2e}")
    assert E[0] > 0.0 and drift <= 1e-13


def test_unstable_above_the_critical_step(oracle):
    """the other side of the limit: at 1.05 of the critical step the solution grows without bound"""
    om, model, K, s1, s2, lam = case(oracle, "P2")
    dt = 1.05 * 2.0 / np.sqrt(lam)
    st = State(model, boundary=False)
    st.u_n[:] = np.random.default_rng(0).uniform(-1, 1, st.m.size)
    lh.leapfrog(st, K, s1, s2, 0.0, 400 * dt - 1e-13, dt)
    assert np.abs(st.u_n).max() > 1e30


def test_second_order_convergence(oracle):
    """P2 4^3 with its boundary sets and source: the error at a fixed time against a fine RK4 run falls by a factor in
    [3.8, 4.2] per halving of the step (40, 80, 160 steps).  The time is the source's ramp, four periods, so that the
    coarsest run has 10 steps per period (0.5 of the critical step): the ratio 4 is the asymptotic one and needs every
    run to resolve the forcing."""
    om, model, K, s1, s2, lam = case(oracle, "P2")
    T = 4.0 / FREQ
    assert T / 40 < 2.0 / np.sqrt(lam)
    fine = 1280
    model.init()
    _, steps = model.rk4(0.0, T - 1e-13, T / fine)
    assert steps == fine
    uref = model.u_n.copy()
    err = []
    for n in (40, 80, 160):
        st = State(model)
        _, steps = lh.leapfrog(st, K, s1, s2, 0.0, T - 1e-13, T / n)
        assert steps == n
        err.append(float(np.abs(st.u_n - uref).max() / np.abs(uref).max()))
    ratios = [err[0] / err[1], err[1] / err[2]]
    print(f"leapfrog error against RK4 with {fine} steps: {err}, ratios {ratios}")
    assert all(3.8 <= r <= 4.2 for r in ratios), (err, ratios)


@pytest.mark.parametrize("name", list(CASES))
def test_split_run_equals_continuous_run(oracle, name):
    """17 + 23 steps against 40: u and v to <= 1e-13 of their maxima (start-up and finish are exact inverses)"""
    om, model, K, s1, s2, lam = case(oracle, name)
    dt, _ = oracle.cfl_time_step(om, CASES[name][0], C0, FREQ, CFL=0.5)
    whole, parts = State(model), State(model)
    lh.leapfrog(whole, K, s1, s2, 0.0, 40 * dt - 1e-13, dt)
    t, n1 = lh.leapfrog(parts, K, s1, s2, 0.0, 17 * dt - 1e-13, dt)
    t, n2 = lh.leapfrog(parts, K, s1, s2, t, 40 * dt - 1e-13, dt)
    assert (n1, n2) == (17, 23)
    du = float(np.abs(parts.u_n - whole.u_n).max() / np.abs(whole.u_n).max())
    dv = float(np.abs(parts.v_n - whole.v_n).max() / np.abs(whole.v_n).max())
    print(f"{name}: 17 + 23 steps against 40: u {du:.2e} v {dv:.2e}")
    assert du <= 1e-13 and dv <= 1e-13


def test_bounded_at_the_reference_cfl_where_rk4_is_not(oracle):
    """CFL 0.5 on the P2 cube (0.85 of leapfrog's critical step): 3000 leapfrog steps settle into the forced
    oscillation -- the last third is no larger than twice the middle third -- while the oracle's RK4 overflows at the
    same step (corner dofs carry three absorbing faces)."""
    om, model, K, s1, s2, lam = case(oracle, "P2")
    dt, _ = oracle.cfl_time_step(om, 2, C0, FREQ, CFL=0.5)
    assert dt < 2.0 / np.sqrt(lam)
    print(f"CFL 0.5 is {dt * np.sqrt(lam) / 2.0:.3f} of the critical step")
    st = State(model)
    hist = []
    lh.leapfrog(st, K, s1, s2, 0.0, 3000 * dt - 1e-13, dt, history=hist)
    peak = np.array([np.abs(u).max() for u in hist])
    assert np.isfinite(peak).all() and peak[1000:2000].max() > 0.0
    assert peak[2000:].max() <= 2.0 * peak[1000:2000].max()
    model.init()
    with np.errstate(all="ignore"):
        model.rk4(0.0, 3000 * dt - 1e-13, dt)
    assert not np.isfinite(model.u_n).all() or np.abs(model.u_n).max() > 1e30 * peak.max()


def test_refusals_before_any_device_call():
    """null vectors, forbidden aliases and a non-positive step are refused on the host: the pointers are never followed"""
    from wave_fenics_amd import _lib
    Lb = _lib.lib()
    n, dt = 100, 0.1
    p = {k: 0x10000 + 0x1000 * i for i, k in enumerate(("b", "m", "u", "up", "un", "v"))}   # disjoint fake addresses

    def call(**kw):
        a = dict(p, **kw)
        return Lb.wf_leapfrog_step(n, a.get("dt", dt), a["b"], a["m"], a["u"], a["up"], a["un"], a["v"], None)

    for k in ("b", "m", "u", "up", "un"):
        assert call(**{k: None}) == -1 and b"null" in Lb.wf_last_error()
    for k in ("u", "b", "m"):
        assert call(un=p[k]) == -1 and b"alias" in Lb.wf_last_error()
    for k in ("b", "m", "u", "up", "un"):
        assert call(v=p[k]) == -1 and b"alias" in Lb.wf_last_error()
    assert call(un=p["up"] + 8) == -1                      # overlapping u_prev without being u_prev
    for bad in (0.0, -0.1, float("nan")):
        assert call(dt=bad) == -1 and b"time step" in Lb.wf_last_error()
    assert Lb.wf_leapfrog_step_bc(n, dt, p["b"], p["m"], p["u"], p["up"], p["un"], p["v"], None, 0.0, 0.0, None) == -1
    assert b"plan" in Lb.wf_last_error()
    for nn in (0, -1):                                     # a no-op, whatever the pointers
        assert Lb.wf_leapfrog_step(nn, dt, None, None, None, None, None, None, None) == 0
    with pytest.raises(_lib.WavehipError):
        _lib.check(call(un=p["u"]))
