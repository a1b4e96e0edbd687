"""Fourth-order leapfrog (modified-equation) time stepping without a GPU: the headroom of the kernel test's bounds, the
properties of the scheme on the numpy stepper of leapfrog4_helpers over the oracle's operator (what
LinearGLLOpt.leapfrog4 is compared against on the device), and the refusals of the new entries that are decided before
anything touches a device.

The case is test_leapfrog_host's P2 box (4^3 cells, 729 dofs, c0 = 1500, f = 0.5 MHz) with the oracle's operator as the
dense matrix leapfrog_helpers.dense_operator builds (the stiffness apply column by column, symmetrised), so that the
thousands of steps of the order tests take seconds.  lambda_max is eigvalsh's; the stability limit of the scheme is
dt_max = sqrt(12) / sqrt(lambda_max).

Closed-domain tests (no boundary sets) excite the six lowest non-constant eigenmodes of the discrete operator only,
through the initial state and through the shape of a smooth load sin(w t): every excited mode then has omega dt <= 0.45
at the coarsest step and the observed orders are the asymptotic ones.  The errors are relative to max|reference|.

Energy.  Without boundary sets the scheme conserves 1/2 v^T m v - 1/2 u^{n+1 T} K' u^n with K' = K + (dt^2/12) K M^-1 K
(leapfrog4_helpers.modified_energy).  The float64 stepper's drift over 400 steps is measured and held to ten times the
drift recorded for it (1.1e-15); the stepper in long double drifts at least ten times less, which shows the float64 figure
to be rounding; leapfrog's energy with K alone, which the scheme does not conserve, varies by O(dt^2).  On the device
tests/test_gpu_leapfrog4_model.py holds the drift to ten times the float64 stepper's on the same states.

Equal number of applies, recorded from test_equal_applies (error of u at the final time against a fine reference):
  no boundary sets, from the low-mode state, T = 16 * 0.9 dt_max   leapfrog4 at 32 steps 1.6e-05, leapfrog at 64 steps 2.8e-03
  boundary sets and plane source from rest, T = 12 * 0.9 dt_max    leapfrog4 at 96 steps 1.1e-03, leapfrog at 192 steps 7.2e-03
The absorbing term is second order in both schemes (test_second_order_with_absorbing_sets); on this box the plane wave's
phase error in the interior still dominates leapfrog's error, so the fourth-order interior shows.  A 1-D damped problem
measured the other way round (1.3e-3 against 5.4e-4): which scheme wins with absorbing faces depends on the problem.  The
figures are printed by the test; it asserts only that the closed-domain error is the smaller one."""
import numpy as np
import pytest

import leapfrog4_helpers as l4
import leapfrog_helpers as lh
import test_gpu_leapfrog_kernel as tk
import test_gpu_vector_kernels as vk
import test_leapfrog_host as th
from leapfrog_helpers import LD

_CACHE = {}
NMODES = 6


def problem(oracle):
    """(model, K as a dense product, s1, s2, lambda_max, dt_max, modes [n, NMODES] in the M-orthonormal basis, their
    frequencies), computed once"""
    if not _CACHE:
        om, model, K, s1, s2, lam = th.case(oracle, "P2")
        A = lh.dense_operator(K, model.m)
        lams, V = np.linalg.eigh(A)
        sm = np.sqrt(model.m)

        def Kd(u):
            return -(sm * (A @ (sm * u)))
        first = int(np.argmax(lams > 1e-9 * lams[-1]))           # past the constant mode
        modes = V[:, first:first + NMODES] / sm[:, None]
        _CACHE["p"] = (model, Kd, s1, s2, float(lams[-1]), np.sqrt(12.0 / lams[-1]), modes, np.sqrt(lams[first:first + NMODES]))
    return _CACHE["p"]


def closed_case(oracle):
    """(u0, v0, load(t), T, dt0): the low-mode state and load of the closed-domain tests; dt0 = 0.9 dt_max, T = 16 dt0"""
    model, K, s1, s2, lam, dtmax, modes, omega = problem(oracle)
    rng = np.random.default_rng(5)
    u0 = modes @ rng.uniform(-1, 1, NMODES)
    v0 = modes @ (rng.uniform(-1, 1, NMODES) * omega)
    shape = model.m * (modes @ (rng.uniform(-1, 1, NMODES) * omega ** 2))
    dt0 = 0.9 * dtmax
    T = 16 * dt0
    w = 2.0 * np.pi * 1.5 / T
    assert omega.max() * dt0 <= 0.45
    return u0, v0, (lambda t: np.sin(w * t + 0.3) * shape), T, dt0


def run(oracle, n, T, boundary, u0=None, v0=None, load=None, scheme="leapfrog4", **kw):
    model, K, s1, s2, lam, dtmax, modes, omega = problem(oracle)
    st = th.State(model, boundary=boundary)
    if u0 is not None:
        st.u_n[:], st.v_n[:] = u0, v0
    if scheme == "leapfrog4":
        t, steps = l4.leapfrog4(st, K, s1, s2, 0.0, T * (1.0 - 1e-9 / n), T / n, load=load, **kw)
    else:
        assert load is None
        t, steps = lh.leapfrog(st, K, s1, s2, 0.0, T * (1.0 - 1e-9 / n), T / n)
    assert steps == n
    return st.u_n.copy(), st.v_n.copy()


def rel(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def orders(err):
    return [float(np.log2(err[i] / err[i + 1])) for i in range(len(err) - 1)]


def closed_reference(oracle):
    """the closed-domain case at 512 steps, and the proof that it can serve: the run at 1024 steps differs from it by
    more than the rounding floor (so it is truncation that is being measured) and by far less than the errors asserted"""
    if "ref" not in _CACHE:
        u0, v0, load, T, dt0 = closed_case(oracle)
        a = run(oracle, 512, T, False, u0, v0, load)
        b = run(oracle, 1024, T, False, u0, v0, load)
        _CACHE["ref"] = (a, (rel(a[0], b[0]), rel(a[1], b[1])))
    return _CACHE["ref"]


def test_float64_evaluation_has_headroom():
    """The expressions of both kernels in plain float64 numpy (one rounding per operation, what the library's unfused
    evaluation does) against long double on every case of the leapfrog kernel test: w and u_next within B/2 of the bounds
    derived in leapfrog4_helpers; u_star within leapfrog_helpers' own bounds, as test_leapfrog_host holds them."""
    worst = {}
    for n in tk.LENGTHS:
        for bc in tk.BCS:
            host, sets = l4.kernel_case(n, bc)
            plan = None if sets is None else vk.plan_reference(*sets)
            on = np.zeros(n, dtype=bool)
            if plan is not None:
                on[plan[0]] = True
            pa = (host["b"], host["m"], host["u"], host["up"], l4.KERNEL_DT, plan, l4.KERNEL_S1, l4.KERNEL_S2)
            ca = (host["b"], host["m"], host["us"], l4.KERNEL_DT, plan, l4.KERNEL_S1C, l4.KERNEL_S2)
            us64, _, w64, _ = l4.predict_reference(np.float64, *pa)
            usld, usb, wld, wb = l4.predict_reference(LD, *pa)
            un64, _ = l4.correct_reference(np.float64, *ca)
            unld, unb = l4.correct_reference(LD, *ca)
            for name, lo, hi, bound in (("u_star", us64, usld, usb), ("w", w64, wld, wb), ("u_next", un64, unld, unb)):
                for key, sel in (("plain", ~on), ("boundary", on)):
                    if sel.any():
                        share = 1.0 if name == "u_star" else 0.5
                        r, ok, where = lh.worst_ratio(lo[sel], hi[sel], share * bound[sel])
                        assert ok, (n, bc, name, key, where, r)
                        worst[f"{name} {key}"] = max(worst.get(f"{name} {key}", 0.0), share * r)
    for key, r in sorted(worst.items()):
        print(f"float64 numpy against long double, {key}: worst |error| = {r:.3f} of its bound B")
        assert 0.0 < r <= (1.0 if key.startswith("u_star") else 0.5)


def test_two_entry_length():
    """the length test_gpu_leapfrog4_kernel.py runs so that one thread takes two entries, derived from the launch code"""
    n = l4.two_entry_length()
    assert n == 2 ** 30 + 1
    assert l4.entries_per_thread(n - 1, vec=False) == 1 and l4.entries_per_thread(n, vec=False) == 2
    assert l4.entries_per_thread(2 * n - 1, vec=True) == 1 and l4.entries_per_thread(2 * n, vec=True) == 2
    assert all(l4.entries_per_thread(k, vec) <= 1 for k in (1, 2, 3, 511, 1025) for vec in (False, True))


def test_fourth_order_on_a_closed_domain(oracle):
    """no boundary sets, smooth load: u and v of order >= 3.5 over three halvings of the step from 0.9 dt_max; the
    plain central velocity (the finish without its correction) of order <= 2.5"""
    u0, v0, load, T, dt0 = closed_case(oracle)
    (uref, vref), (du, dv) = closed_reference(oracle)
    eu, ev, ec = [], [], []
    for n in (16, 32, 64, 128):
        u, v = run(oracle, n, T, False, u0, v0, load)
        _, vc = run(oracle, n, T, False, u0, v0, load, correct_v=False)
        eu.append(rel(u, uref)), ev.append(rel(v, vref)), ec.append(rel(vc, vref))
    print(f"closed domain, 16..128 steps: u {eu} orders {orders(eu)}; v {ev} orders {orders(ev)}; "
          f"central velocity {ec} orders {orders(ec)}; reference 512 against 1024 steps: u {du:.2e} v {dv:.2e}")
    # the reference is good enough: above the rounding floor, and below a tenth of the smallest error asserted
    assert 1e-13 < du <= 0.1 * eu[-1] and 1e-13 < dv <= 0.1 * ev[-1]
    assert min(orders(eu)) >= 3.5 and min(orders(ev)) >= 3.5, (orders(eu), orders(ev))
    assert max(orders(ec)) <= 2.5, orders(ec)


def test_numerov_weights_of_the_load(oracle):
    """without the second-difference term of the load (step 4 of the step, and s1c) the scheme is second order"""
    u0, v0, load, T, dt0 = closed_case(oracle)
    (uref, vref), _ = closed_reference(oracle)
    eu = [rel(run(oracle, n, T, False, u0, v0, load, numerov=False)[0], uref) for n in (16, 32, 64, 128)]
    print(f"closed domain without the Numerov term of the load: u {eu} orders {orders(eu)}")
    assert all(1.5 <= o <= 2.5 for o in orders(eu)), orders(eu)


def absorbing_reference(oracle):
    """boundary sets and the plane source over T = 12 * 0.9 dt_max (inside the source's ramp): 3072 steps"""
    if "abs" not in _CACHE:
        dt0 = 0.9 * problem(oracle)[5]
        _CACHE["abs"] = (12 * dt0, run(oracle, 3072, 12 * dt0, True))
    return _CACHE["abs"]


def test_second_order_with_absorbing_sets(oracle):
    """The centred absorbing term stays second order: documented as the limit of the scheme.  Observed order >= 1.8
    over 96, 192, 384 steps: at least 25 steps per source period, so that every run resolves the forcing and the
    ratios are the asymptotic ones (the reasoning of test_leapfrog_host.test_second_order_convergence)."""
    T, (uref, vref) = absorbing_reference(oracle)
    assert T < 4.0 / th.FREQ                                      # the window's ramp does not end inside the run
    eu, ev = [], []
    for n in (96, 192, 384):
        u, v = run(oracle, n, T, True)
        eu.append(rel(u, uref)), ev.append(rel(v, vref))
    print(f"boundary sets and plane source, 96..384 steps: u {eu} orders {orders(eu)}; v {ev} orders {orders(ev)}")
    assert min(orders(eu)) >= 1.8 and min(orders(ev)) >= 1.8, (orders(eu), orders(ev))


@pytest.mark.parametrize("boundary", [False, True])
def test_stable_up_to_sqrt12(oracle, boundary):
    """2000 steps at 0.98 dt_max from a random state at rest, no loads.  Without boundary sets mode k obeys
    u^{n+1} - 2 u^n + u^{n-1} = -y u^n, y = x - x^2/12 in [0, 3], and the start-up gives u^{-1} = (1 - y/2) u^0 exactly,
    so u^n = cos(n theta) u^0: the M-norm never exceeds its initial value (1e-6 for rounding).  With absorbing sets the
    energy with K' only decreases; the norm is held to ten times its initial value, where an unstable step multiplies
    it every few steps.  Leapfrog at the same step overflows."""
    model, K, s1, s2, lam, dtmax, modes, omega = problem(oracle)
    dt = 0.98 * dtmax
    st = th.State(model, boundary=boundary)
    st.u_n[:] = np.random.default_rng(3).uniform(-1, 1, st.m.size)
    hist = []
    t, steps = l4.leapfrog4(st, K, lambda t: 0.0, s2, 0.0, 1.0, dt, max_steps=2000, history=hist)
    norm = np.array([np.sqrt(u @ (st.m * u)) for u in hist])
    print(f"boundary={boundary}: max M-norm over 2000 steps at 0.98 dt_max = {norm.max() / norm[0]:.6f} of the initial one")
    assert steps == 2000 and np.isfinite(norm).all()
    assert norm.max() <= norm[0] * ((1.0 + 1e-6) if not boundary else 10.0)
    lf = th.State(model, boundary=boundary)
    lf.u_n[:] = hist[0]
    with np.errstate(all="ignore"):
        lh.leapfrog(lf, K, lambda t: 0.0, s2, 0.0, 1.0, dt, max_steps=2000)
    assert not np.isfinite(lf.u_n).all() or np.abs(lf.u_n).max() > 1e30


def test_unstable_above_sqrt12(oracle):
    model, K, s1, s2, lam, dtmax, modes, omega = problem(oracle)
    st = th.State(model, boundary=False)
    st.u_n[:] = np.random.default_rng(3).uniform(-1, 1, st.m.size)
    with np.errstate(all="ignore"):
        l4.leapfrog4(st, K, lambda t: 0.0, s2, 0.0, 1.0, 1.02 * dtmax, max_steps=2000)
    assert not np.isfinite(st.u_n).all() or np.abs(st.u_n).max() > 1e30


RECORDED_DRIFT = 1.1e-15      # the float64 stepper's K'-energy drift over 400 steps at 0.9 dt_max, as first measured


def test_modified_energy_is_conserved(oracle):
    """the module docstring's energy: the float64 stepper's drift over 400 steps at 0.9 dt_max within ten times the
    drift recorded for it; the same stepper in long double (100 steps) drifts at least ten times less (not 2^11 times:
    dt2 and c12 stay the host's float64 values, so the energy formula with the exact dt^2/12 is off by a float64 rounding
    of its small second term), so what is measured in float64 is rounding and the scheme conserves the energy with K';
    leapfrog's energy with K alone varies by O(dt^2), at least 1e-4 here"""
    model, K, s1, s2, lam, dtmax, modes, omega = problem(oracle)
    u0, v0, _, _, dt = closed_case(oracle)
    start = u0 + 1e-3 * np.random.default_rng(4).uniform(-1, 1, u0.size)

    def drifts(dtype, Kop, steps):
        st = th.State(model, boundary=False)
        st.m, st.mG1, st.mG2 = (np.asarray(a, dtype=dtype) for a in (st.m, st.mG1, st.mG2))
        st.u_n, st.v_n = np.asarray(start, dtype=dtype), np.asarray(v0, dtype=dtype)
        hist = []
        l4.leapfrog4(st, Kop, lambda t: 0.0, s2, 0.0, 1.0, dt, max_steps=steps, history=hist)
        E = np.array([l4.modified_energy(Kop, st.m, hist[i], hist[i + 1], dt) for i in range(steps)])
        E2 = np.array([lh.energy(Kop, st.m, hist[i], hist[i + 1], dt) for i in range(steps)])
        assert E[0] > 0.0
        return float(np.abs(E - E[0]).max() / abs(E[0])), float(np.abs(E2 - E2[0]).max() / abs(E2[0]))

    A = LD(1) * lh.dense_operator(th.case(oracle, "P2")[2], model.m)
    sm = np.sqrt(np.asarray(model.m, dtype=LD))
    d64, k64 = drifts(np.float64, K, 400)
    dld, _ = drifts(LD, lambda u: -(sm * (A @ (sm * u))), 100)
    print(f"energy with K' drifts by {d64:.2e} over 400 steps at 0.9 dt_max in float64 (recorded {RECORDED_DRIFT:.1e}), by {dld:.2e} "
          f"over 100 steps in long double; leapfrog's energy with K varies by {k64:.2e}")
    assert d64 <= 10.0 * RECORDED_DRIFT
    assert dld <= 0.1 * d64
    assert k64 >= 1e-4


def test_split_run_against_continuous_run(oracle):
    """13 + 19 steps against 32: the start-up is a Taylor series and not the inverse of the finish, so the two differ by
    truncation, not by rounding -- by at most five times the continuous run's own error against the fine reference"""
    model, K, s1, s2, lam, dtmax, modes, omega = problem(oracle)
    u0, v0, load, T, dt0 = closed_case(oracle)
    (uref, vref), _ = closed_reference(oracle)
    n, dt = 32, T / 32
    whole, parts = th.State(model, boundary=False), th.State(model, boundary=False)
    for st in (whole, parts):
        st.u_n[:], st.v_n[:] = u0, v0
    l4.leapfrog4(whole, K, s1, s2, 0.0, 1.0, dt, max_steps=32, load=load)
    t, n1 = l4.leapfrog4(parts, K, s1, s2, 0.0, 1.0, dt, max_steps=13, load=load)
    t, n2 = l4.leapfrog4(parts, K, s1, s2, t, 1.0, dt, max_steps=19, load=load)
    assert (n1, n2) == (13, 19)
    eu, ev = rel(whole.u_n, uref), rel(whole.v_n, vref)
    du, dv = rel(parts.u_n, whole.u_n), rel(parts.v_n, whole.v_n)
    print(f"13 + 19 steps against 32: u {du:.2e} v {dv:.2e}; the continuous run's error u {eu:.2e} v {ev:.2e}")
    assert 1e-13 < du <= 5.0 * eu and 1e-13 < dv <= 5.0 * ev


def test_equal_applies(oracle):
    """the comparison of the module docstring: leapfrog4 at n steps against leapfrog at 2 n steps (no point load:
    leapfrog_helpers.leapfrog has none, so the closed case runs from its initial state alone)"""
    u0, v0, load, T, dt0 = closed_case(oracle)
    fine = run(oracle, 1024, T, False, u0, v0)[0]
    a = rel(run(oracle, 32, T, False, u0, v0)[0], fine)
    b = rel(run(oracle, 64, T, False, u0, v0, scheme="leapfrog")[0], fine)
    Ta, (uabs, _) = absorbing_reference(oracle)
    c = rel(run(oracle, 96, Ta, True)[0], uabs)
    d = rel(run(oracle, 192, Ta, True, scheme="leapfrog")[0], uabs)
    print(f"equal applies: closed domain leapfrog4 at 32 steps {a:.1e}, leapfrog at 64 steps {b:.1e}; "
          f"absorbing leapfrog4 at 96 steps {c:.1e}, leapfrog at 192 steps {d:.1e}")
    assert a < b and np.isfinite([c, d]).all()


def test_refusals_before_any_device_call():
    """null vectors, forbidden aliases, a non-positive step, s2 > 0 and bad stencils are refused on the host: the pointers
    are never followed"""
    import ctypes

    from wave_fenics_amd import _lib
    Lb = _lib.lib()
    n, dt = 100, 0.1
    p = {k: 0x10000 + 0x1000 * i for i, k in enumerate(("b", "m", "u", "up", "us", "w", "un", "v"))}   # disjoint fake addresses

    def predict(**kw):
        a = dict(p, **kw)
        return Lb.wf_leapfrog4_predict(n, a.get("dt", dt), a["b"], a["m"], a["u"], a["up"], a["us"], a["w"], None, 0.0, a.get("s2", 0.0), None)

    def correct(**kw):
        a = dict(p, **kw)
        return Lb.wf_leapfrog4_correct(n, a.get("dt", dt), a["b"], a["m"], a["us"], a["up"], a["un"], a["v"], None, 0.0, a.get("s2", 0.0), None)

    for k in ("b", "m", "u", "up", "us", "w"):
        assert predict(**{k: None}) == -1 and b"null" in Lb.wf_last_error()
    for k in ("u", "b", "m"):
        assert predict(us=p[k]) == -1 and b"alias" in Lb.wf_last_error()
    for k in ("b", "m", "u", "up", "us"):
        assert predict(w=p[k]) == -1 and b"alias" in Lb.wf_last_error()
    assert predict(us=p["up"] + 8) == -1 and b"overlaps" in Lb.wf_last_error()
    for k in ("b", "m", "us", "un"):
        assert correct(**{k: None}) == -1 and b"null" in Lb.wf_last_error()
    assert correct(up=None) == -1 and b"u_prev" in Lb.wf_last_error()
    for k in ("b", "m"):
        assert correct(un=p[k]) == -1 and b"alias" in Lb.wf_last_error()
        assert correct(us=p[k]) == -1 and b"alias" in Lb.wf_last_error()
    assert correct(un=p["us"] + 8) == -1 and b"overlaps" in Lb.wf_last_error()
    assert correct(up=p["un"]) == -1 and correct(up=p["us"]) == -1 and correct(up=p["b"]) == -1
    for k in ("b", "m", "us", "up", "un"):
        assert correct(v=p[k]) == -1 and b"alias" in Lb.wf_last_error()
    for call in (predict, correct):
        for bad in (0.0, -0.1, float("nan")):
            assert call(dt=bad) == -1 and b"time step" in Lb.wf_last_error()
        assert call(s2=1e-300) == -1 and b"s2" in Lb.wf_last_error()
    for nn in (0, -1):                                     # a no-op, whatever the pointers
        assert Lb.wf_leapfrog4_predict(nn, dt, None, None, None, None, None, None, None, 0.0, 0.0, None) == 0
        assert Lb.wf_leapfrog4_correct(nn, dt, None, None, None, None, None, None, None, 0.0, 0.0, None) == 0
    two = (ctypes.c_double * 3)(0.0, 1.0, 2.0)
    assert Lb.wf_sources_add_stencil(None, 1, two, two, p["b"], None) == -1 and b"handle" in Lb.wf_last_error()
    assert Lb.wf_wave_work_vectors(2) == 4
    desc = _lib.WaveDesc()
    st = (ctypes.c_double(0.0), ctypes.c_int64(0))
    assert Lb.wf_wave_leapfrog4(None, 0.0, 1.0, 0.1, -1, p["u"], p["v"], _lib.WAVE_STEP_FN(), None, None, ctypes.byref(st[0]), ctypes.byref(st[1]), None) == -1
    assert Lb.wf_wave_leapfrog4(ctypes.byref(desc), 0.0, 1.0, 0.1, -1, None, p["v"], _lib.WAVE_STEP_FN(), None, None, None, None, None) == -1
    assert b"wf_wave_leapfrog4" in Lb.wf_last_error()
    work = (ctypes.c_void_p * 4)(p["u"], p["up"], p["us"], None)         # the fourth work vector is asked for
    desc.n, desc.d_work = n, work
    assert Lb.wf_wave_leapfrog4(ctypes.byref(desc), 0.0, 1.0, 0.1, -1, p["u"], p["v"], _lib.WAVE_STEP_FN(), None, None, None, None, None) == -1
    assert b"null work" in Lb.wf_last_error()
