"""The discrete adjoint of the fourth-order leapfrog loop on the host: the numpy reference of tests/adjoint4_helpers.py
against central finite differences of J in long double, float64 against long double, six wrong adjoints that the
differences must expose, the forward restatement against the stepper of leapfrog4_helpers bit for bit, and the refusals
of misfit_gradient(scheme=...) that need no device.  No GPU; the library's host entry points and the oracle are used."""
from types import SimpleNamespace

import numpy as np
import pytest

import adjoint4_helpers as a4
import adjoint_helpers as ah
import leapfrog4_helpers as l4
from support import LD, wpackage  # noqa: F401


def rel(a, b):
    """max |a - b| over max |b|, per array"""
    return [float(np.abs(np.asarray(a[i], dtype=LD) - b[i]).max() / np.abs(b[i]).max()) for i in range(2)]


@pytest.fixture(scope="module", params=sorted(a4.HOST_CASES))
def case(request, wpackage):
    p, n = a4.HOST_CASES[request.param]
    sc, g64, gld, d64 = a4.reference(p, n)
    fd = a4.finite_differences(sc, LD, ah.FD_H)
    return request.param, sc, g64, gld, d64, fd


def test_scenario_is_what_the_issue_asks(case):
    name, sc, _, gld, _, _ = case
    base = ah.scenario(*a4.HOST_CASES[name])
    assert sc.med is not None and len(set(sc.med.c)) == 2 and len(set(sc.med.rho)) == 2
    assert (sc.c2 > 0).sum() > 0 and (sc.c1 > 0).sum() > 0 and np.abs(sc.u0).max() > 0 and np.abs(sc.v0).max() > 0
    assert sc.observed.shape == (a4.STEPS + 1, 4) and a4.STEPS == 23
    # 0.9 of leapfrog4's limit (three digits), far beyond the step of the second-order scenario, which stays as it was
    K = ah.stiffness_matrix(sc, sc.aK, np.float64)
    m = np.asarray(sc.aM) @ sc.Mc
    lmax = np.abs(np.linalg.eigvals(-K / m[:, None])).max()
    assert abs(sc.dt * np.sqrt(lmax / 12.0) - 0.9) <= 0.005 and sc.dt > 3.0 * base.dt
    assert base.dt == ah.scenario(*a4.HOST_CASES[name]).dt and not np.array_equal(base.observed, sc.observed)
    assert float(gld[0]) > 0 and np.abs(gld[1]).min() > 0 and np.abs(gld[2]).min() > 0


def test_forward_restatement_equals_the_stepper(case):
    """u^0 .. u^N of adjoint4_helpers.forward and of leapfrog4_helpers.leapfrog4: the same bits"""
    from wave_fenics_amd import points
    name, sc, _, _, _, _ = case
    fw = a4.forward(sc, sc.aK, sc.aM, np.float64)
    model = SimpleNamespace(m=fw.m, mG1=sc.c1, mG2=sc.c2, u_n=sc.u0.copy(), v_n=sc.v0.copy())
    SW = a4.ph.source_vector(sc.ndofs, sc.sd, sc.sw, [1.0])
    history = []
    t, steps = l4.leapfrog4(model, lambda x: fw.K @ x, sc.s1, sc.s2, 0.0, a4.tf(sc), sc.dt, history=history,
                            load=lambda t: points.wavelet_value(sc.wavelet, t) * SW)
    assert steps == a4.STEPS == len(fw.ws) and len(history) == a4.STEPS + 1 == len(fw.states) - 1 and t == fw.times[-1]
    for n in range(a4.STEPS + 1):
        assert np.array_equal(history[n], fw.states[n + 1]), f"u^{n}"


def test_adjoint_equals_finite_differences(case):
    """every cell of both arrays, long double: the difference is the truncation error of the differences"""
    name, sc, _, gld, _, fd = case
    e = rel(fd, gld[1:])
    print(f"ADJOINT4 host {name}: |adjoint - FD| / max|g| = {e[0]:.2e} (stiffness) {e[1]:.2e} (mass), h = {ah.FD_H}")
    assert max(e) <= a4.FD_REACHED_4
    assert a4.FD_REACHED_4 <= 4.0 * 1.9e-11        # the recorded value stays what was measured, not a loosened one


def test_float64_against_long_double(case):
    name, sc, g64, gld, d64, _ = case
    dJ = abs(float(g64[0]) - float(gld[0])) / float(gld[0])
    print(f"ADJOINT4 host {name}: d64 = {d64[0]:.2e} (stiffness) {d64[1]:.2e} (mass), J {dJ:.2e}; recorded D64_4 = {a4.D64_4}")
    assert max(d64) <= a4.D64_4 and dJ <= a4.D64_4
    assert a4.D64_4 <= 4.0 * 2.6e-15


@pytest.mark.parametrize("mutant", a4.MUTANTS)
def test_wrong_adjoints_are_exposed(case, mutant):
    name, sc, _, gld, _, fd = case
    good = max(rel(fd, gld[1:]))
    g = a4.adjoint_gradient(sc, sc.aK, sc.aM, LD, mutant)
    bad = max(float(np.abs(fd[i] - g[i + 1]).max() / np.abs(gld[i + 1]).max()) for i in range(2))
    print(f"ADJOINT4 host {name}: mutant {mutant} misses the differences by {bad:.2e}, {bad / good:.2e} times the correct form")
    assert bad / good >= ah.MUTANT_MIN


def test_directional_step_of_the_device_test(case):
    """what the float64 stepper reaches with DIR_H on the quantity the device test compares: truncation, as for leapfrog"""
    name, sc, g64, _, _, _ = case
    d, dK, dM = ah.directional(sc, ah.DIR_H, lambda a, b: float(a4.misfit(sc, a, b, np.float64)))
    gd = float(g64[1] @ dK + g64[2] @ dM)
    size = float(np.abs(g64[1]) @ np.abs(dK) + np.abs(g64[2]) @ np.abs(dM))
    print(f"ADJOINT4 host {name}: directional FD {d:.12e}, g.delta {gd:.12e}, difference {abs(d - gd) / size:.2e} of sum |g||delta|")
    assert abs(d - gd) <= 1.3e-8 * size            # measured 3.2e-9 (P2) and 6.8e-10 (P3)


class _FourReceivers:
    def __len__(self):
        return 4


def test_refusals_that_need_no_device(wpackage):
    """every refusal of misfit_gradient comes before the model's vectors are looked at: an object without them raises
    the refusal itself, for both schemes"""
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    eqn = LinearGLLOpt.__new__(LinearGLLOpt)
    eqn.updater, eqn.sources, eqn.receivers = None, None, _FourReceivers()
    dt, good = 1e-7, np.zeros((a4.STEPS + 1, 4))
    tf = a4.STEPS * dt - 1e-3 * dt
    for scheme in ("leapfrog2", "rk4", "", None, 4):
        with pytest.raises(ValueError, match="scheme"):
            eqn.misfit_gradient(0.0, tf, dt, good, scheme=scheme)
    for scheme in ("leapfrog", "leapfrog4"):
        for bad in (good[:-1], good[:, :3], np.zeros((a4.STEPS + 2, 4)), good.T):
            with pytest.raises(ValueError, match="observed"):
                eqn.misfit_gradient(0.0, tf, dt, bad, scheme=scheme)
        for S in (0, -3):
            with pytest.raises(ValueError, match="checkpoint_every"):
                eqn.misfit_gradient(0.0, tf, dt, good, checkpoint_every=S, scheme=scheme)
        for step in (0.0, -dt, float("nan")):
            with pytest.raises(ValueError, match="time step"):
                eqn.misfit_gradient(0.0, tf, step, good, scheme=scheme)
        eqn.updater = object()
        with pytest.raises(NotImplementedError):
            eqn.misfit_gradient(0.0, tf, dt, good, scheme=scheme)
        eqn.updater, eqn.receivers = None, None
        with pytest.raises(ValueError, match="receivers"):
            eqn.misfit_gradient(0.0, tf, dt, good, scheme=scheme)
        eqn.receivers = _FourReceivers()


def test_loop_with_a_hook_refuses_before_any_launch(wpackage):
    """wf_wave_leapfrog4 with a hook on the made-up descriptors of test_wave_loops_host.py: its refusals without one,
    under its name, and a null entry of d_startup; a refused call writes nothing and calls no hook"""
    import ctypes

    import test_wave_loops_host as wl
    from wave_fenics_amd import _lib
    L = _lib.lib()
    called = []
    hook = _lib.WAVE_STEP_FN(lambda *a: called.append(a) or 0)

    def call(d, startup, u=wl.FAKE + 0x7000, dt=1.0):
        t_end, steps = ctypes.c_double(-1.0), ctypes.c_int64(-1)
        kept = None if startup is None else (ctypes.c_void_p * 3)(*startup)
        rc = L.wf_wave_leapfrog4(None if d is None else ctypes.byref(d), 0.0, 4.5, dt, -1, u, wl.FAKE + 0x8000, hook, None, kept,
                                 ctypes.byref(t_end), ctypes.byref(steps), None)
        assert t_end.value == -1.0 and steps.value == -1 and not called
        return rc, L.wf_last_error().decode()

    good = [wl.FAKE + 0x100000 * (k + 1) for k in range(3)]
    for name, (defect, text) in wl.DESC_DEFECTS.items():
        d = wl.descriptor(_lib)
        defect(d)
        for startup in (None, good):
            assert call(d, startup) == (wl.INVALID, f"wf_wave_leapfrog4: {text}"), name
    assert call(None, good) == (wl.INVALID, "wf_wave_leapfrog4: null descriptor")
    assert call(wl.descriptor(_lib), good, u=None) == (wl.INVALID, "wf_wave_leapfrog4: null state")
    assert call(wl.descriptor(_lib), good, dt=0.0) == (wl.INVALID, "wf_wave_leapfrog4: the time step must be positive")
    for k in range(3):
        startup = [None if j == k else good[j] for j in range(3)]
        assert call(wl.descriptor(_lib), startup) == (wl.INVALID, "wf_wave_leapfrog4: null start-up vector"), k
    assert {"wf_leapfrog4_correlate", "wf_wave_leapfrog4"} <= set(_lib.SIGNATURES)
