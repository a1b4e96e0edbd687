"""The discrete adjoint of the leapfrog loop on the host: the numpy reference of tests/adjoint_helpers.py against central
finite differences of J in long double, float64 against long double, and three wrong adjoints that the differences must
expose.  No GPU; the library's host entry points (facet masses, point weights) and the oracle are used."""
import numpy as np
import pytest

import adjoint_helpers as ah
from support import LD, wpackage  # noqa: F401


def rel(a, b):
    """max |a - b| over max |b|, per array"""
    return [float(np.abs(np.asarray(a[i], dtype=LD) - b[i]).max() / np.abs(b[i]).max()) for i in range(2)]


@pytest.fixture(scope="module", params=sorted(ah.HOST_CASES))
def case(request, wpackage):
    p, n = ah.HOST_CASES[request.param]
    sc, g64, gld, d64 = ah.reference(p, n)
    fd = ah.finite_differences(sc, LD, ah.FD_H)
    return request.param, sc, g64, gld, d64, fd


def test_scenario_is_what_the_issue_asks(case):
    name, sc, _, gld, _, _ = case
    assert sc.med is not None and len(set(sc.med.c)) == 2 and len(set(sc.med.rho)) == 2
    assert (sc.c2 > 0).sum() > 0 and (sc.c1 > 0).sum() > 0 and np.all(sc.c2[sc.c1 > 0] > 0)      # the plane face absorbs too
    from wave_fenics_amd import points
    assert points.wavelet_value(sc.wavelet, 0.0) != 0.0
    assert np.abs(sc.u0).min() >= 0 and np.abs(sc.u0).max() > 0 and np.abs(sc.v0).max() > 0
    assert sc.rec[0][0] == sc.rec[0][1] and sc.observed.shape == (ah.STEPS + 1, 4)
    W = ah.ph.tensor_weights(sc.rw)
    assert np.count_nonzero(W[2]) == 1 and W[2].max() == 1.0                                     # receiver 2 sits on a node
    assert float(gld[0]) > 0 and np.abs(gld[1]).min() > 0 and np.abs(gld[2]).min() > 0


def test_adjoint_equals_finite_differences(case):
    """every cell of both arrays, long double: the difference is the truncation error of the differences"""
    name, sc, _, gld, _, fd = case
    e = rel(fd, gld[1:])
    print(f"ADJOINT host {name}: |adjoint - FD| / max|g| = {e[0]:.2e} (stiffness) {e[1]:.2e} (mass), h = {ah.FD_H}")
    assert max(e) <= ah.FD_REACHED


def test_float64_against_long_double(case):
    name, sc, g64, gld, d64, _ = case
    dJ = abs(float(g64[0]) - float(gld[0])) / float(gld[0])
    print(f"ADJOINT host {name}: d64 = {d64[0]:.2e} (stiffness) {d64[1]:.2e} (mass), J {dJ:.2e}; recorded D64 = {ah.D64}")
    assert max(d64) <= ah.D64 and dJ <= ah.D64
    assert ah.D64 <= 4.0 * 3.8e-14          # the recorded value stays what was measured, not a loosened one


@pytest.mark.parametrize("mutant", ["swap", "no_startup", "late"])
def test_wrong_adjoints_are_exposed(case, mutant):
    name, sc, _, gld, _, fd = case
    good = max(rel(fd, gld[1:]))
    g = ah.adjoint_gradient(sc, sc.aK, sc.aM, LD, mutant)
    bad = max(float(np.abs(fd[i] - g[i + 1]).max() / np.abs(gld[i + 1]).max()) for i in range(2))
    print(f"ADJOINT host {name}: mutant {mutant} misses the differences by {bad:.2e}, {bad / good:.2e} times the correct form")
    assert bad / good >= ah.MUTANT_MIN


def test_directional_step_of_the_device_test(case):
    """what the float64 stepper reaches with DIR_H on the quantity the device test compares"""
    name, sc, g64, _, _, _ = case
    d, dK, dM = ah.directional(sc, ah.DIR_H, lambda a, b: float(ah.misfit(sc, a, b, np.float64)))
    gd = float(g64[1] @ dK + g64[2] @ dM)
    size = float(np.abs(g64[1]) @ np.abs(dK) + np.abs(g64[2]) @ np.abs(dM))
    print(f"ADJOINT host {name}: directional FD {d:.12e}, g.delta {gd:.12e}, difference {abs(d - gd) / size:.2e} of sum |g||delta|")
    assert abs(d - gd) <= 5e-9 * size
