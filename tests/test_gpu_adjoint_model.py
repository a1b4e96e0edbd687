"""LinearGLLOpt.misfit_gradient on the device against the numpy adjoint of tests/adjoint_helpers.py, on the scenario of
tests/test_adjoint_host.py: P2 and P4 on the structured box (owner-computes stiffness kernel: bitwise repeatable), P4 on a
perturbed box through the dofmap path (structured=False: atomic accumulation, repeatable to rounding only) and P2 without
a medium.

Bounds.  Gradient and J: 8 x D64 (adjoint_helpers: what float64 rounding does to the numpy gradient, 4e-14 of max|g|), the
margin of the reciprocity test of the point sources.  Directional derivative: 8 x what the float64 numpy stepper reaches
with the same step DIR_H and the same direction (1.2e-9 .. 1.4e-9 of sum |g| |delta a|, truncation).  Without a medium
the model has no coefficient array to move, so that configuration has no directional test."""
import numpy as np
import pytest

import adjoint_helpers as ah
from support import bits, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

#           degree, perturb, medium, structured
CONFIGS = {"P2": (2, 0.0, True, True), "P4": (4, 0.0, True, True), "P4-perturbed-dofmap": (4, 0.2, True, False),
           "P2-no-medium": (2, 0.0, False, True)}
_made = {}


def made(name, gpu):
    """(scenario, numpy float64 adjoint, model, the first misfit_gradient with the default S) of a configuration, once"""
    import torch
    if name not in _made:
        p, perturb, medium, structured = CONFIGS[name]
        sc, g64, _, _ = ah.reference(p, (2, 2, 2), perturb, medium)
        eqn = ah.device_model(sc, gpu, structured)
        if structured:
            assert eqn.stiff_op.update == "owner"
        J, gK, gM, info = eqn.misfit_gradient(0.0, ah.tf(sc), sc.dt, sc.observed)
        torch.cuda.synchronize()
        first = (J, gK.cpu().numpy(), gM.cpu().numpy(), info, eqn.receivers.traces.cpu().numpy().copy(),
                 eqn.u_n.cpu().numpy(), eqn.v_n.cpu().numpy())
        _made[name] = (sc, g64, eqn, first)
    return _made[name]


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_forward_run_is_leapfrog(gpu, name):
    import torch
    sc, _, eqn, first = made(name, gpu)
    ah.reset(eqn, sc, gpu)
    t, steps = eqn.leapfrog(0.0, ah.tf(sc), sc.dt)
    torch.cuda.synchronize()
    assert steps == ah.STEPS == first[3]["N"] == first[3]["steps"] and t == first[3]["t"]
    traces, u, v = eqn.receivers.traces.cpu().numpy(), eqn.u_n.cpu().numpy(), eqn.v_n.cpu().numpy()
    assert traces.shape == (ah.STEPS + 1, 4) and len(eqn.trace_times) == ah.STEPS + 1
    if CONFIGS[name][3]:
        assert same(traces, first[4]) and same(u, first[5]) and same(v, first[6])
    else:
        for a, b in ((traces, first[4]), (u, first[5]), (v, first[6])):
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_gradient_and_misfit_against_numpy(gpu, name):
    sc, g64, _, first = made(name, gpu)
    J, gK, gM = first[:3]
    assert gK.shape == gM.shape == (sc.nc,)
    tol = 8.0 * ah.D64
    eJ = abs(J - float(g64[0])) / float(g64[0])
    e = [float(np.abs(g - r).max() / np.abs(r).max()) for g, r in ((gK, g64[1]), (gM, g64[2]))]
    print(f"ADJOINT model {name}: |g - numpy| / max|g| = {e[0]:.2e} (stiffness) {e[1]:.2e} (mass), J {eJ:.2e}; allowed {tol:.1e}")
    assert max(e) <= tol and eJ <= tol


@pytest.mark.parametrize("name", [k for k in sorted(CONFIGS) if CONFIGS[k][2]])
def test_directional_derivative(gpu, name):
    import torch
    sc, g64, _, first = made(name, gpu)
    structured = CONFIGS[name][3]
    reach, dK, dM = ah.directional(sc, ah.DIR_H, lambda a, b: float(ah.misfit(sc, a, b, np.float64)))
    size = float(np.abs(g64[1]) @ np.abs(dK) + np.abs(g64[2]) @ np.abs(dM))
    reached = abs(reach - float(g64[1] @ dK + g64[2] @ dM))

    def run(aK, aM):
        eqn = ah.device_model(sc, gpu, structured, coefficients=(aK, aM))
        J = eqn.misfit_gradient(0.0, ah.tf(sc), sc.dt, sc.observed)[0]
        torch.cuda.synchronize()
        return J

    fd, _, _ = ah.directional(sc, ah.DIR_H, run)
    gd = float(first[1] @ dK + first[2] @ dM)
    print(f"ADJOINT model {name}: directional FD {fd:.12e}, g.delta {gd:.12e}: {abs(fd - gd) / size:.2e} of sum |g||delta a|, "
          f"numpy reaches {reached / size:.2e}")
    assert abs(fd - gd) <= 8.0 * reached


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_checkpointing_repeats_and_info(gpu, name):
    import torch
    sc, g64, eqn, first = made(name, gpu)
    structured = CONFIGS[name][3]
    N = ah.STEPS
    assert first[3]["S"] == 5 and first[3]["vectors"] == 2 * 5 + 5 + 5            # ceil(sqrt(23)) = 5, 5 segments
    for S in (None, 1, 3, 5, 23, 100):
        ah.reset(eqn, sc, gpu)
        J, gK, gM, info = eqn.misfit_gradient(0.0, ah.tf(sc), sc.dt, torch.from_numpy(sc.observed.copy()).to(gpu), checkpoint_every=S)
        torch.cuda.synchronize()
        gK, gM = gK.cpu().numpy(), gM.cpu().numpy()
        Su = 5 if S is None else S
        assert info["N"] == N and info["S"] == Su
        assert info["vectors"] == 2 * -(-N // Su) + min(Su, N) + 5 and info["bytes"] == info["vectors"] * sc.ndofs * 8
        assert info["launches"] > 10 * N
        if structured:
            assert J == first[0] and same(gK, first[1]) and same(gM, first[2]), f"S = {S}"
            assert same(eqn.receivers.traces.cpu().numpy(), first[4])
        else:
            tol = 8.0 * ah.D64
            assert abs(J - float(g64[0])) <= tol * float(g64[0])
            assert np.abs(gK - g64[1]).max() <= tol * np.abs(g64[1]).max() and np.abs(gM - g64[2]).max() <= tol * np.abs(g64[2]).max()


def test_max_steps_and_appended_rows(gpu):
    """max_steps cuts the run as in leapfrog; rows are appended to what the receivers already hold"""
    import torch
    sc, _, eqn, first = made("P2", gpu)
    ah.reset(eqn, sc, gpu)
    eqn.receivers.record(eqn.u_n, -1.0)
    J, gK, gM, info = eqn.misfit_gradient(0.0, 1.0, sc.dt, sc.observed[:8], max_steps=7)
    torch.cuda.synchronize()
    assert info["N"] == 7 and info["S"] == 3 and eqn.receivers.traces.shape == (9, 4)
    assert same(eqn.receivers.traces.cpu().numpy()[1:], first[4][:8])
    assert J > 0 and np.abs(gK.cpu().numpy()).min() > 0


def test_refusals_come_before_the_first_launch(gpu):
    import torch
    from wave_fenics_amd import points
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    sc, _, eqn, _ = made("P2", gpu)
    ah.reset(eqn, sc, gpu)
    torch.cuda.synchronize()
    before = eqn.u_n.cpu().numpy()

    def untouched():
        torch.cuda.synchronize()
        assert eqn.receivers._rows == 0 and same(eqn.u_n.cpu().numpy(), before)

    for bad in (sc.observed[:-1], sc.observed[:, :3], np.zeros((ah.STEPS + 2, 4)), sc.observed.T):
        with pytest.raises(ValueError):
            eqn.misfit_gradient(0.0, ah.tf(sc), sc.dt, bad)
        untouched()
    with pytest.raises(ValueError):
        eqn.misfit_gradient(0.0, ah.tf(sc), sc.dt, sc.observed, checkpoint_every=0)
    with pytest.raises(ValueError):
        eqn.misfit_gradient(0.0, ah.tf(sc), -sc.dt, sc.observed)
    eqn.updater = object()
    with pytest.raises(NotImplementedError):
        eqn.misfit_gradient(0.0, ah.tf(sc), sc.dt, sc.observed)
    eqn.updater = None
    untouched()
    rec, eqn.receivers = eqn.receivers, None
    with pytest.raises(ValueError):
        eqn.misfit_gradient(0.0, ah.tf(sc), sc.dt, sc.observed)
    eqn.receivers = rec
    untouched()
