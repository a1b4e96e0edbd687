"""LinearGLLOpt.leapfrog / max_eigenvalue / stable_time_step on the device against the numpy stepper of
leapfrog_helpers over the oracle, and the C++ model (planar3d --scheme leapfrog) against both.

Bounds: u_n and v_n to 1e-9 of their maxima over 20 steps (the bound of the RK4 model tests over the same step counts);
a 5 + 5 step run against a 10 step run to 1e-11 (the numpy stepper's own difference is 1e-15: start-up and finish are
exact inverses, the margin covers only the device's rounding order); the discrete energy without boundary sets to 1e-12
over 200 steps; the power iteration within 1 % below the largest eigenvalue and never above it by more than 1e-10."""
import os
import subprocess

import numpy as np
import pytest

import leapfrog_helpers as lh
from medium_helpers import relerr
from support import comm, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C0, FREQ, P0 = 1500.0, 0.5e6, 6e4
N, HI = (4, 4, 6), (0.01, 0.01, 0.015)
STEPS = 20
TOL = 1e-9
_REF = {}


def space(oracle, n, p, hi):
    import wave_fenics_amd as w
    om = oracle.create_box(n, p, hi=hi)
    mesh = w.BoxMesh(om.n, om.x.copy(), om.geom_dofmap.copy(), (0.0, 0.0, 0.0), hi)
    V = w.create_functionspace(mesh, p)
    assert np.array_equal(V.dofmap, om.dofmap)
    return om, mesh, V


def reference(oracle, p, cfl):
    """the numpy stepper's (u, v) after STEPS steps from rest on the (4, 4, 6) box, computed once"""
    key = (p, cfl)
    if key not in _REF:
        om = oracle.create_box(N, p, hi=HI)
        ref = oracle.LinearGLLOpt(om, p, C0, FREQ, P0)
        dt, _ = oracle.cfl_time_step(om, p, C0, FREQ, CFL=cfl)
        ref.init()
        t, steps = lh.leapfrog(ref, *lh.oracle_parts(ref), 0.0, STEPS * dt - 1e-13, dt)
        assert steps == STEPS and np.abs(ref.u_n).max() > 0.0 and np.abs(ref.v_n).max() > 0.0
        _REF[key] = (dt, ref.u_n.copy(), ref.v_n.copy())
    return _REF[key]


@pytest.mark.parametrize("structured", [True, False])
@pytest.mark.parametrize("cfl", [0.25, 0.5])
@pytest.mark.parametrize("p", [2, 4])
def test_leapfrog_vs_numpy_stepper(gpu, oracle, p, cfl, structured):
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    dt, uref, vref = reference(oracle, p, cfl)
    om, mesh, V = space(oracle, N, p, HI)
    eqn = LinearGLLOpt(V, p, C0, FREQ, P0, structured=structured)
    eqn.init()
    t, steps = eqn.leapfrog(0.0, STEPS * dt - 1e-13, dt)
    assert steps == STEPS and abs(t - STEPS * dt) <= 1e-12 * t
    eu, ev = relerr(eqn.u_n.cpu().numpy(), uref), relerr(eqn.v_n.cpu().numpy(), vref)
    print(f"leapfrog P{p} CFL {cfl} structured={structured}: u {eu:.3e} v {ev:.3e}")
    assert eu <= TOL and ev <= TOL
    assert not eqn.b.cpu().numpy().view(np.uint64).any(), "b is left +0.0"


@pytest.mark.parametrize("p", [2, 4])
def test_restart(gpu, oracle, p):
    """5 + 5 steps against 10, and max_steps against the final time"""
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    dt, _, _ = reference(oracle, p, 0.5)
    om, mesh, V = space(oracle, N, p, HI)
    whole, parts = LinearGLLOpt(V, p, C0, FREQ, P0), LinearGLLOpt(V, p, C0, FREQ, P0)
    whole.init()
    parts.init()
    whole.leapfrog(0.0, 10 * dt - 1e-13, dt)
    t, n1 = parts.leapfrog(0.0, 5 * dt - 1e-13, dt)
    t, n2 = parts.leapfrog(t, 1.0, dt, max_steps=5)
    assert (n1, n2) == (5, 5)
    du = relerr(parts.u_n.cpu().numpy(), whole.u_n.cpu().numpy())
    dv = relerr(parts.v_n.cpu().numpy(), whole.v_n.cpu().numpy())
    print(f"restart P{p}: u {du:.3e} v {dv:.3e}")
    assert du <= 1e-11 and dv <= 1e-11


def test_two_layer_medium(gpu, oracle):
    """medium=: against the stepper on test_gpu_medium_model.numpy_model (heterogeneous diagonals and stiffness)"""
    import test_gpu_medium_model as mm
    from wave_fenics_amd import medium as md
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    p = 2
    om, mesh, V = mm.setup(oracle, p)
    med = mm.two_layer(mesh)
    dt, _ = md.cfl_time_step(mesh, p, med, FREQ, CFL=0.5)
    ref = mm.numpy_model(oracle, om, p, med)
    G, _ = oracle.precompute_geometric_data(om, p)
    Ga = np.ascontiguousarray(G * med.stiff_coeff[:, None, None, None])

    def K(u):
        y = np.zeros_like(u)
        oracle.stiffness_apply_sumfact(om, Ga, 1.0, np.ascontiguousarray(u), y)
        return y

    ref.init()
    t, steps = lh.leapfrog(ref, *lh.medium_parts(ref, K), 0.0, STEPS * dt - 1e-13, dt)
    assert steps == STEPS and np.abs(ref.u_n).max() > 0.0
    for structured in (True, False):
        eqn = LinearGLLOpt(V, p, C0, FREQ, P0, structured=structured, medium=med)
        eqn.init()
        eqn.leapfrog(0.0, STEPS * dt - 1e-13, dt)
        eu, ev = relerr(eqn.u_n.cpu().numpy(), ref.u_n), relerr(eqn.v_n.cpu().numpy(), ref.v_n)
        print(f"leapfrog two-layer medium P{p} structured={structured}: u {eu:.3e} v {ev:.3e}")
        assert eu <= TOL and ev <= TOL


@pytest.mark.parametrize("p", [2, 4])
def test_energy_without_boundary_sets(gpu, oracle, p):
    """tags all 0: 1/2 v^T m v - 1/2 u^{n+1 T} K u^n, v = (u^{n+1} - u^n) / dt, recomputed on the host (oracle K and m)
    from the states the device dumps at steps 0, 1 and 199, 200, drifts by <= 1e-12 at stable_time_step(0.9)"""
    import torch
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    om, mesh, V = space(oracle, N, p, HI)
    eqn = LinearGLLOpt(V, p, C0, FREQ, P0, tags={f: 0 for f in range(6)})
    assert eqn.idx1.numel() == 0 and eqn.idx2.numel() == 0
    dt = eqn.stable_time_step(0.9)
    ref = oracle.LinearGLLOpt(om, p, C0, FREQ, P0)
    K, _, _ = lh.oracle_parts(ref)
    x = oracle.dof_coordinates(om) / np.asarray(HI)
    u0 = np.cos(np.pi * x[:, 0]) * np.cos(2 * np.pi * x[:, 1]) + 0.5 * np.cos(np.pi * x[:, 2]) * np.cos(np.pi * x[:, 0])
    eqn.u_n.copy_(torch.from_numpy(u0))
    eqn.v_n.zero_()
    states = [u0]
    t = 0.0
    for steps in (1, 198, 1):
        t, n = eqn.leapfrog(t, 1.0, dt, max_steps=steps)
        assert n == steps
        states.append(eqn.u_n.cpu().numpy())
    E0, E1 = lh.energy(K, ref.m, states[0], states[1], dt), lh.energy(K, ref.m, states[2], states[3], dt)
    drift = abs(E1 - E0) / abs(E0)
    print(f"P{p}: energy {E0:.6e} at step 1/2, {E1:.6e} at step 199 1/2, drift {drift:.2e} (dt = {dt:.4e})")
    assert E0 > 0.0 and np.isfinite(states[3]).all() and drift <= 1e-12


def test_max_eigenvalue(gpu, oracle):
    """P2 4^3 (729 dofs): the power iteration against eigvalsh of the dense M^-1/2 (-K) M^-1/2 from the oracle"""
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    n, p, hi = (4, 4, 4), 2, (0.01, 0.01, 0.01)
    om, mesh, V = space(oracle, n, p, hi)
    ref = oracle.LinearGLLOpt(om, p, C0, FREQ, P0)
    K, _, _ = lh.oracle_parts(ref)
    lam = float(np.linalg.eigvalsh(lh.dense_operator(K, ref.m))[-1])
    eqn = LinearGLLOpt(V, p, C0, FREQ, P0)
    got = eqn.max_eigenvalue(100)
    print(f"max_eigenvalue(100) = {got:.9e}, eigvalsh {lam:.9e}, ratio {got / lam:.6f}")
    assert 0.99 * lam <= got <= lam * (1.0 + 1e-10)
    assert eqn.stable_time_step(0.9, 100) == pytest.approx(0.9 * 2.0 / np.sqrt(got), rel=1e-12)


def test_eigenvalue_needs_one_rank(gpu, comm):
    from wave_fenics_amd.distributed import VectorUpdater, boundary_tags, create_distributed_box
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    part = create_distributed_box((3, 3, 3), 2, 1, 0, periodic=(False, True, False))
    eqn = LinearGLLOpt(part.V, 2, C0, FREQ, P0, updater=VectorUpdater(part, device=gpu, comm=comm), tags=boundary_tags(part), device=gpu)
    for call in (eqn.max_eigenvalue, eqn.stable_time_step):
        with pytest.raises(NotImplementedError):
            call()


def test_periodic_self_neighbour(gpu, comm, oracle):
    """As test_gpu_comm.py::test_periodic_rk4_vs_oracle: the periodic one-rank partition exchanges with itself over
    native RCCL every step -- overlapped (split) and scatter_fwd / apply / scatter_rev (unsplit) -- against the stepper
    on the oracle's periodic mesh, ghosts included."""
    import test_gpu_comm as tc
    from wave_fenics_amd.distributed import VectorUpdater, boundary_tags
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    p, n, periodic, hi = 4, (4, 3, 6), (False, True, True), (0.01, 0.01, 0.01)
    part, om, l2g = tc.periodic_setup(oracle, n, p, periodic, 0.0, hi=hi)
    vu = VectorUpdater(part, device=gpu, comm=comm)
    ref = oracle.LinearGLLOpt(om, p, C0, FREQ, P0)
    dt, _ = oracle.cfl_time_step(om, p, C0, FREQ, CFL=0.25)
    ref.init()
    lh.leapfrog(ref, *lh.oracle_parts(ref), 0.0, STEPS * dt - 1e-13, dt)
    assert np.abs(ref.u_n).max() > 0.0
    for split in (True, False):
        eqn = LinearGLLOpt(part.V, p, C0, FREQ, P0, updater=vu, tags=boundary_tags(part), device=gpu)
        assert eqn._split
        eqn._split = split
        eqn.init()
        t, steps = eqn.leapfrog(0.0, STEPS * dt - 1e-13, dt)
        assert steps == STEPS
        eu, ev = relerr(eqn.u_n.cpu().numpy(), ref.u_n[l2g]), relerr(eqn.v_n.cpu().numpy(), ref.v_n[l2g])
        print(f"periodic self-neighbour split={split}: u {eu:.3e} v {ev:.3e}")
        assert eu <= TOL and ev <= TOL


def test_cxx_demo(gpu, oracle, tmp_path):
    """planar3d --scheme leapfrog --dump on cfg1 (P2, box 0.01^3, x = 0 the source, the rest absorbing) at 6^3 cells:
    against the Python model to 1e-11 and the stepper to 1e-9; --scheme rk4 is the default path"""
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    out = str(tmp_path / "bin")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), f"OUT={out}"])
    p, size, L = 2, 6, 0.01
    om, mesh, V = space(oracle, (size,) * 3, p, (L,) * 3)
    dt, spp = oracle.cfl_time_step(om, p, C0, FREQ, CFL=0.25)
    ref = oracle.LinearGLLOpt(om, p, C0, FREQ, P0)
    ref.init()
    lh.leapfrog(ref, *lh.oracle_parts(ref), 0.0, STEPS * dt - 1e-13, dt)
    eqn = LinearGLLOpt(V, p, C0, FREQ, P0)
    eqn.init()
    eqn.leapfrog(0.0, STEPS * dt - 1e-13, dt)
    dump = str(tmp_path / "uv.bin")
    r = subprocess.run([os.path.join(out, "planar3d"), "--size", str(size), "--degree", str(p), "--cfl", "0.25", "--steps", str(STEPS),
                        "--length", str(L), "--scheme", "leapfrog", "--dump", dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"Number of step per period: {spp}" in r.stdout and f"Steps taken: {STEPS}" in r.stdout
    uv = np.fromfile(dump, dtype=np.float64)
    nd = om.ndofs
    assert uv.size == 2 * nd
    for name, got, py, np_ in (("u", uv[:nd], eqn.u_n.cpu().numpy(), ref.u_n), ("v", uv[nd:], eqn.v_n.cpu().numpy(), ref.v_n)):
        a, b = relerr(got, py), relerr(got, np_)
        print(f"planar3d --scheme leapfrog {name}: against the Python model {a:.3e}, against the stepper {b:.3e}")
        assert a <= 1e-11 and b <= 1e-9
    r = subprocess.run([os.path.join(out, "planar3d"), "--scheme", "heun"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--scheme rk4|leapfrog" in r.stderr
