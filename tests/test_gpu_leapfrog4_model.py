"""LinearGLLOpt.leapfrog4 / stable_time_step(scheme="leapfrog4") on the device against the numpy stepper of
leapfrog4_helpers over the oracle, and the C++ model (planar3d --scheme leapfrog4) against the Python one.

Bounds: u_n, v_n and every trace row to 1e-9 of their maxima over 20 steps (the bound of the leapfrog and RK4 model
tests over the same step counts); planar3d against the Python model to 1e-11 (test_gpu_leapfrog_model.test_cxx_demo).
Python against C++ bit for bit (test_cxx_bits): both call wf_wave_leapfrog4, so on a P4 box, where the stiffness apply is
the owner kernel (one writer per entry), the two models' u_n and v_n have the same bits.  Each process assembles its own
lumped mass by atomics, which may differ in the last bit (tests/test_gpu_stream_models.py: share_mass): planar3d
--dump-mass writes the C++ model's, and the Python model takes it after the two are shown to agree to 4 eps.  At P2 the
apply itself adds by atomics, so test_cxx_demo there holds 1e-11 and prints the number of differing entries.

Energy on the device (test_energy_on_the_device): the drift of the energy with K' = K + (dt^2/12) K M^-1 K over 200 steps
on the P2 box without boundary sets, evaluated on the host with the oracle's K and m from every state of ONE run (the
states are the operands of the loop's right-hand-side callback, rhs=, which runs the model's own apply: a run split in
two would restart with a Taylor start-up and change the energy by truncation), within ten times the drift of the float64
stepper from the same state, evaluated the same way.

The observed order on the device: the P2 box 3 x 2 x 4 without boundary sets, from a state in the lowest eigenmodes of
the discrete operator (the six lowest that are not constant; the coarsest step has omega dt <= 0.45 for all of them and is at
most 0.9 of the stability limit, so that the orders observed are the asymptotic ones), 8, 16 and 32 steps against the numpy
stepper at 256 steps (its error is 1/4096 of the finest device run's): orders >= 3.5 for u and v."""
import os
import subprocess

import numpy as np
import pytest

import leapfrog4_helpers as l4
import leapfrog_helpers as lh
import points_helpers as ph
from medium_helpers import relerr
from support import bits, comm, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C0, FREQ, P0 = 1500.0, 0.5e6, 6e4
BOXES = {2: ((3, 2, 4), (0.0075, 0.005, 0.01)), 4: ((2, 2, 2), (0.01, 0.01, 0.01))}
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


class Model:
    """what leapfrog4_helpers.leapfrog4 steps: the diagonals of points_helpers.Parts by the stepper's names"""

    def __init__(self, P):
        self.m, self.mG1, self.mG2 = P.m, P.c1, P.c2
        self.u_n, self.v_n = np.zeros_like(P.m), np.zeros_like(P.m)


def reference(oracle, p):
    """the numpy stepper's (dt, u, v) after STEPS steps from rest on the box of degree p, computed once"""
    if p not in _REF:
        n, hi = BOXES[p]
        om = oracle.create_box(n, p, hi=hi)
        ref = oracle.LinearGLLOpt(om, p, C0, FREQ, P0)
        dt, _ = oracle.cfl_time_step(om, p, C0, FREQ, CFL=0.5)
        ref.init()
        t, steps = l4.leapfrog4(ref, *lh.oracle_parts(ref), 0.0, STEPS * dt - 1e-13, dt)
        assert steps == STEPS and np.abs(ref.u_n).max() > 0.0 and np.abs(ref.v_n).max() > 0.0
        _REF[p] = (dt, ref.u_n.copy(), ref.v_n.copy())
    return _REF[p]


@pytest.mark.parametrize("structured", [True, False])
@pytest.mark.parametrize("p", [2, 4])
def test_leapfrog4_vs_numpy_stepper(gpu, oracle, p, structured):
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    dt, uref, vref = reference(oracle, p)
    om, mesh, V = space(oracle, BOXES[p][0], p, BOXES[p][1])
    eqn = LinearGLLOpt(V, p, C0, FREQ, P0, structured=structured)
    eqn.init()
    t, steps = eqn.leapfrog4(0.0, STEPS * dt - 1e-13, dt)
    assert steps == STEPS and abs(t - STEPS * dt) <= 1e-12 * t
    eu, ev = relerr(eqn.u_n.cpu().numpy(), uref), relerr(eqn.v_n.cpu().numpy(), vref)
    print(f"leapfrog4 P{p} structured={structured}: u {eu:.3e} v {ev:.3e}")
    assert eu <= TOL and ev <= TOL
    assert not eqn.b.cpu().numpy().view(np.uint64).any(), "b is left +0.0"
    # max_steps against the final time: the same steps, the same bits where the apply is repeatable
    again = LinearGLLOpt(V, p, C0, FREQ, P0, structured=structured)
    again.init()
    t2, steps2 = again.leapfrog4(0.0, 1.0, dt, max_steps=STEPS)
    assert steps2 == STEPS and relerr(again.u_n.cpu().numpy(), eqn.u_n.cpu().numpy()) <= 1e-11


@pytest.mark.parametrize("name", ["perturbed-p2", "two-layer"])
def test_sources_receivers_and_medium(gpu, oracle, name):
    """the cases of test_gpu_points_model: a perturbed box on the generic path (structured=False) and the two-layer medium,
    each with a Ricker point source and receivers: u_n, v_n and every trace row against the stepper with the load and
    the sampler of points_helpers"""
    import test_gpu_points_model as pm
    V, _, _, parts, dts, src, wl, rec = pm.case(oracle, name)
    dt = dts[0.5]
    f, sample = ph.load_and_sampler(V, src, wl, rec)
    runs = {}
    for key, load in (("points", f), ("plain", None)):
        P, hist = parts(), []
        M = Model(P)
        t, steps = l4.leapfrog4(M, P.K, P.s1, P.s2, 0.0, STEPS * dt - 1e-13 * dt, dt, history=hist, load=load)
        assert steps == STEPS and len(hist) == STEPS + 1
        runs[key] = (np.array([sample(u) for u in hist]), M.u_n.copy(), M.v_n.copy())
    rows, uref, vref = runs["points"]
    assert relerr(runs["plain"][0], rows) >= 0.05, "the point sources matter: without them the traces differ visibly"
    eqn = pm.build(oracle, name)
    eqn.init()
    t, steps = eqn.leapfrog4(0.0, STEPS * dt - 1e-13 * dt, dt)
    assert steps == STEPS
    got = eqn.receivers.traces.cpu().numpy()
    assert got.shape == rows.shape and len(eqn.trace_times) == STEPS + 1
    assert np.abs(np.array(eqn.trace_times) - dt * np.arange(STEPS + 1)).max() <= 1e-12 * STEPS * dt
    scale = np.abs(rows).max()
    worst_row = max(float(np.abs(got[k] - rows[k]).max() / scale) for k in range(STEPS + 1))
    eu, ev = relerr(eqn.u_n.cpu().numpy(), uref), relerr(eqn.v_n.cpu().numpy(), vref)
    print(f"leapfrog4 {name}: worst trace row {worst_row:.3e} of max|traces|, u {eu:.3e} v {ev:.3e}")
    assert worst_row <= TOL and eu <= TOL and ev <= TOL


def test_two_layer_medium_both_paths(gpu, oracle):
    """medium= without points, structured and generic, against the stepper on test_gpu_medium_model.numpy_model"""
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
    t, steps = l4.leapfrog4(ref, *lh.medium_parts(ref, K), 0.0, STEPS * dt - 1e-13, dt)
    assert steps == STEPS and np.abs(ref.u_n).max() > 0.0
    for structured in (True, False):
        eqn = LinearGLLOpt(V, p, C0, FREQ, P0, structured=structured, medium=med)
        eqn.init()
        eqn.leapfrog4(0.0, STEPS * dt - 1e-13, dt)
        eu, ev = relerr(eqn.u_n.cpu().numpy(), ref.u_n), relerr(eqn.v_n.cpu().numpy(), ref.v_n)
        print(f"leapfrog4 two-layer medium P{p} structured={structured}: u {eu:.3e} v {ev:.3e}")
        assert eu <= TOL and ev <= TOL


def test_periodic_self_neighbour(gpu, comm, oracle):
    """As test_gpu_leapfrog_model.test_periodic_self_neighbour: the periodic one-rank partition exchanges with itself
    over native RCCL around both applies of every step -- overlapped (split) and scatter_fwd / apply / scatter_rev
    (unsplit) -- against the stepper on the oracle's periodic mesh, ghosts included."""
    import test_gpu_comm as tc
    from wave_fenics_amd.distributed import VectorUpdater, boundary_tags
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    p, n, periodic, hi = 4, (4, 3, 6), (False, True, True), (0.01, 0.01, 0.01)
    part, om, l2g = tc.periodic_setup(oracle, n, p, periodic, 0.0, hi=hi)
    vu = VectorUpdater(part, device=gpu, comm=comm)
    ref = oracle.LinearGLLOpt(om, p, C0, FREQ, P0)
    dt, _ = oracle.cfl_time_step(om, p, C0, FREQ, CFL=0.25)
    ref.init()
    l4.leapfrog4(ref, *lh.oracle_parts(ref), 0.0, STEPS * dt - 1e-13, dt)
    assert np.abs(ref.u_n).max() > 0.0
    for split in (True, False):
        eqn = LinearGLLOpt(part.V, p, C0, FREQ, P0, updater=vu, tags=boundary_tags(part), device=gpu)
        assert eqn._split
        eqn._split = split
        eqn.init()
        t, steps = eqn.leapfrog4(0.0, STEPS * dt - 1e-13, dt)
        assert steps == STEPS
        eu, ev = relerr(eqn.u_n.cpu().numpy(), ref.u_n[l2g]), relerr(eqn.v_n.cpu().numpy(), ref.v_n[l2g])
        print(f"leapfrog4 periodic self-neighbour split={split}: u {eu:.3e} v {ev:.3e}")
        assert eu <= TOL and ev <= TOL


def test_observed_order_on_the_device(gpu, oracle):
    """the module docstring's order test"""
    import torch
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    p = 2
    n, hi = BOXES[p]
    om, mesh, V = space(oracle, n, p, hi)
    ref = oracle.LinearGLLOpt(om, p, C0, FREQ, P0)
    K, s1, s2 = lh.oracle_parts(ref)
    A = lh.dense_operator(K, ref.m)
    lams, vecs = np.linalg.eigh(A)
    sm = np.sqrt(ref.m)
    first = int(np.argmax(lams > 1e-9 * lams[-1]))               # past the constant mode
    modes, omega = vecs[:, first:first + 6] / sm[:, None], np.sqrt(lams[first:first + 6])
    dt0 = min(0.9 * np.sqrt(12.0 / lams[-1]), 0.45 / omega.max())
    rng = np.random.default_rng(8)
    u0 = modes @ rng.uniform(-1, 1, omega.size)
    v0 = modes @ (rng.uniform(-1, 1, omega.size) * omega)
    T = 8 * dt0

    class Closed:
        m, mG1, mG2 = ref.m, np.zeros_like(ref.m), np.zeros_like(ref.m)

    fine = Closed()
    fine.u_n, fine.v_n = u0.copy(), v0.copy()
    _, steps = l4.leapfrog4(fine, lambda u: -(sm * (A @ (sm * u))), lambda t: 0.0, s2, 0.0, 1.0, T / 256, max_steps=256)
    assert steps == 256
    eqn = LinearGLLOpt(V, p, C0, FREQ, P0, tags={f: 0 for f in range(6)})
    assert eqn.idx1.numel() == 0 and eqn.idx2.numel() == 0
    eu, ev = [], []
    for k in (8, 16, 32):
        eqn.u_n.copy_(torch.from_numpy(u0))
        eqn.v_n.copy_(torch.from_numpy(v0))
        t, steps = eqn.leapfrog4(0.0, 1.0, T / k, max_steps=k)
        assert steps == k
        eu.append(relerr(eqn.u_n.cpu().numpy(), fine.u_n)), ev.append(relerr(eqn.v_n.cpu().numpy(), fine.v_n))
    ou = [float(np.log2(eu[i] / eu[i + 1])) for i in range(2)]
    ov = [float(np.log2(ev[i] / ev[i + 1])) for i in range(2)]
    print(f"device leapfrog4 at 8, 16, 32 steps against the stepper at 256: u {eu} orders {ou}; v {ev} orders {ov}")
    assert eu[-1] > 1e-11 and ev[-1] > 1e-11, "the errors measured stand above the rounding floor"
    assert min(ou) >= 3.5 and min(ov) >= 3.5


def test_stable_beyond_leapfrog(gpu, oracle):
    """stable_time_step(scheme="leapfrog4") is sqrt(3) times the default; at 1.5 times leapfrog's limit
    (stable_time_step(1.0)), with the model's boundary sets and a silent source, 300 steps of leapfrog4 keep the M-norm of
    a random state within ten times its initial value (the reasoning of test_leapfrog4_host.test_stable_up_to_sqrt12),
    where leapfrog multiplies its highest mode by 6.8 per step and overflows"""
    import torch
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    p = 2
    n, hi = BOXES[p]
    om, mesh, V = space(oracle, n, p, hi)
    eqn = LinearGLLOpt(V, p, C0, FREQ, 0.0)
    assert eqn.idx2.numel() > 0
    limit = eqn.stable_time_step(1.0)
    assert eqn.stable_time_step(0.9, scheme="leapfrog4") == pytest.approx(np.sqrt(3.0) * eqn.stable_time_step(0.9), rel=1e-12)
    assert eqn.stable_time_step(1.0, scheme="leapfrog") == limit          # the default, bit for bit
    with pytest.raises(ValueError):
        eqn.stable_time_step(scheme="rk4")
    dt = 1.5 * limit
    u0 = torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, V.ndofs)).to(gpu)
    norm = lambda u: float(torch.sqrt((u * eqn.m * u).sum()).item())   # noqa: E731
    eqn.u_n.copy_(u0)
    eqn.v_n.zero_()
    peak = norm(eqn.u_n)
    t = 0.0
    for _ in range(6):
        t, steps = eqn.leapfrog4(t, 1.0, dt, max_steps=50)
        assert steps == 50
        peak = max(peak, norm(eqn.u_n))
    print(f"leapfrog4 at 1.5 of leapfrog's limit: peak M-norm {peak / norm(u0):.4f} of the initial one over 300 steps")
    assert np.isfinite(peak) and peak <= 10.0 * norm(u0)
    eqn.u_n.copy_(u0)
    eqn.v_n.zero_()
    eqn.leapfrog(0.0, 1.0, dt, max_steps=300)
    assert not bool(torch.isfinite(eqn.u_n).all()) or norm(eqn.u_n) > 1e30 * norm(u0)


def test_energy_on_the_device(gpu, oracle):
    """the module docstring's energy test; also the rhs= callback path of the loop (the torch transport's)"""
    import torch
    from wave_fenics_amd._lib import WF_WAVE_LEAPFROG, WF_WAVE_LEAPFROG4, WF_WAVE_RK4_FUSED
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    p, N = 2, 200
    n, hi = BOXES[p]
    om, mesh, V = space(oracle, n, p, hi)
    eqn = LinearGLLOpt(V, p, C0, FREQ, P0, tags={f: 0 for f in range(6)})
    assert eqn.idx1.numel() == 0 and eqn.idx2.numel() == 0
    dt = eqn.stable_time_step(0.9, scheme="leapfrog4")
    ref = oracle.LinearGLLOpt(om, p, C0, FREQ, P0)
    K, _, s2 = lh.oracle_parts(ref)
    x = oracle.dof_coordinates(om) / np.asarray(hi)
    u0 = np.cos(np.pi * x[:, 0]) * np.cos(2 * np.pi * x[:, 1]) + 0.5 * np.cos(np.pi * x[:, 2]) * np.cos(np.pi * x[:, 0])
    eqn.u_n.copy_(torch.from_numpy(u0))
    eqn.v_n.zero_()
    seen = []

    def rhs(xd, b):
        seen.append(xd.clone())
        eqn.stiff_op(xd, b)

    t, steps = eqn._run(WF_WAVE_LEAPFROG4, 0.0, 1.0, dt, N, rhs=rhs)
    # start-up: K u0, K v0, K a0; per step K u^n, K w; finish: K u^N, K w, K v
    assert steps == N and len(seen) == 3 + 2 * N + 3
    hist = [seen[3 + 2 * k].cpu().numpy() for k in range(N + 1)]
    assert np.array_equal(bits(hist[0]), bits(u0)) and np.array_equal(bits(hist[N]), bits(eqn.u_n.cpu().numpy()))
    with pytest.raises(ValueError):                       # what the library does not have: a hook in rk4_fused ...
        eqn._run(WF_WAVE_RK4_FUSED, 0.0, 1.0, dt, 1, keep=lambda *a: None)
    with pytest.raises(ValueError):                       # ... and start-up derivatives of another loop than leapfrog4
        eqn._run(WF_WAVE_LEAPFROG, 0.0, 1.0, dt, 1, startup=(eqn.u, eqn.v, eqn.b))

    class Closed:
        m, mG1, mG2 = ref.m, np.zeros_like(ref.m), np.zeros_like(ref.m)

    st, href = Closed(), []
    st.u_n, st.v_n = u0.copy(), np.zeros_like(u0)
    l4.leapfrog4(st, K, lambda t: 0.0, s2, 0.0, 1.0, dt, max_steps=N, history=href)

    def drift(h):
        E = np.array([l4.modified_energy(K, ref.m, h[i], h[i + 1], dt) for i in range(N)])
        assert E[0] > 0.0 and np.isfinite(E).all()
        return float(np.abs(E - E[0]).max() / abs(E[0]))

    dd, dh = drift(hist), drift(href)
    print(f"energy with K' over {N} steps at 0.9 of the limit (dt = {dt:.4e}): device drift {dd:.2e}, float64 stepper {dh:.2e}; "
          f"last state against the stepper {relerr(hist[N], href[N]):.2e}")
    assert dd <= 10.0 * dh


def test_cxx_bits(gpu, tmp_path):
    """the module docstring's bit-for-bit comparison: planar3d --scheme leapfrog4 on a P4 box of 3^3 cells against the
    Python model on the same partition description, with the C++ model's lumped mass"""
    import torch
    from wave_fenics_amd.distributed import boundary_tags, create_distributed_box
    from wave_fenics_amd.linear_gll import LinearGLLOpt, cfl_time_step
    out = str(tmp_path / "bin")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), f"OUT={out}"])
    p, size, L = 4, 3, 0.01
    dump, mass = str(tmp_path / "uv.bin"), str(tmp_path / "m.bin")
    r = subprocess.run([os.path.join(out, "planar3d"), "--size", str(size), "--degree", str(p), "--cfl", "0.25", "--steps", str(STEPS),
                        "--length", str(L), "--scheme", "leapfrog4", "--dump", dump, "--dump-mass", mass],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"Steps taken: {STEPS}" in r.stdout, r.stdout + r.stderr
    part = create_distributed_box(size, p, 1, 0, hi=(L, L, L))
    eqn = LinearGLLOpt(part.V, p, C0, FREQ, P0, tags=boundary_tags(part), device=gpu)
    assert eqn.stiff_op.update == "owner"
    nd = eqn.u_n.numel()
    uv, m = np.fromfile(dump, dtype=np.float64), np.fromfile(mass, dtype=np.float64)
    assert uv.size == 2 * nd and m.size == nd
    mine = eqn.m.cpu().numpy()
    assert np.abs(mine - m).max() <= 4 * 2.0 ** -52 * np.abs(m).max()
    print(f"planar3d --dump-mass: {int((bits(mine) != bits(m)).sum())} of {nd} entries of m differ between the two models")
    eqn.m.copy_(torch.from_numpy(m))
    dt, _ = cfl_time_step(part.mesh, p, C0, FREQ, CFL=0.25)
    eqn.init()
    t, steps = eqn.leapfrog4(0.0, STEPS * dt - 1e-13, dt)
    assert steps == STEPS and np.abs(uv).max() > 0.0
    for name, got, py in (("u", uv[:nd], eqn.u_n.cpu().numpy()), ("v", uv[nd:], eqn.v_n.cpu().numpy())):
        off = np.nonzero(bits(got) != bits(py))[0]
        assert off.size == 0, (name, "entries off the Python model", off.size, "first", off[:8], got[off[:4]], py[off[:4]])


def test_cxx_demo(gpu, oracle, tmp_path):
    """planar3d --scheme leapfrog4 --dump on cfg1 (P2, box 0.01^3, x = 0 the source, the rest absorbing) at 6^3 cells:
    against the Python model to 1e-11 and the stepper to 1e-9"""
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    out = str(tmp_path / "bin")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), f"OUT={out}"])
    p, size, L = 2, 6, 0.01
    om, mesh, V = space(oracle, (size,) * 3, p, (L,) * 3)
    dt, spp = oracle.cfl_time_step(om, p, C0, FREQ, CFL=0.25)
    ref = oracle.LinearGLLOpt(om, p, C0, FREQ, P0)
    ref.init()
    l4.leapfrog4(ref, *lh.oracle_parts(ref), 0.0, STEPS * dt - 1e-13, dt)
    eqn = LinearGLLOpt(V, p, C0, FREQ, P0)
    eqn.init()
    eqn.leapfrog4(0.0, STEPS * dt - 1e-13, dt)
    dump = str(tmp_path / "uv.bin")
    r = subprocess.run([os.path.join(out, "planar3d"), "--size", str(size), "--degree", str(p), "--cfl", "0.25", "--steps", str(STEPS),
                        "--length", str(L), "--scheme", "leapfrog4", "--dump", dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"Number of step per period: {spp}" in r.stdout and f"Steps taken: {STEPS}" in r.stdout
    uv = np.fromfile(dump, dtype=np.float64)
    nd = om.ndofs
    assert uv.size == 2 * nd
    for name, got, py, np_ in (("u", uv[:nd], eqn.u_n.cpu().numpy(), ref.u_n), ("v", uv[nd:], eqn.v_n.cpu().numpy(), ref.v_n)):
        a, b = relerr(got, py), relerr(got, np_)
        off = int((bits(got) != bits(py)).sum())
        print(f"planar3d --scheme leapfrog4 {name}: against the Python model {a:.3e} ({off} of {nd} entries differ in their bits), "
              f"against the stepper {b:.3e}")
        assert a <= 1e-11 and b <= 1e-9
    r = subprocess.run([os.path.join(out, "planar3d"), "--scheme", "heun"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--scheme rk4|leapfrog|leapfrog4" in r.stderr
