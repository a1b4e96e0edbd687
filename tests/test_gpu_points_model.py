"""LinearGLLOpt(sources=, receivers=) on the device against the numpy steppers of points_helpers (the oracle's stiffness,
the same load vector and start-up): every row of the traces, for leapfrog, rk4 and rk4_fused, on a P4 box, a perturbed
P2 box with structured=False and a two-layer medium.

Bounds, all taken from the existing model tests: traces to 1e-9 of the reference's maximum (TOL of
test_gpu_leapfrog_model.py, TOL_RK4 of test_gpu_medium_model.py, scaled the same way: support.relerr); a split run against
a continuous one and rk4 against rk4_fused to 1e-11 (test_gpu_leapfrog_model.test_restart, test_gpu_parity).

Reciprocity (test_reciprocity): source at A, receiver at B against source at B, receiver at A, all faces absorbing,
leapfrog (points_helpers.RECIP_*).  The numpy stepper's own difference is 1.1e-15 of max|trace|
(tests/test_points_host.py); the device is allowed 8x what points_helpers.recip_host measures, because it sums K in
another order.  Measured on the MI355X: 3.5e-16 on the device (allowed 8.5e-15); B's weights in the wrong cell give 1.7
(DESIGN.md section 4.17).

Free space: the comparison with s(t - r/c) / (4 pi c^2 r) is a property of the scheme and is made on the numpy stepper
(tests/test_points_host.py, 1.9 %); here the device trace matches the stepper's, which test_traces covers."""
import os

import numpy as np
import pytest

import leapfrog_helpers as lh
import points_helpers as ph
from support import bits, gpu, relerr  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 40
TOL, TOL_SPLIT = 1e-9, 1e-11
_CASE, _REF = {}, {}


def case(oracle, name):
    """what a case needs, built once: (V, model keyword arguments, Parts factory, constants, sources, receivers)"""
    if name in _CASE:
        return _CASE[name]
    import wave_fenics_amd as w
    from wave_fenics_amd import points
    if name == "box-p4":
        p, c0, freq, p0, hi = 4, 1500.0, 0.5e6, 6e4, (0.01, 0.01, 0.01)
        om = oracle.create_box((4, 4, 4), p, hi=hi)
        mesh = w.BoxMesh(om.n, om.x.copy(), om.geom_dofmap.copy(), (0.0, 0.0, 0.0), hi)
        V = w.create_functionspace(mesh, p)
        kw = {}
        parts = lambda: ph.oracle_parts(oracle, om, p, c0, freq, p0)     # noqa: E731
        dts = {cfl: oracle.cfl_time_step(om, p, c0, freq, CFL=cfl)[0] for cfl in (0.25, 0.5)}
        src = [(0.0031, 0.0042, 0.0036), (0.0052, 0.0050, 0.0075)]      # the second on the face z = 0.0075 of two cells
        wl = [points.ricker(1.0e6, 1.5e-6, 2.0e9), points.ricker(0.8e6, 1.2e-6, -1.0e9)]
        rec = [(0.0058, 0.0059, 0.0061), (0.0025, 0.0025, 0.0025), (0.0012, 0.0081, 0.0044)]     # the second on a vertex
    elif name == "perturbed-p2":
        p, c0, freq, p0 = 2, 1.0, 0.5, 1.0
        om = oracle.create_box((3, 3, 3), p, perturb=0.2)
        mesh = w.create_box((3, 3, 3), perturb=0.2)
        assert np.array_equal(mesh.x, om.x)
        V = w.create_functionspace(mesh, p)
        kw = {"structured": False}
        parts = lambda: ph.oracle_parts(oracle, om, p, c0, freq, p0)     # noqa: E731
        dts = {cfl: oracle.cfl_time_step(om, p, c0, freq, CFL=cfl)[0] for cfl in (0.25, 0.5)}
        src = [(0.41, 0.52, 0.37)]
        wl = [points.ricker(2.0, 0.75, 5.0)]
        rec = [(0.62, 0.48, 0.55), (0.2, 0.7, 0.81)]
    else:
        import test_gpu_medium_model as mm
        from wave_fenics_amd import medium as md
        p, c0, freq, p0 = 2, 1500.0, mm.FREQ, mm.P0
        om, mesh, V = mm.setup(oracle, p)
        med = mm.two_layer(mesh)
        kw = {"medium": med}
        G, _ = oracle.precompute_geometric_data(om, p)
        Ga = np.ascontiguousarray(G * med.stiff_coeff[:, None, None, None])

        def K(u):
            y = np.zeros_like(u)
            oracle.stiffness_apply_sumfact(om, Ga, 1.0, np.ascontiguousarray(u), y)
            return y

        def parts():
            ref = mm.numpy_model(oracle, om, p, med)
            return ph.Parts(ref.m, ref.mG1, ref.mG2, *lh.medium_parts(ref, K))
        dts = {cfl: md.cfl_time_step(mesh, p, med, freq, CFL=cfl)[0] for cfl in (0.25, 0.5)}
        src = [(0.0042, 0.0051, 0.0055)]                                 # below the interface at z = 0.006
        wl = [points.ricker(1.0e6, 1.5e-6, 1.0)]
        rec = [(0.0061, 0.0048, 0.0047), (0.0033, 0.0062, 0.0094)]       # one in each layer
    _CASE[name] = (V, (p, c0, freq, p0), kw, parts, dts, src, wl, rec)
    return _CASE[name]


def reference(oracle, name, scheme):
    """(dt, traces, times, u_n, v_n) of the numpy stepper, once per (case, leapfrog | rk4)"""
    kind = "leapfrog" if scheme == "leapfrog" else "rk4"
    if (name, kind) not in _REF:
        V, _, _, parts, dts, src, wl, rec = case(oracle, name)
        dt = dts[0.5 if kind == "leapfrog" else 0.25]
        P = parts()
        f, sample = ph.load_and_sampler(V, src, wl, rec)
        _, steps, rows, times = (ph.leapfrog if kind == "leapfrog" else ph.rk4)(P, f, sample, 0.0, STEPS * dt - 1e-13 * dt, dt)
        assert steps == STEPS and rows.shape == (STEPS + 1, len(rec)) and np.isfinite(rows).all()
        # the point sources matter: without them the traces differ visibly
        _, _, plain, _ = (ph.leapfrog if kind == "leapfrog" else ph.rk4)(parts(), lambda t: 0.0, sample, 0.0, STEPS * dt - 1e-13 * dt, dt)
        assert relerr(plain, rows) >= 0.05, relerr(plain, rows)
        _REF[(name, kind)] = (dt, rows, times, P.u_n.copy(), P.v_n.copy())
    return _REF[(name, kind)]


def build(oracle, name, with_points=True):
    from wave_fenics_amd import points
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    V, (p, c0, freq, p0), kw, _, _, src, wl, rec = case(oracle, name)
    if not with_points:
        return LinearGLLOpt(V, p, c0, freq, p0, **kw)
    return LinearGLLOpt(V, p, c0, freq, p0, sources=points.Sources(V, src, wl), receivers=points.Receivers(V, rec), **kw)


@pytest.mark.parametrize("scheme", ["leapfrog", "rk4", "rk4_fused"])
@pytest.mark.parametrize("name", ["box-p4", "perturbed-p2", "two-layer"])
def test_traces(gpu, oracle, name, scheme):
    dt, rows, times, uref, vref = reference(oracle, name, scheme)
    eqn = build(oracle, name)
    eqn.init()
    t, steps = getattr(eqn, scheme)(0.0, STEPS * dt - 1e-13 * dt, dt)
    assert steps == STEPS
    got = eqn.receivers.traces.cpu().numpy()
    assert got.shape == rows.shape and len(eqn.trace_times) == STEPS + 1
    assert np.abs(np.array(eqn.trace_times) - times).max() <= 1e-12 * times[-1]
    worst = max(relerr(got[:, r], rows[:, r]) for r in range(rows.shape[1]))
    eu, ev = relerr(eqn.u_n.cpu().numpy(), uref), relerr(eqn.v_n.cpu().numpy(), vref)
    print(f"{name} {scheme}: traces {relerr(got, rows):.3e} (worst receiver against its own maximum {worst:.3e}), u {eu:.3e} v {ev:.3e}")
    assert relerr(got, rows) <= TOL and eu <= TOL and ev <= TOL


@pytest.mark.parametrize("scheme", ["leapfrog", "rk4", "rk4_fused"])
def test_split_run(gpu, oracle, scheme):
    """25 + 15 steps against 40: the traces concatenated, the duplicated row (recorded at the end of the first call and
    at the start of the second) dropped"""
    name = "box-p4"
    dt = reference(oracle, name, scheme)[0]
    whole, parts = build(oracle, name), build(oracle, name)
    whole.init()
    parts.init()
    getattr(whole, scheme)(0.0, STEPS * dt - 1e-13 * dt, dt)
    t, n1 = getattr(parts, scheme)(0.0, 1.0, dt, max_steps=25)
    first = parts.receivers.traces.cpu().numpy().copy()
    t, n2 = getattr(parts, scheme)(t, 1.0, dt, max_steps=15)
    assert (n1, n2) == (25, 15)
    both = parts.receivers.traces.cpu().numpy()
    assert both.shape[0] == STEPS + 2 and np.array_equal(bits(both[:26]), bits(first))
    assert parts.trace_times[25] == parts.trace_times[26]
    d_dup = relerr(both[26], both[25])
    joined = np.concatenate([both[:26], both[27:]])
    d = relerr(joined, whole.receivers.traces.cpu().numpy())
    print(f"split run {scheme}: duplicated row {d_dup:.3e}, joined traces against the continuous run {d:.3e}")
    assert d_dup <= TOL_SPLIT and d <= TOL_SPLIT
    parts.receivers.reset()
    assert parts.receivers.traces.shape[0] == 0 and parts.trace_times == []


def test_rk4_and_fused_agree(gpu, oracle):
    name = "box-p4"
    dt = reference(oracle, name, "rk4")[0]
    out = []
    for scheme in ("rk4", "rk4_fused"):
        eqn = build(oracle, name)
        eqn.init()
        getattr(eqn, scheme)(0.0, STEPS * dt - 1e-13 * dt, dt)
        out.append(eqn.receivers.traces.cpu().numpy())
    d = relerr(out[1], out[0])
    print(f"rk4 against rk4_fused traces: {d:.3e}")
    assert d <= TOL_SPLIT


@pytest.mark.parametrize("scheme", ["leapfrog", "rk4", "rk4_fused"])
def test_without_points_nothing_changes(gpu, oracle, scheme):
    """sources=None, receivers=None: the states are bit for bit those of a model built without the arguments (on the
    owner-computes stiffness kernel and one lumped mass for both, as tools/time_step_bits.py: the default stiffness
    kernel of this box and the lumped-mass set-up add with atomics and do not repeat their own bits; tags with disjoint
    boundary sets, as there: the unfused boundary launch adds a dof of both sets from two threads)"""
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    V, (p, c0, freq, p0), kw, _, dts, _, _, _ = case(oracle, "box-p4")
    kw = dict(kw, tuning={"update": "owner"}, tags={0: 1, 1: 2})
    a = LinearGLLOpt(V, p, c0, freq, p0, **kw)
    b = LinearGLLOpt(V, p, c0, freq, p0, sources=None, receivers=None, **kw)
    assert a.stiff_op.update == "owner" and b.stiff_op.update == "owner"
    assert float((a.m - b.m).abs().max() / a.m.abs().max()) < 1e-14
    b.m.copy_(a.m)
    for eqn in (a, b):
        eqn.init()
        getattr(eqn, scheme)(0.0, 10 * dts[0.25] - 1e-13 * dts[0.25], dts[0.25])
    assert np.abs(a.u_n.cpu().numpy()).max() > 0.0 and b.trace_times == []
    assert np.array_equal(bits(a.u_n.cpu().numpy()), bits(b.u_n.cpu().numpy()))
    assert np.array_equal(bits(a.v_n.cpu().numpy()), bits(b.v_n.cpu().numpy()))


def recip_run(oracle, V_rec, s, r):
    from wave_fenics_amd import points
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    om, V = ph.recip_space(oracle)
    eqn = LinearGLLOpt(V, ph.RECIP_P, ph.RECIP_C0, ph.RECIP_F, 0.0, tags={f: 2 for f in range(6)},
                       sources=points.Sources(V, [s], [ph.recip_wavelet()]), receivers=points.Receivers(V_rec or V, [r]))
    eqn.init()
    dt = ph.recip_dt()
    _, steps = eqn.leapfrog(0.0, ph.RECIP_STEPS * dt - 1e-13 * dt, dt)
    assert steps == ph.RECIP_STEPS
    return eqn.receivers.traces.cpu().numpy()[:, 0]


def test_reciprocity(gpu, oracle):
    import wave_fenics_amd as w
    host_ab, host_ba, host = ph.recip_host(oracle)
    ab, ba = recip_run(oracle, None, ph.RECIP_A, ph.RECIP_B), recip_run(oracle, None, ph.RECIP_B, ph.RECIP_A)
    d = ph.recip_diff(ab, ba)
    print(f"reciprocity: device |AB - BA| / max|trace| = {d:.3e}, numpy stepper {host:.3e}, allowed {8 * host:.3e}; "
          f"device against the stepper {relerr(ab, host_ab):.3e}")
    assert relerr(ab, host_ab) <= TOL and relerr(ba, host_ba) <= TOL
    # negative control: B's weights applied in the wrong cell must fail the check
    om, V = ph.recip_space(oracle)
    wrong = w.FunctionSpace(V.mesh, V.degree, np.roll(V.dofmap, 1, axis=0), V.index_map, V.lattice, structured=False)
    bad = ph.recip_diff(recip_run(oracle, wrong, ph.RECIP_A, ph.RECIP_B), ba)
    print(f"reciprocity, receiver weights in the wrong cell: {bad:.3e}")
    assert bad > 8 * host and bad > 1e-3
    assert d <= 8 * host


def test_cxx_demo_traces(gpu, oracle, tmp_path):
    """planar3d --source --receiver --traces (the C++ model: wavehip::Sources, wavehip::Receivers, set_sources,
    set_receivers) reproduces the Python model's traces, for each loop, to the 1e-11 to which planar3d reproduces the
    Python states (test_gpu_leapfrog_model.test_cxx_demo); --amplitude 0 silences the plane source, so the traces are the
    point source's alone"""
    import subprocess
    from wave_fenics_amd import points
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    out = str(tmp_path / "bin")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), f"OUT={out}"])
    V, (p, c0, freq, _), _, _, dts, _, _, _ = case(oracle, "box-p4")
    src, f0 = (0.0031, 0.0042, 0.0036), 1.0e6
    rec = [(0.0058, 0.0059, 0.0061), (0.0025, 0.0025, 0.0025)]
    for scheme, flags, cfl in (("leapfrog", ["--scheme", "leapfrog"], 0.5), ("rk4_fused", [], 0.25), ("rk4", ["--reference-order"], 0.25)):
        dt = dts[cfl]
        eqn = LinearGLLOpt(V, p, c0, freq, 0.0, sources=points.Sources(V, [src], [points.ricker(f0, 1.5 / f0)]),
                           receivers=points.Receivers(V, rec))
        eqn.init()
        getattr(eqn, scheme)(0.0, STEPS * dt - 1e-13, dt)
        want = eqn.receivers.traces.cpu().numpy()
        path = str(tmp_path / f"traces_{scheme}.txt")
        cmd = [os.path.join(out, "planar3d"), "--size", "4", "--degree", str(p), "--cfl", str(cfl), "--steps", str(STEPS), "--length", "0.01",
               "--amplitude", "0", "--source", ",".join(repr(v) for v in (*src, f0)), "--traces", path, *flags]
        for r in rec:
            cmd += ["--receiver", ",".join(repr(v) for v in r)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f"Steps taken: {STEPS}" in r.stdout, r.stdout + r.stderr
        got = np.loadtxt(path)
        assert got.shape == (STEPS + 1, 1 + len(rec)) and np.abs(want).max() > 0.0
        assert np.abs(got[:, 0] - np.array(eqn.trace_times)).max() <= 1e-12 * got[-1, 0]
        d = relerr(got[:, 1:], want)
        print(f"planar3d {scheme} traces against the Python model: {d:.3e}")
        assert d <= TOL_SPLIT
    r = subprocess.run([os.path.join(out, "planar3d"), "--traces", path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--receiver" in r.stderr
