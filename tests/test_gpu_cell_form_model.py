"""LinearGLLOpt.cell_forms() and cell_energy(): the model's cell forms against the model's own operators and against forms
built by hand, and the C++ wrapper's program (tests/cxx/cell_form_checksum.cpp) against Python, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import cell_form_helpers as cf
import stiffness_entry_helpers as se
from support import EPS, LD, bits, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 20
N = (4, 4, 6)
HI = (0.01, 0.01, 0.015)
FREQ, P0 = 0.5e6, 6e4
P = 4


def setup(oracle, p):
    import wave_fenics_amd as w
    om = oracle.create_box(N, p, hi=HI)
    mesh = w.BoxMesh(om.n, om.x.copy(), om.geom_dofmap.copy(), (0.0, 0.0, 0.0), HI)
    V = w.create_functionspace(mesh, p)
    assert np.array_equal(V.dofmap, om.dofmap)
    return om, mesh, V


def two_layer(mesh):
    from wave_fenics_amd.medium import Medium
    return Medium.from_centroids(mesh, lambda xc: (np.where(xc[:, 2] < 0.4 * HI[2], 1500.0, 2800.0),
                                                   np.where(xc[:, 2] < 0.4 * HI[2], 1000.0, 1850.0)))


def test_cell_energy_after_twenty_leapfrog_steps(gpu, oracle):
    """sum_c cell_energy = 1/2 v^T (m .* v) - 1/2 u^T K u with the model's own m and K, within the bounds summed over the
    cells; and every cell against the long-double reference.  The model's side of the comparison is evaluated in long
    double from the device's m and K u: m_d is a sum of at most eight stored det J w a_c (within B_lumped eps of its
    magnitude), (K u)_i is within B_apply eps mag_i + gerr_i of the reference (stiffness_entry_helpers.bound for the
    geometry form the model's operator runs), and sum_i |u_i| mag_i = sum_c mag_c: the allowance of that side is the
    form's own with B_apply in the place of B."""
    import torch
    from wave_fenics_amd import medium as md
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    om, mesh, V = setup(oracle, P)
    med = two_layer(mesh)
    dt, _ = md.cfl_time_step(mesh, P, med, FREQ, CFL=0.25)
    eqn = LinearGLLOpt(V, P, 1500.0, FREQ, P0, medium=med)
    eqn.init()
    _, steps = eqn.leapfrog(0.0, STEPS * dt - 1e-13, dt)
    assert steps == STEPS
    u, v = eqn.u_n.cpu().numpy(), eqn.v_n.cpu().numpy()
    assert np.abs(u).max() > 0 and np.abs(v).max() > 0
    kform, mform = eqn.cell_forms()
    assert eqn.cell_forms()[0] is kform                              # built once
    assert kform.info.cell_coeff == 1 and mform.info.cell_coeff == 1
    energy = eqn.cell_energy()
    torch.cuda.synchronize()
    e = energy.cpu().numpy()
    assert e.shape == (om.ncells,)
    what = "cell" if kform.geometry == "per_cell" else "point"
    geo = se.geometry_ld(om, P, what)
    kref, kmag, kgerr = cf.stiffness_reference(om, P, geo, u, u, a=med.stiff_coeff, c0=1.0)
    mref, mmag, mgerr = cf.lumped_reference(om, P, v, v, a=med.mass_coeff)
    Bk, Bm = cf.bound(what, P), cf.bound("lumped", P)
    ref = LD(0.5) * mref - LD(0.5) * kref
    allowed = LD(0.5) * (LD(Bm) * LD(EPS) * mmag + mgerr) + LD(0.5) * (LD(Bk) * LD(EPS) * kmag + kgerr)
    err = np.abs(e.astype(LD) - ref)
    print(f"CELLFORM model: worst cell uses {float(np.max(err / allowed)):.3f} of its allowance; "
          f"energy {float(ref.sum()):.6e}, cells {float(ref.min()):.3e} .. {float(ref.max()):.3e}")
    assert np.all(err <= allowed)
    assert float(ref.sum()) > 0
    # the model's own operators
    y = torch.zeros_like(eqn.u_n)
    eqn.stiff_op(eqn.u_n, y)
    torch.cuda.synchronize()
    own = LD(0.5) * (v.astype(LD) * eqn.m.cpu().numpy().astype(LD) * v.astype(LD)).sum() \
        - LD(0.5) * (u.astype(LD) * y.cpu().numpy().astype(LD)).sum()
    form = {"per_cell": "axes" if eqn.stiff_op.metric == "axes" else "cell_full", "per_point": "point"}[eqn.stiff_op.geometry]
    Ba = se.bound(form, P)
    both = allowed.sum() + LD(0.5) * (LD(Bm) * LD(EPS) * mmag + mgerr).sum() + LD(0.5) * (LD(Ba) * LD(EPS) * kmag + kgerr).sum()
    gap = abs(e.astype(LD).sum() - own)
    print(f"CELLFORM model: |sum_c e_c - own| = {float(gap):.3e}, allowed {float(both):.3e}, energy {float(own):.6e}")
    assert gap <= both
    # out= is honoured
    out = torch.full((om.ncells,), float("nan"), dtype=torch.float64, device=gpu)
    assert eqn.cell_energy(out) is out
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(e))


def test_cell_forms_with_a_medium_are_the_forms_built_by_hand(gpu, oracle):
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    for p in (2, 4):
        om, mesh, V = setup(oracle, p)
        med = two_layer(mesh)
        lam, u = (torch.from_numpy(np.array(a)).to(gpu) for a in cf.pair(om.ndofs, 70 + p))
        for medium in (med, None):
            eqn = LinearGLLOpt(V, p, 1500.0, FREQ, P0, medium=medium)
            kform, mform = eqn.cell_forms()
            if medium is None:
                hand = (w.CellForm(V, p, "stiffness", {"c0": 1500.0}), w.CellForm(V, p, "mass_lumped"))
            else:
                hand = (w.CellForm(V, p, "stiffness", {"c0": 1.0}, cell_coeff=med.stiff_coeff),
                        w.CellForm(V, p, "mass_lumped", cell_coeff=med.mass_coeff))
            for mine, theirs in zip(hand, (kform, mform)):
                assert (mine.kind, mine.geometry, mine.info.cell_coeff) == (theirs.kind, theirs.geometry, theirs.info.cell_coeff)
                a, b = mine.eval(lam, u), theirs.eval(lam, u)
                torch.cuda.synchronize()
                assert np.abs(a.cpu().numpy()).min() > 0
                assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
                mine.close()


def test_cell_energy_with_updater_raises(gpu, oracle):
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    _, _, V = setup(oracle, 2)
    eqn = LinearGLLOpt(V, 2, 1500.0, FREQ, P0)
    eqn.updater = object()                       # as max_eigenvalue: a partitioned model is refused before any work
    with pytest.raises(NotImplementedError):
        eqn.cell_energy()
    with pytest.raises(NotImplementedError):
        eqn.cell_forms()
    eqn.updater = None


def test_cxx_cell_form_bits(gpu, tmp_path):
    """tests/cxx/cell_form_checksum.cpp: the wrapper's forms on a P2 box with a two-value coefficient; every e_c against
    the same forms created in Python, bit for bit"""
    import torch
    import wave_fenics_amd as w
    import idx_cell_helpers as ich
    from nonbox_helpers import cell_coords
    exe = str(tmp_path / "cell_form_checksum")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "cell_form_checksum.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "wave_fenics_amd"), "-lwavehip",
                           "-Wl,-rpath," + os.path.join(ROOT, "wave_fenics_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for ln in r.stdout.splitlines():
        f = ln.split()
        if len(f) == 7 and f[5] == "bits":
            got.setdefault(f[0], {"geometry": int(f[2]), "bits": []})["bits"].append(int(f[6], 16))
    Pc, n = 2, (9, 3, 5)
    coord = lambda m: np.array([0.75 * i + 0.75 * (i // 2) for i in range(m + 1)])   # noqa: E731
    mesh = ich.box_with(n, x=ich.lattice_x(coord(n[0]), coord(n[1]), coord(n[2])))
    V = w.create_functionspace(mesh, Pc)
    cx, _, cz = cell_coords(n).T
    a = np.where(cx + cz < 5, 1.0, 8.0)
    i = np.arange(V.ndofs, dtype=np.int64)
    u = torch.from_numpy(((i * 7919) % 1009) / 1024.0 - 0.5).to(gpu)
    lam = torch.from_numpy(((i * 104729) % 1013) / 1024.0 + 0.5).to(gpu)
    forms = {"stiffness": (w.CellForm(V, Pc, "stiffness", {"c0": 1500.0}, cell_coeff=a), 2),
             "stiffness_point": (w.CellForm(V, Pc, "stiffness", {"c0": 1500.0}, cell_coeff=a, tuning={"geometry": "per_point"}), 1),
             "lumped": (w.CellForm(V, Pc, "mass_lumped", cell_coeff=a), 0)}
    assert set(got) == set(forms)
    for name, (form, geometry) in forms.items():
        e = form.eval(lam, u)
        torch.cuda.synchronize()
        assert got[name]["geometry"] == geometry == form.info.geometry
        mine = bits(e.cpu().numpy()).view(np.uint64)
        assert np.array_equal(mine, np.array(got[name]["bits"], dtype=np.uint64)), name
        assert np.abs(e.cpu().numpy()).min() > 0
