"""Point sources and receivers on the host, without a GPU: the point location walked under the sanitizers, the package's
locate on holed and shuffled meshes, the interpolation weights against long double, the merge of sources against numpy,
the refusals, and the two physical checks of the numpy stepper that the GPU tests lean on.

Reciprocity (test_reciprocity_of_the_stepper).  Source at A and receiver at B against source at B and receiver at A
(points_helpers.RECIP_*: P4, 4x4x4 cells of a 1 cm box, all faces absorbing, leapfrog, 48 steps of 1e-7 s, Ricker at
1 MHz).  The scheme's transfer matrix is symmetric for symmetric K and diagonal M and D, so the traces differ by rounding
only: measured 1.1e-15 of max|trace| (3.7e-3) on the numpy stepper.  The GPU test allows 8x the value this module measures.

Free space (test_free_space_of_the_stepper).  u_tt - c^2 Lap u = s(t) delta(x - x_s) has u = s(t - r/c) / (4 pi c^2 r).
Geometry: the unit cube in 8x8x8 cells of degree 4 (33 dof planes per axis), c = 1, source at the centre, receiver at
r = 0.15 along the diagonal; Ricker with wavelength 0.28 (9 dof planes per wavelength), delay 1.5/f.  The shortest
source-wall-receiver path is the distance from the receiver to the nearest image source, sqrt((1 - d)^2 + 2 d^2) = 0.9215
with d = 0.15/sqrt(3); the window ends at c t = 0.90 < 0.9215 (checked), so no reflection has arrived, however poor
the absorbing condition.  Measured (120 steps): the stepper's trace differs from the formula by 1.9 % of the formula's maximum --
the discretisation error of a point load at nine planes per wavelength with a second-order time step; the test bounds it by 5 %."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import points_helpers as ph
from support import EPS, LD, wpackage  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_point_locate_walk_sanitized(tmp_path):
    """point_locate.cpp beside tables.cpp (its GLL nodes and the error string) and tests/cxx/point_locate_walk.cpp, built
    into a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer; every check of the walk holds."""
    from wave_fenics_amd import build
    csrc = os.path.join(ROOT, "wave_fenics_amd", "csrc")
    exe = str(tmp_path / "point_locate_walk")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san, "-I", os.path.join(ROOT, "include"),
                           "-I", csrc, os.path.join(csrc, "point_locate.cpp"), os.path.join(csrc, "tables.cpp"),
                           os.path.join(ROOT, "tests", "cxx", "point_locate_walk.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-600:])
    assert out.returncode == 0 and " 0 failures" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
    cases = [ln for ln in out.stdout.splitlines() if ln.startswith("case ")]
    assert len(cases) == 3 * 3 * 4 + 4
    # the residual against a few ulp of the coordinate magnitude for the probes the clamp cannot move, with the clamp's
    # tol term only for the probes on vertices, edges and faces: the worst ratio of each group
    worst = [float(ln.split()[-1]) for ln in out.stdout.splitlines() if ln.startswith("worst residual")]
    assert len(worst) == 2 and all(0.0 < r <= 1.0 for r in worst), worst


def trilinear(xc, xi):
    """x(xi) of cells with vertices xc [..][8][3]"""
    out = 0.0
    for v in range(8):
        N = np.ones(xi.shape[:-1])
        for d in range(3):
            N = N * (xi[..., d] if (v >> d) & 1 else 1.0 - xi[..., d])
        out = out + N[..., None] * xc[..., v, :]
    return out


@pytest.mark.parametrize("name", ["cavity", "pillar-shuffled", "L"])
def test_locate_on_holed_meshes(wpackage, name):
    """points.locate on the holed meshes of nonbox_helpers: random points of every cell of the FULL box come back in
    the cell of the holed mesh that kept them, points of the deleted cells in no cell"""
    import nonbox_helpers as nb
    from wave_fenics_amd import points
    case = nb.holed_case(name, 2)
    full = wpackage.create_box(nb.HOLED_BOX, perturb=nb.PERTURB)
    assert np.array_equal(full.x, case.mesh.x)
    rng = np.random.default_rng(5)
    xi = rng.uniform(0.05, 0.95, size=(full.ncells, 2, 3))
    pts = trilinear(full.x[full.geom_dofmap][:, None], xi)
    index = {tuple(c): i for i, c in enumerate(case.coords)}
    expect = np.array([index.get(tuple(c), -1) for c in nb.cell_coords(nb.HOLED_BOX)])
    assert (expect < 0).any() and (expect >= 0).any()
    cell, ref = points.locate(case.V, pts.reshape(-1, 3))
    assert np.array_equal(cell.reshape(full.ncells, 2), np.repeat(expect[:, None], 2, axis=1))
    found = cell >= 0
    assert np.abs(ref[found] - xi.reshape(-1, 3)[found]).max() <= 1e-10


def test_locate_on_a_mesh_file(wpackage, tmp_path):
    """a mesh with reoriented cells, written to a file and read back (mesh_io), locates every point in the cell the box
    does, at reference coordinates that map back to the point"""
    from wave_fenics_amd import mesh_io, points
    box = wpackage.create_box((3, 2, 2), perturb=0.2)
    V = wpackage.create_functionspace(box, 2)
    pts = np.random.default_rng(2).uniform(0.01, 0.99, size=(50, 3))
    cell, ref = points.locate(V, pts)
    assert (cell >= 0).all()
    turned = mesh_io.reorient_cells(box, [1, 4, 7, 10], [5, 17, 30, 47])
    path = str(tmp_path / "box.xdmf")
    mesh_io.write_mesh(path, "mesh", turned)
    mesh = mesh_io.read_mesh(path, "mesh")
    Vf = mesh_io.create_functionspace(mesh, 2)
    cell_f, ref_f = points.locate(Vf, pts)
    assert np.array_equal(cell_f, cell)
    assert np.abs(trilinear(np.asarray(mesh.x)[np.asarray(mesh.geom_dofmap)[cell_f]], ref_f) - pts).max() <= 1e-12
    same = ~np.isin(cell, [1, 4, 7, 10])
    assert np.abs(ref_f[same] - ref[same]).max() <= 1e-12 and np.abs(ref_f[~same] - ref[~same]).max() > 1e-3


def gll_nodes(w, p):
    return w.tabulate_gll(p)[0]


@pytest.mark.parametrize("p", range(1, 8))
def test_weights_rows(wpackage, p):
    """each 1-D row sums to 1 within (P+1) eps; a coordinate on a node gives an exact 0/1 row"""
    from wave_fenics_amd import points
    nodes = gll_nodes(wpackage, p)
    rng = np.random.default_rng(p)
    ref = np.concatenate([rng.uniform(0.0, 1.0, size=(200, 3)), nodes[rng.integers(0, p + 1, size=(50, 3))],
                          np.nextafter(nodes, 2.0)[rng.integers(0, p, size=(20, 3))]])
    w = points.weights(p, ref)
    assert np.abs(w.astype(LD).sum(axis=2) - 1).max() <= (p + 1) * EPS
    on = ref[:, :, None] == nodes[None, None, :]
    rows = on.any(axis=2)
    assert rows.sum() >= 150
    assert np.array_equal(w[rows], on[rows].astype(np.float64))
    assert np.isfinite(w).all()


@pytest.mark.parametrize("p", range(1, 8))
def test_weights_reproduce_polynomials(wpackage, p):
    """sum_l W_l q(node_l) = q(x) for a random polynomial of degree <= P per variable, within WEIGHT_B eps sum |W||q|
    (points_helpers: the running error analysis of the barycentric form); in reference space and, through locate, on
    an affine anisotropic box, where the residual of locate enters through |grad q|"""
    from wave_fenics_amd import points
    n = p + 1
    nodes = gll_nodes(wpackage, p).astype(LD)
    rng = np.random.default_rng(100 + p)
    coef = rng.uniform(-1.0, 1.0, size=(n, n, n)).astype(LD)

    def q(x, along=None):      # x [..][3] in long double; along = d: the derivative dq/dx_d
        px = [np.stack([x[..., d] ** e if d != along else (e * x[..., d] ** max(e - 1, 0)) for e in range(n)], axis=-1) for d in range(3)]
        return np.einsum("abc,...a,...b,...c->...", coef, px[0], px[1], px[2])

    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    loc = np.stack([nodes[i.reshape(-1)], nodes[j.reshape(-1)], nodes[k.reshape(-1)]], axis=1)     # [nd][3], l = i + n(j + nk)
    ref = rng.uniform(0.0, 1.0, size=(300, 3))
    w = points.weights(p, ref)
    W = ph.tensor_weights(w, LD)
    qn = q(loc)
    got, mag = (W * qn[None]).sum(axis=1), (np.abs(W) * np.abs(qn)[None]).sum(axis=1)
    leb = float(np.abs(w).sum(axis=2).max())
    B = ph.WEIGHT_B(n, leb)
    worst = float((np.abs(got - q(ref.astype(LD))) / (EPS * mag)).max())
    print(f"P{p}: reference space worst |err| / (eps mag) = {worst:.2f}, bound {B:.1f} (Lebesgue {leb:.2f})")
    assert worst <= B
    # through locate on an affine box: the physical polynomial q((x - lo) / (hi - lo)) per cell
    lo, hi = (-0.3, 0.1, 2.0), (1.7, 0.35, 2.9)
    mesh = wpackage.create_box((2, 3, 2), lo=lo, hi=hi)
    V = wpackage.create_functionspace(mesh, p)
    pts = np.asarray(lo) + rng.uniform(0.0, 1.0, size=(200, 3)) * (np.asarray(hi) - np.asarray(lo))
    cell, xi = points.locate(V, pts)
    assert (cell >= 0).all() and xi.min() > 0.0 and xi.max() < 1.0
    xc = mesh.x[mesh.geom_dofmap[cell]].astype(LD)                       # [r][8][3]
    x0, ext = xc[:, 0], xc[:, 7] - xc[:, 0]
    xn = x0[:, None, :] + loc[None] * ext[:, None, :]                    # the cell's nodes in physical space
    phys = lambda x: q((x - np.asarray(lo, dtype=LD)) / (np.asarray(hi, dtype=LD) - np.asarray(lo, dtype=LD)))   # noqa: E731
    w = points.weights(p, xi)
    W = ph.tensor_weights(w, LD)
    qn = phys(xn)
    got, mag = (W * qn).sum(axis=1), (np.abs(W) * np.abs(qn)).sum(axis=1)
    # the residual bound of locate (tests/cxx/point_locate_walk.cpp) moves q by |grad q| times it, to first order
    diam = float(np.linalg.norm(ext.astype(np.float64), axis=1).max())
    # without its clamp term: no point here lies on a cell boundary
    res = 32 * EPS * diam + 4 * EPS * float(np.abs(mesh.x).max())
    s = (pts.astype(LD) - np.asarray(lo, dtype=LD)) / (np.asarray(hi, dtype=LD) - np.asarray(lo, dtype=LD))
    grad = sum(np.abs(q(s, along=d)) / LD(hi[d] - lo[d]) for d in range(3))
    err = np.abs(got - phys(pts.astype(LD)))
    lim = ph.WEIGHT_B(n, float(np.abs(w).sum(axis=2).max())) * EPS * mag + 1.01 * grad * res
    print(f"P{p}: affine box worst |err| / limit = {float((err / lim).max()):.3f}")
    assert (err <= lim).all()


def merged_reference(ndofs, dofs, w):
    """the CSR from numpy: per dof ascending, per source ascending, weights (wx wy) wz, exact zeros dropped"""
    W = ph.tensor_weights(w)
    ent = sorted((int(dofs[s, l]), s, float(W[s, l])) for s in range(dofs.shape[0]) for l in range(dofs.shape[1]) if W[s, l] != 0.0)
    dof = sorted({e[0] for e in ent})
    off = [0]
    for d in dof:
        off.append(off[-1] + sum(1 for e in ent if e[0] == d))
    return np.array(dof), np.array(off), np.array([e[1] for e in ent]), np.array([e[2] for e in ent])


@pytest.mark.parametrize("case", ["one cell", "adjacent cells", "on a node", "duplicates"])
def test_sources_merge(wpackage, case):
    from wave_fenics_amd import points
    p = 2
    mesh = wpackage.create_box((2, 1, 1))
    V = wpackage.create_functionspace(mesh, p)
    xyz = {"one cell": [(0.1, 0.3, 0.7), (0.4, 0.2, 0.6)], "adjacent cells": [(0.3, 0.3, 0.7), (0.8, 0.2, 0.6)],
           "on a node": [(0.25, 0.5, 1.0), (0.3, 0.3, 0.3)], "duplicates": [(0.6, 0.3, 0.7)] * 3}[case]
    dofs, w = ph.host_points(V, xyz)
    dof, off, src, wt = points.merge_sources(p, dofs, w)
    rd, ro, rs, rw = merged_reference(V.ndofs, dofs, w)
    assert np.array_equal(dof, rd) and np.array_equal(off, ro) and np.array_equal(src, rs)
    assert np.array_equal(wt.view(np.int64), rw.view(np.int64))
    assert (np.diff(dof) > 0).all() and (wt != 0.0).all()
    if case == "on a node":
        assert (src == 0).sum() == 1 and wt[src == 0][0] == 1.0          # one dof of the nodal source survives
    if case == "adjacent cells":
        assert (np.diff(off) == 2).sum() == 9                            # the shared face carries both sources
    if case == "duplicates":
        assert (np.diff(off) == 3).all()
    # the dense load it stands for
    vals = np.arange(1.0, len(xyz) + 1.0)
    f = np.zeros(V.ndofs)
    for u in range(dof.size):
        f[dof[u]] = sum(wt[e] * vals[src[e]] for e in range(off[u], off[u + 1]))
    assert np.abs(f - ph.source_vector(V.ndofs, dofs, w, vals)).max() <= 4 * EPS


def test_refusals(wpackage):
    from wave_fenics_amd import _lib, points
    L = _lib.lib()
    ref = np.full((1, 3), 0.5)
    w = np.zeros((1, 3, 9))
    for bad in (0, 8):
        assert L.wf_points_weights(bad, 1, _lib._dp(ref), _lib._dp(w)) == -2 and b"degree" in L.wf_last_error()
        with pytest.raises(_lib.WavehipError):
            points.weights(bad, ref)
    # a dof index out of range: refused before anything is allocated on a device
    dofs = np.arange(8, dtype=np.int32).reshape(1, 8)
    w1 = points.weights(1, ref)
    h = ctypes.c_void_p()
    for bad in (8, -1):
        d = dofs.copy()
        d[0, 3] = bad
        assert L.wf_points_create(1, 8, 1, _lib._ip(d), _lib._dp(w1), ctypes.byref(h)) == -1 and b"out of range" in L.wf_last_error()
        assert not h.value
    assert L.wf_points_create(0, 8, 1, _lib._ip(dofs), _lib._dp(w1), ctypes.byref(h)) == -2 and b"degree" in L.wf_last_error()
    # wavelet tables
    with pytest.raises(ValueError, match="at least 2"):
        points.sampled([1.0], 0.0, 0.1)
    for dt in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="dt"):
            points.sampled([1.0, 2.0], 0.0, dt)
    with pytest.raises(ValueError):
        points.ricker(0.0, 1.0)
    # a receiver outside the mesh, named
    mesh = wpackage.create_box((2, 2, 2))
    V = wpackage.create_functionspace(mesh, 2)
    with pytest.raises(ValueError, match="point 1 "):
        points.Receivers(V, [(0.5, 0.5, 0.5), (0.5, 1.5, 0.5), (2.0, 2.0, 2.0)])
    with pytest.raises(ValueError, match="point 0 "):
        points.Sources(V, [(-0.1, 0.5, 0.5)], [points.ricker(1.0, 1.0)])
    with pytest.raises(ValueError, match="wavelets"):
        points.Sources(V, [(0.1, 0.5, 0.5)], [])


def test_updater_is_refused(wpackage):
    """sources= / receivers= with updater= raise before the model touches a device"""
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    mesh = wpackage.create_box((2, 2, 2))
    V = wpackage.create_functionspace(mesh, 2)
    for kw in ({"sources": object()}, {"receivers": object()}):
        with pytest.raises(NotImplementedError, match="updater="):
            LinearGLLOpt(V, 2, 1500.0, 1e6, 1.0, updater=object(), **kw)


def test_host_wavelets(wpackage):
    """points.wavelet_value (float64) against long double: Ricker before, at and far after the delay, tables at, between
    and outside the nodes"""
    from wave_fenics_amd import points
    rk = points.ricker(2.0, 0.75, 3.0)
    for t in (0.0, 0.3, 0.75, 1.1, 5.0, 1e3):
        got, ref = points.wavelet_value(rk, t), ph.wavelet_ld(rk, t)
        assert np.isfinite(got) and abs(got - ref) <= 64 * EPS * 3.0 * max(1.0, (np.pi * 2.0 * (t - 0.75)) ** 2) * float(np.exp(-min((np.pi * 2.0 * (t - 0.75)) ** 2, 700.0))) + 1e-300
    assert points.wavelet_value(rk, 0.75) == 3.0 and points.wavelet_value(rk, 1e3) == 0.0
    tb = points.sampled([1.0, -2.0, 0.5, 4.0], 0.25, 0.125)
    for k, v in enumerate(tb["values"]):
        assert points.wavelet_value(tb, 0.25 + 0.125 * k) == v
    assert points.wavelet_value(tb, 0.25 + 0.125 * 1.5) == 0.5 * (-2.0) + 0.5 * 0.5
    assert points.wavelet_value(tb, 0.2499) == 0.0 and points.wavelet_value(tb, 0.6251) == 0.0


def test_reciprocity_of_the_stepper(wpackage, oracle):
    ab, ba, diff = ph.recip_host(oracle)
    print(f"reciprocity of the numpy stepper: max|trace| {np.abs(ab).max():.3e}, |AB - BA| / max = {diff:.3e}")
    assert np.abs(ab).max() > 0.0 and diff <= 1e-11
    # the wave has arrived: the trace is no numerical precursor
    assert np.abs(ab[-12:]).max() >= 0.2 * np.abs(ab).max() and np.abs(ab[:8]).max() <= 1e-3 * np.abs(ab).max()
    # negative control: B's weights in the wrong cell break it
    om, V = ph.recip_space(oracle)
    wrong = wpackage.FunctionSpace(V.mesh, V.degree, np.roll(V.dofmap, 1, axis=0), V.index_map, V.lattice, structured=False)
    P = ph.oracle_parts(oracle, om, ph.RECIP_P, ph.RECIP_C0, ph.RECIP_F, 0.0, absorbing_only=True)
    f, _ = ph.load_and_sampler(V, [ph.RECIP_A], [ph.recip_wavelet()], [ph.RECIP_B])
    _, sample = ph.load_and_sampler(wrong, [ph.RECIP_A], [ph.recip_wavelet()], [ph.RECIP_B])
    dt = ph.recip_dt()
    _, _, rows, _ = ph.leapfrog(P, f, sample, 0.0, ph.RECIP_STEPS * dt - 1e-13, dt)
    assert ph.recip_diff(rows[:, 0], ba) > 1e-3


def test_free_space_of_the_stepper(wpackage, oracle):
    from wave_fenics_amd import points
    n, p, c = 8, 4, 1.0
    lam = 0.28
    f0 = c / lam
    d = 0.15 / np.sqrt(3.0)
    src, rec = (0.5, 0.5, 0.5), (0.5 + d, 0.5 + d, 0.5 + d)
    r = float(np.linalg.norm(np.subtract(rec, src)))
    image = min(float(np.linalg.norm(np.subtract(rec, np.where(np.arange(3) == a, 2.0 * side - 0.5, 0.5)))) for a in range(3) for side in (0.0, 1.0))
    t_end = 0.90 / c
    assert abs(image - np.sqrt((1 - d) ** 2 + 2 * d * d)) <= 1e-12 and c * t_end < image      # no reflection inside the window
    assert r / c + 1.5 / f0 + 0.6 / f0 < t_end                                              # the main lobe is inside it
    om = oracle.create_box((n,) * 3, p)
    mesh = wpackage.BoxMesh(om.n, om.x.copy(), om.geom_dofmap.copy())
    V = wpackage.create_functionspace(mesh, p)
    P = ph.oracle_parts(oracle, om, p, c, f0, 0.0, absorbing_only=True)
    wl = points.ricker(f0, 1.5 / f0)
    f, sample = ph.load_and_sampler(V, [src], [wl], [rec])
    dt = 0.7 * 1.4315e-7 * (1500.0 / c) * ((1.0 / n) / 0.0025)        # 0.7 of the limit measured on the 2.5 mm cells of RECIP, scaled
    steps = int(np.ceil(t_end / dt))
    _, done, rows, times = ph.leapfrog(P, f, sample, 0.0, steps * dt - 1e-13, dt)
    assert done == steps and np.isfinite(rows).all()
    exact = np.array([points.wavelet_value(wl, t - r / c) if t >= r / c else 0.0 for t in times]) / (4.0 * np.pi * c * c * r)
    err = float(np.abs(rows[:, 0] - exact).max() / np.abs(exact).max())
    print(f"free space: {steps} steps, max|exact| {np.abs(exact).max():.4e}, max|stepper - exact| / max|exact| = {err:.4f}")
    assert err <= 0.05
