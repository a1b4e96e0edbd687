"""The dense mass Phi^T diag(det J w) Phi (common/cuda/mass.hpp:18-107) with RECTANGULAR
1-D tables, nq1 != P+1, on the MI355X: the any-rule kernel k_mass_dense (mass_batch.hip) and
the host code around it (batch size, unique-dof tile, LDS size, device det J * w).

Every case runs both constructors -- the reference's argument list (rule, 1-D table and
det J * w built by the library, det J on the device) and explicit phi1 / detJ tables from
the oracle -- starts from a non-zero y (the operator accumulates) and compares with
oracle.dense_mass_apply, the dense Phi [nq][nd] product of the C oracle:

  * P1..P7 with Gauss rules of P+2 and P+3 points (both exact), Basix' GLL rule of the
    reference's default degree P+1 (4, 5, 5, 6 points at P4..P7: nq1 < P+1) and a single
    Gauss point;
  * batch edges (a partial last batch, one cell), more than 64 KB of LDS (16 points),
    more than 2048 batches (the grid-stride loop), reoriented meshes, an element
    permutation, every kernel hint, and the errors a bad table must raise;
  * oracle-free invariants: sum(M 1) = |Omega|, two exact rules agree, M is symmetric and
    positive definite when nq1 >= P+1;
  * the C++ host path, examples/operator_demo --op dense.

Tolerance: one apply against the oracle 1e-12 (fp64, summation order)."""
import os
import re
import subprocess

import numpy as np
import pytest

from support import dev, gpu, make, relerr  # noqa: F401
from test_gpu_unstructured import build_mesh, oracle_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
ORACLE_VARIANT = {"gll_warped": "gll", "equispaced": "equispaced"}


def npts(quad, qd):
    """Basix' point count of the 1-D rule of degree qd."""
    return max(2, (qd + 4) // 2) if quad == "gll" else (qd + 2) // 2


def mass_dense_cells_per_batch(mx):
    """Cells per workgroup of k_mass_dense; mirrors mass_dense_cells_per_batch (mass_batch.hip)."""
    return max(1, min(1400 // mx ** 3, 32))


def lds_bytes(p, m, unique):
    """Dynamic LDS of k_mass_dense: ping/pong tiles [CB][mx^3], phi1 [m][n] and, with the
    batch-unique lists, the unique-dof tile [CB * n^3] (launch_mass_dense)."""
    n = p + 1
    mx = max(n, m)
    CB = mass_dense_cells_per_batch(mx)
    return 8 * (2 * CB * mx ** 3 + m * n + (CB * n ** 3 if unique else 0))


def tables(oracle, om, p, variant, quad, qd):
    pts, wts, phi1, phi, X, W = oracle.tabulate_mass_tables(p, ORACLE_VARIANT[variant], quad, qd)
    assert phi1.shape == (npts(quad, qd), p + 1)
    return pts, wts, phi1, phi, oracle.compute_detJ_generic(om, X, W)


def check_operator(op, y0, x, mx, gpu, m, ncells, nd, what):
    """kernel, sizes and two applies onto y0: y0 + M x, then y0 + 2 M x."""
    assert op.kernel == "mass_dense_any", (what, op.kernel)
    assert op.num_quads() == m ** 3 and op.flops() == 4.0 * ncells * m ** 3 * nd, what
    y, xd = dev(y0, gpu), dev(x, gpu)
    op.apply(xd, y)
    err = relerr(y.cpu().numpy() - y0, mx)
    assert err <= TOL, (what, "first apply", err)
    op.apply(xd, y)
    err = relerr(y.cpu().numpy() - y0, 2 * mx)
    assert err <= TOL, (what, "second apply", err)


def run_case(gpu, oracle, om, V, p, variant, quad, qd, seed=0, tuning=None, perm=None):
    """Both constructors against the oracle; returns (M x, x, op built from the rule)."""
    import wave_fenics_amd as w
    pts, wts, phi1, phi, detJ = tables(oracle, om, p, variant, quad, qd)
    m = phi1.shape[0]
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, om.ndofs)
    mx = np.zeros(om.ndofs)
    oracle.dense_mass_apply(om, phi, detJ, x, mx)
    y0 = rng.uniform(-1, 1, om.ndofs) * np.abs(mx).max()     # same scale as M x: an error in M x cannot hide
    what = (p, variant, quad, qd, m)
    op_rule = w.MassOperator(V, p, variant=variant, quad=quad, qdegree=qd, perm=perm, tuning=tuning)
    assert np.abs(op_rule.points1 - pts).max() <= 3e-16 and np.abs(op_rule.weights1 - wts).max() <= 1e-15
    check_operator(op_rule, y0, x, mx, gpu, m, om.ncells, (p + 1) ** 3, what + ("rule",))
    op_tab = w.MassOperator(V, p, phi1, detJ, perm=perm, tuning=tuning)
    check_operator(op_tab, y0, x, mx, gpu, m, om.ncells, (p + 1) ** 3, what + ("tables",))
    return mx, x, op_rule


def apply(op, x, gpu):
    import torch
    y = torch.zeros(x.size, dtype=torch.float64, device=gpu)
    op.apply(dev(x, gpu), y)
    return y.cpu().numpy()


# --------------------------------------------------------------------------- degrees and rules
# (quad, qd): Gauss with P+2 / P+3 points (exact), the reference's default GLL degree P+1
# (P4..P7: 4, 5, 5, 6 points), a single Gauss point
RULES = [(p, "gauss_jacobi", 2 * p + 2) for p in range(1, 8)] + \
        [(p, "gauss_jacobi", 2 * p + 4) for p in range(1, 8)] + \
        [(p, "gll", p + 1) for p in range(4, 8)] + \
        [(2, "gauss_jacobi", 0), (7, "gauss_jacobi", 0)]
MESH = (5, 3, 3)   # 45 cells: more than one batch and a partial last batch for every CB > 1 below


@pytest.mark.parametrize("p,quad,qd", RULES)
def test_rule_vs_oracle(gpu, oracle, p, quad, qd):
    variant = "gll_warped" if p % 2 == 0 else "equispaced"
    m, n = npts(quad, qd), p + 1
    assert m != n
    CB = mass_dense_cells_per_batch(max(m, n))
    om, mesh, V = make(oracle, MESH, p)
    assert CB == 1 or (om.ncells > CB and om.ncells % CB != 0)
    mx, x, op = run_case(gpu, oracle, om, V, p, variant, quad, qd, seed=p * 100 + qd)
    # oracle-free: sum(M 1) = sum_q det J w = |Omega| = 1 (the boundary stays in its planes) for every rule
    # exact for det J (degree <= 2 per variable); symmetry y^T M x = x^T M y; M > 0 when nq1 >= P+1
    if m >= 2:
        assert abs(apply(op, np.ones(om.ndofs), gpu).sum() - 1.0) <= 1e-13
    yv = np.random.default_rng(qd).uniform(-1, 1, om.ndofs)
    mxd, myd = apply(op, x, gpu), apply(op, yv, gpu)
    a, b = yv @ mxd, x @ myd
    assert abs(a - b) <= 1e-13 * (np.abs(yv) @ np.abs(mxd))
    if m >= n:                      # (an under-integrating rule leaves M only semi-definite)
        assert x @ mxd > 0


@pytest.mark.parametrize("p", range(1, 8))
def test_exact_rules_agree(gpu, p):
    """Gauss with P+2 and with P+3 points both integrate phi_i phi_j det J exactly: the same M x,
    whichever oracle convention -- no oracle involved."""
    import wave_fenics_amd as w
    mesh = w.create_box(MESH, perturb=0.2)
    V = w.create_functionspace(mesh, p)
    x = np.random.default_rng(p).uniform(-1, 1, V.ndofs)
    y1, y2 = (apply(w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=qd), x, gpu)
              for qd in (2 * p + 2, 2 * p + 4))
    assert relerr(y1, y2) <= 1e-13


# --------------------------------------------------------------------------- batch edges, LDS, grid stride
@pytest.mark.parametrize("p,quad,qd", [(2, "gauss_jacobi", 6), (4, "gll", 5)])
def test_one_cell(gpu, oracle, p, quad, qd):
    om, mesh, V = make(oracle, (1, 1, 1), p)
    assert om.ncells < mass_dense_cells_per_batch(max(p + 1, npts(quad, qd)))
    run_case(gpu, oracle, om, V, p, "gll_warped", quad, qd, seed=5)


@pytest.mark.parametrize("p,n", [(3, (2, 1, 2)), (7, (2, 1, 1))])
def test_sixteen_points_above_64k_lds(gpu, oracle, p, n):
    """nq1 = 16 (Gauss of degree 30): the launch raises the workgroup's dynamic LDS limit.
    P3 carries the unique-dof tile, P7 gathers and scatters through the dofmap."""
    m = npts("gauss_jacobi", 30)
    assert m == 16 and mass_dense_cells_per_batch(m) == 1
    assert lds_bytes(p, m, unique=p <= 3) > 65536
    om, mesh, V = make(oracle, n, p)
    run_case(gpu, oracle, om, V, p, "equispaced", "gauss_jacobi", 30, seed=p)


@pytest.mark.parametrize("p,qd,n", [(2, 2, (41, 41, 40)), (4, 10, (25, 25, 21))])
def test_grid_stride_batches(gpu, oracle, p, qd, n):
    """More batches than the 2048 workgroups launched: every workgroup loops.  P2 reloads the
    unique-dof tile in each iteration, P4 runs the dofmap path."""
    m = npts("gauss_jacobi", qd)
    CB = mass_dense_cells_per_batch(max(p + 1, m))
    ncells = n[0] * n[1] * n[2]
    nbatch = (ncells + CB - 1) // CB
    assert (m, CB) == {2: (2, 32), 4: (6, 6)}[p]
    assert nbatch > 2048 and ncells % CB != 0
    om, mesh, V = make(oracle, n, p)
    run_case(gpu, oracle, om, V, p, "gll_warped", "gauss_jacobi", qd, seed=9)


# --------------------------------------------------------------------------- meshes, permutation, hints
@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("kind", ["glued_rotated", "glued_reflected", "random_orient", "ogrid"])
def test_reoriented_meshes(gpu, oracle, kind, p):
    from wave_fenics_amd import mesh_io
    mesh, _ = build_mesh(kind, p)
    V = mesh_io.create_functionspace(mesh, p)
    om = oracle_mesh(oracle, mesh, V)
    # over-integrated Gauss (P+3 points) and an under-integrating rule (P2: 2 Gauss points, P4: 4 GLL points)
    for quad, qd in (("gauss_jacobi", 2 * p + 4), ("gauss_jacobi", 2) if p == 2 else ("gll", 5)):
        run_case(gpu, oracle, om, V, p, "gll_warped", quad, qd, seed=p)


def test_element_permutation(gpu, oracle):
    """An element-ordered dofmap + perm (common/permute.hpp:10-27) with a rectangular table."""
    import wave_fenics_amd as w
    p, n = 3, (3, 2, 2)
    om, mesh, V = make(oracle, n, p)
    rng = np.random.default_rng(17)
    eperm = rng.permutation((p + 1) ** 3).astype(np.int32)
    inv = np.empty_like(eperm)
    inv[eperm] = np.arange(eperm.size, dtype=np.int32)
    Vp = w.FunctionSpace(mesh, p, np.ascontiguousarray(om.dofmap[:, inv]), w.IndexMap(om.ndofs), V.lattice,
                         structured=False)
    run_case(gpu, oracle, om, Vp, p, "equispaced", "gauss_jacobi", 8, seed=4, perm=eperm)


@pytest.mark.parametrize("p,quad,qd", [(2, "gauss_jacobi", 6), (3, "gauss_jacobi", 2), (4, "gll", 5)])
def test_hints_on_rectangular_tables(gpu, oracle, p, quad, qd):
    """Every kernel hint lands on the any-rule kernel for nq1 != P+1; "elementwise" drops the
    unique-dof tile (P <= 3), which shows in the operator's device memory."""
    om, mesh, V = make(oracle, MESH, p)
    nbytes = {}
    for hint in (None, "march", "batch", "mass_any", "elementwise"):
        _, _, op = run_case(gpu, oracle, om, V, p, "gll_warped", quad, qd, seed=3,
                            tuning=None if hint is None else {"kernel": hint})
        nbytes[hint] = op.info.device_bytes
    assert nbytes[None] == nbytes["march"] == nbytes["batch"] == nbytes["mass_any"]
    if p <= 3:
        assert nbytes["elementwise"] < nbytes[None]
    else:
        assert nbytes["elementwise"] == nbytes[None]


def test_bad_tables_raise(gpu, oracle):
    import wave_fenics_amd as w
    p = 2
    om, mesh, V = make(oracle, (2, 2, 1), p)
    nc = om.ncells
    with pytest.raises(w.WavehipError):                     # 17 rows: more than WF_MAX_QUAD_POINTS
        w.MassOperator(V, p, np.full((17, p + 1), 1.0 / (p + 1)), np.ones(nc * 17 ** 3))
    with pytest.raises(w.WavehipError):
        w.quadrature_1d("gauss_jacobi", 32)
    with pytest.raises(w.WavehipError):
        w.MassOperator(V, p, quad="gauss_jacobi", qdegree=32)
    _, _, phi1, _, detJ = tables(oracle, om, p, "equispaced", "gauss_jacobi", 6)
    with pytest.raises(w.WavehipError):                     # detJ of the wrong size
        w.MassOperator(V, p, phi1, detJ.reshape(-1)[:-1])
    with pytest.raises(w.WavehipError):                     # phi1 with P columns, not P+1
        w.MassOperator(V, p, np.ascontiguousarray(phi1[:, :p]), detJ)
    # the library is still usable afterwards
    run_case(gpu, oracle, om, V, p, "equispaced", "gauss_jacobi", 6, seed=1)


# --------------------------------------------------------------------------- C++ host path
def test_cxx_operator_demo_dense(gpu, tmp_path):
    """examples/operator_demo --op dense through wavehip::MassOperator(V, degree, variant, quad, qd):
    the default qdegree P+1 (4-point GLL at P4) and Gauss of degree 10 (6 points).  On the
    undisplaced box, sum(M 1) = |Omega| = sum of the lumped mass."""
    out = str(tmp_path / "bin")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), f"OUT={out}",
                           "CXXFLAGS=-O1 -std=c++17 -Wall -Werror", os.path.join(out, "operator_demo")])
    for extra, m in (([], 4), (["--quad", "gauss", "--qdegree", "10"], 6)):
        r = subprocess.run([os.path.join(out, "operator_demo"), "--op", "dense", "--degree", "4", "--size", "4",
                            "--check", "--reps", "2"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        s = re.search(r"check: sum\(y\) = (\S+)\s+sum\(lumped\) = (\S+)", r.stdout)
        assert s, r.stdout
        sy, sl = float(s.group(1)), float(s.group(2))
        assert abs(sy - sl) <= 1e-12 * abs(sl) and abs(sl - 1.0) <= 1e-12, r.stdout
        assert f"Number of quads: {m ** 3}" in r.stdout, r.stdout
