"""Known-answer tests pinning the CPU oracle (oracle/wave_oracle.{py,c}).

The reference ships no golden vectors (parity unpinned), so the
restatement is pinned by analytic identities of the operators it restates:
  sum(M 1) = |Omega|, K const = 0, x^T K x = -c0^2 |Omega| for x = X-coordinate,
  K symmetric, dense (reference form) == sum-factorised.
"""
import numpy as np
import pytest


@pytest.mark.parametrize("n", [2, 3, 4, 5, 7, 8])
def test_gll_rule(oracle, n):
    x, w = oracle.gll_points_weights(n)
    assert x[0] == 0.0 and x[-1] == 1.0
    assert np.all(np.diff(x) > 0)
    assert abs(w.sum() - 1.0) < 1e-15
    # exact for polynomials up to degree 2n-3
    for d in range(2 * n - 2):
        assert abs(np.dot(w, x ** d) - 1.0 / (d + 1)) < 1e-14


def test_gll_known_values(oracle):
    x, w = oracle.gll_points_weights(3)
    assert np.allclose(x, [0, 0.5, 1]) and np.allclose(w, [1 / 6, 4 / 6, 1 / 6])
    x, w = oracle.gll_points_weights(5)
    ref = 0.5 * (1 + np.array([-1, -np.sqrt(3 / 7), 0, np.sqrt(3 / 7), 1]))
    assert np.allclose(x, ref, atol=1e-15)
    assert np.allclose(w, 0.5 * np.array([0.1, 49 / 90, 32 / 45, 49 / 90, 0.1]), atol=1e-15)


def test_derivative_matrix_p2(oracle):
    _, _, phi, D = oracle.tabulate_1d_gll(2)
    assert np.array_equal(phi, np.eye(3))
    assert np.allclose(D, [[-3, 4, -1], [-1, 0, 1], [1, -4, 3]], atol=1e-14)


@pytest.mark.parametrize("p", [2, 3, 4])
def test_dense_table_structure(oracle, p):
    perm, table = oracle.tabulate_basis_and_permutation(p)
    nd = (p + 1) ** 3
    assert table.shape == (4, nd, nd)
    assert np.array_equal(table[0], np.eye(nd))          # collocation: Phi is the identity
    # derivative rows sum to zero (derivative of the constant)
    assert np.abs(table[1:].sum(axis=2)).max() < 1e-12
    assert np.array_equal(perm, np.arange(nd))


@pytest.mark.parametrize("p,n,perturb", [(2, 3, 0.0), (2, 3, 0.2), (4, 2, 0.2), (3, (3, 2, 2), 0.15)])
def test_mass_sums_to_volume(oracle, p, n, perturb):
    mesh = oracle.create_box(n, p, perturb=perturb)
    op = oracle.MassOperatorCPU(mesh, p)
    m = np.zeros(mesh.ndofs)
    op(np.ones(mesh.ndofs), m)
    assert abs(m.sum() - 1.0) < 1e-13
    assert m.min() > 0


@pytest.mark.parametrize("p,n,perturb", [(2, 3, 0.0), (2, 3, 0.2), (4, 2, 0.2), (5, 2, 0.1)])
def test_stiffness_kats(oracle, p, n, perturb):
    mesh = oracle.create_box(n, p, perturb=perturb)
    K = oracle.StiffnessOperator(mesh, p)
    c0 = 1500.0
    N = mesh.ndofs
    # K const = 0
    y = np.zeros(N)
    K(np.ones(N), y)
    assert np.abs(y).max() < 1e-6 * c0 * c0 * 1e-2
    # x^T K x = -c0^2 |Omega| for x = X coordinate (|grad x|^2 = 1)
    X = oracle.dof_coordinates(mesh)
    y[:] = 0
    K(X[:, 0].copy(), y)
    assert abs(np.dot(X[:, 0], y) / (-c0 * c0) - 1.0) < 1e-9   # clamp of G, see below
    # mixed: x^T K y = 0 for the X and Y coordinates.  Only to 1e-7: the
    # reference clamps |G| <= 1e-8 to zero (precomputation.hpp:105-107), which
    # perturbs small off-diagonal entries of G on distorted cells.
    assert abs(np.dot(X[:, 1], y) / (c0 * c0)) < 1e-7
    # symmetry
    rng = np.random.default_rng(0)
    u, v = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
    Ku, Kv = np.zeros(N), np.zeros(N)
    K(u, Ku)
    K(v, Kv)
    assert abs(np.dot(v, Ku) - np.dot(u, Kv)) < 1e-12 * abs(np.dot(v, Ku))
    # accumulate semantics: y += K x
    y2 = Ku.copy()
    K(u, y2)
    assert np.allclose(y2, 2 * Ku, rtol=1e-14)


@pytest.mark.parametrize("p,n", [(2, 3), (4, 2), (6, 1)])
def test_dense_equals_sumfact(oracle, p, n):
    mesh = oracle.create_box(n, p, perturb=0.2)
    K = oracle.StiffnessOperator(mesh, p)
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, mesh.ndofs)
    y1, y2 = np.zeros(mesh.ndofs), np.zeros(mesh.ndofs)
    K(x, y1)
    oracle.stiffness_apply_sumfact(mesh, K.G, K.c0, x, y2)
    assert np.abs(y1 - y2).max() <= 1e-13 * np.abs(y1).max()


def test_geometry_affine_cell(oracle):
    # unit cube split in 2^3: J = diag(1/2), G = detJ*w * 4 I, detJ = w/8
    mesh = oracle.create_box(2, 2)
    G, detJ = oracle.precompute_geometric_data(mesh)
    _, W = oracle.quadrature_weights_hex(2)
    assert np.allclose(detJ, W[None, :] / 8, rtol=1e-14)
    expect = np.einsum("q,ij->qij", W / 8 * 4, np.eye(3))
    assert np.allclose(G, expect[None], rtol=1e-13, atol=0)
    assert np.all(G[:, :, 0, 1] == 0.0)


def test_dense_mass_matches_lumped_when_collocated(oracle):
    p = 3
    mesh = oracle.create_box(2, p, perturb=0.2)
    pts, wts, phi1, phi, X, W = oracle.tabulate_mass_tables(p, "gll", "gll", p + 1)
    detJ = oracle.compute_detJ_generic(mesh, X, W)
    x = np.random.default_rng(3).uniform(-1, 1, mesh.ndofs)
    y1, y2 = np.zeros(mesh.ndofs), np.zeros(mesh.ndofs)
    oracle.dense_mass_apply(mesh, phi, detJ, x, y1)
    oracle.MassOperatorCPU(mesh, p)(x, y2)
    assert np.abs(y1 - y2).max() < 1e-14 * np.abs(y2).max()


def test_mass_table_rule_sizes_match_product(oracle):
    """The oracle's 1-D rules are the product's (wf_quadrature_1d, host code): Basix's
    point counts, (qd+2)//2 Gauss-Jacobi and max(2, (qd+4)//2) GLL, and the same points
    and weights, for every degree up to the product's 16-point limit."""
    import wave_fenics_amd as w
    from wave_fenics_amd import _lib
    for quad in ("gll", "gauss_jacobi"):
        for qd in range(0, 31):
            m = max(2, (qd + 4) // 2) if quad == "gll" else (qd + 2) // 2
            pts, wts, phi1, phi, X, W = oracle.tabulate_mass_tables(3, "gll", quad, qd)
            assert pts.size == wts.size == phi1.shape[0] == m, (quad, qd)
            assert phi.shape == (m ** 3, 64) and X.shape == (m ** 3, 3) and W.shape == (m ** 3,)
            if m > _lib.WF_MAX_QUAD_POINTS:
                with pytest.raises(w.WavehipError):
                    w.quadrature_1d(quad, qd)
                continue
            pw, ww = w.quadrature_1d(quad, qd)
            assert pw.size == m, (quad, qd)
            assert np.abs(pw - pts).max() <= 3e-16 and np.abs(ww - wts).max() <= 1e-15, (quad, qd)


def test_dense_mass_under_integrated_gll_is_not_lumped(oracle):
    """P4 with the default qdegree P+1: Basix's GLL rule has 4 points, not the 5 nodes,
    so Phi^T D Phi is a full (non-collocated) matrix and differs from the lumped mass."""
    p = 4
    mesh = oracle.create_box(2, p, perturb=0.2)
    pts, wts, phi1, phi, X, W = oracle.tabulate_mass_tables(p, "gll", "gll", p + 1)
    assert phi1.shape == (4, 5)
    detJ = oracle.compute_detJ_generic(mesh, X, W)
    x = np.random.default_rng(3).uniform(-1, 1, mesh.ndofs)
    y1, y2 = np.zeros(mesh.ndofs), np.zeros(mesh.ndofs)
    oracle.dense_mass_apply(mesh, phi, detJ, x, y1)
    oracle.MassOperatorCPU(mesh, p)(x, y2)
    assert np.abs(y1 - y2).max() > 1e-3 * np.abs(y2).max()
    # the reference-cell matrix Phi^T diag(W) Phi is not diagonal
    Me = phi.T @ (W[:, None] * phi)
    assert np.abs(Me - np.diag(np.diag(Me))).max() > 1e-2 * np.abs(Me).max()
    # ... and it still integrates constants: 1^T M 1 = |Omega|
    y = np.zeros(mesh.ndofs)
    oracle.dense_mass_apply(mesh, phi, detJ, np.ones(mesh.ndofs), y)
    assert abs(y.sum() - 1.0) < 1e-13


def test_dense_mass_exact_integration(oracle):
    # equispaced P2 + Gauss rule of degree 4: 1^T M 1 = |Omega| on an affine mesh
    p = 2
    mesh = oracle.create_box(3, p)
    pts, wts, phi1, phi, X, W = oracle.tabulate_mass_tables(p, "equispaced", "gauss_jacobi", 2 * p)
    detJ = oracle.compute_detJ_generic(mesh, X, W)
    y = np.zeros(mesh.ndofs)
    oracle.dense_mass_apply(mesh, phi, detJ, np.ones(mesh.ndofs), y)
    assert abs(y.sum() - 1.0) < 1e-13


def test_facet_mass_area(oracle):
    mesh = oracle.create_box((3, 2, 2), 3, perturb=0.2)   # boundary vertices stay on the box
    m1 = oracle.facet_lumped_mass(mesh, 1)
    m2 = oracle.facet_lumped_mass(mesh, 2)
    assert abs(m1.sum() - 1.0) < 1e-13
    assert abs(m2.sum() - 5.0) < 1e-13


def test_rk4_runs_and_is_stable(oracle):
    # The reference's CFL = 0.5 (demo/cpu_planar3d/main.cpp:61) with h = cell
    # diameter is unstable on a uniform cube whose corners carry three absorbing
    # faces (explicit damping rate * dt = 3.6 > 2.785, the RK4 real-axis limit);
    # every RK4 test in this repo uses CFL = 0.25 with the same dt formula.
    p = 2
    mesh = oracle.create_box(4, p, hi=(0.01, 0.01, 0.01))
    eqn = oracle.LinearGLLOpt(mesh, p, 1500.0, 0.5e6, 6e4)
    dt, spp = oracle.cfl_time_step(mesh, p, 1500.0, 0.5e6, CFL=0.25)
    eqn.init()
    t, steps = eqn.rk4(0.0, 100 * dt - 1e-13, dt)
    assert steps == 100
    assert np.isfinite(eqn.u_n).all() and np.abs(eqn.u_n).max() > 0
    assert np.abs(eqn.u_n).max() < 100 * 6e4      # stays at the source's pressure scale
