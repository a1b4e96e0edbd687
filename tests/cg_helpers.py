"""Shared pieces of the CG tests (test_gpu_cg.py, test_gpu_cg_iteration.py): the oracle's dense mass matrix, numpy
restatements of the solver's loop in float64 and long double, the measured bound of the per-iterate comparison and the
diagonal problems whose iteration count is forced.  Imports without a GPU and without torch."""
import functools

import numpy as np

from support import LD, oracle_module


def numpy_cg(A, b, kmax, rtol):
    """Textbook CG with the reference's stopping rule (cg.hpp:103)."""
    x = np.zeros_like(b)
    r = b.copy()
    p = r.copy()
    rr0 = rr = r @ r
    k = 0
    while k < kmax:
        k += 1
        y = A @ p
        alpha = rr / (p @ y)
        x += alpha * p
        r -= alpha * y
        rr_new = r @ r
        if rr_new / rr0 < rtol * rtol:
            break
        p = r + (rr_new / rr) * p
        rr = rr_new
    return x, k


def assemble(oracle, om, phi, detJ):
    """The oracle's mass matrix, column by column (A e_j)."""
    A = np.zeros((om.ndofs, om.ndofs))
    e, col = np.zeros(om.ndofs), np.zeros(om.ndofs)
    for j in range(om.ndofs):
        e[:] = 0.0
        e[j] = 1.0
        col[:] = 0.0
        oracle.dense_mass_apply(om, phi, detJ, e, col)
        A[:, j] = col
    return A


def dense_mass_setup(oracle, p, n, perturb=0.2):
    """Consistent (non-diagonal) mass: GLL-warped basis, Gauss rule of degree 2P."""
    import wave_fenics_amd as w
    om = oracle.create_box(n, p, perturb=perturb)
    mesh = w.create_box(n, perturb=perturb)
    V = w.create_functionspace(mesh, p)
    pts, wts, phi1, phi, X, W = oracle.tabulate_mass_tables(p, "gll", "gauss_jacobi", 2 * p)
    detJ = oracle.compute_detJ_generic(om, X, W)
    return om, V, phi1, np.abs(detJ), assemble(oracle, om, phi, np.abs(detJ))


# ---- the loop of wf_cg without a stopping test -------------------------------------------------------------------

def ordered_matvec(A, rng):
    """v -> A v in float64, every row summed term by term in an order of its own drawn from rng: what a device operator
    that adds its contributions with atomics may do to the product."""
    n = A.shape[0]
    order = np.argsort(rng.random((n, n)), axis=1)
    Ao = np.take_along_axis(A, order, axis=1)

    def mv(v):
        return np.cumsum(Ao * v[order], axis=1)[:, -1]      # cumsum adds left to right (np.sum would pair)
    return mv


def cg_iterates(matvec, b, kmax, x0=None, dtype=np.float64):
    """kmax iterations of wf_cg's loop (r = b - A x0; alpha = rr / <p, A p>; beta = rr' / rr) in `dtype`.
    Returns (xs, rel): xs[k] the k-th iterate and rel[k] = sqrt(rr_k / rr_0), k = 0..kmax."""
    b = np.asarray(b, dtype=dtype)
    x = np.zeros_like(b) if x0 is None else np.asarray(x0, dtype=dtype).copy()
    r = b - matvec(x) if x0 is not None else b.copy()
    p = r.copy()
    rr0 = rr = r @ r
    xs, rel = [x.copy()], [dtype(1.0)]
    for _ in range(kmax):
        y = matvec(p)
        alpha = rr / (p @ y)
        x = x + alpha * p
        r = r - alpha * y
        rr_new = r @ r
        xs.append(x.copy())
        rel.append(np.sqrt(rr_new / rr0))
        p = r + (rr_new / rr) * p
        rr = rr_new
    return xs, rel


ORDER_SEEDS = (11, 12, 13, 14, 15, 16)
BOUND_FACTOR, BOUND_FLOOR = 16.0, 1e-14


def iterate_reference(A, b, kmax, x0=None):
    """The long-double iterates of CG on A, and the bound of a float64 solver's deviation from them, measured on the
    reference alone: D[k] is the largest deviation, relative to max|x_k|, of float64 runs whose products A p sum every
    row in a seeded random order (ORDER_SEEDS); the bound is BOUND_FACTOR * D[k], at least BOUND_FLOOR.  The factor
    covers fma contraction and the device's different tree of partial sums.
    Returns (xs, rel, D, bound), each indexed by k = 0..kmax."""
    AL = A.astype(LD)
    xs, rel = cg_iterates(lambda v: AL @ v, b, kmax, x0, dtype=LD)
    D = np.zeros(kmax + 1)
    for seed in ORDER_SEEDS:
        xf, _ = cg_iterates(ordered_matvec(A, np.random.default_rng(seed)), b, kmax, x0)
        for k in range(kmax + 1):
            D[k] = max(D[k], float(np.abs(xf[k].astype(LD) - xs[k]).max() / max(np.abs(xs[k]).max(), LD(1e-300))))
    return xs, rel, D, np.maximum(BOUND_FACTOR * D, BOUND_FLOOR)


def deviation(x, xref):
    """max|x - xref| / max|xref| with the difference taken in long double."""
    return float(np.abs(np.asarray(x, dtype=LD) - xref).max() / np.abs(xref).max())


KMAX_ITERATES = 8
DENSE_CASES = [(2, (3, 3, 2)), (3, (2, 2, 2))]


@functools.lru_cache(maxsize=None)
def dense_case(p, n):
    """dense_mass_setup(p, n) with a right-hand side, the dense solve and the reference of the first KMAX_ITERATES
    iterates from x0 = 0 and of the first four from a non-zero x0 that is not the solution.  Computed once per (p, n)
    and shared: nothing in it is written to."""
    oracle = oracle_module()
    oracle.build()
    om, V, phi1, detJ, A = dense_mass_setup(oracle, p, n)
    rng = np.random.default_rng(8)
    b = rng.uniform(-1, 1, om.ndofs)
    xsol = np.linalg.solve(A, b)
    x0 = 0.5 * xsol + 0.01 * np.abs(xsol).max()
    return dict(om=om, V=V, phi1=phi1, detJ=detJ, A=A, b=b, xsol=xsol, cond=float(np.linalg.cond(A)),
                ref=iterate_reference(A, b, KMAX_ITERATES), x0=x0, ref_x0=iterate_reference(A, b, 4, x0))


# ---- diagonal operators: CG ends at the number of distinct eigenvalues ----------------------------------------------

DIAG_RTOL, DIAG_KMAX = 1e-8, 50


def diagonal_problem(n, m, seed=5):
    """(d, b): the eigenvalues 1..m spread over n entries by a seeded permutation; |b| uniform in [0.5, 1.5], random
    signs."""
    assert 1 <= m <= n
    rng = np.random.default_rng(seed + 1000 * m + n)
    d = ((np.arange(n) % m) + 1.0)[rng.permutation(n)]
    b = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    return d, b


def require_forced_count(d, b, m, rtol=DIAG_RTOL):
    """The condition under which `its == m` is forced for a float64 CG on diag(d): over four summation orders of the
    scalar products, the relative residual after m - 1 iterations is at least 1e3 rtol and after m iterations at most
    1e-3 rtol, so no rounding moves the stop.  An input that fails this is a wrong input.  Returns (smallest residual
    after m - 1, largest after m)."""
    n = d.size
    before, after = np.inf, 0.0
    for seed in (None, 21, 22, 23):
        perm = None if seed is None else np.random.default_rng(seed).permutation(n)
        dot = (lambda u, v: float(u @ v)) if perm is None else (lambda u, v: float(np.cumsum((u * v)[perm])[-1]))
        x, r = np.zeros(n), b.copy()
        p = r.copy()
        rr0 = rr = dot(r, r)
        rel = [1.0]
        for _ in range(m):
            y = d * p
            alpha = rr / dot(p, y)
            x += alpha * p
            r -= alpha * y
            rr_new = dot(r, r)
            rel.append(np.sqrt(rr_new / rr0))
            if rr_new == 0.0:
                break
            p = r + (rr_new / rr) * p
            rr = rr_new
        assert len(rel) == m + 1, "the reference's residual vanished before iteration m"
        before, after = min(before, rel[m - 1]), max(after, rel[m])
    assert before >= 1e3 * rtol, (before, rtol)
    assert after <= 1e-3 * rtol, (after, rtol)
    return before, after
