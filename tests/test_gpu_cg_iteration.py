"""The iteration of wf_cg (csrc/cg.hip, la.cg) itself, not only where it ends: every iterate against a long-double CG,
iteration counts that the mathematics forces, the edges of the loop and of the argument checks, ghost entries on a
periodic partition, and a solve queued behind work on a side stream.

Out of scope: RCCL does not put two ranks on one device, and the gloo workers of test_gpu_partition_models.py cannot
drive wf_cg, so a CG over several ranks stays untested; the one-rank periodic partition exchanges with itself."""
import ctypes

import numpy as np
import pytest

from cg_helpers import (DENSE_CASES, DIAG_KMAX, DIAG_RTOL, KMAX_ITERATES, assemble, dense_case, deviation, diagonal_problem,
                        iterate_reference, numpy_cg, require_forced_count)
from support import LD, bits, comm, dev, gpu, relerr  # noqa: F401

pytestmark = pytest.mark.gpu


def check_iterates(gpu, Aop, b, ref, cond, ks, x0=None, label=""):
    """la.cg(kmax=k, rtol=0) is the k-th iterate: compare it and the returned residual with the long-double run.
    Prints every figure before asserting."""
    import torch
    from wave_fenics_amd import la
    xs, rel, D, bound = ref
    for k in ks:
        x = torch.zeros_like(b) if x0 is None else x0.clone()
        its, res = la.cg(x, b, Aop, kmax=k, rtol=0.0)
        dx = deviation(x.cpu().numpy(), xs[k])
        dres = abs(LD(res) - rel[k]) / rel[k]
        print(f"{label} k={k}: D_k={D[k]:.2e} bound={bound[k]:.2e} device={dx:.2e} res dev={float(dres):.2e} (bound {bound[k] * cond:.2e})")
        assert its == k
        assert dx <= bound[k], (k, dx, bound[k])
        assert dres <= bound[k] * cond, (k, float(dres), bound[k] * cond)


# ---- 1. each iterate against long double ----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["handle", "callback"])
@pytest.mark.parametrize("p,n", DENSE_CASES)
def test_cg_iterates_vs_long_double(gpu, oracle, p, n, mode):
    """The k-th iterate (kmax = k, rtol = 0, x0 = 0), k = 1..8, against CG on the assembled matrix in long double, and
    the returned residual against sqrt(rr_k / rr_0) of that run.  The bound is measured on the reference alone
    (cg_helpers.iterate_reference): 16 D_k, at least 1e-14, D_k the largest deviation of float64 runs whose row sums
    are taken in six seeded random orders; for the residual that bound times cond(A).

    Measured D_k, k = 1..8 (relative to max|x_k|):
      P2 (3,3,2), 245 dofs, cond 185:  2.6e-16 4.9e-16 6.0e-16 6.4e-16 7.6e-16 6.6e-16 6.3e-16 5.1e-16
      P3 (2,2,2), 343 dofs, cond 414:  3.8e-16 6.2e-16 5.6e-16 7.0e-16 8.0e-16 8.9e-16 8.2e-16 8.6e-16
    so the bound is 1.0e-14 to 1.4e-14.  Deviations of the device on the MI355X, k = 1..8 (handle and callback agree to
    the last figure or nearly; the larger of the two):
      P2:  2.0e-16 2.9e-16 2.6e-16 2.7e-16 2.3e-16 1.9e-16 2.0e-16 2.2e-16
      P3:  1.6e-16 5.9e-16 4.7e-16 4.0e-16 4.4e-16 4.1e-16 3.7e-16 2.8e-16
    and of the returned residual at most 4.9e-16, against a bound of 1.9e-12 (P2) and 4.1e-12 (P3) or more."""
    import wave_fenics_amd as w
    c = dense_case(p, n)
    op = w.MassOperator(c["V"], p, c["phi1"], c["detJ"])
    Aop = op if mode == "handle" else (lambda v, y: op(v, y))
    check_iterates(gpu, Aop, dev(c["b"], gpu), c["ref"], c["cond"], range(1, KMAX_ITERATES + 1), label=f"P{p} {n} {mode}")


# ---- 2. exact iteration counts on a diagonal operator ---------------------------------------------------------------

def diagonal_solve(gpu, d, b):
    """la.cg with the callback y += d * v; (its, res, x as numpy)."""
    import torch
    from wave_fenics_amd import la
    dd, bb = dev(d, gpu), dev(b, gpu)
    x = torch.zeros_like(bb)

    def A(v, y):
        y += dd * v
    its, res = la.cg(x, bb, A, kmax=DIAG_KMAX, rtol=DIAG_RTOL)
    return its, res, x.cpu().numpy()


@pytest.mark.parametrize("n,m", [(n, m) for n in (1, 63, 255, 257, 1000, 524365) for m in (1, 3, 5, 8) if m <= n])
def test_cg_diagonal_exact_count(gpu, n, m):
    """m distinct eigenvalues: CG ends at iteration m exactly.  The reference's residual after m - 1 iterations is at
    least 1e3 rtol (measured: 3.2e-3 and more) and after m at most 1e-3 rtol (9.1e-15 and less), whatever the order of
    the sums, so neither the atomics nor an fma move the count; an off-by-one in the stopping test does.
    n = 524365 = 2048 workgroups x 256 threads + 77: every grid-stride loop takes a second pass with a partial last
    workgroup."""
    d, b = diagonal_problem(n, m)
    print("reference residual after m - 1, after m:", require_forced_count(d, b, m))
    its, res, x = diagonal_solve(gpu, d, b)
    print(f"its={its} res={res:.3e} err={relerr(x, b / d):.3e}")
    assert its == m
    assert res < DIAG_RTOL
    assert relerr(x, b / d) <= 1e-14


def test_cg_lumped_mass_exact_count(gpu):
    """The handle path: the lumped P1 mass of the uniform box (2, 2, 2) is diagonal with four values in ratio
    1:2:4:8 (a dof at a corner of the box lies in one cell, on an edge in two, on a face in four, inside in eight), so
    its == 4."""
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd import la
    V = w.create_functionspace(w.create_box(2), 1)
    M = w.MassOperatorLumped(V, 1)
    ndofs = V.ndofs
    dm = torch.zeros(ndofs, dtype=torch.float64, device=gpu)
    M(torch.ones(ndofs, dtype=torch.float64, device=gpu), dm)
    d = dm.cpu().numpy()
    vals = np.unique(np.round(d / d.min() * 2.0 ** 40))
    m = vals.size
    assert np.array_equal(vals / 2.0 ** 40, [1.0, 2.0, 4.0, 8.0])
    rng = np.random.default_rng(17)
    b = rng.uniform(0.5, 1.5, ndofs) * rng.choice([-1.0, 1.0], ndofs)
    print("reference residual after m - 1, after m:", require_forced_count(d, b, m))
    bb = dev(b, gpu)
    x = torch.zeros_like(bb)
    its, res = la.cg(x, bb, M, kmax=DIAG_KMAX, rtol=DIAG_RTOL)
    assert its == m
    assert res < DIAG_RTOL
    assert relerr(x.cpu().numpy(), b / d) <= 1e-14


# ---- 3. edges of the loop -------------------------------------------------------------------------------------------

def scaled_identity(s):
    def A(v, y):
        y += s * v
    return A


def test_cg_kmax_zero_and_zero_rhs(gpu):
    import torch
    from wave_fenics_amd import la
    rng = np.random.default_rng(3)
    b = dev(rng.uniform(-1, 1, 300), gpu)
    x0 = rng.uniform(-1, 1, 300)
    x = dev(x0, gpu)
    assert la.cg(x, b, scaled_identity(2.0), kmax=0, rtol=1e-8) == (0, 1.0)
    assert np.array_equal(bits(x.cpu().numpy()), bits(x0))
    x = torch.zeros_like(b)
    assert la.cg(x, torch.zeros_like(b), scaled_identity(2.0), kmax=5, rtol=1e-8) == (0, 0.0)
    assert np.array_equal(bits(x.cpu().numpy()), bits(np.zeros(300)))


def test_cg_empty_vector(gpu, comm):
    """n = 0: nothing to solve alone; with a communicator the rank still takes part in the reductions (of one rank
    here)."""
    import torch
    from wave_fenics_amd import la

    def never(v, y):
        raise AssertionError("no product of an empty vector")
    e = torch.zeros(0, dtype=torch.float64, device=gpu)
    assert la.cg(e, e.clone(), never, kmax=5, rtol=1e-8) == (0, 0.0)
    assert la.cg(e, e.clone(), never, kmax=5, rtol=1e-8, comm=comm) == (0, 0.0)


@pytest.mark.parametrize("rtol", [0.0, 1e-200])
def test_cg_zero_residual_stops(gpu, rtol):
    """A = 2 I: p = b, pAp = 2 rr in the same order of sums, so alpha = 1/2 and r = b - (1/2)(2 b) = 0 exactly after one
    iteration.  With rtol^2 = 0 (rtol = 0 is 'run kmax iterations', 1e-200 squares to 0) the loop must stop there: the
    next pass would form beta = 0 / rr, p = 0, alpha = 0 / 0 and overwrite x with NaN."""
    import torch
    from wave_fenics_amd import la
    b = np.random.default_rng(4).uniform(-1, 1, 300)
    bb = dev(b, gpu)
    x = torch.zeros_like(bb)
    from wave_fenics_amd._lib import WavehipError
    try:
        its, res = la.cg(x, bb, scaled_identity(2.0), kmax=5, rtol=rtol)
    except WavehipError as e:
        pytest.fail(f"the loop ran past the zero residual (NaN in x: {bool(torch.isnan(x).any())}): {e}")
    xh = x.cpu().numpy()
    assert not np.isnan(xh).any()
    assert (its, res) == (1, 0.0)
    assert np.array_equal(bits(xh), bits(b / 2))


@pytest.mark.parametrize("p,n", DENSE_CASES)
def test_cg_iterates_from_nonzero_guess(gpu, oracle, p, n):
    """r0 = b - A x0: the k-th iterate from a guess that is not the solution, k = 1..4, against the long-double run
    from the same guess.  Measured D_k: P2 3.4e-17 1.8e-16 1.9e-16 3.4e-16, P3 3.7e-17 8.3e-17 6.9e-17 1.0e-16 (the
    bound is its floor, 1e-14).  Device on the MI355X: P2 3.3e-17 7.1e-17 8.3e-17 1.3e-16, P3 3.7e-17 4.8e-17 6.9e-17
    7.3e-17; residual at most 5.1e-16."""
    import wave_fenics_amd as w
    c = dense_case(p, n)
    op = w.MassOperator(c["V"], p, c["phi1"], c["detJ"])
    check_iterates(gpu, op, dev(c["b"], gpu), c["ref_x0"], c["cond"], range(1, 5), x0=dev(c["x0"], gpu), label=f"P{p} {n} x0")


def test_cg_callback_errors(gpu):
    import torch
    from wave_fenics_amd import _lib, la
    b = dev(np.random.default_rng(5).uniform(-1, 1, 300), gpu)
    x = torch.zeros_like(b)

    def broken(v, y):
        raise ValueError("from the callback")
    with pytest.raises(_lib.WavehipError):
        la.cg(x, b, broken, kmax=5, rtol=1e-8)
    assert b"matvec callback" in _lib.lib().wf_last_error()
    # the failed call leaves nothing behind: the same tensors solve with a good operator
    its, res = la.cg(x, b, scaled_identity(2.0), kmax=5, rtol=1e-8)
    assert its == 1 and res < 1e-8
    assert relerr(x.cpu().numpy(), b.cpu().numpy() / 2) <= 1e-15
    # A = 0 is not positive definite: alpha = rr / 0, reported as a status
    x = torch.zeros_like(b)
    with pytest.raises(_lib.WavehipError) as ei:
        la.cg(x, b, lambda v, y: None, kmax=5, rtol=1e-8)
    assert ei.value.status == -1 and "positive definite" in str(ei.value)       # WF_ERR_INVALID


def test_cg_argument_checks(gpu, periodic_case):
    """The C entry point refuses what it cannot run, before any device work: a non-zero status, `iterations` as it was
    or zero."""
    import torch
    from wave_fenics_amd import _lib
    from wave_fenics_amd.operators import _ptr
    L = _lib.lib()
    op, vu, n = periodic_case["op"], periodic_case["vu"], periodic_case["owned"].size
    b = torch.ones(n, dtype=torch.float64, device=gpu)          # every call gets vectors of the length it names
    x = torch.zeros_like(b)

    def desc(**kw):
        d = _lib.CGDesc()
        d.n, d.op, d.kmax, d.rtol = n, op._h, 5, 1e-8
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d):
        its, res = ctypes.c_int(77), ctypes.c_double(0.0)
        rc = L.wf_cg(ctypes.byref(d) if d is not None else None, _ptr(x), _ptr(b), ctypes.byref(its), ctypes.byref(res), 0)
        return rc, its.value
    rc, its = call(desc())                                     # the good descriptor runs
    assert rc == 0 and 1 <= its <= 5, (rc, its)
    refused = [None, desc(op=None),                            # no descriptor; neither an operator nor a matvec
               desc(kmax=-1), desc(updater=vu._h)]             # an updater without its communicator
    for d in refused:
        rc, its = call(d)
        assert rc != 0 and its in (77, 0), (rc, its)


# ---- 4. ghosts ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def periodic_case(gpu, oracle, comm):
    """The one-rank periodic set-up of test_cg_periodic_partition_native_rccl with what the ghost tests add: the owner
    of every ghost entry (through the oracle's periodic numbering) and the long-double iterates on the periodic
    matrix."""
    import wave_fenics_amd as w
    from wave_fenics_amd.distributed import VectorUpdater, create_distributed_box
    p, n, per = 2, (3, 2, 3), (True, False, True)
    part = create_distributed_box(n, p, 1, 0, perturb=0.0, periodic=per, build_dofmap=True)
    om = oracle.create_box(n, p)
    l2g = oracle.make_periodic(om, per)
    pts, wts, phi1, phi, X, W = oracle.tabulate_mass_tables(p, "gll", "gauss_jacobi", 2 * p)
    detJ = np.abs(oracle.compute_detJ_generic(om, X, W))
    A = assemble(oracle, om, phi, detJ)
    vu = VectorUpdater(part, device=gpu, comm=comm)
    part.V.structured = False
    op = w.MassOperator(part.V, p, phi1, detJ)       # local (non-periodic) operator; periodicity comes from the exchange
    owned = part.owned_mask()
    ghosts = np.flatnonzero(~owned)
    assert np.array_equal(np.sort(vu.h_ghost_pos), ghosts)
    owner_of = np.full(om.ndofs, -1)
    owner_of[l2g[owned]] = np.flatnonzero(owned)
    owners = owner_of[l2g[ghosts]]
    assert (owners >= 0).all() and owned[owners].all()
    bg = np.random.default_rng(2).uniform(-1, 1, om.ndofs)
    yield dict(op=op, vu=vu, owned=owned, ghosts=ghosts, owners=owners, l2g=l2g, bg=bg, xs=np.linalg.solve(A, bg),
               ref=iterate_reference(A, bg, 4), cond=float(np.linalg.cond(A)), k_np=numpy_cg(A, bg, 300, 1e-9)[1])
    vu.close()


@pytest.mark.parametrize("mode", ["handle", "callback"])
def test_cg_ghost_entries(gpu, periodic_case, mode):
    """Ghost entries of b and x0 hold NaN: the solver reads neither (r is zeroed there, x0 takes its owner's value in
    the forward update), so the owned solution, the count and the residual are those of the clean run, the fourth
    iterate still matches long double, and every ghost entry of x ends with its owner's bits.  The callback together
    with updater= runs here as well."""
    import torch
    from wave_fenics_amd import la
    c = periodic_case
    op, vu, owned, l2g = c["op"], c["vu"], c["owned"], c["l2g"]
    Aop = op if mode == "handle" else (lambda v, y: op(v, y))
    runs = {}
    for fill in (0.0, np.nan):
        b = dev(np.where(owned, c["bg"][l2g], fill), gpu)
        x = dev(np.where(owned, 0.0, fill), gpu)
        its, res = la.cg(x, b, Aop, kmax=300, rtol=1e-9, updater=vu)
        xh = x.cpu().numpy()
        runs[fill == 0.0] = (its, res)
        print(f"{mode} ghosts={fill}: its={its} res={res:.3e} numpy its={c['k_np']}")
        assert res < 1e-9 and abs(its - c["k_np"]) <= max(3, c["k_np"] // 25)       # (atomics: see test_gpu_cg.py)
        assert np.abs(xh[owned] - c["xs"][l2g[owned]]).max() <= 1e-7 * np.abs(c["xs"]).max()
        assert np.array_equal(bits(xh[c["ghosts"]]), bits(xh[c["owners"]]))
        # a fixed number of iterations: the iterate and its residual are the clean run's to rounding
        xk = dev(np.where(owned, 0.0, fill), gpu)
        its4, res4 = la.cg(xk, b, Aop, kmax=4, rtol=0.0, updater=vu)
        d4 = deviation(xk.cpu().numpy()[owned], c["ref"][0][4][l2g[owned]])
        dres = float(abs(LD(res4) - c["ref"][1][4]) / c["ref"][1][4])
        print(f"  k=4: device={d4:.2e} bound={c['ref'][3][4]:.2e} res dev={dres:.2e}")
        assert its4 == 4 and d4 <= c["ref"][3][4] and dres <= c["ref"][3][4] * c["cond"]
    (its_c, res_c), (its_n, res_n) = runs[True], runs[False]
    assert abs(its_n - its_c) <= max(3, its_c // 25)


def test_cg_refuses_torch_updater(gpu):
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd import _lib, la
    from wave_fenics_amd.distributed import VectorUpdater, create_distributed_box
    part = create_distributed_box((2, 2, 2), 1, 1, 0)
    vu = VectorUpdater(part, device=gpu, transport="torch")
    M = w.MassOperatorLumped(part.V, 1)
    b = torch.ones(part.V.ndofs, dtype=torch.float64, device=gpu)
    with pytest.raises(_lib.WavehipError, match="native"):
        la.cg(torch.zeros_like(b), b, M, updater=vu)


# ---- 5. streams -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stream_load(gpu):
    """2^24 entries for the side stream to work on before it writes b."""
    import torch
    return torch.ones(2 ** 24, dtype=torch.float64, device=gpu)


@pytest.mark.parametrize("mode", ["handle", "callback"])
def test_cg_on_side_stream(gpu, oracle, stream_load, mode):
    """Every kernel of the solver runs on the caller's stream: b is NaN until a few milliseconds of work queued on a side
    stream end by writing it, and la.cg is called at once.  A kernel on the null stream would read NaN or the scalars
    of another iteration.  wf_cg returns host values, so it has synchronised its stream: x is then read from the
    default stream with no synchronise."""
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd import la
    p, n = DENSE_CASES[0]
    c = dense_case(p, n)
    op = w.MassOperator(c["V"], p, c["phi1"], c["detJ"])
    Aop = op if mode == "handle" else (lambda v, y: op(v, y))
    good = dev(c["b"], gpu)
    x = torch.zeros_like(good)
    its0, res0 = la.cg(x, good, Aop, kmax=200, rtol=1e-10)                 # the default-stream run
    assert res0 < 1e-10
    side = torch.cuda.Stream()
    for kmax, rtol in ((200, 1e-10), (4, 0.0)):
        b = torch.full_like(good, float("nan"))
        x = torch.zeros_like(good)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(50):
                stream_load.mul_(1.0)
            b.copy_(good)
            its, res = la.cg(x, b, Aop, kmax=kmax, rtol=rtol)
        xh = x.cpu().numpy()                                               # default stream, no synchronise
        if rtol:
            print(f"{mode}: side stream its={its} res={res:.3e}; default its={its0} res={res0:.3e}")
            assert res < 1e-10 and abs(its - its0) <= max(3, its0 // 25)
            assert np.abs(xh - c["xsol"]).max() <= 1e-7 * np.abs(c["xsol"]).max()
        else:
            d4 = deviation(xh, c["ref"][0][4])
            print(f"{mode}: side stream k=4 device={d4:.2e} bound={c['ref'][3][4]:.2e}")
            assert its == 4 and d4 <= c["ref"][3][4]
    torch.cuda.synchronize()


def test_cg_diagonal_on_side_stream(gpu, stream_load):
    """The forced count at the size that spans the grid, on a side stream behind queued work.  At this size a vector
    kernel runs long enough that one launched on the null stream overlaps its neighbours on the side stream (the count
    then came out as 19, not 5); on the few hundred dofs of test_cg_on_side_stream such a kernel ends before the next
    one starts and goes unseen."""
    import torch
    from wave_fenics_amd import la
    n, m = 524365, 5
    d, b = diagonal_problem(n, m)
    require_forced_count(d, b, m)
    dd, good = dev(d, gpu), dev(b, gpu)
    bb = torch.full_like(good, float("nan"))
    x = torch.zeros_like(good)

    def A(v, y):
        y += dd * v
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(50):
            stream_load.mul_(1.0)
        bb.copy_(good)
        its, res = la.cg(x, bb, A, kmax=DIAG_KMAX, rtol=DIAG_RTOL)
    xh = x.cpu().numpy()
    assert its == m and res < DIAG_RTOL
    assert relerr(xh, b / d) <= 1e-14
    torch.cuda.synchronize()
