"""Every path of the dense simplex mass operator (csrc/mass_dense_simplex.hip), entry by entry, against long double.

The operator is created through the C ABI (`DenseMassDesc`, `wf_op_create_dense_simplex_mass`) so that the module hands
over its own table, weights, dofmap, geometry and flags; cases, references and the bound B = nd + v + 8 are in
tet_mass_helpers.py (its docstring derives B), and test_tet_mass_host.py asserts without a GPU that every case is what
it is named and that the references have headroom.  What each group of cases reaches in `launch_mass_dense_simplex` /
`k_mass_dense_simplex` (NCB = 64 cells per batch, numax = most unique dofs of a batch, G = min(nbatch, GRID) workgroups,
GRID = kMassGridBound = 256 * kMassWgsPerCU = 512: the constants under "Workgroups per CU of the persistent grid"):

  case                                  instantiation <KT,DT,4,NU>      path
  P1_q8, P1_q1                          <1,1,.,5>                       one k-step, one tile; nq = 8 and 1
  P2_q27, P2_q1                         <3,1,.,5>                       three k-steps (the read-ahead pipeline fills), packed
                                                                        index pairs with an odd KT
  P3_q64, P3_q27                        <5,2,.,5>                       two tiles, scatter rows 16 .. 19 of the second
  P4_q125, P4_q1, P4_q27                <9,3,.,5>                       three tiles, rows 32 .. 34 of the third; nq = 125, 1, 27
  g3x5, g11x13, g18x20, g33x50_shared,  the same four, NU = 5           nd % 4 != 0: padded k lanes feed 0, padded rows of A
  g36x17_shared                                                         are zero and do not scatter; nd = 36: no padding in k
  g33x50_spread                         <9,3,.,9>                       NU = 9 on a padded shape
  P3_broken                             <5,2,.,5>                       numax == 1280: every slot of NU = 5 in use
  g36x17_broken                         <9,3,.,9>                       numax == 2304: every slot of NU = 9 in use
  P4_control / P4_scattered, P4_broken  <9,3,.,5> / <9,3,.,9>           well numbered / scattered; alternating handles with
                                                                        different dynamic LDS sizes (44 and 50 KB)
  P4_n1 .. P4_n129                      NU = 5 (1, 129) and 9 (63..65)  one cell, a last batch short of one cell, whole, of
                                                                        one cell: padded cell slots carry s = 0 and do not
                                                                        scatter; empty: ncells = 0, no launch
  *_all_inverted, *_half_inverted       P2 and P4                       det J < 0: |det J| (flags 0) or the sign kept
                                                                        (WF_FLAG_NO_FABS) in dense_mass_setup
  P2_rounds4, P4_rounds2                NU = 5 / NU = 9                 nbatch > GRID: the persistent loop with its prefetch
                                                                        stages (b + G, b + 2G, b + 3G), more than two rounds,
                                                                        a last round with one live workgroup, a last batch of
                                                                        one cell

64 nd > 1280 needs nd > 20, so NU = 9 exists for the nd = 33 .. 36 shapes only; for KT <= 5 the NU = 9 instantiations are
compiled but no input can select them.  Small cases: reference (a), long double, |got - ref| <= B eps mag for every entry.
Large cases: reference (b), float64, TOL = 1e-12 of max|ref|.  `y` is non-zero on entry everywhere and of the size of the
entries of M x; no entry is skipped or masked."""
import ctypes
import time

import numpy as np
import pytest

from support import gpu  # noqa: F401
from tet_mass_helpers import (BIG, EPS, GRID, LD, NCB, NO_FABS, NU9_CASES, ORIENTATION_CASES, PAD, SENTINEL, SMALL, TOL,
                              MassOp, batch_unique, created, det_j, empty_case, lds_bytes, mesh_case, nu_of, ratio, reference,
                              relerr, small, small_reference, upright_of)

gpu_test = pytest.mark.gpu
WORST = {}                        # (nd, NU) -> (worst ratio, its B)
T0 = time.time()


def check_entries(case, got, ref, mag, what, B=None):
    B = case.B if B is None else B
    worst, ok, where = ratio(got, ref, mag, B)
    key = (case.nd, nu_of(case) if case.ncells else 5)
    if worst >= WORST.get(key, (-1.0, 0))[0]:
        WORST[key] = (worst, B)
    print(f"{what}: worst entry {worst:.3f} eps of its magnitude (B = {B})")
    assert ok, f"{what}: entry {where} is {worst:.3f} eps of its magnitude from the reference (bound {B})"
    return worst


def check_untouched(case, got):
    untouched = np.ones(case.ndofs, dtype=bool)
    untouched[case.dm.reshape(-1)] = False
    assert np.array_equal(got[untouched].view(np.uint64), case.y0[untouched].view(np.uint64)), "a dof of no cell was written"


# ---------------------------------------------------------------------------------------------------------------------
# every small case against the long-double reference
# ---------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("name", [n for n in SMALL if n not in ORIENTATION_CASES])
def test_small_case(gpu, name):
    """reference (a), entry by entry; the NU = 9 cases twice on one handle; the float64 reference (b) at TOL as well"""
    case = small(name)
    ref, mag = small_reference(name)
    op = created(case)
    info = op.info()
    assert (info.kind, info.degree, info.num_dofs_cell, info.num_quads, info.num_cells) == (2, 0, case.nd, case.nq, case.ncells)
    assert (info.kernel, info.geometry, info.metric, info.update) == (10, 0, 0, 0)
    assert info.flops == 4.0 * case.ncells * case.nq * case.nd
    assert info.alg_bytes == case.ncells * (8.0 + 4.0 * case.nd) + 16.0 * case.ndofs
    assert info.device_bytes >= 8 * case.nbatch * NCB + 4 * int(batch_unique(case.dm).sum())
    for k in range(2 if name in NU9_CASES else 1):
        got = op.host(gpu, case.x, case.y0)
        check_entries(case, got, ref, mag, f"{name} apply {k}")
        check_untouched(case, got)
        assert relerr(got, reference(case, 0, np.float64)[0]) <= TOL
    assert op.close() == 0


@gpu_test
def test_empty_mesh(gpu):
    """ncells = 0: the creation succeeds and the apply is a no-op (y bitwise untouched)"""
    case = empty_case()
    op = created(case)
    assert op.info().num_cells == 0 and op.info().kernel == 10
    got = op.host(gpu, case.x, case.y0)
    assert np.array_equal(got.view(np.uint64), case.y0.view(np.uint64))
    assert op.close() == 0


@gpu_test
@pytest.mark.parametrize("name", ORIENTATION_CASES)
def test_orientation(gpu, name):
    """flags 0: the result is that of the upright mesh, cell for cell; WF_FLAG_NO_FABS: the sign of det J is kept.  The
    two references differ by far more than the bound (asserted here, and with figures in test_tet_mass_host.py)"""
    case = small(name)
    ref0, mag = small_reference(name, 0)
    ref1, _ = small_reference(name, NO_FABS)
    assert float(np.max(np.abs(ref0 - ref1) / (LD(EPS) * mag))) >= 1e6 * case.B, "the two runs would not tell the flags apart"
    got0 = created(case, 0).host(gpu, case.x, case.y0)
    check_entries(case, got0, ref0, mag, f"{name} flags 0")
    up = upright_of(case)
    assert np.all(det_j(up.xv, up.gd, np.float64) > 0.0)
    gotu = created(up, 0).host(gpu, case.x, case.y0)
    check_entries(case, gotu, ref0, mag, f"{name} upright mesh, flags 0")
    w, ok, where = ratio(got0, np.asarray(gotu, dtype=LD), mag, case.B)
    assert ok, (where, w)
    got1 = created(case, NO_FABS).host(gpu, case.x, case.y0)
    check_entries(case, got1, ref1, mag, f"{name} WF_FLAG_NO_FABS")
    # on the upright mesh the flag changes nothing
    gotu1 = created(up, NO_FABS).host(gpu, case.x, case.y0)
    check_entries(case, gotu1, ref0, mag, f"{name} upright mesh, WF_FLAG_NO_FABS")


@gpu_test
def test_alternating_handles_with_different_lds(gpu):
    """two handles of one instantiation (P4, NU = 9) with different numax, hence different dynamic LDS sizes, applied
    alternately, and a handle of the NU = 5 instantiation of the same shape in between"""
    a, b = small("P4_scattered"), small("P4_broken")
    assert lds_bytes(a) != lds_bytes(b)
    ops = {c.name: created(c) for c in (a, b)}
    for k, c in enumerate((a, b, a, b, b, a)):
        got = ops[c.name].host(gpu, c.x, c.y0)
        check_entries(c, got, *small_reference(c.name), f"alternating, step {k}: {c.name}")
    c = small("P4_control")
    check_entries(c, created(c).host(gpu, c.x, c.y0), *small_reference(c.name), "alternating: P4_control")
    got = ops[a.name].host(gpu, a.x, a.y0)
    check_entries(a, got, *small_reference(a.name), "alternating, after NU = 5")


@gpu_test
@pytest.mark.parametrize("name", ["P4_control", "P4_scattered"])
def test_8_byte_aligned_vectors(gpu, name):
    """x and y one entry off 16-byte alignment inside padded buffers; nothing outside y is written"""
    import torch
    case = small(name)
    hx = np.full(PAD + case.ndofs + PAD + 1, SENTINEL)
    hy = hx.copy()
    hx[PAD + 1:PAD + 1 + case.ndofs] = case.x
    hy[PAD + 1:PAD + 1 + case.ndofs] = case.y0
    bx, by = torch.from_numpy(hx).to(gpu), torch.from_numpy(hy).to(gpu)
    dx, dy = bx[PAD + 1:PAD + 1 + case.ndofs], by[PAD + 1:PAD + 1 + case.ndofs]
    assert bx.data_ptr() % 16 == 0 and dx.data_ptr() % 16 == 8 and dy.data_ptr() % 16 == 8
    op = created(case)
    op(dx, dy)
    torch.cuda.synchronize()
    gx, gy = bx.cpu().numpy(), by.cpu().numpy()
    assert np.array_equal(gx.view(np.uint64), hx.view(np.uint64)), "x or its padding was written"
    pad = np.ones(hy.size, dtype=bool)
    pad[PAD + 1:PAD + 1 + case.ndofs] = False
    assert np.array_equal(gy.view(np.uint64)[pad], hy.view(np.uint64)[pad]), "an entry outside y was written"
    check_entries(case, gy[PAD + 1:PAD + 1 + case.ndofs], *small_reference(name), f"{name}, x and y 8-byte aligned")


@gpu_test
@pytest.mark.parametrize("name", ["P2_q27", "P4_control", "P4_scattered"])
def test_two_applies_accumulate(gpu, name):
    """two applies in a row give y0 + 2 M x.  Each apply is within B eps / 2 of the magnitude of what it adds to (the
    chain behind B, in units of u = eps / 2), and both magnitudes are below |y0| + 2 mag(M x): the bound stays B"""
    case = small(name)
    ref2, mag2 = reference(case, 0, LD, times=2)
    got = created(case).host(gpu, case.x, case.y0, applies=2)
    check_entries(case, got, ref2, mag2, f"{name}, two applies")
    ref1, _ = small_reference(name)
    assert float(np.max(np.abs(ref2 - ref1) / (LD(EPS) * mag2))) >= 1e6 * case.B      # a single apply would be seen


@gpu_test
@pytest.mark.parametrize("name", ["P4_control", "P4_scattered", "P2_half_inverted"])
def test_repeatable_to_the_entry_bound(gpu, name):
    """two applies of one handle on the same input agree to B eps mag per entry (the atomics leave the order of the sums
    free, so bitwise equality is not the claim: WF_FLAG_ORDERED stays unsupported)"""
    case = small(name)
    ref, mag = small_reference(name)
    op = created(case)
    a, b = op.host(gpu, case.x, case.y0), op.host(gpu, case.x, case.y0)
    check_entries(case, a, ref, mag, f"{name} first apply")
    check_entries(case, b, ref, mag, f"{name} second apply")
    worst, ok, where = ratio(a, np.asarray(b, dtype=LD), mag, case.B)
    print(f"{name}: two applies differ by at most {worst:.3f} eps of the magnitude")
    assert ok, (where, worst)


@gpu_test
def test_batch_kernel_has_no_parts(gpu):
    """wf_op_apply_part (any part but ALL) and wf_op_set_ghost_* are WF_ERR_UNSUPPORTED; WF_PART_ALL is the apply"""
    import torch
    case = small("P2_q27")
    op = created(case)
    L = op.lib
    ghosts = np.zeros(1, dtype=np.int32)
    assert L.wf_op_set_ghost_faces(op.h, 1, 0, 0) == -2 and L.wf_last_error()
    assert L.wf_op_set_ghost_dofs(op.h, ghosts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1) == -2
    dx, dy = torch.from_numpy(case.x).to(gpu), torch.from_numpy(case.y0).to(gpu)
    for part in (1, 2, 3, 4):
        assert L.wf_op_apply_part(op.h, dx.data_ptr(), dy.data_ptr(), part, None) == -2
        assert b"batch kernel" in L.wf_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(dy.cpu().numpy().view(np.uint64), case.y0.view(np.uint64))
    assert L.wf_op_apply_part(op.h, dx.data_ptr(), dy.data_ptr(), 0, None) == 0
    torch.cuda.synchronize()
    check_entries(case, dy.cpu().numpy(), *small_reference(case.name), "wf_op_apply_part(WF_PART_ALL)")


# ---------------------------------------------------------------------------------------------------------------------
# more batches than workgroups, against the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("name", list(BIG))
def test_persistent_loop(gpu, name):
    """nbatch above the grid bound kMassGridBound = 512 (mass_dense_simplex.hip, `constexpr int kMassGridBound`; the
    launch takes std::min(d->nbatch, kMassGridBound) workgroups): four rounds at P2, two at P4 on the NU = 9 path, each
    with a last round of one live workgroup whose batch holds one cell.  Reference (b): 1e-12 of max|ref| over all
    entries and over the dofs of the last round on their own scale (a wrong last round must not hide behind the largest
    entry of the mesh); two applies of the handle"""
    assert GRID == 512
    case = BIG[name]()
    assert case.nbatch > GRID and (case.nbatch - 1) % GRID == 0 and case.ncells % NCB == 1
    assert (nu_of(case) == 9) == name.startswith("P4")
    ref = reference(case, 0, np.float64)[0]
    op = created(case)
    last = np.unique(case.dm[(case.nbatch - 1) // GRID * GRID * NCB:])
    assert last.size == case.nd
    for k in range(2):
        got = op.host(gpu, case.x, case.y0)
        err, err_last = relerr(got, ref), relerr(got[last], ref[last])
        print(f"{name} apply {k}: {err:.3e} of max|y|; dofs of the last round of batches {err_last:.3e}")
        assert err <= TOL and err_last <= TOL
        check_untouched(case, got)
    assert op.close() == 0


# ---------------------------------------------------------------------------------------------------------------------
# known answers and the solver
# ---------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("p,n,perturb", [(1, (2, 2, 2), 0.2), (2, (3, 2, 2), 0.2), (3, (2, 2, 2), 0.2), (4, (2, 2, 2), 0.2),
                                         (4, (2, 2, 1), 0.0)])
def test_volume_and_symmetry(gpu, p, n, perturb):
    """1^T M 1 is the volume of the box (1: perturbing moves interior vertices only) and x^T (M z) = z^T (M x), each to
    (nd + v + 8 + log2 ndofs) eps of the sum of the magnitudes of the terms; no reference involved"""
    case = mesh_case("volume", p, n, perturb=perturb, seed=50 + p)
    op = created(case)
    bound = (case.nd + case.v + 8 + np.log2(case.ndofs)) * LD(EPS)
    zero, one = np.zeros(case.ndofs), np.ones(case.ndofs)
    m1 = np.asarray(op.host(gpu, one, zero), dtype=LD)
    # magnitude of 1^T M 1: sum_c |s_c| sum_ab |A_ab| >= the sum of the |terms| the kernel and this sum add up
    Aabs = np.einsum("q,qa,qb->ab", case.W, np.abs(case.phi), np.abs(case.phi))
    magsum = LD(np.abs(det_j(case.xv, case.gd, np.float64)).sum()) * LD(Aabs.sum())
    vol = np.sum(np.abs(det_j(case.xv, case.gd, LD))) / 6
    assert abs(vol - 1) <= 16 * LD(EPS)
    total = np.sum(m1)
    print(f"P{p}: 1^T M 1 - 1 = {float(total - 1):.3e}, {float(abs(total - 1) / (LD(EPS) * magsum)):.3f} eps of the magnitude sum "
          f"(bound {float(bound / LD(EPS)):.1f})")
    assert abs(total - 1) <= bound * magsum
    x, z = case.x, np.random.default_rng(9).uniform(-1.0, 1.0, case.ndofs)
    mx, mz = np.asarray(op.host(gpu, x, zero), dtype=LD), np.asarray(op.host(gpu, z, zero), dtype=LD)
    magx = reference(case, 0, np.float64, y0=zero)[1]                   # mag of M x per entry
    case_z = mesh_case("volume", p, n, perturb=perturb, seed=50 + p)
    case_z.x = z
    magz = reference(case_z, 0, np.float64, y0=zero)[1]
    lhs, rhs = np.sum(np.asarray(x, dtype=LD) * mz), np.sum(np.asarray(z, dtype=LD) * mx)
    mags = np.sum(np.abs(x) * magz) + np.sum(np.abs(z) * magx)
    print(f"P{p}: x^T M z - z^T M x = {float(lhs - rhs):.3e}, {float(abs(lhs - rhs) / (LD(EPS) * mags)):.3f} eps of the magnitude sum")
    assert abs(lhs - rhs) <= bound * mags


@gpu_test
@pytest.mark.parametrize("p", [2, 4])
def test_cg_solves_the_mass_system(gpu, p):
    """M a = b (the problem of demo/gpu_cg on a tetrahedral space) with la.cg on TetMassOperator, kmax = 500,
    rtol = 1e-10, against numpy.linalg.solve on the dense assembled M: max|u - u_np| <= 1e-7 max|u_np|, the gate of
    test_gpu_cg.py.  Convergence is asserted, not the iteration count (CPU conjugate gradients on the assembled matrices
    took 56 and 122 iterations; the atomics move the count by a few)."""
    import torch
    from wave_fenics_amd import la, tet
    V = tet.create_kuhn_box((2, 2, 2), p, perturb=0.2)
    X, W = tet.tet_quadrature(p + 1)
    phi, _ = tet.tabulate_tet(p, X)
    A = np.einsum("q,qa,qb->ab", W, phi, phi)
    s = np.abs(det_j(V.x, V.geom_dofmap, np.float64))
    M = np.zeros((V.ndofs, V.ndofs))
    np.add.at(M, (V.dofmap[:, :, None], V.dofmap[:, None, :]), s[:, None, None] * A[None, :, :])
    rng = np.random.default_rng(70 + p)
    b = rng.uniform(-1.0, 1.0, V.ndofs) * s.mean()
    u_np = np.linalg.solve(M, b)
    op = tet.TetMassOperator(V, p)
    assert op.kernel == "dense_simplex_mass" and op.num_quads() == (p + 1) ** 3 and op.num_dofs() == phi.shape[1]
    # the operator is the assembled matrix
    xd = torch.from_numpy(rng.uniform(-1.0, 1.0, V.ndofs)).to(gpu)
    yd = torch.zeros_like(xd)
    op(xd, yd)
    assert relerr(yd.cpu().numpy(), M @ xd.cpu().numpy()) <= TOL
    u, bd = torch.zeros(V.ndofs, dtype=torch.float64, device=gpu), torch.from_numpy(b).to(gpu)
    its, res = la.cg(u, bd, op, kmax=500, rtol=1e-10)
    torch.cuda.synchronize()
    err = relerr(u.cpu().numpy(), u_np)
    print(f"P{p}: {its} iterations, relative residual {res:.3e}, max|u - u_np| / max|u_np| = {err:.3e}, cond {np.linalg.cond(M):.0f}")
    assert its < 500 and res < 1e-10, "CG did not converge"
    assert err <= 1e-7


@gpu_test
def test_default_rule_of_the_python_operator(gpu):
    """TetMassOperator(V, degree) takes the rule of degree 2 * degree (m = degree + 1 points per direction)"""
    from wave_fenics_amd import tet
    V = tet.create_kuhn_box((2, 2, 1), 3, perturb=0.2)
    op = tet.TetMassOperator(V, 3)
    assert op.num_quads() == 4 ** 3 and op.num_dofs() == 20 and op.kernel == "dense_simplex_mass"
    assert tet.TetMassOperator(V, 3, qdegree=2).num_quads() == 2 ** 3


@gpu_test
def test_report_worst_ratios(gpu):
    """the record of the run: worst |got - ref| / (eps * magnitude) per shape and NU (runs last; the bound stays B)"""
    assert WORST, "no entry check has run"
    for (nd, nu) in sorted(WORST):
        r, B = WORST[(nd, nu)]
        print(f"worst ratio nd = {nd} NU = {nu}: {r:.3f} (B = {B})")
        assert r <= B
    print(f"module wall time {time.time() - T0:.1f} s")
