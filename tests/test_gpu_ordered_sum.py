"""Order-fixed accumulation (WF_FLAG_ORDERED, ordered.hip) on the MI355X: pass 1 stores every cell's element-local result
to v[slot], pass 2 (wf_segment_sum_add) gives every y entry to one thread that sums its run front to back.  No atomics,
so y is a pure function of the inputs -- on perturbed boxes, caller-supplied dofmaps, the dense and the lumped mass.

  1. wf_segment_sum_add against a numpy loop doing the same sequential fp64 adds, bit for bit;
  2. parity with the CPU oracle, 1e-12 of max|y| (TOL of test_gpu_parity.py), accumulating into a non-zero y;
  3. bitwise repeatability: 20 applies, two separately created operators, two streams, the lumped diagonal;
  4. independence of the dof numbering: relabelling the dofs relabels y bit for bit (what atomics or per-batch
     pre-sums would fail);
  5. the box operator with the flag IS the dofmap operator;
  6. errors, selection, alg_bytes.

Shapes: per degree a perturbed box whose cell count spans at least two batches of CB = 256 // (P+1)^2 cells and is no
multiple of CB.  Every test asserts kernel == "cells_ordered" and update == "ordered": a silent fallback cannot pass."""
import numpy as np
import pytest

from nonbox_helpers import ORDERED
from support import dev, gpu, relerr  # noqa: F401
from test_gpu_owner_high_degree import DEFAULT, form
from test_gpu_unstructured import build_mesh, oracle_mesh

pytestmark = pytest.mark.gpu

TOL = 1e-12
# degree -> box (cells); CB = 64, 28, 16, 10, 7, 5, 4
BOXES = {1: (5, 4, 4), 2: (5, 4, 4), 3: (3, 3, 2), 4: (3, 2, 2), 5: (3, 2, 2), 6: (3, 2, 2), 7: (3, 3, 2)}


def box(oracle, p, perturb=0.2, n=None):
    import wave_fenics_amd as w
    n = BOXES[p] if n is None else n
    om = oracle.create_box(n, p, perturb=perturb)
    mesh = w.create_box(n, perturb=perturb)
    V = w.create_functionspace(mesh, p)
    assert np.array_equal(V.dofmap, om.dofmap) and np.array_equal(mesh.x, om.x)
    CB = 256 // (p + 1) ** 2
    assert om.ncells > CB and om.ncells % CB != 0
    return om, V


def stiffness(V, p, structured=False, flags=None, tuning=None):
    import wave_fenics_amd as w
    return w.StiffnessOperator(V, p, {"c0": 1500.0}, structured=structured, flags=ORDERED() if flags is None else flags,
                               tuning=tuning)


def is_ordered(op):
    return op.kernel == "cells_ordered" and op.update == "ordered"


def apply(op, x, y0, gpu, stream=None):
    """y0 + A x as a device tensor; on `stream` (a torch stream) when given."""
    import torch
    xd, y = dev(x, gpu), dev(y0, gpu)
    torch.cuda.synchronize()
    if stream is None:
        op(xd, y)
    else:
        with torch.cuda.stream(stream):
            op(xd, y)
    torch.cuda.synchronize()
    return y


def inputs(ndofs, seed, scale=1e6):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, ndofs), rng.uniform(-1, 1, ndofs) * scale


# ---------------------------------------------------------------------------------------------------------------------
# 1. pass 2 as a free kernel
# ---------------------------------------------------------------------------------------------------------------------
def segment_case(n, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, n)
    if n > 1:
        lens[rng.integers(0, n, max(1, n // 10))] = 0      # empty rows for certain
    row_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nv = int(row_off[-1])
    vals = rng.uniform(-1, 1, nv) * 10.0 ** rng.uniform(-8, 8, nv)
    y0 = rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-3, 3, n)
    assert np.all(y0 != 0.0)
    want = y0.copy()
    for d in range(n):
        if row_off[d + 1] > row_off[d]:
            s = vals[row_off[d]]
            for e in range(row_off[d] + 1, row_off[d + 1]):
                s = s + vals[e]
            want[d] = want[d] + s
    return row_off, vals, y0, want


@pytest.mark.parametrize("n", [1, 255, 1000])
def test_segment_sum_add_bitwise(gpu, n):
    import torch
    import wave_fenics_amd as w
    row_off, vals, y0, want = segment_case(n, seed=n)
    if n > 1:   # the order matters for these values: a pairwise / sorted sum gives other bits somewhere
        other = y0 + np.array([np.sum(vals[row_off[d]:row_off[d + 1]][::-1]) for d in range(n)])
        assert np.any(other.view(np.int64) != want.view(np.int64))
    ro = dev(row_off, gpu)
    # default stream; a non-default stream; vals at an address that is 8 but not 16 bytes aligned (scalar loads only)
    padded = dev(np.concatenate([[123.0], vals]), gpu)
    side = torch.cuda.Stream(device=gpu)
    for name, v, stream in (("default", dev(vals, gpu), None), ("side", dev(vals, gpu), side), ("unaligned", padded[1:], None)):
        assert (v.data_ptr() % 16 == 8) == (name == "unaligned")
        y = dev(y0, gpu)
        torch.cuda.synchronize()
        if stream is None:
            w.segment_sum_add(n, ro, v, y)
        else:
            with torch.cuda.stream(stream):
                w.segment_sum_add(n, ro, v, y)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        bad = np.nonzero(got.view(np.int64) != want.view(np.int64))[0]
        assert bad.size == 0, (name, n, bad[:5], got[bad[:5]], want[bad[:5]])


def test_segment_sum_add_edges(gpu):
    """n = 0 is a no-op (null pointers allowed); rows that are all empty leave y untouched; a first row that starts at an
    odd entry and rows of length 1, 2 and 3 take every branch of the 16-byte sweep."""
    import wave_fenics_amd as w
    from wave_fenics_amd import _lib
    assert _lib.lib().wf_segment_sum_add(0, None, None, None, None) == 0
    assert _lib.lib().wf_segment_sum_add(-1, None, None, None, None) == -1
    y0 = np.array([1.5, -2.5, 3.5])
    y = dev(y0, gpu)
    w.segment_sum_add(3, dev(np.zeros(4, dtype=np.int32), gpu), dev(np.zeros(1), gpu), y)
    assert np.array_equal(y.cpu().numpy(), y0)
    row_off = np.array([0, 1, 3, 6, 6, 7, 10, 12], dtype=np.int32)
    vals = np.array([1e16, 1.0, -1e16, 3.0, 1e-3, 1e16, -7.0, 1.0, 1e16, -1e16, 2.0, 1e-30])
    y0 = np.arange(1.0, 8.0)
    want = y0.copy()
    for d in range(7):
        if row_off[d + 1] > row_off[d]:
            s = vals[row_off[d]]
            for e in range(row_off[d] + 1, row_off[d + 1]):
                s = s + vals[e]
            want[d] = want[d] + s
    y = dev(y0, gpu)
    w.segment_sum_add(7, dev(row_off, gpu), dev(vals, gpu), y)
    assert np.array_equal(y.cpu().numpy().view(np.int64), want.view(np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# 2. parity with the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6, 7])
def test_stiffness_parity(gpu, oracle, p):
    om, V = box(oracle, p)
    x, y0 = inputs(om.ndofs, p)
    yref = y0.copy()
    oracle.StiffnessOperator(om, p)(x, yref)
    for structured in (False, True):
        op = stiffness(V, p, structured=structured)
        assert is_ordered(op) and op.geometry == "per_point" and op.info.structured == int(structured)
        err = relerr(apply(op, x, y0, gpu).cpu().numpy(), yref)
        print(f"P{p} {BOXES[p]} structured={structured}: ordered stiffness vs oracle {err:.3e}")
        assert err <= TOL, (p, structured, err)


@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("kind", ["random_orient", "ogrid"])
def test_stiffness_parity_unstructured(gpu, oracle, kind, p):
    from wave_fenics_amd import mesh_io
    mesh, _ = build_mesh(kind, p)
    V = mesh_io.create_functionspace(mesh, p)
    om = oracle_mesh(oracle, mesh, V)
    K = oracle.StiffnessOperator(om, p)
    x, y0 = inputs(V.ndofs, 1234)
    yref = y0.copy()
    K(x, yref)
    for Garg in (None, K.G):      # geometry from the mesh on the device, and handed over in the reference layout
        import wave_fenics_amd as w
        op = w.StiffnessOperator(V, p, {"c0": 1500.0}, G=Garg, structured=False, flags=ORDERED())
        assert is_ordered(op)
        err = relerr(apply(op, x, y0, gpu).cpu().numpy(), yref)
        print(f"P{p} {kind} G={'given' if Garg is not None else 'mesh'}: ordered stiffness vs oracle {err:.3e}")
        assert err <= TOL, (kind, p, err)


@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("rule", ["square", "rectangular"])
def test_dense_mass_parity(gpu, oracle, p, rule):
    """Gauss of degree 2P (P+1 points: a square table) and of degree 2P+2 (nq1 = P+2)."""
    import wave_fenics_amd as w
    om, V = box(oracle, p)
    qd = 2 * p if rule == "square" else 2 * p + 2
    pts, wts, phi1, phi, Xq, Wq = oracle.tabulate_mass_tables(p, "equispaced", "gauss_jacobi", qd)
    assert phi1.shape[0] == (p + 1 if rule == "square" else p + 2)
    detJ = oracle.compute_detJ_generic(om, Xq, Wq)
    x = np.random.default_rng(p).uniform(-1, 1, om.ndofs)
    mx = np.zeros(om.ndofs)
    oracle.dense_mass_apply(om, phi, detJ, x, mx)
    y0 = np.random.default_rng(p + 10).uniform(-1, 1, om.ndofs) * np.abs(mx).max()   # the scale of M x: nothing hides
    yref = y0 + mx
    ops = (w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=qd, flags=ORDERED()),
           w.MassOperator(V, p, phi1, detJ, flags=ORDERED()))
    for op in ops:
        assert is_ordered(op) and op.num_quads() == phi1.shape[0] ** 3
        err = relerr(apply(op, x, y0, gpu).cpu().numpy() - y0, mx)
        print(f"P{p} {rule}: ordered dense mass vs oracle {err:.3e}")
        assert err <= TOL, (p, rule, err)
        assert relerr(apply(op, x, y0, gpu).cpu().numpy(), yref) <= TOL


def test_lumped_mass_parity(gpu, oracle):
    import wave_fenics_amd as w
    from wave_fenics_amd._lib import WF_FLAG_MASS_ELEMENTWISE
    p = 3
    om, V = box(oracle, p)
    x = np.random.default_rng(7).uniform(-1, 1, om.ndofs)
    mx = np.zeros(om.ndofs)
    oracle.MassOperatorCPU(om, p)(x, mx)
    y0 = np.random.default_rng(8).uniform(-1, 1, om.ndofs) * np.abs(mx).max()
    op = w.MassOperatorLumped(V, p, structured=False, flags=ORDERED() | WF_FLAG_MASS_ELEMENTWISE)
    assert is_ordered(op)
    assert relerr(apply(op, x, y0, gpu).cpu().numpy() - y0, mx) <= TOL
    # without ELEMENTWISE the kernel stays the diagonal; it is assembled through the ordered passes
    for structured in (False, True):
        diag = w.MassOperatorLumped(V, p, structured=structured, flags=ORDERED())
        assert diag.kernel == "diagonal" and diag.update == "none"
        assert relerr(apply(diag, x, y0, gpu).cpu().numpy() - y0, mx) <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# 3. bitwise repeatability
# ---------------------------------------------------------------------------------------------------------------------
def operators_for_repeat(oracle, p):
    import wave_fenics_amd as w
    from wave_fenics_amd._lib import WF_FLAG_MASS_ELEMENTWISE
    om, V = box(oracle, p)
    return V, {
        "stiffness": lambda: stiffness(V, p),
        "dense mass": lambda: w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=2 * p + 2, flags=ORDERED()),
        "lumped mass": lambda: w.MassOperatorLumped(V, p, structured=False, flags=ORDERED() | WF_FLAG_MASS_ELEMENTWISE),
    }


@pytest.mark.parametrize("p", [2, 5])
def test_bitwise_repeatable(gpu, oracle, p):
    import torch
    V, makers = operators_for_repeat(oracle, p)
    x, y0 = inputs(V.ndofs, 6, scale=1.0)
    side = torch.cuda.Stream(device=gpu)
    for name, make in makers.items():
        op = make()
        assert is_ordered(op), name
        first = apply(op, x, y0, gpu)
        for _ in range(19):
            assert torch.equal(apply(op, x, y0, gpu), first), name
        assert torch.equal(apply(make(), x, y0, gpu), first), (name, "a second operator")
        assert torch.equal(apply(op, x, y0, gpu, stream=side), first), (name, "side stream")


def test_lumped_diagonal_bitwise(gpu, oracle):
    import torch
    import wave_fenics_amd as w
    p = 3
    om, V = box(oracle, p)
    ones, zero = np.ones(om.ndofs), np.zeros(om.ndofs)
    ys = [apply(w.MassOperatorLumped(V, p, structured=False, flags=ORDERED()), ones, zero, gpu) for _ in range(3)]
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    # m is the fixed-order sum of det J w over the entries of the caller's dofmap
    _, detJ = w.precompute_geometric_data(V.mesh, p, use_fabs=True, clamp=False, want_G=False)
    m = np.zeros(om.ndofs)
    for d, v in zip(V.dofmap.reshape(-1), detJ.reshape(-1)):   # front to back
        m[d] = m[d] + v if m[d] != 0.0 else v
    assert np.array_equal(ys[0].cpu().numpy().view(np.int64), m.view(np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# 4. independence of the dof numbering
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [2, 4])
def test_dof_numbering_does_not_enter(gpu, oracle, p):
    import torch
    import wave_fenics_amd as w
    om, V = box(oracle, p)
    x, y0 = inputs(V.ndofs, 40 + p, scale=1.0)
    perm = np.random.default_rng(p).permutation(V.ndofs).astype(np.int32)
    V2 = w.renumber(V, perm)
    x2, y02 = np.empty_like(x), np.empty_like(y0)
    x2[perm], y02[perm] = x, y0
    pd = dev(perm.astype(np.int64), gpu)
    results = []
    for keep in (False, True):
        tuning = {"keep_cell_order": keep}
        a, b = stiffness(V, p, tuning=tuning), stiffness(V2, p, tuning=tuning)
        assert is_ordered(a) and is_ordered(b)
        y = apply(a, x, y0, gpu)
        y2 = apply(b, x2, y02, gpu)
        assert torch.equal(y2[pd], y), (p, keep)
        results.append(y)
    assert torch.equal(results[0], results[1])     # the internal cell order does not enter either
    # the default (atomic) operator on the same pair agrees to rounding only -- it is the ordered one that is exact
    yd = apply(stiffness(V2, p, flags=0), x2, y02, gpu)
    assert relerr(yd[pd].cpu().numpy(), results[0].cpu().numpy()) <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# 5. the box is the dofmap operator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [3, 6])
def test_box_is_the_dofmap_operator(gpu, oracle, p):
    import torch
    om, V = box(oracle, p)
    x, y0 = inputs(V.ndofs, p, scale=1.0)
    a, b = stiffness(V, p, structured=True), stiffness(V, p, structured=False)
    assert is_ordered(a) and is_ordered(b) and a.info.structured == 1 and b.info.structured == 0
    assert a.info.alg_bytes == b.info.alg_bytes and a.info.device_bytes == b.info.device_bytes
    assert torch.equal(apply(a, x, y0, gpu), apply(b, x, y0, gpu))


# ---------------------------------------------------------------------------------------------------------------------
# 6. errors and selection
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_selection(gpu, oracle):
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd import tet
    from wave_fenics_amd._lib import WF_PART_ALL, WF_PART_INTERIOR
    p = 4
    om, V = box(oracle, p)
    for structured in (True, False):
        for bad in ({"update": "owner"}, {"kernel": "march"}, {"geometry": "per_cell"}, {"update": 3}, {"lz": 2}):
            with pytest.raises(w.WavehipError):
                stiffness(V, p, structured=structured, tuning=bad)
        op = stiffness(V, p, structured=structured, tuning={"keep_cell_order": True})
        assert is_ordered(op)
        assert op.set_ghost_faces(True, False, False) is False
        assert op.set_ghost_dofs(np.arange(5, dtype=np.int32)) is False
        x, y0 = inputs(V.ndofs, 3, scale=1.0)
        xd, y = dev(x, gpu), dev(y0, gpu)
        op.apply_part(xd, y, WF_PART_ALL)
        torch.cuda.synchronize()
        assert torch.equal(y, apply(op, x, y0, gpu))
        with pytest.raises(w.WavehipError):
            op.apply_part(xd, y, WF_PART_INTERIOR)
    # wf_tuning.update = 3 stays an error without the flag as well
    with pytest.raises(w.WavehipError):
        stiffness(V, p, structured=True, flags=0, tuning={"update": 3})
    Vt = tet.create_kuhn_box((2, 2, 2), 2)
    tet.TetStiffnessOperator(Vt, 2)
    with pytest.raises(w.WavehipError, match="ORDERED"):
        tet.TetStiffnessOperator(Vt, 2, flags=ORDERED())


@pytest.mark.parametrize("p", [5, 6, 7])
def test_defaults_unchanged(gpu, oracle, p):
    """Without the flag the default selection is what it was."""
    import wave_fenics_amd as w
    om, V = box(oracle, p, perturb=0.0, n=(3, 3, 3))
    assert form(stiffness(V, p, structured=True, flags=0)) == DEFAULT
    om, V = box(oracle, p)
    assert form(stiffness(V, p, structured=True, flags=0)) == DEFAULT
    assert stiffness(V, p, flags=0).kernel in ("march_idx", "batch_unique")
    assert w.MassOperatorLumped(V, p, structured=False).kernel == "diagonal"
    assert w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=2 * p).kernel in ("march_idx", "batch_unique")
    assert w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=2 * p + 2).kernel == "mass_dense_any"


@pytest.mark.parametrize("p", [2, 4])
def test_alg_bytes_and_device_bytes(gpu, oracle, p):
    import wave_fenics_amd as w
    from wave_fenics_amd._lib import WF_FLAG_MASS_ELEMENTWISE
    om, V = box(oracle, p)
    nc, nd, N = om.ncells, (p + 1) ** 3, om.ndofs
    extra = 20 * nc * nd + 4 * (N + 1)
    K = stiffness(V, p)
    assert K.info.alg_bytes == nc * (48 * nd + 4 * nd) + 16 * N + extra
    Kb = stiffness(V, p, flags=0, tuning={"kernel": "elementwise"})     # the same arrays without the ordered plan
    assert K.info.device_bytes == Kb.info.device_bytes + 12 * nc * nd + 4 * (N + 1)
    M = w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=2 * p + 2, flags=ORDERED())
    assert M.info.alg_bytes == nc * (8 * (p + 2) ** 3 + 4 * nd) + 16 * N + extra
    L = w.MassOperatorLumped(V, p, structured=False, flags=ORDERED() | WF_FLAG_MASS_ELEMENTWISE)
    assert L.info.alg_bytes == nc * (8 * nd + 4 * nd) + 16 * N + extra
    D = w.MassOperatorLumped(V, p, structured=False, flags=ORDERED())
    assert D.info.alg_bytes == 24 * N and D.info.device_bytes == w.MassOperatorLumped(V, p, structured=False).info.device_bytes


def test_cg_takes_an_ordered_operator(gpu, oracle):
    """wf_cg with an ordered dense mass (SPD): the operator is applied like any other.  The reductions of wf_dot keep
    their atomics, so only convergence is asserted, not the iteration count."""
    import torch
    import wave_fenics_amd as w
    p = 2
    om, V = box(oracle, p)
    M = w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=2 * p + 2, flags=ORDERED())
    assert is_ordered(M)
    xs = np.random.default_rng(1).uniform(-1, 1, om.ndofs)
    b = apply(M, xs, np.zeros(om.ndofs), gpu)
    x = torch.zeros_like(b)
    its, res = w.la.cg(x, b, M, kmax=200, rtol=1e-10)
    torch.cuda.synchronize()
    assert 0 < its < 200 and res < 1e-10
    assert relerr(x.cpu().numpy(), xs) <= 1e-7
