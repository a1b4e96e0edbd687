"""P4 owner kernel with the in-cell products by lane exchange ("r18").

A cell's 4 x 4 lines are one DPP row of a wave: the +x / +y line operands come from other lanes' registers, the -x / -y
lines are read by the first line of a cell only.  A wrong source lane, a wrong rotated coefficient or a wrong cell scale
changes single entries of K, which a smooth x can hide, so the whole matrix of a small graded box is compared with the
oracle's entry by entry.  The other cases run every cross-section on boxes that leave partial columns and columns that
hold only the closing line, split the apply at ghost planes, and repeat it."""
import itertools

import numpy as np
import pytest

from owner_helpers import apply, box, graded, owner
from support import gpu, relerr  # noqa: F401

pytestmark = pytest.mark.gpu

P = 4
TOL_ORACLE = 1e-12   # of max|y_ref|: the suite's stiffness bound; of max|K| for the matrix
TOL_FORM = 1e-13     # against the atomic axes form: only the summation order differs
VARIANTS = {0: "4x4", 1: "8x2", 2: "2x8"}
# cells: one more than the cross-section (a partial column) and exactly the cross-section (a column of the closing line alone)
PARTIAL = {1: [(9, 3, 3), (8, 2, 2)], 0: [(5, 5, 3), (4, 4, 2)], 2: [(3, 9, 2), (2, 8, 2)]}


_matrix = {}


def oracle_matrix(oracle):
    if "K" not in _matrix:
        om, V = graded(oracle, (3, 3, 3), P, seed=4)
        op = oracle.StiffnessOperator(om, P)
        K = np.zeros((om.ndofs, om.ndofs))
        e = np.zeros(om.ndofs)
        for c in range(om.ndofs):
            e[c] = 1.0
            op(e, K[c])   # row c of the array = K e_c
            e[c] = 0.0
        K.setflags(write=False)
        _matrix["K"] = (V, K)
    return _matrix["K"]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_full_matrix(gpu, oracle, variant):
    """Every entry of K on a graded 3 x 3 x 3 box (2 197 dofs), to 1e-12 of max|K|, and its symmetry to the same bound."""
    import torch
    V, Kref = oracle_matrix(oracle)
    n = V.ndofs
    assert n == 2197
    op = owner(V, P, variant=variant)
    X = torch.eye(n, dtype=torch.float64, device=gpu)
    Y = torch.zeros(n, n, dtype=torch.float64, device=gpu)
    for c in range(n):
        op(X[c], Y[c])
    torch.cuda.synchronize()
    K = Y.cpu().numpy()
    scale = np.abs(Kref).max()
    err = np.abs(K - Kref).max() / scale
    asym = np.abs(K - K.T).max() / scale
    print(f"{VARIANTS[variant]}: max|K - K_oracle| / max|K| = {err:.3e}, asymmetry {asym:.3e}")
    assert err <= TOL_ORACLE, err
    assert asym <= TOL_ORACLE, asym


@pytest.mark.parametrize("variant,n", [(v, n) for v in sorted(PARTIAL) for n in PARTIAL[v]])
def test_partial_columns(gpu, oracle, variant, n):
    V, x, y0, yref, yatom = box(oracle, n, P, sum(n), gpu)
    for lz in (1, 2, n[2]):
        op = owner(V, P, variant=variant, lz=lz)
        assert op.info.plan_lz == lz
        y = apply(op, x, y0, gpu)
        eo, ea = relerr(y, yref), relerr(y, yatom)
        print(f"{VARIANTS[variant]} {n} lz {lz}: oracle {eo:.3e}, atomic form {ea:.3e}")
        assert eo <= TOL_ORACLE, (lz, eo)
        assert ea <= TOL_FORM, (lz, ea)


@pytest.mark.parametrize("lz0", [1, 3])
@pytest.mark.parametrize("ghost", list(itertools.product((0, 1), repeat=3)))
def test_ghost_split(gpu, oracle, ghost, lz0):
    """interior + interface == the whole apply, bitwise (every y entry has one owner and one order of summation), and the
    interior part stays finite with the ghost planes of x set to NaN: a lane that skips the -x / -y reads adds no NaN."""
    import torch
    from wave_fenics_amd._lib import WF_PART_INTERFACE, WF_PART_INTERIOR
    n = (9, 3, 3)
    V, x_np, _, _, _ = box(oracle, n, P, sum(n), gpu)
    NX, NY, NZ = V.lattice
    lat = np.arange(V.ndofs).reshape(NZ, NY, NX)
    gpos = np.unique(np.concatenate([lat[:, :, 0].ravel() if ghost[0] else [], lat[:, 0, :].ravel() if ghost[1] else [],
                                     lat[0, :, :].ravel() if ghost[2] else []])).astype(np.int64)
    x = torch.from_numpy(x_np.copy()).to(gpu)
    xp = x.clone()
    if gpos.size:
        xp[torch.from_numpy(gpos).to(gpu)] = float("nan")
    for variant in sorted(VARIANTS):
        op = owner(V, P, variant=variant, lz=3, lz0=lz0)
        assert op.set_ghost_faces(*[bool(g) for g in ghost])
        assert (op.info.items_interface > 0) == any(ghost)
        yall = torch.zeros_like(x)
        op(x, yall)
        y = torch.zeros_like(x)
        op.apply_part(xp, y, WF_PART_INTERIOR)
        assert bool(torch.isfinite(y).all()), (VARIANTS[variant], "interior part read a ghost dof")
        op.apply_part(x, y, WF_PART_INTERFACE)
        torch.cuda.synchronize()
        d = (y != yall).nonzero().flatten().cpu().numpy()
        if d.size:
            print(f"{VARIANTS[variant]} ghost {ghost} lz0 {lz0}: {d.size} entries differ, max {float((y - yall).abs().max()):.3e}; "
                  f"first at (I, J, K) = {[(int(q % NX), int(q // NX % NY), int(q // (NX * NY))) for q in d[:6]]}")
        assert torch.equal(y, yall), VARIANTS[variant]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_repeatable(gpu, oracle, variant):
    import torch
    V, x_np, y0_np, _, _ = box(oracle, PARTIAL[variant][0], P, sum(PARTIAL[variant][0]), gpu)
    op = owner(V, P, variant=variant)
    x, y0 = torch.from_numpy(x_np.copy()).to(gpu), torch.from_numpy(y0_np.copy()).to(gpu)
    first = None
    for _ in range(50):
        y = y0.clone()
        op(x, y)
        if first is None:
            first = y
        else:
            assert torch.equal(y, first)
