"""Owner form of the box stiffness operator: the prologue of a run ("r20").

Before its first layer a workgroup loads the own x line below the run, y of the first layer, the G_c of two layers and
the x planes 0..P of the first layer, the plane loads unconditionally on clamped addresses and as early as their
addresses allow.  That can go wrong where a run starts, at the mesh edges and in what the clamped loads touch, so:

  * every cut from one layer per run (every plane passes through a prologue) to whole columns, and at P4 a caller's
    table of one-layer runs listed top layer first;
  * boxes of one cell, of a closing lattice line that is a column of its own (nx a multiple of BX), and of partial
    columns on both axes;
  * x and y inside guarded buffers (tests/guard_helpers.py), the padding of x NaN: a load that strays outside the
    vector and is used makes y non-finite, a stray store changes the padding of y.

y is compared with the oracle; at P4 every cut must give the bits of the default cut, at P2 and P6 (whose body does not
promise equal bits for a plane at the start and in the middle of a run) the cuts agree at the oracle's tolerance."""
import numpy as np
import pytest

from guard_helpers import MIN_NORMAL, NAN, NEG_ZERO, box_pad, guarded
from owner_helpers import graded, owner
from support import gpu, owner_columns, relerr  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-12   # of max|y_ref|, as tests/test_gpu_owner_update.py
BOXES = [(1, 1, 1), (8, 2, 2), (9, 3, 3), (17, 5, 2)]
# (degree, wf_tuning.variant - 1 or None for the degree's default cross-section)
FORMS = [(4, 0), (4, 1), (4, 2), (2, None), (6, None)]
P4_SHAPES = {0: (4, 4), 1: (8, 2), 2: (2, 8)}


_cases = {}


def case(oracle, n, p):
    """One graded box: the space, x with a distinct value per dof, a non-zero y0 at the scale of K x, the oracle's
    y0 + K x; computed once and read-only."""
    if (n, p) not in _cases:
        om, V = graded(oracle, n, p)
        rng = np.random.default_rng(100 * p + sum(n))
        x = -1.0 + 2.0 * (rng.permutation(om.ndofs) + 0.5) / om.ndofs
        assert np.unique(x).size == om.ndofs
        kx = np.zeros(om.ndofs)
        oracle.StiffnessOperator(om, p)(x, kx)
        y0 = rng.uniform(0.5, 1.0, om.ndofs) * rng.choice([-1.0, 1.0], om.ndofs) * np.abs(kx).max()
        _cases[(n, p)] = (V, x, y0, y0 + kx)
        for a in _cases[(n, p)][1:]:
            a.setflags(write=False)
    return _cases[(n, p)]


def guarded_apply(op, V, x, y0, gpu, tag):
    """y of the apply in guarded buffers (both alignments, both y sentinels; the four must agree bit for bit)."""
    import torch
    pad = box_pad(V.lattice[0], V.lattice[1])
    first = None
    for shift in (0, 1):
        for yfill in (NEG_ZERO, MIN_NORMAL):
            xg, gx = guarded(x, pad, shift, NAN, gpu)
            yg, gy = guarded(y0, pad, shift, yfill, gpu)
            op(xg, yg)
            torch.cuda.synchronize()
            assert gx.intact(), (tag, shift, "x padding written at", gx.changed()[:8])
            assert gy.intact(), (tag, shift, "y padding changed at", gy.changed()[:8])
            y = yg.cpu().numpy()
            assert np.isfinite(y).all(), (tag, shift, "y not finite at", np.nonzero(~np.isfinite(y))[0][:8])
            if first is None:
                first = y
            assert np.array_equal(y.view(np.int64), first.view(np.int64)), (tag, shift, "differs between buffers")
    return first


@pytest.mark.parametrize("n", BOXES, ids=lambda n: "x".join(map(str, n)))
@pytest.mark.parametrize("p,variant", FORMS, ids=lambda v: str(v))
def test_cuts(gpu, oracle, p, variant, n):
    V, x, y0, yref = case(oracle, n, p)
    tuning = {} if variant is None else {"variant": variant}
    nz = n[2]
    op = owner(V, p, **tuning)
    y_default = guarded_apply(op, V, x, y0, gpu, "default cut")
    e = relerr(y_default, yref)
    print(f"P{p} variant {variant} {n}: default cut lz {op.info.plan_lz}, oracle {e:.3e}")
    assert e <= TOL
    cuts = {f"lz {lz}": owner(V, p, lz=lz, **tuning) for lz in (1, 2, 3)}
    cuts["whole columns"] = owner(V, p, lz=nz, **tuning)
    assert cuts["lz 1"].info.plan_lz == 1 and cuts["whole columns"].info.plan_lz == nz
    if p == 4:
        bx, by = P4_SHAPES[variant]
        ncols = owner_columns(n, p, bx, by)
        table = np.array([(c, z, z + 1) for z in reversed(range(nz)) for c in range(ncols)], dtype=np.int32)
        op.set_runs(table)
        assert np.array_equal(op.runs(), table)
        cuts["one-layer runs, top layer first"] = op
    for name, cut in cuts.items():
        y = guarded_apply(cut, V, x, y0, gpu, name)
        eo, ec = relerr(y, yref), relerr(y, y_default)
        off = int((y.view(np.int64) != y_default.view(np.int64)).sum())
        print(f"  {name}: oracle {eo:.3e}, default cut {ec:.3e}, entries off the default cut {off}")
        assert eo <= TOL, name
        if p == 4:
            assert off == 0, name
        else:
            assert ec <= TOL, name
