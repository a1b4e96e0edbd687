"""Stiffness geometry handed over by the caller (G=) on meshes whose G does not fit one staging slab (stage_G9,
csrc/op_setup.hip).

A caller's G[cell][point][3][3] goes to the device through a temporary of at most 64 MiB and is packed slab by slab into
the blocked upper triangle; the packed destination of a slab is offset by the whole batches before it.  Every other
test that passes G= stays below one slab, where that offset is 0.  The boxes here are the smallest with a second slab:
perturbed by 0.2, so that G differs in every cell and a slab packed one batch off shows.  One route for each caller of
stage_G9: the batch kernels with the caller's array as it is (direct), the batch kernels with a cell coefficient (filled
cell by cell), and the lattice plan (filled slot by slot)."""
from types import SimpleNamespace

import numpy as np
import pytest

from medium_helpers import field
from support import cells_per_batch, dev, gpu, make, relerr  # noqa: F401

TOL = 1e-12        # of max|y_ref|: the bound of every parity test of the project
SEEN = 1e-3        # of max|y_ref|: what a misplaced slab must change at the least for the tests below to see it
C0 = 1500.0
STAGING = 64 << 20                          # bytes of the temporary
BOXES = {4: (20, 20, 19), 6: (14, 14, 14)}  # 7600 cells and 68.4 MB of G, 2744 cells and 67.8 MB
ROUTES = {"direct": ("batch", False, "batch_unique"), "fill_cell": ("batch", True, "batch_unique"),
          "fill_slot": ("march", False, "march_idx")}


def slab_cells(p):
    """cells of a slab: whole batches of CB cells in 64 MiB of G[cell][nd][9]"""
    CB, nd = cells_per_batch(p), (p + 1) ** 3
    return max(CB, (STAGING // (72 * nd)) // CB * CB)


@pytest.fixture(scope="module", params=sorted(BOXES), ids=lambda p: f"P{p}")
def case(request, oracle):
    """One box: the oracle's G, a coefficient that differs in every cell, x, y0 at the scale of K x and the oracle's
    y0 + K x without and with the coefficient.  Computed once per degree, shared, unchanged."""
    p = request.param
    n = BOXES[p]
    om, mesh, V = make(oracle, n, p, perturb=0.2)
    slab = slab_cells(p)
    assert slab == {4: 7450, 6: 2715}[p] and om.ncells == {4: 7600, 6: 2744}[p]
    assert om.ncells > slab
    # the plan's slots are at least the cells, and no batch width makes a slab longer than 64 MiB of G
    assert om.ncells > STAGING // (72 * (p + 1) ** 3)
    K = oracle.StiffnessOperator(om, p, {"c0": C0})
    a = field("distinct", mesh.x, mesh.geom_dofmap)
    rng = np.random.default_rng(sum(n) + p)
    x = rng.uniform(-1, 1, om.ndofs)
    kx, kax = np.zeros(om.ndofs), np.zeros(om.ndofs)
    K(x, kx)
    oracle.stiffness_apply_sumfact(om, np.ascontiguousarray(K.G * a[:, None, None, None]), C0, x, kax)
    y0 = rng.uniform(-1, 1, om.ndofs) * np.abs(kx).max()
    c = SimpleNamespace(p=p, n=n, om=om, V=V, G=K.G, a=a, slab=slab, x=x, y0=y0, yref={False: y0 + kx, True: y0 + kax},
                        second=np.unique(om.dofmap[slab:]))
    for v in (c.G, c.a, c.x, c.y0, c.yref[False], c.yref[True]):
        v.setflags(write=False)
    return c


def test_a_misplaced_slab_shows(case, oracle):
    """The second slab's cells with the G of the cells one batch earlier (its packed destination one batch off): the
    oracle's result changes by more than 1e-3 of max|y_ref|, without and with the coefficient, and on the second slab's
    dofs alone."""
    c = case
    CB, nc = cells_per_batch(c.p), c.om.ncells
    assert 0 < nc - c.slab <= c.slab - CB
    assert all(not np.array_equal(c.G[q], c.G[q - CB]) for q in range(c.slab, nc))
    for coeff in (False, True):
        G = c.G * c.a[:, None, None, None] if coeff else c.G.copy()
        right, wrong = np.zeros(c.om.ndofs), np.zeros(c.om.ndofs)
        oracle.stiffness_apply_sumfact(c.om, G, C0, c.x, right, cells=(c.slab, nc))
        G[c.slab:] = G[c.slab - CB:nc - CB].copy()
        oracle.stiffness_apply_sumfact(c.om, G, C0, c.x, wrong, cells=(c.slab, nc))
        yref = c.yref[coeff]
        whole, second = relerr(wrong, right, np.abs(yref).max()), relerr(wrong[c.second], right[c.second], np.abs(yref[c.second]).max())
        print(f"P{c.p} {c.n} coefficient {coeff}: cells {c.slab}..{nc - 1} one batch off change y by {whole:.3e} of max|y_ref|, "
              f"{second:.3e} on their own dofs")
        assert whole > SEEN and second > SEEN


@pytest.mark.gpu
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_given_G_beyond_one_slab(gpu, case, route):
    import wave_fenics_amd as w
    c = case
    kernel, coeff, want = ROUTES[route]
    op = w.StiffnessOperator(c.V, c.p, {"c0": C0}, G=c.G, structured=False, tuning={"kernel": kernel},
                             cell_coeff=c.a if coeff else None)
    assert op.kernel == want
    y = dev(c.y0.copy(), gpu)   # the shared arrays are read-only
    op(dev(c.x.copy(), gpu), y)
    y = y.cpu().numpy()
    yref = c.yref[coeff]
    whole, second = relerr(y, yref), relerr(y[c.second], yref[c.second])
    print(f"P{c.p} {c.n} {route} ({op.kernel}): {c.om.ncells} cells, slab {c.slab}; oracle {whole:.3e}, "
          f"on the dofs of cells {c.slab}.. {second:.3e}")
    assert whole <= TOL
    if kernel == "batch":
        assert second <= TOL
