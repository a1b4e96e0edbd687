"""Conditions on the reference and the bound of the entry-wise stiffness tests (tests/stiffness_entry_helpers.py).  No GPU.

What keeps tests/test_gpu_stiffness_entries.py honest:
  * the reference's inputs are the kernels' inputs: the oracle's 1-D table is the library's, bit for bit;
  * float64 and long double agree on every clamp decision (window margin >= 1e-3 on every mesh);
  * the per-cell reference G_c is idx_cell_helpers.cell_geometry_longdouble up to its bound, and the host rule's float64
    G_c lies within half of that bound;
  * B is not tight enough to fail a right kernel: both float64 forms of the oracle (dense tables, sum-factorised), fed
    with the reference's G rounded to float64, stay within B / 2 on every field, both y0, every mesh;
  * B is not loose enough to pass a wrong one: an error of 1e-13 max|y| at one quiet entry passes the 1e-12 check of every
    older test and fails this one at that entry; a sign error or a swapped component in the off-diagonal of G moves the
    reference by more than 1e6 B eps mag;
  * the null-space fields ask what they seem to: in the reference every row of K 1 and every interior row of the linear
    field is below B eps mag, while the boundary rows of the linear field are 1e14 times that."""
import numpy as np
import pytest

import idx_cell_helpers as ich
import stiffness_entry_helpers as se
from support import EPS, LD, bits, relerr, wpackage  # noqa: F401


def unique_meshes():
    """one case per (mesh, degree, form)"""
    seen = {}
    for c in se.cases():
        seen.setdefault((c.mesh[0].__name__, c.mesh[1], c.form), c)
    return list(seen.values())


MESHES = unique_meshes()
IDS = [f"{c.mesh[0].__name__}-{'-'.join(str(a) for a in c.mesh[1])}-{c.form}" for c in MESHES]


def test_oracle_table_is_the_library_table(wpackage, oracle):
    for p in range(1, 8):
        _, _, D = wpackage.tabulate_gll(p)
        assert np.array_equal(bits(D), bits(se.table(p)[0])), p


def test_window_margin(wpackage):
    worst = min((se.data(c).margin, i) for c, i in zip(MESHES, IDS))
    print("smallest window margin:", worst)
    assert worst[0] >= se.MARGIN, worst
    # the affine meshes never see the clamp act; the perturbed ones do from P4 on, and the reference follows
    assert all(se.data(c).geo.changed == 0 for c in MESHES if c.affine)
    assert any(se.data(c).geo.changed > 0 for c in MESHES if not c.affine and c.p >= 4)


@pytest.mark.parametrize("kind", ["sheared", "graded"])
def test_cell_rule_reference(wpackage, kind):
    for c in MESHES:
        if c.mesh[0] is not se.box_mesh or c.mesh[1][0] != kind:
            continue
        V, om, _ = se.mesh_of(c)
        G, Gb = se.cell_rule_ld(om.x, om.geom_dofmap)
        plain = ich.cell_geometry_longdouble(V.mesh)
        Gc, bad, reason = wpackage.hex_cell_geometry(V.mesh, c.p)
        assert (bad, reason) == (-1, 0)
        for m, (r, s) in enumerate(ich.COMP):
            assert np.all(np.abs(G[:, r, s] - plain[:, m]) <= Gb[:, r, s]), (c.id, m)
            assert np.all(np.abs(Gc[:, m].astype(LD) - G[:, r, s]) <= Gb[:, r, s] / 2), (c.id, m)
            if kind == "graded" and r != s:
                assert np.all(G[:, r, s] == 0) and np.all(Gb[:, r, s] == 0) and np.all(Gc[:, m] == 0)


@pytest.mark.parametrize("case", MESHES, ids=IDS)
def test_impulse_dofs_are_what_they_are_named(wpackage, case):
    """Every occurrence of an impulse dof in the dofmap: an edge dof has one local coordinate inside 1..P-1, along the named
    axis, and four cells; a face dof two and two cells; the interior dof three and one cell; vertex8 none and eight cells.
    P1 has vertices only; every box and the holed mesh have all nine impulses from P2 on, the batch meshes (a box cut
    off after 2 B + 1 cells) at least an edge, a face and the interior."""
    _, om, _ = se.mesh_of(case)
    p, n = case.p, case.p + 1
    dm = np.asarray(om.dofmap)
    got = dict(se.impulse_dofs(om, p))
    for name, d in got.items():
        cells, local = np.nonzero(dm == d)
        ijk = np.stack([local % n, (local // n) % n, local // (n * n)], axis=1)
        inside = (ijk > 0) & (ijk < p)
        if name == "vertex8":
            assert len(cells) == 8 and not inside.any()
        elif name == "last":
            assert d == dm.max() and not inside.any()
        else:
            axes, ncells = {"edge": (1, 4), "face": (2, 2), "interior": (3, 1)}[name.split("-")[0]]
            assert len(cells) == ncells and np.all(inside.sum(axis=1) == axes), (case.id, name)
            if name != "interior":
                want = np.array([c in name.split("-")[1] for c in "xyz"])
                assert np.all(inside == want[None, :]), (case.id, name)
    if p == 1:
        assert set(got) == {"vertex8", "last"}
    elif case.mesh[0] is se.batch_mesh:
        kinds = {k.split("-")[0] for k in got}
        assert {"edge", "face", "interior", "last"} <= kinds, (case.id, sorted(got))
    else:
        assert set(got) == {"vertex8", "last"} | set(se.IMPULSE_LOCAL), (case.id, sorted(got))


def oracle_forms(oracle, om, p, G64):
    """The two float64 applies of the oracle on the geometry G64.  The dense one has no entry that takes G: the operator
    computes the oracle's own G when it is made and its __call__ reads self.G, so that attribute is replaced (as
    medium_helpers.stiffness_reference does for the coefficient tests); the oracle's G is not used here."""
    K = oracle.StiffnessOperator(om, p, {"c0": se.C0})
    K.G = G64

    def dense(x, y):
        K(np.ascontiguousarray(x), y)

    def sumfact(x, y):
        oracle.stiffness_apply_sumfact(om, G64, se.C0, np.ascontiguousarray(x), y)
    return (("dense", dense), ("sumfact", sumfact))


@pytest.mark.parametrize("case", MESHES, ids=IDS)
def test_oracle_forms_within_half_of_B(wpackage, oracle, case):
    d = se.data(case)
    B = se.bound(case.form, case.p)
    G64 = np.ascontiguousarray(d.geo.G.astype(np.float64))
    worst = {}
    for a, rows in ((None, list(enumerate(d.names))), (d.a, [(0, "hetero")])):
        Ga = G64 if a is None else np.ascontiguousarray(G64 * a[:, None, None, None])
        for form, apply in oracle_forms(oracle, d.om, case.p, Ga):
            for f, name in rows:
                ax, mag, gerr = (d.ax[f], d.mag[f], d.gerr[f]) if a is None else (d.axh, d.magh, d.gerrh)
                for y0 in (np.zeros(d.om.ndofs), se.scaled_y0(mag, 5 + f)):
                    y = y0.copy()
                    apply(d.X[f], y)
                    r, ok, at, _ = se.entry_check(y, y0, ax, mag, gerr, B / 2)
                    worst[form] = max(worst.get(form, 0.0), r)
                    assert ok, (case.id, form, name, "y0" if y0.any() else "y0 = 0", at, r, B / 2)
                    quiet = np.asarray(mag == 0)
                    assert np.array_equal(bits(y[quiet]), bits(y0[quiet])), (case.id, form, name)
    # G_bound's part of the allowance in units of B eps mag: the largest over the entries of the uniform and decay fields,
    # and of the impulses, where an entry can hang on one off-diagonal G(q) alone, whose bound is relative to the diagonal
    share = {}
    for f, name in enumerate(d.names):
        pos = d.mag[f] > 0
        key = "impulse" if name.startswith("impulse") else "fields"
        share[key] = max(share.get(key, 0.0), float(np.max(d.gerr[f][pos] / (LD(B) * LD(EPS) * d.mag[f][pos]))))
    print(f"ENTRY host {IDS[MESHES.index(case)]}: B {B} " + " ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + " gerr / (B eps mag): " + " ".join(f"{k} {v:.2f}" for k, v in share.items()))


def teeth_cases():
    return [c for c in MESHES if (c.family, c.p) in (("march_point", 2), ("march_point", 4), ("owner", 4), ("ksplit", 6))]


@pytest.mark.parametrize("case", teeth_cases(), ids=lambda c: c.id)
def test_entry_check_sees_what_the_max_norm_check_misses(wpackage, oracle, case):
    d = se.data(case)
    B = se.bound(case.form, case.p)
    G64 = np.ascontiguousarray(d.geo.G.astype(np.float64))
    _, apply = oracle_forms(oracle, d.om, case.p, G64)[1]
    planted = []
    for f, name in enumerate(d.names):
        if not (name.startswith("decay") or name.startswith("impulse")):
            continue
        y0 = se.scaled_y0(d.mag[f], 5 + f)
        y = y0.copy()
        apply(d.X[f], y)
        ref = (y0.astype(LD) + d.ax[f]).astype(np.float64)
        assert se.entry_check(y, y0, d.ax[f], d.mag[f], d.gerr[f], B)[1]
        if name.startswith("decay"):     # the quietest entry that the operator touches
            m = np.where(d.mag[f] > 0, np.abs(y0) + d.mag[f], np.inf)
            at = int(np.argmin(m))
        else:                            # an entry outside the impulse's support: only y0 lives there
            out = np.nonzero(~se.support_of(d.om, d.impulses[name]))[0]
            at = int(out[np.argmin(np.abs(y0[out]))])
        stray = 1e-13 * np.abs(y).max()
        y[at] += stray
        assert relerr(y, ref) <= 1e-12, (name, relerr(y, ref))                 # the check in force lets it through
        r, ok, first, _ = se.entry_check(y, y0, d.ax[f], d.mag[f], d.gerr[f], B)
        assert not ok and first == at, (name, at, first, r)
        planted.append((name, at, r))
    assert sum(n.startswith("decay") for n, _, _ in planted) == 6 and sum(n.startswith("impulse") for n, _, _ in planted) >= 3
    for name, at, r in planted:
        print(f"ENTRY teeth {case.id} {name}: 1e-13 max|y| at entry {at} passes relerr <= 1e-12, entry ratio {r:.3e} > B = {B}")


@pytest.mark.parametrize("case", [c for c in MESHES if c.form in ("point", "cell_full") and c.family in ("march_point", "march_cell_full", "ksplit")],
                         ids=lambda c: c.id)
def test_off_diagonal_errors_would_be_told_apart(wpackage, case):
    """G01 with the wrong sign, and G01 and G12 in each other's place (a component order off by a transposition of the
    blocked layout), move the reference by more than 1e6 B eps mag at some entry of the uniform field."""
    from types import SimpleNamespace
    d = se.data(case)
    B = se.bound(case.form, case.p)
    for what in ("sign", "swap"):
        G = d.geo.G.copy()
        if what == "sign":
            G[..., 0, 1] *= -1
            G[..., 1, 0] *= -1
        else:
            G[..., 0, 1], G[..., 1, 2] = d.geo.G[..., 1, 2], d.geo.G[..., 0, 1]
            G[..., 1, 0], G[..., 2, 1] = d.geo.G[..., 2, 1], d.geo.G[..., 1, 0]
        ax, _, _ = se.reference(d.om, case.p, SimpleNamespace(G=G, G_bound=d.geo.G_bound), d.X[:1])
        moved = float(np.max(np.abs(ax[0] - d.ax[0]) / (LD(EPS) * d.mag[0])))
        print(f"ENTRY apart {case.id} {what}: {moved:.3e} eps mag")
        assert moved >= 1e6 * B, (case.id, what, moved)


@pytest.mark.parametrize("case", MESHES, ids=IDS)
def test_null_space_rows_are_at_rounding_level(wpackage, case):
    """What the null-space fields ask of a kernel: in the reference every row of K 1, and every interior row of K (a . X + b)
    on an affine mesh, is below B eps mag -- a result at 1e-16 of its magnitude (not exactly 0: the rows of the float64
    table D sum to a rounding residue, and the dof coordinates are rounded) -- so the entry check is a null-space check
    at every row, which max|K 1| against max|K x| of another field is not."""
    d = se.data(case)
    B = se.bound(case.form, case.p)
    f = d.names.index("ones")
    pos = d.mag[f] > 0
    ones = float(np.max(np.abs(d.ax[f][pos]) / (LD(EPS) * d.mag[f][pos])))
    assert ones <= B, (case.id, ones)
    line = f"ENTRY null {IDS[MESHES.index(case)]}: |K 1| <= {ones:.2f} eps mag"
    if case.affine:
        f = d.names.index("linear")
        NX, NY, NZ = d.om.lattice
        k, j, i = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing="ij")
        inner = ((i > 0) & (i < NX - 1) & (j > 0) & (j < NY - 1) & (k > 0) & (k < NZ - 1)).reshape(-1)
        lin = float(np.max(np.abs(d.ax[f][inner]) / (LD(EPS) * d.mag[f][inner])))
        edge = float(np.max(np.abs(d.ax[f][~inner]) / (LD(EPS) * d.mag[f][~inner])))
        assert lin <= B and edge >= 1e6 * B, (case.id, lin, edge)     # the boundary rows carry the flux: not small
        line += f", interior rows of the linear field <= {lin:.2f}, boundary rows up to {edge:.2e}"
    print(line)
