"""Conditions on the reference, the bound and the cases of the entry-wise mass tests (tests/mass_entry_helpers.py).  No GPU.

What keeps tests/test_gpu_mass_entries.py honest:
  * headroom: two float64 forms of every operator -- the C oracle (oracle.dense_mass_apply, the dense Phi [nq][nd]
    product) or the lumped numpy form, and a sum-factorised form with the passes in another order (z, y, x forward,
    then x, y, z) -- stay within B / 2 at every entry of every field, both y0, every case's mesh and table;
  * the geometry reference's own bound: dbound of hex_geometry_helpers.point_geometry_ld on the meshes of the
    explicit-table cases is up to DBOUND_SHARE times B eps |d| -- not below it -- and the float64 det J w those cases
    hand over lies within it;
  * the gap is real: float64 mutants of a numpy restatement of the marching kernel and of the batch kernel pass
    max|y - y_ref| <= 1e-12 max|y_ref| and miss the entry bound by more than 1e6 B;
  * the deep case reaches what it claims: the ring arithmetic of k_mass_march restated; every cursor of the index ring
    wraps in an item of nine layers, none in the items of at most three layers that the older tests run;
  * bookkeeping: the march cases are WF_MASS_SHAPES, the case counts, the impulse dofs' multiplicities, the unnamed dofs
    of the stair mesh, both checkerboard values in every batch and every item of more than one cell."""
import os

import numpy as np
import pytest

import mass_entry_helpers as me
import stiffness_entry_helpers as se
from guard_helpers import CSRC, compiled_shapes
from owner_helpers import spaces
from support import EPS, LD, bits, cells_per_batch, relerr, wpackage  # noqa: F401

CASES = me.cases()


def unique_data():
    """one case per (operator, mesh, table, det J source): what mass_entry_helpers.data() keys its references by"""
    seen = {}
    for c in CASES:
        seen.setdefault((c.op, c.mesh[0].__name__, c.mesh[1], c.table and (c.table[0].__name__, c.table[1]), c.source), c)
    return list(seen.values())


DATA = unique_data()


def unique_meshes():
    seen = {}
    for c in CASES:
        seen.setdefault((c.mesh[0].__name__, c.mesh[1]), c)
    return list(seen.values())


MESHES = unique_meshes()


def mesh_id(c):
    return f"{c.mesh[0].__name__}-{'-'.join(str(a) for a in c.mesh[1])}"


# ---------------------------------------------------------------------------------------------------------------------
# bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def test_march_cases_are_the_compiled_shapes():
    shapes = compiled_shapes("mass_march.hip", "WF_MASS_SHAPES")
    seg = [c for c in CASES if c.family == "march_segments"]
    assert [(c.p, me.table_of(c).m) + c.tuning["block"][:2] for c in seg] == shapes and len(set(shapes)) == len(shapes)
    for c in seg:
        bx, by, _ = c.tuning["block"]
        assert c.mesh[1][1] == (bx + 1, by + 1, me.NZ) and c.tuning["lz"] == me.LZ
    pairs = sorted({s[:2] for s in shapes})
    deep = [c for c in CASES if c.family == "march_deep"]
    assert sorted((c.p, me.table_of(c).m) for c in deep) == pairs
    for c in deep:
        bx, by = next(s[2:] for s in shapes if s[:2] == (c.p, me.table_of(c).m))       # the pair's default
        assert c.tuning == {"kernel": "mass_march", "block": (bx, by, 0), "lz": me.DEEP_LZ}
        assert c.mesh[1][1] == (bx + 1, by + 1, me.DEEP_LZ + 1)
    assert me.NCASES["march_segments"] == len(shapes) and me.NCASES["march_deep"] == len(pairs)


def test_case_counts():
    got = {}
    for c in CASES:
        got[c.family] = got.get(c.family, 0) + 1
    assert got == me.NCASES and len({c.id for c in CASES}) == len(CASES) == sum(me.NCASES.values())
    for c in CASES:
        if c.family == "column":
            assert me.table_of(c).m == c.p + 1 and me.table_of(c).phi1.shape == (c.p + 1, c.p + 1)
            # not collocated: a square table that is the identity would become the diagonal operator
            assert np.abs(me.table_of(c).phi1 - np.eye(c.p + 1)).max() > 0.1
        if c.family in ("column", "any_rule") or c.mesh[0] is me.cut_mesh:
            m = c.p + 1 if c.op == "lumped" or c.family == "column" else me.table_of(c).m
            cb = cells_per_batch(c.p) if c.op == "lumped" or c.family == "column" else me.mass_dense_cells_per_batch(max(c.p + 1, m))
            assert c.mesh[1][1] == 2 * cb + 1, c.id


@pytest.mark.parametrize("case", MESHES, ids=mesh_id)
def test_impulse_dofs_have_their_multiplicities(wpackage, case):
    _, om, _ = me.mesh_of(case)
    dm = np.asarray(om.dofmap)
    n = case.p + 1
    got = dict(se.impulse_dofs(om, case.p))
    for name, d in got.items():
        cells, local = np.nonzero(dm == d)
        ijk = np.stack([local % n, (local // n) % n, local // (n * n)], axis=1)
        inside = ((ijk > 0) & (ijk < case.p)).sum(axis=1)
        if name == "vertex8":
            assert len(cells) == 8 and not inside.any()
        elif name == "last":
            assert d == dm.max() and not inside.any()
        else:
            axes, ncells = {"edge": (1, 4), "face": (2, 2), "interior": (3, 1)}[name.split("-")[0]]
            assert len(cells) == ncells and np.all(inside == axes), (case.id, name)
    if case.p == 1:
        assert "last" in got
    elif case.mesh[0] is me.cut_mesh or (case.mesh[0] is se.box_mesh and min(case.mesh[1][1]) < 2):
        # a box cut off after 2 CB + 1 cells, the one-cell-thick box of P7: what such a mesh has
        assert {"interior", "last"} <= set(got) and any(k.startswith("face") for k in got), (case.id, sorted(got))
    else:
        assert set(got) == {"vertex8", "last"} | set(se.IMPULSE_LOCAL), (case.id, sorted(got))


def test_stair_mesh_has_unnamed_dofs(wpackage):
    for c in CASES:
        if c.nan:
            _, om, _ = me.mesh_of(c)
            named = np.zeros(om.ndofs, dtype=bool)
            named[np.asarray(om.dofmap).reshape(-1)] = True
            assert 0 < (~named).sum() < om.ndofs, c.id


def test_checkerboard_in_every_batch_and_item(wpackage):
    """both values in every batch (the caller's cell order is kept) and in every work item (column x z segment) that holds
    more than one cell: the one-cell last batch and the corner column's one-layer item cannot"""
    for c in CASES:
        _, om, coords = me.mesh_of(c)
        a = se.checkerboard(coords)
        if c.mesh[0] is me.cut_mesh:
            m = c.p + 1 if c.op == "lumped" or c.family == "column" else me.table_of(c).m
            cb = cells_per_batch(c.p) if c.op == "lumped" or c.family == "column" else me.mass_dense_cells_per_batch(max(c.p + 1, m))
            groups = [a[b:b + cb] for b in range(0, a.size, cb)]
            assert [g.size for g in groups] == [cb, cb, 1] or cb == 1
        elif c.family in ("march_segments", "march_deep"):
            bx, by, _ = c.tuning["block"]
            key = (coords[:, 0] // bx) + 2 * (coords[:, 1] // by) + 4 * (coords[:, 2] // c.tuning["lz"])
            groups = [a[key == k] for k in np.unique(key)]
            assert len(groups) == c.plan["items"]
        else:
            groups = [a]
        for g in groups:
            assert g.size == 1 or {se.CONTRAST, 1.0} == set(g.tolist()), c.id


# ---------------------------------------------------------------------------------------------------------------------
# headroom
# ---------------------------------------------------------------------------------------------------------------------
def cell_mass_zyx(phi, d, u):
    """me.cell_mass with the passes in the other order: z, y, x forward, then x, y, z"""
    t = np.einsum("sk,fckji->fcsji", phi, u)
    t = np.einsum("rj,fcsji->fcsri", phi, t)
    t = np.einsum("qi,fcsri->fcsrq", phi, t) * d[None]
    t = np.einsum("qi,fcsrq->fcsri", phi, t)
    t = np.einsum("rj,fcsri->fcsji", phi, t)
    return np.einsum("sk,fcsji->fckji", phi, t)


def float64_forms(oracle, d, case, a):
    """[(name, f(x, y): y += M x)]: the two float64 forms of the case's operator on the reference's inputs (the library's
    det J w is not computed here: the forms read the reference's d rounded to float64)"""
    om, p = d.om, case.p
    nc = np.asarray(om.dofmap).shape[0]
    d64 = np.ascontiguousarray(d.d.astype(np.float64)) if d.detJ is None else d.detJ
    if a is not None:
        d64 = np.ascontiguousarray(d64 * a[:, None])
    dm = np.asarray(om.dofmap).reshape(-1)
    if case.op == "lumped":
        def gather_scatter(x, y):
            np.add.at(y, dm, x[dm] * d64.reshape(-1))

        def diagonal(x, y):
            m = np.zeros(om.ndofs)
            np.add.at(m, dm, d64.reshape(-1))
            y += m * x
        return (("gather_scatter", gather_scatter), ("diagonal", diagonal))
    phi1 = np.asarray(d.phi1)
    m = phi1.shape[0]
    phi = np.ascontiguousarray(np.kron(phi1, np.kron(phi1, phi1)))

    def dense(x, y):
        oracle.dense_mass_apply(om, phi, d64, np.ascontiguousarray(x), y)

    def zyx(x, y):
        u = me.gathered(om, p, x[None], np.float64)
        y += me.scatter(om, cell_mass_zyx(phi1, d64.reshape(nc, m, m, m), u), 1)[0]
    return (("oracle", dense), ("zyx", zyx))


def entry_ratio(y, y0, ax, mag, derr, B):
    return se.entry_check(y, y0, ax, mag, derr, B)


@pytest.mark.parametrize("case", DATA, ids=lambda c: c.id)
def test_float64_forms_within_half_of_B(wpackage, oracle, case):
    d = me.data(case)
    B = me.bound(case.op, case.p, None if d.table is None else d.table.m)
    worst = {}
    for a, rows in ((None, list(enumerate(d.names))), (d.a, [(0, "hetero")])):
        for form, apply in float64_forms(oracle, d, case, a):
            for f, name in rows:
                ax, mag, derr = (d.ax[f], d.mag[f], d.derr[f]) if a is None else (d.axh, d.magh, d.derrh)
                for y0 in (np.zeros(d.om.ndofs), me.scaled_y0(mag, 5 + f)):
                    y = y0.copy()
                    apply(np.array(d.X[f]), y)
                    r, ok, at, _ = entry_ratio(y, y0, ax, mag, derr, B / 2)
                    worst[form] = max(worst.get(form, 0.0), r)
                    assert ok, (case.id, form, name, "y0" if y0.any() else "y0 = 0", at, r, B / 2)
                    quiet = np.asarray(mag == 0)
                    assert np.array_equal(bits(y[quiet]), bits(y0[quiet])), (case.id, form, name)
    # the known answer of x = 1 in the reference itself
    f = d.names.index("ones")
    assert abs(np.sum(d.ax[f]) - np.sum(d.d)) <= d.slack + LD(1e-17) * np.sum(d.mag[f]), case.id
    print(f"MASS host {case.id}: B {B} " + " ".join(f"{k} {v:.2f}" for k, v in worst.items()))


# dbound / (B eps |d|) at its worst point over the meshes of the explicit-table cases.  The issue expected the geometry's
# bound to stay below B eps |d|; it does not.  det J is built from J = sum_v x_v dphi_v, and the running error bound
# carries |x_v| |dphi_v|: vertex coordinates up to 1 against cell widths of 1/9 to 1/3, a factor 3 to 9 of cancellation
# that B, which counts the roundings of the apply alone, does not have.  Measured here: up to 20 B eps |d| for the dense
# cases (B >= 19), up to 43 for the lumped ones (B = 10).  So wherever the library builds det J w itself (source
# "library": four cases) the allowance is mostly the geometry reference's pessimistic bound, as it is for the per-point
# stiffness kernels on perturbed meshes; the explicit-table cases have derr = 0 and B alone binds, which is why they are
# the primary route.  The figure asserted is the stated factor, a property of the reference and of no kernel.
DBOUND_SHARE = 64.0


@pytest.mark.parametrize("case", [c for c in DATA if c.source == "tables" and c.mesh[0] is not me.oriented_mesh], ids=lambda c: c.id)
def test_geometry_bound_against_B(wpackage, case):
    _, om, _ = me.mesh_of(case)
    if case.op == "dense":
        t = me.table_of(case)
        _, dl, db = me.detj_library(om, t.pts, t.wts, False)
        B = me.bound("dense", case.p, t.m)
    else:
        import hex_geometry_helpers as hg
        _, dl, db = me.detj_library(om, *hg.gll(case.p), True)
        B = me.bound("lumped", case.p)
    share = float(np.max(db / (LD(B) * LD(EPS) * np.abs(dl))))
    print(f"MASS dbound {case.id}: dbound <= {share:.3f} B eps |d|, B {B}")
    assert share <= DBOUND_SHARE, (case.id, share)
    # and the float64 det J w handed to the explicit-table operators is the reference's up to that bound
    d64 = me.data(case).detJ
    assert np.all(np.abs(d64.astype(LD) - (dl if case.op == "dense" else np.abs(dl))) <= db), case.id


# ---------------------------------------------------------------------------------------------------------------------
# the gap is real: mutants
# ---------------------------------------------------------------------------------------------------------------------
MUTANT_P, MUTANT_M, MUTANT_N, MUTANT_LZ = 2, 4, (2, 2, 6), 3
THIN = 0.01


def mutant_mesh(oracle):
    """Perturbed box 2 x 2 x 6 of side 100 whose upper three layers are compressed to a hundredth of their height: under
    the decay that is quiet at the top, s >= 0.99 there and the cells' masses are a hundredth of the loud cells', so
    whatever goes wrong among those layers is below 1e-14 max|y|.  Items of 3 and 3 layers: the second item is the
    quiet one, and its last layer has two layers of its own item below it."""
    from nonbox_helpers import cell_coords
    from support import lattice_x
    nx, ny, nz = MUTANT_N
    h = 100.0 / nz
    vz = np.concatenate([np.arange(nz // 2 + 1) * h, 50.0 + THIN * h * np.arange(1, nz // 2 + 1)])
    x = lattice_x(np.linspace(0.0, 100.0, nx + 1), np.linspace(0.0, 100.0, ny + 1), vz)
    # interior vertices moved by 0.2 of the smallest spacing next to them, per axis
    iz, iy, ix = (v.reshape(-1) for v in np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij"))
    interior = (ix > 0) & (ix < nx) & (iy > 0) & (iy < ny) & (iz > 0) & (iz < nz)
    hz = np.minimum(np.diff(vz)[np.clip(iz - 1, 0, nz - 1)], np.diff(vz)[np.clip(iz, 0, nz - 1)])
    step = np.stack([np.full(x.shape[0], 100.0 / nx), np.full(x.shape[0], 100.0 / ny), hz], axis=1)
    x[interior] += (np.random.default_rng(42).uniform(-1, 1, x.shape) * 0.2 * step)[interior]
    om, V = spaces(oracle, MUTANT_N, MUTANT_P, x=x, hi=(100.0, 100.0, 100.0))
    return om, cell_coords(MUTANT_N)


def march_f64(om, coords, p, phi1, detJ, x, lz, mutant=None):
    """The marching kernel restated in float64 numpy, the whole cross-section one column: per item of lz layers, per
    layer the cells' Phi^T d Phi u; plane 0 picks up the plane P carried from the layer below (zero in an item's first
    layer), planes 0 .. P-1 go to the layer's result tile, which is flushed one layer late, plane P is carried; the
    epilogue flushes the last tile and the carried plane.  mutant, applied in the mesh's last layer only: "detj" (the
    det J of the layer below), "carry" (the carried plane dropped), "tile" (the flush issued during that layer adds the
    tile of two layers below at the positions of the layer below)."""
    n, m = p + 1, phi1.shape[0]
    dm = np.asarray(om.dofmap).reshape(-1, n, n, n)
    d = detJ.reshape(-1, m, m, m)
    nz = int(coords[:, 2].max()) + 1
    y = np.zeros(om.ndofs)
    layer_cells = [np.nonzero(coords[:, 2] == z)[0] for z in range(nz)]     # the same stack order in every layer
    for z0 in range(0, nz, lz):
        carry, tiles = None, []
        for li, z in enumerate(range(z0, min(z0 + lz, nz))):
            cells, last = layer_cells[z], z == nz - 1
            dl = d[layer_cells[z - 1]] if (mutant == "detj" and last) else d[cells]
            r = me.cell_mass(phi1, dl, x[dm[cells]][None])[0]
            if carry is not None and not (mutant == "carry" and last):
                r[:, 0] += carry
            carry = r[:, p].copy()
            tiles.append((dm[cells][:, :p], r[:, :p]))
            if li > 0:
                pos, val = tiles[li - 1]
                if mutant == "tile" and last:
                    val = tiles[li - 2][1]
                np.add.at(y, pos.reshape(-1), val.reshape(-1))
        pos, val = tiles[-1]
        np.add.at(y, pos.reshape(-1), val.reshape(-1))
        np.add.at(y, dm[cells][:, p].reshape(-1), carry.reshape(-1))
    return y


def batch_f64(om, p, phi1, detJ, x, cb, mutant=None):
    """k_mass_dense with the unique-dof tile restated: per batch of cb cells the tile Xu holds x at the batch's unique
    dofs, is zeroed, takes the cells' sums and is added to y.  mutant "tile" leaves x in the tile of the LAST batch."""
    n, m = p + 1, phi1.shape[0]
    dm = np.asarray(om.dofmap)
    nc = dm.shape[0]
    y = np.zeros(om.ndofs)
    for b0 in range(0, nc, cb):
        cells = np.arange(b0, min(b0 + cb, nc))
        uniq, loc = np.unique(dm[cells].reshape(-1), return_inverse=True)
        Xu = x[uniq]
        u = Xu[loc].reshape(1, cells.size, n, n, n)
        if not (mutant == "tile" and b0 + cb >= nc):
            Xu = np.zeros(uniq.size)
        np.add.at(Xu, loc.reshape(-1), me.cell_mass(phi1, detJ[cells].reshape(-1, m, m, m), u).reshape(-1))
        y[uniq] += Xu
    return y


def test_mutants_pass_the_max_norm_check_and_miss_the_entry_bound(wpackage, oracle):
    om, coords = mutant_mesh(oracle)
    p, m = MUTANT_P, MUTANT_M
    t = me.oracle_table(p, *me.rule_of(p, m))
    detJ, d, db = me.detj_tables(om, t)
    assert np.all(detJ > 0)
    names, X, _ = se.fields(om, p, False, seed=3)
    f = names.index("decay-z+")                                     # 2^(-40 s_z): loud at the bottom, quiet at the top
    x = np.array(X[f])
    top = oracle.dof_coordinates(om)[:, 2] >= 49.9
    assert np.abs(x[top]).max() <= 2.0 ** -39 and np.abs(x).max() > 0.5
    ax, mag, derr = me.reference_dense(om, p, t.phi1, d, db, X[f:f + 1])
    ax, mag = ax[0], mag[0]
    ref = ax.astype(np.float64)
    B = me.bound("dense", p, m)
    zero = np.zeros(om.ndofs)
    cb = 21
    assert cb == me.mass_dense_cells_per_batch(m) and om.ncells - cb == 3 and np.all(coords[cb:, 2] == MUTANT_N[2] - 1)
    forms = [("march", None, lambda mu: march_f64(om, coords, p, t.phi1, detJ, x, MUTANT_LZ, mu))] \
        + [("march", mu, lambda mu: march_f64(om, coords, p, t.phi1, detJ, x, MUTANT_LZ, mu)) for mu in ("detj", "carry", "tile")] \
        + [("batch", None, lambda mu: batch_f64(om, p, t.phi1, detJ, x, cb, mu)),
           ("batch", "tile", lambda mu: batch_f64(om, p, t.phi1, detJ, x, cb, mu))]
    for form, mu, run in forms:
        y = run(mu)
        old = relerr(y, ref)
        r, ok, at, _ = se.entry_check(y, zero, ax, mag, derr[0], B)
        print(f"MASS mutant {form} {mu}: relerr {old:.2e}, worst entry {r:.3e} eps mag (B {B})")
        assert old <= 1e-12, (form, mu, old)                        # the check in force lets every one of them through
        if mu is None:
            assert ok and r <= B / 2, (form, r)                     # the restatement itself is a third float64 form
        else:
            assert not ok and r > 1e6 * B, (form, mu, r)
            assert top[at], (form, mu, at)                          # and the first entry outside lies in the quiet layers


# ---------------------------------------------------------------------------------------------------------------------
# the index ring of k_mass_march
# ---------------------------------------------------------------------------------------------------------------------
def ring_walk(P, nl):
    """The ring of index planes of k_mass_march (csrc/mass_march.hip) in an item of nl layers, in units of planes (every
    base, advance and span is a multiple of TP): RP = 4 P + 1 planes; bases rb_flush = 0, rb_x = P + 1, rb_in = 2 P + 1;
    ring(base, pos) = base + pos, minus RP when that reaches RP; ring_advance adds P planes and subtracts RP when the sum
    reaches RP.  Per layer l: the flush of layer l - 1 (l > 0) reads P planes at rb_flush; with has_next (l + 1 < nl) the
    x prefetch and its store read P planes at rb_x (in the last layer the loads go to ring(rb_x, RP - P) and are
    dropped: checked for range only); with has_next2 (l + 2 < nl) P planes arrive at rb_in; then rb_flush (l > 0),
    rb_x, rb_in advance.  Epilogue: the flush of layer nl - 1 at rb_flush, one advance, the carried plane at rb_flush.
    The ring's contents are tracked, so every read is checked to return the plane the kernel's comments say it does.
    Returns {cursor: set of "split" (an access that straddles the ring's end: ring() wraps for some of its positions)
    and "turn" (an access at a base that ring_advance has wrapped)}."""
    RP = 4 * P + 1
    held = {s: s for s in range(2 * P + 1)}          # ring slot -> linear plane of the item's table; prologue: 0 .. 2 P
    base = {"rb_flush": 0, "rb_x": P + 1, "rb_in": 2 * P + 1}
    turned = dict.fromkeys(base, False)
    events = {k: set() for k in base}
    assert 2 * P + 1 < RP

    def slots(cursor, span):
        b = base[cursor]
        assert 0 <= b < RP
        if b + span > RP:
            events[cursor].add("split")
        if turned[cursor]:
            events[cursor].add("turn")
        return [b + s - RP if b + s >= RP else b + s for s in range(span)]

    def advance(cursor):
        base[cursor] += P
        if base[cursor] >= RP:
            base[cursor] -= RP
            turned[cursor] = True

    for l in range(nl):
        has_next, has_next2 = l + 1 < nl, l + 2 < nl
        if l > 0:
            assert [held[s] for s in slots("rb_flush", P)] == list(range(P * (l - 1), P * l)), (P, nl, l)
        if has_next:
            assert [held[s] for s in slots("rb_x", P)] == list(range(P * (l + 1) + 1, P * (l + 2) + 1)), (P, nl, l)
        else:
            b = base["rb_x"] + RP - P
            b = b - RP if b >= RP else b
            assert 0 <= b and all((b + s - RP if b + s >= RP else b + s) in held for s in range(P)), (P, nl, l)
        if has_next2:
            for s, plane in zip(slots("rb_in", P), range(P * (l + 2) + 1, P * (l + 3) + 1)):
                # the slot being overwritten is dead: its plane lies below those the flush of layer l - 1 may still be reading
                assert s not in held or held[s] < P * (l - 1), (P, nl, l, s)
                held[s] = plane
        if l > 0:
            advance("rb_flush")
        advance("rb_x")
        advance("rb_in")
    assert [held[s] for s in slots("rb_flush", P)] == list(range(P * (nl - 1), P * nl)), (P, nl)
    advance("rb_flush")
    assert [held[s] for s in slots("rb_flush", 1)] == [P * nl], (P, nl)
    return events


def test_ring_walk_mirrors_the_source():
    with open(os.path.join(CSRC, "mass_march.hip")) as f:
        text = f.read()
    for line in ("static constexpr int RP = 4 * P + 1, RPT = RP * TP;",
                 "int rb_flush = 0, rb_x = (P + 1) * TP, rb_in = (2 * P + 1) * TP;",
                 "return e >= RPT ? e - RPT : e;",
                 "if (base >= RPT) base -= RPT;",
                 "const int rbx = has_next ? rb_x : ring(rb_x, RPT - P * TP);",
                 "if (l > 0) ring_advance(rb_flush, P * TP);",
                 "ring_advance(rb_x, P * TP);",
                 "ring_advance(rb_in, P * TP);",
                 "ring_advance(rb_flush, P * TP);                 // -> plane P nl"):
        assert line in text, line


def test_deep_items_wrap_every_cursor():
    """In an item of nine layers every cursor has wrapped (turn) at every degree and, from P2 on, straddles the ring's end
    inside an access (split); at P1 an access is one plane and cannot straddle.  In items of at most three layers -- all
    that tests/test_gpu_mass_march_rect.py and the others run -- nothing wraps.  The first depths: rb_flush splits and turns in
    an item of 5 layers already, both in the epilogue (the flush of layer 4 starts at plane 4 P of 4 P + 1, and the advance
    to the carried plane wraps); inside the layer loop it does at 6.  rb_x and rb_in turn at 5 and split at 9."""
    first = {}
    for P in range(1, 8):
        for nl in range(1, 33):
            ev = ring_walk(P, nl)
            for cursor, kinds in ev.items():
                for k in kinds:
                    first.setdefault((P, cursor, k), nl)
            if nl <= 3:
                assert not any(ev.values()), (P, nl, ev)
        deep = ring_walk(P, me.DEEP_LZ)
        want = {"turn"} if P == 1 else {"turn", "split"}
        assert all(kinds == want for kinds in deep.values()), (P, deep)
        assert ("split" in {k for (q, _, k) in first if q == P}) == (P > 1)
        if P > 1:
            assert max(first[(P, c, k)] for c in ("rb_flush", "rb_x", "rb_in") for k in ("turn", "split")) == me.DEEP_LZ
            assert (first[(P, "rb_flush", "turn")], first[(P, "rb_flush", "split")]) == (5, 5)
            assert all(first[(P, c, "turn")] == 5 and first[(P, c, "split")] == 9 for c in ("rb_x", "rb_in"))
    print("MASS ring: first item depth per (P, cursor, event):", sorted(first.items()))
    for c in CASES:
        if c.family == "march_deep":
            assert c.tuning["lz"] == me.DEEP_LZ and c.mesh[1][1][2] == me.DEEP_LZ + 1
