"""Host side of the holed-mesh and periodic-numbering tests (tests/nonbox_helpers.py, tests/test_gpu_nonbox.py):
the meshes are what their names say, the folded box reference equals the oracle on the periodic dofmap, and the
two host plans that see such dofmaps -- wf_lattice_numbering and wf_ordered_slots -- keep their contracts on
them.  No GPU."""
import numpy as np
import pytest

import nonbox_helpers as nh
from support import relerr, wpackage as w  # noqa: F401
from test_ordered_plan import numpy_plan

# the folded reference against the oracle on the periodic dofmap: the four cases it was measured on (<= 5e-17 of
# max|y|) and one with two cells along a periodic axis
FOLD_CASES = [((3, 3, 3), (True, True, True), 2), ((1, 3, 2), (True, False, True), 4), ((2, 2, 2), (True, True, True), 3),
              ((1, 2, 3), (True, False, False), 6), ((2, 3, 3), (True, False, False), 2)]
# every mesh of the GPU file (test_gpu_nonbox.PERIODIC)
PERIODIC = [((3, 3, 3), (True, False, False)), ((3, 3, 3), (True, True, True)), ((4, 3, 5), (False, False, True)),
            ((7, 4, 3), (True, True, False)), ((2, 3, 3), (True, False, False)), ((2, 2, 2), (True, True, True)),
            ((1, 3, 3), (True, False, False)), ((3, 3, 1), (False, False, True))]


# --------------------------------------------------------------------------- the meshes
def test_meshes_are_what_their_names_say(w):
    coords = {name: nh.cell_coords(nh.HOLED_BOX)[nh.keep_mask(name)] for name in nh.MASKS}
    assert {k: len(v) for k, v in coords.items()} == {"L": 150, "cavity": 204, "stair": 135, "pillar": 160}
    for lz in (3, 8):
        for name in ("pillar", "stair", "cavity"):
            assert nh.has_cell_above_gap(coords[name], lz), (name, lz)
        assert nh.first_layer_empty(coords["stair"], lz)
        # ... as whole work items too at the cross-sections of P4 (5 x 2) and P6 (2 x 2); P1's 8 x 8 holds the whole mesh
        assert nh.first_layer_empty(coords["stair"], lz, (5, 2)) and nh.first_layer_empty(coords["stair"], lz, (2, 2))
        assert not nh.first_layer_empty(coords["stair"], lz, (8, 8))
        assert not nh.has_cell_above_gap(coords["L"], lz) and not nh.first_layer_empty(coords["L"], lz)
    # cells per slot of the plan's items: whole items deleted give 1.0 (cavity, 2 x 1 cells, one layer per item)
    assert nh.expected_fill(coords["cavity"], 1, (2, 1)) == 1.0 and nh.expected_fill(coords["cavity"], 3, (2, 1)) < 1.0
    assert nh.expected_fill(coords["pillar"], 3, (5, 2)) == 160 / (18 * 30) and nh.expected_fill(coords["L"], 1, (8, 8)) == 150 / (7 * 64)
    for name in nh.MASKS:   # one layer per item: nothing to be above of (the plan's own choice on meshes this small)
        assert not nh.has_cell_above_gap(coords[name], 1) and not nh.first_layer_empty(coords[name], 1)
    # a shuffled cell list is the same set of cells
    s = nh.holed_case("pillar-shuffled", 2)
    assert not np.array_equal(s.coords, coords["pillar"])
    assert sorted(map(tuple, s.coords)) == sorted(map(tuple, coords["pillar"]))
    assert nh.has_cell_above_gap(s.coords, 3)


@pytest.mark.parametrize("p", [1, 2, 4, 6])
@pytest.mark.parametrize("name", ["pillar", "cavity"])
def test_subset_and_topological_numbering(w, name, p):
    """"subset" leaves dofs no cell names (inside the hole); "topological" has none and is the same dofmap up to a
    renumbering of the dofs."""
    a, b = nh.holed_case(name, p, "subset"), nh.holed_case(name, p, "topological")
    nx, ny, nz = nh.HOLED_BOX
    assert a.V.ndofs == (p * nx + 1) * (p * ny + 1) * (p * nz + 1)
    unlisted = int((~a.listed).sum())
    # pillar: the (5 p - 1)(5 p + 1)(2 p - 1) dofs strictly inside the 5 x 5 x 2 deleted block, open towards x = 1;
    # cavity: the (2 p - 1)(p - 1)(3 p - 1) strictly inside the 2 x 1 x 3 inclusion (none at P1)
    assert unlisted == {"pillar": 5 * p * (5 * p + 1) * (2 * p - 1), "cavity": (2 * p - 1) * (p - 1) * (3 * p - 1)}[name]
    assert b.listed.all() and b.V.ndofs == a.V.ndofs - unlisted
    assert np.array_equal(a.mesh.geom_dofmap, b.mesh.geom_dofmap)
    da, db = a.V.dofmap.reshape(-1), b.V.dofmap.reshape(-1)
    ren = np.full(a.V.ndofs, -1, dtype=np.int64)
    ren[da] = db
    assert np.array_equal(ren[da], db)                                  # a function of the subset dof ...
    assert np.unique(ren[a.listed]).size == b.V.ndofs                   # ... that is one-to-one on the listed ones


def test_shuffled_variant_is_a_relabelling(w):
    a, s = nh.holed_case("pillar", 2), nh.holed_case("pillar-shuffled", 2)
    assert s.V.ndofs == a.V.ndofs and s.listed.sum() == a.listed.sum()
    key = lambda c: [tuple(r) for r in c.coords]      # noqa: E731
    row = {k: i for i, k in enumerate(key(a))}
    order = np.array([row[k] for k in key(s)])
    assert not np.array_equal(order, np.arange(order.size))
    ren = np.full(a.V.ndofs, -1, dtype=np.int64)
    ren[a.V.dofmap[order].reshape(-1)] = s.V.dofmap.reshape(-1)
    assert np.array_equal(ren[a.V.dofmap[order]], s.V.dofmap) and np.unique(ren[a.listed]).size == a.listed.sum()
    assert np.array_equal(a.mesh.geom_dofmap[order], s.mesh.geom_dofmap)


def test_subset_oracle_against_the_sum_factorised_one(w, oracle):
    """The holed reference (the dense-table oracle on the cell subset) once against the oracle's other
    implementation, restricted with cells=: the box's cell list reordered so that the kept cells are a range."""
    p = 3
    case = nh.holed_case("pillar", p)
    keep = nh.keep_mask("pillar")
    ob = oracle.create_box(nh.HOLED_BOX, p, perturb=nh.PERTURB)
    order = np.concatenate([np.nonzero(keep)[0], np.nonzero(~keep)[0]])
    ob.geom_dofmap = np.ascontiguousarray(ob.geom_dofmap[order])
    ob.dofmap = np.ascontiguousarray(ob.dofmap[order])
    assert np.array_equal(ob.dofmap[: keep.sum()], case.V.dofmap)
    G, _ = oracle.precompute_geometric_data(ob, p)
    x = np.random.default_rng(1).uniform(-1, 1, ob.ndofs)
    y_sub, y_sf, y_all = np.zeros(ob.ndofs), np.zeros(ob.ndofs), np.zeros(ob.ndofs)
    oracle.StiffnessOperator(case.om, p)(x, y_sub)
    oracle.stiffness_apply_sumfact(ob, G, 1500.0, x, y_sf, cells=(0, int(keep.sum())))
    oracle.stiffness_apply_sumfact(ob, G, 1500.0, x, y_all)
    assert relerr(y_sub, y_sf) <= 1e-13
    assert np.all(y_sub[~case.listed] == 0.0) and relerr(y_all, y_sf) > 1e-2      # the deleted cells do matter


# --------------------------------------------------------------------------- the folded reference
@pytest.mark.parametrize("n,periodic,p", FOLD_CASES)
def test_folded_reference_is_the_periodic_oracle(w, oracle, n, periodic, p):
    case = nh.periodic_case(n, p, periodic)
    assert case.V.ndofs == case.om.ndofs == int(case.l2g.max()) + 1 < case.ob.ndofs
    assert np.array_equal(np.unique(case.l2g), np.arange(case.V.ndofs))
    per, box = nh.reference_operators(case.om, p, (2 * p,)), nh.reference_operators(case.ob, p, (2 * p,))
    x = np.random.default_rng(p).uniform(-1, 1, case.V.ndofs)
    for name in ("stiffness", "lumped", ("dense", 2 * p)):
        y = np.zeros(case.V.ndofs)
        per[name](x, y)
        yf = nh.folded_apply(case, box[name], x)
        assert relerr(yf, y) <= 1e-14, (n, periodic, p, name, relerr(yf, y))
    twice = max(len(r) - len(set(r)) for r in case.V.dofmap.tolist())
    one_wide = any(c == 1 and per_ for c, per_ in zip(n, periodic))
    assert (twice > 0) == one_wide        # a mesh one cell wide along a periodic axis: a cell names a dof twice


# --------------------------------------------------------------------------- wf_lattice_numbering
def check_numbering(w, V, listed):
    new = w.lattice_numbering(V)
    assert new.dtype == np.int32 and np.array_equal(np.sort(new), np.arange(V.ndofs))
    if not listed.all():      # dofs no cell names keep their relative order behind the others
        u = new[~listed]
        assert u.min() == listed.sum() and np.all(np.diff(u) > 0)
    return new


@pytest.mark.parametrize("p", [1, 2, 4, 6])
def test_lattice_numbering_on_holed_meshes(w, p):
    for name, route in [(m, "subset") for m in nh.MASKS + ("pillar-shuffled",)] + [("pillar", "topological"), ("cavity", "topological")]:
        case = nh.holed_case(name, p, route)
        check_numbering(w, case.V, case.listed)


@pytest.mark.parametrize("p", [1, 2, 4, 6])
def test_lattice_numbering_on_periodic_numberings(w, p):
    for n, periodic in PERIODIC:
        case = nh.periodic_case(n, p, periodic)
        new = check_numbering(w, case.V, np.ones(case.V.ndofs, dtype=bool))
        if min(c for c, per_ in zip(n, periodic) if per_) == 2:
            # two cells along a periodic axis share BOTH faces: no lattice, the first-touch numbering of the cell order
            flat = case.V.dofmap.reshape(-1)
            _, first = np.unique(flat, return_index=True)
            assert np.array_equal(new[flat[np.sort(first)]], np.arange(case.V.ndofs))


# --------------------------------------------------------------------------- wf_ordered_slots
@pytest.mark.parametrize("n,periodic,p", [((1, 3, 3), (True, False, False), 2), ((3, 3, 1), (False, False, True), 4),
                                          ((1, 1, 2), (True, True, False), 3)])
def test_ordered_slots_with_a_dof_twice_in_a_cell(w, n, periodic, p):
    """The repeated dof of a cell gets two slots (four with two periodic axes), in element-local order."""
    case = nh.periodic_case(n, p, periodic)
    dm = case.V.dofmap
    row_off, slot = w.ordered_slots(dm, case.V.ndofs)
    ro, sl = numpy_plan(dm, case.V.ndofs)
    assert np.array_equal(row_off, ro) and np.array_equal(slot, sl)
    mult = 2 ** sum(1 for c, per_ in zip(n, periodic) if per_ and c == 1)
    seen = 0
    for c, row in enumerate(dm):
        for d in np.unique(row):
            at = np.nonzero(row == d)[0]
            if at.size > 1:
                seen += 1
                assert at.size in (2, mult) and np.all(np.diff(slot[c, at]) == 1)     # consecutive, ascending with the local index
                assert row_off[d] <= slot[c, at[0]] and slot[c, at[-1]] < row_off[d + 1]
    assert seen >= case.mesh.ncells * (p + 1) ** 2
