"""Shared builders and references for the arbitrary-dofmap operators on meshes that are NOT a union of full boxes
with a one-to-one dof numbering (tests/test_nonbox_host.py, tests/test_gpu_nonbox.py).  No GPU in here.

  * holed_box: a perturbed box with cells deleted -- tile positions of the lattice-column plan
    (csrc/march_plan.cpp) that no cell covers, away from the end of the mesh.  Two numberings: "subset" keeps
    the box space's dof numbers (the dofs inside the hole stay in the vectors, named by no cell), "topological"
    numbers the remaining mesh afresh (csrc/function_space.cpp).
  * periodic_box: the box space with the dofs of opposite faces identified (oracle.make_periodic): one dof at
    two places of a tile, a dof twice in one cell when the mesh is one cell wide.
  * references: the oracle on the cell subset; for periodic numberings the FOLDED box oracle
    y_per = fold(A_box x_per[l2g]), which never passes through a periodic dofmap.
  * has_cell_above_gap / first_layer_empty: what the deleted cells do to the z segments of the plan's work
    items, from the cell coordinates alone."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from support import oracle_module as _oracle

HOLED_BOX = (6, 5, 7)           # 210 cells: the largest mesh of these tests
# cross-section (BX, BY) of the plan's columns per degree, the defaults: the first entry of a degree in WF_IDX_SHAPES
# (csrc/stiffness_march_idx.hip, P <= 4), WF_KS_SHAPES (csrc/stiffness_march_ks.hip, P >= 5) and WF_MASS_SHAPES
# (csrc/mass_march.hip).  wf_op_info_t does not report the cross-section, so these are copies: a retune of a default
# there changes them here (test_gpu_nonbox.check_fill compares wf_op_info_t.plan_fill with expected_fill below).
STIFFNESS_BLOCK = {1: (8, 8), 2: (7, 4), 3: (4, 4), 4: (5, 2), 5: (3, 1), 6: (2, 1), 7: (2, 1)}
MASS_BLOCK = {1: (8, 8), 2: (7, 4), 3: (4, 4), 4: (4, 2), 5: (2, 2), 6: (2, 2), 7: (2, 1)}
MASKS = ("L", "cavity", "stair", "pillar")
PERTURB = 0.2


def ORDERED():
    from wave_fenics_amd._lib import WF_FLAG_ORDERED
    return WF_FLAG_ORDERED


def cell_coords(n) -> np.ndarray:
    """(cx, cy, cz) of every cell of the box in its cell order (x fastest): int array [ncells][3]."""
    nx, ny, nz = n
    cz, cy, cx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([cx.reshape(-1), cy.reshape(-1), cz.reshape(-1)], axis=1)


def keep_mask(name: str, n=HOLED_BOX) -> np.ndarray:
    """The cells that stay.  L: a re-entrant corner (columns that end early, no gap inside one); cavity: an
    inclusion; stair: every column starts one layer later than its x neighbour; pillar: two layers deleted except
    for one row of cells, so that the mesh stays connected and every other column has a two-layer gap."""
    cx, cy, cz = cell_coords(n).T
    if name == "L":
        return ~((cx >= 3) & (cz >= 3))
    if name == "cavity":
        return ~((cx >= 2) & (cx <= 3) & (cy == 2) & (cz >= 2) & (cz <= 4))
    if name == "stair":
        return cz >= cx
    if name == "pillar":
        return ~(((cz == 2) | (cz == 3)) & (cx != 0))
    raise ValueError(name)


def _stacks(coords):
    """cell coordinates -> {(cx, cy): sorted cz of the cells present}, cz counted from the lowest cell of the mesh
    (the plan counts from the lowest cell of a lattice component; these meshes are one component)."""
    c = np.asarray(coords, dtype=np.int64)
    z0 = int(c[:, 2].min())
    out = {}
    for cx, cy, cz in c:
        out.setdefault((int(cx), int(cy)), []).append(int(cz) - z0)
    return {k: sorted(v) for k, v in out.items()}


def has_cell_above_gap(coords, lz: int) -> bool:
    """Is there a cell with an ABSENT slot below it in its own z segment of lz layers?  Then the work item holding
    the two has a present layer above a missing slot, whatever the cross-section of the columns: the item's layer
    count is the index of the last present layer + 1, not the number of present layers."""
    for zs in _stacks(coords).values():
        have = set(zs)
        for z in zs:
            if any(b not in have for b in range((z // lz) * lz, z)):
                return True
    return False


def first_layer_empty(coords, lz: int, block=(1, 1)) -> bool:
    """Is there a z segment that holds cells but none in its first layer?  block = (1, 1): per stack of cells
    (necessary for every cross-section); block = (BX, BY): per column of BX x BY stacks -- the work items of a plan
    with that cross-section, whose first layers are then empty as a whole."""
    bx, by = block
    x0 = min(k[0] for k in _stacks(coords))
    y0 = min(k[1] for k in _stacks(coords))
    segs = {}
    for (cx, cy), zs in _stacks(coords).items():
        for z in zs:
            segs.setdefault(((cx - x0) // bx, (cy - y0) // by, z // lz), set()).add(z % lz)
    return any(0 not in layers for layers in segs.values())


def expected_fill(coords, lz: int, block) -> float:
    """Cells per cell slot of the plan's work items (wf_op_info_t.plan_fill): items are the (column of BX x BY
    stacks, z segment of lz layers) pairs that hold a cell, each with BX BY lz slots.  1.0 when the deleted cells are
    whole items -- the cavity at a 2 x 1 cross-section with one layer per item.  Columns and segments are counted
    from the smallest cell coordinate per axis, as the plan does from the lowest cell of a lattice component: for
    meshes of one component whose cells agree on their axes (every holed mesh here)."""
    bx, by = block
    c = np.asarray(coords, dtype=np.int64)
    c = c - c.min(axis=0)
    items = {(int(x) // bx, int(y) // by, int(z) // lz) for x, y, z in c}
    return len(c) / (len(items) * bx * by * lz)


def oracle_mesh(mesh, V, cells=None):
    """The oracle's mesh of a (mesh, space) pair, as test_gpu_unstructured.oracle_mesh, or of the listed cells of it
    (same dof numbering)."""
    o = _oracle()
    gd, dm = np.ascontiguousarray(mesh.geom_dofmap), np.ascontiguousarray(V.dofmap)
    if cells is not None:
        gd, dm = np.ascontiguousarray(gd[cells]), np.ascontiguousarray(dm[cells])
    return o.BoxMesh(None, V.degree, np.ascontiguousarray(mesh.x), gd, dm, V.ndofs, None)


def holed_box(n, p: int, keep, route: str, shuffle: int | None = None):
    """The box n (perturbed vertices) reduced to the cells keep[ncells].  route "subset": the box space's dofmap
    rows of those cells and the box's ndofs; "topological": mesh_io.create_functionspace of the remaining cells
    (compact numbering).  shuffle = seed: the cell list permuted and the dofs renumbered at random.
    Returns a namespace: mesh, V, om (the oracle's mesh of the same cells), coords [ncells][3] in the cell order
    of V, listed[ndofs] (the dofs some cell names)."""
    import wave_fenics_amd as w
    from wave_fenics_amd import mesh_io
    keep = np.asarray(keep, dtype=bool)
    box = w.create_box(n, perturb=PERTURB)
    assert keep.shape == (box.ncells,)
    coords = cell_coords(n)[keep]
    mesh = w.BoxMesh(tuple(n), box.x, np.ascontiguousarray(box.geom_dofmap[keep]), box.lo, box.hi)
    if route == "subset":
        Vb = w.create_functionspace(box, p)
        V = w.FunctionSpace(mesh, p, np.ascontiguousarray(Vb.dofmap[keep]), w.IndexMap(Vb.ndofs), None, structured=False)
    elif route == "topological":
        V = mesh_io.create_functionspace(mesh, p)
    else:
        raise ValueError(route)
    if shuffle is not None:
        rng = np.random.default_rng(shuffle)
        cperm = rng.permutation(mesh.ncells)
        new = rng.permutation(V.ndofs).astype(np.int32)
        coords = coords[cperm]
        mesh = w.BoxMesh(tuple(n), box.x, np.ascontiguousarray(mesh.geom_dofmap[cperm]), box.lo, box.hi)
        V = w.FunctionSpace(mesh, p, np.ascontiguousarray(new[V.dofmap[cperm]]), w.IndexMap(V.ndofs), None, structured=False)
    listed = np.zeros(V.ndofs, dtype=bool)
    listed[V.dofmap.reshape(-1)] = True
    return SimpleNamespace(mesh=mesh, V=V, om=oracle_mesh(mesh, V), coords=coords, listed=listed)


@functools.lru_cache(maxsize=None)
def holed_case(name: str, p: int, route: str = "subset"):
    """holed_box of a named mask of HOLED_BOX; "pillar-shuffled" is the pillar with shuffle = 15.  Cached: the tests
    share the meshes (and the references they hang on them) and leave them unchanged."""
    if name.endswith("-shuffled"):
        return holed_box(HOLED_BOX, p, keep_mask(name[: -len("-shuffled")]), route, shuffle=15)
    return holed_box(HOLED_BOX, p, keep_mask(name), route)


def periodic_box(n, p: int, periodic):
    """The box space with new[dofmap] of oracle.make_periodic; the geometry stays the non-periodic mesh's.
    Returns a namespace: mesh, V (nred dofs), l2g[box ndofs] (box dof -> periodic dof), ob (the oracle's
    NON-periodic box, for the folded reference), om (the oracle's mesh on the periodic dofmap)."""
    import wave_fenics_amd as w
    o = _oracle()
    mesh = w.create_box(n, perturb=PERTURB)
    Vb = w.create_functionspace(mesh, p)
    ob = o.create_box(n, p, perturb=PERTURB)
    om = o.create_box(n, p, perturb=PERTURB)
    l2g = o.make_periodic(om, periodic)
    assert np.array_equal(ob.dofmap, Vb.dofmap) and np.array_equal(ob.x, mesh.x)
    dm = np.ascontiguousarray(l2g[Vb.dofmap].astype(np.int32))
    assert np.array_equal(dm, om.dofmap)
    V = w.FunctionSpace(mesh, p, dm, w.IndexMap(int(om.ndofs)), None, structured=False)
    return SimpleNamespace(mesh=mesh, V=V, l2g=l2g, ob=ob, om=om)


@functools.lru_cache(maxsize=None)
def periodic_case(n, p: int, periodic):
    return periodic_box(n, p, periodic)


def fold(l2g, y_box, nred: int) -> np.ndarray:
    """Sum of the box entries that are one periodic dof."""
    y = np.zeros(nred)
    np.add.at(y, l2g, y_box)
    return y


def folded_apply(case, apply_box, x_per) -> np.ndarray:
    """fold(A_box x_per[l2g]); apply_box(x, y) does y += A_box x on the non-periodic box."""
    yb = np.zeros(case.ob.ndofs)
    apply_box(np.ascontiguousarray(x_per[case.l2g]), yb)
    return fold(case.l2g, yb, case.V.ndofs)


def dense_tables(p: int, qdegree: int, variant: str = "equispaced"):
    """Gauss rule of degree qdegree for the dense mass: (phi1, phi, X, W) of oracle.tabulate_mass_tables."""
    _, _, phi1, phi, X, W = _oracle().tabulate_mass_tables(p, variant, "gauss_jacobi", qdegree)
    return phi1, phi, X, W


def reference_operators(om, p: int, qdegrees=()):
    """{"stiffness", "lumped", ("dense", qd)...}: functions (x, y) -> y += A x of the oracle on the mesh om."""
    o = _oracle()
    K, M = o.StiffnessOperator(om, p), o.MassOperatorCPU(om, p)
    ops = {"stiffness": K, "lumped": M}
    for qd in qdegrees:
        _, phi, X, W = dense_tables(p, qd)
        detJ = o.compute_detJ_generic(om, X, W)
        ops[("dense", qd)] = (lambda phi, detJ: lambda x, y: o.dense_mass_apply(om, phi, detJ, x, y))(phi, detJ)
    ops["G"] = K.G
    return ops
