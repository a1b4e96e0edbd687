"""Shared cases and references of the cell-coefficient tests (tests/test_medium_host.py, tests/test_gpu_medium_*.py).
No GPU in here.

An operator created with cell_coeff = a applies y += sum_c a_c P_c^T A_c P_c x.  The reference is the oracle fed with
scaled geometry: G * a[:, None, None, None] into the sum-factorised (or dense) stiffness apply, detJ * a[:, None] into
the lumped and dense mass applies.  The bound is TOL = 1e-12 of max|y_ref| (every parity test of the project), TOL_FORM
= 1e-13 between two forms of one sum; test_medium_host.py shows that the oracle's own two forms agree to TOL / 10 on
every case and field here.

Coefficient fields (contrast within 1:8, what 1 / (rho c^2) spans from water to bone):
  distinct   a_c = 0.5 + frac(phi c) 3.5, phi the golden ratio: all cells differ, so a permuted array shows
  slab       1 in the cells whose centroid lies below a plane x = const, 8 above.  The plane is below the
             int(0.43 m)-th of the m distinct centroid abscissae: cell 3 of 9, 2 of 6, 2 of 5, 1 of 4, 1 of 3 on the boxes
             here, never a multiple of a block or column width in x (8, 5, 4, 3, 2); being normal to x it crosses every z
             segment
  zeros      `distinct` with every third cell 0
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import idx_cell_helpers as ich
import nonbox_helpers as nh
from support import bits, relerr  # noqa: F401

TOL = 1e-12
TOL_FORM = 1e-13
C0 = 1500.0
GOLDEN = (1.0 + 5.0 ** 0.5) / 2.0
FIELDS = ("distinct", "slab", "zeros")


def dof_match(coords_a, coords_b):
    """b_of_a with coords_b[b_of_a[i]] == coords_a[i] (to 1e-11 of the extent): two numberings of one set of dofs"""
    ca, cb = np.asarray(coords_a), np.asarray(coords_b)
    assert ca.shape == cb.shape
    ext = np.abs(ca).max()
    key = lambda c: np.lexsort(np.round(c / ext, 9).T)
    ia, ib = key(ca), key(cb)
    b_of_a = np.empty(ca.shape[0], dtype=np.int64)
    b_of_a[ia] = ib
    assert np.abs(cb[b_of_a] - ca).max() <= 1e-11 * ext
    return b_of_a


def centroids(x, geom_dofmap):
    return np.asarray(x)[np.asarray(geom_dofmap)].mean(axis=1)


def field(name: str, x, geom_dofmap, cut_fraction: float = 0.43):
    """The coefficient field `name` on the cells geom_dofmap (any cell type)."""
    nc = np.asarray(geom_dofmap).shape[0]
    distinct = 0.5 + np.modf(GOLDEN * np.arange(nc))[0] * 3.5
    if name == "distinct":
        return distinct
    if name == "zeros":
        a = distinct.copy()
        a[::3] = 0.0
        return a
    if name == "slab":
        xc = centroids(x, geom_dofmap)[:, 0]
        xs = np.unique(np.round(xc, 9))
        return np.where(xc < xs[int(cut_fraction * len(xs))] - 1e-9, 1.0, 8.0)
    raise ValueError(name)


# ---------------------------------------------------------------------------------------------------------------------
# hexahedral cases: name -> (mesh builder, degree, structured, tuning, flags / extras, the path the case means to reach)
# ---------------------------------------------------------------------------------------------------------------------
def _box(kind, n):
    return ich.box_with(n, perturb=0.2) if kind == "perturbed" else ich.base_box(kind, n)


# (kernel, geometry, metric, update) as the operator properties name them
OWNER = ("march_box", "per_cell", "axes", "owner")
POINT = ("march_box", "per_point", "none", "none")
STIFFNESS_BOX = {
    # the owner form: P4 default on (9, 3, 7) -- two owner columns in x (8 cells each, the second partial), a partial
    # column in y, geometry blocked 5 x 2 with partial blocks, uneven z segments; P2, P5, P6, P7 on request with two
    # columns along an axis and nz >= 4 (cross-sections 8x8, 5x2, 2x3, 2x2)
    "owner-P4": ("graded", (9, 3, 7), 4, {}, OWNER),
    "owner-P4-lz3": ("graded", (9, 3, 7), 4, {"lz": 3}, OWNER),
    "owner-P4-wide": ("graded", (9, 9, 7), 4, {}, OWNER),   # 2 x 5 owner columns: wf_op_replan_runs(8) plans 16 runs
    "owner-P2": ("graded", (9, 2, 4), 2, {"update": "owner"}, OWNER),
    "owner-P5": ("graded", (6, 3, 4), 5, {"update": "owner"}, OWNER),
    "owner-P6": ("graded", (3, 4, 4), 6, {"update": "owner"}, OWNER),
    "owner-P7": ("graded", (3, 3, 4), 7, {"update": "owner"}, OWNER),
    "point-P2": ("perturbed", (6, 6, 3), 2, {}, POINT),
    "point-P4": ("perturbed", (6, 3, 3), 4, {}, POINT),
    "cell-full-P3": ("sheared", (5, 5, 3), 3, {}, ("march_box", "per_cell", "full", "none")),
    "axes-atomic-P1": ("graded", (9, 9, 3), 1, {}, ("march_box", "per_cell", "axes", "atomic")),
    "axes-atomic-P3": ("graded", (5, 5, 3), 3, {}, ("march_box", "per_cell", "axes", "atomic")),
    "box-block-P2": ("perturbed", (4, 4, 4), 2, {"kernel": "box_block"}, ("box_block", "per_point", "none", "none")),
    "ksplit-P5": ("perturbed", (4, 2, 3), 5, {}, POINT),
    "ksplit-P6": ("perturbed", (3, 2, 3), 6, {}, POINT),
}


@functools.lru_cache(maxsize=None)
def box_case(name: str):
    """A box stiffness case: mesh, space, the oracle's mesh, the unscaled oracle geometry.  Cached, shared, unchanged."""
    import wave_fenics_amd as w
    from oracle import wave_oracle as o
    kind, n, p, tuning, want = STIFFNESS_BOX[name]
    mesh = _box(kind, n)
    V = w.create_functionspace(mesh, p)
    om = o.BoxMesh(tuple(n), p, mesh.x, mesh.geom_dofmap, V.dofmap, V.ndofs, V.lattice)
    return SimpleNamespace(name=name, mesh=mesh, V=V, om=om, p=p, structured=True, tuning=dict(tuning), want=want, flags=0,
                           given_G=False)


MARCH_POINT = ("march_idx", "per_point", "none", "none")
BATCH = ("batch_unique", "per_point", "none", "none")
STIFFNESS_DOFMAP = {
    # randomly re-oriented cells (48 orientations): the multiply follows the cell into its slot of the lattice plan
    "reoriented-point-P2": ("affine", "graded-random", 2, {"kernel": "march"}, MARCH_POINT),
    "reoriented-point-P4": ("affine", "graded-random", 4, {"kernel": "march"}, MARCH_POINT),
    "reoriented-full-P3": ("affine", "sheared-random", 3, {"geometry": "per_cell"}, ("march_idx", "per_cell", "full", "none")),
    "reoriented-axes-P3": ("affine", "graded-random", 3, {"geometry": "per_cell"}, ("march_idx", "per_cell", "axes", "atomic")),
    "holed-P2": ("holed", "cavity", 2, {"kernel": "march"}, MARCH_POINT),
    "periodic-P2": ("periodic", (4, 3, 3), 2, {"kernel": "march"}, MARCH_POINT),
    "unstructured-P5": ("box", (4, 2, 3), 5, {"kernel": "march"}, MARCH_POINT),
    # the batch kernels on more than one batch (28 cells per batch at P2), internal cell order sorted and kept
    "batch-P2": ("holed", "pillar-shuffled", 2, {"kernel": "batch"}, BATCH),
    "batch-keep-P2": ("holed", "pillar-shuffled", 2, {"kernel": "batch", "keep_cell_order": True}, BATCH),
    "elementwise-P2": ("holed", "pillar-shuffled", 2, {"kernel": "elementwise"}, ("elementwise", "per_point", "none", "none")),
    # the caller's own h_G, scaled the same way: on the plan and on the batches
    "given-G-march-P2": ("affine", "graded-random", 2, {"kernel": "march"}, MARCH_POINT),
    "given-G-batch-P2": ("holed", "pillar-shuffled", 2, {"kernel": "batch"}, BATCH),
}


@functools.lru_cache(maxsize=None)
def dofmap_case(name: str):
    import wave_fenics_amd as w
    source, what, p, tuning, want = STIFFNESS_DOFMAP[name]
    if source == "affine":
        mesh, V = ich.affine_mesh(what), ich.space(what, p)
        om = ich.oracle_mesh(mesh, V)
    elif source == "holed":
        case = nh.holed_case(what, p, "subset")
        mesh, V, om = case.mesh, case.V, case.om
    elif source == "periodic":
        case = nh.periodic_case(what, p, (True, False, False))
        mesh, V, om = case.mesh, case.V, case.om
    else:
        mesh = ich.box_with(what, perturb=0.2)
        Vb = w.create_functionspace(mesh, p)
        V = w.FunctionSpace(mesh, p, Vb.dofmap, Vb.index_map, Vb.lattice, structured=False)
        om = ich.oracle_mesh(mesh, V)
    return SimpleNamespace(name=name, mesh=mesh, V=V, om=om, p=p, structured=False, tuning=dict(tuning), want=want, flags=0,
                           given_G=name.startswith("given-G"))


def stiffness_case(name: str):
    return box_case(name) if name in STIFFNESS_BOX else dofmap_case(name)


STIFFNESS_CASES = tuple(STIFFNESS_BOX) + tuple(STIFFNESS_DOFMAP)


@functools.lru_cache(maxsize=None)
def oracle_geometry(name: str):
    """(G, detJ) of the oracle on a stiffness case's mesh, without a coefficient.  Cached, shared, unchanged."""
    from oracle import wave_oracle as o
    case = stiffness_case(name)
    return o.precompute_geometric_data(case.om, case.p)


def vectors(ndofs: int, seed: int = 1234):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, ndofs), rng.uniform(-1, 1, ndofs)


def stiffness_reference(case, a, x, c0=C0, dense=False):
    """K[a] x by the oracle with G * a: sum-factorised, or through the dense tables (the second form)."""
    from oracle import wave_oracle as o
    G, _ = oracle_geometry(case.name)
    Ga = np.ascontiguousarray(G * np.asarray(a)[:, None, None, None])
    y = np.zeros(case.om.ndofs)
    if dense:
        K = o.StiffnessOperator(case.om, case.p, {"c0": c0})
        K.G = Ga
        K(x, y)
    else:
        o.stiffness_apply_sumfact(case.om, Ga, c0, x, y)
    return y


def make_stiffness(case, a, **extra):
    """The operator of a case with cell_coeff = a (None: without)."""
    import wave_fenics_amd as w
    G = oracle_geometry(case.name)[0] if case.given_G else None
    return w.StiffnessOperator(case.V, case.p, {"c0": extra.pop("c0", C0)}, G=G, structured=case.structured,
                               flags=extra.pop("flags", case.flags), tuning=extra.pop("tuning", case.tuning), cell_coeff=a)


def path_of(op):
    return (op.kernel, op.geometry, op.metric, op.update)


def selection_of(op):
    """Everything the coefficient must not enter: the path, the plan fields and alg_bytes."""
    i = op.info
    return path_of(op) + (i.plan_items, i.plan_patterns, i.plan_lz, i.plan_reoriented, i.plan_fill, i.alg_bytes, i.structured)


# ---------------------------------------------------------------------------------------------------------------------
# mass references
# ---------------------------------------------------------------------------------------------------------------------
def lumped_reference(om, p, a, x, dense=False):
    """M[a] x of the lumped mass: oracle_mass_apply with detJ * a, or the dense mass apply with the collocated table."""
    from oracle import wave_oracle as o
    M = o.MassOperatorCPU(om, p)
    detJ = np.ascontiguousarray(M.detJ * np.asarray(a)[:, None])
    y = np.zeros(om.ndofs)
    if dense:
        o.dense_mass_apply(om, M.phi, detJ, x, y)
    else:
        M.detJ = detJ
        M(x, y)
    return y


def dense_mass_reference(om, p, qdegree, a, x):
    """Phi^T diag(detJ w a_c) Phi x at the Gauss rule of degree qdegree, equispaced Lagrange (det J signed, as
    MassOperator computes it from the mesh)."""
    from oracle import wave_oracle as o
    _, phi, X, W = nh.dense_tables(p, qdegree)
    detJ = np.ascontiguousarray(o.compute_detJ_generic(om, X, W) * np.asarray(a)[:, None])
    y = np.zeros(om.ndofs)
    o.dense_mass_apply(om, phi, detJ, x, y)
    return y


def cell_volumes(om, p):
    """sum_q |det J| w_q per cell"""
    from oracle import wave_oracle as o
    return o.precompute_geometric_data(om, p)[1].sum(axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# tetrahedra
# ---------------------------------------------------------------------------------------------------------------------
def tet_unclamped_G(top):
    """G of a tet_oracle.TetStiffnessOperator before the -1/0/1 clamp (the operator of WF_FLAG_NO_CLAMP)."""
    m = top.mesh
    xc = m.x[m.geom_dofmap]
    J = np.stack([xc[:, 1] - xc[:, 0], xc[:, 2] - xc[:, 0], xc[:, 3] - xc[:, 0]], axis=2)
    Ji = np.linalg.inv(J)
    detJ = np.abs(np.linalg.det(J))[:, None] * top.W[None, :]
    return np.einsum("cik,cq,cjk->cqij", Ji, detJ, Ji)


def tet_meshes(n, p, perturb=0.2, scale=1.0):
    """(TetSpace of the package, TetMesh of the oracle) of one Kuhn box, vertices times `scale`."""
    from oracle import tet_oracle as to
    from wave_fenics_amd import tet
    V = tet.create_kuhn_box(n, p, perturb=perturb)
    om = to.create_kuhn_box(n, p, perturb=perturb)
    assert np.array_equal(V.dofmap, om.dofmap) and np.array_equal(V.x, om.x)
    if scale != 1.0:
        V.x = np.ascontiguousarray(V.x * scale)
        om.x = np.ascontiguousarray(om.x * scale)
    return V, om


def tet_clamp_scale(n, p):
    """The scale of the unperturbed Kuhn box that puts its largest product w_q C_e at 1 + 3e-6: inside the clamp's
    window at 1 (half width 1e-5), where the clamp changes the operator by 3e-6 -- far above the bound.  C is linear in
    the scale."""
    from oracle import tet_oracle as to
    om = to.create_kuhn_box(n, p, perturb=0.0)
    top = to.TetStiffnessOperator(om, p)
    return (1.0 + 3e-6) / np.abs(tet_unclamped_G(top)).max()


def tet_stiffness_reference(top, a, x, clamp=True):
    from oracle import wave_oracle as o
    G = top.G if clamp else tet_unclamped_G(top)
    keep = top.G
    top.G = np.ascontiguousarray(G * np.asarray(a)[:, None, None, None])
    y = np.zeros(top.mesh.ndofs)
    try:
        top(x, y)
    finally:
        top.G = keep
    return y


def tet_mass_reference(V, p, a, x, use_fabs=True):
    """The dense mass apply of the oracle on the tetrahedral tables, det J w a_c per cell and point."""
    from oracle import wave_oracle as o
    from wave_fenics_amd import tet
    X, W = tet.tet_quadrature((2 * p + 2) // 2)
    phi, _ = tet.tabulate_tet(p, X)
    xc = V.x[V.geom_dofmap]
    J = np.stack([xc[:, 1] - xc[:, 0], xc[:, 2] - xc[:, 0], xc[:, 3] - xc[:, 0]], axis=2)
    det = np.linalg.det(J)
    s = (np.abs(det) if use_fabs else det) * np.asarray(a)
    detJ = np.ascontiguousarray(s[:, None] * W[None, :])
    y = np.zeros(V.ndofs)
    om = SimpleNamespace(ncells=V.ncells, dofmap=np.ascontiguousarray(V.dofmap, dtype=np.int32))
    o.dense_mass_apply(om, np.ascontiguousarray(phi), detJ, x, y)
    return y
