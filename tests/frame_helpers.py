"""The caller's frame of wf_op_create, restated independently of the library (tests/test_frame_host.py,
tests/test_gpu_caller_frame.py).  numpy only, no GPU, no tests in here; nothing is imported from wave_fenics_amd for
the maps (only the mesh builders the other tests already share).

The contract (include/wavehip.h, wf_op_desc): a point (i, j, k) of an m^3 tensor grid, i along x, has

    fast(i, j, k, m) = i + m (j + m k)      the engine's index (x fastest)
    slow(i, j, k, m) = (i m + j) m + k      the caller's index under WF_FLAG_TENSOR_X_SLOWEST

and a caller in the frame (perm, xslow) hands over

    dofmap   dm_elem[c][perm[l']] = dm_tensor'[c][l'],  l' the caller's tensor index of the node, m = P + 1
             (dm_elem = dm_tensor' without perm);
    G, detJ  the point index in the caller's tensor order of the rule's m^3 points (m = nq1 for the dense mass);
             the 3 x 3 of G is untouched: reference axes 0, 1, 2 are x, y, z in both conventions.

x and y are in the global numbering, which no frame touches.  Everything below is written with explicit loops over
(i, j, k) so that it shares no expression with CallerFrame / PointMaps (csrc/op_setup.hip)."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from support import oracle_module as _oracle
from support import relerr  # noqa: F401

FRAMES = ("id", "perm", "xslow", "xslow+perm")
HI = (1.0, 0.37, 2.3)        # the anisotropic box of test_gpu_parity.test_x_slowest_tensor_order
PERTURB = 0.2
# cells of the box per degree: the default cross-section of the dofmap marching kernels (8x8, 7x4, 4x4, 5x2, 3x1, 2x1,
# 2x1) is filled to more than kMinPlanFill = 0.55, so the default route is the plan; two layers
BOX_N = {1: (7, 6, 2), 2: (8, 4, 2), 3: (5, 4, 2), 4: (6, 2, 2), 5: (4, 2, 2), 6: (3, 2, 2), 7: (3, 2, 2)}
MESHES = ("box", "random_orient", "stair")
# spacings of the sheared affine box (3 * 2^-k: every coordinate exact, three different G_c diagonals)
SHEARED_H = (0.375, 0.125, 0.75)
SHEARED_N = (5, 3, 3)


def fast(i, j, k, m):
    return i + m * (j + m * k)


def slow(i, j, k, m):
    return (i * m + j) * m + k


@functools.lru_cache(maxsize=None)
def _caller_index(m: int, xslow: bool):
    """t[engine index] = the caller's index of the same point of an m^3 grid"""
    t = np.empty(m ** 3, dtype=np.int64)
    for k in range(m):
        for j in range(m):
            for i in range(m):
                t[fast(i, j, k, m)] = slow(i, j, k, m) if xslow else fast(i, j, k, m)
    return t


def caller_index(m: int, xslow: bool) -> np.ndarray:
    return _caller_index(int(m), bool(xslow)).copy()


def draw_perm(nd: int, seed: int = 12) -> np.ndarray:
    """A seeded element permutation that is no involution and moves more than half its entries (an involution could
    not tell perm from its inverse)."""
    rng = np.random.default_rng(seed * 1000 + nd)
    ident = np.arange(nd)
    while True:
        pm = rng.permutation(nd)
        if not np.array_equal(pm[pm], ident) and int((pm != ident).sum()) * 2 > nd:
            return pm.astype(np.int32)


def inverse(perm) -> np.ndarray:
    inv = np.empty(len(perm), dtype=np.int32)
    for l in range(len(perm)):
        inv[perm[l]] = l
    return inv


def frame(name: str, p: int):
    """One of FRAMES at degree p: .name, .xslow, .perm (int32 [nd] or None)"""
    assert name in FRAMES
    return SimpleNamespace(name=name, xslow=name.startswith("xslow"), perm=draw_perm((p + 1) ** 3) if name.endswith("perm") else None)


def grid_points(npoints: int) -> int:
    m = int(round(npoints ** (1.0 / 3.0)))
    assert m ** 3 == npoints, npoints
    return m


def caller_points(a, xslow: bool) -> np.ndarray:
    """A per-point array [ncells][m^3][...] in the caller's point order."""
    a = np.asarray(a)
    t = _caller_index(grid_points(a.shape[1]), bool(xslow))
    out = np.empty_like(a)
    for l in range(a.shape[1]):
        out[:, t[l]] = a[:, l]
    return np.ascontiguousarray(out)


def engine_points(a, xslow: bool) -> np.ndarray:
    """What an engine that takes the point order for (xslow) reads from a caller's per-point array."""
    a = np.asarray(a)
    t = _caller_index(grid_points(a.shape[1]), bool(xslow))
    out = np.empty_like(a)
    for l in range(a.shape[1]):
        out[:, l] = a[:, t[l]]
    return np.ascontiguousarray(out)


def caller_dofmap(dm, perm, xslow: bool) -> np.ndarray:
    dm = np.asarray(dm)
    t = _caller_index(grid_points(dm.shape[1]), bool(xslow))
    tensor = np.empty_like(dm)                  # dm_tensor'[c][l']
    for l in range(dm.shape[1]):
        tensor[:, t[l]] = dm[:, l]
    if perm is None:
        return np.ascontiguousarray(tensor)
    elem = np.empty_like(dm)
    for lp in range(dm.shape[1]):
        elem[:, perm[lp]] = tensor[:, lp]
    return np.ascontiguousarray(elem)


def engine_dofmap(dm_elem, perm, xslow: bool) -> np.ndarray:
    """The tensor dofmap (x fastest) an engine that takes the frame for (perm, xslow) derives from a caller's dofmap."""
    dm_elem = np.asarray(dm_elem)
    t = _caller_index(grid_points(dm_elem.shape[1]), bool(xslow))
    tensor = np.empty_like(dm_elem)
    for lp in range(dm_elem.shape[1]):
        tensor[:, lp] = dm_elem[:, perm[lp] if perm is not None else lp]
    out = np.empty_like(dm_elem)
    for l in range(dm_elem.shape[1]):
        out[:, l] = tensor[:, t[l]]
    return np.ascontiguousarray(out)


def effective_perm(perm, xslow: bool, n: int):
    """engine tensor position -> the caller's element-local index (None: the identity): the one permutation both
    conventions fold into"""
    if perm is None and not xslow:
        return None
    out = np.empty(n ** 3, dtype=np.int32)
    for k in range(n):
        for j in range(n):
            for i in range(n):
                lp = slow(i, j, k, n) if xslow else fast(i, j, k, n)
                out[fast(i, j, k, n)] = perm[lp] if perm is not None else lp
    return out


def caller_inputs(canon: dict, perm, xslow: bool) -> dict:
    """canon: canonical (engine-frame) arrays under the keys "dofmap" [ncells][nd], "G" [ncells][nq][3][3], "detJ"
    [ncells][nq] (any subset).  Returns what a caller in the frame (perm, xslow) would hand over, same keys."""
    out = {}
    for key, a in canon.items():
        out[key] = caller_dofmap(a, perm, xslow) if key == "dofmap" else caller_points(a, xslow)
    return out


def engine_view(caller: dict, perm, xslow: bool) -> dict:
    """The inverse of caller_inputs: the canonical arrays an engine reads that takes the frame for (perm, xslow).
    With the frame the arrays were made in it gives the canonical arrays back; with another one, the mis-framed
    arrays a frame error of that kind would compute with."""
    out = {}
    for key, a in caller.items():
        out[key] = engine_dofmap(a, perm, xslow) if key == "dofmap" else engine_points(a, xslow)
    return out


def rows_differing(a, b) -> float:
    """share of the rows (cells) of two arrays that differ somewhere"""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.mean(np.any((a != b).reshape(a.shape[0], -1), axis=1)))


# ---------------------------------------------------------------------------------------------------------------------
# meshes: (mesh, V, oracle mesh) with the canonical dofmap
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def box_of(n, p: int):
    """The anisotropic perturbed box n as a dofmap operator's space."""
    import wave_fenics_amd as w
    o = _oracle()
    om = o.create_box(n, p, hi=HI, perturb=PERTURB)
    mesh = w.BoxMesh(om.n, om.x.copy(), om.geom_dofmap.copy(), (0.0, 0.0, 0.0), HI)
    V = w.FunctionSpace(mesh, p, np.ascontiguousarray(om.dofmap), w.IndexMap(om.ndofs), om.lattice, structured=False)
    return SimpleNamespace(name=f"box{n}", mesh=mesh, V=V, om=om, p=p, reoriented=False)


@functools.lru_cache(maxsize=None)
def mesh_case(name: str, p: int):
    """"box": BOX_N[p] cells of the anisotropic perturbed box; "random_orient": test_gpu_unstructured.build_mesh, every
    cell in one of the 48 orientations; "stair": nonbox_helpers.holed_case, empty plan slots and dofs no cell names;
    "sheared" / "sheared_random": an affine sheared box (per-cell geometry) and its randomly re-oriented version.
    Cached: shared and left unchanged."""
    from wave_fenics_amd import mesh_io
    o = _oracle()
    if name == "box":
        c = box_of(BOX_N[p], p)
        return SimpleNamespace(name=name, mesh=c.mesh, V=c.V, om=c.om, p=p, reoriented=False)
    if name == "random_orient":
        from test_gpu_unstructured import build_mesh, oracle_mesh
        mesh, _ = build_mesh("random_orient", p)
        V = mesh_io.create_functionspace(mesh, p)
        return SimpleNamespace(name=name, mesh=mesh, V=V, om=oracle_mesh(o, mesh, V), p=p, reoriented=True)
    if name == "stair":
        from nonbox_helpers import holed_case
        c = holed_case("stair", p)
        return SimpleNamespace(name=name, mesh=c.mesh, V=c.V, om=c.om, p=p, reoriented=False)
    if name in ("sheared", "sheared_random"):
        from idx_cell_helpers import oracle_mesh, random_orientations
        from owner_helpers import spaces
        from support import lattice_x
        x = lattice_x(*[np.arange(m + 1) * h for m, h in zip(SHEARED_N, SHEARED_H)])
        x[:, 0] += 0.25 * x[:, 1]
        om, V = spaces(o, SHEARED_N, p, x=x)
        if name == "sheared":
            return SimpleNamespace(name=name, mesh=V.mesh, V=V, om=om, p=p, reoriented=False)
        mesh = random_orientations(V.mesh)
        Vr = mesh_io.create_functionspace(mesh, p)
        return SimpleNamespace(name=name, mesh=mesh, V=Vr, om=oracle_mesh(mesh, Vr), p=p, reoriented=True)
    raise ValueError(name)


def coefficient(ncells: int, seed: int = 3) -> np.ndarray:
    """a seeded per-cell coefficient field in [0.5, 2]"""
    return np.random.default_rng(seed).uniform(0.5, 2.0, ncells)


def cell_shuffle(ncells: int, seed: int = 4) -> np.ndarray:
    """a seeded order of the caller's rows that is not the identity anywhere near"""
    rng = np.random.default_rng(seed)
    while True:
        cp = rng.permutation(ncells)
        if int((cp != np.arange(ncells)).sum()) * 2 > ncells:
            return cp


def library_keeps_cell_order(dofmap) -> bool:
    """Whether the batch route's internal cell order (a stable sort of the cells by their smallest dof) is the caller's:
    the `identity_cells` switch of the restaging steps.  The smallest dof of a row does not depend on the frame."""
    key = np.asarray(dofmap).min(axis=1)
    return bool(np.array_equal(np.argsort(key, kind="stable"), np.arange(len(key))))


# ---------------------------------------------------------------------------------------------------------------------
# geometry and references on the canonical mesh
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stiffness_canon(name: str, p: int):
    """the oracle's stiffness operator of a mesh (its .G is the canonical geometry) and |det J| w at the nodes"""
    o = _oracle()
    return o.StiffnessOperator(mesh_case(name, p).om, p)


RULES = ("square", "rect", "collocated")
# the rectangular pair of WF_MASS_SHAPES used per degree: Gauss of degree 2P + 2, nq1 = P + 2
GLL_COLLOCATED_DEGREE = {1: 1, 2: 3, 3: 4, 4: 6, 5: 8, 6: 10, 7: 12}     # Basix' GLL rule with P + 1 points


def rule_of(kind: str, p: int):
    """(variant for the library, variant for the oracle, quad, qdegree, nq1) of a dense-mass table kind"""
    if kind == "square":       # Gauss of degree 2P: P + 1 points, not collocated; equispaced Lagrange
        return "equispaced", "equispaced", "gauss_jacobi", 2 * p, p + 1
    if kind == "rect":         # Gauss of degree 2P + 2: P + 2 points; the 1-D table phi1[P+2][P+1] is not symmetric
        return "equispaced", "equispaced", "gauss_jacobi", 2 * p + 2, p + 2
    if kind == "collocated":   # the GLL rule on the GLL nodes: phi1 = identity
        return "gll_warped", "gll", "gll", GLL_COLLOCATED_DEGREE[p], p + 1
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def mass_canon(name: str, p: int, kind: str):
    """tables and det J w of a dense-mass rule on a mesh: .phi1, .phi, .detJ (signed, as MassOperator computes it from the
    mesh), .variant, .quad, .qdegree, .nq1"""
    o = _oracle()
    variant, ovariant, quad, qd, m = rule_of(kind, p)
    pts, wts, phi1, phi, X, W = o.tabulate_mass_tables(p, ovariant, quad, qd)
    assert phi1.shape == (m, p + 1), (phi1.shape, m, p)
    detJ = o.compute_detJ_generic(mesh_case(name, p).om, X, W)
    return SimpleNamespace(phi1=np.ascontiguousarray(phi1), phi=np.ascontiguousarray(phi), detJ=detJ, variant=variant, quad=quad,
                           qdegree=qd, nq1=m)


@functools.lru_cache(maxsize=None)
def lumped_canon(name: str, p: int):
    return _oracle().MassOperatorCPU(mesh_case(name, p).om, p)


def _vectors(ndofs, seed, apply):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, ndofs)
    ax = np.zeros(ndofs)
    apply(x, ax)
    y0 = rng.uniform(-1, 1, ndofs) * np.abs(ax).max()       # at the scale of A x: an error in A x cannot hide
    yref = y0 + ax
    return SimpleNamespace(x=x, y0=y0, yref=yref, scale=float(np.abs(yref).max()), ax=ax)


@functools.lru_cache(maxsize=None)
def stiffness_reference(name: str, p: int, coeff: bool = False):
    """x, y0 and y_ref = y0 + K x of the oracle on the canonical mesh; coeff: with coefficient() folded into G, as
    medium_helpers does.  Cached: computed once, shared, left unchanged."""
    o = _oracle()
    case, K = mesh_case(name, p), stiffness_canon(name, p)
    if not coeff:
        return _vectors(case.om.ndofs, 100 + p, K)
    Ga = np.ascontiguousarray(K.G * coefficient(case.om.ncells)[:, None, None, None])
    return _vectors(case.om.ndofs, 100 + p, lambda x, y: o.stiffness_apply_sumfact(case.om, Ga, K.c0, x, y))


@functools.lru_cache(maxsize=None)
def lumped_reference(name: str, p: int):
    return _vectors(mesh_case(name, p).om.ndofs, 200 + p, lumped_canon(name, p))


@functools.lru_cache(maxsize=None)
def mass_reference(name: str, p: int, kind: str, coeff: bool = False):
    o = _oracle()
    case, t = mesh_case(name, p), mass_canon(name, p, kind)
    detJ = t.detJ if not coeff else np.ascontiguousarray(t.detJ * coefficient(case.om.ncells)[:, None])
    return _vectors(case.om.ndofs, 300 + p, lambda x, y: o.dense_mass_apply(case.om, t.phi, detJ, x, y))


# ---------------------------------------------------------------------------------------------------------------------
# what a frame error would compute (the oracle on mis-framed arrays)
# ---------------------------------------------------------------------------------------------------------------------
def misframed_stiffness(p: int, dofmap, G, x, c0: float = 1500.0) -> np.ndarray:
    o = _oracle()
    dm = np.ascontiguousarray(dofmap, dtype=np.int32)
    y = np.zeros(len(x))
    o.stiffness_apply_sumfact(SimpleNamespace(p=p, dofmap=dm, ncells=dm.shape[0]), np.ascontiguousarray(G), c0, x, y)
    return y


def misframed_dense_mass(dofmap, phi, detJ, x) -> np.ndarray:
    o = _oracle()
    dm = np.ascontiguousarray(dofmap, dtype=np.int32)
    y = np.zeros(len(x))
    o.dense_mass_apply(SimpleNamespace(ncells=dm.shape[0], dofmap=dm), phi, np.ascontiguousarray(detJ), x, y)
    return y


def misframed_lumped_mass(dofmap, detJ, x) -> np.ndarray:
    dm = np.asarray(dofmap)
    y = np.zeros(len(x))
    np.add.at(y, dm.reshape(-1), (np.asarray(detJ) * x[dm]).reshape(-1))
    return y
