"""Reference, bound and meshes of the hexahedral geometry tests (tests/test_hex_geometry_host.py,
tests/test_gpu_hex_geometry.py).  No GPU in here, and neither oracle/ nor the library computes any reference value.

The set-up code writes G = J^-1 J^-T |det J| w and det J w per cell and point through hex_point_geometry
(csrc/hex_geometry.hip; common/precomputation.hpp:49-107) and, for affine cells, through the host rule cell_geometry
(csrc/hex_cell_geometry.cpp).  point_geometry_ld restates the per-point formula in numpy long double, operation by
operation in the order the kernel evaluates it:

    f_d = (1 - X_d, X_d);   dphi_v = (g_a f1_b f2_c, f0_a g_b f2_c, f0_a f1_b g_c), g = (-1, 1), v = a + 2 b + 4 c
    [clamp of dphi]
    J[i][d] = sum_v x_v[i] dphi_v[d]   (v = 0 .. 7 in turn);   det J by the first row;   idet = 1 / det J
    d = (|det J| or det J) * ((w_i w_j) w_k);   J^-1 = adjugate * idet;   G[a][b] = sum_k (J^-1[a][k] d) J^-1[b][k]
    [clamp of G]

The bound.  Every quantity is carried as a pair (value, e) with e >= |float64 evaluation - value| to first order
(running error analysis): inputs (vertex coordinates, points, weights: float64 numbers) have e = 0, and
    a +- b: e = e_a + e_b + u |a +- b|,   a b: e = |a| e_b + |b| e_a + u |a b|,   1 / a: e = e_a / a^2 + u / |a|,
    |a|: e = e_a,   a clamped value: e = 0,
u = 2^-53.  The absolute values carry the cancellation of sum_v x_v dphi_v into every later quantity: a cell at
offset 2^12 gets a bound 2^12 times that of the same cell at the origin.  The bound returned is 2 e: the factor 2
covers (i) the second-order terms -- the first-order relative errors here stay below 1e-9, so they are below 1e-9 of
e -- and (ii) the compiler's freedom to contract a b + c into one fma, which replaces two roundings counted above
(u |a b| and u |a b + c|) by one (u |a b + c|): the contracted result differs from the exact one by no more than the
uncontracted count allows, and differs from the uncontracted float64 result by at most that count again, hence 2.  It
is derived, not measured; test_hex_geometry_host.py shows plain float64 numpy stays within half of it.

The clamp maps |v| <= 1e-8 to 0 and |v -+ 1| <= 1e-5 + 1e-8 to +-1.  Three things describe what it did:
  mask    entries inside a window whose distance to the window's constant exceeds their bound 2 e: the clamp CHANGED
          them (G_mask per entry of G, d_mask per entry of dphi);
  near    entries inside a window that equal the constant up to their bound (the rounding residue of an off-diagonal
          of a rectilinear cell, a dphi that is exactly 0 or +-1): the clamp makes them the constant exactly, the
          reference holds the constant with bound 0, and they count neither as changed nor as unchanged;
  margin  over every value a clamp comparison sees, the smallest | |v - b| - T_b | / T_b, b in (-1, 0, 1), T the
          window's half width: the distance to the nearest window edge in units of the window.  With margin >= 1e-3
          (1e-11 in absolute terms, far above any bound here) float64 and long double agree on the side of every edge.
  margin_value  the same distance relative to the edge as a value of v, |v - E| / |E| for E = +-1e-8, +-(1 -+ T): the
          measure the host rule's slack uses (it refuses a cell when a G_c w_i w_j w_k lies within 1e-6, relative, of
          a window).  The two agree at the zero window; at +-1 margin_value = margin * T.

Meshes (mesh_case).  Entry-wise tests run on N_ENTRY = (3, 2, 2) cells: 12 cells leave a partial last batch at every
degree (CB = 256 // (P+1)^2 = 64, 28, 16, 10, 7, 5, 4) and a partial last workgroup of the geometry launch (12 (P+1)^3
points, 256 per workgroup) at every degree but P3 and P7: at P3 (64 points per cell) N_P3_PARTIAL = (3, 3, 2) adds one,
at P7 (512 points per cell) every launch is whole workgroups.  Operator tests run on (BX + 1, BY + 1, 3) of the
kernel's cross-section (operator_n).
  perturbed      unit box, interior vertices moved by 0.2 h.  mask 0 up to P3; from P4 on off-diagonal entries at
                 the points of the smallest weights fall below 1e-8: 48, 210, 614, 1122 entries of the (3, 2, 2) mesh
                 at P4 .. P7 (the same count on mirrored and half_mirrored, which are this mesh in other frames)
  sheared        0.125 lattice, x += 0.25 y                                           mask 0
  anisotropic    spacings 3, 3/32, 96                                                 mask 0
  far            unit cells at offset 2^12 on every axis                              mask 0
  mirrored       perturbed with x -> 1 - x: det J < 0 everywhere                      mask as perturbed
  half_mirrored  perturbed, the cells of the upper half in z with their local x reversed (vertex relabelling,
                 orientation code 1): det J < 0 there.  Not a box: operators take it as a dofmap   mask as perturbed
  tiny           uniform, h the power of two nearest 1e-8 / sqrt(W_a W_b), W_a < W_b the two smallest distinct
                 w_i w_j w_k: the 8 corner points' 3 diagonal entries fall below 1e-8, nothing else does
                 (P2..P7: h = 2^-20, 2^-17, 2^-15, 2^-13, 2^-12, 2^-10; the two
                 values nearest 1e-8 lie a factor 0.32 to 3.3 from it).  P1: spacings (h, h, 4 h), h W = 2e-8:
                 G22 = h W / 4 is clamped at all 8 points, G00 = G11 = 4 h W are not.
                 mask per cell: P1 8, P2..P7 24
  unit_above /   uniform, h = (1 +- 4e-6) / W_m, W_m the upper median of the distinct w_i w_j w_k: the diagonal
  unit_below     entries of the points of that weight become exactly 1.
                 mask per cell = 3 * (points of weight W_m): P1 24, P2 18, P3 72, P4 18, P5 72, P6 24, P7 24
  unit_negative  unit_above with x -> -x, for use without |det J| (WF_FLAG_NO_FABS): the same entries become -1
  rule           the caller rule RULE_POINTS on `perturbed` (wf_geometry_hex_rule): dphi products f f' fall into the
                 zero window (1e-9 * anything, (4e-6)(1 - 0.3) ...) and the +1 window ((1 - 1e-9)(1 - 1e-9), ...):
                 d_mask non-empty, which no GLL rule achieves: 480 of the 8 x 3 x 64 dphi entries change, and 388
                 entries of G on the 12 cells
test_hex_geometry_host.py asserts these counts.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from support import LD

U = LD(2.0) ** -53
T0 = 1e-8                 # half width of the zero window
T1 = 1e-8 + 1e-5          # of the windows at +-1, as the kernel forms it
BOUND_FACTOR = 2.0
TOL_ORACLE = 1e-12
C0 = 1500.0
N_ENTRY = (3, 2, 2)
N_P3_PARTIAL = (3, 3, 2)
RULE_POINTS = np.array([1e-9, 0.3, 0.62, 1.0 - 4e-6])
RULE_WEIGHTS = np.array([0.11, 0.37, 0.29, 0.23])
DEGREES = (1, 2, 3, 4, 5, 6, 7)
FLAGS = ((True, True), (True, False), (False, True), (False, False))   # (use_fabs, clamp)
PLAIN = ("perturbed", "sheared", "anisotropic", "far", "mirrored", "half_mirrored")
CLAMPED = ("tiny", "unit_above", "unit_below", "unit_negative")
MESHES = PLAIN + CLAMPED


# ---------------------------------------------------------------------------------------------------------------------
# (value, running error) arithmetic
# ---------------------------------------------------------------------------------------------------------------------
class Num:
    """A value with its first-order running error bound, in the dtype of the value (long double: the reference and
    its bound; float64: the same expressions as numpy evaluates them, the error part then unused)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = np.zeros_like(v) if e is None else e

    def _u(self):
        return self.v.dtype.type(U)

    def __add__(self, o):
        v = self.v + o.v
        return Num(v, self.e + o.e + self._u() * np.abs(v))

    def __sub__(self, o):
        v = self.v - o.v
        return Num(v, self.e + o.e + self._u() * np.abs(v))

    def __mul__(self, o):
        v = self.v * o.v
        return Num(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self._u() * np.abs(v))

    def recip(self):
        v = 1.0 / self.v
        return Num(v, self.e / (self.v * self.v) + self._u() * np.abs(v))

    def fabs(self):
        return Num(np.abs(self.v), self.e)


def _clamp(a: Num, stats: dict):
    """clamp101 of the kernel on a Num: (clamped Num, mask, near).  stats["margin"] and stats["margin_value"] take the
    smallest distance to a window edge over the leading axis' entries (per cell for G, one number for dphi)."""
    v, dt = a.v, a.v.dtype.type
    t0, t1 = dt(T0), dt(T1)
    tgt = np.full(v.shape, np.nan, dtype=v.dtype)
    width, value = [], []
    for b, t in ((-1.0, t1), (0.0, t0), (1.0, t1)):   # the windows are disjoint: the order does not matter
        d = np.abs(v - dt(b))
        tgt = np.where(d <= t, dt(b), tgt)
        width.append(np.abs(d - t) / t)
        value += [np.abs(v - (dt(b) + s * t)) / np.abs(dt(b) + s * t) for s in (-1.0, 1.0)]
    for key, dist in (("margin", width), ("margin_value", value)):
        rel = np.min(dist, axis=0)
        stats[key] = np.minimum(stats[key], rel.min(axis=1) if rel.ndim == 2 else rel.min())
    inside = ~np.isnan(tgt)
    with np.errstate(invalid="ignore"):
        changed = inside & (np.abs(v - tgt) > dt(BOUND_FACTOR) * a.e)
    out = Num(np.where(inside, tgt, v), np.where(inside, dt(0.0), a.e))
    return out, changed, inside & ~changed


def clamp_with_bound(G, G_bound):
    """clamp101 on values G [c][...] that carry the bounds G_bound (2 e, as point_geometry_ld returns them): (clamped G,
    its bound, the mask of changed entries, the smallest window margin); for references that form G outside
    _evaluate, such as a per-cell G_c times the weights"""
    stats = {"margin": np.inf, "margin_value": np.inf}
    shape = G.shape
    f = G.dtype.type(BOUND_FACTOR)
    num, mask, _ = _clamp(Num(G.reshape(shape[0], -1), G_bound.reshape(shape[0], -1) / f), stats)
    return num.v.reshape(shape), (f * num.e).reshape(shape), mask.reshape(shape), float(np.min(stats["margin"]))


def _evaluate(xverts, geom_dofmap, pts, wts, use_fabs, clamp, dtype, points=None):
    """hex_point_geometry of the kernel at the tensor points pts^3 (or the listed ones of them), for every cell, in
    `dtype`"""
    dt = np.dtype(dtype).type
    xc = np.asarray(xverts, dtype=np.float64)[np.asarray(geom_dofmap)].astype(dtype)   # [c][8][3]
    pts, wts = np.asarray(pts, dtype=np.float64), np.asarray(wts, dtype=np.float64)
    n1 = len(pts)
    q = np.arange(n1 ** 3) if points is None else np.asarray(points)
    idx = (q % n1, (q // n1) % n1, q // (n1 * n1))
    X = [Num(pts[i].astype(dtype)) for i in idx]
    one = Num(np.ones(len(q), dtype=dtype))
    f = [(one - X[d], X[d]) for d in range(3)]
    g = (Num(-np.ones(len(q), dtype=dtype)), one)
    stats = {"margin": np.inf, "margin_value": np.inf}
    d_mask = np.zeros((8, 3, len(q)), dtype=bool)
    dphi = []
    for v in range(8):
        a, b, c = v & 1, (v >> 1) & 1, (v >> 2) & 1
        d = [g[a] * f[1][b] * f[2][c], f[0][a] * g[b] * f[2][c], f[0][a] * f[1][b] * g[c]]
        if clamp:
            for k in range(3):
                d[k], d_mask[v, k], _ = _clamp(d[k], stats)
        dphi.append(d)
    J = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for d in range(3):
            s = None
            for v in range(8):
                t = Num(xc[:, v, i][:, None]) * Num(dphi[v][d].v[None, :], dphi[v][d].e[None, :])
                s = t if s is None else s + t   # the kernel's 0.0 + t is exact
            J[i][d] = s
    A = [J[i][d] for i in range(3) for d in range(3)]
    det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6])
    idet = det.recip()
    w = (Num(wts[idx[0]].astype(dtype)) * Num(wts[idx[1]].astype(dtype))) * Num(wts[idx[2]].astype(dtype))
    dw = (det.fabs() if use_fabs else det) * Num(w.v[None, :], w.e[None, :])
    Ji = [(A[4] * A[8] - A[5] * A[7]) * idet, (A[2] * A[7] - A[1] * A[8]) * idet, (A[1] * A[5] - A[2] * A[4]) * idet,
          (A[5] * A[6] - A[3] * A[8]) * idet, (A[0] * A[8] - A[2] * A[6]) * idet, (A[2] * A[3] - A[0] * A[5]) * idet,
          (A[3] * A[7] - A[4] * A[6]) * idet, (A[1] * A[6] - A[0] * A[7]) * idet, (A[0] * A[4] - A[1] * A[3]) * idet]
    shape = dw.v.shape + (3, 3)
    G, Ge = np.zeros(shape, dtype=dtype), np.zeros(shape, dtype=dtype)
    G_mask, G_near = np.zeros(shape, dtype=bool), np.zeros(shape, dtype=bool)
    for a in range(3):
        for b in range(3):
            s = None
            for k in range(3):
                t = (Ji[a * 3 + k] * dw) * Ji[b * 3 + k]
                s = t if s is None else s + t
            if clamp:
                s, G_mask[..., a, b], G_near[..., a, b] = _clamp(s, stats)
            G[..., a, b], Ge[..., a, b] = s.v, s.e
    return SimpleNamespace(G=G, detJw=dw.v, G_bound=dt(BOUND_FACTOR) * Ge, detJw_bound=dt(BOUND_FACTOR) * dw.e,
                           G_mask=G_mask, G_near=G_near, d_mask=d_mask, margin=float(np.min(stats["margin"])),
                           margin_value_cell=np.broadcast_to(np.asarray(stats["margin_value"], dtype=np.float64), (xc.shape[0],)))


def point_geometry_ld(xverts, geom_dofmap, pts, wts, use_fabs, clamp, points=None):
    """G[c][q][3][3] and detJw[c][q] in long double at the tensor points pts^3 (q = i + n1 (j + n1 k)), with the
    per-entry bounds G_bound, detJw_bound, the clamp masks G_mask [c][q][3][3], d_mask [8][3][q], G_near and the
    window margin (module docstring), at every point of the rule or at the listed ones; margin_value_cell [c] is margin_value over the values of one cell (and of dphi)."""
    return _evaluate(xverts, geom_dofmap, pts, wts, use_fabs, clamp, LD, points)


def point_geometry_f64(xverts, geom_dofmap, pts, wts, use_fabs, clamp):
    """the same expressions in plain float64 numpy (no fma): G, detJw"""
    r = _evaluate(xverts, geom_dofmap, pts, wts, use_fabs, clamp, np.float64)
    return r.G, r.detJw


# ---------------------------------------------------------------------------------------------------------------------
# rules and weights
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gll(p: int):
    import wave_fenics_amd as w
    pts, wts, _ = w.tabulate_gll(p)
    return pts, wts


@functools.lru_cache(maxsize=None)
def weight_products(p: int):
    """the distinct w_i w_j w_k of the degree's rule, ascending (products equal to 1e-12 count once)"""
    _, wts = gll(p)
    W = np.sort(((wts[:, None, None] * wts[None, :, None]) * wts[None, None, :]).reshape(-1))
    keep = np.concatenate([[True], np.diff(W) > 1e-12 * W[1:]])
    return W[keep]


def point_weights(p: int):
    """w_i w_j w_k per point q = i + n (j + n k), as the kernel forms it"""
    _, wts = gll(p)
    n = p + 1
    q = np.arange(n ** 3)
    return (wts[q % n] * wts[(q // n) % n]) * wts[q // (n * n)]


def tiny_h(p: int):
    """spacings of `tiny`"""
    W = weight_products(p)
    if p == 1:
        h = 2e-8 / W[0]
        return (h, h, 4.0 * h)
    h = 2.0 ** np.round(np.log2(1e-8 / np.sqrt(W[0] * W[1])))
    return (h, h, h)


def unit_h(p: int, sign: float):
    W = weight_products(p)
    return (1.0 + sign * 4e-6) / W[len(W) // 2]


def operator_n(p: int):
    """(BX + 1, BY + 1, 3) of the box kernels' cross-sections: marching 8x8, 5x5, 4x4, 5x2 -- at P4 the owner form's
    8x2 --, k-split 3x1, 2x1, 2x1"""
    return {1: (9, 9, 3), 2: (6, 6, 3), 3: (5, 5, 3), 4: (9, 3, 3), 5: (4, 2, 3), 6: (3, 2, 3), 7: (3, 2, 3)}[p]


# ---------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------
def _uniform(n, h, reverse_x=False):
    from support import lattice_x
    ax = [np.arange(m + 1) * hh for m, hh in zip(n, h)]
    if reverse_x:
        ax[0] = -ax[0]
    return lattice_x(*ax)


def mesh_coordinates(name: str, p: int, n):
    """vertex coordinates of the box `name` on n cells (None: the unit box's own; perturbed boxes are made by spaces)"""
    from support import lattice_x
    if name == "sheared":
        x = lattice_x(*[np.arange(m + 1) * 0.125 for m in n])
        x[:, 0] += 0.25 * x[:, 1]
        return x
    if name == "anisotropic":
        return _uniform(n, (3.0, 3.0 / 32.0, 96.0))
    if name == "far":
        return lattice_x(*[np.arange(m + 1) + 4096.0 for m in n])
    if name == "tiny":
        return _uniform(n, tiny_h(p))
    if name in ("unit_above", "unit_below", "unit_negative"):
        h = unit_h(p, -1.0 if name == "unit_below" else 1.0)
        return _uniform(n, (h, h, h), reverse_x=name == "unit_negative")
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def mesh_case(name: str, p: int, n=N_ENTRY, structured: bool = True, reorient_seed: int | None = None):
    """The mesh `name` at degree p on n cells: mesh, space V, the oracle's mesh om (its dofmap drives the reference
    apply), rule.  structured=False (always for half_mirrored): the space of mesh_io on the mesh as a dofmap mesh;
    reorient_seed: every cell but cell 0 then in a random one of the 48 orientations.  Cached, shared, unchanged."""
    import wave_fenics_amd as w
    from oracle import wave_oracle as o
    from wave_fenics_amd import mesh_io
    from owner_helpers import spaces
    if name in ("perturbed", "mirrored", "half_mirrored"):
        om, V = spaces(o, n, p, perturb=0.2)
        if name == "mirrored":
            x = om.x.copy()
            x[:, 0] = 1.0 - x[:, 0]
            om, V = spaces(o, n, p, x=x)
    else:
        om, V = spaces(o, n, p, x=mesh_coordinates(name, p, n))
    mesh = V.mesh
    if name == "half_mirrored":
        upper = np.nonzero(np.arange(mesh.ncells) // (n[0] * n[1]) >= n[2] // 2 + n[2] % 2)[0]
        mesh = mesh_io.reorient_cells(mesh, upper, 1)
        structured = False
    if not structured:
        if reorient_seed is not None:
            codes = np.random.default_rng(reorient_seed).integers(0, 48, mesh.ncells)
            codes[0] = 0
            mesh = mesh_io.reorient_cells(mesh, np.arange(mesh.ncells), codes)
        V = mesh_io.create_functionspace(mesh, p)
        om = o.BoxMesh(None, p, np.ascontiguousarray(mesh.x), np.ascontiguousarray(mesh.geom_dofmap),
                       np.ascontiguousarray(V.dofmap), V.ndofs, None)
    pts, wts = gll(p)
    return SimpleNamespace(name=name, p=p, n=tuple(n), mesh=mesh, V=V, om=om, pts=pts, wts=wts, structured=structured)


@functools.lru_cache(maxsize=None)
def reference(name: str, p: int, use_fabs: bool, clamp: bool, n=N_ENTRY, structured: bool = True,
              reorient_seed: int | None = None):
    """point_geometry_ld on a named mesh at its GLL rule.  Cached, shared, unchanged."""
    c = mesh_case(name, p, n, structured, reorient_seed)
    return point_geometry_ld(c.mesh.x, c.mesh.geom_dofmap, c.pts, c.wts, use_fabs, clamp)


@functools.lru_cache(maxsize=None)
def rule_case(which: str):
    """(mesh case, points1, weights1) of the wf_geometry_hex_rule tests: the caller rule RULE_POINTS, or the 3-point
    Gauss rule (nq1 = 3 on a P4 mesh: nq1 != P + 1)"""
    import wave_fenics_amd as w
    c = mesh_case("perturbed", 4)
    if which == "caller":
        return c, RULE_POINTS, RULE_WEIGHTS
    pts, wts = w.quadrature_1d("gauss_jacobi", 4)
    assert len(pts) == 3
    return c, pts, wts


@functools.lru_cache(maxsize=None)
def rule_reference(which: str, use_fabs: bool, clamp: bool):
    c, pts, wts = rule_case(which)
    return point_geometry_ld(c.mesh.x, c.mesh.geom_dofmap, pts, wts, use_fabs, clamp)


# ---------------------------------------------------------------------------------------------------------------------
# operator references: the oracle's sum-factorised apply fed with the long-double G rounded to float64
# ---------------------------------------------------------------------------------------------------------------------
def cell_coefficients(ncells: int):
    """three distinct values, cycling so that neighbouring cells differ"""
    return np.array([0.75, 2.0, 5.5])[np.arange(ncells) % 3]


def vectors(case, seed=1234):
    """x random in (-1, 1); y0 is scaled by the caller to the size of A x"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, case.V.ndofs), rng.uniform(-1, 1, case.V.ndofs)


def apply_reference(case, G, x):
    from oracle import wave_oracle as o
    y = np.zeros(case.V.ndofs)
    o.stiffness_apply_sumfact(case.om, np.ascontiguousarray(np.asarray(G, dtype=np.float64)), C0, x, y)
    return y


@functools.lru_cache(maxsize=None)
def operator_reference(name: str, p: int, use_fabs: bool, clamp: bool, n=None, structured: bool = True,
                       reorient_seed: int | None = None, coeff: str = "none"):
    """x, y0 and yref = y0 + A x of the stiffness operator on a named mesh.  coeff: "none", "after" (clamp(G) a_c: the
    documented order) or "before" (clamp(G a_c)).  Cached, shared, unchanged."""
    n = operator_n(p) if n is None else n
    case = mesh_case(name, p, n, structured, reorient_seed)
    if coeff == "before":
        a = cell_coefficients(case.mesh.ncells).astype(LD)
        r = reference(name, p, use_fabs, False, n, structured, reorient_seed)
        G = Num(r.G * a[:, None, None, None], r.G_bound)
        G = _clamp(G, {"margin": np.inf, "margin_value": np.inf})[0].v if clamp else G.v
    else:
        G = reference(name, p, use_fabs, clamp, n, structured, reorient_seed).G
        if coeff == "after":
            G = G * cell_coefficients(case.mesh.ncells).astype(LD)[:, None, None, None]
    x, y0 = vectors(case)
    Ax = apply_reference(case, G, x)
    y0 = y0 * np.abs(Ax).max()
    return SimpleNamespace(x=x, y0=y0, Ax=Ax, yref=y0 + Ax, scale=float(np.abs(y0 + Ax).max()))


# ---------------------------------------------------------------------------------------------------------------------
# the host rule's sweep: single cells scaled by 400 log-spaced factors
# ---------------------------------------------------------------------------------------------------------------------
# (rounded to 24 bits, so that 1.25 f and 4 f are exact and the scaled cells stay bitwise affine)
SWEEP_FACTORS = np.logspace(-11.0, 4.0, 400).astype(np.float32).astype(np.float64)
SWEEP_SHAPES = ("uniform", "h_h_4h", "sheared")


def sweep_cell(shape: str):
    """the 8 vertices [v][3] of the unscaled single cell, v = a + 2 b + 4 c"""
    e = {"uniform": np.eye(3), "h_h_4h": np.diag([1.0, 1.0, 4.0]),
         "sheared": np.array([[1.0, 0.0, 0.0], [0.25, 1.0, 0.0], [0.0, 0.0, 1.0]])}[shape]   # rows: edge vectors
    v = np.arange(8)
    return (v & 1)[:, None] * e[0] + ((v >> 1) & 1)[:, None] * e[1] + ((v >> 2) & 1)[:, None] * e[2]


@functools.lru_cache(maxsize=None)
def sweep_mesh(shape: str):
    """One mesh of 400 disjoint cells, cell f the single cell scaled by SWEEP_FACTORS[f].  Scaling the vertices of a
    cell at the origin keeps its edge vectors bitwise equal (each is one coordinate minus 0, or a difference of two
    coordinates that share the scaled shear term only in the `sheared` cell -- checked by the host test)."""
    import wave_fenics_amd as w
    base = sweep_cell(shape)
    x = np.concatenate([base * f for f in SWEEP_FACTORS])
    gd = np.arange(8 * len(SWEEP_FACTORS), dtype=np.int32).reshape(-1, 8)
    return w.BoxMesh(None, np.ascontiguousarray(x), gd, (0.0,) * 3, (1.0,) * 3)


@functools.lru_cache(maxsize=None)
def sweep_reference(shape: str, p: int, clamp: bool, full: bool = True):
    """point_geometry_ld on sweep_mesh: at every point, or (full=False) at representative_points(p)"""
    m = sweep_mesh(shape)
    pts, wts = gll(p)
    return point_geometry_ld(m.x, m.geom_dofmap, pts, wts, True, clamp, None if full else representative_points(p))


def representative_points(p: int):
    """one point per distinct w_i w_j w_k, ascending in the weight: on an affine cell G(q) = G_c w_q, so the clamp acts
    somewhere in the cell exactly when it acts at one of these (test_hex_geometry_host.py checks that on the sweep)"""
    W = point_weights(p)
    order = np.argsort(W, kind="stable")
    first = np.concatenate([[True], np.diff(W[order]) > 1e-12 * W[order][1:]])
    return order[first]


@functools.lru_cache(maxsize=None)
def sweep_acts(shape: str, p: int):
    """per cell of sweep_mesh, in long double at the representative points: acts[c] -- does the clamp change an entry of
    G --, and near[c][3][3] -- the components that are a window's constant up to rounding (the off-diagonals that are 0
    in exact arithmetic: the kernel's sum over the vertices leaves a residue of a few 1e-17 |G| there once the compiler
    contracts x_v dphi_v + s, and the clamp makes that residue the 0.0 that G_c holds)"""
    r = sweep_reference(shape, p, True, full=False)
    return SimpleNamespace(acts=r.G_mask.any(axis=(1, 2, 3)), near=r.G_near.any(axis=1))


# ---------------------------------------------------------------------------------------------------------------------
# operator cases shared by the host conditions and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
BOX_OPERATOR_MESHES = ("tiny", "unit_above", "unit_below", "unit_negative")
COEFF_CASES = tuple((name, p) for name in ("tiny", "unit_above", "unit_below") for p in (2, 4))
DOFMAP_MESHES = ("tiny", "unit_above", "half_mirrored")
DOFMAP_DEGREES = (2, 5)
# (BX + 1, BY + 1, 3) of the dofmap marching kernels' cross-sections: 7x4 at P2, the k-split kernel's 3x1 at P5
DOFMAP_N = {2: (8, 5, 3), 5: (4, 2, 3)}
REORIENT_SEED = 5


def operator_fabs(name: str) -> bool:
    """unit_negative is the mesh of WF_FLAG_NO_FABS"""
    return name != "unit_negative"


def dofmap_variants(name: str):
    """(use_fabs, clamp, reorient_seed) of the dofmap operator tests on a mesh"""
    v = [(True, True, None), (True, False, None)]
    if name == "half_mirrored":
        v += [(False, True, REORIENT_SEED), (False, False, REORIENT_SEED)]
    return v
