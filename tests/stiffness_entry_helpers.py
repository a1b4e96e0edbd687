"""Reference, bound, fields and cases of the entry-wise stiffness tests (tests/test_stiffness_entry_host.py,
tests/test_gpu_stiffness_entries.py).  No tests and no GPU in here; torch is never imported.

Every other test of a hexahedral stiffness kernel asks max|y - y_ref| <= 1e-12 max|y_ref| against the float64 oracle
with x ~ U(-1, 1).  That is about 4000 roundings at the loudest entry and says nothing where the field is quiet: with x
decaying over twelve decades, 1e-12 max|y| is some 1e14 roundings at the quiet end, so a plane read from the wrong
buffer there passes.  Here every entry i is held to

    |y_i - ref_i| <= B eps mag_i + gerr_i,      eps = 2^-52,

    ref  = y0 + sum_c a_c P_c^T (-c0^2 D^T G_c D) P_c x                 numpy long double, sum-factorised
    mag  = |y0| + sum_c |a_c| c0^2 |D|^T |G_c| |D| |x_e|                what the roundings of entry i are relative to
    gerr = sum_c |a_c| c0^2 |D|^T G_bound_c |D| |x_e|                   the part of the error that is G's, not the apply's

D is the 1-D table oracle.tabulate_1d_gll (the library's table is the same bits: the host test asserts it), scattered
with np.add.at over the dofmap.  An entry with mag = 0 must be exact (support.ratio).

Geometry.  G is neither the code under test's nor the float64 oracle's:
  "point"  hex_geometry_helpers.point_geometry_ld, the per-point formula with the reference's clamp, and its G_bound;
  "cell"   affine cells: G(q) = G_c w_i w_j w_k with G_c by the host rule's formula (csrc/hex_cell_geometry.cpp: edge
           vectors x1-x0, x2-x0, x4-x0, det by the first row, adjugate * (1 / det), sum_k (Ji[a][k] |det|) Ji[b][k])
           in the (value, running error) arithmetic of hex_geometry_helpers.Num, in long double; G_bound = 2 e W as
           there.  The value is idx_cell_helpers.cell_geometry_longdouble up to that bound (host test).  The clamp is
           applied to G_c W: the rule refuses a cell in which it would change anything, so it only turns the exact
           zeros of a rectilinear cell into the constant 0 they already are.
Both report the clamp margin (hex_geometry_helpers); every mesh here has margin >= 1e-3, so float64 and long double
agree on every clamp decision (host test).  On the perturbed boxes at P4 and above the clamp changes entries of G; the
reference clamps too, so the bound holds there as everywhere.

The bound B.  Roundings of one entry, counted in u = eps / 2, n = P + 1; a sum of m products in any order, with or
without fma, is within m u (1 + O(u)) of its magnitude sum |a_i b_i|:

  per-point G ("point"):
      n     the contraction w_s = sum_a D[q_s][a] x_a, one per direction s (three sums of n terms, each n deep)
      3     the product with the row of G, G_r0 w_0 + G_r1 w_1 + G_r2 w_2
      3     the scale: -c0^2 itself, the product with it, and a_c folded into G and rounded once
      3 n   the contraction sum_a D[a][i] f_0 + D[a][j] f_1 + D[a][k] f_2, one sum of 3 n terms
      8     the sum over at most eight cells and y0 (stores, atomics or registers: any order)
      B_point = 4 n + 14
  per-cell G, all six components ("cell_full"): G(q) is formed as w_k ((coeff w_i w_j) G_c) where the reference has the
      exact product: 3 more.  B_cell = 4 n + 17
  separable ("axes": diagonal G_c, atomic and owner updates): the 1-D operators A = D^T diag(w) D are multiplied out
      beforehand, out = w_k (sx A_i. x + sy A_j. x) + sz A_k. x.  An entry of A is a sum of n products of three factors,
      within (n + 1) u of |D|^T W |D|, which is the magnitude the general form has for the same term (w > 0, G_c
      diagonal and positive), so mag is unchanged:
      n + 1 A;  n the one contraction;  9 the scales (a_c, -c0^2, two weight products, the product with the sum, the
      two additions, w_k);  8 the sum over cells and y0.  B_axes = 2 n + 18 <= B_point
In units of eps those chains are B / 2: the factor two covers the second-order terms and the compiler's freedom to
contract (one rounding where two were counted: the contracted result is off the exact one by no more than the count,
and off the uncontracted float64 one by at most the count again), as in tet_mass_helpers and hex_geometry_helpers.  B is
derived, not measured; test_stiffness_entry_host.py shows both float64 oracle forms within B / 2 everywhere.

Fields (fields()): uniform U(-1, 1); six decays u_i 2^(-40 s_i), s the dof's fraction of the mesh's extent along x, y, z
(from oracle.dof_coordinates), ascending and descending, twelve decades; impulses e_d at a mesh vertex shared by eight cells, and for
P >= 2 at an edge-interior dof shared by four cells along each of x, y, z, a face-interior dof shared by two cells in each
of the three orientations and a cell-interior dof (impulse_dofs(): chosen by element-local index, so that the columns
1..P-1 of D are used, per axis where the mesh has such a cell), and at the last dof a cell names (a corner of the mesh:
the closing lattice line of the owner form); the null space x = 1 and, on affine meshes, x = a . X + b.  y0 is 0
or U(-1, 1) mag_i (where A x has mag_i = 0: U(-1, 1) max(mag), never 0, so that a stray add or store shows in its bits).
One heterogeneous operator per case: a_c = 2^20 and 1 on the cells' checkerboard.

Cases (cases()): the families of tests/test_gpu_guarded_buffers.py at the first cross-section of each degree's WF_*_SHAPES
list, forced the same way; meshes (BX + 1, BY + 1, 5) at lz = 2 for the marching kernels."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import hex_geometry_helpers as hg
from guard_helpers import compiled_shapes
from nonbox_helpers import HOLED_BOX, STIFFNESS_BLOCK, cell_coords, keep_mask
from nonbox_helpers import oracle_mesh as space_oracle_mesh
from owner_helpers import graded, spaces
from support import EPS, LD, cells_per_batch, lattice_x, oracle_module, ratio

C0 = 1500.0
NZ, LZ = 5, 2
MARGIN = 1e-3
CONTRAST = 2.0 ** 20
DECAY_BITS = 40.0
BLOCKS = {1: (4, 4, 4), 2: (3, 3, 3), 3: (4, 2, 2), 4: (2, 2, 2), 5: (2, 2, 1), 6: (2, 2, 1), 7: (2, 2, 1)}
BATCH_BOX = {1: (5, 5, 6), 2: (4, 4, 5), 3: (4, 3, 4), 4: (3, 3, 3), 5: (3, 3, 2), 6: (3, 2, 2), 7: (3, 3, 1)}
# Seeds of the vertex perturbation where the default (42) leaves a value of G within 1e-3 window widths of a clamp
# window's edge: with 1e5 to 1e6 values per mesh some seed does.  The first seed from 1 up with a margin >= 2e-3.
SEEDS = {("perturbed", (6, 3, 5), 4): 1, ("stair", 5): 2, ("stair", 6): 4, ("stair", 7): 3}


def bound(form: str, p: int) -> int:
    """B of the module docstring for the geometry form of a kernel: "point", "cell_full", "axes" """
    n = p + 1
    return {"point": 4 * n + 14, "cell_full": 4 * n + 17, "axes": 2 * n + 18}[form]


# ---------------------------------------------------------------------------------------------------------------------
# geometry references
# ---------------------------------------------------------------------------------------------------------------------
def cell_rule_ld(xverts, geom_dofmap):
    """G_c[c][3][3] of the host rule in long double with its running error bound (2 e), from the edge vectors"""
    xc = np.asarray(xverts, dtype=np.float64)[np.asarray(geom_dofmap)].astype(LD)   # [c][8][3]
    A = [hg.Num(xc[:, v, i]) - hg.Num(xc[:, 0, i]) for i in range(3) for v in (1, 2, 4)]   # J[i * 3 + d]
    det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6])
    idet = det.recip()
    Ji = [(A[4] * A[8] - A[5] * A[7]) * idet, (A[2] * A[7] - A[1] * A[8]) * idet, (A[1] * A[5] - A[2] * A[4]) * idet,
          (A[5] * A[6] - A[3] * A[8]) * idet, (A[0] * A[8] - A[2] * A[6]) * idet, (A[2] * A[3] - A[0] * A[5]) * idet,
          (A[3] * A[7] - A[4] * A[6]) * idet, (A[1] * A[6] - A[0] * A[7]) * idet, (A[0] * A[4] - A[1] * A[3]) * idet]
    d = det.fabs()
    G, Ge = np.zeros((xc.shape[0], 3, 3), dtype=LD), np.zeros((xc.shape[0], 3, 3), dtype=LD)
    for a in range(3):
        for b in range(3):
            s = None
            for k in range(3):
                t = (Ji[a * 3 + k] * d) * Ji[b * 3 + k]
                s = t if s is None else s + t
            G[:, a, b], Ge[:, a, b] = s.v, s.e
    return G, LD(hg.BOUND_FACTOR) * Ge


def geometry_ld(om, p: int, form: str):
    """G[c][q][3][3], G_bound and the clamp margin of the mesh om at the degree's GLL rule; form "point" or "cell" """
    pts, wts = hg.gll(p)
    if form == "point":
        r = hg.point_geometry_ld(om.x, om.geom_dofmap, pts, wts, True, True)
        return SimpleNamespace(G=r.G, G_bound=r.G_bound, margin=r.margin, changed=int(r.G_mask.sum()))
    Gc, Gcb = cell_rule_ld(om.x, om.geom_dofmap)
    n = p + 1
    q = np.arange(n ** 3)
    w = np.asarray(wts, dtype=np.float64).astype(LD)
    W = w[q % n] * w[(q // n) % n] * w[q // (n * n)]
    G = Gc[:, None, :, :] * W[None, :, None, None]
    Gb = Gcb[:, None, :, :] * W[None, :, None, None]
    G, Gb, mask, margin = hg.clamp_with_bound(G, Gb)
    return SimpleNamespace(G=G, G_bound=Gb, margin=margin, changed=int(mask.sum()))


# ---------------------------------------------------------------------------------------------------------------------
# the apply in long double
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(p: int):
    """D[q][a] of oracle.tabulate_1d_gll as float64 and as long double"""
    D = np.ascontiguousarray(oracle_module().tabulate_1d_gll(p)[3])
    D.setflags(write=False)
    return D, D.astype(LD)


def _grad(D, u):
    return (np.einsum("ia,fckja->fckji", D, u), np.einsum("ja,fckai->fckji", D, u), np.einsum("ka,fcaji->fckji", D, u))


def _grad_t(D, f):
    return (np.einsum("ai,fckja->fckji", D, f[0]) + np.einsum("aj,fckai->fckji", D, f[1])
            + np.einsum("ak,fcaji->fckji", D, f[2]))


def _cell_apply(D, G, u):
    """D^T G D u per cell: u [f][c][k][j][i], G [c][k][j][i][3][3]"""
    w = _grad(D, u)
    return _grad_t(D, [G[None, ..., r, 0] * w[0] + G[None, ..., r, 1] * w[1] + G[None, ..., r, 2] * w[2] for r in range(3)])


def reference(om, p: int, geo, X, a=None, c0: float = C0):
    """(A x, mag, gerr) of the module docstring without y0, each [nf][ndofs] in long double, for the fields X [nf][ndofs]
    (float64) and the cell coefficients a (None: 1)."""
    n = p + 1
    _, D = table(p)
    dm = np.asarray(om.dofmap)
    nc, nf = dm.shape[0], X.shape[0]
    u = np.asarray(X, dtype=np.float64).astype(LD)[:, dm].reshape(nf, nc, n, n, n)
    G = geo.G.reshape(nc, n, n, n, 3, 3)
    Gb = geo.G_bound.reshape(nc, n, n, n, 3, 3)
    c2 = LD(c0) * LD(c0)
    ac = np.ones(nc, dtype=LD) if a is None else np.asarray(a, dtype=np.float64).astype(LD)
    s = ac[None, :, None, None, None]
    Da, ua = np.abs(D), np.abs(u)
    parts = (-c2 * s * _cell_apply(D, G, u), c2 * np.abs(s) * _cell_apply(Da, np.abs(G), ua),
             c2 * np.abs(s) * _cell_apply(Da, Gb, ua))
    out = []
    for v in parts:
        y = np.zeros((om.ndofs, nf), dtype=LD)
        np.add.at(y, dm.reshape(-1), np.moveaxis(v.reshape(nf, -1), 0, 1))
        out.append(np.ascontiguousarray(y.T))
    return tuple(out)


def entry_check(got, y0, ax, mag, gerr, B):
    """|got - (y0 + ax)| <= B eps (|y0| + mag) + gerr at every entry, through support.ratio with gerr folded into the
    magnitude.  Returns (plain, ok, at, used): the worst err / (eps (|y0| + mag)), a figure without gerr; all within;
    the first index outside; the largest fraction of its allowance an entry uses."""
    y0 = np.asarray(y0, dtype=np.float64).astype(LD)
    m = np.abs(y0) + mag
    folded, ok, at = ratio(got, y0 + ax, m + gerr / (LD(B) * LD(EPS)), B)
    return ratio(got, y0 + ax, m, B)[0], ok, at, folded / B


def scaled_y0(mag, seed: int):
    """U(-1, 1) mag_i per entry; U(-1, 1) max(mag) where mag_i = 0.  Never 0."""
    m = np.asarray(mag, dtype=np.float64)
    m = np.where(m > 0.0, m, m.max())
    y0 = np.random.default_rng(seed).uniform(-1, 1, m.shape) * m
    assert np.all(y0 != 0.0)
    return y0


# ---------------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------------
# element-local (i, j, k) of the impulses that are not mesh vertices: name -> (local index, cells that share the dof)
IMPULSE_LOCAL = {"edge-x": ((1, 0, 0), 4), "edge-y": ((0, 1, 0), 4), "edge-z": ((0, 0, 1), 4),
                 "face-xy": ((1, 1, 0), 2), "face-xz": ((1, 0, 1), 2), "face-yz": ((0, 1, 1), 2), "interior": ((1, 1, 1), 1)}


def impulse_dofs(om, p: int):
    """[(name, dof)]: the first mesh vertex shared by 8 cells (where the mesh has one); for P >= 2 the dof at the local
    index of IMPULSE_LOCAL -- one index in 1..P-1 along the named axis for an edge, two for a face, three for the
    interior -- of the first cell where that dof is shared by four (edge), two (face) cells, per axis where the mesh has
    such a cell; the last dof a cell names (a corner vertex of the mesh)."""
    dm = np.asarray(om.dofmap)
    n = p + 1
    count = np.bincount(dm.reshape(-1), minlength=om.ndofs)
    nodal = np.zeros(om.ndofs, dtype=bool)   # mesh vertices: every local coordinate 0 or P
    nodal[dm[:, [i + n * (j + n * k) for k in (0, p) for j in (0, p) for i in (0, p)]].reshape(-1)] = True
    out = []
    if (nodal & (count == 8)).any():
        out.append(("vertex8", int(np.nonzero(nodal & (count == 8))[0][0])))
    if p >= 2:
        for name, ((i, j, k), cells) in IMPULSE_LOCAL.items():
            col = dm[:, i + n * (j + n * k)]
            hit = np.nonzero(count[col] == cells)[0]
            if name == "interior":
                hit = hit[hit >= dm.shape[0] // 2]      # the middle cell
            if hit.size:
                d = int(col[hit[0]])
                assert count[d] == cells and not nodal[d] and (i, j, k).count(1) == {4: 1, 2: 2, 1: 3}[cells]
                out.append((name, d))
    out.append(("last", int(dm.max())))
    return out


def support_of(om, dof: int):
    """mask of the dofs of the cells that contain dof"""
    dm = np.asarray(om.dofmap)
    inside = np.zeros(om.ndofs, dtype=bool)
    inside[dm[(dm == dof).any(axis=1)].reshape(-1)] = True
    return inside


def fields(om, p: int, affine: bool, seed: int):
    """(names, X [nf][ndofs] float64, {field name: impulse dof}) of the module docstring"""
    dm = np.asarray(om.dofmap)
    listed = np.zeros(om.ndofs, dtype=bool)
    listed[dm.reshape(-1)] = True
    xd = oracle_module().dof_coordinates(om)
    lo, hi = xd[listed].min(axis=0), xd[listed].max(axis=0)
    s = np.clip((xd - lo) / (hi - lo), 0.0, 1.0)
    u = np.random.default_rng(seed).uniform(-1, 1, om.ndofs)
    names, X, impulses = ["uniform"], [u], {}
    for axis in range(3):
        for down in (False, True):
            names.append(f"decay-{'xyz'[axis]}{'-' if down else '+'}")
            X.append(u * 2.0 ** (-DECAY_BITS * (1.0 - s[:, axis] if down else s[:, axis])))
    for name, d in impulse_dofs(om, p):
        e = np.zeros(om.ndofs)
        e[d] = 1.0
        names.append(f"impulse-{name}")
        X.append(e)
        impulses[names[-1]] = d
    names.append("ones")
    X.append(np.ones(om.ndofs))
    if affine:
        names.append("linear")
        X.append(xd @ np.array([0.75, -1.25, 0.5]) + 0.25)
    X = np.ascontiguousarray(np.stack(X))
    X.setflags(write=False)
    return names, X, impulses


def checkerboard(coords):
    c = np.asarray(coords)
    return np.where(c.sum(axis=1) % 2 == 0, CONTRAST, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# meshes and cases
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def box_mesh(kind: str, n, p: int):
    """the boxes of test_gpu_guarded_buffers.stiffness_box: "perturbed", "sheared" (x += 0.25 y on a 0.125 lattice),
    "graded" (rectilinear): (space, oracle mesh, cell coordinates)"""
    o = oracle_module()
    if kind == "perturbed":
        om, V = spaces(o, n, p, perturb=0.2)
        if (kind, n, p) in SEEDS:
            import wave_fenics_amd as w
            om, V = spaces(o, n, p, x=w.create_box(n, perturb=0.2, seed=SEEDS[(kind, n, p)]).x)
    elif kind == "sheared":
        xv = lattice_x(*[np.arange(m + 1) * 0.125 for m in n])
        xv[:, 0] += 0.25 * xv[:, 1]
        om, V = spaces(o, n, p, x=xv)
    else:
        om, V = graded(o, n, p)
    return V, om, cell_coords(n)


@functools.lru_cache(maxsize=None)
def batch_mesh(p: int, ncells: int | None = None):
    """the first 2 B + 1 cells of the perturbed box BATCH_BOX[p] with the box's dof numbers, B = 256 // (P+1)^2 (or the
    first ncells: the mass kernels with another batch size)"""
    import wave_fenics_amd as w
    if ncells is None:
        ncells = 2 * cells_per_batch(p) + 1
    box = w.create_box(BATCH_BOX[p], perturb=0.2)
    Vb = w.create_functionspace(box, p)
    assert ncells <= box.ncells
    dm = np.ascontiguousarray(Vb.dofmap[:ncells].astype(np.int32))
    mesh = w.BoxMesh(box.n, box.x, np.ascontiguousarray(box.geom_dofmap[:ncells]), box.lo, box.hi)
    V = w.FunctionSpace(mesh, p, dm, w.IndexMap(Vb.ndofs), None, structured=False)
    return V, space_oracle_mesh(mesh, V), cell_coords(BATCH_BOX[p])[:ncells]


@functools.lru_cache(maxsize=None)
def holed_mesh(p: int):
    """the "stair" of nonbox_helpers (holed_box, route "subset": the box space's dof numbers) with the seed of SEEDS"""
    import wave_fenics_amd as w
    keep = keep_mask("stair")
    box = w.create_box(HOLED_BOX, perturb=0.2, seed=SEEDS.get(("stair", p), 42))
    mesh = w.BoxMesh(tuple(HOLED_BOX), box.x, np.ascontiguousarray(box.geom_dofmap[keep]), box.lo, box.hi)
    Vb = w.create_functionspace(box, p)
    V = w.FunctionSpace(mesh, p, np.ascontiguousarray(Vb.dofmap[keep]), w.IndexMap(Vb.ndofs), None, structured=False)
    return V, space_oracle_mesh(mesh, V), cell_coords(HOLED_BOX)[keep]


def first_shape(shapes, p: int):
    return next(s for s in shapes if s[0] == p)


@functools.lru_cache(maxsize=None)
def cases():
    """Every case of the entry tests: family, id, p, mesh = (builder, arguments), form ("point", "cell_full", "axes": the
    bound and, through data(), the reference's G), structured, tuning, flags (0 or "ordered"), want = (kernel, geometry,
    metric, update)."""
    march = compiled_shapes("stiffness_march.hip", "WF_MARCH_SHAPES")           # (P, variant, BX, BY)
    ks = compiled_shapes("stiffness_march_ks.hip", "WF_KS_SHAPES")              # (P, BX, BY)
    owner = compiled_shapes("stiffness_march_owner.hip", "WF_OWNER_SHAPES")     # (P, variant, BX, BY)
    idx = compiled_shapes("stiffness_march_idx.hip", "WF_IDX_SHAPES")
    out = []

    def add(family, what, p, mesh, form, structured, tuning, want, flags=0):
        out.append(SimpleNamespace(family=family, id=f"{family}-{what}", p=p, mesh=mesh, form=form, structured=structured,
                                   tuning=tuning, want=want, flags=flags, affine=form != "point"))

    forms = (("march_point", "perturbed", "point", {"geometry": "per_point"}, ("march_box", "per_point", "none", "none")),
             ("march_cell_full", "sheared", "cell_full", {"geometry": "per_cell", "metric": "full"}, ("march_box", "per_cell", "full", "none")),
             ("march_axes_atomic", "graded", "axes", {"geometry": "per_cell", "metric": "axes", "update": "atomic"},
              ("march_box", "per_cell", "axes", "atomic")))
    for family, kind, form, tuning, want in forms:
        for p in range(1, 5):
            _, variant, bx, by = first_shape(march, p)
            add(family, f"P{p}-{bx}x{by}", p, (box_mesh, (kind, (bx + 1, by + 1, NZ), p)), form, True,
                dict(tuning, variant=variant, lz=LZ), want)
    for p in range(4, 8):
        _, bx, by = first_shape(ks, p)
        tuning = {"block": (bx, by, 1), "lz": LZ}
        if p == 4:
            tuning["variant"] = 3
        add("ksplit", f"P{p}-{bx}x{by}", p, (box_mesh, ("perturbed", (bx + 1, by + 1, NZ), p)), "point", True, tuning,
            ("march_box", "per_point", "none", "none"))
    for p in range(1, 8):
        _, variant, bx, by = first_shape(owner, p)
        for exact in (False, True):
            n = (bx, by, NZ - 1) if exact else (bx + 1, by + 1, NZ)
            add("owner", f"P{p}-{bx}x{by}-{'exact' if exact else 'partial'}", p, (box_mesh, ("graded", n, p)), "axes", True,
                {"update": "owner", "variant": variant, "lz": LZ}, ("march_box", "per_cell", "axes", "owner"))
    for p in range(1, 8):
        block = BLOCKS[p]
        add("box_block", f"P{p}", p, (box_mesh, ("perturbed", tuple(b + 1 for b in block), p)), "point", True,
            {"kernel": "box_block", "block": block}, ("box_block", "per_point", "none", "none"))
    idx_forms = (("point", "perturbed", "point", {}, ("march_idx", "per_point", "none", "none"), range(1, 8)),
                 ("cell_full", "sheared", "cell_full", {"geometry": "per_cell", "metric": "full"}, ("march_idx", "per_cell", "full", "none"), range(1, 5)),
                 ("cell_axes", "graded", "axes", {"geometry": "per_cell", "metric": "axes"}, ("march_idx", "per_cell", "axes", "atomic"), range(1, 5)))
    for name, kind, form, tuning, want, degrees in idx_forms:
        for p in degrees:
            bx, by = STIFFNESS_BLOCK[p]
            assert (p, bx, by) == (first_shape(idx, p) if p <= 4 else first_shape(ks, p))
            add("idx", f"{name}-P{p}-{bx}x{by}", p, (box_mesh, (kind, (bx + 1, by + 1, NZ), p)), form, False,
                dict(tuning, kernel="march", lz=LZ), want)
    for p in range(1, 8):
        add("idx", f"holed-P{p}", p, (holed_mesh, (p,)), "point", False, {"kernel": "march", "lz": LZ},
            ("march_idx", "per_point", "none", "none"))
    for hint, kernel in (("batch", "batch_unique"), ("elementwise", "elementwise")):
        for p in range(1, 8):
            add("batch", f"{hint}-P{p}", p, (batch_mesh, (p,)), "point", False, {"kernel": hint, "keep_cell_order": True},
                (kernel, "per_point", "none", "none"))
    for p in (2, 5):
        add("ordered", f"P{p}", p, (batch_mesh, (p,)), "point", False, None, ("cells_ordered", "per_point", "none", "ordered"),
            flags="ordered")
    return tuple(out)


def mesh_of(case):
    """(space, oracle mesh, cell coordinates) of a case"""
    builder, args = case.mesh
    return builder(*args)


_data = {}


def data(case):
    """Everything the comparison needs for the mesh and degree of a case, computed once, shared by the cases on that
    mesh and left unchanged: names, X, impulses, B-free references ax, mag, gerr (and axh, magh, gerrh of the
    heterogeneous operator under the uniform field, with its coefficients a), margin."""
    key = (case.mesh[0].__name__, case.mesh[1], "point" if case.form == "point" else "cell")
    if key not in _data:
        V, om, coords = mesh_of(case)
        geo = geometry_ld(om, case.p, key[2])
        names, X, impulses = fields(om, case.p, case.affine, seed=17 + case.p)
        ax, mag, gerr = reference(om, case.p, geo, X)
        a = checkerboard(coords)
        axh, magh, gerrh = reference(om, case.p, geo, X[:1], a)
        _data[key] = SimpleNamespace(V=V, om=om, geo=geo, names=names, X=X, impulses=impulses, ax=ax, mag=mag, gerr=gerr,
                                     a=a, axh=axh[0], magh=magh[0], gerrh=gerrh[0], margin=geo.margin)
    return _data[key]
