"""Reference, bound, fields and cases of the entry-wise hexahedral mass tests (tests/test_mass_entry_host.py,
tests/test_gpu_mass_entries.py).  No tests and no GPU in here; torch is never imported.

Every other test of a hexahedral mass kernel asks max|y - y_ref| <= 1e-12 max|y_ref| against the float64 oracle with
x ~ U(-1, 1), which says nothing where the field is quiet (tests/stiffness_entry_helpers.py on the same weakness of the
stiffness tests).  Here every entry i of y = y0 + M x is held to

    |y_i - ref_i| <= B eps mag_i + derr_i,      eps = 2^-52,

  dense    ref  = y0 + sum_c P_c^T Phi^T diag(d_c) Phi P_c x             numpy long double, sum-factorised,
           mag  = |y0| + sum_c P_c^T |Phi|^T diag(|d_c|) |Phi| |P_c x|   Phi = phi1 (x) phi1 (x) phi1
           derr = sum_c P_c^T |Phi|^T diag(dbound_c) |Phi| |P_c x|
  lumped   ref  = y0 + (sum_c d_c) x,  mag = |y0| + (sum_c |d_c|) |x|,  derr = (sum_c dbound_c) |x|

scattered with np.add.at over the dofmap; d_c carries the cell coefficient a_c where there is one.  An entry with
mag = 0 keeps the bits of y0 (support.ratio, support.bits).

Inputs.  "tables": the operator is created from float64 arrays that the reference reads as well -- phi1 of
oracle.tabulate_mass_tables (or a random table), det J w of oracle.compute_detJ_generic -- so both sides start from the
same numbers, derr = 0 and B alone binds.  "library": the operator builds det J w itself (the rule-built MassOperator,
the structured lumped mass through the box geometry kernel); then d and dbound are
hex_geometry_helpers.point_geometry_ld's detJw and detJw_bound at the same rule (the 1-D table is the library's
tabulate_1d, read by both sides), and derr is the share of the allowance that is the geometry's, not the apply's.

The bound B.  Roundings of one entry, counted in u = eps / 2; a sum of k products in any order, with or without fma, is
within k u (1 + O(u)) of its magnitude sum |a_i b_i|.  n = P + 1 nodes, m points per direction:

  dense:   3 n   the three forward contractions sum_a phi1[q][a] v_a, one per direction, each n terms deep
           1     the product with d
           1     a_c folded into d and rounded once (exact for the powers of two used here; counted as it is for any a_c)
           3 m   the three transposed contractions sum_q phi1[q][a] w_q, each m terms deep
           8     the additions of at most eight cells' values and y0, in any order and grouping: LDS adds into a
                 zeroed tile (0 + v is exact), the carried z plane, the epilogue's sum over four cells, the unique-dof
                 tile, the ordered segment sum, global atomics -- nine terms, eight additions
           B_dense = 3 n + 3 m + 10
  lumped:  1 the product x d;  1 a_c;  8 the additions as above (pre-assembled diagonal: at most seven additions into m,
           one product m x, one addition to y0, and a_c: ten as well)
           B_lumped = 10
In units of eps those chains are B / 2: the factor two covers the second-order terms and the compiler's freedom to
contract (stiffness_entry_helpers, hex_geometry_helpers).  B is derived, not measured; test_mass_entry_host.py shows two
float64 forms of each operator within B / 2 everywhere.

Fields: those of stiffness_entry_helpers.fields (uniform; six decays u_i 2^(-40 s_i); impulses at a vertex of eight
cells, edge-, face- and cell-interior dofs and the last dof; x = 1), each with y0 = 0 and y0 = U(-1, 1) mag; one
heterogeneous operator per case, a_c = 2^20 and 1 on the cells' checkerboard, through cell_coeff=.  x = 1 has the known
answer sum(y) = sum(d) up to the table's partition-of-unity residue (ones_slack).

Cases (cases()): see the header of tests/test_gpu_mass_entries.py."""
from __future__ import annotations

import functools
import os
import re
from types import SimpleNamespace

import numpy as np

import hex_geometry_helpers as hg
import stiffness_entry_helpers as se
from guard_helpers import CSRC, compiled_shapes
from nonbox_helpers import cell_coords
from nonbox_helpers import oracle_mesh as space_oracle_mesh
from support import EPS, LD, cells_per_batch, oracle_module

NZ, LZ = 5, 2              # march, segments: items of 2, 2 and 1 layers
DEEP_LZ = 9                # march, deep items: every ring cursor wraps (test_mass_entry_host.py); nz = lz + 1
STAIR_PAIRS = ((2, 3), (2, 4), (4, 5), (4, 4))
ORIENT_BOX = (5, 4, 3)     # the box of test_gpu_unstructured.build_mesh("random_orient")


def bound(family: str, p: int, m: int | None = None) -> int:
    """B of the module docstring: family "dense" (m points per direction) or "lumped" """
    return 3 * (p + 1) + 3 * m + 10 if family == "dense" else 10


def npts(quad: str, qd: int) -> int:
    """points of the 1-D rule of degree qd (oracle.tabulate_mass_tables)"""
    return max(2, (qd + 4) // 2) if quad == "gll" else (qd + 2) // 2


def rule_of(p: int, m: int):
    """(variant, quad, qdegree) of a compiled pair (P, M) of WF_MASS_SHAPES: the square Gauss rule of degree 2 P, the
    Gauss rule of degree 2 P + 2 (M = P + 2), else the GLL rule of degree P + 1"""
    variant = "gll_warped" if p % 2 == 0 else "equispaced"
    quad, qd = ("gauss_jacobi", 2 * p) if m == p + 1 else ("gauss_jacobi", 2 * p + 2) if m == p + 2 else ("gll", p + 1)
    assert npts(quad, qd) == m, (p, m)
    return variant, quad, qd


ORACLE_VARIANT = {"gll_warped": "gll", "equispaced": "equispaced"}


def mass_dense_cells_per_batch(mx: int) -> int:
    """cells per workgroup of k_mass_dense, asserted against the source text (csrc/mass_batch.hip)"""
    with open(os.path.join(CSRC, "mass_batch.hip")) as f:
        text = f.read()
    body = re.search(r"int mass_dense_cells_per_batch\(int mx\)\s*\{\s*return ([^;]+);", text)
    assert body and body.group(1) == "std::max(1, std::min(1400 / (mx * mx * mx), 32))", body
    return max(1, min(1400 // mx ** 3, 32))


# ---------------------------------------------------------------------------------------------------------------------
# tables and det J w
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_table(p: int, variant: str, quad: str, qd: int):
    """phi1 [m][n], the 1-D rule and the 3-D points X, weights W of oracle.tabulate_mass_tables (float64, read-only)"""
    pts, wts, phi1, _, X, W = oracle_module().tabulate_mass_tables(p, ORACLE_VARIANT[variant], quad, qd)
    phi1 = np.ascontiguousarray(phi1)
    phi1.setflags(write=False)
    return SimpleNamespace(phi1=phi1, pts=pts, wts=wts, X=X, W=W, m=phi1.shape[0])


@functools.lru_cache(maxsize=None)
def random_table(p: int, m: int, seed: int):
    """a table that does not read the same backwards: U(-1, 1) [m][n]; points and weights of the Gauss rule of m points"""
    t = oracle_table(p, "gll_warped", "gauss_jacobi", 2 * m - 2)
    assert t.m == m
    phi1 = np.random.default_rng(seed).uniform(-1, 1, (m, p + 1))
    assert np.abs(phi1[::-1, ::-1] - phi1).max() > 0.1
    phi1.setflags(write=False)
    return SimpleNamespace(phi1=phi1, pts=t.pts, wts=t.wts, X=t.X, W=t.W, m=m)


@functools.lru_cache(maxsize=None)
def library_table(p: int, variant: str, quad: str, qd: int):
    """what MassOperator(V, p, variant=, quad=, qdegree=) builds its operator from: the library's rule and 1-D table"""
    import wave_fenics_amd as w
    pts, wts = w.quadrature_1d(quad, qd)
    phi1 = np.ascontiguousarray(w.tabulate_1d(p, pts, 0, variant), dtype=np.float64)
    phi1.setflags(write=False)
    return SimpleNamespace(phi1=phi1, pts=np.asarray(pts), wts=np.asarray(wts), X=None, W=None, m=phi1.shape[0])


@functools.lru_cache(maxsize=None)
def lumped_rule(p: int):
    """the GLL rule of the lumped mass as the oracle tabulates it: X, W of quadrature_weights_hex"""
    X, W = oracle_module().quadrature_weights_hex(p)
    return SimpleNamespace(X=X, W=W, m=p + 1)


def detj_tables(om, rule):
    """det J w (no fabs) of oracle.compute_detJ_generic: the float64 array handed to the operator; dbound = 0"""
    d = np.ascontiguousarray(oracle_module().compute_detJ_generic(om, rule.X, rule.W))
    d.setflags(write=False)
    return d, d.astype(LD), np.zeros(d.shape, dtype=LD)


def detj_library(om, pts, wts, use_fabs: bool):
    """(None, d, dbound) of hex_geometry_helpers.point_geometry_ld at the rule pts^3: what the library's own det J w is
    held to"""
    r = hg.point_geometry_ld(om.x, om.geom_dofmap, pts, wts, use_fabs, False)
    return None, r.detJw, r.detJw_bound


# ---------------------------------------------------------------------------------------------------------------------
# the applies in long double (and, for the host tests, in float64)
# ---------------------------------------------------------------------------------------------------------------------
def cell_mass(phi, d, u):
    """Phi^T diag(d) Phi u per cell in the dtype of the arguments: phi [m][n], d [c][qk][qj][qi], u [f][c][k][j][i]"""
    t = np.einsum("qi,fckji->fckjq", phi, u)
    t = np.einsum("rj,fckjq->fckrq", phi, t)
    t = np.einsum("sk,fckrq->fcsrq", phi, t) * d[None]
    t = np.einsum("sk,fcsrq->fckrq", phi, t)
    t = np.einsum("rj,fckrq->fckjq", phi, t)
    return np.einsum("qi,fckjq->fckji", phi, t)


def scatter(om, v, nf):
    """sum_c P_c^T v_c: v [f][c][...nd] -> [f][ndofs]"""
    y = np.zeros((om.ndofs, nf), dtype=v.dtype)
    np.add.at(y, np.asarray(om.dofmap).reshape(-1), np.moveaxis(v.reshape(nf, -1), 0, 1))
    return np.ascontiguousarray(y.T)


def gathered(om, p: int, X, dtype):
    n = p + 1
    dm = np.asarray(om.dofmap)
    return np.asarray(X, dtype=np.float64).astype(dtype)[:, dm].reshape(X.shape[0], dm.shape[0], n, n, n)


def coefficients(nc: int, a):
    return np.ones(nc, dtype=LD) if a is None else np.asarray(a, dtype=np.float64).astype(LD)


def reference_dense(om, p: int, phi1, d, dbound, X, a=None):
    """(M x, mag, derr) of the module docstring without y0, each [nf][ndofs] in long double, for the fields X [nf][ndofs],
    the table phi1 [m][n] (float64), d and dbound [ncells][m^3] (long double) and the cell coefficients a (None: 1)"""
    m, nf, nc = phi1.shape[0], X.shape[0], np.asarray(om.dofmap).shape[0]
    phi = np.asarray(phi1, dtype=np.float64).astype(LD)
    u = gathered(om, p, X, LD)
    s = coefficients(nc, a)[:, None, None, None]
    dd, db = (d.reshape(nc, m, m, m) * s), (dbound.reshape(nc, m, m, m) * np.abs(s))
    pa, ua = np.abs(phi), np.abs(u)
    return tuple(scatter(om, v, nf) for v in (cell_mass(phi, dd, u), cell_mass(pa, np.abs(dd), ua), cell_mass(pa, db, ua)))


def reference_lumped(om, p: int, d, dbound, X, a=None):
    """the same for the lumped mass: d, dbound [ncells][n^3] at the GLL nodes"""
    n, nf, nc = p + 1, X.shape[0], np.asarray(om.dofmap).shape[0]
    u = gathered(om, p, X, LD)
    s = coefficients(nc, a)[:, None, None, None]
    dd, db = (d.reshape(nc, n, n, n) * s)[None], (dbound.reshape(nc, n, n, n) * np.abs(s))[None]
    return tuple(scatter(om, v, nf) for v in (dd * u, np.abs(dd) * np.abs(u), db * np.abs(u)))


def ones_slack(phi1, d):
    """sum_i (M 1)_i = sum_q d_q (r r r)_q^2 with r = phi1 1 the table's row sums: |sum(ref) - sum(d)| <=
    sum|d| ((1 + delta)^6 - 1), delta = max|r - 1| in long double (0 for the lumped mass: phi1 None)"""
    if phi1 is None:
        return LD(0)
    delta = np.max(np.abs(np.asarray(phi1, dtype=np.float64).astype(LD).sum(axis=1) - 1))
    return np.sum(np.abs(d)) * ((1 + delta) ** 6 - 1)


def scaled_y0(mag, seed: int):
    """stiffness_entry_helpers.scaled_y0; where M x has no magnitude at all (an impulse that the one-point rule at the
    cell centre does not see) U(-1, 1)"""
    m = np.asarray(mag, dtype=np.float64)
    return se.scaled_y0(m if (m > 0).any() else np.ones_like(m), seed)


# ---------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oriented_mesh(p: int):
    """the randomly re-oriented box of test_gpu_unstructured.build_mesh("random_orient"), topological numbering"""
    from wave_fenics_amd import mesh_io
    from test_gpu_unstructured import build_mesh
    mesh, _ = build_mesh("random_orient", p)
    V = mesh_io.create_functionspace(mesh, p)
    assert mesh.ncells == ORIENT_BOX[0] * ORIENT_BOX[1] * ORIENT_BOX[2]
    return V, space_oracle_mesh(mesh, V), cell_coords(ORIENT_BOX)


def cut_mesh(p: int, ncells: int):
    return se.batch_mesh(p, ncells)


def mesh_of(case):
    """(space, oracle mesh, cell coordinates) of a case"""
    builder, args = case.mesh
    return builder(*args)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    """Every case of the entry tests.  family; id; p; op "dense" or "lumped"; mesh = (builder, arguments); table = (maker,
    arguments) or None (lumped); source "tables" or "library" (module docstring); tuning; flags (names of WF_FLAG_*);
    structured; kernel (op.kernel); plan (None or the plan fields to assert); nan (x is NaN where no cell names the dof);
    twice (two applies agree bit for bit)."""
    shapes = compiled_shapes("mass_march.hip", "WF_MASS_SHAPES")      # (P, M, BX, BY)
    out = []

    def add(family, what, p, op, mesh, table, kernel, tuning=None, source="tables", flags=(), structured=False, plan=None,
            nan=False, twice=False):
        out.append(SimpleNamespace(family=family, id=f"{family}-{what}", p=p, op=op, mesh=mesh, table=table, kernel=kernel,
                                   tuning=tuning, source=source, flags=tuple(flags), structured=structured, plan=plan,
                                   nan=nan, twice=twice))

    def pair_table(p, m):
        return (oracle_table, (p,) + rule_of(p, m))

    # 1. march, segments: every compiled shape, partly filled columns, items of 2, 2 and 1 layers
    for p, m, bx, by in shapes:
        add("march_segments", f"P{p}-M{m}-{bx}x{by}", p, "dense", (se.box_mesh, ("perturbed", (bx + 1, by + 1, NZ), p)),
            pair_table(p, m), "march_idx", {"kernel": "mass_march", "block": (bx, by, 0), "lz": LZ},
            plan={"lz": LZ, "items": 4 * 3, "reoriented": 0})
    # 2. march, deep items: the default cross-section of every pair, items of 9 and 1 layers
    defaults = {}
    for p, m, bx, by in shapes:
        defaults.setdefault((p, m), (bx, by))
    for (p, m), (bx, by) in defaults.items():
        add("march_deep", f"P{p}-M{m}-{bx}x{by}", p, "dense", (se.box_mesh, ("perturbed", (bx + 1, by + 1, DEEP_LZ + 1), p)),
            pair_table(p, m), "march_idx", {"kernel": "mass_march", "block": (bx, by, 0), "lz": DEEP_LZ},
            plan={"lz": DEEP_LZ, "items": 4 * 2, "reoriented": 0})
    # 3. march, other meshes
    for p, m in STAIR_PAIRS:
        assert (p, m) in defaults
        add("march_meshes", f"stair-P{p}-M{m}", p, "dense", (se.holed_mesh, (p,)), pair_table(p, m), "march_idx",
            {"kernel": "mass_march", "lz": LZ}, plan={"lz": LZ, "reoriented": 0})
        add("march_meshes", f"oriented-P{p}-M{m}", p, "dense", (oriented_mesh, (p,)), pair_table(p, m), "march_idx",
            {"kernel": "mass_march"}, plan={"reoriented_above": ORIENT_BOX[0] * ORIENT_BOX[1] * ORIENT_BOX[2] // 2})
    bx, by = defaults[(2, 4)]
    add("march_meshes", "nonsymmetric-P2-M4", 2, "dense", (se.box_mesh, ("perturbed", (bx + 1, by + 1, NZ), 2)),
        (random_table, (2, 4, 31)), "march_idx", {"kernel": "mass_march", "lz": LZ}, plan={"lz": LZ, "reoriented": 0})
    # 4. column: square Gauss tables of degree 2 P; a whole batch, a whole batch, a one-cell batch
    for p in range(1, 8):
        add("column", f"P{p}", p, "dense", (cut_mesh, (p, 2 * cells_per_batch(p) + 1)), pair_table(p, p + 1), "batch_unique",
            {"kernel": "batch", "keep_cell_order": True})
    # 5. any-rule
    def any_case(what, p, table, m, tuning=None):
        ncells = 2 * mass_dense_cells_per_batch(max(p + 1, m)) + 1
        add("any_rule", what, p, "dense", (cut_mesh, (p, ncells)), table, "mass_dense_any", dict(tuning or {}, keep_cell_order=True))
        if p <= 3:   # once more without the unique-dof tile
            add("any_rule", what + "-elementwise", p, "dense", (cut_mesh, (p, ncells)), table, "mass_dense_any",
                dict(tuning or {}, kernel="elementwise", keep_cell_order=True))
    for p in range(1, 8):
        any_case(f"P{p}-M{p + 2}", p, pair_table(p, p + 2), p + 2)
    for p in range(4, 8):
        m = npts("gll", p + 1)
        assert m < p + 1
        any_case(f"gll-P{p}-M{m}", p, pair_table(p, m), m)
    any_case("one-point-P2", 2, (oracle_table, (2, "gll_warped", "gauss_jacobi", 0)), 1)
    any_case("square-P3", 3, pair_table(3, 4), 4, {"kernel": "mass_any"})
    # 6. ordered
    for p, m in ((2, 4), (5, 6)):
        ncells = 2 * mass_dense_cells_per_batch(max(p + 1, m)) + 1
        add("ordered", f"dense-P{p}-M{m}", p, "dense", (cut_mesh, (p, ncells)), pair_table(p, m), "cells_ordered",
            {"keep_cell_order": True}, flags=("ORDERED",), twice=True)
    for p in (2, 5):
        add("ordered", f"lumped-P{p}", p, "lumped", (cut_mesh, (p, 2 * cells_per_batch(p) + 1)), None, "cells_ordered",
            {"keep_cell_order": True}, flags=("ORDERED", "MASS_ELEMENTWISE"), twice=True)
    add("ordered", "diagonal-P3", 3, "lumped", (cut_mesh, (3, 2 * cells_per_batch(3) + 1)), None, "diagonal",
        {"keep_cell_order": True}, flags=("ORDERED",), twice=True)
    # 7. lumped
    for p in range(1, 8):
        box = (se.box_mesh, ("perturbed", se.BATCH_BOX[p], p))
        cut = (cut_mesh, (p, 2 * cells_per_batch(p) + 1))
        add("lumped", f"diagonal-P{p}", p, "lumped", box, None, "diagonal")
        add("lumped", f"box-P{p}", p, "lumped", box, None, "diagonal", source="library", structured=True)
        add("lumped", f"unique-P{p}", p, "lumped", cut, None, "batch_unique", {"kernel": "batch", "keep_cell_order": True},
            flags=("MASS_ELEMENTWISE",))
        add("lumped", f"elementwise-P{p}", p, "lumped", cut, None, "elementwise", {"kernel": "elementwise", "keep_cell_order": True},
            flags=("MASS_ELEMENTWISE",))
        add("lumped", f"stair-P{p}", p, "lumped", (se.holed_mesh, (p,)), None, "diagonal", nan=True)
    # the second route of the dense family: the rule-built constructor, det J w by the library
    add("library", "march-P2-M4", 2, "dense", (se.box_mesh, ("perturbed", (8, 5, NZ), 2)), (library_table, (2,) + rule_of(2, 4)),
        "march_idx", {"kernel": "mass_march", "lz": LZ}, source="library", plan={"lz": LZ, "reoriented": 0})
    add("library", "any-P4-M6", 4, "dense", (cut_mesh, (4, 2 * mass_dense_cells_per_batch(6) + 1)),
        (library_table, (4,) + rule_of(4, 6)), "mass_dense_any", {"keep_cell_order": True}, source="library")
    return tuple(out)


NCASES = {"march_segments": 23, "march_deep": 17, "march_meshes": 9, "column": 7, "any_rule": 7 + 3 + 4 + 2 + 2,
          "ordered": 5, "lumped": 35, "library": 2}


def table_of(case):
    if case.table is None:
        return None
    maker, args = case.table
    return maker(*args)


def flag_bits(case) -> int:
    from wave_fenics_amd import _lib
    bits = 0
    for name in case.flags:
        bits |= getattr(_lib, "WF_FLAG_" + name)
    return bits


_data = {}


def data(case):
    """Everything the comparison needs for a case's mesh, table and det J source, computed once, shared by the cases
    with the same three and left unchanged: the fields (names, X, impulses), the float64 arrays the operator is created
    from (phi1, detJ: None where the library builds them), d and dbound, the references ax, mag, derr (axh, magh, derrh
    of the heterogeneous operator under the uniform field, with its coefficients a), named (the dofs a cell names) and
    the slack of the known answer sum(M 1) = sum(d)."""
    key = (case.op, case.mesh[0].__name__, case.mesh[1], None if case.table is None else (case.table[0].__name__, case.table[1]),
           case.source)
    if key not in _data:
        V, om, coords = mesh_of(case)
        t = table_of(case)
        if case.source == "tables":
            detJ, d, db = detj_tables(om, t if case.op == "dense" else lumped_rule(case.p))
        elif case.op == "dense":
            detJ, d, db = detj_library(om, t.pts, t.wts, False)
        else:
            detJ, d, db = detj_library(om, *hg.gll(case.p), True)
        names, X, impulses = se.fields(om, case.p, False, seed=29 + case.p)
        a = se.checkerboard(coords)
        if case.op == "dense":
            ax, mag, derr = reference_dense(om, case.p, t.phi1, d, db, X)
            axh, magh, derrh = reference_dense(om, case.p, t.phi1, d, db, X[:1], a)
        else:
            ax, mag, derr = reference_lumped(om, case.p, d, db, X)
            axh, magh, derrh = reference_lumped(om, case.p, d, db, X[:1], a)
        named = np.zeros(om.ndofs, dtype=bool)
        named[np.asarray(om.dofmap).reshape(-1)] = True
        _data[key] = SimpleNamespace(V=V, om=om, coords=coords, table=t, phi1=None if t is None else t.phi1, detJ=detJ, d=d,
                                     dbound=db, names=names, X=X, impulses=impulses, ax=ax, mag=mag, derr=derr, a=a,
                                     axh=axh[0], magh=magh[0], derrh=derrh[0], named=named,
                                     slack=ones_slack(None if t is None else t.phi1, d))
    return _data[key]
