"""Every operator kernel applied with x and y inside guarded buffers (tests/guard_helpers.py).

The other GPU tests hand an operator whole torch allocations: an add one row past the end of y lands in the allocator's
slack and a read in front of x[0] returns whatever lies there, and the comparison with the oracle still passes.  Here x
sits in NaN padding and y in sentinel padding, at a 16-byte and at an 8-byte aligned address (shift = 0, 1), and every
case asserts, for both alignments and both y sentinels (NEG_ZERO, MIN_NORMAL: together they see every stray store and
every stray add except an add of -0.0):

  1. all padding of x and y is bitwise unchanged;
  2. y is finite (a USED out-of-range x would be NaN);
  3. y = y0 + A x of the oracle within TOL_ORACLE = 1e-12 of max|y_ref| (the bound of every older test of these kernels);
     y0 is random at the scale of A x;
  4. y equals the same operator's y in ordinary buffers: bit for bit for the owner form and WF_FLAG_ORDERED (documented as
     pure functions of the inputs), within TOL_FORM = 1e-13 of max|y| for kernels that add with atomics;
  5. op.kernel / geometry / metric / update are what the case means to test, and the requested cross-section is the one
     that ran (the work-item count of an empty split, or plan_items).

Cross-sections (BX, BY) are read from the WF_*_SHAPES lists in csrc (guard_helpers.compiled_shapes).  The marching
shapes are the smallest with a partial column in x and in y and a last z segment shorter than the others: (BX + 1,
BY + 1, 5) cells at lz = 2.

  family              cases  cross-sections                      mesh
  march_point           12   WF_MARCH_SHAPES, P1-P4              perturbed box (BX+1, BY+1, 5)
  march_cell_full       12   the same                            sheared affine box, same shape
  march_axes_atomic     12   the same                            graded rectilinear box, update = atomic
  ksplit                11   WF_KS_SHAPES, P4 as variant 3       perturbed box (BX+1, BY+1, 5)
  owner                 48   WF_OWNER_SHAPES, P1-P7              graded box (BX+1, BY+1, 5) and the exact multiple (BX, BY, 4),
                                                                 where the last column is the closing lattice line alone;
                                                                 P4 once more with the whole apply from a run table
  box_block              7   one block per degree                perturbed box, block + 1 cells per axis (P5-P7: a block holds
                                                                 at most 7 / 5 / 4 cells, so 2 x 2 x 1)
  idx                   22   WF_IDX_SHAPES, k-split defaults     the box as a dofmap: P1-P7 per point, P1-P4 per cell full
                                                                 (sheared) and axes (graded); the holed box "stair" of
                                                                 nonbox_helpers at P1-P7 (-1 tile entries, x = NaN at the
                                                                 dofs no cell names)
  batch                 54   -                                   the first 2 B + 1 cells of a perturbed box, B the kernel's
                                                                 cells per batch (x = NaN at the dofs no cell names); P2 and
                                                                 P5 again with the numbering reversed, so that the highest
                                                                 dof belongs to the first cell
  mass_march            24   WF_MASS_SHAPES: square, Gauss       perturbed box (BX+1, BY+1, 5), lz = 2; k_mass_dense
                             2P+2, rectangular GLL               ("mass_any") once, for the rectangular pair (4, 6)
  ordered                6   -                                   the batch meshes of P2 and P5: stiffness, dense mass,
                                                                 element-wise lumped mass
  tet                    4   -                                   72 Kuhn tetrahedra, P1-P4: batches of 64, 64 + 8

  batch constants (csrc/cell_batch.h, csrc/mass_batch.hip): B = CB = 256 // (P+1)^2 cells for k_stiffness_generic_up2 (P1-P4) and _up (P5-P7)
  ("batch"), k_stiffness_generic ("elementwise"), k_mass_lumped_u and k_mass_dense_col ("batch"); B = CBd =
  min(1400 // (P+1)^3, 32) for k_mass_dense without unique-dof lists (dense mass, "elementwise"); k_mass_lumped (lumped
  mass, "elementwise") takes 256 dofmap entries per workgroup, whatever the cells.

Covered before: the tetrahedral mass runs inside padded buffers (test_gpu_tet_mass.py); wf_tsmm and the tetrahedral
stiffness at 8-byte aligned addresses (test_gpu_parity.py, test_gpu_tet_dense_paths.py).  No
stiffness or hexahedral mass kernel did.  wf_tsmm's padded buffers in test_gpu_parity.py reach the kernel's tail only;
test_gpu_tsmm_paths.py runs every path of its launch plan, the main loop included, inside padded buffers at both
alignments."""
import functools

import numpy as np
import pytest

from guard_helpers import MIN_NORMAL, NAN, NEG_ZERO, batch_pad, box_pad, compiled_shapes, guarded
from nonbox_helpers import STIFFNESS_BLOCK, holed_case
from nonbox_helpers import oracle_mesh as space_oracle_mesh
from owner_helpers import graded, spaces
from support import cells_per_batch, gpu, lattice_x, make, owner_columns  # noqa: F401
from test_gpu_dense_mass_rules import tables

pytestmark = pytest.mark.gpu

TOL_ORACLE = 1e-12   # of max|y_ref|: TOL / TOL_ORACLE of the tests of every one of these kernels
TOL_FORM = 1e-13     # of max|y|: TOL_FORM of tests/test_gpu_owner_update.py, TOL_POINT of test_gpu_affine_geometry.py
C0 = {"c0": 1500.0}
NZ, LZ = 5, 2        # layers and layers per z segment of the marching cases: segments of 2, 2 and 1 layers

MARCH_SHAPES = compiled_shapes("stiffness_march.hip", "WF_MARCH_SHAPES")           # (P, variant, BX, BY)
KS_SHAPES = compiled_shapes("stiffness_march_ks.hip", "WF_KS_SHAPES")              # (P, BX, BY)
OWNER_SHAPES = compiled_shapes("stiffness_march_owner.hip", "WF_OWNER_SHAPES")     # (P, variant, BX, BY)
MASS_SHAPES = compiled_shapes("mass_march.hip", "WF_MASS_SHAPES")                  # (P, M, BX, BY)
BLOCKS = {1: (4, 4, 4), 2: (3, 3, 3), 3: (4, 2, 2), 4: (2, 2, 2), 5: (2, 2, 1), 6: (2, 2, 1), 7: (2, 2, 1)}
BATCH_BOX = {1: (5, 5, 6), 2: (4, 4, 5), 3: (4, 3, 4), 4: (3, 3, 3), 5: (3, 3, 2), 6: (3, 2, 2), 7: (3, 3, 1)}
TET_BOX = (3, 2, 2)


def dense_cells_per_batch(p):
    """CBd of k_mass_dense without unique-dof lists (mass_dense_cells_per_batch, csrc/mass_batch.hip), square table"""
    return max(1, min(1400 // (p + 1) ** 3, 32))


def segments(nz, lz, lz0):
    return 1 + -(-max(nz - lz0, 0) // lz)


def columns(n, bx, by):
    return -(-n[0] // bx) * -(-n[1] // by)


# ---------------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------------
def run_guarded(gpu, family, what, op, x, y0, yref, pad, bitwise):
    import torch
    scale = float(np.abs(yref).max())
    xd, yp = torch.from_numpy(np.array(x)).to(gpu), torch.from_numpy(np.array(y0)).to(gpu)
    op(xd, yp)
    torch.cuda.synchronize()
    y_plain = yp.cpu().numpy()
    assert np.isfinite(y_plain).all(), (what, "plain buffers")
    worst_o = worst_p = 0.0
    for shift in (0, 1):
        for yfill in (NEG_ZERO, MIN_NORMAL):
            tag = (what, f"shift {shift}", "y padding -0.0" if yfill == 0.0 else "y padding 2^-1022")
            xg, gx = guarded(x, pad, shift, NAN, gpu)
            yg, gy = guarded(y0, pad, shift, yfill, gpu)
            op(xg, yg)
            torch.cuda.synchronize()
            assert gx.intact(), tag + ("x padding written at", gx.changed()[:8])
            assert gy.intact(), tag + ("y padding changed at", gy.changed()[:8])
            y = yg.cpu().numpy()
            assert np.isfinite(y).all(), tag + ("y not finite at", np.nonzero(~np.isfinite(y))[0][:8])
            eo = float(np.abs(y - yref).max() / scale)
            ep = float(np.abs(y - y_plain).max() / np.abs(y_plain).max())
            worst_o, worst_p = max(worst_o, eo), max(worst_p, ep)
            assert eo <= TOL_ORACLE, tag + ("oracle", eo)
            if bitwise:
                diff = np.nonzero(y.view(np.int64) != y_plain.view(np.int64))[0]
                assert diff.size == 0, tag + ("entries off the plain-buffer apply", diff.size, ep)
            else:
                assert ep <= TOL_FORM, tag + ("plain buffers", ep)
    print(f"GUARD {family} {what}: oracle {worst_o:.3e} plain {worst_p:.3e}")


def expect(op, kernel, geometry="none", metric="none", update="none"):
    assert (op.kernel, op.geometry, op.metric, op.update) == (kernel, geometry, metric, update)


# ---------------------------------------------------------------------------------------------------------------------
# references, computed once per (mesh, degree) and left unchanged
# ---------------------------------------------------------------------------------------------------------------------
def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def inputs(apply, ndofs, seed, listed=None):
    """x, y0 at the scale of A x, y0 + A x; x is NaN at the dofs no cell names"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, ndofs)
    if listed is not None:
        x[~listed] = np.nan
    ax = np.zeros(ndofs)
    apply(x, ax)
    assert np.isfinite(ax).all() and np.abs(ax).max() > 0.0
    y0 = rng.uniform(-1, 1, ndofs) * np.abs(ax).max()
    return frozen(x, y0, y0 + ax)


_boxes = {}


def stiffness_box(oracle, kind, n, p):
    """(V, x, y0, yref) of the box n: "perturbed" (per-point geometry), "sheared" (affine, full G_c), "graded"
    (rectilinear, diagonal G_c)"""
    key = (kind, n, p)
    if key not in _boxes:
        if kind == "perturbed":
            om, V = spaces(oracle, n, p, perturb=0.2)
        elif kind == "sheared":   # x += 0.25 y on a dyadic lattice, as test_gpu_affine_geometry.py
            xv = lattice_x(*[np.arange(m + 1) * 0.125 for m in n])
            xv[:, 0] += 0.25 * xv[:, 1]
            om, V = spaces(oracle, n, p, x=xv)
        else:
            om, V = graded(oracle, n, p)
        _boxes[key] = (V,) + inputs(oracle.StiffnessOperator(om, p), om.ndofs, sum(n) + p)
    return _boxes[key]


@functools.lru_cache(maxsize=None)
def batch_space(p, ncells, reverse):
    """The first ncells cells of the perturbed box BATCH_BOX[p] with the box's dof numbers (reverse: dof d renamed
    ndofs - 1 - d, so that the first cell holds the highest dof): (V, oracle mesh, listed[ndofs])."""
    import wave_fenics_amd as w
    box = w.create_box(BATCH_BOX[p], perturb=0.2)
    Vb = w.create_functionspace(box, p)
    assert ncells <= box.ncells
    dm = Vb.dofmap[:ncells].astype(np.int32)
    if reverse:
        dm = (Vb.ndofs - 1 - dm).astype(np.int32)
    mesh = w.BoxMesh(box.n, box.x, np.ascontiguousarray(box.geom_dofmap[:ncells]), box.lo, box.hi)
    V = w.FunctionSpace(mesh, p, np.ascontiguousarray(dm), w.IndexMap(Vb.ndofs), None, structured=False)
    listed = np.zeros(V.ndofs, dtype=bool)
    listed[dm.reshape(-1)] = True
    if reverse:
        assert dm[0].max() == V.ndofs - 1
    return V, space_oracle_mesh(mesh, V), listed


_batch_refs = {}


def batch_reference(oracle, kind, p, ncells, reverse):
    key = (kind, p, ncells, reverse)
    if key not in _batch_refs:
        V, om, listed = batch_space(p, ncells, reverse)
        if kind == "stiffness":
            apply = oracle.StiffnessOperator(om, p)
        elif kind == "lumped":
            apply = oracle.MassOperatorCPU(om, p)
        else:   # dense mass, Gauss rule of degree 2 P: a square table
            _, _, _, phi, detJ = tables(oracle, om, p, "gll_warped", "gauss_jacobi", 2 * p)
            apply = lambda x, y: oracle.dense_mass_apply(om, phi, detJ, x, y)   # noqa: E731
        _batch_refs[key] = (V,) + inputs(apply, om.ndofs, 100 * p + ncells, listed)
    return _batch_refs[key]


def batch_operator(kind, V, p, kernel=None, flags=0):
    import wave_fenics_amd as w
    from wave_fenics_amd._lib import WF_FLAG_MASS_ELEMENTWISE
    tuning = None if kernel is None else {"kernel": kernel, "keep_cell_order": True}
    if kind == "stiffness":
        return w.StiffnessOperator(V, p, C0, structured=False, flags=flags, tuning=tuning)
    if kind == "lumped":
        return w.MassOperatorLumped(V, p, structured=False, flags=flags | WF_FLAG_MASS_ELEMENTWISE, tuning=tuning)
    return w.MassOperator(V, p, variant="gll_warped", quad="gauss_jacobi", qdegree=2 * p, flags=flags, tuning=tuning)


def mass_rule(p, m):
    """the rule of the pair (P, M): Gauss of degree 2 P (square), Gauss of degree 2 P + 2, else Basix' GLL rule of P + 1"""
    return ("gauss_jacobi", 2 * p) if m == p + 1 else ("gauss_jacobi", 2 * p + 2) if m == p + 2 else ("gll", p + 1)


_mass_refs = {}


def mass_box(oracle, n, p, m):
    key = (n, p, m)
    if key not in _mass_refs:
        quad, qd = mass_rule(p, m)
        om, _, V = make(oracle, n, p)
        _, _, phi1, phi, detJ = tables(oracle, om, p, "gll_warped", quad, qd)
        assert phi1.shape[0] == m
        _mass_refs[key] = (V,) + inputs(lambda x, y: oracle.dense_mass_apply(om, phi, detJ, x, y), om.ndofs, sum(n) + p + m)
    return _mass_refs[key]


# ---------------------------------------------------------------------------------------------------------------------
# box marching kernels
# ---------------------------------------------------------------------------------------------------------------------
def box_case(gpu, oracle, family, what, kind, n, p, tuning, want, ncols, bitwise=False, after=None):
    import wave_fenics_amd as w
    V, x, y0, yref = stiffness_box(oracle, kind, n, p)
    op = w.StiffnessOperator(V, p, C0, structured=True, tuning=dict(tuning, lz=LZ))
    expect(op, *want)
    assert op.info.plan_lz == LZ
    if after:
        after(op)
    run_guarded(gpu, family, what, op, x, y0, yref, box_pad(V.lattice[0], V.lattice[1]), bitwise)
    # the cross-section that ran: an empty split lists every work item, columns x z segments
    assert op.set_ghost_dofs(np.zeros(0, dtype=np.int32))
    assert (op.info.items_interior, op.info.items_interface) == (ncols * segments(n[2], LZ, LZ), 0)


MARCH_FORMS = {"march_point": ("perturbed", {"geometry": "per_point"}, ("march_box", "per_point")),
               "march_cell_full": ("sheared", {"geometry": "per_cell", "metric": "full"}, ("march_box", "per_cell", "full")),
               "march_axes_atomic": ("graded", {"geometry": "per_cell", "metric": "axes", "update": "atomic"},
                                     ("march_box", "per_cell", "axes", "atomic"))}


@pytest.mark.parametrize("p,variant,bx,by", MARCH_SHAPES, ids=[f"P{s[0]}-{s[2]}x{s[3]}" for s in MARCH_SHAPES])
@pytest.mark.parametrize("family", sorted(MARCH_FORMS))
def test_box_march(gpu, oracle, family, p, variant, bx, by):
    assert len(MARCH_SHAPES) == 12
    kind, tuning, want = MARCH_FORMS[family]
    n = (bx + 1, by + 1, NZ)
    box_case(gpu, oracle, family, f"P{p} {bx}x{by} {n}", kind, n, p, dict(tuning, variant=variant), want, columns(n, bx, by))


@pytest.mark.parametrize("p,bx,by", KS_SHAPES, ids=[f"P{s[0]}-{s[1]}x{s[2]}" for s in KS_SHAPES])
def test_box_ksplit(gpu, oracle, p, bx, by):
    assert len(KS_SHAPES) == 11
    n = (bx + 1, by + 1, NZ)
    tuning = {"block": (bx, by, 1)}
    if p == 4:
        tuning["variant"] = 3     # the k-split kernel at P4 (P >= 5: the default)
    box_case(gpu, oracle, "ksplit", f"P{p} {bx}x{by} {n}", "perturbed", n, p, tuning, ("march_box", "per_point"), columns(n, bx, by))


def with_run_table(op, ncols, nz):
    """the whole apply from a run table: planned for 8 workgroups, or (where that plan is the uniform one) every column
    cut after its first layer"""
    op.replan_runs(8)
    if len(op.runs()) == 0:
        op.set_runs(np.array([(c, a, b) for a, b in ((0, 1), (1, nz)) for c in range(ncols)], dtype=np.int32))
    assert len(op.runs()) > 0


OWNER_CASES = [(p, v, bx, by, exact, table) for p, v, bx, by in OWNER_SHAPES for exact in (False, True)
               for table in ((False, True) if p == 4 else (False,))]


@pytest.mark.parametrize("p,variant,bx,by,exact,table", OWNER_CASES,
                         ids=[f"P{c[0]}-{c[2]}x{c[3]}-{'exact' if c[4] else 'partial'}{'-table' if c[5] else ''}" for c in OWNER_CASES])
def test_box_owner(gpu, oracle, p, variant, bx, by, exact, table):
    import wave_fenics_amd as w
    assert len(OWNER_SHAPES) == 21
    n = (bx, by, NZ - 1) if exact else (bx + 1, by + 1, NZ)
    ncols = owner_columns(n, p, bx, by)
    # exact: 2 x 2 columns, the closing lattice line a column of its own; partial: one cell more than a column holds
    # (P + 1 lines: a third column where the column is one cell wide)
    assert ncols == (4 if exact else (3 if bx == 1 else 2) * (3 if by == 1 else 2))
    V, x, y0, yref = stiffness_box(oracle, "graded", n, p)
    op = w.StiffnessOperator(V, p, C0, structured=True, tuning={"update": "owner", "variant": variant, "lz": LZ})
    expect(op, "march_box", "per_cell", "axes", "owner")
    assert op.info.plan_lz == LZ and len(op.runs()) == 0
    if table:
        with_run_table(op, ncols, n[2])
    run_guarded(gpu, "owner", f"P{p} {bx}x{by} {n}{' run table' if table else ''}", op, x, y0, yref,
                box_pad(V.lattice[0], V.lattice[1]), bitwise=True)
    assert op.set_ghost_dofs(np.zeros(0, dtype=np.int32))
    assert (op.info.items_interior, op.info.items_interface) == (ncols * segments(n[2], LZ, LZ), 0)


@pytest.mark.parametrize("p", sorted(BLOCKS))
def test_box_block(gpu, oracle, p):
    import wave_fenics_amd as w
    block = BLOCKS[p]
    assert block[0] * block[1] * block[2] * (p + 1) ** 2 <= 256
    n = tuple(b + 1 for b in block)       # the block divides none of nx, ny (and nz, where a block has two layers)
    V, x, y0, yref = stiffness_box(oracle, "perturbed", n, p)
    op = w.StiffnessOperator(V, p, C0, structured=True, tuning={"kernel": "box_block", "block": block})
    expect(op, "box_block", "per_point")
    run_guarded(gpu, "box_block", f"P{p} block {block} {n}", op, x, y0, yref, box_pad(V.lattice[0], V.lattice[1]), False)


# ---------------------------------------------------------------------------------------------------------------------
# dofmap marching kernels
# ---------------------------------------------------------------------------------------------------------------------
IDX_FORMS = {"point": ("perturbed", {}, ("march_idx", "per_point")),
             "cell_full": ("sheared", {"geometry": "per_cell", "metric": "full"}, ("march_idx", "per_cell", "full")),
             "cell_axes": ("graded", {"geometry": "per_cell", "metric": "axes"}, ("march_idx", "per_cell", "axes", "atomic"))}
IDX_CASES = [("point", p) for p in range(1, 8)] + [(f, p) for f in ("cell_full", "cell_axes") for p in range(1, 5)]


@pytest.mark.parametrize("form,p", IDX_CASES, ids=[f"{f}-P{p}" for f, p in IDX_CASES])
def test_dofmap_march_box(gpu, oracle, form, p):
    """the box as a dofmap: k_march_idx at P <= 4 (WF_IDX_SHAPES), the k-split kernel's dofmap form at P >= 5"""
    import wave_fenics_amd as w
    if p <= 4:
        assert (p,) + STIFFNESS_BLOCK[p] in compiled_shapes("stiffness_march_idx.hip", "WF_IDX_SHAPES")
    else:
        assert (p,) + STIFFNESS_BLOCK[p] == next(s for s in KS_SHAPES if s[0] == p)
    bx, by = STIFFNESS_BLOCK[p]
    n = (bx + 1, by + 1, NZ)
    kind, tuning, want = IDX_FORMS[form]
    V, x, y0, yref = stiffness_box(oracle, kind, n, p)
    op = w.StiffnessOperator(V, p, C0, structured=False, tuning=dict(tuning, kernel="march", lz=LZ))
    expect(op, *want)
    assert (op.info.plan_lz, op.info.plan_items) == (LZ, columns(n, bx, by) * -(-NZ // LZ))
    run_guarded(gpu, "idx", f"{form} P{p} {bx}x{by} {n}", op, x, y0, yref, box_pad(V.lattice[0], V.lattice[1]), False)


_holed = {}


@pytest.mark.parametrize("p", range(1, 8))
def test_dofmap_march_holed(gpu, oracle, p):
    """the "stair" of nonbox_helpers (every stack of cells starts one layer later than its x neighbour): tile positions
    no cell covers (-1 pattern entries) at every cross-section, dofs no cell names"""
    import wave_fenics_amd as w
    case = holed_case("stair", p)
    if p not in _holed:
        _holed[p] = inputs(oracle.StiffnessOperator(case.om, p), case.V.ndofs, 40 + p, case.listed)
    x, y0, yref = _holed[p]
    assert not case.listed.all()
    op = w.StiffnessOperator(case.V, p, C0, structured=False, tuning={"kernel": "march", "lz": LZ})
    expect(op, "march_idx", "per_point")
    assert 0.0 < op.info.plan_fill < 1.0 and op.info.plan_lz == LZ
    nx, ny, _ = case.mesh.n
    run_guarded(gpu, "idx", f"holed stair P{p}", op, x, y0, yref, box_pad(p * nx + 1, p * ny + 1), False)


# ---------------------------------------------------------------------------------------------------------------------
# batch kernels
# ---------------------------------------------------------------------------------------------------------------------
BATCH_KERNELS = [("stiffness", "batch", "batch_unique", "per_point"), ("stiffness", "elementwise", "elementwise", "per_point"),
                 ("lumped", "batch", "batch_unique", "none"), ("lumped", "elementwise", "elementwise", "none"),
                 ("dense", "batch", "batch_unique", "none"), ("dense", "elementwise", "mass_dense_any", "none")]
BATCH_CASES = [(p, False) for p in range(1, 8)] + [(2, True), (5, True)]


@pytest.mark.parametrize("kind,hint,kernel,geometry", BATCH_KERNELS, ids=[f"{k[0]}-{k[1]}" for k in BATCH_KERNELS])
@pytest.mark.parametrize("p,reverse", BATCH_CASES, ids=[f"P{p}{'-reversed' if r else ''}" for p, r in BATCH_CASES])
def test_batch_kernels(gpu, oracle, p, reverse, kind, hint, kernel, geometry):
    """ncells = 2 B + 1 for the kernel's cells per batch B: two full batches and one of a single cell.  (k_mass_lumped
    works on 256 dofmap entries per workgroup, whatever the cells: its last workgroup is partial at every degree but P7,
    where a cell is two workgroups.)"""
    cb = dense_cells_per_batch(p) if (kind, hint) == ("dense", "elementwise") else cells_per_batch(p)
    ncells = 2 * cb + 1
    V, x, y0, yref = batch_reference(oracle, kind, p, ncells, reverse)
    op = batch_operator(kind, V, p, hint)
    expect(op, kernel, geometry)
    assert op.num_cells() == ncells and ncells % cb == 1
    run_guarded(gpu, "batch", f"{kind} {hint} P{p} {ncells} cells{' reversed numbering' if reverse else ''}", op, x, y0, yref,
                batch_pad((p + 1) ** 3), False)


@pytest.mark.parametrize("kind", ["stiffness", "dense", "lumped"])
@pytest.mark.parametrize("p", [2, 5])
def test_ordered(gpu, oracle, p, kind):
    from wave_fenics_amd._lib import WF_FLAG_ORDERED
    ncells = 2 * cells_per_batch(p) + 1
    V, x, y0, yref = batch_reference(oracle, kind, p, ncells, False)
    op = batch_operator(kind, V, p, flags=WF_FLAG_ORDERED)
    expect(op, "cells_ordered", "per_point" if kind == "stiffness" else "none", "none", "ordered")
    run_guarded(gpu, "ordered", f"{kind} P{p} {ncells} cells", op, x, y0, yref, batch_pad((p + 1) ** 3), bitwise=True)


# ---------------------------------------------------------------------------------------------------------------------
# dense mass on lattice columns
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,m,bx,by", MASS_SHAPES, ids=[f"P{s[0]}-M{s[1]}-{s[2]}x{s[3]}" for s in MASS_SHAPES])
def test_mass_march(gpu, oracle, p, m, bx, by):
    import wave_fenics_amd as w
    assert len(MASS_SHAPES) == 23
    n = (bx + 1, by + 1, NZ)
    quad, qd = mass_rule(p, m)
    V, x, y0, yref = mass_box(oracle, n, p, m)
    op = w.MassOperator(V, p, variant="gll_warped", quad=quad, qdegree=qd,
                        tuning={"kernel": "mass_march", "block": (bx, by, 0), "lz": LZ})
    expect(op, "march_idx")
    assert op.num_quads() == m ** 3
    assert (op.info.plan_lz, op.info.plan_items) == (LZ, columns(n, bx, by) * -(-NZ // LZ))
    run_guarded(gpu, "mass_march", f"P{p} M{m} {bx}x{by} {n}", op, x, y0, yref, box_pad(V.lattice[0], V.lattice[1]), False)


def test_mass_any_rectangular(gpu, oracle):
    """k_mass_dense with a rectangular table, (P, M) = (4, 6), on the marching case's box"""
    import wave_fenics_amd as w
    p, m = 4, 6
    bx, by = next(s[2:] for s in MASS_SHAPES if s[:2] == (p, m))
    n = (bx + 1, by + 1, NZ)
    quad, qd = mass_rule(p, m)
    V, x, y0, yref = mass_box(oracle, n, p, m)
    op = w.MassOperator(V, p, variant="gll_warped", quad=quad, qdegree=qd, tuning={"kernel": "mass_any"})
    expect(op, "mass_dense_any")
    assert op.num_quads() == m ** 3
    run_guarded(gpu, "mass_march", f"mass_any P{p} M{m} {n}", op, x, y0, yref, box_pad(V.lattice[0], V.lattice[1]), False)


# ---------------------------------------------------------------------------------------------------------------------
# tetrahedral MFMA stiffness (the tetrahedral mass has this check in tests/test_gpu_tet_mass.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_tet_stiffness(gpu, oracle, p):
    from oracle import tet_oracle
    from wave_fenics_amd import tet
    om = tet_oracle.create_kuhn_box(TET_BOX, p, perturb=0.2)
    V = tet.create_kuhn_box(TET_BOX, p, perturb=0.2)
    assert np.array_equal(V.dofmap, om.dofmap) and np.array_equal(V.geom_dofmap, om.geom_dofmap)
    assert V.ncells > 64 and V.ncells % 64 != 0      # 64-cell batches: the last one is partial
    x, y0, yref = inputs(tet_oracle.TetStiffnessOperator(om, p), om.ndofs, 70 + p)
    op = tet.TetStiffnessOperator(V, p, C0)
    expect(op, "dense_simplex", "per_cell")
    run_guarded(gpu, "tet", f"P{p} {V.ncells} cells", op, x, y0, yref, batch_pad(V.dofmap.shape[1]), False)


# ---------------------------------------------------------------------------------------------------------------------
# the helper itself
# ---------------------------------------------------------------------------------------------------------------------
def test_guard_helper_detects_what_it_says(gpu):
    """Plain in-bounds torch operations on the padding: a store, += 0.0, += -0.0 and += 1e-300 are reported or missed by
    each y sentinel exactly as guard_helpers says; the NaN padding of x reports a store."""
    import torch
    n, pad = 37, 4096
    values = np.random.default_rng(0).uniform(-1, 1, n)
    assert np.array([NEG_ZERO]).view(np.int64)[0] == np.int64(-2 ** 63) and MIN_NORMAL == np.finfo(np.float64).tiny
    reported = {}
    for fill in (NEG_ZERO, MIN_NORMAL, NAN):
        for shift in (0, 1):
            view, g = guarded(values, pad, shift, fill, gpu)
            assert view.data_ptr() % 16 == 8 * shift and view.data_ptr() % 8 == 0
            assert np.array_equal(view.cpu().numpy(), values) and g.intact()
            view += 1.0           # in-bounds work on the data is never reported
            assert g.intact()
        for name, act in (("store", lambda t: t.fill_(fill)), ("store other", lambda t: t.fill_(3.0)),
                          ("add +0.0", lambda t: t.add_(0.0)), ("add -0.0", lambda t: t.add_(-0.0)),
                          ("add 1e-300", lambda t: t.add_(1e-300))):
            for where in (-1, n, -pad, n + pad - 1):     # next to the data and at both ends of the allocation
                view, g = guarded(values, pad, 0, fill, gpu)
                at = g.lo + where
                act(g.buf[at:at + 1])
                torch.cuda.synchronize()
                hit = g.changed()
                assert hit.size in (0, 1) and (hit.size == 0 or hit[0] == where), (fill, name, where, hit)
                reported.setdefault((fill if fill == fill else "nan", name), set()).add(bool(hit.size))
    got = {k: v for k, v in reported.items()}
    assert all(len(v) == 1 for v in got.values()), got
    seen = {k: next(iter(v)) for k, v in got.items()}
    # a store of the sentinel's own bits is no change; any other store is
    for fill in (NEG_ZERO, MIN_NORMAL, "nan"):
        assert seen[(fill, "store")] is False and seen[(fill, "store other")] is True
    assert (seen[(NEG_ZERO, "add +0.0")], seen[(NEG_ZERO, "add -0.0")], seen[(NEG_ZERO, "add 1e-300")]) == (True, False, True)
    assert (seen[(MIN_NORMAL, "add +0.0")], seen[(MIN_NORMAL, "add -0.0")], seen[(MIN_NORMAL, "add 1e-300")]) == (False, False, True)
    # why y is never padded with NaN: an add keeps its bits
    assert (seen[("nan", "add +0.0")], seen[("nan", "add 1e-300")]) == (False, False)
