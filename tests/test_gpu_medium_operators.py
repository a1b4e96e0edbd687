"""Cell coefficients on every operator path, on the GPU: parity against the oracle fed with scaled geometry
(tests/medium_helpers.py; TOL = 1e-12 of max|y_ref|, TOL_FORM = 1e-13 between two forms of one sum), on every coefficient
field, with the kernel path of every case asserted and compared with the operator created without a coefficient.

The set-up writes the geometry in an internal order -- blocked box layouts with partial blocks, batches after the sort
by smallest dof, lattice-plan slots after re-orientation -- and the multiply by a_c has to follow the cell through it:
the `distinct` field (all cells differ) shows a permuted array, the `slab` a shifted block, `zeros` a read of a wrong
slot's value into a cell that must contribute nothing."""
import numpy as np
import pytest

import medium_helpers as mh
from medium_helpers import TOL, TOL_FORM, bits, relerr
from support import dev, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

ORDERED, ELEMENTWISE, NO_FABS, NO_CLAMP = 16, 4, 1, 2


def applied(op, x, gpu, y0=None):
    """y0 + A x (y0 = None: zeros) as a numpy array"""
    import torch
    y = dev(np.zeros_like(x) if y0 is None else y0, gpu)
    op(dev(x, gpu), y)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def fields_of(case):
    return [(f, mh.field(f, case.mesh.x, case.mesh.geom_dofmap)) for f in mh.FIELDS]


def check_stiffness(case, gpu, make=None, after=None, tag=""):
    """parity of a stiffness case on every field; the path asserted, and equal to the operator's without a coefficient"""
    make = make or (lambda a: mh.make_stiffness(case, a))
    plain = make(None)
    after and after(plain)
    assert mh.path_of(plain) == case.want and not plain.cell_coeff, (case.name, mh.path_of(plain))
    x, r = mh.vectors(case.V.ndofs)
    for f, a in fields_of(case):
        op = make(a)
        after and after(op)
        assert op.cell_coeff and mh.selection_of(op) == mh.selection_of(plain), (case.name, f, mh.selection_of(op), mh.selection_of(plain))
        kx = mh.stiffness_reference(case, a, x)
        y0 = r * np.abs(kx).max()                      # accumulate semantics: y += K x
        err = relerr(applied(op, x, gpu, y0), y0 + kx)
        print(f"MEDIUM stiffness {case.name}{tag} {f} {mh.path_of(op)}: {err:.3e}")
        assert err <= TOL, (case.name, tag, f, err)


# ---------------------------------------------------------------------------------------------------------------------
# stiffness: every family, box and dofmap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mh.STIFFNESS_CASES)
def test_stiffness_parity(gpu, oracle, name):
    check_stiffness(mh.stiffness_case(name), gpu)


def test_owner_with_run_table(gpu, oracle):
    """the P4 owner form by a run table.  wf_op_replan_runs with a small number of resident workgroups plans one where
    the model finds a cheaper plan than the uniform z segments: on the 2 x 5 columns of (9, 9, 7) with 8 resident.  The
    four columns of (9, 3, 7) never get one that way, so there a table of the caller's is installed (wf_op_set_runs):
    uneven cuts, columns in reverse order."""
    def replanned(op):
        op.replan_runs(8)
        assert op.runs().shape[0] == 16

    check_stiffness(mh.stiffness_case("owner-P4-wide"), gpu, after=replanned, tag=" replan_runs(8)")

    def own_table(op):
        cuts = [0, 1, 4, 6, 7]
        op.set_runs(np.array([(c, a, b) for a, b in zip(cuts[:-1], cuts[1:]) for c in reversed(range(4))], dtype=np.int32))
        assert op.runs().shape[0] == 16

    check_stiffness(mh.stiffness_case("owner-P4"), gpu, after=own_table, tag=" set_runs")


def test_owner_interior_interface_split(gpu, oracle):
    """set_ghost_faces(1, 1, 1) on the P4 owner form: INTERIOR + INTERFACE is the whole apply to TOL_FORM, and every
    y entry belongs to one part -- the owner form's items own lattice nodes -- which carries the reference's value
    there while the other part leaves it alone."""
    from wave_fenics_amd._lib import WF_PART_INTERFACE, WF_PART_INTERIOR
    import torch
    case = mh.stiffness_case("owner-P4")
    x, _ = mh.vectors(case.V.ndofs)
    for f, a in fields_of(case):
        op = mh.make_stiffness(case, a)
        assert op.set_ghost_faces(True, True, True) and mh.path_of(op) == case.want
        assert op.info.items_interior > 0 and op.info.items_interface > 0
        whole = applied(op, x, gpu)
        parts = {}
        for part in (WF_PART_INTERIOR, WF_PART_INTERFACE):
            y = dev(np.zeros_like(x), gpu)
            op.apply_part(dev(x, gpu), y, part)
            torch.cuda.synchronize()
            parts[part] = y.cpu().numpy()
        yi, yf = parts[WF_PART_INTERIOR], parts[WF_PART_INTERFACE]
        assert relerr(yi + yf, whole) <= TOL_FORM, (f, relerr(yi + yf, whole))
        kx = mh.stiffness_reference(case, a, x)
        scale = np.abs(kx).max()
        owned_i, owned_f = bits(yi) != bits(np.zeros_like(yi)), bits(yf) != bits(np.zeros_like(yf))
        assert not (owned_i & owned_f).any(), (f, "a y entry written by both parts")
        assert np.abs(np.where(owned_f, 0.0, yi - kx)).max() <= TOL * scale      # the interior's entries: the reference
        assert np.abs(np.where(owned_i, 0.0, yf - kx)).max() <= TOL * scale      # the interface's
        assert np.abs(kx[~(owned_i | owned_f)]).max(initial=0.0) <= TOL * scale  # nobody's: the reference is zero there


# ---------------------------------------------------------------------------------------------------------------------
# lumped mass
# ---------------------------------------------------------------------------------------------------------------------
LUMPED = [("box", True, 0, {}, "diagonal"), ("dofmap", False, 0, {}, "diagonal"),
          ("dofmap", False, ELEMENTWISE, {}, "batch_unique"), ("dofmap", False, ELEMENTWISE, {"kernel": "elementwise"}, "elementwise"),
          ("shuffled", False, 0, {}, "diagonal"), ("shuffled", False, ELEMENTWISE, {}, "batch_unique")]


@pytest.mark.parametrize("mesh_kind,structured,flags,tuning,want", LUMPED, ids=[f"{m}-{k}" for m, _, _, _, k in LUMPED])
def test_lumped_mass(gpu, oracle, mesh_kind, structured, flags, tuning, want):
    """diagonal, element-wise and batch-unique forms, box and dofmap (more than one batch; `shuffled`: the pillar mesh
    in a random cell order, whose batches are sorted); known answer sum(M[a] 1) = sum_c a_c vol_c"""
    import wave_fenics_amd as w
    p = 2
    case = mh.stiffness_case("batch-P2" if mesh_kind == "shuffled" else "point-P2")
    V = case.V if structured or mesh_kind == "shuffled" else w.FunctionSpace(case.mesh, p, case.V.dofmap, case.V.index_map,
                                                                             case.V.lattice, structured=False)
    plain = w.MassOperatorLumped(V, p, structured=structured, flags=flags, tuning=tuning or None)
    assert plain.kernel == want and not plain.cell_coeff
    x, r = mh.vectors(V.ndofs)
    vol = mh.cell_volumes(case.om, p)
    listed = np.zeros(V.ndofs, dtype=bool)
    listed[V.dofmap.reshape(-1)] = True
    for f, a in fields_of(case):
        op = w.MassOperatorLumped(V, p, structured=structured, flags=flags, tuning=tuning or None, cell_coeff=a)
        assert op.cell_coeff and mh.selection_of(op) == mh.selection_of(plain)
        mx = mh.lumped_reference(case.om, p, a, x)
        y0 = r * np.abs(mx).max()
        err = relerr(applied(op, x, gpu, y0)[listed], (y0 + mx)[listed])
        total = applied(op, np.ones(V.ndofs), gpu)[listed].sum()
        print(f"MEDIUM lumped {mesh_kind} {op.kernel} {f}: {err:.3e}, sum {total:.15e} vs {np.dot(a, vol):.15e}")
        assert err <= TOL, (mesh_kind, want, f, err)
        assert abs(total - np.dot(a, vol)) <= TOL * np.dot(np.abs(a), vol), (f, total, np.dot(a, vol))


# ---------------------------------------------------------------------------------------------------------------------
# dense mass
# ---------------------------------------------------------------------------------------------------------------------
DENSE = [("march-P2", 2, 4, {}, "march_idx"), ("march-P4", 4, 8, {}, "march_idx"),
         ("march-rect-4-6", 4, 10, {"kernel": "mass_march"}, "march_idx"), ("column-P2", 2, 4, {"kernel": "batch"}, "batch_unique"),
         ("any-P2", 2, 6, {}, "mass_dense_any")]


@pytest.mark.parametrize("name,p,qd,tuning,want", DENSE, ids=[d[0] for d in DENSE])
def test_dense_mass(gpu, oracle, name, p, qd, tuning, want):
    """mass_march square (P2, P4) and rectangular (4, 6), mass_column, mass_any with a rectangular rule and no hint;
    Gauss rule of degree qd on equispaced Lagrange, det J w computed from the mesh"""
    import wave_fenics_amd as w
    case = mh.stiffness_case("point-P2" if p == 2 else "point-P4")
    V = w.FunctionSpace(case.mesh, p, case.V.dofmap, case.V.index_map, case.V.lattice, structured=False)
    make = lambda a: w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=qd, tuning=tuning or None, cell_coeff=a)
    plain = make(None)
    assert plain.kernel == want and plain.num_quads() == ((qd + 2) // 2) ** 3
    x, r = mh.vectors(V.ndofs)
    for f, a in fields_of(case):
        op = make(a)
        assert op.cell_coeff and mh.selection_of(op) == mh.selection_of(plain)
        mx = mh.dense_mass_reference(case.om, p, qd, a, x)
        y0 = r * np.abs(mx).max()
        err = relerr(applied(op, x, gpu, y0), y0 + mx)
        print(f"MEDIUM dense mass {name} {op.kernel} {f}: {err:.3e}")
        assert err <= TOL, (name, f, err)


def test_dense_mass_given_detJ(gpu, oracle):
    """the caller's own h_detJ is scaled the same way (plan and batches)"""
    import wave_fenics_amd as w
    p, qd = 2, 4
    case = mh.stiffness_case("point-P2")
    V = w.FunctionSpace(case.mesh, p, case.V.dofmap, case.V.index_map, case.V.lattice, structured=False)
    phi1, _, X, W = mh.nh.dense_tables(p, qd)
    detJ = oracle.compute_detJ_generic(case.om, X, W)
    x, _ = mh.vectors(V.ndofs)
    for tuning, want in (({}, "march_idx"), ({"kernel": "batch"}, "batch_unique")):
        for f, a in fields_of(case):
            op = w.MassOperator(V, p, phi1=phi1, detJ=detJ, tuning=tuning or None, cell_coeff=a)
            assert op.kernel == want and op.cell_coeff
            err = relerr(applied(op, x, gpu), mh.dense_mass_reference(case.om, p, qd, a, x))
            assert err <= TOL, (want, f, err)


# ---------------------------------------------------------------------------------------------------------------------
# WF_FLAG_ORDERED: y a pure function of the inputs, the coefficient one of them
# ---------------------------------------------------------------------------------------------------------------------
ORDERED_CASES = [("stiffness", True), ("stiffness", False), ("lumped", True), ("lumped", False), ("dense", False)]   # the dense mass has no box entry point


@pytest.mark.parametrize("kind,structured", ORDERED_CASES, ids=[f"{k}-{'box' if s else 'dofmap'}" for k, s in ORDERED_CASES])
def test_ordered(gpu, oracle, kind, structured):
    """parity; two applies bitwise equal; two dof numberings give y bitwise equal up to the relabelling"""
    import wave_fenics_amd as w
    p, qd = 2, 6
    case = mh.stiffness_case("point-P2")
    Vs = case.V
    Vd = w.FunctionSpace(case.mesh, p, Vs.dofmap, Vs.index_map, Vs.lattice, structured=False)
    new = np.random.default_rng(8).permutation(Vs.ndofs).astype(np.int32)
    Vr = w.renumber(Vd, new)

    def make(V, a, box):
        if kind == "stiffness":
            return w.StiffnessOperator(V, p, {"c0": mh.C0}, structured=box, flags=ORDERED, cell_coeff=a)
        if kind == "lumped":
            return w.MassOperatorLumped(V, p, structured=box, flags=ORDERED | ELEMENTWISE, cell_coeff=a)
        return w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=qd, flags=ORDERED, cell_coeff=a)

    x, _ = mh.vectors(Vs.ndofs)
    xr = np.zeros_like(x)
    xr[new] = x
    for f, a in fields_of(case):
        op = make(Vs if structured else Vd, a, structured)
        assert op.kernel == "cells_ordered" and op.update == "ordered" and op.cell_coeff
        ref = (mh.stiffness_reference(case, a, x) if kind == "stiffness" else mh.lumped_reference(case.om, p, a, x)
               if kind == "lumped" else mh.dense_mass_reference(case.om, p, qd, a, x))
        y1, y2 = applied(op, x, gpu), applied(op, x, gpu)
        assert relerr(y1, ref) <= TOL, (kind, f, relerr(y1, ref))
        assert np.array_equal(bits(y1), bits(y2)), (kind, f, "two applies differ")
        yr = applied(make(Vr, a, False), xr, gpu)
        assert np.array_equal(bits(yr[new]), bits(y1)), (kind, f, "the renumbered operator differs")


# ---------------------------------------------------------------------------------------------------------------------
# tetrahedra
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_kuhn():
    """a perturbed Kuhn box of 33 048 cells per degree: 517 batches of 64 -- more than the persistent grid of 512
    workgroups -- the last one partial (24 cells).  The oracle operator is built once per degree and shared."""
    cache = {}

    def get(p):
        if p not in cache:
            from oracle import tet_oracle as to
            V, om = mh.tet_meshes((18, 18, 17), p)
            assert V.ncells == 33048 and -(-V.ncells // 64) == 517 and V.ncells % 64 == 24
            cache[p] = (V, to.TetStiffnessOperator(om, p, c0=mh.C0))
        return cache[p]
    return get


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_tet_stiffness(gpu, oracle, big_kuhn, p):
    from wave_fenics_amd import tet
    V, top = big_kuhn(p)
    plain = tet.TetStiffnessOperator(V, p, {"c0": mh.C0})
    assert plain.kernel == "dense_simplex" and not plain.cell_coeff
    x, r = mh.vectors(V.ndofs)
    for f in mh.FIELDS:
        a = mh.field(f, V.x, V.geom_dofmap)
        op = tet.TetStiffnessOperator(V, p, {"c0": mh.C0}, cell_coeff=a)
        assert op.cell_coeff and mh.path_of(op) == mh.path_of(plain)
        assert op.info.alg_bytes == plain.info.alg_bytes + 8.0 * V.ncells          # the one array the coefficient adds
        kx = mh.tet_stiffness_reference(top, a, x)
        y0 = r * np.abs(kx).max()
        err = relerr(applied(op, x, gpu, y0), y0 + kx)
        print(f"MEDIUM tet stiffness P{p} {f}: {err:.3e}")
        assert err <= TOL, (p, f, err)


@pytest.mark.parametrize("flags", [0, NO_CLAMP], ids=["clamp", "no-clamp"])
def test_tet_stiffness_clamp_hit(gpu, oracle, flags):
    """a batch in which the -1/0/1 clamp takes effect (the unperturbed Kuhn box scaled so that its largest w_q C_e is
    1 + 3e-6): the coefficient is applied AFTER the clamp, so the reference is clamp(G) * a, and G * a under
    WF_FLAG_NO_CLAMP; the two references differ by 3e-6, far above the bound"""
    from oracle import tet_oracle as to
    from wave_fenics_amd import tet
    p, n = 4, (3, 2, 2)
    V, om = mh.tet_meshes(n, p, perturb=0.0, scale=mh.tet_clamp_scale(n, p))
    top = to.TetStiffnessOperator(om, p, c0=mh.C0)
    assert np.abs(top.G - mh.tet_unclamped_G(top)).max() > 1e-6          # the clamp acts on this mesh
    x, _ = mh.vectors(V.ndofs)
    for f in mh.FIELDS:
        a = mh.field(f, V.x, V.geom_dofmap)
        op = tet.TetStiffnessOperator(V, p, {"c0": mh.C0}, flags=flags, cell_coeff=a)
        ref = mh.tet_stiffness_reference(top, a, x, clamp=not flags)
        other = mh.tet_stiffness_reference(top, a, x, clamp=bool(flags))
        err = relerr(applied(op, x, gpu), ref)
        print(f"MEDIUM tet clamp hit flags {flags} {f}: {err:.3e} (other reference {relerr(other, ref):.3e})")
        assert relerr(other, ref) > 1e3 * TOL
        assert err <= TOL, (flags, f, err)


@pytest.mark.parametrize("flags", [0, NO_FABS], ids=["fabs", "no-fabs"])
@pytest.mark.parametrize("p", [2, 4])
def test_tet_mass(gpu, oracle, p, flags):
    from wave_fenics_amd import tet
    V, _ = mh.tet_meshes((5, 4, 3), p)          # 360 cells: six batches, the last partial
    plain = tet.TetMassOperator(V, p, flags=flags)
    assert plain.kernel == "dense_simplex_mass"
    x, r = mh.vectors(V.ndofs)
    for f in mh.FIELDS:
        a = mh.field(f, V.x, V.geom_dofmap)
        op = tet.TetMassOperator(V, p, flags=flags, cell_coeff=a)
        assert op.cell_coeff and mh.selection_of(op) == mh.selection_of(plain)
        mx = mh.tet_mass_reference(V, p, a, x, use_fabs=not flags)
        y0 = r * np.abs(mx).max()
        err = relerr(applied(op, x, gpu, y0), y0 + mx)
        print(f"MEDIUM tet mass P{p} flags {flags} {f}: {err:.3e}")
        assert err <= TOL, (p, flags, f, err)


# ---------------------------------------------------------------------------------------------------------------------
# properties, on every family at one degree
# ---------------------------------------------------------------------------------------------------------------------
FIXED_ORDER = ("owner-P4", "owner-P2")      # + the ordered operators and the diagonal, below
PROPERTY_CASES = ("owner-P4", "owner-P2", "point-P4", "cell-full-P3", "axes-atomic-P3", "box-block-P2", "ksplit-P5",
                  "reoriented-point-P2", "reoriented-full-P3", "reoriented-axes-P3", "batch-P2", "elementwise-P2")


def check_properties(make, x_verts, geom_dofmap, dofmap, ndofs, gpu, fixed, stiffness, what):
    """The five properties of one family; make(a) creates its operator with cell_coeff = a (None: without).
      1. a = 1 reproduces the operator without a coefficient: bitwise where the summation order is fixed, else TOL_FORM;
      2. a = 2 gives 2 y: exactly where the order is fixed, else TOL_FORM;
      3. stiffness only: K[a] const = 0 to TOL of max|a_c| max|K[1] x_random| (constants are in the kernel of every
         cell matrix);
      4. x^T A[a] z = z^T A[a] x, to TOL max|A x| per entry of the two sums;
      5. a dof touched only by zero-coefficient cells keeps its y bitwise (the slab field with its lower value 0)."""
    nc = np.asarray(geom_dofmap).shape[0]
    x, z = mh.vectors(ndofs, seed=77)
    y_plain = applied(make(None), x, gpu)
    y_one, y_two = applied(make(np.ones(nc)), x, gpu), applied(make(np.full(nc, 2.0)), x, gpu)
    if fixed:
        assert np.array_equal(bits(y_one), bits(y_plain)), (what, "a = 1 is not the operator without a coefficient")
        assert np.array_equal(bits(y_two), bits(2.0 * y_plain)), (what, "a = 2 is not exactly 2 y")
    else:
        assert relerr(y_one, y_plain) <= TOL_FORM and relerr(y_two, 2.0 * y_plain) <= TOL_FORM, (what, relerr(y_one, y_plain))
    a = mh.field("distinct", x_verts, geom_dofmap)
    op = make(a)
    if stiffness:
        yc = applied(op, np.full(ndofs, 0.75), gpu)
        assert np.abs(yc).max() <= TOL * np.abs(a).max() * np.abs(y_plain).max(), (what, "K[a] const", np.abs(yc).max())
    ax, az = applied(op, x, gpu), applied(op, z, gpu)
    assert abs(np.dot(z, ax) - np.dot(x, az)) <= TOL * np.abs(ax).max() * ndofs, (what, "symmetry")
    a0 = mh.field("slab", x_verts, geom_dofmap)
    a0[a0 == 1.0] = 0.0
    live = np.zeros(ndofs, dtype=bool)
    live[np.asarray(dofmap)[a0 != 0.0].reshape(-1)] = True
    dead = ~live
    dead[np.setdiff1d(np.arange(ndofs), np.asarray(dofmap).reshape(-1))] = False     # dofs no cell names are not the point
    assert dead.any() and live.any(), what
    y0 = mh.vectors(ndofs, seed=5)[1] * np.abs(y_plain).max()
    got = applied(make(a0), x, gpu, y0)
    assert np.array_equal(bits(got[dead]), bits(y0[dead])), (what, "a dof of zero-coefficient cells changed")
    assert not np.array_equal(bits(got[live]), bits(y0[live])), what
    return x, a0, y0, got


def props_of_case(case, make, gpu, fixed, stiffness, what, V=None):
    V = V or case.V
    return check_properties(make, case.mesh.x, case.mesh.geom_dofmap, V.dofmap, V.ndofs, gpu, fixed, stiffness, what)


@pytest.mark.parametrize("name", PROPERTY_CASES)
def test_stiffness_properties(gpu, oracle, name):
    case = mh.stiffness_case(name)
    x, a0, y0, got = props_of_case(case, lambda a: mh.make_stiffness(case, a), gpu, name in FIXED_ORDER, True, name)
    assert relerr(got, y0 + mh.stiffness_reference(case, a0, x)) <= TOL


def test_ordered_and_diagonal_properties(gpu, oracle):
    """the fixed-order forms besides the owner kernel: the three WF_FLAG_ORDERED operators, and the pre-assembled
    diagonal on a uniform box (equal contributions per dof, so that the order of the set-up's atomic adds does not
    enter)"""
    import wave_fenics_amd as w
    case = mh.stiffness_case("point-P2")
    Vd = w.FunctionSpace(case.mesh, 2, case.V.dofmap, case.V.index_map, case.V.lattice, structured=False)
    props_of_case(case, lambda a: w.StiffnessOperator(Vd, 2, {"c0": mh.C0}, structured=False, flags=ORDERED, cell_coeff=a),
                  gpu, True, True, "ordered stiffness", Vd)
    props_of_case(case, lambda a: w.MassOperatorLumped(Vd, 2, structured=False, flags=ORDERED | ELEMENTWISE, cell_coeff=a),
                  gpu, True, False, "ordered lumped", Vd)
    props_of_case(case, lambda a: w.MassOperator(Vd, 2, variant="equispaced", quad="gauss_jacobi", qdegree=6, flags=ORDERED, cell_coeff=a),
                  gpu, True, False, "ordered dense mass", Vd)
    mesh = mh.ich.box_with((4, 4, 4), hi=(4.0, 4.0, 4.0))
    Vu = w.create_functionspace(mesh, 2)
    for structured in (True, False):
        make = lambda a: w.MassOperatorLumped(Vu, 2, structured=structured, cell_coeff=a)
        assert make(None).kernel == "diagonal"
        check_properties(make, mesh.x, mesh.geom_dofmap, Vu.dofmap, Vu.ndofs, gpu, True, False, f"diagonal structured={structured}")


MASS_FAMILIES = [("lumped batch_unique", "batch_unique"), ("lumped elementwise", "elementwise"), ("mass_march", "march_idx"),
                 ("mass_column", "batch_unique"), ("mass_any", "mass_dense_any")]


@pytest.mark.parametrize("family,want", MASS_FAMILIES, ids=[m[0].replace(" ", "-") for m in MASS_FAMILIES])
def test_mass_properties(gpu, oracle, family, want):
    """the mass families whose apply adds with atomics"""
    import wave_fenics_amd as w
    p = 2
    case = mh.stiffness_case("point-P2")
    V = w.FunctionSpace(case.mesh, p, case.V.dofmap, case.V.index_map, case.V.lattice, structured=False)
    make = {
        "lumped batch_unique": lambda a: w.MassOperatorLumped(V, p, structured=False, flags=ELEMENTWISE, cell_coeff=a),
        "lumped elementwise": lambda a: w.MassOperatorLumped(V, p, structured=False, flags=ELEMENTWISE, tuning={"kernel": "elementwise"}, cell_coeff=a),
        "mass_march": lambda a: w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=4, cell_coeff=a),
        "mass_column": lambda a: w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=4, tuning={"kernel": "batch"}, cell_coeff=a),
        "mass_any": lambda a: w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=6, cell_coeff=a),
    }[family]
    assert make(None).kernel == want
    props_of_case(case, make, gpu, False, False, family, V)


def test_tet_properties(gpu, oracle):
    """the tetrahedral stiffness -- the one kernel that applies a_c itself -- and the tetrahedral mass"""
    from wave_fenics_amd import tet
    p = 3
    V, _ = mh.tet_meshes((4, 3, 3), p)
    for make, stiffness, what in ((lambda a: tet.TetStiffnessOperator(V, p, {"c0": mh.C0}, cell_coeff=a), True, "tet stiffness"),
                                  (lambda a: tet.TetMassOperator(V, p, cell_coeff=a), False, "tet mass")):
        check_properties(make, V.x, V.geom_dofmap, V.dofmap, V.ndofs, gpu, False, stiffness, what)
