"""The caller's frame of wf_op_create -- the element permutation h_perm and WF_FLAG_TENSOR_X_SLOWEST -- on every set-up
path that consumes it, on the MI355X.  The frame is pure index work: a wrong map gives an operator that is wrong by
O(1) for one class of callers and leaves every other test green.

Every case creates the operator in the four frames of tests/frame_helpers.py (id, perm, xslow, xslow+perm: an
independent restatement of the contract, checked on the CPU by tests/test_frame_host.py) and asserts
  1. op.kernel (geometry / update where they apply) is the one the case names;
  2. y = y0 + A x against the CPU oracle on the CANONICAL mesh, y0 random at the scale of A x: 1e-12 of max|y_ref| for the
     stiffness and the dense mass, 1e-14 for the lumped mass; x and y are in the global numbering, which no frame touches;
  3. y against the twin created from the canonical (id) inputs on the same route: within 1e-13 of max|y| for kernels that
     add with atomics, BIT FOR BIT for WF_FLAG_ORDERED (wf_ordered_slots orders a dof's entries by their place in the
     caller's dofmap; two entries of one dof lie in different cells on these meshes, so neither perm nor the axis order
     changes the order of the sum) and for the host-assembled collocated diagonal (summed in cell order).
Both bitwise expectations hold in the code as it is.  Each test prints its worst figures ("FRAME ..." lines) and the
module prints one line per family at the end.

Set-up sites (csrc/op_create.hip) and the cases that reach them:

  site                                     cases
  1 tensor_dofmap                          every case but the collocated ones (frames perm, xslow, xslow+perm)
  2 create_mass_diagonal                   test_dense_mass[collocated-*]: h_detJ (qmap) and rule + mesh (raw_points)
  3 plan_stiffness_geometry, h_G branch    test_stiffness[plan-*], source "G": box (code 0), stair (code 0, empty slots),
                                           random_orient (the 48 orientation codes composed with the point order);
                                           test_stiffness_ksplit_cross_sections
  4 plan_mass_detJ                         test_dense_mass[square-plan-*], [rect-march-*] (M = nq1 = P + 2): h_detJ
                                           (PointMaps, codes != 0 on random_orient) and rule + mesh (raw_points)
  5 build_ordered_plan                     test_stiffness[ordered-*], test_lumped_mass[*-ordered-*], test_dense_mass[*-ordered-*]
  6 batch_stiffness, h_G branch            test_stiffness[batch-*], [elementwise-*], [ordered-*];
                                           test_restaging_switches[stiffness-*]: shuffled x xslow x coeff, all eight,
                                           exactly one of them the direct upload (000)
  7 create_batch, h_detJ restage           test_lumped_mass, test_dense_mass on the batch routes;
                                           test_restaging_switches[dense-*]: the same eight, qmap(nq1)
  per-cell geometry                        test_stiffness_per_cell: the sheared affine box and its randomly re-oriented
                                           version at P1-P4 (site 1; the geometry comes from the mesh)
  k_march_ks<P, BX, BY, true>              test_stiffness_ksplit_cross_sections: P5 3x1 7x1 2x1, P6 2x1 1x1 5x1, P7 2x1 2x2
                                           1x1 (read from WF_KS_SHAPES), (BX+1, BY+1, 5) cells at lz = 2 (items of 2, 2, 1
                                           layers) and lz = 5 (one item per column); the cross-section that ran is
                                           asserted through plan_items (4 columns) and plan_fill (cells per slot, which gives BX BY)

The plan route is the default tuning on the box (sized in frame_helpers.BOX_N so that the plan is adopted) and
{"kernel": "march"} on random_orient and stair, which only overrides the fill threshold of create_on_plan.

Negative controls (test_controls): per operator kind and route family the x-slowest inputs WITHOUT the flag and the perm
inputs with the INVERSE permutation must miss the oracle by more than 1e-3; the same route with the truth told is
checked first, kernel included.  For the mass operators the x-slowest
control takes det J from the mesh: a consistent exchange of x and z in dofs and points is a symmetry of Phi^T D Phi
and of the lumped mass, so handing over det J in the same (wrong) order gives the right operator
(test_frame_host.test_misframed_*_mass_moves).  All indices stay in range.

Refusals (test_refusals, creation only): a perm with a repeated or an out-of-range entry, WF_FLAG_ORDERED with a block
tuning, per-cell geometry on the perturbed box.  No combination of the matrix is refused by the library."""
import numpy as np
import pytest

import frame_helpers as fh
from guard_helpers import compiled_shapes
from support import open_gpu

pytestmark = pytest.mark.gpu

TOL_ORACLE = 1e-12    # of max|y_ref|: stiffness, dense mass
TOL_LUMPED = 1e-14    # the bound of test_gpu_parity.test_x_slowest_tensor_order
TOL_FORM = 1e-13      # of max|y|: two creations of one atomic sum
DIFFERS = 1e-3
WF_ERR_INVALID, WF_ERR_UNSUPPORTED = -1, -2     # wf_status, include/wavehip.h
C0 = {"c0": 1500.0}
KS_SHAPES = [s for s in compiled_shapes("stiffness_march_ks.hip", "WF_KS_SHAPES") if s[0] >= 5]     # (P, BX, BY)
MASS_SHAPES = compiled_shapes("mass_march.hip", "WF_MASS_SHAPES")                                   # (P, M, BX, BY)

STATS = {}


@pytest.fixture(scope="module")
def gpu():
    dev = open_gpu()
    yield dev
    for family, s in STATS.items():
        print(f"FRAME-FAMILY {family}: operators {s['n']} worst oracle {s['oracle']:.3e} worst twin {s['twin']:.3e} "
              f"bitwise twins {s['bitwise']} of {s['twins']}")


def F():
    from wave_fenics_amd import _lib
    return _lib


def xflag(fr):
    return F().WF_FLAG_TENSOR_X_SLOWEST if fr.xslow else 0


def space_of(case, dofmap, rows=None):
    """the caller's space: its dofmap on the case's mesh (rows: the caller's cell order)"""
    import wave_fenics_amd as w
    mesh = case.mesh
    if rows is not None:
        mesh = w.BoxMesh(mesh.n, mesh.x, np.ascontiguousarray(mesh.geom_dofmap[rows]), mesh.lo, mesh.hi)
    return w.FunctionSpace(mesh, case.p, np.ascontiguousarray(dofmap, dtype=np.int32), w.IndexMap(case.V.ndofs),
                           getattr(case.V, "lattice", None), structured=False)


def apply(op, ref, gpu):
    import torch
    y = torch.from_numpy(ref.y0.copy()).to(gpu)
    op(torch.from_numpy(ref.x.copy()).to(gpu), y)
    torch.cuda.synchronize()
    out = y.cpu().numpy()
    assert np.isfinite(out).all()
    return out


def expect(op, want, what):
    if isinstance(want, str):
        want = {"kernel": want}
    for key, value in want.items():
        assert getattr(op, key) == value, (what, key, getattr(op, key), value)


def record(family, eo, et, bitwise, is_twin):
    s = STATS.setdefault(family, {"n": 0, "oracle": 0.0, "twin": 0.0, "bitwise": 0, "twins": 0})
    s["n"] += 1
    s["oracle"] = max(s["oracle"], eo)
    if is_twin:
        s["twins"] += 1
        s["twin"] = max(s["twin"], et)
        s["bitwise"] += int(bitwise)


def run_frames(gpu, family, what, p, canon, ref, build, want, tol=TOL_ORACLE, bitwise=False, frames=fh.FRAMES):
    """build(fr, inputs) -> operator, for every frame; the checks 1-3 of the module docstring.  Returns the id operator."""
    assert frames[0] == "id"
    twin, first, worst_o, worst_t = None, None, 0.0, 0.0
    for name in frames:
        fr = fh.frame(name, p)
        op = build(fr, fh.caller_inputs(canon, fr.perm, fr.xslow))
        expect(op, want, (what, name))
        y = apply(op, ref, gpu)
        eo = fh.relerr(y, ref.yref, ref.scale)
        if twin is None:
            twin, first, et, same = y, op, 0.0, True
        else:
            et = fh.relerr(y, twin)
            same = bool(np.array_equal(y.view(np.int64), twin.view(np.int64)))
        record(family, eo, et, same, name != "id")
        worst_o, worst_t = max(worst_o, eo), max(worst_t, et)
        print(f"FRAME {family} {what} {name}: oracle {eo:.3e} twin {et:.3e}{' bitwise' if same and name != 'id' else ''}")
        assert eo <= tol, (what, name, "oracle", eo)
        if bitwise:
            assert same, (what, name, "twin not bitwise", et)
        else:
            assert et <= TOL_FORM, (what, name, "twin", et)
    return first


# ---------------------------------------------------------------------------------------------------------------------
# stiffness
# ---------------------------------------------------------------------------------------------------------------------
def plan_tuning(mesh):
    return None if mesh == "box" else {"kernel": "march"}


def stiffness_route(route, mesh):
    """(tuning, flags, what op must report)"""
    if route == "plan":
        return plan_tuning(mesh), 0, {"kernel": "march_idx", "geometry": "per_point"}
    if route == "batch":
        return {"kernel": "batch"}, 0, {"kernel": "batch_unique", "geometry": "per_point"}
    if route == "elementwise":
        return {"kernel": "elementwise"}, 0, {"kernel": "elementwise", "geometry": "per_point"}
    if route == "ordered":
        return None, F().WF_FLAG_ORDERED, {"kernel": "cells_ordered", "update": "ordered"}
    raise ValueError(route)


def make_stiffness(case, p, fr, inp, source, tuning, flags, rows=None, coeff=None):
    import wave_fenics_amd as w
    return w.StiffnessOperator(space_of(case, inp["dofmap"], rows), p, C0, G=inp["G"] if source == "G" else None, perm=fr.perm,
                               structured=False, flags=flags | xflag(fr), tuning=tuning, cell_coeff=coeff)


STIFFNESS = [("plan", m, p) for m in fh.MESHES for p in range(1, 8)] \
    + [(r, m, p) for r in ("batch", "elementwise", "ordered") for m in ("box", "random_orient") for p in (2, 4, 6)]


@pytest.mark.parametrize("route,mesh,p", STIFFNESS, ids=[f"{r}-{m}-P{p}" for r, m, p in STIFFNESS])
def test_stiffness(gpu, oracle, route, mesh, p):
    case, K, ref = fh.mesh_case(mesh, p), fh.stiffness_canon(mesh, p), fh.stiffness_reference(mesh, p)
    tuning, flags, want = stiffness_route(route, mesh)
    canon = {"dofmap": case.om.dofmap, "G": K.G}
    for source in ("G", "mesh"):
        op = run_frames(gpu, f"stiffness-{route}", f"{mesh} P{p} {source}", p, canon, ref,
                        lambda fr, inp: make_stiffness(case, p, fr, inp, source, tuning, flags), want, bitwise=route == "ordered")
        if route == "plan":
            assert op.info.plan_items > 0 and 0.0 < op.info.plan_fill <= 1.0
            if mesh == "random_orient":   # orientation codes != 0: most cells are looked at in another frame than their own
                assert op.info.plan_reoriented > case.om.ncells // 2, op.info.plan_reoriented
            if mesh == "stair":
                assert op.info.plan_fill < 1.0


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("mesh", ["sheared", "sheared_random"])
def test_stiffness_per_cell(gpu, oracle, mesh, p):
    case, ref = fh.mesh_case(mesh, p), fh.stiffness_reference(mesh, p)
    want = {"kernel": "march_idx", "geometry": "per_cell", "metric": "full"}
    op = run_frames(gpu, "stiffness-per-cell", f"{mesh} P{p}", p, {"dofmap": case.om.dofmap}, ref,
                    lambda fr, inp: make_stiffness(case, p, fr, inp, "mesh", {"geometry": "per_cell"}, 0), want)
    if mesh == "sheared_random":
        assert op.info.plan_reoriented > case.om.ncells // 2


@pytest.mark.parametrize("lz", [2, 5])
@pytest.mark.parametrize("p,bx,by", KS_SHAPES, ids=[f"P{p}-{bx}x{by}" for p, bx, by in KS_SHAPES])
def test_stiffness_ksplit_cross_sections(gpu, oracle, p, bx, by, lz):
    """k_march_ks<P, BX, BY, true> at every compiled cross-section through tuning["block"] on a dofmap operator.  lz = 2:
    work items of 2, 2 and 1 layers; lz = 5: one item of five layers per column (the plan's own choice on a mesh this
    small is one layer per item, so both are requested)."""
    assert len(KS_SHAPES) == 9
    n, nz = (bx + 1, by + 1, 5), 5
    case = fh.box_of(n, p)
    K = oracle.StiffnessOperator(case.om, p)
    ref = fh._vectors(case.om.ndofs, 400 + p, K)
    canon = {"dofmap": case.om.dofmap, "G": K.G}
    tuning = {"kernel": "march", "block": (bx, by, 1), "lz": lz}
    for source in ("G", "mesh"):
        op = run_frames(gpu, "stiffness-ksplit", f"P{p} {bx}x{by} lz{lz} {source}", p, canon, ref,
                        lambda fr, inp: make_stiffness(case, p, fr, inp, source, tuning, 0),
                        {"kernel": "march_idx", "geometry": "per_point"}, frames=("id", "xslow+perm"))
        plz = op.info.plan_lz
        print(f"FRAME stiffness-ksplit P{p} {bx}x{by} requested lz {lz}: plan_lz {plz} plan_items {op.info.plan_items}")
        assert plz == lz, (p, bx, by, lz, plz)
        # (BX + 1) x (BY + 1) cells are 2 x 2 columns of the requested cross-section; plan_fill = cells per cell slot of
        # the items then gives BX BY, which no two compiled cross-sections of a degree share
        assert op.info.plan_items == 4 * -(-nz // plz), (p, bx, by, op.info.plan_items, plz)
        assert abs(op.info.plan_fill - case.om.ncells / (op.info.plan_items * bx * by * plz)) <= 1e-12, (p, bx, by, op.info.plan_fill)
        assert len({s[1] * s[2] for s in KS_SHAPES if s[0] == p}) == 3


# ---------------------------------------------------------------------------------------------------------------------
# lumped mass
# ---------------------------------------------------------------------------------------------------------------------
def lumped_route(route):
    L = F()
    return {"diagonal": (0, "diagonal"), "elementwise": (L.WF_FLAG_MASS_ELEMENTWISE, "batch_unique"),
            "diagonal-ordered": (L.WF_FLAG_ORDERED, "diagonal"),
            "elementwise-ordered": (L.WF_FLAG_MASS_ELEMENTWISE | L.WF_FLAG_ORDERED, "cells_ordered")}[route]


def make_lumped(case, p, fr, inp, source, flags, tuning=None):
    import wave_fenics_amd as w
    return w.MassOperatorLumped(space_of(case, inp["dofmap"]), p, detJ=inp["detJ"] if source == "detJ" else None, perm=fr.perm,
                                structured=False, flags=flags | xflag(fr), tuning=tuning)


@pytest.mark.parametrize("p", [2, 4, 6])
@pytest.mark.parametrize("mesh", ["box", "random_orient"])
@pytest.mark.parametrize("route", ["diagonal", "elementwise", "diagonal-ordered", "elementwise-ordered"])
def test_lumped_mass(gpu, oracle, route, mesh, p):
    case, M, ref = fh.mesh_case(mesh, p), fh.lumped_canon(mesh, p), fh.lumped_reference(mesh, p)
    flags, kernel = lumped_route(route)
    canon = {"dofmap": case.om.dofmap, "detJ": M.detJ}
    for source in ("detJ", "mesh"):
        run_frames(gpu, f"lumped-{route}", f"{mesh} P{p} {source}", p, canon, ref,
                   lambda fr, inp: make_lumped(case, p, fr, inp, source, flags), kernel, tol=TOL_LUMPED,
                   bitwise=route.endswith("ordered"))


# ---------------------------------------------------------------------------------------------------------------------
# dense mass
# ---------------------------------------------------------------------------------------------------------------------
def dense_route(kind, route, mesh):
    """(tuning, flags, kernel)"""
    table = {("square", "plan"): (plan_tuning(mesh), 0, "march_idx"), ("square", "batch"): ({"kernel": "batch"}, 0, "batch_unique"),
             ("square", "any"): ({"kernel": "mass_any"}, 0, "mass_dense_any"), ("square", "ordered"): (None, F().WF_FLAG_ORDERED, "cells_ordered"),
             ("rect", "march"): ({"kernel": "mass_march"}, 0, "march_idx"), ("rect", "any"): ({"kernel": "mass_any"}, 0, "mass_dense_any"),
             ("rect", "ordered"): (None, F().WF_FLAG_ORDERED, "cells_ordered"), ("collocated", "diagonal"): (None, 0, "diagonal")}
    return table[(kind, route)]


DENSE_ROUTES = [("square", "plan"), ("square", "batch"), ("square", "any"), ("square", "ordered"), ("rect", "march"), ("rect", "any"),
                ("rect", "ordered"), ("collocated", "diagonal")]


def make_dense(case, p, t, fr, inp, source, tuning, flags, rows=None, coeff=None):
    import wave_fenics_amd as w
    V = space_of(case, inp["dofmap"], rows)
    if source == "detJ":
        return w.MassOperator(V, p, t.phi1, inp["detJ"], perm=fr.perm, tuning=tuning, flags=flags | xflag(fr), cell_coeff=coeff)
    return w.MassOperator(V, p, perm=fr.perm, variant=t.variant, quad=t.quad, qdegree=t.qdegree, tuning=tuning,
                          flags=flags | xflag(fr), cell_coeff=coeff)


@pytest.mark.parametrize("p", [2, 3, 4, 6])
@pytest.mark.parametrize("mesh", ["box", "random_orient"])
@pytest.mark.parametrize("kind,route", DENSE_ROUTES, ids=[f"{k}-{r}" for k, r in DENSE_ROUTES])
def test_dense_mass(gpu, oracle, kind, route, mesh, p):
    case, t, ref = fh.mesh_case(mesh, p), fh.mass_canon(mesh, p, kind), fh.mass_reference(mesh, p, kind)
    tuning, flags, kernel = dense_route(kind, route, mesh)
    if kind == "rect":
        assert any(s[:2] == (p, t.nq1) for s in MASS_SHAPES), (p, t.nq1)
    if kind == "collocated":
        assert np.array_equal(np.round(t.phi1, 13), np.eye(p + 1))
    canon = {"dofmap": case.om.dofmap, "detJ": t.detJ}
    for source in ("detJ", "mesh"):
        op = run_frames(gpu, f"dense-{kind}-{route}", f"{mesh} P{p} {source}", p, canon, ref,
                        lambda fr, inp: make_dense(case, p, t, fr, inp, source, tuning, flags), kernel,
                        bitwise=route in ("ordered", "diagonal"))
        assert op.num_quads() == t.nq1 ** 3
        if kernel == "march_idx" and mesh == "random_orient":
            assert op.info.plan_reoriented > case.om.ncells // 2


# ---------------------------------------------------------------------------------------------------------------------
# the restaging switches of the batch route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [2, 5])
@pytest.mark.parametrize("kind", ["stiffness", "dense"])
def test_restaging_switches(gpu, oracle, kind, p):
    """{caller's cell order shuffled} x {xslow} x {cell_coeff} on the batch route with the caller's own h_G / h_detJ: the
    upload is direct for exactly one of the eight, restaged through the cell order, qmap and the coefficient for the
    others.  The twin is the id frame in the mesh's own cell order with the same coefficient."""
    case = fh.mesh_case("box", p)
    nc = case.om.ncells
    cp, a = fh.cell_shuffle(nc), fh.coefficient(nc)
    if kind == "stiffness":
        canon = {"dofmap": case.om.dofmap, "G": fh.stiffness_canon("box", p).G}
        refs = {c: fh.stiffness_reference("box", p, coeff=c) for c in (False, True)}
        build = lambda fr, inp, rows, coeff: make_stiffness(case, p, fr, inp, "G", {"kernel": "batch"}, 0, rows, coeff)
    else:
        t = fh.mass_canon("box", p, "square")
        canon = {"dofmap": case.om.dofmap, "detJ": t.detJ}
        refs = {c: fh.mass_reference("box", p, "square", coeff=c) for c in (False, True)}
        build = lambda fr, inp, rows, coeff: make_dense(case, p, t, fr, inp, "detJ", {"kernel": "batch"}, 0, rows, coeff)
    ident = fh.frame("id", p)
    direct = []
    for coeff in (False, True):
        ref = refs[coeff]
        twin = apply(build(ident, fh.caller_inputs(canon, None, False), None, a if coeff else None), ref, gpu)
        for shuffled in (False, True):
            for xslow in (False, True):
                fr = fh.frame("xslow+perm" if xslow else "perm", p)
                inp = fh.caller_inputs(canon, fr.perm, fr.xslow)
                if shuffled:
                    inp = {k: np.ascontiguousarray(v[cp]) for k, v in inp.items()}
                keeps = fh.library_keeps_cell_order(inp["dofmap"])
                assert keeps == (not shuffled)
                if keeps and not xslow and not coeff:
                    direct.append((shuffled, xslow, coeff))
                op = build(fr, inp, cp if shuffled else None, (a[cp] if shuffled else a) if coeff else None)
                expect(op, "batch_unique", (kind, p, shuffled, xslow, coeff))
                assert op.cell_coeff == coeff
                y = apply(op, ref, gpu)
                eo, et = fh.relerr(y, ref.yref, ref.scale), fh.relerr(y, twin)
                record(f"switches-{kind}", eo, et, bool(np.array_equal(y.view(np.int64), twin.view(np.int64))), True)
                print(f"FRAME switches-{kind} P{p} shuffled {int(shuffled)} xslow {int(xslow)} coeff {int(coeff)}: oracle {eo:.3e} twin {et:.3e}")
                assert eo <= TOL_ORACLE and et <= TOL_FORM, (kind, p, shuffled, xslow, coeff, eo, et)
    assert direct == [(False, False, False)]


# ---------------------------------------------------------------------------------------------------------------------
# negative controls
# ---------------------------------------------------------------------------------------------------------------------
CONTROLS = [("stiffness", "plan", "box", 3), ("stiffness", "plan", "random_orient", 2), ("stiffness", "plan", "box", 5),
            ("stiffness", "batch", "box", 2), ("stiffness", "elementwise", "box", 4), ("stiffness", "ordered", "box", 2),
            ("lumped", "diagonal", "box", 2), ("lumped", "elementwise", "random_orient", 4),
            ("dense", "square-plan", "box", 3), ("dense", "square-batch", "random_orient", 2), ("dense", "rect-march", "box", 4),
            ("dense", "rect-any", "box", 2), ("dense", "collocated-diagonal", "box", 4)]


@pytest.mark.parametrize("kind,route,mesh,p", CONTROLS, ids=[f"{k}-{r}-{m}-P{p}" for k, r, m, p in CONTROLS])
def test_controls(gpu, oracle, kind, route, mesh, p):
    """The hazard is real and these inputs can see it: (a) the x-slowest inputs without the flag, (b) the perm inputs with
    the inverse permutation.  Every index stays in range: both are valid inputs of another operator."""
    case = fh.mesh_case(mesh, p)
    xs, pe = fh.frame("xslow", p), fh.frame("perm", p)
    plain = fh.frame("id", p)                                     # what the library is told in (a): no flag, no perm
    liar = fh.frame("perm", p)
    liar.perm = fh.inverse(pe.perm)                               # what it is told in (b)
    assert not np.array_equal(liar.perm, pe.perm)
    if kind == "stiffness":
        canon, ref = {"dofmap": case.om.dofmap, "G": fh.stiffness_canon(mesh, p).G}, fh.stiffness_reference(mesh, p)
        tuning, flags, want = stiffness_route(route, mesh)
        build = lambda fr, inp, source: make_stiffness(case, p, fr, inp, source, tuning, flags)
        sources = ("G", "G")
    elif kind == "lumped":
        canon, ref = {"dofmap": case.om.dofmap, "detJ": fh.lumped_canon(mesh, p).detJ}, fh.lumped_reference(mesh, p)
        flags, want = lumped_route(route)
        build = lambda fr, inp, source: make_lumped(case, p, fr, inp, source, flags)
        sources = ("mesh", "detJ")
    else:
        tk, tr = route.split("-")
        t = fh.mass_canon(mesh, p, tk)
        canon, ref = {"dofmap": case.om.dofmap, "detJ": t.detJ}, fh.mass_reference(mesh, p, tk)
        tuning, flags, want = dense_route(tk, tr, mesh)
        build = lambda fr, inp, source: make_dense(case, p, t, fr, inp, source, tuning, flags)
        sources = ("mesh", "detJ")
    # the same route with the truth told passes (so the controls below fail for the frame alone)
    for fr in (xs, pe):
        op = build(fr, fh.caller_inputs(canon, fr.perm, fr.xslow), sources[0])
        expect(op, want, (kind, route, fr.name))
        y = apply(op, ref, gpu)
        assert fh.relerr(y, ref.yref, ref.scale) <= TOL_ORACLE
    for what, told, truth, source in (("xslow inputs, no flag", plain, xs, sources[0]), ("perm inputs, inverse perm", liar, pe, sources[1])):
        # no kernel is asserted here: a dofmap read in the wrong frame is no tensor dofmap, and what the lattice plan makes of
        # it (columns of single cells, or none and then the batch kernels) is not the subject
        op = build(told, fh.caller_inputs(canon, truth.perm, truth.xslow), source)
        err = fh.relerr(apply(op, ref, gpu), ref.yref, ref.scale)
        print(f"FRAME control {kind} {route} {mesh} P{p} {what}: off by {err:.3e}")
        assert err > DIFFERS, (kind, route, mesh, p, what, err)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu, oracle):
    import wave_fenics_amd as w
    L = F()
    p = 2
    case, K = fh.mesh_case("box", p), fh.stiffness_canon("box", p)
    nd = (p + 1) ** 3
    fr = fh.frame("perm", p)
    inp = fh.caller_inputs({"dofmap": case.om.dofmap, "G": K.G}, fr.perm, False)
    V = space_of(case, inp["dofmap"])

    def refused(make, status, text):
        with pytest.raises(w.WavehipError) as e:
            make()
        assert e.value.status == status, (e.value.status, status, str(e.value))
        assert text in str(e.value) and text.encode() in L.lib().wf_last_error(), str(e.value)

    repeated, outside = fr.perm.copy(), fr.perm.copy()
    repeated[3] = repeated[4]
    outside[5] = nd
    for bad in (repeated, outside, -1 - fr.perm):
        for xf in (0, L.WF_FLAG_TENSOR_X_SLOWEST):
            refused(lambda: w.StiffnessOperator(V, p, C0, G=inp["G"], perm=bad, structured=False, flags=xf), WF_ERR_INVALID,
                    "perm is not a permutation")
        refused(lambda: w.MassOperatorLumped(V, p, perm=bad, structured=False), WF_ERR_INVALID, "perm is not a permutation")
    refused(lambda: w.StiffnessOperator(V, p, C0, perm=fr.perm, structured=False, flags=L.WF_FLAG_ORDERED,
                                        tuning={"block": (7, 4, 1)}), WF_ERR_INVALID, "WF_FLAG_ORDERED takes no wf_tuning field")
    refused(lambda: w.StiffnessOperator(V, p, C0, perm=fr.perm, structured=False, tuning={"geometry": "per_cell"}),
            WF_ERR_INVALID, "is not affine")
    refused(lambda: w.StiffnessOperator(V, p, C0, G=inp["G"], perm=fr.perm, structured=False, tuning={"geometry": "per_cell"}),
            WF_ERR_UNSUPPORTED, "h_G must be NULL")
    # the library is usable afterwards, and the same inputs with the truth told are accepted
    op = w.StiffnessOperator(V, p, C0, G=inp["G"], perm=fr.perm, structured=False)
    ref = fh.stiffness_reference("box", p)
    assert fh.relerr(apply(op, ref, gpu), ref.yref, ref.scale) <= TOL_ORACLE
