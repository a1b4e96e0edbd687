"""The arbitrary-dofmap operators on meshes that are NOT a union of full boxes with a one-to-one dof numbering
(builders and references: tests/nonbox_helpers.py; their host side: tests/test_nonbox_host.py).

  * HOLED meshes, a 6 x 5 x 7 box with cells deleted (re-entrant corner "L", inclusion "cavity", "stair", "pillar"):
    the lattice-column plan (csrc/march_plan.cpp) then has tile positions that no cell covers AWAY from the end of
    the mesh -- a present cell above an absent one inside one work item, items whose first layers are empty, a hole
    between two present slots of a layer.  The plan's own segment rule picks one layer per item on meshes this small,
    so the gaps inside an item appear with wf_tuning.lz fixed (3 and 8; mass: 5).
    On the "subset" numbering the dofs inside the hole stay in the vectors, named by no cell: x holds NaN there and
    y a sentinel that must come back bit for bit -- an uncovered tile position is neither read nor written.
  * PERIODIC numberings (oracle.make_periodic applied to the dofmap itself, not a ghost exchange): one dof at two
    positions of a tile once a column or a z segment spans the period; two cells along a periodic axis share both
    faces, the plan refuses the mesh and a forced "march" lands on the batch kernel; one cell along a periodic axis
    names a dof twice (batch-unique lists, element-wise scatter, ordered slots, the host-assembled diagonal).
    Reference: the FOLDED box oracle, y = fold(A_box x[l2g]), which never sees a periodic dofmap.

Every operator is created with an explicit kernel hint and its kernel is asserted through wf_op_info_t.kernel.
Tolerances are those of test_gpu_unstructured.py: 1e-12 of max|y_ref| for the stiffness operator and the dense mass
(fp64, summation order), 1e-13 for the lumped mass (one product per entry, at most eight summands).  y0 is random at
the scale of A x (stiffness: 1e6; max|K x| is 5e6 to 1e7 on these boxes at c0 = 1500), so an error in A x cannot hide
behind it.  Each check prints its figure before it asserts (pytest -s); the module prints the worst error per operator
and kernel and what "auto" chose when it is done."""
import functools
import time

import numpy as np
import pytest

import nonbox_helpers as nh
from nonbox_helpers import ORDERED
from support import dev, open_gpu, relerr
from test_gpu_cg import numpy_cg

pytestmark = pytest.mark.gpu

TOL, TOL_LUMPED = 1e-12, 1e-13
DEGREES = [1, 2, 4, 6]
STIFFNESS_HINTS = (("auto", False), ("march", False), ("march", True), ("batch", False), ("elementwise", False))   # (hint, G given)
HOLED = [("L", "subset"), ("cavity", "subset"), ("cavity", "topological"), ("stair", "subset"), ("pillar", "subset"),
         ("pillar", "topological"), ("pillar-shuffled", "subset")]
HOLED_CASES = [(m, r, p) for m, r in HOLED for p in DEGREES] + [("pillar", "subset", p) for p in (3, 5, 7)]
X, XYZ = (True, False, False), (True, True, True)
PERIODIC = [((3, 3, 3), X), ((3, 3, 3), XYZ), ((4, 3, 5), (False, False, True)), ((7, 4, 3), (True, True, False)),
            ((2, 3, 3), X), ((2, 2, 2), XYZ), ((1, 3, 3), X), ((3, 3, 1), (False, False, True))]
PERIODIC_CASES = [(n, per, p) for n, per in PERIODIC for p in DEGREES] + [((3, 3, 3), XYZ, p) for p in (3, 5, 7)]
RECT = {2: 6, 4: 10}      # degree -> Gauss degree 2P + 2 (P + 2 points): the rectangular tables compiled at these degrees

WORST = {}                # (operator, kernel) -> (error, where)
AUTO = {}                 # (operator, case, degree, lz) -> kernel


@pytest.fixture(scope="module")
def gpu():
    dev = open_gpu()
    t0 = time.time()
    yield dev
    print(f"\nnonbox: wall time of the module {time.time() - t0:.1f} s")
    for (opname, kernel), (err, where) in sorted(WORST.items()):
        print(f"nonbox: worst {opname:10s} {kernel:14s} {err:.3e}  {where}")
    for key, kernel in sorted(AUTO.items(), key=str):
        print(f"nonbox: auto {key} -> {kernel}")


def record(opname, op, err, where, hint=None):
    print(f"nonbox: {opname} {op.kernel} {where} hint={hint}: {err:.3e}")
    if not err <= WORST.get((opname, op.kernel), (-1.0, None))[0]:
        WORST[(opname, op.kernel)] = (err, where)
    if hint == "auto":
        AUTO[(opname,) + where] = op.kernel


def tuning(hint, lz):
    t = {"kernel": hint}
    if lz is not None:
        t["lz"] = lz
    return t


def ELEMENTWISE():
    from wave_fenics_amd._lib import WF_FLAG_MASS_ELEMENTWISE
    return WF_FLAG_MASS_ELEMENTWISE


def expected_lz(p, lz):
    """wf_tuning.lz is honoured up to what the kernel's LDS budget allows (the index tile of lz layers lives in LDS):
    at P7, 2 x 1 cells, the k-split kernel's 56.5 KB + 480 B per tile plane fit its 79 KB share of a CU up to 50
    planes = 7 layers; every other (degree, lz) of this file fits."""
    return 7 if (p, lz) == (7, 8) else lz


# =====================================================================================================================
# holed meshes
# =====================================================================================================================
SENTINEL_SEED = 99


def poisoned(case, x, y0):
    """x with NaN and y0 with a sentinel of the same scale in every dof no cell names."""
    xp, yp = x.copy(), y0.copy()
    hole = ~case.listed
    xp[hole] = np.nan
    yp[hole] = np.random.default_rng(SENTINEL_SEED).uniform(1.0, 2.0, int(hole.sum())) * max(np.abs(y0).max(), 1.0)
    return xp, yp


def check_holed(case, op, xp, yp, yref, tol, opname, where, gpu, hint=None):
    """One apply onto the poisoned vectors: the unlisted entries of y come back bit for bit, the others are finite and
    within tol of the reference."""
    y = dev(yp, gpu)
    op(dev(xp, gpu), y)
    got = y.cpu().numpy()
    hole = ~case.listed
    assert np.array_equal(got[hole].view(np.int64), yp[hole].view(np.int64)), (opname, op.kernel, where, "a dof no cell names was written")
    assert np.isfinite(got[case.listed]).all(), (opname, op.kernel, where, "a dof no cell names was read")
    err = relerr(got[case.listed], yref[case.listed])
    record(opname, op, err, where, hint)
    assert err <= tol, (opname, op.kernel, where, err)
    return got


def check_fill(op, case, block, where):
    """wf_op_info_t.plan_fill is the cells per slot of the items the mask leaves: below 1 wherever an item has a gap
    (always with several layers per item on these meshes), exactly 1 only where the deleted cells are whole items (the
    cavity at P6 / P7, 2 x 1 cells, one layer per item)."""
    want = nh.expected_fill(case.coords, op.info.plan_lz, block)
    assert op.info.plan_items > 0 and 0.0 < op.info.plan_fill <= 1.0, (where, op.info.plan_fill)
    assert abs(op.info.plan_fill - want) <= 1e-12, (
        where, op.info.plan_fill, want, "cross-section assumed (nonbox_helpers.STIFFNESS_BLOCK / MASS_BLOCK)", block)


@functools.lru_cache(maxsize=None)
def holed_stiffness_reference(name, route, p):
    from oracle import wave_oracle as oracle
    case = nh.holed_case(name, p, route)
    K = oracle.StiffnessOperator(case.om, p)
    rng = np.random.default_rng(1234)
    x = rng.uniform(-1, 1, case.V.ndofs)
    y0 = rng.uniform(-1, 1, case.V.ndofs) * 1e6
    yref = y0.copy()
    K(x, yref)
    xp, yp = poisoned(case, x, y0)
    yref[~case.listed] = yp[~case.listed]
    return case, K.G, xp, yp, yref


@pytest.mark.parametrize("name,route,p", HOLED_CASES)
def test_stiffness_holed(gpu, oracle, name, route, p):
    """y += K x for lz in {the plan's choice, 3, 8} with the plan by default, forced (geometry from the mesh and handed
    over), and once each on the batch kernel, the element-wise kernel and the order-fixed form (no z segments there)."""
    import torch
    import wave_fenics_amd as w
    case, G, xp, yp, yref = holed_stiffness_reference(name, route, p)
    V = case.V
    gaps = {lz: nh.has_cell_above_gap(case.coords, expected_lz(p, lz)) for lz in (3, 8)}
    assert all(gaps.values()) == (not name.startswith("L"))
    for lz in (None, 3, 8):
        for hint, given in STIFFNESS_HINTS:
            if lz is not None and hint in ("batch", "elementwise"):
                continue      # no z segments in these kernels: once is every case
            op = w.StiffnessOperator(V, p, {"c0": 1500.0}, G=G if given else None, structured=False, tuning=tuning(hint, lz))
            where = (name, route, p, lz)
            if hint == "march":
                assert op.kernel == "march_idx", (where, op.kernel)
                check_fill(op, case, nh.STIFFNESS_BLOCK[p], where)
                if lz is not None:
                    assert op.info.plan_lz == expected_lz(p, lz), (where, op.info.plan_lz)
                    assert op.info.plan_fill < 1.0, (where, op.info.plan_fill)
                if name.endswith("-shuffled"):
                    assert op.info.plan_patterns == op.info.plan_items      # random numbering: no two items share a table
            elif hint == "auto":
                assert op.kernel in ("march_idx", "batch_unique"), (where, op.kernel)
            else:
                assert op.kernel == {"batch": "batch_unique", "elementwise": "elementwise"}[hint], (where, op.kernel)
            check_holed(case, op, xp, yp, yref, TOL, "stiffness", where, gpu, hint)
    op = w.StiffnessOperator(V, p, {"c0": 1500.0}, structured=False, flags=ORDERED())
    assert op.kernel == "cells_ordered" and op.update == "ordered"
    first = check_holed(case, op, xp, yp, yref, TOL, "stiffness", (name, route, p, None), gpu)
    again = check_holed(case, op, xp, yp, yref, TOL, "stiffness", (name, route, p, None), gpu)
    assert np.array_equal(first.view(np.int64), again.view(np.int64)), "the order-fixed form is not bitwise repeatable"
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def holed_mass_reference(name, p):
    case = nh.holed_case(name, p, "subset")
    refs = nh.reference_operators(case.om, p, (2 * p,) + ((RECT[p],) if p in RECT else ()))
    rng = np.random.default_rng(77)
    x = rng.uniform(-1, 1, case.V.ndofs)
    out = {}
    for key in [k for k in refs if k not in ("stiffness", "G")]:
        mx = np.zeros(case.V.ndofs)
        refs[key](x, mx)
        y0 = rng.uniform(-1, 1, case.V.ndofs) * np.abs(mx).max()
        xp, yp = poisoned(case, x, y0)
        yref = y0 + mx
        yref[~case.listed] = yp[~case.listed]
        out[key] = (xp, yp, yref)
    # the collocated rule (GLL points = the nodes, phi1 = identity): the dense mass that is created as a diagonal
    from oracle import wave_oracle as oracle
    _, _, phi1, phi, Xq, Wq = oracle.tabulate_mass_tables(p, "gll", "gll", collocated_qdegree(p))
    assert phi1.shape == (p + 1, p + 1) and np.abs(phi1 - np.eye(p + 1)).max() <= 1e-14
    mx = np.zeros(case.V.ndofs)
    oracle.dense_mass_apply(case.om, phi, oracle.compute_detJ_generic(case.om, Xq, Wq), x, mx)
    y0 = rng.uniform(-1, 1, case.V.ndofs) * np.abs(mx).max()
    xp, yp = poisoned(case, x, y0)
    yref = y0 + mx
    yref[~case.listed] = yp[~case.listed]
    out["collocated"] = (xp, yp, yref)
    return case, out


def collocated_qdegree(p):
    """The GLL rule with P + 1 points: max(2, (qdegree + 4) // 2) points (oracle.tabulate_mass_tables)."""
    return 1 if p == 1 else 2 * p - 2


MASS_HOLED_CASES = [(name, p) for name in ("pillar", "stair") for p in DEGREES] + [("pillar", p) for p in (3, 5, 7)]


@pytest.mark.parametrize("name,p", MASS_HOLED_CASES)
def test_mass_holed(gpu, oracle, name, p):
    """Lumped mass (host-assembled diagonal, batch-unique and flat element-wise forms) and dense mass (Gauss of degree
    2P: lattice plan, batch column kernel, any-rule kernel; Gauss of degree 2P + 2, a rectangular table: the marching
    kernel on request against the any-rule kernel; the collocated GLL rule: the diagonal assembled on the host, and the
    dense kernels under a hint), lz in {the plan's choice, 5}."""
    import wave_fenics_amd as w
    case, refs = holed_mass_reference(name, p)
    V = case.V
    assert nh.has_cell_above_gap(case.coords, 5)
    where = (name, "subset", p, None)
    for flags, tun, want in ((0, None, "diagonal"), (ELEMENTWISE(), None, "batch_unique"),
                             (ELEMENTWISE(), {"kernel": "elementwise"}, "elementwise"),
                             (ELEMENTWISE() | ORDERED(), None, "cells_ordered"), (ORDERED(), None, "diagonal")):
        op = w.MassOperatorLumped(V, p, structured=False, flags=flags, tuning=tun)
        assert op.kernel == want, (where, op.kernel)
        check_holed(case, op, *refs["lumped"], TOL_LUMPED, "lumped", where, gpu)
    # collocated rule: "auto" is the diagonal assembled on the host from det J w (create_mass_diagonal); the same
    # rule under a hint runs the dense kernels
    for hint, want in (("auto", "diagonal"), ("march", "march_idx"), ("mass_any", "mass_dense_any")):
        op = w.MassOperator(V, p, variant="gll_warped", quad="gll", qdegree=collocated_qdegree(p), tuning={"kernel": hint})
        assert op.kernel == want and op.num_quads() == (p + 1) ** 3, (where, hint, op.kernel)
        check_holed(case, op, *refs["collocated"], TOL, "dense_gll", where, gpu)
    for lz in (None, 5):
        where = (name, "subset", p, lz)
        for hint, want in (("auto", None), ("march", "march_idx"), ("batch", "batch_unique"), ("mass_any", "mass_dense_any")):
            if lz is not None and hint in ("batch", "mass_any"):
                continue
            op = w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=2 * p, tuning=tuning(hint, lz))
            assert op.kernel == want if want else op.kernel in ("march_idx", "batch_unique"), (where, hint, op.kernel)
            if hint == "march":
                assert lz is None or (op.info.plan_lz == lz and op.info.plan_fill < 1.0)
                check_fill(op, case, nh.MASS_BLOCK[p], where)
            check_holed(case, op, *refs[("dense", 2 * p)], TOL, "dense", where, gpu, hint)
        if p in RECT:
            for hint, want in (("mass_march", "march_idx"), ("mass_any", "mass_dense_any")):
                if lz is not None and hint == "mass_any":
                    continue
                op = w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=RECT[p], tuning=tuning(hint, lz))
                assert op.kernel == want and op.num_quads() == (p + 2) ** 3, (where, hint, op.kernel)
                if hint == "mass_march":
                    assert lz is None or (op.info.plan_lz == lz and op.info.plan_fill < 1.0)
                    check_fill(op, case, nh.MASS_BLOCK[p], where)
                check_holed(case, op, *refs[("dense", RECT[p])], TOL, "dense_rect", where, gpu, hint)


@pytest.mark.parametrize("p", [4, 6])
def test_parts_on_holed_mesh(gpu, oracle, p):
    """The interior / interface split of the ghost exchange (wf_op_set_ghost_dofs) on the pillar with three layers
    per item, ghost dofs = the plane x = 0.  A missing slot multiplies zero geometry by whatever x its footprint holds,
    so it must never sit in an interior item next to a ghost: with the ghosts poisoned the interior part stays finite."""
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd._lib import WF_PART_INTERFACE, WF_PART_INTERIOR, WF_PART_INTERIOR_A, WF_PART_INTERIOR_B
    case = nh.holed_case("pillar", p, "subset")
    V = case.V
    NX = p * nh.HOLED_BOX[0] + 1
    gpos = np.nonzero((np.arange(V.ndofs) % NX == 0) & case.listed)[0].astype(np.int32)
    assert gpos.size == (p * nh.HOLED_BOX[1] + 1) * (p * nh.HOLED_BOX[2] + 1)      # the whole plane is listed (cx = 0 stays)
    op = w.StiffnessOperator(V, p, {"c0": 1500.0}, structured=False, tuning={"kernel": "march", "lz": 3})
    assert op.kernel == "march_idx" and op.info.plan_lz == 3
    assert op.set_ghost_dofs(gpos)
    assert op.info.items_interior > 0 and op.info.items_interface > 0
    x = dev(np.random.default_rng(8).uniform(-1, 1, V.ndofs), gpu)
    yall = torch.zeros_like(x)
    op(x, yall)
    xp = x.clone()
    xp[torch.from_numpy(gpos.astype(np.int64)).to(gpu)] = float("nan")
    ya = torch.zeros_like(x)
    op.apply_part(xp, ya, WF_PART_INTERIOR)
    assert bool(torch.isfinite(ya).all()), "the interior part read a ghost dof"
    op.apply_part(x, ya, WF_PART_INTERFACE)
    err = relerr(ya.cpu().numpy(), yall.cpu().numpy())
    print(f"nonbox: parts P{p} interior + interface {err:.3e}")
    assert err <= 1e-13
    yb = torch.zeros_like(x)
    for part in (WF_PART_INTERIOR_A, WF_PART_INTERFACE, WF_PART_INTERIOR_B):
        op.apply_part(x, yb, part)
    err = relerr(yb.cpu().numpy(), yall.cpu().numpy())
    print(f"nonbox: parts P{p} interior A + interface + interior B {err:.3e}")
    assert err <= 1e-13
    # and the whole is the oracle's
    K = oracle.StiffnessOperator(case.om, p)
    yref = np.zeros(V.ndofs)
    K(x.cpu().numpy(), yref)
    assert relerr(yall.cpu().numpy(), yref) <= TOL


# =====================================================================================================================
# periodic numberings
# =====================================================================================================================
def tiles(n, periodic):
    """Does the lattice plan take the mesh?  Not with exactly two cells along a periodic axis: they share both faces."""
    return not any(per and c == 2 for c, per in zip(n, periodic))


@functools.lru_cache(maxsize=None)
def periodic_reference(n, periodic, p):
    case = nh.periodic_case(n, p, periodic)
    box = nh.reference_operators(case.ob, p, (2 * p,) + ((RECT[p],) if p in RECT else ()))
    rng = np.random.default_rng(4321)
    N = case.V.ndofs
    x = rng.uniform(-1, 1, N)
    out = {}
    for key in [k for k in box if k != "G"]:
        ax = nh.folded_apply(case, box[key], x)
        y0 = rng.uniform(-1, 1, N) * (1e6 if key == "stiffness" else np.abs(ax).max())
        out[key] = (x, y0, y0 + ax)
    diag = nh.folded_apply(case, box["lumped"], np.ones(N))
    return case, box["G"], out, diag


def check_periodic(op, ref, tol, opname, where, gpu, hint=None):
    x, y0, yref = ref
    y = dev(y0, gpu)
    op(dev(x, gpu), y)
    got = y.cpu().numpy()
    err = relerr(got, yref)
    record(opname, op, err, where, hint)
    assert err <= tol, (opname, op.kernel, where, hint, err)
    return got


@pytest.mark.parametrize("n,periodic,p", PERIODIC_CASES)
def test_periodic_dofmap(gpu, oracle, n, periodic, p):
    """All three operators on a dofmap with identified dofs, lz in {the plan's choice, 8}, against the folded box
    reference.  "march" is the marching kernel where the mesh tiles and -- silently, WF_OK -- the batch kernel where two
    cells share both faces; a rectangular table has no batch form of "mass_march" and raises there."""
    import wave_fenics_amd as w
    case, G, refs, diag = periodic_reference(n, periodic, p)
    V = case.V
    ok = tiles(n, periodic)
    one_wide = any(per and c == 1 for c, per in zip(n, periodic))
    assert (max(len(r) - len(set(r)) for r in V.dofmap.tolist()) > 0) == one_wide
    for lz in (None, 8):
        where = (n, periodic, p, lz)
        # ---- stiffness
        for hint, given in STIFFNESS_HINTS:
            if lz is not None and hint in ("batch", "elementwise"):
                continue
            op = w.StiffnessOperator(V, p, {"c0": 1500.0}, G=G if given else None, structured=False, tuning=tuning(hint, lz))
            if hint == "march":
                assert op.kernel == ("march_idx" if ok else "batch_unique"), (where, op.kernel)
                if ok and lz is not None:
                    assert op.info.plan_lz == expected_lz(p, lz)
            elif hint == "auto":
                assert op.kernel in ("march_idx", "batch_unique")
            else:
                assert op.kernel == {"batch": "batch_unique", "elementwise": "elementwise"}[hint]
            check_periodic(op, refs["stiffness"], TOL, "stiffness", where, gpu, hint)
        # ---- dense mass, square table
        for hint, want in (("auto", None), ("march", "march_idx" if ok else "batch_unique"), ("batch", "batch_unique"),
                           ("mass_any", "mass_dense_any")):
            if lz is not None and hint in ("batch", "mass_any"):
                continue
            op = w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=2 * p, tuning=tuning(hint, lz))
            assert op.kernel == want if want else op.kernel in ("march_idx", "batch_unique"), (where, hint, op.kernel)
            check_periodic(op, refs[("dense", 2 * p)], TOL, "dense", where, gpu, hint)
        # ---- dense mass, rectangular table
        if p in RECT:
            make = lambda hint: w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=RECT[p],      # noqa: E731
                                               tuning=tuning(hint, lz))
            if ok:
                op = make("mass_march")
                assert op.kernel == "march_idx" and op.num_quads() == (p + 2) ** 3
                check_periodic(op, refs[("dense", RECT[p])], TOL, "dense_rect", where, gpu, "mass_march")
            else:
                with pytest.raises(w.WavehipError, match="does not tile"):
                    make("mass_march")
            if lz is None:
                op = make("mass_any")
                assert op.kernel == "mass_dense_any"
                check_periodic(op, refs[("dense", RECT[p])], TOL, "dense_rect", where, gpu, "mass_any")
    # ---- no z segments: the order-fixed forms and the lumped mass
    where = (n, periodic, p, None)
    op = w.StiffnessOperator(V, p, {"c0": 1500.0}, structured=False, flags=ORDERED())
    assert op.kernel == "cells_ordered"
    first = check_periodic(op, refs["stiffness"], TOL, "stiffness", where, gpu)
    assert np.array_equal(first.view(np.int64), check_periodic(op, refs["stiffness"], TOL, "stiffness", where, gpu).view(np.int64))
    op = w.MassOperator(V, p, variant="equispaced", quad="gauss_jacobi", qdegree=2 * p, flags=ORDERED())
    assert op.kernel == "cells_ordered"
    check_periodic(op, refs[("dense", 2 * p)], TOL, "dense", where, gpu)
    for flags, tun, want in ((0, None, "diagonal"), (ELEMENTWISE(), None, "batch_unique"),
                             (ELEMENTWISE(), {"kernel": "elementwise"}, "elementwise"),
                             (ELEMENTWISE() | ORDERED(), None, "cells_ordered"), (ORDERED(), None, "diagonal")):
        op = w.MassOperatorLumped(V, p, structured=False, flags=flags, tuning=tun)
        assert op.kernel == want, (where, op.kernel)
        check_periodic(op, refs["lumped"], TOL_LUMPED, "lumped", where, gpu)
        # M 1 is the folded diagonal of the box
        m = dev(np.zeros(V.ndofs), gpu)
        op(dev(np.ones(V.ndofs), gpu), m)
        err = relerr(m.cpu().numpy(), diag)
        print(f"nonbox: lumped {op.kernel} {where} M 1 vs folded diagonal: {err:.3e}")
        assert err <= TOL_LUMPED, (where, op.kernel, err)


def test_cg_periodic_dense_mass(gpu, oracle):
    """wf_cg on the dense mass of the (3, 3, 3) box periodic in x, y and z at P2 against numpy's solve of the FOLDED box
    matrix; the bounds are those of test_gpu_cg.test_cg_dense_mass_vs_numpy."""
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd import la
    p = 2
    case = nh.periodic_case((3, 3, 3), p, XYZ)
    _, _, phi1, phi, Xq, Wq = oracle.tabulate_mass_tables(p, "gll", "gauss_jacobi", 2 * p)
    detJ = np.abs(oracle.compute_detJ_generic(case.ob, Xq, Wq))
    Nb, N = case.ob.ndofs, case.V.ndofs
    Ab = np.zeros((Nb, Nb))
    e, col = np.zeros(Nb), np.zeros(Nb)
    for j in range(Nb):
        e[:] = 0.0
        e[j] = 1.0
        col[:] = 0.0
        oracle.dense_mass_apply(case.ob, phi, detJ, e, col)
        Ab[:, j] = col
    A = np.zeros((N, N))
    np.add.at(A, (case.l2g[:, None], case.l2g[None, :]), Ab)
    assert np.abs(A - A.T).max() <= 1e-14 * np.abs(A).max()
    op = w.MassOperator(case.V, p, phi1, detJ)
    AUTO[("dense (cg)", (3, 3, 3), XYZ, p, None)] = op.kernel
    b = np.random.default_rng(8).uniform(-1, 1, N)
    xs = np.linalg.solve(A, b)
    _, k_np = numpy_cg(A, b, 200, 1e-10)
    x = torch.zeros(N, dtype=torch.float64, device=gpu)
    its, res = la.cg(x, torch.from_numpy(b).to(gpu), op, kmax=200, rtol=1e-10)
    print(f"nonbox: cg periodic dense mass {op.kernel}: its {its} (numpy {k_np}) res {res:.3e}")
    assert abs(its - k_np) <= max(3, k_np // 25), (its, k_np)
    assert res < 1e-10
    assert np.abs(x.cpu().numpy() - xs).max() <= 1e-7 * np.abs(xs).max()


# =====================================================================================================================
# renumbering
# =====================================================================================================================
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("kind", ["pillar-shuffled", "periodic"])
def test_lattice_renumbering_keeps_the_operator(gpu, oracle, kind, p):
    """renumber(V, lattice_numbering(V)) is a relabelling: K x moves with the permutation (1e-12).  Every degree on
    both meshes, the shuffled pillar (dofs no cell names go behind the others) and (3, 3, 3) periodic in x, y and z."""
    import wave_fenics_amd as w
    if kind == "periodic":
        case, _, refs, _ = periodic_reference((3, 3, 3), XYZ, p)
        x, y0, yref = refs["stiffness"]
        listed = np.ones(case.V.ndofs, dtype=bool)
    else:
        case, _, x, y0, yref = holed_stiffness_reference(kind, "subset", p)
        listed = case.listed
    V = case.V
    new = w.lattice_numbering(V)
    assert np.array_equal(np.sort(new), np.arange(V.ndofs))
    Vn = w.renumber(V, new)
    xn, yn = np.empty_like(x), np.empty_like(y0)
    xn[new], yn[new] = x, y0
    op = w.StiffnessOperator(Vn, p, {"c0": 1500.0}, structured=False, tuning={"kernel": "march"})
    assert op.kernel == "march_idx"
    y = dev(yn, gpu)
    op(dev(xn, gpu), y)
    got = y.cpu().numpy()[new]
    assert np.array_equal(got[~listed].view(np.int64), y0[~listed].view(np.int64))
    err = relerr(got[listed], yref[listed])
    print(f"nonbox: renumbered {kind} P{p}: {err:.3e}")
    assert err <= TOL
