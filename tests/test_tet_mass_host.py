"""Host side of the dense simplex mass operator (wf_op_create_dense_simplex_mass): every refusal with its status and a
wf_last_error that names the offending thing, the kernel's public name, and the reference of test_gpu_tet_mass.py
against something that is not the kernel.  No GPU: every check of the creation precedes the first device call."""
import ctypes

import numpy as np
import pytest

from support import wlib  # noqa: F401
from tet_mass_helpers import (EPS, GRID, LD, NCB, NO_FABS, NU9_CASES, ORDERED, ORIENTATION_CASES, SMALL, SMALL_COUNTS, BIG,
                              Case, MassOp, batch_unique, collapsed_float64, det_j, generic_case, lds_bytes, nu_of, ratio,
                              reference, relerr, small, small_reference, upright_of, TOL)

INVALID, UNSUPPORTED = -1, -2


def refused(case, status, *words, flags=0, null=None):
    op = MassOp(case, flags, null)
    assert op.rc == status and not op.h.value, (case.name, op.rc, op.message)
    assert "wf_op_create_dense_simplex_mass" in op.message, op.message
    for w in words:
        assert w in op.message, (w, op.message)
    return op.message


def with_arrays(case, name, **arrays):
    d = dict(name=name, nd=case.nd, nq=case.nq, phi=case.phi, W=case.W, xv=case.xv, gd=case.gd, dm=case.dm, ndofs=case.ndofs,
             x=case.x, y0=case.y0)
    d.update(arrays)
    return Case(**d)


def test_kernel_name_and_constants(wlib):
    from wave_fenics_amd import operators
    assert operators.KERNEL_NAMES[10] == "dense_simplex_mass"
    assert wlib.WF_KERNEL_DENSE_SIMPLEX_MASS == 10 and wlib.WF_KERNEL_CELLS_ORDERED == 9 and wlib.WF_KERNEL_DENSE_SIMPLEX == 7
    assert hasattr(wlib.lib(), "wf_op_create_dense_simplex_mass")
    assert "wf_op_create_dense_simplex_mass" in wlib.SIGNATURES
    from wave_fenics_amd import tet
    assert hasattr(tet, "TetMassOperator")


def test_degenerate_cell_is_refused(wlib):
    """a zero-volume cell is WF_ERR_INVALID and the message names the cell"""
    flat = small("P4_n65")
    gd = flat.gd.copy()
    gd[5, 3] = gd[5, 0]                      # two equal vertices: a zero column of J
    refused(with_arrays(flat, "repeated vertex", gd=gd), INVALID, "cell 5", "degenerate")
    xv = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]])   # four points of one plane
    one = np.array([[0, 1, 2, 3]], dtype=np.int32)
    p1 = small("P1_q8")
    refused(with_arrays(p1, "flat cell", xv=xv, gd=one, dm=one.copy(), ndofs=4, x=p1.x[:4], y0=p1.y0[:4]), INVALID, "cell 0",
            "degenerate")
    xv = flat.xv.copy()
    xv[flat.gd[64, 2], 1] = np.nan
    msg = refused(with_arrays(flat, "NaN vertex", xv=xv), INVALID, "degenerate")
    first = int(np.argmax(np.isnan(det_j(xv, flat.gd, np.float64))))
    assert f"cell {first} " in msg
    refused(with_arrays(flat, "NaN vertex, signed", xv=xv), INVALID, "degenerate", flags=NO_FABS)


@pytest.mark.parametrize("nd,nq", [(37, 27), (21, 8), (5, 1), (40, 64), (16, 4), (32, 125)])
def test_uncompiled_shape_is_refused_at_creation(wlib, nd, nq):
    """an nd whose tile counts are not compiled (37: KT = 10; 21: KT = 6) is WF_ERR_UNSUPPORTED and the message names nd"""
    refused(generic_case("uncompiled", nd, nq, 20, None, 1), UNSUPPORTED, "not compiled", f"nd = {nd}")


@pytest.mark.parametrize("nq", [1, 7, 64, 125, 343])
def test_any_rule_size_passes_the_shape_check(wlib, nq):
    """nq does not enter the shape check (the stiffness kernel's point tiles must not leak into this operator): with a
    compiled nd and any nq the creation gets past every host check, to the degenerate cell planted in the mesh"""
    c = generic_case("any nq", 35, nq, 20, None, 2)
    gd = c.gd.copy()
    gd[19, 1] = gd[19, 2]
    refused(with_arrays(c, "any nq", gd=gd), INVALID, "cell 19", "degenerate")


def test_flags(wlib):
    c = small("P2_q27")
    refused(c, UNSUPPORTED, "WF_FLAG_ORDERED", flags=ORDERED)
    refused(c, UNSUPPORTED, "WF_FLAG_ORDERED", flags=ORDERED | NO_FABS)
    for bit in (2, 4, 8, 32, 1 << 20):
        refused(c, INVALID, "unknown flag", str(bit), flags=bit)
        refused(c, INVALID, "unknown flag", str(bit | NO_FABS), flags=bit | NO_FABS)


@pytest.mark.parametrize("field", ["h_dofmap", "h_phi", "h_weights", "h_xverts", "h_geom_dofmap"])
def test_null_array(wlib, field):
    refused(small("P2_q27"), INVALID, "null array", field, null=field)


def test_null_arguments_and_sizes(wlib):
    L = wlib.lib()
    h = ctypes.c_void_p()
    assert L.wf_op_create_dense_simplex_mass(None, ctypes.byref(h)) == INVALID
    assert b"wf_op_create_dense_simplex_mass" in L.wf_last_error() and b"null" in L.wf_last_error()
    d = wlib.DenseMassDesc()
    assert L.wf_op_create_dense_simplex_mass(ctypes.byref(d), None) == INVALID
    c = small("P2_q27")
    for name, bad in (("nd", 0), ("nd", -4), ("nq", 0), ("ndofs", -1)):
        refused(with_arrays(c, "bad " + name, **{name: bad}), INVALID, "bad sizes")


def test_index_ranges(wlib):
    c = small("P2_q27")
    for bad in (-1, c.ndofs):
        dm = c.dm.copy()
        dm[7, 3] = bad
        refused(with_arrays(c, "dofmap", dm=dm), INVALID, "dofmap entry out of range")
    for bad in (-1, c.xv.shape[0]):
        gd = c.gd.copy()
        gd[70, 2] = bad
        refused(with_arrays(c, "vertex", gd=gd), INVALID, "vertex index out of range")


def test_reference_headroom():
    """Neither reference is the code under test, and both have ample headroom: on every small case a float64 numpy
    evaluation of the collapsed form s_c (A x_e) -- what a correct kernel computes, up to the order of its sums -- and
    the two-stage form in float64 stay below B / 10 of the long-double reference, entry by entry (a factor ten of headroom;
    the worst seen is 0.05 B, on the cases whose dofs belong to one cell each and whose B is smallest); the float64
    two-stage form (reference (b)) is within TOL / 100 of it in the max norm"""
    worst = 0.0
    for name in SMALL:
        c = small(name)
        for flags in ((0, NO_FABS) if name in ORIENTATION_CASES else (0,)):
            ref, mag = small_reference(name, flags)
            for what, y in (("collapsed", collapsed_float64(c, flags)), ("two-stage", reference(c, flags, np.float64)[0])):
                r, ok, where = ratio(y, ref, mag, c.B)
                worst = max(worst, r / c.B)
                assert ok and r <= 0.1 * c.B, (name, flags, what, where, r, c.B)
            assert relerr(reference(c, flags, np.float64)[0], np.asarray(ref, dtype=np.float64)) <= TOL / 100
    print(f"float64 evaluations against long double: worst {worst:.4f} B")
    assert 0.0 < worst


def test_cases_are_what_they_name():
    """tile pairs, NU, full slots, LDS sizes, batch counts and orientation of every named case, from its dofmap and
    geometry the way dense_mass_setup and launch_mass_dense_simplex compute them"""
    nu = {name: batch_unique(small(name).dm) for name in SMALL}
    expect = {"P1_q8": (1, 1), "P1_q1": (1, 1), "P2_q27": (3, 1), "P2_q1": (3, 1), "P3_q64": (5, 2), "P3_q27": (5, 2),
              "P4_q125": (9, 3), "P4_q1": (9, 3), "P4_q27": (9, 3), "g3x5": (1, 1), "g11x13": (3, 1), "g18x20": (5, 2),
              "g33x50_shared": (9, 3), "g33x50_spread": (9, 3), "g36x17_shared": (9, 3), "g36x17_broken": (9, 3)}
    for name, t in expect.items():
        assert small(name).tiles == t, name
    assert {small(n).tiles for n in SMALL} == {(1, 1), (3, 1), (5, 2), (9, 3)}            # every compiled pair
    assert [small(n).nq for n in ("P1_q8", "P2_q27", "P3_q64", "P4_q125")] == [8, 27, 64, 125]   # (p + 1)^3: degree >= 2p
    assert [small(n).nq for n in ("P1_q1", "P2_q1", "P4_q1")] == [1, 1, 1]
    assert all(small(n).nq % 16 for n in ("P3_q27", "P4_q27", "P4_q125", "g3x5", "g11x13", "g18x20", "g33x50_shared", "g36x17_shared"))
    assert [small(n).nd for n in ("g3x5", "g11x13", "g18x20", "g33x50_shared", "g36x17_shared")] == [3, 11, 18, 33, 36]
    for name in SMALL:
        c = small(name)
        assert (nu_of(c) == 9) == (name in NU9_CASES), name
        assert lds_bytes(c) <= 64 * 1024, name                       # no launch needs the large-LDS attribute
        assert c.dm.min() >= 0 and c.dm.max() < c.ndofs and c.gd.max() < c.xv.shape[0]
        assert all(np.unique(row).size == c.nd for row in c.dm), "a cell names a dof twice"
        assert np.all(c.W > 0) and np.all(c.y0 != 0.0)
        det = det_j(c.xv, c.gd, np.float64)
        assert np.all(det != 0.0), name
        if c.inverted is not None:
            assert np.array_equal(det < 0.0, c.inverted), name
            assert np.all(det_j(c.xv, c.upright_gd, np.float64) > 0.0)
    # unique-tile size: well numbered, scattered, and every slot of NU = 5 / NU = 9 in use
    assert nu["P4_control"].max() <= 1280 < nu["P4_scattered"].max() and nu["P4_scattered"].size == 6
    assert nu["P3_broken"].max() == 1280 == 5 * 256 and nu["P3_broken"][-1] == 2 * 20
    assert nu["g36x17_broken"].max() == 2304 == 9 * 256
    assert nu["P4_broken"].max() == 2240
    assert lds_bytes(small("P4_scattered")) != lds_bytes(small("P4_broken"))          # the two handles applied alternately
    # batch edges
    for n in SMALL_COUNTS:
        c = small(f"P4_n{n}")
        assert c.ncells == n and c.nbatch == (n + 63) // 64
    assert small("P4_n65").ncells % NCB == 1 and small("P4_n129").ncells % NCB == 1   # a last batch of one cell
    # orientation
    assert [n for n in SMALL if small(n).inverted is not None] == ORIENTATION_CASES
    assert small("P2_all_inverted").inverted.all() and small("P4_all_inverted").inverted.all()
    for name in ("P2_half_inverted", "P4_half_inverted"):
        inv = small(name).inverted
        assert 0.3 < inv.mean() < 0.7 and inv[:NCB].any() and not inv[:NCB].all()


def test_orientation_references_discriminate():
    """flags 0: the reference is that of the upright mesh, cell for cell (|det J| does not see the swap of two vertices);
    WF_FLAG_NO_FABS: the sign is kept, and the two references differ by far more than the entry bound, so a kernel or a
    set-up that takes the wrong one fails"""
    for name in ORIENTATION_CASES:
        c = small(name)
        up = upright_of(c)
        s_abs, s_up = np.abs(det_j(c.xv, c.gd, LD)), det_j(up.xv, up.gd, LD)
        assert np.all(np.abs(s_abs - s_up) <= 4 * np.finfo(LD).eps * s_up)               # cell for cell
        ref0, mag = small_reference(name, 0)
        refu, _ = reference(up, 0)
        assert np.all(np.abs(ref0 - refu) <= 4 * np.finfo(LD).eps * c.nd * mag)
        ref1, mag1 = small_reference(name, NO_FABS)
        assert np.array_equal(mag, mag1)
        diff = np.abs(ref0 - ref1)
        worst = float(np.max(diff / (LD(EPS) * mag)))
        print(f"{name}: the references of flags 0 and WF_FLAG_NO_FABS differ by {worst:.3e} eps of the magnitude (B = {c.B})")
        assert worst >= 1e6 * c.B
        if c.inverted.all():                        # every cell negative: M x changes sign as a whole
            y0 = np.asarray(c.y0, dtype=LD)
            assert np.all(np.abs((ref1 - y0) + (ref0 - y0)) <= 4 * np.finfo(LD).eps * c.nd * mag)


def test_big_cases_are_what_they_name():
    """the persistent-loop cases against the grid bound they assume (GRID = kMassGridBound of mass_dense_simplex.hip)"""
    c = BIG["P2_rounds4"]()
    assert c.nbatch == 3 * GRID + 1 and c.ncells % NCB == 1 and nu_of(c) == 5        # > two rounds; round 4: one workgroup, one cell
    c = BIG["P4_rounds2"]()
    nu = batch_unique(c.dm)
    assert c.nbatch == GRID + 1 and c.ncells % NCB == 1 and 1280 < nu[:-1].min() and nu.max() <= 2304 and nu[-1] == 35
