"""Conditions on the reference and the bound of the cell-form tests (tests/cell_form_helpers.py), and the refusals of
wf_cell_form_create that need no device.  No GPU.

  * B is not tight enough to fail a right kernel: the float64 oracle, cell by cell (its apply restricted to one cell,
    then lambda . y), stays within B / 2 of the long-double reference at P1 to P7;
  * the reference is the form it claims to be: sum_c e_c = lambda^T K u, and e_c(lambda, u) = e_c(u, lambda);
  * B is not loose enough to pass a wrong cell mapping: the reference with its rows rotated by one cell, or evaluated
    with the next cell's lambda and u, misses by more than 1e6 bounds at every cell;
  * every argument check of wf_cell_form_create precedes the first device call: the refusals below run on a machine
    without a GPU and report the documented code and a word of wf_last_error."""
import ctypes

import numpy as np
import pytest

import cell_form_helpers as cf
import stiffness_entry_helpers as se
from support import EPS, LD, wpackage  # noqa: F401

DEGREES = (1, 2, 3, 4, 5, 6, 7)


@pytest.mark.parametrize("p", DEGREES)
def test_oracle_within_half_of_B(wpackage, oracle, p):
    d = cf.data(p, cf.HOST_BOX[p])
    assert d.margin >= se.MARGIN, d.margin
    B = cf.bound("point", p)
    K = oracle.StiffnessOperator(d.om, p, {"c0": cf.C0})
    e = np.zeros(d.om.ncells)
    for c in range(d.om.ncells):
        y = np.zeros(d.om.ndofs)
        K(np.ascontiguousarray(d.u), y, cells=(c, c + 1))
        e[c] = float(d.lam @ y)
    # lambda . y sums ndofs products where the form sums nd: the zeros outside the cell add nothing
    plain, ok, at, used = cf.cell_check(e, d.ref, d.mag, d.gerr, B / 2)
    share = float(np.max(d.gerr / (LD(EPS) * d.mag)))
    cancel = float(np.max(d.mag / np.abs(d.ref)))
    print(f"CELLFORM host P{p} {cf.HOST_BOX[p]}: B {B}, oracle {plain:.2f} eps mag, gerr up to {share:.0f} eps mag, "
          f"mag/|e_c| up to {cancel:.0f}, allowance used {used:.2f}")
    assert ok, (p, at, plain, B / 2)


@pytest.mark.parametrize("p", DEGREES)
def test_sum_and_symmetry(wpackage, oracle, p):
    d = cf.data(p, cf.HOST_BOX[p])
    B = cf.bound("point", p)
    ax, mag, gerr = se.reference(d.om, p, d.geo, np.ascontiguousarray(d.u)[None, :])
    lam = np.asarray(d.lam).astype(LD)
    total, total_mag = (lam * ax[0]).sum(), (np.abs(lam) * mag[0]).sum()
    assert abs(d.ref.sum() - total) <= 4 * d.om.ndofs * np.finfo(LD).eps * total_mag     # two orders of one exact sum
    ref_t, mag_t, gerr_t = cf.stiffness_reference(d.om, p, d.geo, d.u, d.lam)
    # K_c is symmetric: D^T G D with G symmetric; the two orders differ by the long double's own roundings only
    assert np.all(np.abs(ref_t - d.ref) <= 8 * (p + 1) ** 3 * np.finfo(LD).eps * d.mag)
    assert np.all(np.abs(ref_t - d.ref) <= B * LD(EPS) * d.mag + d.gerr)
    assert np.all(np.abs(mag_t - d.mag) <= 8 * (p + 1) ** 3 * np.finfo(LD).eps * d.mag)


@pytest.mark.parametrize("p", DEGREES)
def test_wrong_cell_mapping_would_be_caught(wpackage, oracle, p):
    d = cf.data(p, cf.HOST_BOX[p])
    B = cf.bound("point", p)
    nc = d.om.ncells
    rotated = np.roll(d.ref, 1)
    nxt = cf.subset_oracle(d.om, np.roll(np.arange(nc), -1))      # cell c's geometry with the next cell's lambda and u
    swapped, _, _ = cf.stiffness_reference(fields_of(d.om, nxt), p, d.geo, d.lam, d.u)
    for what, other in (("rows rotated", rotated), ("next cell's fields", swapped)):
        m = cf.misses(other, d.ref, d.mag, d.gerr, B)
        print(f"CELLFORM control P{p} {what}: nearest cell misses by {m:.3e} bounds")
        assert m > 1e6, (p, what, m)


def fields_of(om, nxt):
    """om's geometry rows with nxt's dofmap rows: the fields of the next cell on this cell's geometry"""
    from types import SimpleNamespace
    return SimpleNamespace(x=om.x, geom_dofmap=om.geom_dofmap, dofmap=nxt.dofmap, ndofs=om.ndofs, p=om.p)


def test_lumped_reference_is_the_diagonal(wpackage, oracle):
    """sum_c e^M_c(1, u) = sum_d m_d u_d with the oracle's lumped mass"""
    for p in (1, 2, 4):
        d = cf.data(p, cf.HOST_BOX[p])
        ref, mag, gerr = cf.lumped_reference(d.om, p, np.ones(d.om.ndofs), d.u)
        y = np.zeros(d.om.ndofs)
        oracle.MassOperatorCPU(d.om, p)(np.ascontiguousarray(d.u), y)
        assert abs(float(ref.sum()) - y.sum()) <= 1e-13 * float(mag.sum())


# ---------------------------------------------------------------------------------------------------------------------
# refusals that need no device
# ---------------------------------------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -2


def make_desc(wlib, p=2, n=(2, 1, 1), kind=0, with_G=False):
    import wave_fenics_amd as w
    mesh = w.create_box(n, perturb=0.0)
    V = w.create_functionspace(mesh, p)
    keep = [np.ascontiguousarray(V.dofmap, dtype=np.int32), np.ascontiguousarray(mesh.x, dtype=np.float64),
            np.ascontiguousarray(mesh.geom_dofmap, dtype=np.int32)]
    d = wlib.OpDesc()
    d.kind, d.degree, d.ncells, d.ndofs = kind, p, mesh.ncells, V.ndofs
    d.h_dofmap = wlib._ip(keep[0])
    d.c0 = 1500.0
    if with_G:
        keep.append(np.zeros((mesh.ncells, (p + 1) ** 3, 3, 3)))
        d.h_G = wlib._dp(keep[-1])
    else:
        d.nverts = keep[1].shape[0]
        d.h_xverts = wlib._dp(keep[1])
        d.h_geom_dofmap = wlib._ip(keep[2])
    return d, keep


def refused(wlib, d, out=True):
    h = ctypes.c_void_p()
    rc = wlib.lib().wf_cell_form_create(ctypes.byref(d) if d is not None else None, ctypes.byref(h) if out else None)
    assert not h.value
    return rc, wlib.lib().wf_last_error().decode()


def test_refusals_before_any_device_call(wpackage):
    from wave_fenics_amd import _lib as wlib
    L = wlib.lib()
    d, keep = make_desc(wlib, kind=wlib.WF_OP_MASS_DENSE)
    rc, msg = refused(wlib, d)
    assert rc == UNSUPPORTED and "dense" in msg
    for flag, word in ((wlib.WF_FLAG_ORDERED, "WF_FLAG_ORDERED"), (wlib.WF_FLAG_MASS_ELEMENTWISE, "WF_FLAG_MASS_ELEMENTWISE")):
        for kind in (wlib.WF_OP_STIFFNESS, wlib.WF_OP_MASS_LUMPED):
            d, keep = make_desc(wlib, kind=kind)
            d.flags = flag
            rc, msg = refused(wlib, d)
            assert rc == INVALID and word in msg, (flag, kind, rc, msg)
    for field in ("kernel", "variant", "lz", "lz0", "bx", "by", "bz", "keep_cell_order", "orient", "metric", "update"):
        d, keep = make_desc(wlib)
        t = wlib.Tuning()
        setattr(t, field, 1)
        d.tuning = ctypes.pointer(t)
        rc, msg = refused(wlib, d)
        assert rc == INVALID and "wf_tuning" in msg, (field, rc, msg)
    d, keep = make_desc(wlib)
    t = wlib.Tuning()
    t.geometry = 3
    d.tuning = ctypes.pointer(t)
    rc, msg = refused(wlib, d)
    assert rc == INVALID and "geometry" in msg
    d, keep = make_desc(wlib, with_G=True)
    t = wlib.Tuning()
    t.geometry = 2
    d.tuning = ctypes.pointer(t)
    rc, msg = refused(wlib, d)
    assert rc == UNSUPPORTED and "h_G" in msg
    d, keep = make_desc(wlib)
    a = np.array([1.0, float("nan")])
    d.h_cell_coeff = wlib._dp(a)
    rc, msg = refused(wlib, d)
    assert rc == INVALID and "cell 1" in msg and "finite" in msg
    # null pointers: the descriptor, the output, the dofmap, the geometry; eval, info
    assert refused(wlib, None)[0] == INVALID
    d, keep = make_desc(wlib)
    rc, msg = refused(wlib, d, out=False)
    assert rc == INVALID and "null" in msg
    d, keep = make_desc(wlib)
    d.h_dofmap = None
    rc, msg = refused(wlib, d)
    assert rc == INVALID and "dofmap" in msg
    for kind in (wlib.WF_OP_STIFFNESS, wlib.WF_OP_MASS_LUMPED):
        d, keep = make_desc(wlib, kind=kind)
        d.h_xverts = None
        rc, msg = refused(wlib, d)
        assert rc == INVALID and "mesh" in msg
    d, keep = make_desc(wlib)
    keep[0][1, 3] = d.ndofs
    rc, msg = refused(wlib, d)
    assert rc == INVALID and "out of range" in msg
    d, keep = make_desc(wlib)
    keep[2][0, 0] = -1
    rc, msg = refused(wlib, d)
    assert rc == INVALID and "vertex" in msg
    d, keep = make_desc(wlib)
    d.degree = 8
    assert refused(wlib, d)[0] == UNSUPPORTED
    h = ctypes.c_void_p()
    x = np.zeros(3 * 2 * 2 * 3)
    assert L.wf_cell_form_create_box(0, 2, 2, 1, 1, None, 1500.0, None, 0, None, ctypes.byref(h)) == INVALID
    assert L.wf_cell_form_create_box(2, 2, 2, 1, 1, wlib._dp(x), 1500.0, None, 0, None, ctypes.byref(h)) == UNSUPPORTED
    assert L.wf_cell_form_eval(None, None, None, 1.0, 0, None, None) == INVALID
    assert "null" in L.wf_last_error().decode()
    assert L.wf_cell_form_info(None, None) == INVALID


def test_per_cell_request_names_the_cell(wpackage):
    """PER_CELL on a perturbed box: WF_ERR_INVALID naming the first cell that is not affine, on the host"""
    from wave_fenics_amd import _lib as wlib
    import wave_fenics_amd as w
    d, keep = make_desc(wlib, p=2, n=(3, 3, 3))
    keep[1][:] = w.create_box((3, 3, 3), perturb=0.2).x
    t = wlib.Tuning()
    t.geometry = 2
    d.tuning = ctypes.pointer(t)
    rc, msg = refused(wlib, d)
    assert rc == INVALID and "WF_GEOMETRY_PER_CELL: cell 0 is not affine" in msg, msg
