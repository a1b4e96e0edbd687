"""wf_geometry_hex_cell (host only): the per-cell geometry of affine hexahedra and the test that decides whether a
stiffness operator may store it -- the rule of wf_op_create_box and of wf_op_create with wf_tuning.geometry =
WF_GEOMETRY_PER_CELL.  No GPU.

  * the meshes of tests/test_gpu_idx_cell_geometry.py really are affine by the bitwise rule, and the rectilinear ones
    have exactly diagonal G_c (checked with numpy, without the library);
  * G_c against a long-double numpy evaluation of J^-1 J^-T |det J| at 4 eps relative per component, exact zeros
    staying exact -- the double evaluation rounds 1 / det J, each adjugate entry, its two products and the sum of
    three, a handful of half-ulp steps per component;
  * first_bad and reason on the meshes a per-cell request refuses;
  * the box's own decision on the cases of tests/test_gpu_affine_geometry.py.
"""
import numpy as np
import pytest

import idx_cell_helpers as h

EPS = np.finfo(np.float64).eps
OFFDIAG = [1, 2, 4]   # G01 G02 G12 in the order of h.COMP


def check_against_longdouble(mesh, p, use_fabs=True):
    import wave_fenics_amd as w
    Gc, bad, reason = w.hex_cell_geometry(mesh, p, use_fabs=use_fabs, clamp=True)
    assert (bad, reason) == (-1, 0)
    ref = h.cell_geometry_longdouble(mesh, use_fabs)
    zero = ref == 0
    assert np.all(Gc[zero] == 0.0)
    err = np.abs(Gc.astype(np.longdouble) - ref)[~zero] / np.abs(ref[~zero])
    print(f"worst relative error {float(err.max() / EPS):.2f} eps over {err.size} components")
    assert err.max() <= 4 * EPS, float(err.max() / EPS)
    return Gc


@pytest.mark.parametrize("name", h.PARITY_MESHES + ("glued_mirrored",) + h.HOLED + ("column-7", "column-12"))
def test_meshes_are_affine_and_match_longdouble(name):
    mesh = h.affine_mesh(name)
    assert h.is_bitwise_affine(mesh).all()
    ref = h.cell_geometry_longdouble(mesh)
    assert np.all(ref[:, OFFDIAG] == 0) == h.is_rectilinear(name)
    if name.startswith("sheared"):
        assert np.all((ref[:, OFFDIAG] != 0).sum(axis=1) == 1)   # the G01 of x += 0.25 y, wherever a cell's frame puts it
    Gc = check_against_longdouble(mesh, 2)
    assert np.all(Gc[:, OFFDIAG] == 0.0) == h.is_rectilinear(name)
    if name == "glued_mirrored":   # det J < 0 in block 2: the sign is kept without fabs
        sign = h.cell_det_sign(mesh)
        assert (sign < 0).sum() == 48 and (sign > 0).sum() == 32
        Gs = check_against_longdouble(mesh, 2, use_fabs=False)
        assert np.array_equal(Gs, Gc * sign[:, None])


def test_sheared_frames_keep_their_off_diagonal():
    """A cell's own frame and the lattice frame differ by a signed permutation of the axes: the set of |G_c| entries of
    a randomly turned cell is that of the cell as given."""
    import wave_fenics_amd as w
    a, _, _ = w.hex_cell_geometry(h.affine_mesh("sheared-asis"), 3)
    b, _, _ = w.hex_cell_geometry(h.affine_mesh("sheared-random"), 3)
    assert np.array_equal(np.sort(np.abs(a), axis=1), np.sort(np.abs(b), axis=1))
    assert np.array_equal(a[0], b[0])   # cell 0 keeps its frame


@pytest.mark.parametrize("kind", ["perturbed", "one_vertex", "tiny"])
def test_refusals_name_the_cell_and_the_reason(kind):
    import wave_fenics_amd as w
    mesh, cell, reason = h.refusal_mesh(kind)
    for p in (2, 4):
        Gc, bad, why = w.hex_cell_geometry(mesh, p)
        assert (bad, why) == (cell, reason), (kind, p, bad, why)
    if kind == "tiny":   # without the clamp the mesh qualifies
        assert w.hex_cell_geometry(mesh, 4, clamp=False)[1:] == (-1, 0)
        assert w.hex_cell_geometry(mesh, 1)[1:] == (-1, 0)   # P1: 1e-7 w^3 = 1.25e-8, above the clamp's 1e-8


def test_degenerate_cell_and_bad_arguments():
    import wave_fenics_amd as w
    mesh = h.box_with((2, 2, 2))
    x = mesh.x.copy()
    x[:, 2] = 0.0                # flat: det J = 0, still affine
    flat = h.box_with((2, 2, 2), x=x)
    assert w.hex_cell_geometry(flat, 2)[1:] == (0, 2)
    x = mesh.x.copy()
    x[0, 0] = np.nan             # NaN != NaN: not affine
    assert w.hex_cell_geometry(h.box_with((2, 2, 2), x=x), 2)[1:] == (0, 1)
    with pytest.raises(w.WavehipError):
        w.hex_cell_geometry(mesh, 8)
    bad = w.BoxMesh(mesh.n, mesh.x, mesh.geom_dofmap + 100)
    with pytest.raises(w.WavehipError, match="vertex index"):
        w.hex_cell_geometry(bad, 2)
    empty = w.BoxMesh(None, mesh.x, np.zeros((0, 8), dtype=np.int32))
    assert w.hex_cell_geometry(empty, 2)[1:] == (-1, 0)


# the box cases of tests/test_gpu_affine_geometry.py (AFFINE and its two non-affine ones), built as there
BOX_SHAPES = [(1, (6, 5, 4)), (2, (5, 4, 3)), (3, (4, 3, 3)), (4, (5, 3, 4))]


def affine_box_case(case, n):
    if case == "unit":
        return h.box_with(n)
    if case == "anisotropic":
        return h.box_with(n, hi=(2.0, 1.0, 0.5))
    if case == "far":
        import wave_fenics_amd as w
        return w.create_box(n, lo=(0.9,) * 3, hi=(1.0,) * 3)
    if case == "graded":
        rng = np.random.default_rng(7)
        axes = [np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, m))]) for m in n]
        return h.box_with(n, x=h.lattice_x(*axes))
    x = h.lattice_x(*[np.arange(m + 1) * 0.125 for m in n])
    x[:, 0] += 0.25 * x[:, 1]
    return h.box_with(n, x=x)


@pytest.mark.parametrize("p,n", BOX_SHAPES)
@pytest.mark.parametrize("case", ["unit", "anisotropic", "far", "graded", "sheared"])
def test_box_decision_affine(case, p, n):
    mesh = affine_box_case(case, n)
    assert h.is_bitwise_affine(mesh).all()
    check_against_longdouble(mesh, p)


@pytest.mark.parametrize("p,n", [(2, (4, 4, 3)), (4, (4, 3, 3))])
@pytest.mark.parametrize("case", ["perturbed", "one_vertex"])
def test_box_decision_non_affine(case, p, n):
    import wave_fenics_amd as w
    if case == "perturbed":
        mesh = h.box_with(n, perturb=0.2)
    else:
        x = h.box_with(n).x.copy()
        nx, ny, _ = n
        x[1 + (nx + 1) * (1 + (ny + 1) * 1), 1] += 0.01
        mesh = h.box_with(n, x=x)
    _, bad, reason = w.hex_cell_geometry(mesh, p)
    assert bad == int(np.nonzero(~h.is_bitwise_affine(mesh))[0][0]) and reason == 1
    # x += 0.3 y on linspace coordinates rounds each vertex differently: that box keeps per-point geometry too
    x = h.box_with(n).x.copy()
    x[:, 0] += 0.3 * x[:, 1]
    assert w.hex_cell_geometry(h.box_with(n, x=x), p)[2] == 1
