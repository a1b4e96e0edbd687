"""Cell coefficients (heterogeneous media), the part that needs no GPU: the headroom of the reference, the refusals of
non-finite coefficients, the Medium class and the weighted facet mass.  The references and cases are those of
tests/medium_helpers.py, shared with the GPU tests."""
import numpy as np
import pytest

import medium_helpers as mh
from support import wpackage as wlib  # noqa: F401


# ---------------------------------------------------------------------------------------------------------------------
# the oracle alone: its two forms of every reference agree to TOL / 10, so the bound has headroom
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mh.STIFFNESS_CASES)
def test_oracle_stiffness_headroom(oracle, wlib, name):
    """dense against sum-factorised stiffness with G * a on every case's mesh and every field"""
    case = mh.stiffness_case(name)
    x, _ = mh.vectors(case.om.ndofs)
    for f in mh.FIELDS:
        a = mh.field(f, case.mesh.x, case.mesh.geom_dofmap)
        assert a.shape == (case.om.ncells,) and np.isfinite(a).all()
        nz = a[a != 0.0]
        assert nz.max() / nz.min() <= 8.0 and (f != "zeros" or (a == 0.0).any()) and (f != "distinct" or np.unique(a).size == a.size)
        ys, yd = mh.stiffness_reference(case, a, x), mh.stiffness_reference(case, a, x, dense=True)
        err = mh.relerr(ys, yd)
        print(f"HEADROOM stiffness {name} {f}: {err:.3e}")
        assert err <= mh.TOL / 10, (name, f, err)


@pytest.mark.parametrize("name", ["point-P2", "owner-P4", "batch-P2", "periodic-P2", "ksplit-P6"])
def test_oracle_mass_headroom(oracle, wlib, name):
    """the lumped mass apply against the dense mass apply with the collocated table, both with detJ * a"""
    case = mh.stiffness_case(name)
    x, _ = mh.vectors(case.om.ndofs)
    for f in mh.FIELDS:
        a = mh.field(f, case.mesh.x, case.mesh.geom_dofmap)
        err = mh.relerr(mh.lumped_reference(case.om, case.p, a, x), mh.lumped_reference(case.om, case.p, a, x, dense=True))
        print(f"HEADROOM mass {name} {f}: {err:.3e}")
        assert err <= mh.TOL / 10, (name, f, err)


def test_slab_interface_is_inside_blocks():
    """the slab's plane on the owner case: cells 0..2 of 9 in x, not at the geometry block (5) nor the owner column (8)"""
    case = mh.stiffness_case("owner-P4")
    a = mh.field("slab", case.mesh.x, case.mesh.geom_dofmap).reshape(7, 3, 9)
    assert np.array_equal(a[0, 0], [1, 1, 1, 8, 8, 8, 8, 8, 8]) and (a == a[0, 0]).all()


# ---------------------------------------------------------------------------------------------------------------------
# refusals: a NaN or infinite entry is WF_ERR_INVALID naming the cell, through every creation function, with no device
# ---------------------------------------------------------------------------------------------------------------------
def _refused(make, ncells, cell, value):
    a = np.ones(ncells)
    a[cell] = value
    a[min(cell + 2, ncells - 1)] = value   # the FIRST bad cell is named
    with pytest.raises(Exception) as e:
        make(a)
    assert getattr(e.value, "status", None) == -1, e.value           # WF_ERR_INVALID
    assert f"cell {cell}" in str(e.value) and "not finite" in str(e.value), e.value


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_coefficient_is_refused(wlib, value):
    w = wlib
    from wave_fenics_amd import tet
    mesh = w.create_box((3, 2, 2), perturb=0.2)
    V = w.create_functionspace(mesh, 2)
    nc = mesh.ncells
    phi1 = np.eye(3)
    detJ = np.ones((nc, 27))
    makers = {
        "wf_op_create_box stiffness": lambda a: w.StiffnessOperator(V, 2, cell_coeff=a),
        "wf_op_create_box lumped": lambda a: w.MassOperatorLumped(V, 2, cell_coeff=a),
        "wf_op_create_box ordered": lambda a: w.StiffnessOperator(V, 2, flags=16, cell_coeff=a),
        "wf_op_create stiffness": lambda a: w.StiffnessOperator(V, 2, structured=False, cell_coeff=a),
        "wf_op_create lumped": lambda a: w.MassOperatorLumped(V, 2, structured=False, cell_coeff=a),
        "wf_op_create spectral": lambda a: w.SpectralMassOperator(V, 2, structured=False, cell_coeff=a),
        "wf_op_create dense mass": lambda a: w.MassOperator(V, 2, phi1=phi1, detJ=detJ, cell_coeff=a),
    }
    for what, make in makers.items():
        _refused(make, nc, 5, value)
    T = tet.create_kuhn_box((2, 1, 1), 2, perturb=0.1)
    _refused(lambda a: tet.TetStiffnessOperator(T, 2, cell_coeff=a), T.ncells, 7, value)
    _refused(lambda a: tet.TetMassOperator(T, 2, cell_coeff=a), T.ncells, 7, value)


def test_coefficient_length_is_checked(wlib):
    w = wlib
    V = w.create_functionspace(w.create_box((3, 2, 2)), 2)
    with pytest.raises(w.WavehipError, match="cell_coeff has 11 entries"):
        w.StiffnessOperator(V, 2, cell_coeff=np.ones(11))


# ---------------------------------------------------------------------------------------------------------------------
# Medium
# ---------------------------------------------------------------------------------------------------------------------
def test_medium_coefficients(wlib):
    from wave_fenics_amd.medium import Medium
    rng = np.random.default_rng(3)
    c, rho = rng.uniform(1400.0, 4000.0, 17), rng.uniform(900.0, 1900.0, 17)
    m = Medium(c, rho)
    assert m.ncells == 17
    assert np.array_equal(m.mass_coeff, 1.0 / (rho * c ** 2))
    assert np.array_equal(m.stiff_coeff, 1.0 / rho)
    assert np.array_equal(m.admittance, 1.0 / (rho * c))
    m1 = Medium(c)
    assert np.array_equal(m1.rho, np.ones(17)) and np.array_equal(m1.stiff_coeff, np.ones(17))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        cb = c.copy()
        cb[4] = bad
        with pytest.raises(ValueError, match=r"c\[4\]"):
            Medium(cb)
    with pytest.raises(ValueError):
        Medium(c, rho[:5])


def test_medium_from_centroids(wlib):
    w = wlib
    from wave_fenics_amd.medium import Medium
    mesh = w.create_box((4, 3, 2), hi=(4.0, 3.0, 2.0))
    m = Medium.from_centroids(mesh, lambda xc: (np.where(xc[:, 2] < 1.0, 1500.0, 3000.0), np.where(xc[:, 0] < 2.0, 1000.0, 1800.0)))
    c, rho = m.c.reshape(2, 3, 4), m.rho.reshape(2, 3, 4)     # cell order cx + nx (cy + ny cz)
    assert (c[0] == 1500.0).all() and (c[1] == 3000.0).all()
    assert (rho[:, :, :2] == 1000.0).all() and (rho[:, :, 2:] == 1800.0).all()
    assert np.array_equal(Medium.from_centroids(mesh, lambda xc: 1500.0 + xc[:, 0]).rho, np.ones(24))


def test_cfl_time_step(wlib):
    w = wlib
    from wave_fenics_amd import linear_gll, medium
    # a uniform medium gives the homogeneous function's result
    for n, hi, p in (((4, 3, 5), (0.01, 0.01, 0.02), 2), ((3, 3, 3), (1.0, 2.0, 0.5), 4)):
        mesh = w.create_box(n, hi=hi, perturb=0.15)
        got = medium.cfl_time_step(mesh, p, medium.Medium(np.full(mesh.ncells, 1500.0)), 0.5e6, 0.25)
        assert got == linear_gll.cfl_time_step(mesh, p, 1500.0, 0.5e6, 0.25)
    # two speeds, differing cell sizes: three slabs in x of widths 1, 4, 2 (y and z extents 1): diameters sqrt(3),
    # sqrt(18), sqrt(6); speeds 1, 3, 3: crossing times 1.73, 1.41, 0.82 -> the limiting cell is the LAST one: not the
    # smallest cell (slab 0, in the slow medium), and of the two cells of the fast medium the smaller one
    x = mh.ich.lattice_x(np.array([0.0, 1.0, 5.0, 7.0]), np.array([0.0, 1.0]), np.array([0.0, 1.0]))
    mesh = mh.ich.box_with((3, 1, 1), x=x)
    med = medium.Medium([1.0, 3.0, 3.0])
    h = medium.cell_diameters(mesh)
    assert np.allclose(h, np.sqrt([3.0, 18.0, 6.0]))
    limiting = int(np.argmin(h / med.c))
    assert limiting == 2 and limiting != int(np.argmin(h)) and limiting != int(np.argmax(med.c))
    dt, spp = medium.cfl_time_step(mesh, 2, med, 0.01, 0.5)
    raw = 0.5 * (np.sqrt(6.0) / 3.0) / 4.0
    assert spp == int(100.0 / raw + 1) and dt == 100.0 / spp and dt <= raw


# ---------------------------------------------------------------------------------------------------------------------
# weighted facet mass
# ---------------------------------------------------------------------------------------------------------------------
TAGS = {0: 1, 1: 2, 2: 2, 3: 2, 4: 2, 5: 2}


def _numpy_facet_mass(oracle, om, tag, weight):
    """an independent sum: facet by facet, each facet's oracle mass times the weight of its cell"""
    m = np.zeros(om.ndofs)
    for cells, lf, t in oracle.box_facets(om):
        if t != tag:
            continue
        for c in cells:
            m += weight[c] * _facet_of_cell(oracle, om, int(c), lf)
    return m


def _facet_of_cell(oracle, om, c, lf):
    """the collocated mass of local face lf of cell c, from the formula w_a w_b |t_a x t_b|"""
    p, n = om.p, om.p + 1
    pts, wts = oracle.gll_points_weights(n)
    axis, side = lf // 2, lf % 2
    ta, tb = [d for d in range(3) if d != axis]
    out = np.zeros(om.ndofs)
    xv = om.x[om.geom_dofmap[c]]
    for b in range(n):
        for a in range(n):
            X = np.zeros((1, 3))
            X[0, axis], X[0, ta], X[0, tb] = float(side), pts[a], pts[b]
            _, dphi = oracle.cmap_tabulate(X)
            J = np.einsum("vi,jv->ij", xv, dphi[:, 0, :])
            l = [0, 0, 0]
            l[axis], l[ta], l[tb] = side * p, a, b
            out[om.dofmap[c, l[0] + n * (l[1] + n * l[2])]] += wts[a] * wts[b] * np.linalg.norm(np.cross(J[:, ta], J[:, tb]))
    return out


@pytest.mark.parametrize("p", [2, 3])
def test_weighted_facet_mass(oracle, wlib, tmp_path, p):
    w = wlib
    from wave_fenics_amd import linear_gll, mesh_io
    n = (3, 2, 4)
    mesh = w.create_box(n, perturb=0.2)
    V = w.create_functionspace(mesh, p)
    om = oracle.create_box(n, p, perturb=0.2)
    weight = mh.field("slab", mesh.x, mesh.geom_dofmap, cut_fraction=0.5) / 8.0 + 0.25
    assert np.unique(weight).size == 2
    for tag in (1, 2):
        i0, m0 = linear_gll.facet_lumped_mass(V, TAGS, tag)
        i1, m1 = linear_gll.facet_lumped_mass(V, TAGS, tag, np.ones(mesh.ncells))
        assert np.array_equal(i0, i1) and np.array_equal(mh.bits(m0), mh.bits(m1))      # weight 1: bit for bit
        iw, mw = linear_gll.facet_lumped_mass(V, TAGS, tag, weight)
        ref = _numpy_facet_mass(oracle, om, tag, weight)
        assert np.array_equal(iw, i0) and np.array_equal(np.nonzero(ref)[0], iw)
        assert np.abs(mw - ref[iw]).max() <= 1e-14 * np.abs(ref).max()
        assert np.abs(mw - m0).max() > 1e-3 * np.abs(m0).max()                           # the weight is felt
    # the host function for meshes read from a file, on the box written to and read from XDMF
    lat = np.arange(mesh.x.shape[0]).reshape(n[2] + 1, n[1] + 1, n[0] + 1)
    faces = {0: lat[:, :, 0], 1: lat[:, :, -1], 2: lat[:, 0, :], 3: lat[:, -1, :], 4: lat[0], 5: lat[-1]}
    fv, vals = [], []
    for lf, plane in faces.items():
        for i in range(plane.shape[0] - 1):
            for j in range(plane.shape[1] - 1):
                fv.append([plane[i, j], plane[i, j + 1], plane[i + 1, j], plane[i + 1, j + 1]])
                vals.append(TAGS[lf])
    tags = mesh_io.MeshTags(np.asarray(fv, dtype=np.int32), np.asarray(vals, dtype=np.int32))
    path = str(tmp_path / "box.xdmf")
    mesh_io.write_mesh(path, "mesh", mesh, "boundaries", tags)
    fmesh, ftags = mesh_io.read_mesh(path, "mesh", "boundaries")
    assert np.array_equal(fmesh.geom_dofmap, mesh.geom_dofmap)      # same cell order: the weight applies as it is
    FV = mesh_io.create_functionspace(fmesh, p)
    ob = oracle.BoxMesh(n, p, fmesh.x, fmesh.geom_dofmap, FV.dofmap, FV.ndofs, None)
    for tag in (1, 2):
        facets = mesh_io.locate_facets(fmesh, ftags, tag)
        i0, m0 = mesh_io.facet_lumped_mass(FV, facets)
        i1, m1 = mesh_io.facet_lumped_mass(FV, facets, np.ones(fmesh.ncells))
        assert np.array_equal(i0, i1) and np.array_equal(mh.bits(m0), mh.bits(m1))
        iw, mw = mesh_io.facet_lumped_mass(FV, facets, weight)
        ref = np.zeros(FV.ndofs)
        for c, axis, side in facets:
            ref += weight[c] * _facet_of_cell(oracle, ob, c, 2 * axis + side)
        assert np.array_equal(iw, np.nonzero(ref)[0])
        assert np.abs(mw - ref[iw]).max() <= 1e-14 * np.abs(ref).max()
    (sa, sb) = mesh_io.boundary_sets(FV, ftags, cell_weight=weight)
    assert np.array_equal(sb[0], iw) and np.array_equal(mh.bits(sb[1]), mh.bits(mw))
    # the file's sets are the tag-derived sets of the box, dof for dof (the two spaces number the same dofs; matched by
    # their coordinates): what LinearGLLOpt(..., boundary=, medium=) gets is what it derives itself from tags
    f_of_box = mh.dof_match(oracle.dof_coordinates(om), FV.dof_coordinates)
    for k, tag in enumerate((1, 2)):
        ib, mb = linear_gll.facet_lumped_mass(V, TAGS, tag, weight)
        dense = np.zeros(FV.ndofs)
        dense[f_of_box[ib]] = mb
        fi, fm = (sa, sb)[k]
        assert np.array_equal(np.nonzero(dense)[0], fi)
        assert np.array_equal(mh.bits(fm), mh.bits(dense[fi]))       # one loop behind both paths, the facets in one order
