"""The hexahedral geometry set-up on the device against a long-double reference (tests/hex_geometry_helpers.py):
k_geometry_hex, k_geometry_hex_slots and k_geometry_box of csrc/hex_geometry.hip, every flag combination, both clamp windows,
the per-cell upload of the box operator and its fall-back to per-point geometry.

a. k_geometry_hex entry by entry (precompute_geometric_data): every G entry and det J w within the helper's bound of
   the long-double value -- 2 x the first-order running error of the float64 evaluation, derived in the helper, never
   moved --; where the clamp acts the value is exactly 0.0 / 1.0 / -1.0, and it acts on exactly the reference's mask.
b. the same through wf_geometry_hex_rule at a caller's rule whose coordinate-map derivatives meet both windows, and at
   a Gauss rule with nq1 != P + 1.
c. box operators: y against the oracle's sum-factorised apply fed with the long-double G (1e-12 of max|y|), on meshes
   where the clamp acts: the fall-back of the default path to per-point geometry, per-cell geometry under
   WF_FLAG_NO_CLAMP, the refusals, the k-split and block kernels, the lumped mass diagonals on mirrored cells, and the
   order "clamp first, then cell coefficient".
d. dofmap operators: k_geometry_hex_slots (marching) and k_geometry_hex (batch, element-wise) on the same meshes,
   mirrored cells in random orientations included.
e. the host rule's promise: where it allows per-cell geometry the device's per-point G is the same, bit for bit, with
   and without the clamp; where the long-double clamp acts the two differ.  Components that are 0 in exact arithmetic
   are set apart: from degree 3 on the unclamped kernel leaves a rounding residue there (x_v dphi_v + s contracted into
   an fma no longer cancels exactly), which the clamp turns into the exact 0.0 of G_c -- that is asserted instead.

test_hex_geometry_host.py holds the conditions under which these comparisons mean something (window margin, mask counts,
headroom of the bound, discrimination of the operator references).  test_report_worst_ratios prints the worst
|got - ref| / bound per kernel: a record."""
import numpy as np
import pytest

import hex_geometry_helpers as h
from support import bits, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

LD = h.LD
INVALID, UNSUPPORTED = -1, -2     # wf_status
WORST = {}                        # (kernel, case name) -> (worst |got - ref| / bound on the device, case)


def record(kernel, case, got, ref, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, np.abs(got.astype(LD) - ref) / bound, 0.0)
    worst = float(ratio.max())
    if worst > WORST.get((kernel, case[0]), (-1.0, None))[0]:
        WORST[kernel, case[0]] = (worst, case)
    return worst


def check_entries(kernel, case, G, detJ, r, G_plain=None):
    """G, detJ: device arrays at the flags of the reference r.  G_plain: the device's G without the clamp when r is a
    clamped reference -- the entries the clamp changed on the device are then exactly r's mask."""
    worst = record(kernel, case, detJ, r.detJw, r.detJw_bound)
    assert np.all(np.abs(detJ.astype(LD) - r.detJw) <= r.detJw_bound), (case, "detJ", worst)
    worst = record(kernel, case, G, r.G, r.G_bound)
    assert np.all(np.abs(G.astype(LD) - r.G) <= r.G_bound), (case, "G", worst)
    # symmetry: the kernel sums (Ji[a][k] d) Ji[b][k], which is not the same rounding as (Ji[b][k] d) Ji[a][k]
    Gt = np.swapaxes(G, -1, -2)
    assert np.all(np.abs(G.astype(LD) - Gt.astype(LD)) <= r.G_bound + np.swapaxes(r.G_bound, -1, -2)), (case, "symmetry")
    inside = r.G_mask | r.G_near
    if inside.any():   # bit for bit the window's constant (+0.0, not -0.0)
        assert np.array_equal(bits(G[inside]), bits(r.G[inside].astype(np.float64))), (case, "clamped entries")
    if G_plain is not None:
        acted = bits(G) != bits(G_plain)
        assert np.array_equal(acted & ~r.G_near, r.G_mask), (case, int(acted.sum()), int(r.G_mask.sum()))
        assert not (acted & ~inside).any(), (case, "the clamp acted outside the windows")


# ---------------------------------------------------------------------------------------------------------------------
# a. k_geometry_hex, entry by entry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_fabs", [True, False], ids=["fabs", "signed"])
@pytest.mark.parametrize("name", h.MESHES)
@pytest.mark.parametrize("p", h.DEGREES)
def test_geometry_hex_entries(gpu, p, name, use_fabs):
    import wave_fenics_amd as w
    c = h.mesh_case(name, p)
    Gp, dp = w.precompute_geometric_data(c.mesh, p, use_fabs, False)
    Gc, dc = w.precompute_geometric_data(c.mesh, p, use_fabs, True)
    check_entries("k_geometry_hex", (name, p, use_fabs, False), Gp, dp, h.reference(name, p, use_fabs, False))
    check_entries("k_geometry_hex", (name, p, use_fabs, True), Gc, dc, h.reference(name, p, use_fabs, True), G_plain=Gp)
    assert np.array_equal(bits(dp), bits(dc))   # the clamp of G leaves det J w alone (no dphi is clamped at a GLL rule)
    if name in ("mirrored", "unit_negative"):
        assert np.all(dp < 0.0) if not use_fabs else np.all(dp > 0.0)
    if name == "half_mirrored" and not use_fabs:
        assert (dp < 0.0).any() and (dp > 0.0).any()


@pytest.mark.parametrize("name", ["perturbed", "tiny"])
def test_geometry_hex_partial_workgroup_at_P3(gpu, name):
    """18 cells of 64 points: 4.5 workgroups (the 12 cells above fill 3)"""
    import wave_fenics_amd as w
    n = h.N_P3_PARTIAL
    c = h.mesh_case(name, 3, n)
    assert (c.mesh.ncells * 64) % 256 != 0
    Gp, dp = w.precompute_geometric_data(c.mesh, 3, True, False)
    Gc, dc = w.precompute_geometric_data(c.mesh, 3, True, True)
    check_entries("k_geometry_hex", (name, 3, True, False, n), Gp, dp, h.reference(name, 3, True, False, n))
    check_entries("k_geometry_hex", (name, 3, True, True, n), Gc, dc, h.reference(name, 3, True, True, n), G_plain=Gp)


def test_geometry_hex_without_G(gpu):
    """want_G = False (the mass operators' call): det J w alone, the same bits"""
    import wave_fenics_amd as w
    c = h.mesh_case("half_mirrored", 3)
    _, d = w.precompute_geometric_data(c.mesh, 3, False, True)
    G0, d0 = w.precompute_geometric_data(c.mesh, 3, False, True, want_G=False)
    assert G0 is None and np.array_equal(bits(d), bits(d0))


# ---------------------------------------------------------------------------------------------------------------------
# b. wf_geometry_hex_rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_fabs", [True, False], ids=["fabs", "signed"])
@pytest.mark.parametrize("which", ["caller", "gauss"])
def test_geometry_rule_entries(gpu, which, use_fabs):
    import wave_fenics_amd as w
    c, pts, wts = h.rule_case(which)
    assert len(pts) != c.p + 1
    Gp, dp = w.compute_geometry_rule(c.mesh, pts, wts, use_fabs, False, want_G=True)
    Gc, dc = w.compute_geometry_rule(c.mesh, pts, wts, use_fabs, True, want_G=True)
    plain, clamped = h.rule_reference(which, use_fabs, False), h.rule_reference(which, use_fabs, True)
    check_entries("k_geometry_hex (rule)", (which, use_fabs, False), Gp, dp, plain)
    # with clamped map derivatives J itself moves, so the clamp's action on G is not read off Gc != Gp here
    check_entries("k_geometry_hex (rule)", (which, use_fabs, True), Gc, dc, clamped)
    if which == "caller":   # the derivative clamp took effect, and only when asked to
        assert clamped.d_mask.any() and not np.array_equal(bits(dp), bits(dc))
    else:
        assert np.array_equal(bits(dp), bits(dc))
    _, d0 = w.compute_geometry_rule(c.mesh, pts, wts, use_fabs, True, want_G=False)
    assert np.array_equal(bits(d0), bits(dc))


# ---------------------------------------------------------------------------------------------------------------------
# c. box operators
# ---------------------------------------------------------------------------------------------------------------------
def flags_of(use_fabs, clamp):
    from wave_fenics_amd._lib import WF_FLAG_NO_CLAMP, WF_FLAG_NO_FABS
    return (0 if use_fabs else WF_FLAG_NO_FABS) | (0 if clamp else WF_FLAG_NO_CLAMP)


def apply_on(op, ref, gpu):
    import torch
    y = torch.from_numpy(ref.y0.copy()).to(gpu)
    op(torch.from_numpy(ref.x).to(gpu), y)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def assert_matches(op, ref, gpu, what):
    y = apply_on(op, ref, gpu)
    err = float(np.abs(y - ref.yref).max() / ref.scale)
    print(f"{what}: max|y - yref| / max|yref| = {err:.3e}")
    assert err <= h.TOL_ORACLE, (what, err)


def box_operator(name, p, clamp, tuning=None, cell_coeff=None):
    import wave_fenics_amd as w
    c = h.mesh_case(name, p, h.operator_n(p))
    return w.StiffnessOperator(c.V, p, {"c0": h.C0}, structured=True, flags=flags_of(h.operator_fabs(name), clamp),
                               tuning=tuning, cell_coeff=cell_coeff)


@pytest.mark.parametrize("name", h.BOX_OPERATOR_MESHES)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_box_falls_back_to_per_point_where_the_clamp_acts(gpu, p, name):
    op = box_operator(name, p, True)
    assert (op.kernel, op.geometry, op.update) == ("march_box", "per_point", "none")
    assert_matches(op, h.operator_reference(name, p, h.operator_fabs(name), True), gpu, (name, p, "default"))


@pytest.mark.parametrize("name", h.BOX_OPERATOR_MESHES)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_box_without_clamp_takes_per_cell_geometry(gpu, p, name):
    op = box_operator(name, p, False)
    assert (op.kernel, op.geometry, op.metric) == ("march_box", "per_cell", "axes")
    assert op.update == ("owner" if p == 4 else "atomic")
    assert_matches(op, h.operator_reference(name, p, h.operator_fabs(name), False), gpu, (name, p, "NO_CLAMP"))


@pytest.mark.parametrize("name", h.BOX_OPERATOR_MESHES)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_box_requests_refused_where_the_clamp_acts(gpu, p, name):
    import wave_fenics_amd as w
    with pytest.raises(w.WavehipError) as e:
        box_operator(name, p, True, tuning={"geometry": "per_cell"})
    assert e.value.status == INVALID and "clamp" in str(e.value), str(e.value)
    # choose_box_stiffness: no per-cell geometry, so no separable form for the owner update to run on
    with pytest.raises(w.WavehipError) as e:
        box_operator(name, p, True, tuning={"update": "owner"})
    assert e.value.status == UNSUPPORTED, str(e.value)
    assert "the owner update needs the separable (axes) form of the marching kernel" in str(e.value)
    # the same requests stand without the clamp
    assert box_operator(name, p, False, tuning={"geometry": "per_cell"}).geometry == "per_cell"
    assert box_operator(name, p, False, tuning={"update": "owner"}).update == "owner"


@pytest.mark.parametrize("clamp", [True, False], ids=["clamp", "NO_CLAMP"])
@pytest.mark.parametrize("name", h.BOX_OPERATOR_MESHES)
@pytest.mark.parametrize("p,tuning", [(5, None), (6, None), (7, None), (2, {"kernel": "box_block"})])
def test_box_per_point_kernels(gpu, p, tuning, name, clamp):
    op = box_operator(name, p, clamp, tuning=tuning)
    assert (op.kernel, op.geometry) == ("box_block" if tuning else "march_box", "per_point")
    assert_matches(op, h.operator_reference(name, p, h.operator_fabs(name), clamp), gpu, (name, p, tuning, clamp))


@pytest.mark.parametrize("name,p", h.COEFF_CASES)
def test_box_clamp_first_then_coefficient(gpu, name, p):
    c = h.mesh_case(name, p, h.operator_n(p))
    a = h.cell_coefficients(c.mesh.ncells)
    op = box_operator(name, p, True, cell_coeff=a)
    assert op.geometry == "per_point" and op.cell_coeff
    assert_matches(op, h.operator_reference(name, p, True, True, coeff="after"), gpu, (name, p, "clamp(G) a_c"))
    # and not clamp(G a_c): the host test shows the two references are 1e3 tolerances apart
    before = h.operator_reference(name, p, True, True, coeff="before")
    assert np.abs(apply_on(op, before, gpu) - before.yref).max() > h.TOL_ORACLE * before.scale


def lumped_diagonal(op, ndofs, gpu):
    import torch
    y = torch.zeros(ndofs, dtype=torch.float64, device=gpu)
    op(torch.ones(ndofs, dtype=torch.float64, device=gpu), y)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("p", [2, 5])
@pytest.mark.parametrize("name", ["mirrored", "half_mirrored"])
def test_lumped_mass_diagonal_on_mirrored_cells(gpu, name, p):
    """m = sum of det J w over the points that share a dof: |det J| for MassOperatorLumped, det J signed for
    SpectralMassOperator.  Bound: the entries' bounds plus the sum of at most 8 terms in any order, 7 u sum|terms|."""
    import wave_fenics_amd as w
    c = h.mesh_case(name, p)
    dm = np.asarray(c.V.dofmap).reshape(-1)
    for cls, use_fabs in ((w.MassOperatorLumped, True), (w.SpectralMassOperator, False)):
        op = cls(c.V, p)
        assert op.kernel == "diagonal"
        r = h.reference(name, p, use_fabs, False)
        ref, bound = np.zeros(c.V.ndofs, dtype=LD), np.zeros(c.V.ndofs, dtype=LD)
        np.add.at(ref, dm, r.detJw.reshape(-1))
        np.add.at(bound, dm, r.detJw_bound.reshape(-1) + 7 * h.U * np.abs(r.detJw.reshape(-1)))
        m = lumped_diagonal(op, c.V.ndofs, gpu)
        worst = record("lumped diagonal (%s)" % ("k_geometry_box" if c.structured else "k_geometry_hex"), (name, p, use_fabs),
                       m, ref, bound)
        assert np.all(np.abs(m.astype(LD) - ref) <= bound), (name, p, cls.__name__, worst)
        if use_fabs:
            assert np.all(m > 0.0)
        elif name == "mirrored":
            assert np.all(m < 0.0)
        else:
            assert (m < 0.0).any() and (m > 0.0).any()


# ---------------------------------------------------------------------------------------------------------------------
# d. dofmap operators
# ---------------------------------------------------------------------------------------------------------------------
KERNELS = {"march": "march_idx", "batch": "batch_unique", "elementwise": "elementwise"}


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", h.DOFMAP_MESHES)
@pytest.mark.parametrize("p", h.DOFMAP_DEGREES)
def test_dofmap_operators(gpu, p, name, kernel):
    import wave_fenics_amd as w
    for use_fabs, clamp, seed in h.dofmap_variants(name):
        c = h.mesh_case(name, p, h.DOFMAP_N[p], False, seed)
        op = w.StiffnessOperator(c.V, p, {"c0": h.C0}, structured=False, flags=flags_of(use_fabs, clamp),
                                 tuning={"kernel": kernel})
        assert (op.kernel, op.geometry) == (KERNELS[kernel], "per_point"), (op.kernel, op.geometry)
        if seed is not None and kernel == "march":
            assert op.info.plan_reoriented > 0   # the cell_sign branch of k_geometry_hex_slots
        ref = h.operator_reference(name, p, use_fabs, clamp, h.DOFMAP_N[p], False, seed)
        assert_matches(op, ref, gpu, (name, p, kernel, use_fabs, clamp, seed))


# ---------------------------------------------------------------------------------------------------------------------
# e. the host rule's promise on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", h.DEGREES)
def test_rule_promise_on_the_device(gpu, p):
    import wave_fenics_amd as w
    from types import SimpleNamespace
    for shape in h.SWEEP_SHAPES:
        mesh = h.sweep_mesh(shape)
        Gc, _ = w.precompute_geometric_data(mesh, p, True, True)
        Gp, _ = w.precompute_geometric_data(mesh, p, True, False)
        reason = np.zeros(mesh.ncells, dtype=int)
        for cell in range(mesh.ncells):
            one = SimpleNamespace(x=mesh.x[8 * cell:8 * cell + 8], geom_dofmap=np.arange(8, dtype=np.int32).reshape(1, 8))
            reason[cell] = w.hex_cell_geometry(one, p, use_fabs=True, clamp=True)[2]
        ref = h.sweep_acts(shape, p)
        near = np.broadcast_to(ref.near[:, None], Gc.shape)
        differ = bits(Gc) != bits(Gp)
        real = (differ & ~near).any(axis=(1, 2, 3))   # a component that is not a rounding residue changed
        print(f"P{p} {shape}: rule allows {int((reason == 0).sum())} cells, clamp acts on {int(ref.acts.sum())}, "
              f"device arrays differ on {int(real.sum())}; residues zeroed in {int((differ & near).any(axis=(1, 2, 3)).sum())} cells")
        assert (reason == 0).any() and ref.acts.any()
        assert not np.any(real[reason == 0]), (shape, p, h.SWEEP_FACTORS[(reason == 0) & real])
        assert np.all(real[ref.acts]), (shape, p, h.SWEEP_FACTORS[ref.acts & ~real])
        # the residues: the clamped array holds the 0.0 that G_c holds, whatever the unclamped one holds
        allowed = np.broadcast_to((reason == 0)[:, None, None, None], Gc.shape)
        assert np.array_equal(bits(Gc[near & allowed]), np.zeros(int((near & allowed).sum()), dtype=np.int64)), (shape, p)


def test_report_worst_ratios(gpu):
    """the record of the run: the worst |got - ref| / bound seen on the device per kernel and case (runs last; the bound
    is 1 in these units and stays there)"""
    for (kernel, name), (worst, case) in sorted(WORST.items()):
        print(f"worst |got - ref| / bound  {kernel:32s} {name:14s} {worst:.3f}  at {case}")
        assert worst <= 1.0
    for kernel in sorted({k for k, _ in WORST}):
        print(f"worst |got - ref| / bound  {kernel:32s} {max(v[0] for (k, _), v in WORST.items() if k == kernel):.3f}")
