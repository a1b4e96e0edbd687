"""Cell forms on the device (wf_cell_form, csrc/cell_form.hip) against the long-double reference of
tests/cell_form_helpers.py: every cell within B eps mag_c + gerr_c, B derived there; bits where the contract says bits.

Shapes: per degree the perturbed box cf.GPU_BOX -- at least three batches of CB = 256 // (P+1)^2 cells with a partial
last one -- and its first 1, CB and CB + 1 cells; small affine boxes for the per-cell form."""
import numpy as np
import pytest

import cell_form_helpers as cf
import frame_helpers as fh
import hex_geometry_helpers as hg
import stiffness_entry_helpers as se
from guard_helpers import NAN, batch_pad, guarded
from support import EPS, LD, bits, cells_per_batch, dev, gpu  # noqa: F401

pytestmark = pytest.mark.gpu
DEGREES = (1, 2, 3, 4, 5, 6, 7)
PARAMS = {"c0": cf.C0}


def form_of(V, p, kind="stiffness", **kw):
    import wave_fenics_amd as w
    return w.operators.CellForm(V, p, kind=kind, params=PARAMS, **kw)


def run(form, lam, u, gpu, **kw):
    """e on the host"""
    import torch
    out = form.eval(dev(lam, gpu), dev(u, gpu), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(tag, got, ref, mag, gerr, B, base=None):
    plain, ok, at, used = cf.cell_check(got, ref, mag, gerr, B, base)
    print(f"CELLFORM {tag}: B {B}, worst {plain:.2f} eps mag, allowance used {used:.3f}")
    assert ok, (tag, at, plain, B)


def decay_pair(om, p):
    """one twelve-decade decay for each of lambda and u (fields() of the entry tests)"""
    names, X, _ = se.fields(om, p, False, seed=31 + p)
    return X[names.index("decay-x+")], X[names.index("decay-y-")]


# ---------------------------------------------------------------------------------------------------------------------
# 1. stiffness, per point
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", DEGREES)
def test_stiffness_per_point(gpu, p):
    d = cf.data(p, cf.GPU_BOX[p])
    assert d.margin >= se.MARGIN
    CB, nc = cells_per_batch(p), d.om.ncells
    assert nc >= 2 * CB + 1 and nc % CB != 0
    B = cf.bound("point", p)
    Vu = cf.unstructured(d.V)
    form = form_of(Vu, p)
    assert form.geometry == "per_point" and form.info.num_cells == nc and form.info.cell_coeff == 0
    nd = (p + 1) ** 3
    assert form.info.alg_bytes == nc * 48.0 * nd + 4.0 * nd * nc + 8.0 * nc + 16.0 * d.om.ndofs
    full = run(form, d.lam, d.u, gpu)
    check(f"point P{p} uniform", full, d.ref, d.mag, d.gerr, B)
    lam, u = decay_pair(d.om, p)
    ref, mag, gerr = cf.stiffness_reference(d.om, p, d.geo, lam, u)
    assert float(mag.max() / mag[mag > 0].min()) > 1e6          # quiet cells next to loud ones
    check(f"point P{p} decay", run(form, lam, u, gpu), ref, mag, gerr, B)
    form.close()
    # one cell, exactly one batch, one batch and a cell: the reference of a cell does not depend on its neighbours
    for k in (1, CB, CB + 1):
        sub = form_of(cf.subset_space(Vu, np.arange(k)), p)
        got = run(sub, d.lam, d.u, gpu)
        assert got.shape == (k,)
        check(f"point P{p} first {k} cells", got, d.ref[:k], d.mag[:k], d.gerr[:k], B)
        assert np.array_equal(bits(got), bits(full[:k])), k
        sub.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. per-cell geometry on affine boxes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["graded", "sheared"])
@pytest.mark.parametrize("p", DEGREES)
def test_stiffness_per_cell(gpu, p, kind):
    n = cf.AFFINE_BOX[p]
    dc = cf.data(p, n, "cell", kind)
    dp = cf.data(p, n, "point", kind)
    off = np.abs(dc.geo.G[..., 0, 1]).max()
    assert (off > 0) == (kind == "sheared")                     # the sheared box has off-diagonals, the graded one none
    auto = form_of(dc.V, p)
    point = form_of(dc.V, p, tuning={"geometry": "per_point"})
    forced = form_of(dc.V, p, tuning={"geometry": "per_cell"})
    assert (auto.geometry, point.geometry, forced.geometry) == ("per_cell", "per_point", "per_cell")
    nd, nc = (p + 1) ** 3, dc.om.ncells
    assert auto.info.alg_bytes == nc * 48.0 + 4.0 * nd * nc + 8.0 * nc + 16.0 * dc.om.ndofs
    assert auto.info.device_bytes < point.info.device_bytes
    Bc, Bp = cf.bound("cell", p), cf.bound("point", p)
    ec, ep = run(auto, dc.lam, dc.u, gpu), run(point, dc.lam, dc.u, gpu)
    check(f"cell P{p} {kind}", ec, dc.ref, dc.mag, dc.gerr, Bc)
    check(f"cell P{p} {kind} per point", ep, dp.ref, dp.mag, dp.gerr, Bp)
    assert np.array_equal(bits(run(forced, dc.lam, dc.u, gpu)), bits(ec))
    both = (LD(Bc) * LD(EPS) * dc.mag + dc.gerr) + (LD(Bp) * LD(EPS) * dp.mag + dp.gerr)
    assert np.all(np.abs(ec.astype(LD) - ep.astype(LD)) <= both)
    for f in (auto, point, forced):
        f.close()


def test_per_cell_request_on_a_perturbed_box(gpu):
    import wave_fenics_amd as w
    d = cf.data(2, cf.GPU_BOX[2])
    for V in (d.V, cf.unstructured(d.V)):
        with pytest.raises(w.WavehipError) as e:
            form_of(V, 2, tuning={"geometry": "per_cell"})
        assert e.value.status == -1 and "WF_GEOMETRY_PER_CELL: cell " in str(e.value) and "not affine" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------
# 3. lumped mass
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", DEGREES)
def test_lumped(gpu, p):
    d = cf.data(p, cf.GPU_BOX[p])
    B = cf.bound("lumped", p)
    ref, mag, gerr = cf.lumped_reference(d.om, p, d.lam, d.u)
    form = form_of(cf.unstructured(d.V), p, "mass_lumped", tuning={"geometry": "per_cell"})   # the field is ignored
    assert form.geometry == "none"
    nd, nc = (p + 1) ** 3, d.om.ncells
    assert form.info.alg_bytes == nc * (12.0 * nd + 8.0) + 16.0 * d.om.ndofs
    check(f"lumped P{p}", run(form, d.lam, d.u, gpu), ref, mag, gerr, B)
    form.close()


@pytest.mark.parametrize("p", [2, 5])
def test_lumped_on_mirrored_cells(gpu, p):
    from wave_fenics_amd import _lib
    c = hg.mesh_case("half_mirrored", p)
    lam, u = cf.pair(c.om.ndofs, 7 + p)
    B = cf.bound("lumped", p)
    signs = {}
    for use_fabs in (True, False):
        ref, mag, gerr = cf.lumped_reference(c.om, p, lam, u, use_fabs=use_fabs)
        form = form_of(c.V, p, "mass_lumped", flags=0 if use_fabs else _lib.WF_FLAG_NO_FABS)
        got = run(form, lam, u, gpu)
        check(f"lumped mirrored P{p} fabs={use_fabs}", got, ref, mag, gerr, B)
        signs[use_fabs] = got
        form.close()
    flipped = signs[True] != signs[False]
    assert flipped.any() and not flipped.all()                  # the mirrored half changes sign, the other does not
    assert np.array_equal(bits(signs[True][flipped]), bits(-signs[False][flipped]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. coefficient
# ---------------------------------------------------------------------------------------------------------------------
def coefficient(coords):
    a = se.checkerboard(coords).astype(np.float64)
    a[1], a[2] = 0.0, -3.0
    return a


@pytest.mark.parametrize("p,kind,what", [(2, "perturbed", "point"), (4, "perturbed", "point"), (3, "sheared", "cell"),
                                         (2, "perturbed", "lumped"), (5, "perturbed", "lumped")])
def test_cell_coefficient(gpu, p, kind, what):
    n = cf.GPU_BOX[p] if kind == "perturbed" else cf.AFFINE_BOX[p]
    d = cf.data(p, n, "cell" if what == "cell" else "point", kind)
    a = coefficient(d.coords)
    assert a[1] == 0 and a[2] < 0 and a.max() == se.CONTRAST
    if what == "lumped":
        ref, mag, gerr = cf.lumped_reference(d.om, p, d.lam, d.u, a)
        form = form_of(d.V, p, "mass_lumped", cell_coeff=a)
    else:
        ref, mag, gerr = cf.stiffness_reference(d.om, p, d.geo, d.lam, d.u, a)
        form = form_of(d.V, p, cell_coeff=a)
        assert form.geometry == ("per_cell" if what == "cell" else "per_point")
    assert form.info.cell_coeff == 1
    got = run(form, d.lam, d.u, gpu)
    check(f"coefficient P{p} {what}", got, ref, mag, gerr, cf.bound(what, p))
    assert got[1] == 0.0
    form.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. alpha, accumulate, lambda is u; guarded buffers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,what", [(4, "point"), (2, "point"), (3, "cell"), (4, "lumped")])
def test_alpha_accumulate_alias_in_guarded_buffers(gpu, p, what):
    import torch
    kind = "sheared" if what == "cell" else "perturbed"
    n = cf.AFFINE_BOX[p] if what == "cell" else cf.GPU_BOX[p]
    d = cf.data(p, n, "cell" if what == "cell" else "point", kind)
    B = cf.bound(what, p)
    form = form_of(d.V, p, "mass_lumped" if what == "lumped" else "stiffness")
    pad = batch_pad((p + 1) ** 3)

    def reference(lam, u):
        if what == "lumped":
            return cf.lumped_reference(d.om, p, lam, u)
        return cf.stiffness_reference(d.om, p, d.geo, lam, u)
    alpha = -0.75
    for alias in (False, True):
        lam_h = d.u if alias else d.lam
        ref, mag, gerr = reference(lam_h, d.u)
        base = np.random.default_rng(5).uniform(-1, 1, d.om.ncells) * np.asarray(mag, dtype=np.float64)
        u_t, gu = guarded(d.u, pad, 0, NAN, gpu)
        lam_t, gl = (u_t, gu) if alias else guarded(d.lam, pad, 1, NAN, gpu)
        for accumulate in (False, True):
            out_t, go = guarded(base, pad, 1, NAN, gpu)
            ret = form.eval(lam_t, u_t, out=out_t, alpha=alpha, accumulate=accumulate)
            torch.cuda.synchronize()
            assert ret is out_t
            assert go.intact() and gu.intact() and gl.intact(), (go.changed(), gu.changed(), gl.changed())
            assert np.array_equal(bits(u_t.cpu().numpy()), bits(d.u)) and np.array_equal(bits(lam_t.cpu().numpy()), bits(lam_h))
            check(f"alpha P{p} {what} alias={alias} accumulate={accumulate}", out_t.cpu().numpy(), LD(alpha) * ref, abs(alpha) * mag,
                  abs(alpha) * gerr, B, base if accumulate else None)
    form.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,what", [(4, "point"), (2, "point"), (4, "lumped"), (2, "cell")])
def test_bits_repeat_permute_submesh(gpu, p, what):
    kind = "sheared" if what == "cell" else "perturbed"
    n = cf.AFFINE_BOX[p] if what == "cell" else cf.GPU_BOX[p]
    d = cf.data(p, n, "cell" if what == "cell" else "point", kind)
    k = "mass_lumped" if what == "lumped" else "stiffness"
    Vu = cf.unstructured(d.V)
    nc, CB = d.om.ncells, cells_per_batch(p)
    a = fh.coefficient(nc)
    form = form_of(Vu, p, k, cell_coeff=a)
    first = run(form, d.lam, d.u, gpu)
    assert np.array_equal(bits(run(form, d.lam, d.u, gpu)), bits(first))
    form.close()
    order = fh.cell_shuffle(nc)
    shuffled = form_of(cf.subset_space(Vu, order), p, k, cell_coeff=a[order])
    assert np.array_equal(bits(run(shuffled, d.lam, d.u, gpu)), bits(first[order]))
    shuffled.close()
    for c in sorted({0, min(CB - 1, nc - 1), min(CB, nc - 1), nc - 1}):
        one = form_of(cf.subset_space(Vu, [c]), p, k, cell_coeff=a[[c]])
        assert np.array_equal(bits(run(one, d.lam, d.u, gpu)), bits(first[[c]])), c
        one.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. frames and meshes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [2, 3])
def test_caller_frame_gives_the_canonical_bits(gpu, p):
    import wave_fenics_amd as w
    from wave_fenics_amd import _lib
    c = fh.mesh_case("box", p)
    f = fh.frame("xslow+perm", p)
    lam, u = cf.pair(c.om.ndofs, 40 + p)
    Vc = w.FunctionSpace(c.mesh, p, fh.caller_dofmap(c.V.dofmap, f.perm, True).astype(np.int32), w.IndexMap(c.om.ndofs), None,
                         structured=False)
    K = fh.stiffness_canon("box", p)
    canon = {"G": K.G, "detJ": K.detJ}
    caller = fh.caller_inputs(canon, f.perm, True)
    flags = _lib.WF_FLAG_TENSOR_X_SLOWEST
    pairs = ((form_of(c.V, p), form_of(Vc, p, perm=f.perm, flags=flags)),
             (form_of(c.V, p, G=canon["G"]), form_of(Vc, p, G=caller["G"], perm=f.perm, flags=flags)),
             (form_of(c.V, p, "mass_lumped"), form_of(Vc, p, "mass_lumped", perm=f.perm, flags=flags)),
             (form_of(c.V, p, "mass_lumped", detJ=canon["detJ"]),
              form_of(Vc, p, "mass_lumped", detJ=caller["detJ"], perm=f.perm, flags=flags)))
    for twin, framed in pairs:
        e = run(twin, lam, u, gpu)
        assert np.abs(e).min() > 0
        assert np.array_equal(bits(run(framed, lam, u, gpu)), bits(e))
        twin.close()
        framed.close()


@pytest.mark.parametrize("p", [2, 5])
def test_holed_mesh_with_unnamed_dofs(gpu, p):
    V, om, _ = se.holed_mesh(p)
    geo = se.geometry_ld(om, p, "point")
    assert geo.margin >= se.MARGIN
    named = np.zeros(om.ndofs, dtype=bool)
    named[np.asarray(om.dofmap).reshape(-1)] = True
    assert not named.all()
    lam, u = (v.copy() for v in cf.pair(om.ndofs, 50 + p))
    ref, mag, gerr = cf.stiffness_reference(om, p, geo, np.where(named, lam, 0.0), np.where(named, u, 0.0))
    lam[~named] = np.nan                                          # dofs no cell names are never read
    u[~named] = np.nan
    form = form_of(V, p)
    check(f"holed P{p}", run(form, lam, u, gpu), ref, mag, gerr, cf.bound("point", p))
    form.close()
    lform = form_of(V, p, "mass_lumped")
    ref, mag, gerr = cf.lumped_reference(om, p, np.where(named, lam, 0.0), np.where(named, u, 0.0))
    check(f"holed lumped P{p}", run(lform, lam, u, gpu), ref, mag, gerr, cf.bound("lumped", p))
    lform.close()


@pytest.mark.parametrize("p", [2, 3])
def test_randomly_reoriented_cells(gpu, p):
    c = fh.mesh_case("sheared_random", p)
    lam, u = cf.pair(c.om.ndofs, 60 + p)
    for tuning, what in ((None, "cell"), ({"geometry": "per_point"}, "point")):
        geo = se.geometry_ld(c.om, p, what)
        assert geo.margin >= se.MARGIN
        ref, mag, gerr = cf.stiffness_reference(c.om, p, geo, lam, u)
        form = form_of(c.V, p, tuning=tuning)
        assert form.geometry == "per_" + what
        check(f"reoriented P{p} {what}", run(form, lam, u, gpu), ref, mag, gerr, cf.bound(what, p))
        form.close()


@pytest.mark.parametrize("p,kind,k", [(4, "perturbed", "stiffness"), (3, "sheared", "stiffness"), (2, "graded", "stiffness"),
                                      (4, "perturbed", "mass_lumped")])
def test_box_entry_point_is_the_dofmap_entry_point(gpu, p, kind, k):
    n = cf.GPU_BOX[p] if kind == "perturbed" else cf.AFFINE_BOX[p]
    d = cf.data(p, n, "point", kind)
    a = fh.coefficient(d.om.ncells)
    box, dofmap = form_of(d.V, p, k, cell_coeff=a), form_of(cf.unstructured(d.V), p, k, cell_coeff=a)
    assert getattr(d.V, "structured", False) and box.geometry == dofmap.geometry
    assert box.info.device_bytes == dofmap.info.device_bytes
    assert np.array_equal(bits(run(box, d.lam, d.u, gpu)), bits(run(dofmap, d.lam, d.u, gpu)))
    box.close()
    dofmap.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. the identity the feature exists for
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [2, 4])
def test_form_is_the_derivative_of_the_operator(gpu, p):
    import torch
    import wave_fenics_amd as w
    d = cf.data(p, cf.GPU_BOX[p])
    nc, CB = d.om.ncells, cells_per_batch(p)
    Bf, Ba = cf.bound("point", p), se.bound("point", p)
    Vu = cf.unstructured(d.V)
    form = form_of(Vu, p)
    e = run(form, d.lam, d.u, gpu).astype(LD)
    form.close()
    lam = np.asarray(d.lam).astype(LD)
    x = dev(d.u, gpu)

    def apply(V, structured, a):
        op = w.StiffnessOperator(V, p, PARAMS, structured=structured, cell_coeff=a)      # the library's own kernel choice
        y = torch.zeros(d.om.ndofs, dtype=torch.float64, device=gpu)
        op(x, y)
        torch.cuda.synchronize()
        op.close()
        return y.cpu().numpy().astype(LD)
    drawn = int(np.random.default_rng(p).integers(1, nc - 1))
    for c in sorted({0, CB - 1, CB, nc - 1, drawn}):
        a = np.zeros(nc)
        a[c] = 1.0
        # y = K_c u entry by entry within B_apply eps mag_i + gerr_i, and sum_i |lambda_i| mag_i = mag_c
        allowed = LD(Bf + Ba) * LD(EPS) * d.mag[c] + 2 * d.gerr[c]
        for V, structured in ((Vu, False), (d.V, True)):
            ly = (lam * apply(V, structured, a)).sum()
            assert abs(ly - e[c]) <= allowed, (p, c, structured, float(abs(ly - e[c]) / (LD(EPS) * d.mag[c])))
    a = coefficient(d.coords)
    absa = np.abs(a).astype(LD)
    allowed = LD(Bf + Ba) * LD(EPS) * (absa * d.mag).sum() + 2 * (absa * d.gerr).sum()
    total = (a.astype(LD) * e).sum()
    for V, structured in ((Vu, False), (d.V, True)):
        ly = (lam * apply(V, structured, a)).sum()
        assert abs(ly - total) <= allowed, (p, structured, float(abs(ly - total) / allowed))


# ---------------------------------------------------------------------------------------------------------------------
# 9. streams
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["point", "lumped"])
def test_two_streams_one_handle(gpu, what):
    import torch
    p = 4
    d = cf.data(p, cf.GPU_BOX[p])
    form = form_of(d.V, p, "mass_lumped" if what == "lumped" else "stiffness")
    lam, u = dev(d.lam, gpu), dev(d.u, gpu)
    serial = (form.eval(lam, u).cpu().numpy(), form.eval(u, u, alpha=2.0).cpu().numpy())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    o1, o2 = torch.empty_like(lam[:d.om.ncells]), torch.empty_like(lam[:d.om.ncells])
    torch.cuda.synchronize()
    for _ in range(4):
        with torch.cuda.stream(s1):
            form.eval(lam, u, out=o1)
        with torch.cuda.stream(s2):
            form.eval(u, u, out=o2, alpha=2.0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(o1.cpu().numpy()), bits(serial[0])) and np.array_equal(bits(o2.cpu().numpy()), bits(serial[1]))
    form.close()
