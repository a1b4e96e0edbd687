"""Conditions on the reference of the hexahedral geometry tests (tests/hex_geometry_helpers.py), and the host rule
of per-cell geometry (csrc/hex_cell_geometry.cpp) against that reference.  No GPU.

These are what keeps tests/test_gpu_hex_geometry.py from hiding a failure: that float64 and long double take the same
side of every clamp window, that the clamp acts where the cases mean it to, that the bound is neither loose enough to
pass a wrong kernel nor tight enough to fail a right one, and that the operator references tell a clamped operator from
an unclamped one."""
from types import SimpleNamespace

import numpy as np
import pytest

import hex_geometry_helpers as h

MARGIN = 1e-3
# clamp mask counts per cell (helper docstring).  The perturbed family: off-diagonal entries of a perturbed cell at the
# points of the smallest weights drop below 1e-8 from degree 4 on (whole mesh, (3, 2, 2) cells).
TINY_PER_CELL = {1: 8, 2: 24, 3: 24, 4: 24, 5: 24, 6: 24, 7: 24}
UNIT_PER_CELL = {1: 24, 2: 18, 3: 72, 4: 18, 5: 72, 6: 24, 7: 24}
PERTURBED_TOTAL = {1: 0, 2: 0, 3: 0, 4: 48, 5: 210, 6: 614, 7: 1122}


def all_entry_cases():
    for p in h.DEGREES:
        for name in h.MESHES:
            for use_fabs, clamp in h.FLAGS:
                yield name, p, use_fabs, clamp


def gpu_test_references():
    """every reference the GPU tests compare against (clamp on): name, the reference"""
    for name, p, use_fabs, clamp in all_entry_cases():
        if clamp:
            yield (name, p, use_fabs), h.reference(name, p, use_fabs, True)
    for which in ("caller", "gauss"):
        for use_fabs in (True, False):
            yield (which, use_fabs), h.rule_reference(which, use_fabs, True)
    for name in ("perturbed", "tiny"):
        yield (name, 3, h.N_P3_PARTIAL), h.reference(name, 3, True, True, h.N_P3_PARTIAL)
    for name in h.BOX_OPERATOR_MESHES:
        for p in h.DEGREES:
            yield (name, p, "operator"), h.reference(name, p, h.operator_fabs(name), True, h.operator_n(p))
    for name in h.DOFMAP_MESHES:
        for p in h.DOFMAP_DEGREES:
            for use_fabs, clamp, seed in h.dofmap_variants(name):
                if clamp:
                    yield (name, p, "dofmap", use_fabs), h.reference(name, p, use_fabs, True, h.DOFMAP_N[p], False, seed)


def test_window_margin():
    worst = min((r.margin, key) for key, r in gpu_test_references())
    print("smallest window margin:", worst)
    assert worst[0] >= MARGIN, worst


def test_tiny_spacings_are_the_recorded_powers_of_two():
    assert [int(np.log2(h.tiny_h(p)[0])) for p in range(2, 8)] == [-20, -17, -15, -13, -12, -10]
    for p in range(2, 8):   # the two values nearest 1e-8 lie a factor 0.32 (P6) to 3.3 (P7) from it, on either side
        v = h.tiny_h(p)[0] * h.weight_products(p)
        assert 0.32e-8 <= v[0] < 0.6e-8 and 1.7e-8 < v[1] <= 3.3e-8, (p, v[:2])


@pytest.mark.parametrize("p", h.DEGREES)
def test_clamp_mask_counts(p):
    for name in h.MESHES:
        for use_fabs in (True, False):
            r = h.reference(name, p, use_fabs, True)
            nc = r.G.shape[0]
            count = int(r.G_mask.sum())
            assert not r.d_mask.any(), (name, p)   # a GLL rule's dphi are 0, +-1 or far from both
            mirrored = name in ("mirrored", "unit_negative")   # without |det J| the sign of G flips, the windows mirror
            if name == "tiny":
                assert count == nc * TINY_PER_CELL[p], (name, p, use_fabs, count / nc)
                diag = r.G_mask[:, :, [0, 1, 2], [0, 1, 2]]
                assert count == diag.sum() and (p == 1 or diag.sum(axis=(0, 2)).astype(bool).sum() == 8)
            elif name.startswith("unit"):
                assert count == nc * UNIT_PER_CELL[p], (name, p, use_fabs, count / nc)
                want = -1.0 if (mirrored and not use_fabs) else 1.0
                assert np.all(r.G[r.G_mask] == want)
            elif name in ("sheared", "anisotropic", "far"):
                assert count == 0, (name, p, count)
            else:   # perturbed, mirrored, half_mirrored: one set of cells, frames and signs differ
                assert count == PERTURBED_TOTAL[p], (name, p, use_fabs, count)
                assert np.all(r.G[r.G_mask] == 0.0)
    # without the clamp nothing is marked
    assert not h.reference("tiny", p, True, False).G_mask.any()


def test_caller_rule_meets_both_windows_of_the_map_derivatives():
    r = h.rule_reference("caller", True, True)
    c, pts, wts = h.rule_case("caller")
    plain = h.point_geometry_ld(c.mesh.x, c.mesh.geom_dofmap, pts, wts, True, False)
    assert r.d_mask.any() and not plain.d_mask.any()
    f = np.concatenate([1.0 - pts, pts])
    prod = np.outer(f, f).reshape(-1)   # |dphi| = f f' of two axes
    assert ((prod > 0) & (prod <= h.T0)).any() and ((prod < 1) & (np.abs(prod - 1) <= h.T1)).any()   # both windows
    assert (int(r.d_mask.sum()), int(r.G_mask.sum())) == (480, 388)   # the helper's record
    # J moved by far more than the bound
    assert np.abs(r.detJw - plain.detJw).max() > 1e3 * float(plain.detJw_bound.max())
    print("caller rule: dphi entries changed", int(r.d_mask.sum()), "G entries changed", int(r.G_mask.sum()))
    assert not h.rule_reference("gauss", True, True).d_mask.any()


def test_headroom_and_non_vacuity():
    """plain float64 numpy stays within half the bound on every entry; the bound is below 1e-9 of the cell's largest
    |G| except on `far`, whose bound is 2^10 times that of the same cells at offset 0 or more"""
    worst = 0.0
    for name, p, use_fabs, clamp in all_entry_cases():
        c, r = h.mesh_case(name, p), h.reference(name, p, use_fabs, clamp)
        G, d = h.point_geometry_f64(c.mesh.x, c.mesh.geom_dofmap, c.pts, c.wts, use_fabs, clamp)
        assert np.all(np.abs(G - r.G) <= 0.5 * r.G_bound), (name, p, use_fabs, clamp)
        assert np.all(np.abs(d - r.detJw) <= 0.5 * r.detJw_bound), (name, p, use_fabs, clamp)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(r.G_bound > 0, np.abs(G - r.G) / r.G_bound, 0.0)
        worst = max(worst, float(ratio.max()))
        nc = r.G.shape[0]
        rel = (r.G_bound.reshape(nc, -1).max(axis=1) / np.abs(r.G).reshape(nc, -1).max(axis=1)).max()
        assert rel < (1e-9 if name != "far" else 1e-6), (name, p, float(rel))
    print("float64 numpy against long double, worst |diff| / bound:", worst)
    for which in ("caller", "gauss"):
        c, pts, wts = h.rule_case(which)
        for use_fabs, clamp in h.FLAGS:
            r = h.rule_reference(which, use_fabs, clamp)
            G, d = h.point_geometry_f64(c.mesh.x, c.mesh.geom_dofmap, pts, wts, use_fabs, clamp)
            assert np.all(np.abs(G - r.G) <= 0.5 * r.G_bound) and np.all(np.abs(d - r.detJw) <= 0.5 * r.detJw_bound)
    for p in h.DEGREES:
        from support import lattice_x
        c, far = h.mesh_case("far", p), h.reference("far", p, True, False)
        x0 = lattice_x(*[np.arange(m + 1.0) for m in c.n])
        near = h.point_geometry_ld(x0, c.mesh.geom_dofmap, c.pts, c.wts, True, False)
        d = [0, 1, 2]   # (entry by entry: the same cells, points and weights)
        assert np.all(far.G_bound[..., d, d] >= 2.0 ** 10 * near.G_bound[..., d, d]), p


def _differs(a, b, scale):
    return np.abs(a - b).max() > 1e3 * h.TOL_ORACLE * scale


def test_operator_references_discriminate():
    """y with and without the clamp, with and without |det J|, and with the coefficient before or after the clamp differ
    by more than 1e3 TOL_ORACLE max|y|: a kernel that took the wrong one of a pair fails the GPU test"""
    for name in h.BOX_OPERATOR_MESHES:
        fabs = h.operator_fabs(name)
        for p in h.DEGREES:
            on, off = h.operator_reference(name, p, fabs, True), h.operator_reference(name, p, fabs, False)
            assert _differs(on.Ax, off.Ax, on.scale), (name, p)
            if name == "unit_negative":
                pos = h.operator_reference(name, p, True, True)
                assert _differs(on.Ax, pos.Ax, on.scale), (name, p)
    for name, p in h.COEFF_CASES:
        after = h.operator_reference(name, p, True, True, coeff="after")
        before = h.operator_reference(name, p, True, True, coeff="before")
        plain = h.operator_reference(name, p, True, True)
        assert _differs(after.Ax, before.Ax, after.scale) and _differs(after.Ax, plain.Ax, after.scale), (name, p)
    for name in h.DOFMAP_MESHES:
        for p in h.DOFMAP_DEGREES:
            refs = {(f, c): h.operator_reference(name, p, f, c, h.DOFMAP_N[p], False, s) for f, c, s in h.dofmap_variants(name)}
            if name != "half_mirrored":
                assert _differs(refs[True, True].Ax, refs[True, False].Ax, refs[True, True].scale), (name, p)
            else:   # the signs: |det J| against det J on the reoriented mesh
                signed = refs[False, True]
                fabs = h.operator_reference(name, p, True, True, h.DOFMAP_N[p], False, h.REORIENT_SEED)
                assert _differs(signed.Ax, fabs.Ax, signed.scale), (name, p)


# ---------------------------------------------------------------------------------------------------------------------
# the host rule against the reference
# ---------------------------------------------------------------------------------------------------------------------
def cell_reasons(mesh, p):
    """the rule's verdict on every cell of a mesh of disjoint cells, each asked on its own: reason[c], Gc[c][6]"""
    import wave_fenics_amd as w
    reasons, Gcs = [], []
    for c in range(mesh.ncells):
        one = SimpleNamespace(x=mesh.x[8 * c:8 * c + 8], geom_dofmap=np.arange(8, dtype=np.int32).reshape(1, 8))
        Gc, bad, reason = w.hex_cell_geometry(one, p, use_fabs=True, clamp=True)
        assert (bad < 0) == (reason == 0)
        reasons.append(reason)
        Gcs.append(Gc[0])
    return np.array(reasons), np.array(Gcs)


@pytest.mark.parametrize("p", h.DEGREES)
def test_host_rule_against_the_reference(p):
    """Every point of the rule up to P4; one point per distinct w_i w_j w_k from P5 on (on an affine cell G(q) = G_c w_q,
    and up to P4 the test shows that those points give the same mask)."""
    COMP = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    full = p <= 4
    W = h.point_weights(p).astype(h.LD)
    if not full:
        W = W[h.representative_points(p)]
    seen = set()
    for shape in h.SWEEP_SHAPES:
        mesh, r = h.sweep_mesh(shape), h.sweep_reference(shape, p, True, full)
        reason, Gc = cell_reasons(mesh, p)
        assert set(reason) <= {0, 3}, (shape, set(reason))   # every scaled cell is affine and regular
        acted = r.G_mask.any(axis=(1, 2, 3))
        short = h.sweep_acts(shape, p)   # the GPU test's short cut: the representative points say the same
        assert np.array_equal(acted, short.acts), (shape, p)
        assert np.array_equal(r.G_near, np.broadcast_to(short.near[:, None], r.G_near.shape)), (shape, p)
        assert np.all(reason[acted] == 3), (shape, p, h.SWEEP_FACTORS[acted & (reason != 3)])
        clear = ~acted & (r.margin_value_cell > 1e-5)
        assert np.all(reason[clear] == 0), (shape, p, h.SWEEP_FACTORS[clear & (reason != 0)])
        seen |= set(reason)
        ok = reason == 0
        for m, (a, b) in enumerate(COMP):
            got = Gc[ok, m].astype(h.LD)[:, None] * W[None, :]
            assert np.all(np.abs(got - r.G[ok, :, a, b]) <= r.G_bound[ok, :, a, b]), (shape, p, a, b)
        print(f"P{p} {shape}: reason 0 on {int(ok.sum())} cells, 3 on {int((~ok).sum())}, clamp acts on {int(acted.sum())}, "
              f"undecided {int((~acted & ~clear).sum())}")
    assert seen == {0, 3}
