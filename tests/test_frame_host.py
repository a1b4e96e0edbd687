"""Conditions of tests/test_gpu_caller_frame.py, on the CPU (tests/frame_helpers.py): the helper is a bijection, it
agrees with the one host-only entry of the C ABI that speaks of the frame (wf_reorder_dofmap), and the inputs of the
GPU file can tell a frame error from none -- the caller's arrays differ from the canonical ones, the meshes are
anisotropic, and the CPU oracle fed the arrays a frame error would compute with moves the result by more than 1e-3.
A case that cannot tell fails here; nothing is skipped.  No GPU."""
import ctypes

import numpy as np
import pytest

import frame_helpers as fh
from support import wpackage as w  # noqa: F401

STIFFNESS_CASES = [(m, p) for m in ("box", "random_orient", "stair") for p in range(1, 8)] \
    + [(m, p) for m in ("sheared", "sheared_random") for p in range(1, 5)]
MASS_CASES = [(m, p) for m in ("box", "random_orient") for p in (2, 3, 4, 6)]
MOVES = 1e-3


def moved(y, yref):
    return fh.relerr(y, yref)


# --------------------------------------------------------------------------- the helper itself
@pytest.mark.parametrize("m", range(2, 10))
@pytest.mark.parametrize("xslow", [False, True])
def test_caller_inputs_round_trip(m, xslow):
    rng = np.random.default_rng(m)
    nd = m ** 3
    canon = {"dofmap": rng.integers(0, 10 * nd, (5, nd)).astype(np.int32), "G": rng.uniform(-1, 1, (5, nd, 3, 3)),
             "detJ": rng.uniform(0.5, 1, (5, nd))}
    t = fh.caller_index(m, xslow)
    assert sorted(t.tolist()) == list(range(nd))
    assert (not xslow and np.array_equal(t, np.arange(nd))) or (xslow and t[1] == m * m and t[m * m] == 1)
    for perm in (None, fh.draw_perm(nd)):
        caller = fh.caller_inputs(canon, perm, xslow)
        back = fh.engine_view(caller, perm, xslow)
        for key in canon:
            assert back[key].dtype == canon[key].dtype and np.array_equal(back[key].view(np.uint8), canon[key].view(np.uint8)), key
        # the 3 x 3 of G travels with its point, untouched
        assert np.array_equal(caller["G"][:, t[7]], canon["G"][:, 7])
        if perm is not None:   # the convention of wavehip.h: dm_elem[c][perm[l']] = dm_tensor'[c][l']
            assert np.array_equal(caller["dofmap"][:, perm], fh.caller_inputs({"dofmap": canon["dofmap"]}, None, xslow)["dofmap"])


def test_perm_is_no_involution():
    for p in range(1, 8):
        nd = (p + 1) ** 3
        pm = fh.draw_perm(nd)
        assert sorted(pm.tolist()) == list(range(nd))
        assert not np.array_equal(pm[pm], np.arange(nd)) and (pm != np.arange(nd)).sum() * 2 > nd
        assert not np.array_equal(fh.inverse(pm), pm) and np.array_equal(fh.inverse(pm)[pm], np.arange(nd))


@pytest.mark.parametrize("p", range(1, 8))
@pytest.mark.parametrize("name", fh.FRAMES)
def test_reorder_dofmap_gives_the_tensor_dofmap(w, name, p):
    """wf_reorder_dofmap with the folded permutation takes the caller's dofmap back to the canonical one, in every
    frame; with the caller's own perm it gives the caller's tensor dofmap."""
    from wave_fenics_amd import _lib
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    fr = fh.frame(name, p)
    canon = fh.mesh_case("box", p).om.dofmap
    dm = fh.caller_dofmap(canon, fr.perm, fr.xslow)
    eff = fh.effective_perm(fr.perm, fr.xslow, p + 1)
    if name == "id":
        assert eff is None and np.array_equal(dm, canon)
        return
    out = np.zeros_like(dm)
    _lib.check(_lib.lib().wf_reorder_dofmap(dm.shape[0], dm.shape[1], ip(eff), ip(dm), ip(out)))
    assert np.array_equal(out, canon)
    if fr.perm is not None:
        _lib.check(_lib.lib().wf_reorder_dofmap(dm.shape[0], dm.shape[1], ip(fr.perm), ip(dm), ip(out)))
        assert np.array_equal(out, fh.caller_dofmap(canon, None, fr.xslow))


# --------------------------------------------------------------------------- the inputs discriminate
def anisotropy(G):
    """smallest pairwise relative difference of three positive numbers: the diagonal of the mean G"""
    d = np.asarray(G).mean(axis=(0, 1)).diagonal()
    return min(abs(d[a] - d[b]) / max(abs(d[a]), abs(d[b])) for a, b in ((0, 1), (0, 2), (1, 2)))


def sorted_anisotropy(G):
    """the same of the mean over cells of each cell's own three diagonal means, sorted: free of the labels of the cells'
    axes, which a re-oriented mesh draws at random (there the plain mean mixes the axes)"""
    d = np.sort(np.abs(np.asarray(G).mean(axis=1)[:, [0, 1, 2], [0, 1, 2]]), axis=1).mean(axis=0)
    return min(abs(d[a] - d[b]) / max(d[a], d[b]) for a, b in ((0, 1), (0, 2), (1, 2)))


@pytest.mark.parametrize("mesh,p", STIFFNESS_CASES)
def test_stiffness_inputs_discriminate(w, mesh, p):
    case, K = fh.mesh_case(mesh, p), fh.stiffness_canon(mesh, p)
    canon = {"dofmap": case.om.dofmap, "G": K.G, "detJ": K.detJ}
    assert np.array_equal(case.V.dofmap, case.om.dofmap)
    for name in fh.FRAMES[1:]:
        fr = fh.frame(name, p)
        caller = fh.caller_inputs(canon, fr.perm, fr.xslow)
        assert fh.rows_differing(caller["dofmap"], canon["dofmap"]) > 0.5, name
        if mesh.startswith("sheared"):   # per-cell geometry comes from the mesh: no G is handed over (affine: G_c w_q)
            continue
        if fr.xslow:   # perm alone does not touch the points
            assert fh.rows_differing(caller["G"], canon["G"]) > 0.5 and fh.rows_differing(caller["detJ"], canon["detJ"]) > 0.5, name
        else:
            assert np.array_equal(caller["G"], canon["G"])
    assert sorted_anisotropy(K.G) > 0.1, (mesh, p, sorted_anisotropy(K.G))
    if not case.reoriented:
        assert anisotropy(K.G) > 0.1, (mesh, p, anisotropy(K.G))
    # the switches of the restaging steps: the box keeps its cell order, the shuffled caller does not
    if mesh == "box":
        assert fh.library_keeps_cell_order(canon["dofmap"])
        cp = fh.cell_shuffle(case.om.ncells)
        assert not fh.library_keeps_cell_order(canon["dofmap"][cp]) and (cp != np.arange(len(cp))).sum() * 2 > len(cp)
        a = fh.coefficient(case.om.ncells)
        assert a.min() >= 0.5 and a.max() <= 2.0 and np.unique(a).size == a.size


@pytest.mark.parametrize("mesh", ["sheared", "sheared_random"])
def test_sheared_meshes_take_per_cell_geometry(w, mesh):
    """hex_cell_geometry accepts the sheared box and its re-oriented version at P1-P4 (host only)."""
    for p in range(1, 5):
        _, bad, reason = w.operators.hex_cell_geometry(fh.mesh_case(mesh, p).mesh, p)
        assert (bad, reason) == (-1, 0), (mesh, p, bad, reason)
    _, bad, reason = w.operators.hex_cell_geometry(fh.mesh_case("box", 2).mesh, 2)
    assert bad >= 0 and reason == 1       # the perturbed box: the refusal of the GPU file


@pytest.mark.parametrize("mesh,p", STIFFNESS_CASES)
def test_misframed_stiffness_moves(w, mesh, p):
    """K x of the oracle on the arrays a frame error would compute with, against K x on the canonical ones."""
    case, K = fh.mesh_case(mesh, p), fh.stiffness_canon(mesh, p)
    ref = fh.stiffness_reference(mesh, p)
    canon = {"dofmap": case.om.dofmap, "G": K.G}
    # the canonical arrays through the same function: it is the sum-factorised form, 1e-12 from the dense reference
    assert moved(fh.misframed_stiffness(p, canon["dofmap"], canon["G"], ref.x), ref.ax) <= 1e-12
    pm = fh.draw_perm((p + 1) ** 3)
    xs = fh.caller_inputs(canon, None, True)
    pe = fh.caller_inputs(canon, pm, False)
    both = fh.caller_inputs(canon, pm, True)
    wrong = {
        "G_xs read as x-fastest": (canon["dofmap"], xs["G"]),
        "dofmap_xs read as x-fastest": (xs["dofmap"], canon["G"]),
        "xslow inputs without the flag": (fh.engine_view(xs, None, False)["dofmap"], fh.engine_view(xs, None, False)["G"]),
        "perm inverted": (fh.engine_dofmap(pe["dofmap"], fh.inverse(pm), False), canon["G"]),
        "perm dropped": (fh.engine_dofmap(pe["dofmap"], None, False), canon["G"]),
        "xslow+perm, perm inverted": (fh.engine_dofmap(both["dofmap"], fh.inverse(pm), True), canon["G"]),
        "xslow+perm without the flag": (fh.engine_dofmap(both["dofmap"], pm, False), fh.engine_points(both["G"], False)),
    }
    if mesh.startswith("sheared"):
        # per-cell geometry: G comes from the mesh, never from the caller (on an affine cell G = G_c w_i w_j w_k is the same
        # in both point orders anyway, up to rounding); the dofmap is all a frame reaches
        assert np.abs(xs["G"] - canon["G"]).max() <= 1e-14 * np.abs(canon["G"]).max()
        del wrong["G_xs read as x-fastest"]
    for what, (dm, G) in wrong.items():
        err = moved(fh.misframed_stiffness(p, dm, G, ref.x), ref.ax)
        assert err > MOVES, (mesh, p, what, err)


@pytest.mark.parametrize("kind", ["square", "rect"])
@pytest.mark.parametrize("mesh,p", MASS_CASES)
def test_misframed_dense_mass_moves(w, mesh, p, kind):
    """The dense mass with det J w in the caller's order.  A consistent exchange of x and z in the dofs AND the points is
    a symmetry of Phi^T D Phi (one 1-D table on all three axes), so the whole set of x-slowest inputs read as x-fastest
    is the right operator: the errors that show are the halves -- det J alone, the dofmap alone (the mesh as the source
    of det J) -- and the element permutation."""
    case, t = fh.mesh_case(mesh, p), fh.mass_canon(mesh, p, kind)
    ref = fh.mass_reference(mesh, p, kind)
    canon = {"dofmap": case.om.dofmap, "detJ": t.detJ}
    assert kind != "rect" or (t.phi1.shape[0] != t.phi1.shape[1])
    assert np.abs(t.phi1[:p + 1] - t.phi1[:p + 1].T).max() > 0.01        # the 1-D table is not symmetric
    pm = fh.draw_perm((p + 1) ** 3)
    xs = fh.caller_inputs(canon, None, True)
    pe = fh.caller_inputs(canon, pm, False)
    assert fh.rows_differing(xs["detJ"], canon["detJ"]) > 0.5
    assert moved(fh.misframed_dense_mass(canon["dofmap"], t.phi, canon["detJ"], ref.x), ref.ax) <= 1e-13
    wrong = {
        "detJ_xs read as x-fastest": (canon["dofmap"], xs["detJ"]),
        "dofmap_xs read as x-fastest": (xs["dofmap"], canon["detJ"]),
        "perm inverted": (fh.engine_dofmap(pe["dofmap"], fh.inverse(pm), False), canon["detJ"]),
        "perm dropped": (fh.engine_dofmap(pe["dofmap"], None, False), canon["detJ"]),
    }
    for what, (dm, detJ) in wrong.items():
        err = moved(fh.misframed_dense_mass(dm, t.phi, detJ, ref.x), ref.ax)
        assert err > MOVES, (mesh, p, kind, what, err)
    sym = moved(fh.misframed_dense_mass(xs["dofmap"], t.phi, xs["detJ"], ref.x), ref.ax)
    assert sym <= 1e-13, (mesh, p, kind, sym)       # the symmetry named above


@pytest.mark.parametrize("mesh,p", [(m, p) for m in ("box", "random_orient") for p in (2, 4, 6)])
def test_misframed_lumped_mass_moves(w, mesh, p):
    """The lumped mass pairs dofmap[c][l] with detJ[c][l]: any consistent reordering of the two is the same operator, so a
    frame error shows only where one of them keeps its order -- the halves, and the element permutation."""
    case, M = fh.mesh_case(mesh, p), fh.lumped_canon(mesh, p)
    ref = fh.lumped_reference(mesh, p)
    canon = {"dofmap": case.om.dofmap, "detJ": M.detJ}
    pm = fh.draw_perm((p + 1) ** 3)
    xs = fh.caller_inputs(canon, None, True)
    pe = fh.caller_inputs(canon, pm, False)
    assert moved(fh.misframed_lumped_mass(canon["dofmap"], canon["detJ"], ref.x), ref.ax) <= 1e-14
    wrong = {
        "detJ_xs read as x-fastest": (canon["dofmap"], xs["detJ"]),
        "dofmap_xs read as x-fastest": (xs["dofmap"], canon["detJ"]),
        "perm inverted": (fh.engine_dofmap(pe["dofmap"], fh.inverse(pm), False), canon["detJ"]),
        "perm dropped": (fh.engine_dofmap(pe["dofmap"], None, False), canon["detJ"]),
    }
    for what, (dm, detJ) in wrong.items():
        err = moved(fh.misframed_lumped_mass(dm, detJ, ref.x), ref.ax)
        assert err > MOVES, (mesh, p, what, err)
    assert moved(fh.misframed_lumped_mass(xs["dofmap"], xs["detJ"], ref.x), ref.ax) <= 1e-14


@pytest.mark.parametrize("p", [5, 6, 7])
def test_ksplit_boxes_discriminate(w, p):
    """the (BX + 1, BY + 1, 5) boxes of the k-split cross-sections: anisotropic, and a frame error moves K x"""
    from guard_helpers import compiled_shapes
    shapes = [s for s in compiled_shapes("stiffness_march_ks.hip", "WF_KS_SHAPES") if s[0] == p]
    assert len(shapes) == 3
    for _, bx, by in shapes:
        c = fh.box_of((bx + 1, by + 1, 5), p)
        K = fh._oracle().StiffnessOperator(c.om, p)
        assert anisotropy(K.G) > 0.1, (p, bx, by, anisotropy(K.G))
        x = np.random.default_rng(p).uniform(-1, 1, c.om.ndofs)
        y = np.zeros(c.om.ndofs)
        K(x, y)
        fr = fh.frame("xslow+perm", p)
        both = fh.caller_inputs({"dofmap": c.om.dofmap, "G": K.G}, fr.perm, True)
        bad = fh.misframed_stiffness(p, fh.engine_dofmap(both["dofmap"], fr.perm, False), fh.engine_points(both["G"], False), x)
        assert moved(bad, y) > MOVES
