"""Owner-computes update of the separable box stiffness form (wf_tuning.update, wf_op_info_t.update).

The owner form gives every y entry to one thread, which gathers it from the cells around the node and reads and
writes it once: no atomics.  Every case is checked against the CPU oracle (1e-12 of max|y|) and against the atomic
form of the same operator (1e-13: only the summation order differs); the apply accumulates into a non-zero y."""
import itertools

import numpy as np
import pytest

from owner_helpers import apply, graded, inputs, reference, spaces, stiffness
from support import gpu, lattice_x, relerr  # noqa: F401

pytestmark = pytest.mark.gpu

TOL_ORACLE = 1e-12
TOL_FORM = 1e-13


# nx, ny multiples of the default cross-section (the closing lattice line is a column of its own) and not
@pytest.mark.parametrize("p,n", [(1, (16, 9, 3)), (1, (9, 7, 5)), (2, (8, 8, 3)), (2, (7, 5, 3)),
                                 (3, (5, 5, 4)), (3, (7, 3, 3)), (4, (8, 4, 3)), (4, (7, 5, 3))])
@pytest.mark.parametrize("case", ["unit", "graded"])
def test_owner_matches_atomic_and_oracle(gpu, oracle, p, n, case):
    om, V = spaces(oracle, n, p, hi=(1.0, 0.7, 1.3)) if case == "unit" else graded(oracle, n, p)
    x, y0 = inputs(om, p)
    yref = reference(oracle, om, p, x, y0)
    own, atom = stiffness(V, p, update="owner"), stiffness(V, p, update="atomic")
    assert own.kernel == atom.kernel == "march_box"
    assert (own.metric, own.update, atom.metric, atom.update) == ("axes", "owner", "axes", "atomic")
    y = apply(own, x, y0, gpu)
    assert relerr(y, yref) <= TOL_ORACLE, relerr(y, yref)
    assert relerr(y, apply(atom, x, y0, gpu)) <= TOL_FORM


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_every_owner_cross_section(gpu, oracle, p, variant):
    for n in [(9, 7, 4), (8, 8, 3)]:
        om, V = graded(oracle, n, p)
        x, y0 = inputs(om, 7)
        op = stiffness(V, p, variant=variant, update="owner")
        assert op.update == "owner"
        y = apply(op, x, y0, gpu)
        assert relerr(y, reference(oracle, om, p, x, y0)) <= TOL_ORACLE, n
        assert relerr(y, apply(stiffness(V, p, update="atomic"), x, y0, gpu)) <= TOL_FORM, n


@pytest.mark.parametrize("p", [2, 4])
def test_z_segments(gpu, oracle, p):
    n = (7, 5, 6)
    om, V = graded(oracle, n, p, seed=3)
    x, y0 = inputs(om, 9)
    yref = reference(oracle, om, p, x, y0)
    ya = apply(stiffness(V, p, update="atomic"), x, y0, gpu)
    for lz in (1, 2, 3, n[2]):
        op = stiffness(V, p, lz=lz, update="owner")
        assert op.info.plan_lz == lz and op.update == "owner"
        y = apply(op, x, y0, gpu)
        assert relerr(y, yref) <= TOL_ORACLE, lz
        assert relerr(y, ya) <= TOL_FORM, lz


@pytest.mark.parametrize("p", [2, 4])
def test_mirrored_box(gpu, oracle, p):
    """det J < 0: WF_FLAG_NO_FABS negates the operator in the owner form as in the atomic one."""
    from wave_fenics_amd._lib import WF_FLAG_NO_FABS
    n = (5, 4, 3)
    axes = [np.linspace(0.0, 1.0, m + 1) for m in n]
    axes[0] = axes[0][::-1].copy()
    om, V = spaces(oracle, n, p, x=lattice_x(*axes))
    x = np.random.default_rng(5).uniform(-1, 1, om.ndofs)
    zero = np.zeros(om.ndofs)
    ys = {}
    for flags in (0, WF_FLAG_NO_FABS):
        own, atom = stiffness(V, p, flags, update="owner"), stiffness(V, p, flags, update="atomic")
        assert own.update == "owner"
        ys[flags] = apply(own, x, zero, gpu)
        assert relerr(ys[flags], apply(atom, x, zero, gpu)) <= TOL_FORM, flags
    assert relerr(ys[0], reference(oracle, om, p, x, zero)) <= TOL_ORACLE
    assert relerr(ys[WF_FLAG_NO_FABS], -ys[0]) <= TOL_FORM


def test_selection(gpu, oracle):
    """AUTO picks the owner form for the separable kernel at P4 only; the other forms keep their atomics."""
    import wave_fenics_amd as w
    for p in (1, 2, 3, 4):
        _, V = spaces(oracle, (3, 3, 3), p)
        assert stiffness(V, p).update == ("owner" if p == 4 else "atomic")
        assert stiffness(V, p, update="atomic").update == "atomic"
        assert stiffness(V, p, update="owner").update == "owner"
        assert stiffness(V, p, metric="full").update == "none"
        with pytest.raises(w.WavehipError):
            stiffness(V, p, metric="full", update="owner")
    _, V = spaces(oracle, (3, 3, 3), 4)
    with pytest.raises(w.WavehipError):
        stiffness(V, 4, update=3)


@pytest.mark.parametrize("lz0", [1, 3])
@pytest.mark.parametrize("ghost", list(itertools.product((0, 1), repeat=3)))
def test_parts_sum_to_the_full_apply(gpu, oracle, ghost, lz0):
    """interior + interface (and interior A + interface + interior B) == the full apply; the interior part reads no
    ghost dof of x (poisoned with NaN) -- its footprint reaches P lines / planes below what it owns."""
    import torch
    from wave_fenics_amd._lib import WF_PART_INTERFACE, WF_PART_INTERIOR, WF_PART_INTERIOR_A, WF_PART_INTERIOR_B
    p, n = 4, (9, 6, 8)
    om, V = graded(oracle, n, p, seed=5)
    NX, NY, NZ = V.lattice
    lat = np.arange(om.ndofs).reshape(NZ, NY, NX)
    gpos = np.unique(np.concatenate([lat[:, :, 0].ravel() if ghost[0] else [], lat[:, 0, :].ravel() if ghost[1] else [],
                                     lat[0, :, :].ravel() if ghost[2] else []])).astype(np.int32)
    x = torch.from_numpy(np.random.default_rng(8).uniform(-1, 1, om.ndofs)).to(gpu)
    for mode in ("faces", "dofs"):
        op = stiffness(V, p, lz=3, lz0=lz0, update="owner")
        assert op.update == "owner"
        if mode == "faces":
            assert op.set_ghost_faces(*[bool(g) for g in ghost])
        else:
            assert op.set_ghost_dofs(gpos)
        if any(ghost):
            assert op.info.items_interface > 0 and op.info.items_interior > 0
        else:
            assert op.info.items_interface == 0
        yall = torch.zeros_like(x)
        op(x, yall)
        y = torch.zeros_like(x)
        xp = x.clone()
        if gpos.size:
            xp[torch.from_numpy(gpos.astype(np.int64)).to(gpu)] = float("nan")
        op.apply_part(xp, y, WF_PART_INTERIOR)
        assert bool(torch.isfinite(y).all()), (mode, "interior part read a ghost dof")
        op.apply_part(x, y, WF_PART_INTERFACE)
        torch.cuda.synchronize()
        assert relerr(y.cpu().numpy(), yall.cpu().numpy()) <= TOL_FORM, mode
        yb = torch.zeros_like(x)
        for part in (WF_PART_INTERIOR_A, WF_PART_INTERFACE, WF_PART_INTERIOR_B):
            op.apply_part(x, yb, part)
        torch.cuda.synchronize()
        assert relerr(yb.cpu().numpy(), yall.cpu().numpy()) <= TOL_FORM, mode


@pytest.mark.parametrize("structured", [True, False])
def test_resplit_gives_back_the_old_item_lists(gpu, oracle, structured):
    """wf_op_info_t.device_bytes across two interior / interface splits: the four work-item lists (interior, interface
    and the two interior halves, 4 B per item) come on top of what the operator held before the first split, and a
    second split with another ghost set replaces the lists of the first instead of adding to them.  The parts of either
    split sum to the full apply."""
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd._lib import WF_PART_INTERFACE, WF_PART_INTERIOR, WF_PART_INTERIOR_A, WF_PART_INTERIOR_B
    p, n = 2, (3, 3, 6)
    om, V = spaces(oracle, n, p)
    # (the dofmap operator marches on request: at this size its plan fills too few cell slots for the default to take it)
    tuning = {"lz": 2} if structured else {"lz": 2, "kernel": "march"}
    op = w.StiffnessOperator(V, p, {"c0": 1500.0}, structured=structured, tuning=tuning)
    assert op.kernel == ("march_box" if structured else "march_idx")
    NX, NY, NZ = V.lattice
    lat = np.arange(om.ndofs).reshape(NZ, NY, NX)
    below = lat[0, :, :].ravel().astype(np.int32)
    below_and_left = np.unique(np.concatenate([below, lat[:, :, 0].ravel()])).astype(np.int32)
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, om.ndofs)).to(gpu)
    yall = torch.zeros_like(x)
    op(x, yall)
    before = op.info.device_bytes
    assert before > 0 and op.info.items_interior == 0 and op.info.items_interface == 0
    counts = []
    for split in (0, 1):
        if split == 0:
            assert op.set_ghost_faces(False, False, True) if structured else op.set_ghost_dofs(below)
        else:
            assert op.set_ghost_dofs(below_and_left)
        info = op.info
        counts.append((info.items_interior, info.items_interface))
        assert info.items_interface > 0
        assert info.device_bytes == before + 4 * (2 * info.items_interior + info.items_interface), (split, counts)
        for parts in ((WF_PART_INTERIOR, WF_PART_INTERFACE), (WF_PART_INTERIOR_A, WF_PART_INTERFACE, WF_PART_INTERIOR_B)):
            y = torch.zeros_like(x)
            for part in parts:
                op.apply_part(x, y, part)
            torch.cuda.synchronize()
            assert relerr(y.cpu().numpy(), yall.cpu().numpy()) <= TOL_FORM, (split, parts)
    assert counts[0][0] > 0 and counts[1] != counts[0], counts   # the second ghost set moved items to the interface


@pytest.mark.parametrize("p,n", [(2, (7, 6, 9)), (4, (10, 9, 8))])
def test_owner_applies_are_bitwise_repeatable(gpu, oracle, p, n):
    import torch
    _, V = graded(oracle, n, p, seed=2)
    op = stiffness(V, p, update="owner")
    x = torch.from_numpy(np.random.default_rng(6).uniform(-1, 1, V.ndofs)).to(gpu)
    y0 = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, V.ndofs)).to(gpu)
    first = None
    for _ in range(100):
        y = y0.clone()
        op(x, y)
        if first is None:
            first = y
        else:
            assert torch.equal(y, first)
