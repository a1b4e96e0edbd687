"""Owner form of the box stiffness operator: the whole apply by a run table ("r19").

A table gives every workgroup one run (column, z0, z1) planned on the host.  The boxes here are small, so at creation
their uniform plan needs one round and they have no table; wf_op_replan_runs plans them again for a handful of
workgroups, which takes many rounds and builds one.  The boxes have, in x and in y, a partial column (one cell more than
a multiple of the cross-section) or a column of the closing lattice line alone (an exact multiple), and 7 or 6 layers,
which the shares of no plan divide: the tables hold runs that start at layer 1 and single layers that end at the top.

At P4 a plane gets the same bits whichever run it falls into, so y must equal, bit for bit, the same operator's y before
the re-plan, that of an operator of 3 layers per segment, and the sum of the interior and interface parts."""
import numpy as np
import pytest

from owner_helpers import apply, box, graded, owner
from support import gpu, owner_columns, relerr  # noqa: F401

pytestmark = pytest.mark.gpu

TOL_ORACLE = 1e-12   # of max|y_ref|, as tests/test_gpu_owner_lane_exchange.py and tests/test_gpu_owner_update.py
TOL_FORM = 1e-13     # tests/test_gpu_owner_update.py: parts against the whole apply
RESIDENT = (8, 16, 24, 56)
VARIANTS = {0: "4x4", 1: "8x2", 2: "2x8"}
# P4, per cross-section: (partial columns, 33 columns of 7 layers), (closing-line columns, 57 columns of 6 layers)
BOXES_P4 = {0: [(9, 41, 7), (8, 72, 6)], 1: [(17, 21, 7), (16, 36, 6)], 2: [(21, 17, 7), (36, 16, 6)]}
# default owner cross-sections: P2 8x8, P6 2x3; partial columns in x and y, 33 columns of 7 layers
BOXES_P = {2: (17, 81, 7), 6: (5, 31, 7)}


def check_table(op, ncols, nz, bytes_without):
    """The table of a re-planned operator against the getter: present, an exact cover, counted in device_bytes, with a run
    that starts at layer 1 and a single layer that ends at the top."""
    runs = op.runs()
    assert len(runs) > 0, "no run table"
    col, z0, z1 = runs.T
    assert (col >= 0).all() and (col < ncols).all() and (z0 >= 0).all() and (z0 < z1).all() and (z1 <= nz).all()
    cover = np.zeros((ncols, nz), dtype=np.int64)
    for c, a, b in runs:
        cover[c, a:b] += 1
    assert (cover == 1).all()
    assert (z0 == 1).any(), "no run starts at layer 1"
    assert ((z1 == nz) & (z1 - z0 == 1)).any(), "no single layer ends at nz"
    assert op.info.device_bytes == bytes_without + runs.size * 4
    assert op.info.plan_lz == int((z1 - z0).max())
    return runs


@pytest.mark.parametrize("variant,n", [(v, n) for v in sorted(BOXES_P4) for n in BOXES_P4[v]])
def test_p4_bitwise(gpu, oracle, variant, n):
    import wave_fenics_amd as w
    p = 4
    V, x, y0, yref, _ = box(oracle, n, p, sum(n) + p)
    bx, by = {0: (4, 4), 1: (8, 2), 2: (2, 8)}[variant]
    ncols = owner_columns(n, p, bx, by)
    assert ncols == (33 if n[2] == 7 else 57)
    op = owner(V, p, variant=variant)
    before = op.info.device_bytes
    lz = op.info.plan_lz
    assert len(op.runs()) == 0 and lz < n[2], "one round of cut columns at creation: no table"
    y_uniform = apply(op, x, y0, gpu)
    y_lz3 = apply(owner(V, p, variant=variant, lz=3), x, y0, gpu)
    e0 = relerr(y_uniform, yref)
    print(f"{VARIANTS[variant]} {n}: uniform lz {lz}, oracle {e0:.3e}")
    assert e0 <= TOL_ORACLE
    for resident in RESIDENT:
        op.replan_runs(resident)
        runs = check_table(op, ncols, n[2], before)
        y = apply(op, x, y0, gpu)
        eo = relerr(y, yref)
        print(f"  resident {resident}: {len(runs)} runs, longest {op.info.plan_lz}, oracle {eo:.3e}, "
              f"entries off the uniform apply {int((y != y_uniform).sum())}, off lz = 3 {int((y != y_lz3).sum())}")
        assert np.array_equal(y, y_uniform), resident
        assert np.array_equal(y, y_lz3), resident
        assert eo <= TOL_ORACLE, resident
    with pytest.raises(w.WavehipError):
        op.replan_runs(-1)
    op.replan_runs(0)
    assert len(op.runs()) == 0 and op.info.device_bytes == before and op.info.plan_lz == lz
    assert np.array_equal(apply(op, x, y0, gpu), y_uniform)


@pytest.mark.parametrize("variant", sorted(BOXES_P4))
def test_p4_parts_equal_the_replanned_apply(gpu, oracle, variant):
    """interior + interface keep their item lists and z segments (first segment short under the z ghost plane); their sum
    equals the whole apply by the table bit for bit."""
    import torch
    from wave_fenics_amd._lib import WF_PART_INTERFACE, WF_PART_INTERIOR
    p, n = 4, BOXES_P4[variant][0]
    V, x_np, y0_np, _, _ = box(oracle, n, p, sum(n) + p)
    op = owner(V, p, variant=variant)
    assert op.set_ghost_faces(True, True, True)
    info = op.info
    assert info.items_interface > 0 and info.items_interior > 0
    items = (info.items_interior, info.items_interface)
    x, y0 = torch.from_numpy(x_np.copy()).to(gpu), torch.from_numpy(y0_np.copy()).to(gpu)
    for resident in RESIDENT:
        op.replan_runs(resident)
        assert len(op.runs()) > 0 and (op.info.items_interior, op.info.items_interface) == items
        yall = y0.clone()
        op(x, yall)
        y = y0.clone()
        op.apply_part(x, y, WF_PART_INTERIOR)
        op.apply_part(x, y, WF_PART_INTERFACE)
        torch.cuda.synchronize()
        assert torch.equal(y, yall), (VARIANTS[variant], resident, int((y != yall).sum()))


@pytest.mark.parametrize("p", sorted(BOXES_P))
def test_other_degrees(gpu, oracle, p):
    """P2 and P6 owner operators (the body there does not promise equal bits for a plane at the start and in the middle of
    a run): the re-planned apply against the uniform one and against the oracle."""
    n = BOXES_P[p]
    V, x, y0, yref, _ = box(oracle, n, p, sum(n) + p)
    bx, by = {2: (8, 8), 6: (2, 3)}[p]
    ncols = owner_columns(n, p, bx, by)
    assert ncols == 33
    op = owner(V, p)
    before = op.info.device_bytes
    assert len(op.runs()) == 0
    y_uniform = apply(op, x, y0, gpu)
    assert relerr(y_uniform, yref) <= TOL_ORACLE
    for resident in RESIDENT:
        op.replan_runs(resident)
        check_table(op, ncols, n[2], before)
        y = apply(op, x, y0, gpu)
        ef, eo = relerr(y, y_uniform), relerr(y, yref)
        print(f"P{p} {n} resident {resident}: {len(op.runs())} runs, uniform apply {ef:.3e}, oracle {eo:.3e}")
        assert ef <= TOL_FORM, resident
        assert eo <= TOL_ORACLE, resident
    op.replan_runs(0)
    assert len(op.runs()) == 0 and op.info.device_bytes == before


def test_only_the_owner_form_replans(gpu, oracle):
    import wave_fenics_amd as w
    _, V = graded(oracle, (3, 3, 3), 2)
    op = w.StiffnessOperator(V, 2, {"c0": 1500.0}, structured=True, tuning={"update": "atomic"})
    assert op.update == "atomic" and len(op.runs()) == 0
    with pytest.raises(w.WavehipError):
        op.replan_runs(8)


def test_a_callers_table(gpu, oracle):
    """wf_op_set_runs: a table of the caller's (every column cut at the same places, runs of 1 to 3 layers, in an order
    of its own) gives the same bits; tables that leave a layer out, cover one twice or leave the mesh are refused and
    the operator keeps what it had."""
    import wave_fenics_amd as w
    p, variant, n = 4, 1, BOXES_P4[1][0]
    V, x, y0, _, _ = box(oracle, n, p, sum(n) + p)
    ncols = owner_columns(n, p, 8, 2)
    op = owner(V, p, variant=variant)
    before = op.info.device_bytes
    y_uniform = apply(op, x, y0, gpu)
    cuts = [0, 1, 4, 6, 7]
    table = np.array([(c, a, b) for a, b in zip(cuts[:-1], cuts[1:]) for c in reversed(range(ncols))], dtype=np.int32)
    op.set_runs(table)
    assert np.array_equal(op.runs(), table) and op.info.plan_lz == 3
    assert op.info.device_bytes == before + table.size * 4
    assert np.array_equal(apply(op, x, y0, gpu), y_uniform)
    for bad in (table[:-1], np.concatenate([table, table[:1]]), np.concatenate([table[:-1], [(ncols, 6, 7)]]),
                np.concatenate([table[:-1], [(0, 6, 8)]])):
        with pytest.raises(w.WavehipError):
            op.set_runs(bad)
        assert np.array_equal(op.runs(), table)
    op.set_runs(np.zeros((0, 3), dtype=np.int32))
    assert len(op.runs()) == 0 and op.info.device_bytes == before
    assert np.array_equal(apply(op, x, y0, gpu), y_uniform)
