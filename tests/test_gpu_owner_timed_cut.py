"""Owner form of the P4 box stiffness operator: the cut of the whole apply that creation chooses by timing
(tune_owner_runs, csrc/op_create_box.hip; DESIGN §4.2, "r19").

Where the uniform plan needs more than one round of the resident workgroups, creation times it against the tables
aligned_runs(ncols, nz, nseg) of owner_cut_candidates(nz) and installs the winner.  Which table an operator gets is a
timing result, so every candidate has to be right.  tests/test_gpu_owner_run_table.py reaches run tables through
replan_runs(resident), which builds box_run_plan tables, another family, on boxes of one round.

Here: every candidate table of 27-layer boxes installed with set_runs (the boxes are small and have no table of their
own), and the timed path itself on boxes of 2051 columns, more than any occupancy leaves resident.  At P4 a plane gets
the same bits whichever run it falls into, so every y must equal the uniform apply's bit for bit."""
import math
import time

import numpy as np
import pytest

from owner_helpers import aligned_runs, apply, box, graded, owner, owner_cut_candidates
from support import gpu, owner_columns, relerr  # noqa: F401

TOL_ORACLE = 1e-12   # of max|y_ref|, as tests/test_gpu_owner_run_table.py
P = 4
SECTIONS = {0: (4, 4), 1: (8, 2), 2: (2, 8)}   # owner cross-sections by tuning["variant"]
# 33 columns of 27 layers each, with a partial column in x and in y
BOXES = {0: (9, 41, 27), 1: (17, 21, 27), 2: (21, 17, 27)}
NZ = 27
# 2051 columns of 13 layers: more work items than 8 workgroups of 256 threads on every CU hold
LONG_BOXES = {"8x2": ((1, 4100, 13), {}), "2x8": ((4100, 1, 13), {"variant": 2})}
LONG_COLS, LONG_NZ = 2051, 13


def is_cover(table, ncols, nz):
    cover = np.zeros((ncols, nz), dtype=np.int64)
    for c, a, b in table:
        assert 0 <= c < ncols and 0 <= a < b <= nz
        cover[c, a:b] += 1
    return bool((cover == 1).all())


def test_candidate_tables_of_27_layers():
    """nz = 27: candidates 3 to 6.  Their tables are exact covers of 33 columns, and between them hold runs of even and of
    odd length that start at even and at odd layers, all four combinations (the direct-to-LDS form picks its buffer by
    the parity of the layer within the run)."""
    assert owner_cut_candidates(NZ) == [3, 4, 5, 6]
    assert [owner_cut_candidates(nz) for nz in (7, 8, 13)] == [[], [2], [2, 3]]
    assert owner_cut_candidates(54) == list(range(5, 14)) and owner_cut_candidates(200) == list(range(17, 51, 3))
    seen = set()
    for nseg in owner_cut_candidates(NZ):
        table = aligned_runs(33, NZ, nseg)
        assert table.shape == (33 * nseg, 3) and is_cover(table, 33, NZ)
        length = table[:, 2] - table[:, 1]
        assert length.max() == math.ceil(NZ / nseg) and 4 <= length.min() and length.max() - length.min() <= 1
        kinds = {(int(z0) & 1, int(n) & 1) for z0, n in zip(table[:, 1], length)}
        print(f"nseg {nseg}: cuts {sorted(set(table[:, 1].tolist()))}, (start, length) parities {sorted(kinds)}")
        seen |= kinds
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # entry e belongs to XCD e mod 8: each XCD's entries are a contiguous share of the segment-major sequence
    table = aligned_runs(33, NZ, 4)
    position = {0: 0, 6: 1, 13: 2, 20: 3}
    order = [position[int(z0)] * 33 + int(c) for k in range(8) for c, z0, _ in table[k::8]]
    assert order == list(range(132))


@pytest.mark.parametrize("variant", sorted(BOXES))
def test_column_counts(variant):
    assert owner_columns(BOXES[variant], P, *SECTIONS[variant]) == 33
    n, tuning = LONG_BOXES["8x2" if variant == 1 else "2x8"]
    assert owner_columns(n, P, *SECTIONS[tuning.get("variant", 1)]) == LONG_COLS


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(BOXES))
def test_every_candidate_table(gpu, oracle, variant):
    """Each candidate of nz = 27 through set_runs: the getter, plan_lz, device_bytes, and y bit for bit the uniform apply's
    and that of 3 layers per segment, within the bound of the oracle."""
    n = BOXES[variant]
    ncols = owner_columns(n, P, *SECTIONS[variant])
    assert ncols == 33
    V, x, y0, yref, _ = box(oracle, n, P, sum(n) + P)
    op = owner(V, P, variant=variant)
    before, lz = op.info.device_bytes, op.info.plan_lz
    assert len(op.runs()) == 0, "one round at creation: no table"
    y_uniform = apply(op, x, y0, gpu)
    y_lz3 = apply(owner(V, P, variant=variant, lz=3), x, y0, gpu)
    e0 = relerr(y_uniform, yref)
    print(f"{SECTIONS[variant]} {n}: uniform lz {lz}, oracle {e0:.3e}")
    assert e0 <= TOL_ORACLE
    for nseg in owner_cut_candidates(NZ):
        table = aligned_runs(ncols, NZ, nseg)
        op.set_runs(table)
        assert np.array_equal(op.runs(), table), nseg
        assert op.info.plan_lz == math.ceil(NZ / nseg), nseg
        assert op.info.device_bytes == before + 4 * table.size, nseg
        y = apply(op, x, y0, gpu)
        eo = relerr(y, yref)
        print(f"  nseg {nseg}: {len(table)} runs, oracle {eo:.3e}, entries off the uniform apply {int((y != y_uniform).sum())}, "
              f"off lz = 3 {int((y != y_lz3).sum())}")
        assert np.array_equal(y, y_uniform), nseg
        assert np.array_equal(y, y_lz3), nseg
        assert eo <= TOL_ORACLE, nseg
    # a mesh of one round: the tuner returns to no table
    op.replan_runs(0)
    assert len(op.runs()) == 0 and op.info.device_bytes == before and op.info.plan_lz == lz
    assert np.array_equal(apply(op, x, y0, gpu), y_uniform)


@pytest.mark.gpu
def test_parts_under_every_candidate_table(gpu, oracle):
    """With ghost planes below in x, y and z the interior and interface parts keep their item lists under every candidate;
    interior then interface equals the whole apply by the table bit for bit."""
    import torch
    from wave_fenics_amd._lib import WF_PART_INTERFACE, WF_PART_INTERIOR
    variant = 1
    n = BOXES[variant]
    V, x_np, y0_np, _, _ = box(oracle, n, P, sum(n) + P)
    op = owner(V, P, variant=variant)
    y_uniform = apply(op, x_np, y0_np, gpu)
    assert op.set_ghost_faces(True, True, True)
    items = (op.info.items_interior, op.info.items_interface)
    assert items[0] > 0 and items[1] > 0
    x, y0 = torch.from_numpy(x_np.copy()).to(gpu), torch.from_numpy(y0_np.copy()).to(gpu)
    for nseg in owner_cut_candidates(NZ):
        op.set_runs(aligned_runs(33, NZ, nseg))
        assert len(op.runs()) == 33 * nseg and (op.info.items_interior, op.info.items_interface) == items
        yall = y0.clone()
        op(x, yall)
        y = y0.clone()
        op.apply_part(x, y, WF_PART_INTERIOR)
        op.apply_part(x, y, WF_PART_INTERFACE)
        torch.cuda.synchronize()
        assert torch.equal(y, yall), (nseg, int((y != yall).sum()))
        assert np.array_equal(yall.cpu().numpy(), y_uniform), nseg


def long_box(oracle, n):
    """(V, x, y0 non-zero everywhere at the scale of K x, the oracle's y0 + K x) of a graded box of 2051 columns; not kept"""
    om, V = graded(oracle, n, P)
    rng = np.random.default_rng(sum(n) + P)
    x = rng.uniform(-1, 1, om.ndofs)
    yref = np.zeros(om.ndofs)
    oracle.StiffnessOperator(om, P)(x, yref)
    y0 = rng.uniform(-1, 1, om.ndofs) * np.abs(yref).max()
    assert np.abs(y0).min() > 0.0
    yref += y0
    return V, x, y0, yref


def tuned_state(op, bytes_uniform, what):
    """The state creation may leave: no table, or exactly one of the candidate tables.  Which is a timing result."""
    runs = op.runs()
    if len(runs) == 0:
        print(f"{what}: the uniform plan, lz {op.info.plan_lz}")
    else:
        assert len(runs) % LONG_COLS == 0
        nseg = len(runs) // LONG_COLS
        assert nseg in owner_cut_candidates(LONG_NZ) and np.array_equal(runs, aligned_runs(LONG_COLS, LONG_NZ, nseg))
        assert op.info.plan_lz == math.ceil(LONG_NZ / nseg)
        print(f"{what}: aligned_runs of nseg {nseg}, {len(runs)} runs")
    assert op.info.device_bytes == bytes_uniform + 4 * runs.size


@pytest.mark.gpu
@pytest.mark.parametrize("section", sorted(LONG_BOXES))
def test_the_timed_path(gpu, oracle, section):
    """2051 columns: creation times the candidates 2 and 3 of nz = 13 whatever the occupancy query says.  What it installs
    is valid, counted in device_bytes and gives the bits of the operators the tuner leaves alone (wf_tuning.lz).  Both
    candidate tables are then installed by hand as well, so that the one the timing passed over is applied too.
    (On an MI355X the timing kept the uniform plan of whole columns on both boxes, at creation and again; the oracle
    stands at 1.8e-13 and 3.9e-13 of max|y_ref| here, above the 1e-15 of the short boxes: the axis of 4100 graded cells
    reaches coordinates of 5000.)"""
    import torch
    import wave_fenics_amd as w
    n, tuning = LONG_BOXES[section]
    assert owner_cut_candidates(LONG_NZ) == [2, 3]
    assert owner_columns(n, P, *SECTIONS[tuning.get("variant", 1)]) == LONG_COLS
    # a CU holds 32 waves of 64, a workgroup is 256 threads: at most 8 resident per CU
    assert LONG_COLS > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    t0 = time.perf_counter()
    V, x, y0, yref = long_box(oracle, n)
    t1 = time.perf_counter()
    op = w.StiffnessOperator(V, P, {"c0": 1500.0}, structured=True, tuning=tuning or None)
    torch.cuda.synchronize()
    print(f"{section} {n}: oracle {t1 - t0:.2f} s, creation with the timing {time.perf_counter() - t1:.2f} s")
    assert (op.kernel, op.metric, op.update) == ("march_box", "axes", "owner")
    y_fixed = {}
    for lz in (13, 4):
        fixed = owner(V, P, lz=lz, **tuning)
        assert len(fixed.runs()) == 0 and fixed.info.plan_lz == lz, "wf_tuning.lz: the tuner is off"
        bytes_uniform = fixed.info.device_bytes
        y_fixed[lz] = apply(fixed, x, y0, gpu)
        del fixed
    tuned_state(op, bytes_uniform, "creation")
    y = apply(op, x, y0, gpu)
    eo = relerr(y, yref)
    print(f"  oracle {eo:.3e}, entries off lz = 13 {int((y != y_fixed[13]).sum())}, off lz = 4 {int((y != y_fixed[4]).sum())}")
    assert np.array_equal(y, y_fixed[13]) and np.array_equal(y, y_fixed[4])
    assert eo <= TOL_ORACLE
    # every candidate the timing may have passed over
    for nseg in owner_cut_candidates(LONG_NZ):
        op.set_runs(aligned_runs(LONG_COLS, LONG_NZ, nseg))
        assert np.array_equal(apply(op, x, y0, gpu), y), nseg
    op.replan_runs(0)   # the tuner again
    tuned_state(op, bytes_uniform, "replan_runs(0)")
    assert np.array_equal(apply(op, x, y0, gpu), y)
    op.set_runs(np.zeros((0, 3), dtype=np.int32))
    assert len(op.runs()) == 0 and op.info.device_bytes == bytes_uniform
    assert np.array_equal(apply(op, x, y0, gpu), y)
