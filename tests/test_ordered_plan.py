"""wf_ordered_slots, the plan of the order-fixed accumulation (WF_FLAG_ORDERED): a stable counting sort of the flattened
dofmap.  The slots of dof d are row_off[d] .. row_off[d+1]-1 and ascend with the position of the entry in the caller's
dofmap -- compared with numpy's stable argsort / bincount.  Host only: no GPU."""
import ctypes

import numpy as np
import pytest

from support import wpackage as w  # noqa: F401


def numpy_plan(dofmap, ndofs):
    flat = np.asarray(dofmap).reshape(-1)
    order = np.argsort(flat, kind="stable")          # order[s] = the entry that lands in slot s
    slot = np.empty(flat.size, dtype=np.int64)
    slot[order] = np.arange(flat.size)
    row_off = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=ndofs))])
    return row_off, slot.reshape(np.asarray(dofmap).shape)


def check_plan(w, dofmap, ndofs):
    row_off, slot = w.ordered_slots(dofmap, ndofs)
    ro, sl = numpy_plan(dofmap, ndofs)
    assert row_off.dtype == np.int32 and slot.dtype == np.int32
    assert row_off.shape == (ndofs + 1,) and slot.shape == np.asarray(dofmap).shape
    assert np.array_equal(row_off, ro)
    assert np.array_equal(slot, sl)
    # the contract in words: a permutation of the slots; within the run of a dof the entries ascend front to back
    flat, fs = np.asarray(dofmap).reshape(-1), slot.reshape(-1)
    assert np.array_equal(np.sort(fs), np.arange(flat.size))
    for d in range(ndofs):
        e = np.nonzero(flat == d)[0]
        assert np.array_equal(fs[e], np.arange(row_off[d], row_off[d + 1]))
    return row_off, slot


def box_space(w, p=2, n=(3, 2, 2)):
    return w.create_functionspace(w.create_box(n), p)


def test_box_dofmap(w):
    V = box_space(w)
    row_off, _ = check_plan(w, V.dofmap, V.ndofs)
    counts = np.diff(row_off)
    assert counts.min() == 1 and counts.max() == 8 and row_off[-1] == V.dofmap.size


def test_shuffled_cells_and_renumbered_dofs(w):
    V = box_space(w)
    rng = np.random.default_rng(3)
    dm = rng.permutation(V.ndofs).astype(np.int32)[V.dofmap][rng.permutation(V.mesh.ncells)]
    check_plan(w, np.ascontiguousarray(dm), V.ndofs)


def test_cell_listing_a_dof_twice(w):
    V = box_space(w)
    dm = V.dofmap.copy()
    dm[5, 7] = dm[5, 3]          # cell 5 lists one dof at positions 3 and 7
    row_off, slot = check_plan(w, dm, V.ndofs)
    assert slot[5, 7] > slot[5, 3]
    assert row_off[V.dofmap[5, 7] + 1] - row_off[V.dofmap[5, 7]] == np.count_nonzero(dm == V.dofmap[5, 7])


def test_unused_dofs_give_empty_rows(w):
    V = box_space(w)
    dm = (2 * V.dofmap + 3).astype(np.int32)     # only odd dofs >= 3 are used
    ndofs = 2 * V.ndofs + 9
    row_off, _ = check_plan(w, dm, ndofs)
    counts = np.diff(row_off)
    assert np.all(counts[0::2] == 0) and counts[1] == 0 and np.all(counts[2 * V.ndofs + 3:] == 0)
    # no cells at all: every row empty
    row_off, slot = w.ordered_slots(np.zeros((0, 27), dtype=np.int32), 5)
    assert np.array_equal(row_off, np.zeros(6, dtype=np.int32)) and slot.size == 0


def test_out_of_range_index_is_an_error(w):
    from wave_fenics_amd import _lib
    V = box_space(w)
    for bad in (V.ndofs, -1):
        dm = V.dofmap.copy()
        dm[2, 11] = bad
        with pytest.raises(w.WavehipError):
            w.ordered_slots(dm, V.ndofs)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))   # noqa: E731
    dm = V.dofmap.copy()
    dm[0, 0] = V.ndofs
    row_off, slot = np.zeros(V.ndofs + 1, dtype=np.int32), np.zeros(dm.size, dtype=np.int32)
    assert _lib.lib().wf_ordered_slots(dm.shape[0], dm.shape[1], V.ndofs, ip(dm), ip(row_off), ip(slot)) == -1
    assert b"out of range" in _lib.lib().wf_last_error()
    # ncells * nd beyond int32: refused before any array is read
    assert _lib.lib().wf_ordered_slots(1 << 26, 64, V.ndofs, ip(dm), ip(row_off), ip(slot)) == -2


def test_constants(w):
    from wave_fenics_amd import _lib, operators
    assert _lib.WF_FLAG_ORDERED == 16 and _lib.WF_KERNEL_CELLS_ORDERED == 9 and _lib.WF_UPDATE_ORDERED == 3
    assert operators.KERNEL_NAMES[9] == "cells_ordered"
