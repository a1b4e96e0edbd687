"""Host planner of the owner form's run table (wf_box_run_plan; DESIGN §4.2, "r19").

The planner gives every workgroup one run (column, z0, z1).  Entry e of the table is workgroup e, which runs on XCD
e mod 8; an XCD's slots take its entries in order as they free up, and a run of L layers costs L + prologue.  The checks
recompute the makespan with a scheduler of their own, so a table is judged by the model and not by what the planner
reports about it."""
import heapq

import numpy as np
import pytest

NXCD = 8
PROLOGUE = 1.5
RESIDENT = 768   # three 256-thread workgroups on each of 256 CUs


@pytest.fixture(scope="module")
def plan():
    from wave_fenics_amd import build
    build.build()
    import wave_fenics_amd as w
    return w.box_run_plan


def owner_columns(cells, p=4, bx=8, by=2):
    """Columns of the owner form on a cube of `cells` per edge: lattice lines in pieces of p bx x p by."""
    lines = p * cells + 1
    return -(-lines // (p * bx)) * -(-lines // (p * by))


def makespan(runs, resident, prologue=PROLOGUE):
    worst = 0.0
    for k in range(NXCD):
        slots = [0.0] * (resident // NXCD + (1 if k < resident % NXCD else 0))
        heapq.heapify(slots)
        for col, z0, z1 in runs[k::NXCD]:
            t = heapq.heappop(slots) + (z1 - z0) + prologue
            heapq.heappush(slots, t)
            worst = max(worst, t)
    return worst


def uniform_cost(ncols, nz, resident, prologue=PROLOGUE):
    """rounds * (lz + prologue), minimised over equal cuts of at least 3 layers: what the library did before."""
    best = None
    for nseg in range(1, nz + 1):
        lz = -(-nz // nseg)
        if lz < 3 and nseg > 1:
            break
        cost = -(-ncols * -(-nz // lz) // resident) * (lz + prologue)
        if best is None or cost < best - 1e-9:
            best = cost
    return best


def check_table(runs, ncols, nz, resident):
    assert runs.ndim == 2 and runs.shape[1] == 3 and len(runs) > 0
    col, z0, z1 = runs.T
    assert (col >= 0).all() and (col < ncols).all()
    assert (0 <= z0).all() and (z0 < z1).all() and (z1 <= nz).all()   # a run stays inside one column
    cover = np.zeros((ncols, nz), dtype=np.int64)
    for c, a, b in runs:
        cover[c, a:b] += 1
    assert (cover == 1).all(), "every (column, layer) exactly once"
    counts = [len(runs[k::NXCD]) for k in range(NXCD)]
    assert max(counts) - min(counts) <= -(-resident // NXCD), counts
    # every XCD keeps a contiguous range of columns, in the order of the column sequence
    for k in range(NXCD - 1):
        assert runs[k::NXCD, 0].max() <= runs[k + 1::NXCD, 0].min(), k


CUBES = {54: 196, 64: 297, 80: 451, 100: 663}


def test_column_counts():
    assert {n: owner_columns(n) for n in CUBES} == CUBES


@pytest.mark.parametrize("cells", sorted(CUBES))
def test_benchmark_shapes(plan, cells):
    ncols, nz = CUBES[cells], cells
    runs, cost, ucost, ulz = plan(ncols, nz, RESIDENT, NXCD, PROLOGUE)
    assert ucost == uniform_cost(ncols, nz, RESIDENT)
    check_table(runs, ncols, nz, RESIDENT)
    m = makespan(runs, RESIDENT)
    print(f"{ncols} x {nz}: uniform {ucost} (lz {ulz}) -> {m} in {len(runs)} runs, longest {int((runs[:, 2] - runs[:, 1]).max())}")
    assert m == cost
    assert m < ucost
    if cells == 54:
        assert ucost == 19.0 and m <= 17.0


@pytest.mark.parametrize("seed", range(40))
def test_small_random_shapes(plan, seed):
    rng = np.random.default_rng(seed)
    ncols, nz, resident = int(rng.integers(1, 90)), int(rng.integers(1, 24)), int(rng.integers(8, 65))
    runs, cost, ucost, ulz = plan(ncols, nz, resident, NXCD, PROLOGUE)
    assert ucost == uniform_cost(ncols, nz, resident)
    if len(runs) == 0:
        assert cost == ucost
        return
    check_table(runs, ncols, nz, resident)
    m = makespan(runs, resident)
    assert m == cost and m < ucost, (ncols, nz, resident)


def test_random_shapes_reach_both_outcomes(plan):
    """The seeds above are no use if they all end the same way."""
    outcomes = set()
    for seed in range(40):
        rng = np.random.default_rng(seed)
        ncols, nz, resident = int(rng.integers(1, 90)), int(rng.integers(1, 24)), int(rng.integers(8, 65))
        outcomes.add(len(plan(ncols, nz, resident, NXCD, PROLOGUE)[0]) > 0)
    assert outcomes == {False, True}


@pytest.mark.parametrize("cells", [24, 36, 48, 72])
def test_one_round_keeps_the_uniform_plan(plan, cells):
    ncols = owner_columns(cells)
    runs, cost, ucost, ulz = plan(ncols, cells, RESIDENT, NXCD, PROLOGUE)
    assert ncols * -(-cells // ulz) <= RESIDENT, "the uniform plan of this mesh needs one round"
    assert len(runs) == 0 and cost == ucost == ulz + PROLOGUE


@pytest.mark.parametrize("lz", [1, 3, 8, 200])
def test_tuned_lz_keeps_the_uniform_plan(plan, lz):
    for cells, ncols in CUBES.items():
        runs, cost, ucost, ulz = plan(ncols, cells, RESIDENT, NXCD, PROLOGUE, lz=lz)
        assert len(runs) == 0 and ulz == lz and cost == ucost
