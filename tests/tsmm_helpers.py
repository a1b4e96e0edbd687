"""Cases, data and references of the wf_tsmm path tests (tests/test_tsmm_host.py, tests/test_gpu_tsmm_paths.py).  No
torch and no GPU in here.

The plan.  launches(ncells, K, N) restates csrc/tsmm_plan.h -- the column passes and row ranges of wf_tsmm and the
per-launch plan of launch_tsmm_t -- so that a GPU test can say which rows a path touches.  It is a copy, and is trusted
only as far as tests/test_tsmm_host.py compares it, field by field, with what tests/cxx/tsmm_plan_walk.cpp prints from
the header itself for every case below.

The cases.  CASES names every shape with the path it is there for: `want` lists, launch by launch, (NT, nt, nch, ACC,
tail_ct, rounds of the main loop), and cmod = ncells % 16 is the partial cell tile.  test_tsmm_host.py asserts these
against the header and asserts that the table as a whole covers the sets in REQUIRED_* below.

Exact data.  in = integers in [-15, 15] times 2^e_c per cell, phi = integers in [-15, 15] times 2^e_n per column, e in
[-20, 20].  Every product is an integer of at most 225 times 2^(e_c + e_n) and every partial sum of a fixed (cell, column)
an integer of at most 225 K < 2^53 times the same power of two: exactly representable in any order of summation, fused
or not, through stored and reloaded partial sums.  The device must return the integer product, scaled, as numbers
(np.array_equal; the sign of a zero is free), in every entry.

Rounding data.  FIELDS: U(-1, 1); decays 2^(-40 s) along the cell index with the quiet end in the first tile
("cell_up") and in the last, partial one ("cell_down"); decays along k (on `in`) and along n (on phi).  The bound is per
entry, |got - ref| <= B eps mag with mag = |in| |phi| and B = K + 2: a sum of K products in any order, with or without
fma, lies within K u (1 + O(u)) of its magnitude (u = eps / 2: every term passes through at most one rounding as a
product and K - 1 as part of a partial sum, each of at most u times a magnitude that never exceeds mag's share of it),
and stored and reloaded partial sums are exact.  K u = (K / 2) eps; with the project's factor two of headroom
B = K + 2 in the units of support.ratio (K eps for the sum, 2 eps over it).  This assumes round-to-nearest in the MFMA
pipe, as the tetrahedral tests do.  B is derived, not measured, and is not to be widened.
The reference is a long-double sum of K outer products (support.LD), on the rows of subset_rows() only -- the exact
check already covers every entry; mag is the float64 product |in| |phi|, itself within K u of its value."""
from __future__ import annotations

import functools

import numpy as np

from support import EPS, LD

GRID, WAVES, CHUNK = 256, 8, 8     # kTsmmGrid, kTsmmWaves, kTsmmChunk of csrc/tsmm_plan.h
LDS_LIMIT = 160 * 1024
FIELDS = ("uniform", "cell_up", "cell_down", "k_decay", "n_decay")
LAUNCH_KEYS = ("ncells", "Kfull", "N", "n0", "NT", "nt", "k0", "K", "nch", "acc", "nb", "ntiles", "rem", "main_tiles", "tail_ct",
               "rounds", "units", "cmod", "lds")


def bound(K):
    """B of |got - ref| <= B eps mag for a product over K table rows (module docstring)"""
    return K + 2


# ---- the plan, restated ----
def launches(ncells, K, N):
    """one dict per launch of wf_tsmm(ncells, K, N), keys LAUNCH_KEYS, in launch order"""
    tiles = (N + 15) // 16
    npass = (tiles + 7) // 8
    tpp = (tiles + npass - 1) // npass
    nk = (K + 127) // 128
    kc = 32 * (((K + nk - 1) // nk + 31) // 32)
    out = []
    for n0 in range(0, N, 16 * tpp):
        nt = min(tpp, (N - n0 + 15) // 16)
        NT = 4 if nt == 3 else min(nt, 8)
        for k0 in range(0, K, kc):
            kk = min(kc, K - k0)
            KT = (kk + 3) // 4
            nch = (KT + CHUNK - 1) // CHUNK
            NW = 16 * NT
            NP = NW + (0 if (NW & 31) == 16 else 16)
            ntiles = (ncells + 15) // 16
            nb = min(ntiles, GRID)
            nwaves = nb * WAVES
            rem = ntiles % nwaves
            main_tiles, tail_ct = ntiles, 0
            if rem > 0 and KT <= 4 * CHUNK:
                for ct in (1, 2, 4):
                    if ct < NT and rem * ((NT + ct - 1) // ct) <= nwaves:
                        tail_ct, main_tiles = ct, ntiles - rem
                        break
            out.append(dict(ncells=ncells, Kfull=K, N=N, n0=n0, NT=NT, nt=nt, k0=k0, K=kk, nch=nch, acc=int(k0 > 0), nb=nb,
                            ntiles=ntiles, rem=rem, main_tiles=main_tiles, tail_ct=tail_ct, rounds=(main_tiles + nwaves - 1) // nwaves,
                            units=(NT + tail_ct - 1) // tail_ct if tail_ct else 0, cmod=ncells % 16,
                            lds=(4 * CHUNK * nch + 4) * NP * 8))
    return out


def parse_walk(text):
    """the `launch` lines of tests/cxx/tsmm_plan_walk.cpp as dicts of ints"""
    rows = []
    for line in text.splitlines():
        if line.startswith("launch "):
            rows.append({k: int(v) for k, v in (kv.split("=") for kv in line.split()[1:])})
    return rows


def path_text(ls):
    """one line that names the path of a product's launches"""
    def one(l):
        main = f"main x{l['rounds']}" if l["main_tiles"] else "no main"
        tail = f"tail ct{l['tail_ct']} ({l['ntiles'] - l['main_tiles']} tiles, {l['units']} units)" if l["tail_ct"] else "no tail"
        return f"<{l['NT']},{'acc' if l['acc'] else 'ovw'}> nt{l['nt']} nch{l['nch']} {main}, {tail}"
    return " | ".join(one(l) for l in ls) + f"; cmod {ls[0]['cmod']}"


# ---- the cases: (name, (ncells, K, N), cmod, [(NT, nt, nch, ACC, tail_ct, rounds) per launch]) ----
def _tail(ncells, N, NT, nt, ct):
    # K = 129: row ranges 96 + 33, the second one ACC; the whole product in the tail (at most 2048 units)
    return (f"tail_ct{ct}_nt{NT}", (ncells, 129, N), ncells % 16, [(NT, nt, 3, 0, ct, 0), (NT, nt, 2, 1, ct, 0)])


CASES = [
    ("main_nt2_nch1_partial", (16395, 8, 24), 11, [(2, 2, 1, 0, 0, 1)]),
    ("main_nt8_nch2_partial_cells_and_columns", (16395, 40, 125), 11, [(8, 8, 2, 0, 0, 1)]),
    ("main_nt4_for_nt3_acc", (16395, 129, 40), 11, [(4, 3, 3, 0, 0, 1), (4, 3, 2, 1, 0, 1)]),
    ("main_passes_nt5_nt4_acc", (17591, 130, 129), 7, [(5, 5, 3, 0, 0, 1), (5, 5, 2, 1, 0, 1), (4, 4, 3, 0, 0, 1), (4, 4, 2, 1, 0, 1)]),
    ("main_nt7_three_ranges", (16395, 257, 104), 11, [(7, 7, 3, 0, 0, 1), (7, 7, 3, 1, 0, 1), (7, 7, 3, 1, 0, 1)]),
    ("main_nt6_three_ranges", (16395, 257, 96), 11, [(6, 6, 3, 0, 0, 1), (6, 6, 3, 1, 0, 1), (6, 6, 3, 1, 0, 1)]),
    ("main_nt8_acc", (16395, 129, 125), 11, [(8, 8, 3, 0, 0, 1), (8, 8, 2, 1, 0, 1)]),
    ("main_nt5_nch2_two_rounds", (49165, 40, 72), 13, [(5, 5, 2, 0, 0, 2)]),
    ("main_nt2_nch4_nch3_acc_two_rounds", (49165, 216, 24), 13, [(2, 2, 4, 0, 0, 2), (2, 2, 3, 1, 0, 2)]),
    ("main_two_exact_rounds_no_tail", (65536, 12, 32), 0, [(2, 2, 1, 0, 0, 2)]),
    ("main_three_rounds_nch1", (81933, 8, 24), 13, [(2, 2, 1, 0, 0, 3)]),
    # a fourth round consumes what the third hand-off loaded: in three rounds at nch 1 no chunk reads that set again
    ("main_four_rounds_nch1", (16 * (3 * 2048 + 1025) - 3, 8, 24), 13, [(2, 2, 1, 0, 0, 4)]),
    ("tail_ct4_nt5_after_main", (43961, 4, 80), 9, [(5, 5, 1, 0, 4, 1)]),
    ("tail_ct4_nt8_after_main", (16 * (2048 + 600) - 5, 8, 125), 11, [(8, 8, 1, 0, 4, 1)]),
    # every reachable (NT, tail_ct), each with ACC and a partial tile: 7 / 600 / 500 / 700 cell tiles
    _tail(100, 24, 2, 2, 1), _tail(100, 40, 4, 3, 1), _tail(100, 72, 5, 5, 1), _tail(100, 96, 6, 6, 1), _tail(100, 104, 7, 7, 1),
    _tail(100, 125, 8, 8, 1),
    _tail(9595, 40, 4, 3, 2), _tail(9595, 72, 5, 5, 2), _tail(9595, 96, 6, 6, 2), _tail(7995, 104, 7, 7, 2), _tail(7995, 125, 8, 8, 2),
    _tail(11195, 72, 5, 5, 4), _tail(11195, 96, 6, 6, 4), _tail(11195, 104, 7, 7, 4), _tail(11195, 125, 8, 8, 4),
]
CASE_IDS = [c[0] for c in CASES]
NAN_CASES = [("main", (16395, 40, 125)), ("tail", (100, 27, 40))]
STREAM_CASE = (16395, 257, 40)      # three row ranges, two of them ACC
HEADROOM_CASES = [(16395, 40, 125), (100, 27, 40), (130, 343, 216)]

# what the case table must cover, per layout (every case runs in both): sets of (NT, ...) tuples
MAIN_NT = (2, 4, 5, 6, 7, 8)
REQUIRED_MAIN_ACC = {(NT, acc) for NT in MAIN_NT for acc in (0, 1)}
REQUIRED_MAIN_PARTIAL = set(MAIN_NT)                       # cmod != 0 and the partial tile in the main loop
REQUIRED_MAIN_ROUNDS = {1, 2, 3, 4}                        # nch with at least two rounds
REQUIRED_TAIL = {(NT, 1) for NT in MAIN_NT} | {(NT, 2) for NT in (4, 5, 6, 7, 8)} | {(NT, 4) for NT in (5, 6, 7, 8)}


def coverage(all_launches):
    """(main (NT, acc), main NT with the partial tile, main nch with >= 2 rounds, tail (NT, ct), the same with ACC, the
    same with a partial tile) of a list of launch dicts"""
    main = [l for l in all_launches if l["main_tiles"] > 0]
    tail = [l for l in all_launches if l["tail_ct"] > 0]
    return ({(l["NT"], l["acc"]) for l in main},
            {l["NT"] for l in main if l["cmod"] and l["tail_ct"] == 0},
            {l["nch"] for l in main if l["rounds"] >= 2},
            {(l["NT"], l["tail_ct"]) for l in tail},
            {(l["NT"], l["tail_ct"]) for l in tail if l["acc"]},
            {(l["NT"], l["tail_ct"]) for l in tail if l["cmod"]})


# ---- rows of the rounding check ----
def required_rows(ncells, ls):
    """The rows the rounding check must hold, apart from the random ones: every cell of the first tile, of the last
    whole tile, of the partial tile, of the first and last tile of every round of every launch, and of every tile a
    tail takes when there are at most 64 (otherwise of the first and the last)."""
    ntiles = (ncells + 15) // 16
    tiles = {0, ntiles - 1}
    if ncells >= 16:
        tiles.add(ncells // 16 - 1)
    for l in ls:
        nwaves = l["nb"] * WAVES
        for r in range(l["rounds"]):
            tiles |= {r * nwaves, min((r + 1) * nwaves, l["main_tiles"]) - 1}
        if l["tail_ct"]:
            t0 = l["main_tiles"]
            tiles |= set(range(t0, ntiles)) if ntiles - t0 <= 64 else {t0, ntiles - 1}
    return _cells(tiles, ncells)


def _cells(tiles, ncells):
    rows = (np.asarray(sorted(tiles), dtype=np.int64)[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)
    return rows[rows < ncells]


def subset_rows(ncells, ls, seed=0):
    """required_rows, 32 random tiles of a tail of more than 64 tiles, and 256 random rows; sorted, unique.  The
    subset is a condition of the test, not a tolerance: asserted here."""
    rng = np.random.default_rng(seed)
    ntiles = (ncells + 15) // 16
    need = required_rows(ncells, ls)
    extra = [rng.choice(ncells, size=min(256, ncells), replace=False)]
    for l in ls:
        t0 = l["main_tiles"]
        if l["tail_ct"] and ntiles - t0 > 64:
            extra.append(_cells(set(t0 + rng.choice(ntiles - t0, size=32, replace=False)), ncells))
    rows = np.unique(np.concatenate([need] + extra))
    assert np.isin(need, rows).all() and rows[0] == 0 and rows[-1] == ncells - 1 and rows.size >= min(ncells, 256)
    return rows


# ---- data ----
def exact_data(ncells, K, N, seed=1):
    """(in [ncells, K], phi [K, N], in . phi [ncells, N]) of the exact data; the product is exact (module docstring)"""
    rng = np.random.default_rng([seed, ncells, K, N])
    ai = rng.integers(-15, 16, (ncells, K)).astype(np.float64)
    pi = rng.integers(-15, 16, (K, N)).astype(np.float64)
    ec = rng.integers(-20, 21, ncells)
    en = rng.integers(-20, 21, N)
    assert 225 * K < 2 ** 53
    prod = ai @ pi                                     # integers below 2^53: exact in float64 in any order
    return np.ldexp(ai, ec[:, None]), np.ldexp(pi, en[None, :]), np.ldexp(prod, ec[:, None] + en[None, :])


def rounding_data(ncells, K, N, field, seed=2):
    """(in [ncells, K], phi [K, N]) of one of FIELDS"""
    rng = np.random.default_rng([seed, ncells, K, N])
    a = rng.uniform(-1, 1, (ncells, K))
    p = rng.uniform(-1, 1, (K, N))
    s = lambda n: np.arange(n) / max(n - 1, 1)
    if field == "cell_up":                             # quiet in the first tile
        a *= np.exp2(-40.0 * (1.0 - s(ncells)))[:, None]
    elif field == "cell_down":                         # quiet in the last (partial) tile
        a *= np.exp2(-40.0 * s(ncells))[:, None]
    elif field == "k_decay":
        a *= np.exp2(-40.0 * s(K))[None, :]
    elif field == "n_decay":
        p *= np.exp2(-40.0 * s(N))[None, :]
    else:
        assert field == "uniform", field
    return a, p


def reference(a_rows, p):
    """(ref, mag) of a_rows . p: the long-double sum of K outer products, and the float64 |a_rows| |p|"""
    ref = np.zeros((a_rows.shape[0], p.shape[1]), dtype=LD)
    al, pl = a_rows.astype(LD), p.astype(LD)
    for k in range(p.shape[0]):
        ref += al[:, k, None] * pl[k, None, :]
    return ref, np.abs(a_rows) @ np.abs(p)


@functools.lru_cache(maxsize=2)
def case_data(name):
    """Everything of a case that does not depend on layout or alignment, computed once: its launches, the rows of the
    rounding check, the exact data and, per field, (in, phi, ref on the rows, mag on the rows).  Read-only."""
    ncells, K, N = next(c[1] for c in CASES if c[0] == name)
    ls = launches(ncells, K, N)
    rows = subset_rows(ncells, ls)
    d = {"shape": (ncells, K, N), "launches": ls, "rows": rows, "exact": exact_data(ncells, K, N), "fields": {}}
    for f in FIELDS:
        a, p = rounding_data(ncells, K, N, f)
        d["fields"][f] = (a, p) + reference(a[rows], p)
    for arrs in [d["exact"]] + list(d["fields"].values()):
        for x in arrs:
            x.setflags(write=False)
    return d


def flat_in(a, layout):
    """in as wf_tsmm takes it: [cell][k] (layout 0) or [k][cell] (layout 1)"""
    return (a if layout == 0 else np.ascontiguousarray(a.T)).reshape(-1)


def unflat_out(v, ncells, N, layout):
    """[ncells, N] view of out as wf_tsmm leaves it"""
    return v.reshape(ncells, N) if layout == 0 else v.reshape(N, ncells).T
