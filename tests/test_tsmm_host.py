"""wf_tsmm without a GPU: the launch plan (csrc/tsmm_plan.h, the header tsmm.hip launches from) walked by
tests/cxx/tsmm_plan_walk.cpp, the case table of tests/tsmm_helpers.py held against it, the references of the GPU
tests (tests/test_gpu_tsmm_paths.py) and wf_tsmm's refusals, which precede every device call.

The refusals are here and not in tests/golden/refusal_table.json: that table's generator (tests/refusal_helpers.py)
builds operator descriptors for the four creation entry points and takes no free function."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tsmm_helpers as th
from support import ratio, wlib  # noqa: F401
from test_op_lists_host import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """tsmm_plan_walk.cpp as a stand-alone program: plain C++17 with the csrc directory as the only include path (no HIP
    header is in reach, so tsmm_plan.h is HIP-free), under AddressSanitizer and UndefinedBehaviorSanitizer (host code
    only; nothing of it is loaded into this process).  Returns run(args) -> stdout, asserting a clean exit."""
    exe = str(tmp_path_factory.mktemp("tsmm") / "tsmm_plan_walk")
    subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "wave_fenics_amd", "csrc"), os.path.join(ROOT, "tests", "cxx", "tsmm_plan_walk.cpp"),
                           "-o", exe])

    def run(args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        lines = out.stdout.splitlines()
        assert out.returncode == 0 and lines and lines[-1] == "0 failures", out.stdout[-4000:] + out.stderr[-4000:]
        return out.stdout
    return run


def walked(walk, shapes):
    """the header's launches of each (ncells, K, N), one list per shape"""
    rows = th.parse_walk(walk([v for s in shapes for v in s]))
    out = {s: [r for r in rows if (r["ncells"], r["Kfull"], r["N"]) == tuple(s)] for s in shapes}
    assert sum(len(v) for v in out.values()) == len(rows)
    return out


def test_cases_take_the_paths_they_are_named_for(walk):
    """Every case of tsmm_helpers.CASES, walked through the header: launch by launch (NT, nt, nch, ACC, tail_ct, rounds)
    and the partial cell tile are what the table says; the Python restatement the GPU tests take their rows from agrees
    with the header in every field, for the cases, the NaN and stream cases and the shapes of the three older tests."""
    older = [(1000, 125, 125), (37, 27, 27), (513, 64, 64), (100, 8, 8), (77, 35, 192), (50, 125, 216), (16, 3, 5), (300, 216, 216),
             (130, 343, 343), (40, 512, 512), (64, 129, 40), (33, 216, 125), (100000, 125, 125), (40000, 125, 125), (60000, 125, 125),
             (70000, 27, 27), (35000, 216, 216), (32768, 64, 64), (4099, 125, 125), (1, 1, 1), (1, 129, 216), (50, 35, 1)]
    shapes = [c[1] for c in th.CASES] + [s for _, s in th.NAN_CASES] + [th.STREAM_CASE] + th.HEADROOM_CASES + older
    shapes = list(dict.fromkeys(shapes))
    got = walked(walk, shapes)
    for s in shapes:
        assert got[s] == th.launches(*s), s
        assert all(set(r) == set(th.LAUNCH_KEYS) for r in got[s])
    for name, shape, cmod, want in th.CASES:
        ls = got[shape]
        assert [(l["NT"], l["nt"], l["nch"], l["acc"], l["tail_ct"], l["rounds"]) for l in ls] == want, (name, th.path_text(ls))
        assert all(l["cmod"] == cmod for l in ls), name
        if name.startswith("main"):
            assert all(l["main_tiles"] == l["ntiles"] and l["tail_ct"] == 0 for l in ls), name
        if "after_main" in name:
            assert all(l["main_tiles"] == 2048 and l["units"] == 2 for l in ls), name
        if name.startswith("tail_ct") and "after_main" not in name:
            assert all(l["main_tiles"] == 0 for l in ls), name
    # named paths the tuple does not show
    by = {c[0]: got[c[1]] for c in th.CASES}
    assert [l["K"] for l in by["main_nt4_for_nt3_acc"]] == [96, 33]
    assert [l["K"] for l in by["main_nt7_three_ranges"]] == [96, 96, 65] and [l["K"] for l in by["main_nt2_nch4_nch3_acc_two_rounds"]] == [128, 88]
    assert by["main_two_exact_rounds_no_tail"][0]["rem"] == 0 and by["main_two_exact_rounds_no_tail"][0]["ntiles"] == 4096
    assert by["tail_ct4_nt5_after_main"][0]["NT"] % by["tail_ct4_nt5_after_main"][0]["tail_ct"] != 0      # last unit not full
    # the NaN cases: one in the main loop, one in the tail; the stream case: three launches, K > 128
    nan_main, nan_tail = got[th.NAN_CASES[0][1]], got[th.NAN_CASES[1][1]]
    assert all(l["tail_ct"] == 0 for l in nan_main) and all(l["tail_ct"] == 1 and l["main_tiles"] == 0 for l in nan_tail)
    assert [l["acc"] for l in got[th.STREAM_CASE]] == [0, 1, 1]
    # what the issue found of the older tests: with N > 16 their small shapes never enter the main loop
    for s in older:
        if s[0] <= 4099 and s[2] > 16:
            assert all(l["main_tiles"] == 0 or l["NT"] == 1 for l in got[s]), s


def test_case_table_covers_every_path(walk):
    """Per layout (every case runs in both): the main loop at every NT with ACC false and true, at every NT with the
    partial cell tile in the main loop, at nch 1..4 with at least two rounds; the tail at every reachable (NT, tail_ct),
    each with ACC and each with a partial tile.  Computed from the header's walk, not from the restatement."""
    got = walked(walk, [c[1] for c in th.CASES])
    main_acc, main_partial, main_rounds, tail, tail_acc, tail_partial = th.coverage([l for ls in got.values() for l in ls])
    assert main_acc >= th.REQUIRED_MAIN_ACC, th.REQUIRED_MAIN_ACC - main_acc
    assert main_partial >= th.REQUIRED_MAIN_PARTIAL, th.REQUIRED_MAIN_PARTIAL - main_partial
    assert main_rounds >= th.REQUIRED_MAIN_ROUNDS, th.REQUIRED_MAIN_ROUNDS - main_rounds
    assert tail == th.REQUIRED_TAIL, tail ^ th.REQUIRED_TAIL          # equality: no other pair is reachable at these shapes
    assert tail_acc == th.REQUIRED_TAIL and tail_partial == th.REQUIRED_TAIL
    # every array of every case stays under 64 MB, but for `in` of (49165, 216, 24) with 81 MB: two rounds at nch = 4 need
    # 49165 cells (3073 cell tiles) of more than 96 table rows
    big = [(name, 8 * nc * max(K, N)) for name, (nc, K, N), _, _ in th.CASES if 8 * nc * max(K, N) >= 64 * 2 ** 20]
    assert big == [("main_nt2_nch4_nch3_acc_two_rounds", 8 * 49165 * 216)]


def test_plan_tiles_every_table_once_within_lds(walk):
    """Exhaustive: for every K, N in 1..600 the row ranges and column passes tile [0, K) x [0, N) exactly once, no LDS
    table exceeds 160 KB, and every launch is one k_tsmm can take (an instantiation that exists, at most four chunks,
    ranges on chunk boundaries, a pass's ranges in ascending order)."""
    out = walk(["--exhaustive", 600])
    line = next(ln for ln in out.splitlines() if ln.startswith("exhaustive "))
    f = {k: int(v) for k, v in (kv.split("=") for kv in line.split()[1:])}
    assert f["kmax"] == 600 and f["products"] == 360000 and f["launches"] >= f["products"]
    assert f["lds_limit"] == th.LDS_LIMIT and f["max_lds"] <= th.LDS_LIMIT
    assert f["max_launches"] == 25                                     # 600 = 5 passes x 5 ranges


def test_row_subset_holds_the_required_rows():
    """the rows of the rounding check: first tile, last whole tile, partial tile, first and last tile of every round,
    the tail's tiles (all of at most 64; else first, last and 32 random), 256 random rows"""
    for name, (ncells, K, N), cmod, _ in th.CASES:
        ls = th.launches(ncells, K, N)
        rows = th.subset_rows(ncells, ls)
        ntiles = (ncells + 15) // 16
        assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < ncells
        have = set((rows // 16).tolist())
        assert np.isin(np.arange(16), rows).all() and np.isin(np.arange(16 * (ntiles - 1), ncells), rows).all()
        if ncells >= 16:
            assert np.isin(np.arange(16 * (ncells // 16 - 1), 16 * (ncells // 16)), rows).all()
        for l in ls:
            nwaves = l["nb"] * th.WAVES
            for r in range(l["rounds"]):
                assert {r * nwaves, min((r + 1) * nwaves, l["main_tiles"]) - 1} <= have, (name, r)
            if l["tail_ct"]:
                taken = set(range(l["main_tiles"], ntiles))
                assert taken <= have if len(taken) <= 64 else len(taken & have) >= 34 and {l["main_tiles"], ntiles - 1} <= have, name
        assert rows.size >= min(ncells, 256)


def test_exact_data_is_exact():
    """the exact data's product is the same number in long double, and summed in the reverse order"""
    for ncells, K, N in ((100, 129, 125), (531, 257, 40)):
        a, p, c = th.exact_data(ncells, K, N)
        ref, _ = th.reference(a, p)
        assert np.array_equal(ref, c.astype(th.LD)) and np.array_equal(a[:, ::-1] @ p[::-1], c)
        assert np.abs(np.log2(np.abs(a[a != 0]))).max() <= 24 and len(np.unique(np.abs(c))) > 1000


@pytest.mark.parametrize("shape", th.HEADROOM_CASES)
def test_reference_headroom(shape):
    """The float64 numpy product of the rounding data stays inside B = K + 2 of the long-double reference, entry by entry,
    on the rows the GPU tests check: the bound has room for a correct float64 product (measured here: about 2 to 3
    eps mag at K = 27 .. 343)."""
    ncells, K, N = shape
    rows = th.subset_rows(ncells, th.launches(ncells, K, N))
    for f in th.FIELDS:
        a, p = th.rounding_data(ncells, K, N, f)
        ref, mag = th.reference(a[rows], p)
        worst, ok, first = ratio(a[rows] @ p, ref, mag, th.bound(K))
        print(f"tsmm headroom {shape} {f}: {worst:.2f} eps mag, B = {th.bound(K)}")
        assert ok, (f, worst, first)
        assert worst > 0.0                                              # the reference is not the float64 product itself


# ---- refusals ----
WANT_LAYOUT = "wf_tsmm: layout must be 0 (cell-major) or 1 (cell-minor)"
WANT_ARGS = "wf_tsmm: bad arguments"
WANT_CELLS = "wf_tsmm: at most 2^27 cells per call (32-bit lane offsets)"


def test_tsmm_refusals_before_any_device_call(wlib):
    """layout = 2, K = 0, N = 0, ncells < 0, ncells = 2^27 and each null pointer: WF_ERR_INVALID with wf_tsmm's text, on
    a machine without a GPU, so before any device call (the pointers are host addresses, never dereferenced);
    ncells = 0 returns WF_OK and leaves out as it was."""
    L = wlib.lib()
    buf = np.full(64, -7.0e77)
    before = buf.copy()
    ptr = buf.ctypes.data

    def call(layout=0, ncells=4, K=3, N=5, d_in=ptr, d_phi=ptr + 128, d_out=ptr + 256):
        rc = L.wf_tsmm(layout, ncells, K, N, d_in, d_phi, d_out, None)
        return rc, L.wf_last_error().decode()

    INVALID = -1
    assert call(layout=2) == (INVALID, WANT_LAYOUT) and call(layout=-1) == (INVALID, WANT_LAYOUT)
    for kw in (dict(K=0), dict(N=0), dict(K=-3), dict(ncells=-1), dict(d_in=None), dict(d_phi=None), dict(d_out=None)):
        assert call(**kw) == (INVALID, WANT_ARGS), kw
    assert call(ncells=2 ** 27) == (INVALID, WANT_CELLS) and call(ncells=2 ** 40) == (INVALID, WANT_CELLS)
    # the order of the checks: layout first, then the arguments, then the cell count
    assert call(layout=2, K=0) == (INVALID, WANT_LAYOUT) and call(ncells=2 ** 27, N=0) == (INVALID, WANT_ARGS)
    for layout in (0, 1):
        assert call(layout=layout, ncells=0)[0] == 0
    assert np.array_equal(buf.view(np.int64), before.view(np.int64))
