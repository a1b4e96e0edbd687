"""k_tsmm (csrc/tsmm.hip) on every path of its launch plan, entry by entry.

The older wf_tsmm tests (test_gpu_parity.py: test_tsmm_vs_numpy, test_tsmm_overwrites_out,
test_tsmm_8_byte_aligned_operands) reach the straight-line main loop with more than one accumulator tile per wave
(NT >= 2) only at six large shapes, with out zeroed, no sentinels and 1e-13 of the global maximum; a partial cell tile in
the main loop, several tiles per wave at nch = 2 or 3, tail_ct = 4 and <2, *, true> ran nowhere.  Here every case of
tsmm_helpers.CASES -- walked through csrc/tsmm_plan.h by tests/test_tsmm_host.py, which asserts the path each one is
named for and the coverage of the table as a whole -- runs

  * in both layouts, with in, phi and out inside padded buffers (16 sentinels of -7e77 on either side, as tsmm_check of
    test_gpu_parity.py), once 16-byte aligned and once one entry off, out full of NaN on entry;
  * on the exact data: EVERY entry of out equals the integer product, scaled (np.array_equal; no tolerance), which sees
    an indexing, overwrite or accumulate mistake anywhere;
  * on the five rounding fields: |got - ref| <= B eps mag per entry, B = K + 2 derived in tsmm_helpers, against the
    long-double reference on the rows of tsmm_helpers.subset_rows;
  * with the sentinels of all three buffers and the inputs unchanged bit for bit;

and prints one line with the path, the worst err / (eps mag) per field and B.  NaN isolation (what the clamped loads
re-read reaches no stored entry), stream order and ncells = 0 follow; the refusals need no GPU and are in
tests/test_tsmm_host.py.

That the tests bite: three variants of a scratch copy of tsmm.hip that change values only and no address, each run once
on an MI355X against this file and the three older tests (166 tests with the 28 cases the table then had; the unchanged
kernel passes all of them).
  (a) the main loop's ACC reload dropped, `if (ACC)` -> `if (false)` in chunk(), so that later row ranges overwrite:
      26 tests of this file fail -- all four runs of each of the six main-loop ACC cases (main_nt4_for_nt3_acc,
      main_passes_nt5_nt4_acc, main_nt7_three_ranges, main_nt6_three_ranges, main_nt8_acc,
      main_nt2_nch4_nch3_acc_two_rounds) on the exact check, and test_tsmm_runs_in_stream_order in both layouts; the
      tail's own ACC reload is untouched and every tail case passes.  Of the older tests
      test_tsmm_vs_numpy[35000-216-216] and test_tsmm_overwrites_out[33-343-1] (NT = 1) catch it; the rest pass.
  (b) the tail's B-operand column offset wrong for c >= 2, `16 * c` -> `16 * (c >= 2 ? c - 2 : c)` (an LDS read inside
      the table), which only tail_ct = 4 executes: 24 tests fail -- all four runs of the six tail_ct = 4 cases
      (tail_ct4_nt5_after_main, tail_ct4_nt8_after_main, tail_ct4_nt5 .. nt8); everything else passes.  The three older
      tests pass: none of them catches it.
  (c) the third hand-off of the unrolled main loop loading into the wrong register set, `chunk(a2, a1)` ->
      `chunk(a2, a0)`: wrong from the fourth (cell tile, chunk) pair of a wave on.  8 tests fail -- all four runs of
      main_nt5_nch2_two_rounds (nch = 2, two rounds: four pairs) and of main_nt2_nch4_nch3_acc_two_rounds; cases of at
      most three pairs per wave pass, main_three_rounds_nch1 among them, which is why main_four_rounds_nch1 was added
      after this run.  Of the older tests test_tsmm_vs_numpy at (100000 | 40000 | 60000, 125, 125) and (35000, 216, 216)
      and test_tsmm_overwrites_out[33-343-1] catch it."""
import numpy as np
import pytest

import tsmm_helpers as th
from support import gpu, ratio  # noqa: F401

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 16, -7.0e77


class Padded:
    """`values` on the device inside PAD sentinels on either side (and one more behind), `shift` entries off 16-byte
    alignment; untouched() compares the whole buffer, or with data=False the sentinels alone, with what was put there,
    bit for bit and on the device."""

    def __init__(self, gpu, values, shift):
        import torch
        self.lo, self.n = PAD + shift, values.size
        h = np.full(PAD + values.size + PAD + 1, SENTINEL)
        h[self.lo:self.lo + self.n] = values
        self.buf = torch.from_numpy(h).to(gpu)
        self.before = self.buf.clone()
        self.view = self.buf[self.lo:self.lo + self.n]
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == 8 * shift

    def untouched(self, data=True):
        import torch
        now, was = self.buf.view(torch.int64), self.before.view(torch.int64)
        if data:
            return torch.equal(now, was)
        return torch.equal(now[:self.lo], was[:self.lo]) and torch.equal(now[self.lo + self.n:], was[self.lo + self.n:])


def product(gpu, shape, layout, shift, a, p, stream=None):
    """wf_tsmm on (a, p) in padded buffers, out full of NaN on entry: out as [ncells, N], after the assertions on the
    sentinels and the inputs"""
    import torch
    import wave_fenics_amd as w
    ncells, K, N = shape
    b_in, b_phi = Padded(gpu, th.flat_in(a, layout), shift), Padded(gpu, p.reshape(-1), shift)
    b_out = Padded(gpu, np.full(ncells * N, np.nan), shift)
    w.tsmm(ncells, b_in.view, b_phi.view.view(K, N), b_out.view, layout=layout, stream=stream)
    torch.cuda.synchronize()
    assert b_out.untouched(data=False), "an entry outside out was written"
    assert b_in.untouched() and b_phi.untouched(), "an input or its padding was written"
    return th.unflat_out(b_out.view.cpu().numpy(), ncells, N, layout)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("name", th.CASE_IDS)
def test_tsmm_path(gpu, name, layout, shift):
    """one case of the table: exact in every entry, within B eps mag on every rounding field, nothing else touched"""
    d = th.case_data(name)
    shape, rows = d["shape"], d["rows"]
    B = th.bound(shape[1])
    a, p, c = d["exact"]
    got = product(gpu, shape, layout, shift, a, p)
    exact = np.array_equal(got, c)
    bad = np.argwhere(got != c)
    worst, fails = {}, []
    for f in th.FIELDS:
        a, p, ref, mag = d["fields"][f]
        got = product(gpu, shape, layout, shift, a, p)
        assert np.isfinite(got).all(), (f, "out was accumulated onto, not overwritten")
        worst[f], ok, first = ratio(got[rows], ref, mag, B)
        if not ok:
            fails.append((f, worst[f], int(rows[first // shape[2]]), first % shape[2]))
    print(f"tsmm {name} {shape} layout {layout} shift {shift}: {th.path_text(d['launches'])}; exact {'yes' if exact else 'NO'}; "
          + ", ".join(f"{f} {worst[f]:.2f}" for f in th.FIELDS) + f" eps mag, B = {B}")
    assert exact, f"{bad.shape[0]} entries differ from the exact product, the first at (cell, column) {bad[:5].tolist()}"
    assert not fails, fails


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which,shape", th.NAN_CASES)
def test_tsmm_nan_stays_in_its_row_and_column(gpu, which, shape, layout):
    """A NaN in `in` at one cell of a whole tile and at the last k of the last cell (of the partial tile: the entry the
    clamped loads of the rows past ncells and of the k past K read again) makes exactly those rows of out NaN; a NaN in
    the last row of one column of phi exactly that column.  Every other entry is the clean run's, bit for bit (no
    atomics: an entry is one wave's sum in a fixed order)."""
    ncells, K, N = shape
    assert ncells % 16 and K % 32                      # rows past ncells and k-steps past K exist, and are loaded clamped
    a, p = th.rounding_data(ncells, K, N, "uniform")
    clean = product(gpu, shape, layout, 0, a, p)
    assert np.isfinite(clean).all()
    c1, col = 37, 17
    an = a.copy()
    an[c1, 0] = an[ncells - 1, K - 1] = np.nan
    got = product(gpu, shape, layout, 0, an, p)
    nan_rows = np.zeros((ncells, N), dtype=bool)
    nan_rows[[c1, ncells - 1]] = True
    assert np.array_equal(np.isnan(got), nan_rows), np.argwhere(np.isnan(got) != nan_rows)[:5]
    assert np.array_equal(got[~nan_rows], clean[~nan_rows])
    pn = p.copy()
    pn[K - 1, col] = np.nan
    got = product(gpu, shape, layout, 0, a, pn)
    nan_col = np.zeros((ncells, N), dtype=bool)
    nan_col[:, col] = True
    assert np.array_equal(np.isnan(got), nan_col), np.argwhere(np.isnan(got) != nan_col)[:5]
    assert np.array_equal(got[~nan_col], clean[~nan_col])


@pytest.mark.parametrize("layout", [0, 1])
def test_tsmm_runs_in_stream_order(gpu, layout):
    """The three launches of a K > 128 product on a side stream, behind work and a fill of `in` queued on that stream:
    the result is that of the filled `in` (exact data, every entry)."""
    import torch
    import wave_fenics_amd as w
    ncells, K, N = th.STREAM_CASE
    a, p, c = th.exact_data(ncells, K, N)
    src = torch.from_numpy(th.flat_in(a, layout)).to(gpu)
    d_in = torch.zeros_like(src)
    d_phi = torch.from_numpy(p).to(gpu)
    d_out = torch.full((ncells * N,), float("nan"), dtype=torch.float64, device=gpu)
    busy = torch.ones(2048, 2048, dtype=torch.float64, device=gpu)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        for _ in range(4):
            busy = busy @ busy * 2.0 ** -11            # queued in front of the fill: the stream is busy when wf_tsmm returns
        d_in.copy_(src)
    w.tsmm(ncells, d_in, d_phi, d_out, layout=layout, stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(th.unflat_out(d_out.cpu().numpy(), ncells, N, layout), c)


@pytest.mark.parametrize("layout", [0, 1])
def test_tsmm_no_cells_leaves_out_untouched(gpu, layout):
    """ncells = 0: WF_OK and nothing written"""
    import torch
    import wave_fenics_amd as w
    b = Padded(gpu, np.full(64, np.nan), 1)
    phi = torch.ones(3, 5, dtype=torch.float64, device=gpu)
    w.tsmm(0, b.view, phi, b.view, layout=layout)
    torch.cuda.synchronize()
    assert b.untouched()
