"""Guarded device buffers for the operator tests (tests/test_gpu_guarded_buffers.py, tests/test_gpu_parts_matrix.py).

guarded(values, pad, shift, fill, device) puts a vector in the middle of one larger allocation,

    [ pad sentinels | shift sentinels | the data | pad sentinels ]

and returns the 1-D contiguous float64 view of the data with a handle that says, after a run, which padding entries
no longer hold the sentinel.  Padding is compared as bit patterns (.view(torch.int64)), never with == on doubles: -0.0
== +0.0, and NaN != NaN.  shift = 1 moves the data to an address that is 8 but not 16 bytes aligned, which is all
include/wavehip.h promises for a d_ pointer.

Sentinels:
  x  NaN             any padding value that is USED makes y non-finite (assert y finite)
  y  NEG_ZERO -0.0   changes under a plain store, under an add of anything non-zero and under an add of +0.0
                     (-0.0 + +0.0 = +0.0); it does not change under an add of -0.0, which an idle lane can produce
                     (the stiffness kernels scale by coeff = -c0^2)
  y  MIN_NORMAL      2^-1022: changes under every store and under every add except +-0.0
Two runs, one with each y sentinel, leave exactly one stray access unseen: an add of -0.0.  (NaN is no sentinel for
y: an add onto NaN keeps its bits.)

pad is chosen by the caller so that an overrun of a row or a plane (box operators: 2 NX NY + NX entries) or of a
batch (2 nd entries) stays inside the allocation; at least 4096 entries either way."""
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wave_fenics_amd", "csrc")


def compiled_shapes(source, macro):
    """The entries X(a, b, ...) of the list `#define <macro>(X) ...` in csrc/<source>, as tuples of ints in the order
    of the list: the kernels that file compiles (WF_MARCH_SHAPES, WF_KS_SHAPES, WF_OWNER_SHAPES, WF_MASS_SHAPES,
    WF_IDX_SHAPES).  Read from the source, so that a retuned list moves the tests' shapes with it."""
    with open(os.path.join(CSRC, source)) as f:
        lines = f.read().split("\n")
    start = next(i for i, ln in enumerate(lines) if ln.startswith(f"#define {macro}(X)"))
    body, i = [lines[start][len(f"#define {macro}(X)"):]], start
    while lines[i].rstrip().endswith("\\"):
        i += 1
        body.append(lines[i])
    out = [tuple(int(v) for v in m.split(",")) for m in re.findall(r"X\(([0-9, ]+)\)", " ".join(body))]
    assert out, (source, macro)
    return out


NAN = float("nan")
NEG_ZERO = -0.0
MIN_NORMAL = 2.0 ** -1022


def box_pad(NX, NY):
    """padding of a vector on the dof lattice NX x NY x NZ: two planes and a row, at least 4096"""
    return max(4096, 2 * NX * NY + NX)


def batch_pad(nd):
    """padding of a vector of a cell-batch kernel with nd dofs per cell"""
    return 4096 + 2 * nd


class Guard:
    """The padding of one guarded buffer: changed() lists the padding entries whose bits are no longer the sentinel's,
    as offsets from the first data entry (negative: in front of the data; >= n: behind it)."""

    def __init__(self, buf, lo, n, fill):
        self.buf, self.lo, self.n = buf, lo, n
        self.fill_bits = int(np.array([fill], dtype=np.float64).view(np.int64)[0])

    def changed(self):
        import torch
        bad = self.buf.view(torch.int64) != self.fill_bits
        bad[self.lo:self.lo + self.n] = False
        return (torch.nonzero(bad).flatten() - self.lo).cpu().numpy()

    def intact(self):
        return self.changed().size == 0


def guarded(values, pad, shift, fill, device):
    """(view, guard): the float64 device vector `values` inside pad + shift sentinels in front and pad behind.  pad is
    rounded up to an even count, so that shift alone decides the alignment of the view: 16 bytes at shift = 0, 8 at 1."""
    import torch
    assert shift in (0, 1)
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    pad = int(pad) + (int(pad) & 1)
    lo, n = pad + shift, v.size
    host = np.full(lo + n + pad, fill, dtype=np.float64)     # numpy keeps the sentinel's bits (the sign of -0.0)
    host[lo:lo + n] = v
    buf = torch.from_numpy(host).to(device)
    view = buf[lo:lo + n]
    assert view.is_contiguous() and view.numel() == n and view.data_ptr() % 16 == 8 * shift
    return view, Guard(buf, lo, n, fill)
