#!/usr/bin/env python3
"""Three steps of one time loop of LinearGLLOpt for a kernel trace: one rank, P2 on a 4 x 3 x 3 box, --points adds one
point source and one receiver.  Public names of the package only, so the same file runs on the checkout of another
commit (--root), and the kernel-name sequences of two commits can be compared (profiles/r36_summary.md):

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/loop_trace.py --loop rk4_fused [--points] [--root OTHER]

Set-up ends with a marker -- a cumulative sum of five int16, a kernel nothing else here launches -- and a synchronise;
the loop's launches are what follows the marker in the trace, sorted by start time."""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="checkout whose package runs (its library must be built)")
ap.add_argument("--loop", required=True, choices=["rk4", "rk4_fused", "leapfrog"])
ap.add_argument("--points", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import wave_fenics_amd as w  # noqa: E402
from wave_fenics_amd import points  # noqa: E402
from wave_fenics_amd.linear_gll import LinearGLLOpt, cfl_time_step  # noqa: E402

dev = torch.device("cuda", 0)
p, n, hi = 2, (4, 3, 3), (0.01, 0.0075, 0.0075)
mesh = w.create_box(n, hi=hi)
V = w.create_functionspace(mesh, p)
dt, _ = cfl_time_step(mesh, p, 1500.0, 0.5e6, CFL=0.25)
src = rec = None
if args.points:
    src = points.Sources(V, [(0.003, 0.004, 0.002)], [points.ricker(0.5e6, 3.0e-6, 1.0e9)])
    rec = points.Receivers(V, [(0.006, 0.002, 0.005)], device=dev)
eqn = LinearGLLOpt(V, p, 1500.0, 0.5e6, 6e4, device=dev, tags={0: 1, 1: 2}, sources=src, receivers=rec)
eqn.init()
torch.cuda.synchronize()
mark = torch.arange(5, device=dev, dtype=torch.int16).cumsum(0)
torch.cuda.synchronize()
t, steps = getattr(eqn, args.loop)(0.0, 3 * dt - 1e-13, dt)
torch.cuda.synchronize()
assert steps == 3 and int(mark[-1]) == 10
print("ok", args.loop, args.points, t, steps)
