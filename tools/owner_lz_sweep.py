"""Prologue of a work item of the owner kernel, in layers: one point of a wf_tuning.lz sweep, and the fit.

  python3 tools/owner_lz_sweep.py point LZ [SIZE] >> sweep.jsonl     one process per lz: HIP-event median of the apply
  python3 tools/owner_lz_sweep.py fit sweep.jsonl                    t = a + b rounds lz + c rounds;  prologue = c / b

The planner's cost model (box_run_plan.h) charges a work item of L layers L + prologue; kOwnerPrologue is this fit."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def point(lz, size):
    import torch
    import wave_fenics_amd as w
    p, dev = 4, torch.device("cuda", 0)
    V = w.create_functionspace(w.create_box(size), p)
    V.structured = True
    op = w.StiffnessOperator(V, p, {"c0": 1500.0}, tuning={"lz": lz})
    assert op.update == "owner" and op.info.plan_lz == lz and len(op.runs()) == 0
    x = torch.rand(V.ndofs, dtype=torch.float64, device=dev)
    y = torch.zeros_like(x)
    for _ in range(1000):   # past the power ramp after idle
        op(x, y)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(200)]
    for a, b in ev:
        a.record()
        op(x, y)
        b.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3
    ncols = -(-(p * size + 1) // 32) * -(-(p * size + 1) // 8)   # the default 8 x 2 cross-section
    items = ncols * -(-size // lz)
    resident = 3 * torch.cuda.get_device_properties(0).multi_processor_count
    print(json.dumps({"size": size, "lz": lz, "items": items, "resident": resident, "rounds": -(-items // resident),
                      "median_us": round(float(np.median(t)), 3), "min_us": round(float(t.min()), 3)}), flush=True)


def fit(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    A = np.array([[1.0, r["rounds"] * r["lz"], r["rounds"]] for r in rows])
    t = np.array([r["median_us"] for r in rows])
    (a, b, c), *_ = np.linalg.lstsq(A, t, rcond=None)
    res = A @ np.array([a, b, c]) - t
    for r, d in zip(rows, res):
        print(f"lz {r['lz']:3d}  items {r['items']:5d}  rounds {r['rounds']:2d}  median {r['median_us']:8.2f} us  fit {d:+6.2f}")
    print(f"a = {a:.2f} us, b = {b:.3f} us per layer and round, c = {c:.3f} us per round: prologue = c / b = {c / b:.2f} layers "
          f"(rms residual {float(np.sqrt((res ** 2).mean())):.2f} us)")


if __name__ == "__main__":
    if sys.argv[1] == "point":
        point(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 54)
    else:
        fit(sys.argv[2])
