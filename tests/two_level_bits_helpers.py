"""The generator of tests/golden/two_level_bits.json and the runs of tests/test_gpu_two_level_bits.py: the bits of the
fourth-order leapfrog loop and of both misfit gradients on the two boxes of tests/wave_loop_helpers.py (P2 on 3 x 2 x 2
cells, P4 on 2 x 2 x 2; owner-computes stiffness kernel, ordered mass, one source, two receivers), where a build
reproduces its own bits.

runs() lists, per box:
  leapfrog4, leapfrog4_max{0,1,4}, leapfrog4_t0_at_tf, leapfrog4_t0_past_tf_max1
      the runs wave_loop_helpers.runs() has for the other two loops, digested by wave_loop_helpers.digest;
  gradient_{leapfrog,leapfrog4}_S{1,3,7,None}
      misfit_gradient of N = 7 steps against a seeded observed [8, 2], by checkpoint_every;
  gradient_{leapfrog,leapfrog4}_medium
      the same (checkpoint_every = 3) on a model with a seeded medium, whose gradients end with the division by the
      medium's coefficients.
A gradient's SHA-256 runs over J, g_stiff, g_mass, the sorted items of info, the traces, u_n and v_n.

Public names only (LinearGLLOpt's methods, Medium, the operators), so the same file runs on an older checkout:

    python tests/two_level_bits_helpers.py --root CHECKOUT --write     records the fixture from the package at CHECKOUT

Everything runs twice, and nothing is written unless both passes give the same hashes: a fixture its own commit does
not reproduce pins nothing.  The fixture in the tree was recorded from commit 0c79b90, the last one with the two misfit
gradients written out side by side and the hooked fourth-order loop an entry of its own."""
import argparse
import hashlib
import json
import os
import struct
import sys

import numpy as np

import wave_loop_helpers as wh

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "two_level_bits.json")
N = 7
CHECKPOINTS = (1, 3, 7, None)
SCHEMES = ("leapfrog", "leapfrog4")


def observed(box):
    """the seeded [N + 1, 2] traces the misfit compares with, of the size of the start state"""
    return np.random.default_rng(200 + box.p).uniform(-1.0, 1.0, (N + 1, len(wh.RECEIVERS_AT)))


def medium_model(box):
    """box.model() with a seeded medium: c in [1400, 1600], rho in [900, 1100] per cell, m from the ordered mass"""
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd import _lib, points
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    from wave_fenics_amd.operators import MassOperatorLumped
    rng = np.random.default_rng(300 + box.p)
    ncells = box.mesh.ncells
    medium = w.Medium(rng.uniform(1400.0, 1600.0, ncells), rng.uniform(900.0, 1100.0, ncells))
    mass = MassOperatorLumped(box.V, box.p, structured=False, flags=_lib.WF_FLAG_ORDERED, cell_coeff=medium.mass_coeff)
    m = torch.zeros(box.V.ndofs, dtype=torch.float64, device=box.dev)
    mass(torch.ones_like(m), m)
    src = points.Sources(box.V, wh.SOURCE_AT, [points.ricker(wh.FREQ, 1.5 / wh.FREQ, 3.0e9)])
    rec = points.Receivers(box.V, wh.RECEIVERS_AT, device=box.dev, capacity=64)
    eqn = LinearGLLOpt(box.V, box.p, wh.C0, wh.FREQ, wh.P0, device=box.dev, tags={0: 1, 1: 2}, tuning={"update": "owner"},
                       medium=medium, sources=src, receivers=rec)
    assert float((eqn.m - m).abs().max() / m.abs().max()) < 1e-14
    eqn.m.copy_(m)
    eqn.u_n.copy_(box.u0)
    eqn.v_n.copy_(box.v0)
    return eqn


def runs(box):
    """name -> ("loop", t0, tf, max_steps) or ("gradient", scheme, checkpoint_every, with a medium)"""
    dt = box.dt
    out = {"leapfrog4": ("loop", 0.0, wh.STEPS * dt - 1e-13, None)}
    for k in (0, 1, wh.STEPS):
        out[f"leapfrog4_max{k}"] = ("loop", 0.0, 1.0, k)
    out["leapfrog4_t0_at_tf"] = ("loop", 3 * dt, 3 * dt, None)
    out["leapfrog4_t0_past_tf_max1"] = ("loop", 3 * dt, 2 * dt, 1)
    for scheme in SCHEMES:
        for S in CHECKPOINTS:
            out[f"gradient_{scheme}_S{S}"] = ("gradient", scheme, S, False)
        out[f"gradient_{scheme}_medium"] = ("gradient", scheme, 3, True)
    return out


def run(box, kind, *spec):
    """the digest of one entry of runs()"""
    import torch
    if kind == "loop":
        t0, tf, max_steps = spec
        eqn = box.model()
        t, steps = eqn.leapfrog4(t0, tf, box.dt, max_steps=max_steps)
        assert eqn.receivers.traces.shape[0] == steps + 1
        return wh.digest(eqn, t, steps)
    scheme, S, with_medium = spec
    eqn = medium_model(box) if with_medium else box.model()
    J, g_stiff, g_mass, info = eqn.misfit_gradient(0.0, N * box.dt - 1e-13, box.dt, observed(box), checkpoint_every=S,
                                                   scheme=scheme)
    torch.cuda.synchronize()
    assert info["N"] == info["steps"] == N and eqn.receivers.traces.shape[0] == N + 1
    assert float(g_stiff.abs().max()) > 0.0 and float(g_mass.abs().max()) > 0.0
    h = hashlib.sha256()
    h.update(struct.pack("<d", float(J)))
    for r in (g_stiff, g_mass, eqn.receivers.traces, eqn.u_n, eqn.v_n):
        a = r.cpu().numpy()
        assert np.isfinite(a).all()
        h.update(np.ascontiguousarray(a).tobytes())
    for key, value in sorted(info.items()):
        h.update(key.encode() + (struct.pack("<d", value) if isinstance(value, float) else struct.pack("<q", int(value))))
    return h.hexdigest()


def record(dev):
    out = {}
    for p, n in wh.BOXES:
        box = wh.Box(p, n, dev)
        for name, spec in runs(box).items():
            out[f"P{p}_{name}"] = run(box, *spec)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout whose package runs (its library must be built)")
    ap.add_argument("--write", action="store_true", help="write the fixture (else print the hashes)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    first, second = record(torch.device("cuda", 0)), record(torch.device("cuda", 0))
    differ = sorted(k for k in first if first[k] != second[k])
    print(json.dumps(first, sort_keys=True))
    if differ:
        sys.exit(f"two passes of the same build differ in {differ}: nothing written")
    if args.write:
        with open(FIXTURE, "w") as f:
            json.dump(first, f, indent=0, sort_keys=True)
            f.write("\n")
