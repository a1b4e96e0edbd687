#!/usr/bin/env python3
"""SHA-256 of everything the time-stepping layer writes, for comparing two builds bit for bit.

Uses public names of the package only, so the same file runs in a checkout of an older commit:

  python tools/time_step_bits.py                 (this tree)
  python tools/time_step_bits.py --root OTHER    (the package of the checkout at OTHER)

Seeded inputs.  Kernel groups: every compiled form of wf_rk4_stage(_bc), wf_leapfrog_step(_bc), wf_boundary_apply and
wf_boundary_apply_plan -- n in {1, 2, 65, 257, 385}, buffers shifted by 0 (16-byte aligned: the 16-byte kernels) and by
1 double (the scalar kernels), no plan and a random 30 % plan whose Gamma_1 and Gamma_2 overlap, has_next / v on and off.
Model groups: 5 steps each of rk4, rk4_fused and leapfrog on a P2 4x3x3 and a P4 3x2x2 box, one rank, with and without a
medium.  One JSON line: group -> hash over all output vectors of the group.

Only what is reproducible from run to run can be compared between builds, and atomic accumulation is not: the same
build gives other bits on every run.  So the models run the owner-computes stiffness kernel ({"update": "owner"}, no
atomics), take their diagonal m from a lumped mass operator with order-fixed accumulation (WF_FLAG_ORDERED) in place
of the atomically assembled one of the constructor, and carry Gamma_1 on the face x = lo and Gamma_2 on the face x = hi, which share no dof: wf_boundary_apply
adds both terms atomically, and a dof in both sets would receive them in either order.  For the same reason the
boundary_apply group starts from b = 0 at the dofs that lie in both sets (0 + x + y does not depend on the order).
The fused passes take overlapping sets from the plan, which accumulates on the host."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

SIZES = (1, 2, 65, 257, 385)
SHIFTS = (0, 1)


def boundary_sets(rng, n):
    """a random 30 % of the dofs, split into two overlapping sets with positive masses"""
    union = np.flatnonzero(rng.random(n) < 0.3).astype(np.int32)
    r = rng.random(union.size)
    i1, i2 = union[r < 0.6], union[r > 0.4]     # 0.4 .. 0.6: in both
    return i1, rng.uniform(0.5, 1.5, i1.size), i2, rng.uniform(0.5, 1.5, i2.size)


def kernel_hashes(torch, la, dev):
    out = {}

    def vec(rng, n, shift, lo=-1.0, hi=1.0):
        buf = torch.zeros(n + 2, dtype=torch.float64, device=dev)
        v = buf[shift:shift + n]
        v.copy_(torch.from_numpy(rng.uniform(lo, hi, n)))
        return v

    for group in ("rk4_stage", "leapfrog_step", "boundary_apply"):
        h = hashlib.sha256()
        rng = np.random.default_rng(27)
        for n in SIZES:
            for shift in SHIFTS:
                for planned in (False, True):
                    i1, m1, i2, m2 = boundary_sets(rng, n)
                    plan = la.BoundaryPlan(n, i1, m1, i2, m2) if planned else None
                    for flag in (False, True):
                        if group == "rk4_stage":
                            b, vn, ur, vr, u0, v0 = (vec(rng, n, shift) for _ in range(6))
                            m = vec(rng, n, shift, 0.5, 1.5)
                            u_, v_, un, vn_next = (vec(rng, n, shift) for _ in range(4))
                            nxt = dict(adt_next=0.4, u0=u0, v0=v0, un=un, vn_next=vn_next) if flag else {}
                            la.rk4_stage(b, m, vn, ur, vr, u_, v_, 0.3, bc=plan, s1_next=1.7, s2=-1.3, **nxt)
                            res = (b, u_, v_, un, vn_next)
                        elif group == "leapfrog_step":
                            b, u, up = (vec(rng, n, shift) for _ in range(3))
                            m = vec(rng, n, shift, 0.5, 1.5)
                            un, v = vec(rng, n, shift), vec(rng, n, shift)
                            la.leapfrog_step(b, m, u, up, un, 0.05, v=v if flag else None, bc=plan, s1=1.7, s2=-1.3)
                            la.leapfrog_step(b, m, u, up, up, 0.05, v=v if flag else None, bc=plan, s1=0.9, s2=-1.3)   # in place
                            res = (b, un, up, v)
                        else:
                            if not planned:
                                continue
                            b, v = vec(rng, n, shift), vec(rng, n, shift)
                            b[torch.from_numpy(np.intersect1d(i1, i2)).to(dev, dtype=torch.int64)] = 0.0
                            if flag:
                                plan.apply(1.7, -1.3, v, b)
                            else:
                                t = lambda a, dt: torch.from_numpy(a).to(dev, dtype=dt)
                                la.boundary_apply(t(i1, torch.int32), t(m1, torch.float64), 1.7, t(i2, torch.int32), t(m2, torch.float64),
                                                  -1.3, v, b)
                            res = (b,)
                        torch.cuda.synchronize()
                        for r in res:
                            h.update(r.cpu().numpy().tobytes())
        out[group] = h.hexdigest()
    return out


def model_hashes(torch, w, dev):
    from wave_fenics_amd import _lib
    from wave_fenics_amd.linear_gll import LinearGLLOpt, cfl_time_step
    from wave_fenics_amd.operators import MassOperatorLumped
    out = {}
    for p, n in ((2, (4, 3, 3)), (4, (3, 2, 2))):
        mesh = w.create_box(n, hi=(0.01, 0.0075, 0.0075))
        V = w.create_functionspace(mesh, p)
        dt, _ = cfl_time_step(mesh, p, 1500.0, 0.5e6, CFL=0.25)
        rng = np.random.default_rng(p)
        media = {"": None, "_medium": w.Medium(rng.uniform(1400.0, 1600.0, mesh.ncells), rng.uniform(900.0, 1100.0, mesh.ncells))}
        for mname, medium in media.items():
            mass = MassOperatorLumped(V, p, structured=False, flags=_lib.WF_FLAG_ORDERED,
                                      cell_coeff=None if medium is None else medium.mass_coeff)
            m = torch.zeros(V.ndofs, dtype=torch.float64, device=dev)
            mass(torch.ones_like(m), m)
            for scheme in ("rk4", "rk4_fused", "leapfrog"):
                eqn = LinearGLLOpt(V, p, 1500.0, 0.5e6, 6e4, device=dev, medium=medium, tags={0: 1, 1: 2},
                                   tuning={"update": "owner"})
                assert float((eqn.m - m).abs().max() / m.abs().max()) < 1e-14
                eqn.m.copy_(m)
                eqn.init()
                # two calls: the second starts from a state that is not at rest
                getattr(eqn, scheme)(0.0, 2 * dt - 1e-13, dt)
                getattr(eqn, scheme)(2 * dt, 5 * dt - 1e-13, dt)
                torch.cuda.synchronize()
                h = hashlib.sha256()
                for r in (eqn.u_n, eqn.v_n):
                    a = r.cpu().numpy()
                    assert np.isfinite(a).all() and np.abs(a).max() > 0.0, (p, mname, scheme)
                    h.update(a.tobytes())
                out[f"P{p}{mname}_{scheme}"] = h.hexdigest()
    return out


def hashes():
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd import la
    dev = torch.device("cuda", 0)
    return {**kernel_hashes(torch, la, dev), **model_hashes(torch, w, dev)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout whose package runs (its library must be built)")
    sys.path.insert(0, os.path.abspath(ap.parse_args().root))
    print(json.dumps(hashes(), sort_keys=True))
