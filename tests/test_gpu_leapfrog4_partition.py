"""LinearGLLOpt.leapfrog4 and leapfrog over the library's own ghost exchange, from a state in which every interface is live.

test_gpu_partition_models.py runs the loops on several ranks, where the halo is the model's _rhs over gloo, a callback of
the loop.  The route a multi-GPU run takes is another: Loop::rhs of csrc/wave_loops.cpp -- wf_op_apply_overlapped (split),
or wf_updater_fwd / wf_op_apply / wf_updater_rev (unsplit) -- over RCCL.  One process can drive it: a one-rank periodic
partition is its own neighbour (test_gpu_comm.py).  The tests of that route so far start from rest, where the start-up's
K v0 multiplies zeros and 20 steps hardly reach an interface (test_partition_scenario_host.py).  Here the state is the
random one of partition_helpers.initial_state on the periodic global numbering, taken to local through l2g:

  box (3, 3, 4), periodic y and z     absorbing x faces cut by the y and z self-interfaces
  box (3, 4, 3), fully periodic       no boundary set at all, every face a self-interface

P2, 20 steps at CFL 0.5 (the cfl_lf of the P2 cases of partition_helpers), each of box kernel / marching dofmap kernel
x split / unsplit, for leapfrog4 and for leapfrog:

* u_n and v_n, ghosts included, to 1e-9 of their maxima against the numpy steppers (leapfrog4_helpers.leapfrog4,
  leapfrog_helpers.leapfrog) on the oracle's periodic mesh -- the bound of the model tests over the same 20 steps;
* every ghost entry carries its owner's bits (the finish of leapfrog4 corrects v_n at ghosts from a b that is only the
  rank's own part there; the closing forward halo puts the owner's value back);
* b is left +0.0 on every owned entry (the next call's apply adds onto it); the ghost entries that are not are counted;
* leapfrog4, 5 + 5 steps against the stepper split 5 + 5, to 1e-9 (a split run differs from the continuous one by
  truncation: the start-up is a Taylor series).

The C++ model: planar3d --scheme leapfrog4 --periodic yz from rest (the example has no random state) -- the header's
fourth work vector under an updater and its update_fwd after the loop -- against the Python model on the same partition
to 1e-11 and against the stepper to 1e-9, the two bounds of test_gpu_partition_models.test_cxx_partition_leapfrog."""
import os
import subprocess

import numpy as np
import pytest

import leapfrog4_helpers as l4
import leapfrog_helpers as lh
import partition_helpers as ph
import test_gpu_comm as tc
from support import bits, comm, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, CFL, TOL, LIVE = 2, 0.5, 1e-9, 0.25
BOXES = {"yz": ((3, 3, 4), (False, True, True)), "xyz": ((3, 4, 3), (True, True, True))}
VARIANTS = {"box_split": (True, True), "box_unsplit": (True, False), "map_split": (False, True), "map_unsplit": (False, False)}
_SETUP, _REF = {}, {}


def setup(oracle, box):
    """(partition, oracle mesh with the periodic numbering, l2g, dt, u0 and v0 on the global numbering), built once"""
    if box not in _SETUP:
        n, periodic = BOXES[box]
        part, om, l2g = tc.periodic_setup(oracle, n, P, periodic, 0.0, hi=ph.HI)
        dt = oracle.cfl_time_step(om, P, ph.C0, ph.FREQ, CFL=CFL)[0]
        u0, v0, p0 = ph.initial_state(om.ndofs, dt, "random")
        assert p0 == 0.0 and l2g.size == part.V.ndofs and om.ndofs < l2g.size
        _SETUP[box] = (part, om, l2g, dt, u0, v0)
    return _SETUP[box]


def reference(oracle, box, scheme, segments=(ph.STEPS,)):
    """(u_n, v_n) of the numpy stepper on the global numbering, computed once and left unchanged"""
    key = (box, scheme, segments)
    if key not in _REF:
        part, om, l2g, dt, u0, v0 = setup(oracle, box)
        ref = oracle.LinearGLLOpt(om, P, ph.C0, ph.FREQ, 0.0)
        assert bool((ref.mG2 != 0.0).any()) == (box == "yz"), "absorbing faces on x alone; fully periodic: no boundary set"
        ref.init()
        ref.u_n[:] = u0
        ref.v_n[:] = v0
        ph.run_stepper(ref, scheme, dt, segments)
        u, v = ref.u_n.copy(), ref.v_n.copy()
        assert np.isfinite(u).all() and np.isfinite(v).all() and np.abs(u).max() <= 10.0, "the reference is bounded"
        for a in (u, v):
            a.setflags(write=False)
        _REF[key] = (u, v)
    return _REF[key]


def model(gpu, vu, part, l2g, u0, v0, structured, split):
    import torch
    from wave_fenics_amd.distributed import boundary_tags
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    eqn = LinearGLLOpt(part.V, P, ph.C0, ph.FREQ, 0.0, updater=vu, tags=boundary_tags(part), device=gpu, structured=structured,
                       tuning=None if structured else {"kernel": "march"})
    assert (eqn.stiff_op.kernel == "march_idx") == (not structured), eqn.stiff_op.kernel
    assert eqn._split, f"the overlap is not available (structured={structured})"
    eqn._split = split
    eqn.init()                                                   # the state is set after init()
    eqn.u_n.copy_(torch.from_numpy(ph.to_local(u0, l2g)))        # ghosts included: they start consistent
    eqn.v_n.copy_(torch.from_numpy(ph.to_local(v0, l2g)))
    return eqn


def check(label, eqn, part, om, l2g, uref, vref):
    """the three assertions of the module docstring on one finished run"""
    owned = part.owned_mask()
    got = {"u_n": eqn.u_n.cpu().numpy(), "v_n": eqn.v_n.cpu().numpy()}
    eu, ev = ph.relerr(got["u_n"], uref[l2g]), ph.relerr(got["v_n"], vref[l2g])
    b = bits(eqn.b.cpu().numpy())
    print(f"{label}: u {eu:.3e} v {ev:.3e}; {int(np.count_nonzero(b[~owned]))} of {int((~owned).sum())} ghost entries of b are not +0.0")
    assert eu <= TOL and ev <= TOL, (label, eu, ev)
    for name, x in got.items():
        rank = [{"l2g": l2g, "owned": owned, "x": x}]
        xg, count = ph.assemble_owned(om.ndofs, rank, "x")
        assert count.min() == 1 and count.max() == 1
        assert ph.ghost_mismatches(xg, rank, "x") == 0, f"{label}: ghost entries of {name} differ from their owner's bits"
    assert not b[owned].any(), f"{label}: b is left +0.0 on the owned entries"


@pytest.mark.parametrize("scheme", ["leapfrog4", "leapfrog"])
@pytest.mark.parametrize("box", list(BOXES))
def test_native_route_from_a_live_state(gpu, comm, oracle, box, scheme):
    from wave_fenics_amd.distributed import VectorUpdater
    part, om, l2g, dt, u0, v0 = setup(oracle, box)
    uref, vref = reference(oracle, box, scheme)
    owned = part.owned_mask()
    live = float(np.abs(uref[l2g[~owned]]).max() / np.abs(uref).max())
    assert (~owned).any() and live >= LIVE, f"the self-interfaces carry {live:.3f} of the global maximum"
    vu = VectorUpdater(part, device=gpu, comm=comm)
    try:
        assert vu.transport == "native" and vu.active
        for name, (structured, split) in VARIANTS.items():
            eqn = model(gpu, vu, part, l2g, u0, v0, structured, split)
            t, steps = getattr(eqn, scheme)(0.0, ph.STEPS * dt - 1e-13, dt)
            assert steps == ph.STEPS
            check(f"{scheme} native {box} {name}", eqn, part, om, l2g, uref, vref)
    finally:
        vu.close()


def test_native_route_restart(gpu, comm, oracle):
    """5 + 5 steps of leapfrog4 on the box path, split, the second call from the first's t: against the stepper split the
    same way (module docstring)"""
    from wave_fenics_amd.distributed import VectorUpdater
    box = "yz"
    part, om, l2g, dt, u0, v0 = setup(oracle, box)
    uref, vref = reference(oracle, box, "leapfrog4", (5, 5))
    uc, _ = reference(oracle, box, "leapfrog4", (10,))
    assert ph.relerr(uc, uref) >= 1e-6, "a split run differs from the continuous one by truncation: this is not that run"
    vu = VectorUpdater(part, device=gpu, comm=comm)
    try:
        assert vu.transport == "native" and vu.active
        eqn = model(gpu, vu, part, l2g, u0, v0, True, True)
        t, n1 = eqn.leapfrog4(0.0, 5 * dt - 1e-13, dt)
        t, n2 = eqn.leapfrog4(t, 1.0, dt, max_steps=5)
        assert (n1, n2) == (5, 5) and abs(t - 10 * dt) <= 1e-12 * t
        check(f"leapfrog4 native {box} restart 5 + 5", eqn, part, om, l2g, uref, vref)
    finally:
        vu.close()


def test_cxx_partition_leapfrog4(gpu, oracle, tmp_path):
    """planar3d --scheme leapfrog4 --periodic yz on one rank, P2, 6^3 cells, 20 steps at CFL 0.25 from rest (module
    docstring)"""
    from wave_fenics_amd.comm import Comm
    from wave_fenics_amd.distributed import VectorUpdater, boundary_tags, create_distributed_box
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    out = str(tmp_path / "bin")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), f"OUT={out}", os.path.join(out, "planar3d")])
    N, L, periodic = 6, 0.01, (False, True, True)
    om = oracle.create_box(N, P, hi=(L, L, L))
    l2g = oracle.make_periodic(om, periodic)
    dt, spp = oracle.cfl_time_step(om, P, ph.C0, ph.FREQ, CFL=0.25)
    ref = oracle.LinearGLLOpt(om, P, ph.C0, ph.FREQ, ph.P0)
    ref.init()
    t, steps = l4.leapfrog4(ref, *lh.oracle_parts(ref), 0.0, ph.STEPS * dt - 1e-13, dt)
    assert steps == ph.STEPS and np.abs(ref.u_n).max() > 0.0 and np.abs(ref.v_n).max() > 0.0
    part = create_distributed_box(N, P, 1, 0, hi=(L, L, L), periodic=periodic)
    comm = Comm.single()
    try:
        vu = VectorUpdater(part, device=gpu, comm=comm)
        assert vu.transport == "native" and vu.active
        eqn = LinearGLLOpt(part.V, P, ph.C0, ph.FREQ, ph.P0, updater=vu, tags=boundary_tags(part), device=gpu)
        assert eqn._split
        eqn.init()
        eqn.leapfrog4(0.0, ph.STEPS * dt - 1e-13, dt)
        py_u, py_v = eqn.u_n.cpu().numpy(), eqn.v_n.cpu().numpy()
        vu.close()
    finally:
        comm.close()
    env = dict(os.environ, WF_COMM_FILE=str(tmp_path / "comm_id"), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dump = str(tmp_path / "uv.bin")
    r = subprocess.run([os.path.join(out, "planar3d"), "--size", str(N), "--degree", str(P), "--cfl", "0.25", "--steps", str(ph.STEPS),
                        "--length", str(L), "--scheme", "leapfrog4", "--periodic", "yz", "--dump", dump],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"Number of step per period: {spp}" in r.stdout and f"Steps taken: {ph.STEPS}" in r.stdout
    assert f"Degrees of freedom: {om.ndofs}" in r.stdout
    uv = np.fromfile(dump, dtype=np.float64)
    n = part.V.ndofs
    assert uv.size == 2 * n and l2g.size == n
    for name, got, py, np_ in (("u", uv[:n], py_u, ref.u_n[l2g]), ("v", uv[n:], py_v, ref.v_n[l2g])):
        a, b = ph.relerr(got, py), ph.relerr(got, np_)
        print(f"planar3d --scheme leapfrog4 --periodic yz {name}: against the Python model {a:.3e}, against the stepper {b:.3e}")
        assert a <= 1e-11 and b <= 1e-9
