"""LinearGLLOpt.leapfrog / leapfrog4 / rk4 / rk4_fused on real partitions of 2 and 4 ranks and a periodic pair, from a state in which every plane where
ranks meet is live from the first step (partition_helpers; test_partition_scenario_host.py shows on the oracle that the
scenario can see an error made there), and the C++ model's leapfrog on a partition.

Mechanics of test_gpu_parity.py::test_distributed_on_one_gpu: spawned workers share cuda:0, gloo carries the halo, the HIP
pack / unpack kernels and operators run.  One spawn per case; every scheme and variant runs inside the workers, which
return their local vectors, and the parent compares with the single-domain oracle.

Bounds, none of them new: u_n and v_n to 1e-9 of their global maxima against the references over 20 steps (TOL of
test_gpu_leapfrog_model.py, the RK4 bound of test_distributed_on_one_gpu); 5 + 5 steps against 10 to 1e-11
(test_restart); one apply to 1e-12.  Exact: every ghost entry of u_n and v_n carries its owner's bits, and the owned
entries of all ranks cover every global dof once.  Leapfrog with the interior / interface overlap and without it sum the
cells of a dof in different orders, so nothing in the code says they agree bit for bit: the number of differing entries is
printed and each run is held to the reference.

Leapfrog4 (the same four variants as leapfrog, both scenarios, at the leapfrog step): two applies per step, the second on
the predictor's w, whose ghosts only its forward halo makes right; v_n is an operand of an apply in the start-up and in
the finish, which no other loop exchanges; the finish corrects v_n at ghost entries too, and the closing forward halo
restores the owner's bits.  Here ranks meet over gloo, so every halo is the model's _rhs as the loop's callback
(test_gpu_leapfrog4_partition.py drives the library's own exchange).  Rows of the parent:
  {scenario}/l4_*    u_n, v_n to 1e-9 against leapfrog4_helpers.leapfrog4 on the oracle; ghosts bit for bit their owner's
  restart/l4_parts   5 + 5 steps to 1e-9 against the stepper SPLIT 5 + 5 (a split run differs from the continuous one by
                     truncation, 5e-4 to 9e-2 here: the start-up is a Taylor series, not the inverse of the finish)
  stale/l4_*         v_n's ghost entries overwritten with -7 / (STEPS dt) before the run (u_n's stay consistent): to 1e-9
                     against the same reference, box and dofmap path; the entries that differ in bits from the run with
                     consistent ghosts are counted and printed
test_partition_scenario_host.py shows that the random state sees a halo of w or of v that is not made, and that from rest
the start-up's apply on v multiplies zeros."""
import os
import queue
import subprocess
import time

import numpy as np
import pytest

import partition_helpers as ph
from support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, TOL_RESTART, TOL_APPLY = 1e-9, 1e-11, 1e-12
CPUS = 16                                   # what a run is given; nothing here is sized by the machine's count
LEAPFROG = {"lf_box_split": (True, True), "lf_box_unsplit": (True, False), "lf_map_split": (False, True),
            "lf_map_unsplit": (False, False)}          # name: (structured, split)
LEAPFROG4 = {name.replace("lf_", "l4_"): variant for name, variant in LEAPFROG.items()}      # the same four, eqn.leapfrog4
STALE = {"l4_box": True, "l4_map": False}              # stale ghosts of v_n: name: structured (both split)
APPLY_SEED = 5


def _worker(rank, world, port, case, dts, q):
    try:
        import sys
        clock = [time.monotonic()]
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import torch
        torch.set_num_threads(max(1, CPUS // world))
        import torch.distributed as dist
        from dist_helpers import init_pg, local_to_global
        import partition_helpers as ph
        import wave_fenics_amd as w
        from wave_fenics_amd.distributed import VectorUpdater, boundary_tags, create_distributed_box
        from wave_fenics_amd.linear_gll import LinearGLLOpt
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        init_pg(rank, world, port, "gloo")      # ranks share cuda:0, the halo is staged through the host
        c = ph.CASES[case]
        p = c["p"]
        part = create_distributed_box(c["n"], p, world, rank, hi=ph.HI, build_dofmap=True, periodic=c["periodic"])
        assert tuple(part.procs) == c["procs"], part.procs
        vu = VectorUpdater(part, device=dev)
        l2g, owned = local_to_global(part), part.owned_mask()
        G = ph.global_lattice(case)
        nd = G[0] * G[1] * G[2]
        tags = boundary_tags(part)
        out = {"l2g": l2g, "owned": owned, "neighbours": len(set(vu.send_neighbors) | set(vu.recv_neighbors))}
        clock.append(time.monotonic())

        def model(structured, split, scenario, dt):
            part.V.structured = structured
            u0, v0, p0 = ph.initial_state(nd, dt, scenario)
            # (the dofmap path at these sizes: the marching kernel on request, the only dofmap kernel that splits)
            eqn = LinearGLLOpt(part.V, p, ph.C0, ph.FREQ, p0, updater=vu, tags=tags, device=dev,
                               tuning=None if structured else {"kernel": "march"})
            assert structured or eqn.stiff_op.kernel == "march_idx", eqn.stiff_op.kernel
            assert eqn._split, f"the overlap is not available (structured={structured})"
            eqn._split = split
            eqn.init()                                           # the state is set after init()
            eqn.u_n.copy_(torch.from_numpy(ph.to_local(u0, l2g)))    # ghosts included: they start consistent
            eqn.v_n.copy_(torch.from_numpy(ph.to_local(v0, l2g)))
            return eqn

        def state(eqn):
            return eqn.u_n.cpu().numpy(), eqn.v_n.cpu().numpy()

        for scenario in ph.SCENARIOS:
            dt = dts["leapfrog"]
            for name, (structured, split) in LEAPFROG.items():
                eqn = model(structured, split, scenario, dt)
                t, steps = eqn.leapfrog(0.0, ph.STEPS * dt - 1e-13, dt)
                assert steps == ph.STEPS
                out[f"{scenario}/{name}"] = state(eqn)
            for name, (structured, split) in LEAPFROG4.items():
                eqn = model(structured, split, scenario, dt)
                t, steps = eqn.leapfrog4(0.0, ph.STEPS * dt - 1e-13, dt)
                assert steps == ph.STEPS
                out[f"{scenario}/{name}"] = state(eqn)
            dt = dts["rk4"]
            for name in ("rk4", "rk4_fused"):
                eqn = model(True, True, scenario, dt)
                t, steps = getattr(eqn, name)(0.0, ph.STEPS * dt - 1e-13, dt)
                assert steps == ph.STEPS
                out[f"{scenario}/{name}"] = state(eqn)
        # 5 + 5 steps against 10, both on the partition
        dt = dts["leapfrog"]
        whole, parts = model(True, True, "random", dt), model(True, True, "random", dt)
        whole.leapfrog(0.0, 10 * dt - 1e-13, dt)
        t, n1 = parts.leapfrog(0.0, 5 * dt - 1e-13, dt)
        t, n2 = parts.leapfrog(t, 1.0, dt, max_steps=5)
        assert (n1, n2) == (5, 5)
        out["restart/whole"], out["restart/parts"] = state(whole), state(parts)
        # leapfrog4: 5 + 5 steps, the second call from the first's t (the parent holds it to the stepper split likewise)
        parts = model(True, True, "random", dt)
        t, n1 = parts.leapfrog4(0.0, 5 * dt - 1e-13, dt)
        t, n2 = parts.leapfrog4(t, 1.0, dt, max_steps=5)
        assert (n1, n2) == (5, 5)
        out["restart/l4_parts"] = state(parts)
        # leapfrog4 from a v_n whose ghost entries are wrong (finite, of the size of v0); u_n's stay consistent
        ghost = torch.from_numpy(~owned).to(dev)      # (the lowest rank owns all it shares: the parent asserts that some rank has ghosts)
        for name, structured in STALE.items():
            eqn = model(structured, True, "random", dt)
            eqn.v_n[ghost] = -7.0 / (ph.STEPS * dt)
            t, steps = eqn.leapfrog4(0.0, ph.STEPS * dt - 1e-13, dt)
            assert steps == ph.STEPS
            out[f"stale/{name}"] = state(eqn)
        if c["procs"][2] > 1:
            # one apply across a z interface between different ranks, both paths
            xg = np.random.default_rng(APPLY_SEED).uniform(-1, 1, nd)
            for structured in (True, False):
                part.V.structured = structured
                K = w.StiffnessOperator(part.V, p, {"c0": ph.C0})
                x = torch.from_numpy(np.where(owned, xg[l2g], 0.0)).to(dev)
                y = torch.zeros_like(x)
                vu.update_fwd(x)
                K(x, y)
                vu.update_rev(y)
                out[f"apply/K{int(structured)}"] = y.cpu().numpy()
        part.V.structured = True
        dist.barrier()
        clock.append(time.monotonic())
        out["seconds"] = (clock[1] - clock[0], clock[2] - clock[1])      # start-up (imports, process group, partition), runs
        dist.destroy_process_group()
        q.put((rank, out, None))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, None, traceback.format_exc()))


def run_workers(case, dts, timeout=300.0):
    """one spawn of the case's ranks; their results by rank.  A worker that reports a traceback, dies or does not answer
    in time ends the test: the others are terminated and nothing else is started."""
    import torch.multiprocessing as mp
    from dist_helpers import free_port
    world = ph.CASES[case]["world"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, dts, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res, problem, end = {}, None, time.monotonic() + timeout
    while len(res) < world and problem is None:
        try:
            rank, out, tb = q.get(timeout=2.0)
        except queue.Empty:
            dead = [(r, pr.exitcode) for r, pr in enumerate(procs) if r not in res and pr.exitcode not in (None, 0)]
            if dead:
                problem = f"workers died without an answer (rank, exit code): {dead}"
            elif time.monotonic() > end:
                problem = f"no answer from ranks {sorted(set(range(world)) - set(res))} within {timeout:.0f} s"
            continue
        if tb is not None:
            problem = f"rank {rank} failed:\n{tb}"
        else:
            res[rank] = out
    if problem is not None:
        for pr in procs:
            if pr.is_alive():
                pr.terminate()
        for pr in procs:
            pr.join(timeout=30)
        pytest.fail(f"{case}: {problem}")
    for pr in procs:
        pr.join(timeout=60)
    return [res[r] for r in range(world)]


# The 8-rank case (2 x 2 x 2, the only one with a z interface between different ranks) is NOT run here.  Alone it passed
# in 4.2 s at errors of 1e-15 (profiles/r26_summary.md); inside the whole suite, where the pytest process itself holds GPU
# queues by then, the same run took 272 s, and after test_gpu_comm.py alone no worker had answered after 300 s.  Eight
# workers and the parent are nine processes with queues on one GPU, one more than the eight the hardware scheduler runs
# side by side, after which it time-slices them -- the likely cause, not verified by a second run.  The worker keeps its
# z branch (one apply across the z interface) for the day the case can run with at most eight processes.
GPU_CASES = [name for name, c in ph.CASES.items() if c["world"] < 8]


@pytest.mark.parametrize("case", GPU_CASES)
def test_models_on_partitions(gpu, oracle, case):
    c = ph.CASES[case]
    om = ph.global_mesh(oracle, case)
    dts = {s: ph.time_step(oracle, case, s) for s in ("leapfrog", "rk4", "leapfrog4")}
    assert dts["leapfrog4"] == dts["leapfrog"], "the workers run both at the leapfrog step"
    t0 = time.monotonic()
    ranks = run_workers(case, dts)
    wall = time.monotonic() - t0
    print(f"{case}: {c['world']} workers answered after {wall:.1f} s (slowest start-up {max(r['seconds'][0] for r in ranks):.1f} s, "
          f"slowest runs {max(r['seconds'][1] for r in ranks):.1f} s); neighbours per rank {[r['neighbours'] for r in ranks]}")
    # the owned entries of all ranks cover every global dof exactly once
    for r in ranks:
        assert r["l2g"].min() >= 0 and r["l2g"].max() < om.ndofs and r["owned"].shape == r["l2g"].shape
    _, count = ph.assemble_owned(om.ndofs, [dict(r, x=np.zeros(r["l2g"].size)) for r in ranks], "x")
    assert count.min() == 1 and count.max() == 1, f"global dofs owned {count.min()} to {count.max()} times"
    assert any((~r["owned"]).any() for r in ranks)

    failures = []

    def glob(key):
        """(u, v) on the global numbering from the owned entries, after the ghost check"""
        got = []
        for i, name in enumerate(("u_n", "v_n")):
            per_rank = [dict(r, x=r[key][i]) for r in ranks]
            xg, _ = ph.assemble_owned(om.ndofs, per_rank, "x")
            bad = ph.ghost_mismatches(xg, per_rank, "x")
            if bad:
                failures.append(f"{key}: {bad} ghost entries of {name} differ from their owner's bits")
            got.append(xg)
        return got

    results = {}
    for scenario in ph.SCENARIOS:
        for variant in (*LEAPFROG, *LEAPFROG4, "rk4", "rk4_fused"):
            scheme = "leapfrog" if variant in LEAPFROG else "leapfrog4" if variant in LEAPFROG4 else "rk4"
            dt, uref, vref = ph.reference(oracle, case, scheme, scenario)
            assert dt == dts[scheme]
            if scenario == "rest" and not any(c["periodic"]):
                assert np.abs(uref).max() > 0.0 and np.abs(vref).max() > 0.0
            key = f"{scenario}/{variant}"
            u, v = results[key] = glob(key)
            eu, ev = ph.relerr(u, uref), ph.relerr(v, vref)
            print(f"{case} {key}: u {eu:.3e} v {ev:.3e}")
            if not (eu <= TOL and ev <= TOL):
                failures.append(f"{key}: u {eu:.3e} v {ev:.3e} against the oracle, bound {TOL:.0e}")
        for a, b in (("lf_box_split", "lf_box_unsplit"), ("lf_map_split", "lf_map_unsplit"),
                     ("l4_box_split", "l4_box_unsplit"), ("l4_map_split", "l4_map_unsplit")):
            du, dv = (ph.differing_entries(x, y) for x, y in zip(results[f"{scenario}/{a}"], results[f"{scenario}/{b}"]))
            print(f"{case} {scenario}: {a} against {b}: {du} of {om.ndofs} entries of u_n and {dv} of v_n differ in their bits")
    (uw, vw), (up, vp) = glob("restart/whole"), glob("restart/parts")
    du, dv = ph.relerr(up, uw), ph.relerr(vp, vw)
    print(f"{case} restart 5 + 5 against 10: u {du:.3e} v {dv:.3e}")
    if not (du <= TOL_RESTART and dv <= TOL_RESTART):
        failures.append(f"restart: u {du:.3e} v {dv:.3e}, bound {TOL_RESTART:.0e}")
    # leapfrog4, 5 + 5: against the numpy stepper split the same way, to TOL -- not to TOL_RESTART against a 10-step run: its
    # start-up is a Taylor series, not the inverse of its finish, so a split run differs from the continuous one by
    # truncation (5e-4 to 9e-2 here on the oracle), which no bound on rounding can hold
    _, uref, vref = ph.reference(oracle, case, "leapfrog4", "random", steps=(5, 5))
    up, vp = glob("restart/l4_parts")
    du, dv = ph.relerr(up, uref), ph.relerr(vp, vref)
    print(f"{case} leapfrog4 restart 5 + 5 against the stepper split 5 + 5: u {du:.3e} v {dv:.3e}")
    if not (du <= TOL and dv <= TOL):
        failures.append(f"restart/l4_parts: u {du:.3e} v {dv:.3e} against the split stepper, bound {TOL:.0e}")
    # leapfrog4 from stale ghosts of v_n: the loop exchanges v before its start-up apply reads a ghost of it, so the run
    # is held to the same reference as the run from consistent ghosts
    _, uref, vref = ph.reference(oracle, case, "leapfrog4", "random")
    for name, structured in STALE.items():
        us, vs = glob(f"stale/{name}")
        du, dv = ph.relerr(us, uref), ph.relerr(vs, vref)
        uc, vc = results[f"random/{name}_split"]
        print(f"{case} leapfrog4 from stale ghosts of v_n, {name}: u {du:.3e} v {dv:.3e}; {ph.differing_entries(us, uc)} of {om.ndofs} "
              f"entries of u_n and {ph.differing_entries(vs, vc)} of v_n differ in their bits from the run with consistent ghosts")
        if not (du <= TOL and dv <= TOL):
            failures.append(f"stale/{name}: u {du:.3e} v {dv:.3e} against the oracle, bound {TOL:.0e}: a ghost of v_n is read "
                            "before it is exchanged")
    if c["procs"][2] > 1:
        xg = np.random.default_rng(APPLY_SEED).uniform(-1, 1, om.ndofs)
        yref = np.zeros(om.ndofs)
        oracle.StiffnessOperator(om, c["p"])(xg, yref)
        for key in ("apply/K1", "apply/K0"):
            y, _ = ph.assemble_owned(om.ndofs, [dict(r, x=r[key]) for r in ranks], "x")
            e = ph.relerr(y, yref)
            print(f"{case} {key}: {e:.3e}")
            if not e <= TOL_APPLY:
                failures.append(f"{key}: {e:.3e}, bound {TOL_APPLY:.0e}")
    assert not failures, "\n".join(failures)


def test_cxx_partition_leapfrog(gpu, oracle, tmp_path):
    """planar3d --scheme leapfrog --periodic yz on one rank: the header's leapfrog with its updater and the overlap, and
    the partition branch of the example.  P2, 6^3 cells, 20 steps at CFL 0.25 from rest: a plane wave with periodic y
    and z crosses every self-interface.  Against the numpy stepper on the oracle's periodic mesh to 1e-9 and against the
    Python model on the same partition (native exchange) to 1e-11 -- the two bounds of test_cxx_demo."""
    import leapfrog_helpers as lh
    from wave_fenics_amd.comm import Comm
    from wave_fenics_amd.distributed import VectorUpdater, boundary_tags, create_distributed_box
    from wave_fenics_amd.linear_gll import LinearGLLOpt
    out = str(tmp_path / "bin")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), f"OUT={out}", os.path.join(out, "planar3d")])
    p, N, L, periodic = 2, 6, 0.01, (False, True, True)
    om = oracle.create_box(N, p, hi=(L, L, L))
    l2g = oracle.make_periodic(om, periodic)
    dt, spp = oracle.cfl_time_step(om, p, ph.C0, ph.FREQ, CFL=0.25)
    ref = oracle.LinearGLLOpt(om, p, ph.C0, ph.FREQ, ph.P0)
    ref.init()
    t, steps = lh.leapfrog(ref, *lh.oracle_parts(ref), 0.0, ph.STEPS * dt - 1e-13, dt)
    assert steps == ph.STEPS and np.abs(ref.u_n).max() > 0.0 and np.abs(ref.v_n).max() > 0.0
    part = create_distributed_box(N, p, 1, 0, hi=(L, L, L), periodic=periodic)
    comm = Comm.single()
    try:
        vu = VectorUpdater(part, device=gpu, comm=comm)
        assert vu.transport == "native" and vu.active
        eqn = LinearGLLOpt(part.V, p, ph.C0, ph.FREQ, ph.P0, updater=vu, tags=boundary_tags(part), device=gpu)
        assert eqn._split
        eqn.init()
        eqn.leapfrog(0.0, ph.STEPS * dt - 1e-13, dt)
        py_u, py_v = eqn.u_n.cpu().numpy(), eqn.v_n.cpu().numpy()
        vu.close()
    finally:
        comm.close()
    env = dict(os.environ, WF_COMM_FILE=str(tmp_path / "comm_id"), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dump = str(tmp_path / "uv.bin")
    r = subprocess.run([os.path.join(out, "planar3d"), "--size", str(N), "--degree", str(p), "--cfl", "0.25", "--steps", str(ph.STEPS),
                        "--length", str(L), "--scheme", "leapfrog", "--periodic", "yz", "--dump", dump],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"Number of step per period: {spp}" in r.stdout and f"Steps taken: {ph.STEPS}" in r.stdout
    assert f"Degrees of freedom: {om.ndofs}" in r.stdout
    uv = np.fromfile(dump, dtype=np.float64)
    n = part.V.ndofs
    assert uv.size == 2 * n and l2g.size == n
    for name, got, py, np_ in (("u", uv[:n], py_u, ref.u_n[l2g]), ("v", uv[n:], py_v, ref.v_n[l2g])):
        a, b = ph.relerr(got, py), ph.relerr(got, np_)
        print(f"planar3d --scheme leapfrog --periodic yz {name}: against the Python model {a:.3e}, against the stepper {b:.3e}")
        assert a <= 1e-11 and b <= 1e-9
