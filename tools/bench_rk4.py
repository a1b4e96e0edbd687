#!/usr/bin/env python3
"""Secondary benchmark (not the driver's line): the full RK4 loop of
BASELINE.json configs[3] -- P4 box, 54^3 cells per GPU, domain-decomposed, RCCL
ghost exchange, LinearGLLOpt.rk4_fused -- launched like bench.py:

  python tools/bench_rk4.py [--steps K] [--size N]                      (1 GPU)
  python -m torch.distributed.run --nproc-per-node N tools/bench_rk4.py (N GPUs)

Prints one JSON line: ms per RK4 time step and dof-stages/s over all ranks.
--scheme leapfrog times LinearGLLOpt.leapfrog at the same step instead (the same keys, per leapfrog step; the timed
window includes the scheme's start-up and finish, two extra stiffness applies).
--scheme leapfrog4 times LinearGLLOpt.leapfrog4 likewise (two applies per step; start-up and finish are six more).
--compare (one rank): leapfrog, leapfrog4 and rk4_fused on one model, timed alternately --rounds times with device events
after a warm-up of each, at each scheme's own step -- stable_time_step(0.9) of leapfrog, sqrt(3) times it for leapfrog4,
sqrt(2) times it for RK4 (its limit on the imaginary axis is sqrt(8) / sqrt(lambda_max)) -- and at the common CFL step;
prints ms per step and ms per microsecond of simulated time for each.
--receivers N / --sources S (one rank): the same loop with N point receivers recorded every step and S Ricker point
sources, against the loop without them -- two models in one process, timed alternately --rounds times after one warm-up
each; prints medians and ranges of both and the difference per step.
--scheme leapfrog --gradient (one rank): LinearGLLOpt.misfit_gradient against LinearGLLOpt.leapfrog on one model with
--receivers (default 1000) receivers and --sources (default 1) source, --steps (default 200) steps each, timed alternately
--rounds times with device events after a warm-up of both; prints ms per step of both, their ratio and the time per
backward step (the difference).  The split of a backward step by kernel comes from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/bench_rk4.py --scheme leapfrog --gradient --rounds 1`.
--scheme leapfrog4 --gradient (one rank): misfit_gradient(scheme="leapfrog4") against leapfrog4 and against the leapfrog
gradient of the line above, the three alternately in one process, each scheme at its own stable_time_step(0.9); prints ms
per step of the three, ms per microsecond of simulated time of the two gradients and their ratio."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 100; 200 with --gradient)")
    ap.add_argument("--warmup", type=int, default=150, help="untimed steps; long enough to pass the power ramp after idle (profiles/r03_power_ramp.md)")
    ap.add_argument("--size", type=int, default=54)
    ap.add_argument("--degree", type=int, default=4)
    ap.add_argument("--unfused", action="store_true")
    ap.add_argument("--scheme", choices=["rk4", "leapfrog", "leapfrog4"], default="rk4",
                    help="leapfrog / leapfrog4: LinearGLLOpt.leapfrog / leapfrog4 at the same step (one / two stiffness applies per step; "
                         "ms_per_rk4_step is then ms per step of that scheme)")
    ap.add_argument("--compare", action="store_true", help="leapfrog, leapfrog4 and rk4_fused alternately, at their own steps and a common one")
    ap.add_argument("--receivers", type=int, default=0, help="point receivers recorded every step (A/B against the plain loop)")
    ap.add_argument("--sources", type=int, default=0, help="Ricker point sources (A/B against the plain loop)")
    ap.add_argument("--gradient", action="store_true", help="with --scheme leapfrog / leapfrog4: time misfit_gradient against the loop")
    ap.add_argument("--checkpoint-every", type=int, default=None, help="--gradient: steps between checkpoints (default ceil(sqrt(steps)))")
    ap.add_argument("--rounds", type=int, default=5, help="alternating timed runs per variant of the A/B")
    ap.add_argument("--periodic", default="", help="axes identified with their opposite face (one rank: RCCL exchange with itself)")
    args = ap.parse_args()
    if args.gradient and args.scheme not in ("leapfrog", "leapfrog4"):
        sys.exit("--gradient needs --scheme leapfrog or leapfrog4")
    if args.steps is None:
        args.steps = 200 if args.gradient else 100
    if args.gradient:
        args.receivers, args.sources = args.receivers or 1000, args.sources or 1
    import torch
    import torch.distributed as dist
    import wave_fenics_amd as w
    from wave_fenics_amd.distributed import VectorUpdater, boundary_tags, create_distributed_box
    from wave_fenics_amd.linear_gll import LinearGLLOpt, cfl_time_step

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("WF_BENCH_BACKEND", "nccl")
    dev_index = local_rank if backend == "nccl" else local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    p, n = args.degree, args.size
    L = 0.1
    periodic = tuple(c in args.periodic for c in "xyz")
    part = create_distributed_box(n, p, world, rank, hi=(L, L, L), periodic=periodic)
    updater = VectorUpdater(part, device=dev) if (world > 1 or any(periodic)) else None
    eqn = LinearGLLOpt(part.V, p, 1500.0, 0.5e6, 6e4, updater=updater, tags=boundary_tags(part), device=dev)
    dt, _ = cfl_time_step(part.mesh, p, 1500.0, 0.5e6, CFL=0.25)
    eqn.init()
    run = {"leapfrog": eqn.leapfrog, "leapfrog4": eqn.leapfrog4}.get(args.scheme, eqn.rk4 if args.unfused else eqn.rk4_fused)
    applies = {"leapfrog": 1.0, "leapfrog4": 2.0}.get(args.scheme, 4.0)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if args.compare:
        if updater is not None:
            sys.exit("--compare runs on one rank without --periodic")
        compare(args, eqn, dt, part.size_global)
        return
    if args.receivers or args.sources:
        if updater is not None:
            sys.exit("--receivers / --sources run on one rank without --periodic")
        import statistics

        import numpy as np
        from wave_fenics_amd import points
        V = w.create_functionspace(part.mesh, p)      # with its dofmap, which the point location reads
        rng = np.random.default_rng(0)
        rec = points.Receivers(V, rng.uniform(0.05 * L, 0.95 * L, size=(args.receivers, 3)), device=dev) if args.receivers else None
        src = points.Sources(V, rng.uniform(0.3 * L, 0.7 * L, size=(args.sources, 3)),
                             [points.ricker(0.5e6, 3.0e-6, 1.0e9)] * args.sources) if args.sources else None
        with_points = LinearGLLOpt(V, p, 1500.0, 0.5e6, 6e4, tags=boundary_tags(part), device=dev, sources=src, receivers=rec)
        with_points.init()
        if args.gradient:
            (gradient4_ab if args.scheme == "leapfrog4" else gradient_ab)(args, with_points, rec, dt, part.size_global)
            return
        models = {"plain": eqn, "points": with_points}
        name = args.scheme if args.scheme != "rk4" else "rk4" if args.unfused else "rk4_fused"
        times = {k: [] for k in models}
        t_at = {k: 0.0 for k in models}
        for rnd in range(args.rounds + 1):            # round 0 is the warm-up of both
            steps = args.warmup if rnd == 0 else args.steps
            for k, model in models.items():
                if rec is not None:
                    rec.reset()
                sync()
                t0 = time.perf_counter()
                t_at[k], done = getattr(model, name)(t_at[k], 1.0e9, dt, max_steps=steps)
                sync()
                if rnd:
                    times[k].append((time.perf_counter() - t0) / done * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps({"metric": f"{name} step with and without point sources / receivers, ms per step", "scheme": args.scheme,
                          "receivers": args.receivers, "sources": args.sources, "rounds": args.rounds, "steps": args.steps,
                          "global_dofs": part.size_global,
                          "plain_ms": {"median": med["plain"], "min": min(times["plain"]), "max": max(times["plain"])},
                          "points_ms": {"median": med["points"], "min": min(times["points"]), "max": max(times["points"])},
                          "difference_us_per_step": (med["points"] - med["plain"]) * 1e3,
                          "unique_source_dofs": src.num_unique_dofs if src is not None else 0,
                          "finite": bool(torch.isfinite(with_points.u_n).all() and torch.isfinite(eqn.u_n).all())}), flush=True)
        return

    run(0.0, args.warmup * dt - 1e-13, dt)
    sync()
    t0 = time.perf_counter()
    run(args.warmup * dt, (args.warmup + args.steps) * dt - 1e-13, dt)
    sync()
    el = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([el], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        el = float(tt.item())
    ok = bool(torch.isfinite(eqn.u_n).all())
    if rank == 0:
        print(json.dumps({"metric": "RK4 time step, P4 hex box, full loop (4 x [ghost fwd, K, boundary, ghost rev, vector algebra])",
                          "ms_per_rk4_step": el / args.steps * 1e3, "dof_stages_per_s": applies * part.size_global * args.steps / el, "scheme": args.scheme,
                          "n_gpus": world, "global_dofs": part.size_global, "cells_per_gpu": part.mesh.ncells,
                          "fused": not args.unfused, "periodic": args.periodic,
                          "exchange": updater.transport if updater is not None else None, "finite": ok, "scaling": "weak"}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def compare(args, eqn, dt_cfl, global_dofs):
    """the three loops on one model, alternately, each run timed by a pair of device events; the timed window includes
    each scheme's start-up and finish (leapfrog two applies, leapfrog4 six)"""
    import math
    import statistics

    import torch
    steps = args.steps
    dt_lf = eqn.stable_time_step(0.9)
    own = {"leapfrog": dt_lf, "leapfrog4": eqn.stable_time_step(0.9, scheme="leapfrog4"), "rk4_fused": dt_lf * math.sqrt(2.0)}
    out = {"metric": "leapfrog, leapfrog4 and rk4_fused, ms per step (device events)", "steps": steps, "rounds": args.rounds,
           "global_dofs": global_dofs, "dt_common": dt_cfl, "dt_own": own}

    def timed(name, dt, n):
        eqn.init()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        getattr(eqn, name)(0.0, 1.0e9, dt, max_steps=n)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    for label, dts in (("own", own), ("common", {k: dt_cfl for k in own})):
        for name in own:
            timed(name, dts[name], args.warmup)
        times = {k: [] for k in own}
        for _ in range(args.rounds):
            for name in own:
                times[name].append(timed(name, dts[name], steps))
        finite = {}
        for name in own:                                       # after a timed run of each: did it stay bounded at this step
            timed(name, dts[name], steps)
            finite[name] = bool(torch.isfinite(eqn.u_n).all())
        out[label] = {k: {"ms_per_step": statistics.median(v), "min": min(v), "max": max(v),
                          "ms_per_simulated_us": statistics.median(v) / (dts[k] * 1e6), "finite": finite[k]} for k, v in times.items()}
    print(json.dumps(out), flush=True)


def gradient_ab(args, eqn, rec, dt, global_dofs):
    """misfit_gradient against leapfrog on one model, alternately, each run timed by a pair of device events"""
    import statistics

    import torch
    steps = args.steps

    def timed(fn):
        rec.reset()
        eqn.init()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps, out

    forward = lambda: eqn.leapfrog(0.0, 1.0e9, dt, max_steps=steps)    # noqa: E731
    eqn.leapfrog(0.0, 1.0e9, dt, max_steps=args.warmup)
    timed(forward)
    observed = 0.9 * rec.traces.clone()                                # a misfit that is not zero
    gradient = lambda: eqn.misfit_gradient(0.0, 1.0e9, dt, observed, checkpoint_every=args.checkpoint_every, max_steps=steps)    # noqa: E731
    timed(gradient)
    times = {"leapfrog": [], "gradient": []}
    for _ in range(args.rounds):
        times["leapfrog"].append(timed(forward)[0])
        ms, (J, gK, gM, info) = timed(gradient)
        times["gradient"].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    stat = lambda v, m: {"median": m, "min": min(v), "max": max(v)}    # noqa: E731
    print(json.dumps({"metric": "misfit_gradient against leapfrog, ms per step (device events)", "steps": steps, "rounds": args.rounds,
                      "receivers": args.receivers, "sources": args.sources, "global_dofs": global_dofs,
                      "leapfrog_ms": stat(times["leapfrog"], med["leapfrog"]), "gradient_ms": stat(times["gradient"], med["gradient"]),
                      "gradient_over_leapfrog": med["gradient"] / med["leapfrog"],
                      "backward_step_ms": med["gradient"] - med["leapfrog"],
                      "S": info["S"], "vectors": info["vectors"], "bytes": info["bytes"], "launches": info["launches"], "J": J,
                      "finite": bool(torch.isfinite(gK).all() and torch.isfinite(gM).all())}), flush=True)


def gradient4_ab(args, eqn, rec, dt, global_dofs):
    """misfit_gradient(scheme="leapfrog4") against leapfrog4 and against the leapfrog gradient on one model, alternately,
    each scheme at its own stable step, each run timed by a pair of device events"""
    import statistics

    import torch
    steps = args.steps
    dts = {"leapfrog": eqn.stable_time_step(0.9), "leapfrog4": eqn.stable_time_step(0.9, scheme="leapfrog4")}

    def timed(fn):
        rec.reset()
        eqn.init()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps, out

    eqn.leapfrog4(0.0, 1.0e9, dts["leapfrog4"], max_steps=args.warmup)
    observed = {}
    for scheme, loop in (("leapfrog", eqn.leapfrog), ("leapfrog4", eqn.leapfrog4)):
        timed(lambda: loop(0.0, 1.0e9, dts[scheme], max_steps=steps))
        observed[scheme] = 0.9 * rec.traces.clone()                    # a misfit that is not zero
    runs = {"leapfrog4": lambda: eqn.leapfrog4(0.0, 1.0e9, dts["leapfrog4"], max_steps=steps)}
    for scheme in ("leapfrog4", "leapfrog"):
        runs["gradient_" + scheme] = lambda scheme=scheme: eqn.misfit_gradient(
            0.0, 1.0e9, dts[scheme], observed[scheme], checkpoint_every=args.checkpoint_every, max_steps=steps, scheme=scheme)
    times, last = {k: [] for k in runs}, {}
    for rnd in range(args.rounds + 1):                                 # round 0 is the warm-up of all three
        for k, fn in runs.items():
            ms, last[k] = timed(fn)
            if rnd:
                times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    stat = lambda k: {"median": med[k], "min": min(times[k]), "max": max(times[k])}    # noqa: E731
    per_us = {k: med["gradient_" + k] / (dts[k] * 1e6) for k in dts}
    J, gK, gM, info = last["gradient_leapfrog4"]
    print(json.dumps({"metric": "misfit_gradient(leapfrog4) against leapfrog4 and misfit_gradient(leapfrog), ms per step (device events)",
                      "steps": steps, "rounds": args.rounds, "receivers": args.receivers, "sources": args.sources,
                      "global_dofs": global_dofs, "dt": dts, "leapfrog4_ms": stat("leapfrog4"),
                      "gradient_leapfrog4_ms": stat("gradient_leapfrog4"), "gradient_leapfrog_ms": stat("gradient_leapfrog"),
                      "gradient_over_leapfrog4": med["gradient_leapfrog4"] / med["leapfrog4"],
                      "backward_step_ms": med["gradient_leapfrog4"] - med["leapfrog4"],
                      "gradient_ms_per_simulated_us": per_us,
                      "leapfrog4_over_leapfrog_per_simulated_time": per_us["leapfrog4"] / per_us["leapfrog"],
                      "S": info["S"], "vectors": info["vectors"], "bytes": info["bytes"], "launches": info["launches"], "J": J,
                      "finite": bool(torch.isfinite(gK).all() and torch.isfinite(gM).all()
                                     and torch.isfinite(last["gradient_leapfrog"][1]).all())}), flush=True)


if __name__ == "__main__":
    main()
