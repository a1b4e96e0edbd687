"""Can the partitioned model tests see an error made where ranks meet?  On the oracle alone, no GPU.

Why the random-state scenario of partition_helpers exists: from rest, with the source on x = 0, 20 steps at CFL 0.25
hardly reach the planes where the ranks of test_gpu_parity.py::test_distributed_on_one_gpu meet.  Largest |u| on the
interface plane relative to the global maximum, measured on the oracle with that test's meshes:

  case                         scheme     x interface   y interface
  world 2, P2, global 6x4x4    RK4        2.9e-3        -
  world 2, P2, global 6x4x4    leapfrog   2.8e-3        -
  world 4, P4, global 6x6x4    RK4        2.4e-7        0.92
  world 4, P4, global 6x6x4    leapfrog   2.7e-7        0.92

Against a bound of 1e-9 of the global maximum, a relative error of 4e-3 in everything the model does on the x interface
of the world-4 case passes (test_from_rest_hardly_reaches_the_x_interface recomputes the figures).

For every case of test_gpu_partition_models.py and both schemes, from the random state, two conditions (conditions,
not tolerances -- they keep the GPU test from being blind):

* the interfaces are live: after STEPS steps max |u| on EVERY interface plane is >= 0.25 of the global maximum
  (measured with seed 11: 0.51 to 1.0 for leapfrog);
* a mutant is visible: the same run with the absorbing facet mass mG2 halved on the interface planes -- masses not
  assembled across ranks -- moves u_n by >= 1e-3 of its maximum (measured: 0.09 to 0.18 for leapfrog), eight orders
  of magnitude above the GPU test's bound of 1e-9.

The fourth-order leapfrog is held to both conditions as well (measured: 0.67 to 1.0; 0.07 to 0.19), and has halos of its
own -- of w, the operand of each step's second apply, and of v, an operand of its start-up and finish
(test_leapfrog4_halo_mutants_are_visible).  Measured on the four cases, as the larger of the moves of u_n and v_n: the
second apply's operand zeroed on the interface planes 0.11 to 1.2; the start-up's K v0 operand zeroed there 2.3e-3 to
8.2e-3 (and exactly nothing from rest); every apply perturbed by one rounding 2.0e-15 to 5.1e-15."""
import numpy as np
import pytest

import partition_helpers as ph

LIVE, VISIBLE = 0.25, 1e-3
MUTANT_VISIBLE, ROUNDING = 1e-4, 1e-11     # leapfrog4: 1e5 times the GPU bound of 1e-9, and a hundredth of it


def plane_ratios(case, u):
    top = np.abs(u).max()
    return {name: float(np.abs(u[mask]).max() / top) for name, mask in ph.interface_planes(case).items()}


@pytest.mark.parametrize("scheme", ["leapfrog", "rk4", "leapfrog4"])
@pytest.mark.parametrize("case", list(ph.CASES))
def test_interfaces_are_live_and_a_mutant_is_visible(oracle, case, scheme):
    dt, u, v = ph.reference(oracle, case, scheme, "random")
    assert np.isfinite(u).all() and np.isfinite(v).all()
    ratios = plane_ratios(case, u)
    on_planes = np.logical_or.reduce(list(ph.interface_planes(case).values()))
    _, um, _ = ph.reference(oracle, case, scheme, "random", halve_mG2=on_planes)
    moved = ph.relerr(um, u)
    print(f"{case} {scheme}: max |u| {np.abs(u).max():.3f}, interface / global maximum "
          + ", ".join(f"{k}: {r:.3f}" for k, r in ratios.items()) + f"; mutant moves u_n by {moved:.3e}")
    assert min(ratios.values()) >= LIVE, ratios
    assert moved >= VISIBLE


@pytest.mark.parametrize("case", list(ph.CASES))
def test_leapfrog4_halo_mutants_are_visible(oracle, case):
    """The fourth-order leapfrog exchanges more than the other loops: the operand w of every step's second apply, and v,
    an operand of the start-up's K v0 and the finish's K vt.  From the random state each of three mutants -- the
    absorbing facet mass halved on the interface planes, the operand of every second apply zeroed there, the operand
    of the start-up's K v0 zeroed there (partition_helpers) -- moves u_n or v_n by at least MUTANT_VISIBLE of its maximum,
    1e5 times the GPU test's bound of 1e-9; and the unmutated stepper with every apply's result perturbed by one rounding
    moves them by at most ROUNDING, a hundredth of that bound (measured: 1.8e-15), so the bound has the headroom.

    From REST the start-up's K v0 multiplies zeros: zeroing its operand on the interface planes changes the result by
    exactly nothing, bit for bit (asserted on the non-periodic cases, the ones with a source).  A run from rest cannot
    see a forward halo of v that is not made: the reason the GPU runs of leapfrog4 use the random state."""
    dt, u, v = ph.reference(oracle, case, "leapfrog4", "random")
    assert np.isfinite(u).all() and np.isfinite(v).all()
    on_planes = np.logical_or.reduce(list(ph.interface_planes(case).values()))
    moved = {}
    for name, kw in (("halve_mG2", dict(halve_mG2=on_planes)), ("second_apply", dict(mutant="second_apply")),
                     ("startup_v", dict(mutant="startup_v")), ("rounding", dict(mutant="rounding"))):
        dtm, um, vm = ph.reference(oracle, case, "leapfrog4", "random", **kw)
        assert dtm == dt
        moved[name] = (ph.relerr(um, u), ph.relerr(vm, v))
    print(f"{case} leapfrog4, random state: max |u| {np.abs(u).max():.3f}; moved (u, v): "
          + ", ".join(f"{k}: {a:.3e} {b:.3e}" for k, (a, b) in moved.items()))
    for name in ("halve_mG2", "second_apply", "startup_v"):
        assert max(moved[name]) >= MUTANT_VISIBLE, (name, moved[name])
    assert max(moved["rounding"]) <= ROUNDING, moved["rounding"]
    if not any(ph.CASES[case]["periodic"]):
        _, u, v = ph.reference(oracle, case, "leapfrog4", "rest")
        _, um, vm = ph.reference(oracle, case, "leapfrog4", "rest", mutant="startup_v")
        assert np.abs(u).max() > 0.0 and np.abs(v).max() > 0.0
        assert ph.differing_entries(um, u) == 0 and ph.differing_entries(vm, v) == 0


@pytest.mark.parametrize("case", ["w2_p2", "w4_p4"])
def test_from_rest_hardly_reaches_the_x_interface(oracle, case):
    """the figures of the module docstring: the reason the random-state scenario exists (the meshes of these two cases
    are those of test_distributed_on_one_gpu; RK4 and leapfrog both at CFL 0.25 as there)"""
    c = ph.CASES[case]
    om = ph.global_mesh(oracle, case)
    dt, _ = oracle.cfl_time_step(om, c["p"], ph.C0, ph.FREQ, CFL=0.25)
    for scheme in ("rk4", "leapfrog"):
        ref = oracle.LinearGLLOpt(om, c["p"], ph.C0, ph.FREQ, ph.P0)
        ref.init()
        if scheme == "rk4":
            ref.rk4(0.0, ph.STEPS * dt - 1e-13, dt)
        else:
            ph.lh.leapfrog(ref, *ph.lh.oracle_parts(ref), 0.0, ph.STEPS * dt - 1e-13, dt)
        ratios = plane_ratios(case, ref.u_n)
        print(f"{case} {scheme} from rest: " + ", ".join(f"{k}: {r:.2e}" for k, r in ratios.items()))
        x = [r for k, r in ratios.items() if k.startswith("x=")]
        assert len(x) == 1 and 0.0 < x[0] < 1e-2


@pytest.mark.parametrize("case", list(ph.CASES))
def test_bookkeeping_on_the_library_partition(oracle, case):
    """what the GPU test's parent relies on, on the library's own partition of every case: the global numbering of
    dist_helpers.local_to_global is the oracle's, the owned entries of all ranks cover every global dof once, the ghosts
    are exactly what the neighbours send, and global -> local -> global returns the vector with no ghost mismatch (and
    counts one for a ghost that was changed)"""
    from dist_helpers import local_to_global
    from wave_fenics_amd.distributed import create_distributed_box
    c = ph.CASES[case]
    om = ph.global_mesh(oracle, case)
    u0, v0, p0 = ph.initial_state(om.ndofs, 1e-8, "random")
    assert p0 == 0.0 and np.array_equal(u0, ph.initial_state(om.ndofs, 1e-8, "random")[0])
    ranks, neighbours = [], []
    for rank in range(c["world"]):
        part = create_distributed_box(c["n"], c["p"], c["world"], rank, hi=ph.HI, periodic=c["periodic"], build_dofmap=True)
        assert tuple(part.procs) == c["procs"]
        l2g, owned = local_to_global(part), part.owned_mask()
        n, gn = c["n"], ph.global_cells(case)
        cz, cy, cx = (a.reshape(-1) for a in np.meshgrid(*(np.arange(n[a]) + n[a] * part.coords[a] for a in (2, 1, 0)), indexing="ij"))
        assert np.array_equal(l2g[part.V.dofmap], om.dofmap[cx + gn[0] * (cy + gn[1] * cz)]), "the rank's cells in the oracle's numbering"
        ghosts = np.sort(np.concatenate([np.zeros(0, dtype=np.int32), *part.recv_fwd.values()]))
        assert np.array_equal(ghosts, np.nonzero(~owned)[0])
        neighbours.append(len(set(part.send_fwd) | set(part.recv_fwd)))
        ranks.append({"l2g": l2g, "owned": owned, "x": ph.to_local(u0, l2g)})
    xg, count = ph.assemble_owned(om.ndofs, ranks, "x")
    assert count.min() == 1 and count.max() == 1
    assert np.array_equal(xg, u0) and ph.ghost_mismatches(xg, ranks, "x") == 0
    g = np.nonzero(~ranks[-1]["owned"])[0][0]
    ranks[-1]["x"][g] = np.nextafter(ranks[-1]["x"][g], 2.0)
    assert ph.ghost_mismatches(xg, ranks, "x") == 1 and ph.differing_entries(xg, u0) == 0
    if case == "w8_p4":
        # the lowest rank owns what it shares: rank 0 sends to the seven others, rank 7 receives from all of them
        assert neighbours[0] == 7 and neighbours[7] == 7, neighbours
    if case == "w2_p2_periodic":
        assert all(0 in r and 1 in r for r in (part.send_fwd, part.recv_fwd)), "a peer on both sides in x, itself in y"
