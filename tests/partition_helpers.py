"""The scenarios, references and bookkeeping of the partitioned time-stepping tests (test_partition_scenario_host.py,
test_gpu_partition_models.py).

Two scenarios on the global box [0, 0.01]^3, c0 = 1500, f = 0.5 MHz:

* "random": no source (pressureAmplitude = 0), u0 = uniform(-1, 1) and v0 = uniform(-1, 1) / (STEPS dt) drawn with
  np.random.default_rng(SEED) on the GLOBAL dof numbering, every absorbing face active.  Every plane where two ranks meet
  carries a value of the size of the global maximum from the first step on, so an error made there -- a facet mass
  not assembled across ranks, a ghost entry not refreshed, a reverse add lost -- is an error of the result.
* "rest": from rest with the source (p0 = 6e4) on x = 0, the scenario of the older model tests; it keeps the s1 c1 term
  of a source face cut by a rank interface in the run.

The references are the single-domain oracle on the global mesh (oracle.make_periodic first in the periodic case):
leapfrog_helpers.leapfrog for leapfrog, leapfrog4_helpers.leapfrog4 for the fourth-order leapfrog (at the leapfrog
runs' step, inside its own limit, which is sqrt(3) times leapfrog's), oracle.LinearGLLOpt.rk4 for RK4.  Local vectors are
the global ones taken through dist_helpers.local_to_global, ghosts included.

Mutants of the leapfrog4 reference, for the host test (mutant= of reference()): each wraps the stepper's K and counts its
calls -- three applies in the start-up (K u0, K v0, K a0), two per step (K u, K w), three in the finish (K u, K w, K vt):

* "second_apply": the operand of every step's second apply (the finish's included) is zeroed on the interface planes
  -- the forward halo of w not made;
* "startup_v": the operand of the second start-up apply, v0, is zeroed there -- the forward halo of v not made;
* "rounding": no mutant, the yardstick of the bound: every apply's result times (1 + 2^-52)."""
import numpy as np

import leapfrog4_helpers as l4
import leapfrog_helpers as lh
from support import relerr  # noqa: F401

C0, FREQ, P0 = 1500.0, 0.5e6, 6e4
STEPS, HI, SEED = 20, (0.01, 0.01, 0.01), 11
SCENARIOS = ("random", "rest")

# name: world, procs, degree, cells per rank, periodic axes, CFL of the leapfrog runs, CFL of the RK4 runs.  The smallest
# shapes at which each feature exists: absorbing faces cut by an x interface; the source face cut in y, an edge shared by
# four ranks and the owner kernel at P4; a z ghost plane between different ranks and corner peers (7 neighbours); the
# same peer on both sides in x with a self-neighbour in y and no source face.  (The host test runs all four; the GPU test
# leaves the 8-rank case out, see test_gpu_partition_models.GPU_CASES.)
CASES = {
    "w2_p2": dict(world=2, procs=(2, 1, 1), p=2, n=(3, 4, 4), periodic=(False, False, False), cfl_lf=0.5, cfl_rk=0.25),
    "w4_p4": dict(world=4, procs=(2, 2, 1), p=4, n=(3, 3, 4), periodic=(False, False, False), cfl_lf=0.25, cfl_rk=0.25),
    "w8_p4": dict(world=8, procs=(2, 2, 2), p=4, n=(2, 2, 2), periodic=(False, False, False), cfl_lf=0.5, cfl_rk=0.25),
    "w2_p2_periodic": dict(world=2, procs=(2, 1, 1), p=2, n=(3, 4, 4), periodic=(True, True, False), cfl_lf=0.5, cfl_rk=0.25),
}
MUTANTS = ("second_apply", "startup_v", "rounding")
_MESH, _REF = {}, {}


def global_cells(case):
    c = CASES[case]
    return tuple(c["procs"][a] * c["n"][a] for a in range(3))


def global_lattice(case):
    """points per axis of the global dof numbering (a periodic axis has lost its upper plane)"""
    c = CASES[case]
    return tuple(c["p"] * g + (0 if per else 1) for g, per in zip(global_cells(case), c["periodic"]))


def global_mesh(oracle, case):
    """the oracle's mesh of the whole box (periodic axes identified), built once and never modified afterwards"""
    if case not in _MESH:
        c = CASES[case]
        om = oracle.create_box(global_cells(case), c["p"], hi=HI)
        if any(c["periodic"]):
            oracle.make_periodic(om, c["periodic"])
        G = global_lattice(case)
        assert om.ndofs == G[0] * G[1] * G[2]
        _MESH[case] = om
    return _MESH[case]


def time_step(oracle, case, scheme):
    c = CASES[case]
    return oracle.cfl_time_step(global_mesh(oracle, case), c["p"], C0, FREQ, CFL=c["cfl_lf" if scheme in ("leapfrog", "leapfrog4") else "cfl_rk"])[0]


def initial_state(ndofs, dt, scenario):
    """(u0, v0, pressure amplitude) on the global numbering"""
    if scenario == "rest":
        return np.zeros(ndofs), np.zeros(ndofs), P0
    rng = np.random.default_rng(SEED)
    u0 = rng.uniform(-1.0, 1.0, ndofs)
    v0 = rng.uniform(-1.0, 1.0, ndofs) / (STEPS * dt)
    return u0, v0, 0.0


def interface_planes(case):
    """{name: boolean mask over the global dofs} of every lattice plane on which two ranks (or a rank and itself, through
    a periodic axis) meet"""
    c = CASES[case]
    G = global_lattice(case)
    K, J, I = np.meshgrid(np.arange(G[2]), np.arange(G[1]), np.arange(G[0]), indexing="ij")
    coord = (I.reshape(-1), J.reshape(-1), K.reshape(-1))
    planes = {}
    for a in range(3):
        at = [c["p"] * c["n"][a] * r for r in range(1, c["procs"][a])] + ([0] if c["periodic"][a] else [])
        for i in at:
            planes[f"{'xyz'[a]}={i}"] = coord[a] == i
    assert planes
    return planes


def mutated(K, mutant, steps, planes):
    """K of the stepper under a mutant of the module docstring (steps: the steps of the ONE call of leapfrog4 that
    follows; planes: a mask of dofs).  Returns (the wrapper, a list holding the number of calls made)."""
    assert mutant in MUTANTS, mutant
    calls = [0]
    second = {3 + 2 * k + 1 for k in range(steps + 1)}

    def wrapped(u):
        i = calls[0]
        calls[0] += 1
        if (mutant == "second_apply" and i in second) or (mutant == "startup_v" and i == 1):
            u = np.where(planes, 0.0, u)
        y = K(u)
        return y * (1.0 + 2.0 ** -52) if mutant == "rounding" else y
    return wrapped, calls


def run_stepper(ref, scheme, dt, segments, mutant=None, planes=None):
    """the numpy stepper of `scheme` ("leapfrog", "leapfrog4") on the oracle model ref from its (u_n, v_n): one call per
    entry of segments (numbers of steps), each from the (t, u_n, v_n) the one before left.  Returns t."""
    K, s1, s2 = lh.oracle_parts(ref)
    calls = None
    if mutant is not None:
        assert scheme == "leapfrog4" and len(segments) == 1
        K, calls = mutated(K, mutant, segments[0], planes)
    step = l4.leapfrog4 if scheme == "leapfrog4" else lh.leapfrog
    t = 0.0
    for k, n in enumerate(segments):
        # the first call as the models' tests make it, the later ones as a restart does: from t, max_steps alone
        t, took = step(ref, K, s1, s2, t, n * dt - 1e-13, dt) if k == 0 else step(ref, K, s1, s2, t, 1.0, dt, max_steps=n)
        assert took == n
    assert calls is None or calls[0] == 3 + 2 * segments[0] + 3, calls
    return t


def reference(oracle, case, scheme, scenario, steps=STEPS, halve_mG2=None, mutant=None):
    """(dt, u_n, v_n) of the single-domain oracle after `steps` steps, computed once per key.  steps: a number, or a tuple
    (steps_a, steps_b, ...) -- the split reference of a restarted run, one call of the stepper per entry (leapfrog and
    leapfrog4).  halve_mG2: a mask of global dofs whose absorbing facet mass is halved (the mutant of the host test:
    masses not assembled across ranks).  mutant: one of MUTANTS, on the interface planes of the case (leapfrog4)."""
    key = (case, scheme, scenario, steps)
    plain = halve_mG2 is None and mutant is None
    if plain and key in _REF:
        return _REF[key]
    c = CASES[case]
    om = global_mesh(oracle, case)
    dt = time_step(oracle, case, scheme)
    u0, v0, p0 = initial_state(om.ndofs, dt, scenario)
    ref = oracle.LinearGLLOpt(om, c["p"], C0, FREQ, p0)
    if halve_mG2 is not None:
        assert (ref.mG2[halve_mG2] > 0.0).any(), "the mutant needs absorbing dofs on the interface planes"
        ref.mG2 = np.where(halve_mG2, 0.5 * ref.mG2, ref.mG2)
    ref.init()
    ref.u_n[:] = u0
    ref.v_n[:] = v0
    if scheme in ("leapfrog", "leapfrog4"):
        planes = np.logical_or.reduce(list(interface_planes(case).values())) if mutant is not None else None
        run_stepper(ref, scheme, dt, steps if isinstance(steps, tuple) else (steps,), mutant, planes)
    else:
        assert mutant is None and not isinstance(steps, tuple)
        t, n = ref.rk4(0.0, steps * dt - 1e-13, dt)
        assert n == steps
    out = (dt, ref.u_n.copy(), ref.v_n.copy())
    for a in out[1:]:
        a.setflags(write=False)
    if plain:
        _REF[key] = out
    return out


def to_local(xg, l2g):
    """global -> local, ghosts included"""
    return np.ascontiguousarray(np.asarray(xg)[l2g])


def assemble_owned(ndofs, ranks, key):
    """local owned -> global: ranks = [{"l2g", "owned", key: local vector}, ...].  Returns (global vector, how many ranks
    own each global dof); a partition is sound when the count is 1 everywhere."""
    xg, count = np.zeros(ndofs), np.zeros(ndofs, dtype=np.int64)
    for r in ranks:
        own = r["owned"]
        xg[r["l2g"][own]] = r[key][own]
        np.add.at(count, r["l2g"][own], 1)
    return xg, count


def ghost_mismatches(xg, ranks, key):
    """number of local entries (the ghosts; the owned ones by construction) whose bits differ from the owner's"""
    bad = 0
    for r in ranks:
        got, want = np.ascontiguousarray(r[key]).view(np.uint64), np.ascontiguousarray(xg[r["l2g"]]).view(np.uint64)
        bad += int(np.count_nonzero(got != want))
    return bad


def differing_entries(a, b):
    """entries whose bits differ"""
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)))
