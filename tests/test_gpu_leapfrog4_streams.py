"""The stream-taking entries of the fourth-order leapfrog (include/wavehip.h) behind work on a side stream, built with
stream_helpers.py exactly as tests/test_gpu_stream_order.py builds its rows (its REFERENCED points here), and five steps of LinearGLLOpt.leapfrog4 behind the load as tests/test_gpu_stream_models.py runs
the other loops.

Rows: wf_leapfrog4_predict with and without a plan, wf_leapfrog4_correct with and without a plan and v, each 16-byte
aligned and shifted by 8 bytes (n = 513: two full workgroups of pairs and the odd last dof); wf_sources_add_stencil on
the points of the sources_add row.  Every input and in/out vector is NaN until the side stream, behind the load, copies
the values in; the call follows at once and must return while the load is still running; the outputs are compared bit
for bit with the same call on the default stream afterwards.

The model: adjoint_helpers.device_model (P2, two-layer medium, a point source, four receivers, all faces absorbing, the
owner stiffness kernel): u_n, v_n and the traces bit for bit against a twin model on the default stream."""
import numpy as np
import pytest

import adjoint_helpers as ah
import stream_helpers as sh
import test_gpu_stream_models as sm
import test_gpu_stream_order as so
import test_stream_table
from support import bits, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

N = so.N
FIRST = 200           # the factor of row k is stream_helpers.factor(FIRST + k): no case of another module shares it
ROWS = []             # (id, entries, builder(gpu, s, rng, request) -> case)
STREAM_ENTRIES = {"wf_leapfrog4_predict", "wf_leapfrog4_correct", "wf_sources_add_stencil", "wf_wave_leapfrog4"}


def la():
    from wave_fenics_amd import la as module
    return module


def sets(rng, s):
    """two overlapping boundary sets over [0, N) with facet masses"""
    i1, i2 = rng.permutation(N)[:N // 4].astype(np.int32), rng.permutation(N)[:N // 3].astype(np.int32)
    return i1, rng.uniform(0.1, 2.0, i1.size) * s, i2, rng.uniform(0.1, 2.0, i2.size) * s


def simple(name, entry, make):
    for off in (0, 1):
        def build(gpu, s, rng, request, make=make, off=off):
            vecs, call, outs = make(gpu, s, rng)
            return so.case(vecs, call, outs, off=off)
        ROWS.append((f"{name}-{'aligned' if off == 0 else 'shifted'}", (entry,), build))


def predict(bc):
    def make(gpu, s, rng):
        vecs = {k: so.uni(rng, N, s) for k in ("b", "u", "u_prev", "u_star", "w")}
        vecs["m"] = rng.uniform(0.5, 1.5, N) * s
        plan = la().BoundaryPlan(N, *sets(rng, s)) if bc else None
        return (vecs, lambda t: la().leapfrog4_predict(t["b"], t["m"], t["u"], t["u_prev"], t["u_star"], t["w"], 0.25, bc=plan,
                                                        s1=0.7 * s, s2=-1.3), ["b", "u_star", "w"])
    return make


def correct(bc, with_v):
    def make(gpu, s, rng):
        vecs = {k: so.uni(rng, N, s) for k in ["b", "u_star", "u_next"] + (["u_prev", "v"] if with_v else [])}
        vecs["m"] = rng.uniform(0.5, 1.5, N) * s
        plan = la().BoundaryPlan(N, *sets(rng, s)) if bc else None
        return (vecs, lambda t: la().leapfrog4_correct(t["b"], t["m"], t["u_star"], t["u_next"], 0.25, u_prev=t.get("u_prev"),
                                                        v=t.get("v"), bc=plan, s1c=-0.04 * s, s2=-1.3),
                ["b", "u_next"] + (["v"] if with_v else []))
    return make


for _bc in (False, True):
    simple(f"leapfrog4_predict{'-bc' if _bc else ''}", "wf_leapfrog4_predict", predict(_bc))
    for _v in (False, True):
        simple(f"leapfrog4_correct{'-bc' if _bc else ''}-{'v' if _v else 'no-v'}", "wf_leapfrog4_correct", correct(_bc, _v))


def stencil_row(gpu, s, rng, request):
    from wave_fenics_amd import points
    V, located = so.points_space(rng)
    src = points.Sources(V, None, [points.ricker(1.0e6, 1.0e-6, s * (1 + i)) for i in range(5)], located=located)
    return so.case({"b": so.uni(rng, V.ndofs, s)},
                   lambda t: src.add_stencil([1.0e-6, 1.2e-6, 1.4e-6], [1.0 / 12.0, -2.0 / 12.0, 1.0 / 12.0], t["b"]), ["b"], keep=src)


ROWS.append(("sources_add_stencil", ("wf_sources_add_stencil",), stencil_row))


def test_every_stream_entry_of_the_header_is_covered():
    """STREAM_ENTRIES are declared with a `void* stream` in include/wavehip.h (the parser of tests/test_stream_table.py),
    and each has a row here or is the loop test_model_behind_queued_work runs"""
    from wave_fenics_amd import _lib
    assert STREAM_ENTRIES <= set(test_stream_table.stream_entries()) and STREAM_ENTRIES <= set(_lib.SIGNATURES)
    assert {e for _, entries, _ in ROWS for e in entries} | {"wf_wave_leapfrog4"} == STREAM_ENTRIES
    assert len({r[0] for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize("k", range(len(ROWS)), ids=[r[0] for r in ROWS])
def test_stream_order(gpu, oracle, request, k):
    rid, entries, build = ROWS[k]
    s = sh.factor(FIRST + k)
    c = build(gpu, s, np.random.default_rng(3000 + k), request)
    work, good = sh.poisoned(gpu, c.vecs, c.off)
    # the gated call first: the first call in the process on this handle and with these values
    r = sh.gated(gpu, work, good, lambda: c.call(work), c.outs)
    sh.require_pending(r, rid)
    ref, _ = sh.twin(gpu, work, good, lambda: c.call(work), c.outs)
    for name, got, want in zip(c.outs, r.snaps, ref):
        off = np.nonzero(bits(got) != bits(want))[0]
        assert name == "b" and rid.startswith("leapfrog4") or np.abs(want).max() > 0.0       # the kernels leave b zero
        assert off.size == 0, (rid, entries, name, "entries off the default-stream twin", off.size, "first", off[:8], got[off[:4]],
                               want[off[:4]])


def test_model_behind_queued_work(gpu, oracle):
    """five steps of leapfrog4, as test_gpu_stream_models.test_one_rank_loops runs leapfrog"""
    sc = ah.scenario(2)
    s = sh.factor(FIRST + len(ROWS))
    u0, v0, dt = sc.u0 * s, sc.v0 * s, sc.dt
    tf = sm.STEPS * dt - 1e-3 * dt

    def run(eqn):
        t, steps = eqn.leapfrog4(0.0, tf, dt)
        assert steps == sm.STEPS

    eqn = ah.device_model(sc, gpu)
    assert eqn.stiff_op.update == "owner"
    work, good = sm.poison(eqn, gpu, u0, v0)
    r = sh.gated(gpu, work, good, lambda: run(eqn), lambda: [eqn.u_n, eqn.v_n, eqn.receivers.traces], passes=sh.MODEL_PASSES)
    sh.require_pending(r, "leapfrog4")
    twin = ah.device_model(sc, gpu)
    print(f"leapfrog4: entries of m that differed between the two models: {sm.share_mass(twin, eqn)}")
    work2, good2 = sm.poison(twin, gpu, u0, v0)
    ref, _ = sh.twin(gpu, work2, good2, lambda: run(twin), lambda: [twin.u_n, twin.v_n, twin.receivers.traces])
    assert r.snaps[2].shape == (sm.STEPS + 1, 4) and np.abs(ref[0]).max() > 0.0 and np.abs(ref[2]).max() > 0.0
    for name, got, want in zip(("u_n", "v_n", "traces"), r.snaps, ref):
        sm.same_bits(("leapfrog4", name), got, want)
