"""The stream-taking entries that the adjoint of the fourth-order leapfrog loop uses (include/wavehip.h) behind work on a
side stream, built with stream_helpers.py as tests/test_gpu_leapfrog4_streams.py builds its rows; REFERENCED of
tests/test_gpu_stream_order.py points here.

Rows: wf_leapfrog4_correlate with and without z, each 16-byte aligned and shifted by 8 bytes (n = 513: two full
workgroups of pairs and the odd last dof).  Every input and in/out vector is NaN until the side stream, behind the load,
copies the values in; the call follows at once and must return while the load is still running; the outputs are compared
bit for bit with the same call on the default stream afterwards.

The loop: five steps of wf_wave_leapfrog4 with a hook that keeps every pair, and the start-up derivatives, on
adjoint_helpers.device_model (P2, two-layer medium, a point source, four receivers, all faces absorbing, the owner
stiffness kernel) at leapfrog4's step: u_n, v_n, the traces, a0, j0, q0 and the kept states bit for bit against a twin
model on the default stream.  Then one misfit_gradient(scheme="leapfrog4") the same way; it returns J as a host number,
so it waits for its own stream and is not held to returning early (as test_gpu_stream_models.py holds leapfrog's)."""
import numpy as np
import pytest

import adjoint4_helpers as a4
import adjoint_helpers as ah
import stream_helpers as sh
import test_gpu_stream_models as sm
import test_gpu_stream_order as so
import test_stream_table
from support import bits, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

N = so.N
FIRST = 300           # the factor of row k is stream_helpers.factor(FIRST + k): no case of another module shares it
ROWS = []             # (id, entries, builder(gpu, s, rng, request) -> case)
STREAM_ENTRIES = {"wf_leapfrog4_correlate", "wf_wave_leapfrog4"}
INPUTS = ("lam", "om", "up", "u", "um", "w")


def correlate(with_z):
    def make(gpu, s, rng):
        from wave_fenics_amd import la
        vecs = {k: so.uni(rng, N, s) for k in INPUTS + ("p",) + (("z",) if with_z else ())}
        return (vecs, lambda t: la.leapfrog4_correlate(t["lam"], t["om"], t["up"], t["u"], t["um"], t["w"], t["p"], t.get("z")),
                ["p"] + (["z"] if with_z else []))
    return make


for _z in (True, False):
    for _off in (0, 1):
        def _build(gpu, s, rng, request, make=correlate(_z), off=_off):
            vecs, call, outs = make(gpu, s, rng)
            return so.case(vecs, call, outs, off=off)
        ROWS.append((f"leapfrog4_correlate{'-z' if _z else ''}-{'aligned' if _off == 0 else 'shifted'}", ("wf_leapfrog4_correlate",), _build))


def test_every_stream_entry_of_the_header_is_covered():
    """STREAM_ENTRIES are declared with a `void* stream` in include/wavehip.h (the parser of tests/test_stream_table.py),
    and each has a row here or is the loop test_loop_with_a_hook_behind_queued_work runs"""
    assert STREAM_ENTRIES <= set(test_stream_table.stream_entries())
    assert {e for _, entries, _ in ROWS for e in entries} | {"wf_wave_leapfrog4"} == STREAM_ENTRIES
    assert len({r[0] for r in ROWS}) == len(ROWS)
    from wave_fenics_amd import _lib
    assert STREAM_ENTRIES <= set(_lib.SIGNATURES)


@pytest.mark.parametrize("k", range(len(ROWS)), ids=[r[0] for r in ROWS])
def test_stream_order(gpu, oracle, request, k):
    rid, entries, build = ROWS[k]
    s = sh.factor(FIRST + k)
    c = build(gpu, s, np.random.default_rng(3300 + k), request)
    work, good = sh.poisoned(gpu, c.vecs, c.off)
    r = sh.gated(gpu, work, good, lambda: c.call(work), c.outs)
    sh.require_pending(r, rid)
    ref, _ = sh.twin(gpu, work, good, lambda: c.call(work), c.outs)
    for name, got, want in zip(c.outs, r.snaps, ref):
        off = np.nonzero(bits(got) != bits(want))[0]
        assert np.abs(want).max() > 0.0 and np.isfinite(want).all()
        assert off.size == 0, (rid, name, "entries off the default-stream twin", off.size, "first", off[:8], got[off[:4]], want[off[:4]])


def _twin_run(gpu, sc, s, run, names, what, pending):
    """run(eqn) -> extra output tensors, behind the load on one model and on the default stream on its twin"""
    u0, v0 = sc.u0 * s, sc.v0 * s

    def outputs(eqn, extra):
        return lambda: [eqn.u_n, eqn.v_n, eqn.receivers.traces] + extra["out"]

    eqn = ah.device_model(sc, gpu)
    assert eqn.stiff_op.update == "owner"
    work, good = sm.poison(eqn, gpu, u0, v0)
    extra = {"out": []}
    r = sh.gated(gpu, work, good, lambda: extra.update(out=run(eqn)), outputs(eqn, extra), passes=sh.MODEL_PASSES)
    if pending:
        sh.require_pending(r, what)
    else:
        print(sh.report(r, what))
    twin = ah.device_model(sc, gpu)
    print(f"{what}: entries of m that differed between the two models: {sm.share_mass(twin, eqn)}")
    work2, good2 = sm.poison(twin, gpu, u0, v0)
    extra2 = {"out": []}
    ref, _ = sh.twin(gpu, work2, good2, lambda: extra2.update(out=run(twin)), outputs(twin, extra2))
    assert len(r.snaps) == len(ref) == len(names)
    assert r.snaps[2].shape == (sm.STEPS + 1, 4) and np.abs(ref[0]).max() > 0.0 and np.abs(ref[2]).max() > 0.0
    for name, got, want in zip(names, r.snaps, ref):
        assert np.isfinite(want).all() and np.abs(want).max() > 0.0, name
        sm.same_bits((what, name), got, want)


def test_loop_with_a_hook_behind_queued_work(gpu, oracle):
    """five steps of wf_wave_leapfrog4: the hook copies u^{n-1} and u^n of every step on the stream it is handed"""
    import torch
    from wave_fenics_amd import la
    from wave_fenics_amd._lib import WF_WAVE_LEAPFROG4
    sc = a4.scenario(2)
    tf = sm.STEPS * sc.dt - 1e-3 * sc.dt

    def run(eqn):
        startup = [torch.full_like(eqn.u_n, float("nan")) for _ in range(3)]
        kept, seen = [], []

        def hook(n, t, u_prev, u, a0):
            assert a0.data_ptr() == startup[0].data_ptr()
            seen.append((n, t))
            pair = (torch.full_like(u, float("nan")), torch.full_like(u, float("nan")))
            la.copy(u_prev, pair[0])
            la.copy(u, pair[1])
            kept.extend(pair)

        t, steps = eqn._run(WF_WAVE_LEAPFROG4, 0.0, tf, sc.dt, None, keep=hook, startup=startup)
        assert steps == sm.STEPS and [k for k, _ in seen] == list(range(sm.STEPS)) and seen[0][1] == 0.0
        assert [tt for _, tt in seen] + [t] == list(eqn.trace_times)[-(sm.STEPS + 1):]
        return startup + kept

    names = ["u_n", "v_n", "traces", "a0", "j0", "q0"] + [f"kept{i}" for i in range(2 * sm.STEPS)]
    _twin_run(gpu, sc, sh.factor(FIRST + len(ROWS)), run, names, "wf_wave_leapfrog4 with a hook", pending=True)


def test_misfit_gradient_behind_queued_work(gpu, oracle):
    import torch
    sc = a4.scenario(2)
    s = sh.factor(FIRST + len(ROWS) + 1)
    tf = sm.STEPS * sc.dt - 1e-3 * sc.dt
    observed = np.ascontiguousarray(sc.observed[:sm.STEPS + 1]) * s

    def run(eqn):
        J, gk, gm, info = eqn.misfit_gradient(0.0, tf, sc.dt, observed, scheme="leapfrog4")
        assert info["steps"] == sm.STEPS and info["S"] == 3
        return [gk, gm, torch.tensor([J], dtype=torch.float64, device=gpu)]

    _twin_run(gpu, sc, s, run, ["u_n", "v_n", "traces", "g_stiff", "g_mass", "J"], "misfit_gradient(leapfrog4)", pending=False)
