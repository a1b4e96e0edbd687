"""The time loops of the library (wf_wave_rk4_fused, wf_wave_leapfrog; csrc/wave_loops.cpp) on the small models of
tests/wave_loop_helpers.py, where a build reproduces its own bits.  Everything is compared bit for bit.

Against the Python loops they replace: tests/golden/wave_loop_bits.json holds the hashes of commit a25be7c for four
steps of each loop, for rk4_fused with fold_boundary = False, for max_steps = 0, 1 and 4, and for calls with t0 >= tf
(no step; leapfrog still does its start-up and its finishing step).  tests/test_gpu_time_step_bits.py holds the loops to
that commit's bits on larger boxes, with and without a medium.

Of the entries themselves: the work vectors are written before they are read (full of NaN or of zeros: the same
results); the per-step callback sees step 0 .. N - 1 at the times of the t += dt accumulation and the start-up
acceleration at step 0; steps and the time returned are wf_wave_step_count's, the traces take steps + 1 rows and the row
behind them keeps its sentinel; the right-hand side given as a callback (the Python model's _rhs) and as the operator
handle give the same results."""
import json

import numpy as np
import pytest

import wave_loop_helpers as wh
from support import bits, gpu  # noqa: F401

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e77


@pytest.fixture(scope="module", params=wh.BOXES, ids=lambda b: f"P{b[0]}")
def box(gpu, request):
    return wh.Box(*request.param, gpu)


@pytest.fixture(scope="module")
def golden():
    with open(wh.FIXTURE) as f:
        return json.load(f)


def scheme_of(loop):
    from wave_fenics_amd import _lib
    return {"rk4_fused": _lib.WF_WAVE_RK4_FUSED, "leapfrog": _lib.WF_WAVE_LEAPFROG}[loop]


def test_bits_of_the_python_loops(box, golden):
    specs = wh.runs(box)
    assert sorted(f"P{p}_{name}" for p, _ in wh.BOXES for name in specs) == sorted(golden)
    differ = []
    for name, spec in specs.items():
        eqn, t, steps = wh.run(box, *spec)
        got = wh.digest(eqn, t, steps)
        print(f"P{box.p}_{name}: steps {steps} t {t!r} rows {eqn.receivers.traces.shape[0]}")
        assert eqn.receivers.traces.shape[0] == steps + 1 == len(eqn.trace_times)
        if got != golden[f"P{box.p}_{name}"]:
            differ.append(name)
    assert not differ, f"other bits than the Python loops of a25be7c in: {differ}"


@pytest.mark.parametrize("loop", wh.LOOPS)
def test_work_vectors_are_written_before_they_are_read(box, golden, loop):
    import torch
    from wave_fenics_amd import _lib
    count = _lib.lib().wf_wave_work_vectors(scheme_of(loop))
    assert count == {"rk4_fused": 7, "leapfrog": 3}[loop]
    got = []
    for fill in (float("nan"), 0.0):
        eqn = box.model()
        work = [torch.full((box.V.ndofs,), fill, dtype=torch.float64, device=box.dev) for _ in range(count)]
        t, steps = eqn._run(scheme_of(loop), 0.0, wh.STEPS * box.dt - 1e-13, box.dt, None, work=work)
        assert steps == wh.STEPS
        got.append(wh.digest(eqn, t, steps))
    assert got[0] == got[1] == golden[f"P{box.p}_{loop}"]


def test_per_step_callback(box, golden):
    import torch
    from wave_fenics_amd import _lib, la
    eqn = box.model()
    dt, t0 = box.dt, 2 * box.dt
    # b / m of the start-up, from the pieces: K u^0, the boundary term at t0 and the point source
    b, a0 = torch.zeros_like(eqn.u_n), torch.zeros_like(eqn.u_n)
    eqn.stiff_op(eqn.u_n, b)
    eqn._bc.apply(eqn._s1(t0), eqn._s2, eqn.v_n, b)
    eqn.sources.add(t0, b)
    la.pointwise_div(b, eqn.m, a0)
    seen = []

    def keep(n, t, u_prev, u, scratch):
        seen.append((n, t, u_prev.clone(), u.clone(), scratch.clone()))

    t_end, steps = eqn._run(_lib.WF_WAVE_LEAPFROG, t0, t0 + wh.STEPS * dt - 1e-13, dt, None, keep=keep)
    torch.cuda.synchronize()
    assert steps == wh.STEPS and [s[0] for s in seen] == list(range(wh.STEPS))
    t, want = t0, []
    for _ in range(wh.STEPS):
        want.append(t)
        t += dt
    assert [s[1].hex() for s in seen] == [w.hex() for w in want] and t_end.hex() == t.hex()
    assert np.array_equal(bits(seen[0][4].cpu().numpy()), bits(a0.cpu().numpy())) and float(a0.abs().max()) > 0.0
    assert np.array_equal(bits(seen[0][3].cpu().numpy()), bits(box.u0.cpu().numpy()))          # u^0
    for k in range(1, wh.STEPS):                                                               # u^{n-1} of a step is u^n of the last
        assert np.array_equal(bits(seen[k][2].cpu().numpy()), bits(seen[k - 1][3].cpu().numpy()))
    # the loop's launches do not depend on the callback: the same results as without one
    ref, t_ref, steps_ref = wh.run(box, "leapfrog", True, t0, t0 + wh.STEPS * dt - 1e-13, None)
    assert wh.digest(eqn, t_end, steps) == wh.digest(ref, t_ref, steps_ref)

    def broken(n, t, u_prev, u, scratch):
        raise KeyError("from the callback")

    with pytest.raises(KeyError, match="from the callback"):                                   # no exception crosses the C boundary
        box.model()._run(_lib.WF_WAVE_LEAPFROG, 0.0, dt, dt, None, keep=broken)


@pytest.mark.parametrize("loop", wh.LOOPS)
def test_max_steps(box, loop):
    import torch
    from wave_fenics_amd import _lib
    L, dt = _lib.lib(), box.dt
    for t0, tf, max_steps in ((0.0, 1.0, 0), (0.0, 1.0, 1), (0.0, 1.0, wh.STEPS), (0.0, wh.STEPS * dt - 1e-13, None),
                              (3 * dt, 3 * dt, None), (3 * dt, 2 * dt, 1)):
        eqn = box.model(capacity=8)
        rec = eqn.receivers
        rec.reserve(0, box.dev)
        rec._buf.fill_(SENTINEL)
        t, steps = getattr(eqn, loop)(t0, tf, dt, max_steps=max_steps)
        torch.cuda.synchronize()
        want = L.wf_wave_step_count(scheme_of(loop), t0, tf, dt, -1 if max_steps is None else max_steps)
        assert steps == want == (0 if t0 >= tf else max(max_steps, 1) if max_steps is not None else wh.STEPS), (t0, tf, max_steps, steps)
        step, acc = dt, t0
        for _ in range(steps):
            if loop == "rk4_fused":
                step = min(step, tf - acc)
            acc += step
        assert t.hex() == acc.hex()
        buf = rec._buf.cpu().numpy().reshape(8, len(rec))
        assert rec.traces.shape == (steps + 1, len(rec)) and len(rec.times) == steps + 1 and rec.times[0] == t0 and rec.times[-1] == t
        assert (buf[:steps + 1] != SENTINEL).all() and np.isfinite(buf[:steps + 1]).all()
        assert (buf[steps + 1:] == SENTINEL).all(), "a row behind the traces was written"
        if t0 >= tf:
            assert np.array_equal(bits(eqn.u_n.cpu().numpy()), bits(box.u0.cpu().numpy()))
            changed = not np.array_equal(bits(eqn.v_n.cpu().numpy()), bits(box.v0.cpu().numpy()))
            assert changed == (loop == "leapfrog")      # its finishing step gives the central velocity; rk4_fused copies


@pytest.mark.parametrize("loop", wh.LOOPS)
def test_rhs_callback_against_operator_handle(box, golden, loop):
    eqn = box.model()
    calls = []

    def rhs(x, b):
        calls.append(1)
        eqn._rhs(x, b)

    t, steps = eqn._run(scheme_of(loop), 0.0, wh.STEPS * box.dt - 1e-13, box.dt, None, rhs=rhs)
    assert len(calls) == (4 * wh.STEPS if loop == "rk4_fused" else wh.STEPS + 2)
    assert wh.digest(eqn, t, steps) == golden[f"P{box.p}_{loop}"]
