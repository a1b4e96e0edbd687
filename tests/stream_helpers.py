"""The queued-work pattern of test_gpu_cg_iteration.py::test_cg_on_side_stream, once, for tests/test_gpu_stream_order.py and
tests/test_gpu_stream_models.py.  No tests in here, and torch is imported inside the functions that need it.

include/wavehip.h promises that every entry taking a `stream` orders all its device work on that stream and returns
without synchronising.  A test that synchronises before and after the call cannot see a violation: a launch on the null
stream, an interior apply that does not wait for the caller's stream, a blocking memset all give the right answer when
nothing else is in flight.  gated() makes something be in flight:

  load      a finite amount of ordinary device work on a non-blocking side stream (torch.cuda.Stream()): `passes` in-place
            passes over 2^24 doubles.  No host-function gate, no spin-until-flag kernel, no graph capture: the load ends
            by itself whatever the call under test does.
  sequence  every input and in/out vector of the call is NaN on the device.  On the side stream, behind the load, the good
            values are copied in and the event `loaded` is recorded; the call under test follows at once, with no
            synchronise in between; then every output is copied to a snapshot on the same stream.  side.synchronize() is
            the only synchronisation before the snapshots are read.
  result    the snapshots, whether `loaded` was still pending when the call returned, what the call returned, its host
            time and the load's duration by events.

A launch on another stream, or a hidden stream that does not wait for the caller's, reads NaN (or writes before the
copies land) while the load is still running.  A case of an asynchronous entry proves this only if `loaded` was pending at
return: require_pending() fails the case otherwise -- it neither skips nor passes.  Entries that synchronise by contract
are held to the inverse by require_completed().

Stale values.  A launch on the wrong stream runs before the call's own earlier launches have produced anything; it can
look right only if right values lie there from an earlier call.  So the gated call is the first call in the process on
its handle and with its values (factor(k) scales the inputs of case k), and the default-stream twin it is compared with
runs afterwards (twin()).

Size of the load, measured on the MI355X (events around the load for its duration, time.perf_counter around the call for
the host time; the figures are printed by every case):
  one pass              40.5 us (16.2 ms per 400, 24.3 ms per 600, 80.8 ms per 2000, 242 ms per 6000)
  ENTRY_PASSES = 600    24.3 ms, in a whole run 24.25 to 24.5 ms; up to 70 ms for the first case of a process and where
                        RCCL sets up a connection beside the load.  Host time of one call of the entry table: 0.02 to
                        0.06 ms for a launch; 0.12 ms for the two overlapped applies back to back; 0.5 to 1.9 ms where a
                        call is the first in the process to launch from its translation unit (the code object is loaded
                        then): the slowest, wf_op_apply on the tetrahedral stiffness operator, 1.90 ms.  The load is 12.8
                        times that.  (At 400 passes, 16.2 ms, it was 8.8 times: too little.)
  MODEL_PASSES = 2000   80.8 ms (81.6 and 144.8 ms on the periodic partition).  Host time of five steps: rk4 2.08 ms,
                        rk4_fused 0.66 ms, leapfrog 0.32 ms; on the periodic partition rk4_fused 1.19 ms (2.3 to 2.7 ms
                        with a profiler attached), leapfrog 0.72 ms.  The load is 39 times the slowest loop.
Both are more than ten times the host time they cover, as the shared machines' jitter asks."""
from __future__ import annotations

import time
from types import SimpleNamespace

import numpy as np

LOAD_ENTRIES = 2 ** 24
ENTRY_PASSES = 600
MODEL_PASSES = 2000
_load = {}


def factor(k: int) -> float:
    """The scale of case k's inputs: (64 + k) / 64, exact in binary, different for every case of a process"""
    return (64.0 + k) / 64.0


def load_buffer(gpu):
    """the 2^24 doubles the load works on, one per process"""
    import torch
    if "buf" not in _load:
        _load["buf"] = torch.ones(LOAD_ENTRIES, dtype=torch.float64, device=gpu)
    return _load["buf"]


def shifted(gpu, n: int, off: int, dtype=None):
    """n entries at `off` entries (8 bytes each for float64) past an allocation's start, NaN-filled: off = 0 is 16-byte
    aligned, off = 1 is not"""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    return torch.full((n + 2,), float("nan"), dtype=dtype, device=gpu)[off:off + n]


def poisoned(gpu, vecs: dict, off: int = 0):
    """(work, good): for every named host vector a NaN-filled device vector (shifted by `off` entries) and the good
    values on the device"""
    import torch
    work, good = {}, {}
    for name, a in vecs.items():
        a = np.ascontiguousarray(a, dtype=np.float64)
        good[name] = torch.from_numpy(a.copy()).to(gpu)
        work[name] = shifted(gpu, a.size, off)
    return work, good


def gated(gpu, work: dict, good: dict, call, outputs, passes: int = ENTRY_PASSES):
    """The sequence of the module docstring.  work / good: the vectors of poisoned(); call(): the call under test, run
    with the side stream current; outputs: names of `work`, or a callable returning the device tensors to snapshot
    (evaluated after the call, on the side stream).  Returns a namespace: snaps (numpy arrays, in the order of outputs),
    pending, result, host_s, load_ms."""
    import torch
    buf = load_buffer(gpu)
    side = torch.cuda.Stream()
    start, loaded = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()              # the NaN fills and the staged good values are in place; nothing is in flight
    with torch.cuda.stream(side):
        start.record(side)
        for _ in range(passes):
            buf.mul_(1.0)
        for name, t in work.items():
            t.copy_(good[name])
        loaded.record(side)
        t0 = time.perf_counter()
        result = call()
        host_s = time.perf_counter() - t0
        pending = not loaded.query()
        outs = outputs() if callable(outputs) else [work[name] for name in outputs]
        snaps = [o.clone() for o in outs]
    side.synchronize()
    return SimpleNamespace(snaps=[s.cpu().numpy() for s in snaps], pending=pending, result=result, host_s=host_s,
                           load_ms=float(start.elapsed_time(loaded)))


def twin(gpu, work: dict, good: dict, call, outputs):
    """The same call on the default stream with nothing in flight, after the gated one: the good values are copied in,
    the call runs, the device is synchronised.  Returns (outputs as numpy arrays, what the call returned)."""
    import torch
    for name, t in work.items():
        t.copy_(good[name])
    torch.cuda.synchronize()
    result = call()
    torch.cuda.synchronize()
    outs = outputs() if callable(outputs) else [work[name] for name in outputs]
    return [o.cpu().numpy() for o in outs], result


def report(r, what: str) -> str:
    return f"STREAM {what}: load {r.load_ms:.2f} ms, call {r.host_s * 1e3:.3f} ms on the host, loaded pending at return: {r.pending}"


def require_pending(r, what: str):
    """An asynchronous entry: the load must still have been running when the call returned."""
    print(report(r, what))
    assert r.pending, (f"{what}: load already finished when the call returned (load {r.load_ms:.2f} ms, call "
                       f"{r.host_s * 1e3:.3f} ms on the host): either the call synchronised, or the run proved nothing")


def require_completed(r, what: str):
    """An entry that synchronises its stream by contract: when it returns, everything queued before it has run."""
    print(report(r, what))
    assert not r.pending, f"{what}: returned while the work queued before it was still running; its contract says it synchronises"
