"""The time loops of the library (csrc/wave_loops.cpp) without a GPU: what they refuse, their step count, and the layout
of their descriptor.

Refusals.  Every case is a complete descriptor with one defect.  The pointers are made-up addresses: a refusal comes
before the first launch and before anything is dereferenced, so the return code is WF_ERR_INVALID with the entry's own
message on a machine with no device (a launch would fail otherwise, with WF_ERR_HIP).

Step count.  wf_wave_step_count against the loops of the Python model as of commit a25be7c, written out here: `while t <
tf` with t += dt, the step shortened to tf - t in rk4_fused only, and max_steps looked at after a step (so 0 takes one
step where t0 < tf, as it always has)."""
import ctypes
import os
import subprocess

import pytest

from support import wlib  # noqa: F401
from test_op_lists_host import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
FAKE = 0x7f0000001000      # never dereferenced


def descriptor(wlib, rows=0):
    d = wlib.WaveDesc()
    d.n, d.d_m, d.d_b, d.bc = 100, FAKE, FAKE + 0x1000, FAKE + 0x2000
    d.d_work = (ctypes.c_void_p * 7)(*[FAKE + 0x10000 * (k + 1) for k in range(7)])
    d.source = wlib.WaveSource(1500.0, 1500.0 ** 2, 6e4, 3.0e6, 0.5e6, 4.0, 2.0e-6, 0)
    d.fold_boundary, d.op = 1, FAKE + 0x4000
    if rows:
        d.receivers, d.d_traces, d.trace_rows = FAKE + 0x5000, FAKE + 0x6000, rows
    return d


def call(wlib, entry, d, u=FAKE + 0x7000, v=FAKE + 0x8000, t0=0.0, tf=4.5, dt=1.0, max_steps=-1):
    L = wlib.lib()
    t_end, steps = ctypes.c_double(-1.0), ctypes.c_int64(-1)
    args = (None if d is None else ctypes.byref(d), t0, tf, dt, max_steps, u, v)
    if entry == "wf_wave_leapfrog":
        rc = L.wf_wave_leapfrog(*args, wlib.WAVE_STEP_FN(), None, ctypes.byref(t_end), ctypes.byref(steps), None)
    elif entry == "wf_wave_leapfrog4":
        rc = L.wf_wave_leapfrog4(*args, wlib.WAVE_STEP_FN(), None, None, ctypes.byref(t_end), ctypes.byref(steps), None)
    else:
        rc = L.wf_wave_rk4_fused(*args, ctypes.byref(t_end), ctypes.byref(steps), None)
    assert t_end.value == -1.0 and steps.value == -1       # a refused call writes nothing
    return rc, L.wf_last_error().decode()


def set_field(**fields):
    def defect(d):
        for k, v in fields.items():
            setattr(d, k, v)
    return defect


DESC_DEFECTS = {
    "n < 0": (set_field(n=-1), "n < 0"),
    "null work": (set_field(d_work=None), "null work"),
    "a null work vector": (set_field(d_work=(ctypes.c_void_p * 7)(FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE)), "null work"),
    "null m": (set_field(d_m=None), "null m, b or boundary plan"),
    "null b": (set_field(d_b=None), "null m, b or boundary plan"),
    "null plan": (set_field(bc=None), "null m, b or boundary plan"),
    "neither op nor callback": (set_field(op=None), "needs an operator handle or a right-hand-side callback"),
    "overlapped without an updater": (set_field(overlapped=1), "overlapped needs an updater"),
    "receivers without a buffer": (set_field(receivers=FAKE + 0x5000, trace_rows=100), "receivers without a trace buffer"),
}


# the work vectors each entry asks for: a null one among them is refused, whichever it is, and one beyond them is not read
WORK_VECTORS = {"wf_wave_rk4_fused": 7, "wf_wave_leapfrog": 3, "wf_wave_leapfrog4": 4}


@pytest.mark.parametrize("entry", ["wf_wave_rk4_fused", "wf_wave_leapfrog", "wf_wave_leapfrog4"])
def test_refusals_before_any_launch(wlib, entry):
    for name, (defect, text) in DESC_DEFECTS.items():
        d = descriptor(wlib)
        defect(d)
        rc, msg = call(wlib, entry, d)
        assert rc == INVALID and msg == f"{entry}: {text}", (name, rc, msg)
    # each work vector alone null, the others not -- for wf_wave_leapfrog4 the fourth, which wf_wave_leapfrog never reads
    for k in range(WORK_VECTORS[entry]):
        d = descriptor(wlib)
        d.d_work = (ctypes.c_void_p * 7)(*[None if j == k else FAKE + 0x10000 * (j + 1) for j in range(7)])
        rc, msg = call(wlib, entry, d)
        assert rc == INVALID and msg == f"{entry}: null work", (k, rc, msg)
    rc, msg = call(wlib, entry, None)
    assert rc == INVALID and msg == f"{entry}: null descriptor", (rc, msg)
    for state in ({"u": None}, {"v": None}):
        rc, msg = call(wlib, entry, descriptor(wlib), **state)
        assert rc == INVALID and msg == f"{entry}: null state", (state, rc, msg)
    for dt in (0.0, -1.0, float("nan")):
        rc, msg = call(wlib, entry, descriptor(wlib), dt=dt)
        assert rc == INVALID and msg == f"{entry}: the time step must be positive", (dt, rc, msg)
    # 4.5 / 1.0: five steps, six rows; max_steps = 2: three rows
    for rows, max_steps in ((5, -1), (1, -1), (2, 2)):
        rc, msg = call(wlib, entry, descriptor(wlib, rows), max_steps=max_steps)
        assert rc == INVALID and msg == f"{entry}: the trace buffer has fewer rows than steps + 1", (rows, max_steps, rc, msg)
    # the host times alone ask for the rows as well
    d = descriptor(wlib)
    times = (ctypes.c_double * 5)()
    d.h_times, d.trace_rows = times, 5
    rc, msg = call(wlib, entry, d)
    assert rc == INVALID and msg == f"{entry}: the trace buffer has fewer rows than steps + 1", (rc, msg)
    assert list(times) == [0.0] * 5


def parent_steps(scheme, t0, tf, dt, max_steps):
    t, step = t0, 0
    while t < tf:
        if scheme == "rk4_fused":
            dt = min(dt, tf - t)
        t += dt
        step += 1
        if max_steps is not None and step >= max_steps:
            break
    return step


def test_step_count(wlib):
    L = wlib.lib()
    schemes = {"rk4_fused": wlib.WF_WAVE_RK4_FUSED, "leapfrog": wlib.WF_WAVE_LEAPFROG, "leapfrog4": wlib.WF_WAVE_LEAPFROG4}
    dt = 1.2345e-8
    runs = [(0.0, 5 * dt - 1e-13, dt), (0.0, 5 * dt, dt), (0.0, 5 * dt + 1e-13, dt), (2 * dt, 5 * dt - 1e-13, dt), (0.0, 0.3, 0.1),
            (0.0, 0.1 + 0.1 + 0.1, 0.1), (0.0, 1.0, 0.1), (1.0, 1.0, 0.1), (2.0, 1.0, 0.1), (0.0, 1.0e9, dt), (0.0, 0.25 * dt, dt),
            (7.0, 7.0 + 1000.5 * dt, dt)]
    seen = set()
    for name, scheme in schemes.items():
        for t0, tf, step in runs:
            for max_steps in (None, 0, 1, 3, 1000):
                if tf == 1.0e9 and max_steps is None:
                    continue
                want = parent_steps(name, t0, tf, step, max_steps)
                got = L.wf_wave_step_count(scheme, t0, tf, step, -1 if max_steps is None else max_steps)
                assert got == want, (name, t0, tf, step, max_steps, got, want)
                seen.add(want)
    assert {0, 1, 3, 5, 1000, 1001} <= seen, sorted(seen)
    assert L.wf_wave_work_vectors(wlib.WF_WAVE_RK4_FUSED) == 7 and L.wf_wave_work_vectors(wlib.WF_WAVE_LEAPFROG) == 3
    assert wlib.WF_WAVE_LEAPFROG4 == 2 and L.wf_wave_work_vectors(wlib.WF_WAVE_LEAPFROG4) == WORK_VECTORS["wf_wave_leapfrog4"] == 4
    assert L.wf_wave_work_vectors(3) == -1 and L.wf_wave_work_vectors(-1) == -1


def test_descriptor_layout(wlib, tmp_path):
    """_lib.WaveDesc and _lib.WaveSource are the structs of include/wavehip.h: sizes and every field's offset, from a
    program compiled against the header"""
    fields = {"wf_wave_source": [f for f, _ in wlib.WaveSource._fields_], "wf_wave_desc": [f for f, _ in wlib.WaveDesc._fields_]}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "wavehip.h"', "int main(void) {"]
    for struct, names in fields.items():
        lines.append(f'  printf("{struct} %zu\\n", sizeof({struct}));')
        lines += [f'  printf("{struct}.{f} %zu\\n", offsetof({struct}, {f}));' for f in names]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.cpp", str(tmp_path / "layout")
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([host_compiler(), "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines())
    for struct, cls in (("wf_wave_source", wlib.WaveSource), ("wf_wave_desc", wlib.WaveDesc)):
        assert int(got[struct]) == ctypes.sizeof(cls)
        for f in fields[struct]:
            assert int(got[f"{struct}.{f}"]) == getattr(cls, f).offset, (struct, f)
