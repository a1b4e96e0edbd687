"""The plane source of the time loops (csrc/wave_source.h) against the expressions the Python model evaluated before
the loops moved into the library, bit for bit, without a GPU.

tests/cxx/wave_source_walk.cpp is compiled as plain C++17 (the csrc and include directories as the only include paths:
the header is HIP-free) into a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer (host code only;
nothing of it is loaded into this process) and prints the bits of window, s1, s1_left_to_right and s2 for every case.
The expected values are the formulas of LinearGLLOpt._window, _boundary_scalars and _s1_fused as of commit a25be7c,
written out below.  The entries of the built library (wf_wave_*, what both front ends call) are held to the same bits.

Grid: three frequencies; speeds 343, 1500 and the first four draws of a seeded search with c0 ** 2 != c0 * c0 (libm's pow
against the product: the Python model passes c0 ** 2); with and without a medium; t = 0, one ulp below, at and one ulp
above period * alpha, and t0 + k dt accumulated as the loops accumulate it with the stage times t + 0.5 dt and t + dt of
every step, from t0 = 0 and from a t0 inside the ramp, through the end of the ramp.
A second, small case passes c0 * c0 and checks s1 against the C++ model's former c0 * c0 * source(t)."""
import math
import os
import subprocess

import numpy as np

from support import wlib  # noqa: F401
from test_op_lists_host import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, P0 = 4.0, 6e4
FREQS = (0.5e6, 1.0e5, 3.3e6)


def window(freq0, t):
    T = 1.0 / freq0
    if t < T * ALPHA:
        return 0.5 * (1.0 - math.cos(freq0 * math.pi * t / ALPHA))
    return 1.0


def expected(c0, c0sq, freq0, medium, t):
    """(window, s1, s1 of rk4_fused, s2) as the Python model formed them; c0sq is the model's c0 ** 2"""
    w0 = 2.0 * math.pi * freq0
    win = window(freq0, t)
    if medium:
        s1 = win * P0 * w0 * math.cos(w0 * t)
        return win, s1, s1, -1.0
    g = win * P0 * w0 / c0 * math.cos(w0 * t)
    return win, c0sq * g, c0sq * win * P0 * w0 / c0 * math.cos(w0 * t), -c0


def odd_speeds(count=4):
    """speeds whose square by libm's pow is not the product, from seeded uniform draws in [300, 6000]"""
    out = []
    for x in np.random.default_rng(36).uniform(300.0, 6000.0, 200000).tolist():
        if x ** 2 != x * x:
            out.append(x)
            if len(out) == count:
                break
    return out


def times(freq0):
    T = 1.0 / freq0
    edge = T * ALPHA
    ts = [0.0, math.nextafter(edge, 0.0), edge, math.nextafter(edge, math.inf), 2.5 * edge]
    dt = 0.013 * T
    for t0, steps in ((0.0, 6), (0.37 * edge, 6), (edge - 3.5 * dt, 6)):
        t = t0
        for _ in range(steps):
            ts += [t, t + 0.5 * dt, t + 1.0 * dt, t + dt]
            t += dt
        ts.append(t)
    return ts


def bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def walk(tmp_path, cases):
    """the program's four words per case, for cases (c0, c0sq, freq0, medium, t)"""
    exe, path = str(tmp_path / "wave_source_walk"), str(tmp_path / "cases.txt")
    subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "wave_fenics_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "wave_source_walk.cpp"), "-o", exe])
    with open(path, "w") as f:
        for c0, c0sq, freq0, medium, t in cases:
            words = [bits(v) for v in (c0, c0sq, P0, 2.0 * math.pi * freq0, freq0, ALPHA, 1.0 / freq0, t)] + [int(medium)]
            f.write(" ".join(f"{int(w):x}" for w in words) + "\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1] == f"{len(cases)} cases", out.stdout[-2000:] + out.stderr[-4000:]
    return [[int(w, 16) for w in line.split()] for line in lines[:-1]]


def library(wlib, case):
    import ctypes
    c0, c0sq, freq0, medium, t = case
    p = wlib.WaveSource(c0, c0sq, P0, 2.0 * math.pi * freq0, freq0, ALPHA, 1.0 / freq0, int(medium))
    L, r = wlib.lib(), ctypes.byref
    return [L.wf_wave_window(r(p), t), L.wf_wave_s1(r(p), t), L.wf_wave_s1_left_to_right(r(p), t), L.wf_wave_s2(r(p))]


def compare(wlib, tmp_path, cases, want):
    got = walk(tmp_path, cases)
    names = ("window", "s1", "s1_left_to_right", "s2")
    for case, g, w in zip(cases, got, want):
        lib_vals = library(wlib, case)
        for name, gb, wv, lv in zip(names, g, w, lib_vals):
            assert gb == int(bits(wv)), (name, case, float(np.array([gb], dtype=np.uint64).view(np.float64)[0]), wv)
            assert int(bits(lv)) == int(bits(wv)), ("library", name, case, lv, wv)


def test_source_scalars_bit_for_bit(wlib, tmp_path):
    odd = odd_speeds()
    assert len(odd) >= 3 and all(x ** 2 != x * x for x in odd), odd
    cases = [(c0, c0 ** 2, f, medium, t) for c0 in [343.0, 1500.0] + odd for f in FREQS for medium in (False, True) for t in times(f)]
    want = [expected(*c) for c in cases]
    # the grid reaches what it is meant to: both sides of the ramp's end, both associations apart somewhere
    assert any(w[0] == 1.0 for w in want) and any(0.0 < w[0] < 1.0 for w in want)
    assert any(w[1] != w[2] for w in want)
    compare(wlib, tmp_path, cases, want)
    print(f"{len(cases)} cases; s1 and s1_left_to_right differ in {sum(w[1] != w[2] for w in want)}; speeds {odd}")


def test_cxx_front_end_s1(wlib, tmp_path):
    """c0_squared = c0 * c0, as the C++ model passes it: s1 is its former c0 * c0 * source(t)"""
    odd = odd_speeds(2)
    cases = [(c0, c0 * c0, f, False, t) for c0 in [1500.0] + odd for f in FREQS[:2] for t in times(f)[:12]]
    want = []
    for c0, _, f, _, t in cases:
        win, _, _, s2 = expected(c0, c0 * c0, f, False, t)
        source = win * P0 * (2.0 * math.pi * f) / c0 * math.cos(2.0 * math.pi * f * t)
        want.append((win, c0 * c0 * source, (c0 * c0) * win * P0 * (2.0 * math.pi * f) / c0 * math.cos(2.0 * math.pi * f * t), s2))
    compare(wlib, tmp_path, cases, want)
