"""wf_leapfrog4_correlate (csrc/adjoint4.hip, include/wavehip.h) entry by entry against long double, in
sentinel-guarded buffers (guard_helpers), and the C++ wrapper's program against Python bit for bit.

The bound is derived, not measured; eps = 2^-52, one rounding = eps / 2, the library evaluates as written:

* p = (p + lam * ((up - 2 u) + um)) + 12 (om * w): 2 u is exact; the difference, the sum with um, the product with lam,
  the sum with p, the product om w, its product with 12 and the last sum round once each -- seven roundings, each of a
  partial result no larger than M = |p| + |lam| (|up| + 2 |u| + |um|) + 12 |om| |w|:
  |got - ref| <= 7 (eps / 2) M (1 + O(eps)) <= CORRELATE4_B eps M with CORRELATE4_B = 4.
* z = u + w is one rounding of two float64 numbers: numpy's u + w, bit for bit.

No case beyond one grid stride: the loop is sweep<> of csrc/sweep.h, which test_gpu_adjoint_kernels.py walks at
n = 2^31 + 3 through wf_leapfrog_correlate; this kernel adds an entry body only."""
import os
import subprocess

import numpy as np
import pytest

import guard_helpers as gh
from support import LD, bits, gpu, ratio  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORRELATE4_B = 4.0
LENGTHS = [1, 2, 3, 255, 256, 257, 513]
INPUTS = ("lam", "om", "up", "u", "um", "w")
NAMES = INPUTS + ("p", "z")
PAD = 4096
Z_FILL = -7.0                                             # what z holds before the call


def case(n):
    rng = np.random.default_rng(4400 + n)
    host = {k: rng.uniform(-1.0, 1.0, n) for k in INPUTS + ("p",)}
    host["z"] = np.full(n, Z_FILL)
    return host


def run(gpu, host, shifts, with_z=True):
    """one call in guarded buffers (shifts: name -> 0 / 1); (p, z) as the device left them.  Input padding is NaN, so a
    stray read shows in p or z; the padding of p and z is the smallest normal number, which any store or add changes."""
    import torch
    from wave_fenics_amd import la
    d, g = {}, {}
    for k in NAMES:
        d[k], g[k] = gh.guarded(host[k], PAD, shifts.get(k, 0), gh.MIN_NORMAL if k in ("p", "z") else gh.NAN, gpu)
    la.leapfrog4_correlate(d["lam"], d["om"], d["up"], d["u"], d["um"], d["w"], d["p"], d["z"] if with_z else None)
    torch.cuda.synchronize()
    for k in NAMES:
        assert g[k].intact(), f"padding of {k} changed at {g[k].changed()[:8]}"
        if k in INPUTS:
            assert np.array_equal(bits(d[k].cpu().numpy()), bits(host[k])), f"input {k} was written"
    return d["p"].cpu().numpy(), d["z"].cpu().numpy()


@pytest.mark.parametrize("n", LENGTHS)
def test_correlate4(gpu, n):
    host = case(n)
    L = {k: host[k].astype(LD) for k in NAMES}
    ref = (L["p"] + L["lam"] * ((L["up"] - LD(2.0) * L["u"]) + L["um"])) + LD(12.0) * (L["om"] * L["w"])
    mag = (np.abs(L["p"]) + np.abs(L["lam"]) * (np.abs(L["up"]) + LD(2.0) * np.abs(L["u"]) + np.abs(L["um"]))
           + LD(12.0) * np.abs(L["om"]) * np.abs(L["w"]))
    zref = host["u"] + host["w"]
    first = None
    for shift in (0, 1):                                  # 16-byte form, scalar form
        p, z = run(gpu, host, {k: shift for k in NAMES})
        worst, ok, where = ratio(p, ref, mag, CORRELATE4_B)
        print(f"ADJOINT4 correlate n={n} shift={shift}: worst |err| / (eps M) = {worst:.3f} (bound {CORRELATE4_B})")
        assert ok, f"n={n} shift={shift}: p[{where}] outside its bound"
        assert np.array_equal(z, zref) and np.array_equal(bits(z), bits(zref)), "z is not u + w"
        first = p if first is None else first
        assert np.array_equal(bits(p), bits(first)), "the 16-byte and the scalar form differ"
    for k in NAMES:                                       # any one operand 8 bytes off: the scalar form, the same bits
        p, z = run(gpu, host, {k: 1})
        assert np.array_equal(bits(p), bits(first)) and np.array_equal(bits(z), bits(zref)), f"{k} shifted"
    for shifts in ({}, {k: 1 for k in NAMES}, {"z": 1}):  # no z: no store into the vector not handed over, p the same bits
        p, z = run(gpu, host, shifts, with_z=False)
        assert np.array_equal(bits(p), bits(first)), "p differs without z"
        assert np.array_equal(bits(z), bits(host["z"])), "z was written though NULL was passed"


def test_correlate4_refusals_write_nothing(gpu):
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd import la
    from wave_fenics_amd._lib import lib
    from wave_fenics_amd.operators import _ptr
    n = 257
    host = case(n)
    d = {k: torch.from_numpy(host[k]).to(gpu) for k in NAMES}
    big_host = np.concatenate([host["p"], host["lam"]])
    big = torch.from_numpy(big_host).to(gpu)
    call = lambda a: la.leapfrog4_correlate(a["lam"], a["om"], a["up"], a["u"], a["um"], a["w"], a["p"], a["z"])   # noqa: E731
    for out in ("p", "z"):
        for k in INPUTS:
            a = dict(d)                                   # the output is an input
            a[out] = d[k]
            with pytest.raises(w.WavehipError):
                call(a)
            assert b"overlap" in lib().wf_last_error()
            a = dict(d)                                   # the output overlaps an input without being it
            a[k], a[out] = big[1:n + 1], big[:n]
            with pytest.raises(w.WavehipError):
                call(a)
    for a in (dict(d, z=d["p"]), dict(d, p=big[:n], z=big[n - 1:2 * n - 1]), dict(d, z=big[:n], p=big[n - 1:2 * n - 1])):
        with pytest.raises(w.WavehipError):               # p and z overlap each other
            call(a)
        assert b"overlap" in lib().wf_last_error()
    ptr = {k: _ptr(d[k]) for k in NAMES}
    order = lambda q: [q[k] for k in NAMES]               # noqa: E731  (the C argument order)
    for null in INPUTS + ("p",):
        assert lib().wf_leapfrog4_correlate(n, *order(dict(ptr, **{null: 0})), 0) != 0
        assert b"null" in lib().wf_last_error()
    for nn in (0, -3):
        assert lib().wf_leapfrog4_correlate(nn, *order(ptr), 0) == 0
        assert lib().wf_leapfrog4_correlate(nn, *([0] * 8), 0) == 0
    torch.cuda.synchronize()
    for k in NAMES:
        assert np.array_equal(bits(d[k].cpu().numpy()), bits(host[k])), k
    assert np.array_equal(bits(big.cpu().numpy()), bits(big_host))
    a = dict(d, om=d["lam"], up=d["lam"], um=d["lam"], w=d["u"])          # inputs may be one vector
    call(a)
    torch.cuda.synchronize()


def test_cxx_adjoint4_bits(gpu, tmp_path):
    """tests/cxx/adjoint4_smoke.cpp: leapfrog4_correlate through the C++ wrapper with and without z; every entry of p and
    z against the same calls from Python, bit for bit"""
    import torch
    from wave_fenics_amd import la
    exe = str(tmp_path / "adjoint4_smoke")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "adjoint4_smoke.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "wave_fenics_amd"), "-lwavehip",
                           "-Wl,-rpath," + os.path.join(ROOT, "wave_fenics_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {"p": [], "z": [], "q": []}
    for ln in r.stdout.splitlines():
        f = ln.split()
        if len(f) == 4 and f[2] == "bits":
            assert int(f[1]) == len(got[f[0]])
            got[f[0]].append(int(f[3], 16))
    N = 523
    i = np.arange(N, dtype=np.int64)
    f = lambda mul, mod, off: torch.from_numpy(((i * mul) % mod) / 1024.0 - off).to(gpu)    # noqa: E731
    lam, om, up = f(7919, 1009, 0.5), f(31337, 1033, 0.5), f(104729, 1013, 0.25)
    u, um, w, p = f(1299709, 1019, 0.75), f(15485863, 1021, 0.5), f(27644437, 1039, 0.5), f(611953, 1031, 0.5)
    q, z = p.clone(), torch.full_like(p, -1.0)
    la.leapfrog4_correlate(lam, om, up, u, um, w, p, z)
    la.leapfrog4_correlate(lam, om, up, u, um, w, q)
    torch.cuda.synchronize()
    for name, t in (("p", p), ("z", z), ("q", q)):
        mine = bits(t.cpu().numpy()).view(np.uint64)
        assert len(got[name]) == N and np.array_equal(mine, np.array(got[name], dtype=np.uint64)), name
    assert got["p"] == got["q"] and np.array_equal(z.cpu().numpy(), (u + w).cpu().numpy())
