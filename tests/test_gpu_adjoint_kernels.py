"""wf_leapfrog_correlate and wf_sources_add_values (csrc/adjoint.hip) entry by entry against long double, in
sentinel-guarded buffers (guard_helpers), and the C++ wrappers' program against Python bit for bit.

Bounds are derived, not measured; eps = 2^-52, one rounding = eps / 2, the library evaluates as written:

* correlate, p + lam * ((up - 2 u) + um): 2 u is exact; the difference, the sum with um, the product and the sum with p
  round once each -- four roundings, each of a partial result no larger than M = |p| + |lam| (|up| + 2 |u| + |um|):
  |got - ref| <= 4 (eps / 2) M (1 + O(eps)) <= CORRELATE_B eps M with CORRELATE_B = 3, the count of
  leapfrog_helpers.BOUND_PLAIN for the same number of roundings.
* add_values, b + scale * sum_e W_e v_e over the k entries of a dof: W_e = (wx wy) wz is formed by the host merge (two
  roundings against the exact product of the float64 1-D weights the reference takes), each product rounds once, the k
  additions, the product with scale and the addition onto b once each: at most k + 5 roundings on a path, each of a partial
  result no larger than M = |b| + |scale| sum_e |W_e| |v_e|: |got - ref| <= ceil((k + 5) / 2) eps M.
* transpose identity, <sample(x), r> against <x, R^T r> (both products taken in long double from what the device wrote):
  the two sides differ by at most (SAMPLE_B(nd) + max_d ceil((k_d + 5) / 2)) eps sum_r sum_l |W_rl| |x_l| |r_r|."""
import math
import os
import subprocess

import numpy as np
import pytest

import guard_helpers as gh
import points_helpers as ph
from support import EPS, LD, bits, gpu, ratio  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORRELATE_B = 3.0
LENGTHS = [1, 2, 3, 255, 256, 257, 513]
NAMES = ("lam", "up", "u", "um", "p")
PAD = 4096


def correlate_case(n):
    rng = np.random.default_rng(4000 + n)
    return {k: rng.uniform(-1.0, 1.0, n) for k in NAMES}


def correlate_run(gpu, host, shifts):
    """one call in guarded buffers (shifts: name -> 0 / 1); p as the device left it.  Input padding is NaN, so a stray
    read shows in p; p's padding is the smallest normal number, which any store or add changes."""
    import torch
    from wave_fenics_amd import la
    d, g = {}, {}
    for k in NAMES:
        d[k], g[k] = gh.guarded(host[k], PAD, shifts.get(k, 0), gh.MIN_NORMAL if k == "p" else gh.NAN, gpu)
    la.leapfrog_correlate(d["lam"], d["up"], d["u"], d["um"], d["p"])
    torch.cuda.synchronize()
    for k in NAMES:
        assert g[k].intact(), f"padding of {k} changed at {g[k].changed()[:8]}"
        if k != "p":
            assert np.array_equal(bits(d[k].cpu().numpy()), bits(host[k])), f"input {k} was written"
    return d["p"].cpu().numpy()


@pytest.mark.parametrize("n", LENGTHS)
def test_correlate(gpu, n):
    host = correlate_case(n)
    L = {k: host[k].astype(LD) for k in NAMES}
    ref = L["p"] + L["lam"] * ((L["up"] - LD(2.0) * L["u"]) + L["um"])
    mag = np.abs(L["p"]) + np.abs(L["lam"]) * (np.abs(L["up"]) + LD(2.0) * np.abs(L["u"]) + np.abs(L["um"]))
    first = None
    for shift in (0, 1):                                  # 16-byte form, scalar form
        p = correlate_run(gpu, host, {k: shift for k in NAMES})
        worst, ok, where = ratio(p, ref, mag, CORRELATE_B)
        print(f"ADJOINT correlate n={n} shift={shift}: worst |err| / (eps M) = {worst:.3f} (bound {CORRELATE_B})")
        assert ok, f"n={n} shift={shift}: p[{where}] outside its bound"
        first = p if first is None else first
        assert np.array_equal(bits(p), bits(first)), "the 16-byte and the scalar form differ"
    for k in NAMES:                                       # any one operand 8 bytes off: the scalar form, the same bits
        assert np.array_equal(bits(correlate_run(gpu, host, {k: 1})), bits(first)), f"{k} shifted"


@pytest.mark.parametrize("shift", [0, 1])
def test_correlate_beyond_one_grid_stride(gpu, shift):
    """The grid is capped at 2^22 workgroups of 256: with n = 2^31 + 3 every thread of both forms takes a second trip
    (16-byte form: 2^30 + 1 pairs and the odd last dof; scalar form: two full trips and a ragged one) and entry indices
    pass 2^31.  The inputs are four views of one buffer, two doubles apart (they may overlap each other), the reference
    the same four roundings by elementwise device operations, compared bit for bit, padding included."""
    import torch
    from wave_fenics_amd import la
    n, pad = 2 ** 31 + 3, 4096
    gen = torch.Generator(device=gpu)
    gen.manual_seed(5)
    X = torch.empty(n + 8 + shift, dtype=torch.float64, device=gpu)
    X.uniform_(-1.0, 1.0, generator=gen)
    lam, up, u, um = (X[shift + 2 * i:shift + 2 * i + n] for i in range(4))
    Pbuf = torch.full((pad + shift + n + pad,), gh.MIN_NORMAL, dtype=torch.float64, device=gpu)
    p = Pbuf[pad + shift:pad + shift + n]
    p.uniform_(-1.0, 1.0, generator=gen)
    assert p.data_ptr() % 16 == 8 * shift and lam.data_ptr() % 16 == 8 * shift
    ref = torch.sub(up, u, alpha=2.0)                     # 2 u is exact: one rounding with or without contraction
    ref.add_(um).mul_(lam).add_(p)
    xsum = float(X.sum().item())
    la.leapfrog_correlate(lam, up, u, um, p)
    torch.cuda.synchronize()
    same = bool((p.view(torch.int64) == ref.view(torch.int64)).all().item())
    del ref
    assert same, "p differs from the elementwise reference"
    fill = int(np.array([gh.MIN_NORMAL]).view(np.int64)[0])
    assert bool((Pbuf[:pad + shift].view(torch.int64) == fill).all().item()) and bool((Pbuf[pad + shift + n:].view(torch.int64) == fill).all().item())
    assert float(X.sum().item()) == xsum                  # inputs untouched
    del X, Pbuf, p, lam, up, u, um
    torch.cuda.empty_cache()                              # 52 GB back to the device


def test_correlate_refusals_write_nothing(gpu):
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd import la
    from wave_fenics_amd._lib import lib
    from wave_fenics_amd.operators import _ptr
    n = 257
    host = correlate_case(n)
    d = {k: torch.from_numpy(host[k]).to(gpu) for k in NAMES}
    big = torch.from_numpy(np.concatenate([host["p"], host["lam"]])).to(gpu)
    for k in ("lam", "up", "u", "um"):                    # p is an input
        a = dict(d)
        a["p"] = d[k]
        with pytest.raises(w.WavehipError):
            la.leapfrog_correlate(a["lam"], a["up"], a["u"], a["um"], a["p"])
        a = dict(d)                                       # p overlaps an input without being it
        a[k], a["p"] = big[1:n + 1], big[:n]
        with pytest.raises(w.WavehipError):
            la.leapfrog_correlate(a["lam"], a["up"], a["u"], a["um"], a["p"])
    assert b"overlap" in lib().wf_last_error()
    ptr = {k: _ptr(d[k]) for k in NAMES}
    for null in NAMES:
        q = dict(ptr, **{null: 0})
        assert lib().wf_leapfrog_correlate(n, q["lam"], q["up"], q["u"], q["um"], q["p"], 0) != 0
    for nn in (0, -3):
        assert lib().wf_leapfrog_correlate(nn, ptr["lam"], ptr["up"], ptr["u"], ptr["um"], ptr["p"], 0) == 0
    torch.cuda.synchronize()
    for k in NAMES:
        assert np.array_equal(bits(d[k].cpu().numpy()), bits(host[k]))
    assert np.array_equal(bits(big.cpu().numpy()), bits(np.concatenate([host["p"], host["lam"]])))
    la.leapfrog_correlate(d["lam"], d["lam"], d["lam"], d["u"], d["p"])      # inputs may be one vector
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
BOX = {1: (3, 2, 2), 2: (2, 2, 2), 3: (2, 2, 2), 4: (2, 2, 2), 5: (2, 1, 1), 6: (2, 1, 1), 7: (2, 1, 1)}


def points_case(p, npoints):
    """(V, cell, ref): random points; from two points on, point 1 shares the cell of point 0, and from three on point 2 is
    the far vertex of that cell (a node, and a dof that up to eight cells share)"""
    import wave_fenics_amd as w
    V = w.create_functionspace(w.create_box(BOX[p]), p)
    rng = np.random.default_rng(100 * p + npoints)
    cell = rng.integers(0, V.mesh.ncells, npoints).astype(np.int32)
    ref = rng.uniform(0.0, 1.0, (npoints, 3))
    if npoints > 1:
        cell[1] = cell[0]
    if npoints > 2:
        cell[2], ref[2] = cell[0], (1.0, 1.0, 1.0)
    return V, cell, ref


@pytest.mark.parametrize("npoints", [1, 2, 3, 64, 257])
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6, 7])
def test_add_values(gpu, p, npoints):
    import torch
    from wave_fenics_amd import points
    V, cell, ref = points_case(p, npoints)
    src = points.Sources(V, None, [points.ricker(1.0, 0.0, 0.0)] * npoints, located=(cell, ref))
    rec = points.Receivers(V, None, located=(cell, ref))
    assert np.array_equal(src.dofs, rec.dofs) and np.array_equal(src.w, rec.w)
    rng = np.random.default_rng(7 * p + npoints)
    vals, b0, x = rng.uniform(-1, 1, npoints), rng.uniform(-1, 1, V.ndofs), rng.uniform(-1, 1, V.ndofs)
    scale = -2.5
    k = np.bincount(src.dofs.reshape(-1), minlength=V.ndofs)
    B = np.ceil((k + 5) / 2.0)
    touched = k > 0
    if npoints > 2:
        W = ph.tensor_weights(src.w)
        assert np.count_nonzero(W[2]) == 1 and k.max() >= 3          # the node point, and a dof three sources load
    load = ph.source_vector(V.ndofs, src.dofs, src.w, vals, LD)
    mag = ph.source_vector(V.ndofs, src.dofs, np.abs(src.w), np.abs(vals), LD)
    reference = b0.astype(LD) + LD(scale) * load
    first = None
    for shift in (0, 1):
        b, guard = gh.guarded(b0, PAD, shift, gh.MIN_NORMAL, gpu)
        v, vguard = gh.guarded(vals, PAD, shift, gh.NAN, gpu)
        src.add_values(v, b, scale=scale)
        torch.cuda.synchronize()
        assert guard.intact() and vguard.intact()
        got = b.cpu().numpy()
        err = np.abs(got.astype(LD) - reference)
        allowed = B * LD(EPS) * (np.abs(b0).astype(LD) + abs(scale) * mag)
        assert np.all(err[touched] <= allowed[touched]), f"P{p} {npoints} points: dof {np.argmax(err - allowed)} outside its bound"
        assert np.array_equal(bits(got[~touched]), bits(b0[~touched])), "a dof no point touches was written"
        first = got if first is None else first
        assert np.array_equal(bits(got), bits(first))
    worst = float(np.max(err[touched] / (LD(EPS) * (np.abs(b0).astype(LD) + abs(scale) * mag)[touched])))
    print(f"ADJOINT add_values P{p} {npoints} points: worst |err| / (eps M) = {worst:.3f}, bounds {B[touched].min():.0f} .. {B.max():.0f}")
    # scale = 0 adds +0.0: the bits of a non-zero b stay
    b = torch.from_numpy(b0).to(gpu)
    src.add_values(torch.from_numpy(vals).to(gpu), b, scale=0.0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(b.cpu().numpy()), bits(b0))
    # <sample(x), r> = <x, R^T r>
    xd = torch.from_numpy(x).to(gpu)
    g = torch.zeros(V.ndofs, dtype=torch.float64, device=gpu)
    src.add_values(torch.from_numpy(vals).to(gpu), g)
    s = rec.sample(xd)
    torch.cuda.synchronize()
    lhs = (s.cpu().numpy().astype(LD) * vals.astype(LD)).sum()
    rhs = (x.astype(LD) * g.cpu().numpy().astype(LD)).sum()
    Wabs = np.abs(ph.tensor_weights(src.w, LD))
    size = (Wabs * np.abs(x.astype(LD))[src.dofs] * np.abs(vals.astype(LD))[:, None]).sum()
    allowed = (ph.SAMPLE_B((p + 1) ** 3) + B.max()) * LD(EPS) * size
    print(f"ADJOINT transpose P{p} {npoints} points: |<Rx, r> - <x, R^T r>| = {float(abs(lhs - rhs)):.3e}, allowed {float(allowed):.3e}")
    assert abs(lhs - rhs) <= allowed
    src.close()
    rec.close()


def test_add_values_refusals(gpu):
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd import points
    from wave_fenics_amd._lib import lib
    from wave_fenics_amd.operators import _ptr
    V, cell, ref = points_case(2, 3)
    src = points.Sources(V, None, [points.ricker(1.0, 0.0, 0.0)] * 3, located=(cell, ref))
    b = torch.zeros(V.ndofs, dtype=torch.float64, device=gpu)
    v = torch.ones(3, dtype=torch.float64, device=gpu)
    with pytest.raises(w.WavehipError):
        src.add_values(v[:2], b)
    with pytest.raises(w.WavehipError):
        src.add_values(v, b[:-1])
    with pytest.raises(w.WavehipError):
        src.add_values(v, b, scale=float("nan"))
    assert lib().wf_sources_add_values(None, _ptr(v), 1.0, _ptr(b), 0) != 0
    assert lib().wf_sources_add_values(src._s, 0, 1.0, _ptr(b), 0) != 0
    assert lib().wf_sources_add_values(src._s, _ptr(v), 1.0, 0, 0) != 0
    torch.cuda.synchronize()
    assert not bits(b.cpu().numpy()).any()
    T = points.Receivers(V, None, located=(cell, ref)).transpose()
    assert np.array_equal(T.dofs, src.dofs) and np.array_equal(T.w, src.w) and T.num_unique_dofs == src.num_unique_dofs
    T.add(0.3, b)                                         # zero-amplitude wavelets load nothing
    torch.cuda.synchronize()
    assert not np.any(b.cpu().numpy())


def test_cxx_adjoint_bits(gpu, tmp_path):
    """tests/cxx/adjoint_smoke.cpp: Sources::add_values and leapfrog_correlate through the C++ wrapper on a P3 box; every
    entry of b and p against the same calls from Python, bit for bit"""
    import torch
    import wave_fenics_amd as w
    from wave_fenics_amd import la, points
    exe = str(tmp_path / "adjoint_smoke")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "adjoint_smoke.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "wave_fenics_amd"), "-lwavehip",
                           "-Wl,-rpath," + os.path.join(ROOT, "wave_fenics_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {"b": [], "p": []}
    for ln in r.stdout.splitlines():
        f = ln.split()
        if len(f) == 4 and f[2] == "bits":
            assert int(f[1]) == len(got[f[0]])
            got[f[0]].append(int(f[3], 16))
    V = w.create_functionspace(w.create_box((3, 2, 2), hi=(3.0, 2.0, 2.0)), 3)
    N = V.ndofs
    i = np.arange(N, dtype=np.int64)
    f = lambda mul, mod, den, off: torch.from_numpy(((i * mul) % mod) / den - off).to(gpu)    # noqa: E731
    b, lam, up = f(31, 17, 16.0, 0.5), f(7919, 1009, 1024.0, 0.5), f(104729, 1013, 1024.0, 0.25)
    u, um, p = f(1299709, 1019, 1024.0, 0.75), f(15485863, 1021, 1024.0, 0.5), f(611953, 1031, 1024.0, 0.5)
    src = points.Sources(V, [(0.5, 0.25, 0.75), (0.75, 0.5, 0.25), (1.0, 1.0, 1.0)], [points.ricker(1.0, 0.0, 0.0)] * 3)
    assert src.cell[0] == src.cell[1] and math.isclose(float(np.abs(ph.tensor_weights(src.w)[2]).max()), 1.0)
    src.add_values(torch.tensor([0.625, -1.75, 3.0], dtype=torch.float64, device=gpu), b, scale=-2.5)
    la.leapfrog_correlate(lam, up, u, um, p)
    torch.cuda.synchronize()
    for name, t in (("b", b), ("p", p)):
        mine = bits(t.cpu().numpy()).view(np.uint64)
        assert len(got[name]) == N and np.array_equal(mine, np.array(got[name], dtype=np.uint64)), name
    assert np.count_nonzero(b.cpu().numpy() != f(31, 17, 16.0, 0.5).cpu().numpy()) >= 60      # the 64 dofs of cell 0, the node among them
