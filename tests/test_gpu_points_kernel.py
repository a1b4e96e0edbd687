"""wf_points_sample and wf_sources_add on the device against long double (bounds: points_helpers), in guarded buffers.

Sample: P = 1..7 (nd = 8 .. 512: fewer entries than lanes, counts that are no multiple of 64, eight entries per lane),
npoints in {1, 3, 4, 5, 257} (a partial last workgroup, several workgroups), the box numbering and a random renumbering;
points on nodes return x[d] bit for bit; 257 points together equal the same points one at a time, bit for bit.
Add: the same degrees, 1 to 40 sources (8 to > 256 unique dofs), shared dofs, b pre-filled; untouched dofs keep their bits.

Wavelet bounds (eps = 2^-52).  Ricker: arg = pi f (t - delay) rounds three times (pi included), a = arg^2 is within
4.5 eps a, so e^{-a} is within (4.5 a + 2) eps of itself (one more ulp for the library's exp), 1 - 2a within
9 eps a + eps/2 |1 - 2a|; with the two products
    |ds| <= eps |amp| e^{-a} (|1 - 2a| (4.5 a + 4) + 9 a).
Table: u = (t - t_start)/dt is within eps (|t| + |t_start|)/dt + eps u of itself, theta inherits that, and the three operations of the
interpolation round once each: |ds| <= (|v_k| + |v_k+1|) (du + 2 eps) + |v_k+1 - v_k| du."""
import numpy as np
import pytest

import points_helpers as ph
from guard_helpers import MIN_NORMAL, NAN, NEG_ZERO, batch_pad, guarded
from support import EPS, LD, bits, gpu, ratio  # noqa: F401

pytestmark = pytest.mark.gpu

N = (3, 2, 2)
COUNTS = (1, 3, 4, 5, 257)
_SPACE = {}


def space(p, numbering):
    """the perturbed box N at degree p, box numbering or renumbered at random; cached, never changed"""
    key = (p, numbering)
    if key not in _SPACE:
        import wave_fenics_amd as w
        mesh = w.create_box(N, perturb=0.2)
        V = w.create_functionspace(mesh, p)
        if numbering == "renumbered":
            V = w.renumber(V, np.random.default_rng(17 + p).permutation(V.ndofs).astype(np.int32))
        _SPACE[key] = V
    return _SPACE[key]


def random_points(V, count, seed):
    """(cell, ref) of `count` points: random cells, random reference coordinates, a few on faces and edges"""
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, V.mesh.ncells, size=count).astype(np.int32)
    ref = rng.uniform(0.0, 1.0, size=(count, 3))
    ref[rng.uniform(size=(count, 3)) < 0.1] = 1.0
    ref[rng.uniform(size=(count, 3)) < 0.1] = 0.0
    return cell, ref


@pytest.mark.parametrize("numbering", ["box", "renumbered"])
@pytest.mark.parametrize("p", range(1, 8))
def test_sample(gpu, p, numbering):
    import torch
    from wave_fenics_amd import points
    V = space(p, numbering)
    nd = (p + 1) ** 3
    rng = np.random.default_rng(1000 + p)
    x = rng.uniform(-1.0, 1.0, V.ndofs) * 10.0 ** rng.integers(-3, 4, V.ndofs)
    xd, xg = guarded(x, batch_pad(nd), 1, NAN, gpu)
    for count in COUNTS:
        cell, ref = random_points(V, count, 31 * p + count)
        rec = points.Receivers(V, None, located=(cell, ref))
        want, mag = ph.sample_reference(rec.dofs, rec.w, x)
        results = []
        for fill in (NEG_ZERO, MIN_NORMAL):
            big, og = guarded(np.full(count + 7, fill), 4096, 0, fill, gpu)
            out = big[7:]                                   # d_out at an odd offset inside a larger buffer
            rec.sample(xd, out)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert og.intact() and bits(big[:7].cpu().numpy()).tolist() == bits(np.full(7, fill)).tolist()
            worst, ok, at = ratio(got, want, mag, ph.SAMPLE_B(nd))
            assert ok, (p, count, at, worst)
            results.append(got)
        assert np.array_equal(bits(results[0]), bits(results[1])), "a repeat equals itself"
        assert np.array_equal(bits(rec.sample(xd).cpu().numpy()), bits(results[0]))
        print(f"sample P{p} {numbering} npoints {count}: worst |err| / (eps mag) = {worst:.2f} (bound {ph.SAMPLE_B(nd)})")
        if count == 257 and numbering == "box":
            # each point alone gives the bits it gives among 257
            alone = np.array([points.Receivers(V, None, located=(cell[r:r + 1], ref[r:r + 1])).sample(xd).item() for r in range(count)])
            assert np.array_equal(bits(alone), bits(results[0]))
    assert xg.intact()


@pytest.mark.parametrize("p", range(1, 8))
def test_sample_on_nodes_is_exact(gpu, p):
    """points on nodes: out = x[d] bit for bit, for every node of a cell (and so for every lane and iteration)"""
    from wave_fenics_amd import points
    import wave_fenics_amd as w
    V = space(p, "renumbered")
    nodes = w.tabulate_gll(p)[0]
    n = p + 1
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    ref = np.stack([nodes[i.reshape(-1)], nodes[j.reshape(-1)], nodes[k.reshape(-1)]], axis=1)
    cell = np.full(ref.shape[0], 5, dtype=np.int32)
    x = np.random.default_rng(p).uniform(0.5, 2.0, V.ndofs)
    xd, _ = guarded(x, batch_pad(n ** 3), 0, NAN, gpu)
    got = points.Receivers(V, None, located=(cell, ref)).sample(xd).cpu().numpy()
    assert np.array_equal(bits(got), bits(x[V.dofmap[5]]))


def ds_bound(wl, t):
    """|float64 s(t) - exact s(t)| / eps (module docstring)"""
    if wl["kind"] == "ricker":
        a = float((np.pi * wl["frequency"] * (t - wl["delay"])) ** 2)
        return abs(wl["amplitude"]) * float(np.exp(-min(a, 740.0))) * (abs(1 - 2 * a) * (4.5 * a + 4) + 9 * a) + 1e-300 / EPS
    v = wl["values"]
    u = (t - wl["t_start"]) / wl["dt"]
    if not (0.0 <= u <= v.size - 1):
        return 0.0
    k = min(int(u), v.size - 2)
    du = (abs(t) + abs(wl["t_start"])) / wl["dt"] + u
    return (abs(v[k]) + abs(v[k + 1])) * (du + 2) + abs(v[k + 1] - v[k]) * du


def add_reference(V, src, wavelets, t, b):
    """(ref, bound in units of eps) of b after add(t, b), per dof, in long double"""
    W = ph.tensor_weights(src.w, LD)
    s = np.array([ph.wavelet_ld(wl, t) for wl in wavelets], dtype=LD)
    ds = np.array([ds_bound(wl, t) for wl in wavelets], dtype=LD)
    acc, mag, err, cnt = (np.zeros(V.ndofs, dtype=LD) for _ in range(4))
    for i in range(len(wavelets)):
        np.add.at(acc, src.dofs[i], W[i] * s[i])
        np.add.at(mag, src.dofs[i], np.abs(W[i] * s[i]))
        np.add.at(err, src.dofs[i], np.abs(W[i]) * ds[i])
        np.add.at(cnt, src.dofs[i], (W[i] != 0).astype(LD))
    bl = np.asarray(b, dtype=LD)
    # the weight product rounds twice, w * s once, one addition per entry, then the addition onto b
    bound = err + (0.5 * cnt + 2.0) * mag + 0.5 * (np.abs(bl) + mag)
    return bl + acc, bound, cnt > 0


@pytest.mark.parametrize("nsrc", [1, 2, 40])
@pytest.mark.parametrize("p", range(1, 8))
def test_add(gpu, p, nsrc):
    import torch
    from wave_fenics_amd import points
    V = space(p, "renumbered")
    nd = (p + 1) ** 3
    rng = np.random.default_rng(7 * p + nsrc)
    cell, ref = random_points(V, nsrc, 500 + 13 * p + nsrc)
    if nsrc >= 2:
        cell[1], ref[1] = cell[0], ref[0]                 # a duplicate: every dof of source 0 is shared
    wavelets = [points.ricker(2.0 + 0.1 * i, 0.75, 1.0 + i) if i % 2 == 0 else
                points.sampled(rng.uniform(-2.0, 2.0, 5 + i % 3), 0.25, 0.125) for i in range(nsrc)]
    src = points.Sources(V, None, wavelets, located=(cell, ref))
    uniq = np.unique(src.dofs[ph.tensor_weights(src.w) != 0.0]).size
    assert src.num_unique_dofs == uniq
    b0 = rng.uniform(-1.0, 1.0, V.ndofs)
    for t in (0.0, 0.3, 0.5, 0.75, 0.8125, 5.0):        # before, around and far after the Ricker delay; in and off the tables
        want, bound, touched = add_reference(V, src, wavelets, t, b0)
        results = []
        for shift in (0, 1):
            bd, bg = guarded(b0, batch_pad(nd), shift, MIN_NORMAL, gpu)
            src.add(t, bd)
            torch.cuda.synchronize()
            got = bd.cpu().numpy()
            assert bg.intact() and np.isfinite(got).all()
            assert np.array_equal(bits(got[~touched]), bits(b0[~touched])), "dofs no source touches keep their bits"
            worst, ok, at = ratio(got, want, bound, 1.0)
            assert ok, (p, nsrc, t, at, worst)
            results.append(got)
        assert np.array_equal(bits(results[0]), bits(results[1])), "a repeat equals itself"
    print(f"add P{p} {nsrc} sources, {uniq} unique dofs: worst |err| / (eps bound) at the last time = {worst:.3f}")


def test_unique_dof_counts_straddle_a_workgroup(gpu):
    """the cases of test_add cover fewer and more unique dofs than the 256 threads of a workgroup"""
    from wave_fenics_amd import points
    counts = []
    for p, nsrc in ((1, 1), (7, 1), (4, 40)):
        V = space(p, "renumbered")
        cell, ref = random_points(V, nsrc, 500 + 13 * p + nsrc)
        if nsrc == 1:
            ref[0] = (0.3, 0.4, 0.6)                      # inside the cell: all (P+1)^3 weights are non-zero
        src = points.Sources(V, None, [points.ricker(1.0, 0.0)] * nsrc, located=(cell, ref))
        counts.append(src.num_unique_dofs)
    assert counts[0] == 8 and counts[1] == 512 and counts[2] > 256, counts


def test_wavelets_exact_values(gpu):
    """one source on a node (weight exactly 1) onto b = 0: b[d] is s(t) itself.  Ricker: amplitude at the delay, a clean
    +0.0 far after it (a large, e^{-a} underflows), no NaN at a huge time; table: the samples at the nodes, the midpoint
    between two, exact zeros outside."""
    import torch
    from wave_fenics_amd import points
    V = space(2, "box")
    cell, ref = np.array([3], dtype=np.int32), np.array([[0.5, 1.0, 0.0]])
    d = int(V.dofmap[3][1 + 3 * 2 + 0])
    table = [1.0, -2.0, 0.5, 4.0]

    def value(wl, t):
        b = torch.zeros(V.ndofs, dtype=torch.float64, device=gpu)
        points.Sources(V, None, [wl], located=(cell, ref)).add(t, b)
        out = b.cpu().numpy()
        assert np.count_nonzero(out) <= 1 and np.isfinite(out).all()
        return out[d]

    rk = points.ricker(2.0, 0.75, 3.0)
    assert value(rk, 0.75) == 3.0
    for t in (0.75 + 5.0, 1e6, 1e300):
        assert bits(np.array([value(rk, t)]))[0] == 0
    assert abs(value(rk, 0.6) - float(ph.wavelet_ld(rk, 0.6))) <= EPS * ds_bound(rk, 0.6)
    tb = points.sampled(table, 0.25, 0.125)
    for k, v in enumerate(table):
        assert value(tb, 0.25 + 0.125 * k) == v
    assert value(tb, 0.25 + 0.125 * 1.5) == 0.5 * (-2.0) + 0.5 * 0.5
    for t in (0.2499, 0.6251, -1e9, 1e9):
        assert bits(np.array([value(tb, t)]))[0] == 0


@pytest.mark.parametrize("p", [1, 4, 7])
def test_transpose_identity(gpu, p):
    """a . sample(x) = add(.) . x for constant wavelets a_i (two-sample tables): sampling is the transpose of loading.
    Both sides from the device's outputs in long double; bound: the sample bound plus the add bound, times |a_i|"""
    import torch
    from wave_fenics_amd import points
    V = space(p, "renumbered")
    nd = (p + 1) ** 3
    rng = np.random.default_rng(p)
    count = 9
    cell, ref = random_points(V, count, 77 + p)
    a = rng.uniform(-2.0, 2.0, count)
    x = rng.uniform(-1.0, 1.0, V.ndofs)
    xd = torch.from_numpy(x).to(gpu)
    rec = points.Receivers(V, None, located=(cell, ref))
    src = points.Sources(V, None, [points.sampled([ai, ai], 0.0, 1.0) for ai in a], located=(cell, ref))
    b = torch.zeros(V.ndofs, dtype=torch.float64, device=gpu)
    src.add(0.5, b)
    lhs = (a.astype(LD) * rec.sample(xd).cpu().numpy().astype(LD)).sum()
    rhs = (b.cpu().numpy().astype(LD) * x.astype(LD)).sum()
    _, mag = ph.sample_reference(rec.dofs, rec.w, x)
    lim = EPS * (ph.SAMPLE_B(nd) + 0.5 * count + 4.0) * float((np.abs(a) * mag).sum())
    print(f"transpose identity P{p}: |lhs - rhs| = {abs(float(lhs - rhs)):.3e}, limit {lim:.3e}")
    assert abs(lhs - rhs) <= lim


def test_device_refusals(gpu):
    """what needs the plan: wavelet descriptors through the C entry, a vector too short"""
    import ctypes
    from wave_fenics_amd import _lib, points
    V = space(1, "box")
    rec = points.Receivers(V, [(0.5, 0.5, 0.5)])
    L = _lib.lib()
    one = np.zeros(1, dtype=np.int32)
    h = ctypes.c_void_p()
    tab = np.array([1.0, 2.0])
    for nsamples, dt in ((1, 0.1), (2, 0.0), (2, -1.0)):
        wl = _lib.Wavelet(_lib.WF_WAVELET_SAMPLED, 1.0, 0.0, 0.0, nsamples, _lib._dp(tab), 0.0, dt)
        assert L.wf_sources_create(rec._h, 1, _lib._ip(one), ctypes.byref(wl), ctypes.byref(h)) == -1 and not h.value
    one[0] = 1
    wl = _lib.Wavelet(_lib.WF_WAVELET_RICKER, 1.0, 1.0, 0.0, 0, None, 0.0, 0.0)
    assert L.wf_sources_create(rec._h, 1, _lib._ip(one), ctypes.byref(wl), ctypes.byref(h)) == -1
    import torch
    with pytest.raises(_lib.WavehipError):
        rec.sample(torch.zeros(V.ndofs - 1, dtype=torch.float64, device=gpu))
