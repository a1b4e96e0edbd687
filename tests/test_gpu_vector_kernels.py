"""Every path of csrc/vector_kernels.hip and the stage and boundary kernels of csrc/time_step.hip, entry by entry, against
numpy in long double.

The streaming kernels of the RK4 loop (fill, copy, axpy, scale, pointwise_div, pointwise_mult_add, dot, the boundary
term, gather / scatter / transform1) and the fused stage `wf_rk4_stage(_bc)` are driven through the C ABI
(wave_fenics_amd.la / .operators) on vectors that live inside padded buffers:

* `Pool.padded(n, shift, fill)`: G + n + G + 1 entries filled with a finite sentinel, the vector is
  buf[G + shift : G + shift + n].  shift = 0 is 16-byte aligned (the 16-byte kernels), shift = 1 only 8-byte aligned
  (the scalar kernels, which nothing else in the suite launches).  After every call `Pool.check` asserts that every
  sentinel of every buffer and every vector that was not an output are bitwise unchanged.
* lengths on both sides of a pair, a 64-dof bitmap word, a wave of pairs (128 dofs) and a workgroup (512 dofs), odd
  and even; the bench vector length (10 218 313, odd) for the stage with a plan, pointwise_div and pointwise_mult_add.

Tolerances are derived, not measured (the library is built without fast-math: division is correctly rounded and the
only freedom of the compiler is contracting a * b + c into one fma).  eps = 2^-52, u = eps / 2:

* one IEEE operation (fill, copy, scale, gather, scatter_set, transform1, pointwise_div): bitwise equal to numpy float64;
* a * b + c (axpy, pointwise_mult_add, the four outputs of the stage): |got - ref| <= 2 eps (|a b| + |c|) per entry,
  ref in long double.  Worst case: the divide kv = b / m, the product and the sum round once each, u each = 1.5 eps
  of that magnitude; 2 eps leaves room for the second-order terms.  The same expressions in plain float64 numpy (no
  fma) reach 1.3 eps (test_reference_headroom, no GPU needed), so the bound holds whichever way the compiler contracts.
  Two float64 evaluations that share the correctly rounded kv (fused against unfused, 16-byte against scalar form, the
  device against torch at full size) are each within 2 u of the exact a * b + c and so within 2 eps of each other;
* the boundary term the stage leaves in b: |got - ref| <= 2 eps (|s1 c1| + |s2 c2 v'|), v' = the vn_next (last stage:
  v_) the device wrote, read back; c1 / c2 by np.add.at in index order (the host loop's order, hence exact); +0.0
  bitwise outside the union of the two sets.  (s2 c2, its product with v', s1 c1 and the sum: at most 3 u.)
  The unfused sequence (pointwise_div, axpy x 2 or 4, fill, BoundaryPlan.apply) is held to the same bounds: its four
  vectors against the fused ones, its b against the reference evaluated from the v' that sequence wrote -- the two
  v' may differ in the last bit, and |s2 c2| times that difference is not an error of the boundary expression;
* sums whose order is free (dot, boundary_apply and scatter_add with repeated indices): small integers / dyadic
  data, every partial sum exact, bitwise equality.

No entry is skipped or masked; the bounds are absolute, so zero entries need no mask.  The worst observed
|got - ref| / (eps * magnitude) per kernel is printed by test_report_worst_ratios (a record; the bound stays 2)."""
import numpy as np
import pytest

from support import EPS, LD, gpu, ratio, relerr  # noqa: F401

gpu_test = pytest.mark.gpu

BOUND = 2.0                      # in units of eps * magnitude
G = 16                           # sentinel entries in front of and behind every vector
SENTINEL = -7.0e77               # finite, so that it compares equal to itself
LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 4097, 100003]
FULL = 10218313                  # the bench vector length (P4, 54^3 cells), odd
BDT, ADT = 2.6180339887e-3, 7.853981634e-3
S1, S2 = 0.8137, -1483.7
WORST = {}                       # kernel -> worst |got - ref| / (eps * magnitude) seen on the device


# ---------------------------------------------------------------------------------------------------------------------
# harness
# ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want):
    return got.shape == want.shape and bool(np.array_equal(bits(got), bits(want)))


class Pool:
    """The device buffers of one kernel call and their expected contents on the host."""

    def __init__(self, device):
        self.device = device
        self.bufs = []

    def padded(self, n, shift, fill, dtype=np.float64):
        import torch
        host = np.full(G + n + G + 1, SENTINEL if dtype == np.float64 else -123456789, dtype=dtype)
        host[G + shift:G + shift + n] = fill
        buf = torch.from_numpy(host).to(self.device)
        view = buf[G + shift:G + shift + n]
        item = host.dtype.itemsize
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (item * shift) % 16 and view.is_contiguous()
        self.bufs.append((buf, host, G + shift, n, view))
        return view

    def check(self, written=()):
        """Sentinels of every buffer and every vector not in `written` are bitwise unchanged; the host copies of the
        written vectors are refreshed, so a later call is checked against what this one left."""
        import torch
        torch.cuda.synchronize()
        out = {v.data_ptr() for v in written}
        for k, (buf, host, lo, n, view) in enumerate(self.bufs):
            got = buf.cpu().numpy()
            pad = np.ones(got.size, dtype=bool)
            pad[lo:lo + n] = False
            assert np.array_equal(bits(got)[pad], bits(host)[pad]), f"buffer {k}: an entry outside [0, n) was written"
            if view.data_ptr() in out:
                host[lo:lo + n] = got[lo:lo + n]
            else:
                assert np.array_equal(bits(got)[lo:lo + n], bits(host)[lo:lo + n]), f"buffer {k}: an input was modified"


def values(rng, n):
    """magnitudes spread over 1e-3 ... 1e3, both signs"""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3.0, 3.0, n)


def divisors(rng, n):
    return rng.uniform(0.5, 2.0, n)


def junk(n):
    return 777.0 + np.arange(n, dtype=np.float64)


def within(kernel, got, ref, mag, what):
    worst, ok, where = ratio(got, ref, mag, BOUND)
    if kernel is not None:
        WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    assert ok, f"{what}: entry {where} is {worst:.3f} eps of its magnitude from the reference (bound {BOUND})"
    return worst


def fma_reference(a, b, c):
    """a * b + c in long double and the magnitude |a b| + |c| of the bound"""
    ab = np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD)
    c = np.asarray(c, dtype=LD)
    return ab + c, np.abs(ab) + np.abs(c)


def alignments(k):
    """all aligned, all shifted by one entry, exactly one operand shifted"""
    return [(0,) * k, (1,) * k] + ([tuple(int(i == j) for i in range(k)) for j in range(k)] if k > 1 else [])


# ---------------------------------------------------------------------------------------------------------------------
# the fused stage: operands, reference, boundary sets
# ---------------------------------------------------------------------------------------------------------------------
LOGICAL = ["b", "m", "vn", "ur", "vr", "u_", "v_", "u0", "v0", "un", "vnn"]
# the vectors that exist in each argument shape, and which arguments share one
PHYS = {"stage0": ["b", "m", "u0", "v0", "u_", "v_"], "later": ["b", "m", "vn", "u_", "v_"],
        "distinct": ["b", "m", "vn", "ur", "vr", "u_", "v_"]}
NEXT = {"stage0": ["un", "vnn"], "later": ["u0", "v0", "un", "vnn"], "distinct": ["u0", "v0", "un", "vnn"]}
ALIAS = {"stage0": {"vn": "v0", "ur": "u0", "vr": "v0"},      # stage 0: u_read = u0, v_read = v0 = vn
         "later": {"ur": "u_", "vr": "v_"},                   # stages 1 to 3: read and written by the same thread
         "distinct": {}}
OUTPUTS = ["u_", "v_", "un", "vnn"]


def stage_names(shape, has_next):
    return PHYS[shape] + (NEXT[shape] if has_next else [])


def stage_host(n, shape, has_next, rng):
    """seeded contents of the vectors of one call; pure outputs start from junk that no reference contains"""
    host = {}
    for k in stage_names(shape, has_next):
        pure_output = k in ("un", "vnn") or (k in ("u_", "v_") and shape != "later")
        host[k] = junk(n) if pure_output else divisors(rng, n) if k == "m" else values(rng, n)
    return host


def logical(vectors, shape):
    """argument name -> vector, following the aliasing of the shape"""
    return {k: vectors[ALIAS[shape].get(k, k)] for k in LOGICAL if ALIAS[shape].get(k, k) in vectors}


def stage_device(pool, host, shape, shift):
    n = host["b"].size
    dev = {k: pool.padded(n, shift[k] if isinstance(shift, dict) else shift, a) for k, a in host.items()}
    return logical(dev, shape)


def stage_reference(dtype, h, bdt, adt, has_next):
    """The stage in `dtype` arithmetic, one operation at a time (numpy does not contract):
    kv = b / m, ku = vn; u_ = ku bdt + u_read, v_ = kv bdt + v_read; un = ku adt + u0, vn_next = kv adt + v0."""
    c = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    kv, ku = c(h["b"]) / c(h["m"]), c(h["vn"])
    out = {"u_": ku * dtype(bdt) + c(h["ur"]), "v_": kv * dtype(bdt) + c(h["vr"])}
    if has_next:
        out["un"] = ku * dtype(adt) + c(h["u0"])
        out["vnn"] = kv * dtype(adt) + c(h["v0"])
    return out


def stage_magnitudes(h, bdt, adt, has_next):
    """|a b| + |c| of each output, in long double"""
    kv, ku = np.abs(np.asarray(h["b"], dtype=LD) / np.asarray(h["m"], dtype=LD)), np.abs(np.asarray(h["vn"], dtype=LD))
    mag = {"u_": ku * LD(abs(bdt)) + np.abs(h["ur"]).astype(LD), "v_": kv * LD(abs(bdt)) + np.abs(h["vr"]).astype(LD)}
    if has_next:
        mag["un"] = ku * LD(abs(adt)) + np.abs(h["u0"]).astype(LD)
        mag["vnn"] = kv * LD(abs(adt)) + np.abs(h["v0"]).astype(LD)
    return mag


SETS = ["ends", "pair_both", "pair_even", "pair_odd", "word_seams", "gamma1_only", "gamma2_only", "mixed", "repeated",
        "one_block", "random30"]
BCS = ["none", "empty"] + SETS


def boundary_set(name, n, rng, dyadic=False):
    """(idx1, m1, idx2, m2) of the named case, intersected with [0, n)"""
    def keep(a):
        a = np.asarray(a, dtype=np.int64)
        return a[(a >= 0) & (a < n)].astype(np.int32)

    e = 2 * ((n // 2) // 2)                  # an even dof in the middle: the pair (e, e + 1) is one 16-byte entry
    if name == "empty":
        i1 = i2 = keep([])
    elif name == "ends":                     # dof n - 1 is the tail entry when n is odd
        i1 = i2 = np.unique(keep([0, n - 1]))
    elif name == "pair_both":
        i1 = i2 = keep([e, e + 1])
    elif name == "pair_even":
        i1 = i2 = keep([e])
    elif name == "pair_odd":                 # the coefficient index must not step
        i1 = i2 = keep([e + 1])
    elif name == "word_seams":               # ends of bitmap words and the seam between two waves of pairs
        i1 = i2 = keep([62, 63, 64, 65, 126, 127, 128, 129])
    elif name == "gamma1_only":
        i1, i2 = keep(np.arange(0, n, 7)), keep([])
    elif name == "gamma2_only":
        i1, i2 = keep([]), keep(np.arange(0, n, 7))
    elif name == "mixed":                    # d % 5: 0 in Gamma_1 only, 1 in both, 2 in Gamma_2 only, 3 and 4 in neither
        d = np.arange(n)
        i1, i2 = keep(d[(d % 5 == 0) | (d % 5 == 1)]), keep(d[(d % 5 == 1) | (d % 5 == 2)])
    elif name == "repeated":                 # repeated inside idx1 and inside idx2, each occurrence with its own mass
        d = [(37 * j + 3) % n for j in range(4)]
        i1 = keep([d[0], d[1], d[0], d[2], d[0], d[3]])
        i2 = keep([d[3], d[3], d[1], d[2], d[1], d[1], d[0]])
    elif name == "one_block":                # one 128-dof block of the vector: every other wave takes the skip path
        lo = 128 * ((n // 128) // 2)
        blk = np.arange(lo, min(lo + 128, n))
        i1, i2 = keep(blk[rng.random(blk.size) < 0.5]), keep(blk[rng.random(blk.size) < 0.5])
    elif name == "random30":                 # many set bits below every dof: the popcount rank
        i1, i2 = keep(np.flatnonzero(rng.random(n) < 0.3)), keep(np.flatnonzero(rng.random(n) < 0.3))
        i1, i2 = rng.permutation(i1).astype(np.int32), rng.permutation(i2).astype(np.int32)
    else:
        raise KeyError(name)
    mass = (lambda k: rng.integers(1, 17, k) / 8.0) if dyadic else (lambda k: rng.uniform(0.1, 3.0, k))
    return i1, mass(i1.size), i2, mass(i2.size)


def plan_reference(idx1, m1, idx2, m2):
    """the union of the two sets in dof order and the coefficient arrays of wf_boundary_create: np.add.at adds in
    index order, as the host loop does"""
    dofs = np.union1d(idx1, idx2).astype(np.int64)
    c1, c2 = np.zeros(dofs.size), np.zeros(dofs.size)
    np.add.at(c1, np.searchsorted(dofs, idx1), m1)
    np.add.at(c2, np.searchsorted(dofs, idx2), m2)
    return dofs, c1, c2


def boundary_term(dtype, c1, c2, s1, s2, vp):
    """s1 c1 + s2 c2 v' one operation at a time in `dtype`, and its magnitude in long double"""
    c = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    ref = dtype(s1) * c(c1) + dtype(s2) * c(c2) * c(vp)
    mag = np.abs(LD(s1) * np.asarray(c1, dtype=LD)) + np.abs(LD(s2) * np.asarray(c2, dtype=LD) * np.asarray(vp, dtype=LD))
    return ref, mag


def check_b(kernel, b, plan_ref, vp, what):
    """b holds the boundary term on the union of the sets (from the v' given) and +0.0 bitwise everywhere else"""
    dofs, c1, c2 = plan_ref
    other = np.ones(b.size, dtype=bool)
    other[dofs] = False
    assert not bits(b)[other].any(), f"{what}: b is not +0.0 outside the boundary sets"
    if dofs.size:
        ref, mag = boundary_term(LD, c1, c2, S1, S2, vp[dofs])
        within(kernel, b[dofs], ref, mag, f"{what}: boundary term in b")


def make_plan(n, sets):
    from wave_fenics_amd import la
    return la.BoundaryPlan(n, *sets)


def call_fused(d, has_next, plan):
    from wave_fenics_amd import la
    kw = dict(u0=d["u0"], v0=d["v0"], un=d["un"], vn_next=d["vnn"]) if has_next else {}
    la.rk4_stage(d["b"], d["m"], d["vn"], d["ur"], d["vr"], d["u_"], d["v_"], BDT, ADT if has_next else 0.0, bc=plan,
                 s1_next=S1, s2=S2, **kw)
    return [d[k] for k in ["b", "u_", "v_"] + (["un", "vnn"] if has_next else [])]


def call_unfused(pool, d, has_next, plan, shift):
    """what the loop runs without the fused kernel: divide, the axpys, zero b, the boundary launch"""
    from wave_fenics_amd import la
    n = d["b"].numel()
    kv = pool.padded(n, shift, junk(n))
    la.pointwise_div(d["b"], d["m"], kv)
    la.axpy(d["u_"], BDT, d["vn"], d["ur"])
    la.axpy(d["v_"], BDT, kv, d["vr"])
    if has_next:
        la.axpy(d["un"], ADT, d["vn"], d["u0"])
        la.axpy(d["vnn"], ADT, kv, d["v0"])
    la.fill(d["b"], 0.0)
    if plan is not None:
        plan.apply(S1, S2, d["vnn"] if has_next else d["v_"], d["b"])
    return [kv] + [d[k] for k in ["b", "u_", "v_"] + (["un", "vnn"] if has_next else [])]


def read(d, has_next):
    return {k: d[k].cpu().numpy() for k in ["b", "u_", "v_"] + (["un", "vnn"] if has_next else [])}


def run_stage_case(gpu, n, bc, shape, has_next, shift, seed, unfused=True):
    """One fused call against the long double reference (and the unfused sequence); returns what the device wrote."""
    rng = np.random.default_rng(seed)
    host = stage_host(n, shape, has_next, rng)
    h = logical(host, shape)
    ref, mag = stage_reference(LD, h, BDT, ADT, has_next), stage_magnitudes(h, BDT, ADT, has_next)
    sets = None if bc == "none" else boundary_set(bc, n, rng)
    plan = None if sets is None else make_plan(n, sets)
    plan_ref = plan_reference(*sets) if sets is not None else (np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0))
    form = ("vec2" if shift == 0 else "vec1") + ("_next" if has_next else "") + ("_bc" if plan_ref[0].size else "")
    what = f"n={n} bc={bc} {shape} has_next={has_next} shift={shift}"
    pool = Pool(gpu)
    d = stage_device(pool, host, shape, shift)
    pool.check(written=call_fused(d, has_next, plan))
    got = read(d, has_next)
    for k in ref:
        within("rk4_stage<" + form + ">", got[k], ref[k], mag[k], f"{what}: {k}")
    check_b("rk4_stage<" + form + "> b", got["b"], plan_ref, got["vnn" if has_next else "v_"], what)
    if unfused:
        pool2 = Pool(gpu)
        d2 = stage_device(pool2, host, shape, shift)
        pool2.check(written=call_unfused(pool2, d2, has_next, plan, shift if isinstance(shift, int) else 0))
        got2 = read(d2, has_next)
        for k in ref:
            within(None, got2[k], got[k], mag[k], f"{what}: unfused {k} against the fused call")
        check_b("boundary_apply_plan", got2["b"], plan_ref, got2["vnn" if has_next else "v_"], what + " unfused")
    if plan is not None:
        plan.close()
    return got


# ---------------------------------------------------------------------------------------------------------------------
# no GPU: the reference's own error, so the headroom under the bound is pinned
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_headroom():
    """The module's stage reference and boundary term in plain float64 (three roundings, no fma) against long double
    over every length, shape and boundary set: the worst ratio (expected near 1.3) must stay under the bound of 2."""
    worst = {"stage": 0.0, "boundary term": 0.0}
    for n in LENGTHS:
        for shape in PHYS:
            for has_next in (0, 1):
                rng = np.random.default_rng(1000 * n + has_next)
                h = logical(stage_host(n, shape, has_next, rng), shape)
                lo, hi = stage_reference(np.float64, h, BDT, ADT, has_next), stage_reference(LD, h, BDT, ADT, has_next)
                mag = stage_magnitudes(h, BDT, ADT, has_next)
                for k in hi:
                    r, ok, where = ratio(lo[k], hi[k], mag[k], BOUND)
                    assert ok, (n, shape, has_next, k, where, r)
                    worst["stage"] = max(worst["stage"], r)
        for name in SETS:
            rng = np.random.default_rng(7 * n)
            dofs, c1, c2 = plan_reference(*boundary_set(name, n, rng))
            vp = values(rng, dofs.size)
            lo, _ = boundary_term(np.float64, c1, c2, S1, S2, vp)
            hi, mag = boundary_term(LD, c1, c2, S1, S2, vp)
            r, ok, where = ratio(lo, hi, mag, BOUND)
            assert ok, (n, name, where, r)
            worst["boundary term"] = max(worst["boundary term"], r)
    for k, r in worst.items():
        print(f"float64 numpy against long double, {k}: worst |error| = {r:.3f} eps of the magnitude (bound {BOUND})")
        assert 0.0 < r <= BOUND


def test_boundary_sets_hit_the_cases_they_name():
    """the index sets are what their names promise at the lengths where the case exists"""
    rng = np.random.default_rng(0)
    for n in LENGTHS:
        for name in SETS + ["empty"]:
            i1, m1, i2, m2 = boundary_set(name, n, rng)
            assert i1.size == m1.size and i2.size == m2.size
            assert all(((0 <= i) & (i < n)).all() for i in (i1, i2))
        if n >= 3:
            assert boundary_set("pair_odd", n, rng)[0][0] % 2 == 1 and boundary_set("pair_even", n, rng)[0][0] % 2 == 0
            assert boundary_set("ends", n, rng)[0].tolist() == [0, n - 1]
        if n >= 129:
            i1, _, i2, _ = boundary_set("repeated", n, rng)
            assert np.unique(i1).size < i1.size and np.unique(i2).size < i2.size
            assert boundary_set("word_seams", n, rng)[0].size >= 7
        if n >= 4097:
            i1, _, i2, _ = boundary_set("one_block", n, rng)
            assert i1.size and i2.size and len({int(d) // 128 for d in np.concatenate([i1, i2])}) == 1
    dofs, c1, c2 = plan_reference(np.array([5, 2, 5]), np.array([1.0, 2.0, 4.0]), np.array([9, 5]), np.array([8.0, 16.0]))
    assert dofs.tolist() == [2, 5, 9] and c1.tolist() == [2.0, 5.0, 0.0] and c2.tolist() == [0.0, 16.0, 8.0]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: one IEEE operation per entry, bitwise
# ---------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("n", LENGTHS)
def test_fill_copy_scale(gpu, n):
    """k_fill2 / k_fill, hipMemcpy, k_scale2 / k_scale; also over the first n - 1 entries of a longer vector"""
    from wave_fenics_amd import la
    rng = np.random.default_rng(n)
    a = values(rng, n)
    for shift in (0, 1):
        for m in sorted({n, max(n - 1, 1)}):
            pool = Pool(gpu)
            x = pool.padded(n, shift, a)
            la.fill(x, 2.5, m)
            pool.check(written=[x])
            want = a.copy()
            want[:m] = 2.5
            assert same_bits(x.cpu().numpy(), want), ("fill", n, m, shift)
            x = pool.padded(n, shift, a)
            la.scale(-0.37, x, m)
            pool.check(written=[x])
            want = a.copy()
            want[:m] = a[:m] * -0.37
            assert same_bits(x.cpu().numpy(), want), ("scale", n, m, shift)
        for sx, sy in alignments(2):
            pool = Pool(gpu)
            x, y = pool.padded(n, sx, a), pool.padded(n, sy, junk(n))
            la.copy(x, y)
            pool.check(written=[y])
            assert same_bits(y.cpu().numpy(), a), ("copy", n, sx, sy)


@gpu_test
@pytest.mark.parametrize("n", LENGTHS)
def test_pointwise_div(gpu, n):
    """k_div2 (all operands 16-byte aligned and distinct) and k_div (anything else): correctly rounded division"""
    from wave_fenics_amd import la
    rng = np.random.default_rng(n + 1)
    b, m = values(rng, n), divisors(rng, n)
    for sb, sm, so in alignments(3):
        pool = Pool(gpu)
        db, dm, out = pool.padded(n, sb, b), pool.padded(n, sm, m), pool.padded(n, so, junk(n))
        la.pointwise_div(db, dm, out)
        pool.check(written=[out])
        assert same_bits(out.cpu().numpy(), b / m), ("div", n, sb, sm, so)
    for shift in (0, 1):                     # out aliasing an input: the scalar form, every thread reads before it writes
        for alias in ("b", "m"):
            pool = Pool(gpu)
            db, dm = pool.padded(n, shift, b), pool.padded(n, shift, m)
            out = db if alias == "b" else dm
            la.pointwise_div(db, dm, out)
            pool.check(written=[out])
            assert same_bits(out.cpu().numpy(), b / m), ("div in place", n, alias, shift)


@gpu_test
@pytest.mark.parametrize("n", LENGTHS)
def test_gather_scatter_set_transform1(gpu, n):
    from wave_fenics_amd import operators as ops
    rng = np.random.default_rng(n + 2)
    nin = n + 5
    a, dj = values(rng, nin), divisors(rng, n)
    idx = rng.integers(0, nin, n).astype(np.int32)                # gather: repeats allowed
    perm = rng.permutation(nin)[:n].astype(np.int32)              # scatter_set: distinct targets
    for si, sa, so in alignments(3):
        pool = Pool(gpu)
        di, src, out = pool.padded(n, si, idx, np.int32), pool.padded(nin, sa, a), pool.padded(n, so, junk(n))
        ops.gather(n, di, src, out)
        pool.check(written=[out])
        assert same_bits(out.cpu().numpy(), a[idx]), ("gather", n, si, sa, so)
        pool = Pool(gpu)
        di, src, out = pool.padded(n, si, perm, np.int32), pool.padded(n, sa, a[:n]), pool.padded(nin, so, junk(nin))
        ops.scatter_set(n, di, src, out)
        pool.check(written=[out])
        want = junk(nin)
        want[perm] = a[:n]
        assert same_bits(out.cpu().numpy(), want), ("scatter_set", n, si, sa, so)
        pool = Pool(gpu)
        src, det, out = pool.padded(n, si, a[:n]), pool.padded(n, sa, dj), pool.padded(n, so, junk(n))
        ops.transform1(n, src, det, out)
        pool.check(written=[out])
        assert same_bits(out.cpu().numpy(), a[:n] * dj), ("transform1", n, si, sa, so)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: a * b + c per entry
# ---------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("n", LENGTHS)
def test_axpy(gpu, n):
    """k_axpy2 / k_axpy: r = x alpha + y, r a vector of its own or aliasing y (LinearGLL.hpp:253) or x"""
    from wave_fenics_amd import la
    rng = np.random.default_rng(n + 3)
    a, b, alpha = values(rng, n), values(rng, n), 0.37
    ref, mag = fma_reference(a, alpha, b)
    worst = 0.0
    for sx, sy, sr in alignments(3):
        pool = Pool(gpu)
        x, y, r = pool.padded(n, sx, a), pool.padded(n, sy, b), pool.padded(n, sr, junk(n))
        la.axpy(r, alpha, x, y)
        pool.check(written=[r])
        worst = max(worst, within("axpy2" if sx + sy + sr == 0 and n > 1 else "axpy", r.cpu().numpy(), ref, mag,
                                  f"axpy n={n} shifts {sx}{sy}{sr}"))
    for shift in (0, 1):
        for alias in ("y", "x"):
            pool = Pool(gpu)
            x, y = pool.padded(n, shift, a), pool.padded(n, shift, b)
            r = y if alias == "y" else x
            la.axpy(r, alpha, x, y)
            pool.check(written=[r])
            worst = max(worst, within("axpy2" if shift == 0 and n > 1 else "axpy", r.cpu().numpy(), ref, mag,
                                      f"axpy n={n} r = {alias} shift {shift}"))
    m = max(n - 1, 1)                        # the first n - 1 entries only (size_local of a vector with ghosts)
    for shift in (0, 1):
        pool = Pool(gpu)
        x, y, r = pool.padded(n, shift, a), pool.padded(n, shift, b), pool.padded(n, shift, junk(n))
        la.axpy(r, alpha, x, y, m)
        pool.check(written=[r])
        got = r.cpu().numpy()
        within("axpy", got[:m], ref[:m], mag[:m], f"axpy n={n} over {m} entries")
        assert same_bits(got[m:], junk(n)[m:])
    print(f"axpy n={n}: worst {worst:.3f} eps of |alpha x| + |y|")


@gpu_test
@pytest.mark.parametrize("n", LENGTHS)
def test_pointwise_mult_add(gpu, n):
    """k_mult_add2 / k_mult_add (the whole structured lumped mass apply): y += m x"""
    from wave_fenics_amd import la
    rng = np.random.default_rng(n + 4)
    m, a, b = divisors(rng, n), values(rng, n), values(rng, n)
    ref, mag = fma_reference(m, a, b)
    worst = 0.0
    for sm, sx, sy in alignments(3):
        pool = Pool(gpu)
        dm, x, y = pool.padded(n, sm, m), pool.padded(n, sx, a), pool.padded(n, sy, b)
        la.pointwise_mult_add(dm, x, y)
        pool.check(written=[y])
        worst = max(worst, within("mult_add2" if sm + sx + sy == 0 and n > 1 else "mult_add", y.cpu().numpy(), ref, mag,
                                  f"mult_add n={n} shifts {sm}{sx}{sy}"))
    for shift in (0, 1):                     # y aliasing x or m: the scalar form
        pool = Pool(gpu)
        dm, y = pool.padded(n, shift, m), pool.padded(n, shift, a)
        la.pointwise_mult_add(dm, y, y)
        pool.check(written=[y])
        r2, g2 = fma_reference(m, a, a)
        worst = max(worst, within("mult_add", y.cpu().numpy(), r2, g2, f"mult_add n={n} y = x shift {shift}"))
        pool = Pool(gpu)
        y, x = pool.padded(n, shift, m), pool.padded(n, shift, a)
        la.pointwise_mult_add(y, x, y)
        pool.check(written=[y])
        r3, g3 = fma_reference(m, a, m)
        worst = max(worst, within("mult_add", y.cpu().numpy(), r3, g3, f"mult_add n={n} y = m shift {shift}"))
    print(f"pointwise_mult_add n={n}: worst {worst:.3f} eps of |m x| + |y|")


# ---------------------------------------------------------------------------------------------------------------------
# GPU: sums whose order is free, on data that makes every partial sum exact
# ---------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("n", LENGTHS + [2048 * 256 * 3 + 17])
def test_dot_exact(gpu, n):
    """k_dot: its grid is capped at 2048 workgroups of 256, so the last length makes three trips and a ragged one.
    Integers in [-8, 8]: every partial sum is an integer below 2^53.  The vectors are longer than n; the entries
    behind n would change the result by at least 2^20 if they were read."""
    from wave_fenics_amd import la
    rng = np.random.default_rng(n + 5)
    a, b = rng.integers(-8, 9, n + 3).astype(np.float64), rng.integers(-8, 9, n + 3).astype(np.float64)
    a[n:], b[n:] = 2.0 ** 10, 2.0 ** 10
    want = float(np.dot(a[:n].astype(np.int64), b[:n].astype(np.int64)))
    for sx, sy in alignments(2):
        pool = Pool(gpu)
        x, y = pool.padded(n + 3, sx, a), pool.padded(n + 3, sy, b)
        got = la.inner_product(x, y, n)
        pool.check()
        assert got == want, (n, sx, sy, got, want)


@gpu_test
@pytest.mark.parametrize("n", LENGTHS)
def test_scatter_add_repeated_indices(gpu, n):
    """k_scatter_add with targets hit several times: multiples of 1/8, sums exact in any order"""
    from wave_fenics_amd import operators as ops
    rng = np.random.default_rng(n + 6)
    nout = max(n // 3, 1)
    idx = rng.integers(0, nout, n).astype(np.int32)
    a, y0 = rng.integers(-64, 65, n) / 8.0, rng.integers(-64, 65, nout) / 8.0
    want = y0.copy()
    np.add.at(want, idx, a)
    for si, sa, so in alignments(3):
        pool = Pool(gpu)
        di, src, out = pool.padded(n, si, idx, np.int32), pool.padded(n, sa, a), pool.padded(nout, so, y0)
        ops.scatter(n, di, src, out)
        pool.check(written=[out])
        assert np.array_equal(out.cpu().numpy(), want), ("scatter_add", n, si, sa, so)


@gpu_test
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", SETS)
def test_boundary_apply_exact(gpu, name, n):
    """k_boundary through BoundaryPlan.apply (wf_boundary_apply_plan) and through la.boundary_apply on the same
    sets: b[idx1] += s1 m1, b[idx2] += s2 m2 v[idx2] with dyadic data (masses k / 8, s1 = 0.75, s2 = -1.5, integer
    v and b), so that repeated indices add up exactly in any order: both equal the numpy sum bitwise."""
    from wave_fenics_amd import la
    rng = np.random.default_rng(31 * n + 7)
    i1, m1, i2, m2 = boundary_set(name, n, rng, dyadic=True)
    v, b0 = rng.integers(-8, 9, n).astype(np.float64), rng.integers(-8, 9, n).astype(np.float64)
    s1, s2 = 0.75, -1.5
    want = b0.copy()
    np.add.at(want, i1, s1 * m1)
    np.add.at(want, i2, s2 * m2 * v[i2])
    plan = make_plan(n, (i1, m1, i2, m2))
    for sv, sb in alignments(2):
        pool = Pool(gpu)
        dv, db = pool.padded(n, sv, v), pool.padded(n, sb, b0)
        plan.apply(s1, s2, dv, db)
        pool.check(written=[db])
        assert same_bits(db.cpu().numpy(), want), ("BoundaryPlan.apply", name, n, sv, sb)
        pool = Pool(gpu)
        dv, db = pool.padded(n, sv, v), pool.padded(n, sb, b0)
        idx = [pool.padded(i.size, s, i, np.int32) if i.size else None for i, s in ((i1, sv), (i2, sb))]
        mass = [pool.padded(m.size, s, m) if m.size else None for m, s in ((m1, sb), (m2, sv))]
        la.boundary_apply(idx[0], mass[0], s1, idx[1], mass[1], s2, dv, db)
        pool.check(written=[db])
        assert same_bits(db.cpu().numpy(), want), ("la.boundary_apply", name, n, sv, sb)
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the fused stage
# ---------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("bc", BCS)
def test_rk4_stage(gpu, bc, n):
    """has_next x the two argument shapes of the loop x all operands aligned / all shifted by one entry: the four
    outputs against long double, b against the boundary term of the v' the device wrote (none / empty: all +0.0),
    sentinels and inputs untouched, and the unfused sequence against the fused call."""
    worst = 0.0
    for shape in ("stage0", "later"):
        for has_next in (0, 1):
            for shift in (0, 1):
                run_stage_case(gpu, n, bc, shape, has_next, shift, seed=100 * n + 10 * has_next + shift)
    for k, r in WORST.items():
        if k.startswith("rk4_stage"):
            worst = max(worst, r)
    print(f"rk4_stage n={n} bc={bc}: worst so far over the stage kernels {worst:.3f} eps of the magnitude")


ONE_SHIFTED = [(1, k) for k in stage_names("distinct", 1)] + [(0, k) for k in stage_names("distinct", 0)]


@gpu_test
@pytest.mark.parametrize("has_next,operand", ONE_SHIFTED, ids=[f"next{h}-{k}" for h, k in ONE_SHIFTED])
@pytest.mark.parametrize("bc", ["none", "random30"])
@pytest.mark.parametrize("n", [65, 257])
def test_rk4_stage_one_operand_shifted(gpu, n, bc, has_next, operand):
    """The host picks the 16-byte kernel only if every pointer it passes is 16-byte aligned, one term per pointer:
    with any single operand 8 bytes off the scalar kernel runs, and gives what the 16-byte kernel gives."""
    seed = 7000 + n
    shift = {k: int(k == operand) for k in stage_names("distinct", has_next)}
    got = run_stage_case(gpu, n, bc, "distinct", has_next, shift, seed, unfused=False)
    aligned = run_stage_case(gpu, n, bc, "distinct", has_next, 0, seed, unfused=False)
    rng = np.random.default_rng(seed)
    h = logical(stage_host(n, "distinct", has_next, rng), "distinct")
    mag = stage_magnitudes(h, BDT, ADT, has_next)
    for k in mag:
        within(None, got[k], aligned[k], mag[k], f"n={n} bc={bc} {operand} shifted: {k} against the 16-byte kernel")


@gpu_test
@pytest.mark.parametrize("shift", [0, 1])
def test_rk4_stage_refuses_aliased_vn_next(gpu, shift):
    """vn_next == vn would let a thread's neighbour read what it wrote: refused, nothing touched"""
    import wave_fenics_amd as w
    n = 257
    rng = np.random.default_rng(5)
    host = stage_host(n, "distinct", 1, rng)
    for bc in ("none", "random30"):
        pool = Pool(gpu)
        d = stage_device(pool, host, "distinct", shift)
        d["vnn"] = d["vn"]
        plan = None if bc == "none" else make_plan(n, boundary_set(bc, n, rng))
        with pytest.raises(w.WavehipError):
            call_fused(d, 1, plan)
        pool.check()
    pool = Pool(gpu)                         # a plan built for another vector length
    d = stage_device(pool, host, "distinct", shift)
    with pytest.raises(w.WavehipError):
        call_fused(d, 1, make_plan(n + 1, boundary_set("ends", n + 1, rng)))
    pool.check()


@gpu_test
@pytest.mark.parametrize("shift", [0, 1])
def test_full_size(gpu, shift):
    """The bench vector length: the stage with a plan (30 % of the dofs in each set), pointwise_div and
    pointwise_mult_add against the same expressions evaluated by torch in float64 on the device, one operation at a
    time.  Both sides share the correctly rounded kv and are within 2 u of the exact a b + c, so within 2 eps of
    each other; the division is bitwise."""
    import torch
    from wave_fenics_amd import la
    n = FULL
    rng = np.random.default_rng(99 + shift)
    host = stage_host(n, "later", 1, rng)
    sets = boundary_set("random30", n, rng)
    dofs, c1, c2 = plan_reference(*sets)
    plan = make_plan(n, sets)
    pool = Pool(gpu)
    d = stage_device(pool, host, "later", shift)
    t = {k: torch.from_numpy(a).to(gpu) for k, a in logical(host, "later").items()}
    kv = t["b"] / t["m"]
    ref = {"u_": t["vn"] * BDT + t["ur"], "v_": kv * BDT + t["vr"], "un": t["vn"] * ADT + t["u0"], "vnn": kv * ADT + t["v0"]}
    mag = {"u_": (t["vn"] * BDT).abs() + t["ur"].abs(), "v_": (kv * BDT).abs() + t["vr"].abs(),
           "un": (t["vn"] * ADT).abs() + t["u0"].abs(), "vnn": (kv * ADT).abs() + t["v0"].abs()}
    pool.check(written=call_fused(d, 1, plan))
    for k in ref:
        err = (d[k] - ref[k]).abs()
        assert bool((err <= BOUND * EPS * mag[k]).all()), (k, float((err / (EPS * mag[k])).max()))
        print(f"full size shift {shift}: {k} against torch, worst {float((err / (EPS * mag[k])).max()):.3f} eps")
    idx = torch.from_numpy(dofs).to(gpu)
    t1, t2 = S1 * torch.from_numpy(c1).to(gpu), S2 * torch.from_numpy(c2).to(gpu) * d["vnn"][idx]
    err = (d["b"][idx] - (t1 + t2)).abs()
    bmag = t1.abs() + t2.abs()
    assert bool((err <= BOUND * EPS * bmag).all()), float((err / (EPS * bmag)).max())
    print(f"full size shift {shift}: boundary term against torch, worst {float((err / (EPS * bmag)).max()):.3f} eps")
    other = torch.ones(n, dtype=torch.bool, device=gpu)
    other[idx] = False
    assert not bool(d["b"].view(torch.int64)[other].any()), "b is not +0.0 outside the boundary sets"
    plan.close()
    del pool, d, ref, mag, t1, t2, err, bmag
    pool = Pool(gpu)
    b, m, out = pool.padded(n, shift, host["b"]), pool.padded(n, shift, host["m"]), pool.padded(n, shift, 777.0)
    la.pointwise_div(b, m, out)
    pool.check(written=[out])
    assert torch.equal(out, t["b"] / t["m"])
    y = pool.padded(n, shift, host["vn"])
    la.pointwise_mult_add(m, b, y)
    pool.check(written=[y])
    prod = t["m"] * t["b"]
    err = (y - (prod + t["vn"])).abs()
    ymag = prod.abs() + t["vn"].abs()
    assert bool((err <= BOUND * EPS * ymag).all()), float((err / (EPS * ymag)).max())
    print(f"full size shift {shift}: pointwise_mult_add against torch, worst {float((err / (EPS * ymag)).max()):.3f} eps")


# ---------------------------------------------------------------------------------------------------------------------
# GPU: operators on vectors that are only 8-byte aligned
# ---------------------------------------------------------------------------------------------------------------------


def apply_shifted(op, x, y0, gpu):
    """y += A x with x and y both one entry off 16-byte alignment inside padded buffers, y non-zero on entry"""
    pool = Pool(gpu)
    dx, dy = pool.padded(x.size, 1, x), pool.padded(y0.size, 1, y0)
    op(dx, dy)
    pool.check(written=[dy])
    return dy.cpu().numpy()


def box(oracle, n, p, perturb):
    import wave_fenics_amd as w
    om = oracle.create_box(n, p, perturb=perturb)
    mesh = w.create_box(n, perturb=perturb)
    V = w.create_functionspace(mesh, p)
    assert np.array_equal(V.dofmap, om.dofmap) and np.array_equal(mesh.x, om.x)
    return om, V


@gpu_test
@pytest.mark.parametrize("structured", [True, False])
@pytest.mark.parametrize("kind", ["lumped", "spectral"])
@pytest.mark.parametrize("p,n", [(2, (4, 3, 3)), (4, (3, 2, 2))])
def test_mass_on_8_byte_aligned_vectors(gpu, oracle, p, n, kind, structured):
    """the pre-assembled diagonal through k_mult_add, the scalar form (1e-13 of max|y| as test_lumped_mass_vs_oracle)"""
    import wave_fenics_amd as w
    om, V = box(oracle, n, p, 0.2)
    rng = np.random.default_rng(5)
    x, y0 = rng.uniform(-1, 1, om.ndofs), rng.uniform(-1, 1, om.ndofs)
    yref = y0.copy()
    oracle.MassOperatorCPU(om, p)(x, yref)
    op = (w.MassOperatorLumped if kind == "lumped" else w.SpectralMassOperator)(V, p, structured=structured)
    assert op.kernel == "diagonal" and op.info.structured == int(structured)
    err = relerr(apply_shifted(op, x, y0, gpu), yref)
    print(f"{kind} mass P{p} structured={structured}, x and y 8-byte aligned: {err:.3e}")
    assert err <= 1e-13


STIFFNESS_FORMS = {   # request -> (kernel, geometry, update) the operator must report
    "P2_default": (2, {}, ("march_box", "per_cell", "atomic")),
    "P4_default": (4, {}, ("march_box", "per_cell", "owner")),
    "P6_default": (6, {}, ("march_box", "per_point", "none")),          # the k-split kernel
    "P6_owner": (6, {"update": "owner"}, ("march_box", "per_cell", "owner")),
}


@gpu_test
@pytest.mark.parametrize("case", list(STIFFNESS_FORMS))
def test_box_stiffness_on_8_byte_aligned_vectors(gpu, oracle, case):
    """every box form on a small rectilinear box (1e-12 of max|y|, the tolerance of their own parity tests)"""
    import wave_fenics_amd as w
    p, tuning, form = STIFFNESS_FORMS[case]
    n = (5, 4, 3)
    om = oracle.create_box(n, p, hi=(1.0, 0.7, 1.3))
    V = w.create_functionspace(w.create_box(n, hi=(1.0, 0.7, 1.3)), p)
    assert np.array_equal(V.mesh.x, om.x)
    rng = np.random.default_rng(p)
    x, y0 = rng.uniform(-1, 1, om.ndofs), rng.uniform(-1, 1, om.ndofs) * 1e6
    yref = y0.copy()
    oracle.StiffnessOperator(om, p)(x, yref)
    op = w.StiffnessOperator(V, p, {"c0": 1500.0}, structured=True, tuning=tuning or None)
    assert (op.kernel, op.geometry, op.update) == form
    err = relerr(apply_shifted(op, x, y0, gpu), yref)
    print(f"{case}, x and y 8-byte aligned: {err:.3e}")
    assert err <= 1e-12


@gpu_test
@pytest.mark.parametrize("hint,kernel", [("march", "march_idx"), ("batch", "batch_unique")])
def test_generic_stiffness_on_8_byte_aligned_vectors(gpu, oracle, hint, kernel):
    import wave_fenics_amd as w
    p, n = 3, (4, 3, 3)
    om, V = box(oracle, n, p, 0.2)
    rng = np.random.default_rng(1234)
    x, y0 = rng.uniform(-1, 1, om.ndofs), rng.uniform(-1, 1, om.ndofs) * 1e6
    yref = y0.copy()
    oracle.StiffnessOperator(om, p)(x, yref)
    op = w.StiffnessOperator(V, p, {"c0": 1500.0}, structured=False, tuning={"kernel": hint})
    assert op.kernel == kernel
    err = relerr(apply_shifted(op, x, y0, gpu), yref)
    print(f"generic stiffness P{p} {kernel}, x and y 8-byte aligned: {err:.3e}")
    assert err <= 1e-12


@gpu_test
def test_dense_mass_on_8_byte_aligned_vectors(gpu, oracle):
    import wave_fenics_amd as w
    p, n = 2, (3, 2, 4)
    om, V = box(oracle, n, p, 0.2)
    pts, wts, phi1, phi, X, W = oracle.tabulate_mass_tables(p, "equispaced", "gauss_jacobi", 2 * p)
    detJ = oracle.compute_detJ_generic(om, X, W)
    rng = np.random.default_rng(11)
    x, y0 = rng.uniform(-1, 1, om.ndofs), rng.uniform(-1, 1, om.ndofs)
    yref = y0.copy()
    oracle.dense_mass_apply(om, phi, detJ, x, yref)
    op = w.MassOperator(V, p, phi1, detJ, tuning={"kernel": "march"})
    assert op.kernel == "march_idx"
    err = relerr(apply_shifted(op, x, y0, gpu), yref)
    print(f"dense mass P{p} {op.kernel}, x and y 8-byte aligned: {err:.3e}")
    assert err <= 1e-12


@gpu_test
def test_report_worst_ratios(gpu):
    """the record of the run: worst |got - ref| / (eps * magnitude) per kernel (runs last; the bound stays 2)"""
    for k in sorted(WORST):
        print(f"worst ratio {k}: {WORST[k]:.3f}")
        assert WORST[k] <= BOUND
