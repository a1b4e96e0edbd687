"""wf_leapfrog_step / wf_leapfrog_step_bc entry by entry against long double, in the harness of
test_gpu_vector_kernels.py (sentinel-padded buffers, shift 0 = 16-byte aligned -> the 16-byte kernel, shift 1 -> the
scalar kernel; boundary sets by name).

All eight compiled forms {16-byte, scalar} x {plan, none} x {v, no v}, in place (u_next = u_prev) and out of place, at
lengths on both sides of a pair, a bitmap word, a wave of pairs and a workgroup.

Bounds are derived, not measured (leapfrog_helpers restates the expressions and the count); eps = 2^-52, one rounding
= eps / 2, the library evaluates the expressions as written:

* plain dof, four roundings (b/m, dt2*a, 2u - u_prev, the sum):   |got - ref| <= 3 eps (|dt2 b/m| + 2|u| + |u_prev|)
* boundary dof, at most seven roundings on any path, the two of the denominator included:
      |got - ref| <= 5 eps T / (m + h),  T = dt2 (|b| + |s1 c1|) + 2 m |u| + (m + h) |u_prev|
* v, two roundings (difference, quotient):   |got - ref| <= 2 eps (|u_next| + |u_prev|) / (2 dt), from the u_next the
  device wrote.

Bitwise: b is +0.0 everywhere; with a plan every dof outside the union equals the no-plan form; the 16-byte form
equals the scalar form; in place equals out of place.  No entry is masked; sentinels and the vectors that are not
outputs are unchanged after every call; a refused call returns an error and writes nothing."""
import numpy as np
import pytest

import leapfrog_helpers as lh
import test_gpu_vector_kernels as vk
from leapfrog_helpers import LD
from support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 513, 4097]
BCS = ["none", "empty", "ends", "pair_both", "pair_even", "pair_odd", "word_seams", "gamma1_only", "gamma2_only", "mixed",
       "repeated", "random30"]
DT, S1, S2 = lh.KERNEL_DT, lh.KERNEL_S1, lh.KERNEL_S2
WORST = {}


def run(gpu, host, shift, has_v, inplace, plan):
    """one call on fresh padded buffers; returns (u_next, v or None, b) as the device left them"""
    from wave_fenics_amd import la
    n = host["b"].size
    pool = vk.Pool(gpu)
    d = {k: pool.padded(n, shift, host[k]) for k in ("b", "m", "u", "up")}
    un = d["up"] if inplace else pool.padded(n, shift, vk.junk(n))
    v = pool.padded(n, shift, vk.junk(n)) if has_v else None
    la.leapfrog_step(d["b"], d["m"], d["u"], d["up"], un, DT, v=v, bc=plan, s1=S1, s2=S2)
    pool.check(written=[d["b"], un] + ([v] if has_v else []))
    return un.cpu().numpy(), v.cpu().numpy() if has_v else None, d["b"].cpu().numpy()


def record(form, worst):
    WORST[form] = max(WORST.get(form, 0.0), worst)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("bc", BCS)
def test_leapfrog_step(gpu, bc, n):
    host, sets = lh.kernel_case(n, bc)
    plan = None if sets is None else vk.make_plan(n, sets)
    plan_ref = None if sets is None else vk.plan_reference(*sets)
    ref, bound = lh.step_reference(LD, host["b"], host["m"], host["u"], host["up"], DT, plan_ref, S1, S2)
    outside = np.ones(n, dtype=bool)
    if plan_ref is not None:
        outside[plan_ref[0]] = False
    first = {}
    for shift in (0, 1):
        for has_v in (False, True):
            noplan = run(gpu, host, shift, has_v, False, None)[0] if plan is not None else None
            for inplace in (False, True):
                what = f"n={n} bc={bc} shift={shift} v={has_v} inplace={inplace}"
                form = ("vec2" if shift == 0 else "vec1") + ("_bc" if plan_ref is not None and plan_ref[0].size else "") \
                    + ("_v" if has_v else "")
                un, v, b = run(gpu, host, shift, has_v, inplace, plan)
                assert not vk.bits(b).any(), f"{what}: b is not +0.0 everywhere"
                worst, ok, where = lh.worst_ratio(un, ref, bound)
                record(form, worst)
                assert ok, f"{what}: u_next[{where}] is {worst:.3f} of its bound from the reference"
                if has_v:
                    vref, vmag = lh.velocity(LD, un, host["up"], DT)
                    worst, ok, where = lh.worst_ratio(v, vref, lh.BOUND_V * vmag)
                    record(form + " v", worst)
                    assert ok, f"{what}: v[{where}] is {worst:.3f} of its bound from the reference"
                if noplan is not None:
                    assert vk.same_bits(un[outside], noplan[outside]), f"{what}: a dof outside the sets differs from the no-plan form"
                # the scalar form, in place, with and without v: all the same bits as the first call
                assert vk.same_bits(un, first.setdefault("un", un)), f"{what}: u_next differs between compiled forms"
                if has_v:
                    assert vk.same_bits(v, first.setdefault("v", v)), f"{what}: v differs between compiled forms"
    if plan is not None:
        plan.close()
    print(f"leapfrog_step n={n} bc={bc}: worst ratios to the bounds so far " + ", ".join(f"{k} {r:.3f}" for k, r in sorted(WORST.items())))


@pytest.mark.parametrize("operand", ["b", "m", "u", "up", "un", "v"])
@pytest.mark.parametrize("bc", ["none", "random30"])
def test_one_operand_shifted(gpu, bc, operand):
    """the 16-byte kernel needs every pointer 16-byte aligned: with any one 8 bytes off the scalar kernel runs and gives
    the same bits"""
    from wave_fenics_amd import la
    n = 257
    host, sets = lh.kernel_case(n, bc)
    plan = None if sets is None else vk.make_plan(n, sets)
    out = []
    for shifted in (None, operand):
        pool = vk.Pool(gpu)
        d = {k: pool.padded(n, int(k == shifted), host[k]) for k in ("b", "m", "u", "up")}
        un, v = pool.padded(n, int(shifted == "un"), vk.junk(n)), pool.padded(n, int(shifted == "v"), vk.junk(n))
        la.leapfrog_step(d["b"], d["m"], d["u"], d["up"], un, DT, v=v, bc=plan, s1=S1, s2=S2)
        pool.check(written=[d["b"], un, v])
        out.append((un.cpu().numpy(), v.cpu().numpy(), d["b"].cpu().numpy()))
    for a, b in zip(*out):
        assert vk.same_bits(a, b)
    if plan is not None:
        plan.close()


@pytest.mark.parametrize("shift", [0, 1])
def test_refusals_write_nothing(gpu, shift):
    import wave_fenics_amd as w
    from wave_fenics_amd import la
    from wave_fenics_amd._lib import lib
    from wave_fenics_amd.operators import _ptr
    n = 257
    host, sets = lh.kernel_case(n, "random30")
    plan = vk.make_plan(n, sets)
    other = vk.make_plan(n + 1, vk.boundary_set("ends", n + 1, np.random.default_rng(0)))

    def fresh():
        pool = vk.Pool(gpu)
        d = {k: pool.padded(n, shift, host[k]) for k in ("b", "m", "u", "up")}
        d["un"], d["v"] = pool.padded(n, shift, vk.junk(n)), pool.padded(n, shift, vk.junk(n))
        return pool, d

    def refused(d, pool, **kw):
        a = dict(b=d["b"], m=d["m"], u=d["u"], u_prev=d["up"], u_next=d["un"], dt=DT, v=d["v"], bc=plan, s1=S1, s2=S2)
        a.update(kw)
        with pytest.raises(w.WavehipError):
            la.leapfrog_step(**a)
        pool.check()

    for bc in (plan, None):
        for k in ("u", "b", "m"):                       # u_next on an input other than u_prev
            pool, d = fresh()
            refused(d, pool, u_next=d[k], bc=bc)
        for k in ("b", "m", "u", "up", "un"):           # v on any other vector of the call
            pool, d = fresh()
            refused(d, pool, v=d[k], bc=bc)
        for dt in (0.0, -DT, float("nan")):
            pool, d = fresh()
            refused(d, pool, dt=dt, bc=bc)
        pool, d = fresh()                               # overlapping without being the same vector
        refused(d, pool, u_next=d["up"][1:], u_prev=d["up"][:-1], b=d["b"][:-1], m=d["m"][:-1], u=d["u"][:-1], v=None, bc=None)
    pool, d = fresh()
    refused(d, pool, s2=1.0e-300)
    pool, d = fresh()
    refused(d, pool, bc=other)
    pool, d = fresh()                                   # null vectors and a null plan, straight through the C ABI
    p = {k: _ptr(t) for k, t in d.items()}
    for null in ("b", "m", "u", "up", "un"):
        q = dict(p, **{null: 0})
        assert lib().wf_leapfrog_step(n, DT, q["b"], q["m"], q["u"], q["up"], q["un"], q["v"], 0) != 0
        assert lib().wf_leapfrog_step_bc(n, DT, q["b"], q["m"], q["u"], q["up"], q["un"], q["v"], plan._h, S1, S2, 0) != 0
    assert lib().wf_leapfrog_step_bc(n, DT, p["b"], p["m"], p["u"], p["up"], p["un"], p["v"], None, S1, S2, 0) != 0
    assert b"plan" in lib().wf_last_error()
    pool.check()
    for nn in (0, -3):                                  # n <= 0: a no-op that succeeds
        assert lib().wf_leapfrog_step(nn, DT, p["b"], p["m"], p["u"], p["up"], p["un"], p["v"], 0) == 0
    pool.check()
    plan.close()
    other.close()


def test_report_worst_ratios(gpu):
    """the record of the run (runs last): worst |got - ref| as a fraction of each form's bound"""
    for k in sorted(WORST):
        print(f"worst ratio to the bound, {k}: {WORST[k]:.3f}")
        assert WORST[k] <= 1.0
