"""wf_leapfrog4_predict, wf_leapfrog4_correct and wf_sources_add_stencil entry by entry against long double, in the
guarded buffers of guard_helpers.py (inputs inside NaN padding, outputs inside 2^-1022 padding; shift 0 = 16-byte aligned
-> the 16-byte sweep, shift 1 -> the scalar sweep).

Every compiled form: predictor {16-byte, scalar} x {plan, none}; corrector the same x {v, no v}; in place (u_star =
u_prev; u_next = u_star) and out of place; boundary sets by the names of test_gpu_vector_kernels.boundary_set: none,
empty, Gamma_1 only, Gamma_2 only, mixed (a dof in one, the other, both, neither), random30, word_seams.  Lengths 1, 2,
3, 511, 1025, and 2^30 + 1 = leapfrog4_helpers.two_entry_length(): the smallest length at which one thread of a sweep
takes two entries (the scalar sweep past the cap of capped_grid; the derivation is asserted in test_leapfrog4_host.py).

Bounds are derived, not measured (leapfrog4_helpers states the expressions and the counts): w within 2 eps (plain) and
4 eps (union set) of its magnitude, u_next within 3 and 7, u_star within leapfrog_helpers' 3 and 5, v within 2.

Bitwise: b is +0.0 everywhere; u_star equals what wf_leapfrog_step(_bc) stores in u_next from the same inputs; every
compiled form of a kernel gives the same bits, in place as out of place; with a plan every dof outside the union equals
the no-plan form.  No entry is masked; padding and inputs are unchanged after every call; a refused call returns an error
and writes nothing.

The two-entry length runs the scalar forms in place on five vectors of 8 GiB that repeat a block of 2^20 entries: every
block of the result equals, bit for bit, the call on the block alone (checked against long double like every other
length), and the dofs of a four-dof plan at both ends -- dof 2^30, thread 0's second entry, among them -- are held to
the long-double bound.

wf_sources_add_stencil: nt = 1 with weight 1 against wf_sources_add bit for bit; nt = 2, 3 against long double with
the wavelet bounds of test_gpu_points_kernel (each s(t_k) with its own, plus one rounding per product and per addition
of the stencil: nt eps sum_k |a_k s(t_k)|); duplicate points (shared dofs); dofs no source touches keep their bits."""
import numpy as np
import pytest

import guard_helpers as gh
import leapfrog4_helpers as l4
import leapfrog_helpers as lh
import points_helpers as ph
import test_gpu_vector_kernels as vk
from leapfrog_helpers import LD
from support import EPS, bits, gpu, ratio  # noqa: F401

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 511, 1025]
BCS = ["none", "empty", "gamma1_only", "gamma2_only", "mixed", "random30", "word_seams"]
DT, S1, S2, S1C = l4.KERNEL_DT, l4.KERNEL_S1, l4.KERNEL_S2, l4.KERNEL_S1C
PAD = 4096
WORST = {}


class Bufs:
    """the guarded device vectors of one call and their host copies"""

    def __init__(self, device):
        self.device, self.items = device, []

    def _add(self, values, shift, fill):
        view, guard = gh.guarded(values, PAD, shift, fill, self.device)
        self.items.append((view, guard, np.array(values, dtype=np.float64)))
        return view

    def inp(self, values, shift):
        return self._add(values, shift, gh.NAN)

    def out(self, n, shift):
        return self._add(vk.junk(n), shift, gh.MIN_NORMAL)

    def check(self, written=()):
        """padding intact everywhere; every vector not in `written` holds its bits"""
        import torch
        torch.cuda.synchronize()
        out = {v.data_ptr() for v in written}
        for k, (view, guard, host) in enumerate(self.items):
            assert guard.intact(), f"buffer {k}: padding entries {guard.changed()[:8]} were written"
            if view.data_ptr() not in out:
                assert np.array_equal(bits(view.cpu().numpy()), bits(host)), f"buffer {k}: a vector that is no output was modified"


def record(form, worst):
    WORST[form] = max(WORST.get(form, 0.0), worst)


def outside(n, plan_ref):
    o = np.ones(n, dtype=bool)
    if plan_ref is not None:
        o[plan_ref[0]] = False
    return o


def run_predict(gpu, host, shift, inplace, plan):
    from wave_fenics_amd import la
    n = host["b"].size
    B = Bufs(gpu)
    d = {k: B.inp(host[k], shift) for k in ("b", "m", "u", "up")}
    us = d["up"] if inplace else B.out(n, shift)
    w = B.out(n, shift)
    la.leapfrog4_predict(d["b"], d["m"], d["u"], d["up"], us, w, DT, bc=plan, s1=S1, s2=S2)
    B.check(written=[d["b"], us, w])
    return us.cpu().numpy(), w.cpu().numpy(), d["b"].cpu().numpy()


def run_correct(gpu, host, shift, has_v, inplace, plan):
    from wave_fenics_amd import la
    n = host["b"].size
    B = Bufs(gpu)
    d = {k: B.inp(host[k], shift) for k in ("b", "m", "us", "up")}
    un = d["us"] if inplace else B.out(n, shift)
    v = B.out(n, shift) if has_v else None
    la.leapfrog4_correct(d["b"], d["m"], d["us"], un, DT, u_prev=d["up"] if has_v else None, v=v, bc=plan, s1c=S1C, s2=S2)
    B.check(written=[d["b"], un] + ([v] if has_v else []))
    return un.cpu().numpy(), v.cpu().numpy() if has_v else None, d["b"].cpu().numpy()


def run_leapfrog(gpu, host, plan):
    """u_next of wf_leapfrog_step(_bc) from the predictor's inputs"""
    from wave_fenics_amd import la
    n = host["b"].size
    B = Bufs(gpu)
    d = {k: B.inp(host[k], 0) for k in ("b", "m", "u", "up")}
    un = B.out(n, 0)
    la.leapfrog_step(d["b"], d["m"], d["u"], d["up"], un, DT, bc=plan, s1=S1, s2=S2)
    B.check(written=[d["b"], un])
    return un.cpu().numpy()


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("bc", BCS)
def test_predict(gpu, bc, n):
    host, sets = l4.kernel_case(n, bc)
    plan = None if sets is None else vk.make_plan(n, sets)
    plan_ref = None if sets is None else vk.plan_reference(*sets)
    us_ref, us_bound, w_ref, w_bound = l4.predict_reference(LD, host["b"], host["m"], host["u"], host["up"], DT, plan_ref, S1, S2)
    off = outside(n, plan_ref)
    step = run_leapfrog(gpu, host, plan)
    first = {}
    for shift in (0, 1):
        noplan = run_predict(gpu, host, shift, False, None) if plan is not None else None
        for inplace in (False, True):
            what = f"predict n={n} bc={bc} shift={shift} inplace={inplace}"
            form = "predict " + ("vec2" if shift == 0 else "vec1") + ("_bc" if plan_ref is not None and plan_ref[0].size else "")
            us, w, b = run_predict(gpu, host, shift, inplace, plan)
            assert not vk.bits(b).any(), f"{what}: b is not +0.0 everywhere"
            for name, got, ref, bound in (("u_star", us, us_ref, us_bound), ("w", w, w_ref, w_bound)):
                worst, ok, where = lh.worst_ratio(got, ref, bound)
                record(f"{form} {name}", worst)
                assert ok, f"{what}: {name}[{where}] is {worst:.3f} of its bound from the reference"
            assert vk.same_bits(us, step), f"{what}: u_star differs from the u_next of wf_leapfrog_step"
            if noplan is not None:
                assert vk.same_bits(us[off], noplan[0][off]) and vk.same_bits(w[off], noplan[1][off]), \
                    f"{what}: a dof outside the sets differs from the no-plan form"
            assert vk.same_bits(us, first.setdefault("us", us)) and vk.same_bits(w, first.setdefault("w", w)), \
                f"{what}: the compiled forms differ"
    if plan is not None:
        plan.close()


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("bc", BCS)
def test_correct(gpu, bc, n):
    host, sets = l4.kernel_case(n, bc)
    plan = None if sets is None else vk.make_plan(n, sets)
    plan_ref = None if sets is None else vk.plan_reference(*sets)
    ref, bound = l4.correct_reference(LD, host["b"], host["m"], host["us"], DT, plan_ref, S1C, S2)
    off = outside(n, plan_ref)
    first = {}
    for shift in (0, 1):
        for has_v in (False, True):
            noplan = run_correct(gpu, host, shift, has_v, False, None)[0] if plan is not None else None
            for inplace in (False, True):
                what = f"correct n={n} bc={bc} shift={shift} v={has_v} inplace={inplace}"
                form = "correct " + ("vec2" if shift == 0 else "vec1") + ("_bc" if plan_ref is not None and plan_ref[0].size else "") \
                    + ("_v" if has_v else "")
                un, v, b = run_correct(gpu, host, shift, has_v, inplace, plan)
                assert not vk.bits(b).any(), f"{what}: b is not +0.0 everywhere"
                worst, ok, where = lh.worst_ratio(un, ref, bound)
                record(form, worst)
                assert ok, f"{what}: u_next[{where}] is {worst:.3f} of its bound from the reference"
                if has_v:
                    vref, vmag = lh.velocity(LD, un, host["up"], DT)
                    worst, ok, where = lh.worst_ratio(v, vref, lh.BOUND_V * vmag)
                    record(form + " v", worst)
                    assert ok, f"{what}: v[{where}] is {worst:.3f} of its bound from the reference"
                    assert vk.same_bits(v, first.setdefault("v", v)), f"{what}: v differs between compiled forms"
                if noplan is not None:
                    assert vk.same_bits(un[off], noplan[off]), f"{what}: a dof outside the sets differs from the no-plan form"
                assert vk.same_bits(un, first.setdefault("un", un)), f"{what}: u_next differs between compiled forms"
    if plan is not None:
        plan.close()


@pytest.mark.parametrize("operand", ["b", "m", "u", "up", "us", "w", "un", "v"])
@pytest.mark.parametrize("bc", ["none", "random30"])
def test_one_operand_shifted(gpu, bc, operand):
    """the 16-byte sweeps need every pointer 16-byte aligned: with any one 8 bytes off the scalar sweep runs and gives the
    same bits (an operand a kernel does not take leaves its call as it is)"""
    from wave_fenics_amd import la
    n = 257
    host, sets = l4.kernel_case(n, bc)
    plan = None if sets is None else vk.make_plan(n, sets)
    out = []
    for shifted in (None, operand):
        sh = lambda k: int(k == shifted)   # noqa: E731
        B = Bufs(gpu)
        d = {k: B.inp(host[k], sh(k)) for k in ("b", "m", "u", "up")}
        us, w = B.out(n, sh("us")), B.out(n, sh("w"))
        la.leapfrog4_predict(d["b"], d["m"], d["u"], d["up"], us, w, DT, bc=plan, s1=S1, s2=S2)
        B.check(written=[d["b"], us, w])
        C = Bufs(gpu)
        e = {k: C.inp(host[k], sh(k)) for k in ("b", "m", "us", "up")}
        un, v = C.out(n, sh("un")), C.out(n, sh("v"))
        la.leapfrog4_correct(e["b"], e["m"], e["us"], un, DT, u_prev=e["up"], v=v, bc=plan, s1c=S1C, s2=S2)
        C.check(written=[e["b"], un, v])
        out.append([t.cpu().numpy() for t in (us, w, d["b"], un, v, e["b"])])
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
    host, sets = l4.kernel_case(n, "random30")
    plan = vk.make_plan(n, sets)
    other = vk.make_plan(n + 1, vk.boundary_set("ends", n + 1, np.random.default_rng(0)))

    def fresh():
        B = Bufs(gpu)
        d = {k: B.inp(host[k], shift) for k in ("b", "m", "u", "up", "us")}
        d.update({k: B.out(n, shift) for k in ("w", "un", "v", "star")})
        return B, d

    def predict(d, B, **kw):
        a = dict(b=d["b"], m=d["m"], u=d["u"], u_prev=d["up"], u_star=d["star"], w=d["w"], dt=DT, bc=plan, s1=S1, s2=S2)
        a.update(kw)
        with pytest.raises(w.WavehipError):
            la.leapfrog4_predict(**a)
        B.check()

    def correct(d, B, **kw):
        a = dict(b=d["b"], m=d["m"], u_star=d["us"], u_next=d["un"], dt=DT, u_prev=d["up"], v=d["v"], bc=plan, s1c=S1C, s2=S2)
        a.update(kw)
        with pytest.raises(w.WavehipError):
            la.leapfrog4_correct(**a)
        B.check()

    for bc in (plan, None):
        for k in ("u", "b", "m", "w"):                  # u_star on an input other than u_prev, or on w
            B, d = fresh()
            predict(d, B, u_star=d[k], bc=bc)
        for k in ("b", "m", "u", "up"):                 # w on any other vector of the call
            B, d = fresh()
            predict(d, B, w=d[k], bc=bc)
        for k in ("b", "m"):                            # u_next or u_star on b or m
            B, d = fresh()
            correct(d, B, u_next=d[k], bc=bc)
            B, d = fresh()
            correct(d, B, u_star=d[k], bc=bc)
        for k in ("un", "us", "b"):                     # with v, u_prev must be a vector of its own
            B, d = fresh()
            correct(d, B, u_prev=d[k], bc=bc)
        for k in ("b", "m", "us", "up", "un"):          # v on any other vector of the call
            B, d = fresh()
            correct(d, B, v=d[k], bc=bc)
        B, d = fresh()
        correct(d, B, u_prev=None, bc=bc)               # v without u_prev
        for dt in (0.0, -DT, float("nan")):
            B, d = fresh()
            predict(d, B, dt=dt, bc=bc)
            correct(d, B, dt=dt, bc=bc)
        B, d = fresh()                                  # overlapping without being the same vector
        predict(d, B, u_star=d["up"][1:], u_prev=d["up"][:-1], b=d["b"][:-1], m=d["m"][:-1], u=d["u"][:-1], w=d["w"][:-1], bc=None)
        correct(d, B, u_next=d["us"][1:], u_star=d["us"][:-1], b=d["b"][:-1], m=d["m"][:-1], u_prev=None, v=None, bc=None)
    for call in (predict, correct):
        B, d = fresh()
        call(d, B, s2=1.0e-300)
        call(d, B, bc=other)
    B, d = fresh()                                      # null vectors, straight through the C ABI
    p = {k: _ptr(t) for k, t in d.items()}
    for null in ("b", "m", "u", "up", "star", "w"):
        q = dict(p, **{null: 0})
        assert lib().wf_leapfrog4_predict(n, DT, q["b"], q["m"], q["u"], q["up"], q["star"], q["w"], plan._h, S1, S2, 0) != 0
    for null in ("b", "m", "us", "un"):
        q = dict(p, **{null: 0})
        assert lib().wf_leapfrog4_correct(n, DT, q["b"], q["m"], q["us"], q["up"], q["un"], q["v"], plan._h, S1C, S2, 0) != 0
    B.check()
    for nn in (0, -3):                                  # n <= 0: a no-op that succeeds
        assert lib().wf_leapfrog4_predict(nn, DT, p["b"], p["m"], p["u"], p["up"], p["star"], p["w"], plan._h, S1, S2, 0) == 0
        assert lib().wf_leapfrog4_correct(nn, DT, p["b"], p["m"], p["us"], p["up"], p["un"], p["v"], plan._h, S1C, S2, 0) == 0
    B.check()
    plan.close()
    other.close()


def test_two_entries_per_thread(gpu):
    """n = 2^30 + 1, scalar sweeps (every vector 8 bytes off), in place, with a four-dof plan: the module docstring's test"""
    import torch
    from wave_fenics_amd import la
    n, blk = l4.two_entry_length(), 2 ** 20
    assert l4.entries_per_thread(n, vec=False) == 2 and (n - 1) % blk == 0
    reps = (n - 1) // blk
    host, _ = l4.kernel_case(blk, "none")
    dofs = np.array([0, 5, n - 2, n - 1], dtype=np.int32)
    sets = (dofs[[0, 1, 3]], np.array([0.7, 1.3, 0.9]), dofs[[1, 2, 3]], np.array([0.4, 2.1, 1.6]))
    plan, plan_ref = vk.make_plan(n, sets), vk.plan_reference(*sets)
    pos = plan_ref[0] % blk                              # where the plan's dofs lie in the block

    def big(values, fill):
        """the block repeated, plus its first entry once more, inside PAD + 1 sentinels in front and PAD behind"""
        buf = torch.full((PAD + 1 + n + PAD,), fill, dtype=torch.float64, device=gpu)
        view = buf[PAD + 1:PAD + 1 + n]
        small = torch.from_numpy(values).to(gpu)
        view[:n - 1].view(reps, blk).copy_(small.expand(reps, blk))
        view[n - 1:].copy_(small[:1])
        assert view.data_ptr() % 16 == 8
        return buf, view

    def check(buf, view, want, fill, name):
        """every block equals `want` bit for bit except at the plan's dofs; the padding holds its bits"""
        w64 = torch.from_numpy(np.ascontiguousarray(want)).to(gpu).view(torch.int64)
        diff = view[:n - 1].view(torch.int64).view(reps, blk) != w64
        diff[0, pos[plan_ref[0] < blk].tolist()] = False
        diff[reps - 1, pos[(plan_ref[0] >= n - 1 - blk) & (plan_ref[0] < n - 1)].tolist()] = False
        assert not bool(diff.any()), f"{name}: an entry differs from the call on one block"
        fb = int(np.array([fill]).view(np.int64)[0])
        pad = torch.cat([buf[:PAD + 1], buf[PAD + 1 + n:]]).view(torch.int64)
        assert bool((pad == fb).all()), f"{name}: padding was written"

    # the calls on one block (scalar sweep, no plan): what every block of the long vectors must equal
    sb = Bufs(gpu)
    s = {k: sb.inp(host[k], 1) for k in ("b", "m", "u", "up")}
    sw = sb.out(blk, 1)
    la.leapfrog4_predict(s["b"], s["m"], s["u"], s["up"], s["up"], sw, DT, s2=S2)
    us_small, w_small = s["up"].cpu().numpy(), sw.cpu().numpy()
    s["b"].copy_(torch.from_numpy(host["b"]).to(gpu))
    la.leapfrog4_correct(s["b"], s["m"], s["up"], s["up"], DT, s2=S2)
    un_small = s["up"].cpu().numpy()
    del sb, s, sw
    vec = {k: big(host[k], gh.NAN) for k in ("b", "m", "u", "up")}
    vec["w"] = big(vk.junk(blk), gh.MIN_NORMAL)
    v = {k: t[1] for k, t in vec.items()}
    la.leapfrog4_predict(v["b"], v["m"], v["u"], v["up"], v["up"], v["w"], DT, bc=plan, s1=S1, s2=S2)
    torch.cuda.synchronize()
    assert not bool(v["b"].view(torch.int64).any()), "b is not +0.0 everywhere"
    check(*vec["up"], us_small, gh.NAN, "u_star")
    check(*vec["w"], w_small, gh.MIN_NORMAL, "w")
    idx = torch.from_numpy(plan_ref[0]).to(gpu).long()
    hb = {k: host[k][pos] for k in ("b", "m", "u", "up")}
    local = (np.arange(pos.size), plan_ref[1], plan_ref[2])
    us_ref, us_bound, w_ref, w_bound = l4.predict_reference(LD, hb["b"], hb["m"], hb["u"], hb["up"], DT, local, S1, S2)
    us_plan = v["up"][idx].cpu().numpy()
    for name, got, ref, bound in (("u_star", us_plan, us_ref, us_bound), ("w", v["w"][idx].cpu().numpy(), w_ref, w_bound)):
        worst, ok, where = lh.worst_ratio(got, ref, bound)
        record(f"predict vec1_bc two entries {name}", worst)
        assert ok, f"two entries per thread: {name} at dof {plan_ref[0][where]} is {worst:.3f} of its bound"
    for k in ("m", "u"):
        check(*vec[k], host[k], gh.NAN, k)               # inputs unchanged (the plan's dofs included: excluded entries are equal anyway)
    # the corrector in place on u_star, b refilled
    v["b"][:n - 1].view(reps, blk).copy_(torch.from_numpy(host["b"]).to(gpu).expand(reps, blk))
    v["b"][n - 1:].copy_(torch.from_numpy(host["b"][:1]).to(gpu))
    la.leapfrog4_correct(v["b"], v["m"], v["up"], v["up"], DT, bc=plan, s1c=S1C, s2=S2)
    torch.cuda.synchronize()
    assert not bool(v["b"].view(torch.int64).any()), "b is not +0.0 everywhere"
    check(*vec["up"], un_small, gh.NAN, "u_next")
    un_ref, un_bound = l4.correct_reference(LD, hb["b"], hb["m"], us_plan, DT, local, S1C, S2)
    worst, ok, where = lh.worst_ratio(v["up"][idx].cpu().numpy(), un_ref, un_bound)
    record("correct vec1_bc two entries", worst)
    assert ok, f"two entries per thread: u_next at dof {plan_ref[0][where]} is {worst:.3f} of its bound"
    # the last dof alone, off the block structure: dof 2^30 is in the plan and was held to the bound above
    assert plan_ref[0][-1] == n - 1
    plan.close()
    del vec, v
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# wf_sources_add_stencil
# ---------------------------------------------------------------------------------------------------------------------
def stencil_reference(V, src, wavelets, times, weights, b):
    """(ref, bound in units of eps, touched) of b after add_stencil, per dof, in long double: add_reference of
    test_gpu_points_kernel with S = sum_k a_k s(t_k) for s(t) and the bound of the module docstring for ds"""
    import test_gpu_points_kernel as tp
    W = ph.tensor_weights(src.w, LD)
    nt = len(times)
    s = np.array([sum(LD(a) * ph.wavelet_ld(wl, t) for a, t in zip(weights, times)) for wl in wavelets], dtype=LD)
    sabs = np.array([sum(abs(LD(a) * ph.wavelet_ld(wl, t)) for a, t in zip(weights, times)) for wl in wavelets], dtype=LD)
    ds = np.array([sum(abs(a) * tp.ds_bound(wl, t) for a, t in zip(weights, times)) for wl in wavelets], dtype=LD) + nt * sabs
    acc, mag, err, cnt = (np.zeros(V.ndofs, dtype=LD) for _ in range(4))
    for i in range(len(wavelets)):
        np.add.at(acc, src.dofs[i], W[i] * s[i])
        np.add.at(mag, src.dofs[i], np.abs(W[i]) * sabs[i])
        np.add.at(err, src.dofs[i], np.abs(W[i]) * ds[i])
        np.add.at(cnt, src.dofs[i], (W[i] != 0).astype(LD))
    bl = np.asarray(b, dtype=LD)
    bound = err + (0.5 * cnt + 2.0) * mag + 0.5 * (np.abs(bl) + mag)
    return bl + acc, bound, cnt > 0


@pytest.mark.parametrize("p", [2, 4])
def test_sources_add_stencil(gpu, p):
    import torch
    import test_gpu_points_kernel as tp
    from wave_fenics_amd import points
    V = tp.space(p, "renumbered")
    nd = (p + 1) ** 3
    nsrc = 5
    rng = np.random.default_rng(90 + p)
    cell, ref = tp.random_points(V, nsrc, 700 + p)
    cell[1], ref[1] = cell[0], ref[0]                     # a duplicate: every dof of source 0 is shared
    wavelets = [points.ricker(2.0 + 0.1 * i, 0.75, 1.0 + i) if i % 2 == 0 else
                points.sampled(rng.uniform(-2.0, 2.0, 5 + i % 3), 0.25, 0.125) for i in range(nsrc)]
    src = points.Sources(V, None, wavelets, located=(cell, ref))
    b0 = rng.uniform(-1.0, 1.0, V.ndofs)
    h = 0.0625
    for t in (0.3, 0.75, 0.8125):
        # nt = 1, weight 1: the bits of wf_sources_add
        got = []
        for call in (lambda b: src.add(t, b), lambda b: src.add_stencil([t], [1.0], b)):
            bd, bg = gh.guarded(b0, gh.batch_pad(nd), 1, gh.MIN_NORMAL, gpu)
            call(bd)
            torch.cuda.synchronize()
            assert bg.intact()
            got.append(bd.cpu().numpy())
        assert np.array_equal(bits(got[0]), bits(got[1])), "nt = 1 with weight 1 differs from wf_sources_add"
        for times, weights in (([t - h, t + h], [-1.0 / (2 * h), 1.0 / (2 * h)]),
                               ([t - h, t, t + h], [1.0 / 12.0, -2.0 / 12.0, 1.0 / 12.0]),
                               ([t - h, t, t + h], [1.0 / h ** 2, -2.0 / h ** 2, 1.0 / h ** 2]), ([t], [-3.5])):
            want, bound, touched = stencil_reference(V, src, wavelets, times, weights, b0)
            results = []
            for shift in (0, 1):
                bd, bg = gh.guarded(b0, gh.batch_pad(nd), shift, gh.MIN_NORMAL, gpu)
                src.add_stencil(times, weights, bd)
                torch.cuda.synchronize()
                res = bd.cpu().numpy()
                assert bg.intact() and np.isfinite(res).all()
                assert np.array_equal(bits(res[~touched]), bits(b0[~touched])), "dofs no source touches keep their bits"
                worst, ok, at = ratio(res, want, bound, 1.0)
                record(f"sources_add_stencil nt={len(times)}", worst)
                assert ok, (p, t, times, at, worst)
                results.append(res)
            assert np.array_equal(bits(results[0]), bits(results[1])), "a repeat equals itself"
    src.close()


def test_sources_add_stencil_refusals(gpu):
    import ctypes

    import test_gpu_points_kernel as tp
    from wave_fenics_amd import points
    from wave_fenics_amd._lib import lib
    V = tp.space(2, "box")
    cell, ref = tp.random_points(V, 2, 3)
    src = points.Sources(V, None, [points.ricker(2.0, 0.75, 1.0)] * 2, located=(cell, ref))
    bd, bg = gh.guarded(np.ones(V.ndofs), 4096, 0, gh.MIN_NORMAL, gpu)
    arr = lambda *a: (ctypes.c_double * len(a))(*a)   # noqa: E731
    ok3 = arr(0.1, 0.2, 0.3)
    L = lib()
    for nt in (0, -1, 4):
        assert L.wf_sources_add_stencil(src._s, nt, ok3, ok3, bd.data_ptr(), None) == -1 and b"nt" in L.wf_last_error()
    assert L.wf_sources_add_stencil(src._s, 2, None, ok3, bd.data_ptr(), None) == -1
    assert L.wf_sources_add_stencil(src._s, 2, ok3, None, bd.data_ptr(), None) == -1
    assert L.wf_sources_add_stencil(src._s, 3, arr(0.1, float("nan"), 0.3), ok3, bd.data_ptr(), None) == -1
    assert L.wf_sources_add_stencil(src._s, 3, ok3, arr(0.1, 0.2, float("inf")), bd.data_ptr(), None) == -1
    assert L.wf_sources_add_stencil(src._s, 2, arr(0.1, 0.2, float("nan")), ok3, bd.data_ptr(), None) == 0   # the third is not read
    assert L.wf_sources_add_stencil(src._s, 1, ok3, ok3, None, None) == -1
    with pytest.raises(ValueError):
        src.add_stencil([0.1, 0.2], [1.0], bd)
    import torch
    torch.cuda.synchronize()
    assert bg.intact()
    src.close()


def test_report_worst_ratios(gpu):
    """the record of the run (runs last): worst |got - ref| as a fraction of each form's bound"""
    for k in sorted(WORST):
        print(f"worst ratio to the bound, {k}: {WORST[k]:.3f}")
        assert WORST[k] <= 1.0
