"""Stream order of every public entry that takes a stream: one table, every row behind work on a side stream
(tests/stream_helpers.py).

include/wavehip.h: "all device work is stream-ordered and asynchronous, nothing synchronises".  Each row poisons the
inputs and in/out vectors of one call with NaN, queues the load on a non-blocking side stream, copies the good values in
behind it, calls at once, and snapshots the outputs on the same stream.  The snapshots must equal those of the same call on
the default stream with nothing in flight (the twin, which runs afterwards, on the same handle), and the call must have
returned while the load was still running.  Rows of the entries that synchronise by contract (wf_sync, wf_comm_barrier,
wf_cg) assert the inverse: at return the load has completed.

Comparison.  Bit for bit where the entry's contract says bits or the kernel has one writer per entry: the vector and
time-step kernels, the point kernels, the cell forms, the owner and ordered operators, the exchange (copies; the reverse
exchange and wf_scatter_add / wf_dot are fed small integers times the case's factor, whose sums are exact in any order;
wf_boundary_apply, which adds by atomics, gets two disjoint sets, one writer per entry: with a dof in both sets one entry
came out a rounding apart from its twin in one run of three).
Where an operator adds by atomics, the bound that family's own repeat test uses: TOL_FORM = 1e-13 of max|y|
(test_gpu_owner_update.py) for the hex forms, B eps mag per entry (the "two applies agree" bound of
test_gpu_tet_dense_paths.py and test_gpu_tet_mass.py) for the tetrahedral ones.  A poisoned input gives NaN or an error of
the order of the values, so nothing hangs on the tolerance.

Rows (ROWS; tests/test_stream_table.py holds every prototype of the header with a `void* stream` to this table):
  vectors     wf_copy, fill, axpy, scale, pointwise_div, pointwise_mult_add, dot, gather, scatter_add, scatter_set,
              transform1, segment_sum_add, memset; wf_boundary_apply and _apply_plan; wf_rk4_stage and _bc with and without a
              next stage; wf_leapfrog_step and _bc with and without v; wf_leapfrog_correlate: n = 513 (two full workgroups
              and one entry; an odd count for the 16-byte forms), once 16-byte aligned and once with every base shifted
              by 8 bytes (the scalar forms)
  points      wf_points_sample, wf_sources_add, wf_sources_add_values: P4, five points, two of them in one cell
  cell forms  wf_cell_form_eval: stiffness per point, stiffness per cell, lumped mass; P2 on cell_form_helpers.GPU_BOX[2]
  operators   wf_op_apply: the first case of stiffness_entry_helpers.cases() per (kernel, geometry, metric, update) and
              both ordered cases; the first case of mass_entry_helpers.cases() per (operator, kernel, ordered); one
              tetrahedral stiffness and one tetrahedral mass shape.  Uniform field, y0 = U(-1, 1); the selected kernel is
              asserted as those tests assert it
  parts       wf_op_apply_part: interior then interface on the gated stream against the whole apply (the owner box of
              test_gpu_parts_matrix.py at P2)
  updater     wf_updater_fwd, _rev, and the split phases with an axpy queued between begin and end, on the default updater
              (the exchange runs on the updater's stream and must wait for the pack, which the gate holds back) and on
              WF_UPDATER_INLINE; one-rank periodic partition, native transport
  overlapped  wf_op_apply_overlapped at P2 and P4, owner kernel, same partition: two applies back to back with no
              synchronise between them (the events are recorded again while they may be in use); the interior part runs
              on the updater's low-priority stream and must wait for the gate through ev_main
  collectives wf_comm_allreduce behind the gate; wf_comm_barrier, wf_sync(stream) and wf_cg synchronise
wf_tsmm has tests/test_gpu_tsmm_paths.py and wf_cg tests/test_gpu_cg_iteration.py::test_cg_on_side_stream for the values
behind queued work; they are referenced (REFERENCED), not exempt.

What this proves, and what it does not.  A launch on another stream, and a missing wait at the head of a hidden stream
(ev_main, ev_packed), are caught deterministically: the poisoned inputs are read while the load is still running.  A
missing join at the tail -- `stream` no longer waiting for ev_interior, or fwd_end no longer waiting for ev_done -- is NOT
caught deterministically: the snapshot on the same stream sees it only when the hidden stream happens to be late."""
import ctypes
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import mass_entry_helpers as me
import stiffness_entry_helpers as se
import stream_helpers as sh
from support import EPS, LD, bits, comm, gpu, ratio  # noqa: F401

pytestmark = pytest.mark.gpu

N = 513
TOL_FORM = 1e-13      # of max|y|: tests/test_gpu_owner_update.py
# The one-rank periodic partition: x and z periodic as in test_gpu_cg_iteration.py.  Nine cells along x: the owner kernel's
# columns hold eight, so the footprint of a second column stands clear of the ghost plane I = 0; five along z in the
# segments [0, 1), [1, 3), [3, 5) (lz = 2, lz0 = 1): the footprint of the third stands clear of the ghost plane K = 0,
# so the second column's third segment is an interior item.
PARTITION = dict(n=(9, 2, 5), periodic=(True, False, True))
REFERENCED = {"wf_tsmm": "tests/test_gpu_tsmm_paths.py (every plan path behind queued work on a side stream)",
              "wf_cg": "tests/test_gpu_cg_iteration.py::test_cg_on_side_stream; the row `cg-synchronises` here",
              "wf_wave_rk4_fused": "tests/test_gpu_stream_models.py (rk4_fused behind queued work, one rank and a z-periodic partition)",
              "wf_wave_leapfrog": "tests/test_gpu_stream_models.py (leapfrog and misfit_gradient behind queued work, one rank and a "
                                  "z-periodic partition)",
              "wf_leapfrog4_predict": "tests/test_gpu_leapfrog4_streams.py::test_stream_order (rows leapfrog4_predict*)",
              "wf_leapfrog4_correct": "tests/test_gpu_leapfrog4_streams.py::test_stream_order (rows leapfrog4_correct*)",
              "wf_sources_add_stencil": "tests/test_gpu_leapfrog4_streams.py::test_stream_order (row sources_add_stencil)",
              "wf_leapfrog4_correlate": "tests/test_gpu_adjoint4_streams.py::test_stream_order (rows leapfrog4_correlate*)",
              "wf_wave_leapfrog4": "tests/test_gpu_leapfrog4_streams.py::test_model_behind_queued_work (leapfrog4, no hook) and "
                                   "tests/test_gpu_adjoint4_streams.py::test_loop_with_a_hook_behind_queued_work (hook and start-up)"}
ROWS = []             # (id, entries, builder(gpu, s, rng, request) -> case)


def row(rid, *entries):
    def register(build):
        ROWS.append((rid, entries, build))
        return build
    return register


def case(vecs, call, outs, off=0, tol=None, sync=False, check=None, keep=None):
    """vecs: name -> host vector (poisoned on the device); call(t): the call on the device vectors t; outs: the names to
    compare; tol: None for bits, else the share of max|twin|; sync: the entry synchronises by contract; check(name, got,
    twin): a comparison of its own; keep: whatever must outlive the calls"""
    return SimpleNamespace(vecs=vecs, call=call, outs=outs, off=off, tol=tol, sync=sync, check=check, keep=keep)


def L():
    from wave_fenics_amd import _lib
    return _lib.lib()


def ptr(t):
    return int(t.data_ptr())


def cur(t):
    from wave_fenics_amd.operators import _stream
    return _stream(t)


def ok(rc):
    from wave_fenics_amd._lib import check
    check(rc)


def ints(rng, n, s):
    """small integers times the case's factor: sums and products of a few hundred of them are exact in any order"""
    return rng.integers(-8, 9, n).astype(np.float64) * s


def uni(rng, n, s):
    return rng.uniform(-1.0, 1.0, n) * s


def i32(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(gpu)


# ---------------------------------------------------------------------------------------------------------------------
# vector and time-step entries: n = 513, 16-byte aligned (off = 0) and shifted by 8 bytes (off = 1)
# ---------------------------------------------------------------------------------------------------------------------
def vector_rows():
    def simple(name, entry, make):
        for off in (0, 1):
            def build(gpu, s, rng, request, make=make, off=off):
                vecs, call, outs = make(gpu, s, rng)
                return case(vecs, call, outs, off=off)
            ROWS.append((f"{name}-{'aligned' if off == 0 else 'shifted'}", (entry,), build))

    def la():
        from wave_fenics_amd import la as module
        return module

    simple("copy", "wf_copy", lambda gpu, s, rng: (
        {"x": uni(rng, N, s), "y": uni(rng, N, s)}, lambda t: la().copy(t["x"], t["y"]), ["y"]))
    simple("fill", "wf_fill", lambda gpu, s, rng: (
        {"y": uni(rng, N, s)}, lambda t: la().fill(t["y"], 2.5 * s), ["y"]))
    simple("axpy", "wf_axpy", lambda gpu, s, rng: (
        {"x": uni(rng, N, s), "y": uni(rng, N, s), "r": uni(rng, N, s)}, lambda t: la().axpy(t["r"], -0.75, t["x"], t["y"]), ["r"]))
    simple("scale", "wf_scale", lambda gpu, s, rng: (
        {"x": uni(rng, N, s)}, lambda t: la().scale(1.5, t["x"]), ["x"]))
    simple("pointwise_div", "wf_pointwise_div", lambda gpu, s, rng: (
        {"b": uni(rng, N, s), "m": rng.uniform(0.5, 1.5, N) * s, "out": uni(rng, N, s)},
        lambda t: la().pointwise_div(t["b"], t["m"], t["out"]), ["out"]))
    simple("pointwise_mult_add", "wf_pointwise_mult_add", lambda gpu, s, rng: (
        {"m": uni(rng, N, s), "x": uni(rng, N, s), "y": uni(rng, N, s)},
        lambda t: la().pointwise_mult_add(t["m"], t["x"], t["y"]), ["y"]))
    simple("dot", "wf_dot", lambda gpu, s, rng: (
        {"x": ints(rng, N, s), "y": ints(rng, N, s), "res": ints(rng, 1, s)},
        lambda t: ok(L().wf_dot(N, ptr(t["x"]), ptr(t["y"]), ptr(t["res"]), cur(t["x"]))), ["res"]))

    def indexed(fn, entry, unique, exact):
        def make(gpu, s, rng):
            from wave_fenics_amd import operators
            idx = rng.permutation(N) if unique else rng.integers(0, N // 4, N)
            d_idx = i32(gpu, idx)
            draw = ints if exact else uni
            vecs = {"in": draw(rng, N, s), "out": draw(rng, N, s)}
            return vecs, lambda t: getattr(operators, fn)(N, d_idx, t["in"], t["out"]), ["out"]
        return make
    simple("gather", "wf_gather", indexed("gather", "wf_gather", False, False))
    simple("scatter_add", "wf_scatter_add", indexed("scatter", "wf_scatter_add", False, True))
    simple("scatter_set", "wf_scatter_set", indexed("scatter_set", "wf_scatter_set", True, False))

    def transform1(gpu, s, rng):
        from wave_fenics_amd import operators
        return ({"in": uni(rng, N, s), "detJ": uni(rng, N, s), "out": uni(rng, N, s)},
                lambda t: operators.transform1(N, t["in"], t["detJ"], t["out"]), ["out"])
    simple("transform1", "wf_transform1", transform1)

    def segment_sum(gpu, s, rng):
        from wave_fenics_amd import operators
        off = np.concatenate([[0], np.cumsum(rng.integers(0, 4, N))])
        d_off = i32(gpu, off)
        return ({"vals": uni(rng, int(off[-1]), s), "y": uni(rng, N, s)},
                lambda t: operators.segment_sum_add(N, d_off, t["vals"], t["y"]), ["y"])
    simple("segment_sum_add", "wf_segment_sum_add", segment_sum)
    simple("memset", "wf_memset", lambda gpu, s, rng: (
        {"y": uni(rng, N, s)}, lambda t: ok(L().wf_memset(ptr(t["y"]), 0, 8 * (N - 1), cur(t["y"]))), ["y"]))

    def boundary_sets(rng, s, disjoint=False):
        """two sets of unique dofs with their facet masses: overlapping for the fused passes, whose plan gives every dof
        of the union one writer; disjoint for wf_boundary_apply, which adds by atomics, so that a dof of both sets would
        take its two terms in either order"""
        both = rng.choice(N, 298, replace=False)
        i1, i2 = np.sort(rng.choice(N, 97, replace=False)), np.sort(rng.choice(N, 201, replace=False))
        if disjoint:
            i1, i2 = np.sort(both[:97]), np.sort(both[97:])
        else:
            assert np.intersect1d(i1, i2).size > 0
        return i1.astype(np.int32), rng.uniform(0.5, 1.5, i1.size) * s, i2.astype(np.int32), rng.uniform(0.5, 1.5, i2.size) * s

    def boundary_apply(gpu, s, rng):
        i1, m1, i2, m2 = boundary_sets(rng, s, disjoint=True)
        d1, d2 = i32(gpu, i1), i32(gpu, i2)
        return ({"m1": m1, "m2": m2, "v": uni(rng, N, s), "b": uni(rng, N, s)},
                lambda t: la().boundary_apply(d1, t["m1"], 0.7 * s, d2, t["m2"], -1.3, t["v"], t["b"]), ["b"])
    simple("boundary_apply", "wf_boundary_apply", boundary_apply)

    def boundary_plan(gpu, s, rng):
        plan = la().BoundaryPlan(N, *boundary_sets(rng, s, disjoint=True))
        return {"v": uni(rng, N, s), "b": uni(rng, N, s)}, lambda t: plan.apply(0.7 * s, -1.3, t["v"], t["b"]), ["b"]
    simple("boundary_apply_plan", "wf_boundary_apply_plan", boundary_plan)

    def rk4(bc, has_next):
        def make(gpu, s, rng):
            names = ["b", "vn", "u_read", "v_read", "u", "v"] + (["u0", "v0", "un", "vn_next"] if has_next else [])
            vecs = {k: uni(rng, N, s) for k in names}
            vecs["m"] = rng.uniform(0.5, 1.5, N) * s
            plan = la().BoundaryPlan(N, *boundary_sets(rng, s)) if bc else None
            nxt = (lambda t: dict(u0=t["u0"], v0=t["v0"], un=t["un"], vn_next=t["vn_next"])) if has_next else (lambda t: {})
            return (vecs, lambda t: la().rk4_stage(t["b"], t["m"], t["vn"], t["u_read"], t["v_read"], t["u"], t["v"], 0.125, 0.5,
                                                    bc=plan, s1_next=0.7 * s, s2=-1.3, **nxt(t)),
                    ["b", "u", "v"] + (["un", "vn_next"] if has_next else []))
        return make
    for bc in (False, True):
        for has_next in (False, True):
            simple(f"rk4_stage{'_bc' if bc else ''}-{'next' if has_next else 'last'}", "wf_rk4_stage_bc" if bc else "wf_rk4_stage",
                   rk4(bc, has_next))

    def leapfrog(bc, with_v):
        def make(gpu, s, rng):
            names = ["b", "u", "u_prev", "u_next"] + (["v"] if with_v else [])
            vecs = {k: uni(rng, N, s) for k in names}
            vecs["m"] = rng.uniform(0.5, 1.5, N) * s
            plan = la().BoundaryPlan(N, *boundary_sets(rng, s)) if bc else None
            return (vecs, lambda t: la().leapfrog_step(t["b"], t["m"], t["u"], t["u_prev"], t["u_next"], 0.25, v=t.get("v"),
                                                        bc=plan, s1=0.7 * s, s2=-1.3),
                    ["b", "u_next"] + (["v"] if with_v else []))
        return make
    for bc in (False, True):
        for with_v in (False, True):
            simple(f"leapfrog_step{'_bc' if bc else ''}-{'v' if with_v else 'no-v'}", "wf_leapfrog_step_bc" if bc else "wf_leapfrog_step",
                   leapfrog(bc, with_v))
    simple("leapfrog_correlate", "wf_leapfrog_correlate", lambda gpu, s, rng: (
        {k: uni(rng, N, s) for k in ("lam", "up", "u", "um", "p")},
        lambda t: la().leapfrog_correlate(t["lam"], t["up"], t["u"], t["um"], t["p"]), ["p"]))


vector_rows()


# ---------------------------------------------------------------------------------------------------------------------
# points: P4, five points, two of them in cell 0
# ---------------------------------------------------------------------------------------------------------------------
def points_space(rng):
    import wave_fenics_amd as w
    V = w.create_functionspace(w.create_box((2, 2, 2)), 4)
    return V, (np.array([0, 0, 3, 5, 6], dtype=np.int32), rng.uniform(0.1, 0.9, (5, 3)))


@row("points_sample", "wf_points_sample")
def _(gpu, s, rng, request):
    from wave_fenics_amd import points
    V, located = points_space(rng)
    rec = points.Receivers(V, None, located=located)
    return case({"x": uni(rng, V.ndofs, s), "out": uni(rng, 5, s)}, lambda t: rec.sample(t["x"], t["out"]), ["out"], keep=rec)


@row("sources_add", "wf_sources_add")
def _(gpu, s, rng, request):
    from wave_fenics_amd import points
    V, located = points_space(rng)
    src = points.Sources(V, None, [points.ricker(1.0e6, 1.0e-6, s * (1 + i)) for i in range(5)], located=located)
    return case({"b": uni(rng, V.ndofs, s)}, lambda t: src.add(1.2e-6, t["b"]), ["b"], keep=src)


@row("sources_add_values", "wf_sources_add_values")
def _(gpu, s, rng, request):
    from wave_fenics_amd import points
    V, located = points_space(rng)
    src = points.Sources(V, None, [points.ricker(1.0e6, 1.0e-6, 1.0)] * 5, located=located)
    return case({"values": uni(rng, 5, s), "b": uni(rng, V.ndofs, s)}, lambda t: src.add_values(t["values"], t["b"], scale=0.5),
                ["b"], keep=src)


# ---------------------------------------------------------------------------------------------------------------------
# cell forms: P2 on GPU_BOX[2]
# ---------------------------------------------------------------------------------------------------------------------
def cell_form_row(name, kind, mesh_kind, tuning, geometry):
    @row(f"cell_form-{name}", "wf_cell_form_eval")
    def _(gpu, s, rng, request):
        import cell_form_helpers as cf
        import wave_fenics_amd as w
        V, om, _ = se.box_mesh(mesh_kind, tuple(cf.GPU_BOX[2]), 2)
        form = w.operators.CellForm(V, 2, kind=kind, params={"c0": se.C0}, tuning=tuning)
        assert form.geometry == geometry
        return case({"lam": uni(rng, V.ndofs, s), "u": uni(rng, V.ndofs, s), "out": uni(rng, om.ncells, s)},
                    lambda t: form.eval(t["lam"], t["u"], out=t["out"], alpha=0.5), ["out"], keep=form)


cell_form_row("stiffness-per-point", "stiffness", "perturbed", {"geometry": "per_point"}, "per_point")
cell_form_row("stiffness-per-cell", "stiffness", "sheared", {"geometry": "per_cell"}, "per_cell")
cell_form_row("lumped-mass", "mass_lumped", "perturbed", None, "none")


# ---------------------------------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------------------------------
def first_per_key(cases, key, always=lambda c: False):
    seen, out = set(), []
    for c in cases:
        if always(c) or key(c) not in seen:
            out.append(c)
        seen.add(key(c))
    return out


STIFFNESS_CASES = first_per_key(se.cases(), lambda c: c.want, lambda c: c.flags == "ordered")
MASS_CASES = first_per_key(me.cases(), lambda c: (c.op, c.kernel, "ORDERED" in c.flags))


def apply_case(op, ndofs, s, rng, x, tol):
    return case({"x": x * s, "y": uni(rng, ndofs, s)}, lambda t: op(t["x"], t["y"]), ["y"], tol=tol, keep=op)


def stiffness_row(c):
    @row(f"op-stiffness-{c.id}", "wf_op_apply")
    def _(gpu, s, rng, request):
        from test_gpu_stiffness_entries import operator
        V, om, _ = se.mesh_of(c)
        op = operator(c, V, None)                    # asserts (kernel, geometry, metric, update) == c.want
        x = np.random.default_rng(17 + c.p).uniform(-1, 1, om.ndofs)          # the uniform field of se.fields
        return apply_case(op, om.ndofs, s, rng, x, None if op.update in ("owner", "ordered") else TOL_FORM)


def mass_row(c):
    @row(f"op-mass-{c.id}", "wf_op_apply")
    def _(gpu, s, rng, request):
        from test_gpu_mass_entries import operator
        V, om, _ = me.mesh_of(c)
        t = me.table_of(c)
        detJ = me.detj_tables(om, t if c.op == "dense" else me.lumped_rule(c.p))[0] if c.source == "tables" else None
        d = SimpleNamespace(V=V, om=om, table=t, phi1=None if t is None else t.phi1, detJ=detJ)
        op = operator(c, d, None)                    # asserts the kernel
        x = np.random.default_rng(29 + c.p).uniform(-1, 1, om.ndofs)
        return apply_case(op, om.ndofs, s, rng, x, None if op.update == "ordered" else TOL_FORM)


for _c in STIFFNESS_CASES:
    stiffness_row(_c)
for _c in MASS_CASES:
    mass_row(_c)


def tet_row(name, module, small_name, make_op, reference):
    @row(f"op-{name}", "wf_op_apply")
    def _(gpu, s, rng, request):
        base = module().small(small_name)
        c = dataclasses.replace(base, x=base.x * s, y0=base.y0 * s)
        op = make_op(module(), c)
        _, mag = reference(module(), c)

        def check(name, got, ref):
            worst, good, where = ratio(got, np.asarray(ref, dtype=LD), mag, c.B)
            print(f"{small_name}: gated and default-stream applies differ by at most {worst:.3f} eps of the magnitude (B = {c.B})")
            assert good, (where, worst)
        return case({"x": c.x, "y": c.y0}, lambda t: op(t["x"], t["y"]), ["y"], check=check, keep=op)


def _tet_stiffness():
    import test_gpu_tet_dense_paths as m
    return m


def _tet_mass():
    import tet_mass_helpers as m
    return m


tet_row("tet-stiffness-P2_half_inverted", _tet_stiffness, "P2_half_inverted", lambda m, c: m.created(c, Op=m.DenseOp),
        lambda m, c: m.reference(c, True))
tet_row("tet-mass-P2_half_inverted", _tet_mass, "P2_half_inverted", lambda m, c: m.created(c), lambda m, c: m.reference(c))


@row("op_apply_part-owner-P2", "wf_op_apply_part")
def _(gpu, s, rng, request):
    """interior then interface on the gated stream; the twin is the whole apply"""
    import wave_fenics_amd as w
    from test_gpu_parts_matrix import NZ, cross_section
    from wave_fenics_amd._lib import WF_PART_INTERFACE, WF_PART_INTERIOR
    bx, by, select = cross_section("owner", 2)
    V, om, _ = se.box_mesh("graded", (bx + 1, by + 1, NZ), 2)
    op = w.StiffnessOperator(V, 2, {"c0": se.C0}, structured=True, tuning=dict(select, update="owner", lz=2, lz0=1))
    assert (op.kernel, op.update) == ("march_box", "owner") and op.set_ghost_faces(True, True, True)
    assert op.info.items_interior > 0 and op.info.items_interface > 0
    state = {"gated": True}

    def call(t):
        if state["gated"]:
            state["gated"] = False
            op.apply_part(t["x"], t["y"], WF_PART_INTERIOR)
            op.apply_part(t["x"], t["y"], WF_PART_INTERFACE)
        else:
            op(t["x"], t["y"])
    return case({"x": uni(rng, om.ndofs, s), "y": uni(rng, om.ndofs, s)}, call, ["y"], tol=TOL_FORM, keep=op)


# ---------------------------------------------------------------------------------------------------------------------
# the ghost exchange and the overlapped apply: one-rank periodic partition, native transport
# ---------------------------------------------------------------------------------------------------------------------
class Updater:
    """wf_updater_create with the flags of the row (the Python VectorUpdater always passes WF_UPDATER_DEFAULT)"""

    def __init__(self, part, comm, flags):
        from wave_fenics_amd._lib import UpdaterDesc, _ip
        g, nbp = part.ghosts, lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        d = UpdaterDesc(g.ndofs, len(g.send_neighbors), nbp(g.send_neighbors), _ip(g.send_offsets), _ip(g.send_indices),
                        len(g.recv_neighbors), nbp(g.recv_neighbors), _ip(g.recv_offsets), _ip(g.ghost_positions), flags)
        self.h = ctypes.c_void_p()
        ok(L().wf_updater_create(comm._h, ctypes.byref(d), ctypes.byref(self.h)))

    def __call__(self, fn, x):
        ok(getattr(L(), "wf_updater_" + fn)(self.h, ptr(x), cur(x)))

    def __del__(self):
        if self.h is not None and self.h.value:
            L().wf_updater_destroy(self.h)
            self.h = None


def partition(p):
    from wave_fenics_amd.distributed import create_distributed_box
    part = create_distributed_box(PARTITION["n"], p, 1, 0, periodic=PARTITION["periodic"], build_dofmap=True)
    assert not part.owned_mask().all()
    return part


def updater_row(direction, split, flags, fname):
    @row(f"updater-{direction}{'-split' if split else ''}-{fname}",
         *((f"wf_updater_{direction}_begin", f"wf_updater_{direction}_end") if split else (f"wf_updater_{direction}",)))
    def _(gpu, s, rng, request):
        from wave_fenics_amd import la
        part = partition(2)
        u = Updater(part, request.getfixturevalue("comm"), flags)
        owned = part.owned_mask()
        if direction == "fwd":
            x = np.where(owned, uni(rng, owned.size, s), -7.0)      # the ghosts start with a wrong value
        else:
            x = ints(rng, owned.size, s)                            # the owners' sums are exact in any order
        vecs = {"x": x, "z": uni(rng, N, s), "w": uni(rng, N, s)}

        def call(t):
            if split:
                u(direction + "_begin", t["x"])
                la.axpy(t["w"], 0.5, t["z"], t["z"])
                u(direction + "_end", t["x"])
            else:
                u(direction, t["x"])
        return case(vecs, call, ["x", "w"] if split else ["x"], keep=u)


def overlapped_row(p):
    @row(f"op_apply_overlapped-owner-P{p}", "wf_op_apply_overlapped")
    def _(gpu, s, rng, request):
        import wave_fenics_amd as w
        from wave_fenics_amd._lib import WF_UPDATER_DEFAULT
        part = partition(p)
        u = Updater(part, request.getfixturevalue("comm"), WF_UPDATER_DEFAULT)
        part.V.structured = True
        op = w.StiffnessOperator(part.V, p, {"c0": se.C0}, tuning={"update": "owner", "lz": 2, "lz0": 1})
        assert (op.kernel, op.update) == ("march_box", "owner") and op.set_ghost_faces(*[bool(v) for v in part.owned_lo])
        assert op.info.items_interior > 0 and op.info.items_interface > 0
        owned = part.owned_mask()
        vecs = {"x": np.where(owned, uni(rng, owned.size, s), -7.0), "y1": uni(rng, owned.size, s), "y2": uni(rng, owned.size, s)}

        def call(t):
            for y in ("y1", "y2"):      # back to back: the second records the updater's events while the first may use them
                ok(L().wf_op_apply_overlapped(op._h, u.h, ptr(t["x"]), ptr(t[y]), cur(t["x"])))
        return case(vecs, call, ["x", "y1", "y2"], tol=TOL_FORM, keep=(u, op))


def exchange_rows():
    from wave_fenics_amd._lib import WF_UPDATER_DEFAULT, WF_UPDATER_INLINE
    for flags, fname in ((WF_UPDATER_DEFAULT, "default"), (WF_UPDATER_INLINE, "inline")):
        for direction in ("fwd", "rev"):
            for split in (False, True):
                updater_row(direction, split, flags, fname)
    overlapped_row(2)
    overlapped_row(4)


exchange_rows()


@row("comm_allreduce", "wf_comm_allreduce")
def _(gpu, s, rng, request):
    c = request.getfixturevalue("comm")
    return case({"in": uni(rng, 5, s), "out": uni(rng, 5, s)}, lambda t: c.allreduce(t["in"], "sum", out=t["out"]), ["out"])


# ---- entries that synchronise by contract: at return the load has completed ----
@row("sync-synchronises", "wf_sync")
def _(gpu, s, rng, request):
    return case({"x": uni(rng, N, s)}, lambda t: ok(L().wf_sync(cur(t["x"]))), ["x"], sync=True)


@row("comm_barrier-synchronises", "wf_comm_barrier")
def _(gpu, s, rng, request):
    c = request.getfixturevalue("comm")
    return case({"x": uni(rng, N, s)}, lambda t: c.barrier(cur(t["x"])), ["x"], sync=True)


@row("cg-synchronises", "wf_cg")
def _(gpu, s, rng, request):
    """the lumped P1 mass of the box (2, 2, 2): four iterations (test_gpu_cg_iteration.py); wf_cg returns host values"""
    import wave_fenics_amd as w
    from wave_fenics_amd import la
    V = w.create_functionspace(w.create_box(2), 1)
    M = w.MassOperatorLumped(V, 1)
    b = rng.uniform(0.5, 1.5, V.ndofs) * s
    return case({"x": np.zeros(V.ndofs), "b": b}, lambda t: la.cg(t["x"], t["b"], M, kmax=4, rtol=0.0)[0], ["x"], tol=1e-12, sync=True,
                keep=M)


ENTRIES = {e for _, entries, _ in ROWS for e in entries}


@pytest.mark.parametrize("k", range(len(ROWS)), ids=[r[0] for r in ROWS])
def test_stream_order(gpu, oracle, request, k):
    rid, entries, build = ROWS[k]
    s = sh.factor(k)
    c = build(gpu, s, np.random.default_rng(1000 + k), request)
    work, good = sh.poisoned(gpu, c.vecs, c.off)
    # the gated call first: the first call in the process on this handle and with these values
    r = sh.gated(gpu, work, good, lambda: c.call(work), c.outs)
    (sh.require_completed if c.sync else sh.require_pending)(r, rid)
    ref, ref_result = sh.twin(gpu, work, good, lambda: c.call(work), c.outs)
    if isinstance(r.result, int):
        assert r.result == ref_result, (rid, "returned", r.result, ref_result)
    for name, got, want in zip(c.outs, r.snaps, ref):
        what = (rid, entries, name)
        if c.check is not None:
            c.check(name, got, want)
        elif c.tol is None:
            off = np.nonzero(bits(got) != bits(want))[0]
            assert off.size == 0, what + ("entries off the default-stream twin", off.size, "first", off[:8], got[off[:4]], want[off[:4]])
        else:
            assert np.isfinite(got).all(), what + ("not finite at", np.nonzero(~np.isfinite(got))[0][:8])
            err = float(np.abs(got - want).max() / np.abs(want).max())
            assert err <= c.tol, what + ("against the default-stream twin", err, c.tol)
