"""Every hexahedral mass kernel, entry by entry, against a long-double reference (tests/mass_entry_helpers.py).

The other tests of these kernels ask max|y - y_ref| <= 1e-12 max|y_ref| under x ~ U(-1, 1) and say nothing where the
field is quiet: a plane, a tile half or a det J set taken from the wrong buffer in a quiet layer passes them
(tests/test_mass_entry_host.py builds such mutants).  Here every entry of y = y0 + M x satisfies
|y_i - ref_i| <= B eps mag_i + derr_i, B derived in the helper's docstring (dense 3 n + 3 m + 10, lumped 10), on the
fields of the entry-wise stiffness tests: uniform; six decays over twelve decades; impulses at a vertex of eight cells,
at edge-, face- and cell-interior dofs and at the last dof (outside the impulse's cells y keeps the bits of y0); x = 1
with its known answer sum(y) = sum(d); and the uniform field under cell_coeff = 2^20 and 1 on the cells' checkerboard;
each with y0 = 0 and y0 = U(-1, 1) mag.  No entry is left out; an entry whose mag is 0 keeps the bits of y0.

The operators are created from the float64 tables the reference reads (phi1, det J w of the oracle: derr = 0, B alone
binds) except where the family says "library": there the library builds det J w itself and derr is the share of
hex_geometry_helpers.point_geometry_ld's bound, which is larger than B eps mag (test_mass_entry_host.py).  Each case
asserts op.kernel and, where there is a plan, its fields.

  march_segments  k_mass_march, all 23 entries of WF_MASS_SHAPES: perturbed box (BX + 1, BY + 1, 5), the cross-section
                  by wf_tuning.block, lz = 2: partly filled columns, items of 2, 2 and 1 layers
  march_deep      the default cross-section of each of the 17 pairs (P, M): box (BX + 1, BY + 1, 10), lz = 9: items of 9
                  and 1 layers, in which every cursor of the index ring wraps
  march_meshes    the holed "stair" mesh and a randomly re-oriented mesh at (2, 3), (2, 4), (4, 5), (4, 4); a table that
                  does not read the same backwards at (2, 4)
  column          k_mass_dense_col<P> P1..P7, square Gauss tables of degree 2 P, 2 CB + 1 cells ({"kernel": "batch"})
  any_rule        k_mass_dense: P1..P7 with m = n + 1, the GLL rules with m < n at P4..P7, one Gauss point at P2, a
                  square table under {"kernel": "mass_any"} at P3; 2 CB + 1 cells of its own batch size; P <= 3 with the
                  unique-dof tile and once more under {"kernel": "elementwise"} without it
  ordered         WF_FLAG_ORDERED: dense P2 rectangular and P5 square, lumped element-wise P2 and P5, the ordered
                  pre-assembled diagonal P3; two applies agree bit for bit
  lumped          P1..P7: the diagonal on a box created unstructured; the structured box (library det J: derr);
                  lumped_unique and lumped_elementwise on 2 CB + 1 cells; the stair mesh with NaN in the entries of x that
                  no cell names (k_diagonal_named)
  library         the rule-built dense constructor on the marching kernel (2, 4) and on the any-rule kernel (4, 6)

Out of scope: the grid-stride loops beyond 2048 batches keep their max-norm tests (tests/test_gpu_dense_mass_rules.py,
tests/test_gpu_batch_persistent.py): the meshes that reach them are too large for an entry-wise long-double reference;
the tetrahedral mass has tests/test_gpu_tet_mass.py.

Each case prints one line: B, the worst err / (eps mag) -- without derr -- over the fields and over the impulses with the
field it came from, and the largest share of the allowance B eps mag + derr that any entry uses.

Measured on the MI355X (a record, not the bound; worst err / (eps mag) per family: fields, impulses; largest share used):
  march_segments  B 22..58   1.90 (P3 M4 4x4, decay-y+)       3.02 (P7 M8 2x1, vertex8)         0.063
  march_deep      B 22..58   1.90 (P3 M4 4x4, decay-y+)       3.02 (P7 M8 2x1, vertex8)         0.063
  march_meshes    B 28..40   3.60 (oriented P4 M5, decay-y-)  9.33 (oriented P4 M5, edge-y)     0.233
  column          B 22..58   1.65 (P3, decay-x+)              2.94 (P7, face-yz)                0.060
  any_rule        B 22..61   1.89 (gll P5 M5, decay-z+)       2.04 (gll P7 M6, interior)        0.052
  ordered         B 10..46   1.24 (lumped P2, uniform)        1.92 (dense P5 M6, edge-y)        0.124
  lumped          B 10       1.50 (stair P6, hetero)          0.73 (stair P7, edge-y)           0.150   explicit det J w
  lumped box      B 10       4.55 (P3, decay-y+)              1.51 (P2, vertex8)                0.096   library det J w: derr
  library         B 31, 43   2.82 (march P2 M4, decay-y+)     1.88 (march P2 M4, edge-z)        0.028   library det J w: derr
No kernel exceeded its bound."""
import numpy as np
import pytest

import mass_entry_helpers as me
import stiffness_entry_helpers as se
from owner_helpers import apply
from support import EPS, LD, bits, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = me.cases()


def operator(case, d, a):
    import wave_fenics_amd as w
    flags = me.flag_bits(case)
    if case.op == "dense":
        if case.source == "library":
            variant, quad, qd = case.table[1][1:]
            op = w.MassOperator(d.V, case.p, variant=variant, quad=quad, qdegree=qd, tuning=case.tuning, flags=flags, cell_coeff=a)
            assert np.array_equal(op.points1, d.table.pts) and np.array_equal(op.weights1, d.table.wts)
        else:
            op = w.MassOperator(d.V, case.p, d.phi1, d.detJ, tuning=case.tuning, flags=flags, cell_coeff=a)
        assert op.num_quads() == d.table.m ** 3
    else:
        op = w.MassOperatorLumped(d.V, case.p, detJ=d.detJ, structured=case.structured, flags=flags, tuning=case.tuning,
                                  cell_coeff=a)
    what = (case.id, "coefficients" if a is not None else "")
    assert op.kernel == case.kernel, what + (op.kernel,)
    assert op.update == ("ordered" if case.kernel == "cells_ordered" else "none"), what
    assert op.cell_coeff == (a is not None) and op.num_cells() == d.om.ncells, what
    if case.plan:
        info = op.info
        assert info.plan_items > 0 and 0.0 < info.plan_fill <= 1.0, what
        if "lz" in case.plan:
            assert info.plan_lz == case.plan["lz"], what + (info.plan_lz,)
        if "items" in case.plan:
            assert info.plan_items == case.plan["items"] and info.plan_fill < 1.0, what + (info.plan_items,)
        if "reoriented" in case.plan:
            assert info.plan_reoriented == case.plan["reoriented"], what + (info.plan_reoriented,)
        if "reoriented_above" in case.plan:
            assert info.plan_reoriented > case.plan["reoriented_above"], what + (info.plan_reoriented,)
    return op


def test_case_count():
    assert len(CASES) == sum(me.NCASES.values()) == 23 + 17 + 9 + 7 + 18 + 5 + 35 + 2


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_entries(gpu, case):
    d = me.data(case)
    B = me.bound(case.op, case.p, None if d.table is None else d.table.m)
    worst, used = {"fields": (0.0, "-"), "impulses": (0.0, "-")}, 0.0
    op = operator(case, d, None)
    for f, name in enumerate(d.names):
        mag = d.mag[f]
        quiet = np.asarray(mag == 0)
        x = np.array(d.X[f])
        if case.nan:
            x[~d.named] = np.nan                 # entries no cell names: the apply must not read them into y
            assert quiet[~d.named].all()
        for y0 in (np.zeros(d.om.ndofs), me.scaled_y0(mag, 5 + f)):
            tag = (case.id, name, "y0 = U mag" if y0.any() else "y0 = 0")
            y = apply(op, x, y0, gpu)
            r, ok, at, u = se.entry_check(y, y0, d.ax[f], mag, d.derr[f], B)
            key = "impulses" if name in d.impulses else "fields"
            worst[key], used = max(worst[key], (r, name)), max(used, u)
            assert ok, tag + ("entry", at, "err / (eps mag)", r, "B", B)
            if case.twice:
                assert np.array_equal(bits(apply(op, x, y0, gpu)), bits(y)), tag + ("two applies differ",)
            if y0.any():
                # where no cell with a non-zero x_e reaches, every contribution is an exact zero: y0 + 0.0 keeps its bits
                off = np.nonzero(bits(y[quiet]) != bits(y0[quiet]))[0]
                assert off.size == 0, tag + ("y0 not kept at", np.nonzero(quiet)[0][off][:8])
                if name in d.impulses:
                    assert quiet[~se.support_of(d.om, d.impulses[name])].all(), tag
            if name == "ones":
                # the known answer: sum(M 1) = sum(d), up to the entries' allowance and the table's row-sum residue
                total = np.sum(y.astype(LD) - y0.astype(LD))
                allow = LD(B) * LD(EPS) * np.sum(np.abs(y0).astype(LD) + mag) + np.sum(d.derr[f]) + d.slack
                assert abs(total - np.sum(d.d)) <= allow, tag + ("sum(y) - sum(d)", float(total - np.sum(d.d)), float(allow))
    oph = operator(case, d, d.a)
    x = np.array(d.X[0])
    if case.nan:
        x[~d.named] = np.nan
    for y0 in (np.zeros(d.om.ndofs), me.scaled_y0(d.magh, 3)):
        y = apply(oph, x, y0, gpu)
        r, ok, at, u = se.entry_check(y, y0, d.axh, d.magh, d.derrh, B)
        worst["fields"], used = max(worst["fields"], (r, "hetero")), max(used, u)
        assert ok, (case.id, "hetero", "y0 = U mag" if y0.any() else "y0 = 0", "entry", at, "err / (eps mag)", r, "B", B)
        if case.twice:
            assert np.array_equal(bits(apply(oph, x, y0, gpu)), bits(y)), (case.id, "hetero", "two applies differ")
    print(f"MASS gpu {case.id}: B {B}, err / (eps mag) fields {worst['fields'][0]:.2f} ({worst['fields'][1]}) impulses "
          f"{worst['impulses'][0]:.2f} ({worst['impulses'][1]}), of the allowance B eps mag + derr at most {used:.3f}")
