"""Every hexahedral stiffness kernel, entry by entry, against a long-double reference (tests/stiffness_entry_helpers.py).

The other tests of these kernels ask max|y - y_ref| <= 1e-12 max|y_ref| under x ~ U(-1, 1): some 4000 roundings at the
loudest entry, and no statement at all where the field is quiet.  Here every entry of y = y0 + A x satisfies
|y_i - ref_i| <= B eps mag_i (+ the share of the reference geometry's own bound), B derived in the helper's docstring,
on fields that put quiet entries next to loud ones:

  uniform     U(-1, 1): puts a number on each kernel's rounding
  decay       u_i 2^(-40 s_i) along x, y, z, ascending and descending: twelve decades, the quiet end once in the first
              column or z segment and once in the partial last one
  impulse     e_d at a mesh vertex shared by 8 cells; from P2 on at an edge-interior dof shared by 4 cells along each of
              x, y, z, a face-interior dof shared by 2 cells in each orientation and a cell-interior dof, chosen by
              element-local index (the columns 1..P-1 of D); the last dof, a corner (the owner form's closing line):
              inside the cells of d the entry bound; outside them y keeps the bits of y0
  null space  x = 1, and x = a . X + b on the affine meshes: K x is about 1e-16 of its magnitude in every row (of the
              linear field: every interior row), which the bound sees and 1e-12 max|y| of another field does not
  hetero      the uniform field under cell_coeff = 2^20 and 1 on the cells' checkerboard: loud cells beside quiet ones

each with y0 = 0 and with y0_i = U(-1, 1) mag_i.  No entry is left out; an entry whose mag is 0 (a dof no cell names)
keeps the bits of y0.  On the perturbed meshes at P4 and above the -1/0/1 clamp changes entries of G; the reference
clamps too (window margin >= 1e-3, asserted in test_stiffness_entry_host.py), so the bound applies unchanged.

Families, cross-sections and tunings are those of tests/test_gpu_guarded_buffers.py (the first cross-section of each
degree; that file walks the others), and each case asserts op.kernel / geometry / metric / update:

  march_point / march_cell_full / march_axes_atomic   P1-P4   perturbed / sheared / graded box (BX+1, BY+1, 5), lz = 2
  ksplit                                              P4 (variant 3), P5-P7   perturbed box, same shape
  owner                                               P1-P7   graded box (BX+1, BY+1, 5) and the exact multiple (BX, BY, 4)
  box_block                                           P1-P7   perturbed box, block + 1 cells per axis
  idx                                                 k_march_idx P1-P4 (per point, per cell full, per cell axes), the
                                                      k-split kernel's dofmap form P5-P7; the holed "stair" P1-P7
  batch                                               k_stiffness_generic_up2 P1-P4, _up P5-P7, k_stiffness_generic
                                                      (element-wise) P1-P7, on the first 2 B + 1 cells of a perturbed box
  ordered                                             WF_FLAG_ORDERED stiffness P2, P5, the batch meshes
k_stiffness_generic_u, which the issue names, is not in the library as built: csrc/stiffness_batch.hip instantiates and
launches it only under -DWF_DIAG or -DWF_GENERIC_PIPELINED=0.  It has no case here, as it has none in
test_gpu_guarded_buffers.py.

Each case prints one line: B, the worst err / (eps mag) -- a plain figure, without the geometry's share -- over the uniform,
decay, null-space and heterogeneous fields and over the impulses, with the field it came from, and the largest fraction
of its allowance B eps mag + gerr that any entry uses.  Under an impulse an entry can hang on a single off-diagonal G(q),
whose float64 value is exact to an eps of the DIAGONAL (the cancellation in J^-1 J^-T): there the plain figure of the
per-point kernels runs into the hundreds and thousands, all of it inside G_bound, and stays below 4 on the affine meshes,
whose G_c comes from the edge vectors.  Said plainly: at those entries of the perturbed meshes gerr is up to 1e4 B eps
mag, so there the test holds a kernel to the geometry reference's pessimistic running-error bound and not to B; B is
what binds on the affine meshes (gerr about 1.5 B eps mag) and, on the perturbed ones, under the other fields, where the
measured figures stay below B without gerr."""
import numpy as np
import pytest

import stiffness_entry_helpers as se
from owner_helpers import apply
from support import bits, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = se.cases()


def operator(case, V, a):
    import wave_fenics_amd as w
    from wave_fenics_amd._lib import WF_FLAG_ORDERED
    flags = WF_FLAG_ORDERED if case.flags == "ordered" else 0
    op = w.StiffnessOperator(V, case.p, {"c0": se.C0}, structured=case.structured, flags=flags, tuning=case.tuning, cell_coeff=a)
    assert (op.kernel, op.geometry, op.metric, op.update) == case.want, (case.id, "coefficients" if a is not None else "")
    if case.tuning and "lz" in case.tuning:
        assert op.info.plan_lz == se.LZ
    assert op.cell_coeff == (a is not None)
    return op


def test_cases_are_the_guarded_buffer_families():
    import test_gpu_guarded_buffers as g
    assert (se.BLOCKS, se.BATCH_BOX, se.NZ, se.LZ, se.C0) == (g.BLOCKS, g.BATCH_BOX, g.NZ, g.LZ, g.C0["c0"])
    for family, (kind, tuning, want) in g.MARCH_FORMS.items():
        mine = [c for c in CASES if c.family == family]
        assert [c.p for c in mine] == [1, 2, 3, 4]
        for c in mine:
            assert c.mesh[1][0] == kind and c.want == want + ("none",) * (4 - len(want))
            assert {k: v for k, v in c.tuning.items() if k not in ("variant", "lz")} == tuning
    assert len(CASES) == 12 + 4 + 14 + 7 + 15 + 7 + 14 + 2


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_entries(gpu, case):
    d = se.data(case)
    B = se.bound(case.form, case.p)
    worst, used = {"fields": (0.0, "-"), "impulses": (0.0, "-")}, 0.0
    op = operator(case, d.V, None)
    if case.family == "owner":
        assert len(op.runs()) == 0
    for f, name in enumerate(d.names):
        mag = d.mag[f]
        quiet = np.asarray(mag == 0)
        for y0 in (np.zeros(d.om.ndofs), se.scaled_y0(mag, 5 + f)):
            tag = (case.id, name, "y0 = U mag" if y0.any() else "y0 = 0")
            y = apply(op, d.X[f], y0, gpu)
            r, ok, at, u = se.entry_check(y, y0, d.ax[f], mag, d.gerr[f], B)
            key = "impulses" if name in d.impulses else "fields"
            worst[key], used = max(worst[key], (r, name)), max(used, u)
            assert ok, tag + ("entry", at, "err / (eps mag)", r, "B", B)
            if y0.any():
                # where no cell with a non-zero x_e reaches (outside an impulse's support, dofs no cell names), every
                # contribution is an exact zero: a store or an atomic of y0 + 0.0 keeps the bits of y0
                off = np.nonzero(bits(y[quiet]) != bits(y0[quiet]))[0]
                assert off.size == 0, tag + ("y0 not kept at", np.nonzero(quiet)[0][off][:8])
                if name in d.impulses:
                    assert quiet[~se.support_of(d.om, d.impulses[name])].all(), tag
    oph = operator(case, d.V, d.a)
    for y0 in (np.zeros(d.om.ndofs), se.scaled_y0(d.magh, 3)):
        y = apply(oph, d.X[0], y0, gpu)
        r, ok, at, u = se.entry_check(y, y0, d.axh, d.magh, d.gerrh, B)
        worst["fields"], used = max(worst["fields"], (r, "hetero")), max(used, u)
        assert ok, (case.id, "hetero", "y0 = U mag" if y0.any() else "y0 = 0", "entry", at, "err / (eps mag)", r, "B", B)
    print(f"ENTRY gpu {case.id}: B {B}, err / (eps mag) fields {worst['fields'][0]:.2f} ({worst['fields'][1]}) impulses "
          f"{worst['impulses'][0]:.2f} ({worst['impulses'][1]}), of the allowance B eps mag + gerr at most {used:.3f}")
