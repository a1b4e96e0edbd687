"""The interior / interface split (wf_op_set_ghost_faces, wf_op_set_ghost_dofs, wf_op_apply_part) as a matrix:
operator x z segmentation x ghost set, in guarded buffers (tests/guard_helpers.py).

The contract (include/wavehip.h, DESIGN "Interior / interface split"): an interface item reads a ghost value of x OR
ADDS INTO ONE OF y.  The interior parts run while the forward halo still writes x's ghost entries and the reverse halo
reads y's, so an interior item that reads or adds into a ghost position is a race that no single-stream comparison shows.
Here it shows: x is NaN at the ghost positions and in the padding, and y's ghost entries and padding must come back
bit for bit.

  operators (one default cross-section per degree; nz = 5, one cell more than a column holds in x and in y)
    point        P1-P4   k_stiffness_march, per-point geometry     8x8 5x5 4x4 5x2    perturbed box (BX+1, BY+1, 5)
    cell_full    P1-P4   per-cell full form                        the same           sheared affine box
    axes_atomic  P1-P4   per-cell axes form, update = atomic       the same           graded rectilinear box
    ksplit       P4-P7   k_march_ks (P4 as variant 3)              5x1 3x1 2x1 2x1    perturbed box
    owner        P1-P7   k_stiffness_owner                         16x16 8x8 5x5 8x2 5x2 2x3 2x2   graded box
    idx          P2 P4 P6  the dofmap kernels (structured=False)   7x4 5x2 2x1        perturbed box as a dofmap
  segmentations (lz, lz0)
    (2, 1)  [0,1) [1,3) [3,5) under a z ghost plane      (3, 2)  [0,2) [2,5)      (2, default)  the unsplit layout
    (the dofmap kernels have no short first segment: their items are the plan's, ceil(nz / lz) per column)
  ghost sets
    none; the lower planes x0, y0, z0 alone and together, through BOTH APIs on box operators; the upper planes x1, y1,
    z1 alone (I = NX-1, J = NY-1, K = NZ-1); z0 with x1; five single dofs of a fixed seed; one dof on a column
    boundary (I = P BX), one on the boundary plane of segment 1 (K = P z0), one P lines below a column (I = P BX - P,
    the owner form's halo)

Per (operator, segmentation, ghost set), for both y sentinels:
  1. INTERIOR, INTERIOR_A and INTERIOR_B, each on its own y0, with x = NaN at the ghosts: y finite everywhere;
  2. after each, y's ghost entries and all padding equal y0 bit for bit;
  3. INTERIOR + INTERFACE and A + INTERFACE + B against the whole apply: bit for bit for the P4 owner form (as
     test_gpu_owner_lane_exchange.py and test_gpu_owner_run_table.py), within TOL_FORM = 1e-13 of max|y| otherwise;
  4. the whole apply against the oracle within TOL_ORACLE = 1e-12;
  5. items_interior + items_interface == columns x segments, segments = 1 + ceil(max(nz - lz0s, 0) / lz) with
     lz0s = max(1, min(lz0 or 3, lz)) under a z ghost plane, else lz (the rule of wavehip.h / csrc/common.h, written
     out here); none: no interface item; any other set: some; the two APIs agree on the counts, and on the owner form
     on the bits of INTERIOR;
  6. a second wf_op_set_ghost_dofs replaces the first split (every ghost set here is installed over the previous one;
     at the end y0's split is installed over x1's and checks 1, 2 and 5 run again).

Covered before: lz0 < lz for the P4 per-point kernel (test_gpu_comm.py) and the owner forms
(test_gpu_owner_update.py, _high_degree.py, _lane_exchange.py); lower planes through both APIs at lz0 = lz for P4 /
P6 (test_gpu_parity.py::test_interior_interface_split, which reads x but never looks at y's ghost entries).  New: the
second half of the contract (no add into a ghost y) everywhere; a short first segment for the k-split kernel, the
per-cell forms and the per-point kernel at P1-P3; ghosts on upper faces and scattered in the interior."""
import numpy as np
import pytest

from guard_helpers import MIN_NORMAL, NAN, NEG_ZERO, box_pad, guarded
from nonbox_helpers import STIFFNESS_BLOCK
from support import bits, gpu, owner_columns  # noqa: F401
from test_gpu_guarded_buffers import C0, KS_SHAPES, MARCH_SHAPES, OWNER_SHAPES, columns, stiffness_box

pytestmark = pytest.mark.gpu

TOL_ORACLE = 1e-12   # of max|y_ref|
TOL_FORM = 1e-13     # of max|y|: tests/test_gpu_owner_update.py, parts against the whole apply
NZ = 5
SEGMENTATIONS = [(2, 1), (3, 2), (2, None)]
MARCH_DEFAULT = {1: 0, 2: 0, 3: 0, 4: 1}                      # kDefaultVariant, csrc/op_create_box.hip
OWNER_DEFAULT = {1: 0, 2: 0, 3: 0, 4: 1, 5: 1, 6: 2, 7: 0}    # the same and kOwnerDefaultHi
FAMILIES = {"point": ("perturbed", {"geometry": "per_point"}, ("march_box", "per_point", "none", "none")),
            "cell_full": ("sheared", {"geometry": "per_cell", "metric": "full"}, ("march_box", "per_cell", "full", "none")),
            "axes_atomic": ("graded", {"geometry": "per_cell", "metric": "axes", "update": "atomic"},
                            ("march_box", "per_cell", "axes", "atomic")),
            "ksplit": ("perturbed", {}, ("march_box", "per_point", "none", "none")),
            "owner": ("graded", {"update": "owner"}, ("march_box", "per_cell", "axes", "owner")),
            "idx": ("perturbed", {"kernel": "march"}, ("march_idx", "per_point", "none", "none"))}
OPERATORS = ([(f, p) for f in ("point", "cell_full", "axes_atomic") for p in range(1, 5)] + [("ksplit", p) for p in range(4, 8)]
             + [("owner", p) for p in range(1, 8)] + [("idx", p) for p in (2, 4, 6)])


def cross_section(family, p):
    """(BX, BY, tuning that selects it)"""
    if family in ("point", "cell_full", "axes_atomic"):
        bx, by = next(s[2:] for s in MARCH_SHAPES if s[:2] == (p, MARCH_DEFAULT[p]))
        return bx, by, {"variant": MARCH_DEFAULT[p]}
    if family == "ksplit":
        bx, by = next(s[1:] for s in KS_SHAPES if s[0] == p)
        return bx, by, {"variant": 3} if p == 4 else {}
    if family == "owner":
        bx, by = next(s[2:] for s in OWNER_SHAPES if s[:2] == (p, OWNER_DEFAULT[p]))
        return bx, by, {"variant": OWNER_DEFAULT[p]}
    return STIFFNESS_BLOCK[p] + ({},)


def segments(nz, lz, lz0, z_ghost_plane):
    lz0s = max(1, min(lz0 or 3, lz)) if z_ghost_plane else lz
    return 1 + -(-max(nz - lz0s, 0) // lz)


def ghost_sets(lattice, p, bx, lz):
    """[(name, positions, faces or None, holds the plane z0)]"""
    NX, NY, NZd = lattice
    lat = np.arange(NX * NY * NZd).reshape(NZd, NY, NX)
    x0, y0, z0 = lat[:, :, 0].ravel(), lat[:, 0, :].ravel(), lat[0].ravel()
    x1, y1, z1 = lat[:, :, NX - 1].ravel(), lat[:, NY - 1, :].ravel(), lat[NZd - 1].ravel()
    five = np.sort(np.random.default_rng(5).choice(lat[1:].ravel(), 5, replace=False))     # K >= 1: no z ghost plane
    sets = [("none", np.zeros(0, dtype=np.int64), (0, 0, 0), False),
            ("x0", x0, (1, 0, 0), False), ("y0", y0, (0, 1, 0), False), ("z0", z0, (0, 0, 1), True),
            ("x0 y0 z0", np.concatenate([x0, y0, z0]), (1, 1, 1), True),
            ("x1", x1, None, False), ("y1", y1, None, False), ("z1", z1, None, False),
            ("z0 x1", np.concatenate([z0, x1]), None, True),
            ("five dofs", five, None, False),
            ("column boundary", lat[1, 1, p * bx:p * bx + 1], None, False),
            # no z ghost plane: the first segment has lz layers and segment 1 starts at layer lz
            ("segment boundary", lat[p * lz, 1, 1:2], None, False),
            ("below a column", lat[1, 1, p * bx - p:p * bx - p + 1], None, False)]
    return [(name, np.asarray(g, dtype=np.int32), faces, zp) for name, g, faces, zp in sets]


class Bench:
    """one operator with its vectors, the whole apply per y sentinel, and the checks of one split"""

    def __init__(self, gpu, op, x, y0, yref, pad, bitwise, what):
        import torch
        self.gpu, self.op, self.x, self.y0, self.pad, self.bitwise, self.what = gpu, op, x, y0, pad, bitwise, what
        self.worst_parts = 0.0
        self.yall = {}
        for fill in (NEG_ZERO, MIN_NORMAL):
            xg, gx = guarded(x, pad, 0, NAN, gpu)
            yg, gy = guarded(y0, pad, 0, fill, gpu)
            op(xg, yg)
            torch.cuda.synchronize()
            assert gx.intact() and gy.intact(), (what, "whole apply", gx.changed()[:8], gy.changed()[:8])
            self.yall[fill] = yg.cpu().numpy()
            self.worst_oracle = float(np.abs(self.yall[fill] - yref).max() / np.abs(yref).max())
            assert self.worst_oracle <= TOL_ORACLE, (what, "whole apply against the oracle", self.worst_oracle)

    def parts(self, xg, fill, parts, tag):
        """y0 + the parts in turn, in a guarded y"""
        import torch
        yg, gy = guarded(self.y0, self.pad, 0, fill, self.gpu)
        for part in parts:
            self.op.apply_part(xg, yg, part)
        torch.cuda.synchronize()
        assert gy.intact(), tag + (parts, "y padding changed at", gy.changed()[:8])
        return yg.cpu().numpy()

    def check(self, name, gpos, mode):
        """checks 1 to 3 of the split that is installed; returns the INTERIOR result per y sentinel"""
        from wave_fenics_amd._lib import WF_PART_INTERFACE, WF_PART_INTERIOR, WF_PART_INTERIOR_A, WF_PART_INTERIOR_B
        x_nan = np.array(self.x)
        x_nan[gpos] = np.nan
        interior = {}
        for fill in (NEG_ZERO, MIN_NORMAL):
            tag = (self.what, name, mode, "y padding -0.0" if fill == 0.0 else "y padding 2^-1022")
            xg, gx = guarded(x_nan, self.pad, 0, NAN, self.gpu)
            for part in (WF_PART_INTERIOR, WF_PART_INTERIOR_A, WF_PART_INTERIOR_B):
                y = self.parts(xg, fill, (part,), tag)
                wrote = np.nonzero(bits(y[gpos]) != bits(self.y0[gpos]))[0]
                assert np.isfinite(y).all(), tag + (part, "read a ghost x: y not finite at", np.nonzero(~np.isfinite(y))[0][:8],
                                                    "ghost entries of y changed", wrote.size)
                assert wrote.size == 0, tag + (part, "added into ghost entries of y", gpos[wrote][:8])
                if part == WF_PART_INTERIOR:
                    interior[fill] = y
            assert gx.intact(), tag + ("x padding written at", gx.changed()[:8])
            xc, gxc = guarded(self.x, self.pad, 0, NAN, self.gpu)
            yall = self.yall[fill]
            for parts in ((WF_PART_INTERIOR, WF_PART_INTERFACE), (WF_PART_INTERIOR_A, WF_PART_INTERFACE, WF_PART_INTERIOR_B)):
                y = self.parts(xc, fill, parts, tag)
                err = float(np.abs(y - yall).max() / np.abs(yall).max())
                self.worst_parts = max(self.worst_parts, err)
                if self.bitwise:
                    off = np.nonzero(bits(y) != bits(yall))[0]
                    assert off.size == 0, tag + (parts, "entries off the whole apply", off.size, err)
                else:
                    assert err <= TOL_FORM, tag + (parts, "against the whole apply", err)
            assert gxc.intact(), tag
        return interior


@pytest.mark.parametrize("lz,lz0", SEGMENTATIONS, ids=[f"lz{a}-lz0{'default' if b is None else b}" for a, b in SEGMENTATIONS])
@pytest.mark.parametrize("family,p", OPERATORS, ids=[f"{f}-P{p}" for f, p in OPERATORS])
def test_parts_matrix(gpu, oracle, family, p, lz, lz0):
    import wave_fenics_amd as w
    kind, tuning, want = FAMILIES[family]
    bx, by, select = cross_section(family, p)
    n = (bx + 1, by + 1, NZ)
    V, x, y0, yref = stiffness_box(oracle, kind, n, p)
    tuning = dict(tuning, lz=lz, **select)
    box = family != "idx"
    if lz0 is not None and box:     # the dofmap kernels' items are the plan's: no first segment to shorten
        tuning["lz0"] = lz0
    op = w.StiffnessOperator(V, p, C0, structured=box, tuning=tuning)
    assert (op.kernel, op.geometry, op.metric, op.update) == want and op.info.plan_lz == lz
    ncols = owner_columns(n, p, bx, by) if family == "owner" else columns(n, bx, by)
    if not box:
        assert op.info.plan_items == ncols * -(-NZ // lz)
        assert op.set_ghost_faces(True, False, False) is False       # no lattice faces: the dofs API only
    what = f"{family} P{p} {bx}x{by} {n} lz {lz} lz0 {lz0}"
    bench = Bench(gpu, op, x, y0, yref, box_pad(V.lattice[0], V.lattice[1]), (family, p) == ("owner", 4), what)

    def install(mode, gpos, faces, z_plane):
        """installs the split over whatever split the operator has, checks the bookkeeping, returns the counts"""
        if mode == "faces":
            assert op.set_ghost_faces(*[bool(f) for f in faces])
        else:
            assert op.set_ghost_dofs(gpos)
        counts = (op.info.items_interior, op.info.items_interface)
        nseg = segments(NZ, lz, lz0, z_plane) if box else -(-NZ // lz)
        assert sum(counts) == ncols * nseg, (what, mode, counts, ncols, nseg)
        return counts

    seen = {}
    for name, gpos, faces, z_plane in ghost_sets(V.lattice, p, bx, lz):
        for mode in (("faces", "dofs") if box and faces is not None else ("dofs",)):
            counts = install(mode, gpos, faces, z_plane)
            seen[(name, mode)] = (counts, bench.check(name, gpos, mode))
            assert (counts[1] == 0) == (gpos.size == 0), (what, name, mode, "interface items", counts)
        if ("faces" in [m for (nm, m) in seen if nm == name]):
            (cf, yf), (cd, yd) = seen[(name, "faces")], seen[(name, "dofs")]
            assert cf == cd, (what, name, "item counts of the two APIs", cf, cd)
            if family == "owner":
                for fill in yf:
                    off = np.nonzero(bits(yf[fill]) != bits(yd[fill]))[0]
                    assert off.size == 0, (what, name, "INTERIOR of the two APIs differs in", off.size, "entries")
    # a second call replaces the first split: y0's over x1's
    sets = {name: (gpos, faces, z_plane) for name, gpos, faces, z_plane in ghost_sets(V.lattice, p, bx, lz)}
    install("dofs", *sets["x1"])
    assert install("dofs", *sets["y0"]) == seen[("y0", "dofs")][0]
    bench.check("y0 over x1", sets["y0"][0], "dofs")
    print(f"PARTS {family} {what}: oracle {bench.worst_oracle:.3e} parts {bench.worst_parts:.3e}")
