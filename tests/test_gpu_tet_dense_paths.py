"""Every path of the dense simplex operator (csrc/stiffness_dense.hip), entry by entry, against long double.

The operator is created through the C ABI (`DenseDesc`, `wf_op_create_dense_simplex`) so that the module hands over its
own tables, dofmaps, geometry and flags.  What each group of cases reaches in `launch_stiffness_dense` /
`k_stiffness_dense` (NCB = 64 cells per batch, numax = most unique dofs of a batch, G = min(nbatch, 512) workgroups):

  case                                   instantiation <QT,KT,DT,4,NU,XR>    path
  P1_n*, P2_*                            <1,1,1,.,5,0> / <1,3,1,.,5,0>       X = 0 shapes of the Lagrange tables
  g3x5, g11x13                           the same two                         X = 0 with padded rows (nd % 4 != 0) and points
  P3_control, P3_scattered               <2,5,2,.,5,4>                        XR = 4 extra rows, numax <= 1280
  P3_broken                              <2,5,2,.,5,4>                        numax == 1280: every slot of NU = 5 in use
  g18x20                                 <2,5,2,.,5,0>                        the X = 0 form of the P3 tiles (nd = 18)
  P4_control, P4_n1 .. n17, P4_n129      <4,9,3,.,5,3>                        XR = 3, numax <= 1280; LDS on both sides of 64 KB
                                                                              (P4_n1: 59 KB, P4_control: above, numax > 416)
  P4_scattered, P4_broken, P4_n63 .. n65 <4,9,3,.,9,3>                        NU = 9; LDS 86 to 96 KB -> hipFuncSetAttribute
  g33x50_*, g34x64_*                     <4,9,3,.,5 and 9,0>                  X = 0 form of the P4 tiles, both NU
  g36x64_broken                          <4,9,3,.,9,0>                        numax == 2304 = 9 * 256: every slot of NU = 9
  P4q4_control, P4q4_scattered           <2,9,3,.,5 and 9,3>                  P4 with the 27-point rule
  g36x17_*                               <2,9,3,.,5 and 9,0>                  its X = 0 form
  clamp_one, clamp_zero, clamp_partial   <4,9,3,.,5,3>                        clamp_here on (flags 0) and off (WF_FLAG_NO_CLAMP
                                                                              on marked batches; unmarked batches of clamp_partial)
  *_all_inverted, *_half_inverted        P2 and P4                            det J < 0 (fabs in dense_setup) in every cell / in a
                                                                              random half and det J > 0 in the rest; a Kuhn box
                                                                              as it comes alternates (three cells of six per cube)
  P2_b511 ... P2_b1538, P4_b513          NU = 5 / NU = 9                      nbatch > 512: the persistent loop with its three
                                                                              prefetch stages (b + G, b + 2G, b + 3G), a last round
                                                                              with one live workgroup, a last batch of one cell

64 nd > 1280 needs nd > 20, so NU = 9 exists for the nd = 33 .. 36 shapes only (KT = 9); for KT <= 5 the NU = 9
instantiations are compiled but no input can select them.  The NU, LDS and batch-count claims above are asserted from the
dofmaps by test_cases_are_what_they_name (no GPU needed), not taken on trust.

References.  (a) The float64 oracle (oracle_stiffness_apply) fed with G[c][q] = J^-1 |det J| w_q J^-T built here, with the
-1/0/1 clamp or without according to the flag under test: max|got - ref| <= 1e-12 max|ref|, the tolerance of
test_tet_dense_stiffness_vs_oracle, for every case.  (b) For the small cases the same expression in long double (numpy,
np.add.at over the dofmap), which also returns the magnitude of every entry,
    mag = |y0| + sum_cells |dphi|^T |G| |dphi| |x| c0^2,
and the entry check |got - ref| <= B eps mag with B = nd + 3 nq + v + 8, v = most cells sharing one dof.  B is derived, not
measured: a sum of n products evaluated in any order (MFMA k-steps, fma chains, atomics in LDS and in global memory) is
within n u (1 + O(u)) of its magnitude, u = eps / 2; the chain of one entry is the first contraction (nd terms), the 3x3
product with G (3 terms), the second contraction (3 nq terms) and the sum over the cells of the dof and y0 (v + 1 terms),
each stage's relative error adding up: (nd + 3 + 3 nq + v + 1) u.  Forming G itself (J, its cofactors and determinant,
K |det J| K^T, w_q C, the scale by c0^2) is a fixed number of operations; its error is bounded by a small multiple of
eps max|G_c|, which the remaining nd/2 + 3 nq/2 + v/2 + 8 covers for the cells of these meshes (perturbation 0.2: the
entries of |G_c| are within a factor 10 of each other on the diagonal).  The float64 oracle itself stays far inside B
(test_reference_headroom, no GPU needed), so the reference is checked against something that is not the kernel.

The clamp: every crafted product w_q C_e lies a factor 3 inside its window (the kernel forms w C in another order
than the references), every other product a factor 3 outside; the random meshes are checked to have no product within
1e-6 (relative) of a window edge.  `y` is non-zero on entry everywhere; no entry is skipped or masked."""
import ctypes
import functools
import time
from dataclasses import dataclass, field

import numpy as np
import pytest

from support import EPS, LD, gpu, ratio, relerr, wlib  # noqa: F401
from tet_mass_helpers import NCB, batch_unique, created, cross, generic_parts, lagrange_tables, named_cases, nu_of

gpu_test = pytest.mark.gpu

C0 = 1500.0
GRID = 512                        # workgroups of the persistent grid
TOL = 1e-12                       # max-norm tolerance against the float64 oracle
WIN0, WIN1 = 1e-8, 1e-8 + 1e-5    # half widths of the clamp windows at 0 and at +-1 (np.isclose defaults)
NO_CLAMP = 2                      # WF_FLAG_NO_CLAMP
PAD = 16                          # sentinel entries around a shifted vector
SENTINEL = -7.0e77
WORST = {}                        # (nd, nq, NU) -> (worst ratio, its B)
T0 = time.time()


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    nd: int
    nq: int
    dphi: np.ndarray          # [3][nq][nd]
    W: np.ndarray             # [nq]
    xv: np.ndarray            # [nverts][3]
    gd: np.ndarray            # [ncells][4] int32
    dm: np.ndarray            # [ncells][nd] int32
    ndofs: int
    x: np.ndarray
    y0: np.ndarray
    inverted: np.ndarray = field(default=None)   # orientation cases: the cells that were given det J < 0

    @property
    def ncells(self):
        return int(self.gd.shape[0])

    @property
    def nbatch(self):
        return (self.ncells + NCB - 1) // NCB

    @property
    def v(self):
        return int(np.bincount(self.dm.reshape(-1)).max())

    @property
    def B(self):
        return self.nd + 3 * self.nq + self.v + 8


def lds_bytes(case):
    QT, KT = (case.nq + 15) // 16, (case.nd + 3) // 4
    return 8 * (3 * 16 * QT * (4 * KT + 2) + 16 * QT + 2 * int(batch_unique(case.dm).max()))


def vectors(rng, ndofs):
    return rng.uniform(-1.0, 1.0, ndofs), rng.uniform(-1.0, 1.0, ndofs) * 1e3


def mesh_case(name, p, n, *, qdegree=None, perturb=0.2, ncells=None, shuffle=False, renumber=False, broken=False,
              invert=0.0, scale=1.0, shear=0.0, seed=0):
    """Kuhn box of degree p, then: a subset of `ncells` cells, a random cell order, a random permutation of the dof
    numbers, a dofmap in which every cell has dofs of its own, a fraction `invert` of the cells with det J < 0 and
    every other cell with det J > 0 (vertices 1 and 2 swapped where the sign has to change)."""
    from wave_fenics_amd import tet
    V = tet.create_kuhn_box(n, p, perturb=perturb)
    rng = np.random.default_rng(seed)
    xv = np.array(V.x, dtype=np.float64)
    if shear:
        xv[:, 0] += shear * xv[:, 1]
    xv *= scale
    cells = np.arange(V.ncells)
    if ncells is not None:
        assert ncells <= V.ncells
        cells = np.sort(rng.choice(V.ncells, ncells, replace=False))
    if shuffle:
        cells = rng.permutation(cells)
    gd, dm, ndofs = V.geom_dofmap[cells].copy(), V.dofmap[cells].copy(), V.ndofs
    if renumber:
        dm = rng.permutation(ndofs).astype(np.int32)[dm]
    if broken:
        ndofs = dm.size
        dm = np.arange(ndofs, dtype=np.int32).reshape(dm.shape)
    inverted = None
    if invert:
        # (three of the six Kuhn tetrahedra of a cube have det J < 0 as they come; here the sign is the case's choice)
        inverted = np.ones(gd.shape[0], dtype=bool) if invert >= 1.0 else rng.random(gd.shape[0]) < invert
        swap = (jacobian(xv, gd, np.float64)[3] < 0.0) != inverted
        gd[swap] = gd[swap][:, [0, 2, 1, 3]]
    q = 2 * p - 2 if qdegree is None else qdegree
    dphi, W = lagrange_tables(p, (q + 2) // 2, gradients=True)
    x, y0 = vectors(rng, ndofs)
    return Case(name, dphi.shape[2], dphi.shape[1], dphi, W, np.ascontiguousarray(xv), np.ascontiguousarray(gd, dtype=np.int32),
                np.ascontiguousarray(dm, dtype=np.int32), ndofs, x, y0, inverted)


def generic_case(name, nd, nq, ncells, pool, seed):
    """Gradient tables and weights from a seeded generator (tet_mass_helpers.generic_parts)."""
    rng, dphi, W, xv, gd, dm, ndofs = generic_parts(nd, nq, ncells, pool, seed, (3, nq, nd))
    x, y0 = vectors(rng, ndofs)
    return Case(name, nd, nq, dphi, W, xv, gd, dm, ndofs, x, y0)


def c6(case):
    """the six distinct entries of C_c = |det J| J^-1 J^-T in float64, [c][6] (00 01 02 11 12 22)"""
    C = cell_tensor(case.xv, case.gd, np.float64)
    return C[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]


def products(case):
    """|w_q C_e| for every cell, point and entry: what dense_setup tests against the clamp windows"""
    return np.abs(case.W[None, :, None] * c6(case)[:, None, :])


def in_window(a):
    return ((a > 0.0) & (a <= WIN0)) | ((a != 1.0) & (np.abs(a - 1.0) <= WIN1))


def batch_marks(case):
    """the clampb array of dense_setup: batches with a product inside a clamp window"""
    hit = in_window(products(case)).any(axis=(1, 2))
    return np.array([hit[b:b + NCB].any() for b in range(0, case.ncells, NCB)])


def clamp_box(n, scale=1.0, shear=0.0):
    return mesh_case("tmp", 4, n, perturb=0.0, scale=scale, shear=shear, seed=77)


def clamp_one_scale(n):
    """the scale that puts the largest product w_q C_e of the unperturbed box at 1 + 3e-6 (G is linear in the scale)"""
    return (1.0 + 3e-6) / products(clamp_box(n)).max()


def clamp_zero_shear(n):
    """the shear x += g y that puts the largest of the products it makes non-zero at 3e-9 (they are linear in g)"""
    g0 = 1e-7
    a = products(clamp_box(n, shear=g0))
    new = a[(a > 0.0) & (a < 1e-6)]
    assert new.size, "the shear creates no small product"
    return g0 * 3e-9 / new.max()


def clamp_partial_case():
    """a scaled copy (window at 1 hit) followed by an unscaled copy of one box, no vertex or dof in common:
    batches 0 and 1 hold scaled cells, batch 2 none"""
    n = (4, 2, 2)
    a, b = clamp_box(n, scale=clamp_one_scale(n)), clamp_box(n)
    xb = b.xv.copy()
    xb[:, 0] -= 1.5
    rng = np.random.default_rng(78)
    x, y0 = vectors(rng, a.ndofs + b.ndofs)
    return Case("clamp_partial", a.nd, a.nq, a.dphi, a.W, np.concatenate([a.xv, xb]),
                np.concatenate([a.gd, b.gd + a.xv.shape[0]]).astype(np.int32),
                np.concatenate([a.dm, b.dm + a.ndofs]).astype(np.int32), a.ndofs + b.ndofs, x, y0)


SMALL_COUNTS = [1, 15, 16, 17, 63, 64, 65, 129]
BATCH_COUNTS = {511: 511 * NCB, 512: 512 * NCB, 513: 513 * NCB, 1024: 1024 * NCB, 1025: 1025 * NCB,
                1537: 1536 * NCB + 1,      # three whole rounds, then one workgroup with a batch of one cell
                1538: 1537 * NCB + 1}      # the other reading of "1537 batches plus one cell"

SMALL = {
    # unique-tile size
    "P3_control": lambda: mesh_case("P3_control", 3, (3, 3, 2), seed=1),
    "P4_control": lambda: mesh_case("P4_control", 4, (3, 2, 2), seed=2),
    "P3_scattered": lambda: mesh_case("P3_scattered", 3, (4, 4, 4), shuffle=True, renumber=True, seed=3),
    "P4_scattered": lambda: mesh_case("P4_scattered", 4, (4, 4, 4), shuffle=True, renumber=True, seed=4),
    "P3_broken": lambda: mesh_case("P3_broken", 3, (3, 3, 3), ncells=130, broken=True, seed=5),
    "P4_broken": lambda: mesh_case("P4_broken", 4, (3, 3, 3), ncells=130, broken=True, seed=6),
    "g36x64_broken": lambda: generic_case("g36x64_broken", 36, 64, 130, None, 7),
    # shapes
    "P4q4_control": lambda: mesh_case("P4q4_control", 4, (3, 2, 2), qdegree=4, seed=8),
    "P4q4_scattered": lambda: mesh_case("P4q4_scattered", 4, (4, 4, 4), qdegree=4, shuffle=True, renumber=True, seed=9),
    "g3x5": lambda: generic_case("g3x5", 3, 5, 150, 120, 10),
    "g11x13": lambda: generic_case("g11x13", 11, 13, 150, 500, 11),
    "g18x20": lambda: generic_case("g18x20", 18, 20, 150, 900, 12),
    "g33x50_shared": lambda: generic_case("g33x50_shared", 33, 50, 150, 1100, 13),
    "g33x50_spread": lambda: generic_case("g33x50_spread", 33, 50, 150, 30000, 14),
    "g34x64_shared": lambda: generic_case("g34x64_shared", 34, 64, 150, 1200, 15),
    "g34x64_spread": lambda: generic_case("g34x64_spread", 34, 64, 150, 30000, 16),
    "g36x17_shared": lambda: generic_case("g36x17_shared", 36, 17, 150, 1280, 17),
    "g36x17_spread": lambda: generic_case("g36x17_spread", 36, 17, 150, 30000, 18),
    # clamp
    "clamp_one": lambda: clamp_box((2, 2, 1), scale=clamp_one_scale((2, 2, 1))),
    "clamp_zero": lambda: clamp_box((2, 2, 1), shear=clamp_zero_shear((2, 2, 1))),
    "clamp_partial": clamp_partial_case,
    # orientation
    "P2_all_inverted": lambda: mesh_case("P2_all_inverted", 2, (3, 2, 2), invert=1.0, seed=19),
    "P2_half_inverted": lambda: mesh_case("P2_half_inverted", 2, (3, 2, 2), invert=0.5, seed=20),
    "P4_all_inverted": lambda: mesh_case("P4_all_inverted", 4, (3, 2, 2), invert=1.0, seed=21),
    "P4_half_inverted": lambda: mesh_case("P4_half_inverted", 4, (3, 2, 2), invert=0.5, seed=22),
}
for _p in (1, 4):
    for _n in SMALL_COUNTS:
        SMALL[f"P{_p}_n{_n}"] = functools.partial(mesh_case, f"P{_p}_n{_n}", _p, (3, 3, 3), ncells=_n, seed=100 * _p + _n)
CLAMP_CASES = ["clamp_one", "clamp_zero", "clamp_partial"]
NU9_CASES = ["P4_scattered", "P4_broken", "g36x64_broken", "P4q4_scattered", "g33x50_spread", "g34x64_spread", "g36x17_spread",
             "P4_n63", "P4_n64", "P4_n65"]     # (63 to 65 cells picked at random out of 162 share few dofs)

BIG = {f"P2_b{nb}": functools.partial(mesh_case, f"P2_b{nb}", 2, (26, 26, 25), ncells=nc, seed=nb)
       for nb, nc in BATCH_COUNTS.items()}
BIG["P4_b513"] = lambda: mesh_case("P4_b513", 4, (18, 18, 17), ncells=513 * NCB, shuffle=True, renumber=True, seed=513)
small = named_cases(SMALL)


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def jacobian(xv, gd, dtype):
    """columns of J (edge vectors v_j - v_0) and det J of every cell"""
    xc = np.asarray(xv, dtype=dtype)[gd]
    a, b, c = xc[:, 1] - xc[:, 0], xc[:, 2] - xc[:, 0], xc[:, 3] - xc[:, 0]
    return a, b, c, np.sum(a * cross(b, c), axis=1)


def cell_tensor(xv, gd, dtype):
    """C_c = J^-1 |det J| J^-T, [c][3][3]; the rows of J^-1 are the cross products of the columns of J over det J"""
    a, b, c, det = jacobian(xv, gd, dtype)
    K = np.stack([cross(b, c), cross(c, a), cross(a, b)], axis=1) / det[:, None, None]
    return np.einsum("cik,cjk->cij", K * np.abs(det)[:, None, None], K)


def clamp101(G):
    """the -1/0/1 clamp of precomputation.hpp:105-107 (np.isclose with its default tolerances), any dtype"""
    G = G.copy()
    a = np.abs(G)
    one = np.abs(a - 1.0) <= WIN1
    G[one] = np.sign(G[one])
    G[a <= WIN0] = 0.0
    return G


def geometry(case, dtype, clamp):
    """G[c][q][3][3] = J^-1 |det J| w_q J^-T"""
    G = cell_tensor(case.xv, case.gd, dtype)[:, None, :, :] * np.asarray(case.W, dtype=dtype)[None, :, None, None]
    return clamp101(G) if clamp else G


def reference(case, clamp):
    """y0 - c0^2 sum_cells dphi^T G dphi x in long double and the magnitude of every entry"""
    G = geometry(case, LD, clamp)
    dphi = np.asarray(case.dphi, dtype=LD)
    xl = np.asarray(case.x, dtype=LD)[case.dm]
    c02 = LD(C0) * LD(C0)

    def chain(T, Gc, u):
        w = np.einsum("iqd,cd->cqi", T, u)
        f = np.einsum("cqij,cqj->cqi", Gc, w)
        return np.einsum("iqd,cqi->cd", T, f)

    y = np.asarray(case.y0, dtype=LD).copy()
    np.add.at(y, case.dm, -c02 * chain(dphi, G, xl))
    mag = np.abs(np.asarray(case.y0, dtype=LD))
    np.add.at(mag, case.dm, c02 * chain(np.abs(dphi), np.abs(G), np.abs(xl)))
    return y, mag


def oracle_apply(oracle, case, clamp):
    G = np.ascontiguousarray(geometry(case, np.float64, clamp))
    y = case.y0.copy()
    dphi = np.ascontiguousarray(case.dphi)
    oracle.lib().oracle_stiffness_apply(0, case.ncells, case.nd, case.nq, oracle._ip(case.dm), oracle._dp(G), oracle._dp(dphi),
                                        C0, oracle._dp(case.x), oracle._dp(y))
    return y


# ---------------------------------------------------------------------------------------------------------------------
# the operator through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
class DenseOp:
    """wf_op_create_dense_simplex on the arrays of a case; `rc` is the status of the creation"""

    def __init__(self, case, flags=0):
        from wave_fenics_amd import _lib
        self.lib = _lib.lib()
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        self.keep = [np.ascontiguousarray(case.dm, dtype=np.int32), np.ascontiguousarray(case.dphi, dtype=np.float64),
                     np.ascontiguousarray(case.W, dtype=np.float64), np.ascontiguousarray(case.xv, dtype=np.float64),
                     np.ascontiguousarray(case.gd, dtype=np.int32)]
        d = _lib.DenseDesc()
        d.nd, d.nq, d.ncells, d.ndofs = case.nd, case.nq, case.ncells, case.ndofs
        d.h_dofmap, d.h_dphi, d.h_weights = ip(self.keep[0]), dp(self.keep[1]), dp(self.keep[2])
        d.nverts, d.h_xverts, d.h_geom_dofmap = self.keep[3].shape[0], dp(self.keep[3]), ip(self.keep[4])
        d.c0, d.flags = C0, flags
        self.h = ctypes.c_void_p()
        self.rc = self.lib.wf_op_create_dense_simplex(ctypes.byref(d), ctypes.byref(self.h))
        self.message = self.lib.wf_last_error().decode(errors="replace") if self.rc else ""

    def apply_rc(self, dx, dy):
        import torch
        return self.lib.wf_op_apply(self.h, dx.data_ptr(), dy.data_ptr(), int(torch.cuda.current_stream().cuda_stream))

    def __call__(self, dx, dy):
        rc = self.apply_rc(dx, dy)
        assert rc == 0, (rc, self.lib.wf_last_error())

    def host(self, gpu, x, y0):
        """y0 + A x for host vectors"""
        import torch
        dx, dy = torch.from_numpy(x).to(gpu), torch.from_numpy(y0).to(gpu)
        self(dx, dy)
        torch.cuda.synchronize()
        return dy.cpu().numpy()

    def close(self):
        rc = self.lib.wf_op_destroy(self.h) if self.h.value else 0
        self.h = ctypes.c_void_p()
        return rc

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def record(case, worst):
    key = (case.nd, case.nq, nu_of(case))
    if worst >= WORST.get(key, (-1.0, 0))[0]:
        WORST[key] = (worst, case.B)


def check_entries(case, got, ref, mag, what):
    worst, ok, where = ratio(got, ref, mag, case.B)
    record(case, worst)
    print(f"{what}: worst entry {worst:.3f} eps of its magnitude (B = {case.B})")
    assert ok, f"{what}: entry {where} is {worst:.3f} eps of its magnitude from the reference (bound {case.B})"
    return worst


def check_small(gpu, oracle, name, flags=0, applies=1):
    case = small(name)
    clamp = not (flags & NO_CLAMP)
    ref, mag = reference(case, clamp)
    yo = oracle_apply(oracle, case, clamp)
    op = created(case, flags, DenseOp)
    for k in range(applies):
        got = op.host(gpu, case.x, case.y0)
        check_entries(case, got, ref, mag, f"{name} flags {flags} apply {k}")
        err = relerr(got, yo)
        print(f"{name} flags {flags} apply {k}: {err:.3e} of max|y| from the float64 oracle")
        assert err <= TOL
    assert op.close() == 0


# ---------------------------------------------------------------------------------------------------------------------
# no GPU: the reference against the oracle, the cases against their names, the clamp constructions, creation errors
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_headroom(oracle):
    """the float64 oracle stays within B of the long-double reference on every small case (clamp on and off where the
    case is about the clamp), so the reference and the bound are checked against something that is not the kernel"""
    worst = {}
    for name in SMALL:
        case = small(name)
        for clamp in ((True, False) if name in CLAMP_CASES else (True,)):
            ref, mag = reference(case, clamp)
            yo = oracle_apply(oracle, case, clamp)
            r, ok, where = ratio(yo, ref, mag, case.B)
            assert ok, (name, clamp, where, r, case.B)
            key = (case.nd, case.nq)
            worst[key] = max(worst.get(key, 0.0), r)
            assert relerr(yo, np.asarray(ref, dtype=np.float64)) <= TOL
    for (nd, nq), r in sorted(worst.items()):
        print(f"float64 oracle against long double, (nd, nq) = ({nd}, {nq}): worst {r:.3f} eps of the magnitude (B >= {nd + 3 * nq + 9})")
        assert 0.0 < r <= nd + 3 * nq + 9


def test_clamp_helper_is_the_reference_clamp():
    from wave_fenics_amd import tet
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.uniform(-2, 2, 1000), 1.0 + rng.uniform(-3, 3, 1000) * WIN1, -1.0 + rng.uniform(-3, 3, 1000) * WIN1,
                        rng.uniform(-3, 3, 1000) * WIN0, [0.0, 1.0, -1.0]])
    assert np.array_equal(clamp101(a), tet.clamp101(a))
    assert np.array_equal(np.asarray(clamp101(a.astype(LD)), dtype=np.float64), tet.clamp101(a))


def test_cases_are_what_they_name():
    """NU, the LDS attribute path, the shape variant, batch counts, orientation and the clamp marks of every named case,
    computed from its dofmap and geometry the way dense_setup and launch_stiffness_dense do"""
    nu = {name: batch_unique(small(name).dm) for name in SMALL}
    # unique-tile size
    assert nu["P3_control"].max() <= 1280 and nu["P4_control"].max() <= 1280 and nu["P4q4_control"].max() <= 1280
    assert nu["P3_control"].max() < nu["P3_scattered"].max() <= 1280
    assert nu["P3_broken"].max() == 1280 and nu["P3_broken"][-1] == 2 * 20
    assert nu["P4_broken"].max() == 2240
    assert nu["g36x64_broken"].max() == 2304 == 9 * 256
    for name in ("P4_scattered", "P4q4_scattered"):
        assert 1280 < nu[name].max() < 2240 and nu[name].size == 6
    for name in SMALL:
        c = small(name)
        assert (nu_of(c) == 9) == (name in NU9_CASES), name
        assert lds_bytes(c) <= 160 * 1024
        if name in NU9_CASES and c.nq > 32:
            assert lds_bytes(c) > 64 * 1024, name
        assert c.dm.min() >= 0 and c.dm.max() < c.ndofs and c.gd.max() < c.xv.shape[0]
        assert all(np.unique(row).size == c.nd for row in c.dm), "a cell names a dof twice"
    # (the P4 tables alone take 58.9 KB: NU = 5 launches pass the 64 KB limit too once numax > 416, both sides occur)
    assert lds_bytes(small("P4_n1")) <= 64 * 1024 < lds_bytes(small("P4_control"))
    assert all(lds_bytes(small(n)) <= 64 * 1024 for n in ("P3_broken", "P3_scattered", "g18x20", "g11x13", "P2_all_inverted"))
    assert nu["P4_scattered"].max() != nu["P4_broken"].max()          # the two handles applied alternately
    # shapes: (QT, KT, DT) and whether the extra-row form (nd = 16 (DT - 1) + XR) is taken
    tiles = lambda c: ((c.nq + 15) // 16, (c.nd + 3) // 4, (c.nd + 15) // 16)
    expect = {"P1_n1": (1, 1, 1), "P2_all_inverted": (1, 3, 1), "g3x5": (1, 1, 1), "g11x13": (1, 3, 1), "P3_control": (2, 5, 2),
              "g18x20": (2, 5, 2), "P4_control": (4, 9, 3), "g33x50_shared": (4, 9, 3), "g34x64_spread": (4, 9, 3),
              "g36x64_broken": (4, 9, 3), "P4q4_control": (2, 9, 3), "P4q4_scattered": (2, 9, 3), "g36x17_shared": (2, 9, 3)}
    for name, t in expect.items():
        assert tiles(small(name)) == t, name
    assert small("P4q4_control").nq == 27 and small("P4_control").nq == 64
    assert small("P3_control").nd == 20 and small("P4_control").nd == 35         # XR = 4 and XR = 3
    assert all(small(n).nd not in (20, 35) for n in SMALL if n.startswith("g"))   # the X = 0 forms
    for a, b in (("g33x50_shared", "g33x50_spread"), ("g34x64_shared", "g34x64_spread"), ("g36x17_shared", "g36x17_spread")):
        assert nu_of(small(a)) == 5 and nu_of(small(b)) == 9
    # counts
    for p in (1, 4):
        for n in SMALL_COUNTS:
            c = small(f"P{p}_n{n}")
            assert c.ncells == n and c.nbatch == (n + 63) // 64
    # orientation
    for name in SMALL:
        c = small(name)
        det = jacobian(c.xv, c.gd, np.float64)[3]
        assert np.all(det != 0.0), name
        if c.inverted is not None:
            assert np.array_equal(det < 0.0, c.inverted), name
    assert [n for n in SMALL if small(n).inverted is not None] == ["P2_all_inverted", "P2_half_inverted", "P4_all_inverted",
                                                                   "P4_half_inverted"]
    assert small("P2_all_inverted").inverted.all() and small("P4_all_inverted").inverted.all()
    det = jacobian(small("P4_control").xv, small("P4_control").gd, np.float64)[3]
    assert (det < 0.0).sum() == (det > 0.0).sum()        # a Kuhn box as it comes: three cells of six per cube
    for name in ("P2_half_inverted", "P4_half_inverted"):
        f = small(name).inverted.mean()
        assert 0.3 < f < 0.7 and small(name).inverted[:NCB].any() and not small(name).inverted[:NCB].all()
    # clamp marks: which batches take clamp_here, and the margins of every product
    assert batch_marks(small("clamp_one")).tolist() == [True]
    assert batch_marks(small("clamp_zero")).tolist() == [True]
    assert batch_marks(small("clamp_partial")).tolist() == [True, True, False]
    for name in ("P3_control", "P4_control", "P3_scattered", "P4_scattered", "P4_broken", "P4q4_control"):
        assert not batch_marks(small(name)).any(), name
    for name in SMALL:
        a = products(small(name))
        a = a[a > 0.0]
        if name in CLAMP_CASES:       # a factor 3 inside a window or a factor 3 outside
            inside = (a <= WIN0 / 3) | (np.abs(a - 1.0) <= WIN1 / 3)
            outside = (a >= 3 * WIN0) & (np.abs(a - 1.0) >= 3 * WIN1)
            assert np.all(inside | outside), name
        else:                         # no product within 1e-6 (relative) of a window edge
            assert np.all(np.abs(a - WIN0) > 1e-6 * WIN0) and np.all(np.abs(np.abs(a - 1.0) - WIN1) > 1e-6 * WIN1), name
    a = products(small("clamp_one"))
    assert abs(a.max() - (1.0 + 3e-6)) <= 1e-12 and not ((a > 0) & (a <= WIN0)).any()
    a = products(small("clamp_zero"))
    small_ones = a[(a > 0.0) & (a <= WIN0)]
    assert small_ones.size and abs(small_ones.max() - 3e-9) <= 1e-12 and not (np.abs(a - 1.0) <= WIN1).any()
    # big cases: batch counts (dofmaps only; their geometry is built by the GPU tests)
    assert {nb: (nc + NCB - 1) // NCB for nb, nc in BATCH_COUNTS.items()} == {nb: nb for nb in BATCH_COUNTS}
    assert BATCH_COUNTS[1537] % NCB == 1 and 1537 == 3 * GRID + 1
    assert 26 * 26 * 25 * 6 >= max(BATCH_COUNTS.values()) and 18 * 18 * 17 * 6 >= 513 * NCB


def test_big_cases_are_what_they_name():
    """the batch counts and NU of the persistent-loop cases, from their dofmaps"""
    for nb in (513, 1537):
        c = BIG[f"P2_b{nb}"]()
        assert c.nbatch == nb and batch_unique(c.dm).max() <= 1280
    c = BIG["P2_b1537"]()
    assert c.ncells % NCB == 1 and c.nbatch - 3 * GRID == 1        # round four: one workgroup, one cell
    c = BIG["P4_b513"]()
    nu = batch_unique(c.dm)
    assert c.nbatch == 513 and 1280 < nu.min() and nu.max() <= 2240 and lds_bytes(c) > 64 * 1024


def test_clamp_constructions_discriminate():
    """a kernel that takes the wrong clamp branch misses the tolerance: the clamped and the unclamped reference differ
    by far more than B eps mag, and by at least 1e-10 of max|y| (1e-7 for the window at 1)"""
    for name, least in (("clamp_one", 1e-7), ("clamp_zero", 1e-10), ("clamp_partial", 1e-7)):
        case = small(name)
        on, mag = reference(case, True)
        off, _ = reference(case, False)
        diff = np.abs(on - off)
        rel = float(diff.max() / np.abs(on).max())
        worst = float(np.max(diff / (LD(EPS) * mag)))
        print(f"{name}: clamped and unclamped reference differ by {rel:.3e} of max|y|, {worst:.3e} eps of the magnitude (B = {case.B})")
        assert rel >= least and worst >= 100 * case.B
    # clamp_partial: the unscaled copy is untouched by the clamp
    case = small("clamp_partial")
    on, _ = reference(case, True)
    off, _ = reference(case, False)
    half = case.ndofs // 2
    assert np.array_equal(on[half:], off[half:]) and not np.array_equal(on[:half], off[:half])


def degenerate_cases():
    flat = small("P1_n17")
    gd = flat.gd.copy()
    gd[5, 3] = gd[5, 0]                      # two equal vertices: a zero column of J
    yield Case("repeated vertex", flat.nd, flat.nq, flat.dphi, flat.W, flat.xv, gd, flat.dm, flat.ndofs, flat.x, flat.y0)
    xv = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]])   # four points of one plane
    one = np.array([[0, 1, 2, 3]], dtype=np.int32)
    yield Case("flat cell", flat.nd, flat.nq, flat.dphi, flat.W, xv, one, one.copy(), 4, flat.x[:4], flat.y0[:4])
    xv = flat.xv.copy()
    xv[flat.gd[16, 2], 1] = np.nan
    yield Case("NaN vertex", flat.nd, flat.nq, flat.dphi, flat.W, xv, flat.gd, flat.dm, flat.ndofs, flat.x, flat.y0)


def test_degenerate_cell_is_refused(wlib):
    """a zero-volume cell is WF_ERR_INVALID with a message at creation (host only: no launch precedes the check)"""
    for case in degenerate_cases():
        op = DenseOp(case)
        assert op.rc == -1 and not op.h.value, (case.name, op.rc)
        assert "degenerate" in op.message and "wf_op_create_dense_simplex" in op.message, op.message


@pytest.mark.parametrize("nd,nq", [(5, 1), (40, 64), (21, 8), (4, 65), (37, 27)])
def test_uncompiled_shape_is_refused_at_creation(wlib, nd, nq):
    """a (nd, nq) whose tile counts are not compiled is WF_ERR_UNSUPPORTED with a message, before anything is uploaded"""
    op = DenseOp(generic_case("uncompiled", nd, nq, 20, None, 1))
    assert op.rc == -2 and not op.h.value
    assert "not compiled" in op.message


# ---------------------------------------------------------------------------------------------------------------------
# GPU: every small case against both references
# ---------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("name", [n for n in SMALL if n not in CLAMP_CASES])
def test_small_case(gpu, oracle, name):
    """both references, entry by entry; the NU = 9 cases twice on one handle (the second apply sets the LDS attribute again)"""
    check_small(gpu, oracle, name, applies=2 if name in NU9_CASES else 1)


@gpu_test
@pytest.mark.parametrize("flags", [0, NO_CLAMP])
@pytest.mark.parametrize("name", CLAMP_CASES)
def test_clamp(gpu, oracle, name, flags):
    """clamp on against the clamped references, WF_FLAG_NO_CLAMP against the unclamped ones"""
    check_small(gpu, oracle, name, flags=flags)


@gpu_test
@pytest.mark.parametrize("name", ["P4_control", "P4_scattered"])
def test_no_clamp_flag_is_the_identity_without_hits(gpu, oracle, name):
    check_small(gpu, oracle, name, flags=NO_CLAMP)


@gpu_test
def test_alternating_handles_with_different_lds(gpu, oracle):
    """two handles of one instantiation (P4, NU = 9) with different numax, hence different dynamic LDS sizes, applied
    alternately: the limit is an attribute of the function, not of the handle"""
    a, b = small("P4_scattered"), small("P4_broken")
    assert lds_bytes(a) != lds_bytes(b) and min(lds_bytes(a), lds_bytes(b)) > 64 * 1024
    ops = {c.name: created(c, Op=DenseOp) for c in (a, b)}
    refs = {c.name: reference(c, True) for c in (a, b)}
    for k, c in enumerate((a, b, a, b, b, a)):
        got = ops[c.name].host(gpu, c.x, c.y0)
        check_entries(c, got, *refs[c.name], f"alternating, step {k}: {c.name}")
    # and a handle of the NU = 5 instantiation of the same shape in between
    c = small("P4_control")
    check_entries(c, created(c, Op=DenseOp).host(gpu, c.x, c.y0), *reference(c, True), "alternating: P4_control")
    got = ops[a.name].host(gpu, a.x, a.y0)
    check_entries(a, got, *refs[a.name], "alternating, after NU = 5")


@gpu_test
@pytest.mark.parametrize("nd,nq", [(5, 1), (40, 64)])
def test_uncompiled_shape(gpu, nd, nq):
    """WF_ERR_UNSUPPORTED with a message at creation or at the first apply; y bitwise untouched; destroy works"""
    import torch
    case = generic_case("uncompiled", nd, nq, 70, None, 1)
    op = DenseOp(case)
    if op.rc == 0:
        dx, dy = torch.from_numpy(case.x).to(gpu), torch.from_numpy(case.y0).to(gpu)
        rc = op.apply_rc(dx, dy)
        msg = op.lib.wf_last_error().decode(errors="replace")
        torch.cuda.synchronize()
        assert rc == -2 and msg
        assert np.array_equal(dy.cpu().numpy().view(np.uint64), case.y0.view(np.uint64))
    else:
        assert op.rc == -2 and op.message and not op.h.value
    assert op.close() == 0


@gpu_test
@pytest.mark.parametrize("name", ["P4_control", "P4_scattered"])
def test_8_byte_aligned_vectors(gpu, oracle, name):
    """x and y one entry off 16-byte alignment inside padded buffers; nothing outside y is written"""
    import torch
    case = small(name)
    hx = np.full(PAD + case.ndofs + PAD + 1, SENTINEL)
    hy = hx.copy()
    hx[PAD + 1:PAD + 1 + case.ndofs] = case.x
    hy[PAD + 1:PAD + 1 + case.ndofs] = case.y0
    bx, by = torch.from_numpy(hx).to(gpu), torch.from_numpy(hy).to(gpu)
    dx, dy = bx[PAD + 1:PAD + 1 + case.ndofs], by[PAD + 1:PAD + 1 + case.ndofs]
    assert bx.data_ptr() % 16 == 0 and dx.data_ptr() % 16 == 8 and dy.data_ptr() % 16 == 8
    op = created(case, Op=DenseOp)
    op(dx, dy)
    torch.cuda.synchronize()
    gx, gy = bx.cpu().numpy(), by.cpu().numpy()
    assert np.array_equal(gx.view(np.uint64), hx.view(np.uint64)), "x or its padding was written"
    pad = np.ones(hy.size, dtype=bool)
    pad[PAD + 1:PAD + 1 + case.ndofs] = False
    assert np.array_equal(gy.view(np.uint64)[pad], hy.view(np.uint64)[pad]), "an entry outside y was written"
    got = gy[PAD + 1:PAD + 1 + case.ndofs]
    check_entries(case, got, *reference(case, True), f"{name}, x and y 8-byte aligned")
    assert relerr(got, oracle_apply(oracle, case, True)) <= TOL


@gpu_test
@pytest.mark.parametrize("name", ["P4_control", "P4_scattered", "P2_half_inverted"])
def test_repeatable_to_the_entry_bound(gpu, name):
    """two applies of one handle on the same input agree to B eps mag per entry (the atomics leave the order of the
    sums free, so bitwise equality is not the claim; each apply is itself within B of the reference)"""
    case = small(name)
    ref, mag = reference(case, True)
    op = created(case, Op=DenseOp)
    a, b = op.host(gpu, case.x, case.y0), op.host(gpu, case.x, case.y0)
    check_entries(case, a, ref, mag, f"{name} first apply")
    check_entries(case, b, ref, mag, f"{name} second apply")
    worst, ok, where = ratio(a, np.asarray(b, dtype=LD), mag, case.B)
    print(f"{name}: two applies differ by at most {worst:.3f} eps of the magnitude")
    assert ok, (where, worst)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: more batches than workgroups, against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("name", list(BIG))
def test_persistent_loop(gpu, oracle, name):
    """nbatch on both sides of 512 and 1024, 3 * 512 + 1 with a last batch of one cell, and 513 batches on the NU = 9 path:
    1e-12 of max|y| against the float64 oracle, per batch of cells as well as over all (a wrong last round must not hide
    behind the largest entry of the mesh), and two applies of the handle"""
    case = BIG[name]()
    nb = int(name.split("_b")[1])
    assert case.nbatch == nb and (nu_of(case) == 9) == name.startswith("P4")
    yo = oracle_apply(oracle, case, True)
    op = created(case, Op=DenseOp)
    for k in range(2):
        got = op.host(gpu, case.x, case.y0)
        err = relerr(got, yo)
        # the dofs of the last round of batches, on their own scale
        last = np.unique(case.dm[(case.nbatch - 1) // GRID * GRID * NCB:])
        err_last = relerr(got[last], yo[last])
        print(f"{name} apply {k}: {err:.3e} of max|y|; dofs of the last round of batches {err_last:.3e}")
        assert err <= TOL and err_last <= TOL
        untouched = np.ones(case.ndofs, dtype=bool)
        untouched[case.dm.reshape(-1)] = False
        assert np.array_equal(got[untouched], case.y0[untouched])
    assert op.close() == 0


@gpu_test
def test_report_worst_ratios(gpu):
    """the record of the run: worst |got - ref| / (eps * magnitude) per shape and NU (runs last; the bound stays B)"""
    assert WORST, "no entry check has run"
    for (nd, nq, nu) in sorted(WORST):
        r, B = WORST[(nd, nq, nu)]
        print(f"worst ratio (nd, nq) = ({nd}, {nq}) NU = {nu}: {r:.3f} (B = {B})")
        assert r <= B
    print(f"module wall time {time.time() - T0:.1f} s")
