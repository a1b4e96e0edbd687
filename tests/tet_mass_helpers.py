"""Cases, references and the C-ABI handle shared by test_gpu_tet_mass.py and test_tet_mass_host.py (no tests here).

The operator under test is y += M x on affine tetrahedra (csrc/mass_dense_simplex.hip), created through
`DenseMassDesc` / `wf_op_create_dense_simplex_mass` so that a test hands over its own table of basis values, weights,
dofmap, geometry and flags.

References (neither is the code under test).  The two-stage expression of common/cuda/mass.hpp,
    ref = y0 + sum_c s_c Phi^T (w .* (Phi x_e)),        s_c = |det J_c|  (det J_c under WF_FLAG_NO_FABS)
    mag = |y0| + sum_c |s_c| |Phi|^T (w .* (|Phi| |x_e|)),
evaluated with numpy in any dtype, np.add.at over the dofmap: in long double for the entry check of the small cases,
in float64 at TOL = 1e-12 of max|ref| for the large ones.  The kernel evaluates the collapsed form s_c (A x_e) with
A = Phi^T diag(w) Phi, so the reference shares no intermediate with it.

Entry bound: |got - ref| <= B eps mag for every entry, B = nd + v + 8, v = most cells sharing one dof.  B is derived,
not measured: a sum of n products in any order (MFMA k-steps, atomics in LDS and in global memory) is within
n u (1 + O(u)) of its magnitude, u = eps / 2; one entry is nd terms of the product and v + 1 terms of the sum over the
cells of the dof and y0; the remaining 7 cover the single rounding of A (|A| <= |Phi|^T W |Phi| because the weights are
positive), the determinant and the scale.  In units of eps that chain is about B / 2: a factor two of headroom."""
import ctypes
import functools
from dataclasses import dataclass, field

import numpy as np

from support import EPS, LD, ratio, relerr  # noqa: F401

NCB = 64                 # cells per batch (16 per wave, four waves)
# kMassGridBound = 256 * kMassWgsPerCU of csrc/mass_dense_simplex.hip (the constants under the comment "Workgroups per
# CU of the persistent grid"): the launch uses min(nbatch, GRID) workgroups.  The persistent-loop cases assume it.
WGS_PER_CU = 2
GRID = 256 * WGS_PER_CU
TOL = 1e-12              # max-norm tolerance of the float64 reference (the project's)
NO_FABS = 1              # WF_FLAG_NO_FABS
ORDERED = 16             # WF_FLAG_ORDERED
PAD = 16                 # sentinel entries around a shifted vector
SENTINEL = -7.0e77


@dataclass
class Case:
    name: str
    nd: int
    nq: int
    phi: np.ndarray           # [nq][nd]
    W: np.ndarray             # [nq]
    xv: np.ndarray            # [nverts][3]
    gd: np.ndarray            # [ncells][4] int32
    dm: np.ndarray            # [ncells][nd] int32
    ndofs: int
    x: np.ndarray
    y0: np.ndarray
    inverted: np.ndarray = field(default=None)   # orientation cases: the cells that were given det J < 0
    upright_gd: np.ndarray = field(default=None)  # orientation cases: the same cells, every det J > 0

    @property
    def ncells(self):
        return int(self.gd.shape[0])

    @property
    def nbatch(self):
        return (self.ncells + NCB - 1) // NCB

    @property
    def v(self):
        return int(np.bincount(self.dm.reshape(-1)).max()) if self.dm.size else 0

    @property
    def B(self):
        return self.nd + self.v + 8

    @property
    def tiles(self):
        return (self.nd + 3) // 4, (self.nd + 15) // 16


def batch_unique(dm):
    """unique dofs of every batch of 64 cells, as dense_batch_plan counts them"""
    return np.array([np.unique(dm[b:b + NCB]).size for b in range(0, dm.shape[0], NCB)])


def nu_of(case):
    return 5 if batch_unique(case.dm).max() <= 5 * 256 else 9


def lds_bytes(case):
    KT, DT = case.tiles
    return 8 * (16 * DT * (4 * KT + 2) + 2 * int(batch_unique(case.dm).max()))


def lagrange_tables(p, m, gradients=False):
    """values of P_p on the tetrahedron at the m^3 points of the collapsed Gauss-Jacobi rule (degree 2 m - 1), unclamped;
    gradients: the clamped gradient tables [3][nq][nd] that tet.TetStiffnessOperator hands over instead"""
    from wave_fenics_amd import tet
    X, W = tet.tet_quadrature(m)
    phi, dphi = tet.tabulate_tet(p, X)
    if gradients:
        return np.ascontiguousarray(tet.clamp101(dphi)), np.ascontiguousarray(W)
    return np.ascontiguousarray(phi, dtype=np.float64), np.ascontiguousarray(W, dtype=np.float64)


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def det_j(xv, gd, dtype):
    """det J of every cell (columns of J: the edge vectors v_j - v_0)"""
    xc = np.asarray(xv, dtype=dtype)[gd]
    a, b, c = xc[:, 1] - xc[:, 0], xc[:, 2] - xc[:, 0], xc[:, 3] - xc[:, 0]
    return np.sum(a * cross(b, c), axis=1)


def scales(case, flags, dtype):
    d = det_j(case.xv, case.gd, dtype)
    return d if flags & NO_FABS else np.abs(d)


def two_stage(phi, W, s, xl):
    """s_c Phi^T (w .* (Phi x_e)) per cell, [c][nd]"""
    u = np.einsum("qd,cd->cq", phi, xl)
    return np.einsum("qd,cq->cd", phi, u * W[None, :]) * s[:, None]


def reference(case, flags=0, dtype=LD, y0=None, times=1):
    """y0 + times * M x and the magnitude of every entry, both in `dtype`"""
    phi, W = np.asarray(case.phi, dtype=dtype), np.asarray(case.W, dtype=dtype)
    s = scales(case, flags, dtype)
    xl = np.asarray(case.x, dtype=dtype)[case.dm]
    y0 = case.y0 if y0 is None else y0
    y = np.asarray(y0, dtype=dtype).copy()
    mag = np.abs(np.asarray(y0, dtype=dtype))
    if case.ncells:
        np.add.at(y, case.dm, times * two_stage(phi, W, s, xl))
        np.add.at(mag, case.dm, times * two_stage(np.abs(phi), W, np.abs(s), np.abs(xl)))
    return y, mag


def collapsed_float64(case, flags=0):
    """the collapsed form s_c (A x_e) in plain float64 numpy: what a correct kernel computes, up to the order of sums"""
    A = np.einsum("q,qa,qb->ab", case.W, case.phi, case.phi)
    y = case.y0.copy()
    np.add.at(y, case.dm, (case.x[case.dm] @ A.T) * scales(case, flags, np.float64)[:, None])
    return y


def vectors(rng, case_dm, ndofs, typical):
    """x in [-1, 1]; y0 non-zero everywhere and of the size of the entries of M x (a y0 far above them would hide the
    operator's error behind eps |y0|)"""
    x = rng.uniform(-1.0, 1.0, ndofs)
    y0 = rng.uniform(0.25, 1.0, ndofs) * rng.choice([-1.0, 1.0], ndofs) * typical
    return x, y0


def typical_entry(phi, W, xv, gd):
    """the size of an entry of M |x|: mean |det J| times the mean row sum of |Phi|^T W |Phi| (1 for an empty mesh)"""
    if gd.shape[0] == 0:
        return 1.0
    A = np.einsum("q,qa,qb->ab", W, np.abs(phi), np.abs(phi))
    return float(np.abs(det_j(xv, gd, np.float64)).mean() * A.sum(axis=1).mean())


def mesh_case(name, p, n, *, m=None, perturb=0.2, ncells=None, shuffle=False, renumber=False, broken=False, invert=0.0,
              seed=0):
    """Kuhn box of degree p with the m^3-point rule (default m = p + 1: degree 2p + 1 >= 2p), then: a subset of `ncells`
    cells, a random cell order, a random permutation of the dof numbers, a dofmap in which every cell has dofs of its
    own, a fraction `invert` of the cells with det J < 0 and every other cell with det J > 0 (vertices 1 and 2 swapped
    where the sign has to change)."""
    from wave_fenics_amd import tet
    V = tet.create_kuhn_box(n, p, perturb=perturb)
    rng = np.random.default_rng(seed)
    xv = np.array(V.x, dtype=np.float64)
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
    inverted = upright = None
    if invert:
        # (three of the six Kuhn tetrahedra of a cube have det J < 0 as they come; here the sign is the case's choice)
        inverted = np.ones(gd.shape[0], dtype=bool) if invert >= 1.0 else rng.random(gd.shape[0]) < invert
        neg = det_j(xv, gd, np.float64) < 0.0
        upright = gd.copy()
        upright[neg] = upright[neg][:, [0, 2, 1, 3]]
        swap = neg != inverted
        gd[swap] = gd[swap][:, [0, 2, 1, 3]]
        upright = np.ascontiguousarray(upright, dtype=np.int32)
    phi, W = lagrange_tables(p, p + 1 if m is None else m)
    gd = np.ascontiguousarray(gd, dtype=np.int32)
    x, y0 = vectors(rng, dm, ndofs, typical_entry(phi, W, xv, gd))
    return Case(name, phi.shape[1], phi.shape[0], phi, W, np.ascontiguousarray(xv), gd,
                np.ascontiguousarray(dm, dtype=np.int32), ndofs, x, y0, inverted, upright)


def generic_parts(nd, nq, ncells, pool, seed, table_shape):
    """The seeded draws of a generic case on the cells of a perturbed Kuhn box: the generator (for the vectors, drawn
    last), a table of `table_shape` in (-1, 1), positive weights, vertices, geometry dofmap, dofmap and ndofs.  Every
    cell takes nd distinct dofs out of `pool` (None: dofs of its own), so the sharing is the case's choice."""
    from wave_fenics_amd import tet
    V = tet.create_kuhn_box((3, 3, 3), 1, perturb=0.2)
    rng = np.random.default_rng(seed)
    cells = rng.permutation(V.ncells)[:ncells]
    table = rng.uniform(-1.0, 1.0, table_shape)
    W = rng.uniform(0.5, 1.5, nq) / (6.0 * nq)
    if pool is None:
        ndofs = ncells * nd
        dm = np.arange(ndofs).reshape(ncells, nd)
    else:
        ndofs = pool
        dm = np.stack([rng.choice(pool, nd, replace=False) for _ in range(ncells)])
    xv = np.array(V.x, dtype=np.float64)
    gd = np.ascontiguousarray(V.geom_dofmap[cells], dtype=np.int32)
    return rng, table, W, xv, gd, np.ascontiguousarray(dm, dtype=np.int32), ndofs


def generic_case(name, nd, nq, ncells, pool, seed):
    """Table and (positive) weights from a seeded generator (generic_parts)."""
    rng, phi, W, xv, gd, dm, ndofs = generic_parts(nd, nq, ncells, pool, seed, (nq, nd))
    x, y0 = vectors(rng, dm, ndofs, typical_entry(phi, W, xv, gd))
    return Case(name, nd, nq, phi, W, xv, gd, dm, ndofs, x, y0)


def upright_of(case):
    """the orientation case with every cell turned to det J > 0 (same cells, same dofs, same vectors)"""
    return Case(case.name + "_upright", case.nd, case.nq, case.phi, case.W, case.xv, case.upright_gd, case.dm, case.ndofs,
                case.x, case.y0)


SMALL_COUNTS = [1, 63, 64, 65, 129]

SMALL = {
    # every compiled (KT, DT) on the Lagrange tables: the rule of degree >= 2p, a one-point rule, and point counts that
    # are no multiple of 16 (nq enters A only)
    "P1_q8": lambda: mesh_case("P1_q8", 1, (2, 2, 2), seed=1),
    "P1_q1": lambda: mesh_case("P1_q1", 1, (2, 2, 2), m=1, seed=2),
    "P2_q27": lambda: mesh_case("P2_q27", 2, (3, 2, 2), seed=3),
    "P2_q1": lambda: mesh_case("P2_q1", 2, (3, 2, 2), m=1, seed=4),
    "P3_q64": lambda: mesh_case("P3_q64", 3, (2, 2, 2), seed=5),
    "P3_q27": lambda: mesh_case("P3_q27", 3, (2, 2, 2), m=3, seed=6),
    "P4_q125": lambda: mesh_case("P4_q125", 4, (2, 2, 1), seed=7),
    "P4_q1": lambda: mesh_case("P4_q1", 4, (2, 2, 1), m=1, seed=8),
    "P4_q27": lambda: mesh_case("P4_q27", 4, (2, 2, 1), m=3, seed=9),
    # padded shapes on the same tiles
    "g3x5": lambda: generic_case("g3x5", 3, 5, 150, 120, 10),
    "g11x13": lambda: generic_case("g11x13", 11, 13, 150, 500, 11),
    "g18x20": lambda: generic_case("g18x20", 18, 20, 150, 900, 12),
    "g33x50_shared": lambda: generic_case("g33x50_shared", 33, 50, 150, 1100, 13),
    "g33x50_spread": lambda: generic_case("g33x50_spread", 33, 50, 150, 30000, 14),
    "g36x17_shared": lambda: generic_case("g36x17_shared", 36, 17, 150, 1280, 15),
    "g36x17_broken": lambda: generic_case("g36x17_broken", 36, 17, 130, None, 16),
    # unique-tile size
    "P4_control": lambda: mesh_case("P4_control", 4, (3, 2, 2), seed=17),
    "P4_scattered": lambda: mesh_case("P4_scattered", 4, (4, 4, 4), shuffle=True, renumber=True, seed=18),
    "P4_broken": lambda: mesh_case("P4_broken", 4, (3, 3, 3), ncells=130, broken=True, seed=19),
    "P3_broken": lambda: mesh_case("P3_broken", 3, (3, 3, 3), ncells=130, broken=True, seed=20),
    # orientation
    "P2_all_inverted": lambda: mesh_case("P2_all_inverted", 2, (3, 2, 2), invert=1.0, seed=21),
    "P2_half_inverted": lambda: mesh_case("P2_half_inverted", 2, (3, 2, 2), invert=0.5, seed=22),
    "P4_all_inverted": lambda: mesh_case("P4_all_inverted", 4, (3, 2, 2), invert=1.0, seed=23),
    "P4_half_inverted": lambda: mesh_case("P4_half_inverted", 4, (3, 2, 2), invert=0.5, seed=24),
}
for _n in SMALL_COUNTS:
    SMALL[f"P4_n{_n}"] = functools.partial(mesh_case, f"P4_n{_n}", 4, (3, 3, 3), ncells=_n, seed=400 + _n)
ORIENTATION_CASES = ["P2_all_inverted", "P2_half_inverted", "P4_all_inverted", "P4_half_inverted"]
NU9_CASES = ["g33x50_spread", "g36x17_broken", "P4_scattered", "P4_broken", "P4_n63", "P4_n64", "P4_n65"]

# nbatch above the grid bound.  P2 (NU = 5): three whole rounds and a fourth with one live workgroup whose batch holds
# one cell.  P4 (NU = 9, scattered numbering): one whole round and a second with one live workgroup, one cell.
BIG = {
    "P2_rounds4": lambda: mesh_case("P2_rounds4", 2, (26, 26, 25), ncells=3 * GRID * NCB + 1, seed=31),
    "P4_rounds2": lambda: mesh_case("P4_rounds2", 4, (18, 18, 17), ncells=GRID * NCB + 1, shuffle=True, renumber=True, seed=32),
}


def named_cases(table):
    """small(name) over a table of case constructors: built once per name, named, shared."""
    @functools.lru_cache(maxsize=None)
    def small(name):
        c = table[name]()
        c.name = name
        return c
    return small


small = named_cases(SMALL)


@functools.lru_cache(maxsize=None)
def small_reference(name, flags=0):
    """the long-double reference of a small case, computed once and shared (read-only)"""
    ref, mag = reference(small(name), flags)
    ref.setflags(write=False)
    mag.setflags(write=False)
    return ref, mag


def empty_case():
    c = small("P4_control")
    return Case("empty", c.nd, c.nq, c.phi, c.W, c.xv, np.zeros((0, 4), np.int32), np.zeros((0, c.nd), np.int32), c.ndofs,
                c.x, c.y0)


class MassOp:
    """wf_op_create_dense_simplex_mass on the arrays of a case; `rc` is the status of the creation"""

    def __init__(self, case, flags=0, null=None):
        from wave_fenics_amd import _lib
        self.lib = _lib.lib()
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        self.keep = [np.ascontiguousarray(case.dm, dtype=np.int32), np.ascontiguousarray(case.phi, dtype=np.float64),
                     np.ascontiguousarray(case.W, dtype=np.float64), np.ascontiguousarray(case.xv, dtype=np.float64),
                     np.ascontiguousarray(case.gd, dtype=np.int32)]
        d = _lib.DenseMassDesc()
        d.nd, d.nq, d.ncells, d.ndofs = case.nd, case.nq, case.ncells, case.ndofs
        d.h_dofmap, d.h_phi, d.h_weights = ip(self.keep[0]), dp(self.keep[1]), dp(self.keep[2])
        d.nverts, d.h_xverts, d.h_geom_dofmap = self.keep[3].shape[0], dp(self.keep[3]), ip(self.keep[4])
        d.flags = flags
        if null is not None:
            setattr(d, null, None)
        self.h = ctypes.c_void_p()
        self.rc = self.lib.wf_op_create_dense_simplex_mass(ctypes.byref(d), ctypes.byref(self.h))
        self.message = self.lib.wf_last_error().decode(errors="replace") if self.rc else ""

    def info(self):
        from wave_fenics_amd import _lib
        info = _lib.OpInfo()
        assert self.lib.wf_op_info(self.h, ctypes.byref(info)) == 0
        return info

    def apply_rc(self, dx, dy):
        import torch
        return self.lib.wf_op_apply(self.h, dx.data_ptr(), dy.data_ptr(), int(torch.cuda.current_stream().cuda_stream))

    def __call__(self, dx, dy):
        rc = self.apply_rc(dx, dy)
        assert rc == 0, (rc, self.lib.wf_last_error())

    def host(self, gpu, x, y0, applies=1):
        """y0 + applies * M x for host vectors"""
        import torch
        dx, dy = torch.from_numpy(x).to(gpu), torch.from_numpy(y0).to(gpu)
        for _ in range(applies):
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


def created(case, flags=0, Op=MassOp):
    op = Op(case, flags)
    assert op.rc == 0, (case.name, op.rc, op.message)
    return op
